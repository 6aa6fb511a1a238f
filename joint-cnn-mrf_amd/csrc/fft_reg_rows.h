// Device code shared by the transform kernels of the frequency-domain convolution that keep the whole FFT in the registers of one thread (fft_reg.h):
// conv_fft_reg_inv.hip (inverse rows and columns), conv_fft_reg_fwd.hip (forward rows), conv_fft_reg_fused.hip (the fused hand-overs between two layers)
// and conv_fft_reg_tiles.hip (the 2 x 2 tiles).  One copy of every step two of these kernels have in common.
//
// The LDS row kernels (conv_fft_rows_fwd.hip, conv_fft_rows_inv.hip) give a work group one (image, row, 64 channels) tile: load -> barrier ->
// radix stage -> barrier -> radix stage -> barrier -> store, one butterfly per thread and stage.  Measured (round 4, SQ_INSTS_* / SQ_WAVE_CYCLES,
// DESIGN.md 4.1f): 2-3 work groups per CU (80-110 VGPRs at 6 waves per group), 2.2 resident waves per SIMD, the butterflies a fifth of the
// executed instructions -- the kernels are bound by latency behind barriers, not by HBM (2.2-3.7 TB/s).  Here a THREAD owns one (image, row,
// channel pair): it loads its half spectrum (one 8- or 16-byte load per kx; consecutive lanes are consecutive channel pairs, so every load or
// store instruction of a wave is one contiguous run), transforms it in registers with compile-time indices and literal twiddles, and stores its
// row.  No LDS, no barrier, no index arithmetic; all loads of a thread are in flight before the first butterfly.
#pragma once
#include "conv_fft_common.h"
#include "fft_reg.h"

namespace jcm {
namespace cfft {
using namespace fftr;

// ---- which (thread h of the pair, channel pair p, row by) a thread is.  Two threads per channel pair; a wave is the 32 channel pairs = 64 channels of
// ONE row (C % 64 == 0), so the row is a scalar.  ADJ: the two threads of a pair are adjacent lanes (the kernels that start with an inverse transform: both
// load the same T' entries, one request) -- else thread 0 sits in lanes 0..31 and thread 1 in lanes 32..63 (the forward kernels, see pair_word).
// xcd (512 channels = eight 64-channel blocks per row): work group i runs on XCD i % 8, so let it be block i % 8 of FOUR rows (one per wave) instead of
// four blocks of one row -- an XCD then sees one channel block of every row, and what several rows share stays in its L2 (the coarse rows of the branch
// merge, which 2-8 fine rows read; counters: 3.27 -> 1.9 GB fetched by rows_fwd_merge_reg_kernel, 3.30 GB per 256 bf16 images with the linear mapping for
// 1.54 GB of T' and 0.44 GB of coarse maps in rows_inv_merge_fwd_reg_kernel).  The launcher then starts eight work groups per four rows.
template <bool ADJ>
__device__ __forceinline__ void pair_coords(int CP, int& h, int& p, size_t& by, bool xcd = false) {
  const int lane = threadIdx.x & 63;
  h = ADJ ? lane & 1 : lane >> 5;
  if (xcd) {
    p = (int)(blockIdx.x & 7) * 32 + (ADJ ? lane >> 1 : lane & 31);
    by = (size_t)(blockIdx.x >> 3) * 4 + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  } else {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t q = ADJ ? g >> 1 : (g >> 6) * 32;      // this thread's pair / the first pair of the wave
    p = (int)((ADJ ? q : q + (lane & 31)) % CP);
    by = (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(q / CP));
  }
}
// what a thread of a pair holds, from the other thread of an ADJACENT-lane pair (DPP quad_perm [1,0,3,2])
__device__ __forceinline__ unsigned lane_pair_swap(unsigned w) { return (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ cf lane_pair_swap(cf z) { return cf{__uint_as_float(lane_pair_swap(__float_as_uint(z.x))), __uint_as_float(lane_pair_swap(__float_as_uint(z.y)))}; }

// ---- undoing the fp16 scale of the spectra (Fp16Scale, conv_fft_common.h): the inverse's 1 / (NY NX) times the inverse scales of the filter spectra and of
// word i of sc.tmax -- the image's, or the tile's -- or, for a handle with training state (sc.common), of the largest of its nb words.  That one is taken by
// the wave, not by every thread, and once per kernel: scale_common().
__device__ __forceinline__ float scale_common(const Fp16Scale& sc) {
  float tm = 0.f;
  if (sc.tmax && sc.common) {
    for (int i = (int)(threadIdx.x & 63); i < sc.nb; i += 64) tm = fmaxf(tm, sc.tmax[i]);
    tm = wave_max(tm);
  }
  return tm;
}
__device__ __forceinline__ float scale_undo(float norm0, const Fp16Scale& sc, int i, float tcommon) {
  return sc.tmax ? norm0 * sc.winv[0] * fp16_unscale(sc.common ? tcommon : sc.tmax[i], sc.hf) : norm0;      // powers of two: exact
}
__device__ __forceinline__ float bf16_rn(float v) { return static_cast<float>(static_cast<__bf16>(v)); }
// ---- the layer's epilogue on a channel pair (c, c + 1): z * norm + bias, then ReLU and the folded BatchNorm.  TAIL: the transformed channels may reach behind
// Cout (the padded tail of the plain inverse rows); those keep bias 0.  BF: the activation is a bf16 tensor (the merge hand-over of bf16 handles rounds x1 as
// the unfused route stores it).
template <bool BF = false, bool TAIL = false> struct Epilogue {
  float norm, b0 = 0.f, b1 = 0.f, s0 = 1.f, s1 = 1.f, h0 = 0.f, h1 = 0.f;
  int relu_bn;
  __device__ __forceinline__ Epilogue(const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift, int relu_bn_, int c, int Cout, float norm_)
      : norm(norm_), relu_bn(relu_bn_) {
    const bool two = !TAIL || c + 1 < Cout;
    if (!TAIL || c < Cout) {
      b0 = bias[c];
      if (two) b1 = bias[c + 1];
      if (relu_bn) { s0 = scale[c]; h0 = shift[c]; if (two) { s1 = scale[c + 1]; h1 = shift[c + 1]; } }
    }
  }
  __device__ __forceinline__ cf operator()(cf z) const {
    float v0 = fmaf(z.x, norm, b0), v1 = fmaf(z.y, norm, b1);      // (single roundings: these kernels are instruction-bound)
    if (relu_bn) { v0 = fmaf(fmaxf(v0, 0.f), s0, h0); v1 = fmaf(fmaxf(v1, 0.f), s1, h1); }
    if constexpr (BF) { v0 = bf16_rn(v0); v1 = bf16_rn(v1); }
    return cf{v0, v1};
  }
};

// ---- one row of T'[b][y][kx][c] as the inverse row transform reads it: entry k of the channel pair as (Ya.re, Ya.im, Yb.re, Yb.im).
// Buffer loads: the row's T' is one descriptor, the entry k a SCALAR offset, the lane's channel pair the only vector offset -- no per-lane 64-bit
// address arithmetic (a tenth of the plain inverse kernel's vector instructions when the compiler forms global addresses; it is bound by their issue
// slots -- and with 64-bit addresses per entry the tile kernel keeps the 49 addresses of all four rows and spills them)
template <int NX> struct TInvRow32 {      // complex fp32
  __amdgpu_buffer_rsrc_t d;
  int vo, ko;
  __device__ __forceinline__ TInvRow32(const void* T, size_t row, int C, int p)
      : d(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(static_cast<const float*>(T)) + row * (NX / 2 + 1) * C * 2, 0, (NX / 2 + 1) * C * 8, 0x00020000)), vo(p * 16), ko((C >> 1) * 16) {}
  __device__ __forceinline__ float4 operator()(int k) const {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 q = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(d, vo, k * ko, 0));
    return make_float4(q[0], q[1], q[2], q[3]);
  }
};
// complex fp16 in block floating point (16-bit T' of bf16 handles).  request(): every load goes out at once, in the order of use (the entries are consumed in
// pairs (n, M - n)); the conversions of the first entries then overlap the latency of the later loads.  scales(): the scale words of this wave's tile, one
// 64-channel block of one image, contiguous over kx and the same for all lanes: scalar loads.
template <int NX> struct TInvRow16 {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  u2 raw[NX / 2 + 1];
  const float* ssrc;
  __device__ __forceinline__ void request(const void* T, size_t row, int C, int p) {
    constexpr int NXH = NX / 2 + 1, M = NX / 2;
    const auto d = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(static_cast<const unsigned*>(T)) + row * NXH * C, 0, NXH * C * 4, 0x00020000);
    const int vo = p * 8, ko = (C >> 1) * 8;
#pragma unroll
    for (int n = 0; 2 * n <= M; ++n) {
      raw[n] = __builtin_amdgcn_raw_buffer_load_b64(d, vo, n * ko, 0);
      if (2 * n != M) raw[M - n] = __builtin_amdgcn_raw_buffer_load_b64(d, vo, (M - n) * ko, 0);
    }
  }
  __device__ __forceinline__ void scales(const Fp16Scale& sc, int b, int c, int C) {
    const int nblk = C / sc.t16_cb;
    ssrc = sc.t16_inv + ((size_t)__builtin_amdgcn_readfirstlane(b) * nblk + __builtin_amdgcn_readfirstlane(c / sc.t16_cb)) * (NX / 2 + 1);
  }
  __device__ __forceinline__ float4 operator()(int k) const {
    const float s = ssrc[k];
    const cf ya = unpack_h2_mix_s(raw[k][0], s), yb = unpack_h2_mix_s(raw[k][1], s);
    return make_float4(ya.x, ya.y, yb.x, yb.y);
  }
};

// TWO threads per (image, row, channel pair) -- a 96-point transform does not fit one thread's registers next to its loads (256 VGPRs: 178 spilled).
// Thread h of the two takes the outputs of parity h (decimation in frequency):
//   X[2 m + h] = sum_{n < M} u_h[n] w_M^(n m),   u_h[n] = (Z[n] + (-1)^h Z[n + M]) w_NX^(n h),   M = NX / 2
// i.e. one radix-2 stage whose twiddle is selected per lane, then an M-point transform in registers.  Z comes from the half spectrum of the
// channel pair (Z = Y_c + i Y_{c+1}, Hermitian extension): Z[n] and Z[n + M] = Z[NX - (M - n)] need the loaded entries n and M - n, so the
// entries are consumed in pairs (n, M - n) and both threads load all of them (the same addresses in adjacent lanes: one request).
// ALL: every output goes to `store` (the bf16 layouts stage the whole row in LDS and test the columns when they copy it out: no range test per output here)
template <int NX, int K1, bool ALL = false, class St>
__device__ __forceinline__ void inv_rows_out2(const cf (&u)[NX / 2], int h, int W, int pad, St&& store) {
  constexpr int M = NX / 2, R1 = RPlan<M>::R1, R2 = RPlan<M>::R2;
  cf o[R2];
  step2_row<M, 1, K1>(u, o);
#pragma unroll
  for (int k2 = 0; k2 < R2; ++k2) {
    const int xo = 2 * (K1 + R1 * k2) + h - pad;      // output column of X[2 m + h], m = K1 + R1 k2
    if (ALL || (xo >= 0 && xo < W)) store(K1 + R1 * k2, xo, o[k2]);
  }
  __builtin_amdgcn_sched_barrier(0);      // one row of step 2 and its stores at a time (the scheduler otherwise interleaves all R1 rows and spills)
  if constexpr (K1 + 1 < R1) inv_rows_out2<NX, K1 + 1, ALL>(u, h, W, pad, store);
}
// u[N] (and u[M - N]) of thread h from the half-spectrum entries N and M - N:  q = (Ya.re, Ya.im, Yb.re, Yb.im)
template <int NX, int N>
__device__ __forceinline__ void inv_rows_in2(cf (&u)[NX / 2], const float4& q1, const float4& q2, float sg, bool odd) {
  constexpr int M = NX / 2;
  if constexpr (N == 0) {
    // Z[0] = (Ya[0].re, Yb[0].re), Z[M] = (Ya[M].re, Yb[M].re)   (DC and Nyquist are real); twiddle 1
    u[0] = cf{fmaf(sg, q2.x, q1.x), fmaf(sg, q2.z, q1.z)};
  } else {
    // entry N: Z[N] = (a.x - a.w, a.y + a.z);  entry M - N gives Z[NX - (M - N)] = Z[N + M] = (b.x + b.w, b.z - b.y)
    const cf zn = cf{q1.x - q1.w, q1.y + q1.z}, znm = cf{q2.x + q2.w, q2.z - q2.y};
    cf v = cf{fmaf(sg, znm.x, zn.x), fmaf(sg, znm.y, zn.y)};
    const float wr = odd ? Tw<N, NX>::re : 1.f, wi = odd ? Tw<N, NX>::im : 0.f;
    u[N] = cf{fmaf(-v.y, wi, v.x * wr), fmaf(v.x, wi, v.y * wr)};
    if constexpr (2 * N != M) {
      // entry M - N: Z[M - N] = (b.x - b.w, b.y + b.z);  entry N gives Z[NX - N] = Z[(M - N) + M] = (a.x + a.w, a.z - a.y)
      const cf zm = cf{q2.x - q2.w, q2.y + q2.z}, zmm = cf{q1.x + q1.w, q1.z - q1.y};
      v = cf{fmaf(sg, zmm.x, zm.x), fmaf(sg, zmm.y, zm.y)};
      const float wr2 = odd ? Tw<M - N, NX>::re : 1.f, wi2 = odd ? Tw<M - N, NX>::im : 0.f;
      u[M - N] = cf{fmaf(-v.y, wi2, v.x * wr2), fmaf(v.x, wi2, v.y * wr2)};
    }
  }
}
template <int NX, int N, class Ld>
__device__ __forceinline__ void inv_rows_load2(cf (&u)[NX / 2], float sg, bool odd, Ld&& load) {
  constexpr int M = NX / 2;
  // the loads go out in batches of LDB pairs (a compiler fence between the batches): hoisting all NX/2+1 of them in front of the arithmetic
  // costs more registers than the thread has (measured: 390-640 bytes of scratch per lane)
  constexpr int LDB = 6;
  if constexpr (N % LDB == 0 && N > 0) __builtin_amdgcn_sched_barrier(0);
  const float4 q1 = load(N), q2 = load(M - N);
  inv_rows_in2<NX, N>(u, q1, q2, sg, odd);
  if constexpr (2 * (N + 1) <= M) inv_rows_load2<NX, N + 1>(u, sg, odd, load);
}

// The forward kernels put thread 0 of a pair in lanes 0..31 and thread 1 in lanes 32..63 of the wave (pair_coords<false>; the inverse kernels: adjacent lanes): each half
// wave then reads one contiguous 128-byte run per pixel instead of two runs interleaved lane by lane -- nothing for the plain row pass, 1.51 -> 1.15 ms for
// rows_fwd_merge_reg_kernel with its 126 loads per thread.  The word of the other thread of the pair comes by v_permlane32_swap (lanes i and i + 32).
__device__ __forceinline__ unsigned pair_word(unsigned w, bool odd) {
  const auto r = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return odd ? r[0] : r[1];
}
__device__ __forceinline__ cf pair_word(cf z, bool odd) { return cf{__uint_as_float(pair_word(__float_as_uint(z.x), odd)), __uint_as_float(pair_word(__float_as_uint(z.y), odd))}; }
__device__ __forceinline__ cf px_cf(unsigned bits) { return bf16pair(bits); }      // a pixel of the channel pair: bf16 x 2 in a word, or fp32 x 2
__device__ __forceinline__ cf px_cf(cf z) { return z; }
// u_h[J..M-1] of thread h from its pixels raw[] = z[h M .. h M + M) and the other thread's
template <int NX, int J, class Px>
__device__ __forceinline__ void fwd_rows_in2(cf (&u)[NX / 2], const Px (&raw)[NX / 2], float sg, bool odd) {
  constexpr int M = NX / 2;
  const cf a = px_cf(raw[J]), o = px_cf(pair_word(raw[J], odd));
  cf v = cf{fmaf(sg, a.x, o.x), fmaf(sg, a.y, o.y)};      // h = 0: z[J] = a, z[J + M] = o -> a + o;  h = 1: z[J] = o, z[J + M] = a -> o - a
  if constexpr (J > 0) {
    const float wr = odd ? Tw<-J, NX>::re : 1.f, wi = odd ? Tw<-J, NX>::im : 0.f;      // e^{-2 pi i J / NX} for the odd outputs
    v = cf{fmaf(-v.y, wi, v.x * wr), fmaf(v.x, wi, v.y * wr)};
  }
  u[J] = v;
  if constexpr (J + 1 < M) fwd_rows_in2<NX, J + 1>(u, raw, sg, odd);
}
template <int N, int S, int K1>
__device__ __forceinline__ void step2_inplace(cf (&x)[N]) {      // x[R2 K1 + k2] <- X[K1 + R1 k2]
  constexpr int R1 = RPlan<N>::R1, R2 = RPlan<N>::R2;
  cf o[R2];
  step2_row<N, S, K1>(x, o);
#pragma unroll
  for (int k2 = 0; k2 < R2; ++k2) x[R2 * K1 + k2] = o[k2];
  if constexpr (K1 + 1 < R1) step2_inplace<N, S, K1 + 1>(x);
}
// visit the outputs k = 2 m + h <= NX / 2 of this thread: f(m, X_c[k], X_{c+1}[k]) as (re, im, re, im)
template <int NX, int MI, class F>
__device__ __forceinline__ void fwd_rows_visit(const cf (&u)[NX / 2], bool odd, F&& f) {
  constexpr int M = NX / 2, R1 = RPlan<M>::R1, R2 = RPlan<M>::R2;
  constexpr int m0 = (M - MI) % M, m1 = M - 1 - MI;      // X[NX - k] = X_h[m0] (h = 0) or X_h[m1] (h = 1)
  const cf zk = u[R2 * (MI % R1) + MI / R1], za = u[R2 * (m0 % R1) + m0 / R1], zb = u[R2 * (m1 % R1) + m1 / R1];
  const cf zn = cf{odd ? zb.x : za.x, odd ? zb.y : za.y};
  f(MI, make_float4(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y), 0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x)));
  if constexpr (2 * (MI + 1) <= M) fwd_rows_visit<NX, MI + 1>(u, odd, f);
}
// ---- writing T[kx][c/16][b][y][16] and the word of max |T| that the fp16 scale of the spectra derives from (Fp16Scale)
// entry k of channel pair p of row (b, y) lies at d0 + k * kstride, in units of two channels (t_fwd_index)
struct TRowDst {
  size_t d0, kstride;
  __device__ __forceinline__ TRowDst(int p, int b, int y, int B, int H, int C) : d0(t_fwd_index(0, p >> 5, p & 31, b, y, B, H, C)), kstride((size_t)(C >> 4) * B * H * 8) {}
};
__device__ __forceinline__ float max_abs4(float m, const float4& o) { return fmaxf(fmaxf(m, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w))); }
// the wave's maximum of m -> words[i] (null: nobody wants it): an atomic max, order independent (values >= 0 order like unsigned)
__device__ __forceinline__ void wave_max_to_word(float m, float* __restrict__ words, int i) {
  if (words) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(reinterpret_cast<unsigned*>(words + i), __float_as_uint(m));
  }
}
// this thread's outputs k = 2 m + h <= NX / 2 (the thread of odd parity has one less) as complex fp32; their maximum -> words[i]
template <int NX>
__device__ __forceinline__ void fwd_rows_store_f32(const cf (&u)[NX / 2], int h, float4* __restrict__ T, const TRowDst& d, float* __restrict__ words, int i) {
  float4* dst = T + d.d0;
  float m = 0.f;
  fwd_rows_visit<NX, 0>(u, h != 0, [&](int mi, const float4& o) __attribute__((always_inline)) {
    const int k = 2 * mi + h;
    if (k <= NX / 2) {
      dst[(size_t)k * d.kstride] = o;
      m = max_abs4(m, o);
    }
  });
  wave_max_to_word(m, words, i);
}
// the same as complex fp16 in block floating point: a wave is one (image, row, 64 channels) tile, whose scale derives from the wave's maximum (six shuffles,
// no barrier); *tinv = 1 / scale
template <int NX>
__device__ __forceinline__ void fwd_rows_store_bfp(const cf (&u)[NX / 2], int h, uint2* __restrict__ T, const TRowDst& d, float* __restrict__ tinv, float* __restrict__ words, int i) {
  const bool odd = h != 0;
  float m = 0.f;
  fwd_rows_visit<NX, 0>(u, odd, [&](int mi, const float4& o) __attribute__((always_inline)) {
    if (2 * mi + h <= NX / 2) m = max_abs4(m, o);
  });
  m = wave_max(m);
  const float sc = bfp_scale(m);
  if ((threadIdx.x & 63) == 0) {
    *tinv = 1.0f / sc;
    if (words && m > 0.f) atomicMax(reinterpret_cast<unsigned*>(words + i), __float_as_uint(m));
  }
  uint2* dst = T + d.d0;
  fwd_rows_visit<NX, 0>(u, odd, [&](int mi, const float4& o) __attribute__((always_inline)) {
    const int k = 2 * mi + h;
    if (k <= NX / 2) dst[(size_t)k * d.kstride] = make_uint2(pack_h2(o.x * sc, o.y * sc), pack_h2(o.z * sc, o.w * sc));
  });
}
// the forward transform and the stores of one row whose pixels sit in raw[] as bf16 pairs (thread h: pixels [h M, h M + M)), 16-bit T
template <int NX>
__device__ __forceinline__ void fwd_rows_finish(const unsigned (&raw)[NX / 2], uint2* __restrict__ T, int h, int p, int b, int y, int B, int H, int C, float* __restrict__ tmax,
                                                float* __restrict__ t16) {
  constexpr int M = NX / 2;
  const bool odd = h != 0;
  cf u[M];
  fwd_rows_in2<NX, 0>(u, raw, odd ? -1.f : 1.f, odd);
  step1<M, -1>(u);
  step2_inplace<M, -1, 0>(u);
  fwd_rows_store_bfp<NX>(u, h, T, TRowDst(p, b, y, B, H, C), t16 + ((size_t)b * (C >> 6) + (p >> 5)) * H + y, tmax, b);
}

// ---- the branch merge x = ((x1 + up(x2)) + up(x3)) / 3 (conv_fft_reg_fwd.hip, conv_fft_reg_fused.hip): the TF-1.x taps along x at compile time
template <int W, int WC> struct UpTaps {      // tf1_tap(x, WC, (float)WC / (float)W) at compile time
  static constexpr float scale = (float)WC / (float)W;
  static constexpr int lo(int x) { return (int)((float)x * scale); }
  static constexpr int hi(int x) { return lo(x) + 1 < WC ? lo(x) + 1 : WC - 1; }
  static constexpr float t(int x) { return (float)x * scale - (float)lo(x); }
};
template <int NX, int W, int W3> struct MergeGeom {
  static constexpr int M = NX / 2;
  using T3 = UpTaps<W, W3>;
  static constexpr int base3(int h) { return T3::lo(h * M); }
  static constexpr int span3(int h) { return T3::hi((h + 1) * M - 1 < W ? (h + 1) * M - 1 : W - 1) - base3(h) + 1; }
  static constexpr int N3 = span3(0) > span3(1) ? span3(0) : span3(1);      // x3 pixels a thread fetches per source row
  static constexpr int N2 = M / 2 + 1;                                        // x2 pixels (W = 2 W2: pixel j of either thread lerps locals j / 2 and j / 2 + 1)
};
__device__ __forceinline__ cf lerp_cf(cf a, cf b, float t) { return cf{fmaf(b.x - a.x, t, a.x), fmaf(b.y - a.y, t, a.y)}; }

// ---- the exchange between an inverse and a forward transform of the same two threads (adjacent lanes; conv_fft_reg_fused.hip, conv_fft_reg_tiles.hip):
// u_h[2 I], u_h[2 I + 1] of the forward transform from this thread's pixels a = z[2 I + h] and bq = z[2 I + h + M]
template <int NX, int I>
__device__ __forceinline__ void fwd_rows_mid_pair(const cf a, const cf bq, cf (&uu)[NX / 2], bool odd) {
  const cf sm = a + bq, df = a - bq;                         // j = 2 I + h:  z[j] + z[j + M],  z[j] - z[j + M]
  const cf keep = cf{odd ? df.x : sm.x, odd ? df.y : sm.y}, send = cf{odd ? sm.x : df.x, odd ? sm.y : df.y};
  const cf recv = lane_pair_swap(send);
  // thread 0: u[2 I] = its s, u[2 I + 1] = the neighbour's s;  thread 1: u[2 I] = the neighbour's d, u[2 I + 1] = its d -- times w^(-j) for the odd outputs
  cf e = cf{odd ? recv.x : keep.x, odd ? recv.y : keep.y}, o = cf{odd ? keep.x : recv.x, odd ? keep.y : recv.y};
  if constexpr (I > 0) {
    const float wr = odd ? Tw<-2 * I, NX>::re : 1.f, wi = odd ? Tw<-2 * I, NX>::im : 0.f;
    e = cf{fmaf(-e.y, wi, e.x * wr), fmaf(e.x, wi, e.y * wr)};
  }
  {
    const float wr = odd ? Tw<-(2 * I + 1), NX>::re : 1.f, wi = odd ? Tw<-(2 * I + 1), NX>::im : 0.f;
    o = cf{fmaf(-o.y, wi, o.x * wr), fmaf(o.x, wi, o.y * wr)};
  }
  uu[2 * I] = e;
  uu[2 * I + 1] = o;
}

}  // namespace cfft
}  // namespace jcm
