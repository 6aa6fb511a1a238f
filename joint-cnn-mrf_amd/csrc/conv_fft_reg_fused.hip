// Fused hand-overs between two frequency-domain layers with both transforms in registers (fft_reg_rows.h): plain, and with the branch merge in between.
#include "fft_reg_rows.h"
#include "resize_tf1.h"

namespace jcm {
namespace cfft {

// ---- rows, inverse of layer L + epilogue + rows, forward of layer L+1 (the contract of rows_inv_fwd_kernel, conv_fft_rows_inv.hip; fp32 handles): the activation
// between two frequency-domain layers never goes to HBM.  Two threads per channel pair.  The inverse (decimation in frequency) leaves thread h with the pixels of
// parity h (the kernel's pad is even).  The forward transform wants u_h[j] = (z[j] + (-1)^h z[j + M]) w^(j h), j < M = NX / 2: pixels j and j + M have the same
// parity, so the thread of parity j % 2 forms s = z[j] + z[j + M] and d = z[j] - z[j + M] for ITS 24 values of j, keeps the one its own transform needs
// (thread 0: s, thread 1: d) and swaps the other with its neighbour (DPP) -- 24 complex numbers cross lanes, nothing goes through LDS (fwd_rows_mid_pair).
template <int NX, int PAD, int I, class Act>
__device__ __forceinline__ void fused_rows_mid(const cf (&x)[NX / 2], cf (&uu)[NX / 2], bool odd, int h, int W, Act&& act) {
  constexpr int M = NX / 2, R1 = RPlan<M>::R1, R2 = RPlan<M>::R2, Q = M / 2;
  // this thread's pixels n = 2 i + h, i < M:  the inverse's output X[2 (i + PAD / 2) + h], activated; zero behind the map (the next layer's padding)
  constexpr int ma = I + PAD / 2, mb = I + Q + PAD / 2;      // sample indices of pixels 2 I + h and 2 (I + Q) + h
  cf a = cf{0.f, 0.f}, bq = cf{0.f, 0.f};
  if constexpr (ma < M) { if (2 * I + h < W) a = act(x[R2 * (ma % R1) + ma / R1]); }
  if constexpr (mb < M) { if (2 * (I + Q) + h < W) bq = act(x[R2 * (mb % R1) + mb / R1]); }
  fwd_rows_mid_pair<NX, I>(a, bq, uu, odd);
  if constexpr (I + 1 < Q) fused_rows_mid<NX, PAD, I + 1>(x, uu, odd, h, W, act);
}
template <int NX, int PAD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void rows_inv_fwd_reg_kernel(const float4* __restrict__ T, float4* __restrict__ Tn, const float* __restrict__ bias,
                                                                                                  const float* __restrict__ scale, const float* __restrict__ shift, int relu_bn, int nrows,
                                                                                                  int B, int H, int W, int C, float norm0, Fp16Scale sc) {
  constexpr int M = NX / 2;
  const int CP = C >> 1;
  int h, p;
  size_t by;
  pair_coords<true>(CP, h, p, by);
  if (by >= (size_t)nrows) return;
  const int b = (int)(by / H), y = (int)(by % H), c = 2 * p;
  const bool odd = h != 0;
  cf u[M];
  {
    const float4* src = T + (by * (M + 1) * C) / 2 + p;
    auto load = [&](int k) __attribute__((always_inline)) { return src[(size_t)k * CP]; };      // (Ya.re, Ya.im, Yb.re, Yb.im)
    inv_rows_load2<NX, 0>(u, odd ? -1.f : 1.f, odd, load);
  }
  const Epilogue<> act(bias, scale, shift, relu_bn, c, C, scale_undo(norm0, sc, b, scale_common(sc)));
  step1<M, 1>(u);
  step2_inplace<M, 1, 0>(u);      // u[R2 (m % R1) + m / R1] = X[2 m + h]: the pixel 2 m + h - PAD of this thread's parity
  cf uu[M];
  fused_rows_mid<NX, PAD, 0>(u, uu, odd, h, W, act);
  step1<M, -1>(uu);
  step2_inplace<M, -1, 0>(uu);
  fwd_rows_store_f32<NX>(uu, h, Tn, TRowDst(p, b, y, B, H, C), sc.tmax_next, b);      // + the next layer's per-image word (max |T|) of its spectra's scale
}
// true: launched (96-point rows, pad 2 or 4, whole 64-channel blocks)
bool cfft_rows_inv_fwd_reg(int NX, const FftArgs& a, const cf* T, cf* Tn, int pad, float norm, const Fp16Scale& sc, hipStream_t st) {
  if (NX != 96 || (pad != 2 && pad != 4) || a.Cout % 64 || a.W > NX) return false;
  const int nrows = a.B * a.H;
  const size_t threads = (size_t)nrows * a.Cout;
  const dim3 grid((unsigned)((threads + 255) / 256)), blk(256);
  if (pad == 4) hipLaunchKernelGGL((rows_inv_fwd_reg_kernel<96, 4>), grid, blk, 0, st, reinterpret_cast<const float4*>(T), reinterpret_cast<float4*>(Tn), a.bias, a.scale, a.shift, a.relu_bn, nrows, a.B, a.H, a.W, a.Cout, norm, sc);
  else hipLaunchKernelGGL((rows_inv_fwd_reg_kernel<96, 2>), grid, blk, 0, st, reinterpret_cast<const float4*>(T), reinterpret_cast<float4*>(Tn), a.bias, a.scale, a.shift, a.relu_bn, nrows, a.B, a.H, a.W, a.Cout, norm, sc);
  return true;
}

// ---- rows, inverse of the full-resolution branch's conv4 + epilogue + BRANCH MERGE + rows, forward of conv5 (the contract of rows_inv_merge_fwd_kernel,
// conv_fft_rows_fused.hip, for the model's geometry: 90-column maps, x2 at half and x3 at a quarter of the width): x1 never reaches HBM.
// rows_inv_fwd_reg_kernel with one more step between the transforms: merged = ((act(x1) + up(x2)) + up(x3)) / 3 (main.py:58,67,69-70).  The coarse rows a
// fine row needs -- two source rows of x2 and of x3 -- are lerped ALONG Y FIRST by the wave that owns the row (the same for its 32 channel pairs: the row
// taps are scalars) and staged in the wave's own LDS slice as [x2: 45 columns + a copy of the last | x3: 23 columns][32 pairs]; the lerp along x then
// reads two staged neighbours per map at compile-time offsets (x2: columns i, i + 1 with weight 0 or 1/2 by the thread's parity; x3: the TF-1.x taps of
// UpTaps<90, 23>, the thread's parity picks between two literals).  TF lerps along x first: the two orders differ in the last fp32 bit of the coarse terms
// (as in rows_fwd_merge_reg_kernel), eight orders of magnitude below the 1e-4 the heat maps are held to.  No work-group barrier: a wave reads what it wrote.
// BF (bf16 handles): the three branches are bf16 tensors and so is the merged map -- act() rounds x1 to bf16, the lerps are the FMA forms of
// rows_fwd_merge_reg_kernel, the merged value is rounded to bf16 before it enters conv5's transform.
template <int NX, int PAD, int W, int W3, int IPX, bool BF, class Act>
__device__ __forceinline__ cf merged_px(cf z, bool odd, const cf* c2, const cf* c3, float t2h, Act&& act) {      // pixel n = 2 IPX + h of this thread
  using T3 = UpTaps<W, W3>;
  const cf a = act(z);
  const cf l2 = c2[IPX * 32], r2 = c2[(IPX + 1) * 32];
  constexpr int n0 = 2 * IPX, n1 = 2 * IPX + 1;
  const int lo = odd ? T3::lo(n1) * 32 : T3::lo(n0) * 32, hi = odd ? T3::hi(n1) * 32 : T3::hi(n0) * 32;
  const float t3 = odd ? T3::t(n1) : T3::t(n0);
  const cf l3 = c3[lo], r3 = c3[hi];
  if constexpr (BF) {
    const cf u2 = lerp_cf(l2, r2, t2h), u3 = lerp_cf(l3, r3, t3);
    // the third as ONE multiplication by RN(1/3), as rows_fwd_merge_reg_kernel forms it: the two kernels are bit-identical arms of a bf16 handle.  (Against the
    // correctly rounded quotient the product differs in the last fp32 bit for a third of the values, which moves the bf16 rounding of two values in a million.)
    constexpr float k3 = 0.333333343267440796f;
    return cf{bf16_rn(((a.x + u2.x) + u3.x) * k3), bf16_rn(((a.y + u2.y) + u3.y) * k3)};
  } else {
    const cf u2 = cf{l2.x + (r2.x - l2.x) * t2h, l2.y + (r2.y - l2.y) * t2h};
    const cf u3 = cf{l3.x + (r3.x - l3.x) * t3, l3.y + (r3.y - l3.y) * t3};
    return cf{div3((a.x + u2.x) + u3.x), div3((a.y + u2.y) + u3.y)};
  }
}
template <int NX, int PAD, int W, int W3, int I, bool BF, class Act>
__device__ __forceinline__ void fused_rows_mid_merge(const cf (&x)[NX / 2], cf (&uu)[NX / 2], bool odd, const cf* c2, const cf* c3, float t2h, Act&& act) {
  constexpr int M = NX / 2, R1 = RPlan<M>::R1, R2 = RPlan<M>::R2, Q = M / 2;
  static_assert(W % 2 == 0 && PAD % 2 == 0, "a thread's pixels 2 i + h are inside the map for both parities or for neither");
  constexpr int ma = I + PAD / 2, mb = I + Q + PAD / 2;      // sample indices of pixels 2 I + h and 2 (I + Q) + h
  cf a = cf{0.f, 0.f}, bq = cf{0.f, 0.f};
  if constexpr (ma < M && 2 * I < W) a = merged_px<NX, PAD, W, W3, I, BF>(x[R2 * (ma % R1) + ma / R1], odd, c2, c3, t2h, act);
  if constexpr (mb < M && 2 * (I + Q) < W) bq = merged_px<NX, PAD, W, W3, I + Q, BF>(x[R2 * (mb % R1) + mb / R1], odd, c2, c3, t2h, act);
  fwd_rows_mid_pair<NX, I>(a, bq, uu, odd);
  if constexpr (I % 2 == 1) asm volatile("" ::: "memory");      // two steps' staged reads at a time (the compiler otherwise hoists all of them to the front)
  if constexpr (I + 1 < Q) fused_rows_mid_merge<NX, PAD, W, W3, I + 1, BF>(x, uu, odd, c2, c3, t2h, act);
}
// BF = false: fp32 handles (T' and T complex fp32, x2 / x3 fp32 NHWC).  BF = true: bf16 handles on the one-part route -- T' and T complex fp16 in block floating
// point (sc.t16_inv: the scale words of T'; t16n: those of the T written here, one per (image, row, 64 channels) = per wave), x2 / x3 bf16 NHWC.
template <int NX, int PAD, int W, int W2, int W3, bool BF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void rows_inv_merge_fwd_reg_kernel(const void* __restrict__ T, void* __restrict__ Tn, const float* __restrict__ bias,
                                                                                                        const float* __restrict__ scale, const float* __restrict__ shift, int relu_bn,
                                                                                                        int nrows, int B, int H, int C, float norm0, Fp16Scale sc,
                                                                                                        const void* __restrict__ x2, int H2, const void* __restrict__ x3, int H3, float sy2,
                                                                                                        float sy3, float* __restrict__ t16n) {
  constexpr int NXH = NX / 2 + 1, M = NX / 2;
  constexpr int NC2 = W2 + 1, NCS = NC2 + W3 + 1;      // staged columns per wave: x2 (+ a copy of its last column), x3 (+ one the loop below writes and nobody reads)
  static_assert(W == 2 * W2 && W2 % 2 == 1 && W3 % 2 == 1, "the staging loops below walk the coarse columns in pairs");
  __shared__ cf stage[4][NCS * 32];
  const int CP = C >> 1;
  const int lane = threadIdx.x & 63;
  int h, p;
  size_t by;
  pair_coords<true>(CP, h, p, by, C == 512);
  if (by >= (size_t)nrows) return;
  const int b = (int)(by / H), y = (int)(by % H), c = 2 * p;
  const bool odd = h != 0;
  cf* cs = stage[threadIdx.x >> 6];
  // bf16 handles: T' (complex fp16) goes out FIRST -- 49 eight-byte loads per thread that stay in flight under the coarse rows' loads, lerps and LDS stores
  // (the kernel is bound by the latency of its dependent memory round trips at two waves per SIMD: one round trip less).  fp32 handles load T' in batches
  // behind the staging (a thread cannot hold 49 x 16 bytes next to the coarse rows).
  TInvRow16<NX> t16;
  if constexpr (BF) t16.request(T, by, C, p);
  {
    // the wave's coarse rows: lanes 0..31 take an even column of the wave's 32 channel pairs, lanes 32..63 the odd one next to it; the image is the
    // descriptor, the source row and the column pair scalar offsets
    constexpr int EB = BF ? 4 : 8;      // bytes of a channel pair
    const int bs = __builtin_amdgcn_readfirstlane(b), c0 = __builtin_amdgcn_readfirstlane(p - (lane >> 1));      // first pair of the wave
    const Tap ty2 = tf1_tap(y, H2, sy2), ty3 = tf1_tap(y, H3, sy3);
    const auto d2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(x2)) + (size_t)bs * H2 * W2 * CP * EB, 0, H2 * W2 * CP * EB, 0x00020000);
    const auto d3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(x3)) + (size_t)bs * H3 * W3 * CP * EB, 0, H3 * W3 * CP * EB, 0x00020000);
    const int vo = ((lane >> 5) * CP + c0 + (lane & 31)) * EB, vo_last = (c0 + (lane & 31)) * EB;      // (the last column pair: both halves read the last column)
    const int r2a = ty2.lo * W2 * CP * EB, r2b = ty2.hi * W2 * CP * EB, r3a = ty3.lo * W3 * CP * EB, r3b = ty3.hi * W3 * CP * EB;
    typedef float f2 __attribute__((ext_vector_type(2)));
    constexpr int J2 = (W2 + 1) / 2, J3 = (W3 + 1) / 2;
    auto ld = [&](const auto& d, int v, int so) __attribute__((always_inline)) {
      if constexpr (BF) return bf16pair(__builtin_amdgcn_raw_buffer_load_b32(d, v, so, 0));
      else return cf(__builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(d, v, so, 0)));
    };
    auto ylerp = [&](cf a, cf bb, float t) __attribute__((always_inline)) {
      if constexpr (BF) return lerp_cf(a, bb, t);
      else return cf{a.x + (bb.x - a.x) * t, a.y + (bb.y - a.y) * t};
    };
    cf a2[J2], b2[J2], a3[J3], b3[J3];
#pragma unroll
    for (int j = 0; j < J2; ++j) {
      const int v = j == J2 - 1 ? vo_last : vo;
      a2[j] = ld(d2, v, r2a + 2 * j * CP * EB);
      b2[j] = ld(d2, v, r2b + 2 * j * CP * EB);
    }
#pragma unroll
    for (int j = 0; j < J3; ++j) {
      const int v = j == J3 - 1 ? vo_last : vo;
      a3[j] = ld(d3, v, r3a + 2 * j * CP * EB);
      b3[j] = ld(d3, v, r3b + 2 * j * CP * EB);
    }
    __builtin_amdgcn_sched_barrier(0);      // every load is out before the first lerp
#pragma unroll
    for (int j = 0; j < J2; ++j) cs[lane + 64 * j] = ylerp(a2[j], b2[j], ty2.t);
#pragma unroll
    for (int j = 0; j < J3; ++j) cs[NC2 * 32 + lane + 64 * j] = ylerp(a3[j], b3[j], ty3.t);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  cf u[M];
  if constexpr (BF) {
    t16.scales(sc, b, c, C);      // T' as complex fp16 in block floating point (requested above)
    inv_rows_load2<NX, 0>(u, odd ? -1.f : 1.f, odd, t16);
  } else {
    const float4* src = static_cast<const float4*>(T) + (by * NXH * C) / 2 + p;
    auto load = [&](int k) __attribute__((always_inline)) { return src[(size_t)k * CP]; };      // (Ya.re, Ya.im, Yb.re, Yb.im)
    inv_rows_load2<NX, 0>(u, odd ? -1.f : 1.f, odd, load);
  }
  const Epilogue<BF> act(bias, scale, shift, relu_bn, c, C, scale_undo(norm0, sc, b, scale_common(sc)));      // BF: x1 is a bf16 tensor
  step1<M, 1>(u);
  step2_inplace<M, 1, 0>(u);      // u[R2 (m % R1) + m / R1] = X[2 m + h]: the pixel 2 m + h - PAD of this thread's parity
  cf uu[M];
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const cf* c2 = cs + (lane >> 1);
  fused_rows_mid_merge<NX, PAD, W, W3, 0, BF>(u, uu, odd, c2, c2 + NC2 * 32, odd ? 0.5f : 0.f, act);
  step1<M, -1>(uu);
  step2_inplace<M, -1, 0>(uu);
  // conv5's T, + the tile's scale word (bf16 handles: a wave is one (image, row, 64 channels) tile) and the next layer's per-image word (max |T|) of its spectra's scale
  const TRowDst d(p, b, y, B, H, C);
  if constexpr (BF) fwd_rows_store_bfp<NX>(uu, h, static_cast<uint2*>(Tn), d, t16n + ((size_t)b * (C >> 6) + (p >> 5)) * H + y, sc.tmax_next, b);
  else fwd_rows_store_f32<NX>(uu, h, static_cast<float4*>(Tn), d, sc.tmax_next, b);
}
// true: launched (the model's geometry: 96-point rows, pad 4, 90 / 45 / 23 columns, whole 64-channel blocks)
bool cfft_rows_inv_merge_fwd_reg_supported(int NX, const ConvArgs& a, const FftMerge& m, int pad) {
  if (NX != 96 || pad != 4 || a.Cout % 64 || a.W != 90 || m.W2 != 45 || m.W3 != 23 || m.H2 < 1 || m.H3 < 1) return false;
  return (size_t)m.H2 * m.W2 * a.Cout * 4 < (size_t)1 << 31;      // one buffer descriptor per coarse image
}
// t16n: null = fp32 handles (T', T complex fp32; x2, x3 fp32 NHWC); else the scale words of the 16-bit T written here (bf16 handles: T' 16-bit with sc.t16_inv, x2 / x3 bf16 NHWC)
bool cfft_rows_inv_merge_fwd_reg(int NX, const FftArgs& a, const FftMerge& m, const cf* T, cf* Tn, int pad, float norm, const Fp16Scale& sc, hipStream_t st, float* t16n) {
  if (!cfft_rows_inv_merge_fwd_reg_supported(NX, a, m, pad) || ((t16n != nullptr) != (sc.t16_inv != nullptr))) return false;
  const int nrows = a.B * a.H;
  const size_t threads = a.Cout == 512 ? (size_t)((nrows + 3) / 4) * 8 * 256 : (size_t)nrows * a.Cout;      // (512 channels: eight work groups per four rows)
  const dim3 grid((unsigned)((threads + 255) / 256)), blk(256);
  const float sy2 = (float)m.H2 / (float)a.H, sy3 = (float)m.H3 / (float)a.H;
  if (t16n)
    hipLaunchKernelGGL((rows_inv_merge_fwd_reg_kernel<96, 4, 90, 45, 23, true>), grid, blk, 0, st, static_cast<const void*>(T), static_cast<void*>(Tn), a.bias, a.scale, a.shift, a.relu_bn, nrows, a.B,
                       a.H, a.Cout, norm, sc, m.x2, m.H2, m.x3, m.H3, sy2, sy3, t16n);
  else
    hipLaunchKernelGGL((rows_inv_merge_fwd_reg_kernel<96, 4, 90, 45, 23, false>), grid, blk, 0, st, static_cast<const void*>(T), static_cast<void*>(Tn), a.bias, a.scale, a.shift, a.relu_bn, nrows, a.B,
                       a.H, a.Cout, norm, sc, m.x2, m.H2, m.x3, m.H3, sy2, sy3, nullptr);
  return true;
}

}  // namespace cfft
}  // namespace jcm
