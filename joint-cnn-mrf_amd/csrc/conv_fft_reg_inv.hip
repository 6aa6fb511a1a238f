// Inverse passes with the transform in registers (fft_reg_rows.h): rows + epilogue, columns.
#include "fft_reg_rows.h"

namespace jcm {
namespace cfft {

// ---- rows, inverse + epilogue (the contract of rows_inv_kernel, conv_fft_rows_inv.hip): T'[b][y][kx][c] -> out, LAYOUT 0 = fp32 NHWC, 1 = bf16 NHWC,
// 2 = bf16 planar [B][C/8][H*W][8].  Planar: a 16-byte unit is 8 channels = the words of four threads, so the row goes through a per-wave LDS stage
// ([m][parity][32 channel pairs] words -- exactly the order in which the units are then read back, 16 bytes per lane, no barrier: one wave writes
// and reads its own stage) and leaves as 128-byte runs of 8 consecutive pixels per channel plane.
// Two threads per (image, row, channel pair), adjacent lanes: inv_rows_load2 / inv_rows_out2 (fft_reg_rows.h).
template <int NX, int LAYOUT, bool T16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NX >= 64 ? 2 : 4, NX >= 64 ? 2 : 8))) void rows_inv_reg_kernel(const void* __restrict__ T, void* __restrict__ out, const float* __restrict__ bias,
                                                                                              const float* __restrict__ scale, const float* __restrict__ shift, int relu_bn,
                                                                                              int nrows, int H, int W, int C, int Cout, int pad, float norm0, Fp16Scale sc,
                                                                                              int smH, int smW, int sTY, int sTX) {
  constexpr int M = NX / 2;
  __shared__ __attribute__((aligned(16))) unsigned stage[LAYOUT != 0 ? 4 * M * 64 : 4];      // bf16 outputs: one row (M x 2 pixels x 32 pairs) per wave
  int h, p;
  size_t by;
  pair_coords<true>(C >> 1, h, p, by);
  if (by >= (size_t)nrows) return;
  const int b = (int)(by / H), c = 2 * p;
  const bool odd = h != 0;
  const float sg = odd ? -1.f : 1.f;
  cf u[M];
  if constexpr (T16) {
    TInvRow16<NX> load;
    load.scales(sc, b, c, C);
    load.request(T, by, C, p);
    inv_rows_load2<NX, 0>(u, sg, odd, load);
  } else {
    inv_rows_load2<NX, 0>(u, sg, odd, TInvRow32<NX>(T, by, C, p));      // (in batches of LDB pairs: 49 x 16 bytes in flight at once do not fit the registers)
  }
  const Epilogue<false, true> act(bias, scale, shift, relu_bn, c, Cout, scale_undo(norm0, sc, b, scale_common(sc)));
  const bool two = c + 1 < Cout;
  step1<M, 1>(u);
  const int lane = threadIdx.x & 63;
  // scatter of overlap-save windows (sTX > 0; scalars: the row is the wave's): row `by` = valid row yv of window bw = (image, ty, tx)
  int sc_row = -1, sc_x0 = 0;
  if (LAYOUT == 0 && sTX > 0) {
    const int bw = (int)(by / H), yv = (int)(by % H);
    const int tx = bw % sTX, ty = (bw / sTX) % sTY, bi = bw / (sTX * sTY), ym = ty * H + yv;
    sc_row = ym < smH ? bi * smH + ym : -1;
    sc_x0 = tx * W;
  }
  unsigned* wst = stage + (LAYOUT != 0 ? (threadIdx.x >> 6) * (M * 64) : 0);
  auto store = [&](int m, int xo, cf z) __attribute__((always_inline)) {
    const cf v = act(z);
    if constexpr (LAYOUT == 0) {
      if (sTX > 0) {      // overlap-save windows: the valid region goes straight to its place in the map (the rows / columns of the last windows that hang over the map are dropped)
        const int xm = sc_x0 + xo;
        if (sc_row >= 0 && xm < smW) st_stream(reinterpret_cast<cf*>(static_cast<float*>(out) + ((size_t)sc_row * smW + xm) * Cout + c), v);
      } else {
        st_stream(reinterpret_cast<cf*>(static_cast<float*>(out) + (by * W + xo) * Cout + c), v);
      }
    } else {
      typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
      wst[(m * 2 + h) * 32 + (lane >> 1)] = __builtin_bit_cast(unsigned, bf16x2{static_cast<__bf16>(v.x), static_cast<__bf16>(v.y)});
    }
  };
  if (two || LAYOUT != 0) inv_rows_out2<NX, 0, LAYOUT != 0>(u, h, W, pad, store);      // (the launcher takes even channel counts only; bf16: whole 8-channel units)
  if constexpr (LAYOUT != 0) {
    // a wave = 32 channel pairs = eight 8-channel units of ONE row (C % 64 == 0); unit q = (m, parity, unit) lies at word 4 q of the stage
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int y = (int)(by % H);
    const int c0 = c - (lane >> 1) * 2;      // first channel of this wave
    const uint4* rd = reinterpret_cast<const uint4*>(wst);
#pragma unroll 4
    for (int q = lane; q < M * 16; q += 64) {
      const int m = q >> 4, hh = (q >> 3) & 1, j = q & 7;
      const int xo = 2 * m + hh - pad, cu = c0 + 8 * j;
      if (xo >= 0 && xo < W && cu < Cout) {
        __bf16* o = LAYOUT == 1 ? static_cast<__bf16*>(out) + (by * W + xo) * Cout + cu      // NHWC: the wave's 8 units of a pixel are one 128-byte run
                                : static_cast<__bf16*>(out) + (((size_t)b * (Cout >> 3) + (cu >> 3)) * H * W + (size_t)y * W + xo) * 8;      // planar: 8 consecutive pixels of a plane
        *reinterpret_cast<uint4*>(o) = rd[q];
      }
    }
  }
}

// ---- columns, inverse (the contract of cols_inv_kernel, conv_fft_cols.hip): Yf[ky][kx][b][ldy] -> T'[b][y][kx][c], y < H = row y + pad of the circular
// convolution.  ONE thread per (image, kx, channel): a 64-point transform is 128 registers.  Lanes are consecutive channels: every load is a 512-byte
// run of Yf, every store a 256- / 512-byte run of T'.  T16: the block-floating-point scale of the (image, kx, 64 channels) tile is the WAVE's maximum.
// T16 (bf16 handles, 16-bit intermediates): Yf holds complex FP16 = product * 2^-k (cgemm_split.hip, Y16) and T' is written as complex fp16 in block floating
// point; yinv = 2^k rides in the tile's scale word, so nothing is multiplied here.  A complex number is 4 bytes then: the two lanes of adjacent channels
// (c, c + 1) share their accesses -- the even lane fetches (c, c + 1) of the even ky and stores both channels of the even output rows, the odd lane the
// odd ones, 8 bytes per lane, and they swap the halves they fetched for each other (lane_pair_swap) -- half the memory instructions of one 4-byte access per lane.
template <int NY, bool T16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NY >= 64 ? 2 : 3, NY >= 64 ? 2 : 8))) void cols_inv_reg_kernel(const cf* __restrict__ Yf, void* __restrict__ T, int B, int H, int NXH, int C, int ldy,
                                                                                              int pad, float* __restrict__ t16, float yinv) {
  static_assert(NY % 2 == 0, "ky pairs");
  constexpr int R1 = RPlan<NY>::R1, R2 = RPlan<NY>::R2;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(g % C);
  // (image, kx) are the same for the 64 lanes of a wave (C % 64 == 0): scalar registers, so that every address below is a scalar base + lane offset
  const unsigned bk = (unsigned)__builtin_amdgcn_readfirstlane((int)(g / C));
  const int kx = (int)(bk % (unsigned)NXH), b = (int)(bk / (unsigned)NXH);
  if (b >= B) return;
  const bool odd = (c & 1) != 0;      // = the lane's parity (C is even)
  cf x[NY];
  if constexpr (T16) {
    const uint2* src = reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned*>(Yf) + ((size_t)kx * NY * B + b) * ldy + (c & ~1));      // ldy is even
    const size_t kstep = (size_t)B * ldy / 2;
    uint2 raw[NY / 2];      // every load goes out before the first conversion (left to itself the compiler waits for each load in turn)
#pragma unroll
    for (int i = 0; i < NY / 2; ++i) raw[i] = src[(size_t)(2 * i + (odd ? 1 : 0)) * kstep];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NY / 2; ++i) {
      const unsigned keep = odd ? raw[i].y : raw[i].x, recv = lane_pair_swap(odd ? raw[i].x : raw[i].y);
      x[2 * i] = unpack_h2(odd ? recv : keep, 1.f);
      x[2 * i + 1] = unpack_h2(odd ? keep : recv, 1.f);
    }
  } else {
    const cf* src = Yf + ((size_t)kx * NY * B + b) * ldy + c;
#pragma unroll
    for (int ky = 0; ky < NY; ++ky) x[ky] = src[(size_t)ky * B * ldy];
  }
  step1<NY, 1>(x);
  step2_inplace<NY, 1, 0>(x);      // x[R2 k1 + k2] = X[k1 + R1 k2]
  if constexpr (T16) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      const int y = (i / R2) + R1 * (i % R2) - pad;      // x[i] = X[i / R2 + R1 (i % R2)]
      if (y >= 0 && y < H) m = fmaxf(m, fmaxf(fabsf(x[i].x), fabsf(x[i].y)));
    }
    const float s = bfp_scale(wave_max(m));
    if ((threadIdx.x & 63) == 0) t16[((size_t)b * (C >> 6) + (c >> 6)) * NXH + kx] = (1.0f / s) * yinv;      // powers of two: exact
    uint2* dst = reinterpret_cast<uint2*>(reinterpret_cast<unsigned*>(T) + ((size_t)b * H * NXH + kx) * C + (c & ~1));
    const size_t ystep = (size_t)NXH * C / 2;
#pragma unroll
    for (int k = 0; k < NY; k += 2) {      // output samples X[k], X[k + 1] = rows k - pad, k + 1 - pad: the even lane stores the first, the odd lane the second
      const int ia = R2 * (k % R1) + k / R1, ib = R2 * ((k + 1) % R1) + (k + 1) / R1;
      const unsigned va = pack_h2(x[ia].x * s, x[ia].y * s), vb = pack_h2(x[ib].x * s, x[ib].y * s);
      const unsigned recv = lane_pair_swap(odd ? va : vb);
      const int y = k - pad + (odd ? 1 : 0);
      if (y >= 0 && y < H) st_stream(dst + (size_t)y * ystep, make_uint2(odd ? recv : va, odd ? vb : recv));
    }
  } else {
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      const int y = (i / R2) + R1 * (i % R2) - pad;
      if (y >= 0 && y < H) st_stream(reinterpret_cast<cf*>(T) + ((size_t)(b * H + y) * NXH + kx) * C + c, x[i]);
    }
  }
}
// true: launched (64-point columns, 64-channel tiles)
bool cfft_cols_inv_reg(int NY, const FftArgs& a, const cf* Yf, cf* T, int NXH, int ldy, int pad, hipStream_t st, float* t16, float y16_inv) {
  if (a.CoutP % 64 || ((y16_inv != 0.f) != (t16 != nullptr)) || (t16 && ldy % 2)) return false;      // 16-bit T' comes with fp16 product spectra
  const size_t threads = (size_t)a.B * NXH * a.CoutP;
  const dim3 grid((unsigned)((threads + 255) / 256)), blk(256);
#define CI_LAUNCH(N)                                                                                                                                             \
  do {                                                                                                                                                           \
    if (t16) hipLaunchKernelGGL((cols_inv_reg_kernel<N, true>), grid, blk, 0, st, Yf, static_cast<void*>(T), a.B, a.H, NXH, a.CoutP, ldy, pad, t16, y16_inv);            \
    else hipLaunchKernelGGL((cols_inv_reg_kernel<N, false>), grid, blk, 0, st, Yf, static_cast<void*>(T), a.B, a.H, NXH, a.CoutP, ldy, pad, nullptr, 0.f);          \
  } while (0)
  switch (NY) {      // 64: the 60 x 90 maps; 36 / 20: the half- and quarter-resolution branches; 32: the training step's overlap-save windows
    case 64: CI_LAUNCH(64); break;
    case 36: CI_LAUNCH(36); break;
    case 32: CI_LAUNCH(32); break;
    case 20: CI_LAUNCH(20); break;
    default: return false;
  }
#undef CI_LAUNCH
  return true;
}

template <int NX> static bool launch_rows_inv_reg(const FftArgs& a, FftLayout layout, const cf* T, int pad, float norm, const Fp16Scale& sc, hipStream_t st) {
  const int nrows = a.B * a.H;
  if (a.win_scatter && (layout != kFftF32Nhwc || sc.t16_inv)) return false;      // the scatter of overlap-save windows exists for fp32 outputs
  if ((a.Cout & 1) || a.CoutP % 64) return false;      // channel pairs are stored as one word; a wave = 32 pairs of ONE row (the kernel keeps the row in scalar registers)
  const size_t threads = (size_t)nrows * a.CoutP;      // two threads per channel pair
  const dim3 grid((unsigned)((threads + 255) / 256)), blk(256);
  const bool h16 = sc.t16_inv != nullptr;
  const WinGeom wout = a.win_scatter ? a.win : WinGeom{};      // TY = 0: the kernel stores the batch of valid regions
#define RR_LAUNCH(L, H16) hipLaunchKernelGGL((rows_inv_reg_kernel<NX, L, H16>), grid, blk, 0, st, T, a.out, a.bias, a.scale, a.shift, a.relu_bn, nrows, a.H, a.W, a.CoutP, a.Cout, pad, norm, sc, wout.H, wout.W, wout.TY, wout.TX)
  if (layout == kFftF32Nhwc && !h16) RR_LAUNCH(0, false);
  else if (layout == kFftBf16Nhwc && h16 && a.Cout % 8 == 0) RR_LAUNCH(1, true);
  else if (layout == kFftBf16Nhwc && a.Cout % 8 == 0) RR_LAUNCH(1, false);
  else if (layout == kFftBf16Planar && h16 && a.Cout % 8 == 0) RR_LAUNCH(2, true);
  else if (layout == kFftBf16Planar && a.Cout % 8 == 0) RR_LAUNCH(2, false);
  else return false;
#undef RR_LAUNCH
  return true;
}
// true: launched.  false: no register kernel for this (length, layout) -- the caller takes the LDS kernel.
bool cfft_rows_inv_reg(int NX, const FftArgs& a, FftLayout layout, const cf* T, int pad, float norm, const Fp16Scale& sc, hipStream_t st) {
  if (NX == 96) return launch_rows_inv_reg<96>(a, layout, T, pad, norm, sc, st);
  if (NX == 32 && layout == kFftF32Nhwc) return launch_rows_inv_reg<32>(a, layout, T, pad, norm, sc, st);      // the training step's overlap-save windows (fp32)
  if (NX == 50) return launch_rows_inv_reg<50>(a, layout, T, pad, norm, sc, st);      // the half- and quarter-resolution branches (36 x 50, 20 x 28 transforms)
  if (NX == 28) return launch_rows_inv_reg<28>(a, layout, T, pad, norm, sc, st);
  return false;
}

}  // namespace cfft
}  // namespace jcm
