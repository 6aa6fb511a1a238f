// Forward row passes with the transform in registers (fft_reg_rows.h): of a plain map, of overlap-save windows, of the merged map.
#include "fft_reg_rows.h"
#include "resize_tf1.h"

namespace jcm {
namespace cfft {

// ---- rows, forward (the contract of rows_fwd_kernel<NX, 1, T16 = true>, conv_fft_rows_fwd.hip): bf16 NHWC -> T16[kx][c/16][b][y][16], complex fp16 in block floating
// point, one scale per (image, row, 64 channels) tile.  Two threads per channel pair again; the forward transform is decimation in frequency as well, so thread h
// produces the outputs of parity h:  X[2 m + h] = sum_{j < M} u_h[j] w_M^(j m),  u_h[j] = (z[j] + (-1)^h z[j + M]) w_NX^(j h),  z = x_c + i x_{c+1}.
// Thread h LOADS pixels [h M, h M + M) only and swaps words with the other thread of the pair: each pixel is fetched once.  The Hermitian split into the two channels'
// spectra pairs X[k] with X[NX - k], which has the parity of k: both live in the same thread (at a lane-selected register).  A wave is the 32 channel pairs =
// 64 channels of one row = one block-floating-point tile: its scale is the wave's maximum (six shuffles, no barrier).  The rest: fwd_rows_finish, fft_reg_rows.h.
template <int NX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NX >= 96 ? 3 : 4, NX >= 96 ? 3 : 8))) void rows_fwd_reg_kernel(const unsigned* __restrict__ in, uint2* __restrict__ T, int nrows, int B, int H, int W, int C,
                                                                                              float* __restrict__ tmax, float* __restrict__ t16) {
  constexpr int M = NX / 2;
  const int CP = C >> 1;
  int h, p;
  size_t by;
  pair_coords<false>(CP, h, p, by);
  if (by >= (size_t)nrows) return;
  const int b = (int)(by / H), y = (int)(by % H);
  const unsigned* src = in + (by * W) * CP + p;      // a word = channels (2 p, 2 p + 1) of a pixel
  unsigned raw[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int n = h * M + j;
    raw[j] = n < W ? src[(size_t)n * CP] : 0u;
  }
  fwd_rows_finish<NX>(raw, T, h, p, b, y, B, H, C, tmax, t16);
}
// true: launched (96- / 50- / 28-point rows of a bf16 NHWC tensor -- the 60 x 90, 30 x 45 and 15 x 23 maps --, 16-bit T; W <= NX)
bool cfft_rows_fwd_reg(int NX, const FftArgs& a, FftLayout layout, cf* T, float* tmax, hipStream_t st, float* t16) {
  if ((NX != 96 && NX != 50 && NX != 28) || layout != kFftBf16Nhwc || !t16 || a.Cin % 64 || a.W > NX) return false;
  const int nrows = a.B * a.H;
  const size_t threads = (size_t)nrows * a.Cin;      // two threads per channel pair
  const dim3 grid((unsigned)((threads + 255) / 256)), blk(256);
#define RFR_LAUNCH(N) hipLaunchKernelGGL(rows_fwd_reg_kernel<N>, grid, blk, 0, st, static_cast<const unsigned*>(a.x), reinterpret_cast<uint2*>(T), nrows, a.B, a.H, a.W, a.Cin, tmax, t16)
  if (NX == 96) RFR_LAUNCH(96);
  else if (NX == 50) RFR_LAUNCH(50);      // (round 6: the half- and quarter-resolution branches left the LDS kernel too)
  else RFR_LAUNCH(28);
#undef RFR_LAUNCH
  return true;
}

// ---- rows, forward, of OVERLAP-SAVE WINDOWS read straight from the map they are cut from (fp32 handles, the training step's 32 x 32 windows; the contract of
// window_gather_kernel + rows_fwd_kernel<32, 0>): ONE thread per (window row, channel pair) -- a 32-point transform is 64 registers.  A wave is 64 channel
// pairs of one window row (Cin % 128 == 0), so the window, its row and the validity of each of its 32 pixels are scalars: a pixel inside the map is one buffer
// load (the map row is the descriptor, the column a scalar offset, the lane's channel pair the vector offset), a pixel outside it -- or in the 4-pixel halo
// when the caller wants the valid region only (the weight gradient's dZ) -- a literal zero.  The gathered window tensor (0.4 GB per conv5 pass at 16 images)
// is never written or read.
template <int NX>
__global__ __launch_bounds__(256) void rows_fwd_win_reg_kernel(const float* __restrict__ map, float4* __restrict__ T, int nrows, int BW, int H, int W, int C, int TY, int TX,
                                                               int valid_only, float* __restrict__ tmax) {
  constexpr int NXH = NX / 2 + 1, R1 = RPlan<NX>::R1, R2 = RPlan<NX>::R2, V = NX - 8;
  const int CP = C >> 1;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int p = (int)(g % CP);
  const int row = __builtin_amdgcn_readfirstlane((int)(g / CP));      // (window, wy): the same for the 64 lanes (C % 128 == 0)
  if (row >= nrows) return;
  const int wy = row % NX, bw = row / NX;
  const int tx = bw % TX, ty = (bw / TX) % TY, b = bw / (TX * TY);
  const int y = ty * V - 4 + wy, x0 = tx * V - 4;
  const bool row_in = y >= 0 && y < H && !(valid_only && (wy < 4 || wy >= NX - 4));
  cf z[NX];
  {
    const auto d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(map) + ((size_t)b * H + (row_in ? y : 0)) * W * C, 0, W * C * 4, 0x00020000);
    typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int wx = 0; wx < NX; ++wx) {
      const int x = x0 + wx;
      const bool in = row_in && x >= 0 && x < W && !(valid_only && (wx < 4 || wx >= NX - 4));      // wave-uniform
      z[wx] = cf{0.f, 0.f};
      if (in) z[wx] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(d, p * 8, x * C * 4, 0));
    }
  }
  step1<NX, -1>(z);
  step2_inplace<NX, -1, 0>(z);      // z[R2 (k % R1) + k / R1] = Z[k]
  // Z = FFT(x_c + i x_{c+1}):  X_c[k] = (Z[k] + conj Z[-k]) / 2,  X_{c+1}[k] = (Z[k] - conj Z[-k]) / (2i)  ->  T[kx][c/16][window][wy][16]
  const TRowDst d(p, bw, wy, BW, NX, C);
  float4* dst = T + d.d0;
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < NXH; ++k) {
    const int kn = k == 0 ? 0 : NX - k;
    const cf zk = z[R2 * (k % R1) + k / R1], zn = z[R2 * (kn % R1) + kn / R1];
    const float4 o = make_float4(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y), 0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
    dst[(size_t)k * d.kstride] = o;
    m = max_abs4(m, o);
  }
  wave_max_to_word(m, tmax, bw);      // the window's word of the spectra's scale
}
bool cfft_rows_fwd_win_reg_supported(int NX, int Cin) { return NX == 32 && Cin % 128 == 0; }
bool cfft_rows_fwd_win_reg(int NX, const FftArgs& a, cf* T, float* tmax, hipStream_t st) {
  if (!a.win_map || !cfft_rows_fwd_win_reg_supported(NX, a.Cin) || a.H != NX || a.W != NX || a.B != a.win.BW()) return false;
  if ((size_t)a.win.W * a.Cin * 4 >= (size_t)1 << 31) return false;
  const int nrows = a.B * NX;
  const size_t threads = (size_t)nrows * (a.Cin / 2);
  hipLaunchKernelGGL(rows_fwd_win_reg_kernel<32>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, static_cast<const float*>(a.win_map), reinterpret_cast<float4*>(T), nrows, a.B,
                     a.win.H, a.win.W, a.Cin, a.win.TY, a.win.TX, a.win_valid_only, tmax);
  return true;
}

// ---- rows, forward, of the MERGED map x = ((x1 + up(x2)) + up(x3)) / 3 (main.py:58,67,69-70) of a bf16 handle, for the model's own geometry
// (W x 2 W2 maps: 90 / 45 / 23 columns): the contract of rows_fwd_merge_kernel<NX, true, true> (conv_fft_rows_fwd.hip), whose generic taps -- eight
// gathers, two tap computations and twelve lerps per element -- make it the one transform pass bound by vector-ALU issue slots (1.5 ms per 256 images at
// 2.2 TB/s).  Here the row lives in the registers of its two threads, so the TF-1.x taps along x are COMPILE-TIME constants (UpTaps: the same float32
// products tf1_tap() forms) and a thread fetches each coarse pixel it needs once: 48 + 2 x 25 + 2 x 14 words instead of 9 per element.  The lerp along y
// is taken first, on the few coarse pixels, then the lerp along x per fine pixel (the other order in the generic kernel and in TF: the two differ in the
// last fp32 bit, four orders of magnitude below the bf16 rounding that follows).  The half row of thread 1 sees other x3 taps than thread 0's: both
// candidates are compile-time registers, one v_cndmask picks.
template <int NX, int W, int W3, int J>
__device__ __forceinline__ void merge_px(unsigned (&raw)[NX / 2], const unsigned (&r1)[NX / 2], const cf (&v2)[MergeGeom<NX, W, W3>::N2], const cf (&v3)[MergeGeom<NX, W, W3>::N3], bool odd) {
  using G = MergeGeom<NX, W, W3>;
  using T3 = typename G::T3;
  constexpr int M = NX / 2;
  constexpr int n1 = M + J < W ? M + J : W - 1;      // thread 1's pixel (clamped behind the map: that word becomes 0 below)
  // 2 W2 = W: source position n / 2 for both threads (M is even), i.e. locals J / 2 and J / 2 + 1 with weight 0 or 1/2
  cf u2 = v2[J >> 1];
  if constexpr (J & 1) {
    constexpr int hi2_1 = M / 2 + (J >> 1) + 1 < W / 2 ? (J >> 1) + 1 : W / 2 - 1 - M / 2;      // thread 1: hi = min(lo + 1, W2 - 1), as a local index
    const cf h2 = hi2_1 == (J >> 1) + 1 ? v2[(J >> 1) + 1] : cf{odd ? v2[hi2_1].x : v2[(J >> 1) + 1].x, odd ? v2[hi2_1].y : v2[(J >> 1) + 1].y};
    u2 = lerp_cf(u2, h2, 0.5f);
  }
  constexpr int lo0 = T3::lo(J) - G::base3(0), hi0 = T3::hi(J) - G::base3(0), lo1 = T3::lo(n1) - G::base3(1), hi1 = T3::hi(n1) - G::base3(1);
  static_assert(lo0 >= 0 && hi0 < G::N3 && lo1 >= 0 && hi1 < G::N3, "x3 taps inside the fetched span");
  const cf a3 = cf{odd ? v3[lo1].x : v3[lo0].x, odd ? v3[lo1].y : v3[lo0].y}, b3 = cf{odd ? v3[hi1].x : v3[hi0].x, odd ? v3[hi1].y : v3[hi0].y};
  const cf u3 = lerp_cf(a3, b3, odd ? T3::t(n1) : T3::t(J));
  const cf a = bf16pair(r1[J]);
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  // (the third as one multiplication by RN(1/3): against the exact quotient it moves the bf16 rounding of one value in 2^15 -- the class of the lerp order)
  constexpr float k3 = 0.333333343267440796f;
  const unsigned w = __builtin_bit_cast(unsigned, bf16x2{static_cast<__bf16>(((a.x + u2.x) + u3.x) * k3), static_cast<__bf16>(((a.y + u2.y) + u3.y) * k3)});
  raw[J] = (M + J < W || !odd) ? w : 0u;
  if constexpr (J % 4 == 3) __builtin_amdgcn_sched_barrier(0);      // a few pixels at a time: interleaving all of them costs more registers than the thread has
  if constexpr (J + 1 < M) merge_px<NX, W, W3, J + 1>(raw, r1, v2, v3, odd);
}
template <int NX, int W, int W3>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void rows_fwd_merge_reg_kernel(const unsigned* __restrict__ x1, const unsigned* __restrict__ x2, int H2,
                                                                                                    const unsigned* __restrict__ x3, int H3, uint2* __restrict__ T, int nrows, int B, int H,
                                                                                                    int C, float sy2, float sy3, float* __restrict__ tmax, float* __restrict__ t16) {
  using G = MergeGeom<NX, W, W3>;
  constexpr int M = NX / 2, W2 = W / 2, N2 = G::N2, N3 = G::N3;
  static_assert(W == 2 * W2 && M % 2 == 0 && M <= W && W <= NX, "the x2 taps above");
  const int CP = C >> 1;
  int h, p;
  size_t by;
  pair_coords<false>(CP, h, p, by, C == 512);
  if (by >= (size_t)nrows) return;
  const int b = (int)(by / H), y = (int)(by % H);
  const bool odd = h != 0;
  const Tap ty2 = tf1_tap(y, H2, sy2), ty3 = tf1_tap(y, H3, sy3);      // the source rows: the same for the whole wave
  unsigned r1[M], r2a[N2], r2b[N2], r3a[N3], r3b[N3];
  {
    // Buffer loads: ONE lane offset per source (channel pair + the half row's first column) and a SCALAR offset per pixel -- no vector address arithmetic
    // and no address registers.  A descriptor covers one image; what a half row reads behind its row (thread 1, j >= W - M; the spare coarse columns) is
    // the next row or, behind the image, the zeros of the range check, and is never used: the taps below are clamped at compile time.
    const int bs = __builtin_amdgcn_readfirstlane(b), ys = __builtin_amdgcn_readfirstlane(y);
    const auto d1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(x1) + (size_t)bs * H * W * CP, 0, H * W * CP * 4, 0x00020000);
    const auto d2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(x2) + (size_t)bs * H2 * W2 * CP, 0, H2 * W2 * CP * 4, 0x00020000);
    const auto d3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(x3) + (size_t)bs * H3 * W3 * CP, 0, H3 * W3 * CP * 4, 0x00020000);
    const int cp4 = CP * 4;
    const int o2 = (p + h * (M / 2) * CP) * 4, o3 = (p + (odd ? G::base3(1) : G::base3(0)) * CP) * 4, o1 = (p + h * M * CP) * 4;
    const int s2a = ty2.lo * W2 * cp4, s2b = ty2.hi * W2 * cp4, s3a = ty3.lo * W3 * cp4, s3b = ty3.hi * W3 * cp4, s1 = ys * W * cp4;
    // the coarse rows first: their conversions and the lerps along y run while the row of x1 is still on its way
#pragma unroll
    for (int i = 0; i < N2; ++i) {
      r2a[i] = __builtin_amdgcn_raw_buffer_load_b32(d2, o2, s2a + i * cp4, 0);
      r2b[i] = __builtin_amdgcn_raw_buffer_load_b32(d2, o2, s2b + i * cp4, 0);
    }
#pragma unroll
    for (int i = 0; i < N3; ++i) {
      r3a[i] = __builtin_amdgcn_raw_buffer_load_b32(d3, o3, s3a + i * cp4, 0);
      r3b[i] = __builtin_amdgcn_raw_buffer_load_b32(d3, o3, s3b + i * cp4, 0);
    }
#pragma unroll
    for (int j = 0; j < M; ++j) r1[j] = __builtin_amdgcn_raw_buffer_load_b32(d1, o1, s1 + j * cp4, 0);
  }
  __builtin_amdgcn_sched_barrier(0);      // every load is out before the first conversion
  cf v2[N2], v3[N3];
#pragma unroll
  for (int i = 0; i < N2; ++i) {
    v2[i] = lerp_cf(bf16pair(r2a[i]), bf16pair(r2b[i]), ty2.t);
    if (i % 4 == 3) __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < N3; ++i) {
    v3[i] = lerp_cf(bf16pair(r3a[i]), bf16pair(r3b[i]), ty3.t);
    if (i % 4 == 3) __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_sched_barrier(0);
  unsigned raw[M];
  merge_px<NX, W, W3, 0>(raw, r1, v2, v3, odd);
  fwd_rows_finish<NX>(raw, T, h, p, b, y, B, H, C, tmax, t16);
}
// true: launched (the model's merge on a bf16 handle with 16-bit T: 90-column maps, x2 at half and x3 at a quarter of the width)
bool cfft_rows_fwd_merge_reg(int NX, const FftArgs& a, const FftMerge& m, FftLayout in_layout, cf* T, float* tmax, hipStream_t st, float* t16) {
  if (NX != 96 || in_layout != kFftBf16Nhwc || !t16 || a.Cin % 64 || a.W != 90 || m.W2 != 45 || m.W3 != 23 || m.H2 < 1 || m.H3 < 1) return false;
  const int nrows = a.B * a.H;
  const size_t threads = a.Cin == 512 ? (size_t)((nrows + 3) / 4) * 8 * 256 : (size_t)nrows * a.Cin;      // (512 channels: eight work groups per four rows)
  hipLaunchKernelGGL((rows_fwd_merge_reg_kernel<96, 90, 23>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, static_cast<const unsigned*>(a.x), static_cast<const unsigned*>(m.x2), m.H2,
                     static_cast<const unsigned*>(m.x3), m.H3, reinterpret_cast<uint2*>(T), nrows, a.B, a.H, a.Cin, (float)m.H2 / (float)a.H, (float)m.H3 / (float)a.H, tmax, t16);
  return true;
}

}  // namespace cfft
}  // namespace jcm
