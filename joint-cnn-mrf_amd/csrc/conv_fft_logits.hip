// The logits layer (9x9, Cin -> Cout <= 16, the last layer) of an fp32 handle on the ROW spectra of its input (option "fft_logits_rows").
//
// As a full frequency-domain layer conv6 is 1 % of the model's FLOPs behind two column passes and a channel GEMM whose 9 columns are padded to 32:
// 3 GB of the step's traffic.  The column transform only turns the 9 vertical taps into one product per frequency; with 9 output channels that
// trade goes the wrong way.  Here the channels are contracted directly on the row-transformed tensor T the previous layer's fused row kernel
// hands over -- per kx one real matrix product with K = 9 dy x Cin x (re, im):
//
//   S[kx][b][y][j] = sum_dy sum_ci T[kx][b][y + dy - 4][ci] * A[kx][dy][ci][j],   A[kx][dy][ci][j] = sum_b w[dy][8 - b][ci][j] e^{-2 pi i kx b / NX}
//
// (rows outside 0 .. H-1 are zeros: the SAME padding along y is explicit, nothing wraps; along x the circular transform of NX >= W + 4 points
// is alias-free as on the whole route.)  The inverse row pass of the whole route (rows_inv_kernel, bias epilogue) then finishes the layer from
// S, stored in its input layout T'[b][y][kx][64].
//
// logits_rows_kernel: one work group per (kx, image), 8 waves.  A wave owns every 8th 16-channel chunk of T -- a contiguous 60 x 16 complex
// block in T[kx][c/16][b][y][16] -- and all 64 output rows: it splits the chunk into two fp16 parts under the image's power-of-two scale
// (max|T_b| itself bounds a component: no column transform follows), keeps it in ITS OWN slice of LDS as rows of [part][re 16 | im 16] fp16 with
// four zero rows above and eight below, and takes the nine dy as nine row-shifted fragment reads.  One v_mfma_f32_16x16x32_f16 consumes the
// 16 channels' real and imaginary parts at once: [Tr | Ti] x [Ar ; -Ai] is the real part of the complex product, [Tr | Ti] x [Ai ; Ar] the
// imaginary part, so the operand A is stored as those two stacked forms (the sign is in the operand), in the exact register image of the B
// fragment: a wave's load is one contiguous 1-KB run, straight from L2 into registers, and no element of A is loaded twice by a work group.
// Three products per term (x0 a1 + x1 a0 + x0 a0), fp32 accumulation.  The waves never meet before the end (no work-group barrier in the loop);
// their partial sums are added through LDS in a fixed order, so an image's result depends on nothing but the image.
// Work groups of one kx run on one XCD (block index mod 8 = XCD) so that A[kx] is fetched from that XCD's L2.
#include "conv_fft_common.h"

namespace jcm {
namespace cfft {

constexpr int kLrWaves = 8, kLrRows = 72, kLrUnits = 8;      // LDS slice of a wave: 72 rows (4 zero + 64 + 4 zero) of eight 16-byte units
constexpr int kLrLds = kLrWaves * kLrRows * kLrUnits * 16;   // 73 728 bytes: two work groups per CU
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// unit u (0..3: part 0 [re 0-7 | re 8-15 | im 0-7 | im 8-15], 4..7: part 1) of LDS row r.  The 16 lanes that read one unit of 16 consecutive rows hit
// 16 different 16-byte columns of the 256-byte bank window: the row's parity picks the half, (r >> 1) & 7 permutes the units inside it.
__device__ __forceinline__ int lr_slot(int r, int u) { return r * kLrUnits + (u ^ ((r >> 1) & 7)); }

// ---- the operand: Aop[kx][dy][c/16][form: re p0, re p1, im p0, im p1][lane] of 16 bytes = the B fragment of lane l: column j = l & 15, k = 8 (l >> 4) + e;
// k < 16: channel 16 c + k, real form Ar, imaginary form Ai; k >= 16: channel 16 c + k - 16, real form -Ai, imaginary form Ar.  Columns >= Cout are zero.
// Two fp16 parts of A * 2^k, k from wscale[0] >= max sum |taps| (weight_bound_kernel); wscale[1] = 2^-k for the inverse row pass.
__global__ __launch_bounds__(256) void logits_rows_operand_kernel(const float* __restrict__ w, uint4* __restrict__ Aop, int Cin, int Cout, int NX, float* __restrict__ wscale) {
  __shared__ cf twx[9];
  const int kx = blockIdx.y, KC = Cin >> 4;
  if (threadIdx.x < 9) {
    double sn, cs;
    sincospi(-2.0 * (double)((kx * (int)threadIdx.x) % NX) / (double)NX, &sn, &cs);
    twx[threadIdx.x] = cf{(float)cs, (float)sn};
  }
  __syncthreads();
  int ex = 0;
  const float bound = wscale[0];
  if (bound > 0.f && bound < 3.0e38f) (void)frexpf(bound, &ex);      // bound < 2^ex
  const float wmul = ldexpf(1.f, 14 - ex);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) wscale[1] = ldexpf(1.f, ex - 14);
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 9 * KC * 64) return;
  const int lane = e & 63, c = (e >> 6) % KC, dy = (e >> 6) / KC;
  const int j = lane & 15, g = lane >> 4, ch0 = c * 16 + (g & 1) * 8;
  cf a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = cf{0.f, 0.f};
  if (j < Cout) {
#pragma unroll
    for (int b = 0; b < 9; ++b) {
      const float* tap = w + ((size_t)(dy * 9 + (8 - b)) * Cin + ch0) * Cout + j;      // the flipped kernel row: TF's conv2d is a correlation
      const cf tw = twx[b];
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = sfma(tap[(size_t)i * Cout], tw, a[i]);
    }
  }
  float vr[8], vi[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    vr[i] = g < 2 ? a[i].x : -a[i].y;
    vi[i] = g < 2 ? a[i].y : a[i].x;
  }
  uint4 u[2];
  uint4* dst = Aop + ((((size_t)kx * 9 + dy) * KC + c) * 4) * 64 + lane;
  split8h(vr, wmul, u);
  dst[0] = u[0]; dst[64] = u[1];
  split8h(vi, wmul, u);
  dst[128] = u[0]; dst[192] = u[1];
}

// ---- the contraction.  T: float4 = two channels (re, im, re, im); S: T'[b][y][kx][64] complex fp32 (columns 16 .. 63 written as zeros: the inverse row pass
// transforms whole 64-channel blocks).  per = items of an XCD: block (x = id & 7, i = id >> 3) takes item x per + i of the (kx, image) list.
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void logits_rows_kernel(const float4* __restrict__ T, const uint4* __restrict__ Aop,
                                                                                                       const float* __restrict__ tmax, cf* __restrict__ S, int B, int H, int KC,
                                                                                                       int NXH, int per) {
  extern __shared__ __attribute__((aligned(16))) char lr_smem[];
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, item = xcd * per + slot;
  if (slot >= per || item >= NXH * B) return;      // (the whole work group)
  const int kx = item / B, b = item - kx * B;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  uint4* wl = reinterpret_cast<uint4*>(lr_smem) + wave * (kLrRows * kLrUnits);
  for (int i = lane; i < kLrRows * kLrUnits; i += 64) wl[i] = make_uint4(0u, 0u, 0u, 0u);      // the zero rows stay zero: only rows 4 .. H + 3 are written below
  const float scale = fp16_scale(tmax[b], 1.f);
  f32x4 sr[4], si[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) { sr[m] = f32x4{0.f, 0.f, 0.f, 0.f}; si[m] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  // a lane converts (row y, channel half hh) of the chunk: 64 contiguous bytes of T -> the four units (re | im) x (part 0 | 1) of that half
  const int y0 = lane >> 1, y1 = 32 + (lane >> 1), hh = lane & 1;
  const bool in0 = y0 < H, in1 = y1 < H;
  float4 pre[2][4];
  auto fetch = [&](int c) __attribute__((always_inline)) {
    const float4* src = T + (((size_t)kx * KC + c) * B + b) * H * 8 + hh * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pre[0][q] = in0 ? src[(size_t)y0 * 8 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
      pre[1][q] = in1 ? src[(size_t)y1 * 8 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&](int i, int y) __attribute__((always_inline)) {
    float re[8], im[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) { re[2 * q] = pre[i][q].x; im[2 * q] = pre[i][q].y; re[2 * q + 1] = pre[i][q].z; im[2 * q + 1] = pre[i][q].w; }
    uint4 ur[2], ui[2];
    split8h(re, scale, ur);
    split8h(im, scale, ui);
    const int r = y + 4;
    wl[lr_slot(r, hh)] = ur[0]; wl[lr_slot(r, 2 + hh)] = ui[0];
    wl[lr_slot(r, 4 + hh)] = ur[1]; wl[lr_slot(r, 6 + hh)] = ui[1];
  };
  const int g = lane >> 4, rl = lane & 15;
  if (wave < KC) fetch(wave);
  for (int c = wave; c < KC; c += kLrWaves) {
    if (in0) stash(0, y0);
    if (in1) stash(1, y1);
    if (c + kLrWaves < KC) fetch(c + kLrWaves);
    // the slice is this wave's own: what its lanes wrote is visible to its lanes behind a wave-level fence, no work-group barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint4* bp = Aop + (((size_t)kx * 9 * KC + c) * 4) * 64 + lane;
#pragma unroll 3
    for (int dy = 0; dy < 9; ++dy) {
      const uint4* bq = bp + (size_t)dy * KC * 256;
      const f16x8 br0 = __builtin_bit_cast(f16x8, bq[0]), br1 = __builtin_bit_cast(f16x8, bq[64]);
      const f16x8 bi0 = __builtin_bit_cast(f16x8, bq[128]), bi1 = __builtin_bit_cast(f16x8, bq[192]);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int r = m * 16 + rl + dy;      // LDS row of T row y + dy - 4, y = 16 m + rl
        const f16x8 a0 = __builtin_bit_cast(f16x8, wl[lr_slot(r, g)]), a1 = __builtin_bit_cast(f16x8, wl[lr_slot(r, 4 + g)]);
        sr[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, br1, sr[m], 0, 0, 0);
        si[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bi1, si[m], 0, 0, 0);
        sr[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, br0, sr[m], 0, 0, 0);
        si[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bi0, si[m], 0, 0, 0);
        sr[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, br0, sr[m], 0, 0, 0);
        si[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bi0, si[m], 0, 0, 0);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // every lane has read the chunk before any lane overwrites it
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // the eight partial sums, added in wave order: red[wave][register 0..31 = (re | im, m, i)][lane]
  __syncthreads();
  float* red = reinterpret_cast<float*>(lr_smem);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[(wave * 32 + m * 4 + i) * 64 + lane] = sr[m][i];
      red[(wave * 32 + 16 + m * 4 + i) * 64 + lane] = si[m][i];
    }
  __syncthreads();
  cf* Sb = S + ((size_t)b * H * NXH + kx) * 64;      // row y: + y NXH 64
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int pi = tid + 512 * q, lo = pi & 63, mi = pi >> 6;      // mi = 4 m + i: row 16 m + 4 (lane >> 4) + i, column lane & 15 of the accumulator tile
    float re = 0.f, im = 0.f;
#pragma unroll
    for (int wv = 0; wv < kLrWaves; ++wv) {
      re += red[(wv * 32 + mi) * 64 + lo];
      im += red[(wv * 32 + 16 + mi) * 64 + lo];
    }
    const int row = (mi >> 2) * 16 + (lo >> 4) * 4 + (mi & 3);
    if (row < H) Sb[(size_t)row * NXH * 64 + (lo & 15)] = cf{re, im};
  }
  for (int e = tid; e < H * 24; e += 512) {
    const int row = e / 24, q = e - row * 24;
    *reinterpret_cast<float4*>(Sb + (size_t)row * NXH * 64 + 16 + 2 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

bool cfft_logits_rows_supported(int NX, const FftArgs& a) { return NX == 96 && a.H >= 1 && a.H <= 64 && a.Cin % 16 == 0 && a.Cout >= 1 && a.Cout <= 16 && a.B >= 1; }
size_t cfft_logits_rows_operand_bytes(int NX, int Cin) { return (size_t)(NX / 2 + 1) * 9 * (Cin / 16) * 4 * 64 * sizeof(uint4); }
bool cfft_logits_rows_pack(int NX, const float* w_hwio, void* aop, int Cin, int Cout, float* wscale, hipStream_t st) {
  const dim3 grid((unsigned)((9 * (Cin / 16) * 64 + 255) / 256), (unsigned)(NX / 2 + 1));
  hipLaunchKernelGGL(logits_rows_operand_kernel, grid, dim3(256), 0, st, w_hwio, static_cast<uint4*>(aop), Cin, Cout, NX, wscale);
  return true;
}
bool cfft_logits_rows(int NX, const FftArgs& a, const cf* T, const void* aop, const float* tmax, cf* S, hipStream_t st) {
  if (!cfft_logits_rows_supported(NX, a)) return false;
  static LdsAttr attr;
  if (attr.ensure(reinterpret_cast<const void*>(logits_rows_kernel), kLrLds) != hipSuccess) return false;
  const int NXH = NX / 2 + 1, items = NXH * a.B, per = (items + 7) / 8;
  hipLaunchKernelGGL(logits_rows_kernel, dim3((unsigned)(per * 8)), dim3(512), kLrLds, st, reinterpret_cast<const float4*>(T), static_cast<const uint4*>(aop), tmax, S, a.B, a.H,
                     a.Cin / 16, NXH, per);
  return true;
}

}  // namespace cfft
}  // namespace jcm
