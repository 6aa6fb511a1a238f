// Stride-1 SAME convolution (9x9, 5x5) in the FREQUENCY domain: every such layer of an fp32 handle, the wide 9x9 layers (conv4_*, conv5:
// 256/512 -> 512 channels) of a bf16 handle.
//
// A 9x9 layer with 512 x 512 channels is 229 GFLOP per image as a direct convolution.  With the maps transformed once the layer is, for
// every frequency, one complex matrix product over the channels:  Y[f][b][co] = sum_ci X[f][b][ci] * Wf[f][ci][co].  The transform is a
// CIRCULAR convolution of size NY x NX >= (H + pad) x (W + pad), pad = (k-1)/2: the SAME output y in [0, H) reads inputs y-pad .. y+pad,
// so the wrap-around only has to land in the zero rows H .. NY-1 -- which H + pad rows guarantee (a full linear convolution would need
// H + k - 1).  60x90 maps: 64 x 96 transforms, 64 * 49 = 3136 frequencies, 8*Cin*Cout*3136 = 6.6 GFLOP per image for conv5, 35x fewer
// than the direct form.  In fp32 the route is MORE accurate than the fp32 MFMA accumulation chain it replaces.
//
//   rows_fwd        (image, row, 64 channels)        : NHWC fp32 / bf16 (or planar bf16); two adjacent channels = one complex number
//                                                      z = x_c + i x_{c+1}; complex FFT along x in LDS; X_c, X_{c+1} through the Hermitian
//                                                      symmetry -> T[kx][c/16][b][y][16]   (a column work group's input is contiguous)
//   cols_fwd_split  (8 images, kx, 16 channels)      : FFT along y, then the spectra are SPLIT into bf16 parts and written in the exact
//                                                      LDS image of the channel GEMM: Xs[f][m-tile][c/16][re|im][part][k-half][row][8]
//   cgemm_split     (cgemm_split.hip)                : the channel GEMM on the bf16 matrix cores, one complex product per frequency
//   cols_inv        (image, kx, 64 channels)         : inverse along ky, rows pad .. pad+H-1 kept -> T[b][y][kx][co]
//   rows_inv        (image, row, 64 channels)        : Z = Y_c + i Y_{c+1} (Hermitian extension), inverse complex FFT along kx, columns
//                                                      pad .. pad+W-1, 1/(NY NX), bias, ReLU, folded BatchNorm -> NHWC fp32 / bf16 / planar
// Every transform pass is an LDS kernel for any size with a Plan (conv_fft_rows_fwd.hip, conv_fft_cols.hip, conv_fft_rows_inv.hip; the fused
// hand-overs between two layers: conv_fft_rows_fused.hip) and, at the model's sizes, a kernel with the transform in registers, taken where it
// exists (fft_reg_rows.h: conv_fft_reg_fwd.hip, conv_fft_reg_inv.hip -- rows and columns --, conv_fft_reg_fused.hip, conv_fft_reg_tiles.hip).
// The filter spectra (flipped kernel: TF's conv2d is a correlation) are computed once per (layer, map size) at first use, split into the
// same bf16 parts, in the GEMM's tile-major layout.  FFTs: the in-LDS decimation-in-frequency stages of sm_fused.hip, channel-vectorised
// (consecutive lanes = consecutive channels).  Twiddles come from one table per device, built on the host in double precision.
// This file: the filter-spectra kernels and their packers; then the host side -- sizes (kLens, sizes_of), the hand-over predicates, the FftPlan of a layer call
// (conv_fft_plan.h: sizes, views, workspace regions, twiddles), the refusals that say which variant a call can take, the five pass functions that each choose
// their kernel, and the runners (conv_fft_f32 with its tiled form, conv_fft_logits_f32, conv_fft_spectra), which are sequences of those passes.
// Reference semantics: conv2d SAME stride 1 + bias + ReLU + BatchNorm (main.py:133-135,156-169).
#include <cmath>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "conv_fft_common.h"
#include "conv_fft_plan.h"

namespace jcm {
namespace cfft {

// ---- filter spectra, split: HWIO fp32 [k][k][Cin][Cout] -> Wf[f][ci][co] = sum_{a,b} w[k-1-a][k-1-b][ci][co] e^{-2 pi i (ky a / NY + kx b / NX)}
// (the flipped kernel: TF's conv2d is a correlation; output channels Cout .. CoutP-1 are zero), written as the channel GEMM's operand
// image Ws[f][co/ntl][ci/16][re|im][part][k-half][ntl columns][8 x 16 bit] (cgemm_split.hip).
// A thread owns the 8 consecutive input channels of one 16-byte unit of one output channel and one kx:
// the k row sums of its filters stay in registers, then for one ky after the other the k-term column sum gives their spectra,
// which are split and stored straight from registers -- consecutive threads are consecutive output channels, so a wave's store instruction is
// one contiguous 1-KB run.  No exchange through LDS, no barrier in the loop (round 3: the packer runs once per weight update in the training
// step, where it is 20 % of the step).
// NP = 4: two FP16 parts of the spectrum times 2^k, k from wscale[0] = max over filters of sum |taps| >= |W[f]| (weight_bound_kernel); layout as
// NP = 2; wscale[1] = 2^-k for the inverse row pass.
template <int KS, int NP>
__global__ __launch_bounds__(256) void weight_spectra_split_kernel(const float* __restrict__ w, uint4* __restrict__ Ws, int Cin, int Cout, int CoutP, int ntl, int NY, int NX,
                                                                   int round_bf16, float* __restrict__ wscale) {
  __shared__ cf twy[192][KS - 1], twx[KS];      // e^{-2 pi i ky a / NY} (a = 1..KS-1), e^{-2 pi i kx b / NX} of this block's kx
  const int tid = threadIdx.x;
  const int kx = blockIdx.y;
#pragma unroll 1
  for (int k = tid; k < NY * (KS - 1) + KS; k += 256) {
    const bool isy = k < NY * (KS - 1);
    const int ky = k / (KS - 1), a = isy ? k % (KS - 1) + 1 : k - NY * (KS - 1);
    const int num = isy ? (ky * a) % NY : (kx * a) % NX, den = isy ? NY : NX;
    double sn, cs;
    sincospi(-2.0 * (double)num / (double)den, &sn, &cs);
    cf* dstw = isy ? &twy[ky][a - 1] : &twx[a];
    *dstw = cf{(float)cs, (float)sn};
  }
  __syncthreads();
  constexpr int CPT = 8;                                      // input channels per thread = one 16-byte unit of the layout
  constexpr int NPP = NP == 5 ? 1 : 2;                        // 16-byte units this thread writes per plane (NP = 2: bf16 parts, 4: fp16 parts, 5: one fp16 part)
  static_assert(NP == 2 || NP == 4 || NP == 5, "operand forms of the channel GEMM");
  float wmul = 1.f;
  if constexpr (NP >= 4) {
    int ex = 0;
    const float bound = wscale[0];
    if (bound > 0.f && bound < 3.0e38f) (void)frexpf(bound, &ex);      // bound < 2^ex
    wmul = ldexpf(1.f, 14 - ex);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) wscale[1] = ldexpf(1.f, ex - 14);
  }
  const size_t e = (size_t)blockIdx.x * 256 + tid;
  if (e >= (size_t)(Cin / CPT) * CoutP) return;
  const int co = (int)(e % CoutP), cig = (int)(e / CoutP);
  cf ra[CPT][KS];                                             // row sums of the flipped kernels of input channels CPT cig .. +CPT-1
  const unsigned toff = (unsigned)(cig * CPT * Cout + (co < Cout ? co : Cout - 1));
#pragma unroll
  for (int c = 0; c < CPT; ++c)
#pragma unroll
    for (int a = 0; a < KS; ++a) ra[c][a] = cf{0.f, 0.f};
#pragma unroll 1
  for (int a = 0; a < KS; ++a) {               // a real loop (k x CPT loads in flight, not k x k x CPT and their addresses) ...
    cf sum[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) sum[c] = cf{0.f, 0.f};
#pragma unroll
    for (int b = 0; b < KS; ++b) {
      // uniform tap base + 32-bit lane offset (always in bounds: no branch per load); tap-major so that one address serves the CPT channels
      const float* tap = w + (size_t)((KS - 1 - a) * KS + (KS - 1 - b)) * Cin * Cout;
      const cf tw = twx[b];
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        float wv = tap[toff + (unsigned)(c * Cout)];
        wv = co < Cout ? wv : 0.f;
        if (round_bf16) wv = static_cast<float>(static_cast<__bf16>(wv));       // bf16 handles: the filter the bf16 MFMA kernels multiply with
        sum[c] = sfma(wv, tw, sum[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < CPT; ++c)
#pragma unroll
      for (int aa = 0; aa < KS; ++aa) ra[c][aa] = aa == a ? sum[c] : ra[c][aa];      // ... with the register array written by selects, not by index
  }
  const int KC = Cin / 16, ntiles = CoutP / ntl;
  const int ci0 = cig * CPT, kc = ci0 >> 4, kg = (ci0 >> 3) & 1, nt = co / ntl, sn = co % ntl;
  // 16-byte units: stride between frequencies, and this thread's units inside one frequency
  // NP = 5: stages of 32 channels, the two planes of the NP = 2 layout = the stage's two 16-channel halves: unit ((c * 2 + half) * 2 + kg) * ntl + column
  const size_t fstride = NP == 5 ? (size_t)ntiles * (KC >> 1) * 8 * ntl : (size_t)ntiles * KC * (4 * NPP) * ntl;
  uint4* dst = Ws + (size_t)kx * NY * fstride +
               (NP == 5 ? ((size_t)nt * (KC >> 1) + (kc >> 1)) * 8 * ntl + ((size_t)(kc & 1) * 2 + kg) * ntl + sn :
                          ((size_t)nt * KC + kc) * (4 * NPP) * ntl + (size_t)kg * ntl + sn);
  // the spectrum of one ky -> this thread's units (split into the operand parts of the layout); streaming stores: nothing on this GPU reads them back soon
  typedef unsigned u32x4n __attribute__((ext_vector_type(4)));
  auto put = [](uint4* q, const uint4& v) __attribute__((always_inline)) { __builtin_nontemporal_store(u32x4n{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4n*>(q)); };
  auto emit = [&](uint4* d, const float (&xr)[CPT], const float (&xi)[CPT]) __attribute__((always_inline)) {
    if constexpr (NP == 5) {
      float x8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) x8[c] = xr[c % CPT];
      put(d, round8h(x8, wmul));
#pragma unroll
      for (int c = 0; c < 8; ++c) x8[c] = xi[c % CPT];
      put(d + (size_t)4 * ntl, round8h(x8, wmul));
    } else {
      // [re|im][part][k-half][ntl][8 bf16]
      uint4 u[NPP];
      float x8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) x8[c] = xr[c % CPT];
      if constexpr (NP == 4) split8h(x8, wmul, u);
      else split8<NPP>(x8, u);
#pragma unroll
      for (int p = 0; p < NPP; ++p) put(d + (size_t)p * 2 * ntl, u[p]);
#pragma unroll
      for (int c = 0; c < 8; ++c) x8[c] = xi[c % CPT];
      if constexpr (NP == 4) split8h(x8, wmul, u);
      else split8<NPP>(x8, u);
#pragma unroll
      for (int p = 0; p < NPP; ++p) put(d + (size_t)(NPP + p) * 2 * ntl, u[p]);
    }
  };
  // W[ky] = sum_a R_a e^{-i th_a}, th_a = 2 pi ky a / NY, and its partner W[NY - ky] = sum_a R_a e^{+i th_a} share C = sum_a R_a cos th_a and
  // S = sum_a R_a sin th_a (real weights on the complex row sums: two FMAs per term and sum instead of four):  W[ky] = C - i S,  W[NY - ky] = C + i S.
  // ky = 0 and (NY even) ky = NY / 2 stand alone.  (5x5 layers: 154 -> 95 us per launch; the 9x9 packer is bound by its 3.1 TB/s of writes either way.)
  for (int ky = 0; ky <= NY / 2; ++ky) {
    const int kp = ky == 0 ? 0 : NY - ky;      // partner (== ky for 0 and NY / 2)
    float cs[KS - 1], sn_[KS - 1];
#pragma unroll
    for (int a = 1; a < KS; ++a) { const cf t = twy[ky][a - 1]; cs[a - 1] = t.x; sn_[a - 1] = -t.y; }      // twy = (cos th, -sin th)
    float xr[CPT], xi[CPT], pr[CPT], pi_[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      cf C = ra[c][0], S = cf{0.f, 0.f};
#pragma unroll
      for (int a = 1; a < KS; ++a) { C = sfma(cs[a - 1], ra[c][a], C); S = sfma(sn_[a - 1], ra[c][a], S); }
      xr[c] = C.x + S.y; xi[c] = C.y - S.x;      // C - i S
      pr[c] = C.x - S.y; pi_[c] = C.y + S.x;     // C + i S
    }
    emit(dst + (size_t)ky * fstride, xr, xi);
    if (kp != ky) emit(dst + (size_t)kp * fstride, pr, pi_);
  }
}

// max over (ci, co) of sum_taps |w|: a bound of |W[f][ci][co]| for every frequency (np = 4)
template <int TAPS>
__global__ __launch_bounds__(256) void weight_bound_kernel(const float* __restrict__ w, size_t pairs, int round_bf16, float* __restrict__ wmax) {
  __shared__ float red[4];
  float m = 0.f;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < pairs; e += (size_t)gridDim.x * 256) {
    // every tap's load goes out before the first add (the taps are a compile-time count: round 6 -- with a run-time count the loads went out one by one behind the sum)
    float v[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t) v[t] = w[(size_t)t * pairs + e];
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      float x = v[t];
      if (round_bf16) x = static_cast<float>(static_cast<__bf16>(x));
      sum += fabsf(x);
    }
    m = fmaxf(m, sum);
  }
  block_max_to<256>(m * 1.0001f, wmax, red, threadIdx.x);      // (a hair of slack for the rounding of this sum)
}

struct Sizes { int NY, NX; };
// transform lengths with a radix plan (all even: the row pass packs two real rows into one complex transform and needs a Nyquist bin)
static const int kLens[] = {20, 24, 28, 32, 36, 40, 50, 60, 64, 72, 96, 100, 128, 192};
static bool pick(int need, int* n) {
  for (int v : kLens)
    if (v >= need) { *n = v; return true; }
  return false;
}
static int tw_offset(int n) {
  int off = 0;
  for (int v : kLens) {
    if (v == n) return off;
    off += v;
  }
  return -1;
}
// circular convolution of size >= (H + pad) x (W + pad); one size per map for every kernel size (pad of the 9x9 layers), so that two
// consecutive layers can hand the row-transformed tensor over.  The old limit H + k - 1 <= 192 is kept.
// circ (FftArgs::circ): overlap-save windows -- the H x W input IS the transform (H, W must be transform lengths, at least one valid row / column)
static bool sizes_of(int H, int W, int ks, Sizes* s, int circ = 0) {
  if (circ) {
    s->NY = H; s->NX = W;
    return (ks == 9 || ks == 5) && H > 8 && W > 8 && tw_offset(H) >= 0 && tw_offset(W) >= 0;
  }
  return (ks == 9 || ks == 5) && H + ks - 1 <= 192 && W + ks - 1 <= 192 && pick(H + 4, &s->NY) && pick(W + 4, &s->NX);
}
static int pad64(int c) { return (c + CB - 1) / CB * CB; }
static int padn(int c, int n) { return (c + n - 1) / n * n; }

int persistent_grid(const void* kernel, int ntiles, int threads, int dyn_lds) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> cache;      // (kernel, device) -> resident work groups
  int dev = 0;
  (void)hipGetDevice(&dev);
  int resident = 0;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find({kernel, dev});
    if (it != cache.end()) resident = it->second;
  }
  if (!resident) {
    int ncu = 256, per_cu = 0;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, (size_t)dyn_lds) != hipSuccess || per_cu < 1) per_cu = 1;
    resident = ncu * per_cu;
    std::lock_guard<std::mutex> lk(mu);
    cache[{kernel, dev}] = resident;
  }
  return resident < ntiles ? resident : ntiles;
}

// e^{+2 pi i k / n} for every supported length, one table per device (built on the host in double precision, uploaded at first use)
static const cf* twiddle_table(int dev) {
  static std::mutex mu;
  static std::map<int, cf*> tabs;
  std::lock_guard<std::mutex> lk(mu);
  auto it = tabs.find(dev);
  if (it != tabs.end()) return it->second;
  std::vector<float> h;
  for (int n : kLens)
    for (int k = 0; k < n; ++k) {
      const double ang = 2.0 * 3.14159265358979323846 * (double)k / (double)n;
      h.push_back((float)std::cos(ang));
      h.push_back((float)std::sin(ang));
    }
  cf* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d), h.size() * sizeof(float)) != hipSuccess) return nullptr;
  if (hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
  tabs[dev] = d;
  return d;
}

}  // namespace cfft

using namespace cfft;

// ---- sizes, filter spectra, hand-over predicates ----
bool conv_fft_supported(const ConvArgs& a, int ks, int circ) {
  Sizes s;
  return a.Cin % CB == 0 && a.Cin >= CB && a.Cout >= 1 && a.B >= 1 && sizes_of(a.H, a.W, ks, &s, circ);
}
// np: operand form of the channel GEMM (FftOperand; cgemm_split.hip): 4 = fp32 handles, 5 / 2 = bf16 handles
static bool operand_form(int np) { return np == kFftBf16x2 || np == kFftFp16x2 || np == kFftFp16x1; }
size_t conv_fft_weight_bytes(int H, int W, int ks, int Cin, int Cout, int np, int circ) {
  Sizes s;
  if (!sizes_of(H, W, ks, &s, circ)) return 0;
  return cgemm_split_w_bytes(np, s.NY * (s.NX / 2 + 1), Cin, Cout);
}
hipError_t conv_fft_pack_weights(const float* w_hwio, void* wf, int H, int W, int ks, int Cin, int Cout, int np, bool round_bf16, hipStream_t st, float* wscale, int circ,
                                 const float* bound_from) {
  Sizes s;
  if (!sizes_of(H, W, ks, &s, circ) || Cin % 16 || !operand_form(np) || (np >= 4 && !wscale) || (np == kFftFp16x1 && Cin % 32)) return hipErrorInvalidValue;
  const int ntl = cgemm_split_ntile(np, Cout), CoutP = padn(Cout, ntl);
  const size_t cpt = 8;      // thread = (8 input channels: one 16-byte unit, output channel); one kx per block
  const dim3 grid((unsigned)(((size_t)Cin / cpt * CoutP + 255) / 256), (unsigned)(s.NX / 2 + 1));
  uint4* dst = static_cast<uint4*>(wf);
  const int rb = round_bf16 ? 1 : 0;
  if (np >= 4 && bound_from) {
    // the bound max sum |taps| of this filter is known: the flipped, transposed filter of a data gradient has the forward filter's
    if (hipError_t e = hipMemcpyAsync(wscale, bound_from, sizeof(float), hipMemcpyDeviceToDevice, st); e != hipSuccess) return e;
  } else if (np >= 4) {
    if (hipError_t e = hipMemsetAsync(wscale, 0, 2 * sizeof(float), st); e != hipSuccess) return e;
    const size_t pairs = (size_t)Cin * Cout;
    const dim3 bgrid((unsigned)((pairs + 255) / 256 > 1024 ? 1024 : (pairs + 255) / 256));
    if (ks == 9) hipLaunchKernelGGL(weight_bound_kernel<81>, bgrid, dim3(256), 0, st, w_hwio, pairs, rb, wscale);
    else hipLaunchKernelGGL(weight_bound_kernel<25>, bgrid, dim3(256), 0, st, w_hwio, pairs, rb, wscale);
  }
#define WS_LAUNCH(KS, NPV) hipLaunchKernelGGL((weight_spectra_split_kernel<KS, NPV>), grid, dim3(256), 0, st, w_hwio, dst, Cin, Cout, CoutP, ntl, s.NY, s.NX, rb, wscale)
  if (ks == 9) {
    if (np == 2) WS_LAUNCH(9, 2); else if (np == 4) WS_LAUNCH(9, 4); else WS_LAUNCH(9, 5);
  } else {
    if (np == 2) WS_LAUNCH(5, 2); else if (np == 4) WS_LAUNCH(5, 4); else WS_LAUNCH(5, 5);
  }
#undef WS_LAUNCH
  return hipGetLastError();
}
// Can layer L (a, ks) hand its output to layer L+1 (kernel size ks_next, same map) in row-transformed form?  Same NX for both kernel
// sizes (always: the size depends on the map only), unpadded channel count, two row buffers in LDS.
bool conv_fft_fusable(const ConvArgs& a, int ks, int ks_next) {
  Sizes s, n;
  return sizes_of(a.H, a.W, ks, &s) && sizes_of(a.H, a.W, ks_next, &n) && s.NX == n.NX && a.Cout % CB == 0;
}
static size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
FftHandover16 conv_fft_handover16(int B, int NXH, int H, int C) {
  FftHandover16 h;
  h.words_off = align256((size_t)B * NXH * H * C * 4);
  h.bytes = h.words_off + (size_t)B * H * (C / CB) * sizeof(float);
  return h;
}
// T[kx][c/16][b][y][16] of the next layer, complex fp32.  h16: the 16-bit form (conv_fft_handover16) lives in a buffer of the same size -- 4 instead of 8 bytes per
// complex number leave 4 B NXH H C bytes for at most 255 bytes of alignment and B H C / 16 bytes of scale words, and NXH >= 11, C >= 64: the maximum below is the
// fp32 size for every shape the route takes, and says so in code.
size_t conv_fft_handover_bytes(const ConvArgs& a, int ks, bool h16) {
  Sizes s;
  if (!sizes_of(a.H, a.W, ks, &s)) return 0;
  const int NXH = s.NX / 2 + 1;
  const size_t f32 = (size_t)a.B * NXH * a.H * a.Cout * sizeof(cf);
  const size_t b16 = h16 ? conv_fft_handover16(a.B, NXH, a.H, a.Cout).bytes : 0;
  return f32 > b16 ? f32 : b16;
}
bool conv_fft_win_gather_supported(int win, int Cin, bool fft_reg) { return fft_reg && cfft_rows_fwd_win_reg_supported(win, Cin); }
bool conv_fft_win_scatter_supported(int win, int Cout, bool fft_reg) { return fft_reg && win == 32 && Cout % 64 == 0; }      // rows_inv_reg_kernel<32, 0, false>
// the fused hand-overs across a max pool / the branch merge (FftNext, conv_fft_rows_fused.hip)
bool conv_fft_pool_fusable(const ConvArgs& a, int ks, int ks_next) {
  Sizes s, n;
  return sizes_of(a.H, a.W, ks, &s) && sizes_of((a.H + 1) / 2, (a.W + 1) / 2, ks_next, &n) && cfft_rows_inv_pool_fwd_supported(s.NX, n.NX, a.Cout);
}
size_t conv_fft_pool_handover_bytes(const ConvArgs& a, int ks_next) {      // T[kx][c/16][b][y][16] of the next layer, on the pooled map
  Sizes n;
  if (!sizes_of((a.H + 1) / 2, (a.W + 1) / 2, ks_next, &n)) return 0;
  return (size_t)a.B * (n.NX / 2 + 1) * ((a.H + 1) / 2) * a.Cout * sizeof(cf);
}
// h16: bf16 handles on the one-part route with 16-bit row-transformed tensors -- the register kernel only (the model's geometry)
bool conv_fft_merge_fusable(const ConvArgs& a, int ks, int ks_next, const FftMerge& m, bool fft_reg, bool h16) {
  Sizes s;
  if (!conv_fft_fusable(a, ks, ks_next) || !sizes_of(a.H, a.W, ks, &s)) return false;
  const bool reg = fft_reg && cfft_rows_inv_merge_fwd_reg_supported(s.NX, a, m, (ks - 1) / 2);
  return h16 ? reg : (reg || cfft_rows_inv_merge_fwd_supported(s.NX, a, m));
}
// geometry of the spectra for the weight-gradient kernels
bool conv_fft_geometry(int H, int W, int ks, int B, int Cout, int np, int* NY, int* NX, int* MT, int circ) {
  Sizes s;
  if (!sizes_of(H, W, ks, &s, circ)) return false;
  *NY = s.NY; *NX = s.NX; *MT = cgemm_split_mtile(np, B, Cout);
  return true;
}
size_t conv_fft_logits_weight_bytes(int H, int W, int Cin) {
  Sizes s;
  return sizes_of(H, W, 9, &s) ? cfft_logits_rows_operand_bytes(s.NX, Cin) : 0;
}
hipError_t conv_fft_logits_pack(const float* w_hwio, void* aop, int H, int W, int Cin, int Cout, hipStream_t st, float* wscale) {
  Sizes s;
  if (!sizes_of(H, W, 9, &s) || Cin % 16 || Cout > 16 || !wscale) return hipErrorInvalidValue;
  if (hipError_t e = hipMemsetAsync(wscale, 0, 2 * sizeof(float), st); e != hipSuccess) return e;
  const size_t pairs = (size_t)Cin * Cout;
  const dim3 bgrid((unsigned)((pairs + 255) / 256 > 1024 ? 1024 : (pairs + 255) / 256));
  hipLaunchKernelGGL(weight_bound_kernel<81>, bgrid, dim3(256), 0, st, w_hwio, pairs, 0, wscale);
  if (!cfft_logits_rows_pack(s.NX, w_hwio, aop, Cin, Cout, wscale, st)) return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---- the plan (conv_fft_plan.h) ----
// the one place that lays the workspace out: the regions in this order, each at the next multiple of 256 bytes
static void carve(FftPlan* p, size_t t, size_t xs, size_t yf, size_t sc_fwd, size_t sc_inv) {
  FftRegion* const regions[] = {&p->T, &p->Xs, &p->Yf, &p->t16_fwd, &p->t16_inv};
  const size_t bytes[] = {t, xs, yf, sc_fwd, sc_inv};
  size_t off = 0;
  for (int i = 0; i < 5; ++i) {
    regions[i]->off = off;
    regions[i]->bytes = bytes[i];
    off += align256(bytes[i]);
  }
  p->total = off;
}
FftPlan conv_fft_plan(const FftArgs& a, int ks, int np, int pool_ks_next) {
  FftPlan p;
  Sizes s, n;
  p.ok = a.tiles ? sizes_of(a.H / 2, a.W / 2, ks, &s) : sizes_of(a.H, a.W, ks, &s, a.circ);
  if (!p.ok) return p;
  p.ks = ks; p.np = np;
  p.NY = s.NY; p.NX = s.NX; p.NXH = s.NX / 2 + 1; p.F = s.NY * p.NXH;
  if (pool_ks_next && sizes_of((a.H + 1) / 2, (a.W + 1) / 2, pool_ks_next, &n)) p.NX_next = n.NX;
  p.opad = (ks - 1) / 2 + (a.circ ? 4 : 0);      // windows: the valid region starts 4 rows into the window
  p.norm = 1.0f / (float)(s.NY * s.NX);
  p.map = a;
  p.map.CoutP = pad64(a.Cout);
  p.col = p.map;
  if (a.tiles) { p.col.B = 4 * a.B; p.col.H = s.NY; p.col.W = a.W / 2; p.col.tiles = 0; }
  p.inv = p.col;
  if (a.tiles) p.inv.H = a.H / 2;
  if (a.circ) { p.inv.H = a.H - 8; p.inv.W = a.W - 8; }
  const FftArgs& c = p.col;
  p.ldy = padn(c.Cout, cgemm_split_ntile(np, c.Cout));      // complex numbers per row of the product spectra: whole N tiles, and whole
  if (p.ldy < pad64(c.Cout)) p.ldy = pad64(c.Cout);          // 64-channel blocks of the inverse passes (columns no tile writes are never stored)
  p.MT = cgemm_split_mtile(np, c.B, c.Cout);
  p.inv_cb = s.NY > 100 ? 32 : 64;      // colblk<NY>() of the inverse column pass
  const size_t cop = pad64(c.Cout), cmax = (size_t)c.Cin > cop ? c.Cin : cop;
  const size_t bp = (size_t)(c.B + p.MT - 1) / p.MT * p.MT;
  carve(&p, (size_t)c.B * p.NXH * c.H * cmax * sizeof(cf), (size_t)p.F * bp * c.Cin * 4 * cgemm_split_parts(np), (size_t)p.F * c.B * p.ldy * sizeof(cf),
        (size_t)c.B * c.H * (c.Cin / CB) * sizeof(float), (size_t)c.B * p.NXH * (cop / p.inv_cb) * sizeof(float));
  return p;
}
FftPlan conv_fft_logits_plan(const FftArgs& a) {
  FftPlan p;
  Sizes s;
  p.ok = sizes_of(a.H, a.W, 9, &s);
  if (!p.ok) return p;
  p.ks = 9; p.np = kFftFp16x2;
  p.NY = s.NY; p.NX = s.NX; p.NXH = s.NX / 2 + 1; p.F = s.NY * p.NXH;
  p.opad = 4;
  p.norm = 1.0f / (float)s.NX;      // no column transform
  p.map = a;
  p.map.CoutP = pad64(a.Cout);
  p.col = p.inv = p.map;
  carve(&p, (size_t)a.B * a.H * p.NXH * CB * sizeof(cf), 0, 0, 0, 0);      // S = T'[b][y][kx][64]
  return p;
}
hipError_t conv_fft_plan_twiddles(FftPlan* p) {
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  const cf* twb = twiddle_table(dev);
  if (!twb) return hipErrorOutOfMemory;
  p->twx = twb + tw_offset(p->NX);
  p->twy = twb + tw_offset(p->NY);
  p->twx_next = p->NX_next ? twb + tw_offset(p->NX_next) : nullptr;
  return hipSuccess;
}
size_t conv_fft_workspace_bytes(const FftArgs& a, int ks, int np) {
  const FftPlan p = conv_fft_plan(a, ks, np);
  return p.ok ? p.total : 0;
}
// the split spectra of an NHWC fp32 tensor alone (conv_fft_spectra): xs = conv_fft_xs_bytes() bytes, work = conv_fft_workspace_bytes()
size_t conv_fft_xs_bytes(const FftArgs& a0, int ks, int np) {
  FftArgs a = a0;
  a.tiles = 0;
  const FftPlan p = conv_fft_plan(a, ks, np);
  return p.ok ? align256(p.Xs.bytes) : 0;
}

// ---- what each variant takes: null, or the first condition the call violates ----
const char* conv_fft_refusal(const FftPlan& p, FftLayout in, FftLayout out, const FftLink& k, int t16) {
  const FftArgs& a = p.map;
  if (!p.ok) return "no transform size for this map and kernel size";
  if (a.Cin % CB || a.Cin < CB || a.Cout < 1 || a.B < 1) return "input channels in whole blocks of 64, at least one output channel and one image";
  if (out == kFftBf16Planar && a.Cout % 8) return "planar bf16 output needs whole units of 8 channels";
  if (!operand_form(p.np)) return "operand forms of the channel GEMM: 2, 4, 5";
  if (p.np == kFftFp16x1 && a.Cin % 32) return "the one-part operand stages 32 input channels at a time";
  if (a.circ && (k.t_in || k.t_next || k.merge || in != kFftF32Nhwc || out != kFftF32Nhwc)) return "windows take fp32 NHWC on both sides and no hand-over";
  if ((k.next.pool || k.next.merge) && (!k.t_next || (k.next.pool && k.next.merge))) return "a pool or merge hand-over needs t_next, and only one of the two";
  // bf16 handles: the merge hand-over (conv4_fullres -> conv5) in 16-bit form -- t_next / t_in is a complex-fp16 T followed by its tile scale words
  const bool h16 = t16 && ((k.t_next && k.next.merge && !k.t_in) || (k.t_in && !k.t_next));
  if ((k.t_in || k.t_next) && !h16 && (in != kFftF32Nhwc || out != kFftF32Nhwc)) return "a 32-bit hand-over takes fp32 NHWC tensors on both sides";
  if (k.t_next && a.Cout % CB) return "a hand-over needs output channels in whole blocks of 64";
  if (t16 && p.np != kFftFp16x1) return "16-bit T needs the one-part operand form";
  if (t16 && (in == kFftF32Nhwc || out == kFftF32Nhwc)) return "16-bit T needs bf16 tensors on both sides";
  if (t16 && (k.xs || ((k.t_in || k.t_next) && !h16))) return "16-bit T keeps no spectra and hands over only across the merge";
  if (k.merge && in == kFftBf16Planar) return "the merge reads NHWC";
  if (k.xs_ready && !k.xs) return "ready spectra without their buffer";
  if (k.t_next && k.next.pool && !p.NX_next) return "no transform size for the pooled map";
  return nullptr;
}
// 2 x 2 tiles: a 5x5 layer whose output goes through the pool hand-over into a 5x5 layer, on the model's 120 x 180 map (cfft_tiles_supported)
const char* conv_fft_tiles_refusal(const FftPlan& p, FftLayout in, FftLayout, const FftLink& k) {
  const FftArgs& a = p.map;
  if (!a.tiles) return "not planned as tiles";
  if (p.np != kFftFp16x2 || in != kFftF32Nhwc) return "tiles exist on fp32 handles (operand form 4, fp32 NHWC input)";
  if (k.t_in || k.merge || k.xs || k.xs_ready || k.win_map) return "tiles read their own map: no hand-over in, no merge, no kept spectra, no windows";
  if (!k.t_next || !k.next.pool || k.next.merge) return "tiles feed the pool hand-over and nothing else";
  if (!a.fft_reg) return "tiles exist as register kernels only";
  if (p.ks != 5 || k.next.ks_next != 5) return "tiles exist for a 5x5 layer in front of a 5x5 layer";
  if (a.circ || a.win_map || a.B < 1) return "tiles of whole maps, at least one image";
  if (!conv_fft_pool_fusable(a, p.ks, k.next.ks_next)) return "no pool hand-over for this pair of layers";
  if (a.H % 4 || a.W % 4 || !p.ok || !cfft_tiles_supported(p.NY, p.NX, a)) return "tiles exist for the model's 120 x 180 map geometry";
  return nullptr;
}
// the logits layer on the row spectra of its input: a 9x9 layer with at most 16 output channels whose row-transformed input was handed over at a 96-point row length
const char* conv_fft_logits_refusal(const FftPlan& p, int ks, int np, FftLayout in, FftLayout out, const FftLink& k, int common) {
  const FftArgs& a = p.map;
  if (ks != 9 || np != kFftFp16x2 || in != kFftF32Nhwc || out != kFftF32Nhwc) return "logits rows: a 9x9 layer of an fp32 handle, fp32 NHWC on both sides";
  if (a.circ || a.tiles || a.win_map || k.win_map || k.win_scatter) return "logits rows: whole maps, no windows, no tiles";
  if (!p.ok || !conv_fft_supported(a, 9) || !cfft_logits_rows_supported(p.NX, a)) return "logits rows: 96-point rows, at most 64 rows and 16 output channels";
  if (!k.t_in || k.t_in_16) return "logits rows read a 32-bit row-transformed input";
  if (k.t_next || k.next.pool || k.next.merge || k.merge || k.xs || k.xs_ready) return "logits rows hand nothing over and keep no spectra";
  if (common) return "logits rows scale each image by its own word";
  return nullptr;
}

// ---- the five passes.  Each picks its kernel here, in order of preference; true: launched.  false: no kernel took the case (or a HIP call in front of the launch
// failed, which hipGetLastError() then reports).
namespace {
struct Run {      // one call: the plan bound to its workspace, its scale and its stream
  const FftPlan& p;
  cf* T;
  void* Xs;
  cf* Yf;
  Fp16Scale sc;
  float yshift, yinv;      // 16-bit product spectra (below)
  hipStream_t st;
  bool reg() const { return p.map.fft_reg != 0; }
};
// what the kernels take of the caller's scale: np >= 4 only; hf = the rows a column transform sums; the words of a 16-bit T / T' from the plan's regions
Fp16Scale device_scale(const FftPlan& p, const FftScale* in, float hf, void* work) {
  Fp16Scale sc;
  if (p.np < 4 || !in) return sc;
  sc.tmax = in->tmax; sc.tmax_next = in->tmax_next; sc.winv = in->winv; sc.common = in->common; sc.t16 = in->t16;
  sc.hf = hf;
  sc.nb = p.col.B;
  if (sc.t16) {
    sc.t16_fwd = p.at<float>(work, p.t16_fwd);
    sc.t16_inv = p.at<float>(work, p.t16_inv);
    sc.t16_cb = p.inv_cb;
  }
  return sc;
}
hipError_t refuse(const char** why, const char* reason) {
  if (why) *why = reason;
  return hipErrorInvalidValue;
}
hipError_t not_launched(const char** why, const char* reason) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : refuse(why, reason);
}

// 1. rows, forward: the layer's input -> T.  Tiles: their register kernel.  Merged input: register, else LDS.  Windows cut from their map: the register kernel
// (the only one; conv_fft_win_gather_supported said so).  Plain: register, else LDS.  (The register kernels take bf16 NHWC into a 16-bit T: fp32 input --
// conv_fft_spectra always -- ends on the LDS kernel by this same rule.)
bool pass_rows_fwd(const Run& r, FftLayout in, const FftMerge* merge) {
  const FftPlan& p = r.p;
  const FftArgs& a = p.map;
  if (a.tiles) return cfft_rows_fwd_tile_reg(p.NY, p.NX, a, r.T, r.sc.tmax, r.st);
  if (merge) return (r.reg() && cfft_rows_fwd_merge_reg(p.NX, a, *merge, in, r.T, r.sc.tmax, r.st, r.sc.t16_fwd)) || cfft_rows_fwd_merge(p.NX, a, *merge, in, r.T, p.twx, r.sc.tmax, r.st, r.sc.t16_fwd);
  if (a.win_map) return cfft_rows_fwd_win_reg(p.NX, a, r.T, r.sc.tmax, r.st);
  return (r.reg() && cfft_rows_fwd_reg(p.NX, a, in, r.T, r.sc.tmax, r.st, r.sc.t16_fwd)) || cfft_rows_fwd(p.NX, a, in, r.T, p.twx, r.sc.tmax, r.st, r.sc.t16_fwd);
}
// 2. columns, forward, with the operand split: T (or the handed-over one) -> Xs.  One kernel family (LDS).
bool pass_cols_fwd(const Run& r, const cf* Tin) { return cfft_cols_fwd(r.p.NY, r.p.col, r.p.np, Tin, r.Xs, r.p.twy, r.p.NXH, r.p.MT, r.sc, r.st); }
// 3. the channel GEMM: Xs x filter spectra -> Yf, between the two optional events
hipError_t pass_gemm(const Run& r, hipEvent_t g0, hipEvent_t g1) {
  const FftArgs& c = r.p.col;
  if (g0 && hipEventRecord(g0, r.st) != hipSuccess) return hipErrorUnknown;
  if (hipError_t e = cgemm_split(r.Xs, c.wp, r.Yf, r.p.np, r.p.F, c.B, c.Cin, c.Cout, r.p.ldy, r.st, r.yshift); e != hipSuccess) return e;
  if (g1 && hipEventRecord(g1, r.st) != hipSuccess) return hipErrorUnknown;
  return hipSuccess;
}
// 4. columns, inverse: Yf -> T' (the valid rows).  Register (64-channel work groups only), else LDS; tiles have the register kernel alone.
bool pass_cols_inv(const Run& r) {
  const FftPlan& p = r.p;
  if (r.reg() && p.inv_cb == 64 && cfft_cols_inv_reg(p.NY, p.inv, r.Yf, r.T, p.NXH, p.ldy, p.opad, r.st, r.sc.t16_inv, r.yinv)) return true;
  if (p.map.tiles) return false;
  return cfft_cols_inv(p.NY, p.inv, r.Yf, r.T, p.twy, p.NXH, p.ldy, p.opad, r.st, r.sc.t16_inv, r.yinv);
}
// 5. rows, inverse, with the epilogue: T' -> the layer's output, or -- fused with the next layer's forward rows -- its hand-over t_next.
//    tiles: their pool hand-over.  Pool: the one LDS kernel.  Merge: register, else (32-bit only) LDS.  Same map: register, else LDS.
//    Output: matrix cores (rows_mfma), register, LDS -- the scatter into the map exists in the register kernel only.  lds_only: the logits rows (their S has the
//    64-channel layout of the LDS kernel's T' and an odd channel count).
bool pass_rows_inv(const Run& r, FftLayout out, const FftLink& k, bool lds_only = false) {
  const FftPlan& p = r.p;
  const FftArgs& a = p.map;
  cf* Tn = static_cast<cf*>(k.t_next);
  if (lds_only) return cfft_rows_inv(p.NX, p.inv, out, r.T, p.twx, p.opad, p.norm, r.sc, r.st);
  if (a.tiles) return cfft_rows_inv_pool_tile_reg(p.NY, p.NX, a, r.T, Tn, p.norm, r.sc, r.st);
  if (Tn && k.next.pool) return cfft_rows_inv_pool_fwd(p.NX, p.NX_next, a, r.T, Tn, p.twx, p.twx_next, p.opad, p.norm, r.sc, r.st);
  if (Tn && k.next.merge) {
    if (r.sc.t16) return r.reg() && cfft_rows_inv_merge_fwd_reg(p.NX, a, *k.next.merge, r.T, Tn, p.opad, p.norm, r.sc, r.st, conv_fft_handover16(a.B, p.NXH, a.H, a.Cout).words(Tn));
    return (r.reg() && cfft_rows_inv_merge_fwd_reg(p.NX, a, *k.next.merge, r.T, Tn, p.opad, p.norm, r.sc, r.st)) || cfft_rows_inv_merge_fwd(p.NX, a, *k.next.merge, r.T, Tn, p.twx, p.opad, p.norm, r.sc, r.st);
  }
  if (Tn) return (r.reg() && cfft_rows_inv_fwd_reg(p.NX, a, r.T, Tn, p.opad, p.norm, r.sc, r.st)) || cfft_rows_inv_fwd(p.NX, a, r.T, Tn, p.twx, p.opad, p.norm, r.sc, r.st);
  if ((p.inv.rows_mfma & 1) && cfft_rows_inv_mfma(p.NX, p.inv, out, r.T, p.opad, p.norm, r.sc, r.st)) return true;
  if (r.reg() && cfft_rows_inv_reg(p.NX, p.inv, out, r.T, p.opad, p.norm, r.sc, r.st)) return true;
  if (p.inv.win_scatter) return false;
  return cfft_rows_inv(p.NX, p.inv, out, r.T, p.twx, p.opad, p.norm, r.sc, r.st);
}
const char* scale_refusal(const FftPlan& p, const FftScale* sc, const FftLink& k) {
  if (p.np < 4) return nullptr;
  if (!sc || !sc->tmax || !sc->winv) return "scaled operand forms need the scale words of the input and of the filter spectra";
  if (k.t_next && !sc->tmax_next) return "a hand-over needs the scale words of the next layer";
  return nullptr;
}
}  // namespace

// The five passes on the map, on windows or on tiles (the refusals above say which combinations of link, layouts and operand form exist).
hipError_t conv_fft_f32(FftPlan p, FftLayout in, FftLayout out, void* work, const FftLink& k, hipEvent_t g0, hipEvent_t g1, hipStream_t st, const FftScale* scp, const char** why) {
  const int t16 = p.np >= 4 && scp ? scp->t16 : 0;
  if (const char* no = p.map.tiles ? conv_fft_tiles_refusal(p, in, out, k) : conv_fft_refusal(p, in, out, k, t16)) return refuse(why, no);
  if (const char* no = scale_refusal(p, scp, k)) return refuse(why, no);
  if (hipError_t e = conv_fft_plan_twiddles(&p); e != hipSuccess) return e;
  Run r{p, p.at<cf>(work, p.T), k.xs ? k.xs : p.at<void>(work, p.Xs), p.at<cf>(work, p.Yf), device_scale(p, scp, (float)p.col.H, work), 0.f, 0.f, st};
  // a handed-over 16-bit T carries its scale words behind it (written by the producing layer's fused row kernel)
  if (r.sc.t16 && k.t_in) r.sc.t16_fwd = conv_fft_handover16(p.col.B, p.NXH, p.col.H, p.col.Cin).words(k.t_in);
  // 16-bit intermediates (bf16 handles, one-part route): the product spectra travel as complex fp16 too, under the constant shift of cgemm_split.hip
  // (same-box A/B at 256 images: 19.1 -> 18.0 ms per step, profiles/r05_ab_y16.log)
  r.yshift = r.sc.t16 ? cgemm_split_y16_shift(p.col.Cin) : 0.f;
  r.yinv = r.yshift != 0.f ? 1.0f / r.yshift : 0.f;
  if (!k.xs_ready) {
    if (!k.t_in && !pass_rows_fwd(r, in, k.merge)) return not_launched(why, "no forward row kernel for this case");
    if (!pass_cols_fwd(r, k.t_in ? static_cast<const cf*>(k.t_in) : r.T)) return not_launched(why, "no forward column kernel for this operand form and scale");
  }
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (hipError_t e = pass_gemm(r, g0, g1); e != hipSuccess) return e;
  if (!pass_cols_inv(r)) return not_launched(why, "no inverse column kernel for this case");
  if (!pass_rows_inv(r, out, k)) return not_launched(why, p.inv.win_scatter ? "the scatter into the map exists in the register kernel only" : "no kernel for this hand-over");
  return hipGetLastError();
}

// ---- the logits layer on the row spectra of its input (conv_fft_logits.hip).  No column pass, no filter spectra: the operand A (conv_fft_logits_pack), the
// contraction and one inverse row pass.  p.map.wp = the operand A; link.t_in = T[kx][c/16][b][y][16] with its words sc.tmax.  The image's scale is 2^k with
// tmax[b] 2^k < 2^15 (Fp16Scale::hf = 1: no column transform sums H rows), undone by the inverse row pass together with the operand's.
hipError_t conv_fft_logits_f32(FftPlan p, int ks, int np, FftLayout in, FftLayout out, void* work, const FftLink& k, hipEvent_t g0, hipEvent_t g1, hipStream_t st,
                               const FftScale* scp, const char** why) {
  if (const char* no = conv_fft_logits_refusal(p, ks, np, in, out, k, scp ? scp->common : 0)) return refuse(why, no);
  if (const char* no = scale_refusal(p, scp, k)) return refuse(why, no);
  if (hipError_t e = conv_fft_plan_twiddles(&p); e != hipSuccess) return e;
  const Run r{p, p.at<cf>(work, p.T), nullptr, nullptr, device_scale(p, scp, 1.f, work), 0.f, 0.f, st};
  if (g0 && hipEventRecord(g0, st) != hipSuccess) return hipErrorUnknown;
  if (!cfft_logits_rows(p.NX, p.map, static_cast<const cf*>(k.t_in), p.map.wp, r.sc.tmax, r.T, st)) return not_launched(why, "no logits-rows kernel for this case");
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (g1 && hipEventRecord(g1, st) != hipSuccess) return hipErrorUnknown;
  if (!pass_rows_inv(r, out, k, true)) return not_launched(why, "no inverse row kernel for this case");
  return hipGetLastError();
}

// the split spectra of an NHWC fp32 tensor alone: passes 1 and 2
hipError_t conv_fft_spectra(const FftArgs& a0, int ks, int np, void* work, void* xs, hipStream_t st, float* tmax, int common, const char** why) {
  FftArgs a = a0;
  a.tiles = 0;
  FftPlan p = conv_fft_plan(a, ks, np);
  if (!p.ok || !conv_fft_supported(a, ks, a.circ)) return refuse(why, "no transform size for this map and kernel size, or channels not in whole blocks of 64");
  if (!xs || (np >= 4 && !tmax)) return refuse(why, "spectra need their buffer and, in the scaled operand forms, the scale word");
  if (hipError_t e = conv_fft_plan_twiddles(&p); e != hipSuccess) return e;
  FftScale in;
  in.tmax = tmax; in.common = common;
  const Run r{p, p.at<cf>(work, p.T), xs, nullptr, device_scale(p, &in, (float)a.H, work), 0.f, 0.f, st};
  if (!pass_rows_fwd(r, kFftF32Nhwc, nullptr)) return not_launched(why, "no forward row kernel for this case");
  if (!pass_cols_fwd(r, r.T)) return not_launched(why, "no forward column kernel for this operand form and scale");
  return hipGetLastError();
}

}  // namespace jcm
