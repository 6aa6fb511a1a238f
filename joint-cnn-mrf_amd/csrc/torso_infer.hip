// Torso map from the part detector (include/jcm.h: jcm_torso_infer): the torso cell that the nine part-detector maps and the nine
// learned priors e_{j|torso} explain best, and the 3x3 blob at it -- the tenth channel of the spatial model for an image without annotation.
//   C_j(t) = sum_a e_{j|torso}[59 + (a_y - t_y), 89 + (a_x - t_x)] u_j(a)      the ADJOINT of the pairwise pass: a correlation of joint j's likelihood
//   E(t)   = sum_j log(C_j(t) + d), j = 0 .. 8 in this order                   map with its prior, where the forward pass convolves the torso map
// The direct route ("torso_algo" = 1, the only one), four small steps on the handle's stream:
//   torso_lik_kernel     u_j = smf::lik_of (the expression of the spatial-model forward) as planar rows [B][9][60][96], zeros behind column 89;
//   torso_corr_kernel    one work group per (image, joint): the whole prior in LDS at a pitch of 200 floats behind 6 zeros (96 KB), so that a row of
//                        the window is [zeros | prior row | zeros] and no thread tests a border.  A thread owns 8 consecutive t_x of one t_y and slides
//                        an 8 + 8 register window along a_x, as sm_pair_conv_kernel does along x: per likelihood value 8 FMAs on registers, per 8
//                        values two 16-byte LDS reads.  The likelihood row depends on a_y only, the loop variable: it is uniform over the work group
//                        and comes through the scalar cache.  Summation in two levels like the forward kernel: the 90 (96) terms of a likelihood row
//                        into a fresh partial, the 60 partials into the total.  Where a thread's t_x runs past column 89 its window reads zeros of
//                        the margin or prior values it multiplies into an accumulator that is never stored;
//   torso_finish_kernel  one work group per image: the fixed-order sum of the nine logs, the first-occurrence arg-max (the rules of argmax_kernel,
//                        glue.hip), the cell and the blob;
//   torso_blob_kernel    cells_in given: the blob alone, at the given cells clamped into the map -- the device-side blob writer of the per-person maps.
// No atomics; every store is a vector store of plain C++.
#include <string>

#include "entry.h"
#include "sm_lds_fft.h"

namespace jcm {

namespace {

constexpr int kTiK = 9;                           // joints
constexpr int kTiPJ = kC - 1;                     // pairs per joint in sp_energy: <j>_<c>, c in name order without j; the torso is the last
constexpr int kTiLP = 96;                         // likelihood row pitch (90 -> 96, zero padded)
constexpr int kTiPP = 200;                        // prior row pitch in LDS
constexpr int kTiMG = 6;                          // zeros in front of a prior row: column x of the prior sits at kTiMG + x
constexpr int kTiXT = 8;                          // outputs per thread
constexpr int kTiStrips = kTiLP / kTiXT;          // 12 strips of 8 cover t_x = 0 .. 95
constexpr int kTiThreads = 768;                   // 60 rows x 12 strips = 720 active
constexpr int kTiFinThreads = 256;
constexpr float kTiDelta = 1e-6f;                 // main.py:110
constexpr int kTiNone = 0x7fffffff;
static_assert(kTiMG + kHmW - 1 - (kTiLP - kTiXT) - (kTiXT - 1) == 0, "the window of the last strip starts at LDS column 0");
static_assert((kTiMG + kHmW - 1 - (kTiXT - 1)) % 4 == 0 && kTiPP % 4 == 0, "16-byte LDS reads");
static_assert(kTiMG + kHmW - 1 - (kTiXT - 1) + kTiLP + kTiXT <= kTiPP, "the window of the first strip ends inside the row");
static_assert(kTiMG + kPrW <= kTiPP, "a prior row fits");

__device__ __forceinline__ bool ti_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__global__ void torso_lik_kernel(const float* __restrict__ prob, const float* __restrict__ sc, const float* __restrict__ sh, float* __restrict__ lik, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % kTiLP);
    int64_t r = i / kTiLP;
    const int y = (int)(r % kHmH); r /= kHmH;
    const int j = (int)(r % kTiK);
    const int64_t b = r / kTiK;
    lik[i] = x < kHmW ? smf::lik_of(prob, kTiK, nullptr, 0, sc, sh, (b * kHmH + y) * kHmW + x, j) : 0.f;
  }
}

// corr[b][j][t_y][t_x] = sum_{a_y} sum_{a_x} prior_j[59 + a_y - t_y][89 + a_x - t_x] * lik[b][j][a_y][a_x]
__global__ __launch_bounds__(kTiThreads) void torso_corr_kernel(const float* __restrict__ spe, const float* __restrict__ lik, float* __restrict__ corr) {
  extern __shared__ __attribute__((aligned(16))) float pl[];      // [120][200]
  const int j = blockIdx.x % kTiK, tid = threadIdx.x;      // blockIdx.x = image * 9 + joint
  const float* pr = spe + (size_t)(j * kTiPJ + kTiPJ - 1) * (kPrH * kPrW);      // pair <j>_torso
  for (int i = tid; i < kPrH * kTiPP; i += kTiThreads) {
    const int r = i / kTiPP, c = i - r * kTiPP - kTiMG;
    pl[i] = (unsigned)c < (unsigned)kPrW ? pr[r * kPrW + c] : 0.f;
  }
  __syncthreads();
  const int ty = tid / kTiStrips, x0 = (tid - ty * kTiStrips) * kTiXT;
  if (ty >= kHmH) return;
  const float* lk = lik + (size_t)blockIdx.x * kHmH * kTiLP;      // work-group uniform
  float acc[kTiXT];
#pragma unroll
  for (int q = 0; q < kTiXT; ++q) acc[q] = 0.f;
  for (int ay = 0; ay < kHmH; ++ay) {
    float racc[kTiXT];
#pragma unroll
    for (int q = 0; q < kTiXT; ++q) racc[q] = 0.f;
    // LDS column of prior column 89 + a_x - (x0 + q): kTiMG + 89 - x0 + a_x - q = (88 - x0) + a_x + (7 - q); 88 - x0 is a multiple of 8 in 0 .. 88
    const float* arow = pl + (kHmH - 1 + ay - ty) * kTiPP + (kTiMG + kHmW - 1 - (kTiXT - 1) - x0);
    const float* hrow = lk + ay * kTiLP;
    float win[2 * kTiXT];
    *reinterpret_cast<float4*>(win) = *reinterpret_cast<const float4*>(arow);
    *reinterpret_cast<float4*>(win + 4) = *reinterpret_cast<const float4*>(arow + 4);
#pragma unroll
    for (int tb = 0; tb < kTiLP / kTiXT; ++tb) {
      *reinterpret_cast<float4*>(win + 8) = *reinterpret_cast<const float4*>(arow + tb * 8 + 8);
      *reinterpret_cast<float4*>(win + 12) = *reinterpret_cast<const float4*>(arow + tb * 8 + 12);
#pragma unroll
      for (int i = 0; i < kTiXT; ++i) {
        const float hv = hrow[tb * 8 + i];      // uniform -> scalar load
#pragma unroll
        for (int q = 0; q < kTiXT; ++q) racc[q] = fmaf(hv, win[i + (kTiXT - 1) - q], racc[q]);
      }
#pragma unroll
      for (int q = 0; q < kTiXT; ++q) win[q] = win[q + 8];
    }
#pragma unroll
    for (int q = 0; q < kTiXT; ++q) acc[q] += racc[q];
  }
  float* o = corr + (size_t)blockIdx.x * kHmHW + ty * kHmW + x0;
#pragma unroll
  for (int q = 0; q < kTiXT; ++q)
    if (x0 + q < kHmW) o[q] = acc[q];
}

// the 3x3 binomial blob of data.target_heat_maps centred on (cy, cx), cut at the border: outer([1,2,1],[1,2,1]) / 16, every value exact
__device__ __forceinline__ void ti_write_blob(float* __restrict__ t, int cy, int cx, int tid, int nthreads) {
  for (int p = tid; p < kHmHW; p += nthreads) {
    const int y = p / kHmW, x = p - y * kHmW;
    const int dy = abs(y - cy), dx = abs(x - cx);
    t[p] = (dy <= 1 && dx <= 1) ? (float)((2 - dy) * (2 - dx)) / 16.f : 0.f;
  }
}

__global__ __launch_bounds__(kTiFinThreads) void torso_finish_kernel(const float* __restrict__ corr, float* __restrict__ energy, int32_t* __restrict__ cell,
                                                                    float* __restrict__ torso) {
  __shared__ float rv[kTiFinThreads / 64];
  __shared__ int ri[kTiFinThreads / 64];
  __shared__ int tcell;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* cb = corr + (size_t)b * kTiK * kHmHW;
  float bv = -INFINITY;
  int bi = kTiNone;
  for (int p = tid; p < kHmHW; p += kTiFinThreads) {
    float e = logf(cb[p] + kTiDelta);
#pragma unroll
    for (int j = 1; j < kTiK; ++j) e = e + logf(cb[j * kHmHW + p] + kTiDelta);
    if (energy) energy[(size_t)b * kHmHW + p] = e;
    if (ti_better(e, p, bv, bi)) { bv = e; bi = p; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ti_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { rv[tid >> 6] = bv; ri[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kTiFinThreads / 64; ++w)
      if (ti_better(rv[w], ri[w], bv, bi)) { bv = rv[w]; bi = ri[w]; }
    if (bi == kTiNone) bi = 0;      // NaN everywhere: outside the contract, but a cell of the map all the same
    tcell = bi;
    cell[b * 2] = bi / kHmW;
    cell[b * 2 + 1] = bi - (bi / kHmW) * kHmW;
  }
  __syncthreads();
  if (torso) ti_write_blob(torso + (size_t)b * kHmHW, tcell / kHmW, tcell - (tcell / kHmW) * kHmW, tid, kTiFinThreads);
}

__global__ __launch_bounds__(kTiFinThreads) void torso_blob_kernel(const int32_t* __restrict__ cells_in, float* __restrict__ torso) {
  const int b = blockIdx.x;
  const int cy = min(max(cells_in[b * 2], 0), kHmH - 1), cx = min(max(cells_in[b * 2 + 1], 0), kHmW - 1);      // clamped before any index is formed
  ti_write_blob(torso + (size_t)b * kHmHW, cy, cx, threadIdx.x, kTiFinThreads);
}

}  // namespace

hipError_t torso_infer_direct(const float* prob, int B, const float* sp_energy, const float* bn_scale, const float* bn_shift, float* lik, float* corr,
                              float* energy, int32_t* cell, float* torso, hipStream_t st) {
  if (B < 1 || B > kTorsoMaxB) return hipErrorInvalidValue;
  const int64_t total = (int64_t)B * kTiK * kHmH * kTiLP;
  const int64_t g = (total + 255) / 256;
  hipLaunchKernelGGL(torso_lik_kernel, dim3((int)(g > 8192 ? 8192 : g)), dim3(256), 0, st, prob, bn_scale, bn_shift, lik, total);
  const int lds = kPrH * kTiPP * sizeof(float);
  static LdsAttr attr;
  if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(torso_corr_kernel), lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(torso_corr_kernel, dim3(B * kTiK), dim3(kTiThreads), lds, st, sp_energy, lik, corr);
  hipLaunchKernelGGL(torso_finish_kernel, dim3(B), dim3(kTiFinThreads), 0, st, corr, energy, cell, torso);
  return hipGetLastError();
}

hipError_t torso_blobs(const int32_t* cells_in, int B, float* torso, hipStream_t st) {
  if (B < 1 || B > kTorsoMaxB) return hipErrorInvalidValue;
  hipLaunchKernelGGL(torso_blob_kernel, dim3(B), dim3(kTiFinThreads), 0, st, cells_in, torso);
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_torso_infer(jcm_handle h, const float* prob, int B, int HH, int WW, int K, const int32_t* cells_in, float* energy, int32_t* cell, float* torso) {
  JCM_TRY(check(h, true));
  if (HH != kHmH || WW != kHmW || K != kTiK)
    return fail(JCM_ERR_ARG, "torso_infer: maps of " + std::to_string(HH) + " x " + std::to_string(WW) + " x " + std::to_string(K) + "; the geometry is fixed at 60 x 90 x 9");
  if (B < 1 || B > kTorsoMaxB) return fail(JCM_ERR_ARG, "torso_infer: bad batch size (1 <= B <= " + std::to_string(kTorsoMaxB) + ")");
  if (cells_in ? !torso : (!prob || !cell))
    return fail(JCM_ERR_ARG, "torso_infer: null pointer (prob and cell are required, energy and torso may be NULL; with cells_in, torso is required and nothing else is read or written)");
  if (!cells_in && (!h->has_sm || h->K != kTiK)) return fail(JCM_ERR_STATE, "torso_infer: the handle holds no spatial-model parameters for 9 joints");
  if (!cells_in && h->torso_algo != 1) return fail(JCM_ERR_STATE, "torso_algo must be 1 (direct)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  if (cells_in) return timed_launch(c, "torso_infer", [&] { return torso_blobs(cells_in, B, torso, c->stream); });
  float *lik = nullptr, *corr = nullptr;
  return arena_launch(c, "torso_infer", [&] {
    lik = arena_alloc<float>(c, (size_t)B * kTiK * kHmH * kTiLP);
    corr = arena_alloc<float>(c, (size_t)B * kTiK * kHmHW);
  }, [&] { return torso_infer_direct(prob, B, c->sp_energy, c->bn_sm_scale, c->bn_sm_shift, lik, corr, energy, cell, torso, c->stream); });
}

}  // extern "C"
