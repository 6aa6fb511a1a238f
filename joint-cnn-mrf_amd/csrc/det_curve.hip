// Detection-rate curves of MODEC (evaluation.py:15-36) for every joint and every radius in one launch per batch.
// One work group per image reads the image's targets y[b] [HW][C] ONCE, front to back: a thread owns "quads" of 4 pixels x C channels = C
// consecutive float4, so the channel of every loaded register is a compile-time constant and its C running (value, pixel) bests stay in
// registers.  The bests are folded across the wave with __shfl_xor and across the waves through LDS, the first-occurrence rule of
// argmax_kernel (glue.hip) at every stage: the larger value wins, ties go to the lower pixel, a map of NaN / -inf only gives pixel 0.  Then K
// threads form the normalised distances (fp32, one IEEE operation per step: the library is built with -ffp-contract=off, sqrtf and the
// divide are the correctly rounded ones) and K * R threads add their 0 / 1 into the int32 hit counts -- integer sums, so the order of the
// images does not matter.  Nothing is read back and nothing but the radii (kernel arguments) comes from the host.
#include <string>

#include "entry.h"

namespace jcm {

namespace {

constexpr int kDetThreads = 512;      // >= kDetMaxK * kDetMaxR: one thread per (joint, radius) in the last step
constexpr int kDetWaves = kDetThreads / 64;
constexpr int kDetMinK = 8, kDetMaxK = 16, kDetMaxR = 32;      // joints 0 and 7 span the torso (evaluation.py:26)
constexpr int kNoPixel = 0x7fffffff;
static_assert(kDetThreads >= kDetMaxK * kDetMaxR, "one thread per (joint, radius)");

struct DetRadii { float v[kDetMaxR]; };

__device__ __forceinline__ void det_take(float& bv, int& bi, float v, int p) {
  if (v > bv || (v == bv && p < bi)) { bv = v; bi = p; }
}

// VEC: the image's HW * C floats are read as float4 (every image starts 16-byte aligned); the 0..3 pixels behind the last whole quad, or the
// whole image when !VEC, go pixel by pixel -- C consecutive floats per thread, the channel again a compile-time constant
template <int C, bool VEC>
__global__ __launch_bounds__(kDetThreads) void det_curve_kernel(const int32_t* __restrict__ pred, const float* __restrict__ y, int HW, int WW, int K, DetRadii radii,
                                                                int R, int32_t* __restrict__ true_out, float* __restrict__ nd_out, int32_t* __restrict__ hits) {
  __shared__ float redv[kDetWaves][C];
  __shared__ int redi[kDetWaves][C];
  __shared__ int trow[C], tcol[C];
  __shared__ float nds[kDetMaxK];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* src = y + (size_t)b * HW * C;
  float bv[C];
  int bi[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { bv[c] = -INFINITY; bi[c] = kNoPixel; }
  int p0 = 0;      // first pixel of the scalar sweep
  if constexpr (VEC) {
    const int nquad = HW >> 2;
    const float4* src4 = reinterpret_cast<const float4*>(src);
    for (int q = tid; q < nquad; q += kDetThreads) {
      float v[4 * C];
#pragma unroll
      for (int i = 0; i < C; ++i) {
        const float4 t = src4[(size_t)q * C + i];
        v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
      }
#pragma unroll
      for (int j = 0; j < 4 * C; ++j) det_take(bv[j % C], bi[j % C], v[j], 4 * q + j / C);
    }
    p0 = nquad << 2;
  }
  for (int p = p0 + tid; p < HW; p += kDetThreads) {
#pragma unroll
    for (int c = 0; c < C; ++c) det_take(bv[c], bi[c], src[(size_t)p * C + c], p);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv[c], o);
      const int oi = __shfl_xor(bi[c], o);
      det_take(bv[c], bi[c], ov, oi);
    }
    if ((tid & 63) == 0) { redv[tid >> 6][c] = bv[c]; redi[tid >> 6][c] = bi[c]; }
  }
  __syncthreads();
  if (tid < C) {
    float v = redv[0][tid];
    int i = redi[0][tid];
    for (int w = 1; w < kDetWaves; ++w) det_take(v, i, redv[w][tid], redi[w][tid]);
    if (i == kNoPixel) i = 0;      // all -inf / NaN map: np.argmax returns 0
    const int row = i / WW, col = i - row * WW;
    trow[tid] = row;
    tcol[tid] = col;
    if (true_out && tid < K) {
      true_out[((size_t)b * 2 + 0) * K + tid] = row;
      true_out[((size_t)b * 2 + 1) * K + tid] = col;
    }
  }
  __syncthreads();
  if (tid < K) {
    // evaluation.py:29-30 on integers that fp32 holds exactly
    const long long dr = trow[0] - trow[7], dc = tcol[0] - tcol[7];
    const float torso = sqrtf((float)(dr * dr + dc * dc));
    const long long er = (long long)pred[((size_t)b * 2 + 0) * K + tid] - trow[tid], ec = (long long)pred[((size_t)b * 2 + 1) * K + tid] - tcol[tid];
    const float nd = sqrtf((float)(er * er + ec * ec)) * 100.0f / torso;      // torso 0 -> inf or NaN: never a hit
    nds[tid] = nd;
    if (nd_out) nd_out[(size_t)b * K + tid] = nd;
  }
  __syncthreads();
  if (hits && tid < K * R) {
    const int k = tid / R, r = tid - k * R;
    if (nds[k] <= radii.v[r]) atomicAdd(&hits[k * R + r], 1);
  }
}

template <int C>
void det_launch(bool vec, const int32_t* pred, const float* y, int B, int HW, int WW, int K, const DetRadii& radii, int R, int32_t* true_out, float* nd_out,
                int32_t* hits, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((det_curve_kernel<C, true>), dim3(B), dim3(kDetThreads), 0, st, pred, y, HW, WW, K, radii, R, true_out, nd_out, hits);
  else hipLaunchKernelGGL((det_curve_kernel<C, false>), dim3(B), dim3(kDetThreads), 0, st, pred, y, HW, WW, K, radii, R, true_out, nd_out, hits);
}

}  // namespace

hipError_t det_curve(const int32_t* pred, const float* y, int B, int HW, int WW, int K, int C, const float* radii, int R, int32_t* true_out, float* nd_out,
                     int32_t* hits, hipStream_t st) {
  if (K < kDetMinK || K > kDetMaxK || C < K || C > kDetMaxK || R < 1 || R > kDetMaxR) return hipErrorInvalidValue;
  DetRadii rd;
  for (int r = 0; r < kDetMaxR; ++r) rd.v[r] = r < R ? radii[r] : 0.f;
  // float4 loads need every image to start on 16 bytes
  const bool vec = ((size_t)HW * C) % 4 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0;
  switch (C) {
#define JCM_DET_CASE(n) case n: det_launch<n>(vec, pred, y, B, HW, WW, K, rd, R, true_out, nd_out, hits, st); break;
    JCM_DET_CASE(8) JCM_DET_CASE(9) JCM_DET_CASE(10) JCM_DET_CASE(11) JCM_DET_CASE(12) JCM_DET_CASE(13) JCM_DET_CASE(14) JCM_DET_CASE(15) JCM_DET_CASE(16)
#undef JCM_DET_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_det_curve(jcm_handle h, const int32_t* pred_coords, const float* y, int B, int HH, int WW, int K, int C, const float* radii, int R,
                  int32_t* true_coords, float* norm_dist, int32_t* hits) {
  JCM_TRY(check(h, false));
  if (K < kDetMinK || K > kDetMaxK)
    return fail(JCM_ERR_ARG, "det_curve: K = " + std::to_string(K) + " joints; the torso is joints 0 and 7 (evaluation.py:26), so 8 <= K <= 16");
  if (C < K || C > kDetMaxK) return fail(JCM_ERR_ARG, "det_curve: C = " + std::to_string(C) + " target channels; K <= C <= 16 (K = " + std::to_string(K) + ")");
  if (R < 1 || R > kDetMaxR) return fail(JCM_ERR_ARG, "det_curve: R = " + std::to_string(R) + " radii; 1 <= R <= 32");
  if (B < 1 || HH < 1 || WW < 1 || (int64_t)HH * WW * C >= ((int64_t)1 << 31))
    return fail(JCM_ERR_ARG, "det_curve: bad sizes (B, HH, WW >= 1, HH * WW * C < 2^31)");
  if (!pred_coords || !y || !radii) return fail(JCM_ERR_ARG, "det_curve: null pointer (pred_coords, y and radii are required)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  return timed_launch(h, "det_curve", [&] { return det_curve(pred_coords, y, B, HH * WW, WW, K, C, radii, R, true_coords, norm_dist, hits, h->stream); });
}

}  // extern "C"
