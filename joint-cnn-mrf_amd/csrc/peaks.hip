// Heat-map peaks: the top-P local maxima of every map of hm [B,HH,WW,K], their sub-cell offsets and their scores, one launch.
// Grid over (image, joint group): a work group owns G whole maps of one image, so the 3x3 test and the selection of the top P never leave the
// work group -- no halo, no merge of partial lists across work groups, no second pass.  (Row bands would need exactly that merge: the P best of
// a map can all lie in one band.)  G is the largest count whose planes fit 64 KB of LDS, evened out over the groups: 3 maps at 60x90 (64.8 KB,
// two work groups per CU), 1 map at 120x180 (86.4 KB).
// Stage: the image's HW * K floats are walked front to back, coalesced, as float4 where the image is 16-byte aligned, 8 loads in flight per thread,
// and the group's channels are scattered into planar LDS planes [G][S], S = HW | 1.  Only G of K
// lanes write per ds_write and lanes of one channel are 4 pixels apart, so the scatter is at most a few-way conflict on a step that is bound
// by the loads.  The 3x3 test then reads consecutive pixels in consecutive lanes (conflict-free).
// Selection: a thread tests the pixels tid, tid + T, ... of a plane and keeps its own 8 best local maxima in registers, sorted by (value
// descending, index ascending); at most P rounds of a work-group arg-max over the threads' heads (shuffles in the wave, 8 slots of LDS across
// the waves, double-buffered: one barrier per round), each round retiring its winner from the list of the thread that owns it.
#include <string>

#include "entry.h"

namespace jcm {

namespace {

constexpr int kPkThreads = 512;
constexpr int kPkWaves = kPkThreads / 64;
constexpr int kPkMaxP = 8;
constexpr int kPkUnroll = 8;                          // float4 loads a thread has in flight while staging
constexpr int kPkMaxHW = 21600;                      // 120 x 180, the size of the priors
constexpr int kPkLdsBudget = 64 * 1024;              // planes of one work group, where more than one map fits: two work groups per CU
constexpr int kPkLdsMax = (kPkMaxHW | 1) * 4;        // one map of the largest size
constexpr int kPkNone = 0x7fffffff;

__device__ __forceinline__ bool pk_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

template <bool VEC>
__global__ __launch_bounds__(kPkThreads) void hm_peaks_kernel(const float* __restrict__ hm, int B, int HH, int WW, int K, int G, int NG, int S, int P, float thr,
                                                              int32_t* __restrict__ cells, float* __restrict__ offsets, float* __restrict__ scores,
                                                              int32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) float planes[];      // [gn][S]
  __shared__ float rv[2][kPkWaves];
  __shared__ int ri[2][kPkWaves];
  const int tid = threadIdx.x;
  // Work groups are dealt round-robin over the 8 XCDs, each with an L2 of its own: the groups of one image are given block numbers 8 apart, so
  // that they share an L2 (the image is fetched into it once) and are in flight together.  Images are taken in chunks of 8 (the last may be shorter).
  const int chunk = blockIdx.x / (8 * NG), rem = blockIdx.x - chunk * 8 * NG, m = min(8, B - 8 * chunk);
  const int b = 8 * chunk + rem % m, k0 = (rem / m) * G;
  const int gn = min(G, K - k0);
  const int HW = HH * WW, n = HW * K;
  const float* src = hm + (size_t)b * n;

  int e0 = 0;      // first element of the scalar sweep
  if constexpr (VEC) {
    const float4* src4 = reinterpret_cast<const float4*>(src);
    const int nvec = n >> 2;
    // kPkUnroll loads in flight per thread, issued back to back in straight-line code (a branch around a load makes the compiler wait for the
    // loads before it; one load in flight per thread measured 9 % slower at [64,60,90,9]).  A trip's loads past the end re-read the last float4.
    for (int f0 = tid; f0 < nvec; f0 += kPkThreads * kPkUnroll) {
      float4 t[kPkUnroll];
#pragma unroll
      for (int u = 0; u < kPkUnroll; ++u) t[u] = src4[min(f0 + u * kPkThreads, nvec - 1)];
#pragma unroll
      for (int u = 0; u < kPkUnroll; ++u) {
        const int f = f0 + u * kPkThreads;
        if (f >= nvec) break;
        const float v[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
        int p = (4 * f) / K, c = 4 * f - p * K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if ((unsigned)(c - k0) < (unsigned)gn) planes[(c - k0) * S + p] = v[j];
          if (++c == K) { c = 0; ++p; }
        }
      }
    }
    e0 = nvec << 2;
  }
  for (int e = e0 + tid; e < n; e += kPkThreads) {
    const int p = e / K, c = e - p * K;
    if ((unsigned)(c - k0) < (unsigned)gn) planes[(c - k0) * S + p] = src[e];
  }
  __syncthreads();

  int par = 0;
  for (int g = 0; g < gn; ++g) {
    const float* pl = planes + g * S;
    float cv[kPkMaxP];
    int ci[kPkMaxP];
#pragma unroll
    for (int s = 0; s < kPkMaxP; ++s) { cv[s] = -INFINITY; ci[s] = kPkNone; }
    for (int p = tid; p < HW; p += kPkThreads) {
      const float v = pl[p];
      if (!(v > thr)) continue;
      const int r = p / WW, c = p - r * WW;
      const bool up = r > 0, dn = r < HH - 1, lf = c > 0, rt = c < WW - 1;
      bool ok = true;
      if (up) {      // the neighbours of a smaller index: strictly below
        const float* q = pl + p - WW;
        if (lf) ok &= v > q[-1];
        ok &= v > q[0];
        if (rt) ok &= v > q[1];
      }
      if (lf) ok &= v > pl[p - 1];
      if (rt) ok &= v >= pl[p + 1];
      if (dn) {
        const float* q = pl + p + WW;
        if (lf) ok &= v >= q[-1];
        ok &= v >= q[0];
        if (rt) ok &= v >= q[1];
      }
      if (!ok) continue;
      float nv = v;
      int ni = p;
#pragma unroll
      for (int s = 0; s < kPkMaxP; ++s) {      // sorted insert: the better of (carried, slot) stays, the other is carried on
        if (pk_better(nv, ni, cv[s], ci[s])) {
          const float tv = cv[s];
          const int ti = ci[s];
          cv[s] = nv; ci[s] = ni;
          nv = tv; ni = ti;
        }
      }
    }

    const size_t map = (size_t)b * K + k0 + g;
    int found = 0;
    for (; found < P; ++found) {
      float bv = cv[0];
      int bi = ci[0];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (pk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if ((tid & 63) == 0) { rv[par][tid >> 6] = bv; ri[par][tid >> 6] = bi; }
      __syncthreads();
      bv = rv[par][0];
      bi = ri[par][0];
#pragma unroll
      for (int w = 1; w < kPkWaves; ++w)
        if (pk_better(rv[par][w], ri[par][w], bv, bi)) { bv = rv[par][w]; bi = ri[par][w]; }
      par ^= 1;
      if (bi == kPkNone) break;      // the same for every thread
      if (bi % kPkThreads == tid) {      // mine: retire it
#pragma unroll
        for (int s = 0; s + 1 < kPkMaxP; ++s) { cv[s] = cv[s + 1]; ci[s] = ci[s + 1]; }
        cv[kPkMaxP - 1] = -INFINITY;
        ci[kPkMaxP - 1] = kPkNone;
      }
      if (tid == 0) {
        const int r = bi / WW, c = bi - r * WW;
        const size_t slot = map * P + found;
        cells[2 * slot] = r;
        cells[2 * slot + 1] = c;
        scores[slot] = bv;
        if (offsets) {
          float dr = 0.f, dc = 0.f;
          if (r > 0 && r < HH - 1) {
            const float a = pl[bi - WW], z = pl[bi + WW];
            dr = z > a ? 0.25f : (z < a ? -0.25f : 0.f);
          }
          if (c > 0 && c < WW - 1) {
            const float a = pl[bi - 1], z = pl[bi + 1];
            dc = z > a ? 0.25f : (z < a ? -0.25f : 0.f);
          }
          offsets[2 * slot] = dr;
          offsets[2 * slot + 1] = dc;
        }
      }
    }
    if (tid == 0) count[map] = found;
    if (tid >= found && tid < P) {      // filler
      const size_t slot = map * P + tid;
      cells[2 * slot] = -1;
      cells[2 * slot + 1] = -1;
      scores[slot] = 0.f;
      if (offsets) { offsets[2 * slot] = 0.f; offsets[2 * slot + 1] = 0.f; }
    }
  }
}

}  // namespace

hipError_t hm_peaks(const float* hm, int B, int HH, int WW, int K, int P, float threshold, int32_t* cells, float* offsets, float* scores, int32_t* count,
                    hipStream_t st) {
  const int64_t HW = (int64_t)HH * WW;
  if (B < 1 || HH < 1 || WW < 1 || K < 1 || P < 1 || P > kPkMaxP || HW > kPkMaxHW || HW * K >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
  const int S = (int)HW | 1;
  const int gmax = std::max(1, std::min(K, kPkLdsBudget / (S * 4)));
  const int NG = (K + gmax - 1) / gmax, G = (K + NG - 1) / NG;      // even groups: 10 maps are 3 + 3 + 3 + 1 either way, 4 maps are 2 + 2
  if ((int64_t)B * NG >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  const int lds = G * S * 4;
  // float4 loads need every image to start on 16 bytes
  const bool vec = (HW * K) % 4 == 0 && reinterpret_cast<uintptr_t>(hm) % 16 == 0;
  if (vec) {
    static LdsAttr attr;
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(hm_peaks_kernel<true>), kPkLdsMax); e != hipSuccess) return e;
    hipLaunchKernelGGL(hm_peaks_kernel<true>, dim3(B * NG), dim3(kPkThreads), lds, st, hm, B, HH, WW, K, G, NG, S, P, threshold, cells, offsets, scores, count);
  } else {
    static LdsAttr attr;
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(hm_peaks_kernel<false>), kPkLdsMax); e != hipSuccess) return e;
    hipLaunchKernelGGL(hm_peaks_kernel<false>, dim3(B * NG), dim3(kPkThreads), lds, st, hm, B, HH, WW, K, G, NG, S, P, threshold, cells, offsets, scores, count);
  }
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_hm_peaks(jcm_handle h, const float* hm, int B, int HH, int WW, int K, int P, float threshold, int32_t* cells, float* offsets, float* scores,
                 int32_t* count) {
  JCM_TRY(check(h, false));
  if (P < 1 || P > kPkMaxP) return fail(JCM_ERR_ARG, "hm_peaks: P = " + std::to_string(P) + " peaks per map; 1 <= P <= 8");
  if (B < 1 || HH < 1 || WW < 1 || K < 1) return fail(JCM_ERR_ARG, "hm_peaks: bad sizes (B, HH, WW, K >= 1)");
  if ((int64_t)HH * WW > kPkMaxHW)
    return fail(JCM_ERR_ARG, "hm_peaks: a map of " + std::to_string(HH) + " x " + std::to_string(WW) + " pixels; HH * WW <= 21600 (120 x 180), a larger map is not truncated");
  if ((int64_t)HH * WW * K >= ((int64_t)1 << 30) || (int64_t)B * K >= ((int64_t)1 << 31)) return fail(JCM_ERR_ARG, "hm_peaks: bad sizes (HH * WW * K < 2^30 and B * K < 2^31)");
  if (!hm || !cells || !scores || !count) return fail(JCM_ERR_ARG, "hm_peaks: null pointer (hm, cells, scores and count are required; offsets may be NULL)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  return timed_launch(h, "hm_peaks", [&] { return hm_peaks(hm, B, HH, WW, K, P, threshold, cells, offsets, scores, count, h->stream); });
}

}  // extern "C"
