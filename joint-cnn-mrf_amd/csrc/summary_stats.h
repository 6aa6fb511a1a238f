// Device side of the TF-1.x histogram statistics shared by summary.hip (jcm_tensor_stats) and act_summary.hip (jcm_act_summary):
// the bucket table and its search, the per-thread accumulator, the fixed-order fold of a work group and of a segment's chunks.
// Sums are fixed-order folds in double, min / max are order-free, only the integer bucket counts use atomics.
#pragma once
#include <cfloat>
#include <cmath>

#include "ctx.h"

namespace jcm {

namespace {

constexpr int kPosLimits = JCM_HIST_BUCKETS / 2;     // 1e-12 * 1.1^k below 1e20, then DBL_MAX
constexpr int kStatsThreads = 256;
constexpr int kStatsWaves = kStatsThreads / 64;

// histogram.cc InitDefaultBucketsInner: the positive half of the bucket limits (the table is mirrored around 0.0)
struct PosLimits {
  double v[kPosLimits];
  int n = 0;
  PosLimits() {
    double x = 1.0e-12;
    while (x < 1.0e20 && n < kPosLimits - 1) {
      v[n++] = x;
      x *= 1.1;
    }
    v[n++] = DBL_MAX;
  }
};
const PosLimits& pos_limits() {
  static const PosLimits L;
  return L;
}

// the table on the device (uploaded on the handle's first use, in stream order)
int hist_limits_dev(jcm_ctx* c) {
  if (pos_limits().n != kPosLimits) return fail(JCM_ERR_STATE, "histogram bucket table has the wrong size");
  if (!c->hist_limits) {
    JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->hist_limits), kPosLimits * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->hist_limits, pos_limits().v, kPosLimits * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  return JCM_OK;
}

struct Part {
  float mn, mx;
  double s, ss;
  unsigned num, npos, nnf, pad;
};

// index of the TF bucket of a finite nonzero-or-zero value d = (double)u: std::upper_bound over the full limit table
// [-p[P-1], ..., -p[0], 0.0, p[0], ..., p[P-1]].  The first guess comes from log2 of the float; the loops correct it
// against the double edges (they stop at the DBL_MAX edge, which every finite value lies below).
__device__ __forceinline__ int bucket_of(float u, const double* __restrict__ lim) {
  if (u == 0.f) return kPosLimits + 1;
  const double a = fabs((double)u);
  const float lg = log2f(fabsf(u));
  int g = (int)floorf((lg + 39.863137f) * 7.2725409f) + 1;     // log2(1e12), 1 / log2(1.1)
  g = min(max(g, 0), kPosLimits - 1);
  if (u > 0.f) {               // first k with p[k] > a
    while (g > 0 && lim[g - 1] > a) --g;
    while (lim[g] <= a) ++g;
    return kPosLimits + 1 + g;
  }
  while (g > 0 && lim[g - 1] >= a) --g;     // first k with p[k] >= a
  while (lim[g] < a) ++g;
  return kPosLimits - g;
}

// LDS of one statistics work group: the limits, one sub-histogram per wave and the fold's scratch
struct StatsLds {
  double lim[kPosLimits];
  unsigned hist[kStatsWaves][JCM_HIST_BUCKETS];
  float rmn[kStatsThreads], rmx[kStatsThreads];
  double rs[kStatsThreads], rss[kStatsThreads];
  unsigned rc[3][kStatsThreads];
};

// load the limits, clear the sub-histograms (the caller synchronises before the first add)
__device__ __forceinline__ void stats_lds_init(StatsLds& L, const double* __restrict__ limits) {
  const int t = threadIdx.x;
  for (int i = t; i < kPosLimits; i += kStatsThreads) L.lim[i] = limits[i];
  for (int i = t; i < kStatsWaves * JCM_HIST_BUCKETS; i += kStatsThreads) (&L.hist[0][0])[i] = 0u;
}

// what one thread has seen
struct StatsAcc {
  float mn = INFINITY, mx = -INFINITY;
  double s = 0.0, ss = 0.0;
  unsigned num = 0, npos = 0, nnf = 0;
  __device__ __forceinline__ void add(float u, StatsLds& L) {
    if (!isfinite(u)) {
      ++nnf;
      return;
    }
    mn = fminf(mn, u);
    mx = fmaxf(mx, u);
    const double d = (double)u;
    s += d;
    ss += d * d;
    ++num;
    npos += u > 0.f;
    atomicAdd(&L.hist[threadIdx.x / 64][bucket_of(u, L.lim)], 1u);
  }
};

// fixed-order tree over the work group's threads -> *part (thread 0), then the nonzero bins of the sub-histograms -> the segment's int64 counts cs
__device__ __forceinline__ void stats_block_finish(const StatsAcc& A, StatsLds& L, Part* __restrict__ part, unsigned long long* __restrict__ cs) {
  const int t = threadIdx.x;
  L.rmn[t] = A.mn;
  L.rmx[t] = A.mx;
  L.rs[t] = A.s;
  L.rss[t] = A.ss;
  L.rc[0][t] = A.num;
  L.rc[1][t] = A.npos;
  L.rc[2][t] = A.nnf;
  for (int st = kStatsThreads / 2; st > 0; st >>= 1) {
    __syncthreads();
    if (t < st) {
      L.rmn[t] = fminf(L.rmn[t], L.rmn[t + st]);
      L.rmx[t] = fmaxf(L.rmx[t], L.rmx[t + st]);
      L.rs[t] += L.rs[t + st];
      L.rss[t] += L.rss[t + st];
      L.rc[0][t] += L.rc[0][t + st];
      L.rc[1][t] += L.rc[1][t + st];
      L.rc[2][t] += L.rc[2][t + st];
    }
  }
  __syncthreads();
  if (t == 0) {
    Part P;
    P.mn = L.rmn[0];
    P.mx = L.rmx[0];
    P.s = L.rs[0];
    P.ss = L.rss[0];
    P.num = L.rc[0][0];
    P.npos = L.rc[1][0];
    P.nnf = L.rc[2][0];
    P.pad = 0;
    *part = P;
  }
  for (int b = t; b < JCM_HIST_BUCKETS; b += kStatsThreads) {
    unsigned c = 0;
#pragma unroll
    for (int w = 0; w < kStatsWaves; ++w) c += L.hist[w][b];
    if (c) atomicAdd(cs + b, (unsigned long long)c);
  }
}

// one work group per segment: fixed-order fold of its chunks' partials -> stats [4] = (min, max, sum, sum_squares) and
// counts [0..2] = (num, n_pos, n_nonfinite).  An empty histogram keeps TF's initial min / max (DBL_MAX, -DBL_MAX).
// The chunks of segment s are parts[first[s] .. first[s + 1]), or with first == nullptr parts[s * per .. (s + 1) * per).
__global__ __launch_bounds__(kStatsThreads) void stats_fold_kernel(const Part* __restrict__ parts, const int* __restrict__ first, int per,
                                                                   double* __restrict__ stats, unsigned long long* __restrict__ counts) {
  __shared__ float rmn[kStatsThreads], rmx[kStatsThreads];
  __shared__ double rs[kStatsThreads], rss[kStatsThreads];
  __shared__ unsigned long long rc[3][kStatsThreads];
  const int t = threadIdx.x, seg = blockIdx.x;
  const int lo = first ? first[seg] : seg * per, hi = first ? first[seg + 1] : (seg + 1) * per;
  float mn = INFINITY, mx = -INFINITY;
  double s = 0.0, ss = 0.0;
  unsigned long long num = 0, npos = 0, nnf = 0;
  for (int i = lo + t; i < hi; i += kStatsThreads) {
    const Part P = parts[i];
    mn = fminf(mn, P.mn);
    mx = fmaxf(mx, P.mx);
    s += P.s;
    ss += P.ss;
    num += P.num;
    npos += P.npos;
    nnf += P.nnf;
  }
  rmn[t] = mn;
  rmx[t] = mx;
  rs[t] = s;
  rss[t] = ss;
  rc[0][t] = num;
  rc[1][t] = npos;
  rc[2][t] = nnf;
  for (int st = kStatsThreads / 2; st > 0; st >>= 1) {
    __syncthreads();
    if (t < st) {
      rmn[t] = fminf(rmn[t], rmn[t + st]);
      rmx[t] = fmaxf(rmx[t], rmx[t + st]);
      rs[t] += rs[t + st];
      rss[t] += rss[t + st];
      rc[0][t] += rc[0][t + st];
      rc[1][t] += rc[1][t + st];
      rc[2][t] += rc[2][t + st];
    }
  }
  __syncthreads();
  if (t == 0) {
    double* o = stats + (size_t)seg * 4;
    const bool any = rc[0][0] > 0;
    o[0] = any ? (double)rmn[0] : DBL_MAX;
    o[1] = any ? (double)rmx[0] : -DBL_MAX;
    o[2] = rs[0];
    o[3] = rss[0];
    unsigned long long* c = counts + (size_t)seg * (3 + JCM_HIST_BUCKETS);
    c[0] = rc[0][0];
    c[1] = rc[1][0];
    c[2] = rc[2][0];
  }
}

}  // namespace

}  // namespace jcm
