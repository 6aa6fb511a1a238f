// Frame sequences: a temporal edge on the heat maps hm [S,T,HH,WW,K] of a clip -- the causal forward filter and the most probable track
// (Viterbi, max-product in the probability domain) of a hidden position per (sequence, joint) under a separable truncated motion kernel plus a uniform
// "anywhere" term.  All arithmetic is float64, one correctly rounded operation per step, in the order include/jcm.h states.
// One work group per (sequence, joint) scans the T frames of a launch; the scan itself -- planes, staging, reductions, back-pointers -- is seq_scan.h,
// which seq_tracks.hip shares.  Here: its kernels on the map as it is (SqPlain), the backtrace launch, the tap upload and the entry points.
// The *_moving kernels are the same scans with SqShift: every frame's lattice lies a whole number of cells from the one before.
// seq_centred.hip (a shift per cell) has a pass of its own and shares the backtrace launch, seq_backtrace.
#include <string>

#include "seq_entry.h"
#include "seq_scan.h"

namespace jcm {

namespace {

constexpr int kSqPut = 480;                          // doubles per upload launch: 3840 bytes of its 4096 bytes of arguments

struct SeqPut {
  double v[kSqPut];
};
__global__ __launch_bounds__(256) void seq_put_kernel(SeqPut p, int n, double* __restrict__ dst) {
  for (int i = threadIdx.x; i < n; i += 256) dst[i] = p.v[i];
}

__global__ __launch_bounds__(kSqThreads) void seq_filter_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps, int R,
                                                                double om, double u, const double* __restrict__ state_in, float* __restrict__ filtered,
                                                                int32_t* __restrict__ coords, double* __restrict__ norm, int32_t* __restrict__ reset,
                                                                double* __restrict__ state_out, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // A [HW], C [HW]
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  sq_filter_scan(sq_planes, hm, T, HH, WW, K, taps, R, om, u, state_in, filtered, coords, norm, reset, state_out, vec, s, s, k, SqPlain());
}

__global__ __launch_bounds__(kSqThreads) void seq_viterbi_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps, int R,
                                                                 double om, double u, int16_t* __restrict__ bp, int32_t* __restrict__ amax,
                                                                 double* __restrict__ maxes, int32_t* __restrict__ breaks, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // D [HW], C [HW], dy* [HW] bytes
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  sq_viterbi_scan(sq_planes, hm, T, HH, WW, K, taps, R, om, u, bp, amax, maxes, breaks, vec, s, s, k, (int)blockIdx.x, SqPlain());
}

__global__ __launch_bounds__(kSqThreads) void seq_filter_moving_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps,
                                                                       int R, double om, double u, const int32_t* __restrict__ shift,
                                                                       const double* __restrict__ state_in, float* __restrict__ filtered,
                                                                       int32_t* __restrict__ coords, double* __restrict__ norm, int32_t* __restrict__ reset,
                                                                       double* __restrict__ state_out, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // A [HW], C [HW]
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  sq_filter_scan(sq_planes, hm, T, HH, WW, K, taps, R, om, u, state_in, filtered, coords, norm, reset, state_out, vec, s, s, k, SqPlain(), nullptr,
                 SqShift{shift + (size_t)s * T * 2});
}

__global__ __launch_bounds__(kSqThreads) void seq_viterbi_moving_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps,
                                                                        int R, double om, double u, const int32_t* __restrict__ shift, int16_t* __restrict__ bp,
                                                                        int32_t* __restrict__ amax, double* __restrict__ maxes, int32_t* __restrict__ breaks,
                                                                        int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // D [HW], C [HW], dy* [HW] bytes
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  sq_viterbi_scan(sq_planes, hm, T, HH, WW, K, taps, R, om, u, bp, amax, maxes, breaks, vec, s, s, k, (int)blockIdx.x, SqPlain(),
                  SqShift{shift + (size_t)s * T * 2});
}

// one lane per (sequence, joint)
__global__ __launch_bounds__(64) void seq_backtrace_kernel(const int16_t* __restrict__ bp, const int32_t* __restrict__ amax, int G, int T, int HW, int WW, int K,
                                                           int32_t* __restrict__ path) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= G) return;
  const int s = g / K, k = g - s * K;
  sq_walk_back(bp + (size_t)g * T * HW, amax + (size_t)g * T, T, HW, [&](int t, int cell) {
    const size_t ft = (size_t)s * T + t;
    const int r = cell / WW;
    path[(ft * 2 + 0) * K + k] = r;
    path[(ft * 2 + 1) * K + k] = cell - r * WW;
  });
}

}  // namespace


hipError_t seq_put_taps(const double* taps_host, int n, double* taps_dev, hipStream_t st) {
  for (int i0 = 0; i0 < n; i0 += kSqPut) {
    SeqPut p;
    const int m = std::min(kSqPut, n - i0);
    for (int i = 0; i < kSqPut; ++i) p.v[i] = i < m ? taps_host[i0 + i] : 0.0;
    hipLaunchKernelGGL(seq_put_kernel, dim3(1), dim3(256), 0, st, p, m, taps_dev + i0);
  }
  return hipGetLastError();
}

hipError_t seq_backtrace(const int16_t* bp, const int32_t* amax, int S, int T, int HW, int WW, int K, int32_t* path, hipStream_t st) {
  const int G = S * K;
  hipLaunchKernelGGL(seq_backtrace_kernel, dim3((G + 63) / 64), dim3(64), 0, st, bp, amax, G, T, HW, WW, K, path);
  return hipGetLastError();
}

hipError_t seq_filter(const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double om, double u, const int32_t* shift,
                      const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out, hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, K, R)) return hipErrorInvalidValue;
  const int HW = HH * WW;
  if (shift) {
    static LdsAttr attr;
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(seq_filter_moving_kernel), kSqLdsMax); e != hipSuccess) return e;
    hipLaunchKernelGGL(seq_filter_moving_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8, st, hm, T, HH, WW, K, taps, R, om, u, shift, state_in, filtered,
                       coords, norm, reset, state_out, sq_vec(hm, HW, K) ? 1 : 0);
    return hipGetLastError();
  }
  static LdsAttr attr;
  if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(seq_filter_kernel), kSqLdsMax); e != hipSuccess) return e;
  hipLaunchKernelGGL(seq_filter_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8, st, hm, T, HH, WW, K, taps, R, om, u, state_in, filtered, coords, norm,
                     reset, state_out, sq_vec(hm, HW, K) ? 1 : 0);
  return hipGetLastError();
}

hipError_t seq_viterbi(const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double om, double u, const int32_t* shift,
                       int16_t* bp, int32_t* amax, int32_t* path, double* maxes, int32_t* breaks, hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, K, R)) return hipErrorInvalidValue;
  const int HW = HH * WW;
  if (shift) {
    static LdsAttr attr;
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(seq_viterbi_moving_kernel), kSqLdsMax); e != hipSuccess) return e;
    hipLaunchKernelGGL(seq_viterbi_moving_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8 + ((HW + 7) & ~7), st, hm, T, HH, WW, K, taps, R, om, u, shift, bp,
                       amax, maxes, breaks, sq_vec(hm, HW, K) ? 1 : 0);
  } else {
    static LdsAttr attr;
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(seq_viterbi_kernel), kSqLdsMax); e != hipSuccess) return e;
    hipLaunchKernelGGL(seq_viterbi_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8 + ((HW + 7) & ~7), st, hm, T, HH, WW, K, taps, R, om, u, bp, amax, maxes,
                       breaks, sq_vec(hm, HW, K) ? 1 : 0);
  }
  return seq_backtrace(bp, amax, S, T, HW, WW, K, path, st);
}

}  // namespace jcm

using namespace jcm;

namespace {

// The two filter entries and the two Viterbi entries are one body each: `moving` says whether a shift is required, `what` names the entry point.
int seq_filter_entry(const char* what, bool moving, jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                     const int32_t* shift, const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out) {
  const std::string w(what);
  JCM_TRY(check(h, false));
  JCM_TRY(seq_check_joints(w, hm, S, T, HH, WW, K, taps, R, rho, kSeqMaxHW, kSeqScanPlanes));
  if (!coords) return fail(JCM_ERR_ARG, w + ": null pointer (coords is required; state_in, filtered, norm, reset and state_out may be NULL)");
  if (moving && !shift) return fail(JCM_ERR_ARG, w + ": null pointer (shift is required)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  return seq_launch(h, w, taps, K * (2 * R + 1), [] {}, [&](const double* dtaps) {
    return seq_filter(hm, S, T, HH, WW, K, dtaps, R, om, u, moving ? shift : nullptr, state_in, filtered, coords, norm, reset, state_out, h->stream);
  });
}

int seq_viterbi_entry(const char* what, bool moving, jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R,
                      double rho, const int32_t* shift, int32_t* path, double* maxes, int32_t* breaks) {
  const std::string w(what);
  JCM_TRY(check(h, false));
  JCM_TRY(seq_check_joints(w, hm, S, T, HH, WW, K, taps, R, rho, kSeqMaxHW, kSeqScanPlanes));
  if (!path) return fail(JCM_ERR_ARG, w + ": null pointer (path is required; maxes and breaks may be NULL)");
  if (moving && !shift) return fail(JCM_ERR_ARG, w + ": null pointer (shift is required)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  // the back-pointers: one int16 per (sequence, joint, frame, cell); the workspace grows to hold them, and a clip they cannot fit in is refused
  JCM_TRY(workspace_or_refuse(h, w, (double)S * K * T * HH * WW * 2.0 + (double)S * K * T * 4.0 + 8192.0, "back-pointers", S, T));
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  int16_t* bp = nullptr;
  int32_t* amax = nullptr;
  return seq_launch(h, w, taps, K * (2 * R + 1), [&] {
    bp = arena_alloc<int16_t>(h, (size_t)S * K * T * HH * WW);
    amax = arena_alloc<int32_t>(h, (size_t)S * K * T);
  }, [&](const double* dtaps) {
    return seq_viterbi(hm, S, T, HH, WW, K, dtaps, R, om, u, moving ? shift : nullptr, bp, amax, path, maxes, breaks, h->stream);
  });
}

}  // namespace

extern "C" {

int jcm_seq_filter(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, const double* state_in,
                   float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out) {
  return seq_filter_entry("seq_filter", false, h, hm, S, T, HH, WW, K, taps, R, rho, nullptr, state_in, filtered, coords, norm, reset, state_out);
}

int jcm_seq_viterbi(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, int32_t* path,
                    double* maxes, int32_t* breaks) {
  return seq_viterbi_entry("seq_viterbi", false, h, hm, S, T, HH, WW, K, taps, R, rho, nullptr, path, maxes, breaks);
}

int jcm_seq_filter_moving(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, const int32_t* shift,
                          const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out) {
  return seq_filter_entry("seq_filter_moving", true, h, hm, S, T, HH, WW, K, taps, R, rho, shift, state_in, filtered, coords, norm, reset, state_out);
}

int jcm_seq_viterbi_moving(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                           const int32_t* shift, int32_t* path, double* maxes, int32_t* breaks) {
  return seq_viterbi_entry("seq_viterbi_moving", true, h, hm, S, T, HH, WW, K, taps, R, rho, shift, path, maxes, breaks);
}

}  // extern "C"
