// Several torso tracks through the single-channel maps hm [S,T,HH,WW] of a clip (include/jcm.h: jcm_seq_tracks_viterbi /
// jcm_seq_tracks_filter): M successive passes of the temporal model of sequence.hip.  Pass n runs the scan of seq_scan.h -- the one copy of the
// recurrence -- at K = 1 on an observation in which the (2D+1)^2 neighbourhood of every earlier track's cell is zero, frame by frame.
// The exclusion happens while p_t is staged into the LDS plane (SqTracks::Frame): no masked copy of the maps exists in memory.  The at most three
// earlier cells of a frame and their values are read once per frame at addresses that depend on (clip, pass, frame) only: uniform over the wave.
// One work group per clip and pass; the passes of a call follow each other in stream order -- pass n reads the cells pass n - 1 wrote across the
// kernel boundary -- and Viterbi's back-pointer workspace [S][T][HW] is the same for every pass: its backtrace has run before the next scan starts.
#include <string>

#include "seq_entry.h"
#include "seq_scan.h"

namespace jcm {

namespace {

constexpr int kTrMaxM = 4;
constexpr int kTrMaxD = 64;
constexpr int kTrFar = -(1 << 20);

// The observation of pass n of clip s: cells / value are the outputs [S,M,T,2] / [S,M,T] of the call, of which the rows m < n are complete.
struct SqTracks {
  const int32_t* cells;
  const float* value;
  float* value_out;
  int s, n, M, T, D, WW;

  // cy / cx: one fixed slot per possible earlier track (no indexing by a run-time count, so the slots stay in registers); a slot that excludes
  // nothing holds kTrFar, farther than D from every row of a map
  struct Frame {
    int cy[kTrMaxM - 1], cx[kTrMaxM - 1], D, WW;
    bool any;
    __device__ __forceinline__ double operator()(int p, double v) const {
      if (!any) return v;
      const int y = p / WW, x = p - y * WW;
      bool out = false;
#pragma unroll
      for (int m = 0; m < kTrMaxM - 1; ++m) out = out || (abs(y - cy[m]) <= D && abs(x - cx[m]) <= D);
      return out ? 0.0 : v;
    }
  };
  // an earlier track excludes in frame t only where it has support itself (value > 0)
  __device__ __forceinline__ Frame frame(int t) const {
    Frame f;
    f.D = D;
    f.WW = WW;
    f.any = false;
#pragma unroll
    for (int m = 0; m < kTrMaxM - 1; ++m) {
      f.cy[m] = f.cx[m] = kTrFar;
      if (m < n) {
        const size_t ft = ((size_t)s * M + m) * T + t;
        if (value[ft] > 0.0f) {
          f.cy[m] = cells[ft * 2 + 0];
          f.cx[m] = cells[ft * 2 + 1];
          f.any = true;
        }
      }
    }
    return f;
  }
  // value = the pass's observation at the track's cell
  __device__ __forceinline__ void emit(const Frame& ex, size_t ft, int cell, const float* src) const { value_out[ft] = (float)ex(cell, (double)src[cell]); }
};

__global__ __launch_bounds__(kSqThreads) void tracks_filter_kernel(const float* __restrict__ hm, int T, int HH, int WW, const double* __restrict__ taps, int R,
                                                                   double om, double u, const double* __restrict__ state_in, float* __restrict__ filtered,
                                                                   int32_t* coords, double* __restrict__ norm, int32_t* __restrict__ reset,
                                                                   double* __restrict__ state_out, float* value, int M, int n, int D, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // A [HW], C [HW]
  const int s = blockIdx.x;
  const SqTracks tr{coords, value, value, s, n, M, T, D, WW};
  sq_filter_scan(sq_planes, hm, T, HH, WW, 1, taps, R, om, u, state_in, filtered, coords, norm, reset, state_out, vec, s, s * M + n, 0, tr);
}

__global__ __launch_bounds__(kSqThreads) void tracks_viterbi_kernel(const float* __restrict__ hm, int T, int HH, int WW, const double* __restrict__ taps, int R,
                                                                    double om, double u, int16_t* __restrict__ bp, int32_t* __restrict__ amax,
                                                                    double* __restrict__ maxes, int32_t* __restrict__ breaks, const int32_t* path,
                                                                    const float* value, int M, int n, int D, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // D [HW], C [HW], dy* [HW] bytes
  const int s = blockIdx.x;
  const SqTracks tr{path, value, nullptr, s, n, M, T, D, WW};
  sq_viterbi_scan(sq_planes, hm, T, HH, WW, 1, taps, R, om, u, bp, amax, maxes, breaks, vec, s, s * M + n, 0, s, tr);
}

// one lane per clip: the walk of sequence.hip's backtrace, which also reads the pass's observation at every cell it visits
__global__ __launch_bounds__(64) void tracks_backtrace_kernel(const float* __restrict__ hm, const int16_t* __restrict__ bp, const int32_t* __restrict__ amax, int S,
                                                              int T, int HW, int WW, int32_t* path, float* value, int M, int n, int D) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const SqTracks tr{path, value, value, s, n, M, T, D, WW};
  sq_walk_back(bp + (size_t)s * T * HW, amax + (size_t)s * T, T, HW, [&](int t, int cell) {
    const size_t ft = ((size_t)s * M + n) * T + t;
    const int r = cell / WW;
    path[ft * 2 + 0] = r;
    path[ft * 2 + 1] = cell - r * WW;
    tr.emit(tr.frame(t), ft, cell, hm + ((size_t)s * T + t) * HW);
  });
}

}  // namespace

hipError_t seq_tracks_filter(const float* hm, int S, int T, int HH, int WW, int M, const double* taps, int R, double om, double u, int D,
                             const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out, float* value,
                             hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, 1, R) || M < 1 || M > kTrMaxM || D < 0 || D > kTrMaxD) return hipErrorInvalidValue;
  const int HW = HH * WW;
  static LdsAttr attr;
  if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(tracks_filter_kernel), kSqLdsMax); e != hipSuccess) return e;
  for (int n = 0; n < M; ++n)
    hipLaunchKernelGGL(tracks_filter_kernel, dim3(S), dim3(kSqThreads), 2 * HW * 8, st, hm, T, HH, WW, taps, R, om, u, state_in, filtered, coords, norm, reset,
                       state_out, value, M, n, D, sq_vec(hm, HW, 1) ? 1 : 0);
  return hipGetLastError();
}

hipError_t seq_tracks_viterbi(const float* hm, int S, int T, int HH, int WW, int M, const double* taps, int R, double om, double u, int D, int16_t* bp,
                              int32_t* amax, int32_t* path, double* maxes, int32_t* breaks, float* value, hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, 1, R) || M < 1 || M > kTrMaxM || D < 0 || D > kTrMaxD) return hipErrorInvalidValue;
  const int HW = HH * WW;
  static LdsAttr attr;
  if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(tracks_viterbi_kernel), kSqLdsMax); e != hipSuccess) return e;
  for (int n = 0; n < M; ++n) {
    hipLaunchKernelGGL(tracks_viterbi_kernel, dim3(S), dim3(kSqThreads), 2 * HW * 8 + ((HW + 7) & ~7), st, hm, T, HH, WW, taps, R, om, u, bp, amax, maxes, breaks,
                       path, value, M, n, D, sq_vec(hm, HW, 1) ? 1 : 0);
    hipLaunchKernelGGL(tracks_backtrace_kernel, dim3((S + 63) / 64), dim3(64), 0, st, hm, bp, amax, S, T, HW, WW, path, value, M, n, D);
  }
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

namespace {

// the argument rules the two entry points share: those of jcm_seq_* on single-channel maps, with M and D in the place of K
int tracks_check(const std::string& w, const float* hm, int S, int T, int HH, int WW, int M, const double* taps, int R, double rho, int D) {
  return seq_check(w, hm, S, T, HH, WW, taps, R, rho, "S, T, HH, WW", true, [&] {
    if (M < 1 || M > kTrMaxM) return fail(JCM_ERR_ARG, w + ": M = " + std::to_string(M) + " tracks; 1 <= M <= 4");
    if (D < 0 || D > kTrMaxD) return fail(JCM_ERR_ARG, w + ": D = " + std::to_string(D) + "; 0 <= D <= 64");
    return (int)JCM_OK;
  }, kSeqMaxHW, kSeqScanPlanes, kTrMaxM, "4");
}

}  // namespace

extern "C" {

int jcm_seq_tracks_filter(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int M, const double* taps, int R, double rho, int D,
                          const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out, float* value) {
  const std::string w("seq_tracks_filter");
  JCM_TRY(check(h, false));
  JCM_TRY(tracks_check(w, hm, S, T, HH, WW, M, taps, R, rho, D));
  if (!coords || !value)
    return fail(JCM_ERR_ARG, w + ": null pointer (coords and value are required; state_in, filtered, norm, reset and state_out may be NULL)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  return seq_launch(h, w, taps, 2 * R + 1, [] {}, [&](const double* dtaps) {
    return seq_tracks_filter(hm, S, T, HH, WW, M, dtaps, R, om, u, D, state_in, filtered, coords, norm, reset, state_out, value, h->stream);
  });
}

int jcm_seq_tracks_viterbi(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int M, const double* taps, int R, double rho, int D,
                           int32_t* path, double* maxes, int32_t* breaks, float* value) {
  const std::string w("seq_tracks_viterbi");
  JCM_TRY(check(h, false));
  JCM_TRY(tracks_check(w, hm, S, T, HH, WW, M, taps, R, rho, D));
  if (!path || !value) return fail(JCM_ERR_ARG, w + ": null pointer (path and value are required; maxes and breaks may be NULL)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  // the back-pointers of ONE pass, int16 per (clip, frame, cell): every pass writes them anew after the backtrace of the pass before it
  JCM_TRY(workspace_or_refuse(h, w, (double)S * T * HH * WW * 2.0 + (double)S * T * 4.0 + 8192.0, "back-pointers", S, T));
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  int16_t* bp = nullptr;
  int32_t* amax = nullptr;
  return seq_launch(h, w, taps, 2 * R + 1, [&] {
    bp = arena_alloc<int16_t>(h, (size_t)S * T * HH * WW);
    amax = arena_alloc<int32_t>(h, (size_t)S * T);
  }, [&](const double* dtaps) {
    return seq_tracks_viterbi(hm, S, T, HH, WW, M, dtaps, R, om, u, D, bp, amax, path, maxes, breaks, value, h->stream);
  });
}

}  // extern "C"
