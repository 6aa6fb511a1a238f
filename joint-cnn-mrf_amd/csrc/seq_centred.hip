// Flow-centred frame sequences (include/jcm.h: jcm_seq_filter_centred / jcm_seq_viterbi_centred): the filter and Viterbi of
// sequence.hip with the whole-cell shift of the *_moving entries read PER DESTINATION CELL from centre int32 [S,T,HH,WW,2] = (sy, sx) -- cell (y, x) of
// frame t was cell (y + sy, x + sx) of frame t-1 -- instead of per frame.  All arithmetic is float64, one correctly rounded operation per step, in the
// order include/jcm.h states; a table that is uniform over a frame gives the bits of the moving scans of seq_scan.h, an all-zero one those of the plain ones.
// One work group of 1024 threads per (sequence, joint) scans the T frames of a launch with two float64 planes in LDS, as seq_scan.h does.  What differs
// is the pass: neighbouring cells no longer share a window, so the vertical and the horizontal pass become ONE pass of (2R+1)^2 reads of the belief
// plane A per cell, columns outside, rows inside, both over bounds clipped to the plane (no tap outside it is indexed, none multiplied by zero).  A frame is
//   the pass     A -> P = pred (Viterbi: e, with the source cell of every cell stored to the workspace as it is found: no byte plane of dy*)
//   stage p_t    -> A  (A is dead by then), sq_stage of seq_scan.h
//   b = p_t * P in place, the thread's share of Z (or of max b) in a register; reduction, division and arg-max as in seq_scan.h.
// A cell i belongs to thread i % 1024 in every pass, at most kScCells = 8 cells a thread.  The thread's entries of a frame's table are ONE 8-byte load
// per cell, consecutive lanes consecutive cells, and are issued a frame ahead: before the division loop of frame t-1, whose arg-max barriers they hide
// behind (before the barrier after the state's load for frame 0).  They are clamped to +-(side + R) as SqShift clamps, so that no index sum overflows.
// Lanes whose cells carry different shifts read A at addresses that are no longer consecutive: LDS bank conflicts that the moving scans do not have.
// Sharing with sequence.hip: seq_scan.h for everything but the pass, seq_backtrace for Viterbi's second launch, seq_entry.h for the entry points.
#include <string>

#include "seq_entry.h"
#include "seq_scan.h"

namespace jcm {

namespace {

constexpr int kScCells = kSeqMaxHW / kSqThreads;      // cells of the largest plane per thread
constexpr int kScLdsMax = 2 * kSeqMaxHW * 8;

// the thread's entries of one frame's table, cell tid + q * 1024 in v[q]
__device__ __forceinline__ void sc_load(const int2* __restrict__ tab, int HW, int tid, int2 (&v)[kScCells]) {
#pragma unroll
  for (int q = 0; q < kScCells; ++q) {
    const int i = tid + q * kSqThreads;
    v[q] = i < HW ? tab[i] : make_int2(0, 0);
  }
}

// m of the filter at the cell whose centre in frame t-1's lattice is (ys, xs): per column dx ascending the sum over the rows dy ascending, both from 0.0
__device__ __forceinline__ double sc_blur_sum(const double* A, const double* w, int R, int HH, int WW, int ys, int xs) {
  const int ylo = max(-R, ys - (HH - 1)), yhi = min(R, ys);
  const int xlo = max(-R, xs - (WW - 1)), xhi = min(R, xs);
  double m = 0.0;
  for (int dx = xlo; dx <= xhi; ++dx) {
    const int top = ys * WW + (xs - dx);
    double c = 0.0;                                    // no row inside the map: 0.0, and the term is added all the same
    for (int dy = ylo; dy <= yhi; ++dy) c = c + w[dy + R] * A[top - dy * WW];
    m = m + w[dx + R] * c;
  }
  return m;
}

// m of Viterbi there and its source cell (of frame t-1's lattice; any value when m is not above 0): ascending scans, a strictly greater value replaces,
// the maximum over no row is 0, over no column -1
__device__ __forceinline__ double sc_blur_max(const double* D, const double* w, int R, int HH, int WW, int ys, int xs, int& from) {
  const int ylo = max(-R, ys - (HH - 1)), yhi = min(R, ys);
  const int xlo = max(-R, xs - (WW - 1)), xhi = min(R, xs);
  double best = -1.0;
  from = 0;
  for (int dx = xlo; dx <= xhi; ++dx) {
    const int top = ys * WW + (xs - dx);
    double c = -1.0;
    int src = top;
    for (int dy = ylo; dy <= yhi; ++dy) {
      const double v = w[dy + R] * D[top - dy * WW];
      if (v > c) { c = v; src = top - dy * WW; }
    }
    if (ylo > yhi) c = 0.0;
    const double v = w[dx + R] * c;
    if (v > best) { best = v; from = src; }
  }
  return best;
}

__global__ __launch_bounds__(kSqThreads) void seq_filter_centred_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps,
                                                                        int R, double om, double u, const int32_t* __restrict__ centre,
                                                                        const double* __restrict__ state_in, float* __restrict__ filtered,
                                                                        int32_t* __restrict__ coords, double* __restrict__ norm, int32_t* __restrict__ reset,
                                                                        double* __restrict__ state_out, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // A [HW], P [HW]
  __shared__ double w[kSqTaps];
  __shared__ double rd[kSqWaves];
  __shared__ int ri[kSqWaves];
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  const int tid = threadIdx.x;
  const int HW = HH * WW, n = HW * K;
  double* A = sq_planes;
  double* P = sq_planes + HW;
  const int2* tab = reinterpret_cast<const int2*>(centre) + (size_t)s * T * HW;      // [T][HW] of the group's sequence
  const SqPlain::Frame ex;
  int2 cv[kScCells];
  if (tid < 2 * R + 1) w[tid] = taps[k * (2 * R + 1) + tid];
  const size_t plane0 = ((size_t)s * K + k) * HW;
  bool prev = state_in != nullptr;
  if (prev) {
    sc_load(tab, HW, tid, cv);
    for (int i = tid; i < HW; i += kSqThreads) A[i] = state_in[plane0 + i];
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const size_t ft = (size_t)s * T + t;
    const float* src = hm + ft * n;
    int rs = 0;
    double Z = 0.0;
    if (prev) {
#pragma unroll
      for (int q = 0; q < kScCells; ++q) {
        const int i = tid + q * kSqThreads;
        if (i >= HW) break;
        const int y = i / WW, x = i - y * WW;
        const int sy = min(max(cv[q].x, -(HH + R)), HH + R), sx = min(max(cv[q].y, -(WW + R)), WW + R);
        const double m = sc_blur_sum(A, w, R, HH, WW, y + sy, x + sx);
        P[i] = om * m + u;
      }
      __syncthreads();
      sq_stage(src, n, K, k, vec != 0, A, tid, ex);
      __syncthreads();
      double zp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) {
        const double b = A[i] * P[i];
        A[i] = b;
        zp = zp + b;
      }
      Z = sq_block_sum(zp, rd, tid);
      if (!(Z > 0.0 && Z <= 1.79769313486231570815e308)) rs = 1;      // 0 or not finite (negative values and NaN are outside the contract)
    }
    if (!prev || rs == 1) {      // b = p_t  (thread-uniform: Z is)
      sq_stage(src, n, K, k, vec != 0, A, tid, ex);
      __syncthreads();
      double zp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) zp = zp + A[i];
      Z = sq_block_sum(zp, rd, tid);
      if (Z == 0.0) rs = 2;
    }
    if (t + 1 < T) sc_load(tab + (size_t)(t + 1) * HW, HW, tid, cv);      // the next frame's table, in flight over the division and the arg-max
    const double uni = 1.0 / (double)HW;
    double bv = -1.0;
    int bi = kSqNone;
    for (int i = tid; i < HW; i += kSqThreads) {
      const double a = rs == 2 ? uni : A[i] / Z;
      A[i] = a;
      if (a > bv) { bv = a; bi = i; }
      if (filtered) filtered[(ft * HW + i) * K + k] = (float)a;
    }
    sq_block_argmax(bv, bi, rd, ri, tid);      // its barriers also order this frame's A against the next pass
    if (tid == 0) {
      const int r = bi / WW;
      coords[(ft * 2 + 0) * K + k] = r;
      coords[(ft * 2 + 1) * K + k] = bi - r * WW;
      if (norm) norm[ft * K + k] = Z;
      if (reset) reset[ft * K + k] = rs;
    }
    prev = true;
  }
  if (state_out)
    for (int i = tid; i < HW; i += kSqThreads) state_out[plane0 + i] = A[i];
}

__global__ __launch_bounds__(kSqThreads) void seq_viterbi_centred_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps,
                                                                         int R, double om, double u, const int32_t* __restrict__ centre,
                                                                         int16_t* __restrict__ bp, int32_t* __restrict__ amax, double* __restrict__ maxes,
                                                                         int32_t* __restrict__ breaks, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // D [HW], P [HW]
  __shared__ double w[kSqTaps];
  __shared__ double rd[kSqWaves];
  __shared__ int ri[kSqWaves];
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  const int tid = threadIdx.x;
  const int HW = HH * WW, n = HW * K;
  double* D = sq_planes;
  double* P = sq_planes + HW;
  const int2* tab = reinterpret_cast<const int2*>(centre) + (size_t)s * T * HW;
  const SqPlain::Frame ex;
  int2 cv[kScCells];
  if (tid < 2 * R + 1) w[tid] = taps[k * (2 * R + 1) + tid];
  __syncthreads();
  int16_t* bpg = bp + (size_t)blockIdx.x * T * HW;
  double Dmax = 0.0;      // max and first-occurrence arg-max of d_{t-1}
  int Darg = 0;

  for (int t = 0; t < T; ++t) {
    const size_t ft = (size_t)s * T + t;
    const float* src = hm + ft * n;
    int16_t* bpt = bpg + (size_t)t * HW;
    int brk = 0;
    double M = 0.0;
    if (t > 0) {
      const double jump = u * Dmax;
#pragma unroll
      for (int q = 0; q < kScCells; ++q) {
        const int i = tid + q * kSqThreads;
        if (i >= HW) break;
        const int y = i / WW, x = i - y * WW;
        const int sy = min(max(cv[q].x, -(HH + R)), HH + R), sx = min(max(cv[q].y, -(WW + R)), WW + R);
        int from;
        double best = sc_blur_max(D, w, R, HH, WW, y + sy, x + sx, from);
        if (!(best > 0.0)) { best = 0.0; from = Darg; }      // m = 0 has no source inside the map: b is 0 unless the jump wins
        double e = om * best;
        if (jump > e) { e = jump; from = Darg; }
        P[i] = e;
        bpt[i] = (int16_t)from;
      }
      __syncthreads();
      sq_stage(src, n, K, k, vec != 0, D, tid, ex);
      __syncthreads();
      double mp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) {
        const double b = D[i] * P[i];
        D[i] = b;
        mp = fmax(mp, b);
      }
      int none = kSqNone;
      sq_block_argmax(mp, none, rd, ri, tid);
      M = mp;
      if (M == 0.0) brk = 1;
    }
    if (t == 0 || brk == 1) {      // b = p_t  (thread-uniform: M is)
      sq_stage(src, n, K, k, vec != 0, D, tid, ex);
      __syncthreads();
      double mp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) {
        mp = fmax(mp, D[i]);
        bpt[i] = -1;
      }
      int none = kSqNone;
      sq_block_argmax(mp, none, rd, ri, tid);
      M = mp;
      if (M == 0.0) brk = 2;
    }
    if (t + 1 < T) sc_load(tab + (size_t)(t + 1) * HW, HW, tid, cv);      // the next frame's table, in flight over the division and the arg-max
    double bv = -1.0;
    int bi = kSqNone;
    for (int i = tid; i < HW; i += kSqThreads) {
      const double d = brk == 2 ? 1.0 : D[i] / M;
      D[i] = d;
      if (d > bv) { bv = d; bi = i; }
    }
    sq_block_argmax(bv, bi, rd, ri, tid);
    Dmax = bv;
    Darg = bi;
    if (tid == 0) {
      amax[(size_t)blockIdx.x * T + t] = bi;
      if (maxes) maxes[ft * K + k] = M;
      if (breaks) breaks[ft * K + k] = brk;
    }
  }
}

}  // namespace


hipError_t seq_filter_centred(const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double om, double u, const int32_t* centre,
                              const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out, hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, K, R) || !centre) return hipErrorInvalidValue;
  const int HW = HH * WW;
  static LdsAttr attr;
  if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(seq_filter_centred_kernel), kScLdsMax); e != hipSuccess) return e;
  hipLaunchKernelGGL(seq_filter_centred_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8, st, hm, T, HH, WW, K, taps, R, om, u, centre, state_in, filtered,
                     coords, norm, reset, state_out, sq_vec(hm, HW, K) ? 1 : 0);
  return hipGetLastError();
}

hipError_t seq_viterbi_centred(const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double om, double u, const int32_t* centre,
                               int16_t* bp, int32_t* amax, int32_t* path, double* maxes, int32_t* breaks, hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, K, R) || !centre) return hipErrorInvalidValue;
  const int HW = HH * WW;
  static LdsAttr attr;
  if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(seq_viterbi_centred_kernel), kScLdsMax); e != hipSuccess) return e;
  hipLaunchKernelGGL(seq_viterbi_centred_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8, st, hm, T, HH, WW, K, taps, R, om, u, centre, bp, amax, maxes,
                     breaks, sq_vec(hm, HW, K) ? 1 : 0);
  return seq_backtrace(bp, amax, S, T, HW, WW, K, path, st);
}

}  // namespace jcm

using namespace jcm;

namespace {

constexpr const char* kScPlanes = "two float64 planes";      // what these scans keep in LDS; the map limit is that of the scans of seq_scan.h all the same

// what both entries ask of the table: it is there, and it can be read as one 8-byte load per cell
int centre_check(const std::string& w, const int32_t* centre) {
  if (!centre) return fail(JCM_ERR_ARG, w + ": null pointer (centre is required)");
  if (reinterpret_cast<uintptr_t>(centre) % 8 != 0) return fail(JCM_ERR_ARG, w + ": centre must be aligned to 8 bytes (a cell's pair is one load)");
  return JCM_OK;
}

}  // namespace

extern "C" {

int jcm_seq_filter_centred(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, const int32_t* centre,
                           const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out) {
  const std::string w("seq_filter_centred");
  JCM_TRY(check(h, false));
  JCM_TRY(seq_check_joints(w, hm, S, T, HH, WW, K, taps, R, rho, kSeqMaxHW, kScPlanes));
  if (!coords) return fail(JCM_ERR_ARG, w + ": null pointer (coords is required; state_in, filtered, norm, reset and state_out may be NULL)");
  JCM_TRY(centre_check(w, centre));
  DeviceGuard g(h->device);
  CallOrder order(h);
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  return seq_launch(h, w, taps, K * (2 * R + 1), [] {}, [&](const double* dtaps) {
    return seq_filter_centred(hm, S, T, HH, WW, K, dtaps, R, om, u, centre, state_in, filtered, coords, norm, reset, state_out, h->stream);
  });
}

int jcm_seq_viterbi_centred(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, const int32_t* centre,
                            int32_t* path, double* maxes, int32_t* breaks) {
  const std::string w("seq_viterbi_centred");
  JCM_TRY(check(h, false));
  JCM_TRY(seq_check_joints(w, hm, S, T, HH, WW, K, taps, R, rho, kSeqMaxHW, kScPlanes));
  if (!path) return fail(JCM_ERR_ARG, w + ": null pointer (path is required; maxes and breaks may be NULL)");
  JCM_TRY(centre_check(w, centre));
  DeviceGuard g(h->device);
  CallOrder order(h);
  // the back-pointers of jcm_seq_viterbi: one int16 per (sequence, joint, frame, cell), refused the same way when they cannot fit
  JCM_TRY(workspace_or_refuse(h, w, (double)S * K * T * HH * WW * 2.0 + (double)S * K * T * 4.0 + 8192.0, "back-pointers", S, T));
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  int16_t* bp = nullptr;
  int32_t* amax = nullptr;
  return seq_launch(h, w, taps, K * (2 * R + 1), [&] {
    bp = arena_alloc<int16_t>(h, (size_t)S * K * T * HH * WW);
    amax = arena_alloc<int32_t>(h, (size_t)S * K * T);
  }, [&](const double* dtaps) {
    return seq_viterbi_centred(hm, S, T, HH, WW, K, dtaps, R, om, u, centre, bp, amax, path, maxes, breaks, h->stream);
  });
}

}  // extern "C"
