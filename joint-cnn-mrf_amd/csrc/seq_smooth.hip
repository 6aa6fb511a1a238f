// Frame sequences, offline: the smoothed posterior P(x_t | all T frames) of the hidden position of every (sequence, joint) and the
// expected transition statistics that re-estimate sigma and rho (Baum-Welch; the M-step is host code, predict.seq_fit).  All arithmetic is float64, one
// correctly rounded operation per step, in the order include/jcm.h states; no atomics.
// Two launches, one work group per (sequence, joint) each.  The forward launch is the filter's scan itself (seq_scan.h: sq_filter_scan), which here also
// writes every a_t as float64 [S*K][T][HW] to the workspace.  The backward launch keeps three float64 planes in LDS for all T frames:
//   B   beta_t, then q = p_t * beta_t (staged in place, the staging of the filter with a functor), then beta_{t-1}
//   C   g = a_t * beta_t until gamma_t is out; then the vertical pass of q with the taps w
//   C2  the vertical pass of q with w2[j] = (j - R)^2 w[j]
// The passes use the ADJOINT index of the filter's (q(y + dy, x), c(y, x + dx)): beta_{t-1}(x') sums over where the position goes, not where it came
// from.  Consecutive lanes read consecutive cells of a row dy away, as in the filter's vertical pass: conflict-free ds_read_b64.  A cell i belongs to
// thread i % 1024 in every pass that writes it, so a plane is only read across threads between barriers; every sum is sq_block_sum's.
// The fixed-lag form (jcm_seq_smooth_lag) is the same two steps on a window the caller holds: the scan over the window's new frames from the
// last pending belief, then one work group per (sequence, joint, emitted frame) that runs the same backward step from L frames ahead down to its frame.
#include <string>

#include "seq_entry.h"
#include "seq_scan.h"

namespace jcm {

namespace {

constexpr int kSmLdsMax = 3 * kSeqSmoothMaxHW * 8;

// The staging functor of q = p_t * beta_t: the plane holds beta_t where the widened p_t arrives.  It reads the very plane sq_stage writes through its
// `__restrict__ plane`, which holds only because of how sq_stage visits a plane: every cell is read exactly once, by the thread that then stores it, as an
// operand of that store, and no cell is read or written a second time within the call.  A change to sq_stage that touches a cell twice (a prefetch of
// plane values, a second pass) must drop the in-place use here.
struct SqTimes {
  const double* plane;
  __device__ __forceinline__ double operator()(int p, double v) const { return v * plane[p]; }
};

__global__ __launch_bounds__(kSqThreads) void seq_smooth_fwd_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps,
                                                                    int R, double om, double u, int32_t* __restrict__ coords, double* __restrict__ norm,
                                                                    int32_t* __restrict__ reset, double* __restrict__ belief, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // A [HW], C [HW]
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  // the scan needs a coords buffer: the caller's holds the FILTER's arg-max until the backward launch, next on the stream, overwrites every entry
  sq_filter_scan(sq_planes, hm, T, HH, WW, K, taps, R, om, u, nullptr, nullptr, coords, norm, reset, nullptr, vec, s, s, k, SqPlain(),
                 belief + (size_t)blockIdx.x * T * HH * WW);
}

// The backward pass of one (sequence, joint), the ONE copy of its step (seq_smooth_bwd_kernel and seq_smooth_lag_bwd_kernel call it): beta = 1 at
// frame t_start, then frames t_start down to t_end as include/jcm.h states them.  Frames above t_write only carry beta down (their G test and their
// reset still apply); frames t_write .. t_end write their outputs.  ag: the group's beliefs [.][HW] from the sequence's frame 0;  fin: the index of that
// frame in hm, norm and reset;  fout: the index frame 0 would have in the outputs.  The transition below t_end is not taken.  trans may be NULL.
__device__ __forceinline__ void sq_smooth_back(double* sq_planes, const float* __restrict__ hm, int HH, int WW, int K, const double* __restrict__ taps, int R,
                                               double om, double u, const double* __restrict__ ag, const double* __restrict__ norm,
                                               const int32_t* __restrict__ reset, size_t fin, size_t fout, int k, int t_start, int t_end, int t_write,
                                               float* __restrict__ smoothed, int32_t* __restrict__ coords, float* __restrict__ conf, double* __restrict__ mass,
                                               int32_t* __restrict__ cut, double* __restrict__ trans, int vec) {
  __shared__ double w[kSqTaps];
  __shared__ double w2[kSqTaps];
  __shared__ double rd[kSqWaves];
  __shared__ int ri[kSqWaves];
  const int tid = threadIdx.x;
  const int HW = HH * WW, n = HW * K;
  double* B = sq_planes;
  double* C = sq_planes + HW;
  double* C2 = sq_planes + 2 * (size_t)HW;
  if (tid < 2 * R + 1) {
    const double wv = taps[k * (2 * R + 1) + tid];
    w[tid] = wv;
    w2[tid] = (double)((tid - R) * (tid - R)) * wv;
  }
  for (int i = tid; i < HW; i += kSqThreads) B[i] = 1.0;
  __syncthreads();

  for (int t = t_start; t >= t_end; --t) {
    const size_t ft = fin + t, fo = fout + t;
    const bool wr = t <= t_write;      // thread-uniform
    const double* at = ag + (size_t)t * HW;
    double gp = 0.0;
    for (int i = tid; i < HW; i += kSqThreads) {
      const double g = at[i] * B[i];
      C[i] = g;
      gp = gp + g;
    }
    const double G = sq_block_sum(gp, rd, tid);
    const bool bad = !(G > 0.0 && G <= 1.79769313486231570815e308);      // 0 or not finite: the future is dropped (thread-uniform: G is)
    double bv = -1.0;
    int bi = kSqNone;
    for (int i = tid; i < HW; i += kSqThreads) {
      const double gam = bad ? at[i] : C[i] / G;
      if (bad) B[i] = 1.0;
      if (gam > bv) { bv = gam; bi = i; }
      if (smoothed && wr) smoothed[(fo * HW + i) * K + k] = (float)gam;
    }
    sq_block_argmax(bv, bi, rd, ri, tid);      // its barriers also order B against the staging below
    if (tid == 0 && wr) {
      bi = min(max(bi, 0), HW - 1);
      const int r = bi / WW;
      coords[(fo * 2 + 0) * K + k] = r;
      coords[(fo * 2 + 1) * K + k] = bi - r * WW;
      if (conf) conf[fo * K + k] = (float)bv;
      if (mass) mass[fo * K + k] = G;
      if (cut) cut[fo * K + k] = bad ? 1 : 0;
    }
    double tm = 0.0, tj = 0.0, ts = 0.0;
    if (t > t_end) {
      if (reset[ft * K + k] != 0) {      // frame t never saw frame t-1 (thread-uniform)
        for (int i = tid; i < HW; i += kSqThreads) B[i] = 1.0;
      } else {
        const double Z = norm[ft * K + k];
        sq_stage(hm + ft * n, n, K, k, vec != 0, B, tid, SqTimes{B});
        __syncthreads();
        double qp = 0.0;
        for (int i = tid; i < HW; i += kSqThreads) qp = qp + B[i];
        const double Q = sq_block_sum(qp, rd, tid);
        for (int i = tid; i < HW; i += kSqThreads) {
          const int y = i / WW;
          const int lo = max(-R, -y), hi = min(R, HH - 1 - y);
          double acc = 0.0, acc2 = 0.0;
          for (int dy = lo; dy <= hi; ++dy) {
            const double q = B[i + dy * WW];
            acc = acc + w[dy + R] * q;
            acc2 = acc2 + w2[dy + R] * q;
          }
          C[i] = acc;
          C2[i] = acc2;
        }
        __syncthreads();
        const double uQ = u * Q;
        const double* am = ag + (size_t)(t - 1) * HW;
        double mp = 0.0, sp = 0.0;
        for (int i = tid; i < HW; i += kSqThreads) {
          const int y = i / WW, x = i - y * WW;
          const int lo = max(-R, -x), hi = min(R, WW - 1 - x);
          double m = 0.0, sx = 0.0, sy = 0.0;
          for (int dx = lo; dx <= hi; ++dx) {
            const double c = C[i + dx], c2 = C2[i + dx];
            m = m + w[dx + R] * c;
            sx = sx + w2[dx + R] * c;
            sy = sy + w[dx + R] * c2;
          }
          const double sq = sx + sy;
          const double a = am[i];
          mp = mp + a * m;
          sp = sp + a * sq;
          B[i] = (om * m + uQ) / Z;
        }
        const double M1 = sq_block_sum(mp, rd, tid);
        const double M2 = sq_block_sum(sp, rd, tid);      // the barriers of the two sums also order B, C and C2 against the next frame
        tm = (om * M1) / Z;
        tj = uQ / Z;
        ts = (om * M2) / Z;
      }
    }
    if (trans && wr && tid == 0) {
      trans[(fo * K + k) * 3 + 0] = tm;
      trans[(fo * K + k) * 3 + 1] = tj;
      trans[(fo * K + k) * 3 + 2] = ts;
    }
  }
}

__global__ __launch_bounds__(kSqThreads) void seq_smooth_bwd_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps,
                                                                    int R, double om, double u, const double* __restrict__ belief,
                                                                    const double* __restrict__ norm, const int32_t* __restrict__ reset,
                                                                    float* __restrict__ smoothed, int32_t* __restrict__ coords, float* __restrict__ conf,
                                                                    double* __restrict__ mass, int32_t* __restrict__ cut, double* __restrict__ trans, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // B [HW], C [HW], C2 [HW]
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  const size_t f0 = (size_t)s * T;
  sq_smooth_back(sq_planes, hm, HH, WW, K, taps, R, om, u, belief + (size_t)blockIdx.x * T * HH * WW, norm, reset, f0, f0, k, T - 1, 0, T - 1, smoothed, coords,
                 conf, mass, cut, trans, vec);
}

// The fixed-lag smoother.  Forward: the filter's scan over the new frames P .. W-1 of the window, from the belief of frame P-1 that an
// earlier call left in `belief`.  The scan indexes one sequence's frames from 0, so it is given sequence 0 of pointers that start at the group's frame
// P; its state plane is read at (joint k) * HW of state_in, hence the k * HW taken off the address of frame P-1.  coords: scratch [S][W-P][2][K].
__global__ __launch_bounds__(kSqThreads) void seq_smooth_lag_fwd_kernel(const float* __restrict__ hm, int W, int P, int HH, int WW, int K,
                                                                        const double* __restrict__ taps, int R, double om, double u, int32_t* __restrict__ coords,
                                                                        double* __restrict__ norm, int32_t* __restrict__ reset, double* belief, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // A [HW], C [HW]
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  const size_t HW = (size_t)HH * WW;
  const size_t f0 = (size_t)s * W + P;
  double* bg = belief + ((size_t)blockIdx.x * W + P) * HW;
  const double* prev = P > 0 ? bg - HW - (size_t)k * HW : nullptr;
  sq_filter_scan(sq_planes, hm + f0 * HW * K, W - P, HH, WW, K, taps, R, om, u, prev, nullptr, coords + (size_t)s * (W - P) * 2 * K, norm + f0 * K,
                 reset + f0 * K, nullptr, vec, 0, 0, k, SqPlain(), bg);
}

// Backward: one group per (s, k, e), e fastest (the groups of one (s, k) read the same frames).  Frame e's outputs given frames 0 .. min(e + L, W - 1).
__global__ __launch_bounds__(kSqThreads) void seq_smooth_lag_bwd_kernel(const float* __restrict__ hm, int W, int E, int L, int HH, int WW, int K,
                                                                        const double* __restrict__ taps, int R, double om, double u,
                                                                        const double* __restrict__ belief, const double* __restrict__ norm,
                                                                        const int32_t* __restrict__ reset, float* __restrict__ smoothed,
                                                                        int32_t* __restrict__ coords, float* __restrict__ conf, double* __restrict__ mass,
                                                                        int32_t* __restrict__ cut, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // B [HW], C [HW], C2 [HW]
  const int g = blockIdx.x / E, e = blockIdx.x - g * E;
  const int s = g / K, k = g - s * K;
  const int top = L < W - 1 - e ? e + L : W - 1;
  sq_smooth_back(sq_planes, hm, HH, WW, K, taps, R, om, u, belief + (size_t)g * W * HH * WW, norm, reset, (size_t)s * W, (size_t)s * E, k, top, e, e, smoothed,
                 coords, conf, mass, cut, nullptr, vec);
}

}  // namespace

hipError_t seq_smooth(const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double om, double u, double* belief, float* smoothed,
                      int32_t* coords, float* conf, double* norm, int32_t* reset, double* mass, int32_t* cut, double* trans, hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, K, R) || (int64_t)HH * WW > kSeqSmoothMaxHW || !belief || !coords || !norm || !reset) return hipErrorInvalidValue;
  const int HW = HH * WW;
  const int vec = sq_vec(hm, HW, K) ? 1 : 0;
  static LdsAttr fwd_attr, bwd_attr;
  if (hipError_t e = fwd_attr.ensure(reinterpret_cast<const void*>(seq_smooth_fwd_kernel), kSqLdsMax); e != hipSuccess) return e;
  if (hipError_t e = bwd_attr.ensure(reinterpret_cast<const void*>(seq_smooth_bwd_kernel), kSmLdsMax); e != hipSuccess) return e;
  hipLaunchKernelGGL(seq_smooth_fwd_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8, st, hm, T, HH, WW, K, taps, R, om, u, coords, norm, reset, belief, vec);
  hipLaunchKernelGGL(seq_smooth_bwd_kernel, dim3(S * K), dim3(kSqThreads), 3 * HW * 8, st, hm, T, HH, WW, K, taps, R, om, u, belief, norm, reset, smoothed,
                     coords, conf, mass, cut, trans, vec);
  return hipGetLastError();
}

hipError_t seq_smooth_lag(const float* hm, int S, int W, int P, int E, int L, int HH, int WW, int K, const double* taps, int R, double om, double u,
                          int32_t* scan_coords, double* belief, double* norm, int32_t* reset, float* smoothed, int32_t* coords, float* conf, double* mass,
                          int32_t* cut, hipStream_t st) {
  if (!sq_sizes_ok(S, W, HH, WW, K, R) || (int64_t)HH * WW > kSeqSmoothMaxHW || P < 0 || P > W || E < 0 || E > W || L < 1 || !belief || !norm || !reset ||
      (E > 0 && !coords) || (P < W && !scan_coords) || (int64_t)S * K * W >= ((int64_t)1 << 31))
    return hipErrorInvalidValue;
  const int HW = HH * WW;
  const int vec = sq_vec(hm, HW, K) ? 1 : 0;
  static LdsAttr fwd_attr, bwd_attr;
  if (hipError_t e = fwd_attr.ensure(reinterpret_cast<const void*>(seq_smooth_lag_fwd_kernel), kSqLdsMax); e != hipSuccess) return e;
  if (hipError_t e = bwd_attr.ensure(reinterpret_cast<const void*>(seq_smooth_lag_bwd_kernel), kSmLdsMax); e != hipSuccess) return e;
  if (P < W)
    hipLaunchKernelGGL(seq_smooth_lag_fwd_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8, st, hm, W, P, HH, WW, K, taps, R, om, u, scan_coords, norm, reset,
                       belief, vec);
  if (E > 0)      // a zero-size grid is an error
    hipLaunchKernelGGL(seq_smooth_lag_bwd_kernel, dim3(S * K * E), dim3(kSqThreads), 3 * HW * 8, st, hm, W, E, L, HH, WW, K, taps, R, om, u, belief, norm, reset,
                       smoothed, coords, conf, mass, cut, vec);
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_seq_smooth(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, float* smoothed,
                   int32_t* coords, float* conf, double* norm, int32_t* reset, double* mass, int32_t* cut, double* trans) {
  const std::string w("seq_smooth");
  JCM_TRY(check(h, false));
  // the argument rules of jcm_seq_filter with this entry point's own map limit
  JCM_TRY(seq_check_joints(w, hm, S, T, HH, WW, K, taps, R, rho, kSeqSmoothMaxHW, "three float64 planes"));
  if (!coords) return fail(JCM_ERR_ARG, w + ": null pointer (coords is required; smoothed, conf, norm, reset, mass, cut and trans may be NULL)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  // every a_t, float64 per (sequence, joint, frame, cell): the workspace grows to hold them, and a clip they cannot fit in is refused
  JCM_TRY(workspace_or_refuse(h, w, (double)S * K * T * HH * WW * 8.0 + (double)S * K * T * 12.0 + 8192.0, "beliefs", S, T));
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  double* belief = nullptr;
  double* norm_w = norm;
  int32_t* reset_w = reset;
  return seq_launch(h, w, taps, K * (2 * R + 1), [&] {
    belief = arena_alloc<double>(h, (size_t)S * K * T * HH * WW);
    if (!norm) norm_w = arena_alloc<double>(h, (size_t)S * T * K);
    if (!reset) reset_w = arena_alloc<int32_t>(h, (size_t)S * T * K);
  }, [&](const double* dtaps) {
    return seq_smooth(hm, S, T, HH, WW, K, dtaps, R, om, u, belief, smoothed, coords, conf, norm_w, reset_w, mass, cut, trans, h->stream);
  });
}

int jcm_seq_smooth_lag(jcm_handle h, const float* hm, int S, int W, int P, int HH, int WW, int K, const double* taps, int R, double rho, int L, int flush,
                       double* belief, double* norm, int32_t* reset, float* smoothed, int32_t* coords, float* conf, double* mass, int32_t* cut) {
  const std::string w("seq_smooth_lag");
  JCM_TRY(check(h, false));
  // the argument rules of jcm_seq_smooth on the window (W < 1 is its T < 1), then this entry point's own
  JCM_TRY(seq_check_joints(w, hm, S, W, HH, WW, K, taps, R, rho, kSeqSmoothMaxHW, "three float64 planes"));
  if (P < 0 || P > W) return fail(JCM_ERR_ARG, w + ": P = " + std::to_string(P) + " pending frames in a window of " + std::to_string(W) + "; 0 <= P <= W");
  if (L < 1) return fail(JCM_ERR_ARG, w + ": L = " + std::to_string(L) + "; L >= 1 (lag 0 is the filter: jcm_seq_filter, Engine.seq_filter)");
  if (flush != 0 && flush != 1) return fail(JCM_ERR_ARG, w + ": flush = " + std::to_string(flush) + "; 0 or 1");
  const int E = flush ? W : (W > L ? W - L : 0);
  if (!belief || !norm || !reset) return fail(JCM_ERR_ARG, w + ": null pointer (belief, norm and reset are the caller's window and are required)");
  if (E > 0 && !coords) return fail(JCM_ERR_ARG, w + ": null pointer (coords is required when a frame is emitted; smoothed, conf, mass and cut may be NULL)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  const size_t n_scan = (size_t)S * (W - P) * 2 * K;      // the scan's own arg-max of the new frames, scratch
  JCM_TRY(workspace_or_refuse(h, w, (double)n_scan * 4.0 + 8192.0, "scan coordinates", S, W));
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  int32_t* scan_coords = nullptr;
  return seq_launch(h, w, taps, K * (2 * R + 1), [&] {
    if (P < W) scan_coords = arena_alloc<int32_t>(h, n_scan);
  }, [&](const double* dtaps) {
    return seq_smooth_lag(hm, S, W, P, E, L, HH, WW, K, dtaps, R, om, u, scan_coords, belief, norm, reset, smoothed, coords, conf, mass, cut, h->stream);
  });
}

}  // extern "C"
