// Frame sequences: a temporal edge on the heat maps hm [S,T,HH,WW,K] of a clip -- the causal forward filter and the most probable track
// (Viterbi, max-product in the probability domain) of a hidden position per (sequence, joint) under a separable truncated motion kernel plus a uniform
// "anywhere" term.  All arithmetic is float64, one correctly rounded operation per step, in the order include/jcm.h states.
// One work group per (sequence, joint) scans the T frames of a launch: the belief plane A (a_{t-1} / d_{t-1}) and the scratch plane C live in LDS as
// float64 for the whole launch, Viterbi's byte plane of dy* beside them (2 * 64 KB + 8 KB at the largest map, 8192 cells).  A frame is
//   vertical pass   A -> C                      (consecutive lanes read consecutive cells of a row dy away: conflict-free ds_read_b64)
//   stage p_t       -> A  (A is dead by then)   the frame's HW * K floats walked front to back, coalesced, as float4 where frames are 16-byte aligned
//                                               (the staging of peaks.hip), the group's own channel widened into the plane
//   horizontal pass C -> b = p_t * pred in A,   with the thread's share of Z (or of max b) in a register
//   work-group reduction, division, arg-max.
// A cell i belongs to thread i % 1024 in every pass that writes it, so a plane is only read across threads between barriers.  The sum Z: a thread adds
// its cells in ascending order, the wave a butterfly of shuffles, thread-uniformly the 16 wave sums in wave order -- nothing of it depends on S or T.
// Viterbi writes the source cell of every cell (int16, -1 across a break) to [T][HW] of workspace per group and the arg-max of every d_t; a second launch
// walks them back (its dependent loads see the first launch's stores across the kernel boundary).  No atomics; every store is a plain vector store.
#include <string>

#include "ctx.h"

namespace jcm {

namespace {

constexpr int kSqThreads = 1024;
constexpr int kSqWaves = kSqThreads / 64;
constexpr int kSqUnroll = 4;                         // float4 loads a thread has in flight while staging
constexpr int kSqTaps = 2 * kSeqMaxR + 1;
constexpr int kSqPut = 480;                          // doubles per upload launch: 3840 bytes of its 4096 bytes of arguments
constexpr int kSqNone = 0x7fffffff;
constexpr int kSqLdsMax = 2 * kSeqMaxHW * 8 + kSeqMaxHW;

struct SeqPut {
  double v[kSqPut];
};
__global__ __launch_bounds__(256) void seq_put_kernel(SeqPut p, int n, double* __restrict__ dst) {
  for (int i = threadIdx.x; i < n; i += 256) dst[i] = p.v[i];
}

__device__ __forceinline__ bool sq_better(double v, int i, double w, int j) { return v > w || (v == w && i < j); }

// channel k of one frame [HW][K] -> plane [HW], widened
__device__ __forceinline__ void sq_stage(const float* __restrict__ src, int n, int K, int k, bool vec, double* __restrict__ plane, int tid) {
  int e0 = 0;
  if (vec) {
    const float4* src4 = reinterpret_cast<const float4*>(src);
    const int nvec = n >> 2;
    for (int f0 = tid; f0 < nvec; f0 += kSqThreads * kSqUnroll) {      // a trip's loads past the end re-read the last float4
      float4 t[kSqUnroll];
#pragma unroll
      for (int q = 0; q < kSqUnroll; ++q) t[q] = src4[min(f0 + q * kSqThreads, nvec - 1)];
#pragma unroll
      for (int q = 0; q < kSqUnroll; ++q) {
        const int f = f0 + q * kSqThreads;
        if (f >= nvec) break;
        const float v[4] = {t[q].x, t[q].y, t[q].z, t[q].w};
        int p = (4 * f) / K, c = 4 * f - p * K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (c == k) plane[p] = (double)v[j];
          if (++c == K) { c = 0; ++p; }
        }
      }
    }
    e0 = nvec << 2;
  }
  for (int e = e0 + tid; e < n; e += kSqThreads) {
    const int p = e / K, c = e - p * K;
    if (c == k) plane[p] = (double)src[e];
  }
}

// Both reductions end with every thread holding the same value; rd / ri are free again when they return.
__device__ __forceinline__ double sq_block_sum(double v, double* rd, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  if ((tid & 63) == 0) rd[tid >> 6] = v;
  __syncthreads();
  double z = rd[0];
#pragma unroll
  for (int w = 1; w < kSqWaves; ++w) z = z + rd[w];
  __syncthreads();
  return z;
}

__device__ __forceinline__ void sq_block_argmax(double& bv, int& bi, double* rd, int* ri, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (sq_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { rd[tid >> 6] = bv; ri[tid >> 6] = bi; }
  __syncthreads();
  bv = rd[0];
  bi = ri[0];
#pragma unroll
  for (int w = 1; w < kSqWaves; ++w)
    if (sq_better(rd[w], ri[w], bv, bi)) { bv = rd[w]; bi = ri[w]; }
  __syncthreads();
}

__global__ __launch_bounds__(kSqThreads) void seq_filter_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps, int R,
                                                                double om, double u, const double* __restrict__ state_in, float* __restrict__ filtered,
                                                                int32_t* __restrict__ coords, double* __restrict__ norm, int32_t* __restrict__ reset,
                                                                double* __restrict__ state_out, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // A [HW], C [HW]
  __shared__ double w[kSqTaps];
  __shared__ double rd[kSqWaves];
  __shared__ int ri[kSqWaves];
  const int tid = threadIdx.x;
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  const int HW = HH * WW, n = HW * K;
  double* A = sq_planes;
  double* C = sq_planes + HW;
  if (tid < 2 * R + 1) w[tid] = taps[k * (2 * R + 1) + tid];
  const size_t plane0 = ((size_t)s * K + k) * HW;
  bool prev = state_in != nullptr;
  if (prev)
    for (int i = tid; i < HW; i += kSqThreads) A[i] = state_in[plane0 + i];
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const size_t ft = (size_t)s * T + t;
    const float* src = hm + ft * n;
    int rs = 0;
    double Z = 0.0;
    if (prev) {
      for (int i = tid; i < HW; i += kSqThreads) {
        const int y = i / WW;
        const int lo = max(-R, y - (HH - 1)), hi = min(R, y);
        double acc = 0.0;
        for (int dy = lo; dy <= hi; ++dy) acc = acc + w[dy + R] * A[i - dy * WW];
        C[i] = acc;
      }
      __syncthreads();
      sq_stage(src, n, K, k, vec != 0, A, tid);
      __syncthreads();
      double zp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) {
        const int y = i / WW, x = i - y * WW;
        const int lo = max(-R, x - (WW - 1)), hi = min(R, x);
        double m = 0.0;
        for (int dx = lo; dx <= hi; ++dx) m = m + w[dx + R] * C[i - dx];
        const double pred = om * m + u;
        const double b = A[i] * pred;
        A[i] = b;
        zp = zp + b;
      }
      Z = sq_block_sum(zp, rd, tid);
      if (!(Z > 0.0 && Z <= 1.79769313486231570815e308)) rs = 1;      // 0 or not finite (negative values and NaN are outside the contract)
    }
    if (!prev || rs == 1) {      // b = p_t  (thread-uniform: Z is)
      sq_stage(src, n, K, k, vec != 0, A, tid);
      __syncthreads();
      double zp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) zp = zp + A[i];
      Z = sq_block_sum(zp, rd, tid);
      if (Z == 0.0) rs = 2;
    }
    const double uni = 1.0 / (double)HW;
    double bv = -1.0;
    int bi = kSqNone;
    for (int i = tid; i < HW; i += kSqThreads) {
      const double a = rs == 2 ? uni : A[i] / Z;
      A[i] = a;
      if (a > bv) { bv = a; bi = i; }
      if (filtered) filtered[(ft * HW + i) * K + k] = (float)a;
    }
    sq_block_argmax(bv, bi, rd, ri, tid);      // its barriers also order this frame's A against the next vertical pass
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

__global__ __launch_bounds__(kSqThreads) void seq_viterbi_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps, int R,
                                                                 double om, double u, int16_t* __restrict__ bp, int32_t* __restrict__ amax,
                                                                 double* __restrict__ maxes, int32_t* __restrict__ breaks, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sq_planes[];      // D [HW], C [HW], dy* [HW] bytes
  __shared__ double w[kSqTaps];
  __shared__ double rd[kSqWaves];
  __shared__ int ri[kSqWaves];
  const int tid = threadIdx.x;
  const int s = blockIdx.x / K, k = blockIdx.x - s * K;
  const int HW = HH * WW, n = HW * K;
  double* D = sq_planes;
  double* C = sq_planes + HW;
  uint8_t* dyb = reinterpret_cast<uint8_t*>(sq_planes + 2 * (size_t)HW);
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
      for (int i = tid; i < HW; i += kSqThreads) {
        const int y = i / WW;
        const int lo = max(-R, y - (HH - 1)), hi = min(R, y);
        double best = -1.0;
        int bdy = lo;
        for (int dy = lo; dy <= hi; ++dy) {
          const double v = w[dy + R] * D[i - dy * WW];
          if (v > best) { best = v; bdy = dy; }
        }
        C[i] = best;
        dyb[i] = (uint8_t)(bdy + R);
      }
      __syncthreads();
      sq_stage(src, n, K, k, vec != 0, D, tid);
      __syncthreads();
      const double jump = u * Dmax;
      double mp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) {
        const int y = i / WW, x = i - y * WW;
        const int lo = max(-R, x - (WW - 1)), hi = min(R, x);
        double best = -1.0;
        int bdx = lo;
        for (int dx = lo; dx <= hi; ++dx) {
          const double v = w[dx + R] * C[i - dx];
          if (v > best) { best = v; bdx = dx; }
        }
        const int via = i - bdx;                                 // (y, x - dx*)
        int from = via - ((int)dyb[via] - R) * WW;               // (y - dy*(y, x - dx*), x - dx*)
        double e = om * best;
        if (jump > e) { e = jump; from = Darg; }
        const double b = D[i] * e;
        D[i] = b;
        bpt[i] = (int16_t)from;
        mp = fmax(mp, b);
      }
      int none = kSqNone;
      sq_block_argmax(mp, none, rd, ri, tid);
      M = mp;
      if (M == 0.0) brk = 1;
    }
    if (t == 0 || brk == 1) {      // b = p_t  (thread-uniform: M is)
      sq_stage(src, n, K, k, vec != 0, D, tid);
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

// one lane per (sequence, joint): from the arg-max of d_{T-1} along the source cells; across a break (-1) the earlier segment ends at the arg-max of its last d
__global__ __launch_bounds__(64) void seq_backtrace_kernel(const int16_t* __restrict__ bp, const int32_t* __restrict__ amax, int G, int T, int HW, int WW, int K,
                                                           int32_t* __restrict__ path) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= G) return;
  const int s = g / K, k = g - s * K;
  const int16_t* bpg = bp + (size_t)g * T * HW;
  const int32_t* am = amax + (size_t)g * T;
  int cell = am[T - 1];
  for (int t = T - 1; t >= 0; --t) {
    cell = min(max(cell, 0), HW - 1);
    const size_t ft = (size_t)s * T + t;
    const int r = cell / WW;
    path[(ft * 2 + 0) * K + k] = r;
    path[(ft * 2 + 1) * K + k] = cell - r * WW;
    if (t > 0) {
      const int from = bpg[(size_t)t * HW + cell];
      cell = from >= 0 ? from : am[t - 1];
    }
  }
}

bool sq_sizes_ok(int S, int T, int HH, int WW, int K, int R) {
  return S >= 1 && T >= 1 && HH >= 1 && WW >= 1 && K >= 1 && K <= kSeqMaxK && R >= 0 && R <= kSeqMaxR && (int64_t)HH * WW <= kSeqMaxHW &&
         (int64_t)S * K < ((int64_t)1 << 31);
}
// float4 loads need every frame to start on 16 bytes
bool sq_vec(const float* hm, int HW, int K) { return ((int64_t)HW * K) % 4 == 0 && reinterpret_cast<uintptr_t>(hm) % 16 == 0; }

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

hipError_t seq_filter(const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double om, double u, const double* state_in,
                      float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out, hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, K, R)) return hipErrorInvalidValue;
  const int HW = HH * WW;
  static LdsAttr attr;
  if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(seq_filter_kernel), kSqLdsMax); e != hipSuccess) return e;
  hipLaunchKernelGGL(seq_filter_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8, st, hm, T, HH, WW, K, taps, R, om, u, state_in, filtered, coords, norm,
                     reset, state_out, sq_vec(hm, HW, K) ? 1 : 0);
  return hipGetLastError();
}

hipError_t seq_viterbi(const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double om, double u, int16_t* bp, int32_t* amax,
                       int32_t* path, double* maxes, int32_t* breaks, hipStream_t st) {
  if (!sq_sizes_ok(S, T, HH, WW, K, R)) return hipErrorInvalidValue;
  const int HW = HH * WW;
  static LdsAttr attr;
  if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(seq_viterbi_kernel), kSqLdsMax); e != hipSuccess) return e;
  hipLaunchKernelGGL(seq_viterbi_kernel, dim3(S * K), dim3(kSqThreads), 2 * HW * 8 + ((HW + 7) & ~7), st, hm, T, HH, WW, K, taps, R, om, u, bp, amax, maxes,
                     breaks, sq_vec(hm, HW, K) ? 1 : 0);
  const int G = S * K;
  hipLaunchKernelGGL(seq_backtrace_kernel, dim3((G + 63) / 64), dim3(64), 0, st, bp, amax, G, T, HW, WW, K, path);
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

namespace {

// the argument rules the two entry points share; `what` names the entry point in the message
int seq_check(const char* what, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho) {
  const std::string w(what);
  if (S < 1 || T < 1 || HH < 1 || WW < 1 || K < 1) return fail(JCM_ERR_ARG, w + ": bad sizes (S, T, HH, WW, K >= 1)");
  if (K > kSeqMaxK) return fail(JCM_ERR_ARG, w + ": K = " + std::to_string(K) + " joints; K <= 16");
  if (R < 0 || R > kSeqMaxR) return fail(JCM_ERR_ARG, w + ": R = " + std::to_string(R) + "; 0 <= R <= 16");
  if (!(rho >= 0.0 && rho <= 1.0)) return fail(JCM_ERR_ARG, w + ": rho outside [0, 1]");
  if ((int64_t)HH * WW > kSeqMaxHW)
    return fail(JCM_ERR_ARG, w + ": a map of " + std::to_string(HH) + " x " + std::to_string(WW) +
                                 " cells; HH * WW <= 8192 (two float64 planes and a byte plane in 160 KB of LDS), a larger map is not truncated");
  if ((int64_t)S * T >= ((int64_t)1 << 31) / K) return fail(JCM_ERR_ARG, w + ": bad sizes (S * T * K < 2^31)");
  if (!hm || !taps) return fail(JCM_ERR_ARG, w + ": null pointer (hm and taps are required)");
  return JCM_OK;
}

}  // namespace

extern "C" {

int jcm_seq_filter(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, const double* state_in,
                   float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out) {
  JCM_TRY(check(h, false));
  JCM_TRY(seq_check("seq_filter", hm, S, T, HH, WW, K, taps, R, rho));
  if (!coords) return fail(JCM_ERR_ARG, "seq_filter: null pointer (coords is required; state_in, filtered, norm, reset and state_out may be NULL)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  return with_arena(c, [&] {
    double* dtaps = arena_alloc<double>(c, (size_t)K * (2 * R + 1));
    if (c->dry) return (int)JCM_OK;
    hipEvent_t e0, e1;
    JCM_TRY(prof_begin(c, &e0, &e1));
    hipError_t launch = seq_put_taps(taps, K * (2 * R + 1), dtaps, c->stream);
    if (launch == hipSuccess)
      launch = seq_filter(hm, S, T, HH, WW, K, dtaps, R, om, u, state_in, filtered, coords, norm, reset, state_out, c->stream);
    prof_end(c, "seq_filter", e0, e1, launch == hipSuccess);
    if (launch != hipSuccess) return fail(JCM_ERR_HIP, std::string("seq_filter: ") + hipGetErrorString(launch));
    return (int)JCM_OK;
  });
}

int jcm_seq_viterbi(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, int32_t* path,
                    double* maxes, int32_t* breaks) {
  JCM_TRY(check(h, false));
  JCM_TRY(seq_check("seq_viterbi", hm, S, T, HH, WW, K, taps, R, rho));
  if (!path) return fail(JCM_ERR_ARG, "seq_viterbi: null pointer (path is required; maxes and breaks may be NULL)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  // the back-pointers: one int16 per (sequence, joint, frame, cell); the workspace grows to hold them, and a clip they cannot fit in is refused
  const double need_d = (double)S * K * T * HH * WW * 2.0 + (double)S * K * T * 4.0 + 8192.0;
  if (need_d > (double)c->arena_cap) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need_d > (double)free_b + (double)c->arena_cap)
      return fail(JCM_ERR_STATE, "seq_viterbi: the back-pointers of " + std::to_string(S) + " x " + std::to_string(T) + " frames need " +
                                     std::to_string((unsigned long long)need_d) + " bytes of workspace, " +
                                     std::to_string((unsigned long long)(free_b + c->arena_cap)) + " bytes are available; split the clip");
  }
  const double om = 1.0 - rho, u = rho / (double)(HH * WW);
  return with_arena(c, [&] {
    double* dtaps = arena_alloc<double>(c, (size_t)K * (2 * R + 1));
    int16_t* bp = arena_alloc<int16_t>(c, (size_t)S * K * T * HH * WW);
    int32_t* amax = arena_alloc<int32_t>(c, (size_t)S * K * T);
    if (c->dry) return (int)JCM_OK;
    hipEvent_t e0, e1;
    JCM_TRY(prof_begin(c, &e0, &e1));
    hipError_t launch = seq_put_taps(taps, K * (2 * R + 1), dtaps, c->stream);
    if (launch == hipSuccess) launch = seq_viterbi(hm, S, T, HH, WW, K, dtaps, R, om, u, bp, amax, path, maxes, breaks, c->stream);
    prof_end(c, "seq_viterbi", e0, e1, launch == hipSuccess);
    if (launch != hipSuccess) return fail(JCM_ERR_HIP, std::string("seq_viterbi: ") + hipGetErrorString(launch));
    return (int)JCM_OK;
  });
}

}  // extern "C"
