// The scan of the frame sequences, shared by sequence.hip (one hidden position per (sequence, joint)) and seq_tracks.hip (several torso
// tracks through one single-channel map): ONE copy of the filter's and of Viterbi's recurrence, so that the two files cannot drift apart.
// All arithmetic is float64, one correctly rounded operation per step, in the order include/jcm.h states.
// One work group scans the T frames of a launch: the belief plane A (a_{t-1} / d_{t-1}) and the scratch plane C live in LDS as float64 for the whole
// launch, Viterbi's byte plane of dy* beside them (2 * 64 KB + 8 KB at the largest map, 8192 cells).  A frame is
//   vertical pass   A -> C                      (consecutive lanes read consecutive cells of a row dy away: conflict-free ds_read_b64)
//   stage p_t       -> A  (A is dead by then)   the frame's HW * K floats walked front to back, coalesced, as float4 where frames are 16-byte aligned
//                                               (the staging of peaks.hip), the group's own channel widened into the plane
//   horizontal pass C -> b = p_t * pred in A,   with the thread's share of Z (or of max b) in a register
//   work-group reduction, division, arg-max.
// A cell i belongs to thread i % 1024 in every pass that writes it, so a plane is only read across threads between barriers.  The sum Z: a thread adds
// its cells in ascending order, the wave a butterfly of shuffles, thread-uniformly the 16 wave sums in wave order -- nothing of it depends on S or T.
// Viterbi writes the source cell of every cell (int16, -1 across a break) to [T][HW] of workspace per group and the arg-max of every d_t; a second launch
// walks them back (its dependent loads see the first launch's stores across the kernel boundary).  No atomics; every store is a plain vector store.
//
// The policy `Tr` is what a caller does to the observation: tr.frame(t) gives the frame's functor ex, ex(cell, value) is the value staged for that
// cell, and tr.emit(ex, frame, cell, p) is called by one thread with the filter's arg-max cell of the frame.  SqPlain stages the map as it is.
//
// The policy `Mv` is where a frame's lattice lies on the one before: cell (y, x) of frame t is cell (y + sy, x + sx) of frame t-1, so
// the vertical pass reads A a whole number of rows away and the horizontal pass C a whole number of columns away, with the tap ranges clipped to the
// plane as before -- nothing is interpolated and the planes do not grow.  C is indexed (row of frame t, column of frame t-1).  SqStill is no shift,
// a compile-time zero: with it both scans are, instruction for instruction, what they were without the policy.  SqShift reads (sy, sx) of the frame
// from the sequence's int32 [T][2] row and clamps it to +-(side + R), beyond which no tap reaches the map, so that no index sum can overflow.
#pragma once

#include "ctx.h"

namespace jcm {

namespace {

constexpr int kSqThreads = 1024;
constexpr int kSqWaves = kSqThreads / 64;
constexpr int kSqUnroll = 4;                         // float4 loads a thread has in flight while staging
constexpr int kSqTaps = 2 * kSeqMaxR + 1;
constexpr int kSqNone = 0x7fffffff;
constexpr int kSqLdsMax = 2 * kSeqMaxHW * 8 + kSeqMaxHW;

struct SqPlain {
  struct Frame {
    __device__ __forceinline__ double operator()(int, double v) const { return v; }
  };
  __device__ __forceinline__ Frame frame(int) const { return Frame(); }
  __device__ __forceinline__ void emit(const Frame&, size_t, int, const float*) const {}
};

struct SqStill {
  static constexpr bool kMoving = false;
  __device__ __forceinline__ int sy(int, int) const { return 0; }
  __device__ __forceinline__ int sx(int, int) const { return 0; }
};

struct SqShift {
  static constexpr bool kMoving = true;
  const int32_t* __restrict__ sh;      // [T][2] of the group's sequence
  __device__ __forceinline__ int sy(int t, int lim) const { return min(max(sh[2 * t], -lim), lim); }
  __device__ __forceinline__ int sx(int t, int lim) const { return min(max(sh[2 * t + 1], -lim), lim); }
};

__device__ __forceinline__ bool sq_better(double v, int i, double w, int j) { return v > w || (v == w && i < j); }

// channel k of one frame [HW][K] -> plane [HW], widened
template <class Ex>
__device__ __forceinline__ void sq_stage(const float* __restrict__ src, int n, int K, int k, bool vec, double* __restrict__ plane, int tid, const Ex& ex) {
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
          if (c == k) plane[p] = ex(p, (double)v[j]);
          if (++c == K) { c = 0; ++p; }
        }
      }
    }
    e0 = nvec << 2;
  }
  for (int e = e0 + tid; e < n; e += kSqThreads) {
    const int p = e / K, c = e - p * K;
    if (c == k) plane[p] = ex(p, (double)src[e]);
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

// The filter of one group: it reads sequence s_in of hm, channel k, and writes as sequence s_out of the outputs (the two differ only for the tracks).
// sq_planes: A [HW], C [HW] of dynamic LDS.  belief: the group's own float64 [T][HW], every a_t as it is divided (what the smoother's backward launch
// reads, seq_smooth.hip), or null.
template <class Tr, class Mv = SqStill>
__device__ __forceinline__ void sq_filter_scan(double* sq_planes, const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps,
                                               int R, double om, double u, const double* __restrict__ state_in, float* __restrict__ filtered,
                                               int32_t* coords, double* __restrict__ norm, int32_t* __restrict__ reset, double* __restrict__ state_out,
                                               int vec, int s_in, int s_out, int k, const Tr& tr, double* __restrict__ belief = nullptr,
                                               const Mv& mv = Mv()) {
  __shared__ double w[kSqTaps];
  __shared__ double rd[kSqWaves];
  __shared__ int ri[kSqWaves];
  const int tid = threadIdx.x;
  const int HW = HH * WW, n = HW * K;
  double* A = sq_planes;
  double* C = sq_planes + HW;
  if (tid < 2 * R + 1) w[tid] = taps[k * (2 * R + 1) + tid];
  const size_t plane0 = ((size_t)s_out * K + k) * HW;
  bool prev = state_in != nullptr;
  if (prev)
    for (int i = tid; i < HW; i += kSqThreads) A[i] = state_in[plane0 + i];
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const size_t ft = (size_t)s_out * T + t;
    const float* src = hm + ((size_t)s_in * T + t) * n;
    const auto ex = tr.frame(t);
    int rs = 0;
    double Z = 0.0;
    if (prev) {
      const int sy = mv.sy(t, HH + R), sx = mv.sx(t, WW + R);      // 0 at compile time for SqStill
      for (int i = tid; i < HW; i += kSqThreads) {
        const int y = i / WW + sy;                                 // the cell's row in frame t-1's lattice; an empty range leaves 0.0
        const int lo = max(-R, y - (HH - 1)), hi = min(R, y);
        double acc = 0.0;
        for (int dy = lo; dy <= hi; ++dy) acc = acc + w[dy + R] * A[i + (sy - dy) * WW];
        C[i] = acc;
      }
      __syncthreads();
      sq_stage(src, n, K, k, vec != 0, A, tid, ex);
      __syncthreads();
      double zp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) {
        const int y = i / WW, x = i - y * WW + sx;
        const int lo = max(-R, x - (WW - 1)), hi = min(R, x);
        double m = 0.0;
        for (int dx = lo; dx <= hi; ++dx) m = m + w[dx + R] * C[i + (sx - dx)];
        const double pred = om * m + u;
        const double b = A[i] * pred;
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
    const double uni = 1.0 / (double)HW;
    double bv = -1.0;
    int bi = kSqNone;
    for (int i = tid; i < HW; i += kSqThreads) {
      const double a = rs == 2 ? uni : A[i] / Z;
      A[i] = a;
      if (a > bv) { bv = a; bi = i; }
      if (filtered) filtered[(ft * HW + i) * K + k] = (float)a;
      if (belief) belief[(size_t)t * HW + i] = a;
    }
    sq_block_argmax(bv, bi, rd, ri, tid);      // its barriers also order this frame's A against the next vertical pass
    if (tid == 0) {
      const int r = bi / WW;
      coords[(ft * 2 + 0) * K + k] = r;
      coords[(ft * 2 + 1) * K + k] = bi - r * WW;
      if (norm) norm[ft * K + k] = Z;
      if (reset) reset[ft * K + k] = rs;
      tr.emit(ex, ft, bi, src);
    }
    prev = true;
  }
  if (state_out)
    for (int i = tid; i < HW; i += kSqThreads) state_out[plane0 + i] = A[i];
}

// Viterbi's scan of one group; g_ws: the group's slot of the workspace (bp [.][T][HW], amax [.][T]).  sq_planes: D [HW], C [HW], dy* [HW] bytes.
template <class Tr, class Mv = SqStill>
__device__ __forceinline__ void sq_viterbi_scan(double* sq_planes, const float* __restrict__ hm, int T, int HH, int WW, int K, const double* __restrict__ taps,
                                                int R, double om, double u, int16_t* __restrict__ bp, int32_t* __restrict__ amax, double* __restrict__ maxes,
                                                int32_t* __restrict__ breaks, int vec, int s_in, int s_out, int k, int g_ws, const Tr& tr,
                                                const Mv& mv = Mv()) {
  __shared__ double w[kSqTaps];
  __shared__ double rd[kSqWaves];
  __shared__ int ri[kSqWaves];
  const int tid = threadIdx.x;
  const int HW = HH * WW, n = HW * K;
  double* D = sq_planes;
  double* C = sq_planes + HW;
  uint8_t* dyb = reinterpret_cast<uint8_t*>(sq_planes + 2 * (size_t)HW);
  if (tid < 2 * R + 1) w[tid] = taps[k * (2 * R + 1) + tid];
  __syncthreads();
  int16_t* bpg = bp + (size_t)g_ws * T * HW;
  double Dmax = 0.0;      // max and first-occurrence arg-max of d_{t-1}
  int Darg = 0;

  for (int t = 0; t < T; ++t) {
    const size_t ft = (size_t)s_out * T + t;
    const float* src = hm + ((size_t)s_in * T + t) * n;
    const auto ex = tr.frame(t);
    int16_t* bpt = bpg + (size_t)t * HW;
    int brk = 0;
    double M = 0.0;
    if (t > 0) {
      const int sy = mv.sy(t, HH + R), sx = mv.sx(t, WW + R);      // 0 at compile time for SqStill
      for (int i = tid; i < HW; i += kSqThreads) {
        const int y = i / WW + sy;
        const int lo = max(-R, y - (HH - 1)), hi = min(R, y);
        double best = -1.0;
        int bdy = lo;
        for (int dy = lo; dy <= hi; ++dy) {
          const double v = w[dy + R] * D[i + (sy - dy) * WW];
          if (v > best) { best = v; bdy = dy; }
        }
        if (Mv::kMoving && lo > hi) { best = 0.0; bdy = 0; }       // no tap reaches the map: the maximum over nothing is 0
        C[i] = best;
        dyb[i] = (uint8_t)(bdy + R);
      }
      __syncthreads();
      sq_stage(src, n, K, k, vec != 0, D, tid, ex);
      __syncthreads();
      const double jump = u * Dmax;
      double mp = 0.0;
      for (int i = tid; i < HW; i += kSqThreads) {
        const int y = i / WW, x = i - y * WW + sx;
        const int lo = max(-R, x - (WW - 1)), hi = min(R, x);
        double best = -1.0;
        int bdx = lo;
        for (int dx = lo; dx <= hi; ++dx) {
          const double v = w[dx + R] * C[i + (sx - dx)];
          if (v > best) { best = v; bdx = dx; }
        }
        const int via = Mv::kMoving && lo > hi ? i : i + (sx - bdx);      // (y, x - dx* + sx); with no tap inside the map any cell of the plane
        int from = via + (sy - ((int)dyb[via] - R)) * WW;        // (y - dy*(y, x - dx* + sx) + sy, x - dx* + sx), a cell of frame t-1's lattice
        if (Mv::kMoving && !(best > 0.0)) { best = 0.0; from = Darg; }      // m = 0 has no source inside the map: b is 0 unless the jump wins
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
      amax[(size_t)g_ws * T + t] = bi;
      if (maxes) maxes[ft * K + k] = M;
      if (breaks) breaks[ft * K + k] = brk;
    }
  }
}

// One lane's walk back through a group's source cells: from the arg-max of d_{T-1}; across a break (-1) the earlier segment ends at the arg-max of its
// last d.  put(t, cell) receives the track's cell of every frame, last frame first.
template <class Put>
__device__ __forceinline__ void sq_walk_back(const int16_t* __restrict__ bpg, const int32_t* __restrict__ am, int T, int HW, const Put& put) {
  int cell = am[T - 1];
  for (int t = T - 1; t >= 0; --t) {
    cell = min(max(cell, 0), HW - 1);
    put(t, cell);
    if (t > 0) {
      const int from = bpg[(size_t)t * HW + cell];
      cell = from >= 0 ? from : am[t - 1];
    }
  }
}

inline bool sq_sizes_ok(int S, int T, int HH, int WW, int K, int R) {
  return S >= 1 && T >= 1 && HH >= 1 && WW >= 1 && K >= 1 && K <= kSeqMaxK && R >= 0 && R <= kSeqMaxR && (int64_t)HH * WW <= kSeqMaxHW &&
         (int64_t)S * K < ((int64_t)1 << 31);
}
// float4 loads need every frame to start on 16 bytes
inline bool sq_vec(const float* hm, int HW, int K) { return ((int64_t)HW * K) % 4 == 0 && reinterpret_cast<uintptr_t>(hm) % 16 == 0; }

}  // namespace

}  // namespace jcm
