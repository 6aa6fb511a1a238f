// Clip pose decoding (include/jcm.h: jcm_seq_pose_viterbi): the exact MAP over a chain of fully connected 9-joint pose models -- the
// P^9 poses of jcm_pose_decode per frame -- linked in time by one P x P transition table per joint.  The temporal term factorises over the joints, so a
// max-plus step over P^9 states is nine axis passes of P candidates each.  ONE launch, one work group of 1024 threads per clip, frame after frame; every
// step that needs all states of the step before it is separated from it by the work group's own barrier -- there is no barrier across work groups and no
// flag in memory that anyone waits for.  The plane G / D (P^9 float64, 2 MB at P = 4) and the back-pointers live in the workspace; per frame:
//   passes 0 .. 3 on tiles of (all of digits 0 .. 3) x (C consecutive values of the rest) in LDS, the normalisation D - m of the frame before applied as
//     the tile is read; a thread takes whole lines along the pass's axis -- P values in, P values out, in place, one barrier per pass;
//   passes 4 .. 8 on tiles of consecutive states (digits 4 .. 8 in full, several values of digit 3 at a time), the same line routine;
//   the scores: pose_walk (pose_score.h, the expression of pose_search_kernel) with the prefix (p_0 .. p_5) per thread, D = (double)E + G written back,
//     the first-occurrence arg-max by shuffles and 16 slots of LDS.  A frame with no connection to the one before does this step again with D = (double)E.
// Back-pointers: 2 bits per (frame, pass, state), passes 0 .. 3 in one byte per state and passes 4 .. 8 in one 16-bit word per state.
// The walk back is one thread's chain of 9 dependent loads per frame; the outputs of all frames are then written by all threads.
// No atomics; every store is a vector store of plain C++.
#include <string>

#include "entry.h"
#include "pose_score.h"

namespace jcm {

namespace {

constexpr int kSpThreads = 1024;
constexpr int kSpTile = 4096;      // float64 values of a tile in LDS: 32 KB
constexpr int kSpNone = 0x7fffffff;

constexpr int sp_pow(int P, int k) { return k == 0 ? 1 : P * sp_pow(P, k - 1); }
constexpr int sp_chunk(int P) { return P == 1 ? 1 : P == 3 ? 27 : 16; }      // passes 0 .. 3: consecutive low states per tile; divides P^5
constexpr int sp_batch(int P) { return P == 1 ? 1 : P == 2 ? 16 : P == 3 ? 9 : 4; }      // passes 4 .. 8: values of (p_0 .. p_3) per tile; divides P^4

__device__ __forceinline__ bool sp_better(double v, int i, double w, int j) { return v > w || (v == w && i < j); }

// (value descending, index ascending) over the work group -> every thread holds the winner
__device__ __forceinline__ void sp_block_argmax(double& bv, int& bi, double* rd, int* ri, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (sp_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  __syncthreads();      // the slots may still be read from the reduction before
  if ((tid & 63) == 0) { rd[tid >> 6] = bv; ri[tid >> 6] = bi; }
  __syncthreads();
  bv = rd[0];
  bi = ri[0];
#pragma unroll
  for (int w = 1; w < kSpThreads / 64; ++w)
    if (sp_better(rd[w], ri[w], bv, bi)) { bv = rd[w]; bi = ri[w]; }
}

// Passes J0 .. J1 on the n values of a tile in LDS; digit j of a state has the stride P^(JL - j) * C in the tile (JL: the last axis the tile holds in
// full, C: what lies below it).  A line along axis j: G'(b) = max over a < cp[j], ascending, of G(a) + tau[j][a][b]; a strictly greater value replaces;
// b at or beyond cn[j]: -inf.  The winner goes into bits 2 (j - J0) of the state's pointer word.
template <int P, int J0, int J1, int JL, int C>
__device__ __forceinline__ void sp_passes(double* tile, uint16_t* bpt, int n, const double (*tau)[kPdMaxP][kPdMaxP], const int* cp, const int* cn, int tid) {
#pragma unroll
  for (int j = J0; j <= J1; ++j) {
    const int sj = sp_pow(P, JL - j) * C;
    const int na = cp[j], nb = cn[j];
    for (int l = tid; l < n / P; l += kSpThreads) {
      const int hi = l / sj, lo = l - hi * sj, base = hi * sj * P + lo;
      double g[P];
#pragma unroll
      for (int a = 0; a < P; ++a) g[a] = tile[base + a * sj];
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double best = -INFINITY;
        int arg = 0;
        if (b < nb) {
#pragma unroll
          for (int a = 0; a < P; ++a) {
            if (a < na) {
              const double v = g[a] + tau[j][a][b];
              if (v > best) { best = v; arg = a; }
            }
          }
        }
        tile[base + b * sj] = best;
        bpt[base + b * sj] = (uint16_t)(bpt[base + b * sj] | (arg << (2 * (j - J0))));
      }
    }
    __syncthreads();
  }
}

template <int P>
__global__ __launch_bounds__(kSpThreads) void seq_pose_kernel(const float* __restrict__ V, const float* __restrict__ M, const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ cells, const double* __restrict__ tau, int T, double* __restrict__ plane,
                                                              uint8_t* __restrict__ bpa, uint16_t* __restrict__ bpb, int32_t* __restrict__ amax,
                                                              int32_t* __restrict__ start, int32_t* __restrict__ index, int32_t* __restrict__ coords,
                                                              float* __restrict__ frame_score, double* __restrict__ maxes, int32_t* __restrict__ breaks) {
  constexpr int N = sp_pow(P, 9), L = sp_pow(P, 5), MID = sp_pow(P, 4), C = sp_chunk(P), TB = sp_batch(P), NPRE = sp_pow(P, 6), NLEAF = sp_pow(P, 3);
  static_assert(MID * C <= kSpTile && TB * L <= kSpTile && L % C == 0 && MID % TB == 0, "tile sizes");
  __shared__ double tile[kSpTile];
  __shared__ uint16_t bpt[kSpTile];
  __shared__ float Vs[kPdK][kPdMaxP];
  __shared__ float Ms[kPdPairs][kPdMaxP][kPdMaxP];
  __shared__ double taus[kPdK][kPdMaxP][kPdMaxP];
  __shared__ int cnt[2][kPdK];
  __shared__ double rd[kSpThreads / 64];
  __shared__ int ri[kSpThreads / 64];
  const int s = blockIdx.x, tid = threadIdx.x;
  const size_t f0 = (size_t)s * T;
  plane += (size_t)s * N;
  bpa += f0 * N;
  bpb += f0 * N;
  amax += f0;
  start += f0;

  // the scores of every pose of the staged frame: D = (double)E (fresh) or (double)E + G, -inf where the pose is not valid -> (max, first arg-max)
  auto scores = [&](const int* cn, bool fresh, double& bv, int& bi) {
    bv = -INFINITY;
    bi = kSpNone;
    for (int q = tid; q < NPRE; q += kSpThreads) {
      int p[6], r = q;
      bool live = true;
#pragma unroll
      for (int k = 5; k >= 0; --k) {
        p[k] = r % P;
        r /= P;
        live &= p[k] < cn[k];
      }
      double* d = plane + (size_t)q * NLEAF;
      if (fresh || !live) {      // after the passes a state that is not valid holds -inf already
        for (int l = 0; l < NLEAF; ++l) {
          const int p8 = l % P, p7 = (l / P) % P, p6 = l / (P * P);
          if (!live || p6 >= cn[6] || p7 >= cn[7] || p8 >= cn[8]) d[l] = -INFINITY;
        }
      }
      if (live)
        pose_walk(Vs, Ms, cn, p, [&](int p6, int p7, int p8, float E) {
          const int l = (p6 * P + p7) * P + p8;
          const double v = fresh ? (double)E : (double)E + d[l];
          d[l] = v;
          if (v > bv) { bv = v; bi = q * NLEAF + l; }      // ascending within the thread: the first of equals stays
        });
    }
    sp_block_argmax(bv, bi, rd, ri, tid);
  };

  double mprev = 0.0;
  bool fresh = true;
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    const int* cn = cnt[cur];
    const int* cp = cnt[cur ^ 1];
    __syncthreads();      // the frame before is done with the tables
    pose_tables_stage(V, M, count, (int)(f0 + t), P, Vs, Ms, cnt[cur], tid, kSpThreads);
    if (tid < kPdK * P * P) {
      const int j = tid / (P * P), r = tid - j * (P * P);
      taus[j][r / P][r % P] = t > 0 ? tau[((f0 + t) * kPdK + j) * (P * P) + r] : 0.0;
    }
    __syncthreads();
    bool pose = true;
#pragma unroll
    for (int j = 0; j < kPdK; ++j) pose &= cn[j] > 0;
    double m = 0.0;
    int arg = -1, brk = 0, st = 1;
    if (!pose) {
      brk = 2;
      st = 2;
    } else {
      if (!fresh) {
        st = 0;
        uint8_t* ba = bpa + (size_t)t * N;
        uint16_t* bb = bpb + (size_t)t * N;
        for (int c0 = 0; c0 < L; c0 += C) {      // passes 0 .. 3
          for (int i = tid; i < MID * C; i += kSpThreads) {
            tile[i] = plane[(size_t)(i / C) * L + c0 + i % C] - mprev;
            bpt[i] = 0;
          }
          __syncthreads();
          sp_passes<P, 0, 3, 3, C>(tile, bpt, MID * C, taus, cp, cn, tid);
          for (int i = tid; i < MID * C; i += kSpThreads) {
            const size_t at = (size_t)(i / C) * L + c0 + i % C;
            plane[at] = tile[i];
            ba[at] = (uint8_t)bpt[i];
          }
        }
        __syncthreads();      // every tile of passes 0 .. 3 is in memory
        for (int h0 = 0; h0 < MID; h0 += TB) {      // passes 4 .. 8
          const size_t at0 = (size_t)h0 * L;
          for (int i = tid; i < TB * L; i += kSpThreads) {
            tile[i] = plane[at0 + i];
            bpt[i] = 0;
          }
          __syncthreads();
          sp_passes<P, 4, 8, 8, 1>(tile, bpt, TB * L, taus, cp, cn, tid);
          for (int i = tid; i < TB * L; i += kSpThreads) {
            plane[at0 + i] = tile[i];
            bb[at0 + i] = bpt[i];
          }
        }
        __syncthreads();
      }
      int bi;
      scores(cn, fresh, m, bi);
      if (!fresh && m == -INFINITY) {      // no connection to the frame before (thread-uniform: m is)
        __syncthreads();
        scores(cn, true, m, bi);
        brk = 1;
        st = 1;
      }
      arg = bi == kSpNone ? -1 : bi;
    }
    if (tid == 0) {
      amax[t] = arg;
      start[t] = st;
      if (maxes) maxes[f0 + t] = m;
      if (breaks) breaks[f0 + t] = brk;
    }
    mprev = m;
    fresh = !pose;
  }
  __syncthreads();

  // the walk back, one thread: amax[t] becomes the state of frame t on the best path
  if (tid == 0) {
    int state = -1;
    for (int t = T - 1; t >= 0; --t) {
      const int st = start[t];
      const bool last = t == T - 1 || start[t + 1] != 0;      // the segment ends here: its own arg-max
      if (st == 2) { state = -1; continue; }
      if (last) state = amax[t];
      amax[t] = state;
      if (st == 0 && state >= 0) {      // a_8 from pass 8's pointer at (b_0 .. b_8), a_7 from pass 7's at (b_0 .. b_7, a_8), .. a_0
        const uint8_t* ba = bpa + (size_t)t * N;
        const uint16_t* bb = bpb + (size_t)t * N;
#pragma unroll
        for (int j = kPdK - 1; j >= 0; --j) {
          const int sj = sp_pow(P, kPdK - 1 - j);
          const int a = j >= 4 ? (bb[state] >> (2 * (j - 4))) & 3 : (ba[state] >> (2 * j)) & 3;
          state += (a - (state / sj) % P) * sj;
        }
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < T; t += kSpThreads) {
    const int state = start[t] == 2 ? -1 : amax[t];      // -1 also where every score was -inf, which is outside the contract
    const size_t f = f0 + t;
    int p[kPdK];
    int r = max(state, 0);
#pragma unroll
    for (int j = kPdK - 1; j >= 0; --j) {
      p[j] = r % P;
      r /= P;
    }
#pragma unroll
    for (int j = 0; j < kPdK; ++j) {
      index[f * kPdK + j] = state < 0 ? -1 : p[j];
      if (coords) {
        const int32_t* cl = cells + ((f * kPdK + j) * P + p[j]) * 2;
        coords[(f * 2 + 0) * kPdK + j] = state < 0 ? -1 : cl[0];
        coords[(f * 2 + 1) * kPdK + j] = state < 0 ? -1 : cl[1];
      }
    }
    if (frame_score) frame_score[f] = state < 0 ? -INFINITY : pose_score_of(V + f * kPdK * P, M + f * kPdPairs * P * P, P, p);
  }
}

}  // namespace

size_t seq_pose_states(int P) { return (size_t)sp_pow(P, 9); }      // P^9: 8 bytes of plane per clip and state, 1 + 2 bytes of pointers per frame and state

hipError_t seq_pose_viterbi(const float* V, const float* M, const int32_t* count, const int32_t* cells, const double* tau, int S, int T, int P, double* plane,
                            uint8_t* bpa, uint16_t* bpb, int32_t* amax, int32_t* start, int32_t* index, int32_t* coords, float* frame_score, double* maxes,
                            int32_t* breaks, hipStream_t st) {
  if (S < 1 || T < 1 || P < 1 || P > kPdMaxP) return hipErrorInvalidValue;
#define JCM_SP_LAUNCH(PV)                                                                                                                              \
  hipLaunchKernelGGL(seq_pose_kernel<PV>, dim3(S), dim3(kSpThreads), 0, st, V, M, count, cells, tau, T, plane, bpa, bpb, amax, start, index, coords, \
                     frame_score, maxes, breaks)
  switch (P) {
    case 1: JCM_SP_LAUNCH(1); break;
    case 2: JCM_SP_LAUNCH(2); break;
    case 3: JCM_SP_LAUNCH(3); break;
    default: JCM_SP_LAUNCH(4); break;
  }
#undef JCM_SP_LAUNCH
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_seq_pose_viterbi(jcm_handle h, const float* V, const float* M, const int32_t* count, const int32_t* cells, const double* tau, int S, int T, int P,
                         int32_t* index, int32_t* coords, float* frame_score, double* maxes, int32_t* breaks) {
  const std::string w("seq_pose_viterbi");
  JCM_TRY(check(h, false));
  if (P < 1 || P > kPdMaxP) return fail(JCM_ERR_ARG, w + ": P = " + std::to_string(P) + " candidates per joint; 1 <= P <= 4");
  if (S < 1 || T < 1 || (double)S * (double)T >= 2147483648.0)
    return fail(JCM_ERR_ARG, w + ": bad clip sizes S = " + std::to_string(S) + ", T = " + std::to_string(T) + " (S, T >= 1, S * T < 2^31)");
  if (!V || !M || !count || !cells || !tau || !index)
    return fail(JCM_ERR_ARG, w + ": null pointer (V, M, count, cells, tau and index are required; coords, frame_score, maxes and breaks may be NULL)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  // per clip one float64 plane of P^9 states; per frame 3 bytes of back-pointers per state and two words; refused as jcm_seq_viterbi refuses
  const double N = (double)seq_pose_states(P);
  JCM_TRY(workspace_or_refuse(h, w, (double)S * N * 8.0 + (double)S * T * (N * 3.0 + 8.0) + 8192.0, "plane and back-pointers", S, T));
  double* plane = nullptr;
  uint8_t* bpa = nullptr;
  uint16_t* bpb = nullptr;
  int32_t *amax = nullptr, *start = nullptr;
  jcm_ctx* c = h;
  return arena_launch(c, w, [&] {
    plane = arena_alloc<double>(c, (size_t)S * (size_t)N);
    bpb = arena_alloc<uint16_t>(c, (size_t)S * T * (size_t)N);
    bpa = arena_alloc<uint8_t>(c, (size_t)S * T * (size_t)N);
    amax = arena_alloc<int32_t>(c, (size_t)S * T);
    start = arena_alloc<int32_t>(c, (size_t)S * T);
  }, [&] { return seq_pose_viterbi(V, M, count, cells, tau, S, T, P, plane, bpa, bpb, amax, start, index, coords, frame_score, maxes, breaks, c->stream); });
}

}  // extern "C"
