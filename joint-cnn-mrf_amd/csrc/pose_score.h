// The score of a pose (include/jcm.h: jcm_pose_decode): ONE copy of the fixed-order fp32 sum S_8 over V [9][P] and M [36][P][P], for
// the two kernels that evaluate it for every pose -- pose_search_kernel (pose_decode.hip), which keeps the best, and seq_pose_kernel (seq_pose.hip,
// DESIGN.md 4.30), which keeps them all -- and for the one-pose form pose_finish_kernel and the clip decode report.  Device code only.
//   S_0 = V[0,p_0];  inc_k = (((V[k,p_k] + M[0,k,p_0,p_k]) + M[1,k,p_1,p_k]) + ..) + M[k-1,k,p_{k-1},p_k];  S_k = S_{k-1} + inc_k
// The tables are read from LDS at a pitch of 4 (pose_tables_stage fills them); slots at or beyond P hold 0 and are never added.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace jcm {

constexpr int kPdK = 9;                              // joints
constexpr int kPdPairs = kPdK * (kPdK - 1) / 2;      // 36 unordered joint pairs (a < b), lexicographic
constexpr int kPdMaxP = 4;

__host__ __device__ constexpr int pd_pair(int a, int b) { return a * (17 - a) / 2 + (b - a - 1); }      // a < b
__device__ __forceinline__ int pd_count(const int32_t* __restrict__ count, int b, int j, int P) { return min(max(count[(size_t)b * kPdK + j], 0), P); }

// V [9][P] and M [36][P][P] of image b -> Vs, Ms at a pitch of 4, and the clamped counts; the caller's barrier follows
__device__ __forceinline__ void pose_tables_stage(const float* __restrict__ V, const float* __restrict__ M, const int32_t* __restrict__ count, int b, int P,
                                                  float (*Vs)[kPdMaxP], float (*Ms)[kPdMaxP][kPdMaxP], int* cnt, int tid, int threads) {
  const int PP = P * P;
  for (int i = tid; i < kPdPairs * kPdMaxP * kPdMaxP; i += threads) {
    const int pb = i & 3, pa = (i >> 2) & 3, pr = i >> 4;
    Ms[pr][pa][pb] = (pa < P && pb < P) ? M[((size_t)b * kPdPairs + pr) * PP + pa * P + pb] : 0.f;
  }
  if (tid < kPdK * kPdMaxP) {
    const int j = tid >> 2, p = tid & 3;
    Vs[j][p] = p < P ? V[((size_t)b * kPdK + j) * P + p] : 0.f;
    if (p == 0) cnt[j] = pd_count(count, b, j, P);
  }
}

// Every pose (p_0 .. p_5, p_6, p_7, p_8) with the given prefix and p_6 < cnt[6], p_7 < cnt[7], p_8 < cnt[8], depth-first in ascending order:
// leaf(p_6, p_7, p_8, S_8).  S_5 and the part of inc_6, inc_7, inc_8 that the prefix decides (the first terms of the sum, in its order) are formed
// once, so a leaf costs 3 additions.  The prefix must be below its counts.
template <class Leaf>
__device__ __forceinline__ void pose_walk(const float (*Vs)[kPdMaxP], const float (*Ms)[kPdMaxP][kPdMaxP], const int* cnt, const int (&p)[6], Leaf&& leaf) {
  float S = Vs[0][p[0]];      // S_0
#pragma unroll
  for (int k = 1; k < 6; ++k) {
    float inc = Vs[k][p[k]];
#pragma unroll
    for (int a = 0; a < k; ++a) inc = inc + Ms[pd_pair(a, k)][p[a]][p[k]];
    S = S + inc;              // S_k
  }
  float base[3][kPdMaxP];      // the first terms of inc_6, inc_7, inc_8: V and the pairs with the fixed joints 0 .. 5
#pragma unroll
  for (int k = 6; k < kPdK; ++k)
#pragma unroll
    for (int q = 0; q < kPdMaxP; ++q) {
      float inc = Vs[k][q];
#pragma unroll
      for (int a = 0; a < 6; ++a) inc = inc + Ms[pd_pair(a, k)][p[a]][q];
      base[k - 6][q] = inc;
    }
  const int c6 = cnt[6], c7 = cnt[7], c8 = cnt[8];
#pragma unroll
  for (int p6 = 0; p6 < kPdMaxP; ++p6) {
    if (p6 >= c6) break;
    const float S6 = S + base[0][p6];
#pragma unroll
    for (int p7 = 0; p7 < kPdMaxP; ++p7) {
      if (p7 >= c7) break;
      const float S7 = S6 + (base[1][p7] + Ms[pd_pair(6, 7)][p6][p7]);
#pragma unroll
      for (int p8 = 0; p8 < kPdMaxP; ++p8) {
        if (p8 >= c8) break;
        const float S8 = S7 + ((base[2][p8] + Ms[pd_pair(6, 8)][p6][p8]) + Ms[pd_pair(7, 8)][p7][p8]);
        leaf(p6, p7, p8, S8);
      }
    }
  }
}

// S_8 of ONE pose from the tables in memory (v [9][P], m [36][P][P] of its image), by one lane: the same sum
__device__ __forceinline__ float pose_score_of(const float* __restrict__ v, const float* __restrict__ m, int P, const int* p) {
  const int PP = P * P;
  float S = v[p[0]];
  for (int k = 1; k < kPdK; ++k) {
    float inc = v[k * P + p[k]];
    for (int a = 0; a < k; ++a) inc = inc + m[pd_pair(a, k) * PP + p[a] * P + p[k]];
    S = S + inc;
  }
  return S;
}

}  // namespace jcm
