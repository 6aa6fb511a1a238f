// Pose decoding: of the P <= 4 candidate cells per joint that jcm_hm_peaks returns, the ONE combination (p_0 .. p_8) with the highest
// spatial-model energy -- a joint MAP over P^9 poses in place of nine independent arg-maxes.  Three small launches:
//   pose_tables_kernel, one work group per image: the torso cell (first-occurrence arg-max of channel 9), the likelihood u_c at the 9 P candidate cells
//     and at the torso cell (smf::lik_of, the expression of the spatial-model forward), the 72 P^2 pair terms T[j,c,pj,pc] in LDS (one scattered read of
//     sp_energy and one of sp_bias each), then V [9][P] and M [36][P][P] = T[a,b] + T[b,a]^T to memory;
//   pose_search_kernel, 16 work groups per image: V and M in LDS at a pitch of 4 (2.4 KB).  The score is a fixed-order sum whose partial sum S_k depends on
//     the PREFIX p_0 .. p_k only, so the prefix is what is dealt out: the work group fixes (p_0, p_1), the thread (p_2 .. p_5), and the thread walks
//     (p_6, p_7, p_8) depth-first with S_5, S_6, S_7 in registers.  The part of inc_6, inc_7, inc_8 that the fixed prefix decides (V[k,q] + M[0,k,p_0,q] +
//     .. + M[5,k,p_5,q], the first terms of the sum, in its order) is formed once per thread for the 4 values of q, so a leaf costs 3 additions and a
//     comparison.  p_2 is the wave number: a wave whose slot is at or beyond count leaves at once.  Arg-max by (score descending, pose number ascending;
//     the pose number has p_0 in its top digits, so the lower number is the lexicographically smaller pose): shuffles in the wave, 4 slots of LDS across;
//   pose_finish_kernel, one wave per image: the best of the 16 partial winners by the same rule, index / coords / score, and score0 by one lane.
// LDS reads of M: the lanes of a wave differ in (p_3, p_4, p_5) only, so a read M[a,k,p_a,q] touches at most 4 addresses 4 floats apart (distinct banks,
// the rest broadcasts); the reads of the depth-first walk are wave-uniform.  No atomics; every store is a vector store of plain C++.
#include <string>

#include "entry.h"
#include "pose_score.h"
#include "sm_lds_fft.h"

namespace jcm {

namespace {

// kPdK, kPdPairs, kPdMaxP, pd_pair, pd_count and the score itself: pose_score.h, shared with seq_pose.hip
constexpr int kPdPJ = kC - 1;                  // pairs per joint in sp_energy / sp_bias: <j>_<c>, c in name order without j
constexpr int kPdThreads = 256;
constexpr int kPdGroups = kPdMaxP * kPdMaxP;   // work groups per image of the search: (p_0, p_1)
constexpr float kPdDelta = 1e-6f;              // main.py:110
constexpr int kPdNone = 0x7fffffff;

__device__ __forceinline__ int pd_row(int j, int c) { return j * kPdPJ + (c < j ? c : c - 1); }          // the row of pair <j>_<c> in sp_energy / sp_bias
__device__ __forceinline__ bool pd_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__global__ __launch_bounds__(kPdThreads) void pose_tables_kernel(const float* __restrict__ hm10, const int32_t* __restrict__ cells, const int32_t* __restrict__ count,
                                                                 int P, const float* __restrict__ spe, const float* __restrict__ spb,
                                                                 const float* __restrict__ sc, const float* __restrict__ sh, float* __restrict__ V,
                                                                 float* __restrict__ M) {
  __shared__ float rv[kPdThreads / 64];
  __shared__ int ri[kPdThreads / 64];
  __shared__ int cy[kPdK][kPdMaxP], cx[kPdK][kPdMaxP], cnt[kPdK];
  __shared__ float u[kPdK][kPdMaxP];
  __shared__ float T[kPdK][kPdK][kPdMaxP][kPdMaxP];
  __shared__ int tcell;
  __shared__ float ut;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t pix0 = (int64_t)b * kHmHW;

  // the torso cell: first-occurrence flat arg-max of channel 9 (the rules of argmax_kernel, glue.hip)
  float bv = -INFINITY;
  int bi = kPdNone;
  for (int p = tid; p < kHmHW; p += kPdThreads) {
    const float v = hm10[(pix0 + p) * kC + kPdK];
    if (pd_better(v, p, bv, bi)) { bv = v; bi = p; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (pd_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { rv[tid >> 6] = bv; ri[tid >> 6] = bi; }
  // the candidates: cells of slots below count, clamped into the map for the reads (a cell outside it is outside the contract)
  if (tid < kPdK * kPdMaxP) {
    const int j = tid >> 2, p = tid & 3, n = pd_count(count, b, j, P);
    int y = 0, x = 0;
    float uv = 0.f;
    if (p < n) {
      const int32_t* cl = cells + ((size_t)(b * kPdK + j) * P + p) * 2;
      y = min(max(cl[0], 0), kHmH - 1);
      x = min(max(cl[1], 0), kHmW - 1);
      uv = smf::lik_of(hm10, kC, nullptr, 0, sc, sh, pix0 + y * kHmW + x, j);
    }
    cy[j][p] = y; cx[j][p] = x; u[j][p] = uv;
    if (p == 0) cnt[j] = n;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kPdThreads / 64; ++w)
      if (pd_better(rv[w], ri[w], bv, bi)) { bv = rv[w]; bi = ri[w]; }
    if (bi == kPdNone) bi = 0;
    tcell = bi;
    ut = smf::lik_of(hm10, kC, nullptr, 0, sc, sh, pix0 + bi, kPdK);
  }
  __syncthreads();

  // T[j,c,pj,pc] = log(e_{j|c}[59 + yj - yc, 89 + xj - xc] * u_c + b_{j|c}[yj, xj] + d); slots at or beyond count: 0
  for (int i = tid; i < kPdK * kPdK * kPdMaxP * kPdMaxP; i += kPdThreads) {
    const int pc = i & 3, pj = (i >> 2) & 3, jc = i >> 4, j = jc / kPdK, c = jc - j * kPdK;
    float t = 0.f;
    if (j != c && pj < cnt[j] && pc < cnt[c]) {
      const int yj = cy[j][pj], xj = cx[j][pj];
      const int row = pd_row(j, c);
      const float e = spe[(size_t)row * (kPrH * kPrW) + (kHmH - 1 + yj - cy[c][pc]) * kPrW + (kHmW - 1 + xj - cx[c][pc])];
      const float bs = spb[(size_t)row * kHmHW + yj * kHmW + xj];
      t = logf((e * u[c][pc] + bs) + kPdDelta);
    }
    T[j][c][pj][pc] = t;
  }
  __syncthreads();

  const int PP = P * P;
  for (int i = tid; i < kPdPairs * PP; i += kPdThreads) {
    const int pr = i / PP, q = i - pr * PP, pa = q / P, pb = q - pa * P;
    int a = 0, r = pr;
    while (r >= kPdK - 1 - a) { r -= kPdK - 1 - a; ++a; }
    const int bb = a + 1 + r;
    M[(size_t)b * kPdPairs * PP + i] = (pa < cnt[a] && pb < cnt[bb]) ? T[a][bb][pa][pb] + T[bb][a][pb][pa] : 0.f;
  }
  if (tid < kPdK * P) {
    const int j = tid / P, p = tid - j * P;
    float v = 0.f;
    if (p < cnt[j]) {
      const int yj = cy[j][p], xj = cx[j][p], ty = tcell / kHmW, tx = tcell - ty * kHmW;
      const int row = pd_row(j, kPdK);
      const float e = spe[(size_t)row * (kPrH * kPrW) + (kHmH - 1 + yj - ty) * kPrW + (kHmW - 1 + xj - tx)];
      const float bs = spb[(size_t)row * kHmHW + yj * kHmW + xj];
      v = logf(u[j][p] + kPdDelta) + logf((e * ut + bs) + kPdDelta);
    }
    V[(size_t)b * kPdK * P + tid] = v;
  }
}

__global__ __launch_bounds__(kPdThreads) void pose_search_kernel(const float* __restrict__ V, const float* __restrict__ M, const int32_t* __restrict__ count, int P,
                                                                 float* __restrict__ pscore, int32_t* __restrict__ ppose) {
  __shared__ float Vs[kPdK][kPdMaxP];
  __shared__ float Ms[kPdPairs][kPdMaxP][kPdMaxP];
  __shared__ int cnt[kPdK];
  __shared__ float rv[kPdThreads / 64];
  __shared__ int ri[kPdThreads / 64];
  const int b = blockIdx.x / kPdGroups, g = blockIdx.x - b * kPdGroups, tid = threadIdx.x;
  pose_tables_stage(V, M, count, b, P, Vs, Ms, cnt, tid, kPdThreads);
  __syncthreads();

  const int p[6] = {g >> 2, g & 3, tid >> 6, (tid >> 4) & 3, (tid >> 2) & 3, tid & 3};
  bool live = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) live &= p[k] < cnt[k];
  float bv = -INFINITY;
  int bi = kPdNone;
  if (live) {
    const int n5 = (g << 14) | (tid << 6);      // pose number: 2 bits per joint, p_0 on top
    pose_walk(Vs, Ms, cnt, p, [&](int p6, int p7, int p8, float S8) {
      const int n = n5 | (p6 << 4) | (p7 << 2) | p8;
      if (pd_better(S8, n, bv, bi)) { bv = S8; bi = n; }
    });
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (pd_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { rv[tid >> 6] = bv; ri[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kPdThreads / 64; ++w)
      if (pd_better(rv[w], ri[w], bv, bi)) { bv = rv[w]; bi = ri[w]; }
    pscore[blockIdx.x] = bv;
    ppose[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(64) void pose_finish_kernel(const float* __restrict__ pscore, const int32_t* __restrict__ ppose, const float* __restrict__ V,
                                                         const float* __restrict__ M, const int32_t* __restrict__ cells, const int32_t* __restrict__ count, int P,
                                                         int32_t* __restrict__ index, int32_t* __restrict__ coords, float* __restrict__ score,
                                                         float* __restrict__ score0) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float bv = lane < kPdGroups ? pscore[b * kPdGroups + lane] : -INFINITY;
  int bi = lane < kPdGroups ? ppose[b * kPdGroups + lane] : kPdNone;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (pd_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  const bool none = bi == kPdNone;      // some count is 0: no pose
  if (lane < kPdK) {
    const int pj = none ? -1 : (bi >> (2 * (kPdK - 1 - lane))) & 3;
    index[b * kPdK + lane] = pj;
    if (coords) {
      const int32_t* cl = cells + ((size_t)(b * kPdK + lane) * P + max(pj, 0)) * 2;
      coords[(b * 2 + 0) * kPdK + lane] = none ? -1 : cl[0];
      coords[(b * 2 + 1) * kPdK + lane] = none ? -1 : cl[1];
    }
  }
  if (lane == kPdK && score) score[b] = none ? -INFINITY : bv;
  if (lane == kPdK + 1 && score0) {      // the all-peak-0 pose, the same sum
    float S = -INFINITY;
    if (!none) {
      const int zero[kPdK] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      S = pose_score_of(V + (size_t)b * kPdK * P, M + (size_t)b * kPdPairs * P * P, P, zero);
    }
    score0[b] = S;
  }
}

}  // namespace

hipError_t pose_decode(const float* hm10, int B, const int32_t* cells, const int32_t* count, int P, const float* sp_energy, const float* sp_bias,
                       const float* bn_scale, const float* bn_shift, float* V, float* M, float* pscore, int32_t* ppose, int32_t* index, int32_t* coords,
                       float* score, float* score0, hipStream_t st) {
  if (B < 1 || B > kPoseMaxB || P < 1 || P > kPdMaxP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pose_tables_kernel, dim3(B), dim3(kPdThreads), 0, st, hm10, cells, count, P, sp_energy, sp_bias, bn_scale, bn_shift, V, M);
  hipLaunchKernelGGL(pose_search_kernel, dim3(B * kPdGroups), dim3(kPdThreads), 0, st, V, M, count, P, pscore, ppose);
  hipLaunchKernelGGL(pose_finish_kernel, dim3(B), dim3(64), 0, st, pscore, ppose, V, M, cells, count, P, index, coords, score, score0);
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_pose_decode(jcm_handle h, const float* hm10, int B, const int32_t* cells, const int32_t* count, int P, int32_t* index, int32_t* coords, float* score,
                    float* score0, float* V, float* M) {
  JCM_TRY(check(h, true));
  if (P < 1 || P > kPdMaxP) return fail(JCM_ERR_ARG, "pose_decode: P = " + std::to_string(P) + " candidates per joint; 1 <= P <= 4");
  if (B < 1 || B > kPoseMaxB) return fail(JCM_ERR_ARG, "pose_decode: bad batch size (1 <= B <= " + std::to_string(kPoseMaxB) + ")");
  if (!hm10 || !cells || !count || !index) return fail(JCM_ERR_ARG, "pose_decode: null pointer (hm10, cells, count and index are required; coords, score, score0, V and M may be NULL)");
  if (!h->has_sm || h->K != kPdK) return fail(JCM_ERR_STATE, "pose_decode: the handle holds no spatial-model parameters for 9 joints");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  float *v = V, *m = M, *pscore = nullptr;
  int32_t* ppose = nullptr;
  return arena_launch(c, "pose_decode", [&] {
    if (!V) v = arena_alloc<float>(c, (size_t)B * kPdK * P);
    if (!M) m = arena_alloc<float>(c, (size_t)B * kPdPairs * P * P);
    pscore = arena_alloc<float>(c, (size_t)B * kPdGroups);
    ppose = arena_alloc<int32_t>(c, (size_t)B * kPdGroups);
  }, [&] {
    return pose_decode(hm10, B, cells, count, P, c->sp_energy, c->sp_bias, c->bn_sm_scale, c->bn_sm_shift, v, m, pscore, ppose, index, coords, score, score0,
                       c->stream);
  });
}

}  // extern "C"
