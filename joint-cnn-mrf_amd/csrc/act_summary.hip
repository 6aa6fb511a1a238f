// The per-layer activation summaries of conv_layer (main.py:167-168) in ONE pass over the pre-activation z = conv + b
// [B,H,W,C]: per tower slice (a group of B / n_groups consecutive images) the statistics of tf.summary.histogram / var_summary, the
// activation BN(relu(z)) with the layer's folded inference-mode BatchNorm, and channel pic_channel of the first n_pics activations of
// every slice (the pictures of tf.summary.image('f_activ_' + name, activ[:, :, :, 7:8], 3)).
// Statistics: summary_stats.h -- LDS sub-histograms and integer atomics for the counts, fixed-order folds in double for the sums, so a
// repeated call returns the same bytes.  A work group owns kActChunk consecutive elements of one slice: the grid follows the tensor.
#include <cstdint>

#include "entry.h"
#include "summary_stats.h"

namespace jcm {

namespace {

constexpr int kActChunk = 32768;      // elements per work group (a multiple of 4)

struct ActArgs {
  const float* z;
  const float* scale;      // folded BatchNorm of the layer, or null (a linear layer: activ = z)
  const float* shift;
  float* activ;            // may be null
  float* pics;             // [n_groups][n_pics][H*W], or null (n_pics == 0)
  long long group_elems;   // (B / n_groups) * H * W * C
  unsigned HWC, C, HW;
  int pic_channel, n_pics;
};

// tf.nn.relu keeps a NaN (Eigen's cwiseMax(x, 0) returns x when the comparison fails), then BatchNorm as two rounded operations
__device__ __forceinline__ float activation(float v, const ActArgs& a, unsigned c) {
  if (!a.scale) return v;
  const float r = v > 0.f ? v : (v == v ? 0.f : v);
  return __fadd_rn(__fmul_rn(r, a.scale[c]), a.shift[c]);
}

// VEC: C % 4 == 0 and 16-byte aligned tensors -- a float4 never straddles a pixel; otherwise one element per lane and step
template <bool VEC>
__global__ __launch_bounds__(kStatsThreads) void act_summary_kernel(ActArgs a, const double* __restrict__ limits, Part* __restrict__ parts,
                                                                    unsigned long long* __restrict__ counts) {
  __shared__ StatsLds L;
  const int t = threadIdx.x;
  stats_lds_init(L, limits);
  const int g = blockIdx.y;
  const long long o0 = (long long)blockIdx.x * kActChunk;            // first element of this chunk inside the slice
  const long long left = a.group_elems - o0;
  const int n = left < kActChunk ? (int)left : kActChunk;
  const long long base = (long long)g * a.group_elems + o0;         // ... inside the tensor
  const unsigned img0 = (unsigned)(o0 / a.HWC), r0 = (unsigned)(o0 % a.HWC);
  const float* __restrict__ zp = a.z + base;
  float* __restrict__ ap = a.activ ? a.activ + base : nullptr;
  float* __restrict__ pp = a.pics ? a.pics + (size_t)g * a.n_pics * a.HW : nullptr;
  __syncthreads();
  StatsAcc A;
  constexpr int V = VEC ? 4 : 1;
  for (int i = t * V; i < n; i += kStatsThreads * V) {
    const unsigned r = r0 + (unsigned)i;                             // < HWC + kActChunk < 2^31
    const unsigned img = img0 + r / a.HWC, rr = r % a.HWC;
    const unsigned pix = rr / a.C, c = rr - pix * a.C;
    float v[V], o[V];
    if constexpr (VEC) {
      const float4 q = *reinterpret_cast<const float4*>(zp + i);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = zp[i];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      A.add(v[j], L);
      o[j] = activation(v[j], a, c + j);
      if (pp && (int)(c + j) == a.pic_channel && img < (unsigned)a.n_pics) pp[(size_t)img * a.HW + pix] = o[j];
    }
    if (ap) {
      if constexpr (VEC) *reinterpret_cast<float4*>(ap + i) = make_float4(o[0], o[1], o[2], o[3]);
      else ap[i] = o[0];
    }
  }
  stats_block_finish(A, L, parts + (size_t)g * gridDim.x + blockIdx.x, counts + (size_t)g * (3 + JCM_HIST_BUCKETS) + 3);
}

}  // namespace

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_act_summary(jcm_handle h, const char* scope, const float* z, int B, int H, int W, int C, int n_groups, int pic_channel, int n_pics,
                    float* activ_out, double* stats, int64_t* counts, float* pics_out) {
  JCM_TRY(check(h, true));
  if (!scope || !z || !stats || !counts || B < 1 || H < 1 || W < 1 || C < 1) return fail(JCM_ERR_ARG, "bad act_summary arguments");
  if (n_groups < 1 || n_groups > 65535) return fail(JCM_ERR_ARG, "act_summary: n_groups must be 1 .. 65535, got " + std::to_string(n_groups));
  if (B < n_groups) return fail(JCM_ERR_ARG, "act_summary: " + std::to_string(B) + " images do not fill " + std::to_string(n_groups) + " groups");
  if (pic_channel < 0 || pic_channel >= C)
    return fail(JCM_ERR_ARG, "act_summary: pic_channel " + std::to_string(pic_channel) + " outside the " + std::to_string(C) + " channels");
  const int G = B / n_groups;      // images per group; the B % n_groups trailing images are left out (the reference's tower loop)
  if (n_pics < 0 || n_pics > G)
    return fail(JCM_ERR_ARG, "act_summary: n_pics " + std::to_string(n_pics) + " exceeds the " + std::to_string(G) + " images of a group");
  if (n_pics > 0 && !pics_out) return fail(JCM_ERR_ARG, "act_summary: n_pics > 0 needs pics_out");
  const int64_t HWC = (int64_t)H * W * C;
  if (HWC >= ((int64_t)1 << 30) || G * HWC >= ((int64_t)1 << 40)) return fail(JCM_ERR_ARG, "act_summary: tensor too large");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const ConvLayer* L = conv_of(c, scope);
  if (!L) return fail(JCM_ERR_STATE, std::string("no conv layer '") + scope + "'");
  if (C != L->cout) return fail(JCM_ERR_ARG, std::string("act_summary: layer '") + scope + "' has " + std::to_string(L->cout) + " output channels, C = " + std::to_string(C));
  if (L->has_bn && (!L->scale || !L->shift)) return fail(JCM_ERR_STATE, std::string("act_summary: no folded BatchNorm for '") + scope + "'");
  const int64_t nck = (G * HWC + kActChunk - 1) / kActChunk;
  if (nck >= ((int64_t)1 << 31) || nck * n_groups >= ((int64_t)1 << 31)) return fail(JCM_ERR_ARG, "act_summary: tensor too large");
  JCM_TRY(hist_limits_dev(c));
  ActArgs a;
  a.z = z;
  a.scale = L->has_bn ? L->scale : nullptr;
  a.shift = L->has_bn ? L->shift : nullptr;
  a.activ = activ_out;
  a.pics = n_pics > 0 ? pics_out : nullptr;
  a.group_elems = G * HWC;
  a.HWC = (unsigned)HWC;
  a.C = (unsigned)C;
  a.HW = (unsigned)(H * W);
  a.pic_channel = pic_channel;
  a.n_pics = n_pics;
  const bool vec = C % 4 == 0 && reinterpret_cast<uintptr_t>(z) % 16 == 0 && reinterpret_cast<uintptr_t>(activ_out) % 16 == 0;
  return with_arena(c, [&] {
    Part* parts = arena_alloc<Part>(c, (size_t)nck * n_groups);
    if (c->dry) return (int)JCM_OK;
    auto* cnt = reinterpret_cast<unsigned long long*>(counts);
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_groups * (3 + JCM_HIST_BUCKETS) * sizeof(int64_t), c->stream));
    return timed_launch(c, std::string(scope) + "/act_summary", [&] {
      const dim3 grid((unsigned)nck, (unsigned)n_groups);
      if (vec) hipLaunchKernelGGL(act_summary_kernel<true>, grid, dim3(kStatsThreads), 0, c->stream, a, c->hist_limits, parts, cnt);
      else hipLaunchKernelGGL(act_summary_kernel<false>, grid, dim3(kStatsThreads), 0, c->stream, a, c->hist_limits, parts, cnt);
      hipLaunchKernelGGL(stats_fold_kernel, dim3(n_groups), dim3(kStatsThreads), 0, c->stream, parts, static_cast<const int*>(nullptr), (int)nck, stats, cnt);
      return hipGetLastError();
    });
  });
}

int jcm_bn_folded(jcm_handle h, const char* scope, float* scale_out, float* shift_out, int count) {
  JCM_TRY(check(h, true));
  if (!scope || !scale_out || !shift_out) return fail(JCM_ERR_ARG, "bad bn_folded arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  const ConvLayer* L = conv_of(h, scope);
  if (!L) return fail(JCM_ERR_STATE, std::string("no conv layer '") + scope + "'");
  if (!L->has_bn || !L->scale || !L->shift) return fail(JCM_ERR_ARG, std::string("bn_folded: layer '") + scope + "' has no BatchNorm");
  if (count != L->cout) return fail(JCM_ERR_ARG, std::string("bn_folded: layer '") + scope + "' has " + std::to_string(L->cout) + " channels, count = " + std::to_string(count));
  HIP_TRY(hipMemcpyAsync(scale_out, L->scale, (size_t)count * sizeof(float), hipMemcpyDefault, h->stream));
  HIP_TRY(hipMemcpyAsync(shift_out, L->shift, (size_t)count * sizeof(float), hipMemcpyDefault, h->stream));
  order.release();
  HIP_TRY(hipStreamSynchronize(h->stream));      // the outputs may be host memory
  return JCM_OK;
}

}  // extern "C"
