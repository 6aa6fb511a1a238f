// TensorBoard summaries on the device (tensorboard.py): segmented tensor statistics with TF-1.x histograms,
// the heat-map overlays of show_img_plus_hm (tensorboard.py:60-71) and TF-1.x's float-image quantiser (summary_image_op.cc,
// NormalizeFloatImage).  Sums are fixed-order folds in double, min / max are order-free, and only the integer bucket counts
// use atomics: every result is bitwise the same from call to call.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "resize_tf1.h"
#include "summary_stats.h"

namespace jcm {

namespace {

constexpr int kChunk = 32768;                       // elements per work group of the statistics pass
constexpr int kImgThreads = 256;

struct Chunk {
  const float* p;
  int n;
  int seg;
};

__device__ __forceinline__ float stats_scale(float scale, float clip, const double* __restrict__ sumsq) {
  if (!sumsq) return scale;
  const float norm = (float)sqrt(*sumsq);     // the factor of the optimizer kernels (train_kernels.hip, tf.clip_by_global_norm)
  return clip / fmaxf(norm, clip);
}

// one work group per chunk: partial min / max / sums / counts and the chunk's histogram (one LDS sub-histogram per wave),
// whose nonzero bins are added to the segment's int64 counts (summary_stats.h)
__global__ __launch_bounds__(kStatsThreads) void stats_chunk_kernel(const Chunk* __restrict__ chunks, const double* __restrict__ limits,
                                                                    float scale, float clip, const double* __restrict__ sumsq,
                                                                    Part* __restrict__ parts, unsigned long long* __restrict__ counts) {
  __shared__ StatsLds L;
  const int t = threadIdx.x;
  stats_lds_init(L, limits);
  const Chunk ck = chunks[blockIdx.x];
  const float f = stats_scale(scale, clip, sumsq);
  __syncthreads();
  StatsAcc A;
  for (int i = t; i < ck.n; i += kStatsThreads) A.add(ck.p[i] * f, L);
  stats_block_finish(A, L, parts + blockIdx.x, counts + (size_t)ck.seg * (3 + JCM_HIST_BUCKETS) + 3);
}

// ---- images ---------------------------------------------------------------------------------------

// tf.minimum(a, 1) (Eigen's scalar min: b < a ? b : a -- a NaN stays NaN)
__device__ __forceinline__ float min1(float a) { return 1.f < a ? 1.f : a; }

// block-wide min / max of (mn, mx); result valid in thread 0
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* smn, float* smx) {
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) {
    smn[t / 64] = mn;
    smx[t / 64] = mx;
  }
  __syncthreads();
  if (t == 0)
    for (int w = 1; w < kImgThreads / 64; ++w) {
      mn = fminf(mn, smn[w]);
      mx = fmaxf(mx, smx[w]);
    }
}

// per image: min / max over the finite pixels (a pixel with any non-finite channel is left out); partial per work group
__global__ __launch_bounds__(kImgThreads) void img_minmax_kernel(const float* __restrict__ x, int HW, int C, float2* __restrict__ part) {
  __shared__ float smn[kImgThreads / 64], smx[kImgThreads / 64];
  const int b = blockIdx.y;
  const int i = blockIdx.x * kImgThreads + threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  if (i < HW) {
    const float* px = x + ((size_t)b * HW + i) * C;
    bool fin = true;
    for (int c = 0; c < C; ++c) fin = fin && isfinite(px[c]);
    if (fin)
      for (int c = 0; c < C; ++c) {
        mn = fminf(mn, px[c]);
        mx = fmaxf(mx, px[c]);
      }
  }
  block_minmax(mn, mx, smn, smx);
  if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = make_float2(mn, mx);
}

// one work group per picture: fold its partials and pick NormalizeFloatImage's affine map -> (scale, offset)
__global__ __launch_bounds__(kImgThreads) void img_scale_kernel(const float2* __restrict__ part, int nblk, float2* __restrict__ so) {
  __shared__ float smn[kImgThreads / 64], smx[kImgThreads / 64];
  const int p = blockIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < nblk; i += kImgThreads) {
    const float2 v = part[(size_t)p * nblk + i];
    mn = fminf(mn, v.x);
    mx = fmaxf(mx, v.y);
  }
  block_minmax(mn, mx, smn, smx);
  if (threadIdx.x == 0) {
    const float kZero = 1e-6f;
    float scale, offset;
    if (mn < 0.f) {
      const float a = fabsf(mn), c = fabsf(mx);
      const float mv = a < c ? c : a;              // std::max
      scale = mv < kZero ? 0.f : 127.f / mv;
      offset = 128.f;
    } else {
      scale = mx < kZero ? 0.f : 255.f / mx;
      offset = 0.f;
    }
    so[p] = make_float2(scale, offset);
  }
}

__device__ __forceinline__ unsigned char quant(float v, float2 so) {
  const float q = v * so.x + so.y;                 // truncation, as Eigen's cast<uint8>
  return (unsigned char)(int)fminf(fmaxf(q, 0.f), 255.f);
}

__global__ __launch_bounds__(kImgThreads) void img_write_kernel(const float* __restrict__ x, int HW, int C, const float2* __restrict__ so,
                                                                unsigned char* __restrict__ out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kImgThreads + threadIdx.x;
  if (i >= HW) return;
  const float* px = x + ((size_t)b * HW + i) * C;
  unsigned char* o = out + ((size_t)b * HW + i) * C;
  bool fin = true;
  for (int c = 0; c < C; ++c) fin = fin && isfinite(px[c]);
  const float2 s = so[b];
  for (int c = 0; c < C; ++c) o[c] = fin ? quant(px[c], s) : (c == 0 ? 255 : 0);      // bad colour: red (255 for gray)
}

// ---- show_img_plus_hm ----
constexpr int kOvlJoints = 9, kOvlPics = kOvlJoints + 1;
// colorize (tensorboard.py:6-19), joints lsho lelb lwri rsho relb rwri lhip rhip nose: which of R, G, B carry the heat map
__constant__ unsigned char kColor[kOvlJoints][3] = {{0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {1, 0, 1}, {1, 0, 0}};

// per image: partial max of x [B, HW*3]
__global__ __launch_bounds__(kImgThreads) void ovl_xmax_kernel(const float* __restrict__ x, int n, float* __restrict__ part) {
  __shared__ float smn[kImgThreads / 64], smx[kImgThreads / 64];
  const int b = blockIdx.y;
  float mx = -INFINITY, mn = INFINITY;
  for (int i = blockIdx.x * kImgThreads + threadIdx.x; i < n; i += gridDim.x * kImgThreads) mx = fmaxf(mx, x[(size_t)b * n + i]);
  block_minmax(mn, mx, smn, smx);
  if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = mx;
}

// one work group per image: contrast_x = 1 / max(x) and contrast_hm[j] = 1 / max(hm[..., j]) -> cst [B][1 + 9]
__global__ __launch_bounds__(kImgThreads) void ovl_contrast_kernel(const float* __restrict__ xpart, int nxp, const float* __restrict__ hm, int hhw,
                                                                   float* __restrict__ cst) {
  __shared__ float smn[kImgThreads / 64], smx[kImgThreads / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = t; i < nxp; i += kImgThreads) mx = fmaxf(mx, xpart[(size_t)b * nxp + i]);
  block_minmax(mn, mx, smn, smx);
  if (t == 0) cst[b * kOvlPics] = 1.f / mx;
  for (int j = 0; j < kOvlJoints; ++j) {
    mn = INFINITY;
    mx = -INFINITY;
    for (int i = t; i < hhw; i += kImgThreads) mx = fmaxf(mx, hm[((size_t)b * hhw + i) * kOvlJoints + j]);
    block_minmax(mn, mx, smn, smx);
    if (t == 0) cst[b * kOvlPics + 1 + j] = 1.f / mx;
  }
}

struct OvlGeo {
  int H, W, hh, hw;
  float sy, sx;      // TF-1.x resize scales hh / H, hw / W
};

// the ten pictures of pixel i of image b: v[j] = min(x + c_j, 1) for the nine joints, v[9] = the all-joints picture
__device__ __forceinline__ void ovl_pixel(const float* __restrict__ x, const float* __restrict__ hm, const float* __restrict__ cst, const OvlGeo& G,
                                          int b, int i, float v[kOvlPics][3]) {
  const int r = i / G.W, q = i - r * G.W;
  const Tap ty = tf1_tap(r, G.hh, G.sy), tx = tf1_tap(q, G.hw, G.sx);
  const float* hb = hm + (size_t)b * G.hh * G.hw * kOvlJoints;
  const float* p00 = hb + ((size_t)ty.lo * G.hw + tx.lo) * kOvlJoints;
  const float* p01 = hb + ((size_t)ty.lo * G.hw + tx.hi) * kOvlJoints;
  const float* p10 = hb + ((size_t)ty.hi * G.hw + tx.lo) * kOvlJoints;
  const float* p11 = hb + ((size_t)ty.hi * G.hw + tx.hi) * kOvlJoints;
  const float* px = x + ((size_t)b * G.H * G.W + i) * 3;
  const float* cb = cst + b * kOvlPics;
  const float cx = cb[0];
  float xin[3], acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    xin[c] = px[c];
    acc[c] = cx * xin[c];
  }
#pragma unroll
  for (int j = 0; j < kOvlJoints; ++j) {
    const float hl = cb[1 + j] * lerp2(p00[j], p01[j], p10[j], p11[j], tx.t, ty.t);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float hc = kColor[j][c] ? hl : 0.f;
      v[j][c] = min1(xin[c] + hc);
      acc[c] = min1(acc[c] + hc);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[kOvlJoints][c] = acc[c];
}

__global__ __launch_bounds__(kImgThreads) void ovl_minmax_kernel(const float* __restrict__ x, const float* __restrict__ hm, const float* __restrict__ cst,
                                                                 OvlGeo G, float2* __restrict__ part) {
  __shared__ float smn[kImgThreads / 64], smx[kImgThreads / 64];
  const int b = blockIdx.y;
  const int i = blockIdx.x * kImgThreads + threadIdx.x;
  float v[kOvlPics][3];
  const bool in = i < G.H * G.W;
  if (in) ovl_pixel(x, hm, cst, G, b, i, v);
  for (int p = 0; p < kOvlPics; ++p) {
    float mn = INFINITY, mx = -INFINITY;
    if (in && isfinite(v[p][0]) && isfinite(v[p][1]) && isfinite(v[p][2])) {
      mn = fminf(fminf(v[p][0], v[p][1]), v[p][2]);
      mx = fmaxf(fmaxf(v[p][0], v[p][1]), v[p][2]);
    }
    block_minmax(mn, mx, smn, smx);
    if (threadIdx.x == 0) part[((size_t)b * kOvlPics + p) * gridDim.x + blockIdx.x] = make_float2(mn, mx);
  }
}

__global__ __launch_bounds__(kImgThreads) void ovl_write_kernel(const float* __restrict__ x, const float* __restrict__ hm, const float* __restrict__ cst,
                                                                OvlGeo G, const float2* __restrict__ so, unsigned char* __restrict__ out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kImgThreads + threadIdx.x;
  const int HW = G.H * G.W;
  if (i >= HW) return;
  float v[kOvlPics][3];
  ovl_pixel(x, hm, cst, G, b, i, v);
  for (int p = 0; p < kOvlPics; ++p) {
    const bool fin = isfinite(v[p][0]) && isfinite(v[p][1]) && isfinite(v[p][2]);
    const float2 s = so[b * kOvlPics + p];
    unsigned char* o = out + (((size_t)b * kOvlPics + p) * HW + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = fin ? quant(v[p][c], s) : (c == 0 ? 255 : 0);
  }
}

int blocks_of(int64_t n) { return (int)((n + kImgThreads - 1) / kImgThreads); }

}  // namespace

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_hist_bucket_limits(double* out, int cap) {
  const PosLimits& L = pos_limits();
  const int n = 2 * L.n + 1;
  if (out) {
    if (cap < n) {
      fail(JCM_ERR_ARG, "hist_bucket_limits: cap < " + std::to_string(n));
      return -1;
    }
    for (int k = 0; k < L.n; ++k) {
      out[L.n - 1 - k] = -L.v[k];
      out[L.n + 1 + k] = L.v[k];
    }
    out[L.n] = 0.0;
  }
  return n;
}

int jcm_tensor_stats(jcm_handle h, const float* data, const int64_t* segments, int n_segments, float scale, float clip_norm, double* stats,
                     int64_t* counts) {
  JCM_TRY(check(h, false));
  if (!segments || !stats || !counts || n_segments < 1 || n_segments > (1 << 20)) return fail(JCM_ERR_ARG, "tensor_stats: bad arguments");
  if (!(scale == scale)) return fail(JCM_ERR_ARG, "tensor_stats: scale is NaN");
  jcm_ctx* c = h;
  const double* sumsq = nullptr;
  if (clip_norm > 0.f) {
    sumsq = train_grad_sumsq(c);
    if (!sumsq) return fail(JCM_ERR_STATE, "tensor_stats: clip_norm > 0 needs the gradient norm of a jcm_train_apply of this handle");
  }
  // chunk table (host): every segment cut into pieces of kChunk elements
  std::vector<Chunk> chunks;
  std::vector<int> first((size_t)n_segments + 1);
  for (int s = 0; s < n_segments; ++s) {
    const int64_t off = segments[2 * s], n = segments[2 * s + 1];
    if (off < 0 || n < 0 || n > ((int64_t)1 << 40) || off > ((int64_t)1 << 40))
      return fail(JCM_ERR_ARG, "tensor_stats: bad segment " + std::to_string(s));
    const float* base = data ? data + off : nullptr;
    if (!data && n > 0) {
      base = train_param_range(c, off, n);
      if (!base) return fail(JCM_ERR_ARG, "tensor_stats: segment " + std::to_string(s) + " does not lie inside one stored trainable tensor");
    }
    first[(size_t)s] = (int)chunks.size();
    for (int64_t k = 0; k < n; k += kChunk) chunks.push_back(Chunk{base + k, (int)std::min<int64_t>(kChunk, n - k), s});
    if (chunks.size() > (size_t)(1 << 30)) return fail(JCM_ERR_ARG, "tensor_stats: too many elements");
  }
  first[(size_t)n_segments] = (int)chunks.size();
  const int nck = (int)chunks.size();
  DeviceGuard g(h->device);
  CallOrder order(h);
  JCM_TRY(hist_limits_dev(c));
  return with_arena(c, [&] {
    Chunk* dck = arena_alloc<Chunk>(c, std::max(nck, 1));
    int* dfirst = arena_alloc<int>(c, first.size());
    Part* parts = arena_alloc<Part>(c, std::max(nck, 1));
    if (c->dry) return (int)JCM_OK;
    auto* cnt = reinterpret_cast<unsigned long long*>(counts);
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_segments * (3 + JCM_HIST_BUCKETS) * sizeof(int64_t), c->stream));
    if (nck) HIP_TRY(hipMemcpyAsync(dck, chunks.data(), (size_t)nck * sizeof(Chunk), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dfirst, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (nck) hipLaunchKernelGGL(stats_chunk_kernel, dim3(nck), dim3(kStatsThreads), 0, c->stream, dck, c->hist_limits, scale, clip_norm, sumsq, parts, cnt);
    hipLaunchKernelGGL(stats_fold_kernel, dim3(n_segments), dim3(kStatsThreads), 0, c->stream, parts, dfirst, 0, stats, cnt);
    HIP_TRY(hipGetLastError());
    order.release();
    HIP_TRY(hipStreamSynchronize(c->stream));     // the chunk table lives in host memory of this call
    return (int)JCM_OK;
  });
}

int jcm_image_u8(jcm_handle h, const float* x, int N, int H, int W, int C, uint8_t* out) {
  JCM_TRY(check(h, false));
  if (!x || !out || N < 1 || N > 65535 || H < 1 || W < 1 || (C != 1 && C != 3) || (int64_t)H * W >= ((int64_t)1 << 30))
    return fail(JCM_ERR_ARG, "image_u8: bad arguments (C must be 1 or 3)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const int HW = H * W, nblk = blocks_of(HW);
  return with_arena(c, [&] {
    float2* part = arena_alloc<float2>(c, (size_t)N * nblk);
    float2* so = arena_alloc<float2>(c, N);
    if (c->dry) return (int)JCM_OK;
    hipLaunchKernelGGL(img_minmax_kernel, dim3(nblk, N), dim3(kImgThreads), 0, c->stream, x, HW, C, part);
    hipLaunchKernelGGL(img_scale_kernel, dim3(N), dim3(kImgThreads), 0, c->stream, part, nblk, so);
    hipLaunchKernelGGL(img_write_kernel, dim3(nblk, N), dim3(kImgThreads), 0, c->stream, x, HW, C, so, out);
    HIP_TRY(hipGetLastError());
    return (int)JCM_OK;
  });
}

int jcm_hm_overlay(jcm_handle h, const float* x, const float* hm, int n, int H, int W, int hh, int hw, int K, uint8_t* out) {
  JCM_TRY(check(h, false));
  if (!x || !hm || !out || n < 1 || n > 65535 || H < 1 || W < 1 || hh < 1 || hw < 1 || (int64_t)H * W >= ((int64_t)1 << 28) ||
      (int64_t)hh * hw >= ((int64_t)1 << 28))
    return fail(JCM_ERR_ARG, "hm_overlay: bad arguments");
  if (K != kOvlJoints) return fail(JCM_ERR_ARG, "hm_overlay: colorize knows the 9 joints of the reference, K = " + std::to_string(K));
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const int HW = H * W, nblk = blocks_of(HW), nxp = 64;
  OvlGeo G;
  G.H = H;
  G.W = W;
  G.hh = hh;
  G.hw = hw;
  G.sy = (float)hh / (float)H;
  G.sx = (float)hw / (float)W;
  return with_arena(c, [&] {
    float* xpart = arena_alloc<float>(c, (size_t)n * nxp);
    float* cst = arena_alloc<float>(c, (size_t)n * kOvlPics);
    float2* part = arena_alloc<float2>(c, (size_t)n * kOvlPics * nblk);
    float2* so = arena_alloc<float2>(c, (size_t)n * kOvlPics);
    if (c->dry) return (int)JCM_OK;
    hipLaunchKernelGGL(ovl_xmax_kernel, dim3(nxp, n), dim3(kImgThreads), 0, c->stream, x, HW * 3, xpart);
    hipLaunchKernelGGL(ovl_contrast_kernel, dim3(n), dim3(kImgThreads), 0, c->stream, xpart, nxp, hm, hh * hw, cst);
    hipLaunchKernelGGL(ovl_minmax_kernel, dim3(nblk, n), dim3(kImgThreads), 0, c->stream, x, hm, cst, G, part);
    hipLaunchKernelGGL(img_scale_kernel, dim3(n * kOvlPics), dim3(kImgThreads), 0, c->stream, part, nblk, so);
    hipLaunchKernelGGL(ovl_write_kernel, dim3(nblk, n), dim3(kImgThreads), 0, c->stream, x, hm, cst, G, so, out);
    HIP_TRY(hipGetLastError());
    return (int)JCM_OK;
  });
}

}  // extern "C"
