// Training-time data augmentation (augmentation.py:58-78, applied at main.py:494-497): per image, in the reference's
// order, flip (heat-map channels permuted), brightness, contrast, clip to [0, 1], rotation (ImageProjectiveTransform,
// bilinear, fill 0), crop_and_resize back to the input size, and the heat maps' pow(., 1.6) + 1e-5 renormalisation.
// The semantics are DESIGN.md 4.7 (a restatement of the TF-1.x ops, float32 in the order written; tests/augment_ref.py).
// Three launches: the per-image channel sums of the brightened image (partials, no atomics), the image gather (crop taps ->
// rotated samples -> source taps, the colour steps applied per source tap) and one work group per (image, heat-map channel).
#include "entry.h"
#include "hm_flip.h"
#include "u8.h"

namespace jcm {

namespace {

constexpr int kAugParts = 128;          // partial sums per image (aug_mean_kernel's grid.x)
constexpr int kAugRed = 192;            // reduction width: a multiple of 3, so that slot t always holds channel t % 3
constexpr int kAugImgThreads = 256;
constexpr int kAugHmThreads = 512;
constexpr float kCropSize = 0.95f;      // augmentation.py:40
static_assert(kHmFlipChannels == 10, "aug_hm_kernel permutes the 10 heat-map channels by kHmFlipPerm (hm_flip.h)");

// where image b of the batch comes from: image b of the array itself, or image idx[b] of a data set (jcm_augment_train_indexed; the
// indices travel in the kernel arguments and were checked on the host)
struct SrcDirect {
  __device__ __forceinline__ size_t operator()(int b) const { return (size_t)b; }
};
struct SrcIndexed {
  GatherIdx idx;
  __device__ __forceinline__ size_t operator()(int b) const { return (size_t)idx.v[b]; }
};

// params[b] = (flip, delta, factor, angle, rh, rw)
struct Rot {
  float c, s, xo, yo;
};

// angles_to_projective_transforms for an h x w image; cos / sin in double, rounded (the host restatement uses the same values)
__device__ Rot make_rot(float angle, int h, int w) {
  Rot R;
  R.c = (float)cos((double)angle);
  R.s = (float)sin((double)angle);
  const float wm = (float)(w - 1), hm = (float)(h - 1);
  R.xo = (wm - (R.c * wm - R.s * hm)) / 2.f;
  R.yo = (hm - (R.s * wm + R.c * hm)) / 2.f;
  return R;
}

// one axis of crop_and_resize (crop extent == input extent n): taps lo / hi and weight l; ok = false -> the row / column is 0
struct Axis {
  int lo, hi;
  float l;
  bool ok;
};
__device__ __forceinline__ Axis crop_axis(float b1, int n, int i) {
  const float b2 = b1 + kCropSize;
  const float nm = (float)(n - 1);
  const float scale = ((b2 - b1) * nm) / nm;
  const float in = b1 * nm + (float)i * scale;
  Axis a;
  a.ok = in >= 0.f && in <= nm;            // false for NaN as well: no index is formed from it
  const float t = a.ok ? floorf(in) : 0.f;
  a.lo = (int)t;
  a.hi = a.ok ? (int)ceilf(in) : 0;
  a.l = a.ok ? in - t : 0.f;
  return a;
}

// ImageProjectiveTransform (BILINEAR, fill 0) at output pixel (r, q) of an h x w map; at(yf, xf, v) writes the NC source values
// at the integral float position (yf, xf), or zeros outside [0,h) x [0,w)
template <int NC, class At>
__device__ __forceinline__ void rot_sample(const Rot& R, int r, int q, At at, float* out) {
  const float xi = (R.c * (float)q + (-R.s) * (float)r) + R.xo;
  const float yi = (R.s * (float)q + R.c * (float)r) + R.yo;
#pragma unroll
  for (int k = 0; k < NC; ++k) out[k] = 0.f;
  if (!isfinite(xi) || !isfinite(yi)) return;
  const float x0 = floorf(xi), y0 = floorf(yi), x1 = x0 + 1.f, y1 = y0 + 1.f;
  float p00[NC], p01[NC], p10[NC], p11[NC];
  at(y0, x0, p00);
  at(y0, x1, p01);
  at(y1, x0, p10);
  at(y1, x1, p11);
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float top = (x1 - xi) * p00[k] + (xi - x0) * p01[k];
    const float bot = (x1 - xi) * p10[k] + (xi - x0) * p11[k];
    out[k] = (y1 - yi) * top + (yi - y0) * bot;
  }
}

// crop_and_resize of the rotated map at output pixel (r, q): four rotated samples, each from its four source taps
template <int NC, class At>
__device__ __forceinline__ void crop_rot_sample(const Rot& R, const Axis& Y, const Axis& X, At at, float* out) {
#pragma unroll
  for (int k = 0; k < NC; ++k) out[k] = 0.f;
  if (!Y.ok || !X.ok) return;
  float tl[NC], tr[NC], bl[NC], br[NC];
  rot_sample<NC>(R, Y.lo, X.lo, at, tl);
  rot_sample<NC>(R, Y.lo, X.hi, at, tr);
  rot_sample<NC>(R, Y.hi, X.lo, at, bl);
  rot_sample<NC>(R, Y.hi, X.hi, at, br);
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float t = tl[k] + (tr[k] - tl[k]) * X.l;
    const float b = bl[k] + (br[k] - bl[k]) * X.l;
    out[k] = t + (b - t) * Y.l;
  }
}

// fixed-order fold of red[0 .. kAugRed) into red[0..2] (slot t holds channel t % 3; every stride is a multiple of 3)
__device__ __forceinline__ void fold3(double* red) {
  for (int s = kAugRed / 2; s >= 3; s >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
  }
  __syncthreads();
}

// partials[b][part][c] = sum over the part's pixels of double(float(x + delta)), channel c
// PixT (here and in aug_image_kernel): float, or uint8_t for a byte data set -- every value read goes through px_f32 (u8.h), the sums keep their order
template <class Src, class PixT>
__global__ __launch_bounds__(kAugRed) void aug_mean_kernel(const PixT* __restrict__ x, const float* __restrict__ params, int HW,
                                                           double* __restrict__ partials, Src src) {
  __shared__ double red[kAugRed];
  const int b = blockIdx.y;
  const float delta = params[(size_t)b * 6 + 1];
  const int n = HW * 3;
  const int chunk = (n / 3 + kAugParts - 1) / kAugParts * 3;
  const int lo = blockIdx.x * chunk;
  const int hi = min(n, lo + chunk);
  const PixT* xb = x + src(b) * n;
  double s = 0.0;
  for (int e = lo + (int)threadIdx.x; e < hi; e += kAugRed) s += (double)(px_f32(xb[e]) + delta);
  red[threadIdx.x] = s;
  fold3(red);
  if (threadIdx.x < 3) partials[((size_t)b * kAugParts + blockIdx.x) * 3 + threadIdx.x] = red[threadIdx.x];
}

template <class Src, class PixT>
__global__ __launch_bounds__(kAugImgThreads) void aug_image_kernel(const PixT* __restrict__ x, const float* __restrict__ params, int H, int W,
                                                                   const double* __restrict__ partials, float* __restrict__ x_out, Src src) {
  __shared__ double red[kAugRed];
  __shared__ float s_mean[3];
  __shared__ Rot s_rot;
  const int b = blockIdx.y;
  const float* p = params + (size_t)b * 6;
  const bool flip = p[0] == 1.f;
  const float delta = p[1], factor = p[2];
  const int HW = H * W;
  const int t = threadIdx.x;
  if (t < kAugRed) {      // channel t % 3, parts t / 3 and t / 3 + 64
    const double* pb = partials + (size_t)b * kAugParts * 3;
    red[t] = pb[t] + pb[t + kAugRed];
  }
  if (t == kAugImgThreads - 1) s_rot = make_rot(p[3], H, W);
  fold3(red);
  if (t < 3) s_mean[t] = (float)(red[t] / (double)HW);
  __syncthreads();
  const int i = blockIdx.x * kAugImgThreads + t;
  if (i >= HW) return;
  const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
  const Rot R = s_rot;
  const PixT* xb = x + src(b) * HW * 3;
  // a source pixel after flip, brightness, contrast and clip; zeros outside the image (the rotation's fill)
  auto at = [&](float yf, float xf, float* v) {
    if (yf >= 0.f && yf < (float)H && xf >= 0.f && xf < (float)W) {
      const int xx = (int)xf;
      const PixT* s = xb + ((size_t)(int)yf * W + (flip ? W - 1 - xx : xx)) * 3;
      const float m[3] = {m0, m1, m2};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float u = px_f32(s[k]) + delta;
        u = (u - m[k]) * factor + m[k];
        v[k] = fminf(fmaxf(u, 0.f), 1.f);
      }
    } else {
      v[0] = v[1] = v[2] = 0.f;
    }
  };
  const int r = i / W, q = i - r * W;
  float o[3];
  crop_rot_sample<3>(R, crop_axis(p[4], H, r), crop_axis(p[5], W, q), at, o);
  float* dst = x_out + ((size_t)b * HW + i) * 3;
  dst[0] = o[0];
  dst[1] = o[1];
  dst[2] = o[2];
}

// one work group per (heat-map channel k, image b): flip + channel permutation, rotation, crop, t = pow(v, 1.6) + 1e-5, t / sum(t)
template <class Src>
__global__ __launch_bounds__(kAugHmThreads) void aug_hm_kernel(const float* __restrict__ y, const float* __restrict__ params, int h, int w,
                                                               float* __restrict__ y_out, Src src) {
  __shared__ double red[kAugHmThreads];
  __shared__ Rot s_rot;
  const int k = blockIdx.x, b = blockIdx.y;
  const float* p = params + (size_t)b * 6;
  const bool flip = p[0] == 1.f;
  const int hw = h * w;
  const int t = threadIdx.x;
  if (t == 0) s_rot = make_rot(p[3], h, w);
  __syncthreads();
  const Rot R = s_rot;
  const float* yb = y + src(b) * hw * 10 + (flip ? kHmFlipPerm[k] : k);
  float* ob = y_out + (size_t)b * hw * 10 + k;
  auto at = [&](float yf, float xf, float* v) {
    v[0] = 0.f;
    if (yf >= 0.f && yf < (float)h && xf >= 0.f && xf < (float)w) {
      const int xx = (int)xf;
      v[0] = yb[((size_t)(int)yf * w + (flip ? w - 1 - xx : xx)) * 10];
    }
  };
  double s = 0.0;
  for (int i = t; i < hw; i += kAugHmThreads) {
    const int r = i / w, q = i - r * w;
    float v;
    crop_rot_sample<1>(R, crop_axis(p[4], h, r), crop_axis(p[5], w, q), at, &v);
    const float u = powf(v, 1.6f) + 1e-5f;
    ob[(size_t)i * 10] = u;
    s += (double)u;
  }
  red[t] = s;
  for (int st = kAugHmThreads / 2; st > 0; st >>= 1) {
    __syncthreads();
    if (t < st) red[t] += red[t + st];
  }
  __syncthreads();
  const float tot = (float)red[0];
  for (int i = t; i < hw; i += kAugHmThreads) ob[(size_t)i * 10] = ob[(size_t)i * 10] / tot;     // this thread's own stores
}

// the scratch of a batch: the per-image channel sums of the brightened image
size_t augment_scratch_doubles(int B) { return (size_t)B * kAugParts * 3; }

template <class Src, class PixT>
void augment_launch(const PixT* x, const float* y, const float* params, int B, int H, int W, int hh, int hw, double* scratch, float* x_out,
                    float* y_out, const Src& src, hipStream_t st) {
  static_assert(kAugRed == 3 * (kAugParts / 2) && kAugImgThreads >= kAugRed, "aug_image_kernel folds two parts per reduction slot");
  hipLaunchKernelGGL((aug_mean_kernel<Src, PixT>), dim3(kAugParts, B), dim3(kAugRed), 0, st, x, params, H * W, scratch, src);
  hipLaunchKernelGGL((aug_image_kernel<Src, PixT>), dim3((H * W + kAugImgThreads - 1) / kAugImgThreads, B), dim3(kAugImgThreads), 0, st, x, params, H, W,
                     scratch, x_out, src);
  hipLaunchKernelGGL(aug_hm_kernel<Src>, dim3(10, B), dim3(kAugHmThreads), 0, st, y, params, hh, hw, y_out, src);
}

// x [B,H,W,3], y [B,hh,hw,10], params [B,6] = (flip, delta, factor, angle, rh, rw), all device fp32; three launches on `st`
hipError_t augment_train(const float* x, const float* y, const float* params, int B, int H, int W, int hh, int hw, double* scratch,
                         float* x_out, float* y_out, hipStream_t st) {
  augment_launch(x, y, params, B, H, W, hh, hw, scratch, x_out, y_out, SrcDirect{}, st);
  return hipGetLastError();
}

// augment_train with image idx[b] of (x_all, y_all) as the source of output image b (kGatherMax images a launch); same kernels, same arithmetic
template <class PixT>
hipError_t augment_indexed(const PixT* x_all, const float* y_all, const int* idx, const float* params, int B, int H, int W, int hh, int hw,
                           double* scratch, float* x_out, float* y_out, hipStream_t st) {
  for (int b0 = 0; b0 < B; b0 += kGatherMax) {      // image b0 + i of the batch is image i of its launch: every per-image array starts at b0
    const int nb = B - b0 < kGatherMax ? B - b0 : kGatherMax;
    SrcIndexed src;
    for (int i = 0; i < kGatherMax; ++i) src.idx.v[i] = i < nb ? idx[b0 + i] : 0;
    augment_launch(x_all, y_all, params + (size_t)b0 * 6, nb, H, W, hh, hw, scratch + augment_scratch_doubles(b0), x_out + (size_t)b0 * H * W * 3,
                   y_out + (size_t)b0 * hh * hw * 10, src, st);
  }
  return hipGetLastError();
}
// ... from a float and from a byte image array (every tap converted by u8_to_f32; sums in the same order: the same bits), under the names an error carries
hipError_t augment_train_indexed(const float* x_all, const float* y_all, const int* idx, const float* params, int B, int H, int W, int hh, int hw,
                                 double* scratch, float* x_out, float* y_out, hipStream_t st) {
  return augment_indexed(x_all, y_all, idx, params, B, H, W, hh, hw, scratch, x_out, y_out, st);
}
hipError_t augment_train_indexed_u8(const uint8_t* x_all, const float* y_all, const int* idx, const float* params, int B, int H, int W, int hh, int hw,
                                    double* scratch, float* x_out, float* y_out, hipStream_t st) {
  return augment_indexed(x_all, y_all, idx, params, B, H, W, hh, hw, scratch, x_out, y_out, st);
}

}  // namespace

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_augment_train(jcm_handle h, const float* x, const float* y, const float* params, int B, int H, int W,
                      int hh, int hw, float* x_out, float* y_out) {
  JCM_TRY(check(h, false));
  if (!x || !y || !params || !x_out || !y_out) return fail(JCM_ERR_ARG, "augment_train: null pointer");
  if (B < 1 || B > 65535 || H < 2 || W < 2 || hh < 2 || hw < 2 || (int64_t)H * W * 3 >= (int64_t)1 << 30 || (int64_t)hh * hw * 10 >= (int64_t)1 << 30)
    return fail(JCM_ERR_ARG, "augment_train: bad sizes (B in [1, 65535], H, W, h, w >= 2)");
  if (h->K != 9) return fail(JCM_ERR_ARG, "augment_train: the heat maps have 10 channels (n_joints == 9), this handle has n_joints = " + std::to_string(h->K));
  const size_t nx = (size_t)B * H * W * 3 * sizeof(float), ny = (size_t)B * hh * hw * 10 * sizeof(float), np = (size_t)B * 6 * sizeof(float);
  if (ranges_overlap(x_out, nx, x, nx) || ranges_overlap(x_out, nx, y, ny) || ranges_overlap(x_out, nx, params, np) || ranges_overlap(y_out, ny, x, nx) ||
      ranges_overlap(y_out, ny, y, ny) || ranges_overlap(y_out, ny, params, np) || ranges_overlap(x_out, nx, y_out, ny))
    return fail(JCM_ERR_ARG, "augment_train: x_out / y_out alias an input or each other");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  return with_arena(c, [&] {
    double* scratch = arena_alloc<double>(c, augment_scratch_doubles(B));
    if (c->dry) return (int)JCM_OK;
    HIP_TRY(augment_train(x, y, params, B, H, W, hh, hw, scratch, x_out, y_out, c->stream));
    return (int)JCM_OK;
  });
}

static int augment_indexed_entry(jcm_handle h, const char* who, const void* x_all, bool x_u8, const float* y_all, int64_t N, const int32_t* idx,
                                 const float* params, int B, int H, int W, int hh, int hw, float* x_out, float* y_out) {
  JCM_TRY(check(h, false));
  const std::string w(who);
  if (!params) return fail(JCM_ERR_ARG, w + ": null pointer");
  if (h->K != 9)
    return fail(JCM_ERR_ARG, w + ": the heat maps have 10 channels (n_joints == 9), this handle has n_joints = " + std::to_string(h->K));
  JCM_TRY(check_indexed(who, x_all, x_u8 ? 1 : sizeof(float), y_all, N, idx, params, B, H, W, hh, hw, 10, 2, x_out, y_out));
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  return with_arena(c, [&] {
    double* scratch = arena_alloc<double>(c, augment_scratch_doubles(B));
    if (c->dry) return (int)JCM_OK;
    if (x_u8) HIP_TRY(augment_train_indexed_u8(static_cast<const uint8_t*>(x_all), y_all, idx, params, B, H, W, hh, hw, scratch, x_out, y_out, c->stream));
    else HIP_TRY(augment_train_indexed(static_cast<const float*>(x_all), y_all, idx, params, B, H, W, hh, hw, scratch, x_out, y_out, c->stream));
    return (int)JCM_OK;
  });
}
int jcm_augment_train_indexed(jcm_handle h, const float* x_all, const float* y_all, int64_t N, const int32_t* idx, const float* params, int B,
                              int H, int W, int hh, int hw, float* x_out, float* y_out) {
  return augment_indexed_entry(h, "augment_train_indexed", x_all, false, y_all, N, idx, params, B, H, W, hh, hw, x_out, y_out);
}
int jcm_augment_train_indexed_u8(jcm_handle h, const uint8_t* x_all, const float* y_all, int64_t N, const int32_t* idx, const float* params, int B,
                                 int H, int W, int hh, int hw, float* x_out, float* y_out) {
  return augment_indexed_entry(h, "augment_train_indexed_u8", x_all, true, y_all, N, idx, params, B, H, W, hh, hw, x_out, y_out);
}

}  // extern "C"
