// Affine training augmentation: per image ONE composed affine sample of the picture -- flip, rotation, scale and shift folded into six
// numbers on the host (augmentation.affine_geometry), `pad` outside the source -- and target maps that are REDRAWN, not resampled: every channel's joint
// cell goes through the forward map and the data set's own 3x3 blob ([1,2,1] x [1,2,1] / 16, data.target_heat_maps) is written at the cell it lands in.
// The device code has no transcendental in it: positions, weights and the interpolation are float64, one correctly rounded operation per step in the
// order include/jcm.h states (-ffp-contract=off), the colour steps float32 in the order of augment.hip.
// Three launches per group of kAffMax images, whose parameters (maps, colour, source index) travel by value in the kernel arguments -- no staging buffer,
// no copy, nothing for the host to wait for:
//   aff_mean_kernel   per-image channel sums of the brightened source (partials, fixed order, no atomics: the sums of aug_mean_kernel)
//   aff_image_kernel  one thread per output pixel, three channels: four source taps, colour per tap, bilinear; in the antialiased entries
//                     (jcm_augment_affine_aa*) a triangle filter of the image's half-width, two tap loops, where that is not exactly 1
//   aff_maps_kernel   the ten transformed cells once per work group into LDS, then one thread per output element (a test, no scatter)
#include <cmath>
#include <string>

#include "ctx.h"
#include "hm_flip.h"
#include "u8.h"

namespace jcm {

namespace {

constexpr int kAffMax = 16;             // images per launch: 16 * 112 bytes of its 4096 bytes of arguments
constexpr int kAffParts = 128;          // partial sums per image, reduction width and their fold: those of augment.hip, so that the mean is the same number
constexpr int kAffRed = 192;
constexpr int kAffThreads = 256;
constexpr double kAffMaxWidth = 4.0;    // the widest triangle filter of the antialiased entries: scale 0.25, 9 x 9 taps
static_assert(kHmFlipChannels == 10, "aff_maps_kernel permutes the 10 heat-map channels by kHmFlipPerm (hm_flip.h)");
static_assert(kAffRed == 3 * (kAffParts / 2) && kAffThreads >= kAffRed, "aff_image_kernel folds two parts per reduction slot");

struct AffImage {
  double inv[6];      // output pixel (q, r) reads the source at xs = inv[0] q + inv[1] r + inv[2], ys = inv[3] q + inv[4] r + inv[5]
  double fwd[6];      // source point (x, y) lands on qx = fwd[0] x + fwd[1] y + fwd[2], qy = fwd[3] x + fwd[4] y + fwd[5]
  float delta, factor;
  int flip;
  int src;            // the image of x / cells this output image is made from (checked on the host)
};
struct AffArgs {
  AffImage im[kAffMax];
};

// fixed-order fold of red[0 .. kAffRed) into red[0..2] (slot t holds channel t % 3; every stride is a multiple of 3)
__device__ __forceinline__ void fold3(double* red) {
  for (int s = kAffRed / 2; s >= 3; s >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
  }
  __syncthreads();
}

// partials[b][part][c] = sum over the part's pixels of double(float(x + delta)), channel c
// PixT (here and in aff_image_kernel): float, or uint8_t for a byte data set -- every value read goes through px_f32 (u8.h)
template <class PixT>
__global__ __launch_bounds__(kAffRed) void aff_mean_kernel(const PixT* __restrict__ x, AffArgs A, int HW, double* __restrict__ partials) {
  __shared__ double red[kAffRed];
  const int b = blockIdx.y;
  const float delta = A.im[b].delta;
  const int n = HW * 3;
  const int chunk = (n / 3 + kAffParts - 1) / kAffParts * 3;
  const int lo = blockIdx.x * chunk;
  const int hi = min(n, lo + chunk);
  const PixT* xb = x + (size_t)A.im[b].src * n;
  double s = 0.0;
  for (int e = lo + (int)threadIdx.x; e < hi; e += kAffRed) s += (double)(px_f32(xb[e]) + delta);
  red[threadIdx.x] = s;
  fold3(red);
  if (threadIdx.x < 3) partials[((size_t)b * kAffParts + blockIdx.x) * 3 + threadIdx.x] = red[threadIdx.x];
}

// the contrast means of image b from its partial sums, by every thread of the work group: s_mean[c] = float32(sum_c / HW)
__device__ __forceinline__ void aff_means(const double* __restrict__ partials, int b, int HW, double* red, float* s_mean) {
  const int t = threadIdx.x;
  if (t < kAffRed) {      // channel t % 3, parts t / 3 and t / 3 + 64
    const double* pb = partials + (size_t)b * kAffParts * 3;
    red[t] = pb[t] + pb[t + kAffRed];
  }
  fold3(red);
  if (t < 3) s_mean[t] = (float)(red[t] / (double)HW);
  __syncthreads();
}

// One image's source as the samplers read it: a pixel after brightness, contrast and clip (float32, the order of DESIGN.md 4.7), `pad` itself outside.
template <class PixT>
struct AffSource {
  const PixT* xb;
  int H, W;
  float m[3], delta, factor, pad;

  __device__ __forceinline__ void inside(int j, int i, double* v) const {      // 0 <= j < H, 0 <= i < W
    const PixT* s = xb + ((size_t)j * W + i) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float u = px_f32(s[k]) + delta;
      u = (u - m[k]) * factor + m[k];
      v[k] = (double)fminf(fmaxf(u, 0.f), 1.f);
    }
  }
  __device__ __forceinline__ void tap(double yy, double xx, double* v) const {
    if (yy >= 0.0 && yy <= (double)(H - 1) && xx >= 0.0 && xx <= (double)(W - 1)) {      // only then are they turned into integers
      inside((int)yy, (int)xx, v);
    } else {
      v[0] = v[1] = v[2] = (double)pad;
    }
  }
  // the four taps around a finite position (xs, ys)
  __device__ __forceinline__ void bilinear(double xs, double ys, float* dst) const {
    const double x0 = floor(xs), y0 = floor(ys);
    const double fx = xs - x0, fy = ys - y0;
    double v00[3], v01[3], v10[3], v11[3];
    tap(y0, x0, v00);
    tap(y0, x0 + 1.0, v01);
    tap(y0 + 1.0, x0, v10);
    tap(y0 + 1.0, x0 + 1.0, v11);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double top = (1.0 - fx) * v00[k] + fx * v01[k];
      const double bot = (1.0 - fx) * v10[k] + fx * v11[k];
      dst[k] = (float)((1.0 - fy) * top + fy * bot);
    }
  }
  // The triangle filter of half-width w in (1, 4] around a finite position (include/jcm.h, jcm_augment_affine_aa): at most 9 x 9 taps, walked by two
  // loops -- no array of weights, nothing in scratch.  The weight of a column is formed again in every row: a division more per tap, and no run-time indexed array.
  __device__ __forceinline__ void triangle(double xs, double ys, double w, float* dst) const {
    // every tap of a column (row) range that misses the source is `pad`, and the weighted mean of equal values rounds to that value in float32: such a
    // pixel is `pad` without a loop, and a position far outside never becomes an integer
    if (!(xs + w >= 0.0 && xs - w <= (double)(W - 1) && ys + w >= 0.0 && ys - w <= (double)(H - 1))) {
      dst[0] = dst[1] = dst[2] = pad;
      return;
    }
    const int i0 = (int)ceil(xs - w), i1 = (int)floor(xs + w);      // within [-4, W + 3]
    const int j0 = (int)ceil(ys - w), j1 = (int)floor(ys + w);
    const double padv = (double)pad;
    double Sx = 0.0, Sy = 0.0;
    for (int i = i0; i <= i1; ++i) {
      const double tx = 1.0 - fabs(xs - (double)i) / w;
      if (tx > 0.0) Sx += tx;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = j0; j <= j1; ++j) {
      const double ty = 1.0 - fabs(ys - (double)j) / w;
      if (!(ty > 0.0)) continue;
      Sy += ty;
      const bool row_in = j >= 0 && j < H;
      double row[3] = {0.0, 0.0, 0.0};
      for (int i = i0; i <= i1; ++i) {
        const double tx = 1.0 - fabs(xs - (double)i) / w;
        if (!(tx > 0.0)) continue;
        double v[3] = {padv, padv, padv};
        if (row_in && i >= 0 && i < W) inside(j, i, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) row[k] += tx * v[k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] += ty * row[k];
    }
    const double S = Sx * Sy;
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = (float)(acc[k] / S);
  }
};

// kAA: the antialiased entries -- image b is sampled with the triangle filter of half-width Wd.w[b], or, where that is exactly 1, as the plain entry does
struct AffWidths {
  double w[kAffMax];
};

template <class PixT, bool kAA>
__global__ __launch_bounds__(kAffThreads) void aff_image_kernel(const PixT* __restrict__ x, AffArgs A, AffWidths Wd, int H, int W, float pad,
                                                                const double* __restrict__ partials, float* __restrict__ x_out) {
  __shared__ double red[kAffRed];
  __shared__ float s_mean[3];
  const int b = blockIdx.y;
  const int HW = H * W;
  aff_means(partials, b, HW, red, s_mean);
  const int i = blockIdx.x * kAffThreads + (int)threadIdx.x;
  if (i >= HW) return;
  const int r = i / W, q = i - r * W;
  const double xs = (A.im[b].inv[0] * (double)q + A.im[b].inv[1] * (double)r) + A.im[b].inv[2];
  const double ys = (A.im[b].inv[3] * (double)q + A.im[b].inv[4] * (double)r) + A.im[b].inv[5];
  float* dst = x_out + ((size_t)b * HW + i) * 3;
  if (!std::isfinite(xs) || !std::isfinite(ys)) {      // no index is formed from such a position
    dst[0] = dst[1] = dst[2] = pad;
    return;
  }
  const AffSource<PixT> S{x + (size_t)A.im[b].src * HW * 3, H, W, {s_mean[0], s_mean[1], s_mean[2]}, A.im[b].delta, A.im[b].factor, pad};
  if (kAA && Wd.w[b] != 1.0)
    S.triangle(xs, ys, Wd.w[b], dst);
  else
    S.bilinear(xs, ys, dst);
}

// y_out[b, r, c, k] = the blob weight of cell (r, c) around the transformed cell of channel k (source channel kHmFlipPerm[k] of a flipped image)
__global__ __launch_bounds__(kAffThreads) void aff_maps_kernel(const int32_t* __restrict__ cells, AffArgs A, int hh, int hw, float* __restrict__ y_out) {
  __shared__ int s_cell[kHmFlipChannels][2];
  const int b = blockIdx.y;
  const int t = threadIdx.x;
  if (t < kHmFlipChannels) {
    const int ks = A.im[b].flip ? kHmFlipPerm[t] : t;
    const int32_t* c = cells + ((size_t)A.im[b].src * kHmFlipChannels + ks) * 2;
    const double px = 8.0 * (double)c[1] + 3.5, py = 8.0 * (double)c[0] + 3.5;      // the point a cell stands for
    double qx = (A.im[b].fwd[0] * px + A.im[b].fwd[1] * py) + A.im[b].fwd[2];
    double qy = (A.im[b].fwd[3] * px + A.im[b].fwd[4] * py) + A.im[b].fwd[5];
    const double Wd = (double)(8 * hw), Hd = (double)(8 * hh);
    qx = qx >= 0.0 ? (qx <= Wd ? qx : Wd) : 0.0;      // data.joint_cells' clamp to the image (NaN -> 0): row hh / column hw are possible
    qy = qy >= 0.0 ? (qy <= Hd ? qy : Hd) : 0.0;
    s_cell[t][0] = (int)(qy / 8.0);
    s_cell[t][1] = (int)(qx / 8.0);
  }
  __syncthreads();
  const int n = hh * hw * kHmFlipChannels;
  const int e = blockIdx.x * kAffThreads + t;
  if (e >= n) return;
  const int cell = e / kHmFlipChannels, k = e - cell * kHmFlipChannels;
  const int r = cell / hw, c = cell - r * hw;
  const int dr = r - s_cell[k][0], dc = c - s_cell[k][1];
  float v = 0.f;
  if (dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1) v = (float)((dr == 0 ? 2 : 1) * (dc == 0 ? 2 : 1)) / 16.f;
  y_out[(size_t)b * n + e] = v;
}

template <class PixT>
hipError_t aff_launch(const PixT* x, const int32_t* cells, const int* idx, const float* colour, const double* geom, const double* width, int B, int H, int W,
                      int hh, int hw, float pad, double* scratch, float* x_out, float* y_out, hipStream_t st) {
  const int HW = H * W, ny = hh * hw * kHmFlipChannels;
  for (int b0 = 0; b0 < B; b0 += kAffMax) {      // image b0 + i of the batch is image i of its launches: every per-image array starts at b0
    const int nb = B - b0 < kAffMax ? B - b0 : kAffMax;
    AffArgs A{};
    AffWidths Wd{};
    for (int i = 0; i < nb; ++i) {
      AffImage& P = A.im[i];
      const double* g = geom + (size_t)(b0 + i) * 12;
      for (int j = 0; j < 6; ++j) P.inv[j] = g[j], P.fwd[j] = g[6 + j];
      const float* c = colour + (size_t)(b0 + i) * 3;
      P.flip = c[0] == 1.f;
      P.delta = c[1];
      P.factor = c[2];
      P.src = idx ? idx[b0 + i] : b0 + i;
      Wd.w[i] = width ? width[b0 + i] : 1.0;
    }
    double* part = scratch + (size_t)b0 * kAffParts * 3;
    hipLaunchKernelGGL(aff_mean_kernel<PixT>, dim3(kAffParts, nb), dim3(kAffRed), 0, st, x, A, HW, part);
    const dim3 grid((HW + kAffThreads - 1) / kAffThreads, nb);
    if (width)
      hipLaunchKernelGGL((aff_image_kernel<PixT, true>), grid, dim3(kAffThreads), 0, st, x, A, Wd, H, W, pad, part, x_out + (size_t)b0 * HW * 3);
    else
      hipLaunchKernelGGL((aff_image_kernel<PixT, false>), grid, dim3(kAffThreads), 0, st, x, A, Wd, H, W, pad, part, x_out + (size_t)b0 * HW * 3);
    hipLaunchKernelGGL(aff_maps_kernel, dim3((ny + kAffThreads - 1) / kAffThreads, nb), dim3(kAffThreads), 0, st, cells, A, hh, hw,
                       y_out + (size_t)b0 * ny);
  }
  return hipGetLastError();
}

// the entry points' shared body; idx == nullptr: image b of x / cells itself (N == B); aa: the antialiased entries, which take width[B]
int aff_entry(jcm_handle h, const char* who, const void* x, bool x_u8, const int32_t* cells, int64_t N, const int32_t* idx, bool indexed, const float* colour,
              const double* geom, const double* width, bool aa, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out) {
  JCM_TRY(check(h, false));
  const std::string w(who);
  if (!x || !cells || (indexed && !idx) || !colour || !geom || (aa && !width) || !x_out || !y_out) return fail(JCM_ERR_ARG, w + ": null pointer");
  if (h->K != 9)
    return fail(JCM_ERR_ARG, w + ": the heat maps have 10 channels (n_joints == 9), this handle has n_joints = " + std::to_string(h->K));
  if (N < 1 || N > INT32_MAX || B < 1 || B > 65535 || hh < 1 || hw < 1 || H < 1 || W < 1 || (int64_t)H * W * 3 >= (int64_t)1 << 30)
    return fail(JCM_ERR_ARG, w + ": bad sizes (N in [1, 2^31), B in [1, 65535], h, w >= 1, H * W * 3 < 2^30)");
  if ((int64_t)H != 8 * (int64_t)hh || (int64_t)W != 8 * (int64_t)hw)
    return fail(JCM_ERR_ARG, w + ": an image of " + std::to_string(H) + " x " + std::to_string(W) + " with maps of " + std::to_string(hh) + " x " +
                                 std::to_string(hw) + "; a map cell is 8 x 8 pixels (H == 8 h, W == 8 w)");
  if (!std::isfinite(pad)) return fail(JCM_ERR_ARG, w + ": pad is not finite");
  if (indexed)
    for (int b = 0; b < B; ++b)
      if (idx[b] < 0 || (int64_t)idx[b] >= N)
        return fail(JCM_ERR_ARG, w + ": idx[" + std::to_string(b) + "] = " + std::to_string(idx[b]) + " is outside [0, " + std::to_string(N) + ")");
  for (int b = 0; b < B; ++b) {
    const float* c = colour + (size_t)b * 3;
    if (!(c[0] == 0.f || c[0] == 1.f) || !std::isfinite(c[1]) || !std::isfinite(c[2]))
      return fail(JCM_ERR_ARG, w + ": colour row " + std::to_string(b) + " is not (flip in {0, 1}, finite delta, finite factor)");
    for (int j = 0; j < 12; ++j)
      if (!std::isfinite(geom[(size_t)b * 12 + j]))
        return fail(JCM_ERR_ARG, w + ": geom[" + std::to_string(b) + "][" + std::to_string(j) + "] is not finite");
  }
  if (aa)
    for (int b = 0; b < B; ++b)
      if (!(width[b] >= 1.0 && width[b] <= kAffMaxWidth))      // (a NaN fails both comparisons)
        return fail(JCM_ERR_ARG, w + ": width[" + std::to_string(b) + "] = " + std::to_string(width[b]) + " is not a finite filter half-width in [1, 4]");
  const size_t ix = (size_t)H * W * 3, iy = (size_t)hh * hw * kHmFlipChannels;
  const size_t nxa = (size_t)N * ix * (x_u8 ? 1 : sizeof(float)), nca = (size_t)N * kHmFlipChannels * 2 * sizeof(int32_t);
  const size_t nx = (size_t)B * ix * sizeof(float), ny = (size_t)B * iy * sizeof(float);
  auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
    return pa < pb + nb && pb < pa + na;
  };
  if (overlap(x_out, nx, x, nxa) || overlap(x_out, nx, cells, nca) || overlap(y_out, ny, x, nxa) || overlap(y_out, ny, cells, nca) ||
      overlap(x_out, nx, y_out, ny))
    return fail(JCM_ERR_ARG, w + (indexed ? ": x_out / y_out overlap the data set, the cells or each other" : ": x_out / y_out alias an input or each other"));
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  return with_arena(c, [&] {
    double* scratch = arena_alloc<double>(c, (size_t)B * kAffParts * 3);
    if (c->dry) return (int)JCM_OK;
    const hipError_t launch = x_u8 ? aff_launch(static_cast<const uint8_t*>(x), cells, idx, colour, geom, aa ? width : nullptr, B, H, W, hh, hw, pad, scratch, x_out, y_out, c->stream)
                                   : aff_launch(static_cast<const float*>(x), cells, idx, colour, geom, aa ? width : nullptr, B, H, W, hh, hw, pad, scratch, x_out, y_out, c->stream);
    if (launch != hipSuccess) return fail(JCM_ERR_HIP, w + ": " + hipGetErrorString(launch));
    return (int)JCM_OK;
  });
}

}  // namespace

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_augment_affine(jcm_handle h, const float* x, const int32_t* cells, const float* colour, const double* geom, int B, int H, int W, int hh, int hw,
                       float pad, float* x_out, float* y_out) {
  return aff_entry(h, "augment_affine", x, false, cells, B, nullptr, false, colour, geom, nullptr, false, B, H, W, hh, hw, pad, x_out, y_out);
}

int jcm_augment_affine_indexed(jcm_handle h, const float* x_all, const int32_t* cells_all, int64_t N, const int32_t* idx, const float* colour,
                               const double* geom, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out) {
  return aff_entry(h, "augment_affine_indexed", x_all, false, cells_all, N, idx, true, colour, geom, nullptr, false, B, H, W, hh, hw, pad, x_out, y_out);
}

int jcm_augment_affine_indexed_u8(jcm_handle h, const uint8_t* x_all, const int32_t* cells_all, int64_t N, const int32_t* idx, const float* colour,
                                  const double* geom, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out) {
  return aff_entry(h, "augment_affine_indexed_u8", x_all, true, cells_all, N, idx, true, colour, geom, nullptr, false, B, H, W, hh, hw, pad, x_out, y_out);
}

int jcm_augment_affine_aa(jcm_handle h, const float* x, const int32_t* cells, const float* colour, const double* geom, const double* width, int B, int H,
                          int W, int hh, int hw, float pad, float* x_out, float* y_out) {
  return aff_entry(h, "augment_affine_aa", x, false, cells, B, nullptr, false, colour, geom, width, true, B, H, W, hh, hw, pad, x_out, y_out);
}

int jcm_augment_affine_aa_indexed(jcm_handle h, const float* x_all, const int32_t* cells_all, int64_t N, const int32_t* idx, const float* colour,
                                  const double* geom, const double* width, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out) {
  return aff_entry(h, "augment_affine_aa_indexed", x_all, false, cells_all, N, idx, true, colour, geom, width, true, B, H, W, hh, hw, pad, x_out, y_out);
}

int jcm_augment_affine_aa_indexed_u8(jcm_handle h, const uint8_t* x_all, const int32_t* cells_all, int64_t N, const int32_t* idx, const float* colour,
                                     const double* geom, const double* width, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out) {
  return aff_entry(h, "augment_affine_aa_indexed_u8", x_all, true, cells_all, N, idx, true, colour, geom, width, true, B, H, W, hh, hw, pad, x_out, y_out);
}

}  // extern "C"
