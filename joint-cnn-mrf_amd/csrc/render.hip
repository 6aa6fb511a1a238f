// Poses drawn onto the source images (include/jcm.h: jcm_render_poses): the ragged byte batch of jcm_fit_images, image b
// [h_b, w_b, 3] at any byte offset of one buffer, comes out at the same offset of `out` with two layers on it -- the heat tint (the maps of the
// tower, read back through the inverse of the letterbox fit, added onto the bytes and saturating) and, on top, anti-aliased capsules in
// painter's order.  Both layers are stated in jcm.h in float64 and integers, in an order a sequential restatement reproduces bit for bit.
//   * a work group owns kRenderTile consecutive pixels of one image in row-major order.  Rows follow one another without a gap, so a tile is
//     ONE contiguous byte range whatever the image's width: it is staged into LDS by 16-byte loads wherever a whole aligned chunk lies inside
//     the range (the first and the last chunk byte by byte -- no byte outside the tile's range is ever read or written), drawn on in LDS, and
//     stored the same way.  A tile is read completely before its first byte is written and tiles are disjoint, so out == src is allowed.
//   * the work group culls the image's primitives (at most 256, one thread each) against the rows -- for a tile inside one row, also the
//     columns -- of its tile by bounding box, segment box grown by r, into an LDS list in listing order (ballot + prefix count).  The listed
//     primitives are drawn one after the other, the work group spread over the pixels of the primitive's box inside the tile: the 16 sub-sample
//     test runs for those pixels only, and a pixel far from every primitive costs nothing.  (The first version walked the tile's pixels and
//     tested every listed box per pixel: four LDS reads per pixel and listed primitive made one skeleton an image cost 3.6 copies.)  A tile
//     with an empty list and no tint is copied global -> global and touches no LDS; in place it is nothing at all.
//   * the images of a launch travel in its arguments (RenderBatch, as FitBatch), 64 per launch; the primitives are too many for that (256 x 32
//     bytes an image) and are put into workspace by small launches that carry kRenderPut of them each in THEIR arguments: nothing is copied
//     from caller-owned host memory asynchronously, so nothing has to be waited for.
//   * the per-map maxima the tint normalises by come from a launch of their own (one work group per map) into workspace.
#include <string>

#include "coverage.h"      // render_coverage: the capsule test, shared with synth_people.hip
#include "entry.h"

namespace jcm {

namespace {

constexpr int kRenderThreads = 256;
constexpr int kRenderWaves = kRenderThreads / 64;
constexpr int kRenderBytes = kRenderTile * 3;
constexpr int kRenderPut = 120;      // primitives per upload launch: 3840 bytes of its 4096 bytes of arguments

struct RenderPut {
  int32_t v[kRenderPut * 8];
};
__global__ __launch_bounds__(kRenderThreads) void render_put_kernel(RenderPut p, int n, int32_t* __restrict__ dst) {
  for (int i = threadIdx.x; i < n * 8; i += kRenderThreads) dst[i] = p.v[i];
}

// maxima[b * K + j] = max over the cells of hm[b, :, :, j]
__global__ __launch_bounds__(kRenderThreads) void render_max_kernel(const float* __restrict__ hm, int cells, int K, float* __restrict__ maxima) {
  __shared__ float part[kRenderThreads];
  const int b = blockIdx.x / K, j = blockIdx.x - b * K;
  const float* p = hm + (size_t)b * cells * K + j;
  float m = -INFINITY;
  for (int i = threadIdx.x; i < cells; i += kRenderThreads) m = fmaxf(m, p[(size_t)i * K]);
  part[threadIdx.x] = m;
  __syncthreads();
  for (int s = kRenderThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = fmaxf(part[threadIdx.x], part[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) maxima[blockIdx.x] = part[0];
}

// n bytes src -> dst by the calling work group.  chunk c is the 16 bytes at (first byte's address rounded down to 16) + 16 c: whole chunks inside
// the range move as one uint4 where `wide` (src and dst equally misaligned), everything else byte by byte.
struct RenderSpan {
  int mis, nchunks;
  __device__ __forceinline__ RenderSpan(const void* first, int n) {
    mis = (int)(reinterpret_cast<uintptr_t>(first) & 15u);
    nchunks = (mis + n + 15) >> 4;
  }
};

__device__ __forceinline__ void render_copy(const uint8_t* src, uint8_t* dst, int n) {
  const RenderSpan sp(src, n);
  const bool wide = sp.mis == (int)(reinterpret_cast<uintptr_t>(dst) & 15u);
  for (int c = threadIdx.x; c < sp.nchunks; c += kRenderThreads) {
    const int lo = c * 16 - sp.mis;
    if (wide && lo >= 0 && lo + 16 <= n) {
      *reinterpret_cast<uint4*>(dst + lo) = *reinterpret_cast<const uint4*>(src + lo);
    } else {
      for (int q = 0; q < 16; ++q)
        if (lo + q >= 0 && lo + q < n) dst[lo + q] = src[lo + q];
    }
  }
}

// one axis of the tint's sampling position: source pixel centre -> the fitted frame -> heat-map cells, clamped
__device__ __forceinline__ double render_cell(int p, int content, int n, int origin, int stride, int cells) {
  const double f = ((double)p + 0.5) * (double)content / (double)n - 0.5 + (double)origin;
  return fmin(fmax(f / (double)stride, 0.0), (double)(cells - 1));
}

template <bool kHeat>
__global__ __launch_bounds__(kRenderThreads) void render_kernel(const uint8_t* src, uint8_t* out, RenderBatch rb, int nimg, int b0,
                                                                const int32_t* __restrict__ prims, RenderHeat ht) {
  __shared__ __align__(16) uint8_t px[kRenderBytes + 16];
  __shared__ int lp[kRenderPrimMax][12];      // a listed primitive: its 8 entries, then the pixels its box can touch: ylo, yhi, xlo, xhi
  __shared__ int wave_n[kRenderWaves];
  const int tid = threadIdx.x;

  int bi = 0;
  while (bi + 1 < nimg && (int)blockIdx.x >= rb.first[bi + 1]) ++bi;
  const int h = rb.h[bi], w = rb.w[bi];
  const int p0 = ((int)blockIdx.x - rb.first[bi]) * kRenderTile;      // h * w <= 2^28
  const int np = min(kRenderTile, h * w - p0), nbytes = np * 3;
  const int64_t a = rb.off[bi] + (int64_t)p0 * 3;
  const int ya = p0 / w, xa = p0 - ya * w;
  const int yb = (p0 + np - 1) / w, xb = p0 + np - 1 - yb * w;
  const int tx0 = ya == yb ? xa : 0, tx1 = ya == yb ? xb : w - 1;

  // cull: thread i takes primitive i of the image
  const int pbase = rb.pfirst[bi], pn = rb.pfirst[bi + 1] - pbase;
  int v[8], ylo = 0, yhi = 0, xlo = 0, xhi = 0;
  bool keep = false;
  if (tid < pn) {
    const int4* q = reinterpret_cast<const int4*>(prims + (size_t)(pbase + tid) * 8);      // workspace: 256-byte aligned, 32 bytes a primitive
    const int4 q0 = q[0], q1 = q[1];
    v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
    // pixel y has samples at 16 y - 6 .. 16 y + 6: it can be touched if 16 y + 6 >= lo and 16 y - 6 <= hi (>> 4 floors; the low end may be one early)
    ylo = (min(v[1], v[3]) - v[5] - 6) >> 4;
    yhi = (max(v[1], v[3]) + v[5] + 6) >> 4;
    xlo = (min(v[2], v[4]) - v[5] - 6) >> 4;
    xhi = (max(v[2], v[4]) + v[5] + 6) >> 4;
    keep = ylo <= yb && yhi >= ya && xlo <= tx1 && xhi >= tx0;
  }
  const unsigned long long mask = __ballot(keep);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) wave_n[wave] = __popcll(mask);
  __syncthreads();
  int slot = __popcll(mask & ((1ull << lane) - 1ull)), nlist = 0;
  for (int i = 0; i < kRenderWaves; ++i) {
    if (i < wave) slot += wave_n[i];
    nlist += wave_n[i];
  }
  if (keep) {
#pragma unroll
    for (int i = 0; i < 8; ++i) lp[slot][i] = v[i];
    lp[slot][8] = ylo;
    lp[slot][9] = yhi;
    lp[slot][10] = xlo;
    lp[slot][11] = xhi;
  }

  if (!kHeat && nlist == 0) {      // the same for every thread; in place there is nothing to do
    if (out != src) render_copy(src + a, out + a, nbytes);
    return;
  }

  // stage in: px[mis + i] = byte i of the tile
  const RenderSpan sp(src + a, nbytes);
  for (int c = tid; c < sp.nchunks; c += kRenderThreads) {
    const int lo = c * 16 - sp.mis;
    if (lo >= 0 && lo + 16 <= nbytes) {
      *reinterpret_cast<uint4*>(px + c * 16) = *reinterpret_cast<const uint4*>(src + a + lo);
    } else {
      for (int q = 0; q < 16; ++q)
        if (lo + q >= 0 && lo + q < nbytes) px[c * 16 + q] = src[a + lo + q];
    }
  }
  __syncthreads();

  // layer 1.  pixel idx = tid, tid + 256, ..: (y, x) walks by addition
  if constexpr (kHeat) {
    int y = (p0 + tid) / w, x = p0 + tid - y * w;
    const int dk = kRenderThreads / w, de = kRenderThreads - dk * w;
    const size_t img = (size_t)(b0 + bi);
    for (int idx = tid; idx < np; idx += kRenderThreads) {
      uint8_t* p = px + sp.mis + idx * 3;
      int c0 = p[0], c1 = p[1], c2 = p[2];
      const double cy = render_cell(y, rb.gch[bi], h, rb.gy0[bi], ht.stride, ht.hh);
      const double cx = render_cell(x, rb.gcw[bi], w, rb.gx0[bi], ht.stride, ht.hw);
      const int iy = (int)floor(cy), ix = (int)floor(cx);
      const int iy1 = min(iy + 1, ht.hh - 1), ix1 = min(ix + 1, ht.hw - 1);
      const double ty = cy - (double)iy, tx = cx - (double)ix;
      const float* m0 = ht.hm + ((img * ht.hh + iy) * ht.hw) * ht.K;
      const float* m1 = ht.hm + ((img * ht.hh + iy1) * ht.hw) * ht.K;
      const size_t o0 = (size_t)ix * ht.K, o1 = (size_t)ix1 * ht.K;
      for (int j = 0; j < ht.K; ++j) {
        const int bits = ht.mask[j] & 7;
        const float M = ht.maxima[img * ht.K + j];
        if (bits == 0 || !(M > 0.0f)) continue;
        const double v00 = (double)m0[o0 + j], v01 = (double)m0[o1 + j], v10 = (double)m1[o0 + j], v11 = (double)m1[o1 + j];
        const double s = (1.0 - ty) * ((1.0 - tx) * v00 + tx * v01) + ty * ((1.0 - tx) * v10 + tx * v11);
        const double d = floor(s * 255.0 / (double)M + 0.5);
        const int q = !(d >= 0.0) ? 0 : d > 255.0 ? 255 : (int)d;
        const int add = (q * ht.gain + 127) / 255;
        if (bits & 1) c0 = min(255, c0 + add);
        if (bits & 2) c1 = min(255, c1 + add);
        if (bits & 4) c2 = min(255, c2 + add);
      }
      p[0] = (uint8_t)c0;
      p[1] = (uint8_t)c1;
      p[2] = (uint8_t)c2;
      y += dk;
      x += de;
      if (x >= w) {
        x -= w;
        ++y;
      }
    }
  }

  // layer 2.  One listed primitive at a time, which keeps painter's order: the work group spreads over the pixels of the primitive's box inside
  // the tile's rows (item i = tid, tid + 256, .. of the box, (row, column) by addition) and skips those of the first and last row that belong to
  // a neighbouring tile.  The barrier orders a pixel's bytes between the tint, the primitive before and this one: its thread changes.
  for (int k = 0; k < nlist; ++k) {
    __syncthreads();
    const int* e = lp[k];
    const int ay = e[1], ax = e[2], by = e[3], bx = e[4], r = e[5], rgb = e[6], alpha = e[7];
    const int y0 = max(e[8], ya), y1 = min(e[9], yb), x0 = max(e[10], tx0), x1 = min(e[11], tx1);      // not empty: the primitive passed the cull
    const int ncol = x1 - x0 + 1, n = (y1 - y0 + 1) * ncol;
    const int cr = (rgb >> 16) & 255, cg = (rgb >> 8) & 255, cb = rgb & 255;
    int ry = tid / ncol, rx = tid - ry * ncol;
    const int dk = kRenderThreads / ncol, de = kRenderThreads - dk * ncol;
    for (int i = tid; i < n; i += kRenderThreads) {
      const int y = y0 + ry, x = x0 + rx;
      const int idx = y * w + x - p0;
      if (idx >= 0 && idx < np) {
        const int ca = render_coverage(y, x, ay, ax, by, bx, r) * alpha;
        if (ca != 0) {
          uint8_t* p = px + sp.mis + idx * 3;
          p[0] = (uint8_t)((p[0] * (4080 - ca) + cr * ca + 2040) / 4080);
          p[1] = (uint8_t)((p[1] * (4080 - ca) + cg * ca + 2040) / 4080);
          p[2] = (uint8_t)((p[2] * (4080 - ca) + cb * ca + 2040) / 4080);
        }
      }
      ry += dk;
      rx += de;
      if (rx >= ncol) {
        rx -= ncol;
        ++ry;
      }
    }
  }
  __syncthreads();

  // stage out
  uint8_t* dst = out + a;
  const bool wide = sp.mis == (int)(reinterpret_cast<uintptr_t>(dst) & 15u);
  for (int c = tid; c < sp.nchunks; c += kRenderThreads) {
    const int lo = c * 16 - sp.mis;
    if (wide && lo >= 0 && lo + 16 <= nbytes) {
      *reinterpret_cast<uint4*>(dst + lo) = *reinterpret_cast<const uint4*>(px + c * 16);
    } else {
      for (int q = 0; q < 16; ++q)
        if (lo + q >= 0 && lo + q < nbytes) dst[lo + q] = px[c * 16 + q];
    }
  }
}

// workspace of render_poses: prims_dev = render_prim_ints(NP) ints, maxima = B * K floats (hm only)
size_t render_prim_ints(int NP) { return (size_t)(NP > 0 ? NP : 1) * 8; }

// src / out: the packed buffers; desc HOST int64 [B][3]; prims HOST int32 [NP][8] sorted by image; geom HOST int32 [B][4], heat_mask HOST [K] (hm only).
// Every entry has been checked by the entry point.  The host arrays are read before the call returns; ceil(NP / 120) upload launches, one launch
// for the maxima (hm), one launch per kRenderMax images.  out == src is allowed.
hipError_t render_poses(const uint8_t* src, const int64_t* desc, int B, uint8_t* out, const int32_t* prims, int NP, int32_t* prims_dev,
                        const float* hm, int hh, int hw, int K, int stride, const int32_t* geom, const uint8_t* heat_mask, int heat_gain,
                        float* maxima, hipStream_t st) {
  for (int i0 = 0; i0 < NP; i0 += kRenderPut) {
    const int n = NP - i0 < kRenderPut ? NP - i0 : kRenderPut;
    RenderPut put;
    for (int i = 0; i < n * 8; ++i) put.v[i] = prims[(size_t)i0 * 8 + i];
    hipLaunchKernelGGL(render_put_kernel, dim3(1), dim3(kRenderThreads), 0, st, put, n, prims_dev + (size_t)i0 * 8);
  }
  RenderHeat ht{};
  if (hm) {
    hipLaunchKernelGGL(render_max_kernel, dim3(B * K), dim3(kRenderThreads), 0, st, hm, hh * hw, K, maxima);
    ht.hm = hm;
    ht.maxima = maxima;
    ht.hh = hh;
    ht.hw = hw;
    ht.K = K;
    ht.stride = stride;
    ht.gain = heat_gain;
    for (int j = 0; j < K; ++j) ht.mask[j] = heat_mask[j];
  }
  int pi = 0;      // the first primitive not yet handed to an image
  for (int b0 = 0; b0 < B; b0 += kRenderMax) {
    const int nb = B - b0 < kRenderMax ? B - b0 : kRenderMax;
    RenderBatch rb{};
    for (int i = 0; i < nb; ++i) {
      const int64_t* d = desc + (size_t)(b0 + i) * 3;
      rb.off[i] = d[0];
      rb.h[i] = (int)d[1];
      rb.w[i] = (int)d[2];
      rb.first[i + 1] = rb.first[i] + (int)((d[1] * d[2] + kRenderTile - 1) / kRenderTile);
      rb.pfirst[i] = pi;
      while (pi < NP && prims[(size_t)pi * 8] == b0 + i) ++pi;
      rb.pfirst[i + 1] = pi;
      if (hm) {
        rb.gy0[i] = geom[(size_t)(b0 + i) * 4];
        rb.gx0[i] = geom[(size_t)(b0 + i) * 4 + 1];
        rb.gch[i] = geom[(size_t)(b0 + i) * 4 + 2];
        rb.gcw[i] = geom[(size_t)(b0 + i) * 4 + 3];
      }
    }
    for (int i = nb; i < kRenderMax; ++i) {
      rb.first[i + 1] = rb.first[nb];
      rb.pfirst[i + 1] = rb.pfirst[nb];
    }
    if (hm)
      hipLaunchKernelGGL((render_kernel<true>), dim3(rb.first[nb]), dim3(kRenderThreads), 0, st, src, out, rb, nb, b0, prims_dev, ht);
    else
      hipLaunchKernelGGL((render_kernel<false>), dim3(rb.first[nb]), dim3(kRenderThreads), 0, st, src, out, rb, nb, b0, prims_dev, ht);
  }
  return hipGetLastError();
}

}  // namespace

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_render_poses(jcm_handle h, const uint8_t* src, int64_t src_bytes, const int64_t* desc, int B, uint8_t* out, const int32_t* prims, int NP,
                     const float* hm, int hh, int hw, int K, int stride, const int32_t* geom, const uint8_t* heat_mask, int heat_gain) {
  JCM_TRY(check(h, false));
  const std::string who = "render_poses";
  if (!src || !desc || !out) return fail(JCM_ERR_ARG, who + ": null pointer (src, desc and out are required)");
  if (B < 1 || src_bytes < 1) return fail(JCM_ERR_ARG, who + ": B >= 1 images in src_bytes >= 1 bytes are expected");
  for (int b = 0; b < B; ++b) {
    const int64_t off = desc[b * (int64_t)3], hb = desc[b * (int64_t)3 + 1], wb = desc[b * (int64_t)3 + 2];
    const std::string img = who + ": image " + std::to_string(b);
    if (hb < 1 || hb > 16384 || wb < 1 || wb > 16384)
      return fail(JCM_ERR_ARG, img + " is " + std::to_string(hb) + " x " + std::to_string(wb) + "; both sides lie in 1..16384");
    if (off < 0 || off > src_bytes || hb * wb * 3 > src_bytes - off)
      return fail(JCM_ERR_ARG, img + " (" + std::to_string(hb * wb * 3) + " bytes at offset " + std::to_string(off) + ") does not lie inside the " +
                                   std::to_string(src_bytes) + " bytes of src");
  }
  if (out != src && ranges_overlap(src, (size_t)src_bytes, out, (size_t)src_bytes))
    return fail(JCM_ERR_ARG, who + ": out overlaps src in part (out == src, in place, is allowed)");
  if (NP < 0 || (NP > 0 && !prims)) return fail(JCM_ERR_ARG, who + ": NP >= 0 primitives are expected, and prims with NP > 0");
  constexpr int32_t kCoord = 1 << 20;
  for (int i = 0, run = 0; i < NP; ++i) {
    const int32_t* p = prims + i * (int64_t)8;
    const std::string prim = who + ": primitive " + std::to_string(i);
    if (p[0] < 0 || p[0] >= B || (i > 0 && p[0] < p[-8]))
      return fail(JCM_ERR_ARG, prim + " names image " + std::to_string(p[0]) + "; the images are 0.." + std::to_string(B - 1) + " and the list is sorted by image");
    run = i > 0 && p[0] == p[-8] ? run + 1 : 1;
    if (run > kRenderPrimMax) return fail(JCM_ERR_ARG, who + ": image " + std::to_string(p[0]) + " has more than " + std::to_string(kRenderPrimMax) + " primitives");
    for (int k = 1; k <= 4; ++k)
      if (p[k] < -kCoord || p[k] > kCoord) return fail(JCM_ERR_ARG, prim + ": coordinate " + std::to_string(p[k]) + " outside +-2^20 sixteenths of a pixel");
    if (p[5] < 0 || p[5] > (1 << 16)) return fail(JCM_ERR_ARG, prim + ": r = " + std::to_string(p[5]) + " outside 0..2^16");
    if (p[6] < 0 || p[6] > 0xFFFFFF) return fail(JCM_ERR_ARG, prim + ": rgb outside 0..0xFFFFFF");
    if (p[7] < 0 || p[7] > 255) return fail(JCM_ERR_ARG, prim + ": alpha = " + std::to_string(p[7]) + " outside 0..255");
  }
  if (hm) {
    if (!geom || !heat_mask) return fail(JCM_ERR_ARG, who + ": hm needs geom and heat_mask");
    if (K < 1 || K > 16 || hh < 1 || hw < 1 || stride < 1 || heat_gain < 0 || heat_gain > 255)
      return fail(JCM_ERR_ARG, who + ": hm needs K in 1..16, hh, hw and stride >= 1 and heat_gain in 0..255");
    if ((int64_t)B * hh * hw * K >= ((int64_t)1 << 31)) return fail(JCM_ERR_ARG, who + ": B * hh * hw * K >= 2^31");
    for (int b = 0; b < B; ++b)
      if (geom[b * (int64_t)4 + 2] < 1 || geom[b * (int64_t)4 + 3] < 1)
        return fail(JCM_ERR_ARG, who + ": geom row " + std::to_string(b) + " has a content rectangle without a pixel");
  }
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  int32_t* prims_dev = nullptr;
  float* maxima = nullptr;
  return arena_launch(c, who, [&] {
    prims_dev = arena_alloc<int32_t>(c, render_prim_ints(NP));
    if (hm) maxima = arena_alloc<float>(c, (size_t)B * K);
  }, [&] { return render_poses(src, desc, B, out, prims, NP, prims_dev, hm, hh, hw, K, stride, geom, heat_mask, heat_gain, maxima, c->stream); });
}

}  // extern "C"
