// Rendered people (include/jcm.h: jcm_synth_people): out[B,H,W,3] bytes from one scene record and one list of primitives per image --
// a gradient with four octaves of value noise, capsules and convex quadrilaterals over it in painter's order, sensor noise on top.  Every step is
// integer arithmetic stated in jcm.h (the capsule test: float64 products of small integers, exact), so a sequential restatement gives every byte.
//   * a work group owns kSynthTile consecutive pixels of one image in row-major order (blockIdx.y = the image), as render.hip's does: the tile is
//     ONE contiguous range of the output whatever the width, composed in LDS and stored by 16-byte stores wherever a whole aligned chunk lies
//     inside the range (the first and the last chunk element by element: nothing outside the tile is written).
//   * the background is the cost every pixel pays.  An octave of shift s needs the lattice values of ((rows of the tile) >> s) + 2 by
//     ((columns) >> s) + 2 points: they are hashed ONCE per tile into LDS (a byte each) where there are at most kSynthLat of them, and a pixel
//     then reads four bytes per octave.  An octave with more points than that -- cells of one pixel under a full tile, every pixel its own hash --
//     is hashed per pixel (at s = 0 that is one hash: the weights of the other three corners are zero).  An octave of amplitude 0 is skipped.
//   * the image's primitives (at most 64, one lane of wave 0 each) are culled against the tile's rows -- for a tile inside one row, also its
//     columns -- by bounding box into an LDS list in listing order (ballot + prefix count), and drawn one after the other, the work group spread
//     over the pixels of the primitive's box inside the tile: the 16 sub-sample test and the texture hash run for those pixels only.
//   * records and primitives travel in the arguments of small launches into workspace (SynthPut, as render.hip's RenderPut): nothing is copied
//     from caller-owned host memory asynchronously.
#include <string>

#include "coverage.h"
#include "entry.h"
#include "u8.h"

namespace jcm {

namespace {

constexpr int kSynthThreads = 256;
constexpr int kSynthBytes = kSynthTile * 3;
constexpr int kSynthPut = 960;        // ints per upload launch: 3840 of the 4096 bytes of its arguments (60 primitives, 48 records)
constexpr int kSynthLat = 4096;       // lattice values per octave held in LDS
constexpr uint32_t kSynthNoiseKey = 0x5BD1E995u;      // jcm.h: JCM_SYNTH_NOISE_KEY

struct SynthPut {
  int32_t v[kSynthPut];
};
__global__ __launch_bounds__(kSynthThreads) void synth_put_kernel(SynthPut p, int n, int32_t* __restrict__ dst) {
  for (int i = threadIdx.x; i < n; i += kSynthThreads) dst[i] = p.v[i];
}

// jcm.h: hash32
__device__ __forceinline__ uint32_t synth_hash(uint32_t seed, uint32_t i, uint32_t j) {
  uint32_t h = (seed * 0x9E3779B1u) ^ (i * 0x85EBCA77u) ^ (j * 0xC2B2AE3Du);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ int synth_bilinear(int s, int y, int x, int L00, int L01, int L10, int L11) {
  const int cell = 1 << s, fy = y & (cell - 1), fx = x & (cell - 1);
  return ((cell - fy) * ((cell - fx) * L00 + fx * L01) + fy * ((cell - fx) * L10 + fx * L11)) >> (2 * s);
}

// jcm.h: vnoise, every lattice value hashed here
__device__ __forceinline__ int synth_vnoise(uint32_t seed, int s, int y, int x) {
  const uint32_t i = (uint32_t)(y >> s), j = (uint32_t)(x >> s);
  const int L00 = (int)(synth_hash(seed, i, j) >> 24);
  if (s == 0) return L00;      // cell = 1: fy = fx = 0, the other corners have weight 0
  return synth_bilinear(s, y, x, L00, (int)(synth_hash(seed, i, j + 1) >> 24), (int)(synth_hash(seed, i + 1, j) >> 24),
                        (int)(synth_hash(seed, i + 1, j + 1) >> 24));
}

__device__ __forceinline__ int synth_clamp(int v) { return min(255, max(0, v)); }

// floor(n / d), d > 0
template <class T>
__device__ __forceinline__ T synth_floor_div(T n, T d) {
  const T q = n / d;
  return (n % d != 0 && n < 0) ? q - 1 : q;
}

template <bool kF32>
__global__ __launch_bounds__(kSynthThreads) void synth_people_kernel(const int32_t* __restrict__ recs, const int32_t* __restrict__ prims, int H, int W,
                                                                     void* out) {
  __shared__ __align__(16) uint8_t px[kSynthBytes + 16];
  __shared__ uint8_t lat[4][kSynthLat];
  __shared__ int lp[kSynthPrimMax][kSynthPrimInts + 4];      // a listed primitive: its record, then the pixels its box can touch: ylo, yhi, xlo, xhi
  __shared__ int nlist_s;
  const int tid = threadIdx.x, b = blockIdx.y;
  const int32_t* rec = recs + (size_t)b * kSynthRecInts;
  const int hw = H * W;                                      // <= INT32_MAX (checked by the caller)
  const int p0 = (int)blockIdx.x * kSynthTile;               // < hw
  const int np = min(kSynthTile, hw - p0), nbytes = np * 3;
  const size_t a = ((size_t)b * (size_t)hw + (size_t)p0) * 3;      // the tile's first element of out
  const int ya = p0 / W, xa = p0 - ya * W;
  const int yb = (p0 + np - 1) / W, xb = p0 + np - 1 - yb * W;
  const int tx0 = ya == yb ? xa : 0, tx1 = ya == yb ? xb : W - 1;
  const uint32_t seed = (uint32_t)rec[0];

  // cull: lane i of wave 0 takes primitive i of the image
  if (tid < 64) {
    const int pn = rec[16], pbase = rec[17];
    int v[kSynthPrimInts], ylo = 0, yhi = 0, xlo = 0, xhi = 0;
    bool keep = false;
    if (tid < pn) {
      const int4* q = reinterpret_cast<const int4*>(prims + (size_t)(pbase + tid) * kSynthPrimInts);      // workspace: 256-byte aligned, 64 bytes a primitive
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int4 t = q[i];
        v[4 * i] = t.x;
        v[4 * i + 1] = t.y;
        v[4 * i + 2] = t.z;
        v[4 * i + 3] = t.w;
      }
      int y0, y1, x0, x1;
      if (v[0] == 0) {      // capsule: the segment's box grown by r
        y0 = min(v[1], v[3]) - v[5];
        y1 = max(v[1], v[3]) + v[5];
        x0 = min(v[2], v[4]) - v[5];
        x1 = max(v[2], v[4]) + v[5];
      } else {
        y0 = min(min(v[1], v[3]), min(v[5], v[7]));
        y1 = max(max(v[1], v[3]), max(v[5], v[7]));
        x0 = min(min(v[2], v[4]), min(v[6], v[8]));
        x1 = max(max(v[2], v[4]), max(v[6], v[8]));
      }
      // pixel y has samples at 16 y - 6 .. 16 y + 6: it can be touched if 16 y + 6 >= lo and 16 y - 6 <= hi (>> 4 floors; the low end may be one early)
      ylo = (y0 - 6) >> 4;
      yhi = (y1 + 6) >> 4;
      xlo = (x0 - 6) >> 4;
      xhi = (x1 + 6) >> 4;
      keep = ylo <= yb && yhi >= ya && xlo <= tx1 && xhi >= tx0;
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const int slot = __popcll(mask & ((1ull << tid) - 1ull));
#pragma unroll
      for (int i = 0; i < kSynthPrimInts; ++i) lp[slot][i] = v[i];
      lp[slot][kSynthPrimInts] = ylo;
      lp[slot][kSynthPrimInts + 1] = yhi;
      lp[slot][kSynthPrimInts + 2] = xlo;
      lp[slot][kSynthPrimInts + 3] = xhi;
    }
    if (tid == 0) nlist_s = __popcll(mask);
  }

  // the octaves: lattice points (r0 + r, c0 + c), r < nr, c < nc, cover every pixel of the tile and its lower / right neighbours
  int amp[4], sh[4], r0[4], c0[4], nc[4];
  bool inl[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    amp[o] = rec[7 + o];
    sh[o] = rec[11 + o];
    r0[o] = ya >> sh[o];
    c0[o] = tx0 >> sh[o];
    const int64_t nc64 = (int64_t)(tx1 >> sh[o]) - c0[o] + 2;      // a tile that spans rows has all W columns: up to 2^31 at s = 0
    const int64_t cnt64 = ((int64_t)(yb >> sh[o]) - r0[o] + 2) * nc64;
    inl[o] = cnt64 <= kSynthLat;
    nc[o] = inl[o] ? (int)nc64 : 0;      // read only where the lattice is in LDS
    if (amp[o] != 0 && inl[o]) {
      const int cnt = (int)cnt64;
      for (int i = tid; i < cnt; i += kSynthThreads) {
        const int r = i / nc[o], c = i - r * nc[o];
        lat[o][i] = (uint8_t)(synth_hash(seed + (uint32_t)o, (uint32_t)(r0[o] + r), (uint32_t)(c0[o] + c)) >> 24);
      }
    }
  }
  __syncthreads();

  const int mis = kF32 ? 0 : (int)(reinterpret_cast<uintptr_t>(static_cast<uint8_t*>(out) + a) & 15u);      // px[mis + i] = byte i of the tile
  uint8_t* const tile = px + mis;

  // the background.  pixel idx = tid, tid + 256, ..: (y, x) walks by addition
  {
    const int den = max(H - 1, 1);
    const bool narrow = H <= (1 << 23);      // 255 * y stays inside int32
    int d[3], g[3] = {0, 0, 0}, gy = -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = rec[4 + k] - rec[1 + k];
    const int pt = p0 + min(tid, np - 1);      // (a thread past the tile's end walks nothing: p0 + tid may not fit int)
    int y = pt / W, x = pt - y * W;
    const int dk = kSynthThreads / W, de = kSynthThreads - dk * W;
    for (int idx = tid; idx < np; idx += kSynthThreads) {
      if (y != gy) {
        gy = y;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          g[k] = rec[1 + k] + (narrow ? synth_floor_div<int>(d[k] * y, den) : (int)synth_floor_div<int64_t>((int64_t)d[k] * y, (int64_t)den));
      }
      int nsum = 0;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (amp[o] == 0) continue;
        int vn;
        if (inl[o]) {
          const uint8_t* L = lat[o] + ((y >> sh[o]) - r0[o]) * nc[o] + ((x >> sh[o]) - c0[o]);
          vn = synth_bilinear(sh[o], y, x, L[0], L[1], L[nc[o]], L[nc[o] + 1]);
        } else {
          vn = synth_vnoise(seed + (uint32_t)o, sh[o], y, x);
        }
        nsum += (amp[o] * (vn - 128)) >> 8;      // floor(. / 256)
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) tile[idx * 3 + k] = (uint8_t)synth_clamp(g[k] + nsum);
      y += dk;
      x += de;
      if (x >= W) {
        x -= W;
        ++y;
      }
    }
  }

  // the primitives.  One listed primitive at a time, which keeps painter's order: the work group spreads over the pixels of the primitive's box
  // inside the tile's rows and skips those of the first and last row that belong to a neighbouring tile.  The barrier orders a pixel's bytes
  // between the background, the primitive before and this one: its thread changes.
  const int nlist = nlist_s;      // written before the barrier above
  for (int k = 0; k < nlist; ++k) {
    __syncthreads();
    const int* e = lp[k];
    int q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = e[1 + i];
    const int kind = e[0], tamp = e[12], ts = e[13];
    const uint32_t tseed = (uint32_t)e[14];
    const int col[3] = {e[9], e[10], e[11]};
    const int y0 = max(e[16], ya), y1 = min(e[17], yb), x0 = max(e[18], tx0), x1 = min(e[19], tx1);      // not empty: the primitive passed the cull
    const int ncol = x1 - x0 + 1;                                  // <= W
    const int64_t n = (int64_t)(y1 - y0 + 1) * ncol;               // rows of the tile times W: past int for a very wide image
    int ry = tid / ncol, rx = tid - ry * ncol;
    const int dk = kSynthThreads / ncol, de = kSynthThreads - dk * ncol;
    for (int64_t i = tid; i < n; i += kSynthThreads) {
      const int y = y0 + ry, x = x0 + rx;
      const int idx = y * W + x - p0;
      if (idx >= 0 && idx < np) {
        const int c = kind == 0 ? render_coverage(y, x, q[0], q[1], q[2], q[3], q[4]) : quad_coverage(y, x, q);
        if (c != 0) {
          const int tex = tamp == 0 ? 0 : (tamp * (synth_vnoise(tseed, ts, y, x) - 128)) >> 8;
          uint8_t* p = tile + idx * 3;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) p[ch] = (uint8_t)((c * synth_clamp(col[ch] + tex) + (16 - c) * p[ch] + 8) >> 4);
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

  // sensor noise: y * W + x = p0 + idx
  const int na = rec[15];
  if (na > 0) {
    const uint32_t m = 2u * (uint32_t)na + 1u, nseed = seed ^ kSynthNoiseKey;
    for (int idx = tid; idx < np; idx += kSynthThreads) {
      uint8_t* p = tile + idx * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) p[ch] = (uint8_t)synth_clamp((int)p[ch] + (int)(synth_hash(nseed, (uint32_t)(p0 + idx), (uint32_t)ch) % m) - na);
    }
    __syncthreads();
  }

  // stage out
  if constexpr (kF32) {
    float* dst = static_cast<float*>(out) + a;
    const int misf = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u), nchunks = (misf + nbytes + 3) >> 2;
    for (int c = tid; c < nchunks; c += kSynthThreads) {
      const int lo = c * 4 - misf;
      if (lo >= 0 && lo + 4 <= nbytes) {
        *reinterpret_cast<float4*>(dst + lo) = make_float4(u8_to_f32(tile[lo]), u8_to_f32(tile[lo + 1]), u8_to_f32(tile[lo + 2]), u8_to_f32(tile[lo + 3]));
      } else {
        for (int i = 0; i < 4; ++i)
          if (lo + i >= 0 && lo + i < nbytes) dst[lo + i] = u8_to_f32(tile[lo + i]);
      }
    }
  } else {
    uint8_t* dst = static_cast<uint8_t*>(out) + a;
    const int nchunks = (mis + nbytes + 15) >> 4;
    for (int c = tid; c < nchunks; c += kSynthThreads) {
      const int lo = c * 16 - mis;
      if (lo >= 0 && lo + 16 <= nbytes) {
        *reinterpret_cast<uint4*>(dst + lo) = *reinterpret_cast<const uint4*>(px + c * 16);
      } else {
        for (int i = 0; i < 16; ++i)
          if (lo + i >= 0 && lo + i < nbytes) dst[lo + i] = px[c * 16 + i];
      }
    }
  }
}

void synth_put(const int32_t* host, size_t n, int32_t* dev, hipStream_t st) {
  for (size_t i0 = 0; i0 < n; i0 += kSynthPut) {
    const int m = (int)(n - i0 < (size_t)kSynthPut ? n - i0 : (size_t)kSynthPut);
    SynthPut put;
    for (int i = 0; i < m; ++i) put.v[i] = host[i0 + i];
    hipLaunchKernelGGL(synth_put_kernel, dim3(1), dim3(kSynthThreads), 0, st, put, m, dev + i0);
  }
}

// records HOST int32 [B][20], prims HOST int32 [NP][16], every entry checked by the entry point; both are read before the call returns: they go
// into records_dev (B * 20 ints) and prims_dev (max(NP, 1) * 16 ints) of the workspace by ceil(n / 960) small launches that carry them in their
// arguments.  out: uint8 [B,H,W,3], or float32 (out_f32) = byte / 255.  One more launch.
hipError_t synth_people(const int32_t* records, int B, const int32_t* prims, int NP, int H, int W, bool out_f32, void* out, int32_t* records_dev,
                        int32_t* prims_dev, hipStream_t st) {
  synth_put(records, (size_t)B * kSynthRecInts, records_dev, st);
  synth_put(prims, (size_t)NP * kSynthPrimInts, prims_dev, st);
  const int64_t hw = (int64_t)H * W;
  const dim3 grid((unsigned)((hw + kSynthTile - 1) / kSynthTile), (unsigned)B);
  if (out_f32) hipLaunchKernelGGL((synth_people_kernel<true>), grid, dim3(kSynthThreads), 0, st, records_dev, prims_dev, H, W, out);
  else hipLaunchKernelGGL((synth_people_kernel<false>), grid, dim3(kSynthThreads), 0, st, records_dev, prims_dev, H, W, out);
  return hipGetLastError();
}

}  // namespace

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_synth_people(jcm_handle h, const int32_t* records, int B, const int32_t* prims, int NP, int H, int W, int out_f32, void* out) {
  JCM_TRY(check(h, false));
  const std::string who = "synth_people";
  if (!records || !out) return fail(JCM_ERR_ARG, who + ": null pointer (records and out are required)");
  if (B < 1 || B > 65535) return fail(JCM_ERR_ARG, who + ": B = " + std::to_string(B) + " outside 1..65535");
  if (H < 1 || W < 1) return fail(JCM_ERR_ARG, who + ": H and W >= 1 are expected, got " + std::to_string(H) + " x " + std::to_string(W));
  if ((int64_t)H * W > (int64_t)INT32_MAX) return fail(JCM_ERR_ARG, who + ": H * W = " + std::to_string((int64_t)H * W) + " is over the int32 range");
  if (NP < 0 || (NP > 0 && !prims)) return fail(JCM_ERR_ARG, who + ": NP >= 0 primitives are expected, and prims with NP > 0");
  if (out_f32 && (reinterpret_cast<uintptr_t>(out) & 3u)) return fail(JCM_ERR_ARG, who + ": a float32 out is 4-byte aligned");
  auto byte = [](int32_t v) { return v >= 0 && v <= 255; };
  for (int b = 0; b < B; ++b) {
    const int32_t* r = records + b * (int64_t)kSynthRecInts;
    const std::string img = who + ": image " + std::to_string(b);
    for (int k = 1; k <= 6; ++k)
      if (!byte(r[k])) return fail(JCM_ERR_ARG, img + ": background colour " + std::to_string(r[k]) + " outside 0..255");
    for (int o = 0; o < 4; ++o) {
      if (!byte(r[7 + o])) return fail(JCM_ERR_ARG, img + ": octave amplitude " + std::to_string(r[7 + o]) + " outside 0..255");
      if (r[11 + o] < 0 || r[11 + o] > 8) return fail(JCM_ERR_ARG, img + ": octave shift " + std::to_string(r[11 + o]) + " outside 0..8");
    }
    if (!byte(r[15])) return fail(JCM_ERR_ARG, img + ": sensor-noise amplitude " + std::to_string(r[15]) + " outside 0..255");
    if (r[16] < 0 || r[16] > kSynthPrimMax)
      return fail(JCM_ERR_ARG, img + ": n = " + std::to_string(r[16]) + " primitives outside 0.." + std::to_string(kSynthPrimMax));
    if (r[17] < 0 || (int64_t)r[17] + r[16] > NP)
      return fail(JCM_ERR_ARG, img + ": primitives " + std::to_string(r[17]) + ".." + std::to_string((int64_t)r[17] + r[16]) + " do not lie inside the " +
                                   std::to_string(NP) + " of prims");
  }
  constexpr int32_t kCoord = 1 << 20;
  for (int i = 0; i < NP; ++i) {
    const int32_t* p = prims + i * (int64_t)kSynthPrimInts;
    const std::string prim = who + ": primitive " + std::to_string(i);
    if (p[0] != 0 && p[0] != 1) return fail(JCM_ERR_ARG, prim + ": kind " + std::to_string(p[0]) + " is neither 0 (capsule) nor 1 (quadrilateral)");
    for (int k = 1; k <= (p[0] == 0 ? 4 : 8); ++k)
      if (p[k] < -kCoord || p[k] > kCoord) return fail(JCM_ERR_ARG, prim + ": coordinate " + std::to_string(p[k]) + " outside +-2^20 sixteenths of a pixel");
    if (p[0] == 0 && (p[5] < 0 || p[5] > (1 << 16))) return fail(JCM_ERR_ARG, prim + ": r = " + std::to_string(p[5]) + " outside 0..2^16");
    for (int k = 9; k <= 11; ++k)
      if (!byte(p[k])) return fail(JCM_ERR_ARG, prim + ": colour " + std::to_string(p[k]) + " outside 0..255");
    if (!byte(p[12])) return fail(JCM_ERR_ARG, prim + ": texture amplitude " + std::to_string(p[12]) + " outside 0..255");
    if (p[13] < 0 || p[13] > 8) return fail(JCM_ERR_ARG, prim + ": texture shift " + std::to_string(p[13]) + " outside 0..8");
  }
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  int32_t *records_dev = nullptr, *prims_dev = nullptr;
  return arena_launch(c, who, [&] {
    records_dev = arena_alloc<int32_t>(c, (size_t)B * kSynthRecInts);
    prims_dev = arena_alloc<int32_t>(c, (size_t)(NP > 0 ? NP : 1) * kSynthPrimInts);
  }, [&] { return synth_people(records, B, prims, NP, H, W, out_f32 != 0, out, records_dev, prims_dev, c->stream); });
}

}  // extern "C"
