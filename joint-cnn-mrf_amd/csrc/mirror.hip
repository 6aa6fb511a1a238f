// Mirrored test-time evaluation: the two bandwidth-bound kernels around a forward that sees every image in both orientations.
//   mirror_pairs:  out[2b] = x[b], out[2b+1] = x[b] mirrored left/right -- bit copies of 4-byte (float) or 1-byte (uint8) values.
//   mirror_merge:  the mean over the G copies of a group, the odd ones (maps of mirrored inputs) read mirrored back and with the left/right
//                  channels exchanged (hm_flip.h); the float64 arithmetic of group_mean_kernel (multiscale.hip), g in order.
// mirror_pairs: a work group owns a tile of whole rows of one image (up to 32 KB, contiguous in x and in both outputs).  It reads the tile once,
// 16 bytes per lane, stores the copy from the registers and keeps the tile in LDS; the mirror is then assembled from LDS value by value and leaves
// as 16-byte stores too: x is read once, every store is a full 16 bytes per lane.  Without 16-byte alignment of every tile (odd row sizes, an
// unaligned pointer) the same kernel moves single values.
// mirror_merge: a thread owns 4 consecutive floats of out.  Even copies are 16-byte loads at the same offset; odd copies are four 4-byte loads
// from the mirrored pixels -- the lanes of a wave still cover the same contiguous KiB of the copy, in another order, so every fetched line is used.
#include <string>

#include "entry.h"
#include "hm_flip.h"

namespace jcm {

namespace {

constexpr int kMpThreads = 256;
constexpr int kMpTileBytes = 32 * 1024;      // the tile a work group stages: two work groups per CU and more
constexpr int kMpRowBytesMax = 64 * 1024;    // one row must fit the LDS a launch gets without an attribute
constexpr int kMmThreads = 256;
constexpr int kMmMaxK = 64;                  // channels of a map: the table travels in the kernel arguments

struct MirrorPerm {
  int v[kMmMaxK];
};

// T: uint32_t (the bits of a float) or uint8_t.  Tile `tile` of image b = rows [tile * R, min(H, tile * R + R)); vec != 0: every tile starts on
// 16 bytes in x and in out and is a whole number of 16-byte chunks (arranged on the host), which move as such; vec == 0: value by value.
template <class T>
__global__ __launch_bounds__(kMpThreads) void mirror_pairs_kernel(const T* __restrict__ x, T* __restrict__ out, int H, int W, int C, int R, int tiles, int vec) {
  extern __shared__ uint4 mp_lds[];
  constexpr int E = 16 / (int)sizeof(T);
  T* s = reinterpret_cast<T*>(mp_lds);
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int y0 = tile * R;
  const int rows = min(R, H - y0);
  const int row = W * C;                  // values per row
  const int n = rows * row;               // values of this tile (<= 64 KB / sizeof(T))
  const size_t img = (size_t)H * row;
  const T* src = x + (size_t)b * img + (size_t)y0 * row;
  T* dc = out + (size_t)(2 * b) * img + (size_t)y0 * row;
  T* dm = dc + img;
  const int nv = vec ? n / E : 0;
  const int t = threadIdx.x;
  for (int i = t; i < nv; i += kMpThreads) {
    const uint4 v = reinterpret_cast<const uint4*>(src)[i];
    reinterpret_cast<uint4*>(dc)[i] = v;
    mp_lds[i] = v;
  }
  for (int e = nv * E + t; e < n; e += kMpThreads) {
    const T v = src[e];
    dc[e] = v;
    s[e] = v;
  }
  __syncthreads();
  for (int i = t; i < nv; i += kMpThreads) {
    const int e = i * E;
    int r = e / row;
    const int rem = e - r * row;
    int p = rem / C, c = rem - p * C;
    union {
      T v[E];
      uint4 q;
    } u;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      u.v[j] = s[r * row + (W - 1 - p) * C + c];
      if (++c == C) {
        c = 0;
        if (++p == W) {
          p = 0;
          ++r;
        }
      }
    }
    reinterpret_cast<uint4*>(dm)[i] = u.q;
  }
  for (int e = nv * E + t; e < n; e += kMpThreads) {
    const int r = e / row, rem = e - r * row;
    const int p = rem / C, c = rem - p * C;
    dm[e] = s[r * row + (W - 1 - p) * C + c];
  }
}

// V = 4: M % 4 == 0 and hm, out on 16 bytes (a chunk never crosses an image); V = 1 otherwise.  M = HH * WW * K values per map, total = n * M / V.
template <int V>
__global__ __launch_bounds__(kMmThreads) void mirror_merge_kernel(const float* __restrict__ hm, float* __restrict__ out, int G, int WW, int K, unsigned M,
                                                                  size_t total, MirrorPerm perm) {
  __shared__ int s_perm[kMmMaxK];
  if ((int)threadIdx.x < kMmMaxK) s_perm[threadIdx.x] = perm.v[threadIdx.x];
  __syncthreads();
  const unsigned mc = M / V;
  for (size_t i = (size_t)blockIdx.x * kMmThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kMmThreads) {
    const size_t im = i / mc;
    const unsigned e0 = (unsigned)(i - im * mc) * V;
    unsigned pix = e0 / (unsigned)K;
    unsigned k = e0 - pix * K;
    unsigned y = pix / (unsigned)WW;
    unsigned xx = pix - y * WW;
    unsigned off[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      off[j] = (y * WW + (WW - 1 - xx)) * K + s_perm[k];
      if (++k == (unsigned)K) {
        k = 0;
        if (++xx == (unsigned)WW) {
          xx = 0;
          ++y;
        }
      }
    }
    double acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0;
    const float* even = hm + im * G * M + e0;
    const float* odd = hm + (im * G + 1) * M;
    for (int g = 0; g < G; g += 2, even += 2 * (size_t)M, odd += 2 * (size_t)M) {
      float ev[V], od[V];
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(even);
        ev[0] = q.x;
        ev[1] = q.y;
        ev[2] = q.z;
        ev[3] = q.w;
      } else {
        ev[0] = even[0];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) od[j] = odd[off[j]];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        acc[j] += (double)ev[j];
        acc[j] += (double)od[j];
      }
    }
    float r[V];
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = (float)(acc[j] / (double)G);
    float* dst = out + im * M + e0;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
      dst[0] = r[0];
    }
  }
}

int gcd_int(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

hipError_t mirror_pairs(const void* x, bool x_u8, int B, int H, int W, int C, void* out, hipStream_t st) {
  const int es = x_u8 ? 1 : 4;
  const int64_t rb = (int64_t)W * C * es;      // bytes per row
  if (B < 1 || H < 1 || W < 1 || C < 1 || rb > kMpRowBytesMax) return hipErrorInvalidValue;
  int R = (int)std::max<int64_t>(1, std::min<int64_t>(H, kMpTileBytes / rb));
  int vec = aligned16(x) && aligned16(out) && ((int64_t)H * rb) % 16 == 0;
  if (vec && R < H) {      // every tile but an image's last must be whole 16-byte chunks
    const int step = 16 / gcd_int((int)(rb % 16 == 0 ? 16 : rb % 16), 16);
    if (R >= step) R = R / step * step;
    else if (step * rb <= kMpRowBytesMax && step < H) R = step;
    else vec = 0;
  }
  const int tiles = (H + R - 1) / R;
  if ((int64_t)B * tiles >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  const size_t lds = ((size_t)R * rb + 15) / 16 * 16;
  if (x_u8)
    hipLaunchKernelGGL(mirror_pairs_kernel<uint8_t>, dim3(B * tiles), dim3(kMpThreads), lds, st, static_cast<const uint8_t*>(x), static_cast<uint8_t*>(out), H,
                       W, C, R, tiles, vec);
  else
    hipLaunchKernelGGL(mirror_pairs_kernel<uint32_t>, dim3(B * tiles), dim3(kMpThreads), lds, st, static_cast<const uint32_t*>(x), static_cast<uint32_t*>(out), H,
                       W, C, R, tiles, vec);
  return hipGetLastError();
}

// perm: K host entries, a permutation of 0..K-1 (checked by the caller), K <= 64
hipError_t mirror_merge(const float* hm, int n, int G, int HH, int WW, int K, const int* perm, float* out, hipStream_t st) {
  const int64_t M = (int64_t)HH * WW * K;
  if (n < 1 || G < 2 || G % 2 || HH < 1 || WW < 1 || K < 1 || K > kMmMaxK || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  MirrorPerm p;
  for (int k = 0; k < kMmMaxK; ++k) p.v[k] = k < K ? perm[k] : 0;
  const bool v4 = M % 4 == 0 && aligned16(hm) && aligned16(out);
  const size_t total = (size_t)n * (size_t)M / (v4 ? 4 : 1);
  const size_t g = (total + kMmThreads - 1) / kMmThreads;
  const dim3 grid((unsigned)std::min<size_t>(g, 16384));
  if (v4)
    hipLaunchKernelGGL(mirror_merge_kernel<4>, grid, dim3(kMmThreads), 0, st, hm, out, G, WW, K, (unsigned)M, total, p);
  else
    hipLaunchKernelGGL(mirror_merge_kernel<1>, grid, dim3(kMmThreads), 0, st, hm, out, G, WW, K, (unsigned)M, total, p);
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_mirror_pairs(jcm_handle h, const void* x, int x_u8, int B, int H, int W, int C, void* out) {
  JCM_TRY(check(h, false));
  if (!x || !out) return fail(JCM_ERR_ARG, "mirror_pairs: null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 1) return fail(JCM_ERR_ARG, "mirror_pairs: bad sizes (B, H, W, C >= 1)");
  const int es = x_u8 ? 1 : 4;
  if ((int64_t)W * C * es > kMpRowBytesMax)
    return fail(JCM_ERR_ARG, "mirror_pairs: a row of " + std::to_string((int64_t)W * C * es) + " bytes; W * C * sizeof(value) <= 65536 (a row is staged in LDS)");
  if ((int64_t)H * W * C >= ((int64_t)1 << 31) || (int64_t)B * 2 >= ((int64_t)1 << 31)) return fail(JCM_ERR_ARG, "mirror_pairs: bad sizes (H * W * C < 2^31, B < 2^30)");
  const size_t nx = (size_t)B * H * W * C * es;
  if (ranges_overlap(x, nx, out, 2 * nx)) return fail(JCM_ERR_ARG, "mirror_pairs: out overlaps x");
  DeviceGuard g(h->device);
  CallOrder order(h);
  return timed_launch(h, "mirror_pairs", [&] { return mirror_pairs(x, x_u8 != 0, B, H, W, C, out, h->stream); });
}

int jcm_mirror_merge(jcm_handle h, const float* hm, int n, int G, int HH, int WW, int K, const int32_t* perm, float* out) {
  JCM_TRY(check(h, false));
  if (!hm || !out) return fail(JCM_ERR_ARG, "mirror_merge: null pointer");
  if (G < 2 || G % 2) return fail(JCM_ERR_ARG, "mirror_merge: G = " + std::to_string(G) + " copies per group; G is even (copy 2s + 1 is the mirror image of copy 2s) and >= 2");
  if (n < 1 || HH < 1 || WW < 1 || K < 1) return fail(JCM_ERR_ARG, "mirror_merge: bad sizes (n, HH, WW, K >= 1)");
  if (!perm && K > kHmFlipChannels) return fail(JCM_ERR_ARG, "mirror_merge: perm == NULL is the FLIC table of 10 channels; K = " + std::to_string(K) + " needs a perm");
  if (K > kMmMaxK) return fail(JCM_ERR_ARG, "mirror_merge: K = " + std::to_string(K) + " channels; K <= 64");
  if ((int64_t)HH * WW * K >= ((int64_t)1 << 31)) return fail(JCM_ERR_ARG, "mirror_merge: bad sizes (HH * WW * K < 2^31)");
  int table[kMmMaxK];
  bool seen[kMmMaxK] = {};
  for (int k = 0; k < K; ++k) {
    const int v = perm ? perm[k] : kHmFlipPerm[k];
    if (v < 0 || v >= K || seen[v])
      return fail(JCM_ERR_ARG, "mirror_merge: perm is not a permutation of 0.." + std::to_string(K - 1) + " (entry " + std::to_string(k) + " = " + std::to_string(v) + ")");
    seen[v] = true;
    table[k] = v;
  }
  const size_t no = (size_t)n * HH * WW * K * sizeof(float);
  if (ranges_overlap(hm, no * G, out, no)) return fail(JCM_ERR_ARG, "mirror_merge: out overlaps hm");
  DeviceGuard g(h->device);
  CallOrder order(h);
  return timed_launch(h, "mirror_merge", [&] { return mirror_merge(hm, n, G, HH, WW, K, table, out, h->stream); });
}

}  // extern "C"
