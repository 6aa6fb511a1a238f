// Camera pans: the global whole-pixel translation between consecutive fitted frames, a two-level exhaustive block match on integer
// luma.  Every step is integer arithmetic and every sum is order-free, so the result does not depend on how the work is cut; include/jcm.h
// (jcm_frame_shift) is the definition, tests/frame_shift_ref.py its restatement.
// Five kinds of launch on the handle's stream, nothing read back in between:
//   fs_luma_kernel     L = R + 2G + B of the content rectangle of every frame (and of `prev`), uint16 [frame][ch][cw] in the workspace.  One wave per
//                      row; four pixels = three dwords per lane where the rows are dword aligned (WIDE, chosen per call: W % 4 == 0 and both bases
//                      4-byte aligned), bytes otherwise and at the rectangle's ragged ends.  Nothing outside the rectangle is read.
//   fs_coarse_kernel   C = 4 x 4 block sums of L, uint16 [frame][Hc][Wc] (16 * 1020 fits).
//   fs_sad_coarse      one work group per (pair, dy, chunk of rows): the rows of C_t and the rows dy away of C_{t-1} staged in LDS, then per dx a
//                      per-thread partial sum, a wave reduction, an LDS add and ONE 64-bit global atomic per candidate and work group.
//   fs_sad_fine        one work group per (pair, chunk of rows): the rows of L_{t-1} around the coarse winner (read from device memory) staged in
//                      LDS, 6 rows and 6 columns more than the chunk; every pixel of L_t is read once and meets its 49 neighbours from LDS and the
//                      pixel of zero displacement from global memory: 50 register accumulators, reduced as above.
//   fs_argmin_*        one wave per pair: the candidate that minimises (S, dy^2 + dx^2, dy, dx).
// Per-thread, per-wave and per-group sums are uint32: each is part of one candidate's sum, which is at most H * W * 1020 < 2^32 (checked by the
// entry point).  The slots the groups add into are uint64.
#include <string>

#include "entry.h"

namespace jcm {

namespace {

constexpr int kFsThreads = 256;      // 4 waves; dim3(64, 4) in the plane kernels: one wave per row
constexpr int kFsFine = 50;          // 7 x 7 fine candidates and, last, zero displacement
constexpr int kFsPartBytes = 256;    // the group's candidate sums in front of the tiles (64 uint32; the tiles stay 16-byte aligned)
constexpr int kFsTileBytes = 48 * 1024;

__device__ __forceinline__ unsigned fs_absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

__device__ __forceinline__ unsigned fs_wave_sum(unsigned v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// slot f of the planes: f == 0 is `prev`, f >= 1 frame f - 1 of x
__device__ __forceinline__ const uint8_t* fs_frame(const uint8_t* x, const uint8_t* prev, int f, size_t frame_bytes) {
  return f == 0 ? prev : x + (size_t)(f - 1) * frame_bytes;
}

template <bool WIDE>
__global__ __launch_bounds__(kFsThreads) void fs_luma_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ prev, int H, int W, int y0, int x0,
                                                             int ch, int cw, int f0, uint16_t* __restrict__ L) {
  const int f = f0 + blockIdx.y;
  const uint8_t* src = fs_frame(x, prev, f, (size_t)H * W * 3);
  uint16_t* dst = L + (size_t)f * ch * cw;
  const int lane = threadIdx.x;
  for (int y = blockIdx.x * 4 + threadIdx.y; y < ch; y += gridDim.x * 4) {
    const uint8_t* row = src + ((size_t)(y0 + y) * W) * 3;
    uint16_t* out = dst + (size_t)y * cw;
    if constexpr (WIDE) {
      const int g0 = x0 / 4, g1 = (x0 + cw + 3) / 4;      // groups of four pixels = 12 bytes, dword aligned in a dword-aligned row
      for (int g = g0 + lane; g < g1; g += 64) {
        const int px = 4 * g;
        if (px >= x0 && px + 4 <= x0 + cw) {
          const unsigned* p = reinterpret_cast<const unsigned*>(row + (size_t)px * 3);
          const unsigned a = p[0], b = p[1], c = p[2];
          uint16_t* o = out + (px - x0);
          o[0] = (uint16_t)((a & 255u) + 2u * ((a >> 8) & 255u) + ((a >> 16) & 255u));
          o[1] = (uint16_t)((a >> 24) + 2u * (b & 255u) + ((b >> 8) & 255u));
          o[2] = (uint16_t)(((b >> 16) & 255u) + 2u * (b >> 24) + (c & 255u));
          o[3] = (uint16_t)(((c >> 8) & 255u) + 2u * ((c >> 16) & 255u) + (c >> 24));
        } else {
          for (int q = px < x0 ? x0 : px; q < px + 4 && q < x0 + cw; ++q) {
            const uint8_t* p = row + (size_t)q * 3;
            out[q - x0] = (uint16_t)((unsigned)p[0] + 2u * p[1] + p[2]);
          }
        }
      }
    } else {
      for (int q = lane; q < cw; q += 64) {
        const uint8_t* p = row + (size_t)(x0 + q) * 3;
        out[q] = (uint16_t)((unsigned)p[0] + 2u * p[1] + p[2]);
      }
    }
  }
}

__global__ __launch_bounds__(kFsThreads) void fs_coarse_kernel(const uint16_t* __restrict__ L, int ch, int cw, int Hc, int Wc, int f0, uint16_t* __restrict__ C) {
  const int f = f0 + blockIdx.y;
  const uint16_t* src = L + (size_t)f * ch * cw;
  uint16_t* dst = C + (size_t)f * Hc * Wc;
  for (int Y = blockIdx.x * 4 + threadIdx.y; Y < Hc; Y += gridDim.x * 4)
    for (int X = threadIdx.x; X < Wc; X += 64) {
      unsigned s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint16_t* p = src + (size_t)(4 * Y + j) * cw + 4 * X;
        s += (unsigned)p[0] + p[1] + p[2] + p[3];
      }
      dst[(size_t)Y * Wc + X] = (uint16_t)s;
    }
}

// Candidates (dy, -D .. D) of one pair over the rows [D + chunk * rc, + rc) of the interior [D, Hc - D) x [D, Wc - D).  first: the plane slot of pair 0's
// earlier frame.  Every index stays inside the planes: D <= Y < Hc - D and |dy|, |dx| <= D.
__global__ __launch_bounds__(kFsThreads) void fs_sad_coarse_kernel(const uint16_t* __restrict__ C, int Hc, int Wc, int D, int rc, int chunks, int first,
                                                                   unsigned long long* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fs_smem[];
  const int pair = blockIdx.x / chunks, chunk = blockIdx.x - pair * chunks;
  const int r = blockIdx.y, dy = r - D, nc = 2 * D + 1;
  const int Wi = Wc - 2 * D;
  const int ya = D + chunk * rc;
  const int nr = min(rc, Hc - D - ya);
  unsigned* part = reinterpret_cast<unsigned*>(fs_smem);
  uint16_t* tc = reinterpret_cast<uint16_t*>(fs_smem + kFsPartBytes);      // [rc][Wi]   C_t, the interior columns
  uint16_t* tp = tc + (((size_t)rc * Wi + 7) & ~(size_t)7);                // [rc][Wc]   C_{t-1}, dy rows away, every column
  const size_t plane = (size_t)Hc * Wc;
  const uint16_t* prv = C + (size_t)(first + pair) * plane;
  const uint16_t* cur = prv + plane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int y = wave; y < nr; y += 4) {
    for (int c = lane; c < Wi; c += 64) tc[y * Wi + c] = cur[(size_t)(ya + y) * Wc + D + c];
    for (int c = lane; c < Wc; c += 64) tp[y * Wc + c] = prv[(size_t)(ya + y + dy) * Wc + c];
  }
  if (tid < 64) part[tid] = 0;
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    unsigned acc = 0;
    for (int y = wave; y < nr; y += 4)
      for (int col = lane; col < Wi; col += 64) acc += fs_absdiff(tc[y * Wi + col], tp[y * Wc + col + c]);
    acc = fs_wave_sum(acc);
    if (lane == 0) atomicAdd(&part[c], acc);
  }
  __syncthreads();
  if (tid < nc) atomicAdd(&slots[(size_t)pair * nc * nc + r * nc + tid], (unsigned long long)part[tid]);
}

// The 49 fine candidates around the coarse winner and zero displacement, of one pair over the rows [M + chunk * rc, + rc) of the window
// [M, ch - M) x [M, cw - M), M = 4D + 3.  center: the coarse winners, clamped to [-D, D] here so that no index can leave the plane whatever the
// workspace holds: rows M - 4D - 3 = 0 .. ch - 1, columns likewise.
__global__ __launch_bounds__(kFsThreads) void fs_sad_fine_kernel(const uint16_t* __restrict__ L, int ch, int cw, int D, int rc, int chunks, int first,
                                                                 const int32_t* __restrict__ center, unsigned long long* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fs_smem[];
  const int pair = blockIdx.x / chunks, chunk = blockIdx.x - pair * chunks;
  const int M = 4 * D + 3;
  const int cy = min(max(center[2 * pair], -D), D), cx = min(max(center[2 * pair + 1], -D), D);
  const int Wi = cw - 2 * M, Wp = Wi + 6;
  const int ya = M + chunk * rc;
  const int nr = min(rc, ch - M - ya);
  unsigned* part = reinterpret_cast<unsigned*>(fs_smem);
  uint16_t* tp = reinterpret_cast<uint16_t*>(fs_smem + kFsPartBytes);      // [rc + 6][Wp]   L_{t-1} from (ya + 4cy - 3, M + 4cx - 3)
  const size_t plane = (size_t)ch * cw;
  const uint16_t* prv = L + (size_t)(first + pair) * plane;
  const uint16_t* cur = prv + plane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint16_t* corner = prv + (size_t)(ya + 4 * cy - 3) * cw + (M + 4 * cx - 3);
  for (int y = wave; y < nr + 6; y += 4)
    for (int c = lane; c < Wp; c += 64) tp[y * Wp + c] = corner[(size_t)y * cw + c];
  if (tid < 64) part[tid] = 0;
  __syncthreads();
  unsigned acc[kFsFine];
#pragma unroll
  for (int i = 0; i < kFsFine; ++i) acc[i] = 0;
  for (int y = wave; y < nr; y += 4)
    for (int c = lane; c < Wi; c += 64) {
      const size_t at = (size_t)(ya + y) * cw + M + c;
      const unsigned v = cur[at];
      acc[kFsFine - 1] += fs_absdiff(v, prv[at]);
#pragma unroll
      for (int ey = 0; ey < 7; ++ey)
#pragma unroll
        for (int ex = 0; ex < 7; ++ex) acc[ey * 7 + ex] += fs_absdiff(v, tp[(y + ey) * Wp + c + ex]);
    }
#pragma unroll
  for (int i = 0; i < kFsFine; ++i) {
    const unsigned s = fs_wave_sum(acc[i]);
    if (lane == 0) atomicAdd(&part[i], s);
  }
  __syncthreads();
  if (tid < kFsFine) atomicAdd(&slots[(size_t)pair * kFsFine + tid], (unsigned long long)part[tid]);
}

// (S, dy^2 + dx^2, dy, dx), the smaller tuple wins
struct FsBest {
  unsigned long long s;
  int dy, dx;
};
__device__ __forceinline__ bool fs_less(const FsBest& a, const FsBest& b) {
  if (a.s != b.s) return a.s < b.s;
  const int qa = a.dy * a.dy + a.dx * a.dx, qb = b.dy * b.dy + b.dx * b.dx;
  if (qa != qb) return qa < qb;
  if (a.dy != b.dy) return a.dy < b.dy;
  return a.dx < b.dx;
}
// every lane brings its best (s == ~0 for none); returns the wave's in every lane of lane 0's group.  One wave.
__device__ __forceinline__ FsBest fs_wave_best(FsBest b) {
  __shared__ FsBest all[64];
  all[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < 64; ++i)
      if (fs_less(all[i], b)) b = all[i];
  return b;      // valid in thread 0
}

__global__ __launch_bounds__(64) void fs_argmin_coarse_kernel(const unsigned long long* __restrict__ slots, int D, int32_t* __restrict__ center) {
  const int pair = blockIdx.x, nc = 2 * D + 1, n = nc * nc;
  FsBest b{~0ull, 0, 0};
  for (int i = threadIdx.x; i < n; i += 64) {
    const int r = i / nc;
    const FsBest v{slots[(size_t)pair * n + i], r - D, i - r * nc - D};
    if (fs_less(v, b)) b = v;
  }
  b = fs_wave_best(b);
  if (threadIdx.x == 0) {
    center[2 * pair] = b.dy;
    center[2 * pair + 1] = b.dx;
  }
}

// one group per frame t; without `prev` (first == 1) frame 0 has no pair and its rows are zero
__global__ __launch_bounds__(64) void fs_argmin_fine_kernel(const unsigned long long* __restrict__ slots, const int32_t* __restrict__ center, int D, int first,
                                                            int32_t* __restrict__ disp, long long* __restrict__ sad) {
  const int t = blockIdx.x, pair = t - first;
  if (pair < 0) {
    if (threadIdx.x < 2) {
      disp[2 * t + threadIdx.x] = 0;
      sad[2 * t + threadIdx.x] = 0;
    }
    return;
  }
  const int cy = min(max(center[2 * pair], -D), D), cx = min(max(center[2 * pair + 1], -D), D);
  FsBest b{~0ull, 0, 0};
  if (threadIdx.x < kFsFine - 1) {
    const int ey = threadIdx.x / 7, ex = threadIdx.x - ey * 7;
    b = FsBest{slots[(size_t)pair * kFsFine + threadIdx.x], 4 * cy + ey - 3, 4 * cx + ex - 3};
  }
  b = fs_wave_best(b);
  if (threadIdx.x == 0) {
    disp[2 * t] = b.dy;
    disp[2 * t + 1] = b.dx;
    sad[2 * t] = (long long)b.s;
    sad[2 * t + 1] = (long long)slots[(size_t)pair * kFsFine + kFsFine - 1];
  }
}

int fs_rows_per_group(int row_bytes, int extra_rows, int cap) {
  const int fit = kFsTileBytes / row_bytes - extra_rows;
  return fit < 1 ? 1 : (fit > cap ? cap : fit);
}

}  // namespace

size_t frame_shift_slots(int pairs, int D) { return (size_t)pairs * ((size_t)(2 * D + 1) * (2 * D + 1) + kFsFine); }

hipError_t frame_shift(const uint8_t* x, int T, int H, int W, int y0, int x0, int ch, int cw, int D, const uint8_t* prev, uint16_t* L, uint16_t* C,
                       unsigned long long* slots, int32_t* center, int32_t* disp, int64_t* sad, hipStream_t st) {
  if (T < 1 || T > kFrameShiftMaxT || D < 1 || D > kFrameShiftMaxD || H < 1 || W < 1 || H > kFrameShiftMaxSide || W > kFrameShiftMaxSide ||
      (int64_t)H * W * 1020 >= ((int64_t)1 << 32) || y0 < 0 || x0 < 0 || ch < 8 * D + 7 || cw < 8 * D + 7 || y0 > H - ch || x0 > W - cw)
    return hipErrorInvalidValue;
  const int first = prev ? 0 : 1, pairs = T - first;
  long long* sad_ll = reinterpret_cast<long long*>(sad);
  if (pairs > 0) {
    const int Hc = ch / 4, Wc = cw / 4, nc = 2 * D + 1, M = 4 * D + 3;
    const int frames = T + 1 - first;
    const bool wide = W % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 4 == 0 && reinterpret_cast<uintptr_t>(prev) % 4 == 0;
    const dim3 rows_block(64, 4);
    const dim3 lgrid((unsigned)std::min((ch + 3) / 4, 512), (unsigned)frames), cgrid((unsigned)std::min((Hc + 3) / 4, 512), (unsigned)frames);
    if (hipError_t e = hipMemsetAsync(slots, 0, frame_shift_slots(pairs, D) * sizeof(unsigned long long), st); e != hipSuccess) return e;
    if (wide) hipLaunchKernelGGL(fs_luma_kernel<true>, lgrid, rows_block, 0, st, x, prev, H, W, y0, x0, ch, cw, first, L);
    else hipLaunchKernelGGL(fs_luma_kernel<false>, lgrid, rows_block, 0, st, x, prev, H, W, y0, x0, ch, cw, first, L);
    hipLaunchKernelGGL(fs_coarse_kernel, cgrid, rows_block, 0, st, L, ch, cw, Hc, Wc, first, C);
    unsigned long long* fine_slots = slots + (size_t)pairs * nc * nc;
    {
      const int Wi = Wc - 2 * D, rows = Hc - 2 * D;
      const int rc = fs_rows_per_group((Wi + Wc) * 2 + 16, 0, 32);
      const int chunks = (rows + rc - 1) / rc;
      const size_t lds = kFsPartBytes + ((((size_t)rc * Wi + 7) & ~(size_t)7) + (size_t)rc * Wc) * 2;
      hipLaunchKernelGGL(fs_sad_coarse_kernel, dim3((unsigned)(pairs * chunks), (unsigned)nc), dim3(kFsThreads), lds, st, C, Hc, Wc, D, rc, chunks, first, slots);
      hipLaunchKernelGGL(fs_argmin_coarse_kernel, dim3((unsigned)pairs), dim3(64), 0, st, slots, D, center);
    }
    {
      const int Wp = cw - 2 * M + 6, rows = ch - 2 * M;
      const int rc = fs_rows_per_group(Wp * 2, 6, 16);
      const int chunks = (rows + rc - 1) / rc;
      const size_t lds = kFsPartBytes + (size_t)(rc + 6) * Wp * 2;      // at most 256 + 7 * 4096 * 2 bytes: inside the 64 KB a launch may ask for
      hipLaunchKernelGGL(fs_sad_fine_kernel, dim3((unsigned)(pairs * chunks)), dim3(kFsThreads), lds, st, L, ch, cw, D, rc, chunks, first, center, fine_slots);
    }
    hipLaunchKernelGGL(fs_argmin_fine_kernel, dim3((unsigned)T), dim3(64), 0, st, fine_slots, center, D, first, disp, sad_ll);
  } else {
    hipLaunchKernelGGL(fs_argmin_fine_kernel, dim3(1), dim3(64), 0, st, slots, center, D, first, disp, sad_ll);
  }
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_frame_shift(jcm_handle h, const uint8_t* x, int T, int H, int W, int y0, int x0, int ch, int cw, int D, const uint8_t* prev, int32_t* disp,
                    int64_t* sad) {
  const std::string w("frame_shift");
  JCM_TRY(check(h, false));
  if (!x || !disp || !sad) return fail(JCM_ERR_ARG, w + ": null pointer (x, disp and sad are required; prev may be NULL)");
  if (T < 1 || H < 1 || W < 1) return fail(JCM_ERR_ARG, w + ": bad sizes (T, H, W >= 1)");
  if (T > kFrameShiftMaxT) return fail(JCM_ERR_ARG, w + ": T = " + std::to_string(T) + " frames; T <= 65534, split the clip and pass prev");
  if (D < 1 || D > kFrameShiftMaxD) return fail(JCM_ERR_ARG, w + ": D = " + std::to_string(D) + "; 1 <= D <= 16");
  if (H > kFrameShiftMaxSide || W > kFrameShiftMaxSide)
    return fail(JCM_ERR_ARG, w + ": a frame of " + std::to_string(H) + " x " + std::to_string(W) + "; H, W <= 4096 (seven rows of the window are staged in LDS)");
  if ((int64_t)H * W * 1020 >= ((int64_t)1 << 32))
    return fail(JCM_ERR_ARG, w + ": a frame of " + std::to_string(H) + " x " + std::to_string(W) + "; H * W * 1020 < 2^32 (a candidate's sum is held in 32 bits)");
  JCM_TRY(check_rectangle(w, H, W, y0, x0, ch, cw));
  if (ch < 8 * D + 7 || cw < 8 * D + 7)
    return fail(JCM_ERR_ARG, w + ": a rectangle of " + std::to_string(ch) + " x " + std::to_string(cw) + " at D = " + std::to_string(D) + "; ch, cw >= 8 D + 7 = " +
                                 std::to_string(8 * D + 7) + " (the smallest at which both search windows hold a pixel)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const int first = prev ? 0 : 1, pairs = T - first;
  const size_t nL = pairs > 0 ? (size_t)(T + 1) * ch * cw : 0, nC = pairs > 0 ? (size_t)(T + 1) * (ch / 4) * (cw / 4) : 0;
  const size_t ns = frame_shift_slots(pairs > 0 ? pairs : 0, D);
  JCM_TRY(workspace_or_refuse(c, w, (double)(nL + nC) * 2.0 + (double)ns * 8.0 + (double)T * 8.0 + 8192.0, "luma planes", 1, T));
  uint16_t *L = nullptr, *C = nullptr;
  unsigned long long* slots = nullptr;
  int32_t* center = nullptr;
  return arena_launch(c, w, [&] {
    L = arena_alloc<uint16_t>(c, nL);
    C = arena_alloc<uint16_t>(c, nC);
    slots = arena_alloc<unsigned long long>(c, ns + 1);
    center = arena_alloc<int32_t>(c, (size_t)2 * T);
  }, [&] { return frame_shift(x, T, H, W, y0, x0, ch, cw, D, prev, L, C, slots, center, disp, sad, c->stream); });
}

}  // extern "C"
