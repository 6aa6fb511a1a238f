// Local motion: one whole-pixel displacement per heat-map cell between a frame and each of its R reference frames, by exhaustive
// block matching on the integer luma of 4.26, and the pooling of the neighbours' heat maps warped by it.  include/jcm.h (jcm_frame_flow,
// jcm_hm_flow_pool) is the definition, tests/frame_flow_ref.py its restatement.  The matching is integer arithmetic with order-free sums, the pooling
// float64 in one fixed order: both are bit-equal to the restatement however the work is cut.
// Three kinds of launch on the handle's stream, nothing read back in between:
//   ff_luma_kernel   L = R + 2G + B of the content rectangle of every frame, uint16 [T][ch][cw] in the workspace; one thread per pixel, byte loads
//                    (no load width, so no alignment case).  Nothing outside the rectangle is read.
//   ff_match_kernel  a work group of four waves per (slot (t, r), row of cells, strip of kFfStrip cells), taken from a 1-D grid by a strided loop.  The
//                    strip's rows of L_t and the rows and columns D further of L_s are staged into LDS once as uint16; then one wave per cell,
//                    the lanes spread over the (2D+1)^2 candidates: every lane sums its candidates' absolute differences over the cell's block
//                    and keeps the smallest packed tuple (S, dy^2 + dx^2, dy, dx); a wave reduction picks the winner.
//   ff_pool_kernel   one thread per output value (t, y, x, k).
#include <cmath>
#include <string>

#include "entry.h"

namespace jcm {

namespace {

constexpr int kFfThreads = 256;          // 4 waves
constexpr int kFfStrip = 16;             // cells per work group: 4 per wave
constexpr int kFfBlock = 16;             // the block of a cell: 16 x 16 pixels from 4 before the cell's corner
constexpr int kFfCell = 8;               // fitted-frame pixels per heat-map cell
constexpr int kFfLtStride = kFfCell * kFfStrip + 8;      // 136 uint16: the columns of L_t a strip's blocks cover
constexpr int kFfMaxGroups = 65536;      // the grid's cap; the work items beyond it are reached by the strided loop

// Row stride of the L_s tile in dwords.  Lane l of a wave reads candidate (l / nc, l % nc), nc = 2D + 1: a half wave covers 32 / nc rows (and one more)
// of nc consecutive uint16 = at most D + 1 dwords each.  With the stride congruent to D + 2 (or to its negative) modulo the 32 banks, consecutive rows
// start D + 2 banks apart and do not share a bank.  Computed from the bank rule for a half wave, not measured: the reads are single uint16s, a whole
// wave spans twice the rows, and no conflict counter has been read.
int ff_ls_stride_dwords(int width_u16, int D) {
  int s = (width_u16 + 1) / 2;
  while (s % 32 != (D + 2) % 32 && s % 32 != (32 - (D + 2) % 32) % 32) ++s;
  return s;
}

__device__ __forceinline__ unsigned ff_absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

__global__ __launch_bounds__(kFfThreads) void ff_luma_kernel(const uint8_t* __restrict__ x, int T, int H, int W, int y0, int x0, int ch, int cw,
                                                             uint16_t* __restrict__ L) {
  const size_t plane = (size_t)ch * cw, n = plane * T;
  for (size_t i = (size_t)blockIdx.x * kFfThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kFfThreads) {
    const size_t t = i / plane, r = i - t * plane;
    const int y = (int)(r / cw), q = (int)(r - (size_t)y * cw);
    const uint8_t* p = x + (((size_t)t * H + (y0 + y)) * W + (x0 + q)) * 3;
    L[i] = (uint16_t)((unsigned)p[0] + 2u * p[1] + p[2]);
  }
}

// (S, dy^2 + dx^2, dy + D, dx + D) in 18 + 10 + 6 + 6 bits: S <= 256 * 1020 < 2^18, dy^2 + dx^2 <= 512, dy + D <= 32.  The smaller key is the smaller tuple.
__device__ __forceinline__ unsigned long long ff_key(unsigned s, int dy, int dx, int D) {
  return ((unsigned long long)s << 22) | ((unsigned long long)(dy * dy + dx * dx) << 12) | ((unsigned long long)(dy + D) << 6) | (unsigned long long)(dx + D);
}

// total = T * R * HH * strips work items; item = ((slot * HH) + Y) * strips + strip.  ls_stride in uint16 (even).
// Every global index is inside its plane: rows and columns are clipped to the content rectangle before they are read, and a reference frame outside
// [0, T) is "no such frame".  Every LDS index is inside its tile: a valid candidate's block lies in the content rectangle and within D of the
// strip's rows and columns, which is what is staged.
__global__ __launch_bounds__(kFfThreads) void ff_match_kernel(const uint16_t* __restrict__ L, const int32_t* __restrict__ ref, int T, int R, int HH, int WW, int y0,
                                                              int x0, int ch, int cw, int D, int strips, int ls_stride, long long total,
                                                              int32_t* __restrict__ flow, int32_t* __restrict__ sad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ff_smem[];
  uint16_t* lt = reinterpret_cast<uint16_t*>(ff_smem);                          // [16][kFfLtStride]
  uint16_t* ls = lt + kFfBlock * kFfLtStride;                                     // [16 + 2D][ls_stride]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nc = 2 * D + 1, ncand = nc * nc;
  const size_t plane = (size_t)ch * cw;
  for (long long item = blockIdx.x; item < total; item += gridDim.x) {
    const long long slot = item / ((long long)HH * strips);
    const int rem = (int)(item - slot * HH * strips);
    const int Y = rem / strips, X0 = (rem - Y * strips) * kFfStrip, nX = min(kFfStrip, WW - X0);
    const int t = (int)(slot / R);
    const int s = ref[slot];
    const size_t out0 = (((size_t)slot * HH + Y) * WW + X0) * 2;
    // the rows of this row of cells and the columns of this strip inside the content rectangle, in its own coordinates
    const int ry0 = max(kFfCell * Y - 4 - y0, 0), ry1 = min(kFfCell * Y + 12 - y0, ch);
    const int cx0 = max(kFfCell * X0 - 4 - x0, 0), cx1 = min(kFfCell * (X0 + nX - 1) + 12 - x0, cw);
    if (s < 0 || s >= T || ry0 >= ry1 || cx0 >= cx1) {      // no such frame, or no cell of the strip has a pixel: uniform over the group
      if (tid < 2 * nX) {
        flow[out0 + tid] = 0;
        sad[out0 + tid] = 0;
      }
      continue;
    }
    const int sy0 = max(ry0 - D, 0), sy1 = min(ry1 + D, ch), sx0 = max(cx0 - D, 0), sx1 = min(cx1 + D, cw);
    const uint16_t* Lt = L + (size_t)t * plane;
    const uint16_t* Ls = L + (size_t)s * plane;
    __syncthreads();      // the tiles of the item before are done with
    {
      const int w = cx1 - cx0, n = (ry1 - ry0) * w;
      for (int i = tid; i < n; i += kFfThreads) {
        const int y = i / w, q = i - y * w;
        lt[y * kFfLtStride + q] = Lt[(size_t)(ry0 + y) * cw + cx0 + q];
      }
    }
    {
      const int w = sx1 - sx0, n = (sy1 - sy0) * w;
      for (int i = tid; i < n; i += kFfThreads) {
        const int y = i / w, q = i - y * w;
        ls[y * ls_stride + q] = Ls[(size_t)(sy0 + y) * cw + sx0 + q];
      }
    }
    __syncthreads();
    const int h = ry1 - ry0;
    for (int j = wave; j < nX; j += 4) {
      const int X = X0 + j;
      const int px0 = max(kFfCell * X - 4 - x0, 0), px1 = min(kFfCell * X + 12 - x0, cw);
      unsigned long long best = ~0ull;
      unsigned zero = 0;
      if (px0 < px1) {
        const int w = px1 - px0;
        const uint16_t* a0 = lt + (px0 - cx0);
        const bool whole = h == kFfBlock && w == kFfBlock && ((px0 - cx0) & 1) == 0;      // the interior: a fixed trip count and dword reads of L_t
        for (int c = lane; c < ncand; c += 64) {
          const int cy = c / nc, dy = cy - D, dx = c - cy * nc - D;
          if (ry0 + dy < 0 || ry1 + dy > ch || px0 + dx < 0 || px1 + dx > cw) continue;
          const uint16_t* b0 = ls + (ry0 + dy - sy0) * ls_stride + (px0 + dx - sx0);
          unsigned acc = 0;
          if (whole) {
#pragma unroll 2
            for (int y = 0; y < kFfBlock; ++y) {
              const unsigned* a = reinterpret_cast<const unsigned*>(a0 + y * kFfLtStride);
              const uint16_t* b = b0 + y * ls_stride;
#pragma unroll
              for (int q = 0; q < kFfBlock / 2; ++q) {
                const unsigned v = a[q];
                acc += ff_absdiff(v & 0xffffu, b[2 * q]) + ff_absdiff(v >> 16, b[2 * q + 1]);
              }
            }
          } else {
            for (int y = 0; y < h; ++y)
              for (int q = 0; q < w; ++q) acc += ff_absdiff(a0[y * kFfLtStride + q], b0[y * ls_stride + q]);
          }
          const unsigned long long key = ff_key(acc, dy, dx, D);
          if (key < best) best = key;
          if (dy == 0 && dx == 0) zero = acc;
        }
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long other = __shfl_xor(best, o);
          if (other < best) best = other;
          zero += __shfl_xor(zero, o);      // one lane holds it, the others 0
        }
      }
      if (lane == 0) {
        const size_t o = out0 + 2 * (size_t)j;
        if (px0 < px1) {      // (0,0) is always valid, so there is a winner
          flow[o] = (int)((best >> 6) & 63u) - D;
          flow[o + 1] = (int)(best & 63u) - D;
          sad[o] = (int32_t)(best >> 22);
          sad[o + 1] = (int32_t)zero;
        } else {
          flow[o] = flow[o + 1] = 0;
          sad[o] = sad[o + 1] = 0;
        }
      }
    }
  }
}

struct FfWeights {
  double w[5];
};

// the bilinear sample of plane[.., k] at (py, px), both already clamped to the map; the upper neighbour index is clamped too
__device__ __forceinline__ double ff_sample(const float* __restrict__ plane, int HH, int WW, int K, int k, double py, double px) {
  const double fy0 = floor(py), fx0 = floor(px);
  const int ya = (int)fy0, xa = (int)fx0, yb = min(ya + 1, HH - 1), xb = min(xa + 1, WW - 1);
  const double fy = py - fy0, fx = px - fx0;
  const double v00 = plane[((size_t)ya * WW + xa) * K + k], v01 = plane[((size_t)ya * WW + xb) * K + k];
  const double v10 = plane[((size_t)yb * WW + xa) * K + k], v11 = plane[((size_t)yb * WW + xb) * K + k];
  const double top = (1.0 - fx) * v00 + fx * v01, bot = (1.0 - fx) * v10 + fx * v11;
  return (1.0 - fy) * top + fy * bot;
}

__global__ __launch_bounds__(kFfThreads) void ff_pool_kernel(const float* __restrict__ hm, int T, int HH, int WW, int K, const int32_t* __restrict__ flow, int N,
                                                             FfWeights wt, float* __restrict__ out) {
  const size_t cells = (size_t)HH * WW, per = cells * K, n = per * T;
  for (size_t i = (size_t)blockIdx.x * kFfThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kFfThreads) {
    const int t = (int)(i / per);
    const size_t r = i - (size_t)t * per;
    const size_t cell = r / K;
    const int k = (int)(r - cell * K), y = (int)(cell / WW), x = (int)(cell - (size_t)y * WW);
    double acc = wt.w[0] * (double)hm[i], ws = wt.w[0];
    for (int m = 1; m <= N; ++m)
      for (int side = 0; side < 2; ++side) {
        const int s = side ? t + m : t - m;
        if (s < 0 || s >= T) continue;
        const int32_t* f = flow + ((((size_t)t * 2 * N + 2 * (m - 1) + side) * cells) + cell) * 2;
        double py = (double)y + (double)f[0] / 8.0, px = (double)x + (double)f[1] / 8.0;
        py = fmin(fmax(py, 0.0), (double)(HH - 1));
        px = fmin(fmax(px, 0.0), (double)(WW - 1));
        acc += wt.w[m] * ff_sample(hm + (size_t)s * per, HH, WW, K, k, py, px);
        ws += wt.w[m];
      }
    out[i] = (float)(acc / ws);
  }
}

}  // namespace

hipError_t frame_flow(const uint8_t* x, int T, int H, int W, int y0, int x0, int ch, int cw, int D, const int32_t* ref, int R, uint16_t* L, int32_t* flow,
                      int32_t* sad, hipStream_t st) {
  if (T < 1 || T > kFrameFlowMaxT || D < 1 || D > kFrameFlowMaxD || R < 1 || R > kFrameFlowMaxR || H < 8 || W < 8 || H % 8 || W % 8 || H > kFrameFlowMaxSide ||
      W > kFrameFlowMaxSide || y0 < 0 || x0 < 0 || ch < 1 || cw < 1 || y0 > H - ch || x0 > W - cw)
    return hipErrorInvalidValue;
  const int HH = H / kFfCell, WW = W / kFfCell, strips = (WW + kFfStrip - 1) / kFfStrip;
  const size_t pixels = (size_t)T * ch * cw;
  hipLaunchKernelGGL(ff_luma_kernel, dim3((unsigned)std::min<size_t>((pixels + kFfThreads - 1) / kFfThreads, 65536)), dim3(kFfThreads), 0, st, x, T, H, W, y0, x0, ch,
                     cw, L);
  const int ls_stride = 2 * ff_ls_stride_dwords(kFfLtStride + 2 * D, D);
  const size_t lds = ((size_t)kFfBlock * kFfLtStride + (size_t)(kFfBlock + 2 * D) * ls_stride) * 2;      // at most 4352 + 48 * 220 * 2 = 25472 bytes (D = 16)
  const long long total = (long long)T * R * HH * strips;
  hipLaunchKernelGGL(ff_match_kernel, dim3((unsigned)std::min<long long>(total, kFfMaxGroups)), dim3(kFfThreads), lds, st, L, ref, T, R, HH, WW, y0, x0, ch, cw, D,
                     strips, ls_stride, total, flow, sad);
  return hipGetLastError();
}

hipError_t hm_flow_pool(const float* hm, int T, int HH, int WW, int K, const int32_t* flow, int N, const double* w, float* out, hipStream_t st) {
  if (T < 1 || HH < 1 || WW < 1 || K < 1 || N < 1 || N > kFlowPoolMaxN) return hipErrorInvalidValue;
  FfWeights wt{};
  for (int i = 0; i <= N; ++i) wt.w[i] = w[i];
  const size_t n = (size_t)T * HH * WW * K;
  hipLaunchKernelGGL(ff_pool_kernel, dim3((unsigned)std::min<size_t>((n + kFfThreads - 1) / kFfThreads, 65536)), dim3(kFfThreads), 0, st, hm, T, HH, WW, K, flow, N, wt,
                     out);
  return hipGetLastError();
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_frame_flow(jcm_handle h, const uint8_t* x, int T, int H, int W, int y0, int x0, int ch, int cw, int D, const int32_t* ref, int R, int32_t* flow,
                   int32_t* sad) {
  const std::string w("frame_flow");
  JCM_TRY(check(h, false));
  if (!x || !ref || !flow || !sad) return fail(JCM_ERR_ARG, w + ": null pointer (x, ref, flow and sad are required)");
  if (T < 1 || H < 1 || W < 1) return fail(JCM_ERR_ARG, w + ": bad sizes (T, H, W >= 1)");
  if (T > kFrameFlowMaxT) return fail(JCM_ERR_ARG, w + ": T = " + std::to_string(T) + " frames; T <= 65534, split the clip");
  if (D < 1 || D > kFrameFlowMaxD) return fail(JCM_ERR_ARG, w + ": D = " + std::to_string(D) + "; 1 <= D <= 16");
  if (R < 1 || R > kFrameFlowMaxR) return fail(JCM_ERR_ARG, w + ": R = " + std::to_string(R) + " reference frames per frame; 1 <= R <= 8");
  if (H % 8 || W % 8 || H > kFrameFlowMaxSide || W > kFrameFlowMaxSide)
    return fail(JCM_ERR_ARG, w + ": a frame of " + std::to_string(H) + " x " + std::to_string(W) + "; H and W are multiples of 8 (whole heat-map cells) and <= 4096");
  JCM_TRY(check_rectangle(w, H, W, y0, x0, ch, cw));
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const size_t nL = (size_t)T * ch * cw;
  JCM_TRY(workspace_or_refuse(c, w, (double)nL * 2.0 + 8192.0, "luma planes", 1, T));
  uint16_t* L = nullptr;
  return arena_launch(c, w, [&] { L = arena_alloc<uint16_t>(c, nL); }, [&] { return frame_flow(x, T, H, W, y0, x0, ch, cw, D, ref, R, L, flow, sad, c->stream); });
}

int jcm_hm_flow_pool(jcm_handle h, const float* hm, int T, int HH, int WW, int K, const int32_t* flow, int N, const double* wts, float* out) {
  const std::string w("hm_flow_pool");
  JCM_TRY(check(h, false));
  if (T < 1 || HH < 1 || WW < 1 || K < 1) return fail(JCM_ERR_ARG, w + ": bad sizes (T, HH, WW, K >= 1)");
  if (K > kSeqMaxK) return fail(JCM_ERR_ARG, w + ": K = " + std::to_string(K) + " joints; K <= 16");
  if ((int64_t)HH * WW > kSeqMaxHW)
    return fail(JCM_ERR_ARG, w + ": a map of " + std::to_string(HH) + " x " + std::to_string(WW) + " cells; HH * WW <= 8192 (what the scans take), a larger map is not truncated");
  if (N < 1 || N > kFlowPoolMaxN) return fail(JCM_ERR_ARG, w + ": N = " + std::to_string(N) + " neighbours on either side; 1 <= N <= 4");
  if ((int64_t)T * 2 * N * HH * WW * 2 >= ((int64_t)1 << 40)) return fail(JCM_ERR_ARG, w + ": bad sizes (T * 2N * HH * WW * 2 < 2^40)");
  if (!hm || !flow || !wts || !out) return fail(JCM_ERR_ARG, w + ": null pointer (hm, flow, w and out are required)");
  for (int i = 0; i <= N; ++i)
    if (!std::isfinite(wts[i]) || wts[i] < 0.0 || (i == 0 && !(wts[0] > 0.0)))
      return fail(JCM_ERR_ARG, w + ": w[" + std::to_string(i) + "] = " + std::to_string(wts[i]) + "; w[0] > 0, the others >= 0, all finite");
  const size_t n = (size_t)T * HH * WW * K;
  if (ranges_overlap(hm, n * sizeof(float), out, n * sizeof(float))) return fail(JCM_ERR_ARG, w + ": out overlaps hm (a frame's value reads its neighbours' maps)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  return timed_launch(h, w, [&] { return hm_flow_pool(hm, T, HH, WW, K, flow, N, wts, out, h->stream); });
}

}  // extern "C"
