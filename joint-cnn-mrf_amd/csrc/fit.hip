// Letterbox fit of a ragged batch of byte images (include/jcm.h: jcm_fit_images): image b, [h_b, w_b, C] bytes at any byte offset
// of one buffer, is resampled into the content rectangle of out[b] [OH, OW, C] by a separable triangle filter whose support widens with the
// reduction; everything else of out[b] is the byte `pad`.  The arithmetic is float64 in the order jcm.h states: the row sums first (ascending
// source column), then the column sum (ascending source row).  That order is the order of a streaming kernel:
//   * one work group owns a strip of kFitTW content columns of one image and walks the output rows downward;
//   * the horizontally filtered source rows of the current vertical support live in a ring of doubles in LDS (ring row = source row mod R), so
//     every source row is filtered once per strip and every source byte is loaded about once -- strips overlap by the horizontal support only;
//   * source rows are staged into LDS as aligned dwords (a row starts at any byte: the aligned-down first word and the last word are loaded byte
//     by byte where they leave the buffer), several rows per pass, and read back as bytes by the filter;
//   * the normalised weights t_i / T of the strip's columns are formed once per work group, those of the output rows once per group of rows;
//   * the loops over (row, element) items walk their index pair by addition (FitWalk) and the ring row by wrap-around: no integer division per
//     item -- at 1080 x 1920 -> 405 x 720 the first version of this kernel spent more instructions on index arithmetic than on the filter.
// The images of a launch travel in its kernel arguments (FitBatch, as gather.hip's indices do): nothing is uploaded, nothing for the host to
// wait for.  The grid is the number of strips of the launch's images, not B times the strips of the widest.
//
// Windows (jcm.h: jcm_fit_windows) are the same kernel instantiated on FitWinBatch: the filter runs over the virtual wh x ww image
// -- its rows and columns are the window's -- and only the staging step knows that a staged sample is image[wy0 + row][wx0 + col] where the image
// has one and `pad` elsewhere.  A staged row outside the image is filled with `pad` before any offset is formed from it; the in-image part of a
// staged row is [vb_lo, vb_hi) of its segment bytes and offsets are formed from its first in-image column only.  The strips, the ring and the
// groups of rows are the window's, so the work is the window's whatever the image's size.  The FitBatch instantiation is the code it was.
#include <string>
#include <type_traits>

#include "entry.h"
#include "u8.h"

namespace jcm {

namespace {

constexpr int kFitThreads = 256;
constexpr int kFitStage = 8192;      // bytes of staged source rows per pass; one row of the widest strip is (31 * 32 + 68) * 4 + 6 bytes
constexpr int kFitWyCap = 256;       // vertical weights of one group of output rows (doubles)
constexpr int kFitGMax = 32;         // output rows per group
constexpr int kFitRingCap = 68;      // ring rows at most

// one axis of the filter (jcm.h): output o of m reads source samples [lo, hi) of n around c
struct FitAxis {
  double f, sup;
  int n;
};
__device__ __forceinline__ FitAxis fit_axis(int n, int m) {
  FitAxis a;
  a.f = (double)n / (double)m;
  a.sup = fmax(a.f, 1.0);
  a.n = n;
  return a;
}
__device__ __forceinline__ double fit_centre(const FitAxis& a, int o) { return ((double)o + 0.5) * a.f; }
__device__ __forceinline__ void fit_span(const FitAxis& a, int o, int* lo, int* hi) {
  const double c = fit_centre(a, o);
  *lo = max(0, (int)floor(c - a.sup));
  *hi = min(a.n, (int)ceil(c + a.sup));
}
__device__ __forceinline__ double fit_tap(const FitAxis& a, double c, int i) { return fmax(0.0, 1.0 - fabs((((double)i + 0.5) - c) / a.sup)); }

// raw[x * ld + i] = t_i of `count` outputs starting at o0 (phase 0); w[x * ld + i] = t_i / T, T the ascending sum of the output's raw taps, formed by
// every thread for its own output (phase 1: the same additions in the same order, so the same T).  The caller synchronises between the phases
// and has filled lo[] / cnt[].
__device__ __forceinline__ void fit_weights_raw(const FitAxis& a, int o0, int count, int ld, const int* lo, const int* cnt, double* raw) {
  for (int idx = threadIdx.x; idx < count * ld; idx += kFitThreads) {
    const int x = idx / ld, i = idx - x * ld;
    if (i < cnt[x]) raw[idx] = fit_tap(a, fit_centre(a, o0 + x), lo[x] + i);
  }
}
__device__ __forceinline__ void fit_weights_norm(int count, int ld, const int* cnt, const double* raw, double* w) {
  for (int idx = threadIdx.x; idx < count * ld; idx += kFitThreads) {
    const int x = idx / ld, i = idx - x * ld;
    const int n = cnt[x];
    if (i < n) {
      const double* rx = raw + x * ld;
      double T = 0.0;
      for (int q = 0; q < n; ++q) T = T + rx[q];
      w[idx] = rx[i] / T;
    }
  }
}

template <bool F32>
__device__ __forceinline__ void fit_store(void* out, size_t i, unsigned byte) {
  if constexpr (F32) static_cast<float*>(out)[i] = u8_to_f32(byte);
  else static_cast<uint8_t*>(out)[i] = (uint8_t)byte;
}

// idx = tid, tid + 256, .. split as (row, element) = (idx / per_row, idx % per_row) without a division per item: the step is added to the pair
struct FitWalk {
  int k, e, dk, de, per_row;
  __device__ __forceinline__ FitWalk(int per_row_) : per_row(per_row_) {
    k = (int)threadIdx.x / per_row;
    e = (int)threadIdx.x - k * per_row;
    dk = kFitThreads / per_row;
    de = kFitThreads - dk * per_row;
  }
  __device__ __forceinline__ void next() {
    k += dk;
    e += de;
    if (e >= per_row) {
      e -= per_row;
      ++k;
    }
  }
};

// the size the filter sees: the image's, or the window's
__device__ __forceinline__ int fit_rows(const FitBatch& fb, int i) { return fb.h[i]; }
__device__ __forceinline__ int fit_cols(const FitBatch& fb, int i) { return fb.w[i]; }
__device__ __forceinline__ int fit_rows(const FitWinBatch& fb, int i) { return fb.wh[i]; }
__device__ __forceinline__ int fit_cols(const FitWinBatch& fb, int i) { return fb.ww[i]; }

// R ring rows, TX / TY: leading dimensions of the horizontal / vertical weight tables (>= the taps of any output of the launch's images)
template <bool F32, class Batch>
__global__ __launch_bounds__(kFitThreads) void fit_images_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, Batch fb, int nimg, int b0, int C,
                                                                 int OH, int OW, unsigned pad, int R, int TX, int TY, void* __restrict__ out) {
  extern __shared__ __align__(16) double fit_lds[];
  const int TWC = kFitTW * C;
  double* ring = fit_lds;                          // [R][TWC]
  double* wx = ring + (size_t)R * TWC;             // [kFitTW][TX]
  double* wy = wx + kFitTW * TX;                   // [G][TY], G * TY <= kFitWyCap
  double* raw = wy + kFitWyCap;                    // the taps before they are normalised: max(kFitTW * TX, kFitWyCap)
  uint8_t* stage = reinterpret_cast<uint8_t*>(raw + max(kFitTW * TX, kFitWyCap));      // kFitStage bytes
  int* lox = reinterpret_cast<int*>(stage + kFitStage);             // [kFitTW]
  int* nx = lox + kFitTW;
  int* loy = nx + kFitTW;                          // [kFitGMax]
  int* hiy = loy + kFitGMax;
  int* ny = hiy + kFitGMax;
  int* sloty = ny + kFitGMax;                      // ring row of source row loy
  int* ebyte = sloty + kFitGMax;                   // [kFitTW * 4] element e = x * C + c: byte of its first tap in a staged row, and x
  int* ecol = ebyte + kFitTW * 4;
  const int tid = threadIdx.x;

  int bi = 0;
  while (bi + 1 < nimg && (int)blockIdx.x >= fb.first[bi + 1]) ++bi;
  const int s = blockIdx.x - fb.first[bi], nS = fb.first[bi + 1] - fb.first[bi];
  constexpr bool kWin = std::is_same<Batch, FitWinBatch>::value;
  const int h = fit_rows(fb, bi), w = fit_cols(fb, bi);
  const int64_t off = fb.off[bi];
  const FitGeom g = fit_geometry(h, w, OH, OW);
  const size_t obase = (size_t)(b0 + bi) * OH * OW * C;
  const int rowC = OW * C;

  // the bars: output rows s, s + nS, .. of this image; whole rows outside the content, the two side pieces inside
  for (int r = s; r < OH; r += nS) {
    const size_t ro = obase + (size_t)r * rowC;
    if (r < g.y0 || r >= g.y0 + g.ch) {
      for (int i = tid; i < rowC; i += kFitThreads) fit_store<F32>(out, ro + i, pad);
    } else {
      const int left = g.x0 * C, right = (g.x0 + g.cw) * C;
      for (int i = tid; i < left; i += kFitThreads) fit_store<F32>(out, ro + i, pad);
      for (int i = right + tid; i < rowC; i += kFitThreads) fit_store<F32>(out, ro + i, pad);
    }
  }

  const int xs = s * kFitTW;
  const int tw = min(kFitTW, g.cw - xs), twc = tw * C;
  const FitAxis ax = fit_axis(w, g.cw), ay = fit_axis(h, g.ch);

  // horizontal taps of the strip's columns
  if (tid < tw) {
    int lo, hi;
    fit_span(ax, xs + tid, &lo, &hi);
    lox[tid] = lo;
    nx[tid] = min(hi - lo, TX);
  }
  __syncthreads();
  fit_weights_raw(ax, xs, tw, TX, lox, nx, raw);
  // the source columns the strip reads: [seg_lo, seg_lo + segw); a staged row takes `stride` bytes, the aligned-down head included
  const int seg_lo = lox[0];
  const int segb = (lox[tw - 1] + nx[tw - 1] - seg_lo) * C;
  const int stride = (segb + 6) & ~3, wpr = stride >> 2;
  const int rows_per_pass = max(1, kFitStage / stride);
  if (tid < twc) {
    const int x = tid / C;
    ebyte[tid] = (lox[x] - seg_lo) * C + (tid - x * C);
    ecol[tid] = x;
  }
  __syncthreads();
  fit_weights_norm(tw, TX, nx, raw, wx);
  __syncthreads();

  unsigned* stage32 = reinterpret_cast<unsigned*>(stage);
  // a whole image: every staged sample exists
  const int rowb = w * C;                                                                           // bytes of a source row
  const unsigned base_lo = (unsigned)reinterpret_cast<uintptr_t>(src) + (unsigned)off + (unsigned)seg_lo * C;      // mod 4: the alignment of a segment
  const int64_t seg_off = off + (int64_t)seg_lo * C;                                                // byte offset in src of row 0's segment
  // a window: staged row `row` is image row wy0 + row, staged column 0 image column c0; [vb_lo, vb_hi) of the segment's bytes lie in the image
  int ih = 0, wy0 = 0, vb_lo = 0, vb_hi = 0;
  int64_t irowb = 0, in_off = 0;       // bytes of an image row; byte offset in src of image row 0's first in-image staged sample (segment byte vb_lo)
  unsigned in_lo = 0;                  // mod 4: the alignment of segment byte 0 of image row 0
  if constexpr (kWin) {
    ih = fb.h[bi];
    wy0 = fb.wy0[bi];
    const int iw = fb.w[bi], c0 = fb.wx0[bi] + seg_lo;
    vb_lo = max(0, -c0) * C;
    vb_hi = min(segb / C, iw - c0) * C;
    irowb = (int64_t)iw * C;
    in_off = off + (int64_t)max(c0, 0) * C;
    in_lo = (unsigned)reinterpret_cast<uintptr_t>(src) + (unsigned)in_off - (unsigned)vb_lo;
  }
  // the offset of a staged row's segment in its aligned words
  auto shift_of = [&](int row) -> int {
    if constexpr (kWin) {
      const int ir = wy0 + row;
      if (ir < 0 || ir >= ih || vb_hi <= vb_lo) return 0;      // a row of `pad`: no offset is formed
      return (int)((in_lo + (unsigned)ir * (unsigned)irowb) & 3u);
    } else {
      return (int)((base_lo + (unsigned)row * (unsigned)rowb) & 3u);
    }
  };
  const unsigned pad4 = pad * 0x01010101u;

  int nf = 0;      // source rows below nf have been filtered (or will never be read again)
  for (int o0 = 0; o0 < g.ch;) {
    // the group: as many output rows as the ring and the weight table hold
    if (tid < kFitGMax && o0 + tid < g.ch) fit_span(ay, o0 + tid, &loy[tid], &hiy[tid]);
    __syncthreads();
    const int lo0 = loy[0];
    int G = 1;
    while (G < kFitGMax && o0 + G < g.ch && (G + 1) * TY <= kFitWyCap && hiy[G] - lo0 <= R) ++G;
    const int hiG = hiy[G - 1];
    if (tid < G) {
      ny[tid] = min(min(hiy[tid] - loy[tid], TY), R);
      sloty[tid] = loy[tid] % R;
    }

    // filter the source rows the group needs and the ring does not hold yet
    for (int r = max(nf, lo0); r < hiG;) {
      const int nr = min(hiG - r, rows_per_pass);
      for (FitWalk it(wpr); it.k < nr; it.next()) {
        const int row = r + it.k, wi = it.e;
        const int shift = shift_of(row);
        if constexpr (kWin) {
          const int ir = wy0 + row;
          unsigned v = pad4;
          if (ir >= 0 && ir < ih && vb_lo < vb_hi) {
            const int sb = wi * 4 - shift;                                     // segment byte of the word's first byte
            const int64_t ra = in_off + (int64_t)ir * irowb;                   // offset in src of segment byte vb_lo, a sample of the image
            if (sb >= vb_lo && sb + 4 <= vb_hi) {
              v = *reinterpret_cast<const unsigned*>(src + ra + (sb - vb_lo));    // a 4-byte aligned address, all four bytes in the image
            } else if (sb + 4 > vb_lo && sb < vb_hi) {
              v = 0;
              for (int q = 0; q < 4; ++q) v |= (sb + q >= vb_lo && sb + q < vb_hi ? (unsigned)src[ra + (sb + q - vb_lo)] : pad) << (8 * q);
            }
          }
          stage32[it.k * wpr + wi] = v;
        } else if (wi * 4 < shift + segb) {
          const int64_t wa = seg_off + (int64_t)row * rowb - shift + wi * 4;      // a 4-byte aligned address
          unsigned v;
          if (wa >= 0 && wa + 4 <= src_bytes) {
            v = *reinterpret_cast<const unsigned*>(src + wa);
          } else {
            v = 0;
            for (int q = 0; q < 4; ++q)
              if (wa + q >= 0 && wa + q < src_bytes) v |= (unsigned)src[wa + q] << (8 * q);
          }
          stage32[it.k * wpr + wi] = v;
        }
      }
      __syncthreads();
      const int slot0 = r % R;
      for (FitWalk it(twc); it.k < nr; it.next()) {
        const int row = r + it.k, e = it.e, x = ecol[e];
        const int shift = shift_of(row);
        const uint8_t* p = stage + it.k * stride + shift + ebyte[e];
        const double* wgt = wx + x * TX;
        const int n = nx[x];
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc = acc + wgt[i] * (double)p[i * C];
        int slot = slot0 + it.k;      // it.k < nr <= R
        slot = slot >= R ? slot - R : slot;
        ring[(size_t)slot * TWC + e] = acc;
      }
      __syncthreads();
      r += nr;
    }
    nf = hiG;

    __syncthreads();      // ny / sloty (a group that needed no new row has not synchronised yet)
    fit_weights_raw(ay, o0, G, TY, loy, ny, raw);
    __syncthreads();
    fit_weights_norm(G, TY, ny, raw, wy);
    __syncthreads();

    for (FitWalk it(twc); it.k < G; it.next()) {
      const int gi = it.k, e = it.e;
      const double* wgt = wy + gi * TY;
      const int n = ny[gi];
      int slot = sloty[gi];
      double acc = 0.0;
      for (int j = 0; j < n; ++j) {
        acc = acc + wgt[j] * ring[(size_t)slot * TWC + e];
        slot = slot + 1 == R ? 0 : slot + 1;
      }
      const int v = min(255, max(0, (int)floor(acc + 0.5)));
      fit_store<F32>(out, obase + ((size_t)(g.y0 + o0 + gi) * OW + g.x0 + xs) * C + e, (unsigned)v);
    }
    __syncthreads();      // the next group overwrites ring rows, weights and loy / hiy / ny
    o0 += G;
  }
}

// taps of one output at most: ceil(c + sup) - floor(c - sup) < 2 sup + 2, one more for the roundings of c -+ sup
int fit_taps_bound(int n, int m) {
  const double f = (double)n / (double)m, sup = f > 1.0 ? f : 1.0;
  return (int)std::floor(2.0 * sup) + 3;
}

// the kernel's LDS: ring, horizontal weights, vertical weights, raw taps, staged rows, the small integer tables
int fit_lds_bytes(int R, int C, int TX) {
  const int raw = kFitTW * TX > kFitWyCap ? kFitTW * TX : kFitWyCap;
  return (R * kFitTW * C + kFitTW * TX + kFitWyCap + raw) * (int)sizeof(double) + kFitStage + (2 * kFitTW + 4 * kFitGMax + 8 * kFitTW) * (int)sizeof(int);
}

// one launch per Batch-ful of desc rows: (offset, h, w) of an image, or (offset, h, w, wy0, wx0, wh, ww) of a window.  desc is a HOST array, read
// before the call returns, every entry checked by the entry point: 1 <= C <= 4, sizes, bounds, a reduction of at most 32 per axis (of the window,
// whose image sides are <= 2^24 and which shares a pixel with its image) -> out [B,OH,OW,C] uint8 or (out_f32) float32 = u8_to_f32(byte).
template <class Batch>
hipError_t fit_launch(const uint8_t* src, int64_t src_bytes, const int64_t* desc, int B, int C, int OH, int OW, int pad, bool out_f32, void* out,
                      hipStream_t st) {
  constexpr bool kWin = std::is_same<Batch, FitWinBatch>::value;
  constexpr int kMax = kWin ? kFitWinMax : kFitMax, kDesc = kWin ? 7 : 3;
  static LdsAttr attr_u8, attr_f32;
  const int lds_max = fit_lds_bytes(kFitRingCap, 4, kFitRingCap - 1);
  const void* fn = out_f32 ? reinterpret_cast<const void*>(fit_images_kernel<true, Batch>) : reinterpret_cast<const void*>(fit_images_kernel<false, Batch>);
  if (hipError_t e = (out_f32 ? attr_f32 : attr_u8).ensure(fn, lds_max); e != hipSuccess) return e;
  for (int b0 = 0; b0 < B; b0 += kMax) {
    const int nb = B - b0 < kMax ? B - b0 : kMax;
    Batch fb{};
    int TX = 0, TY = 0, R = 0;
    for (int i = 0; i < nb; ++i) {
      const int64_t* d = desc + (size_t)(b0 + i) * kDesc;
      fb.off[i] = d[0];
      fb.h[i] = (int)d[1];
      fb.w[i] = (int)d[2];
      int fh = fb.h[i], fw = fb.w[i];      // the size the filter sees
      if constexpr (kWin) {
        fb.wy0[i] = (int)d[3];
        fb.wx0[i] = (int)d[4];
        fb.wh[i] = fh = (int)d[5];
        fb.ww[i] = fw = (int)d[6];
      }
      const FitGeom g = fit_geometry(fh, fw, OH, OW);
      fb.first[i + 1] = fb.first[i] + (g.cw + kFitTW - 1) / kFitTW;
      const int tx = fit_taps_bound(fw, g.cw), ty = fit_taps_bound(fh, g.ch);
      TX = tx > TX ? tx : TX;
      TY = ty > TY ? ty : TY;
      // a ring of the vertical support plus about twelve further output rows, so that a group of rows shares one pass over the source
      const int r = ty + (int)std::ceil(12.0 * (double)fh / (double)g.ch);
      R = r > R ? r : R;
    }
    for (int i = nb; i < kMax; ++i) fb.first[i + 1] = fb.first[nb];
    if (TX > kFitRingCap - 1 || TY > kFitRingCap - 1) return hipErrorInvalidValue;      // a reduction above 32: the entry point refuses it
    R = R > kFitRingCap ? kFitRingCap : R;
    const int lds = fit_lds_bytes(R, C, TX);
    if (out_f32)
      hipLaunchKernelGGL((fit_images_kernel<true, Batch>), dim3(fb.first[nb]), dim3(kFitThreads), lds, st, src, src_bytes, fb, nb, b0, C, OH, OW,
                         (unsigned)pad, R, TX, TY, out);
    else
      hipLaunchKernelGGL((fit_images_kernel<false, Batch>), dim3(fb.first[nb]), dim3(kFitThreads), lds, st, src, src_bytes, fb, nb, b0, C, OH, OW,
                         (unsigned)pad, R, TX, TY, out);
  }
  return hipGetLastError();
}

// what jcm_fit_images and jcm_fit_windows check alike (`who` names the entry point in the message): pointers, the frame, the size of out
int fit_check_frame(const std::string& who, const uint8_t* src, int64_t src_bytes, const int64_t* desc, int B, int C, int OH, int OW, int pad,
                    const void* out) {
  if (!src || !desc || !out) return fail(JCM_ERR_ARG, who + ": null pointer (src, desc and out are required, geom may be NULL)");
  if (B < 1 || C < 1 || C > 4 || OH < 1 || OH > 4096 || OW < 1 || OW > 4096 || pad < 0 || pad > 255 || src_bytes < 1)
    return fail(JCM_ERR_ARG, who + ": bad sizes (B >= 1, C in 1..4, OH and OW in 1..4096, pad in 0..255)");
  if ((int64_t)B * OH * OW * C >= ((int64_t)1 << 31)) return fail(JCM_ERR_ARG, who + ": B * OH * OW * C >= 2^31");
  return JCM_OK;
}
// fh x fw, the size the filter sees (an image, or a window), against the size and reduction limits
int fit_check_size(const std::string& who, int64_t fh, int64_t fw, int OH, int OW) {
  if (fh < 1 || fh > 16384 || fw < 1 || fw > 16384)
    return fail(JCM_ERR_ARG, who + " is " + std::to_string(fh) + " x " + std::to_string(fw) + "; both sides lie in 1..16384");
  const FitGeom g = fit_geometry((int)fh, (int)fw, OH, OW);
  if (fh > 32 * (int64_t)g.ch || fw > 32 * (int64_t)g.cw)
    return fail(JCM_ERR_ARG, who + ", " + std::to_string(fh) + " x " + std::to_string(fw) + " into " + std::to_string(g.ch) + " x " + std::to_string(g.cw) +
                                 ": a reduction above 32 (at most 66 taps per axis)");
  return JCM_OK;
}
int fit_check_overlap(const std::string& who, const uint8_t* src, int64_t src_bytes, const void* out, size_t no) {
  if (ranges_overlap(src, (size_t)src_bytes, out, no)) return fail(JCM_ERR_ARG, who + ": out overlaps src");
  return JCM_OK;
}
// geom[i] = the content rectangle of desc row i (`stride` entries a row, the filter's size at entries at, at + 1)
void fit_write_geom(const int64_t* desc, int B, int stride, int at, int OH, int OW, int32_t* geom) {
  for (int b = 0; b < B; ++b) {
    const FitGeom g = fit_geometry((int)desc[b * (int64_t)stride + at], (int)desc[b * (int64_t)stride + at + 1], OH, OW);
    geom[b * (int64_t)4] = g.y0;
    geom[b * (int64_t)4 + 1] = g.x0;
    geom[b * (int64_t)4 + 2] = g.ch;
    geom[b * (int64_t)4 + 3] = g.cw;
  }
}

}  // namespace

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_fit_images(jcm_handle h, const uint8_t* src, int64_t src_bytes, const int64_t* desc, int B, int C, int OH, int OW, int pad, int out_f32,
                   void* out, int32_t* geom) {
  JCM_TRY(check(h, false));
  JCM_TRY(fit_check_frame("fit_images", src, src_bytes, desc, B, C, OH, OW, pad, out));
  for (int b = 0; b < B; ++b) {
    const int64_t off = desc[b * (int64_t)3], hb = desc[b * (int64_t)3 + 1], wb = desc[b * (int64_t)3 + 2];
    const std::string who = "fit_images: image " + std::to_string(b);
    if (hb < 1 || hb > 16384 || wb < 1 || wb > 16384)
      return fail(JCM_ERR_ARG, who + " is " + std::to_string(hb) + " x " + std::to_string(wb) + "; both sides lie in 1..16384");
    if (off < 0 || off > src_bytes || hb * wb * C > src_bytes - off)
      return fail(JCM_ERR_ARG, who + " (" + std::to_string(hb * wb * C) + " bytes at offset " + std::to_string(off) + ") does not lie inside the " +
                                   std::to_string(src_bytes) + " bytes of src");
    JCM_TRY(fit_check_size(who, hb, wb, OH, OW));
  }
  JCM_TRY(fit_check_overlap("fit_images", src, src_bytes, out, (size_t)B * OH * OW * C * (out_f32 ? sizeof(float) : 1)));
  if (geom) fit_write_geom(desc, B, 3, 1, OH, OW, geom);
  DeviceGuard g(h->device);
  CallOrder order(h);
  return timed_launch(h, "fit_images", [&] { return fit_launch<FitBatch>(src, src_bytes, desc, B, C, OH, OW, pad, out_f32 != 0, out, h->stream); });
}

int jcm_fit_windows(jcm_handle h, const uint8_t* src, int64_t src_bytes, const int64_t* desc, int NW, int C, int OH, int OW, int pad, int out_f32,
                    void* out, int32_t* geom) {
  JCM_TRY(check(h, false));
  JCM_TRY(fit_check_frame("fit_windows", src, src_bytes, desc, NW, C, OH, OW, pad, out));
  constexpr int64_t kSide = (int64_t)1 << 24;      // image sides: rows, columns and their sums with a window's stay far inside int
  for (int i = 0; i < NW; ++i) {
    const int64_t* d = desc + i * (int64_t)7;
    const int64_t off = d[0], hb = d[1], wb = d[2], wy0 = d[3], wx0 = d[4], wh = d[5], ww = d[6];
    const std::string who = "fit_windows: window " + std::to_string(i);
    if (hb < 1 || hb > kSide || wb < 1 || wb > kSide)
      return fail(JCM_ERR_ARG, who + ": its image is " + std::to_string(hb) + " x " + std::to_string(wb) + "; both sides lie in 1..2^24");
    if (off < 0 || off > src_bytes || hb * wb * C > src_bytes - off)
      return fail(JCM_ERR_ARG, who + ": its image (" + std::to_string(hb * wb * C) + " bytes at offset " + std::to_string(off) +
                                   ") does not lie inside the " + std::to_string(src_bytes) + " bytes of src");
    JCM_TRY(fit_check_size(who, wh, ww, OH, OW));
    if (wy0 >= hb || wy0 + wh <= 0 || wx0 >= wb || wx0 + ww <= 0)      // wh, ww <= 16384: the sums cannot overflow unless the window is disjoint anyway
      return fail(JCM_ERR_ARG, who + ", rows " + std::to_string(wy0) + ".. and columns " + std::to_string(wx0) + ".., " + std::to_string(wh) + " x " +
                                   std::to_string(ww) + ", shares no pixel with its " + std::to_string(hb) + " x " + std::to_string(wb) + " image");
  }
  JCM_TRY(fit_check_overlap("fit_windows", src, src_bytes, out, (size_t)NW * OH * OW * C * (out_f32 ? sizeof(float) : 1)));
  if (geom) fit_write_geom(desc, NW, 7, 5, OH, OW, geom);
  DeviceGuard g(h->device);
  CallOrder order(h);
  return timed_launch(h, "fit_windows", [&] { return fit_launch<FitWinBatch>(src, src_bytes, desc, NW, C, OH, OW, pad, out_f32 != 0, out, h->stream); });
}

}  // extern "C"
