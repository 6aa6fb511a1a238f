// The host side of one frequency-domain layer call as a value: FftPlan = the transform sizes, the views of the layer its passes take, the workspace as named
// regions and the twiddle pointers, built ONCE per call (conv_fft_plan / conv_fft_logits_plan, conv_fft.hip) and read by everything that sizes, refuses or runs
// the layer: run_conv_fft (conv_route.hip) builds it, asks the *_refusal functions which variant the call can take, allocates plan.total bytes and hands the plan
// to the runner, which refuses by the same functions.  Host code only: no device header is needed to read it.
#pragma once
#include "kernels.h"

namespace jcm {

typedef float fft_cf __attribute__((ext_vector_type(2)));      // = fftl::cf (fft_lds.h)

struct FftRegion {
  size_t off = 0, bytes = 0;      // off: a multiple of 256; bytes: what the passes use of it
};
struct FftPlan {
  bool ok = false;      // the map has transform lengths (sizes_of); nothing below means anything otherwise
  int ks = 0, np = 0;
  int NY = 0, NX = 0, NXH = 0, F = 0;      // the circular transform, NXH = NX / 2 + 1 columns of its half spectrum, F = NY NXH frequencies
  int NX_next = 0;                         // pool hand-over: row length of the pooled map's transform (0: none asked for, or the pooled map has no size)
  int opad = 0;                            // output row y = row y + opad of the circular convolution (whose size is H + 4 for both kernel sizes; windows: + their halo of 4)
  int MT = 0, ldy = 0, inv_cb = 64;        // the GEMM's M tile, channel stride of the product spectra, channels per work group of the inverse column pass
  float norm = 0.f;                        // 1 / (NY NX)
  // the layer as its passes see it (CoutP = Cout padded to 64 in all three)
  FftArgs map;      // on its map: the row passes' view (tiles: the whole Hm x Wm map)
  FftArgs col;      // forward columns and GEMM: = map; tiles: 4 B images of an NY x NX transform whose NY rows are all real
  FftArgs inv;      // inverse passes: = col; windows: their valid region only; tiles: the Ht valid rows of each tile
  // the workspace: T (the larger of the two row-transformed tensors), the split activation spectra, the product spectra, the tile scale words of a 16-bit T / T'
  // (np = 5, FftScale::t16: one per (image, row, 64 input channels) / (image, kx, inv_cb output channels)).  The logits rows use T alone (S = T'[b][y][kx][64]).
  FftRegion T, Xs, Yf, t16_fwd, t16_inv;
  size_t total = 0;
  // e^{+2 pi i k / n} for NX, NY and NX_next: device pointers, filled by the runners (conv_fft_plan_twiddles) -- sizing runs without a device
  const fft_cf *twx = nullptr, *twy = nullptr, *twx_next = nullptr;

  template <class X> X* at(void* work, const FftRegion& r) const { return reinterpret_cast<X*>(static_cast<char*>(work) + r.off); }
};
// pool_ks_next: kernel size of the layer behind the pool hand-over (FftNext::ks_next), 0 without one
FftPlan conv_fft_plan(const FftArgs& a, int ks, int np, int pool_ks_next = 0);
FftPlan conv_fft_logits_plan(const FftArgs& a);      // the logits layer on the row spectra of its input (9x9, np = 4)
hipError_t conv_fft_plan_twiddles(FftPlan* p);

// A handed-over 16-bit T (bf16 handles, conv4_fullres -> conv5): T[kx][c/16][b][y][16] as complex fp16, then -- at the next multiple of 256 bytes -- one scale
// word per (image, row, 64 channels) tile.  The producing row kernel writes both, the consuming column pass reads both.
struct FftHandover16 {
  size_t words_off = 0, bytes = 0;
  float* words(const void* t) const { return reinterpret_cast<float*>(static_cast<char*>(const_cast<void*>(t)) + words_off); }
};
FftHandover16 conv_fft_handover16(int B, int NXH, int H, int C);

// Can this call run as ... ?  Null, or the first condition it violates.  run_conv_fft picks the variant by them, the runners refuse by them.
const char* conv_fft_refusal(const FftPlan& p, FftLayout in, FftLayout out, const FftLink& link, int t16);      // the five passes on the map / on windows
const char* conv_fft_tiles_refusal(const FftPlan& p, FftLayout in, FftLayout out, const FftLink& link);          // ... on 2 x 2 tiles (p.map.tiles)
const char* conv_fft_logits_refusal(const FftPlan& p, int ks, int np, FftLayout in, FftLayout out, const FftLink& link, int common);      // p = conv_fft_logits_plan

// p.map.wp = the split filter spectra of THIS map size and kernel size; `work` = p.total bytes.  g0 / g1: optional events recorded around the GEMM (the dominant
// kernel of the layer) for the roofline record.  link: what ties the layer to its neighbours.  sc: np >= 4.  A refusal returns hipErrorInvalidValue and its
// reason in *why.  p.map.tiles: rows forward from the map into the 4 B tiles, columns, GEMM and inverse columns of the tiles' transform, then the pool hand-over
// that stitches the tiles back together; sc->tmax: 4 B words (one per tile: the GEMM row), sc->tmax_next: B words (one per image).
hipError_t conv_fft_f32(FftPlan p, FftLayout in, FftLayout out, void* work, const FftLink& link, hipEvent_t g0, hipEvent_t g1, hipStream_t st, const FftScale* sc,
                        const char** why);
// The logits layer contracted on the row spectra of its input (conv_fft_logits.hip; fp32 handles): a 9x9 layer with Cout <= 16 whose row-transformed input arrives
// through link.t_in at a 96-point row length, H <= 64.  p.map.wp = the operand packed by conv_fft_logits_pack (conv_fft_logits_weight_bytes; wscale as above);
// out fp32 NHWC, bias epilogue.
hipError_t conv_fft_logits_f32(FftPlan p, int ks, int np, FftLayout in, FftLayout out, void* work, const FftLink& link, hipEvent_t g0, hipEvent_t g1, hipStream_t st,
                               const FftScale* sc, const char** why);

}  // namespace jcm
