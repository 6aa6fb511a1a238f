// A 5x5 layer on 2 x 2 tiles of its map, transforms in registers (fft_reg_rows.h): forward rows of the tiles, and the pool hand-over that stitches them.
#include <type_traits>

#include "fft_reg_rows.h"

namespace jcm {
namespace cfft {

// ---- a 5x5 layer on a map of 2 x 2 TILES (conv_fft.hip, ConvArgs::tiles): the Hm x Wm map is cut into tiles of Ht x Wt = Hm / 2 x Wm / 2, and tile
// b' = (b 2 + ty) 2 + tx is a circular NY x NX transform whose zero padding is replaced by the neighbouring pixels (the halo of the 5x5 filter):
// transform row t holds map row ty Ht + t for t < Ht + 2 and ty Ht + t - NY for t >= NY - 2 (the two rows above the tile), zero in between and
// outside the map; the same along x.  A SAME output pixel of the tile reads transform rows y - 2 .. y + 2 mod NY: exactly those.  The filter spectra,
// the GEMM and the inverse column pass are those of an Ht x Wt map of 4 B images; the forward row pass below gathers the tiles from the map, and
// the pool hand-over below stitches the tiles' outputs back together.

// ---- rows, forward, of the tiles of an NHWC fp32 map -> T[kx][c/16][b'][t][16] with NY rows per tile (all of them real: rows Ht .. NY - 1 carry
// the halo).  Two threads per channel pair as in rows_fwd_reg_kernel: thread h loads pixels [h M, h M + M) of the transform row and swaps them with
// the other thread of the pair (v_permlane32_swap); a pixel outside the map or in the unread gap is a buffer load past the descriptor's range: zero.
template <int NX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void rows_fwd_tile_reg_kernel(const float* __restrict__ map, float4* __restrict__ T, int nrows, int NY,
                                                                                                   int Hm, int Wm, int Ht, int Wt, int C, float* __restrict__ tmax) {
  constexpr int M = NX / 2;
  const int CP = C >> 1;
  int h, p;
  size_t by;
  pair_coords<false>(CP, h, p, by);
  if (by >= (size_t)nrows) return;
  const int bt = (int)(by / NY), t = (int)(by % NY);      // (tile, transform row): scalars
  const int tx = bt & 1, ty = (bt >> 1) & 1, b = bt >> 2;
  const int ym = t < Ht + 2 ? ty * Ht + t : (t >= NY - 2 ? ty * Ht + t - NY : -1);
  const bool row_in = ym >= 0 && ym < Hm;
  const auto d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(map) + ((size_t)b * Hm + (row_in ? ym : 0)) * Wm * C, 0, row_in ? Wm * C * 4 : 0, 0x00020000);
  cf raw[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int n = h * M + j;
    const int xm = n < Wt + 2 ? tx * Wt + n : (n >= NX - 2 ? tx * Wt + n - NX : -1);
    const int off = xm >= 0 && xm < Wm ? xm * C * 4 : Wm * C * 4;      // (past the range: the load returns zeros)
    raw[j] = __builtin_bit_cast(cf, __builtin_amdgcn_raw_buffer_load_b64(d, p * 8 + off, 0, 0));
  }
  const bool odd = h != 0;
  cf u[M];
  fwd_rows_in2<NX, 0>(u, raw, odd ? -1.f : 1.f, odd);
  step1<M, -1>(u);
  step2_inplace<M, -1, 0>(u);
  fwd_rows_store_f32<NX>(u, h, T, TRowDst(p, bt, t, nrows / NY, NY, C), tmax, bt);      // + the TILE's word of the spectra's scale: a tile is one row of the channel GEMM
}

// ---- conv2 -> 2x2/2 max pool -> conv3 from the tiles (the contract of rows_inv_pool_fwd_kernel<192, 96>: conv3's T[kx][c/16][b][r][16] of the pooled
// Ht x Wt map and its per-IMAGE word of max |T|).  A wave = 32 channel pairs of ONE pooled row r; two threads per pair, adjacent lanes (the inverse
// layout).  For each of the two x-tiles: the inverse rows of conv2 rows 2 r and 2 r + 1 (in tile ty = 2 r / Ht; Ht is even), each followed by the
// epilogue under the tile's own scale and the horizontal maximum of pixels (2 i, 2 i + 1) -- one from each thread of the pair: a DPP swap --, then the
// vertical maximum of the two rows.  Pooled pixel q = tx Wt / 2 + i; thread h keeps the pooled pixels of parity h, which is what the forward transform's
// exchange (fwd_rows_mid_pair) starts from.  While the second tile runs, the first tile's pooled pixels wait in a per-wave LDS slice (each lane reads back
// what it wrote: no barrier) -- in registers next to the second tile's transform they spilled (640 bytes per lane).
// one output of the inverse row: pixel 2 I + h of the tile, activated, then the horizontal and (second row) vertical maximum into its pooled slot
template <int NX, int TX, int I, int WT, class Act>
__device__ __forceinline__ void pool_tile_px(const cf x, cf (&zp)[NX / 2], bool odd, bool first, Act&& act) {
  const cf v = act(x);
  const cf w = lane_pair_swap(v);
  const cf pm = cf{fmaxf(v.x, w.x), fmaxf(v.y, w.y)};      // max of pixels 2 I, 2 I + 1 (the same in both threads)
  constexpr int q = TX * (WT / 2) + I;                     // pooled pixel: its slot q / 2 in the thread of parity q % 2
  if (((q & 1) != 0) == odd) zp[q >> 1] = first ? pm : cf{fmaxf(zp[q >> 1].x, pm.x), fmaxf(zp[q >> 1].y, pm.y)};
}
template <int NX, int TX, int K1, int K2, int WT, class Act>
__device__ __forceinline__ void pool_tile_outs(const cf (&o)[RPlan<NX / 2>::R2], cf (&zp)[NX / 2], bool odd, bool first, Act&& act) {
  constexpr int I = K1 + RPlan<NX / 2>::R1 * K2 - 1;      // X[2 m + h], m = K1 + R1 K2, is pixel 2 (m - 1) + h of the tile (pad 2)
  if constexpr (I >= 0 && I < WT / 2) pool_tile_px<NX, TX, I, WT>(o[K2], zp, odd, first, act);
  if constexpr (K2 + 1 < RPlan<NX / 2>::R2) pool_tile_outs<NX, TX, K1, K2 + 1, WT>(o, zp, odd, first, act);
}
// step 2 of the inverse row one output row at a time, each consumed at once (as inv_rows_out2: all of them at once spill)
template <int NX, int TX, int K1, int WT, class Act>
__device__ __forceinline__ void pool_tile_row(const cf (&u)[NX / 2], cf (&zp)[NX / 2], bool odd, bool first, Act&& act) {
  constexpr int M = NX / 2;
  cf o[RPlan<M>::R2];
  step2_row<M, 1, K1>(u, o);
  pool_tile_outs<NX, TX, K1, 0, WT>(o, zp, odd, first, act);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (K1 + 1 < RPlan<M>::R1) pool_tile_row<NX, TX, K1 + 1, WT>(u, zp, odd, first, act);
}
template <int NX, int I>
__device__ __forceinline__ void pool_rows_mid(const cf (&zp)[NX / 2], cf (&uu)[NX / 2], bool odd) {
  fwd_rows_mid_pair<NX, I>(zp[I], zp[I + NX / 4], uu, odd);      // pixels 2 I + h and 2 I + h + M
  if constexpr (I + 1 < NX / 4) pool_rows_mid<NX, I + 1>(zp, uu, odd);
}
template <int NX, int WT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void rows_inv_pool_tile_reg_kernel(const float4* __restrict__ T, float4* __restrict__ Tn, const float* __restrict__ bias,
                                                                                                        const float* __restrict__ scale, const float* __restrict__ shift, int relu_bn,
                                                                                                        int nrows, int B, int Ht, int C, float norm0, Fp16Scale sc) {
  constexpr int M = NX / 2;
  static_assert(WT % 2 == 0 && WT + 4 <= NX, "even tile width with its halo inside the transform");
  const int lane = threadIdx.x & 63;
  int h, p;
  size_t by;      // pooled row b Ht + r
  pair_coords<true>(C >> 1, h, p, by);
  if (by >= (size_t)nrows) return;
  const int b = (int)(by / Ht), r = (int)(by % Ht), c = 2 * p;
  constexpr int KS = (WT / 2 - 1) / 2;      // slots 0 .. KS - 1 hold pooled pixels of the first tile only, in both threads of a pair
  __shared__ cf stash[4][KS][64];
  const int ty = (2 * r) / Ht, yt = 2 * r - ty * Ht;      // conv2 rows 2 r, 2 r + 1 = rows yt, yt + 1 of tile row ty
  const bool odd = h != 0;
  Epilogue<> act(bias, scale, shift, relu_bn, c, C, norm0);
  const float tcommon = scale_common(sc);
  cf zp[M];
#pragma unroll
  for (int k = 0; k < M; ++k) zp[k] = cf{0.f, 0.f};      // (pooled pixels Wt .. NX - 1: the next layer's zero padding)
  auto tile = [&](auto txc) __attribute__((always_inline)) {
    constexpr int tx = decltype(txc)::value;
    const int bt = (b * 2 + ty) * 2 + tx;
    act.norm = scale_undo(norm0, sc, bt, tcommon);      // the tile's scale
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      __builtin_amdgcn_sched_barrier(0);      // one row at a time: the next row's loads do not go out over this one's transform
      cf u[M];
      const TInvRow32<NX> load(T, (size_t)bt * Ht + yt + rr, C, p);
      // the row's own copy of the parity: the lane-selected twiddles of the four rows are the same values, and hoisted out of the rows they
      // occupy ~100 registers for the whole kernel (spilled)
      int hr = h;
      asm volatile("" : "+v"(hr));
      const bool odd_r = hr != 0;
      inv_rows_load2<NX, 0>(u, odd_r ? -1.f : 1.f, odd_r, load);
      step1<M, 1>(u);
      pool_tile_row<NX, tx, 0, WT>(u, zp, odd, rr == 0, act);
    }
  };
  cf(*const slice)[64] = stash[threadIdx.x >> 6];
  tile(std::integral_constant<int, 0>{});
#pragma unroll
  for (int k = 0; k < KS; ++k) slice[k][lane] = zp[k];
  tile(std::integral_constant<int, 1>{});
#pragma unroll
  for (int k = 0; k < KS; ++k) zp[k] = slice[k][lane];
  cf uu[M];
  pool_rows_mid<NX, 0>(zp, uu, odd);
  step1<M, -1>(uu);
  step2_inplace<M, -1, 0>(uu);
  fwd_rows_store_f32<NX>(uu, h, Tn, TRowDst(p, b, r, B, Ht, C), sc.tmax_next, b);      // + the next layer's per-IMAGE word
}
// a: the layer on the whole Hm x Wm map (a.B images); NY x NX: the tiles' transform.  Model geometry only: 90-column tiles, 96-point rows.
bool cfft_tiles_supported(int NY, int NX, const FftArgs& a) {
  return NX == 96 && NY == 64 && a.W == 180 && a.H % 4 == 0 && a.H / 2 + 4 <= NY && a.Cin % 64 == 0 && a.Cout % 64 == 0 &&
         (size_t)a.W * a.Cin * 4 < (size_t)1 << 31;
}
bool cfft_rows_fwd_tile_reg(int NY, int NX, const FftArgs& a, cf* T, float* tmax, hipStream_t st) {
  if (!cfft_tiles_supported(NY, NX, a)) return false;
  const int nrows = 4 * a.B * NY;
  const size_t threads = (size_t)nrows * a.Cin;      // two threads per channel pair
  hipLaunchKernelGGL(rows_fwd_tile_reg_kernel<96>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, static_cast<const float*>(a.x), reinterpret_cast<float4*>(T), nrows, NY,
                     a.H, a.W, a.H / 2, a.W / 2, a.Cin, tmax);
  return true;
}
// T: T'[b'][y][kx][c] of the 4 B tiles (Ht valid rows each, the inverse column pass); Tn: the next layer's T of the pooled Ht x Wt map of B images
bool cfft_rows_inv_pool_tile_reg(int NY, int NX, const FftArgs& a, const cf* T, cf* Tn, float norm, const Fp16Scale& sc, hipStream_t st) {
  if (!cfft_tiles_supported(NY, NX, a)) return false;
  const int Ht = a.H / 2, nrows = a.B * Ht;
  const size_t threads = (size_t)nrows * a.Cout;
  hipLaunchKernelGGL((rows_inv_pool_tile_reg_kernel<96, 90>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(T), reinterpret_cast<float4*>(Tn),
                     a.bias, a.scale, a.shift, a.relu_bn, nrows, a.B, Ht, a.Cout, norm, sc);
  return true;
}

}  // namespace cfft
}  // namespace jcm
