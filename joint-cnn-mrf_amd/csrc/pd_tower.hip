// The part-detector tower (main.py:29-74) and the spatial model (main.py:94-125) as sequences of launches on the handle's stream, and the
// front-end stages the tower shares with jcm_conv1_pool / jcm_conv2_pool.  Host code only.
#include <string>
#include <utility>

#include "ctx.h"

namespace jcm {

// does the stride-2 first layer L1 run fused with its pool (conv1_mfma.hip) on an image whose sub-sampled extents are H x W?  The fused kernels pool whole
// 2x2 windows of whole conv-output pairs: both extents multiples of 4, and the packed 64-filter image of this handle's precision.
bool conv1_pool_fused(const jcm_ctx* c, const ConvLayer* L1, int H, int W) {
  return (c->precision == JCM_PRECISION_BF16 ? L1->wq1_bf16 != nullptr : L1->wq1_f32 != nullptr) && H % 4 == 0 && W % 4 == 0;
}
// ... fp32 handles: on split operands (conv1_mfma_pool_split_kernel) rather than the exact fp32 chain (conv1_mfma_pool_f32_kernel)?
bool conv1_split_route(const jcm_ctx* c, const ConvLayer* L1) { return c->conv9_fft && c->f32_conv == 0 && L1->wq1_split; }

// conv1_<res> + pool1 (main.py:44-45, 52-53, 61-62) of a [B,xh,xw,3] image read at every xsub-th pixel of every xsub-th row (float, or bytes: x_u8), as
// the tower runs them -- and as jcm_conv1_pool does, which calls this too.  Sub-sampled extents that are multiples of 4 with a 64-filter BatchNorm layer:
// ONE MFMA kernel, only the pooled map reaches memory.  fp32 handles take it on split operands on the default route (the stride-1 layers run on split
// operands there anyway), on the exact fp32 MFMA chain otherwise; bf16 handles on bf16 operands.  Every other geometry: the generic stride-2 kernel, then
// the pool.  The pooled map [B, ceil(ceil(xh/xsub/2)/2), ceil(ceil(xw/xsub/2)/2), Cout] (fp32, bf16 on a bf16 handle) goes to `dst`, or to the arena when
// dst is null; *p1 is where it is.
int conv1_pool_stage(jcm_ctx* c, const std::string& scope, const ConvLayer* L1, const void* xin, bool xin_u8, int B, int xh, int xw, int xsub, void* dst, void** p1) {
  const bool bf = c->precision == JCM_PRECISION_BF16;
  const size_t es = bf ? 2 : 4;
  auto act = [&](size_t elems) { return static_cast<void*>(arena_alloc<char>(c, elems * es)); };
  const int h1 = cdiv2(xh / xsub), w1 = cdiv2(xw / xsub);
  const int h2 = cdiv2(h1), w2 = cdiv2(w1);
  if (conv1_pool_fused(c, L1, xh / xsub, xw / xsub)) {      // (xh, xw are multiples of xsub: the tower resizes otherwise, the entry refuses)
    *p1 = dst ? dst : act((size_t)B * h2 * w2 * L1->cout);
    if (c->dry) return JCM_OK;
    if (bf) {
      // bf16 path: conv1 + ReLU/BN + pool1 in one MFMA kernel; only the pooled map touches HBM
      HIP_TRY(conv1_mfma_pool(xin, L1->wq1_bf16, L1->bias, L1->scale, L1->shift, *p1, B, xh, xw, xsub, c->stream, xin_u8));
    } else {
      // fp32 path: conv1 + ReLU/BN + pool1 in one fp32-MFMA kernel (the unpooled 240x360x64 map never reaches HBM)
      // default route (the stride-1 layers run on split operands on the bf16 matrix cores): conv1 too; the exact fp32 MFMA chain otherwise
      HIP_TRY(conv1_split_route(c, L1) ? conv1_mfma_pool_split(xin, L1->wq1_split, L1->bias, L1->scale, L1->shift, static_cast<float*>(*p1), B, xh, xw, xsub, c->stream, xin_u8)
                                       : conv1_mfma_pool_f32(xin, L1->wq1_f32, L1->bias, L1->scale, L1->shift, static_cast<float*>(*p1), B, xh, xw, xsub, c->stream, xin_u8));
    }
    return JCM_OK;
  }
  void* c1 = act((size_t)B * h1 * w1 * L1->cout);
  ConvCall q1 = conv_call(xin, c1, B, xh, xw);
  q1.stride = 2; q1.sub = xsub; q1.act_bf16 = bf; q1.x_u8 = xin_u8;
  JCM_TRY(run_conv(c, scope, q1));
  *p1 = dst ? dst : act((size_t)B * h2 * w2 * L1->cout);
  if (!c->dry) HIP_TRY(max_pool_2x2(c1, *p1, bf, B, h1, w1, L1->cout, c->stream));
  return JCM_OK;
}

// the layout of conv2_<res> -> pool2 on a bf16 handle (Pool2Layout, ctx.h)
Pool2Layout pool2_layout(jcm_ctx* c, const ConvLayer* L2, const ConvLayer* L3, int B, int h2, int w2) {
  const bool bf = c->precision == JCM_PRECISION_BF16;
  const int sk = c->debug_skip;
  Pool2Layout l;
  l.pl23 = bf && takes_c5strip(L2, B, h2, w2) && takes_c5strip(L3, B, cdiv2(h2), cdiv2(w2)) ? 1 : 0;
  l.hp = l.pl23 && c->bf16_hpool && w2 % 2 == 0 && !(sk & 6) ? 1 : 0;
  return l;
}
// the pool behind conv2: c2 as conv2 wrote it under `l` -> p2 [B,ceil(h2/2),ceil(w2/2),C] in the same layout
hipError_t pool2_launch(jcm_ctx* c, const Pool2Layout& l, const void* c2, void* p2, int B, int h2, int w2, int C) {
  const bool bf = c->precision == JCM_PRECISION_BF16;
  if (l.hp) return vpool_2x1_bf16(c2, p2, B * (C / 8), h2, w2 / 2, 8, c->stream);
  if (l.pl23) return max_pool_2x2(c2, p2, bf, B * (C / 8), h2, w2, 8, c->stream);
  return max_pool_2x2(c2, p2, bf, B, h2, w2, C, c->stream);
}

// fp32 handles: two consecutive frequency-domain layers on the same map -- the first one's fused inverse/forward row kernel writes the
// second one's row-transformed input (from the arena) and the activation between them never reaches HBM.  Call right before
// run_conv(first): fills the output side of its link and returns the buffer, or null; hand_over() then gives it to the second layer's link.
static void* offer_handover(jcm_ctx* c, const ConvLayer* La, const ConvLayer* Lb, int B, int H, int W, FftLink& la) {
  if (c->precision != JCM_PRECISION_F32 || !takes_fft(c, La, B, H, W) || !takes_fft(c, Lb, B, H, W)) return nullptr;
  const ConvArgs a = conv_args(La, B, H, W);
  if (La->cout != Lb->cin || !conv_fft_fusable(a, La->ks, Lb->ks)) return nullptr;
  return la.t_next = arena_alloc<char>(c, conv_fft_handover_bytes(a, La->ks));
}
// ... with the 2x2 max pool of main.py:47,55,64 between them: La runs on H x W, Lb on the pooled map; the fused kernel (conv_fft_rows_fused.hip) pools
// a row pair in LDS and writes Lb's row-transformed input -- neither La's output nor the pooled map reaches HBM.
static void* offer_pool_handover(jcm_ctx* c, const ConvLayer* La, const ConvLayer* Lb, int B, int H, int W, FftLink& la) {
  if (!(c->fft_fuse & 1) || c->precision != JCM_PRECISION_F32 || !takes_fft(c, La, B, H, W) || !takes_fft(c, Lb, B, (H + 1) / 2, (W + 1) / 2)) return nullptr;
  const ConvArgs a = conv_args(La, B, H, W);
  if (La->cout != Lb->cin || !conv_fft_pool_fusable(a, La->ks, Lb->ks)) return nullptr;
  la.next.pool = 1;
  la.next.ks_next = Lb->ks;
  return la.t_next = arena_alloc<char>(c, conv_fft_pool_handover_bytes(a, Lb->ks));
}
// the producer has run: its t_next and the words run_conv_fft gave it are the consumer's input
static void hand_over(const FftLink& from, FftLink& to) { to.t_in = from.t_next; to.tmax_in = from.tmax_next; }
// The half- and quarter-resolution branches on the handle's side stream ("fft_fuse" bit 2; jcm_ctx::Side says why everything they write has allocations of its
// own).  fork(): the side stream waits for what the main stream holds so far.  enter() .. leave(): the handle's current stream, arena, scale words and input-scale
// buffer ARE the side ones, so run_conv, conv1_pool_stage, the pool launches, the profiling events, fft_new_words and first-use filter-spectra packing go there
// without knowing; leave() records the join event.  join(): the main stream waits for it -- in front of the first launch that reads x2 / x3.  The destructor
// leaves and joins on every path out, error returns included: no caller buffer, arena region or CallOrder chain event is released while side work is in flight.
// Off (bit 2 clear) or in a dry pass nothing is recorded; a dry pass still swaps, so that the side arena gets its own peak.
struct SideBranches {
  jcm_ctx* c;
  bool on, inside = false, forked = false, fresh = true;
  SideBranches(jcm_ctx* ctx, bool use) : c(ctx), on(use) {}
  SideBranches(const SideBranches&) = delete;
  SideBranches& operator=(const SideBranches&) = delete;
  void swap() {
    jcm_ctx::Side& s = c->side;
    std::swap(c->stream, s.stream);
    std::swap(c->arena, s.arena);
    std::swap(c->arena_cap, s.arena_cap);
    std::swap(c->arena_off, s.arena_off);
    std::swap(c->arena_peak, s.arena_peak);
    std::swap(c->fft_blocks, s.fft_blocks);
    std::swap(c->fft_block_i, s.fft_block_i);
    std::swap(c->fft_word_i, s.fft_word_i);
    std::swap(c->act_scale, s.act_scale);
    std::swap(c->scale_scratch, s.scale_scratch);
  }
  int fork() {
    if (!on) return JCM_OK;
    JCM_TRY(side_init(c));
    if (c->dry) return JCM_OK;
    HIP_TRY(hipEventRecord(c->side.fork, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->side.stream, c->side.fork, 0));
    forked = true;
    return JCM_OK;
  }
  void enter() {
    if (!on || inside) return;
    swap();
    if (fresh) c->arena_off = 0;      // the side arena starts over with every pass (the previous pass's side work is in front of this pass's fork)
    fresh = false;
    inside = true;
  }
  hipError_t leave() {
    if (!inside) return hipSuccess;
    swap();
    inside = false;
    return forked ? hipEventRecord(c->side.join, c->side.stream) : hipSuccess;
  }
  int join() {
    const hipError_t e = leave();
    if (!forked) return JCM_OK;
    forked = false;
    // (a join event that could not be recorded: the host waits instead)
    if (e != hipSuccess || hipStreamWaitEvent(c->stream, c->side.join, 0) != hipSuccess) HIP_TRY(hipStreamSynchronize(c->side.stream));
    return JCM_OK;
  }
  ~SideBranches() { (void)join(); }
};

// model(x, n_joints), main.py:29-74.  x fp32 NHWC, or (x_u8) a byte image whose values k stand for float32(k) / float32(255): only the conv1 kernels
// read it, and their byte-source variants convert at the load (u8.h).  Intermediate activations fp32 or bf16.

int pd_forward_impl(jcm_ctx* c, const void* x, bool x_u8, int B, int H, int W, float* logits) {
  static const char* const kRes[3] = {"fullres", "halfres", "quarterres"};
  const ConvLayer* L4 = conv_of(c, "conv4_fullres");
  const ConvLayer* L5 = conv_of(c, "conv5");
  if (!L4 || !L5 || !conv_of(c, "conv6")) return fail(JCM_ERR_STATE, "part-detector parameters incomplete");
  const bool bf = c->precision == JCM_PRECISION_BF16;
  const size_t es = bf ? 2 : 4;
  auto act = [&](size_t elems) { return static_cast<void*>(arena_alloc<char>(c, elems * es)); };
  void* x4[3];
  int h4[3], w4[3];
  for (int r = 0; r < 3; ++r) {
    const int sub = 1 << r;
    h4[r] = cdiv2(cdiv2(cdiv2(H / sub)));                        // resize_images(x, [H//2, W//2]) main.py:51,60
    w4[r] = cdiv2(cdiv2(cdiv2(W / sub)));
  }
  const int hh = h4[0], ww = w4[0];
  const ConvLayer* L6 = conv_of(c, "conv6");
  // fp32 handles, model geometry: the full-resolution branch's conv4 hands conv5 the row-transformed MERGED map (conv_fft_rows_fused.hip) -- x1 is never
  // written.  The coarse branches then have to be there first: the branches run half, quarter, full.
  FftMerge mg{nullptr, h4[1], w4[1], nullptr, h4[2], w4[2]};
  bool fuse45 = false;
  // bf16 handles: the same hand-over in 16-bit form (one-part route with 16-bit row-transformed tensors, NHWC bf16 branches)
  const bool h16 = bf && fft_np(c) == 5 && c->fft_t16;
  if ((!bf || h16) && !c->debug_skip && takes_fft(c, L4, B, hh, ww) && takes_fft(c, L5, B, hh, ww) && L4->cout == L5->cin) {
    const ConvArgs a = conv_args(L4, B, hh, ww);
    fuse45 = (c->fft_fuse & 2) && conv_fft_merge_fusable(a, L4->ks, L5->ks, mg, c->fft_reg, h16);
  }
  // branch outputs survive the per-branch scratch, so carve them first: x1 (or conv5's row-transformed input) from the arena, x2 / x3 from the arena of the
  // stream their branches run on
  void* t45 = nullptr;
  FftLink k5, k6;      // conv5 -> conv6
  if (fuse45) {
    const ConvArgs a = conv_args(L4, B, hh, ww);
    t45 = arena_alloc<char>(c, conv_fft_handover_bytes(a, L4->ks, h16));
    x4[0] = nullptr;
  } else {
    x4[0] = act((size_t)B * h4[0] * w4[0] * L4->cout);
  }
  SideBranches side(c, (c->fft_fuse & 4) != 0);
  side.enter();
  for (int r = 1; r < 3; ++r) x4[r] = act((size_t)B * h4[r] * w4[r] * L4->cout);
  (void)side.leave();      // (nothing is forked yet: only the arenas changed places)
  mg.x2 = x4[1]; mg.x3 = x4[2];
  // bf16: the 9x9 chain (conv3 out -> conv4 -> merge -> conv5 -> conv6 in) runs on planar activations [B][C/8][H*W][8]
  // when conv5 takes the strip kernel; every producer / consumer on that chain handles the layout.
  const int planar = bf && L6->thin_bf16 && L4->cout % 8 == 0 && L5->cout % 8 == 0 && takes_strip(L5, B, h4[0], w4[0]) ? 1 : 0;
  // ... except between two frequency-domain layers: their row passes read and write NHWC in whole 128-byte lines per pixel, while a planar
  // tensor gives a lane only the 4 bytes of its channel pair inside a 16-byte unit (3.3 against 4.8 TB/s measured for the inverse row pass).
  // So with conv5 in the frequency domain the chain conv4 -> merge -> conv5 is NHWC; conv5's OUTPUT stays planar for the logits kernel.
  const int planar45 = planar && !takes_fft(c, L5, B, h4[0], w4[0]) ? 1 : 0;
  // A branch whose scale is not an integer takes a real bilinear resize, and the resize kernel reads floats: a byte batch is widened ONCE, in front of the
  // branches (the floats the float entry would have been given), and lives until the last branch has run.
  const float* x_wide = nullptr;
  if (x_u8 && (H % 4 || W % 4)) {
    float* xw32 = arena_alloc<float>(c, (size_t)B * H * W * 3);
    if (!c->dry) HIP_TRY(u8_to_f32_array(static_cast<const uint8_t*>(x), xw32, (size_t)B * H * W * 3, c->stream));
    x_wide = xw32;
  }
  JCM_TRY(side.fork());      // behind the widened byte batch, which both streams only read
  static const int kOrder[3] = {1, 2, 0};
  for (int ri = 0; ri < 3; ++ri) {
    const int r = kOrder[ri];
    if (r == 0) HIP_TRY(side.leave());
    else side.enter();
    const size_t mark = c->arena_off;
    const std::string res = kRes[r];
    const int sub = 1 << r;
    const int hin = H / sub, win = W / sub;
    const ConvLayer* L1 = conv_of(c, "conv1_" + res);
    const ConvLayer* L2 = conv_of(c, "conv2_" + res);
    const ConvLayer* L3 = conv_of(c, "conv3_" + res);
    if (!L1 || !L2 || !L3) return fail(JCM_ERR_STATE, "part-detector parameters incomplete (" + res + ")");
    const void* xin = x;
    bool xin_u8 = x_u8;
    int xh = H, xw = W, xsub = sub;
    if (H % sub || W % sub) {   // non-integer scale: a real bilinear resize, not sub-sampling
      const float* xf = x_u8 ? x_wide : static_cast<const float*>(x);
      float* xr = arena_alloc<float>(c, (size_t)B * hin * win * 3);
      if (!c->dry) HIP_TRY(resize_bilinear(xf, xr, B, H, W, 3, hin, win, c->stream));
      xin = xr; xin_u8 = false; xh = hin; xw = win; xsub = 1;
    }
    const int h2 = cdiv2(cdiv2(hin)), w2 = cdiv2(cdiv2(win));
    void* p1 = nullptr;
    const int sk = c->debug_skip;
    if (sk & 1) p1 = act((size_t)B * h2 * w2 * L1->cout);
    else JCM_TRY(conv1_pool_stage(c, "conv1_" + res, L1, xin, xin_u8, B, xh, xw, xsub, nullptr, &p1));      // main.py:44-45,52-53,61-62
    const int h3 = cdiv2(h2), w3 = cdiv2(w2);
    // fp32 handles: conv2 -> pool2 -> conv3 as one hand-over in row-transformed form (the pool inside the fused row kernel)
    FftLink k2, k3, k4;      // conv2 -> (pool) -> conv3 -> conv4 of this branch
    void* t23 = (bf || sk) ? nullptr : offer_pool_handover(c, L2, L3, B, h2, w2, k2);
    void* c2 = t23 ? nullptr : act((size_t)B * h2 * w2 * L2->cout);
    const Pool2Layout lay = pool2_layout(c, L2, L3, B, h2, w2);
    const int pl23 = lay.pl23, hp = lay.hp;
    ConvCall q2 = conv_call(p1, c2, B, h2, w2);
    q2.act_bf16 = bf; q2.out_planar = pl23; q2.link = &k2; q2.hpool = hp;
    if (!(sk & 4)) JCM_TRY(run_conv(c, "conv2_" + res, q2));     // :46,54,63
    void* p2 = t23 ? nullptr : act((size_t)B * h3 * w3 * L2->cout);
    if (!c->dry && !(sk & 2) && !t23) HIP_TRY(pool2_launch(c, lay, c2, p2, B, h2, w2, L2->cout));      // :47,55,64
    const ConvLayer* L4r = conv_of(c, "conv4_" + res);
    if (!L4r) return fail(JCM_ERR_STATE, "part-detector parameters incomplete (conv4_" + res + ")");
    const int in4 = planar && L3->cout % 8 == 0 && takes_strip(L4r, B, h3, w3) && !takes_fft(c, L4r, B, h3, w3) ? 1 : 0;      // the patch kernels and the row pass read NHWC
    void* t34 = (sk & 24) ? nullptr : offer_handover(c, L3, L4r, B, h3, w3, k3);      // (no hand-over when either side is left out)
    void* c3 = t34 ? nullptr : act((size_t)B * h3 * w3 * L3->cout);
    hand_over(k2, k3);
    ConvCall q3 = conv_call(p2, c3, B, h3, w3);
    q3.act_bf16 = bf; q3.in_planar = pl23; q3.out_planar = in4; q3.link = &k3;
    if (!(sk & 8)) JCM_TRY(run_conv(c, "conv3_" + res, q3));   // :48,56,65
    hand_over(k3, k4);
    if (r == 0 && fuse45) { k4.t_next = t45; k4.next.merge = &mg; }      // conv4_fullres writes conv5's row-transformed (merged) input
    ConvCall q4 = conv_call(c3, x4[r], B, h3, w3);
    q4.act_bf16 = bf; q4.in_planar = in4; q4.out_planar = planar45; q4.link = &k4;
    if (r == 0 && fuse45) JCM_TRY(side.join());      // its fused inverse row kernel reads x2 / x3
    if (!(sk & 16)) JCM_TRY(run_conv(c, "conv4_" + res, q4));   // :49,57,66
    if (r == 0 && fuse45) { hand_over(k4, k5); k5.t_in_16 = h16; }
    c->arena_off = mark;
  }
  // conv5 in the frequency domain: its forward row kernel forms ((x1 + up(x2)) + up(x3)) / 3 while it loads the rows (NHWC inputs: fp32, or
  // bf16 on a bf16 handle, where the merged value is rounded to bf16 as the separate merge kernel's output would be) -- unless conv4_fullres
  // handed the row-transformed merged map over already (fuse45, fp32 handles).
  // (Round 5 measured the alternative for bf16 handles -- the merge as its own bandwidth-bound kernel + conv5's register row pass: 20.45 against
  // 20.11 ms per 256-image step with the fused kernel, three interleaved runs each: writing and re-reading the 1.4 GB merged tensor costs more
  // than the fused kernel's slower rows.)
  JCM_TRY(side.join());      // the merge kernel, or conv5's forward row kernel, reads x2 / x3
  const bool fuse_merge = !fuse45 && takes_fft(c, L5, B, hh, ww) && !planar45;
  void* merged = fuse45 ? nullptr : fuse_merge ? x4[0] : act((size_t)B * hh * ww * L4->cout);
  if (!c->dry && !fuse45 && !fuse_merge && !(c->debug_skip & 32)) {                        // :58,67,69-70
    if (planar45) HIP_TRY(upsample_merge3_planar(x4[0], x4[1], h4[1], w4[1], x4[2], h4[2], w4[2], merged, B, hh, ww, L4->cout, c->stream));
    else HIP_TRY(upsample_merge3(x4[0], x4[1], h4[1], w4[1], x4[2], h4[2], w4[2], merged, bf, B, hh, ww, L4->cout, c->stream));
  }
  const int sk = c->debug_skip;
  void* t56 = (sk & 96) ? nullptr : offer_handover(c, L5, conv_of(c, "conv6"), B, hh, ww, k5);
  void* c5 = t56 ? nullptr : act((size_t)B * hh * ww * L5->cout);
  if (fuse_merge) k5.merge = &mg;
  ConvCall q5 = conv_call(merged, c5, B, hh, ww);
  q5.act_bf16 = bf; q5.in_planar = planar45; q5.out_planar = planar; q5.link = &k5;
  if (!(sk & 32)) JCM_TRY(run_conv(c, "conv5", q5));   // :71
  hand_over(k5, k6);
  ConvCall q6 = conv_call(c5, logits, B, hh, ww);
  q6.act_bf16 = bf; q6.out_f32 = true; q6.in_planar = planar; q6.link = &k6;
  if (!(sk & 64)) JCM_TRY(run_conv(c, "conv6", q6));         // :72
  return JCM_OK;
}

// spatial_model(heat_map), main.py:94-125.
// The 10-channel input is given as channels [0,Ca) of `hm` ([B,5400,Ca]) plus `extra` ([B,5400,10-Ca]): Ca = 10 for
// jcm_sm_forward, Ca = 9 + the torso map inside the tower (the tf.concat of main.py:528 is never materialised).
int sm_forward_impl(jcm_ctx* c, const float* hm, int Ca, const float* extra, int B, float* logits, int extra_ld) {
  if (extra_ld <= 0) extra_ld = kC - Ca;
  if (!c->has_sm) return fail(JCM_ERR_STATE, "spatial-model parameters (bn_sm, energy_*, bias_*) were not set");
  const int P = c->K * (kC - 1);
  if (c->sm_algo == 1) {   // direct convolution
    float* lik = arena_alloc<float>(c, (size_t)B * kC * kHmH * 96);
    float* cpre = arena_alloc<float>(c, (size_t)B * P * kCH * kCW);
    if (c->dry) return JCM_OK;
    HIP_TRY(sm_likelihood(hm, Ca, extra, c->bn_sm_scale, c->bn_sm_shift, lik, B, kC, c->stream, extra_ld));
    HIP_TRY(sm_pair_conv(c->sp_energy, lik, c->cond, cpre, B, P, kC, c->stream));
    HIP_TRY(sm_finish(lik, cpre, c->sp_bias, logits, B, c->K, kC, c->stream));
    return JCM_OK;
  }
  if (c->sm_algo == 3) {   // fused: all transforms in LDS, only the 10 likelihood spectra per image leave the CU
    float2* lhat_t = arena_alloc<float2>(c, (size_t)B * kC * kSpec);
    if (c->dry) return JCM_OK;
    void* scr = nullptr;
    unsigned epoch = 0;
    JCM_TRY(sm_scratch_next(c, &scr, &epoch));
    HIP_TRY(sm_fused_forward(hm, Ca, extra, extra_ld, c->bn_sm_scale, c->bn_sm_shift, c->prior_spec_t, c->cond, c->sp_bias, lhat_t, logits, B, c->K, kC,
                             c->stream, nullptr, scr, epoch));
    return JCM_OK;
  }
  return fail(JCM_ERR_STATE, "sm_algo must be 3 (transforms in LDS) or 1 (direct)");
}

}  // namespace jcm
