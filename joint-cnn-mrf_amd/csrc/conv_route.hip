// How one conv layer runs: the route choice (direct kernels or the frequency domain), the launch, and the filter-spectra cache of the
// frequency-domain route.  Host code only.
#include <string>

#include "conv_fft_plan.h"
#include "ctx.h"

namespace jcm {

// bf16 handles: does a [B,H,W,Cin] launch of this 9x9 layer take the flattened-strip kernel (which reads / writes the
// planar activation layout at full speed)?
bool takes_strip(const ConvLayer* L, int B, int H, int W) {
  if (!L->wp_bf16 || L->thin_bf16 || conv_igemm_bf16_bn(L->cout, L->ks) != 256) return false;
  ConvArgs a = conv_args(L, B, H, W);
  a.CoutP = L->coutp_bf16;
  a.out_planar = 1;
  return conv_strip_bf16_supported(a, L->ks);
}

// will this bf16 5x5 layer run on conv5_strip_bf16_kernel (which reads and writes either activation layout)?
bool takes_c5strip(const ConvLayer* L, int B, int H, int W) {
  if (!L->wp_bf16 || L->ks != 5 || conv_igemm_bf16_bn(L->cout, L->ks) != 128 || L->cout % 8) return false;
  ConvArgs a = conv_args(L, B, H, W);
  a.CoutP = L->coutp_bf16;
  return conv5_strip_bf16_supported(a, L->ks);
}

// The direct (not frequency-domain) stride-1 kernel of a layer: the ONE choice behind the launch and behind jcm_conv_kernel_name.
// a: the launch's arguments as far as the *_supported predicates read them (shape, CoutP, layouts, hpool).
enum class DirectConv { KxfoldBf16, ThinBf16, IgemmBf16, ThinSplit16, ThinF32, SplitF32, IgemmF32 };
static DirectConv direct_route(const jcm_ctx* c, const ConvLayer* L, const ConvArgs& a, bool act_bf16, bool out_f32) {
  if (act_bf16) {
    if (L->thin_bf16 && out_f32) return L->wp_kxfold && conv_kxfold_bf16_supported(a, L->ks) ? DirectConv::KxfoldBf16 : DirectConv::ThinBf16;
    return DirectConv::IgemmBf16;
  }
  const bool use_split = L->wp_split && (L->thin ? c->f32_conv == 2 : conv_split_supported(L->ks, L->cin, L->coutp_split, a.B, a.H, a.W, c->split_min_wgs));
  if (L->thin) return use_split ? DirectConv::ThinSplit16 : DirectConv::ThinF32;
  return use_split ? DirectConv::SplitF32 : DirectConv::IgemmF32;
}
// the kernel a stand-alone stride-1 launch of this layer runs on this handle (jcm_conv_kernel_name; the stride-2 first layer is pd_tower.hip's)
const char* conv_kernel_name(jcm_ctx* c, const ConvLayer* L, int B, int H, int W) {
  if (takes_fft(c, L, B, H, W)) return "conv_fft(cgemm_split_kernel)";
  const bool bf = c->precision == JCM_PRECISION_BF16;
  ConvArgs a = conv_args(L, B, H, W);
  a.relu_bn = L->has_bn ? 1 : 0;
  a.CoutP = bf ? L->coutp_bf16 : L->coutp;
  switch (direct_route(c, L, a, bf, L->thin_bf16)) {
    case DirectConv::KxfoldBf16: return "conv_kxfold_bf16_kernel";
    case DirectConv::ThinBf16: return "conv_thin_bf16_kernel";
    case DirectConv::ThinSplit16: return "conv_thin_split16_kernel";
    case DirectConv::ThinF32: return "conv_thin_f32_kernel";
    case DirectConv::SplitF32: return "conv_split_kernel";
    case DirectConv::IgemmF32: return "conv_igemm_f32_kernel";
    case DirectConv::IgemmBf16: break;
  }
  const int bn = conv_igemm_bf16_bn(L->cout, L->ks);      // conv_igemm_bf16 picks among its kernels by these conditions
  return bn == 256 && conv_strip_bf16_supported(a, L->ks) ? "conv_strip_bf16_kernel"
         : L->ks == 5 && bn == 128 && conv5_strip_bf16_supported(a, L->ks) ? "conv5_strip_bf16_kernel" : "conv_igemm_bf16_kernel";
}

// The launch itself (kernel choice by precision / f32_conv); run_conv_layer brackets it with the timing events.
static int launch_conv_layer(jcm_ctx* c, const ConvLayer* L, const ConvCall& q) {
  ConvArgs a = conv_args(L, q.B, q.H, q.W);
  a.x = q.x; a.wp = q.act_bf16 ? L->wp_bf16 : static_cast<const void*>(L->wp); a.bias = L->bias; a.scale = L->scale; a.shift = L->shift; a.out = q.out;
  a.relu_bn = L->has_bn && !q.linear ? 1 : 0;
  a.in_planar = q.in_planar; a.out_planar = q.out_planar;
  a.hpool = q.hpool;
  a.CoutP = q.act_bf16 ? L->coutp_bf16 : L->coutp;
  if ((q.in_planar || q.out_planar) && !q.act_bf16) return fail(JCM_ERR_ARG, "planar activations exist on the bf16 path only");
  if (a.hpool && !q.act_bf16) return fail(JCM_ERR_STATE, "half pool requested on an fp32 layer");
  if (a.hpool && (q.out_f32 || L->thin_bf16 || L->ks != 5 || conv_igemm_bf16_bn(L->cout, L->ks) != 128 || !conv5_strip_bf16_supported(a, L->ks)))
    return fail(JCM_ERR_STATE, "half pool requested for a layer that does not run on conv5_strip_bf16_kernel");
  const DirectConv k = direct_route(c, L, a, q.act_bf16, q.out_f32);
  if (k == DirectConv::ThinSplit16 || k == DirectConv::SplitF32) {     // fp16x3: lift this input into the fp16 range by its own power-of-two scale
    HIP_TRY(pow2_scale_of(static_cast<const float*>(q.x), (size_t)q.B * q.H * q.W * L->cin, c->act_scale, c->scale_scratch, c->stream));
    a.in_scale = c->act_scale;
    a.w_scale = L->wscale;
    a.wp = L->wp_split;
    a.CoutP = k == DirectConv::ThinSplit16 ? 16 : L->coutp_split;
  }
  switch (k) {
    case DirectConv::KxfoldBf16:
      a.wp = L->wp_kxfold;
      HIP_TRY(conv_kxfold_bf16(a, c->stream));
      break;
    case DirectConv::ThinBf16: HIP_TRY(conv_thin_bf16(a, c->stream)); break;
    case DirectConv::IgemmBf16: HIP_TRY(conv_igemm_bf16(a, L->ks, q.out_f32, c->stream)); break;
    case DirectConv::ThinSplit16: HIP_TRY(conv_thin_split16(a, c->stream)); break;
    case DirectConv::ThinF32: HIP_TRY(conv_thin_f32(a, c->stream)); break;
    case DirectConv::SplitF32: HIP_TRY(conv_split_f32(a, L->ks, 2, c->stream)); break;
    case DirectConv::IgemmF32: HIP_TRY(conv_igemm_f32(a, L->ks, c->stream)); break;
  }
  return JCM_OK;
}

// Does this stride-1 layer run in the frequency domain (conv_fft.hip)?  fp32 handles: inference and the training step (forward and data
// gradient; the filter spectra are recomputed after every update -- refresh_derived invalidates them); bf16 handles: inference only.
bool takes_fft(jcm_ctx* c, const ConvLayer* L, int B, int H, int W) {
  if (!c->conv9_fft || c->f32_conv != 0 || (c->train && c->precision != JCM_PRECISION_F32) || (L->ks != 9 && L->ks != 5) || L->cin == 3 || !L->w_raw) return false;
  // bf16 handles: the wide 9x9 layers only.  Round 5 measured the 5x5 layers of a bf16 handle on this route at B = 256 (HIP events per layer, same box):
  // conv2 (64 -> 128) 1.95 / 0.53 / 0.14 ms on conv5_strip_bf16_kernel against 4.20 / 0.90 / 0.25 ms here (its 128 output channels make the fp32
  // product spectra 6 of its 15 GB); conv3 (128 -> 256) 1.82 / 0.50 / 0.17 against 1.73 / 0.53 / 0.18 ms -- break-even, and the tower's error
  // against the bf16-operand oracle grows from 4.3e-3 to 5.9e-3 of the logit scale: both stay on the strip kernels.
  if (c->precision == JCM_PRECISION_BF16 && (L->ks != 9 || L->thin_bf16 || L->cout % 8)) return false;
  return conv_fft_supported(conv_args(L, B, H, W), L->ks);
}
// ---- the filter-spectra cache (jcm_ctx::fft_w): spectra per (layer, map size, form), packed on first use and after every weight update ----
// The one place that spells the keys: "<scope>@HxW" (whole maps), "<scope>@winHxW" (overlap-save windows), "<scope>@rowsHxW" (the logits layer's row spectra).
enum class FftForm { Map, Win, Rows };
static std::string fft_cache_key(const std::string& scope, FftForm form, int H, int W) {
  return scope + (form == FftForm::Win ? "@win" : form == FftForm::Rows ? "@rows" : "@") + std::to_string(H) + "x" + std::to_string(W);
}
bool fft_spectra_valid(jcm_ctx* c, const std::string& scope, int H, int W, int circ) {
  auto it = c->fft_w.find(fft_cache_key(scope, circ ? FftForm::Win : FftForm::Map, H, W));
  return it != c->fft_w.end() && it->second.valid;
}
// A data gradient's pseudo-layer ("dgrad:<scope>", jcm_train.hip) holds the flipped, transposed filter of <scope>: the same set of taps per (ci, co) pair,
// hence the same bound.  The scale words of <scope>'s forward spectra of the same geometry when they are valid (always, inside a step), else null.
static const float* fft_forward_wscale(jcm_ctx* c, const std::string& scope, FftForm form, int H, int W) {
  static const std::string kDgrad = "dgrad:";
  if (scope.compare(0, kDgrad.size(), kDgrad) != 0) return nullptr;
  auto it = c->fft_w.find(fft_cache_key(scope.substr(kDgrad.size()), form, H, W));
  return it != c->fft_w.end() && it->second.valid ? it->second.wscale : nullptr;
}
void fft_cache_drop(jcm_ctx* c) {
  for (auto& kv : c->fft_w) (void)hipFree(kv.second.p);
  c->fft_w.clear();
}
void fft_cache_invalidate(jcm_ctx* c) {
  for (auto& kv : c->fft_w) kv.second.valid = false;
}
// The entry of `key`, created with room for `wbytes` of spectra (+ the two words of their scale, np = 4) when it is not there.  The cache is bounded (option
// "fft_cache_gb", default 64): a caller that walks many image sizes (7.7 GB per size for conv5) makes it drop every spectrum before it grows past the bound.
// (A training handle keeps the spectra of BOTH geometries of a layer -- overlap-save windows for steps of <= 32 images, the whole map for evaluation
// forwards and larger batches -- so that a loop that alternates training steps and evaluation does not re-pack gigabytes and stall the stream at
// every flip (round 5 dropped the other geometry here); the bound is what limits the footprint.)
static int fft_cache_get(jcm_ctx* c, const std::string& scope, const std::string& key, size_t wbytes, jcm_ctx::FftW** out) {
  if (!c->fft_w.count(key)) {
    const size_t cap = (size_t)c->fft_cache_gb << 30;
    size_t held = 0;
    for (auto& kv : c->fft_w) held += kv.second.bytes;
    if (held + wbytes > cap && !c->fft_w.empty()) {
      JCM_TRY(sync_streams(c));            // earlier layers of this forward may still read theirs, on either stream
      fft_cache_drop(c);
    }
  }
  jcm_ctx::FftW& fw = c->fft_w[key];
  if (!fw.p) {
    const size_t wb = (wbytes + 255) & ~size_t(255);
    fw.bytes = wb + 256;
    if (hipMalloc(&fw.p, fw.bytes) != hipSuccess) {
      const size_t mb = fw.bytes >> 20;
      c->fft_w.erase(key);
      return fail(JCM_ERR_HIP, "out of device memory for the filter spectra of '" + scope + "' (" + std::to_string(mb) + " MB); jcm_set_option(\"conv9_fft\", 0) selects the direct kernels");
    }
    fw.wscale = reinterpret_cast<float*>(static_cast<char*>(fw.p) + wb);
  }
  *out = &fw;
  return JCM_OK;
}

// n zeroed device words (one per image of a row-transformed tensor).  Blocks are zeroed when they are created and every time the handle starts
// over at the first one (CallOrder: between calls, in stream order, behind every kernel that read the old words); a word is handed out once per lap.
int fft_new_words(jcm_ctx* c, int n, float** w) {
  if (n < 1) return fail(JCM_ERR_ARG, "fft_new_words: n < 1");
  for (;;) {
    if (c->fft_block_i < (int)c->fft_blocks.size()) {
      jcm_ctx::WordBlock& b = c->fft_blocks[c->fft_block_i];
      if (c->fft_word_i + n <= b.cap) {
        *w = b.p + c->fft_word_i;
        c->fft_word_i += n;
        return JCM_OK;
      }
      ++c->fft_block_i;      // the rest of this block stays unused until the next lap
      c->fft_word_i = 0;
      continue;
    }
    jcm_ctx::WordBlock b;
    b.cap = n > jcm_ctx::kFftWords ? n : jcm_ctx::kFftWords;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.p), (size_t)b.cap * sizeof(float)));
    if (hipError_t e = hipMemsetAsync(b.p, 0, (size_t)b.cap * sizeof(float), c->stream); e != hipSuccess) {
      (void)hipFree(b.p);
      return fail(JCM_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    }
    c->fft_blocks.push_back(b);
  }
}
int run_conv_fft(jcm_ctx* c, const ConvLayer* L, const std::string& scope, const ConvCall& q) {
  FftLink alone;
  FftLink& k = q.link ? *q.link : alone;
  const int B = q.B, H = q.H, W = q.W, circ = q.circ;
  const FftLayout in_layout = q.act_bf16 ? (q.in_planar ? kFftBf16Planar : kFftBf16Nhwc) : kFftF32Nhwc;
  const FftLayout out_layout = (q.act_bf16 && !q.out_f32) ? (q.out_planar ? kFftBf16Planar : kFftBf16Nhwc) : kFftF32Nhwc;
  FftArgs a = fft_args(L, B, H, W);
  a.x = q.x; a.bias = L->bias; a.scale = L->scale; a.shift = L->shift; a.out = q.out;
  a.CoutP = L->cout; a.relu_bn = L->has_bn && !q.linear ? 1 : 0;
  a.circ = circ;
  a.rows_mfma = c->fft_rows_mfma;
  a.fft_reg = c->fft_reg;
  // the windows are gathered by the forward row pass (win_map) and / or scattered by the inverse row pass (win_scatter): one geometry
  a.win_map = k.win_map; a.win_scatter = k.win_scatter; a.win = k.win;
  const size_t mark = c->arena_off;
  const int np = fft_np(c);      // operand form of the channel GEMM (kernels.h: FftOperand)
  const int pool_ks = k.next.pool ? k.next.ks_next : 0;
  // fp32 handles, the pool hand-over conv2 -> pool -> conv3 on the model's 120 x 180 map: the layer runs as 2 x 2 tiles in the 64 x 96 transform of the
  // 60 x 90 maps (FftArgs::tiles, conv_fft_reg_tiles.hip) -- a quarter of the filter spectra, and the register row kernels
  a.tiles = c->fft_tiles && k.next.pool ? 1 : 0;
  FftPlan plan = conv_fft_plan(a, L->ks, np, pool_ks);
  if (a.tiles && conv_fft_tiles_refusal(plan, in_layout, out_layout, k)) {
    a.tiles = 0;
    plan = conv_fft_plan(a, L->ks, np, pool_ks);
  }
  const int wH = a.tiles ? H / 2 : H, wW = a.tiles ? W / 2 : W;      // the map size the filter spectra are for
  // fp32 handles, the last layer behind a hand-over (conv5 -> conv6 of jcm_pd_forward): 9 output channels do not pay for two column passes and a channel GEMM --
  // the channels are contracted on the row spectra that arrive in t_in (conv_fft_logits.hip).  Not on a handle with training state (one scale per tensor there).
  const int common = c->train ? 1 : 0;
  bool lrows = false;
  if (c->fft_logits_rows && k.t_in && !a.tiles) {
    const FftPlan lp = conv_fft_logits_plan(a);
    lrows = !conv_fft_logits_refusal(lp, L->ks, np, in_layout, out_layout, k, common);
    if (lrows) plan = lp;
  }
  void* work = arena_alloc<char>(c, plan.ok ? plan.total : 0);
  c->arena_off = mark;                                   // scratch of this layer only: later layers run behind it on the stream
  if (c->dry) return JCM_OK;
  const FftForm form = circ ? FftForm::Win : lrows ? FftForm::Rows : FftForm::Map;
  jcm_ctx::FftW* fwp = nullptr;
  JCM_TRY(fft_cache_get(c, scope, fft_cache_key(scope, form, wH, wW),
                        lrows ? conv_fft_logits_weight_bytes(wH, wW, L->cin) : conv_fft_weight_bytes(wH, wW, L->ks, L->cin, L->cout, np, circ), &fwp));
  jcm_ctx::FftW& fw = *fwp;
  if (!fw.valid) {
    if (lrows) HIP_TRY(conv_fft_logits_pack(L->w_raw, fw.p, wH, wW, L->cin, L->cout, c->stream, fw.wscale));
    else HIP_TRY(conv_fft_pack_weights(L->w_raw, fw.p, wH, wW, L->ks, L->cin, L->cout, np, c->precision == JCM_PRECISION_BF16, c->stream, fw.wscale, circ,
                                       np >= 4 ? fft_forward_wscale(c, scope, form, wH, wW) : nullptr));
    fw.valid = true;
  }
  plan.map.wp = plan.col.wp = plan.inv.wp = fw.p;
  hipEvent_t e0 = nullptr, e1 = nullptr, g0 = nullptr, g1 = nullptr;
  JCM_TRY(prof_begin(c, &e0, &e1));
  if (c->profile && (prof_event(c, &g0) != JCM_OK || prof_event(c, &g1) != JCM_OK)) { g0 = g1 = nullptr; }
  FftScale sc;
  if (np >= 4) {
    // the word of this layer's input: handed over with t_in / ready spectra, or a fresh one for this layer's own row pass
    sc.tmax = k.tmax_in;
    if ((k.t_in || k.xs_ready) && !sc.tmax) return fail(JCM_ERR_STATE, "conv_fft '" + scope + "': a handed-over tensor without its scale word");
    if (!sc.tmax) JCM_TRY(fft_new_words(c, a.tiles ? 4 * B : B, &sc.tmax));      // (tiles: one word per tile, the row of the channel GEMM)
    if (k.t_next) JCM_TRY(fft_new_words(c, B, &sc.tmax_next));
    sc.winv = fw.wscale + 1;
    sc.common = common;      // a handle with training state: one scale per tensor (the weight gradient sums over the images)
    // 16-bit T / T' between the row and column passes: bf16 tensors on both sides of the layer, one-part spectra, nothing handed over or kept
    // ... except the merge hand-over conv4_fullres -> conv5 of jcm_pd_forward, which exists in 16-bit form (rows_inv_merge_fwd_reg_kernel<.., true>)
    sc.t16 = (np == kFftFp16x1 && c->fft_t16 && in_layout != kFftF32Nhwc && out_layout != kFftF32Nhwc && !k.xs && (!k.t_in || k.t_in_16) && (!k.t_next || (k.next.merge && !k.t_in))) ? 1 : 0;
  }
  k.tmax = sc.tmax;
  k.tmax_next = sc.tmax_next;      // the layer that takes t_next takes its words too
  const char* why = nullptr;
  const hipError_t e = lrows ? conv_fft_logits_f32(plan, L->ks, np, in_layout, out_layout, work, k, g0, g1, c->stream, &sc, &why)
                             : conv_fft_f32(plan, in_layout, out_layout, work, k, g0, g1, c->stream, np >= 4 ? &sc : nullptr, &why);
  if (g0 && g1 && e == hipSuccess) c->prof[scope + "/gemm"].emplace_back(g0, g1);
  else { if (g0) c->event_pool.push_back(g0); if (g1) c->event_pool.push_back(g1); }
  prof_end(c, scope, e0, e1, e == hipSuccess);
  if (e != hipSuccess) return fail(JCM_ERR_HIP, why ? "conv_fft '" + scope + "': " + why : std::string("conv_fft_f32: ") + hipGetErrorString(e));
  return JCM_OK;
}

// One conv layer.  Activations are fp32, or bf16 when the handle runs the bf16 path (`act_bf16`);
// `out_f32` forces an fp32 result (the logits layer).
int run_conv_layer(jcm_ctx* c, const ConvLayer* L, const std::string& scope, const ConvCall& q) {
  const bool fft = q.stride == 1 && takes_fft(c, L, q.B, q.H, q.W);
  // linear (jcm_conv_layer_pre): the epilogue of a BatchNorm layer stops at conv + bias; fp32 handles, a layer that stands alone
  if (q.linear && (q.act_bf16 || q.x_u8 || q.hpool || (q.link && !q.link->empty()))) return fail(JCM_ERR_STATE, "the linear epilogue of layer '" + scope + "' exists for a stand-alone fp32 layer only");
  // a request aimed at a route this layer does not take is an error of the caller, never dropped (nor left for the next layer)
  if (!fft && q.link && !q.link->empty()) return fail(JCM_ERR_STATE, "layer '" + scope + "' was given a frequency-domain hand-over but does not run in the frequency domain");
  if (q.hpool && (fft || q.stride != 1)) return fail(JCM_ERR_STATE, "half pool requested for layer '" + scope + "', which does not run on conv5_strip_bf16_kernel");
  if (q.stride == 2) {
    if (c->dry) return JCM_OK;
    if (!(L->ks == 5 && L->cin == 3 && L->has_bn))
      return fail(JCM_ERR_ARG, "stride-2 kernel exists for 5x5, Cin=3, BN layers only (" + scope + ")");
    HIP_TRY(conv1_5x5s2(q.x, L->w_raw, L->bias, L->scale, L->shift, q.out, q.act_bf16, q.B, q.H, q.W, q.sub, L->cout, c->stream, q.x_u8, q.linear != 0));
    return JCM_OK;
  }
  if (fft) return run_conv_fft(c, L, scope, q);
  if (c->dry) return JCM_OK;
  if (q.stride != 1 || !(q.act_bf16 ? L->wp_bf16 : static_cast<const void*>(L->wp))) return fail(JCM_ERR_ARG, "no kernel for layer '" + scope + "' with stride " + std::to_string(q.stride));
  if (!q.act_bf16 && L->wp_stale) {
    HIP_TRY(pack_weights_f32(L->w_raw, L->wp, L->ks, L->cin, L->cout, L->coutp, c->stream));
    L->wp_stale = false;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  JCM_TRY(prof_begin(c, &e0, &e1));
  const int r = launch_conv_layer(c, L, q);
  prof_end(c, scope, e0, e1, r == JCM_OK);
  return r;
}
int run_conv(jcm_ctx* c, const std::string& scope, const ConvCall& q) {
  const ConvLayer* L = conv_of(c, scope);
  if (!L) return fail(JCM_ERR_STATE, "no conv layer '" + scope + "' (set '" + scope + "/weights' and finalize)");
  if (q.x_u8 && q.stride != 2) return fail(JCM_ERR_ARG, "byte images feed the stride-2 first layer only (" + scope + ")");
  return run_conv_layer(c, L, scope, q);
}

}  // namespace jcm
