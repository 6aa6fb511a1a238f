// Joint training step behind include/jcm.h (main.py:511-577): forward in
// training mode (batch-statistics BatchNorm + moving-average update), the two soft-label spatial
// cross-entropies + weight decay, and the backward pass of the part detector and the spatial model.
// fp32 throughout; every convolution (forward, data gradient, weight gradient) runs on v_mfma_f32_32x32x2_f32.
// The state the step runs on, the optimizer and the state entry points: train.h, train_state.hip.
#include "train.h"

using namespace jcm;

namespace {

// the packed data-gradient filters of a layer on the direct kernels, repacked here after a weight update left them stale (train_state.hip: dgrad_filters_stale)
int ensure_dgrad_packed(jcm_ctx* c, const std::string& scope) {
  TrainState* t = c->train;
  const ConvLayer* L = conv_of(c, scope);
  DgradW& d = t->dgrad[scope];
  if (!d.stale) return JCM_OK;
  d.stale = false;
  if (d.wd_bf16) {
    HIP_TRY(flip_transpose_weights(L->w_raw, t->scratch_flip, L->ks, L->cin, L->cout, d.cinp_bf16, c->stream));
    HIP_TRY(pack_weights_bf16(t->scratch_flip, d.wd_bf16, L->ks, d.cinp_bf16, L->cin, d.coutp_bf16, c->stream));
    return JCM_OK;
  }
  HIP_TRY(flip_transpose_weights(L->w_raw, t->scratch_flip, L->ks, L->cin, L->cout, d.cinp, c->stream));
  HIP_TRY(pack_weights_f32(t->scratch_flip, d.wd, L->ks, d.cinp, L->cin, d.coutp, c->stream));
  // gradients: bf16 parts (full fp32 range) in mode 1; fp16 parts + a per-tensor power-of-two scale in mode 2
  if (d.wd_split) HIP_TRY(pack_weights_split(t->scratch_flip, d.wd_split, L->ks, d.cinp, L->cin, L->cin, 2, c->stream, L->wscale));
  return JCM_OK;
}

// Every write of the gradients with this name prefix has been enqueued on the stream: tell the host, which can start
// reducing that range on another stream (after an event recorded now) while the backward pass goes on.
void notify_ready(jcm_ctx* c, const std::string& prefix) {
  TrainState* t = c->train;
  if (c->dry || !t->ready_fn) return;
  auto it = t->ranges.find(prefix);
  if (it == t->ranges.end() || it->second.second <= 0) return;
  // user code runs WITHOUT the device's call-chain lock (it may call jcm_* entry points, also of this handle: CallOrder::nested)
  if (c->order) c->order->release();
  t->ready_fn(t->ready_user, it->second.first, it->second.second);
  if (c->order) c->order->acquire();
}

float* grad_of(TrainState* t, float* grads, const std::string& name) {
  auto it = t->index.find(name);
  return it == t->index.end() ? nullptr : grads + t->slots[it->second].off;
}

// Activations and their gradients are fp32, or bf16 on a bf16 handle (mixed precision: fp32 master weights,
// statistics, losses, spatial model and optimizer; bf16 tensors between the layers, bf16 MFMA with fp32 accumulate).
inline bool bf(const jcm_ctx* c) { return c->precision == JCM_PRECISION_BF16; }
inline void* act(jcm_ctx* c, size_t elems) { return arena_alloc<char>(c, elems * (bf(c) ? 2 : 4)); }

// ---- overlap-save windows (fp32 handles; FftArgs::circ).  At 16 images per GPU every pass of a wide layer is bound by filter-sized
// spectra -- F Cin Cout complex numbers written by the packers, read by the forward and the data-gradient GEMM, written and read as the weight gradient's
// per-frequency products: 6 x 6.6 GB per step for conv5 on the 64 x 96 transform of its 60 x 90 map.  Cut into 32 x 32 windows (24 x 24 valid pixels + a halo
// of 4, 3 x 4 windows per map) the same layer has 544 frequencies instead of 3136 and 192 "images" instead of 16: the filter-sized tensors shrink 5.8x, the
// activation-sized ones (which were 3 % of the traffic) grow 2.1x.
constexpr int kWin = 32, kWinValid = kWin - 8;
// a layer takes the windows when its map has at least kWinFreqRatio x the frequencies of a window ...
constexpr double kWinFreqRatio = 1.5;      // (round 6: 1.5 -- the 30 x 45 maps too, 936 frequencies against 544: 24.03 -> 23.87 ms; rounds 3-5: 2)
// ... and Cin * Cout >= kWinMinCC
constexpr long kWinMinCC = 128l * 256;      // (round 6: 128 x 256 = conv3_fullres too, now that the windows are gathered and scattered inside the row passes: 24.20 -> 24.03 ms; 64 x 128: 24.87)
static bool takes_windows(jcm_ctx* c, const ConvLayer* L, int B, int H, int W, int* TY, int* TX) {
  if (bf(c) || !c->fft_win || !takes_fft(c, L, B, H, W)) return false;
  int NY = 0, NX = 0, MT = 0;
  if (!conv_fft_geometry(H, W, L->ks, B, L->cout, fft_np(c), &NY, &NX, &MT)) return false;
  if (kWinFreqRatio * kWin * (kWin / 2 + 1) > NY * (NX / 2 + 1)) return false;      // at least half the frequencies, or the larger activation spectra eat the gain (30 x 45 maps: 936 -> 544)
  // ... and filters wide enough that their spectra dominate: the windows cost a gather, a scatter and 2.1x the transform work per channel (measured at 16 images:
  // with every 60 x 90 layer on windows the step stayed at 36 ms -- 9.7 ms saved on filter-sized tensors, as much spent on activation-sized ones)
  if ((long)L->cin * L->cout < kWinMinCC) return false;
  // ... and a batch small enough: what the windows save (filter-sized traffic, independent of the batch: 9.7 ms per step) is spent again on activation-sized work
  // that grows with it (4.4 ms at 16 images)
  if (B > 32) return false;
  *TY = (H + kWinValid - 1) / kWinValid;
  *TX = (W + kWinValid - 1) / kWinValid;
  ConvArgs a = conv_args(L, B * *TY * *TX, kWin, kWin);
  if (!conv_fft_supported(a, L->ks, 1)) return false;
  // the data gradient runs the same windows through the flipped, transposed filter: a layer with Cin = this layer's Cout.  dz reaches it with the
  // stride of the packed data-gradient filter (Cout rounded up to 16), and the weight gradient takes the windows only for a stride that is a
  // multiple of 64: a Cout of 80, 96, 160 ... stays on the whole map, where both gradients fall back to the direct kernels (such a layer on windows
  // ran the data gradient's transform with 96 channels, which conv_fft_f32 refuses: the step failed)
  if (L->cout % 64) return false;
  ConvArgs d = a;
  d.Cin = L->cout; d.Cout = L->cin;
  return conv_fft_supported(d, L->ks, 1);
}


// The windows of a [B, H, W, C] map as the input of a transform.  Where the forward row pass can cut them out of the map itself (round 6) the gathered tensor
// does not exist: *in_pass, and the caller hands the map over as win_map; otherwise they are gathered into the arena buffer returned here (win_gather).
float* win_buffer(jcm_ctx* c, const WinGeom& g, int C, bool* in_pass) {
  *in_pass = conv_fft_win_gather_supported(kWin, C, c->fft_reg);
  return *in_pass ? nullptr : arena_alloc<float>(c, (size_t)g.BW() * kWin * kWin * C);
}
hipError_t win_gather(jcm_ctx* c, const WinGeom& g, const void* map, float* buf, int C, int valid_only) {
  return window_gather_f32(static_cast<const float*>(map), buf, g.B, g.H, g.W, C, kWin, g.TY, g.TX, valid_only, c->stream);
}

// One frequency-domain layer on the windows of a map: in [B, H, W, L->cin] -> gather (or win_map) -> L on BW() circular kWin x kWin "images", filter spectra
// under `key` -> scatter of the valid regions (or win_scatter: the inverse row pass stores into the map) -> out [B, H, W, L->cout].  xs (optional): the windows'
// spectra are kept there, *xs_tmax = their scale words.  The arena is reset behind it (later work runs behind the scatter on the stream).
int run_conv_windows(jcm_ctx* c, const ConvLayer* L, const std::string& key, const WinGeom& g, const void* in, void* out, void* xs = nullptr, float** xs_tmax = nullptr) {
  const size_t mark = c->arena_off;
  bool gw = false;
  float* xw = win_buffer(c, g, L->cin, &gw);
  const bool sw = conv_fft_win_scatter_supported(kWin, L->cout, c->fft_reg);
  float* rw = sw ? static_cast<float*>(out) : arena_alloc<float>(c, (size_t)g.BW() * kWinValid * kWinValid * L->cout);
  if (!c->dry && !gw) HIP_TRY(win_gather(c, g, in, xw, L->cin, 0));
  FftLink k;
  k.win = g;
  if (gw) k.win_map = in;
  k.win_scatter = sw;
  k.xs = xs;
  ConvCall q = conv_call(xw, rw, g.BW(), kWin, kWin);
  q.circ = 1; q.link = &k;
  JCM_TRY(run_conv_fft(c, L, key, q));
  if (!c->dry) {
    if (xs_tmax) *xs_tmax = k.tmax;
    if (!sw) HIP_TRY(window_scatter_f32(rw, static_cast<float*>(out), g.B, g.H, g.W, L->cout, kWin, g.TY, g.TX, c->stream));
  }
  c->arena_off = mark;
  return JCM_OK;
}

// the convolution half: r = relu(conv + b) (or conv + b), the input spectra kept for the weight gradient where the layer runs in the frequency domain
int conv_train_fwd_conv(jcm_ctx* c, LayerFwd& f, int stride, const void* x, int B, int Hin, int Win, int sub) {
  TrainState* t = c->train;
  f.L = conv_of(c, f.scope);
  if (!f.L) return fail(JCM_ERR_STATE, "no conv layer '" + f.scope + "'");
  f.in = x;
  f.H = stride == 2 ? cdiv2(Hin / sub) : Hin;
  f.W = stride == 2 ? cdiv2(Win / sub) : Win;
  const size_t N = (size_t)B * f.H * f.W;
  f.r = f.L->has_bn ? act(c, N * f.L->cout) : static_cast<void*>(arena_alloc<float>(c, N * f.L->cout));   // the logits stay fp32
  ConvLayer L = *f.L;
  L.scale = t->ones;       // epilogue = relu(z + b) * 1 + 0
  L.shift = t->zeros;
  if (int TY = 0, TX = 0; stride == 1 && takes_windows(c, &L, B, Hin, Win, &TY, &TX)) {      // the windows' spectra are kept for the weight gradient
    f.win = WinGeom{B, Hin, Win, TY, TX};
    FftArgs ax = fft_args(&L, f.win.BW(), kWin, kWin);
    ax.circ = 1;
    f.xs = arena_alloc<char>(c, conv_fft_xs_bytes(ax, L.ks, fft_np(c)));
    return run_conv_windows(c, &L, f.scope, f.win, x, f.r, f.xs, &f.xs_tmax);
  }
  FftLink k;
  if (stride == 1 && !bf(c) && takes_fft(c, &L, B, Hin, Win)) {      // keep the input spectra: the weight gradient is taken in the frequency domain too
    f.xs = arena_alloc<char>(c, conv_fft_xs_bytes(fft_args(&L, B, Hin, Win), L.ks, fft_np(c)));
    k.xs = f.xs;
  }
  ConvCall q = conv_call(x, f.r, B, Hin, Win);
  q.stride = stride; q.sub = sub; q.act_bf16 = bf(c); q.out_f32 = !f.L->has_bn; q.link = &k;
  JCM_TRY(run_conv_layer(c, &L, f.scope, q));
  if (f.xs && !c->dry) f.xs_tmax = k.tmax;
  return JCM_OK;
}

// the BatchNorm half, on f.r of a layer whose L / H / W are set: batch statistics into BnSave and the moving averages, y = BN(r) (a layer without BatchNorm: y is r)
// pool_out (optional): the 2x2/2 max pool of the layer's output goes there -- taken by the BatchNorm kernel while it writes y where that form exists
// y_dst (optional): y is written there instead of the arena (jcm_train_bn_fwd: the caller's tensor)
int conv_train_fwd_bn(jcm_ctx* c, LayerFwd& f, int B, void* pool_out, void* y_dst = nullptr) {
  TrainState* t = c->train;
  const size_t N = (size_t)B * f.H * f.W;
  if (!f.L->has_bn) {
    f.y = f.r;
    if (pool_out && !c->dry) HIP_TRY(max_pool_2x2(f.y, pool_out, bf(c), B, f.H, f.W, f.L->cout, c->stream));
    return JCM_OK;
  }
  f.y = y_dst ? y_dst : act(c, N * f.L->cout);
  if (c->dry) return JCM_OK;
  BnSave& s = t->bn[f.scope];
  Tensor& mm = c->params[f.scope + "/BatchNorm/moving_mean"];
  Tensor& mv = c->params[f.scope + "/BatchNorm/moving_variance"];
  HIP_TRY(bn_batch_stats(f.r, bf(c), N, f.L->cout, kBnEps, 0.9f, s.mean, s.rstd, mm.d, mv.d, t->red, c->stream));   // main.py:129,557
  const float *ga = find(c, f.scope + "/BatchNorm/gamma")->d, *be = find(c, f.scope + "/BatchNorm/beta")->d;
  if (pool_out && bn_apply_pool(f.r, s.mean, s.rstd, ga, be, f.y, pool_out, bf(c), B, f.H, f.W, f.L->cout, c->stream)) return hipGetLastError() == hipSuccess ? JCM_OK : fail(JCM_ERR_HIP, "bn_apply_pool");
  HIP_TRY(bn_apply(f.r, s.mean, s.rstd, ga, be, f.y, bf(c), N, f.L->cout, c->stream));
  if (pool_out) HIP_TRY(max_pool_2x2(f.y, pool_out, bf(c), B, f.H, f.W, f.L->cout, c->stream));
  return JCM_OK;
}

// one layer of the step's forward pass: the two halves
int conv_train_fwd(jcm_ctx* c, LayerFwd& f, int stride, const void* x, int B, int Hin, int Win, int sub, void* pool_out = nullptr) {
  JCM_TRY(conv_train_fwd_conv(c, f, stride, x, B, Hin, Win, sub));
  return conv_train_fwd_bn(c, f, B, pool_out);
}

// ---- backward of one BN(relu(conv+b)) layer given dy (scaled by dy_scale): fills the parameter
// gradients, returns dz (arena) for the caller to push through wgrad / dgrad.
// pooled: the layer's output y went through the 2x2/2 max pool and dy is the POOLED gradient: the pool's backward pass is formed inside the BatchNorm backward
// kernels where that form exists (bn_bwd_pooled); otherwise max_pool_bwd writes it to a [B, H, W, C] tensor and the plain kernels run
// dz_dst (optional): dz is written there instead of the arena (jcm_train_bn_bwd: the caller's tensor)
int conv_train_bwd_pre(jcm_ctx* c, const LayerFwd& f, const void* dy, float dy_scale, bool pooled, int B, float* grads, void** dz_out, void* dz_dst = nullptr) {
  TrainState* t = c->train;
  const size_t N = (size_t)B * f.H * f.W;
  const int C = f.L->cout;
  void* dy_full = pooled ? act(c, N * C) : nullptr;
  void* dz = dz_dst ? dz_dst : act(c, N * C);
  *dz_out = dz;
  if (c->dry) return JCM_OK;
  const BnSave& s = t->bn[f.scope];
  float* sums = t->small;   // [2C] <= 1024 floats
  const float* ga = find(c, f.scope + "/BatchNorm/gamma")->d;
  float *dga = grad_of(t, grads, f.scope + "/BatchNorm/gamma"), *dbe = grad_of(t, grads, f.scope + "/BatchNorm/beta"), *db = grad_of(t, grads, f.scope + "/biases");
  if (pooled) {
    hipError_t e = hipSuccess;
    if (bn_bwd_pooled(dy, f.y, f.r, bf(c), s.mean, s.rstd, ga, B, f.H, f.W, C, sums, dga, dbe, dz, db, t->red, c->stream, &e)) {
      HIP_TRY(e);
      return JCM_OK;
    }
    HIP_TRY(max_pool_bwd(f.y, dy, dy_full, bf(c), B, f.H, f.W, C, c->stream));
    dy = dy_full;
  }
  HIP_TRY(bn_bwd_reduce(dy, dy_scale, f.r, bf(c), s.mean, s.rstd, N, C, sums, dga, dbe, t->red, c->stream));
  // (the bias gradient = the column sums of dz: taken while dz is written)
  HIP_TRY(bn_bwd_apply_colsum(dy, dy_scale, f.r, bf(c), s.mean, s.rstd, ga, sums, N, C, 1, dz, db, t->red, c->stream));
  return JCM_OK;
}

// A layer's dz as its two gradient kernels read it: ld = its channel stride; ld_fft = the stride when it differs from the packed data-gradient weights'
// (the logits gradient widened to 64 channels for the frequency-domain route; 0 = DgradW::cinp)
struct Dz {
  const void* p = nullptr;
  int ld = 0, ld_fft = 0;
};
// What a layer's weight gradient leaves for the data gradient of the SAME dz that follows it (layer_grads is the only place that carries one across)
struct DzHandover {
  void* zs = nullptr;          // whole-map frequency route: the split spectra of dz (arena, behind the weight gradient's mark) ...
  float* zs_tmax = nullptr;    // ... the words of their fp16 scaling ...
  int zs_ld = 0;               // ... and the channel stride they were taken with
  bool gscale_set = false;     // split route: TrainState::gscale holds the power-of-two scale of this dz
};

// The weight gradient in the frequency domain (wgrad_fft.hip): spectra of dz, P[f] = conj(X)^T dZ per frequency against the input spectra the forward pass
// kept, k x k taps.  The transform runs on n images of th x tw:
//   win == nullptr: the B maps themselves.  The spectra of dz stay allocated (before the mark) and are handed to `ho`: conv_dgrad of this layer reads them.
//   win: its windows, as the forward pass cut them, but VALID-ONLY (zero halo: every output pixel counts once; in window coordinates the correlation with the
//        forward pass's windows is alias-free for |lag| <= 4).  Everything is released with the mark.
// *taken = false, and nothing done, where the transform has no geometry for the layer.
int wgrad_freq(jcm_ctx* c, const LayerFwd& f, const void* dz, int ldz, int n, int th, int tw, const WinGeom* win, float lmbd, float* grads, DzHandover* ho, bool* taken) {
  const ConvLayer* L = f.L;
  const int np = fft_np(c), circ = win ? 1 : 0;
  int NY = 0, NX = 0, MTx = 0, MTz = 0, ny2 = 0, nx2 = 0;
  *taken = conv_fft_geometry(th, tw, L->ks, n, L->cout, np, &NY, &NX, &MTx, circ) && conv_fft_geometry(th, tw, L->ks, n, L->cin, np, &ny2, &nx2, &MTz, circ);
  if (!*taken) return JCM_OK;
  size_t mark = c->arena_off;
  FftArgs az{};
  az.x = dz; az.B = n; az.H = th; az.W = tw; az.Cin = ldz; az.Cout = L->cin; az.circ = circ;
  bool gw = true;
  float* zw = nullptr;
  if (win) {
    zw = win_buffer(c, *win, ldz, &gw);
    az.x = zw;
    if (gw) { az.win_map = dz; az.win = *win; az.win_valid_only = 1; }
  }
  char* zs = arena_alloc<char>(c, conv_fft_xs_bytes(az, L->ks, np));
  if (!win) mark = c->arena_off;      // zs stays allocated
  char* work = arena_alloc<char>(c, conv_fft_workspace_bytes(az, L->ks, np));
  char* P = arena_alloc<char>(c, wgrad_fft_scratch_bytes(NY, NX, L->cin, ldz));
  if (!c->dry) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    JCM_TRY(prof_begin(c, &e0, &e1));
    float* ztmax = nullptr;
    if (np == 4) JCM_TRY(fft_new_words(c, n, &ztmax));
    hipError_t le = gw ? hipSuccess : win_gather(c, *win, dz, zw, ldz, 1);
    const char* why = nullptr;
    if (le == hipSuccess) le = conv_fft_spectra(az, L->ks, np, work, zs, c->stream, ztmax, 1, &why);
    if (le == hipSuccess)
      le = wgrad_fft(f.xs, zs, P, L->w_raw, lmbd, grad_of(c->train, grads, f.scope + "/weights"), L->ks, NY, NX, n, MTx, MTz, L->cin, ldz, L->cout, c->stream,
                     np, f.xs_tmax, ztmax, th);
    prof_end(c, "wgrad:" + f.scope, e0, e1, le == hipSuccess);
    if (le != hipSuccess) return fail(JCM_ERR_HIP, std::string("frequency-domain weight gradient ") + (win ? "(windows) " : "") + "of '" + f.scope + "': " + (why ? why : hipGetErrorString(le)));
    if (!win) { ho->zs = zs; ho->zs_tmax = ztmax; ho->zs_ld = ldz; }
  }
  c->arena_off = mark;
  notify_ready(c, f.scope + "/");
  return JCM_OK;
}

// dW (+ lmbd*W) of a stride-1 layer: x = layer input [B,H,W,Cin], dz [B,H,W,ldz]
int conv_wgrad(jcm_ctx* c, const LayerFwd& f, const void* dz, int ldz, int B, float lmbd, float* grads, DzHandover* ho) {
  TrainState* t = c->train;
  const ConvLayer* L = f.L;
  if (f.xs && !bf(c) && ldz >= L->cout && ldz % 64 == 0) {      // frequency domain, like the forward pass that kept the input spectra
    bool taken = false;
    if (f.win.TY) {
      JCM_TRY(wgrad_freq(c, f, dz, ldz, f.win.BW(), kWin, kWin, &f.win, lmbd, grads, ho, &taken));
      return taken ? JCM_OK : fail(JCM_ERR_STATE, "window geometry of '" + f.scope + "'");
    }
    ConvLayer Lz;      // dz as the input of a frequency-domain layer: the same pseudo-layer conv_dgrad runs
    Lz.ks = L->ks; Lz.cin = ldz; Lz.cout = L->cin; Lz.has_bn = false; Lz.w_raw = t->scratch_flip;
    if (takes_fft(c, &Lz, B, f.H, f.W)) JCM_TRY(wgrad_freq(c, f, dz, ldz, B, f.H, f.W, nullptr, lmbd, grads, ho, &taken));
    if (taken) return JCM_OK;
  }
  const size_t n = (size_t)L->ks * L->ks * L->cin * L->cout;
  const int splits = wgrad_splits(L->ks, L->cin, L->cout, B, f.H);
  const size_t mark = c->arena_off;
  float* partial = arena_alloc<float>(c, n * splits);
  // handles with f32_conv = 2: the fp16x3 split kernel on pre-split operands (wgrad_split.hip); dz is lifted into the fp16 range by its own power-of-two scale
  const bool h16 = !bf(c) && c->f32_conv == 2 && wgrad_split_supported(L->ks, L->cin, ldz);
  if (bf(c) && !wgrad_split_supported(L->ks, L->cin, ldz)) return fail(JCM_ERR_ARG, "no bf16 weight-gradient kernel for layer '" + f.scope + "'");
  const size_t nx = (size_t)B * f.H * f.W * L->cin, nz = (size_t)B * f.H * f.W * ldz;
  char* xparts = h16 ? arena_alloc<char>(c, nx * 4) : nullptr;
  char* zparts = h16 ? arena_alloc<char>(c, nz * 4) : nullptr;
  if (!c->dry) {
    if (h16) {
      // the scale computed here is reused by conv_dgrad of the same layer
      HIP_TRY(pow2_scale_of(static_cast<const float*>(dz), nz, t->gscale, t->gscratch, c->stream));
      ho->gscale_set = true;
      HIP_TRY(split_parts16(static_cast<const float*>(f.in), xparts, nx, nullptr, c->stream));
      HIP_TRY(split_parts16(static_cast<const float*>(dz), zparts, nz, t->gscale, c->stream));
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    JCM_TRY(prof_begin(c, &e0, &e1));
    hipError_t le;
    if (bf(c)) le = wgrad_bf16(f.in, dz, partial, splits, L->ks, B, f.H, f.W, L->cin, L->cout, ldz, c->stream);
    else if (h16) le = wgrad_split16(xparts, zparts, partial, splits, L->ks, B, f.H, f.W, L->cin, L->cout, ldz, c->stream);
    else le = wgrad_f32(static_cast<const float*>(f.in), static_cast<const float*>(dz), partial, splits, L->ks, B, f.H, f.W, L->cin, L->cout, ldz, c->stream);
    prof_end(c, "wgrad:" + f.scope, e0, e1, le == hipSuccess);      // read with jcm_profile_read("wgrad:<scope>")
    if (le != hipSuccess) return fail(JCM_ERR_HIP, "weight-gradient launch of '" + f.scope + "': " + hipGetErrorString(le));
    HIP_TRY(wgrad_reduce(partial, splits, n, L->w_raw, lmbd, grad_of(t, grads, f.scope + "/weights"), c->stream, h16 ? t->gscale + 1 : nullptr));
  }
  c->arena_off = mark;
  notify_ready(c, f.scope + "/");      // weights were the layer's last gradient (BatchNorm and bias gradients precede them)
  return JCM_OK;
}

// dX = conv_SAME(dZ, flipped weights): z.p [B,H,W,ldz] -> dx [B,H,W,Cin]; ho: what conv_wgrad of this layer left for this dz
int conv_dgrad(jcm_ctx* c, const LayerFwd& f, const Dz& z, int B, void* dx, const DzHandover& ho) {
  TrainState* t = c->train;
  const DgradW& d = t->dgrad[f.scope];
  const ConvLayer* L = f.L;
  if (!bf(c)) {
    const int cin_fft = z.ld_fft ? z.ld_fft : d.cinp;
    // fp32 handles: the data gradient is a SAME correlation with the flipped, transposed filter -- in the frequency domain like the forward
    // pass (conv_fft.hip); its filter spectra ("dgrad:<scope>") are packed from the flipped weights after every update, on first use.
    ConvLayer Ld;
    Ld.ks = L->ks; Ld.cin = cin_fft; Ld.cout = L->cin; Ld.has_bn = false;
    Ld.w_raw = t->scratch_flip; Ld.bias = t->zeros; Ld.scale = t->ones; Ld.shift = t->zeros;
    const bool win = f.win.TY > 0;
    if (win || takes_fft(c, &Ld, B, f.H, f.W)) {
      const std::string key = "dgrad:" + f.scope;
      if ((size_t)L->ks * L->ks * cin_fft * L->cin > t->scratch_flip_n) return fail(JCM_ERR_STATE, "flipped filter of '" + f.scope + "' does not fit its buffer");
      if (!c->dry && !fft_spectra_valid(c, key, win ? kWin : f.H, win ? kWin : f.W, win))
        HIP_TRY(flip_transpose_weights(L->w_raw, t->scratch_flip, L->ks, L->cin, L->cout, cin_fft, c->stream));
      // windows WITH their halo of real gradient pixels -> the flipped, transposed filter's layer on the 32 x 32 transform -> scatter
      if (win) return run_conv_windows(c, &Ld, key, f.win, z.p, dx);
      FftLink k;
      if (!c->dry && ho.zs && ho.zs_ld == cin_fft) { k.xs = ho.zs; k.xs_ready = true; k.tmax_in = ho.zs_tmax; }      // the spectra of dz are there (conv_wgrad just made them)
      ConvCall q = conv_call(z.p, dx, B, f.H, f.W);
      q.link = &k;
      return run_conv_fft(c, &Ld, key, q);
    }
    if (z.ld_fft) return fail(JCM_ERR_STATE, "data gradient of '" + f.scope + "': widened dz without the frequency-domain route");
  }
  if (c->dry) return JCM_OK;
  JCM_TRY(ensure_dgrad_packed(c, f.scope));
  ConvArgs a = conv_args(L, B, f.H, f.W);      // the layer turned round: Cout = its Cin, Cin = dz's stride in the packed filter
  a.x = z.p; a.bias = t->zeros; a.scale = t->ones; a.shift = t->zeros; a.out = dx; a.Cout = L->cin;
  if (bf(c)) {      // bf16 gradients through the bf16 forward kernels on flipped weights
    a.wp = d.wd_bf16; a.Cin = d.cinp_bf16; a.CoutP = d.coutp_bf16;
    HIP_TRY(conv_igemm_bf16(a, L->ks, false, c->stream));
    return JCM_OK;
  }
  a.wp = d.wd; a.Cin = d.cinp; a.CoutP = d.coutp;
  const bool split = d.wd_split && conv_split_supported(L->ks, d.cinp, L->cin, B, f.H, f.W, c->split_min_wgs);
  const int ns = 2;      // fp16 parts (f32_conv = 2)
  if (split) {
    a.wp = d.wd_split; a.CoutP = L->cin;
    // normally this layer's conv_wgrad has left dz's scale; not where the split data-gradient kernel takes a shape the split weight-gradient kernel does not
    if (!ho.gscale_set) HIP_TRY(pow2_scale_of(static_cast<const float*>(z.p), (size_t)B * f.H * f.W * d.cinp, t->gscale, t->gscratch, c->stream));
    a.in_scale = t->gscale;
    a.w_scale = L->wscale;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  JCM_TRY(prof_begin(c, &e0, &e1));
  const hipError_t le = split ? conv_split_f32(a, L->ks, ns, c->stream) : conv_igemm_f32(a, L->ks, c->stream);
  prof_end(c, "dgrad:" + f.scope, e0, e1, le == hipSuccess);
  if (le != hipSuccess) return fail(JCM_ERR_HIP, "data-gradient launch of '" + f.scope + "': " + hipGetErrorString(le));
  return JCM_OK;
}

// Weight gradient, then data gradient, of layer f.  dx: null = no data gradient; *dx null = [B, H, W, Cin] allocated here, between the two (behind what the
// weight gradient leaves allocated).  The hand-over between the two lives only here, where dz and the arena behind it are untouched.
int layer_grads(jcm_ctx* c, const LayerFwd& f, const Dz& z, int B, float lmbd, float* grads, void** dx) {
  DzHandover ho;
  JCM_TRY(conv_wgrad(c, f, z.p, z.ld, B, lmbd, grads, &ho));
  if (!dx) return JCM_OK;
  if (!*dx) *dx = act(c, (size_t)B * f.H * f.W * f.L->cin);
  return conv_dgrad(c, f, z, B, *dx, ho);
}

__global__ void finish_losses_kernel(const float* __restrict__ ce_pd, const float* __restrict__ ce_sm, int n, const double* __restrict__ wsq,
                                     float lmbd, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0, b = 0.0;
  for (int i = 0; i < n; ++i) { a += ce_pd[i]; b += ce_sm[i]; }
  a /= n; b /= n;
  const double l2 = 0.5 * *wsq;
  out[0] = (float)(a + b + (double)lmbd * l2);   // loss_tower (main.py:540)
  out[1] = (float)a;                             // loss_pd
  out[2] = (float)b;                             // loss_sm
  out[3] = (float)l2;                            // weight_decay('weights')
}

int sm_train_impl(jcm_ctx* c, const float* pd_prob, const float* y, int B, float gscale, float* ce_sm, float* dlogits, float* grads);

// The logits gradient travels as fp32 with a 16-channel stride (d16, N pixels).  What the logits layer's gradient kernels read of it: bf16 handles, 32-channel
// bf16 chunks; fp32 handles on the frequency-domain route (the layer kept its input spectra: `freq`), 64-channel blocks for the forward transforms; otherwise d16 itself
int widen_logits_grad(jcm_ctx* c, const float* d16, size_t N, bool freq, Dz* z) {
  constexpr int LDZ = 16, LDZB = 32, LDZF = 64;
  *z = Dz{d16, LDZ, 0};
  if (bf(c)) {
    void* db = act(c, N * LDZB);
    if (!c->dry) HIP_TRY(cast_pad_bf16(d16, LDZ, db, LDZB, N, c->stream));
    *z = Dz{db, LDZB, 0};
  } else if (freq) {
    float* df = arena_alloc<float>(c, N * LDZF);
    if (!c->dry) HIP_TRY(pad_channels_f32(d16, LDZ, df, LDZF, N, c->stream));
    *z = Dz{df, LDZF, LDZF};
  }
  return JCM_OK;
}

// forward + backward of one tower (main.py:522-541,559-560)
int loss_grads_impl(jcm_ctx* c, const float* x, const float* y, int B, int H, int W, int use_sm, float lmbd, float* grads, float* losses) {
  TrainState* t = c->train;
  static const char* const kRes[3] = {"fullres", "halfres", "quarterres"};
  const int K = c->K;
  LayerFwd l[3][4], l5, l6;      // l[r][i]: conv<i+1>_<res r>
  const bool b16 = bf(c);
  for (int r = 0; r < 3; ++r) {
    const int sub = 1 << r;
    if (H % sub || W % sub) return fail(JCM_ERR_ARG, "training needs image sizes divisible by 4");
    const std::string res = kRes[r];
    for (int i = 0; i < 4; ++i) l[r][i].scope = "conv" + std::to_string(i + 1) + "_" + res;
    // (the pools behind conv1 and conv2 are taken by the layers' BatchNorm kernels: conv_train_fwd's pool_out)
    const ConvLayer* L1c = conv_of(c, l[r][0].scope);
    const ConvLayer* L2c = conv_of(c, l[r][1].scope);
    if (!L1c || !L2c) return fail(JCM_ERR_STATE, "part-detector parameters incomplete (" + res + ")");
    const int C1 = L1c->cout, C2 = L2c->cout;
    const int hc1 = cdiv2(H / sub), wc1 = cdiv2(W / sub);      // conv1's output map (stride 2, SAME)
    const int h2 = cdiv2(hc1), w2 = cdiv2(wc1);
    void* p1 = act(c, (size_t)B * h2 * w2 * C1);
    JCM_TRY(conv_train_fwd(c, l[r][0], 2, x, B, H, W, sub, p1));                                // main.py:44-45,52-53,61-62
    if (!c->dry && (l[r][0].H != hc1 || l[r][0].W != wc1)) return fail(JCM_ERR_STATE, "conv1's map is not the size its pool buffer was made for");
    const int h3 = cdiv2(h2), w3 = cdiv2(w2);
    void* p2 = act(c, (size_t)B * h3 * w3 * C2);
    JCM_TRY(conv_train_fwd(c, l[r][1], 1, p1, B, h2, w2, 1, p2));                               // :46-47,54-55,63-64
    JCM_TRY(conv_train_fwd(c, l[r][2], 1, p2, B, h3, w3, 1));                                   // :48,56,65
    JCM_TRY(conv_train_fwd(c, l[r][3], 1, l[r][2].y, B, h3, w3, 1));                            // :49,57,66
  }
  const int hh = l[0][3].H, ww = l[0][3].W, C4 = l[0][3].L->cout;
  const size_t NP = (size_t)B * hh * ww;
  void* merged = act(c, NP * C4);
  if (!c->dry)
    HIP_TRY(upsample_merge3(l[0][3].y, l[1][3].y, l[1][3].H, l[1][3].W, l[2][3].y, l[2][3].H, l[2][3].W, merged, b16, B, hh, ww, C4, c->stream));  // :58,67,69-70
  l5.scope = "conv5"; l6.scope = "conv6";
  JCM_TRY(conv_train_fwd(c, l5, 1, merged, B, hh, ww, 1));                                      // :71
  JCM_TRY(conv_train_fwd(c, l6, 1, l5.y, B, hh, ww, 1));                                        // :72 (no ReLU / BN)
  if (l6.L && (l6.L->has_bn || l6.L->cout != K)) return fail(JCM_ERR_STATE, "conv6 must be the K-channel logits layer");
  float* logits = static_cast<float*>(l6.r);

  // ---- losses and the gradient w.r.t. the part-detector logits, kept with a 16-channel stride
  constexpr int LDZ = 16;
  float* dlog = arena_alloc<float>(c, NP * LDZ);
  float* ce_pd = arena_alloc<float>(c, (size_t)B * K);
  float* ce_sm = arena_alloc<float>(c, (size_t)B * K);
  const float gscale = 1.0f / (float)(B * K);                                                  // reduce_mean over (image, joint), main.py:240
  if (!c->dry) {
    HIP_TRY(hipMemsetAsync(dlog, 0, NP * LDZ * sizeof(float), c->stream));
    // use_sm == 0: hm_pred_sm_logit is hm_pred_pd_logit (main.py:535), so the same term counts twice
    HIP_TRY(softmax_ce(logits, y, B, hh * ww, K, K + 1, use_sm ? gscale : 2.0f * gscale, ce_pd, dlog, LDZ, 0, c->stream));   // main.py:538
  }
  if (use_sm) {
    if (hh != kHmH || ww != kHmW || K + 1 != kC) return fail(JCM_ERR_ARG, "the spatial model is defined for 60x90 heat maps and 9 joints");
    float* prob = arena_alloc<float>(c, NP * K);
    if (!c->dry) HIP_TRY(spatial_softmax(logits, prob, B, hh * ww, K, c->stream));             // main.py:523
    JCM_TRY(sm_train_impl(c, prob, y, B, gscale, ce_sm, dlog, grads));                          // main.py:528-531,539 + backward
    notify_ready(c, "bias_");
    notify_ready(c, "bn_sm/");
    notify_ready(c, "energy_");
  } else if (!c->dry) {
    HIP_TRY(hipMemcpyAsync(ce_sm, ce_pd, (size_t)B * K * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  if (!c->dry) {
    // weight_decay('weights') (main.py:195-205): sum of l2_loss over the conv weights
    HIP_TRY(sum_squares_chunks(t->ck_w, t->ck_start, t->ck_len, t->ck_isw, t->n_chunks, t->sumsq + 1, t->red, c->stream));
    hipLaunchKernelGGL(finish_losses_kernel, dim3(1), dim3(64), 0, c->stream, ce_pd, ce_sm, B * K, t->sumsq + 1, lmbd, losses);
    HIP_TRY(hipGetLastError());
  }

  // ---- backward of the part detector
  // conv6: z = conv(y5) + b
  if (!c->dry) {
    HIP_TRY(col_sum(dlog, false, NP, LDZ, t->small, t->red, c->stream));
    HIP_TRY(hipMemcpyAsync(grad_of(t, grads, "conv6/biases"), t->small, K * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  Dz dl;
  JCM_TRY(widen_logits_grad(c, dlog, NP, l6.xs != nullptr, &dl));
  void *dy5 = nullptr, *dz5 = nullptr;
  JCM_TRY(layer_grads(c, l6, dl, B, lmbd, grads, &dy5));
  JCM_TRY(conv_train_bwd_pre(c, l5, dy5, 1.0f, false, B, grads, &dz5));
  void* dmerged = l5.L->cin == l5.L->cout ? dy5 : nullptr;      // dy5 is dead once dz5 exists; same size when C4 == C5
  JCM_TRY(layer_grads(c, l5, Dz{dz5, l5.L->cout, 0}, B, lmbd, grads, &dmerged));
  for (int r = 0; r < 3; ++r) {
    const size_t mark = c->arena_off;
    // merge: x = (x1 + up(x2) + up(x3)) / 3
    const void* dy = dmerged;
    float sc = 1.0f / 3.0f;
    if (l[r][3].H != hh || l[r][3].W != ww) {
      void* d = act(c, (size_t)B * l[r][3].H * l[r][3].W * C4);
      if (!c->dry) HIP_TRY(resize_bilinear_bwd(dmerged, d, b16, B, l[r][3].H, l[r][3].W, hh, ww, C4, 1.0f / 3.0f, c->stream));
      dy = d;
      sc = 1.0f;
    }
    void* dz = nullptr;
    for (int i = 3; i >= 1; --i) {      // conv4, conv3, conv2; what reaches conv2 and conv1 is the gradient of their POOLED output (pool2, pool1)
      const LayerFwd& f = l[r][i];
      JCM_TRY(conv_train_bwd_pre(c, f, dy, sc, i == 1, B, grads, &dz));
      void* dx = nullptr;
      JCM_TRY(layer_grads(c, f, Dz{dz, f.L->cout, 0}, B, lmbd, grads, &dx));
      dy = dx;
      sc = 1.0f;
    }
    const LayerFwd& f1 = l[r][0];
    JCM_TRY(conv_train_bwd_pre(c, f1, dy, 1.0f, true, B, grads, &dz));
    const int C1 = f1.L->cout;
    const size_t n = (size_t)25 * 3 * C1;
    const int nb = wgrad_conv1_blocks();
    float* partial = arena_alloc<float>(c, n * nb);
    if (!c->dry) {
      HIP_TRY(wgrad_conv1(x, dz, b16, partial, B, H, W, 1 << r, C1, c->stream));
      HIP_TRY(wgrad_reduce_wide(partial, nb, n, f1.L->w_raw, lmbd, grad_of(t, grads, f1.scope + "/weights"), c->stream));
    }
    notify_ready(c, f1.scope + "/");
    c->arena_off = mark;
  }
  return JCM_OK;
}

// spatial model in training mode + its backward (main.py:528-531,539).  pd_prob [B,5400,K]; y [B,5400,K+1];
// adds d loss_sm / d pd_logits into dlog [B,5400,16] and fills the bn_sm / energy / bias gradients.
int sm_train_impl(jcm_ctx* c, const float* pd_prob, const float* y, int B, float gscale, float* ce_sm, float* dlog, float* grads) {
  TrainState* t = c->train;
  const int K = c->K, P = K * (kC - 1);
  const size_t N = (size_t)B * kHmHW;
  float* hm10 = arena_alloc<float>(c, N * kC);
  float* sc = arena_alloc<float>(c, 16);
  float* sh = arena_alloc<float>(c, 16);
  float* frame = arena_alloc<float>(c, (size_t)B * kC * kFrame);      // s_c = sp(bn(h_c)) on zero frames: the backward's d log(s_j + d) term reads it
  float2* lhat = arena_alloc<float2>(c, (size_t)B * kC * kSpec);      // likelihood spectra, transposed [B][C][91][120] (sm_fused.hip), kept for dA
  float* tsave = arena_alloc<float>(c, (size_t)B * P * kHmHW);        // the argument of every pairwise log
  float* sml = arena_alloc<float>(c, N * K);
  float* G = arena_alloc<float>(c, N * K);
  float* dh = arena_alloc<float>(c, N * kC);
  float2* dA_hat = arena_alloc<float2>(c, (size_t)P * kSpec);
  float* dspb = arena_alloc<float>(c, (size_t)P * kHmHW);
  const int Bc = B < c->sm_chunk ? B : c->sm_chunk;
  const size_t mark = c->arena_off;
  BnSave* bs = c->dry ? nullptr : &t->bn["bn_sm"];
  // ---- forward: the fused kernels of the inference path (every transform in LDS), which also leave the log arguments
  if (!c->dry) {
    HIP_TRY(sm_concat_target(pd_prob, y, hm10, N, K, kC, c->stream));                                        // main.py:528
    HIP_TRY(bn_batch_stats(hm10, false, N, kC, kBnEps, 0.9f, bs->mean, bs->rstd, c->params["bn_sm/BatchNorm/moving_mean"].d,
                           c->params["bn_sm/BatchNorm/moving_variance"].d, t->red, c->stream));              // main.py:113
    HIP_TRY(bn_fold_stats(bs->mean, bs->rstd, find(c, "bn_sm/BatchNorm/gamma")->d, find(c, "bn_sm/BatchNorm/beta")->d, sc, sh, kC, c->stream));
    HIP_TRY(sm_pad_frame(hm10, kC, nullptr, sc, sh, frame, B, kC, c->stream));
    void* scr = nullptr;
    unsigned epoch = 0;
    JCM_TRY(sm_scratch_next(c, &scr, &epoch));
    HIP_TRY(sm_fused_forward(hm10, kC, nullptr, 0, sc, sh, c->prior_spec_t, c->cond, c->sp_bias, lhat, sml, B, K, kC, c->stream, tsave, scr, epoch));   // main.py:117-123
    HIP_TRY(softmax_ce(sml, y, B, kHmHW, K, K + 1, gscale, ce_sm, G, K, 0, c->stream));                      // main.py:539
  }
  // ---- backward (sm_train.hip; transforms: sm_lds.hip)
  {
    float2* Dhat = arena_alloc<float2>(c, (size_t)Bc * P * kSpec);
    float2* dLhat = arena_alloc<float2>(c, (size_t)Bc * kC * kSpec);
    float* dLframe = arena_alloc<float>(c, (size_t)Bc * kC * kFrame);      // rows 0..59 are written and read
    float* dAframe = arena_alloc<float>(c, (size_t)P * kFrame);
    float* dhm = arena_alloc<float>(c, N * kC);
    if (!c->dry) {
      for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = B - b0 < Bc ? B - b0 : Bc;
        const float* Gb = G + (size_t)b0 * kHmHW * K;
        const float* Tb = tsave + (size_t)b0 * P * kHmHW;
        HIP_TRY(sm_bwd_dbias(Gb, Tb, dspb, nb, K, P, b0 > 0, c->stream));
        HIP_TRY(sm_lds_fwd_dframes(Gb, Tb, Dhat, nb, K, P, c->stream));      // D_p = R^T (G_j / T_p) on the window, transformed as it is built
        HIP_TRY(sm_bwd_spec_da(Dhat, lhat + (size_t)b0 * kC * kSpec, c->cond, dA_hat, nb, kC, P, b0 > 0, c->stream));
        HIP_TRY(sm_bwd_spec_dl(Dhat, c->prior_spec_t, dLhat, nb, K, kC, c->stream));
        HIP_TRY(sm_lds_inv_frames(dLhat, dLframe, nb * kC, 0, kHmH, 1.0f, c->stream));
        HIP_TRY(sm_bwd_dh(dLframe, Gb, frame + (size_t)b0 * kC * kFrame, hm10 + (size_t)b0 * kHmHW * kC, sc, sh,
                          dh + (size_t)b0 * kHmHW * kC, nb, K, kC, c->stream));
      }
      HIP_TRY(sm_lds_inv_frames(dA_hat, dAframe, P, 0, kPrH, 1.0f, c->stream));
      HIP_TRY(sm_bwd_params(dAframe, dspb, t->e_ptr, t->b_ptr, t->e_off, t->b_off, grads, P, c->stream));
      float* sums = t->small;
      HIP_TRY(bn_bwd_reduce(dh, 1.0f, hm10, false, bs->mean, bs->rstd, N, kC, sums, grad_of(t, grads, "bn_sm/BatchNorm/gamma"),
                            grad_of(t, grads, "bn_sm/BatchNorm/beta"), t->red, c->stream));
      HIP_TRY(bn_bwd_apply(dh, 1.0f, hm10, false, bs->mean, bs->rstd, find(c, "bn_sm/BatchNorm/gamma")->d, sums, N, kC, 0, dhm, c->stream));
      HIP_TRY(softmax_bwd(pd_prob, dhm, B, kHmHW, K, kC, dlog, 16, c->stream));                                // through main.py:523
    }
  }
  c->arena_off = mark;
  return JCM_OK;
}

}  // namespace

extern "C" {

int jcm_train_loss_grads(jcm_handle h, const float* x, const float* y, int B, int H, int W, int use_sm, float lmbd, float* grads,
                         float* losses) {
  JCM_TRY(need_train(h));
  if (!x || !y || !grads || !losses || B < 1 || H < 8 || W < 8) return fail(JCM_ERR_ARG, "bad train_loss_grads arguments");
  if (use_sm && !h->has_sm) return fail(JCM_ERR_STATE, "use_sm needs the spatial-model parameters");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (h->call_depth > 1) return fail(JCM_ERR_STATE, "jcm_train_loss_grads changes the handle's training state or parameters and cannot be called from the gradient-ready callback of the same handle");
  jcm_ctx* c = h;
  HIP_TRY(hipMemsetAsync(grads, 0, c->train->total * sizeof(float), c->stream));   // tensors the loss does not reach keep a zero gradient
  return with_arena(c, [&] { return loss_grads_impl(c, x, y, B, H, W, use_sm, lmbd, grads, losses); });
}

// The two gradient kernels of ONE stride-1 layer on caller-supplied tensors -- the route the training step takes on this handle (frequency
// domain, direct fp32 MFMA chain, split operands), isolated from the rest of the step so that tests can hold the kernels themselves to a tight
// bound (inside a full step a ReLU / max-pool decision that rounds the other way upstream moves a gradient by far more than kernel error).
// On a bf16 handle x, dz and dx_out are bf16 (the step's tensors between the layers); grads stays fp32.
int jcm_train_layer_grads(jcm_handle h, const char* scope, const void* x, const void* dz, int B, int H, int W, float lmbd, float* grads, void* dx_out) {
  JCM_TRY(need_train(h));
  if (!scope || !x || !dz || !grads || B < 1 || H < 1 || W < 1) return fail(JCM_ERR_ARG, "bad train_layer_grads arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  TrainState* t = c->train;
  const ConvLayer* L = conv_of(c, scope);
  if (!L || L->cin == 3 || !grad_of(t, grads, std::string(scope) + "/weights")) return fail(JCM_ERR_ARG, std::string("train_layer_grads: '") + scope + "' is not a stride-1 conv layer");
  return with_arena(c, [&] {
    LayerFwd f;
    f.scope = scope;
    const size_t NPX = (size_t)B * H * W;
    Dz z{dz, L->cout, 0};
    void* dx = dx_out;
    if (bf(c)) {
      // bf16 handles take no frequency-domain gradient route: no forward pass needed.  Both kernels read dz with the 32-channel stride of the
      // packed data-gradient filter (the step's logits gradient: cast_pad_bf16 to 32 channels); a narrower dz is copied into zero padding
      f.L = L; f.in = x; f.H = H; f.W = W;
      const int ldb = t->dgrad[scope].cinp_bf16;
      if (ldb != L->cout) {
        void* dpad = act(c, NPX * ldb);
        if (!c->dry) {
          HIP_TRY(hipMemsetAsync(dpad, 0, NPX * ldb * 2, c->stream));
          HIP_TRY(hipMemcpy2DAsync(dpad, (size_t)ldb * 2, dz, (size_t)L->cout * 2, (size_t)L->cout * 2, NPX, hipMemcpyDeviceToDevice, c->stream));
        }
        z = Dz{dpad, ldb, 0};
      }
      return layer_grads(c, f, z, B, lmbd, grads, dx_out ? &dx : nullptr);
    }
    JCM_TRY(conv_train_fwd_conv(c, f, 1, x, B, H, W, 1));      // (the frequency-domain weight gradient reads the input spectra the forward pass keeps)
    if (L->cout % 16) {      // the logits layer: its gradient travels with a 16-channel stride, as in the step
      constexpr int LDZ = 16;
      float* d16 = arena_alloc<float>(c, NPX * LDZ);
      if (!c->dry) HIP_TRY(pad_channels_f32(static_cast<const float*>(dz), L->cout, d16, LDZ, NPX, c->stream));
      JCM_TRY(widen_logits_grad(c, d16, NPX, f.xs != nullptr, &z));
    }
    return layer_grads(c, f, z, B, lmbd, grads, dx_out ? &dx : nullptr);
  });
}

// ---- the stages between the convolutions on caller-supplied tensors: each entry runs the host function the step runs (conv_train_fwd_bn,
// conv_train_bwd_pre, resize_bilinear_bwd, softmax_ce, softmax_bwd), so that tests can hold every kernel variant behind it to float64 at channel
// counts and map sizes the step itself never sees.  A stage that has no kernel for the request is refused here, with the reason.
static int bn_stage_layer(jcm_ctx* c, const char* who, const char* scope, int B, int H, int W, bool pool, LayerFwd* f) {
  const ConvLayer* L = scope ? conv_of(c, scope) : nullptr;
  if (!L || !L->has_bn) return fail(JCM_ERR_ARG, std::string(who) + ": '" + (scope ? scope : "") + "' is not a conv layer with BatchNorm");
  if (B < 1 || H < 1 || W < 1) return fail(JCM_ERR_ARG, std::string(who) + ": B, H and W must be positive");
  if (pool && L->cout % 4)
    return fail(JCM_ERR_ARG, std::string(who) + ": no 2x2 pool kernel for " + std::to_string(L->cout) + " channels (the pool kernels take four channels per thread: C % 4 == 0)");
  f->scope = scope; f->L = L; f->H = H; f->W = W;
  return JCM_OK;
}

int jcm_train_bn_fwd(jcm_handle h, const char* scope, const void* r, int B, int H, int W, void* y_out, void* pool_out, float* mean_out, float* rstd_out) {
  JCM_TRY(need_train(h));
  if (!r || !y_out) return fail(JCM_ERR_ARG, "bad train_bn_fwd arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (h->call_depth > 1) return fail(JCM_ERR_STATE, "jcm_train_bn_fwd changes the handle's training state or parameters and cannot be called from the gradient-ready callback of the same handle");
  jcm_ctx* c = h;
  LayerFwd f;
  JCM_TRY(bn_stage_layer(c, "train_bn_fwd", scope, B, H, W, pool_out != nullptr, &f));
  f.r = const_cast<void*>(r);
  JCM_TRY(with_arena(c, [&] { return conv_train_fwd_bn(c, f, B, pool_out, y_out); }));
  const BnSave& s = c->train->bn[f.scope];
  const size_t nb = (size_t)f.L->cout * sizeof(float);
  if (mean_out) HIP_TRY(hipMemcpyAsync(mean_out, s.mean, nb, hipMemcpyDeviceToDevice, c->stream));
  if (rstd_out) HIP_TRY(hipMemcpyAsync(rstd_out, s.rstd, nb, hipMemcpyDeviceToDevice, c->stream));
  return JCM_OK;
}

int jcm_train_bn_bwd(jcm_handle h, const char* scope, const void* dy, float dy_scale, int pooled, const void* r, const void* y, const float* mean, const float* rstd,
                     int B, int H, int W, float* grads, void* dz_out) {
  JCM_TRY(need_train(h));
  if (!dy || !r || !grads || !dz_out || (pooled && !y)) return fail(JCM_ERR_ARG, "bad train_bn_bwd arguments (the pooled form reads y)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (h->call_depth > 1) return fail(JCM_ERR_STATE, "jcm_train_bn_bwd changes the handle's training state or parameters and cannot be called from the gradient-ready callback of the same handle");
  jcm_ctx* c = h;
  LayerFwd f;
  JCM_TRY(bn_stage_layer(c, "train_bn_bwd", scope, B, H, W, pooled != 0, &f));
  if (pooled && dy_scale != 1.0f) return fail(JCM_ERR_ARG, "train_bn_bwd: the pooled form takes dy_scale = 1 (bn_bwd_pooled has no scale)");
  f.r = const_cast<void*>(r);
  f.y = const_cast<void*>(y);
  const BnSave& s = c->train->bn[f.scope];
  const size_t nb = (size_t)f.L->cout * sizeof(float);
  if (mean) HIP_TRY(hipMemcpyAsync(s.mean, mean, nb, hipMemcpyDeviceToDevice, c->stream));
  if (rstd) HIP_TRY(hipMemcpyAsync(s.rstd, rstd, nb, hipMemcpyDeviceToDevice, c->stream));
  void* dz = nullptr;
  return with_arena(c, [&] { return conv_train_bwd_pre(c, f, dy, dy_scale, pooled != 0, B, grads, &dz, dz_out); });
}

int jcm_train_resize_bwd(jcm_handle h, const void* dy, int B, int sh, int sw, int H, int W, int C, float scale, void* dx_out) {
  JCM_TRY(need_train(h));
  if (!dy || !dx_out || B < 1 || sh < 1 || sw < 1 || H < 1 || W < 1 || C < 1) return fail(JCM_ERR_ARG, "bad train_resize_bwd arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(resize_bilinear_bwd(dy, dx_out, bf(h), B, sh, sw, H, W, C, scale, h->stream));
  return JCM_OK;
}

int jcm_train_softmax_ce(jcm_handle h, const float* logits, const float* target, int B, int HW, int K, int Kt, float gscale, float* loss, float* dz, int ldz,
                         int accumulate) {
  JCM_TRY(need_train(h));
  if (!logits || !target || !loss || B < 1 || HW < 1 || K < 1 || Kt < K || (dz && ldz < K)) return fail(JCM_ERR_ARG, "bad train_softmax_ce arguments (Kt >= K, ldz >= K)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(softmax_ce(logits, target, B, HW, K, Kt, gscale, loss, dz, ldz, accumulate, h->stream));
  return JCM_OK;
}

int jcm_train_softmax_bwd(jcm_handle h, const float* p, const float* g, int B, int HW, int K, int ldg, float* dz, int ldz) {
  JCM_TRY(need_train(h));
  if (!p || !g || !dz || B < 1 || HW < 1 || K < 1 || ldg < K || ldz < K) return fail(JCM_ERR_ARG, "bad train_softmax_bwd arguments (ldg >= K, ldz >= K)");
  DeviceGuard guard(h->device);
  CallOrder order(h);
  HIP_TRY(softmax_bwd(p, g, B, HW, K, ldg, dz, ldz, h->stream));
  return JCM_OK;
}

// The spatial model's training stage on caller tensors: sm_train_impl, the host function the step calls behind spatial_softmax -- forward in training
// mode (bn_sm's batch statistics, its moving statistics advance), the cross-entropies, and the backward pass in slices of "sm_chunk" images -- so that
// tests can hold it to float64 by itself, at batches and slice widths no whole step of the suite reaches.
int jcm_train_sm_grads(jcm_handle h, const float* pd_prob, const float* y, int B, float gscale, float* ce_out, float* dlog, float* grads) {
  JCM_TRY(need_train(h));
  if (!pd_prob || !y || !ce_out || !dlog || !grads || B < 1) return fail(JCM_ERR_ARG, "bad train_sm_grads arguments (no null pointers, B >= 1)");
  if (!h->has_sm) return fail(JCM_ERR_STATE, "train_sm_grads needs the spatial-model parameters (bn_sm, energy_*, bias_*)");
  if (h->K + 1 != kC) return fail(JCM_ERR_ARG, "train_sm_grads: the spatial model's training stage is defined for 9 joints (n_joints = " + std::to_string(h->K) + ")");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (h->call_depth > 1) return fail(JCM_ERR_STATE, "jcm_train_sm_grads changes the handle's training state or parameters and cannot be called from the gradient-ready callback of the same handle");
  jcm_ctx* c = h;
  return with_arena(c, [&] { return sm_train_impl(c, pd_prob, y, B, gscale, ce_out, dlog, grads); });
}

}  // extern "C"
