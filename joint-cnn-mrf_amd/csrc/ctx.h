// Internal context of libjcm shared by the translation units behind include/jcm.h
// (jcm_api.hip: handle, parameter store, options, layer and tower entry points, call order, arena; entry.h: the launch scaffold of the entry points beside their kernels; conv_route.hip: how one conv layer runs; derived.hip: weight packings; pd_tower.hip: inference graph;
// jcm_train.hip: training step; train_state.hip: training state, optimizer and its entry points, both on train.h).  Not part of the ABI.
#pragma once
#include "../../include/jcm.h"

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"

namespace jcm {

struct CallOrder;

int fail(int code, const std::string& msg);     // sets the thread-local message of jcm_last_error()

#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return ::jcm::fail(JCM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));               \
  } while (0)
#define JCM_TRY(expr)          \
  do {                         \
    int r_ = (expr);           \
    if (r_ != JCM_OK) return r_; \
  } while (0)
// main.py:18 -- channel order of the heat maps and of the pair tables.
extern const char* const kJointNames[10];
constexpr int kC = 10;            // heat-map channels seen by the spatial model (9 joints + torso)
constexpr float kBnEps = 1e-3f;   // tf.contrib.layers.batch_norm default epsilon
constexpr int kHmH = 60, kHmW = 90, kHmHW = kHmH * kHmW;
constexpr int kPrH = 120, kPrW = 180;
constexpr int kCH = 61, kCW = 91;
constexpr size_t kFrame = (size_t)kPrH * kPrW;          // 120*180 real
constexpr size_t kSpec = (size_t)kPrH * (kPrW / 2 + 1); // 120*91 complex

struct Tensor {
  std::vector<int64_t> shape;
  float* d = nullptr;
  size_t n = 0;
};

struct ConvLayer {
  int ks = 0, cin = 0, cout = 0, coutp = 0;
  bool has_bn = false;
  const float* w_raw = nullptr;   // HWIO (conv1 kernel reads it directly)
  float* wp = nullptr;            // packed for conv_igemm_f32
  mutable bool wp_stale = false;  // a refresh after a weight update left `wp` behind: repacked where a direct fp32 kernel next reads it (run_conv_layer)
  void* wp_split = nullptr;       // two fp16 parts per weight for conv_split_f32 (fp32 handles, "f32_conv" = 2)
  int coutp_split = 0;
  float* wscale = nullptr;        // fp16x3: device {Sw, 1/Sw}, the power-of-two scale the packed weights carry
  void* wp_bf16 = nullptr;        // packed for conv_igemm_bf16
  void* wp_kxfold = nullptr;      // logits layer packed for conv_kxfold_bf16 (bf16 handles, Cout == 9)
  void* wq1_bf16 = nullptr;       // packed for conv1_mfma_pool (5x5, Cin=3, Cout=64)
  float* wq1_f32 = nullptr;       // packed for conv1_mfma_pool_f32 (fp32 handles)
  void* wq1_split = nullptr;      // packed for conv1_mfma_pool_split (fp32 handles, default route)
  int coutp_bf16 = 0;
  bool thin = false;              // fp32: conv_thin_f32 instead of conv_igemm_f32
  bool thin_bf16 = false;         // bf16: conv_thin_bf16 (fp32 output) instead of conv_igemm_bf16
  const float* bias = nullptr;
  float* scale = nullptr;
  float* shift = nullptr;
};

struct TrainState;   // train.h
}  // namespace jcm
struct jcm_ctx;
namespace jcm {
// ---- train_state.hip: what the other files need of the training state ----
void train_destroy(jcm_ctx* c);
void dgrad_filters_stale(jcm_ctx* c);      // the weights changed (jcm_train_apply, jcm_update_tensor): the packed data-gradient filters are repacked on next use
// summary.hip's view: the stored trainable tensor that holds [off, off + n) of the
// jcm_train_param_info layout (nullptr if none does), and the device gradient sum of squares of the last jcm_train_apply
// (nullptr before the first one)
const float* train_param_range(jcm_ctx* c, int64_t off, int64_t n);
const double* train_grad_sumsq(jcm_ctx* c);

}  // namespace jcm

struct jcm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int precision = JCM_PRECISION_F32;
  int K = 9;
  bool finalized = false;
  // ---- options (options.h holds the table of keys, ranges and environment defaults; these initialisers are the defaults) ----
  int f32_conv = 0;             // fp32 handles: 0 = default (frequency domain, or the exact fp32 MFMA chain with conv9_fft = 0), 2 = the direct fp16x3 split kernels (forward and gradients)
  int split_min_wgs = 128;      // grids smaller than this keep the exact kernel (option "split_min_wgs")
  int sm_algo = 3;              // 3 = every transform in LDS (sm_fused.hip), 1 = direct sliding-window VALU kernel (the cross-check)
  int conv9_fft = 1;            // fp32 handles: wide 9x9 layers in the frequency domain (conv_fft.hip) when the shape allows; 0 = fp32 MFMA chain
  int fft_tiles = 1;            // fp32 handles, the pool hand-over of conv2_fullres: 2 x 2 tiles of the 120 x 180 map in the 60 x 90 maps' transform (FftArgs::tiles)
  int fft_logits_rows = 1;      // fp32 handles without training state: the logits layer behind conv5's hand-over contracts the channels on the row spectra (conv_fft_logits.hip); 0 = a whole frequency-domain layer
  int fft_fuse = 7;             // jcm_pd_forward: bit 0 = conv2 -> max pool -> conv3 (fp32 handles), bit 1 = conv4_fullres -> branch merge -> conv5 handed over in row-transformed form (conv_fft_rows_fused.hip); bit 2 = the coarse branches on the side stream (Side, SideBranches)
  int fft_single = 1;           // bf16 handles: the channel GEMM on ONE scaled fp16 part per operand (np = 5; 0 = two bf16 parts, three products)
  int fft_t16 = 1;              // bf16 handles on the one-part route (fft_single): the row-transformed tensors T / T' as complex fp16 in block floating point (Fp16Scale::t16)
  int fft_rows_mfma = 1;        // bf16 handles with 16-bit row-transformed tensors: conv5's inverse row pass on the matrix cores (FftArgs::rows_mfma; conv_fft_rows_mfma.hip)
  int fft_reg = 1;              // the register-resident transform kernels of conv_fft_reg_*.hip where they exist (FftArgs::fft_reg); 0 = the LDS kernels for every pass
  int fft_cache_gb = 64;        // bound of the filter-spectra cache (conv_route.hip: a new entry that would grow it past the bound drops the others first)
  int fft_win = 1;              // training step of fp32 handles: frequency-domain layers on 32 x 32 overlap-save windows where that shrinks the filter-sized spectra (jcm_train.hip)
  int bf16_hpool = 1;           // bf16 handles: the horizontal half of pool2 in conv2's epilogue (ConvArgs::hpool) + vpool_2x1_bf16 instead of the 2x2 pool kernel
  int torso_algo = 1;           // jcm_torso_infer: 1 = direct sliding-window kernel (torso_infer.hip), the only route
  int sm_chunk = 32;            // training step: images per slice of the spatial model's backward pass (81 + 10 spectra per image live at once)
  int micro_batch = 0;          // jcm_forward walks a batch in slices of this many images (0 = 256 bf16 / 64 fp32)
  int call_order = 1;           // 0: this handle's calls are not ordered against other handles' (debugging only)
  int debug_skip = 0;           // bisecting aid (jcm_pd_forward): bit 0 conv1(+pool1), 1 pool2, 2 conv2, 3 conv3, 4 conv4, 5 merge + conv5, 6 conv6 are NOT launched
  // ---- parameters and what is derived from them (refresh_derived) ----
  std::map<std::string, jcm::Tensor> params;
  std::map<std::string, jcm::ConvLayer> convs;
  std::vector<void*> owned;   // device allocations made at finalize
  size_t param_bytes = 0;
  bool has_sm = false;          // spatial model tables
  float* sp_energy = nullptr;   // [P][120*180]
  float* sp_bias = nullptr;     // [P][5400]
  float* bn_sm_scale = nullptr; // [10]
  float* bn_sm_shift = nullptr;
  int* cond = nullptr;          // [P] conditioning channel of pair p
  const float** energy_ptrs = nullptr;   // [P] device table of the energy_* / bias_* parameter tensors, graph order
  const float** bias_ptrs = nullptr;
  int* cond0 = nullptr;         // single zero (jcm_conv_mrf)
  float2* prior_spec_t = nullptr; // [P][91][120]: transposed half spectra of softplus5(energy) (sm_lds.hip)
  struct FftW { void* p = nullptr; size_t bytes = 0; bool valid = false; float* wscale = nullptr; };      // wscale: two device floats behind the spectra (np = 4)
  std::map<std::string, FftW> fft_w;   // the filter-spectra cache; touched by the fft_cache_* functions of conv_route.hip only
  double* hist_limits = nullptr;      // summary.hip: the positive half of TF's histogram bucket limits (uploaded on first use)
  jcm::TrainState* train = nullptr;   // created by jcm_train_begin
  // ---- workspace ----
  // arena (stack allocator, grown on demand between forwards)
  char* arena = nullptr;
  size_t arena_cap = 0, arena_off = 0, arena_peak = 0;
  bool dry = false;             // sizing pass: allocate offsets only, launch nothing
  float* act_scale = nullptr;   // fp16x3: device {S, 1/S} of the current layer input (computed before every launch), + scratch
  float* scale_scratch = nullptr;
  void* sm_scratch = nullptr;   // sm_fused.hip: partial sums + flags of sm_inv_finish_kernel's cuts (sm_fused_scratch_bytes(), zeroed once)
  unsigned sm_epoch = 0;        // ... the launch counter its flags carry
  // device words of the fp16 scaling (kernels.h: Fp16Scale): zeroed floats, one per image of every row-transformed tensor of a call.  They come from
  // blocks of kFftWords floats; a call that needs more than a block holds (a forward of > 20 000 images in one piece) gets further blocks on demand,
  // and the blocks are re-zeroed and reused from the start BETWEEN calls (CallOrder), in stream order behind every kernel that read the old words.
  static constexpr int kFftWords = 1 << 18, kFftWordsPerCall = 1 << 16;
  struct WordBlock { float* p = nullptr; int cap = 0; };
  std::vector<WordBlock> fft_blocks;
  int fft_block_i = 0, fft_word_i = 0;      // next free word: fft_blocks[fft_block_i].p + fft_word_i
  // ---- the side stream ("fft_fuse" bit 2; pd_tower.hip: SideBranches) ----
  // jcm_pd_forward runs the half- and quarter-resolution branches beside the full-resolution one.  A kernel that touches lines another stream is producing
  // leaves stale copies in its XCD's L2 (CallOrder, below), and arena alignment does not protect against a look-ahead read past the end of a buffer: so
  // everything the side stream writes while the main stream runs -- workspace, activations, x2 / x3, scale words, the split kernels' input scale -- lives in
  // allocations of its own.  Created at first use (side_init), freed by jcm_destroy.  SideBranches SWAPS these fields with their namesakes above for as long
  // as it enqueues the coarse branches, so every launch site keeps reading c->stream and c->arena: outside of that scope this struct holds the side set,
  // inside of it the main one.
  struct Side {
    hipStream_t stream = nullptr;             // hipStreamNonBlocking: the handle's own stream may be the legacy null stream, which blocking streams serialise against
    hipEvent_t fork = nullptr, join = nullptr;      // hipEventDisableTiming
    char* arena = nullptr;                    // sized by the dry pass that sizes the main arena (with_arena)
    size_t arena_cap = 0, arena_off = 0, arena_peak = 0;
    std::vector<WordBlock> fft_blocks;        // re-zeroed where the main ones are (CallOrder): on the main stream, in front of the fork
    int fft_block_i = 0, fft_word_i = 0;
    float* act_scale = nullptr;
    float* scale_scratch = nullptr;
  } side;
  // per-layer HIP-event timing on the launch stream (bench.py roofline object)
  int profile = 0;              // option "profile"
  std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> prof;
  std::vector<hipEvent_t> event_pool;   // recycled by jcm_profile_read / "profile"=0, destroyed by jcm_destroy
  // ---- call ordering (CallOrder) ----
  std::mutex call_mu;                 // held by the thread whose outermost entry point of this handle is running
  int call_depth = 0;                 // entry points of this handle on that thread's stack (> 1 only inside a gradient-ready callback)
  jcm::CallOrder* order = nullptr;    // the outermost running entry point's chain guard (notify_ready suspends it around the user callback)
};

namespace jcm {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Calls of DIFFERENT handles on one device are ordered on the GPU: an entry point that enqueues work holds the device's lock for as long
// as it is enqueuing (so two host threads never interleave their launches), first makes its stream wait (hipStreamWaitEvent, the host does
// not block) for the event the previous call of another stream recorded, and records the event again behind its own last kernel.  Each
// call fills the chip on its own, so nothing is lost; what is gained is that no kernel of this library ever runs beside a kernel of another
// handle.  The per-XCD L2s are not coherent with each other: a kernel that touches memory another stream is producing (the look-ahead
// reads past the end of a buffer that cgemm_split.hip used to make were such touches) leaves stale lines that the other stream's next
// kernel then consumes -- found by tests/test_gpu_golden.py::test_two_engines_two_streams_soak.  The known over-reads are fixed at the
// source; this ordering is the guarantee that does not depend on having found them all.  jcm_set_option("call_order", 0) takes a handle
// out of the chain (it neither waits nor records; tools/determinism.py and the soak tests use it to look for what the chain would hide).
// The outermost call's constructor also laps the fp16 scale-word ring (a nested call keeps handing out words behind the outer call's).
// The lock is NOT held while the host blocks or while user code runs: release() (record the chain event, unlock) precedes every
// host-side wait at the end of an entry point, and the gradient-ready callback of jcm_train_loss_grads runs between release() and acquire(),
// so a callback may call jcm_* entry points (also of the SAME handle: `nested`).
struct CallOrder {
  jcm_ctx* c;
  std::unique_lock<std::mutex> lk;       // the device's call chain
  std::unique_lock<std::mutex> hlk;      // the handle (outermost call only)
  bool nested = false;
  explicit CallOrder(jcm_ctx* ctx);
  ~CallOrder();
  void acquire();      // lock the device's chain and make this stream wait for the previous call of another stream
  void release();      // record the chain event behind what has been enqueued so far and unlock (idempotent)
  CallOrder(const CallOrder&) = delete;
  CallOrder& operator=(const CallOrder&) = delete;
};

template <class T>
T* arena_alloc(jcm_ctx* c, size_t count) {
  const size_t bytes = (count * sizeof(T) + 255) & ~size_t(255);
  const size_t off = c->arena_off;
  c->arena_off += bytes;
  if (c->arena_off > c->arena_peak) c->arena_peak = c->arena_off;
  return reinterpret_cast<T*>(c->arena + off);   // in a dry pass arena may be null: offsets only
}

int arena_reserve(jcm_ctx* c, size_t bytes, size_t side_bytes);      // both arenas; growing either synchronises both streams first
int side_init(jcm_ctx* c);                  // the side stream, its events and its scale buffer (first use)
int sync_streams(jcm_ctx* c);               // the handle's stream and the side stream
int dev_alloc(jcm_ctx* c, void** p, size_t bytes);
int sm_scratch_next(jcm_ctx* c, void** scratch, unsigned* epoch);      // sm_fused_forward's scratch (allocated + zeroed at first use) and the next launch epoch
const Tensor* find(jcm_ctx* c, const std::string& name);
int check(jcm_handle h, bool need_final);
const ConvLayer* conv_of(jcm_ctx* c, const std::string& scope);
// ---- derived.hip ----
int fold_bn(jcm_ctx* c, const std::string& scope, int n, float** scale, float** shift);
// Rebuild every derived table (packed weights, folded BN, softplus'd priors and their spectra) from
// the parameter store; called by jcm_finalize and after each optimizer update.
int refresh_derived(jcm_ctx* c, bool first);
// ---- jcm_api.hip ----
// HIP-event pairs for the per-layer timing come from a pool: inside a timed region the only cost is two
// hipEventRecord per launch (events are created on first use and recycled by jcm_profile_read).
int prof_event(jcm_ctx* c, hipEvent_t* e);      // one event from the pool
int prof_begin(jcm_ctx* c, hipEvent_t* e0, hipEvent_t* e1);
void prof_end(jcm_ctx* c, const std::string& scope, hipEvent_t e0, hipEvent_t e1, bool ok);
void prof_release_all(jcm_ctx* c, bool destroy);

// ---- conv_route.hip: how one conv layer runs ----
// the zero-initialised launch arguments of layer L on a [B,H,W,Cin] input; callers set further fields after the call
inline ConvArgs conv_args(const ConvLayer* L, int B, int H, int W) {
  ConvArgs a{};
  a.B = B; a.H = H; a.W = W; a.Cin = L->cin; a.Cout = L->cout;
  return a;
}
// ... of the frequency-domain route (kernels.h: FftArgs)
inline FftArgs fft_args(const ConvLayer* L, int B, int H, int W) {
  FftArgs a{};
  static_cast<ConvArgs&>(a) = conv_args(L, B, H, W);
  return a;
}
// One conv-layer request: what run_conv / run_conv_layer / run_conv_fft need beyond the layer.  Call sites name the fields they set.
struct ConvCall {
  const void* x = nullptr;      // [B,H,W,Cin] (stride 2: the image, read at every sub-th pixel of every sub-th row)
  void* out = nullptr;
  int B = 0, H = 0, W = 0;
  int stride = 1, sub = 1;
  bool act_bf16 = false;        // bf16 activations (the handle runs the bf16 path)
  bool out_f32 = false;         // ... with an fp32 result all the same (the logits layer)
  int in_planar = 0, out_planar = 0;      // bf16 layouts: ConvArgs in kernels.h
  bool x_u8 = false;            // the stride-2 layer reads a byte image
  // link (kernels.h: FftLink): what ties the call to the neighbouring frequency-domain layers -- requests read from it, the two scale-word results written to it;
  // null = the layer stands alone.  A non-empty link, or hpool (ConvArgs::hpool), for a layer that does not take the route it is meant for is JCM_ERR_STATE.
  FftLink* link = nullptr;
  int hpool = 0;
  int linear = 0;               // the epilogue stops at conv + bias whatever the layer's BatchNorm (jcm_conv_layer_pre)
  int circ = 0;                 // run_conv_fft only: x is a batch of overlap-save windows [B, H, W, Cin] that fill the transform, out their valid regions [B, H - 8, W - 8, Cout] (FftArgs::circ)
};
inline ConvCall conv_call(const void* x, void* out, int B, int H, int W) {
  ConvCall q;
  q.x = x; q.out = out; q.B = B; q.H = H; q.W = W;
  return q;
}
// takes_fft() says whether a layer / shape goes to the frequency domain; run_conv_fft() runs it (filter spectra from the cache, packed from L->w_raw when
// missing or invalidated); the training step uses both for its data gradient.
bool takes_fft(jcm_ctx* c, const ConvLayer* L, int B, int H, int W);
bool takes_strip(const ConvLayer* L, int B, int H, int W);       // bf16: conv_strip_bf16_kernel
bool takes_c5strip(const ConvLayer* L, int B, int H, int W);     // bf16: conv5_strip_bf16_kernel
const char* conv_kernel_name(jcm_ctx* c, const ConvLayer* L, int B, int H, int W);
// operand form of the channel GEMM on this handle (kernels.h): bf16 handles: 5 (one scaled fp16 part, default) or 2 (two bf16 parts); fp32 handles: 4 (two scaled fp16 parts)
inline int fft_np(const jcm_ctx* c) { return c->precision == JCM_PRECISION_BF16 ? (c->fft_single ? 5 : 2) : 4; }
int fft_new_words(jcm_ctx* c, int n, float** w);      // n zeroed device words of the scaling ring (one per image)
int run_conv_fft(jcm_ctx* c, const ConvLayer* L, const std::string& scope, const ConvCall& q);      // reads x, out, B, H, W, the bf16 layout fields, link, linear, circ
int run_conv_layer(jcm_ctx* c, const ConvLayer* L, const std::string& scope, const ConvCall& q);
int run_conv(jcm_ctx* c, const std::string& scope, const ConvCall& q);      // ... of the stored layer `scope`
// the filter-spectra cache (jcm_ctx::fft_w)
bool fft_spectra_valid(jcm_ctx* c, const std::string& scope, int H, int W, int circ = 0);
void fft_cache_drop(jcm_ctx* c);            // free every entry (the caller has synchronised the stream)
void fft_cache_invalidate(jcm_ctx* c);      // the weights changed: every entry is repacked on next use

inline int cdiv2(int v) { return (v + 1) / 2; }

// Sizing pass then the real pass, so the arena never reallocates mid-graph.  `sizing` runs dry (offsets only, nothing launched) and leaves the peak;
// `real` runs on the reserved arena.  The only place that writes c->dry.
template <class S, class R>
int with_arena(jcm_ctx* c, S&& sizing, R&& real) {
  // a call from inside the gradient-ready callback of this handle's running training step would overwrite that step's workspace
  if (c->call_depth > 1) return fail(JCM_ERR_STATE, "this entry point uses the handle's workspace and cannot be called from the gradient-ready callback of the same handle");
  c->dry = true;
  c->arena_off = 0;
  c->arena_peak = 0;
  c->side.arena_peak = 0;
  int r = sizing();
  c->dry = false;
  if (r != JCM_OK) return r;
  JCM_TRY(arena_reserve(c, c->arena_peak, c->side.arena_peak));
  c->arena_off = 0;
  return real();
}
template <class F>
int with_arena(jcm_ctx* c, F&& body) {
  return with_arena(c, body, body);
}

// ---- pd_tower.hip: the tower and the stages its entry points share with it ----
bool conv1_pool_fused(const jcm_ctx* c, const ConvLayer* L1, int H, int W);
bool conv1_split_route(const jcm_ctx* c, const ConvLayer* L1);
int conv1_pool_stage(jcm_ctx* c, const std::string& scope, const ConvLayer* L1, const void* xin, bool xin_u8, int B, int xh, int xw, int xsub, void* dst, void** p1);
// conv2_<res> -> pool2 on a bf16 handle (main.py:46-47, 54-55, 63-64), a [B,h2,w2,C] map: the activation layout between conv2, the pool and conv3, and where
// the pool's horizontal half is taken.  One place for the tower and jcm_conv2_pool.
struct Pool2Layout {
  // planar activations [B][C/8][H][W][8] when both 5x5 layers take the strip kernel (its window rows are then 1-KB contiguous LDS-DMA reads; from NHWC every
  // 16-byte unit of a pixel is a separate cache line).  A planar tensor IS an NHWC tensor of B*C/8 images with 8 channels: the pooling kernel runs on it unchanged.
  int pl23;
  // ... and the pool's horizontal half is taken in conv2's epilogue (even widths): conv2 then writes the [.., h2, w2 / 2, ..] map of pixel-pair maxima
  int hp;
};
Pool2Layout pool2_layout(jcm_ctx* c, const ConvLayer* L2, const ConvLayer* L3, int B, int h2, int w2);
hipError_t pool2_launch(jcm_ctx* c, const Pool2Layout& l, const void* c2, void* p2, int B, int h2, int w2, int C);
int pd_forward_impl(jcm_ctx* c, const void* x, bool x_u8, int B, int H, int W, float* logits);
int sm_forward_impl(jcm_ctx* c, const float* hm, int Ca, const float* extra, int B, float* logits, int extra_ld = 0);

}  // namespace jcm
