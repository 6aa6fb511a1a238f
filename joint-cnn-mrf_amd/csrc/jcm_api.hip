// libjcm C ABI (include/jcm.h), the part that belongs to no kernel file: the handle's lifetime, the parameter store, the options, the entry points
// of single layers and of the towers (main.py:29-74,94-125,522-531 as a sequence of kernel launches on one HIP stream) and the profile reader,
// with the helpers every translation unit draws on (fail, CallOrder, the arena, find / check / conv_of, prof_*).  Every other entry point sits
// beside its kernels, on the scaffold of entry.h.  No tensor library types cross this boundary -- plain pointers and sizes.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#include <mutex>
#include <vector>

#include "ctx.h"
#include "options.h"

using namespace jcm;

namespace {
thread_local std::string g_err;
}

namespace jcm {

const char* const kJointNames[10] = {"lsho", "lelb", "lwri", "rsho", "relb", "rwri", "lhip", "rhip", "nose", "torso"};

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {
struct Chain { std::mutex mu; hipEvent_t ev = nullptr; hipStream_t last = nullptr; bool armed = false; };
Chain g_chain[64];
}  // namespace
// Handles whose OUTERMOST entry point is running on this host thread.  A call is NESTED only when the same thread re-enters the handle (from the
// gradient-ready callback of its running training step); another thread's call on the same handle waits on the handle's mutex until the whole
// outermost call -- callbacks included -- has returned (the de-facto serialisation of rounds 1-4, without the data race on call_depth).
namespace {
thread_local std::vector<jcm_ctx*> t_active;
}
CallOrder::CallOrder(jcm_ctx* ctx) : c(ctx) {
  if (!c) return;
  for (jcm_ctx* a : t_active) nested = nested || a == c;
  if (!nested) {
    hlk = std::unique_lock<std::mutex>(c->call_mu);      // held for the whole outermost call
    t_active.push_back(c);
  }
  ++c->call_depth;                   // (only ever touched by the thread that holds call_mu)
  acquire();
  if (nested) return;                // the outer call's scale words stay as they are
  c->order = this;
  // the fp16-scale words are reused from the start only BETWEEN calls (a call keeps words of its early layers until its last ones: the training step)
  // (the side stream's words too, on THIS stream: every call has joined its side work before it ended, and the next fork is behind the memset)
  auto lap = [&](std::vector<jcm_ctx::WordBlock>& blocks, int& block_i, int& word_i) {
    if (block_i > 0 || word_i > jcm_ctx::kFftWords - jcm_ctx::kFftWordsPerCall) {
      for (int i = 0; i <= block_i && i < (int)blocks.size(); ++i)
        (void)hipMemsetAsync(blocks[i].p, 0, (size_t)blocks[i].cap * sizeof(float), c->stream);
      block_i = 0;
      word_i = 0;
    }
  };
  lap(c->fft_blocks, c->fft_block_i, c->fft_word_i);
  lap(c->side.fft_blocks, c->side.fft_block_i, c->side.fft_word_i);
}
void CallOrder::acquire() {
  if (!c || lk.owns_lock()) return;
  Chain& ch = g_chain[c->device & 63];
  lk = std::unique_lock<std::mutex>(ch.mu);      // held while the call is queuing kernels: two host threads never interleave their launches
  if (c->call_order) {
    if (!ch.ev && hipEventCreateWithFlags(&ch.ev, hipEventDisableTiming) != hipSuccess) ch.ev = nullptr;
    if (ch.ev && ch.armed && ch.last != c->stream) (void)hipStreamWaitEvent(c->stream, ch.ev, 0);
  }
}
void CallOrder::release() {
  if (!c || !lk.owns_lock()) return;
  if (c->call_order) {
    Chain& ch = g_chain[c->device & 63];
    if (ch.ev && hipEventRecord(ch.ev, c->stream) == hipSuccess) { ch.armed = true; ch.last = c->stream; }
  }
  lk.unlock();
}
CallOrder::~CallOrder() {
  if (!c) return;
  release();
  --c->call_depth;
  if (!nested) {
    c->order = nullptr;
    for (size_t i = t_active.size(); i-- > 0;)
      if (t_active[i] == c) { t_active.erase(t_active.begin() + (long)i); break; }
    hlk.unlock();
  }
}

int sync_streams(jcm_ctx* c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->side.stream) HIP_TRY(hipStreamSynchronize(c->side.stream));
  return JCM_OK;
}

int arena_reserve(jcm_ctx* c, size_t bytes, size_t side_bytes) {
  if (bytes <= c->arena_cap && side_bytes <= c->side.arena_cap) return JCM_OK;
  JCM_TRY(sync_streams(c));
  auto grow = [](char*& arena, size_t& cap, size_t want) {
    if (want <= cap) return (int)JCM_OK;
    if (arena) HIP_TRY(hipFree(arena));
    arena = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&arena), want));
    cap = want;
    return (int)JCM_OK;
  };
  JCM_TRY(grow(c->arena, c->arena_cap, bytes));
  return grow(c->side.arena, c->side.arena_cap, side_bytes);
}

int side_init(jcm_ctx* c) {
  jcm_ctx::Side& s = c->side;
  if (!s.stream) HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  if (!s.fork) HIP_TRY(hipEventCreateWithFlags(&s.fork, hipEventDisableTiming));
  if (!s.join) HIP_TRY(hipEventCreateWithFlags(&s.join, hipEventDisableTiming));
  if (!s.scale_scratch) {      // (the sizes of derived.hip's weight_scale, in one allocation)
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.scale_scratch), (1024 + 64) * sizeof(float)));
    s.act_scale = s.scale_scratch + 1024;
  }
  return JCM_OK;
}

int dev_alloc(jcm_ctx* c, void** p, size_t bytes) {
  HIP_TRY(hipMalloc(p, bytes));
  c->owned.push_back(*p);
  c->param_bytes += bytes;
  return JCM_OK;
}

// the balanced spatial-model kernel's partial sums + flags (sm_fused.hip): allocated and zeroed once per handle; every launch takes the next epoch
int sm_scratch_next(jcm_ctx* c, void** scratch, unsigned* epoch) {
  if (!c->sm_scratch) {
    const size_t n = sm_fused_scratch_bytes();
    JCM_TRY(dev_alloc(c, &c->sm_scratch, n));
    HIP_TRY(hipMemsetAsync(c->sm_scratch, 0, n, c->stream));
  }
  if (++c->sm_epoch == 0) {      // (the counter wrapped: flags of 2^32 launches ago could match -- start over from zeroed flags)
    HIP_TRY(hipMemsetAsync(c->sm_scratch, 0, sm_fused_scratch_bytes(), c->stream));
    c->sm_epoch = 1;
  }
  *scratch = c->sm_scratch;
  *epoch = c->sm_epoch;
  return JCM_OK;
}

const Tensor* find(jcm_ctx* c, const std::string& name) {
  auto it = c->params.find(name);
  return it == c->params.end() ? nullptr : &it->second;
}

int check(jcm_handle h, bool need_final) {
  if (!h) return fail(JCM_ERR_ARG, "null handle");
  if (need_final && !h->finalized) return fail(JCM_ERR_STATE, "jcm_finalize has not been called");
  return JCM_OK;
}

const ConvLayer* conv_of(jcm_ctx* c, const std::string& scope) {
  auto it = c->convs.find(scope);
  return it == c->convs.end() ? nullptr : &it->second;
}

int prof_event(jcm_ctx* c, hipEvent_t* e) {
  if (!c->event_pool.empty()) {
    *e = c->event_pool.back();
    c->event_pool.pop_back();
    return JCM_OK;
  }
  HIP_TRY(hipEventCreate(e));
  return JCM_OK;
}
int prof_begin(jcm_ctx* c, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!c->profile) return JCM_OK;
  JCM_TRY(prof_event(c, e0));
  if (int r = prof_event(c, e1); r != JCM_OK) { c->event_pool.push_back(*e0); *e0 = nullptr; return r; }
  hipError_t e = hipEventRecord(*e0, c->stream);
  if (e != hipSuccess) {
    prof_end(c, "", *e0, *e1, false);
    *e0 = *e1 = nullptr;
    return fail(JCM_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
  }
  return JCM_OK;
}
// ok: the launch went out -> record the closing event and file the pair under `scope`; otherwise return both to the pool
void prof_end(jcm_ctx* c, const std::string& scope, hipEvent_t e0, hipEvent_t e1, bool ok) {
  if (!e0) return;
  if (ok && hipEventRecord(e1, c->stream) == hipSuccess) {
    c->prof[scope].emplace_back(e0, e1);
  } else {
    c->event_pool.push_back(e0);
    c->event_pool.push_back(e1);
  }
}
void prof_release_all(jcm_ctx* c, bool destroy) {
  for (auto& kv : c->prof)
    for (auto& ev : kv.second) { c->event_pool.push_back(ev.first); c->event_pool.push_back(ev.second); }
  c->prof.clear();
  if (destroy) {
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    c->event_pool.clear();
  }
}

}  // namespace jcm

namespace {

const Option* find_option(const char* key) {
  for (const Option& o : kOptions)
    if (key && std::strcmp(key, o.name) == 0) return &o;
  return nullptr;
}
// the value as the option stores it, or JCM_ERR_ARG
int option_value(const Option& o, int64_t* value) {
  if (o.kind == Option::BOOL) *value = *value != 0;
  else if (o.kind == Option::RANGE ? (*value < o.lo || *value > o.hi) : (*value != o.lo && *value != o.hi))
    return fail(JCM_ERR_ARG, std::string(o.name) + " must be " + std::to_string(o.lo) + (o.kind == Option::RANGE ? " .. " : " or ") + std::to_string(o.hi) + " (include/jcm.h)");
  return JCM_OK;
}

}  // namespace

namespace jcm {
int option_profile(jcm_ctx* c, int64_t value) {
  if (value && !c->profile) {
    DeviceGuard g(c->device);
    (void)hipStreamSynchronize(c->stream);
    prof_release_all(c, false);
  }
  return JCM_OK;
}
int option_fft_single(jcm_ctx* c, int64_t value) {
  if (value != c->fft_single) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    fft_cache_drop(c);      // the spectra were packed for the other operand form
  }
  return JCM_OK;
}
}  // namespace jcm

extern "C" {

int jcm_abi_version(void) { return 1; }

const char* jcm_last_error(void) { return g_err.c_str(); }

int jcm_create(int device, void* stream, jcm_handle* out) {
  if (!out) return fail(JCM_ERR_ARG, "null out pointer");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(JCM_ERR_ARG, "device " + std::to_string(device) + " out of range (" + std::to_string(n) + " visible)");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(JCM_ERR_HIP, std::string("libjcm is built for gfx950 (MI355X) only; device reports ") + prop.gcnArchName);
  jcm_ctx* c = new jcm_ctx();
  c->device = device;
  c->stream = static_cast<hipStream_t>(stream);
  // the environment supplies defaults, read here and nowhere else (a value the option would refuse is ignored)
  for (const Option& o : kOptions) {
    const char* e = o.env ? std::getenv(o.env) : nullptr;
    int64_t v = e ? std::atoi(e) : 0;
    if (e && option_value(o, &v) == JCM_OK) c->*o.field = (int)v;
  }
  *out = c;
  return JCM_OK;
}

int jcm_destroy(jcm_handle h) {
  if (!h) return JCM_OK;
  DeviceGuard g(h->device);
  (void)sync_streams(h);
  prof_release_all(h, true);
  if (h->train) train_destroy(h);
  for (auto& kv : h->params) (void)hipFree(kv.second.d);
  for (void* p : h->owned) (void)hipFree(p);
  fft_cache_drop(h);
  for (auto& b : h->fft_blocks) (void)hipFree(b.p);
  if (h->arena) (void)hipFree(h->arena);
  for (auto& b : h->side.fft_blocks) (void)hipFree(b.p);
  if (h->side.arena) (void)hipFree(h->side.arena);
  if (h->side.scale_scratch) (void)hipFree(h->side.scale_scratch);
  if (h->side.fork) (void)hipEventDestroy(h->side.fork);
  if (h->side.join) (void)hipEventDestroy(h->side.join);
  if (h->side.stream) (void)hipStreamDestroy(h->side.stream);
  delete h;
  return JCM_OK;
}

int jcm_set_option(jcm_handle h, const char* key, int64_t value) {
  JCM_TRY(check(h, false));
  const Option* o = find_option(key);
  if (!o) return fail(JCM_ERR_ARG, std::string("unknown option '") + (key ? key : "") + "'");
  if (o->before_finalize && h->finalized) return fail(JCM_ERR_STATE, std::string("option '") + o->name + "' must be set before jcm_finalize");
  JCM_TRY(option_value(*o, &value));
  if (o->on_change) JCM_TRY(o->on_change(h, value));
  h->*o->field = (int)value;
  return JCM_OK;
}

int jcm_get_option(jcm_handle h, const char* key, int64_t* value) {
  JCM_TRY(check(h, false));
  const Option* o = find_option(key);
  if (!o || !value) return fail(JCM_ERR_ARG, std::string("unknown option '") + (key ? key : "") + "' or null value pointer");
  *value = h->*o->field;
  return JCM_OK;
}

int jcm_set_tensor(jcm_handle h, const char* name, const float* data, const int64_t* shape, int ndim) {
  JCM_TRY(check(h, false));
  if (h->finalized) return fail(JCM_ERR_STATE, "parameters must be set before jcm_finalize");
  if (!name || !data || !shape || ndim < 1 || ndim > 4) return fail(JCM_ERR_ARG, "bad set_tensor arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] <= 0) return fail(JCM_ERR_ARG, std::string("non-positive dimension in '") + name + "'");
    n *= (size_t)shape[i];
  }
  Tensor& t = h->params[name];
  if (t.d) { (void)hipFree(t.d); h->param_bytes -= t.n * sizeof(float); }
  t.shape.assign(shape, shape + ndim);
  t.n = n;
  t.d = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t.d), n * sizeof(float)));
  h->param_bytes += n * sizeof(float);
  HIP_TRY(hipMemcpyAsync(t.d, data, n * sizeof(float), hipMemcpyDefault, h->stream));
  order.release();
  HIP_TRY(hipStreamSynchronize(h->stream));   // the caller may free `data` on return
  return JCM_OK;
}

int jcm_finalize(jcm_handle h) {
  JCM_TRY(check(h, false));
  if (h->finalized) return fail(JCM_ERR_STATE, "already finalized");
  DeviceGuard g(h->device);
  CallOrder order(h);
  JCM_TRY(refresh_derived(h, true));
  h->finalized = true;
  return JCM_OK;
}

int jcm_get_tensor(jcm_handle h, const char* name, float* out, int64_t count) {
  JCM_TRY(check(h, false));
  if (!name || !out) return fail(JCM_ERR_ARG, "bad get_tensor arguments");
  const Tensor* t = find(h, name);
  if (!t) return fail(JCM_ERR_STATE, std::string("no parameter '") + name + "'");
  if ((int64_t)t->n != count) return fail(JCM_ERR_ARG, std::string("'") + name + "' has " + std::to_string(t->n) + " elements");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(hipMemcpyAsync(out, t->d, t->n * sizeof(float), hipMemcpyDefault, h->stream));
  order.release();
  HIP_TRY(hipStreamSynchronize(h->stream));
  return JCM_OK;
}

int jcm_update_tensor(jcm_handle h, const char* name, const float* data, int64_t count, int refresh) {
  JCM_TRY(check(h, true));
  if (!name || !data) return fail(JCM_ERR_ARG, "bad update_tensor arguments");
  auto it = h->params.find(name);
  if (it == h->params.end()) return fail(JCM_ERR_STATE, std::string("no parameter '") + name + "'");
  if ((int64_t)it->second.n != count) return fail(JCM_ERR_ARG, std::string("'") + name + "' has " + std::to_string(it->second.n) + " elements");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (h->call_depth > 1) return fail(JCM_ERR_STATE, "jcm_update_tensor changes the handle's training state or parameters and cannot be called from the gradient-ready callback of the same handle");
  HIP_TRY(hipMemcpyAsync(it->second.d, data, it->second.n * sizeof(float), hipMemcpyDefault, h->stream));
  order.release();
  const hipError_t se = hipStreamSynchronize(h->stream);   // the caller may free `data` on return
  if (refresh) order.acquire();
  HIP_TRY(se);
  if (refresh) {
    JCM_TRY(refresh_derived(h, false));
    if (h->train) dgrad_filters_stale(h);
  }
  return JCM_OK;
}

int jcm_conv_layer(jcm_handle h, const char* scope, int stride, int last_layer, const float* x, int B, int H, int W, float* out) {
  JCM_TRY(check(h, true));
  if (!scope || !x || !out || B < 1 || H < 1 || W < 1) return fail(JCM_ERR_ARG, "bad conv_layer arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  const ConvLayer* L = conv_of(h, scope);
  if (!L) return fail(JCM_ERR_STATE, std::string("no conv layer '") + scope + "'");
  if ((last_layer != 0) == L->has_bn)
    return fail(JCM_ERR_ARG, std::string("last_layer flag disagrees with the BatchNorm parameters stored for '") + scope + "'");
  if (h->precision == JCM_PRECISION_F32)      // (the frequency-domain route of the wide 9x9 layers takes its scratch from the arena)
    return with_arena(h, [&] {
      ConvCall q = conv_call(x, out, B, H, W);
      q.stride = stride;
      return run_conv(h, scope, q);
    });
  // bf16 handle: the boundary stays fp32 NHWC; the layer runs exactly as inside the tower -- input rounded to bf16 (the
  // activation type of that path), bf16 MFMA kernel, bf16 result (fp32 for the logits layer) -- and is widened back.
  if (stride != 1) return fail(JCM_ERR_ARG, "bf16 handles run the stride-2 first layer fused with its pool inside jcm_pd_forward only");
  jcm_ctx* c = h;
  return with_arena(c, [&] {
    const size_t nin = (size_t)B * H * W * L->cin, nout = (size_t)B * H * W * L->cout;
    void* xb = arena_alloc<char>(c, nin * 2);
    void* ob = last_layer ? nullptr : static_cast<void*>(arena_alloc<char>(c, nout * 2));
    if (!c->dry) HIP_TRY(cast_pad_bf16(x, L->cin, xb, L->cin, (size_t)B * H * W, c->stream));
    ConvCall q = conv_call(xb, last_layer ? static_cast<void*>(out) : ob, B, H, W);
    q.act_bf16 = true; q.out_f32 = last_layer != 0;
    JCM_TRY(run_conv(c, scope, q));   // (sizes its own scratch in the dry pass)
    if (!c->dry && !last_layer) HIP_TRY(cast_bf16_f32(ob, out, nout, c->stream));
    return (int)JCM_OK;
  });
}

// pre_activ of main.py:160 for any stored layer: the route jcm_conv_layer takes for this layer and geometry (stand-alone: nothing handed over), its
// epilogue stopped at conv + bias (ConvArgs::relu_bn = 0; the stride-2 kernel's linear instantiation).  Everything is checked before the first launch.
int jcm_conv_layer_pre(jcm_handle h, const char* scope, int stride, const float* x, int B, int H, int W, float* z_out) {
  JCM_TRY(check(h, true));
  if (!scope || !x || !z_out || B < 1 || H < 1 || W < 1) return fail(JCM_ERR_ARG, "bad conv_layer_pre arguments");
  if (stride != 1 && stride != 2) return fail(JCM_ERR_ARG, "conv_layer_pre: stride must be 1 or 2, got " + std::to_string(stride));
  if (h->precision != JCM_PRECISION_F32)
    return fail(JCM_ERR_ARG, "conv_layer_pre: fp32 handles only (the pre-activation summaries are fp32; this is a bf16 handle)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  const ConvLayer* L = conv_of(h, scope);
  if (!L) return fail(JCM_ERR_STATE, std::string("no conv layer '") + scope + "'");
  if ((int64_t)B * H * W * std::max(L->cin, L->cout) >= ((int64_t)1 << 40)) return fail(JCM_ERR_ARG, "conv_layer_pre: tensor too large");
  if (stride == 2 && !(L->ks == 5 && L->cin == 3 && L->cout % 16 == 0 && L->cout <= 64))
    return fail(JCM_ERR_ARG, std::string("conv_layer_pre: the stride-2 kernel exists for 5x5, Cin = 3, Cout % 16 == 0, Cout <= 64 ('") + scope + "')");
  if (stride == 1 && !L->wp && !takes_fft(h, L, B, H, W))
    return fail(JCM_ERR_ARG, std::string("conv_layer_pre: no stride-1 kernel for layer '") + scope + "' (size 5 or 9, Cin % 16 == 0)");
  return with_arena(h, [&] {
    ConvCall q = conv_call(x, z_out, B, H, W);
    q.stride = stride; q.linear = 1;
    return run_conv(h, scope, q);
  });
}

// conv_layer(((x1 + up(x2)) + up(x3)) / 3) (main.py:58,67,69-71) exactly as the tower runs it: on the frequency-domain route the merge is formed by the
// layer's forward row pass (rows_fwd_merge*), otherwise by the merge kernel in front of the layer.
int jcm_conv_layer_merged(jcm_handle h, const char* scope, const float* x1, const float* x2, int H2, int W2, const float* x3, int H3, int W3, int B, int H, int W,
                          float* out) {
  JCM_TRY(check(h, true));
  if (!scope || !x1 || !x2 || !x3 || !out || B < 1 || H < 1 || W < 1 || H2 < 1 || W2 < 1 || H3 < 1 || W3 < 1) return fail(JCM_ERR_ARG, "bad conv_layer_merged arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const ConvLayer* L = conv_of(c, scope);
  if (!L) return fail(JCM_ERR_STATE, std::string("no conv layer '") + scope + "'");
  if (!L->has_bn) return fail(JCM_ERR_ARG, "conv_layer_merged: a layer with BatchNorm parameters is expected (conv5)");
  const bool bf = c->precision != JCM_PRECISION_F32;
  if (bf && L->cin % 8) return fail(JCM_ERR_ARG, "conv_layer_merged: Cin % 8 != 0 on a bf16 handle");
  return with_arena(c, [&] {
    const size_t n1 = (size_t)B * H * W * L->cin, n2 = (size_t)B * H2 * W2 * L->cin, n3 = (size_t)B * H3 * W3 * L->cin, nout = (size_t)B * H * W * L->cout;
    const void *a1 = x1, *a2 = x2, *a3 = x3;
    void* ob = out;
    if (bf) {      // the boundary stays fp32 NHWC (jcm_conv_layer): the three maps are rounded to bf16, the result is widened back
      void* b1 = arena_alloc<char>(c, n1 * 2);
      void* b2 = arena_alloc<char>(c, n2 * 2);
      void* b3 = arena_alloc<char>(c, n3 * 2);
      ob = arena_alloc<char>(c, nout * 2);
      if (!c->dry) {
        HIP_TRY(cast_pad_bf16(x1, L->cin, b1, L->cin, (size_t)B * H * W, c->stream));
        HIP_TRY(cast_pad_bf16(x2, L->cin, b2, L->cin, (size_t)B * H2 * W2, c->stream));
        HIP_TRY(cast_pad_bf16(x3, L->cin, b3, L->cin, (size_t)B * H3 * W3, c->stream));
      }
      a1 = b1; a2 = b2; a3 = b3;
    }
    FftMerge mg{a2, H2, W2, a3, H3, W3};
    const void* in = a1;
    FftLink k;
    if (takes_fft(c, L, B, H, W)) {
      k.merge = &mg;
    } else {
      void* merged = arena_alloc<char>(c, n1 * (bf ? 2 : 4));
      if (!c->dry) HIP_TRY(upsample_merge3(a1, a2, H2, W2, a3, H3, W3, merged, bf, B, H, W, L->cin, c->stream));
      in = merged;
    }
    ConvCall q = conv_call(in, ob, B, H, W);
    q.act_bf16 = bf; q.link = &k;
    JCM_TRY(run_conv(c, scope, q));
    if (bf && !c->dry) HIP_TRY(cast_bf16_f32(ob, out, nout, c->stream));
    return (int)JCM_OK;
  });
}

int jcm_max_pool(jcm_handle h, const float* x, int B, int H, int W, int C, float* out) {
  JCM_TRY(check(h, false));
  if (!x || !out || B < 1 || H < 1 || W < 1 || C < 1 || C % 4) return fail(JCM_ERR_ARG, "bad max_pool arguments (C must be a multiple of 4)");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(max_pool_2x2(x, out, false, B, H, W, C, h->stream));
  return JCM_OK;
}

// ((x1 + up(x2)) + up(x3)) / 3 by the launcher the tower calls: upsample_merge3, or upsample_merge3_planar on planar tensors.  No casts, no dependence on
// the handle's precision; everything is checked before the launch.
int jcm_upsample_merge3(jcm_handle h, const void* x1, const void* x2, int H2, int W2, const void* x3, int H3, int W3, int B, int H, int W, int C, int is_bf16,
                        int planar, void* out) {
  JCM_TRY(check(h, false));
  if (!x1 || !x2 || !x3 || !out || B < 1 || H < 1 || W < 1 || C < 1 || H2 < 1 || W2 < 1 || H3 < 1 || W3 < 1)
    return fail(JCM_ERR_ARG, "bad upsample_merge3 arguments");
  if (C % 4) return fail(JCM_ERR_ARG, "upsample_merge3: C must be a multiple of 4, got " + std::to_string(C));
  if (planar && (!is_bf16 || C % 8)) return fail(JCM_ERR_ARG, "upsample_merge3: planar tensors are bf16 with C % 8 == 0");
  const int cu = (planar || (is_bf16 && C % 8 == 0)) ? 8 : 4;      // channels per unit of the kernel that runs
  const auto too_large = [&](int hh, int ww) {      // a product of four ints: each partial product is tested, so nothing wraps
    uint64_t n = (uint64_t)B * (uint64_t)hh;
    if (n >> 32) return true;
    n *= (uint64_t)ww;
    if (n >> 32) return true;
    return (n * (uint64_t)(C / cu)) >> 32 != 0;
  };
  if (too_large(H, W) || too_large(H2, W2) || too_large(H3, W3)) return fail(JCM_ERR_ARG, "upsample_merge3: 2^32 units or more");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (planar) HIP_TRY(upsample_merge3_planar(x1, x2, H2, W2, x3, H3, W3, out, B, H, W, C, h->stream));
  else HIP_TRY(upsample_merge3(x1, x2, H2, W2, x3, H3, W3, out, is_bf16 != 0, B, H, W, C, h->stream));
  return JCM_OK;
}

int jcm_resize_bilinear(jcm_handle h, const float* x, int B, int H, int W, int C, int OH, int OW, float* out) {
  JCM_TRY(check(h, false));
  if (!x || !out || B < 1 || H < 1 || W < 1 || C < 1 || OH < 1 || OW < 1) return fail(JCM_ERR_ARG, "bad resize arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(resize_bilinear(x, out, B, H, W, C, OH, OW, h->stream));
  return JCM_OK;
}

static int pd_forward_entry(jcm_handle h, const void* x, bool x_u8, int B, int H, int W, float* logits_out) {
  JCM_TRY(check(h, true));
  if (!x || !logits_out || B < 1 || H < 8 || W < 8) return fail(JCM_ERR_ARG, "bad pd_forward arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  return with_arena(h, [&] { return pd_forward_impl(h, x, x_u8, B, H, W, logits_out); });
}
int jcm_pd_forward(jcm_handle h, const float* x, int B, int H, int W, float* logits_out) { return pd_forward_entry(h, x, false, B, H, W, logits_out); }
int jcm_pd_forward_u8(jcm_handle h, const uint8_t* x, int B, int H, int W, float* logits_out) { return pd_forward_entry(h, x, true, B, H, W, logits_out); }

// pool1(conv1_<res>(x[:, ::sub, ::sub])) through conv1_pool_stage, the function the tower calls.  Everything is checked before the first launch.
int jcm_conv1_pool(jcm_handle h, const char* scope, const void* x, int x_u8, int B, int H, int W, int sub, void* out) {
  JCM_TRY(check(h, true));
  if (!scope || !x || !out || B < 1 || B > 65535 || H < 1 || W < 1) return fail(JCM_ERR_ARG, "bad conv1_pool arguments (B in [1, 65535], H, W >= 1)");
  if (sub != 1 && sub != 2 && sub != 4) return fail(JCM_ERR_ARG, "conv1_pool: sub must be 1, 2 or 4, got " + std::to_string(sub));
  if (H % sub || W % sub)
    return fail(JCM_ERR_ARG, "conv1_pool: H and W must be multiples of sub (the tower resizes such an image instead of sub-sampling it), got " + std::to_string(H) + " x " + std::to_string(W));
  if ((int64_t)B * H * W * 3 >= ((int64_t)1 << 40)) return fail(JCM_ERR_ARG, "conv1_pool: tensor too large");
  DeviceGuard g(h->device);
  CallOrder order(h);
  const ConvLayer* L = conv_of(h, scope);
  if (!L) return fail(JCM_ERR_STATE, std::string("no conv layer '") + scope + "'");
  if (!(L->ks == 5 && L->cin == 3 && L->has_bn && L->cout % 16 == 0 && L->cout <= 64))
    return fail(JCM_ERR_ARG, std::string("conv1_pool: a 5x5, Cin = 3, BatchNorm layer with Cout % 16 == 0, Cout <= 64 is expected ('") + scope + "')");
  void* p1 = nullptr;
  return with_arena(h, [&] { return conv1_pool_stage(h, scope, L, x, x_u8 != 0, B, H, W, sub, out, &p1); });
}

// pool2(conv2_<res>(p1)) of a bf16 handle as the tower runs it (pool2_layout, pool2_launch), brought to NHWC at the end.
int jcm_conv2_pool(jcm_handle h, const char* scope, const void* p1, int B, int H, int W, void* out) {
  JCM_TRY(check(h, true));
  if (!scope || !p1 || !out || B < 1 || H < 1 || W < 1) return fail(JCM_ERR_ARG, "bad conv2_pool arguments");
  if (std::strncmp(scope, "conv2_", 6) != 0) return fail(JCM_ERR_ARG, std::string("conv2_pool: scope must be conv2_<res>, got '") + scope + "'");
  if (h->precision != JCM_PRECISION_BF16)
    return fail(JCM_ERR_STATE, "conv2_pool: bf16 handles only -- on an fp32 handle the pooled map is never materialised (conv2 hands conv3 its row-transformed input); this is an fp32 handle");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const ConvLayer* L2 = conv_of(c, scope);
  const ConvLayer* L3 = conv_of(c, std::string("conv3_") + (scope + 6));      // the tower's layout choice looks at the consumer too
  if (!L2 || !L3) return fail(JCM_ERR_STATE, std::string("conv2_pool: no conv layer '") + (L2 ? std::string("conv3_") + (scope + 6) : std::string(scope)) + "'");
  if (!(L2->ks == 5 && L2->has_bn && L2->wp_bf16 && L2->cout % 8 == 0))
    return fail(JCM_ERR_ARG, std::string("conv2_pool: a 5x5 BatchNorm layer with Cout % 8 == 0 is expected ('") + scope + "')");
  if ((int64_t)B * H * W * std::max(L2->cin, L2->cout) >= ((int64_t)1 << 40)) return fail(JCM_ERR_ARG, "conv2_pool: tensor too large");
  return with_arena(c, [&] {
    const int h3 = cdiv2(H), w3 = cdiv2(W);
    const Pool2Layout lay = pool2_layout(c, L2, L3, B, H, W);
    void* c2 = arena_alloc<char>(c, (size_t)B * H * W * L2->cout * 2);
    ConvCall q = conv_call(p1, c2, B, H, W);
    q.act_bf16 = true; q.out_planar = lay.pl23; q.hpool = lay.hp;
    JCM_TRY(run_conv(c, scope, q));
    void* p2 = lay.pl23 ? static_cast<void*>(arena_alloc<char>(c, (size_t)B * h3 * w3 * L2->cout * 2)) : out;
    if (c->dry) return (int)JCM_OK;
    HIP_TRY(pool2_launch(c, lay, c2, p2, B, H, W, L2->cout));
    if (lay.pl23) HIP_TRY(planar_to_nhwc_bf16(p2, out, B, h3 * w3, L2->cout, c->stream));
    return (int)JCM_OK;
  });
}

int jcm_spatial_softmax(jcm_handle h, const float* in, int B, int HW, int K, float* out) {
  JCM_TRY(check(h, false));
  if (!in || !out || B < 1 || HW < 1 || K < 1) return fail(JCM_ERR_ARG, "bad spatial_softmax arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(softmax_argmax(in, out, nullptr, B, HW, 1, K, h->stream));   // one-pass kernel for K = 9 maps, general kernel otherwise
  return JCM_OK;
}

int jcm_conv_mrf(jcm_handle h, const float* A, const float* Bmaps, int B, float* out) {
  JCM_TRY(check(h, true));
  if (!A || !Bmaps || !out || B < 1) return fail(JCM_ERR_ARG, "bad conv_mrf arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  return with_arena(c, [&] {
    if (c->sm_algo == 1) {
      float* rev = arena_alloc<float>(c, (size_t)B * kHmH * 96);
      float* cpre = arena_alloc<float>(c, (size_t)B * kCH * kCW);
      if (c->dry) return (int)JCM_OK;
      HIP_TRY(sm_likelihood(Bmaps, 1, nullptr, nullptr, nullptr, rev, B, 1, c->stream));     // reversed, padded copy
      HIP_TRY(sm_pair_conv(A, rev, c->cond0, cpre, B, 1, 1, c->stream));         // main.py:83-87
      HIP_TRY(sm_resize_only(cpre, out, B, c->stream));                          // main.py:89
      return (int)JCM_OK;
    }
    // transforms in LDS (sm_fused.hip / sm_lds.hip), spectra transposed [91][120]: the map in the top-left corner of a zero 120x180 frame, the
    // product, and rows 59..119 of the circular convolution, whose window [59.., 89..] is the VALID true convolution
    float2* lhat = arena_alloc<float2>(c, (size_t)B * kSpec);
    float2* ahat = arena_alloc<float2>(c, kSpec);
    float2* spec = arena_alloc<float2>(c, (size_t)B * kSpec);
    float* cfull = arena_alloc<float>(c, (size_t)B * kFrame);
    if (c->dry) return (int)JCM_OK;
    HIP_TRY(sm_fused_spectra(Bmaps, 1, nullptr, 0, nullptr, nullptr, lhat, B, 1, c->stream));
    HIP_TRY(sm_lds_fwd_frames(A, ahat, 1, c->stream));
    HIP_TRY(sm_spec_mul(lhat, ahat, c->cond0, spec, B, 1, 1, c->stream));        // main.py:83-87 (1 / (120 * 180) inside)
    HIP_TRY(sm_lds_inv_frames(spec, cfull, B, 59, 61, 1.0f, c->stream));
    HIP_TRY(sm_resize_frame(cfull, out, B, c->stream));                          // main.py:89
    return (int)JCM_OK;
  });
}

int jcm_sm_forward(jcm_handle h, const float* hm10, int B, float* logits_out) {
  JCM_TRY(check(h, true));
  if (!hm10 || !logits_out || B < 1) return fail(JCM_ERR_ARG, "bad sm_forward arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  return with_arena(h, [&] { return sm_forward_impl(h, hm10, kC, nullptr, B, logits_out); });
}

int jcm_softmax_argmax(jcm_handle h, const float* logits, int B, int HH, int WW, int K, float* prob, int32_t* coords) {
  JCM_TRY(check(h, false));
  if (!logits || (!prob && !coords) || B < 1 || HH < 1 || WW < 1 || K < 1) return fail(JCM_ERR_ARG, "bad softmax_argmax arguments");
  if (!prob && !(K == 9 && (HH * WW) % 4 == 0 && HH * WW <= 5632))
    return fail(JCM_ERR_ARG, "softmax_argmax without a probability output exists for K = 9 and H*W % 4 == 0, H*W <= 5632 only");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(softmax_argmax(logits, prob, coords, B, HH * WW, WW, K, h->stream));
  return JCM_OK;
}

int jcm_argmax_coords(jcm_handle h, const float* hm, int B, int HH, int WW, int K, int32_t* coords) {
  JCM_TRY(check(h, false));
  if (!hm || !coords || B < 1 || HH < 1 || WW < 1 || K < 1) return fail(JCM_ERR_ARG, "bad argmax arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(argmax_coords(hm, coords, B, HH * WW, WW, K, h->stream));
  return JCM_OK;
}

// The tower of main.py:522-531, optionally with the two cross-entropy terms of main.py:538-539 in inference mode (what
// eval_error runs, main.py:275-283).  The torso channel is `torso` [B,HW,1], or channel K of y [B,HW,K+1] when y is given.
static int forward_impl(jcm_handle h, const void* x, bool x_u8, const float* torso, const float* y, int B, int H, int W, int use_sm,
                        float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords, float* losses) {
  JCM_TRY(check(h, true));
  if (!x || B < 1 || H < 8 || W < 8) return fail(JCM_ERR_ARG, "bad forward arguments");
  const int tld = y ? h->K + 1 : 1;                       // floats per pixel of the tensor the torso channel lives in
  if (y) torso = y + h->K;
  if (use_sm && !torso) return fail(JCM_ERR_ARG, "use_sm needs the torso heat map (y_in[...,K:], main.py:528)");
  if (use_sm && (cdiv2(cdiv2(cdiv2(H))) != kHmH || cdiv2(cdiv2(cdiv2(W))) != kHmW))
    return fail(JCM_ERR_ARG, "the spatial model is defined for 60x90 heat maps (480x720 images) only");
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  const int K = c->K;
  if (use_sm && K + 1 != kC) return fail(JCM_ERR_ARG, "use_sm requires n_joints == 9 (10-channel spatial model)");
  const int hh = cdiv2(cdiv2(cdiv2(H))), ww = cdiv2(cdiv2(cdiv2(W)));
  // Images are independent in inference (moving-statistics BatchNorm, main.py:406), so a large batch -- a rank's
  // share of BASELINE configs[3]'s 2048 -- is walked in micro-batches: the arena is sized for one micro-batch,
  // every launch sequence is the one a batch of that size gets, and the outputs land in the caller's tensors at
  // the image offset.  The arena is sized once, for the largest micro-batch.
  const int mb_opt = c->micro_batch > 0 ? c->micro_batch : (c->precision == JCM_PRECISION_BF16 ? 256 : 64);
  const int mb = B < mb_opt ? B : mb_opt;
  auto body = [&](int b0, int nb) {
    const size_t n = (size_t)nb * hh * ww * K;
    const size_t o = (size_t)b0 * hh * ww * K;
    float* logits = arena_alloc<float>(c, n);
    float* prob = pd_prob ? pd_prob + o : arena_alloc<float>(c, n);
    const size_t mark = c->arena_off;
    const void* xb = static_cast<const char*>(x) + (size_t)b0 * H * W * 3 * (x_u8 ? 1 : sizeof(float));
    JCM_TRY(pd_forward_impl(c, xb, x_u8, nb, H, W, logits));            // main.py:522
    c->arena_off = mark;
    // spatial_softmax (main.py:523) and the argmax of evaluation.py:15-24 in one pass over the logits
    if (!c->dry) HIP_TRY(softmax_argmax(logits, prob, pd_coords ? pd_coords + (size_t)b0 * 2 * K : nullptr, nb, hh * ww, ww, K, c->stream));
    float* ce = losses ? arena_alloc<float>(c, 2 * (size_t)nb * K) : nullptr;            // per (image, joint) cross entropies
    const float* yb = y ? y + (size_t)b0 * hh * ww * (K + 1) : nullptr;
    if (losses && !c->dry) HIP_TRY(softmax_ce(logits, yb, nb, hh * ww, K, K + 1, 0.f, ce, nullptr, 0, 0, c->stream));     // main.py:538
    if (use_sm) {
      float* sml = arena_alloc<float>(c, n);
      float* smp = sm_prob ? sm_prob + o : nullptr;
      hipEvent_t s0 = nullptr, s1 = nullptr;
      if (!c->dry) JCM_TRY(prof_begin(c, &s0, &s1));
      const int rs = sm_forward_impl(c, prob, K, torso + (size_t)b0 * hh * ww * tld, nb, sml, tld);       // main.py:528,530
      if (!c->dry) prof_end(c, "sm", s0, s1, rs == JCM_OK);      // jcm_profile_read("sm"): the spatial model's kernels (bench.py roofline.sm)
      JCM_TRY(rs);
      if (!c->dry && (smp || sm_coords))
        HIP_TRY(softmax_argmax(sml, smp, sm_coords ? sm_coords + (size_t)b0 * 2 * K : nullptr, nb, hh * ww, ww, K, c->stream));   // main.py:531
      if (losses && !c->dry) HIP_TRY(softmax_ce(sml, yb, nb, hh * ww, K, K + 1, 0.f, ce + (size_t)nb * K, nullptr, 0, 0, c->stream));   // main.py:539
    } else if (losses && !c->dry) {
      HIP_TRY(hipMemcpyAsync(ce + (size_t)nb * K, ce, (size_t)nb * K * sizeof(float), hipMemcpyDeviceToDevice, c->stream));       // main.py:535
    }
    if (losses && !c->dry) HIP_TRY(loss_means_accumulate(ce, nb * K, 1.0f / (float)(B * K), losses, b0 == 0, c->stream));      // reduce_mean, main.py:240
    return (int)JCM_OK;
  };
  // sizing pass on the largest micro-batch, then the real passes (the arena never reallocates mid-graph)
  return with_arena(c, [&] { return body(0, mb); }, [&] {
    for (int b0 = 0; b0 < B; b0 += mb) {
      c->arena_off = 0;
      JCM_TRY(body(b0, B - b0 < mb ? B - b0 : mb));
    }
    return (int)JCM_OK;
  });
}

int jcm_forward(jcm_handle h, const float* x, const float* torso, int B, int H, int W, int use_sm,
                float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords) {
  return forward_impl(h, x, false, torso, nullptr, B, H, W, use_sm, pd_prob, sm_prob, pd_coords, sm_coords, nullptr);
}
int jcm_forward_u8(jcm_handle h, const uint8_t* x, const float* torso, int B, int H, int W, int use_sm,
                   float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords) {
  return forward_impl(h, x, true, torso, nullptr, B, H, W, use_sm, pd_prob, sm_prob, pd_coords, sm_coords, nullptr);
}

int jcm_eval_forward(jcm_handle h, const float* x, const float* y, int B, int H, int W, int use_sm,
                     float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords, float* losses) {
  if (!y || !losses) return fail(JCM_ERR_ARG, "eval_forward needs the target heat maps y [B,60,90,K+1] and a 2-float loss buffer");
  return forward_impl(h, x, false, nullptr, y, B, H, W, use_sm, pd_prob, sm_prob, pd_coords, sm_coords, losses);
}
int jcm_eval_forward_u8(jcm_handle h, const uint8_t* x, const float* y, int B, int H, int W, int use_sm,
                        float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords, float* losses) {
  if (!y || !losses) return fail(JCM_ERR_ARG, "eval_forward needs the target heat maps y [B,60,90,K+1] and a 2-float loss buffer");
  return forward_impl(h, x, true, nullptr, y, B, H, W, use_sm, pd_prob, sm_prob, pd_coords, sm_coords, losses);
}

int jcm_window_resize(jcm_handle h, const float* src, int nsrc, int H, int W, int C, const int32_t* windows, int NW,
                      int OH, int OW, float* out) {
  JCM_TRY(check(h, false));
  if (!src || !windows || !out || nsrc < 1 || H < 1 || W < 1 || C < 1 || NW < 1 || OH < 1 || OW < 1)
    return fail(JCM_ERR_ARG, "bad window_resize arguments");
  for (int i = 0; i < NW; ++i) {
    const int32_t* w = windows + i * 5;
    if (w[0] < 0 || w[0] >= nsrc || w[3] < 1 || w[4] < 1) return fail(JCM_ERR_ARG, "bad window " + std::to_string(i));
  }
  DeviceGuard g(h->device);
  CallOrder order(h);
  jcm_ctx* c = h;
  return with_arena(c, [&] {
    int* wdev = arena_alloc<int>(c, (size_t)NW * 5);
    float2* mm = arena_alloc<float2>(c, NW);
    if (c->dry) return (int)JCM_OK;
    HIP_TRY(hipMemcpyAsync(wdev, windows, (size_t)NW * 5 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(window_resize(src, H, W, C, wdev, NW, mm, OH, OW, out, c->stream));
    order.release();
    HIP_TRY(hipStreamSynchronize(c->stream));   // `windows` is caller-owned host memory
    return (int)JCM_OK;
  });
}

int jcm_group_mean(jcm_handle h, const float* in, int n, int G, int64_t M, float* out) {
  JCM_TRY(check(h, false));
  if (!in || !out || n < 1 || G < 1 || M < 1) return fail(JCM_ERR_ARG, "bad group_mean arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(group_mean(in, out, n, G, (size_t)M, h->stream));
  return JCM_OK;
}

int jcm_profile_read(jcm_handle h, const char* scope, double* total_ms, int* launches) {
  JCM_TRY(check(h, false));
  if (!scope || !total_ms || !launches) return fail(JCM_ERR_ARG, "bad profile_read arguments");
  DeviceGuard g(h->device);
  HIP_TRY(hipStreamSynchronize(h->stream));
  double tot = 0;
  int n = 0;
  auto it = h->prof.find(scope);
  if (it != h->prof.end()) {
    for (auto& ev : it->second) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ev.first, ev.second));
      tot += ms;
      ++n;
      h->event_pool.push_back(ev.first);
      h->event_pool.push_back(ev.second);
    }
    h->prof.erase(it);
  }
  *total_ms = tot;
  *launches = n;
  return JCM_OK;
}

int jcm_conv_kernel_name(jcm_handle h, const char* scope, int B, int H, int W, char* name, int cap) {
  JCM_TRY(check(h, true));
  if (!scope || !name || cap < 2 || B < 1 || H < 1 || W < 1) return fail(JCM_ERR_ARG, "bad conv_kernel_name arguments");
  const ConvLayer* L = conv_of(h, scope);
  if (!L) return fail(JCM_ERR_STATE, std::string("no conv layer '") + scope + "'");
  const char* k;
  if (L->cin == 3) {      // H x W: the sub-sampled image; the fused kernels where the tower takes them (conv1_pool_stage), the generic one otherwise
    k = !conv1_pool_fused(h, L, H, W) ? "conv1_5x5s2_kernel"
        : h->precision == JCM_PRECISION_BF16 ? "conv1_mfma_pool_kernel" : conv1_split_route(h, L) ? "conv1_mfma_pool_split_kernel" : "conv1_mfma_pool_f32_kernel";
  } else {
    k = conv_kernel_name(h, L, B, H, W);      // the route choice of the launch (conv_route.hip)
  }
  std::snprintf(name, (size_t)cap, "%s", k);
  return JCM_OK;
}

int64_t jcm_workspace_bytes(jcm_handle h) { return h ? (int64_t)(h->arena_cap + h->side.arena_cap + h->param_bytes) : 0; }

}  // extern "C"
