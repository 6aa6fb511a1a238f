// The training state behind include/jcm.h: its construction (jcm_train_begin), the parameter layout, clip + Adam / momentum (jcm_train_apply,
// main.py:302-309,501-506,576-577), the optimizer state of a saved session and what summary.hip reads of it.  The step itself is jcm_train.hip.
#include <cmath>
#include <cstring>

#include "train.h"

using namespace jcm;

namespace {

bool ends_with(const std::string& s, const char* suf) {
  const size_t n = std::strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}
bool trainable(const std::string& name) { return !ends_with(name, "moving_mean") && !ends_with(name, "moving_variance"); }

// n elements of device memory owned by the handle; a host table on the device: allocation + copy on the stream (the caller synchronises before `v` goes away)
template <class T>
int dev_array(jcm_ctx* c, T** p, size_t n) { return dev_alloc(c, reinterpret_cast<void**>(p), n * sizeof(T)); }
template <class T>
int upload(jcm_ctx* c, const std::vector<T>& v, T** dst) {
  JCM_TRY(dev_array(c, dst, v.size()));
  HIP_TRY(hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return JCM_OK;
}

}  // namespace

extern "C" {

int jcm_train_begin(jcm_handle h) {
  JCM_TRY(check(h, true));
  if (h->train) return fail(JCM_ERR_STATE, "jcm_train_begin was already called");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (h->call_depth > 1) return fail(JCM_ERR_STATE, "jcm_train_begin changes the handle's training state or parameters and cannot be called from the gradient-ready callback of the same handle");
  jcm_ctx* c = h;
  TrainState* t = new TrainState();
  c->train = t;
  for (auto& kv : c->params) {       // std::map: sorted by name
    if (!trainable(kv.first)) continue;
    t->index[kv.first] = t->slots.size();
    t->slots.push_back(Slot{kv.first, kv.second.d, kv.second.n, t->total});
    t->total += kv.second.n;
  }
  for (const Slot& sl : t->slots) {      // contiguous name-prefix ranges: "<scope>/" per layer, "bias_", "bn_sm/", "energy_"
    std::string pre;
    if (sl.name.compare(0, 5, "bias_") == 0) pre = "bias_";
    else if (sl.name.compare(0, 7, "energy_") == 0) pre = "energy_";
    else pre = sl.name.substr(0, sl.name.find('/') + 1);
    auto it = t->ranges.find(pre);
    if (it == t->ranges.end()) t->ranges[pre] = {(int64_t)sl.off, (int64_t)sl.n};
    else if (it->second.first + it->second.second == (int64_t)sl.off) it->second.second += (int64_t)sl.n;
    else return fail(JCM_ERR_STATE, "gradient range of '" + pre + "' is not contiguous");
  }
  size_t max_w = 0;
  for (auto& kv : c->convs) {
    const ConvLayer& L = kv.second;
    if (L.cout > t->maxC) t->maxC = L.cout;
    if (L.cin > t->maxC) t->maxC = L.cin;
    if (L.cin == 3) continue;        // conv1: no data gradient (the image is the input)
    if (L.cin % 16 || !(L.ks == 5 || L.ks == 9)) return fail(JCM_ERR_ARG, "no training kernels for layer '" + kv.first + "'");
    DgradW d;
    d.cinp = (L.cout + 15) / 16 * 16;
    const int bn = conv_igemm_bn(L.cin);
    d.coutp = (L.cin + bn - 1) / bn * bn;
    if (c->precision == JCM_PRECISION_BF16) {
      if (L.cin % 32) return fail(JCM_ERR_ARG, "bf16 training needs Cin % 32 == 0 ('" + kv.first + "')");
      d.cinp_bf16 = (L.cout + 31) / 32 * 32;
      const int bnb = conv_igemm_bf16_bn(L.cin, L.ks);
      d.coutp_bf16 = (L.cin + bnb - 1) / bnb * bnb;
      JCM_TRY(dev_alloc(c, &d.wd_bf16, (size_t)L.ks * L.ks * d.cinp_bf16 * d.coutp_bf16 * 2));
    } else {
      JCM_TRY(dev_array(c, &d.wd, (size_t)L.ks * L.ks * d.cinp * d.coutp));
      if (c->f32_conv == 2 && L.cin % 128 == 0)      // data gradient on the fp16x3 split kernel where its tile fits
        JCM_TRY(dev_alloc(c, &d.wd_split, conv_split_weight_bytes(L.ks, d.cinp, L.cin, 2)));
    }
    // the flipped filter's dz stride: cinp (direct kernels), cinp_bf16, or -- fp32 handles, frequency-domain data gradient -- a dz widened to 64
    // channels (the logits path: Cout % 16 != 0, or conv6 with its 16-channel stride), which conv_dgrad flips for with CoP = 64
    int cop = d.cinp_bf16 > d.cinp ? d.cinp_bf16 : d.cinp;
    if (c->precision == JCM_PRECISION_F32 && cop < 64) cop = 64;
    const size_t nf = (size_t)L.ks * L.ks * cop * L.cin;
    if (nf > max_w) max_w = nf;
    t->dgrad[kv.first] = d;
  }
  if (t->maxC < 16) t->maxC = 16;
  JCM_TRY(dev_array(c, &t->scratch_flip, max_w));
  t->scratch_flip_n = max_w;
  JCM_TRY(dev_array(c, &t->opt_m, t->total));
  JCM_TRY(dev_array(c, &t->opt_v, t->total));
  HIP_TRY(hipMemsetAsync(t->opt_m, 0, t->total * sizeof(float), c->stream));
  HIP_TRY(hipMemsetAsync(t->opt_v, 0, t->total * sizeof(float), c->stream));
  {
    const std::vector<float> one(t->maxC, 1.0f);
    JCM_TRY(upload(c, one, &t->ones));
    JCM_TRY(dev_array(c, &t->zeros, t->maxC));
    HIP_TRY(hipMemsetAsync(t->zeros, 0, t->maxC * sizeof(float), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  for (auto& kv : c->convs) {
    if (!kv.second.has_bn) continue;
    BnSave& s = t->bn[kv.first];
    JCM_TRY(dev_array(c, &s.mean, kv.second.cout));
    JCM_TRY(dev_array(c, &s.rstd, kv.second.cout));
  }
  if (c->has_sm) {
    BnSave& s = t->bn["bn_sm"];
    JCM_TRY(dev_array(c, &s.mean, kC));
    JCM_TRY(dev_array(c, &s.rstd, kC));
    const int P = c->K * (kC - 1);
    std::vector<const float*> ep(P), bp(P);
    std::vector<int64_t> eo(P), bo(P);
    int p = 0;
    for (int j = 0; j < c->K; ++j)
      for (int cc = 0; cc < kC; ++cc) {
        if (cc == j) continue;
        const std::string key = std::string(kJointNames[j]) + "_" + kJointNames[cc];
        ep[p] = find(c, "energy_" + key)->d;
        bp[p] = find(c, "bias_" + key)->d;
        eo[p] = (int64_t)t->slots[t->index["energy_" + key]].off;
        bo[p] = (int64_t)t->slots[t->index["bias_" + key]].off;
        ++p;
      }
    JCM_TRY(upload(c, ep, &t->e_ptr));
    JCM_TRY(upload(c, bp, &t->b_ptr));
    JCM_TRY(upload(c, eo, &t->e_off));
    JCM_TRY(upload(c, bo, &t->b_off));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  {
    constexpr int64_t kChunk = 16384;
    std::vector<float*> cw;
    std::vector<int64_t> cs, co;
    std::vector<int> cl, cf;
    for (const Slot& sl : t->slots)
      for (int64_t st0 = 0; st0 < (int64_t)sl.n; st0 += kChunk) {
        cw.push_back(sl.w); cs.push_back(st0); co.push_back((int64_t)sl.off);
        cf.push_back(sl.name.find("weights") != std::string::npos ? 1 : 0);
        cl.push_back((int)((int64_t)sl.n - st0 < kChunk ? (int64_t)sl.n - st0 : kChunk));
      }
    t->n_chunks = (int)cw.size();
    JCM_TRY(upload(c, cw, &t->ck_w));
    JCM_TRY(upload(c, cs, &t->ck_start));
    JCM_TRY(upload(c, co, &t->ck_off));
    JCM_TRY(upload(c, cl, &t->ck_len));
    JCM_TRY(upload(c, cf, &t->ck_isw));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  JCM_TRY(dev_array(c, &t->gscale, 2));
  JCM_TRY(dev_array(c, &t->gscratch, 1024));
  JCM_TRY(dev_array(c, &t->red, train_reduce_scratch_doubles(t->maxC)));
  JCM_TRY(dev_array(c, &t->sumsq, 2));
  JCM_TRY(dev_array(c, &t->small, (size_t)(2 * t->maxC + 64)));
  return JCM_OK;      // (every packed data-gradient filter starts stale: DgradW::stale)
}

int jcm_train_param_count(jcm_handle h, int64_t* n_tensors, int64_t* n_elements) {
  JCM_TRY(need_train(h));
  if (n_tensors) *n_tensors = (int64_t)h->train->slots.size();
  if (n_elements) *n_elements = (int64_t)h->train->total;
  return JCM_OK;
}

int jcm_train_param_info(jcm_handle h, int64_t index, char* name, int name_cap, int64_t* offset, int64_t* count) {
  JCM_TRY(need_train(h));
  if (index < 0 || index >= (int64_t)h->train->slots.size()) return fail(JCM_ERR_ARG, "parameter index out of range");
  const Slot& s = h->train->slots[(size_t)index];
  if (name) {
    if ((int)s.name.size() + 1 > name_cap) return fail(JCM_ERR_ARG, "name buffer too small");
    std::memcpy(name, s.name.c_str(), s.name.size() + 1);
  }
  if (offset) *offset = (int64_t)s.off;
  if (count) *count = (int64_t)s.n;
  return JCM_OK;
}


int jcm_train_apply(jcm_handle h, const float* grads, int optimizer, float lr, float clip_norm, float* grad_norm_out) {
  JCM_TRY(need_train(h));
  if (!grads || !(lr >= 0.f)) return fail(JCM_ERR_ARG, "bad train_apply arguments");
  if (optimizer != JCM_OPT_ADAM && optimizer != JCM_OPT_MOMENTUM) return fail(JCM_ERR_ARG, "wrong optimizer");   // main.py:506
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (h->call_depth > 1) return fail(JCM_ERR_STATE, "jcm_train_apply changes the handle's training state or parameters and cannot be called from the gradient-ready callback of the same handle");
  jcm_ctx* c = h;
  TrainState* t = c->train;
  const bool clip = clip_norm > 0.f;
  HIP_TRY(sum_squares(grads, t->total, t->sumsq, 0, t->red, c->stream));         // tf.clip_by_global_norm (main.py:302-309)
  const long step = t->step + 1;          // n_iters advances only once the update has been enqueued (a failed launch must not move the LR schedule)
  const double b1 = 0.9, b2 = 0.999;
  const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow(b2, (double)step)) / (1.0 - std::pow(b1, (double)step)));
  if (optimizer == JCM_OPT_ADAM)
    HIP_TRY(optimizer_chunks(t->ck_w, t->ck_start, t->ck_off, t->ck_len, t->n_chunks, grads, t->opt_m, t->opt_v, clip ? t->sumsq : nullptr,
                             clip_norm, lr_t, 0.9f, 0.999f, 1e-8f, 0, c->stream));
  else
    HIP_TRY(optimizer_chunks(t->ck_w, t->ck_start, t->ck_off, t->ck_len, t->n_chunks, grads, t->opt_m, t->opt_v, clip ? t->sumsq : nullptr,
                             clip_norm, lr, 0.9f, 0.f, 0.f, 1, c->stream));
  t->step = step;
  t->grad_sumsq_valid = true;
  if (grad_norm_out) {
    double ss = 0.0;
    HIP_TRY(hipMemcpyAsync(&ss, t->sumsq, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    order.release();      // other host threads of the device go on while this one waits
    const hipError_t se = hipStreamSynchronize(c->stream);
    order.acquire();
    HIP_TRY(se);
    *grad_norm_out = (float)std::sqrt(ss);
  }
  JCM_TRY(refresh_derived(c, false));   // packed weights, folded moving statistics, softplus'd priors + spectra
  dgrad_filters_stale(c);
  return JCM_OK;
}

int jcm_train_set_grad_callback(jcm_handle h, jcm_grad_ready_fn fn, void* user) {
  JCM_TRY(need_train(h));
  h->train->ready_fn = fn;
  h->train->ready_user = user;
  return JCM_OK;
}

// Saver.save / Saver.restore of the optimizer side of the session (main.py:604,612,666 save every global variable: the
// '<var>/Adam', '<var>/Adam_1' -- or '<var>/Momentum' -- slots, beta1_power / beta2_power and n_iters).  slot 0 = first
// moment / momentum accumulator, slot 1 = second moment; same flat layout as the gradient buffer.
int jcm_train_get_state(jcm_handle h, int slot, float* out, int64_t count, int64_t* n_iters) {
  JCM_TRY(need_train(h));
  TrainState* t = h->train;
  if (slot < 0 || slot > 1 || (out && count != (int64_t)t->total)) return fail(JCM_ERR_ARG, "bad train_get_state arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (out) {
    HIP_TRY(hipMemcpyAsync(out, slot ? t->opt_v : t->opt_m, t->total * sizeof(float), hipMemcpyDefault, h->stream));
    order.release();
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  if (n_iters) *n_iters = t->step;
  return JCM_OK;
}

int jcm_train_set_state(jcm_handle h, int slot, const float* data, int64_t count, int64_t n_iters) {
  JCM_TRY(need_train(h));
  TrainState* t = h->train;
  if (slot < 0 || slot > 1 || (data && count != (int64_t)t->total) || n_iters < 0) return fail(JCM_ERR_ARG, "bad train_set_state arguments");
  DeviceGuard g(h->device);
  CallOrder order(h);
  if (data) {
    HIP_TRY(hipMemcpyAsync(slot ? t->opt_v : t->opt_m, data, t->total * sizeof(float), hipMemcpyDefault, h->stream));
    order.release();
    HIP_TRY(hipStreamSynchronize(h->stream));   // the caller may free `data` on return
  }
  t->step = (long)n_iters;
  return JCM_OK;
}

int jcm_train_steps(jcm_handle h, int64_t* n_iters) {
  JCM_TRY(need_train(h));
  if (n_iters) *n_iters = h->train->step;
  return JCM_OK;
}

}  // extern "C"

namespace jcm {
// The weights changed: the packed data-gradient filters are stale.  They are repacked where a layer's data gradient next runs on the direct
// kernels (jcm_train.hip: conv_dgrad) -- layers on the frequency-domain route never read them.
void dgrad_filters_stale(jcm_ctx* c) {
  for (auto& kv : c->train->dgrad) kv.second.stale = true;
}

const float* train_param_range(jcm_ctx* c, int64_t off, int64_t n) {
  if (!c->train || off < 0 || n < 0) return nullptr;
  for (const Slot& s : c->train->slots)
    if ((size_t)off >= s.off && (size_t)(off + n) <= s.off + s.n) return s.w + ((size_t)off - s.off);
  return nullptr;
}

const double* train_grad_sumsq(jcm_ctx* c) { return c->train && c->train->grad_sumsq_valid ? c->train->sumsq : nullptr; }

void train_destroy(jcm_ctx* c) {
  delete c->train;      // device buffers are in c->owned
  c->train = nullptr;
}
}  // namespace jcm
