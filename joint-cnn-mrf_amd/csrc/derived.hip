// Everything the library derives from the parameter store: packed weights, folded BatchNorm, the spatial model's tables (refresh_derived).
// Host code only.
#include <string>
#include <vector>

#include "ctx.h"

namespace jcm {

// Inference BatchNorm folded to y = x*scale + shift:  scale = gamma*rsqrt(var+eps), shift = beta-mean*scale.
// Buffers are allocated on the first call and rewritten in place afterwards (training refresh).
int fold_bn(jcm_ctx* c, const std::string& scope, int n, float** scale, float** shift) {
  const Tensor* t[4];
  static const char* const kNames[4] = {"gamma", "beta", "moving_mean", "moving_variance"};
  for (int i = 0; i < 4; ++i) {
    const std::string name = scope + "/BatchNorm/" + kNames[i];
    t[i] = find(c, name);
    if (!t[i]) return fail(JCM_ERR_STATE, "missing parameter '" + name + "'");
    if (t[i]->n != (size_t)n) return fail(JCM_ERR_STATE, "parameter '" + name + "' has " + std::to_string(t[i]->n) + " elements, expected " + std::to_string(n));
  }
  if (!*scale) JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(scale), n * sizeof(float)));
  if (!*shift) JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(shift), n * sizeof(float)));
  HIP_TRY(bn_fold(t[0]->d, t[1]->d, t[2]->d, t[3]->d, kBnEps, *scale, *shift, n, c->stream));
  return JCM_OK;
}

// fp16x3: {Sw, 1/Sw} with Sw the power of two that brings max|w| just below 2^14 (device scalars, recomputed at every refresh)
static int weight_scale(jcm_ctx* c, const Tensor& w, float** wscale) {
  if (!c->scale_scratch) {
    JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->scale_scratch), 1024 * sizeof(float)));
    JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->act_scale), 2 * sizeof(float)));
  }
  if (!*wscale) JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(wscale), 2 * sizeof(float)));
  HIP_TRY(pow2_scale_of(w.d, w.n, *wscale, c->scale_scratch, c->stream));
  return JCM_OK;
}

int refresh_derived(jcm_ctx* c, bool first) {
  fft_cache_invalidate(c);     // filter spectra follow the weights: recomputed on next use
  // ---- conv layers: every "<scope>/weights" of rank 4
  for (auto& kv : c->params) {
    const std::string& name = kv.first;
    const std::string suffix = "/weights";
    if (name.size() <= suffix.size() || name.compare(name.size() - suffix.size(), suffix.size(), suffix) != 0) continue;
    const Tensor& w = kv.second;
    if (w.shape.size() != 4 || w.shape[0] != w.shape[1]) return fail(JCM_ERR_ARG, "'" + name + "' must be [k,k,Cin,Cout]");
    const std::string scope = name.substr(0, name.size() - suffix.size());
    ConvLayer L;
    if (!first) {
      auto it = c->convs.find(scope);
      if (it == c->convs.end()) return fail(JCM_ERR_STATE, "conv layer '" + scope + "' appeared after jcm_finalize");
      L = it->second;
    }
    L.ks = (int)w.shape[0]; L.cin = (int)w.shape[2]; L.cout = (int)w.shape[3];
    L.w_raw = w.d;
    const Tensor* b = find(c, scope + "/biases");
    if (!b || b->n != (size_t)L.cout) return fail(JCM_ERR_STATE, "missing or mis-sized '" + scope + "/biases'");
    L.bias = b->d;
    L.has_bn = find(c, scope + "/BatchNorm/gamma") != nullptr;
    if (L.has_bn) JCM_TRY(fold_bn(c, scope, L.cout, &L.scale, &L.shift));
    if ((L.ks == 5 || L.ks == 9) && L.cin % 16 == 0 && c->precision == JCM_PRECISION_F32) {
      L.thin = L.ks == 9 && L.cout <= 12;            // logits layer: 4x4x1_16b MFMA kernel, channels padded to 16
      const int bn = L.thin ? 16 : conv_igemm_bn(L.cout);
      L.coutp = (L.cout + bn - 1) / bn * bn;
      const size_t n = (size_t)L.ks * L.ks * L.cin * L.coutp;
      if (!L.wp) JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&L.wp), n * sizeof(float)));
      // after a weight update (training step) the packing waits until a direct kernel reads it: layers on the frequency-domain route never do
      if (first) HIP_TRY(pack_weights_f32(w.d, L.wp, L.ks, L.cin, L.cout, L.coutp, c->stream));
      else L.wp_stale = true;
    }
    if (c->precision == JCM_PRECISION_F32 && c->f32_conv == 2 && (L.ks == 9 || L.ks == 5) && L.cin % 16 == 0 && L.cout % 128 == 0) {
      const int ns = 2;      // operand parts of the direct split kernels: two fp16 parts, three products (fp16x3)
      L.coutp_split = L.cout;
      if (!L.wp_split) JCM_TRY(dev_alloc(c, &L.wp_split, conv_split_weight_bytes(L.ks, L.cin, L.coutp_split, ns)));
      JCM_TRY(weight_scale(c, w, &L.wscale));
      HIP_TRY(pack_weights_split(w.d, L.wp_split, L.ks, L.cin, L.cout, L.coutp_split, ns, c->stream, L.wscale));
    }
    if (c->precision == JCM_PRECISION_F32 && c->f32_conv == 2 && L.ks == 9 && L.cout <= 16 && L.cin % 32 == 0) {   // logits layer, fp16x3
      L.coutp_split = 16;
      if (!L.wp_split) JCM_TRY(dev_alloc(c, &L.wp_split, conv_split_weight_bytes(L.ks, L.cin, 16, 2)));
      JCM_TRY(weight_scale(c, w, &L.wscale));
      HIP_TRY(pack_weights_split(w.d, L.wp_split, L.ks, L.cin, L.cout, 16, 2, c->stream, L.wscale));
    }
    if (L.ks == 5 && L.cin == 3 && L.cout == 64 && L.has_bn && c->precision == JCM_PRECISION_F32) {
      if (!L.wq1_f32) JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&L.wq1_f32), 5 * 16 * 64 * sizeof(float)));
      HIP_TRY(pack_conv1_f32(w.d, L.wq1_f32, c->stream));
      if (!L.wq1_split) JCM_TRY(dev_alloc(c, &L.wq1_split, conv1_split_weight_bytes()));
      HIP_TRY(pack_conv1_split(w.d, L.wq1_split, c->stream));
    }
    if (L.ks == 5 && L.cin == 3 && L.cout == 64 && L.has_bn && c->precision == JCM_PRECISION_BF16) {
      if (!L.wq1_bf16) JCM_TRY(dev_alloc(c, &L.wq1_bf16, 5 * 2 * 64 * 16));
      HIP_TRY(pack_conv1_bf16(w.d, L.wq1_bf16, c->stream));
    }
    if ((L.ks == 5 || L.ks == 9) && c->precision == JCM_PRECISION_BF16 && L.cin != 3) {
      if (L.cin % 32 != 0) return fail(JCM_ERR_ARG, "bf16 path needs Cin % 32 == 0 ('" + scope + "' has " + std::to_string(L.cin) + ")");
      L.thin_bf16 = L.ks == 9 && L.cout <= 16 && !L.has_bn;   // logits layer: 16x16x32 MFMA kernel, fp32 out
      const int bn = L.thin_bf16 ? 16 : conv_igemm_bf16_bn(L.cout, L.ks);
      L.coutp_bf16 = (L.cout + bn - 1) / bn * bn;
      const size_t n = (size_t)L.ks * L.ks * L.cin * L.coutp_bf16;
      if (!L.wp_bf16) JCM_TRY(dev_alloc(c, &L.wp_bf16, n * 2));
      HIP_TRY(pack_weights_bf16(w.d, L.wp_bf16, L.ks, L.cin, L.cout, L.coutp_bf16, c->stream));
      if (L.thin_bf16 && L.cout == 9) {              // the logits layer's second packing: kernel columns folded into N
        if (!L.wp_kxfold) JCM_TRY(dev_alloc(c, &L.wp_kxfold, conv_kxfold_weight_bytes(L.cin)));
        HIP_TRY(pack_weights_kxfold(w.d, L.wp_kxfold, L.cin, c->stream));
      }
    }
    c->convs[scope] = L;
  }
  // ---- spatial model tables (main.py:477-487): pairs in graph order
  if (find(c, "bn_sm/BatchNorm/gamma")) {
    const int P = c->K * (kC - 1);
    JCM_TRY(fold_bn(c, "bn_sm", kC, &c->bn_sm_scale, &c->bn_sm_shift));
    if (first) {
      JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->sp_energy), (size_t)P * kPrH * kPrW * sizeof(float)));
      JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->sp_bias), (size_t)P * kHmHW * sizeof(float)));
      JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->cond), (size_t)P * sizeof(int)));
      JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->prior_spec_t), (size_t)P * kSpec * sizeof(float2)));
    }
    if (first) {
      std::vector<int> cond(P);
      std::vector<const float*> ep(P), bp(P);
      int p = 0;
      for (int j = 0; j < c->K; ++j) {
        for (int cc = 0; cc < kC; ++cc) {
          if (cc == j) continue;
          const std::string key = std::string(kJointNames[j]) + "_" + kJointNames[cc];
          const Tensor* e = find(c, "energy_" + key);
          const Tensor* bi = find(c, "bias_" + key);
          if (!e || e->n != (size_t)kPrH * kPrW) return fail(JCM_ERR_STATE, "missing or mis-sized 'energy_" + key + "' (want [1,120,180,1])");
          if (!bi || bi->n != (size_t)kHmHW) return fail(JCM_ERR_STATE, "missing or mis-sized 'bias_" + key + "' (want [1,60,90,1])");
          ep[p] = e->d;
          bp[p] = bi->d;
          cond[p++] = cc;
        }
      }
      JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->energy_ptrs), P * sizeof(float*)));
      JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->bias_ptrs), P * sizeof(float*)));
      HIP_TRY(hipMemcpyAsync(c->cond, cond.data(), P * sizeof(int), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(c->energy_ptrs, ep.data(), P * sizeof(float*), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(c->bias_ptrs, bp.data(), P * sizeof(float*), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));   // the tables are stack-local
    }
    HIP_TRY(sm_softplus5_multi(c->energy_ptrs, c->sp_energy, P, (int64_t)kPrH * kPrW, c->stream));   // main.py:120
    HIP_TRY(sm_softplus5_multi(c->bias_ptrs, c->sp_bias, P, kHmHW, c->stream));                        // main.py:122
    HIP_TRY(sm_lds_fwd_frames(c->sp_energy, c->prior_spec_t, P, c->stream));      // [pair][91][120]: the layout every consumer reads
    c->has_sm = true;
  }
  if (first) {
    JCM_TRY(dev_alloc(c, reinterpret_cast<void**>(&c->cond0), sizeof(int)));
    HIP_TRY(hipMemsetAsync(c->cond0, 0, sizeof(int), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return JCM_OK;
}

}  // namespace jcm
