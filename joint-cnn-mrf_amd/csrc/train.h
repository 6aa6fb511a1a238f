// The training state of a handle (jcm_ctx::train), shared by jcm_train.hip (the step: layer passes, windows, losses and gradients) and
// train_state.hip (its construction, the optimizer, the state and parameter-layout entry points).  Not part of the ABI.
#pragma once
#include "ctx.h"

namespace jcm {

struct BnSave {
  float* mean = nullptr;   // [C] batch mean
  float* rstd = nullptr;   // [C] 1/sqrt(biased var + eps)
};

struct DgradW {
  float* wd = nullptr;     // packed flipped/transposed weights for conv_igemm_f32
  void* wd_split = nullptr;  // the same in two fp16 parts for conv_split_f32 (handles with f32_conv = 2)
  void* wd_bf16 = nullptr;   // bf16 handles: packed for conv_igemm_bf16
  int cinp_bf16 = 0, coutp_bf16 = 0;
  bool stale = true;       // packed before the last weight update
  int cinp = 0;            // dZ channel stride the kernel reads (= Cout rounded up to 16)
  int coutp = 0;           // packed N extent (= Cin rounded up to the kernel's N tile)
};

struct Slot {
  std::string name;
  float* w;
  size_t n, off;
};

struct TrainState {
  std::vector<Slot> slots;             // trainable tensors, sorted by name
  std::map<std::string, size_t> index; // name -> slot
  size_t total = 0;
  float* opt_m = nullptr;              // Adam m / momentum accumulator, flat [total]
  float* opt_v = nullptr;              // Adam v, flat [total]
  float* ones = nullptr;               // [maxC] identity epilogue scale
  float* zeros = nullptr;              // [maxC]
  std::map<std::string, DgradW> dgrad;
  std::map<std::string, BnSave> bn;
  float* scratch_flip = nullptr;       // largest flipped HWIO weight
  size_t scratch_flip_n = 0;           // ... its size in floats
  double* red = nullptr;               // per-channel reduction scratch
  double* sumsq = nullptr;             // [2]: grad sum of squares, weight sum of squares (l2)
  bool grad_sumsq_valid = false;       // sumsq[0] holds the norm of a jcm_train_apply (summary.hip reads it)
  float* small = nullptr;              // [2*maxC + 64] misc
  // spatial model: per-pair parameter pointers / flat-gradient offsets, graph order
  const float** e_ptr = nullptr;
  const float** b_ptr = nullptr;
  int64_t* e_off = nullptr;
  int64_t* b_off = nullptr;
  float* gscale = nullptr;             // [2] {S, 1/S}: power-of-two scale of the current layer's gradient (f32_conv = 2; DzHandover::gscale_set: of which dz)
  float* gscratch = nullptr;           // [1024]
  // "these gradients are final" notifications (jcm_train_set_grad_callback): name prefix -> [offset, count) of the flat buffer
  jcm_grad_ready_fn ready_fn = nullptr;
  void* ready_user = nullptr;
  std::map<std::string, std::pair<int64_t, int64_t>> ranges;
  // optimizer chunk table (one launch updates every tensor)
  float** ck_w = nullptr;
  int64_t* ck_start = nullptr;
  int64_t* ck_off = nullptr;
  int* ck_len = nullptr;
  int* ck_isw = nullptr;               // the chunk belongs to a '<scope>/weights' tensor (weight decay, main.py:195-205)
  int n_chunks = 0;
  int maxC = 0;
  long step = 0;                       // optimizer updates applied (n_iters, main.py:491)
};

// ---- one conv layer in training mode: r = relu(conv + b) [or conv + b], batch stats, y = BN(r)
struct LayerFwd {
  std::string scope;
  const ConvLayer* L = nullptr;
  const void* in = nullptr;    // input activation (stride-1 layers) or the fp32 image (conv1)
  int H = 0, W = 0;            // output map
  void* r = nullptr;
  void* y = nullptr;
  void* xs = nullptr;          // fp32 handles, frequency-domain layers: the split spectra of the input, kept for the weight gradient (wgrad_fft.hip)
  float* xs_tmax = nullptr;    // ... and the device word of their fp16 scaling (np = 4)
  WinGeom win;                 // (kernels.h) the layer ran on overlap-save windows of kWin x kWin (jcm_train.hip): xs are the WINDOWS' spectra
};

inline int need_train(jcm_handle h) {
  JCM_TRY(check(h, true));
  if (!h->train) return fail(JCM_ERR_STATE, "jcm_train_begin has not been called");
  return JCM_OK;
}

}  // namespace jcm
