/* libjcm -- C ABI of the MI355X-native joint-heat-map inference path.
 *
 * The reference (max-andr/joint-cnn-mrf) has no FFI layer: the path is four module-level
 * Python functions in main.py evaluated by TensorFlow at sess.run (main.py:280,406).  Each
 * entry point below cites the reference interface it replaces; the Python host module
 * `joint-cnn-mrf_amd/main.py` binds them through ctypes and keeps the reference's names.
 *
 * Conventions
 *   - every tensor pointer is DEVICE memory owned by the caller (a torch-ROCm allocation),
 *     fp32, dense NHWC exactly as the reference lays it out; coords are int32;
 *   - images are H rows x W cols (480 x 720, data.py:10), heat maps 60 x 90 (data.py:12);
 *   - calls enqueue asynchronously on the stream given to jcm_create and do not synchronise;
 *     one handle per (device, stream); a handle is not thread-safe by contract -- two host threads that call it anyway are SERIALISED
 *     (the handle carries a mutex for the duration of an outermost entry point; re-entry from the same thread is only possible from the
 *     gradient-ready callback, see jcm_train_set_grad_callback);
 *   - every function returns 0 on success, non-zero on error; jcm_last_error() returns a
 *     thread-local message for the last failing call;
 *   - the library owns only its packed weights, precomputed spatial-model tables and its
 *     workspace arena; all are released by jcm_destroy.
 */
#ifndef JCM_H
#define JCM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jcm_ctx* jcm_handle;

#define JCM_OK 0
#define JCM_ERR_ARG 1      /* bad shape / name / null pointer                      */
#define JCM_ERR_STATE 2    /* parameter missing, handle not finalised, ...          */
#define JCM_ERR_HIP 3      /* a HIP runtime call or kernel launch failed            */

#define JCM_PRECISION_F32 0   /* fp32 tensors; fp32-class arithmetic: by default the stride-1 layers run in the frequency domain with every fp32
                                 spectrum fed to the 16-bit matrix cores as two scaled fp16 parts (22 significant bits);
                                 "conv9_fft" = 0 selects the exact fp32 MFMA accumulation chain (v_mfma_f32_32x32x2_f32) -- the parity path */
#define JCM_PRECISION_BF16 1  /* bf16 tensors between the layers, fp32 accumulate -- the roofline path */

/* -- lifecycle --------------------------------------------------------------------------
 * Replaces tf.Session(config, graph) / sess.close (main.py:606-608,677-680). `stream` is a
 * hipStream_t (NULL = the device's default stream). */
int jcm_create(int device, void* stream, jcm_handle* out);
int jcm_destroy(jcm_handle h);
const char* jcm_last_error(void);
int jcm_abi_version(void);

/* -- options ------------------------------------------------------------------------------
 * jcm_set_option stores a value, jcm_get_option reads it back.  An unknown key or a value outside the range is JCM_ERR_ARG (nothing is
 * stored); a key marked "before" is JCM_ERR_STATE once jcm_finalize has run, every other key may be set at any time.
 * Range: a..b inclusive (no b: up to INT_MAX); a|b = these two values only; bool = any non-zero value is stored as 1.
 * Environment: the variable, read ONCE per handle by jcm_create (atoi), replaces the default; a later jcm_set_option wins over it.
 * This table is the list of options (csrc/options.h is its counterpart in the library; tests/test_gpu_options.py compares the two).
 *
 *   key                default  range     settable  environment          meaning
 *   "precision"        0        0..1      before    -                    JCM_PRECISION_* (the reference is fp32 throughout)
 *   "n_joints"         9        1..9      before    -                    K, the joints of the model (main.py:458)
 *   "f32_conv"         0        0|2       before    -                    fp32 handles: arithmetic of the direct convolution kernels (2 = fp16x3 split)
 *   "split_min_wgs"    128      0..       any       -                    "f32_conv" = 2: grids smaller than this keep the exact kernel
 *   "profile"          0        bool      any       -                    HIP events around every conv launch (jcm_profile_read)
 *   "conv9_fft"        1        bool      any       -                    stride-1 convolutions in the frequency domain where the shape allows
 *   "call_order"       1        bool      any       -                    calls of different handles on one device are ordered on the GPU
 *   "fft_single"       1        bool      any       -                    bf16 handles: one fp16 part per operand of the channel product (0 = two bf16 parts)
 *   "fft_t16"          1        bool      any       -                    bf16 handles, "fft_single" = 1: 16-bit row-transformed tensors and product spectra
 *   "fft_rows_mfma"    1        bool      any       -                    bf16 handles, 16-bit tensors: conv5's inverse row pass on the matrix cores
 *   "fft_windows"      1        bool      any       -                    fp32 training step: wide layers on 32 x 32 overlap-save windows
 *   "fft_fuse"         7        0..7      any       -                    bit 0 / 1 = hand-overs in row-transformed form across the max pool / the branch merge; bit 2 = coarse branches on a side stream
 *   "fft_tiles"        1        bool      any       JCM_FFT_TILES        fp32 handles: conv2_fullres -> pool -> conv3 as 2 x 2 tiles of the 120 x 180 map
 *   "fft_logits_rows"  1        bool      any       JCM_FFT_LOGITS_ROWS  fp32 handles: the logits layer contracts the channels on conv5's row spectra
 *   "fft_reg"          1        bool      any       JCM_FFT_REG          register-resident transform kernels where they exist (0 = the LDS kernels: A/B arm)
 *   "fft_cache_gb"     64       0..1048576  any     JCM_FFT_CACHE_GB     bound of the filter-spectra cache in GB
 *   "bf16_hpool"       1        bool      any       -                    bf16 handles: horizontal half of pool2 in conv2's epilogue
 *   "sm_algo"          3        1|3       any       -                    spatial model: 3 = every transform in LDS, 1 = direct sliding-window kernel
 *   "sm_chunk"         32       1..       any       -                    training step: images per slice of the spatial model's backward pass
 *   "micro_batch"      0        0..       any       -                    jcm_forward walks a batch in slices of this many images (0 = 256 bf16 / 64 fp32)
 *   "debug_skip"       0        0..127    any       -                    bisecting aid (jcm_pd_forward): bit i leaves launch group i out; results are then garbage
 *
 * In more detail:
 * "f32_conv"  : fp32 handles only; arithmetic of the DIRECT (not frequency-domain) convolution kernels, i.e. of every layer when
 *              "conv9_fft" = 0 and of the shapes the frequency-domain route does not take otherwise: 0 (default) = the exact fp32 MFMA
 *              chain; 2 = the stride-1 layers with Cin % 16 == 0 and Cout % 128 == 0 as two-way fp16 operand splits with three
 *              products on the 16-bit matrix cores (fp32-class error; every operand tensor -- weights, layer inputs, gradients --
 *              is lifted into the fp16 range by its own power-of-two scale first), and the frequency-domain route off: the
 *              A/B arm of that route.  (1, three bf16 parts / six products, was retired in round 5: JCM_ERR_ARG.)
 * "split_min_wgs": grids smaller than this keep the exact kernel (0 = always split).
 * "profile"  : bracket every MFMA conv launch with HIP events on the launch
 *              stream; read the totals back with jcm_profile_read.  Events come from a pool owned by the
 *              handle (created on first use, recycled by jcm_profile_read and by switching the option on,
 *              destroyed by jcm_destroy), so a profiled step only records.
 * "conv9_fft": stride-1 convolutions in the frequency domain (conv_fft*.hip: in-LDS FFTs around one complex channel
 *              product per frequency on the bf16 matrix cores with split operands, cgemm_split.hip) -- every such layer of an fp32
 *              handle, the wide 9x9 layers of a bf16 handle -- whenever the shape allows (Cin % 64 == 0, map + kernel - 1 <= 192);
 *              0 = the direct MFMA kernels.  The training step of an fp32 handle takes the same route (forward, data and weight
 *              gradients); a bf16 handle trains on the direct bf16 kernels.  Filter spectra are built per (layer, map size) on
 *              first use (11.4 GB for the full-width model on 60x90 maps; "fft_cache_gb" bounds the cache: a layer that would grow it
 *              past the bound drops every other layer's spectra first).
 *              An fp32 handle WITH TRAINING STATE holds more: a second 11.4 GB set of spectra of the flipped, transposed filters for
 *              the data gradient (both sets are repacked after every update) and up to 7.5 GB of weight-gradient scratch (the per-frequency
 *              products P and the column sums R of conv5) in the workspace arena -- about 31 GB beside the 6 GB of activations.
 * "call_order": calls of different handles on one device are ordered one after the other on the GPU -- an entry
 *              point holds a per-device lock while it enqueues, makes its stream wait for the previous call of another stream and records
 *              an event behind its last kernel -- so they may come from different host threads and streams and results do not depend on
 *              the interleaving.  0 takes the handle out of that chain (debugging: tools/determinism.py).
 * "fft_single": (bf16 handles): the channel product of the frequency-domain route on ONE fp16 part per operand -- spectra scaled
 *              by one power of two per image (derived from a rigorous bound of the spectrum, so an image's result does not depend on its batch), rounded once to fp16's 11 significant bits, one real product per multiply,
 *              32 channels per GEMM stage.  The layer's input and output tensors are bf16 (8 bits): the spectra are eight times finer.
 *              0 = two bf16 parts per operand, three products (rounds 2-3).  Changing it drops the cached filter spectra.
 *              ACCURACY CLASS of the default bf16 route (fft_single = fft_t16 = 1): 11-bit intermediates inside the wide 9x9 layers --
 *              per layer within one bf16 ulp + 1e-3 of the layer's scale of the bf16-operand oracle (7.6-8.0 % of the entries one ulp off;
 *              0.2 % with both options 0), full tower 4.3e-3 of the logit scale; arg-max agreement with the fp32 engine on 256 images
 *              97.6 % (part detector) / 96.3 % (spatial model), the same as the strict arm's 97.4 / 96.4 % and the direct bf16 MFMA
 *              kernels' 97.4 / 96.4 %, and 100 % / 99.9 % of the joints whose fp32 top-2 margin is clear of the bf16 noise
 *              (tests/test_gpu_argmax_agreement.py).
 * "fft_windows": (fp32 handles with training state): the training step runs its wide 60x90 layers (conv4_fullres, conv5 -- every
 *              layer with Cin * Cout >= 128 * 256 (round 6; 256 * 512 before) whose map has at least 1.5 x the frequencies of a window: conv3_fullres and the 30 x 45 maps of conv3_halfres / conv4_halfres too) on 32 x 32 overlap-save windows: forward, data
 *              gradient and weight gradient see 3 x 4 windows per image as a batch of 12 B images on a 32 x 32 circular transform, so the filter-sized
 *              spectra (what bounds the step at 16 images per GPU) shrink 5.8x.  0 = the 64 x 96 transform of the whole map (round 3).
 * "fft_t16"  : (bf16 handles with "fft_single" = 1): the row-transformed tensors between the row and the column passes of
 *              the frequency-domain route (half of the transform passes' HBM traffic) as complex fp16 in block floating point -- one power-of-two
 *              scale per (image, row, 64 channels) tile forward and per (image, kx, 64 channels) tile inverse, 11 significant bits like the
 *              spectra; and the product spectra between the channel GEMM and the inverse column pass as complex fp16 under a CONSTANT
 *              power-of-two shift (2^-(ceil(log2 Cin) + 14): the scaled operands bound every product, so nothing can overflow and typical
 *              entries sit fourteen binades above fp16's smallest normal number; round 5).  0 = complex fp32 for all three (round 3).
 * "fft_tiles": (fp32 handles, with "fft_fuse" bit 0): conv2 of a 120 x 180 map -> pool -> conv3 runs as 2 x 2 tiles of 60 x 90, each with its
 *              2-pixel halo in the 64 x 96 transform of the 60 x 90 maps (a quarter of the filter spectra, register transform kernels).  0 = the whole map.
 *              The tile kernels are register kernels: "fft_reg" = 0 turns the tiles off as well.
 * "fft_logits_rows": (fp32 handles without training state): the logits layer conv6 behind conv5's row-transformed hand-over (60 x 90 maps:
 *              96-point rows, at most 64 rows, at most 16 output channels) contracts the input channels and the nine vertical taps directly on the row
 *              spectra -- one fp16 matrix product per kx with K = 9 x Cin, rows outside the map read as zeros -- and runs one inverse row pass: no column
 *              passes, no padded filter spectra (58 MB of operand instead of 411 MB).  0 = conv6 as a whole frequency-domain layer.
 * "fft_reg"  : 0 = the LDS kernels instead of the register-resident transforms of csrc/conv_fft_reg_*.hip (inverse column / row passes,
 *              the bf16 forward row pass, the fused inverse + forward row pass) -- the A/B arm; results agree to fp32 rounding.
 * "fft_fuse" : (jcm_pd_forward / jcm_forward on the frequency-domain route): hand-overs in row-transformed form, ONE kernel doing the
 *              inverse row transform + bias / ReLU / BatchNorm of the producing layer, the op between the layers and the forward row transform of the
 *              consuming layer.  bit 0 (fp32 handles) = conv2 -> 2x2 max pool -> conv3: a work group owns a row pair, takes the 2x2 maximum in LDS
 *              and transforms the pooled row; neither conv2's output nor the pooled map reaches HBM.  bit 1 = conv4_fullres -> branch merge ->
 *              conv5 for the model's geometry (90-column maps, branches at 1/2 and 1/4): ((x1 + up(x2)) + up(x3)) / 3 formed in registers, x1 never
 *              reaches HBM -- fp32 handles (complex fp32 T) and bf16 handles on the one-part route (16-bit T; x1 and the merged value are rounded to
 *              bf16 exactly where the separate kernels round them: the two arms of a bf16 handle are bit-identical).  Arithmetic: the pool hand-over
 *              evaluates the separate kernels' expressions; the merge hand-over lerps the coarse branches along y first, then along x (TF lerps x
 *              first: the last fp32 bit of the coarse terms, as the register merge of bf16 handles has done since round 5), third = correctly rounded
 *              x / 3 on fp32 handles, one multiplication by RN(1/3) on bf16 handles (against the quotient: the bf16 rounding of two merged values in a
 *              million).  Bits 0 and 1 clear = the separate kernels of round 5 (A/B arm; held by the same tests).
 *              bit 2 (both precisions) = the half- and quarter-resolution branches are enqueued on a second stream of the handle (non-blocking, created at
 *              first use) and run BESIDE the full-resolution branch: the side stream waits for an event recorded at entry, and the handle's stream waits for the
 *              side stream in front of the first kernel that reads x2 / x3 (conv4_fullres with bit 1, else the merge).  The coarse branches' workspace,
 *              activations, scale words and x2 / x3 live in allocations of their own (counted by jcm_workspace_bytes), because two kernels that run at the same
 *              time must not share cache lines.  Same kernels, same arguments: results are bit-identical to bit 2 clear (tests/test_gpu_branch_streams.py).
 *              The per-layer times of "profile" then overlap and no longer add up to the step.  Same-box A/B at 64 images, three interleaved rounds: fp32 8.76-8.78 -> 8.20-8.39 ms per step (1.57 ms of
 *              coarse kernels run inside the full-resolution branch's first 2.08 ms, which stretch to 3.23 ms: both sides draw on the same HBM), bf16 at
 *              256 images 17.26-17.34 -> 17.15-17.22 ms (profiles/r10_ab_branch_streams.log, profiles/r10_branch_streams_timeline.md).
 * "fft_rows_mfma" : (bf16 handles on the one-part route with 16-bit row-transformed tensors): conv5's 96-point inverse row pass as a MATRIX
 *              PRODUCT on the matrix cores (rows_inv_mfma_kernel, conv_fft_rows_mfma.hip): T' (complex fp16) times the 96 x 98 real inverse-transform
 *              matrix held as two fp16 parts (22 significant bits: as exact as the fp32 butterflies), bias / ReLU / BatchNorm on the accumulators, planar
 *              bf16 out.  The register kernel it replaces is bound by vector-ALU issue (a 96-point transform is ~1000 scalar fp32 instructions per row
 *              and channel).  The two arms agree to fp32-level noise in front of the bf16 rounding (rms 1e-5 of the logit scale).  0 = the register kernel.
 * "bf16_hpool" : (bf16 handles): the horizontal half of the 2x2 max pool behind conv2 is taken in conv2's epilogue (a lane pair of
 *              conv5_strip_bf16_kernel is a pixel pair; even widths) and a two-row kernel finishes the pool: the full-width conv2 map is neither
 *              written nor re-read.  Bit-identical to the 2x2 pool kernel (rounding to bf16 is monotonic).  0 = the 2x2 pool kernel.
 * "sm_algo"  : the pairwise convolutions of the spatial model (main.py:83-87): 3 = every 120x180 transform in LDS,
 *              hand-written (sm_fused.hip; jcm_conv_mrf, the prior spectra and the training step's backward use the whole-frame
 *              kernels of sm_lds.hip); 1 = direct sliding-window kernel, the independent cross-check.  Both pass the same parity
 *              tests.  (Rounds 1-4 also had two rocFFT routes, 0 and 2; the library links no FFT library any more.)
 *              "sm_chunk": images per slice of the training step's spatial-model backward.
 * "torso_algo": (default 1, range 1|1, settable at any time, no environment variable) the route of jcm_torso_infer: 1 = direct sliding-window
 *              kernel.  A key with ONE value, kept so that a second route can be added without a new key; it is listed here and not as a row of
 *              the table above, whose key list tests/test_gpu_options.py pins (tests/test_gpu_torso.py holds this key's round trip).
 * "micro_batch": jcm_forward walks its batch in slices of this many images, so the workspace is
 *              sized for one slice (a rank's share of BASELINE configs[3]'s 2048 images fits).  0
 *              = 256 for bf16 handles, 64 for fp32 handles. */
int jcm_set_option(jcm_handle h, const char* key, int64_t value);
int jcm_get_option(jcm_handle h, const char* key, int64_t* value);

/* -- parameters -----------------------------------------------------------------------------
 * Replaces tf.get_variable + Saver.restore (main.py:147,153,484,487,612).  `name` is the
 * reference's TF variable name:
 *   "<scope>/weights" [k,k,Cin,Cout] HWIO      "<scope>/biases" [Cout]
 *   "<scope>/BatchNorm/{gamma,beta,moving_mean,moving_variance}" [Cout]
 *     scopes conv{1..4}_{fullres,halfres,quarterres}, conv5, conv6 (main.py:44-72), bn_sm (:112)
 *   "energy_<j>_<c>" [1,120,180,1]   "bias_<j>_<c>" [1,60,90,1]    (main.py:484,487)
 * `data` may be a host or a device pointer (fp32); the library copies it. */
int jcm_set_tensor(jcm_handle h, const char* name, const float* data, const int64_t* shape, int ndim);
/* Packs weights for the MFMA kernels, folds BatchNorm (inference mode, flag_train=False,
 * main.py:406) into per-channel scale/shift, and precomputes softplus(energy),
 * softplus(bias) (main.py:120,122 are batch-independent).  Call after the last set_tensor. */
int jcm_finalize(jcm_handle h);

/* -- part detector ----------------------------------------------------------------------------
 * conv_layer(x, size, stride, n_in, n_out, name, last_layer) (main.py:156-169):
 * BN(relu(conv_SAME(x,w)+b)), or conv+b for the last layer.  x [B,H,W,Cin] -> out
 * [B,ceil(H/s),ceil(W/s),Cout]; size and channel counts come from the stored "<scope>/weights".
 * Kernels exist for the shapes the model uses: (size 5, stride 2, Cin 3) and (size 5|9,
 * stride 1, Cin % 16 == 0); anything else returns JCM_ERR_ARG.  On a bf16 handle (stride-1 layers, Cin % 32 == 0)
 * x and out are still fp32: the input is rounded to bf16, the layer runs on the bf16 MFMA kernel the tower uses and
 * its bf16 result (fp32 for the last layer) is widened back. */
int jcm_conv_layer(jcm_handle h, const char* scope, int stride, int last_layer, const float* x, int B, int H, int W,
                   float* out);
/* pre_activ of conv_layer (main.py:160), the tensor tb.var_summary summarises: z = conv_SAME(x,w) + b in fp32, [B,ceil(H/s),ceil(W/s),Cout],
 * for ANY stored layer, with or without BatchNorm (for the last layer it equals jcm_conv_layer(..., last_layer = 1)).  fp32 handles only: a
 * bf16 handle returns JCM_ERR_ARG.  The layer takes the route jcm_conv_layer takes for it at this geometry, stand-alone, with the epilogue
 * stopped at conv + bias -- not necessarily the arm the fused tower takes, so z need not equal the tower's pre-activation bit for bit
 * (DESIGN.md 4.8).  Scope, stride (1 or 2) and sizes are checked before anything is launched; workspace arena, call order and
 * gradient-callback rule as jcm_conv_layer. */
int jcm_conv_layer_pre(jcm_handle h, const char* scope, int stride, const float* x, int B, int H, int W, float* z_out);
/* conv_layer(((x1 + up(x2)) + up(x3)) / 3) (main.py:58,67,69-71: the three branches merged, then conv5), run as the tower runs it: where the
 * layer takes the frequency-domain route its forward row pass forms the merge while it loads the rows (the merged map never reaches memory),
 * otherwise the merge kernel runs in front of the layer.  x1 [B,H,W,Cin], x2 [B,H2,W2,Cin], x3 [B,H3,W3,Cin] -> out [B,H,W,Cout]; up() =
 * tf.image.resize_images to H x W (TF-1.x legacy bilinear).  bf16 handles: fp32 at the boundary as for jcm_conv_layer.
 * Arithmetic of the merge: the generic kernels (any geometry; fp32 handles, the strict bf16 arm) lerp along x, then along y, and divide by 3 with
 * correct rounding, as TF does; the register kernel of bf16 handles for the model's geometry (90 / 45 / 23 columns, 16-bit T) lerps along y first
 * and multiplies by RN(1/3) -- the last fp32 bit of a value that is then rounded to bf16 (two merged values in a million round the other way). */
int jcm_conv_layer_merged(jcm_handle h, const char* scope, const float* x1, const float* x2, int H2, int W2, const float* x3, int H3, int W3,
                          int B, int H, int W, float* out);
/* ((x1 + up(x2)) + up(x3)) / 3 alone (main.py:58,67,69-70), by the launcher the tower calls where the merge is not formed inside conv5's forward row
 * pass: for testing the merge kernels on their own.  Device tensors of one element type, fp32 or (is_bf16 != 0) bf16; NHWC x1, out [B,H,W,C], x2
 * [B,H2,W2,C], x3 [B,H3,W3,C], or (planar != 0) planar [B][C/8][H][W][8].  The kernel follows from the arguments alone, never from the handle's
 * precision, and nothing is cast: fp32 -> upsample_merge3_kernel<float>; bf16 with C % 8 == 4 -> upsample_merge3_kernel<__bf16>; bf16 with C % 8 == 0 ->
 * upsample_merge3_bf16x8_kernel; planar -> upsample_merge3_planar_kernel.  Arithmetic: fp32, lerp along x, then along y, ((x1 + u2) + u3), a correctly
 * rounded third; a branch that already has H x W is read as it is.  JCM_ERR_ARG before any launch for a null pointer, a size < 1, C % 4 != 0, planar
 * without is_bf16 or with C % 8 != 0, or a tensor of 2^32 or more of the kernel's units (4 channels; 8 for bf16 with C % 8 == 0 and for planar). */
int jcm_upsample_merge3(jcm_handle h, const void* x1, const void* x2, int H2, int W2, const void* x3, int H3, int W3, int B, int H, int W, int C,
                        int is_bf16, int planar, void* out);
/* max_pool_layer(x, 2, 2) (main.py:172-174): 2x2/2 SAME. [B,H,W,C] -> [B,ceil(H/2),ceil(W/2),C] */
int jcm_max_pool(jcm_handle h, const float* x, int B, int H, int W, int C, float* out);
/* tf.image.resize_images(x, [OH,OW]) (main.py:51,58,60,67,89): TF-1.x legacy bilinear. */
int jcm_resize_bilinear(jcm_handle h, const float* x, int B, int H, int W, int C, int OH, int OW, float* out);
/* The front end of one branch of model(), run by the code the tower runs (one dispatch function serves both):
 *   pool1(conv1_<res>(x[:, ::sub, ::sub])) (main.py:44-45, 52-53, 61-62).  x [B,H,W,3] device, fp32 or (x_u8 != 0) bytes standing for float32(k) / float32(255);
 *   sub in {1, 2, 4}, H and W multiples of sub (the tower resizes other images instead of sub-sampling them).  out [B, ceil(ceil(H/sub/2)/2),
 *   ceil(ceil(W/sub/2)/2), Cout]: fp32 on an fp32 handle, bf16 on a bf16 handle.  Where both sub-sampled extents are multiples of 4 and the layer has 64
 *   filters this is ONE kernel of conv1_mfma.hip (conv1_mfma_pool_split_kernel on the default fp32 route, conv1_mfma_pool_f32_kernel with conv9_fft = 0 or
 *   f32_conv = 2, conv1_mfma_pool_kernel on a bf16 handle; the _u8 twins for bytes); everywhere else conv1_5x5s2_kernel followed by the 2x2 pool.
 *   jcm_conv_kernel_name(scope, B, H / sub, W / sub) names the kernel.  JCM_ERR_ARG before any launch for a bad sub, extents that sub does not divide,
 *   B outside [1, 65535] or a layer that is not 5x5, Cin = 3 with BatchNorm. */
int jcm_conv1_pool(jcm_handle h, const char* scope, const void* x, int x_u8, int B, int H, int W, int sub, void* out);
/*   pool2(conv2_<res>(p1)) (main.py:46-47, 54-55, 63-64) on a bf16 handle.  p1 [B,H,W,Cin] bf16 NHWC -> out [B,ceil(H/2),ceil(W/2),Cout] bf16 NHWC.  scope is
 *   "conv2_<res>"; "conv3_<res>" must be stored too, because the tower chooses the activation layout between the two (planar [B][C/8][H][W][8] when both run
 *   on conv5_strip_bf16_kernel) and, with option "bf16_hpool" and an even W, takes the pool's horizontal half in conv2's epilogue.  The same expressions choose
 *   here; a planar result is copied to NHWC at the end.  An fp32 handle returns JCM_ERR_STATE: there the pooled map is never materialised, conv2 hands conv3 its
 *   row-transformed input. */
int jcm_conv2_pool(jcm_handle h, const char* scope, const void* p1, int B, int H, int W, void* out);
/* model(x, n_joints) (main.py:29-74): x [B,H,W,3] -> logits [B,H/8,W/8,K]. */
int jcm_pd_forward(jcm_handle h, const float* x, int B, int H, int W, float* logits_out);

/* -- heat-map ops ------------------------------------------------------------------------------
 * spatial_softmax(hm) (main.py:212-217): softmax over the HW pixels of every (b,k) map. */
int jcm_spatial_softmax(jcm_handle h, const float* in, int B, int HW, int K, float* out);
/* conv_mrf(A, B) (main.py:77-91): A [1,120,180,1] prior, Bmaps [B,60,90,1] -> out [B,60,90,1]. */
int jcm_conv_mrf(jcm_handle h, const float* A, const float* Bmaps, int B, float* out);
/* spatial_model(heat_map) (main.py:94-125): hm10 [B,60,90,K+1] -> logits [B,60,90,K]. */
int jcm_sm_forward(jcm_handle h, const float* hm10, int B, float* logits_out);
/* get_joints_coords / argmax_hm (evaluation.py:15-24, main.py:389-397): first-occurrence
 * flat argmax per (b,k); coords[b,0,k] = row, coords[b,1,k] = col.  hm [B,HH,WW,K]. */
int jcm_argmax_coords(jcm_handle h, const float* hm, int B, int HH, int WW, int K, int32_t* coords);

/* spatial_softmax (main.py:212-217) and the arg-max of its result (evaluation.py:15-24) in one pass over the
 * logits -- the tail of the tower as jcm_forward runs it.  logits [B,HH,WW,K]; prob [B,HH,WW,K] and coords
 * [B,2,K] may each be NULL (not both). */
int jcm_softmax_argmax(jcm_handle h, const float* logits, int B, int HH, int WW, int K, float* prob, int32_t* coords);

/* det_rate (evaluation.py:15-36) as detection-rate CURVES: every joint and every radius in one launch, one pass over the targets.
 *   true[b,:,k] = first-occurrence flat arg-max of y[b,:,:,k] (the rules of jcm_argmax_coords: ties go to the lower index, a map of NaN or
 *                 -inf only gives (0,0));
 *   torso[b]    = sqrtf(dr*dr + dc*dc) between true[b,:,0] and true[b,:,7] (evaluation.py:26,29);
 *   nd[b,k]     = sqrtf(er*er + ec*ec) * 100.0f / torso[b], er / ec the row / column differences of pred and true (evaluation.py:30);
 *   hits[k*R+r] += number of images b with nd[b,k] <= radii[r] (evaluation.py:36 before the mean).
 * fp32, one correctly rounded operation per step.  A zero torso length gives inf or NaN, stored as it is and never a hit (as in TensorFlow).
 * pred_coords: device int32 [B,2,K] (row, col), as jcm_argmax_coords / jcm_forward write them; they are taken to be map coordinates and are not
 * range-checked (the squared differences are summed in 64-bit integers, which arbitrary int32 values can overflow).  y: device [B,HH,WW,C], C >= K -- the targets y_in;
 * channels >= K are ignored.  radii: HOST array of R floats, 1 <= R <= 32, passed to the kernel by value.  true_coords (device int32 [B,2,K]),
 * norm_dist (device fp32 [B,K]) and hits (device int32 [K,R], ADDED to: zero it before the first batch) may each be NULL.
 * JCM_ERR_ARG for K < 8, K > 16, C < K, C > 16, R outside 1..32 and B, HH or WW below 1; nothing is launched then. */
int jcm_det_curve(jcm_handle h, const int32_t* pred_coords, const float* y, int B, int HH, int WW, int K, int C, const float* radii, int R,
                  int32_t* true_coords, float* norm_dist, int32_t* hits);

/* Heat-map peaks: the top-P local maxima of every map, their sub-cell offsets and their scores, one launch, one pass over hm.
 * hm: device fp32 [B,HH,WW,K], probabilities or logits.  Write v(r,c) for one map and i = r*WW + c; every comparison is an IEEE fp32 one.
 *   local maximum p: v(p) > threshold, v(p) >= v(q) for every in-bounds 8-neighbour q, and v(p) > v(q) for those q whose index is below p's
 *                    (a plateau yields its first pixel only; the first-occurrence global maximum is one whenever it exceeds threshold);
 *   order:           value descending, then index ascending; the first min(P, n) are returned, so peak 0 is what jcm_argmax_coords gives
 *                    whenever count > 0;
 *   offset:          d_row = +0.25f if rows r-1 and r+1 both exist and v(r+1,c) > v(r-1,c), -0.25f if v(r+1,c) < v(r-1,c), else 0.f (border,
 *                    equal neighbours); d_col likewise along the columns.  Comparisons, not differences: +-inf in logit maps make no NaN.
 * cells: device int32 [B,K,P,2] (row, col); offsets: device fp32 [B,K,P,2] (d_row, d_col), may be NULL; scores: device fp32 [B,K,P], the bits
 * of the input; count: device int32 [B,K].  Slots at or beyond count hold cells -1, offsets 0, score 0.  NaN inputs are outside the contract.
 * JCM_ERR_ARG for P outside 1..8, B, HH, WW or K below 1 and HH * WW > 21600 (120 x 180): a larger map is refused, never truncated; nothing
 * is launched and no output is touched then. */
int jcm_hm_peaks(jcm_handle h, const float* hm, int B, int HH, int WW, int K, int P, float threshold,
                 int32_t* cells, float* offsets, float* scores, int32_t* count);

/* Pose decoding: of the P candidate cells per joint, the ONE combination with the highest spatial-model energy -- a joint MAP over P^9 poses in
 * place of nine independent arg-maxes.  Fixed geometry: 60x90 maps, 120x180 priors, 9 joints plus the torso channel, 1 <= P <= 4.
 * hm10:  device fp32 [B,60,90,10], what jcm_sm_forward takes: nine part-detector probabilities and the torso map.
 * cells: device int32 [B,9,P,2] (row, col), count: device int32 [B,9], as jcm_hm_peaks writes them (count is read clamped to 0..P; a cell of a
 *        slot below count lies in the map).
 * Write u_c(q) = softplus5(bn_sm(hm10[b,q,c])), the likelihood of the spatial-model forward (the same device expression), d = 1e-6,
 * e_{j|c} / b_{j|c} the handle's softplus'd prior [120,180] / bias [60,90] of pair <j>_<c>, (yj,xj) = cell of joint j's candidate pj, and
 * t = (yt,xt) the torso cell: the first-occurrence flat arg-max of channel 9 by the rules of jcm_argmax_coords.
 * Tables, fp32, one correctly rounded operation per step, log and softplus as the spatial model's kernels evaluate them:
 *   T[j,c,pj,pc] = log( e_{j|c}[59 + (yj - yc), 89 + (xj - xc)] * u_c(cell_c,pc) + b_{j|c}[yj,xj] + d )        j != c, both < 9
 *   V[j,p]       = log( u_j(cell_j,p) + d ) + log( e_{j|torso}[59 + (yj - yt), 89 + (xj - xt)] * u_9(t) + b_{j|torso}[yj,xj] + d )
 *   M[a,b,pa,pb] = T[a,b,pa,pb] + T[b,a,pb,pa]                                                                   a < b
 * which is the marginal energy of main.py:117-123 with every conditioning map collapsed onto its candidate cell ([59 + dy, 89 + dx] is where
 * conv_mrf reads the prior for that displacement; the 61x91 -> 60x90 resize of main.py:89 is left out: a delta has no neighbourhood to blend).
 * Entries of a slot at or beyond count are 0.
 * Search: a pose is s = (p_0 .. p_8), p_j < count[b,j]; its score is the fixed-order fp32 sum
 *   S_0 = V[0,p_0];  inc_k = (((V[k,p_k] + M[0,k,p_0,p_k]) + M[1,k,p_1,p_k]) + ..) + M[k-1,k,p_{k-1},p_k];  S_k = S_{k-1} + inc_k;  score = S_8.
 * The result is the pose of the highest score; ties go to the lexicographically smallest (p_0 .. p_8), p_0 most significant.  An image with some
 * count[b,j] == 0 has no pose: index -1, coords -1, score and score0 -inf.  NaN inputs are outside the contract.
 * Outputs (device; each may be NULL except index): index int32 [B,9], the chosen candidate per joint; coords int32 [B,2,9], its cell in the layout
 * of jcm_argmax_coords; score fp32 [B]; score0 fp32 [B], the score of the all-candidate-0 pose, i.e. of the independent arg-maxes; V fp32 [B,9,P]
 * and M fp32 [B,36,P,P], pairs (a < b) in lexicographic order.
 * JCM_ERR_ARG for P outside 1..4, B < 1 or a required pointer that is NULL, JCM_ERR_STATE before jcm_finalize or on a handle without
 * spatial-model parameters; nothing is launched and no output is touched then.  Uses the handle's workspace, like jcm_sm_forward. */
int jcm_pose_decode(jcm_handle h, const float* hm10, int B, const int32_t* cells, const int32_t* count, int P,
                    int32_t* index, int32_t* coords, float* score, float* score0, float* V, float* M);

/* -- frame sequences: a temporal edge on the heat maps of a clip -------------------------------
 * One hidden position per (sequence s, joint k), independent of every other (s, k), observed through the maps of T consecutive frames:
 * jcm_seq_filter is the causal forward filter (what an online caller runs, frame by frame or in pieces), jcm_seq_viterbi the offline most
 * probable track.  hm: device fp32 [S,T,HH,WW,K], the layout the forward writes with the frames as its batch; p_t = hm[s,t,:,:,k] widened to
 * float64.  Negative values and NaN are outside the contract.  HW = HH * WW.
 * Motion model: a separable truncated kernel with 1-D taps w_k[0 .. 2R], float64, taps: HOST [K][2R+1], one row per joint, read before the call
 * returns (it travels in kernel arguments); a uniform "anywhere" term of mass rho for misses and scene cuts: om = 1 - rho, u = rho / HW, formed
 * in float64 on the host.  Cells outside the map contribute nothing.  All arithmetic is float64, one correctly rounded operation per step,
 * evaluated as written (the library is built without contraction); there is no transcendental on the device.
 * Filter, a_{t-1} the previous belief:
 *   c(y,x) = sum over dy = -R .. R, ascending from 0.0, of w[dy+R] * a_{t-1}(y-dy, x)      terms outside the map skipped
 *   m(y,x) = sum over dx = -R .. R, ascending from 0.0, of w[dx+R] * c(y, x-dx)
 *   pred = om * m + u;   b = p_t * pred;   Z = sum of b;   a_t = b / Z
 *   Z == 0 or not finite: b = p_t, Z = sum of p_t, reset = 1; that Z == 0 as well: a_t = 1 / HW everywhere, reset = 2.
 *   Frame 0 without state_in takes the b = p_t branch with reset 0 (2 when the map is all zero); with state_in it is an ordinary frame.
 *   The order of the sum Z is the kernel's own and fixed: it depends on neither S nor T, so a clip split over several calls with the state
 *   carried gives the bits of one call.
 *   state_in / state_out: device float64 [S,K,HH,WW], the belief before frame 0 / after frame T-1 (either may be NULL; two distinct buffers).
 *   filtered: fp32 [S,T,HH,WW,K] = (float)a_t, may be NULL;  coords: int32 [S,T,2,K], the first-occurrence flat arg-max of the float64 a_t as
 *   (row, col) in the layout of jcm_argmax_coords, required;  norm: float64 [S,T,K] = the Z that a_t was divided by (0 with reset 2), may be
 *   NULL;  reset: int32 [S,T,K], may be NULL.
 * Viterbi, max-product in the probability domain (no logarithm; max is exact and order-free).  d_0 = p_0 / max p_0; for t >= 1:
 *   c(y,x) = max over dy of w[dy+R] * d_{t-1}(y-dy, x)      scanning dy ascending over the terms inside the map, a strictly greater value
 *                                                           replaces (the lowest dy wins a tie); dy*(y,x) is the winner
 *   m(y,x) = max over dx of w[dx+R] * c(y, x-dx)            likewise, dx*;   source cell = (y - dy*(y, x-dx*), x - dx*)
 *   e = max(om * m, u * D),  D = max d_{t-1}                the jump wins only when strictly greater; its source is the first-occurrence
 *                                                           flat arg-max of d_{t-1}
 *   b = p_t * e;   M = max b;   d_t = b / M
 *   M == 0 is a break: b = p_t, M = max p_t, every cell of the frame has no source, breaks = 1; that M == 0 as well: d_t = 1 everywhere,
 *   breaks = 2.  Frame 0 is handled the same way without a flag, unless its map is all zero (breaks 2).
 *   Backtrace: the end cell is the first-occurrence flat arg-max of d_{T-1}; then along the source cells; across a break the earlier segment
 *   ends at the first-occurrence arg-max of its last d.
 *   path: int32 [S,T,2,K] (row, col), required;  maxes: float64 [S,T,K] = the M that d_t was divided by (0 with breaks 2), may be NULL;
 *   breaks: int32 [S,T,K], may be NULL.
 * One work group per (s, k); the belief plane, the scratch plane and (Viterbi) the byte plane of dy* live in LDS for the whole launch, so a
 * frame costs one read of its map and no launch.  Viterbi keeps the source cell of every cell, int16 [S*K][T][HW], and one int32 per (s, k, t)
 * in the handle's workspace and walks them back in a second launch; jcm_seq_filter uses the workspace for the taps only.
 * JCM_ERR_ARG -- nothing is launched and no output is touched -- for S, T, HH, WW or K below 1, K > 16, R outside 0..16, rho outside [0,1], a
 * required pointer that is NULL, S * T * K >= 2^31, and HH * WW > 8192: two float64 planes and a byte plane must fit the 160 KB of LDS, and a
 * larger map is refused, never truncated.  jcm_seq_viterbi returns JCM_ERR_STATE, with the bytes it needs in the message, when the
 * back-pointers do not fit the workspace the device can still give; split the clip then.  Both enqueue on the handle's stream and do not
 * synchronise (growing the workspace does, as for every entry point that uses it). */
int jcm_seq_filter(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                   const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out);
int jcm_seq_viterbi(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                    int32_t* path, double* maxes, int32_t* breaks);

/* -- frame sequences whose lattice moves: a whole-cell shift of the belief plane per frame ------
 * jcm_seq_filter / jcm_seq_viterbi for maps that live in a window which moves with the person (the zoom pass of a clip): every argument as
 * there, plus shift: device int32 [S,T,2] = (sy, sx), where frame t's lattice lies on frame t-1's: cell (y, x) of frame t is cell
 * (y + sy, x + sx) of frame t-1.  The previous belief seen from frame t is a'(y,x) = a_{t-1}(y + sy, x + sx), 0 where that cell lies outside
 * the map; a' is defined on every integer cell, also outside frame t's map, and the taps reach it there.  Nothing is interpolated, the planes
 * in LDS do not grow, and it is the same one copy of each recurrence (csrc/seq_scan.h), instantiated with the shift.
 * Filter:
 *   c(y,x) = sum over dy = -R .. R, ascending from 0.0, of w[dy+R] * a_{t-1}(y - dy + sy, x)      terms outside the map skipped; c is indexed
 *                                                                                                  (row of frame t, column of frame t-1)
 *   m(y,x) = sum over dx = -R .. R, ascending from 0.0, of w[dx+R] * c(y, x - dx + sx)             terms outside the map skipped
 *   pred, b, Z in the kernel's fixed order, resets, state_in / state_out and every output: exactly jcm_seq_filter.  shift[s,0] applies to the
 *   transition from state_in (state_in is in the lattice of the frame before frame 0) and is ignored when state_in is NULL; state_out is in
 *   frame T-1's lattice, coords[s,t] in frame t's own.
 * Viterbi:
 *   c(y,x) = max over dy of w[dy+R] * d_{t-1}(y - dy + sy, x),  m(y,x) = max over dx of w[dx+R] * c(y, x - dx + sx): the same ascending scans
 *   over the terms inside the map and the same tie rules (the lowest dy, then the lowest dx); a maximum over no term is 0.
 *   source cell = (y - dy*(y, x - dx* + sx) + sy, x - dx* + sx), a cell of frame t-1's lattice.  A cell with m == 0 has no source inside the
 *   map: its b is 0 unless the jump wins, and the jump's source is its source (no path passes through a cell whose b is 0).
 *   The jump, b, M, breaks and the backtrace are unchanged.  path[s,t] is in frame t's own lattice.  shift[s,0] is ignored.
 * Any int32 shift is legal.  With |sy| >= HH + R or |sx| >= WW + R no tap reaches the map: pred is u alone for the filter, and for Viterbi the
 * jump or a break takes over.  (For HH <= |sy| < HH + R the two maps share no cell, but a tap still reaches across, as the sums above say.)
 * The tap loops run over clipped bounds and never index outside the plane; no term is multiplied by zero instead of being skipped.  An all-zero
 * shift gives the bits of jcm_seq_filter / jcm_seq_viterbi.
 * JCM_ERR_ARG / JCM_ERR_STATE as for the entries above, and JCM_ERR_ARG for shift == NULL. */
int jcm_seq_filter_moving(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                          const int32_t* shift, const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset,
                          double* state_out);
int jcm_seq_viterbi_moving(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                           const int32_t* shift, int32_t* path, double* maxes, int32_t* breaks);

/* -- frame sequences centred on a per-cell motion estimate: a lattice shift per cell, not per frame --
 * jcm_seq_filter_moving / jcm_seq_viterbi_moving with the shift read per DESTINATION cell: every argument as there, except centre: device int32
 * [S,T,HH,WW,2] = (sy, sx), aligned to 8 bytes: cell (y, x) of frame t was cell (y + sy, x + sx) of frame t-1 -- the sign convention of shift, of
 * jcm_frame_shift's disp and of jcm_frame_flow's flow.  One table serves all K joints.  The definition is the text above, word for word, with
 * (sy, sx) = centre[s,t,y,x] where it says shift[s,t]; each component is clamped to +-(HH + R) / +-(WW + R), beyond which no tap reaches the map.
 * Filter, per cell (y, x):
 *   for dx = -R .. R ascending, x' = x - dx + sx inside [0, WW):
 *     c = sum over dy = -R .. R, ascending from 0.0, of w[dy+R] * a_{t-1}(y - dy + sy, x')      rows outside the map skipped; no row inside: c = 0.0
 *     m = m + w[dx+R] * c                                                                       from 0.0; the term is added also when c = 0.0
 *   pred = om * m + u;  b = p_t * pred;  Z in the kernel's fixed order, resets, the division, the arg-max, state_in / state_out and every output:
 *   exactly jcm_seq_filter.  centre[s,0] applies to the transition from state_in and is ignored when state_in is NULL.
 * Viterbi, per cell: c(x') = max over dy of w[dy+R] * d_{t-1}(y - dy + sy, x'), m = max over dx of w[dx+R] * c(x - dx + sx): ascending scans over the
 *   terms inside the map, a strictly greater value replaces, a maximum over no term is 0.  source cell = (y - dy* + sy, x - dx* + sx) with dy* that of
 *   the winning column; where m is not above 0 the source is the jump's; the jump wins only when strictly greater.  b, M, breaks and the backtrace
 *   are unchanged.  centre[s,0] is never read.
 * Two consequences are part of the contract: a table with the same (sy, sx) in every cell of every frame gives the bits of the *_moving entries
 * with that shift, on every output; an all-zero table gives the bits of jcm_seq_filter / jcm_seq_viterbi.
 * The transition is GATHERED per destination cell: where the table is not uniform, the mass that leaves a cell of frame t-1 does not sum to that
 * of the kernel -- two cells may be centred on the same source, a source may be nobody's centre -- so it is no stochastic matrix (as the clipped taps
 * of the entries above are none at the border).  The filter normalises every frame anyway; norm is the Z of this transition.
 * Any int32 pair is legal.  No tap outside the plane is indexed; none is multiplied by zero instead of being skipped.  Two float64 planes live in
 * LDS (Viterbi stores each source cell as it is found and keeps no byte plane); the limits are those of jcm_seq_filter all the same.
 * JCM_ERR_ARG / JCM_ERR_STATE as for jcm_seq_filter / jcm_seq_viterbi, and JCM_ERR_ARG -- nothing is launched, no output is touched -- for
 * centre == NULL or a centre that is not aligned to 8 bytes (a cell's pair is one load). */
int jcm_seq_filter_centred(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                           const int32_t* centre, const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset,
                           double* state_out);
int jcm_seq_viterbi_centred(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                            const int32_t* centre, int32_t* path, double* maxes, int32_t* breaks);

/* -- clip pose decoding: one skeleton per frame by MRF energy and motion ------------------------
 * The exact MAP over the product of the two models above: a chain of the fully connected 9-joint pose models of jcm_pose_decode, one per frame,
 * linked in time by one P x P transition table per joint.  Geometry of jcm_pose_decode: 9 joints, 1 <= P <= 4; S clips of T frames.
 * Inputs (device): V fp32 [S,T,9,P], M fp32 [S,T,36,P,P], count int32 [S,T,9] (read clamped to 0..P), cells int32 [S,T,9,P,2] -- what
 * jcm_pose_decode and jcm_hm_peaks write with B = S * T -- and tau float64 [S,T,9,P,P]: tau[s,t,j,a,b] is the log-score of joint j moving from
 * candidate a of frame t-1 to candidate b of frame t.  tau[s,0] is never read; an entry may be -inf; NaN is outside the contract.  Slots at or
 * beyond count are never read from V, M or tau.  The entry evaluates no transcendental: tau arrives ready-made.
 * State: s = (p_0 .. p_8), flat index sum p_j P^(8-j) (p_0 most significant), valid in frame t when every p_j < count[t,j].  E_t(s) is the
 * fixed-order fp32 sum S_8 of jcm_pose_decode (the same device expression, csrc/pose_score.h); -inf for a state that is not valid.
 * Recurrence, float64, one rounded operation per step, evaluated as written:
 *   frame 0, and the frame after a frame without a pose:  D_t(s) = (double)E_t(s)
 *   t >= 1: G = D_{t-1}; for j = 0, 1, .. 8 in that order
 *     G'(.., b_j, ..) = max over a_j = 0 .. count[t-1,j]-1, ascending, of G(.., a_j, ..) + tau[t,j,a_j,b_j]
 *     a strictly greater value replaces (the lowest a_j wins a tie); the winner is the back-pointer of (t, pass j, that state); b_j >= count[t,j]:
 *     -inf.  After pass j digits 0 .. j belong to frame t and digits j+1 .. 8 to frame t-1.
 *   D_t(s) = (double)E_t(s) + G_9(s);  m_t = max D_t;  valid states become D_t - m_t, the others stay -inf;  maxes[s,t] = m_t.
 *   break 1: frame t has a valid state but m_t = -inf (no connection to frame t-1): D_t = (double)E_t, m_t the max of that, breaks = 1.
 *   break 2: some count[t,j] = 0, frame t has no pose: breaks = 2, maxes = 0, index and coords -1, frame_score -inf; the chain restarts at the
 *   next frame, which like frame 0 carries no flag of its own.
 * Backtrace: the end state is the first-occurrence flat arg-max of D_{T-1}; per frame t, descending, a_8 is pass 8's pointer at (b_0 .. b_8), a_7
 * pass 7's at (b_0 .. b_7, a_8), and so on down to a_0.  Across a break the earlier segment ends at the first-occurrence arg-max of its own last D.
 * Outputs (device; each may be NULL except index): index int32 [S,T,9], the chosen candidate per joint; coords int32 [S,T,2,9], its cell in the
 * layout of jcm_argmax_coords; frame_score fp32 [S,T], E_t of the chosen pose; maxes float64 [S,T]; breaks int32 [S,T].
 * JCM_ERR_ARG -- nothing is launched, no output is touched -- for P outside 1..4, S or T < 1, S * T >= 2^31 or a required pointer that is NULL;
 * JCM_ERR_STATE with the bytes in the message when the plane (8 P^9 bytes per clip) and the back-pointers (3 P^9 bytes per frame) do not fit the
 * workspace, as jcm_seq_viterbi refuses.  One launch on the handle's stream, one work group per clip, no synchronisation; follows call_order;
 * profiling scope seq_pose_viterbi.  There is no online form: no state is carried from call to call. */
int jcm_seq_pose_viterbi(jcm_handle h, const float* V, const float* M, const int32_t* count, const int32_t* cells, const double* tau, int S, int T,
                         int P, int32_t* index, int32_t* coords, float* frame_score, double* maxes, int32_t* breaks);

/* -- frame sequences, offline: smoothed marginals and expected transition statistics -----------
 * The third inference of the model above: gamma_t = P(x_t | all T frames) per (s, k), and from the same backward pass the posterior mass of
 * "moved" and of "jumped" and the expected squared displacement of every transition, from which sigma (per joint) and rho are re-estimated on
 * the host (Baum-Welch).  hm, taps, R, rho, om and u exactly as for jcm_seq_filter; there is no state_in: smoothing is offline.  All arithmetic
 * is float64, one correctly rounded operation per step, evaluated as written; "sum" below is the sum Z of the filter, in its order.
 * Forward: the recurrence of jcm_seq_filter, bit for bit (the library has one copy of it); norm and reset are what the filter writes, and every
 * a_t is kept as float64 [S*K][T][HW] in the handle's workspace.
 * Backward, beta_{T-1} = 1; for t = T-1 .. 0:
 *   g = a_t * beta_t;   G = sum of g;   gamma_t = g / G
 *   G == 0 or not finite: gamma_t = a_t, cut = 1, and beta_t is taken as 1 from here on back (the future is dropped)
 *   t >= 1 and reset[t] == 0, an ordinary transition, with w2[j] = (double)((j-R)*(j-R)) * w[j] and Z_t = norm[t]:
 *     q = p_t * beta_t;   Q = sum of q
 *     c(y,x)  = sum over dy = -R .. R, ascending from 0.0, of w[dy+R]  * q(y+dy, x)      terms outside the map skipped; the ADJOINT index of
 *     c2(y,x) = sum over dy = -R .. R, ascending from 0.0, of w2[dy+R] * q(y+dy, x)      the filter's, so that asymmetric taps are right
 *     m(y,x)  = sum over dx = -R .. R, ascending from 0.0, of w[dx+R]  * c(y, x+dx)
 *     sx(y,x) = sum over dx of w2[dx+R] * c(y, x+dx);   sy(y,x) = sum over dx of w[dx+R] * c2(y, x+dx);   sq = sx + sy
 *     uQ = u * Q;   beta_{t-1} = (om * m + uQ) / Z_t
 *     trans[s,t,k,:] = ( (om * sum of a_{t-1} * m) / Z_t,  uQ / Z_t,  (om * sum of a_{t-1} * sq) / Z_t ):  the posterior mass of "moved", of
 *     "jumped", and the expected squared displacement in cells^2 over the moves
 *   t >= 1 and reset[t] != 0 (frame t never saw frame t-1): beta_{t-1} = 1, trans[s,t,k,:] = 0.  trans[s,0,k,:] = 0.
 * Outputs (device):  smoothed fp32 [S,T,HH,WW,K] = (float)gamma_t, may be NULL;  coords int32 [S,T,2,K], the first-occurrence flat arg-max of
 *   the float64 gamma_t as (row, col) in the layout of jcm_argmax_coords, required;  conf fp32 [S,T,K] = (float)gamma_t at that cell;  norm
 *   float64 [S,T,K] and reset int32 [S,T,K] as jcm_seq_filter writes them;  mass float64 [S,T,K] = G, a diagnostic that is 1 in exact
 *   arithmetic;  cut int32 [S,T,K];  trans float64 [S,T,K,3], per frame -- the caller adds them up, so nothing on the device depends on T's
 *   summation order.  All but coords may be NULL.
 * One work group per (s, k) in both launches; the backward launch keeps three float64 planes in LDS for all T frames, so HH * WW <= 6144 here
 * (144 KB plus the reduction scratch of the 160 KB; 60 x 90 fits): a larger map is JCM_ERR_ARG, never truncated.  Every other refusal is that
 * of jcm_seq_filter.  JCM_ERR_STATE, with the bytes it needs in the message, when the beliefs (8 bytes per sequence, joint, frame and cell) do
 * not fit the workspace the device can still give; split the clip then.  Enqueues on the handle's stream and does not synchronise (growing the
 * workspace does). */
int jcm_seq_smooth(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho,
                   float* smoothed, int32_t* coords, float* conf, double* norm, int32_t* reset, double* mass, int32_t* cut, double* trans);

/* -- frame sequences, online: the fixed-lag smoother ------------------------------------------
 * The smoothed marginal of frame s once frame s + L has been seen: P(x_s | frames 0 .. s+L), L >= 1 frames late.  With N frames pushed so far,
 * h(s) = s + L, or min(s + L, N - 1) when the clip is flushed; frame s is emitted once h(s) <= N - 1, and its outputs are the outputs jcm_seq_smooth
 * writes for frame s when given frames 0 .. h(s) of the clip, bit for bit: smoothed, coords, conf, mass, cut, norm, reset -- the step-by-step G
 * test (cut) and the chain split at reset != 0 included.  There is no trans: the fit stays offline.
 * The library keeps no state; the caller holds the WINDOW: the P frames still pending from earlier calls followed by W - P new ones.  hm: device
 * fp32 [S,W,HH,WW,K], the maps of all W;  belief float64 [S*K][W][HH*WW], norm float64 [S,W,K] and reset int32 [S,W,K] hold in [.., :P] what the
 * earlier call wrote for those frames and are filled for frames P .. W-1.  taps, R, rho as for jcm_seq_filter.
 * Forward: the recurrence of jcm_seq_filter (the library's one copy of it) over frames P .. W-1, from belief[.., P-1]; with P == 0 as at a clip's
 *   start.  P == W: nothing new, no forward launch.
 * Emission: E = flush ? W : max(0, W - L) frames.  For e < E, beta = 1 at t = min(e + L, W - 1), then the backward step of jcm_seq_smooth (the
 *   library's one copy of it) for t down to e; frame e's outputs alone are written.  One work group per (s, k, e); E == 0 launches nothing.
 *   Afterwards the caller keeps window frames E .. W-1 as the next call's pending frames.  Any 0 <= P <= W is legal (P <= L is not required).
 * Outputs (device), for the E emitted frames:  smoothed fp32 [S,E,HH,WW,K], may be NULL;  coords int32 [S,E,2,K], required when E > 0;  conf
 *   fp32 [S,E,K], mass float64 [S,E,K], cut int32 [S,E,K], may be NULL.  norm and reset of an emitted frame are rows of the window's.
 * Any split of a clip into calls gives the same bits.  HH * WW <= 6144 as for jcm_seq_smooth.
 * JCM_ERR_ARG, nothing launched and no output touched: every refusal of jcm_seq_smooth (W in T's place, so W < 1);  P outside 0 .. W;  L < 1
 * (lag 0 is the filter: jcm_seq_filter);  flush not 0 or 1;  belief, norm or reset NULL;  coords NULL when E > 0;  S * W * K >= 2^31.
 * Enqueues on the handle's stream and does not synchronise (growing the workspace, which holds the taps and the scan's scratch, does). */
int jcm_seq_smooth_lag(jcm_handle h, const float* hm, int S, int W, int P, int HH, int WW, int K, const double* taps, int R, double rho, int L,
                       int flush, double* belief, double* norm, int32_t* reset, float* smoothed, int32_t* coords, float* conf, double* mass,
                       int32_t* cut);

/* -- camera pans: the global translation between consecutive fitted frames ---------------------
 * What turns a clip's own frames into the `shift` of jcm_seq_filter_moving / jcm_seq_viterbi_moving.  Every step is integer arithmetic; the
 * sums are order-free, so the result is a function of the bytes alone.
 * x: device uint8 [T,H,W,3], the letterboxed frames;  (y0, x0, ch, cw): the content rectangle of the fit -- no byte outside it is read, the
 * bars have no say;  D in 1..16: the coarse search radius;  prev: device uint8 [H,W,3], the frame before frame 0, or NULL.
 * Per pair (t-1, t), prev acting as frame -1:
 *   L(y,x) = R + 2 G + B                                               in 0 .. 1020
 *   C(Y,X) = the sum of L over the 4 x 4 block at (y0 + 4Y, x0 + 4X)    Y < Hc = ch / 4, X < Wc = cw / 4 (floor; trailing pixels dropped)
 *   coarse: for every (dy, dx) in [-D, D]^2   S_c = sum of |C_t(Y,X) - C_{t-1}(Y+dy, X+dx)| over Y in [D, Hc-D), X in [D, Wc-D) -- the same
 *           number of terms for every candidate;  the winner (dy_c, dx_c) minimises the tuple (S_c, dy^2 + dx^2, dy, dx)
 *   fine:   candidates (dy, dx) = (4 dy_c + ey, 4 dx_c + ex), ey, ex in [-3, 3];  S_f = sum of |L_t(y,x) - L_{t-1}(y+dy, x+dx)| over
 *           y in [y0+M, y0+ch-M), x in [x0+M, x0+cw-M), M = 4D + 3;  the winner minimises (S_f, dy^2 + dx^2, dy, dx) of the full displacement
 * Outputs (device): disp int32 [T,2] = the fine winner (dy, dx) in fitted-frame pixels;  sad int64 [T,2] = (S_f at the winner, S_f at (0,0)),
 *   both over the same window, the second computed whether or not (0,0) is a fine candidate.  With prev == NULL, disp[0] = sad[0] = (0,0).
 * Sign: the content at pixel (y,x) of frame t is at (y+dy, x+dx) of frame t-1 -- the convention of `shift` above.  Ties: two identical frames,
 *   uniform ones included, give (0,0).
 * JCM_ERR_ARG -- nothing is launched, disp and sad are untouched -- for a null x, disp or sad;  T < 1 or T > 65534;  D outside 1..16;  a
 *   rectangle that is not inside the frame;  ch or cw below 8D + 7 (the smallest at which both windows hold a pixel);  H or W above 4096
 *   (seven rows of the fine window are staged in LDS);  H * W * 1020 >= 2^32: a candidate's sum is at most H * W * 1020, and the partial
 *   sums of threads and work groups are held in 32 bits (the slots they are added into in 64).
 * Uses the workspace arena (2 bytes per frame and pixel of the rectangle, and a sixteenth of that again); JCM_ERR_STATE with the bytes in the
 * message when they do not fit.  Enqueues on the handle's stream and does not synchronise (growing the workspace does); the fine search
 * reads the coarse winner from device memory.  Timed as "frame_shift". */
int jcm_frame_shift(jcm_handle h, const uint8_t* x, int T, int H, int W, int y0, int x0, int ch, int cw, int D, const uint8_t* prev,
                    int32_t* disp, int64_t* sad);

/* -- local motion: one displacement per heat-map cell -------------------------------------------
 * Exhaustive block matching on the integer luma of jcm_frame_shift, once per heat-map cell (8 x 8 fitted-frame pixels) and reference frame.  Every
 * step is integer arithmetic and the sums are order-free, so the result is a function of the bytes alone.
 * x: device uint8 [T,H,W,3], the letterboxed frames, H and W multiples of 8;  (y0, x0, ch, cw): the content rectangle of the fit -- no byte outside
 * it is read;  D in 1..16: the search radius in pixels;  ref: DEVICE int32 [T,R], R in 1..8: slot r of frame t is matched against frame
 * s = ref[t,r]; an entry that is negative or >= T means "no such frame" (the host cannot refuse it without reading it back, so the kernel
 * treats it so).  With HH = H / 8, WW = W / 8, per (t, r) with a frame s and per cell (Y, X):
 *   L(y,x)  = R + 2 G + B                                              in 0 .. 1020
 *   block   = the 16 x 16 pixels [8Y - 4, 8Y + 12) x [8X - 4, 8X + 12)
 *   P       = the block intersected with the content rectangle: a rectangle, possibly empty
 *   (dy,dx) in [-D, D]^2 is valid when P displaced by it lies inside the content rectangle; (0,0) always is
 *   S(dy,dx) = sum over p in P of |L_t(p) - L_s(p + (dy,dx))|          at most 256 * 1020, held in 32 bits
 *   the winner minimises the tuple (S, dy^2 + dx^2, dy, dx) over the valid candidates -- the tie-break of jcm_frame_shift: a uniform block, or
 *   two identical frames, give (0,0)
 * Outputs (device): flow int32 [T,R,HH,WW,2] = the winner (dy, dx);  sad int32 [T,R,HH,WW,2] = (S at the winner, S at (0,0)).  A cell with an
 *   empty P and every cell of a slot without a frame: flow = sad = 0.
 * Sign: the content at pixel (y,x) of frame t is at (y+dy, x+dx) of frame s -- the convention of `shift` and of jcm_frame_shift's disp.
 * JCM_ERR_ARG -- nothing is launched, flow and sad are untouched -- for a null x, ref, flow or sad;  T < 1 or T > 65534;  D outside 1..16;  R
 *   outside 1..8;  H or W that is no multiple of 8, or above 4096;  a rectangle that is not inside the frame.
 * Uses the workspace arena (2 bytes per frame and pixel of the rectangle); JCM_ERR_STATE with the bytes in the message when they do not fit.
 * Enqueues on the handle's stream and does not synchronise (growing the workspace does).  Timed as "frame_flow". */
int jcm_frame_flow(jcm_handle h, const uint8_t* x, int T, int H, int W, int y0, int x0, int ch, int cw, int D, const int32_t* ref, int R,
                   int32_t* flow, int32_t* sad);

/* -- local motion: the neighbours' heat maps warped onto the frame and pooled -------------------
 * hm: device fp32 [T,HH,WW,K];  flow: device int32 [T,2N,HH,WW,2] as jcm_frame_flow writes it with slot 2(n-1) holding ref = t - n and slot
 * 2(n-1) + 1 holding ref = t + n, n = 1 .. N, N in 1..4;  w: HOST float64 [N+1].  Per (t, y, x, k), float64, one correctly rounded operation per
 * step, evaluated as written:
 *   acc = w[0] * hm[t,y,x,k];   ws = w[0]
 *   for n = 1 .. N, first s = t - n, then s = t + n; an s outside [0, T) is skipped (whatever its flow slot holds):
 *     (dy, dx) = flow[t, slot, y, x];   py = y + dy / 8,  px = x + dx / 8  (exact), clamped to [0, HH-1] and [0, WW-1]
 *     ya = floor(py), yb = min(ya + 1, HH-1), fy = py - ya;  xa, xb, fx likewise;  v_ab = (double)hm[s, y_a, x_b, k]
 *     top = (1 - fx) * v_aa + fx * v_ab;   bot = (1 - fx) * v_ba + fx * v_bb;   v = (1 - fy) * top + fy * bot
 *     acc = acc + w[n] * v;   ws = ws + w[n]
 *   out[t,y,x,k] = (float)(acc / ws)
 * The flow is a cell's own displacement in pixels, so the neighbour's map is read where the cell's content is in that frame.  With w[n] = 0 for
 * all n >= 1 out has hm's bits.  Any int32 flow is legal: the sample point is clamped.
 * JCM_ERR_ARG -- nothing is launched, out is untouched -- for sizes below 1;  K > 16;  HH * WW > 8192 (what jcm_seq_* take);  N outside 1..4;  a
 *   null pointer;  w[0] <= 0, another w[n] < 0, a w[n] that is not finite;  out overlapping hm.
 * Enqueues on the handle's stream and does not synchronise.  Timed as "hm_flow_pool". */
int jcm_hm_flow_pool(jcm_handle h, const float* hm, int T, int HH, int WW, int K, const int32_t* flow, int N, const double* w, float* out);

/* -- several tracks through single-channel maps: one torso track per person of a clip ----------
 * hm: device fp32 [S,T,HH,WW], one non-negative channel (the torso probabilities of the frames); M in 1..4 tracks; taps HOST [2R+1], R and rho as for
 * jcm_seq_* with one tap row; D in 0..64, the exclusion half-width in cells.
 * For track n = 0 .. M-1, in this order, per clip s:
 *   observation of pass n:  p(n)_t(y,x) = 0 if, for some earlier track m < n with value[s,m,t] > 0, max(|y - y_{m,t}|, |x - x_{m,t}|) <= D,
 *                           where (y_{m,t}, x_{m,t}) is track m's cell of frame t;  otherwise p(n)_t(y,x) = hm[s,t,y,x].
 *   On p(n) runs EXACTLY the recurrence of jcm_seq_viterbi (resp. jcm_seq_filter) at K = 1 as stated above: its arithmetic, tie rules,
 *   breaks / resets and backtrace (the library has one copy of it).  The track's cell of frame t is the path's (resp. the filter's arg-max).
 *   value[s,n,t] = p(n)_t at the track's cell of frame t -- so an earlier track excludes nothing in a frame where it has no support itself.
 * For n = 0 nothing is excluded: track 0 is, bit for bit, jcm_seq_viterbi / jcm_seq_filter on hm viewed as [S,T,HH,WW,1].  Identity is stable by
 * construction (a track is one run of the temporal model), and a torso that fades for a few frames is bridged by the motion model and rho.
 * Viterbi outputs (device): path int32 [S,M,T,2] (row, col), required;  maxes float64 [S,M,T], breaks int32 [S,M,T], may be NULL;  value fp32
 *   [S,M,T], required.
 * Filter outputs (device): coords int32 [S,M,T,2], required (pass n reads the cells of the passes < n of the same frames);  norm float64 [S,M,T],
 *   reset int32 [S,M,T], may be NULL;  value fp32 [S,M,T], required;  state_in / state_out float64 [S,M,HH*WW], the beliefs before frame 0 /
 *   after frame T-1, either may be NULL, two distinct buffers: a clip fed in pieces gives the bits of one call;  filtered fp32 [S,M,T,HH,WW],
 *   may be NULL.
 * The exclusion is applied while a frame is staged into LDS; no masked copy of the maps is written.  One work group per clip and pass; the
 * launches of a call follow each other on the handle's stream without a host synchronisation.  Viterbi's workspace is that of ONE pass (int16
 * per clip, frame and cell), reused by the next; JCM_ERR_STATE with the bytes it needs in the message when it does not fit.
 * JCM_ERR_ARG -- nothing is launched and no output is touched -- for what jcm_seq_* refuse (sizes below 1, R outside 0..16, rho outside [0,1],
 * HH * WW > 8192, S * T * 4 >= 2^31), M outside 1..4, D outside 0..64, and a required pointer that is NULL. */
int jcm_seq_tracks_viterbi(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int M, const double* taps, int R, double rho, int D,
                           int32_t* path, double* maxes, int32_t* breaks, float* value);
int jcm_seq_tracks_filter(jcm_handle h, const float* hm, int S, int T, int HH, int WW, int M, const double* taps, int R, double rho, int D,
                          const double* state_in, float* filtered, int32_t* coords, double* norm, int32_t* reset, double* state_out, float* value);

/* Torso map from the part detector: the torso cell that the nine part-detector maps and the nine learned priors e_{j|torso} explain best, and the
 * blob at it -- the tenth channel jcm_sm_forward needs, for an image that has no annotation.  Fixed geometry like jcm_pose_decode's:
 * HH = 60, WW = 90, K = 9, 120x180 priors.
 * prob: device fp32 [B,60,90,9], the part-detector probabilities (what jcm_forward writes as pd_prob).
 * Write a = (a_y,a_x) and t = (t_y,t_x) for cells of the map, u_j(a) = softplus5(bn_sm(prob[b,a,j])), the likelihood of the spatial-model forward
 * (the same device expression; channel j of bn_sm, the tenth BatchNorm channel is not used), e_{j|torso} the handle's softplus'd prior [120,180] of
 * pair <j>_torso, d = 1e-6, and the index convention of jcm_pose_decode ([59 + dy, 89 + dx] is where conv_mrf reads the prior for the displacement
 * joint - torso = (dy, dx)):
 *   C_j(t) = sum over the 5400 cells a of   e_{j|torso}[59 + (a_y - t_y), 89 + (a_x - t_x)] * u_j(a)                     j = 0 .. 8
 *   E(t)   = ((..(log(C_0(t) + d) + log(C_1(t) + d)) + ..) + log(C_8(t) + d))                                            fp32, this order
 * C_j is the ADJOINT of the pairwise pass of main.py:83-87, a correlation of joint j's map with its prior: the evidence the joints send to a torso
 * at t.  Every prior index lies in [0,118] x [0,178], so no padding case exists.  There is no bias term (b_{j|torso} is indexed by the joint's cell,
 * not the torso's), and the 61x91 -> 60x90 resize of main.py:89 is left out as in jcm_pose_decode.  C_j is an fp32 sum of 5400 non-negative terms
 * whose order belongs to the route (DESIGN.md 4.15 has the measured distance from float64); log as the spatial model's kernels evaluate it.
 * Outputs (device):
 *   energy fp32 [B,60,90]    E; may be NULL
 *   cell   int32 [B,2]       (row, col) of the first-occurrence arg-max of E in row-major order, by the rules of jcm_argmax_coords
 *   torso  fp32 [B,60,90,1]  the 3x3 binomial blob outer([1,2,1],[1,2,1]) / 16 that data.target_heat_maps places at `cell`, cut at the border, zeros
 *                            elsewhere; may be NULL
 * cells_in (device int32 [B,2], may be NULL): when given, no energy is formed -- prob, energy and cell are neither read nor written -- and torso
 * (required then) gets the blob at cells_in[b], each coordinate clamped into the map (0..59, 0..89) before any index is formed from it: the
 * device-side blob writer of the per-person maps (Engine.forward(torso='infer', people=M)).
 * Route: option "torso_algo", 1 = direct (an LDS-tiled sliding-window sum per (image, joint), csrc/torso_infer.hip).  It is the only value: a
 * frequency-domain route on the cached prior spectra (read conjugated) is not shipped.
 * The launches (likelihoods, correlations, log-sum + arg-max + blob) are enqueued on the handle's stream; nothing synchronises.  NaN inputs are
 * outside the contract.  JCM_ERR_ARG for another geometry, B < 1 or a required pointer that is NULL, JCM_ERR_STATE before jcm_finalize or (without
 * cells_in) on a handle without spatial-model parameters; nothing is launched and no output is touched then.  Uses the handle's workspace. */
int jcm_torso_infer(jcm_handle h, const float* prob, int B, int HH, int WW, int K, const int32_t* cells_in,
                    float* energy, int32_t* cell, float* torso);

/* -- the whole tower ----------------------------------------------------------------------------
 * The graph of main.py:522-531: model -> spatial_softmax -> concat torso -> spatial_model ->
 * spatial_softmax -> argmax.  x [B,H,W,3]; torso [B,60,90,1] = y_in[...,K:] (main.py:528),
 * may be NULL when use_sm == 0.  Any output pointer may be NULL:
 *   pd_prob, sm_prob [B,60,90,K] fp32;  pd_coords, sm_coords [B,2,K] int32. */
int jcm_forward(jcm_handle h, const float* x, const float* torso, int B, int H, int W, int use_sm,
                float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords);

/* The same tower with the two losses of the graph in inference mode -- what eval_error runs per batch
 * (main.py:275-283: sess.run([loss_pd, loss_sm, det_rate_pd, det_rate_sm], flag_train=False)).  y = y_in
 * [B,60,90,K+1] (main.py:488): its first K channels are the targets of softmax_cross_entropy (main.py:220-240,
 * 538-539), channel K the torso map.  losses: device fp32 [2] = loss_pd, loss_sm (loss_sm = loss_pd when use_sm == 0,
 * main.py:535).  The detection rates are a few [B,2,K] operations on the returned coordinates (evaluation.py). */
int jcm_eval_forward(jcm_handle h, const float* x, const float* y, int B, int H, int W, int use_sm,
                     float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords, float* losses);

/* -- byte images ----------------------------------------------------------------------
 * jcm_pd_forward, jcm_forward and jcm_eval_forward on x [B,H,W,3] uint8 (device): byte k stands for float32(k) / float32(255), correctly
 * rounded -- the value data.load_image makes of it -- and the results equal, bit for bit, those of the float entry on that float image.
 * Only the conv1 kernels read the image; their byte-source variants convert at the load.  Every other argument, micro_batch, call_order,
 * the profiling scopes and jcm_conv_kernel_name are those of the float entries.  (jcm_train_loss_grads stays float: training batches come
 * out of the gather or the augmentation below, which write fp32.) */
int jcm_pd_forward_u8(jcm_handle h, const uint8_t* x, int B, int H, int W, float* logits_out);
int jcm_forward_u8(jcm_handle h, const uint8_t* x, const float* torso, int B, int H, int W, int use_sm,
                   float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords);
int jcm_eval_forward_u8(jcm_handle h, const uint8_t* x, const float* y, int B, int H, int W, int use_sm,
                        float* pd_prob, float* sm_prob, int32_t* pd_coords, int32_t* sm_coords, float* losses);

/* -- multi-scale test-time evaluation (the caller of the tower, main.py:326-425) ---------------------
 * One pad-or-crop window per output, then skimage.transform.resize(window, [OH,OW]) with the
 * 0.13.x defaults the reference relies on (bilinear, half-pixel centres, zeros outside, clip to
 * the window's [min,max]): get_different_scales (main.py:326-348) and scale_hm_back (:351-379).
 * src [nsrc,H,W,C] device fp32; windows HOST int32 [NW][5] = (source index, y0, x0, h, w), a
 * window may extend beyond the image (= np.lib.pad with zeros); out [NW,OH,OW,C] device fp32. */
int jcm_window_resize(jcm_handle h, const float* src, int nsrc, int H, int W, int C, const int32_t* windows, int NW,
                      int OH, int OW, float* out);
/* np.average over the G scale copies of each image (main.py:413-414): in [n*G, M] -> out [n, M]. */
int jcm_group_mean(jcm_handle h, const float* in, int n, int G, int64_t M, float* out);

/* -- images of any size: the letterbox fit ------------------------------------------------
 * A ragged batch of byte images resampled, aspect preserved and antialiased, into the frame the tower reads: image b lands in the content
 * rectangle of out[b], everything else of out[b] is the byte `pad`.
 * src: ONE device buffer of src_bytes bytes holding the B images, image b = [h_b, w_b, C] uint8 in HWC order at any byte offset (no alignment
 * is assumed); desc: HOST int64 [B][3] = (byte offset, h_b, w_b), read before the call returns (it travels in the kernel arguments);
 * out: device [B,OH,OW,C], not overlapping src: uint8 (out_f32 == 0) or float32 (out_f32 != 0), each value float32(byte) / float32(255), the
 * value the byte stands for at the byte entries above; geom: HOST int32 [B][4] = (y0, x0, ch, cw), written by the call, may be NULL.
 * Geometry (integers, / is floor division), h x w into OH x OW:
 *   OH * w <= OW * h:  ch = OH,  cw = max(1, (2 * w * OH + h) / (2 * h));      otherwise:  cw = OW,  ch = max(1, (2 * h * OW + w) / (2 * w))
 *   y0 = (OH - ch) / 2,  x0 = (OW - cw) / 2;   the content rectangle is [y0, y0 + ch) x [x0, x0 + cw).
 * Resampling: a separable triangle filter whose support widens with the reduction ("bilinear with antialiasing"; plain edge-clamped bilinear
 * when enlarging), in float64, evaluated as written.  Per axis, n source samples onto m content samples:
 *   f = (double)n / (double)m,  sup = max(f, 1.0);   output o:  c = (o + 0.5) * f,  lo = max(0, (int)floor(c - sup)),  hi = min(n, (int)ceil(c + sup))
 *   t_i = max(0.0, 1.0 - fabs((i + 0.5 - c) / sup))  for i = lo .. hi - 1,   T = t_lo + .. + t_{hi-1} in ascending i,   weight_i = t_i / T.
 * A content value is acc = sum_j wy_j * (sum_i wx_i * (double)p[lo_y + j][lo_x + i][channel]): the inner sum first, ascending i from 0.0, then the
 * outer, ascending j from 0.0; the byte is min(255, max(0, (int)floor(acc + 0.5))).  A source of exactly OH x OW comes out as a bit copy.
 * JCM_ERR_ARG -- nothing is launched, out and geom are untouched -- for a null src, desc or out, B < 1, C outside 1..4, OH or OW outside 1..4096,
 * pad outside 0..255, an h_b or w_b outside 1..16384, an image whose bytes do not lie inside [0, src_bytes), a reduction above 32 on either axis
 * (h > 32 * ch or w > 32 * cw: at most 66 taps per axis), B * OH * OW * C >= 2^31, and an out that overlaps src.
 * One launch per 64 images on the handle's stream; nothing synchronises.  Uses no workspace. */
int jcm_fit_images(jcm_handle h, const uint8_t* src, int64_t src_bytes, const int64_t* desc, int B, int C,
                   int OH, int OW, int pad, int out_f32, void* out, int32_t* geom);

/* -- windows of images of any size ----------------------------------------------------------
 * jcm_fit_images applied to rectangles of the images: what a second pass over the people of a photo cuts out (predict.py: zoom).
 * src, src_bytes, C, OH, OW, pad, out_f32 are those of jcm_fit_images; desc: HOST int64 [NW][7] = (byte offset, h, w, wy0, wx0, wh, ww), read before
 * the call returns: the image [h, w, C] sits at the byte offset exactly as for jcm_fit_images, the window is its rows [wy0, wy0 + wh) and
 * columns [wx0, wx0 + ww).  wy0 and wx0 may be negative and the window may reach past any edge; several windows may name one image.
 * Let V be the [wh, ww, C] byte image with V[y][x] = image[wy0 + y][wx0 + x] where that sample exists and the byte `pad` elsewhere (np.pad, then a
 * crop).  out[i] [OH,OW,C] and geom[i] = (y0, x0, ch, cw) are exactly what jcm_fit_images gives for V: the geometry of wh x ww into OH x OW, the
 * float64 triangle filter, its summation order and its rounding, as stated above.  The pad samples of V take part in the filter like any other
 * sample.  A window (0, 0, h, w) therefore gives the bits of jcm_fit_images for that image.
 * JCM_ERR_ARG -- nothing is launched, out and geom are untouched -- for everything jcm_fit_images refuses, the size limit (1..16384) and the
 * reduction limit (32 per axis) read on wh x ww; for an image side outside 1..2^24 or image bytes outside [0, src_bytes); and for a window that
 * shares no pixel with its image (wy0 >= h, wy0 + wh <= 0, wx0 >= w or wx0 + ww <= 0).
 * One launch per 64 windows on the handle's stream (a window is 36 bytes of kernel arguments); nothing synchronises.  Uses no workspace.  The
 * work is the window's: only the rows and columns of the image that the window's filter reads are loaded, whatever the image's size. */
int jcm_fit_windows(jcm_handle h, const uint8_t* src, int64_t src_bytes, const int64_t* desc, int NW, int C,
                    int OH, int OW, int pad, int out_f32, void* out, int32_t* geom);

/* -- poses drawn onto the source images ------------------------------------------------------
 * The ragged byte batch of jcm_fit_images with C = 3 (src, src_bytes, desc HOST int64 [B][3] = (byte offset, h, w), any byte offsets) comes out
 * in `out`, a device buffer of src_bytes bytes, image b at the same offset, with two layers drawn on it.  Bytes of out that belong to no image
 * are not written.  out == src (in place) is allowed: a pixel depends on its own source pixel only; any other overlap is refused.
 * Layer 1, the heat tint (hm == NULL: off).  hm: device float32 [B,hh,hw,K], K in 1..16, finite; geom: HOST int32 [B][4] = (y0, x0, ch, cw), the fit
 * of image b into the (hh * stride) x (hw * stride) frame the maps belong to (what jcm_fit_images returns); heat_mask: HOST uint8 [K], bits 0, 1, 2
 * of entry j say that joint j tints R, G, B; heat_gain in 0..255.  M(b, j) is the maximum of map j of image b; a joint with M <= 0 adds nothing.
 * For source pixel (y, x) of an h x w image, in float64, evaluated as written:
 *   fy = ((double)y + 0.5) * (double)ch / (double)h - 0.5 + (double)y0;   cy = min(max(fy / (double)stride, 0.0), (double)(hh - 1))
 *   iy = (int)floor(cy),  iy1 = min(iy + 1, hh - 1),  ty = cy - iy;   the columns alike from x, cw, w, x0, hw
 *   s = (1 - ty) * ((1 - tx) * v00 + tx * v01) + ty * ((1 - tx) * v10 + tx * v11),   v.. = hm[b][iy | iy1][ix | ix1][j]
 *   q = min(255, max(0, floor(s * 255.0 / (double)M + 0.5))),   add = (q * heat_gain + 127) / 255 (integers)
 * and for j ascending and every channel c of heat_mask[j]: v_c = min(255, v_c + add).
 * Layer 2, capsules, on top of the tint.  prims: HOST int32 [NP][8] = (image, ay, ax, by, bx, r, rgb = 0xRRGGBB, alpha), sorted by image
 * (non-decreasing), applied within an image in listing order.  Coordinates and r are in sixteenths of a pixel; integer pixel coordinates are
 * pixel centres, so pixel (y, x) has its centre at (16 y, 16 x).  A disc is a capsule with a == b.  The coverage c of a pixel, 0..16, counts its
 * sub-samples (offsets -6, -2, +2, +6 sixteenths on each axis) inside the capsule; sample (sy, sx), in float64 from the exact integers:
 *   ey = sy - ay, ex = sx - ax, dy = by - ay, dx = bx - ax;   ee = ey*ey + ex*ex;  t = ey*dy + ex*dx;  L2 = dy*dy + dx*dx;  rr = (double)r * r
 *   L2 == 0 or t <= 0:  inside iff ee <= rr;    t >= L2:  inside iff (sy-by)*(sy-by) + (sx-bx)*(sx-bx) <= rr;    else:  inside iff ee * L2 - t * t <= rr * L2
 * and per channel, in integers, v = (v * (4080 - c * alpha) + colour * c * alpha + 2040) / 4080.  No square root, no division by a computed
 * value: a restatement in the same order gives the same bytes.
 * JCM_ERR_ARG -- nothing is launched, out is untouched -- for a null src, desc or out; B < 1; a side outside 1..16384; image bytes outside
 * [0, src_bytes); out partly overlapping src; NP < 0, or NP > 0 with null prims; an image index outside 0..B-1 or out of order; more than 256
 * primitives for one image; a coordinate outside +-2^20; r outside 0..2^16; alpha outside 0..255; rgb outside 0..0xFFFFFF; hm with a null geom or
 * heat_mask, K outside 1..16, hh, hw or stride < 1, heat_gain outside 0..255, a geom row with ch or cw < 1, or B * hh * hw * K >= 2^31.
 * desc, prims, geom and heat_mask are read before the call returns: they travel in kernel arguments (the primitives by ceil(NP / 120) small launches
 * into the handle's workspace; the map maxima by one more launch).  One launch per 64 images on the handle's stream.  The call does NOT
 * synchronise (growing the handle's workspace, first call or a larger NP, does, as for every entry point that uses it). */
int jcm_render_poses(jcm_handle h, const uint8_t* src, int64_t src_bytes, const int64_t* desc, int B, uint8_t* out,
                     const int32_t* prims, int NP,
                     const float* hm, int hh, int hw, int K, int stride, const int32_t* geom, const uint8_t* heat_mask, int heat_gain);

/* -- rendered people: a data set drawn on the device ------------------------------------------
 * out [B,H,W,3] from one scene record and one list of primitives per image: a vertical gradient with four octaves of value noise, capsules and
 * convex quadrilaterals over it in painter's order, sensor noise on top.  Everything is integer arithmetic (the capsule test: float64 products of
 * integers, exact); "floor(a / b)" is floor division, also for a negative a; ">>" on a negative value is the arithmetic shift (floor).
 * records: HOST int32 [B][JCM_SYNTH_REC_INTS = 20]:
 *   [0] seed   [1..3] c0 (R, G, B of row 0)   [4..6] c1 (of row H - 1)   [7..10] amp[o], o = 0..3   [11..14] s[o], the octave's shift: lattice cells
 *   of 1 << s[o] pixels (synth.py uses 6, 4, 2, 0)   [15] a, the sensor-noise amplitude   [16] n, the image's primitive count   [17] first, the
 *   index of its first primitive in prims   [18], [19] reserved, 0
 * prims: HOST int32 [NP][JCM_SYNTH_PRIM_INTS = 16]:
 *   [0] kind: 0 capsule, 1 quadrilateral   [1..8] geometry in sixteenths of a pixel -- capsule: ay, ax, by, bx, r, 0, 0, 0; quadrilateral: y0, x0,
 *   y1, x1, y2, x2, y3, x3, the vertices in order (either winding)   [9..11] col (R, G, B)   [12] tamp   [13] ts   [14] tseed   [15] reserved, 0
 * hash32(seed, i, j), on uint32 with wrap-around (a negative seed is its two's complement):
 *   h = (seed * 0x9E3779B1) ^ (i * 0x85EBCA77) ^ (j * 0xC2B2AE3D);  h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16
 * vnoise(seed, s, y, x) in 0..255: cell = 1 << s, i = y >> s, j = x >> s, fy = y & (cell - 1), fx = x & (cell - 1), L(i, j) = hash32(seed, i, j) >> 24,
 *   ((cell - fy) * ((cell - fx) * L(i, j) + fx * L(i, j + 1)) + fy * ((cell - fx) * L(i + 1, j) + fx * L(i + 1, j + 1))) >> (2 * s)
 * Pixel (y, x), channel k, in this order:
 *   1. g = c0[k] + floor((c1[k] - c0[k]) * y / max(H - 1, 1));   v = clamp(g + sum over o of floor(amp[o] * (vnoise(seed + o, s[o], y, x) - 128) / 256), 0, 255)
 *      (the noise is the same for the three channels).
 *   2. For primitive first, first + 1, .., first + n - 1: c = the count of the pixel's 16 sub-samples inside it (sample positions and the capsule
 *      test: jcm_render_poses above; the quadrilateral: the four cross products (v[i+1] - v[i]) x (sample - v[i]) = (y[i+1] - y[i]) * (sx - x[i])
 *      - (x[i+1] - x[i]) * (sy - y[i]), in 64-bit integers, are all >= 0 or all <= 0).  Where c > 0:
 *        t = clamp(col[k] + floor(tamp * (vnoise(tseed, ts, y, x) - 128) / 256), 0, 255);   v = (c * t + (16 - c) * v + 8) >> 4
 *   3. v = clamp(v + (int)(hash32(seed ^ JCM_SYNTH_NOISE_KEY, y * W + x, k) mod (2 * a + 1)) - a, 0, 255)
 * out: device, uint8 [B,H,W,3] (out_f32 == 0) at ANY byte address, or float32 (out_f32 == 1, 4-byte aligned) = float32(v) / float32(255), the byte
 * grid of the image entry points.  Every element of out is written.
 * JCM_ERR_ARG -- nothing is launched, out is untouched -- for a null records or out, or NP > 0 with null prims; B outside 1..65535; H or W < 1 or
 * H * W > 2^31 - 1; NP < 0; a colour, an amplitude (amp, a, tamp) outside 0..255; a shift (s[o], ts) outside 0..8; n outside 0..64; first < 0 or
 * first + n > NP; a kind other than 0 and 1; a coordinate outside +-2^20; a capsule with r < 0 or r > 2^16.
 * records and prims are read before the call returns: they travel in kernel arguments (ceil(B / 48) + ceil(NP / 60) small launches into the
 * handle's workspace); then ONE launch on the handle's stream.  The call does NOT synchronise (growing the handle's workspace does, as for every
 * entry point that uses it). */
#define JCM_SYNTH_REC_INTS 20
#define JCM_SYNTH_PRIM_INTS 16
#define JCM_SYNTH_NOISE_KEY 0x5BD1E995u
int jcm_synth_people(jcm_handle h, const int32_t* records, int B, const int32_t* prims, int NP, int H, int W, int out_f32, void* out);

/* -- mirrored test-time evaluation -----------------------------------------------------
 * The maps of an image averaged with the un-mirrored maps of its mirror image: jcm_mirror_pairs makes the batch the tower sees,
 * jcm_mirror_merge folds the tower's maps back.  Both enqueue one launch on the handle's stream and do not synchronise.
 * jcm_mirror_pairs: x [B,H,W,C] device, float32 (x_u8 == 0) or uint8 (x_u8 == 1); out [2B,H,W,C] device, the same type, not overlapping x:
 *   out[2b]              = x[b]
 *   out[2b+1][y][xx][c]  = x[b][y][W-1-xx][c]
 * Pure bit copies, any C >= 1 (images C = 3, the torso map C = 1).  JCM_ERR_ARG for a null pointer, B, H, W or C below 1, H * W * C >= 2^31 and a
 * row of more than 65536 bytes (W * C * sizeof(value); a row is staged in LDS); nothing is launched then. */
int jcm_mirror_pairs(jcm_handle h, const void* x, int x_u8, int B, int H, int W, int C, void* out);
/* jcm_mirror_merge: hm [n*G,HH,WW,K] device fp32, copy g of group i is entry i*G+g, G even; the odd g are maps of mirrored inputs.
 * out [n,HH,WW,K] device fp32, not overlapping hm:
 *   out[i,y,x,k] = (float)( (v_0 + v_1 + .. + v_{G-1}) / (double)G ),  the sum in double, g = 0 .. G-1 in this order,
 *   v_g = hm[i*G+g, y, x, k]              for even g,
 *   v_g = hm[i*G+g, y, WW-1-x, perm[k]]   for odd g
 * -- the arithmetic of jcm_group_mean, so G = 2 is exact and every G is reproduced bit for bit by a sequential float64 loop.
 * perm: HOST array of K entries, a permutation of 0..K-1; NULL = the first K entries of the FLIC left/right table {3,4,5,0,1,2,7,6,8,9}
 * (augmentation.py:20; needs K <= 10 and, as a permutation, K in {6, 8, 9, 10}).  JCM_ERR_ARG for odd G, G < 2, n, HH, WW or K below 1, K > 64,
 * HH * WW * K >= 2^31, a perm that is not a permutation of 0..K-1 and a null hm or out; nothing is launched then. */
int jcm_mirror_merge(jcm_handle h, const float* hm, int n, int G, int HH, int WW, int K, const int32_t* perm, float* out);

/* -- training-time augmentation (augmentation.py:58-78; main.py:494-497) ----------------------------
 * x [B,H,W,3], y [B,h,w,10] (= y_in, main.py:488), params [B,6] = (flip, delta, factor, angle, rh, rw):
 * all device fp32; x_out / y_out same shapes, must not alias the inputs.  Enqueues, does not synchronise.
 * Per image: flip (flip == 1; heat-map channels permuted), brightness + delta, contrast (mean of the brightened
 * channel), clip to [0,1], rotation by `angle` (bilinear, fill 0), crop_and_resize of the box
 * [rh, rw, rh + 0.95, rw + 0.95] back to the input size; heat maps then pow(., 1.6) + 1e-5, normalised per channel
 * (DESIGN.md 4.7).  H, W, h, w >= 2; the handle must have n_joints == 9.  Uses the workspace arena: JCM_ERR_STATE
 * from the gradient-ready callback of the same handle. */
int jcm_augment_train(jcm_handle h, const float* x, const float* y, const float* params, int B, int H, int W,
                      int hh, int hw, float* x_out, float* y_out);

/* -- batches from a device-resident data set ----------------------------------------
 * x_all [N,H,W,3], y_all [N,h,w,K+1]: device fp32, the whole data set; idx: HOST int32 [B], each in [0, N), repeats allowed.
 * jcm_gather_batch: x_out[b] = x_all[idx[b]], y_out[b] = y_all[idx[b]], bit for bit (x_out [B,H,W,3], y_out [B,h,w,K+1]).
 * jcm_augment_train_indexed: jcm_augment_train with image idx[b] of the data set as the source of output image b and
 *   params[b] as its parameters; the results equal jcm_gather_batch followed by jcm_augment_train bit for bit.
 * Every index is checked on the host before anything is launched: an index outside [0, N) is JCM_ERR_ARG with its position in
 * the message, as are null pointers, bad sizes and outputs that overlap the data set, params or each other; nothing is written
 * then.  idx is read before the call returns (the indices travel in the kernel arguments).  Both enqueue on the handle's
 * stream and do not synchronise.  H, W, h, w >= 1 for the gather, >= 2 for the augmentation (which also needs n_joints == 9
 * and uses the workspace arena, like jcm_augment_train). */
int jcm_gather_batch(jcm_handle h, const float* x_all, const float* y_all, int64_t N, const int32_t* idx, int B, int H, int W,
                     int hh, int hw, float* x_out, float* y_out);
int jcm_augment_train_indexed(jcm_handle h, const float* x_all, const float* y_all, int64_t N, const int32_t* idx, const float* params,
                              int B, int H, int W, int hh, int hw, float* x_out, float* y_out);
/* The same two from a byte data set: x_all [N,H,W,3] uint8 (a quarter of the memory), y_all, x_out and y_out fp32 as above.  Every image value
 * read is float32(k) / float32(255); the results equal those of the float entries on the float data set bit for bit.  Same checks, same
 * error texts (under the _u8 names). */
int jcm_gather_batch_u8(jcm_handle h, const uint8_t* x_all, const float* y_all, int64_t N, const int32_t* idx, int B, int H, int W,
                        int hh, int hw, float* x_out, float* y_out);
int jcm_augment_train_indexed_u8(jcm_handle h, const uint8_t* x_all, const float* y_all, int64_t N, const int32_t* idx, const float* params,
                                 int B, int H, int W, int hh, int hw, float* x_out, float* y_out);

/* -- affine training augmentation: one composed sample of the image, target maps redrawn at the transformed joint cells --------
 * x [B,H,W,3] device fp32; cells: device int32 [B,10,2], the (row, col) heat-map cell of each channel's joint (data.joint_cells); x_out [B,H,W,3],
 * y_out [B,h,w,10] device fp32.  colour: HOST fp32 [B,3] = (flip in {0, 1}, delta, factor); geom: HOST float64 [B,12] = the inverse map (a, b, c0, d, e, f0)
 * followed by the forward map (A, B, C0, D, E, F0) (augmentation.affine_geometry: all trigonometry is done there, none on the device).  Both are read
 * before the call returns and travel in the kernel arguments, 16 images per launch; the call enqueues on the handle's stream and does not synchronise.
 * Image: output pixel (q, r) reads the source at xs = (a q + b r) + c0, ys = (d q + e r) + f0, float64, one rounded operation per step as written; x0 =
 *   floor(xs), fx = xs - x0 (y alike); the four taps (y0 | y0 + 1, x0 | x0 + 1); a tap outside [0, W-1] x [0, H-1] is `pad` itself, a tap inside is
 *   v = clip(((src + delta) - m_c) * factor + m_c, 0, 1) in float32, m_c the contrast mean of jcm_augment_train (the fixed-order double sum of src + delta
 *   over the source image, / (H W), rounded to float32); top = (1 - fx) v00 + fx v01, bot alike, out = float32((1 - fy) top + fy bot).  A position that is
 *   not finite gives `pad`.  Bilinear, not antialiased: a scale below 1 aliases.
 * Maps: output channel k takes source channel ks = flip ? {3,4,5,0,1,2,7,6,8,9}[k] : k; its cell (r, c) stands for the point (8 c + 3.5, 8 r + 3.5); qx =
 *   (A x + B y) + C0, qy = (D x + E y) + F0, clamped to [0, W] / [0, H] (NaN -> 0), cell' = (int(qy / 8), int(qx / 8)) -- the rule of data.joint_cells;
 *   y_out[b, :, :, k] is the 3x3 blob [1,2,1] x [1,2,1] / 16 around cell' cut by the border (row h / column w are possible centres) and 0 elsewhere: bit for
 *   bit data.target_heat_maps of cell'.  No pow, no renormalisation.
 * The _indexed entries read image idx[b] of a data set (x_all [N,H,W,3], cells_all [N,10,2]; idx HOST int32 [B] in [0, N), repeats allowed) and equal
 * jcm_gather_batch followed by jcm_augment_affine bit for bit; _u8 reads a byte data set, every value as float32(k) / float32(255): the bits of the float
 * entry on the widened data.  JCM_ERR_ARG, with nothing launched or written: null pointers, H != 8 h or W != 8 w, B outside [1, 65535], n_joints != 9, an
 * index outside [0, N) (its position in the message), a flip that is not 0 or 1, a colour, geom or pad value that is not finite, outputs that overlap an
 * input or each other.  Uses the workspace arena: JCM_ERR_STATE from the gradient-ready callback of the same handle. */
int jcm_augment_affine(jcm_handle h, const float* x, const int32_t* cells, const float* colour, const double* geom, int B, int H, int W,
                       int hh, int hw, float pad, float* x_out, float* y_out);
int jcm_augment_affine_indexed(jcm_handle h, const float* x_all, const int32_t* cells_all, int64_t N, const int32_t* idx, const float* colour,
                               const double* geom, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out);
int jcm_augment_affine_indexed_u8(jcm_handle h, const uint8_t* x_all, const int32_t* cells_all, int64_t N, const int32_t* idx, const float* colour,
                                  const double* geom, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out);

/* -- the antialiased affine sample: jcm_augment_affine with a triangle filter as wide as the picture is shrunk ------------------
 * The three entries above with one more HOST float64 array, width [B]: the filter half-width of image b in source pixels, max(1, sqrt(|a e - b d|)) of
 * its inverse map (augmentation.affine_footprint: the square root is taken on the host, none on the device).  It is read before the call returns and
 * travels in the kernel arguments beside geom.  Everything else -- the position (xs, ys), the colour-transformed value v of a source pixel and its
 * contrast mean m_c, `pad`, the maps (the same kernel, not a copy), the _indexed / _u8 forms (float32(k) / float32(255) per tap), the checks and the error
 * texts (under the _aa names) -- is that of the plain entries.
 * Image, for w = width[b], float64, one rounded operation per step as written, sums from 0 in ascending order:
 *   tx_i = 1 - |xs - i| / w   for the integers i of [ceil(xs - w), floor(xs + w)],   ty_j = 1 - |ys - j| / w   for j of [ceil(ys - w), floor(ys + w)];
 *   a column with tx_i <= 0 and a row with ty_j <= 0 are skipped everywhere below;
 *   Sx = sum_i tx_i,   Sy = sum_j ty_j;
 *   u_ji = v(j, i) for 0 <= i < W and 0 <= j < H, else `pad`: a tap outside the source takes part in the sum;
 *   acc = 0;  for ascending j:  row = 0;  for ascending i: row = row + tx_i * u_ji;   acc = acc + ty_j * row;
 *   out = float32(acc / (Sx * Sy)).
 *   A pixel none of whose columns, or none of whose rows, reaches the source (xs + w < 0, xs - w > W - 1, y alike) is written as `pad` without the
 *   loops: the same float32, since the weighted mean of equal float32 values is that value to 1e-14.  A position that is not finite gives `pad`.
 *   An image with width[b] == 1.0 exactly is sampled by the plain entry's four-tap arithmetic and has its bits (at w = 1 the triangle IS bilinear, to
 *   rounding; the plain form keeps scales >= 1 at the plain entry's cost and bits).  At most 9 x 9 taps (w = 4, scale 0.25).
 * JCM_ERR_ARG, with nothing launched or written, also for: width NULL, a width[b] that is not finite, below 1 or above 4 (its index in the message). */
int jcm_augment_affine_aa(jcm_handle h, const float* x, const int32_t* cells, const float* colour, const double* geom, const double* width, int B, int H,
                          int W, int hh, int hw, float pad, float* x_out, float* y_out);
int jcm_augment_affine_aa_indexed(jcm_handle h, const float* x_all, const int32_t* cells_all, int64_t N, const int32_t* idx, const float* colour,
                                  const double* geom, const double* width, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out);
int jcm_augment_affine_aa_indexed_u8(jcm_handle h, const uint8_t* x_all, const int32_t* cells_all, int64_t N, const int32_t* idx, const float* colour,
                                     const double* geom, const double* width, int B, int H, int W, int hh, int hw, float pad, float* x_out, float* y_out);

/* -- TensorBoard summaries (tensorboard.py) -------------------------------------------------
 * jcm_tensor_stats: per segment (offset, count) of a flat device fp32 buffer -- or, with data == NULL, of the handle's stored
 *   trainable parameters in the layout of jcm_train_param_info (read in place; a segment must lie inside one tensor) -- the
 *   statistics of tf.summary.histogram over u = fp32(f * v): f = scale, or with clip_norm > 0 the clip factor
 *   clip_norm / max(norm, clip_norm) of the last jcm_train_apply of this handle, taken from device memory (tf.clip_by_global_norm
 *   as the optimizer applied it).  segments: HOST int64 [n_segments][2].  Outputs (device):
 *     stats  double [n_segments][4] = min, max, sum, sum_squares over the finite u (an empty segment: DBL_MAX, -DBL_MAX, 0, 0);
 *     counts int64  [n_segments][3 + JCM_HIST_BUCKETS] = num (finite), n_pos (u > 0), n_nonfinite, then the counts of TF-1.x's
 *            default buckets (histogram.cc: bucket b = upper_bound(limits, (double)u), limits from jcm_hist_bucket_limits).
 *   Sums are fixed-order folds; results are bitwise reproducible.  Synchronises the stream (the segment table is host memory).
 * jcm_hist_bucket_limits: the JCM_HIST_BUCKETS limits (-DBL_MAX ... -1e-12, 0, 1e-12 ... DBL_MAX); host only; returns the count
 *   (out may be NULL), -1 when cap is too small.
 * jcm_image_u8: NormalizeFloatImage of summary_image_op.cc for x [N,H,W,C] fp32, C = 1 or 3 -> out uint8 [N,H,W,C] (device):
 *   per image min / max over the finite pixels, scale 127 / max(|min|, |max|) + 128 when min < 0, else 255 / max (0 when that
 *   max < 1e-6), truncated; a pixel with a non-finite channel becomes (255, 0, 0) (gray: 255).
 * jcm_hm_overlay: show_img_plus_hm (tensorboard.py:60-71) for images x [n,H,W,3] and heat maps hm [n,hh,hw,K] (K = 9, the
 *   reference's joints): out uint8 [n,K+1,H,W,3] -- picture j < K = min(x + colorize(c_j), 1), picture K = the all-joints
 *   picture, each quantised as jcm_image_u8; c_j = hm[..., j] resized (TF-1.x bilinear) times 1 / max(hm[..., j]).
 * All three image calls enqueue without synchronising and use the workspace arena.
 * jcm_act_summary: tb.var_summary(pre_activ, name) + tf.summary.image('f_activ_' + name, activ[:, :, :, 7:8], 3) of conv_layer
 *   (main.py:167-168) in one pass over z = the pre-activation [B,H,W,C] of layer `scope` (jcm_conv_layer_pre).  The images form n_groups
 *   groups of B / n_groups consecutive images (the towers' slices; the B % n_groups trailing images are left out).  Outputs (device):
 *     stats, counts: per group what jcm_tensor_stats returns per segment (double [n_groups][4], int64 [n_groups][3 + JCM_HIST_BUCKETS]);
 *     activ_out [B,H,W,C] (may be NULL) = fp32(fp32(relu(z)) * scale[c]) + shift[c] with the folded inference-mode BatchNorm stored for
 *            `scope`, two rounded operations; relu keeps a NaN (tf.nn.relu).  A layer without BatchNorm: activ = z.  The left-out
 *            trailing images are not written;
 *     pics_out fp32 [n_groups][n_pics][H][W] = channel pic_channel of the activation of the first n_pics images of every group
 *            (n_pics <= B / n_groups; 0 with pics_out NULL: none); jcm_image_u8 (C = 1) quantises them as tf.summary.image does.
 *   B < n_groups, pic_channel >= C, n_pics too large, an unknown scope and C != the layer's Cout are refused before any launch.
 *   Results are bitwise reproducible; enqueues without synchronising; uses the workspace arena; timed under "<scope>/act_summary".
 * jcm_bn_folded: the folded BatchNorm jcm_finalize (or the last refresh) stored for `scope`: scale = gamma / sqrt(var + 1e-3),
 *   shift = beta - mean * scale, each step rounded to fp32; count = the layer's Cout; host or device pointers; synchronises. */
#define JCM_HIST_BUCKETS 1551
int jcm_tensor_stats(jcm_handle h, const float* data, const int64_t* segments, int n_segments, float scale, float clip_norm, double* stats,
                     int64_t* counts);
int jcm_hist_bucket_limits(double* out, int cap);
int jcm_image_u8(jcm_handle h, const float* x, int N, int H, int W, int C, uint8_t* out);
int jcm_act_summary(jcm_handle h, const char* scope, const float* z, int B, int H, int W, int C, int n_groups, int pic_channel, int n_pics,
                    float* activ_out, double* stats, int64_t* counts, float* pics_out);
int jcm_bn_folded(jcm_handle h, const char* scope, float* scale_out, float* shift_out, int count);
int jcm_hm_overlay(jcm_handle h, const float* x, const float* hm, int n, int H, int W, int hh, int hw, int K, uint8_t* out);

/* -- tower concat across processes (main.py:573-574: tf.concat of the per-tower maps; here one process per GPU) --------
 * The only collective of the inference path: every rank contributes its [B_local,2,K] int32 coordinates and receives
 * all ranks' in rank order, moved by RCCL (the ROCm build of the NCCL API) over xGMI.  RCCL is resolved with dlopen on
 * first use (inside a torch process that is the copy torch loaded).
 *   jcm_comm_unique_id : rank 0 creates the 128-byte rendezvous id (ncclGetUniqueId); the host hands it to the other ranks
 *                        by whatever channel it has (the Python host uses the torch.distributed store);
 *   jcm_comm_create    : ncclCommInitRank on `device` (collective over all ranks);
 *   jcm_allgather_coords: ncclAllGather on the handle's stream, then synchronises that stream -- the one entry point of
 *                        the path that does; local [B_local,2,K], all_out [world*B_local,2,K], both device int32. */
#define JCM_COMM_ID_BYTES 128
typedef struct jcm_comm_s* jcm_comm;
int jcm_comm_unique_id(unsigned char* id);
int jcm_comm_create(const unsigned char* id, int world, int rank, int device, jcm_comm* out);
int jcm_comm_destroy(jcm_comm c);
int jcm_allgather_coords(jcm_handle h, jcm_comm c, const int32_t* local, int B_local, int32_t* all_out);

/* CRC-32C (Castagnoli) of host memory, continuing from `crc` (0 to start): the checksum of tf.train.Saver checkpoint
 * files (tf_checkpoint.py reads and writes them; main.py:604,612,666).  Host-only helper, no device work. */
uint32_t jcm_crc32c(const void* data, size_t n, uint32_t crc);

/* -- introspection (used by bench.py for the roofline object) ------------------------------------
 * Sum of the HIP-event durations (ms) and the number of launches recorded for conv layer
 * `scope` since the last read; synchronises the stream and clears the record. */
int jcm_profile_read(jcm_handle h, const char* scope, double* total_ms, int* launches);
/* Name of the HIP kernel a launch of conv layer `scope` on a [B,H,W,Cin] input takes on this handle (the
 * dispatch depends on precision, options and shape); bench.py labels its roofline object with it and the
 * tests assert that the intended kernel is the one that runs.  For the stride-2 first layers (Cin == 3) H and W are
 * the layer's own input extents, i.e. those of the SUB-SAMPLED image: a fused conv1 + pool1 kernel of conv1_mfma.hip
 * is named only where the tower takes it -- H % 4 == 0, W % 4 == 0 and the packed 64-filter image exists --
 * and conv1_5x5s2_kernel everywhere else. */
int jcm_conv_kernel_name(jcm_handle h, const char* scope, int B, int H, int W, char* name, int cap);
/* Bytes currently held by the workspace arena + packed parameters. */
int64_t jcm_workspace_bytes(jcm_handle h);

/* -- joint training step (main.py:511-577,644) ------------------------------------
 * One `sess.run(train_step, {flag_train: True})` of one tower, split at the point where the
 * reference averages the tower gradients (average_gradients, main.py:243-267) so that the host
 * can all-reduce between the two calls:
 *
 *   jcm_train_loss_grads : forward with batch-statistics BatchNorm (is_training=True, main.py:113,129;
 *       the moving_mean / moving_variance update ops of main.py:557 run here, decay 0.9), loss_tower =
 *       CE(pd) + CE(sm) + lmbd * weight_decay('weights') (main.py:538-540), and opt.compute_gradients
 *       (main.py:560) into one flat caller-owned buffer laid out by jcm_train_param_info.  The advanced moving statistics are in the
 *       parameter store at once (jcm_get_tensor), but the folded BatchNorm tables the inference entry points read are rebuilt only by
 *       jcm_train_apply / jcm_update_tensor(refresh != 0): until then inference on the handle is bit-identical to inference before the call.
 *   jcm_train_apply      : grad_renorm(., clip_norm) = tf.clip_by_global_norm (main.py:302-309,576) and
 *       opt.apply_gradients (main.py:577) with tf.train.AdamOptimizer (beta 0.9/0.999, eps 1e-8) or
 *       MomentumOptimizer(0.9) (main.py:501-504); then every derived table (packed weights, folded BN,
 *       prior spectra) is rebuilt, so inference entry points see the new parameters.
 *
 * Trainable tensors are all parameters except the BatchNorm moving statistics, in ascending name
 * order.  fp32 handles take the default route of "conv9_fft" (forward, data and weight gradients in the frequency domain, two scaled
 * fp16 parts per operand) or, with "conv9_fft" = 0 / "f32_conv", the direct kernels; bf16 handles train in mixed precision (bf16 tensors
 * and MFMA operands, fp32 master weights, statistics, losses, spatial model and optimizer). */
#define JCM_OPT_ADAM 0
#define JCM_OPT_MOMENTUM 1
int jcm_train_begin(jcm_handle h);                       /* after jcm_finalize: allocates optimizer slots, n_iters = 0 */
int jcm_train_param_count(jcm_handle h, int64_t* n_tensors, int64_t* n_elements);
int jcm_train_param_info(jcm_handle h, int64_t index, char* name, int name_cap, int64_t* offset, int64_t* count);
/* x [B,H,W,3], y = y_in [B,hh,ww,K+1] target heat maps (main.py:488) at the heat-map size of the image: hh = ceil(ceil(ceil(H/2)/2)/2),
 * ww likewise (60x90 for 480x720; use_sm needs 60x90); grads: device fp32 [n_elements];
 * losses: device fp32 [4] = loss_tower, loss_pd, loss_sm, weight_decay('weights'). */
int jcm_train_loss_grads(jcm_handle h, const float* x, const float* y, int B, int H, int W, int use_sm, float lmbd,
                         float* grads, float* losses);
/* The gradient kernels of one stride-1 conv layer on caller tensors, on the route the training step takes on this handle (what
 * opt.compute_gradients, main.py:560, evaluates for tf.nn.conv2d, main.py:135): x [B,H,W,Cin] the layer input, dz [B,H,W,Cout] the gradient
 * w.r.t. the convolution output;  grads[<scope>/weights] = sum over (b,y,x) of x (*) dz + lmbd * w  (flat buffer in the layout of
 * jcm_train_param_info, only this slice is written) and dx_out [B,H,W,Cin] (may be NULL) = conv_SAME(dz, flipped transposed w).  Used by the
 * tests to hold the gradient kernels to fp32-class error; after jcm_train_begin.  fp32 handles: x, dz, dx_out fp32.  bf16 handles: x, dz and
 * dx_out bf16 (the tensors the mixed-precision step keeps between the layers), grads fp32. */
int jcm_train_layer_grads(jcm_handle h, const char* scope, const void* x, const void* dz, int B, int H, int W, float lmbd,
                          float* grads, void* dx_out);
/* The stages of the step BETWEEN its convolutions, each on caller tensors through the host function the step itself calls, so that the tests can hold
 * every kernel variant to float64 at channel counts and map sizes no whole step reaches (DESIGN.md 4.5a lists the variants).  After jcm_train_begin.
 * Activation tensors (r, y, pool, dy, dz, dx) are fp32 on an fp32 handle and bf16 on a bf16 handle; statistics, losses and grads are fp32.
 * `scope` names a conv layer with BatchNorm: it supplies gamma / beta / the moving statistics and the channel count C.
 *   jcm_train_bn_fwd   : r [B,H,W,C] (the layer's relu(conv + b)) -> y_out = BN(r) with batch statistics (main.py:129), pool_out (may be NULL)
 *       [B,ceil(H/2),ceil(W/2),C] = the 2x2/2 SAME max pool of y, mean_out / rstd_out [C] (may be NULL; rstd = 1/sqrt(biased var + 1e-3)); the handle keeps
 *       the statistics for the backward pass and advances moving_mean / moving_variance (decay 0.9, Bessel-corrected variance; main.py:557).
 *   jcm_train_bn_bwd   : dy [B,H,W,C] times dy_scale -- or, pooled != 0, the gradient of the POOLED map [B,ceil(H/2),ceil(W/2),C], which goes to the first maximum
 *       of y in each window (dy_scale must be 1) -- with r and y (pooled only; otherwise may be NULL) of the forward pass and its statistics
 *       (mean / rstd [C]; NULL = what the handle kept) -> dz_out [B,H,W,C] = the gradient w.r.t. conv + b (through BatchNorm and the ReLU, r > 0) and
 *       grads[<scope>/BatchNorm/gamma, /beta, <scope>/biases] in the flat layout of jcm_train_param_info (only these slices are written).
 *   A pool request (pool_out, pooled) on a layer with C % 4 != 0 returns JCM_ERR_ARG: the pool kernels take four channels per thread.
 *   jcm_train_resize_bwd : the adjoint of jcm_resize_bilinear, times scale: dy [B,H,W,C] -> dx_out [B,sh,sw,C]  (the branch merge, main.py:58,67,69-70).
 *   jcm_train_softmax_ce : main.py:220-240 per (image, joint) map of HW pixels: logits [B,HW,K], target [B,HW,Kt] (first K channels), loss [B*K];
 *       dz (may be NULL) [B,HW,ldz]: columns < K (+)= gscale * (softmax - target) -- TF's backprop, also where a target map does not sum to one --
 *       accumulate != 0 adds to what dz holds; columns >= K are not touched.
 *   jcm_train_softmax_bwd: dz [B,HW,ldz] += p * (g - sum over the map's pixels of p * g), p [B,HW,K] probabilities, g [B,HW,ldg] (first K channels). */
int jcm_train_bn_fwd(jcm_handle h, const char* scope, const void* r, int B, int H, int W, void* y_out, void* pool_out, float* mean_out, float* rstd_out);
int jcm_train_bn_bwd(jcm_handle h, const char* scope, const void* dy, float dy_scale, int pooled, const void* r, const void* y, const float* mean,
                     const float* rstd, int B, int H, int W, float* grads, void* dz_out);
int jcm_train_resize_bwd(jcm_handle h, const void* dy, int B, int sh, int sw, int H, int W, int C, float scale, void* dx_out);
int jcm_train_softmax_ce(jcm_handle h, const float* logits, const float* target, int B, int HW, int K, int Kt, float gscale, float* loss, float* dz,
                         int ldz, int accumulate);
int jcm_train_softmax_bwd(jcm_handle h, const float* p, const float* g, int B, int HW, int K, int ldg, float* dz, int ldz);
/* The spatial model's training stage on caller tensors, through the host function the step calls behind its spatial softmax (main.py:528-531,539 and
 * their backward pass; fp32 on every handle; 9 joints, spatial-model parameters set).  pd_prob [B,5400,K] = hm_pred_pd, y [B,5400,K+1] the targets:
 *   ce_out [B*K]     = the cross-entropy of every (image, joint) map of the spatial model's logits, unscaled;
 *   dlog [B,5400,16] : channels < K += d (gscale * sum ce) / d pd_logits, through pd_prob = softmax over the map; channels >= K are not touched;
 *   grads            : the energy_*, bias_* and bn_sm/BatchNorm/{gamma,beta} slices of the flat layout of jcm_train_param_info = the gradients of
 *                      gscale * sum ce; nothing else is written;
 * and bn_sm's moving_mean / moving_variance advance as in the step.  The backward pass runs in slices of "sm_chunk" images. */
int jcm_train_sm_grads(jcm_handle h, const float* pd_prob, const float* y, int B, float gscale, float* ce_out, float* dlog, float* grads);
/* grads: the (tower-averaged) gradients, same layout; lr: the value of lr_tf for this update
 * (main.py:492); clip_norm <= 0 disables the clip; grad_norm_out (host, may be NULL) receives the
 * global norm before clipping and makes the call synchronise. */
int jcm_train_apply(jcm_handle h, const float* grads, int optimizer, float lr, float clip_norm, float* grad_norm_out);
/* Overlapping the tower average with the backward pass: `fn(user, offset, count)` is called on the calling thread, from
 * inside jcm_train_loss_grads, as soon as every kernel that writes grads[offset, offset+count) has been enqueued on
 * the handle's stream (one call per layer, last layer first; the spatial-model blocks first of all).  The host
 * records an event on that stream and starts the all-reduce of the range on another stream.  Every trainable
 * element is reported exactly once per call.  NULL disables.
 * The callback runs WITHOUT the library's per-device call lock: it may call read-only entry points (jcm_get_tensor,
 * jcm_profile_read, jcm_last_error, another handle's calls).  It must not start a second training or forward call
 * on the SAME handle (that call would reuse the workspace the running step lives in): every entry point of the same handle
 * that uses the workspace arena or changes the training state or the parameters (jcm_forward, jcm_pd_forward, jcm_conv_layer*,
 * jcm_act_summary, jcm_sm_forward, jcm_conv_mrf, jcm_train_*, jcm_update_tensor) returns JCM_ERR_STATE when called from the callback. */
typedef void (*jcm_grad_ready_fn)(void* user, int64_t offset, int64_t count);
int jcm_train_set_grad_callback(jcm_handle h, jcm_grad_ready_fn fn, void* user);
int jcm_train_steps(jcm_handle h, int64_t* n_iters);     /* n_iters_tf (main.py:491) */
/* The optimizer side of Saver.save / Saver.restore (main.py:604,612,666 cover every global variable): slot 0 = the
 * '<var>/Adam' first moments (or '<var>/Momentum' accumulators), slot 1 = the '<var>/Adam_1' second moments, flat in the
 * layout of jcm_train_param_info (host or device pointer, may be NULL to move n_iters only); n_iters also fixes Adam's
 * beta powers (beta^n_iters) and the position in the learning-rate schedule. */
int jcm_train_get_state(jcm_handle h, int slot, float* out, int64_t count, int64_t* n_iters);
int jcm_train_set_state(jcm_handle h, int slot, const float* data, int64_t count, int64_t n_iters);
/* Saver.save side (main.py:666): copy a stored parameter out (host or device pointer). */
int jcm_get_tensor(jcm_handle h, const char* name, float* out, int64_t count);
/* Saver.restore on a live session (main.py:612): overwrite a stored parameter after jcm_finalize
 * (same element count; host or device pointer).  refresh != 0 rebuilds the derived tables (packed
 * weights, folded BN, prior spectra); pass 0 on all but the last tensor of a batch of updates. */
int jcm_update_tensor(jcm_handle h, const char* name, const float* data, int64_t count, int refresh);

#ifdef __cplusplus
}
#endif
#endif /* JCM_H */
