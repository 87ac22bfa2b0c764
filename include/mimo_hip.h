/*
 * mimo_hip.h — C ABI of libmimo_hip.so: the MI355X (gfx950) execution engine for the
 * MIMO U-Net forward + backward + loss + optimiser hot path.
 *
 * The reference (antonbaumann/MIMO-Unet @ 2024_10_08) has no FFI seam: the path is plain
 * nn.Module composition.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root).  All pointers are raw device
 * pointers unless marked "host"; no torch types cross this boundary.  Every function
 * returns 0 on success or a negative mimo_status; mimo_last_error() gives the message
 * (thread-local).  The plan calls (mimo_forward / mimo_loss_forward / mimo_backward* / mimo_adam_step /
 * mimo_uncertainties / the epilogues) are asynchronous on the given hipStream_t, never synchronise and
 * never allocate device memory after mimo_plan_create(); they are not re-entrant on one plan.  The
 * mimo_op_* single-operator entry points at the end exist for the kernel parity tests only: they allocate
 * their own scratch and synchronise the stream before returning.  mimo_plan_profile_read() synchronises on
 * the recorded events.
 */
#ifndef MIMO_HIP_H
#define MIMO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations below are its whole dynamic symbol table
 * (tests/test_host_cpu.py checks `nm -D` against this header). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct mimo_plan mimo_plan;
typedef void* mimo_stream; /* hipStream_t */

enum mimo_status {
  MIMO_OK = 0,
  MIMO_ERR_INVALID = -1, /* bad argument / unsupported configuration */
  MIMO_ERR_HIP = -2,     /* a HIP runtime call failed */
  MIMO_ERR_STATE = -3    /* call order violated (e.g. backward before forward) */
};

/* Arithmetic of the 3x3 convolutions (BatchNorm statistics, the loss and the optimiser are always fp32; storage is
 * fp32 except in the two *_MIXED modes).
 * MIMO_PREC_FP32: f32-input MFMA everywhere (bit-exact fp32 fma chains).
 * MIMO_PREC_SPLIT16: each fp32 operand is split into a 16-bit hi + lo pair and every product block of the forward and
 *   the data gradient is three 16-bit MFMAs with fp32 accumulation: fp16 pairs in the forward convolution (~2^-22 per
 *   product: fp32-class outputs; the weight image of a layer carries a power-of-two scale that follows its largest |w|,
 *   so any fp32 weight is in range), bf16 pairs (fp32 exponent range, ~1e-5 per product) in the data gradient.  The
 *   weight gradient (round 5) is two fp16 MFMAs per product — the activation as ONE fp16 value, dz as an fp16 (hi, lo) pair
 *   scaled by a power of two taken from max |dz|: 1-4e-4 of a weight-gradient tensor's scale in rounding noise, nothing
 *   of it reaches other layers (environment MIMO_WGRAD_NP=3: three bf16-pair MFMAs, ~1e-5).
 * MIMO_PREC_BF16: mixed precision in the sense of the reference's `precision="16-mixed"` runs
 *   (scripts/train/train_ndvi.py:71) and of BASELINE config 4: convolution operands are rounded to bf16
 *   on the way into the MFMA (one MFMA per product block, fp32 accumulation); master weights, BatchNorm
 *   statistics, the loss, the optimiser and — in this version — the stored activations stay fp32.
 *   Parity against the fp32 oracle at bf16 tolerance (~1e-2).
 * MIMO_PREC_BF16_MIXED / MIMO_PREC_FP16_MIXED: 16-bit STORAGE as well — activations, convolution outputs and their
 *   gradients live in HBM as bf16 / fp16 (half the bytes of every bandwidth-bound pass), convolution operands are that
 *   type (one MFMA per product, fp32 accumulation); master weights, BatchNorm statistics (taken from the fp32
 *   accumulators), the logits, the loss and the optimiser stay fp32.  FP16_MIXED is the reference's production mode
 *   `precision="16-mixed"` (scripts/train/train_ndvi.py:71): run it under a loss scaler (torch.cuda.amp.GradScaler;
 *   FlatAdam unscales, checks for inf / nan and skips the step on the device).  BASELINE config 4 = BF16_MIXED. */
enum mimo_precision {
  MIMO_PREC_FP32 = 0,
  MIMO_PREC_SPLIT16 = 1,
  MIMO_PREC_BF16 = 2,
  MIMO_PREC_BF16_MIXED = 3,
  MIMO_PREC_FP16_MIXED = 4
};

enum mimo_loss_kind { MIMO_LOSS_LAPLACE_NLL = 0, MIMO_LOSS_GAUSSIAN_NLL = 1 };

/* Block variants: the reference's blocks are BatchNorm2d + ReLU (components.py:22-30) and bilinear
 * align_corners up-sampling (components.py:77-85; its ConvTranspose2d branch, components.py:95-104, is unreachable from
 * the LightningModule: mimo_unet.py:73-74 hard-wire bilinear=True).  Those are the values 0 — the only ones implemented
 * and the only ones that can be parity-checked against the reference; mimo_plan_create rejects any other value with
 * MIMO_ERR_INVALID.  The fields exist so that a GroupNorm / SiLU / transposed-convolution variant (BASELINE.json's
 * north_star wording) is a new enum value, not an ABI change. */
enum mimo_norm_kind { MIMO_NORM_BATCH = 0 };
enum mimo_act_kind { MIMO_ACT_RELU = 0 };
enum mimo_up_kind { MIMO_UP_BILINEAR_ALIGN_CORNERS = 0 };

/* Constructor arguments of mimo.models.mimo_components.model.MimoUNet (model.py:31-44) plus
 * the batch geometry the plan is specialised for.  bilinear=True/use_pooling_indices=False are
 * hard-wired exactly as mimo/models/mimo_unet.py:73-74 hard-wires them. */
typedef struct mimo_config {
  int32_t in_channels;
  int32_t out_channels; /* total head width = 2 * targets (mimo_unet.py:110-111) */
  int32_t num_subnetworks;
  int32_t filter_base_count;
  int32_t batch, height, width;
  float encoder_dropout_rate, core_dropout_rate, decoder_dropout_rate; /* Dropout2d, components.py:29 */
  float bn_eps, bn_momentum; /* 1e-5, 0.1: nn.BatchNorm2d defaults (components.py:24,27) */
  int32_t loss_kind;         /* mimo_loss_kind; mimo/losses.py:39,124 */
  float eps_min, eps_max;    /* clamp of the scale/variance, losses.py:42-45,127-130: 1e-5, 1e3 */
  int32_t device;            /* HIP device ordinal */
  int32_t precision;         /* mimo_precision: arithmetic of the 3x3 forward / data-gradient convolutions */
  int32_t inference_only;    /* 0: full plan.  1 (or any value but 0 and 2): no buffers for a backward (pre-activations,
                              * activation gradients, dz / weight-gradient scratch, data-gradient weights); mimo_forward then
                              * requires training = 0 and no_grad = 1.  What torch.no_grad() + eval() means for memory.
                              * 2: input gradient only — what mimo_input_gradient needs (pre-activations, activation
                              * gradients, one dz buffer, data-gradient weights) and nothing only a weight gradient needs
                              * (slabs, split copies of dz, max |dz| slots, further dz buffers, the side stream);
                              * mimo_forward requires training = 0, mimo_plan_bind accepts grads = NULL, mimo_backward* fail
                              * with MIMO_ERR_STATE.  fp32 and split16 only. */
  float center_dropout_rate, final_dropout_rate; /* element-wise nn.Dropout (model.py:213, :277-281): the rates the
                              * in-engine generator uses for those sites (mimo_forward_args.rng_sites) */
  int32_t norm_kind, act_kind, up_kind; /* mimo_norm_kind / mimo_act_kind / mimo_up_kind: 0 = the reference's blocks */
} mimo_config;

const char* mimo_last_error(void);
int mimo_version(void);

/* ---- plan life cycle: replaces MimoUNet.__init__ (model.py:31-92) ---------------------- */
int mimo_plan_create(const mimo_config* cfg, mimo_plan** out);
void mimo_plan_destroy(mimo_plan* plan);
size_t mimo_plan_workspace_bytes(const mimo_plan* plan);

/* Parameter inventory in canonical order, with the reference's state_dict names and OIHW
 * shapes (probe of MimoUNet.state_dict(); SURVEY §5 checkpoint row).  kind: 0 = trainable
 * parameter (offset into the flat parameter / gradient buffers), 1 = BatchNorm running
 * buffer (offset into the flat buffer array).  Offsets are in floats. */
int mimo_plan_num_tensors(const mimo_plan* plan);
int mimo_plan_tensor_info(const mimo_plan* plan, int index, char* name, int name_cap, int64_t shape[4],
                          int* ndim, int* kind, int64_t* offset);
int64_t mimo_plan_param_floats(const mimo_plan* plan);
int64_t mimo_plan_buffer_floats(const mimo_plan* plan);

/* Bind the torch-owned flat storage.  grads may be NULL for inference-only and input-gradient-only plans. */
int mimo_plan_bind(mimo_plan* plan, float* params, float* grads, float* bn_buffers);

/* ---- forward: replaces MimoUNet.forward (model.py:94-117) ------------------------------
 * x is NCHW-strided fp32: element (n,s,c,y,x) at x[n*stride_n + s*stride_s + c*H*W + y*W + x]
 * (stride_s = 0 gives repeat_subnetworks, utils.py:51-61).  perm (int64 [S][N], device) is
 * the gather of apply_input_transform (utils.py:38-41) fused into the load; NULL = identity.
 * out is [N,S,Co,H,W] contiguous.  training: BatchNorm uses batch statistics and updates
 * the running buffers.  drop_masks: host array with one device pointer per DoubleConv (forward
 * order, see mimo_plan_num_double_convs), each [N][Cout] multipliers (0 or 1/(1-p)) or NULL for
 * "no dropout at this site" — Dropout2d (components.py:29) incl. MC-dropout (ensemble.py:54-66). */
typedef struct mimo_forward_args {
  const float* x;
  int64_t stride_n, stride_s;
  const int64_t* perm;
  int32_t training;
  const float* const* drop_masks; /* host array [num_double_convs] or NULL */
  float* out;
  /* element-wise nn.Dropout multipliers (0 or 1/(1-p)), reference layout, or NULL (= none):
   * host array [1 + S] of device pointers, each NULL for "not active":
   *   [0]     center_dropout (model.py:213)        [N][8fS][H/16][W/16]  on down4's output
   *   [1 + s] final_dropouts[s] (model.py:277-281) [N][f][H][W]          in front of head s   */
  const float* const* elem_masks;
  /* Inference fast path (no reference counterpart; what `torch.no_grad()` + `model.eval()` buys the
   * reference is only skipped autograd bookkeeping):
   *   no_grad != 0 with training == 0: no backward will follow this forward — eval-mode BatchNorm +
   *     ReLU (+ Dropout2d multipliers) are folded into the convolution epilogue and the pre-activation
   *     tensors are not stored; mimo_backward after such a forward fails with MIMO_ERR_STATE.
   *   param_version: any value that changes whenever the bound parameters or BatchNorm buffers may have
   *     changed (0 = unknown: re-derive everything).  While it stays the same, eval-mode forwards reuse
   *     the packed weight copies and BatchNorm scale/shift of the previous call. */
  int32_t no_grad;
  int64_t param_version;
  /* In-engine dropout (replaces the Bernoulli draws inside nn.Dropout2d / nn.Dropout, components.py:29,
   * model.py:213,277-281, incl. the MC-dropout passes of ensemble.py:54-66).  rng_sites: host array
   * [num_double_convs + 1 + S] or NULL; a non-zero entry makes the engine draw that site's multipliers itself
   * (Dropout2d sites in DoubleConv order with the config's encoder / core / decoder rates, then center_dropout, then
   * final_dropouts[s]) from a Philox4x32-10 stream keyed by (rng_seed, rng_offset) — take both from the caller's
   * generator and advance its offset.  The backward regenerates the element-wise multipliers from the same pair.
   * Sites given through drop_masks / elem_masks keep their recorded multipliers (parity tests). */
  const uint8_t* rng_sites;
  uint64_t rng_seed, rng_offset;
  /* batch rows of the x tensor (= of the label / mask tensors later given to mimo_loss_forward); 0 = the plan's
   * batch.  With perm the gather may repeat rows (batch_repetitions, utils.py:27-31), so x can hold fewer rows than
   * the plan's batch; the staged (hipGraph) paths copy exactly this many. */
  int64_t x_rows;
} mimo_forward_args;
/* The dropout multipliers of one site as the last mimo_forward used them (tests, and recording a run for bit-level
 * replay through drop_masks / elem_masks): site < num_double_convs -> [N][Cout]; num_double_convs + j -> the
 * element-wise site j (0 = center, 1 + s = final s) in the reference's layout [N][C][H'][W']. */
int mimo_plan_dropout_mask(mimo_plan* plan, int site, float* dst, mimo_stream stream);

/* Numerics status of the plan's kernels since the last clear — the reference has no counterpart (torch raises
 * nothing either; a diverged or out-of-range run shows as NaN losses): the default split16 forward carries
 * activations as fp16 (hi, lo) pairs and weights as fp16 pairs x 2^8, so |activation| >= 65520 or |weight| >= 256
 * overflows where the reference's fp32 path (mimo/models/mimo_components/components.py:23-29) does not.
 * Bits of *flags: MIMO_STATUS_FWD_STATS — a BatchNorm batch statistic of a training forward was not finite;
 * MIMO_STATUS_BWD_STATS — a BatchNorm-backward sum was not finite; MIMO_STATUS_LOGITS — a logit was not finite.
 * The kernels record them for free (one test per finalized channel sum / logit); this call copies the word to the
 * host and is the one plan call that synchronises `stream`.  clear != 0 resets the word. */
#define MIMO_STATUS_FWD_STATS 1
#define MIMO_STATUS_BWD_STATS 2
#define MIMO_STATUS_LOGITS 4
int mimo_plan_status(mimo_plan* plan, int32_t* flags, int32_t clear, mimo_stream stream);
int mimo_plan_num_double_convs(const mimo_plan* plan);
int mimo_plan_double_conv_channels(const mimo_plan* plan, int index); /* Cout of DoubleConv #index */
int mimo_forward(mimo_plan* plan, const mimo_forward_args* args, mimo_stream stream);

/* ---- subnetwork permutations: replaces the draws of apply_input_transform (mimo/models/utils.py:27-36:
 * `torch.randperm(B).repeat(batch_repetitions)`, then per subnetwork `main[:k][torch.randperm(k)]` in front of the shared
 * tail `main[k:]`) by one launch — the `perm` argument of mimo_forward / mimo_loss_forward / mimo_training_epilogue.
 * perm int64 [S][M], M = batch * reps; main_out int64 [M] or NULL; k = int(M * (1 - input_repetition_probability)) as the
 * caller's Python computes it, 0 <= k <= M.  Same structure as the reference, the engine's own generator (so not the
 * reference's values): with bits(stream, j) = 64 bits of philox4x32_10(ctr = (j >> 1, stream, offset_lo, offset_hi),
 * key = seed) — words (x, y) for even j, (z, w) for odd j, the first word low — and key(stream, j) = (bits & ~0xFFF) | j,
 *   base = argsort of key(0, 0 .. batch-1), main[i] = base[i mod batch], sigma_s = argsort of key(1 + s, 0 .. k-1),
 *   perm[s][i] = main[sigma_s[i]] for i < k and main[i] for i >= k.
 * (seed, offset): the caller's generator, which it advances by one counter block (4), as for rng_seed / rng_offset above.
 * One workgroup per subnetwork, a bitonic sort of the 64-bit keys in LDS: M <= 4096 and S <= 64, MIMO_ERR_INVALID beyond
 * (nothing is launched or written).  Asynchronous on the stream; no allocation, no atomics. */
int mimo_draw_permutations(int64_t* perm, int64_t* main_out, int32_t batch, int32_t reps, int32_t k, int32_t s,
                           uint64_t seed, uint64_t offset, mimo_stream stream);

/* ---- loss: replaces UncertaintyLoss.forward(reduce_mean=False).mean((0,2,3,4))
 * (losses.py:132-164, mimo_unet.py:241-242) on the logits of the last mimo_forward.
 * label [N,Ct,H,W], mask [N,1,H,W] or NULL, both gathered through perm like x.
 * loss_out: device [S]. */
int mimo_loss_forward(mimo_plan* plan, const float* label, const float* mask, const int64_t* perm,
                      float* loss_out, mimo_stream stream);

/* ---- backward: replaces autograd through MimoUNet (+ the loss when dloss != NULL) --------
 * dout  [N,S,Co,H,W] upstream gradient of the logits, or NULL.
 * dloss device [S]: upstream gradient of the per-subnetwork losses returned by
 *       mimo_loss_forward (e.g. weights/S, mimo_unet.py:138), or NULL.  The closed-form
 *       Laplace/Gaussian gradient is evaluated inside the head kernel.
 * dx    [N,S,Ci,H,W] gradient w.r.t. the input (FGSM, scripts/test/test_nyuv2_depth.py:41-55)
 *       or NULL to skip the first-layer dgrad.  Requires perm == NULL in the forward.
 * Parameter gradients are written (not accumulated) into the bound flat grads buffer. */
int mimo_backward(mimo_plan* plan, const float* dout, const float* dloss, float* dx, mimo_stream stream);

/* The same backward in stages, for data-parallel training (no reference counterpart: the reference is
 * single-GPU, scripts/train/train_ndvi.py:70 `devices=1`).  Stages run in order 0 .. n-1:
 *   0 heads + S decoders, 1 up3, 2 up2, 3 up1, 4 down4, 5 down3, 6 down2, 7 the S encoders (+ dx).
 * The parameters of a stage are one contiguous range [begin, end) of the flat gradient buffer (laid out encoder |
 * core | decoder | heads) that is final when the stage returns, so its all-reduce can run while the later stages
 * back-propagate: one bucket per core block, as SURVEY 8(e) asks.  The exchange itself is torch.distributed /
 * RCCL on the caller's side (mimo_unet_amd/ddp.py), not part of this ABI: there is no mimo_ddp_* entry point. */
int mimo_plan_num_backward_stages(const mimo_plan* plan);
int mimo_plan_backward_stage_range(const mimo_plan* plan, int stage, int64_t* begin, int64_t* end);
int mimo_backward_stage(mimo_plan* plan, int stage, const float* dout, const float* dloss, float* dx,
                        mimo_stream stream);
/* The same stage without making `stream` wait for the plan's side stream (the weight gradients run there): the stage's
 * range is final on *ready_stream — the side stream, which has been made to wait for `stream`, or `stream` itself when
 * the plan has no side stream / replays a per-stage graph — and the caller issues that range's collective THERE (under
 * torch: `with torch.cuda.stream(ExternalStream(ready))`), so the main stream goes straight on with the next stage.  The
 * last stage joins the two streams.  (What Lightning DDP's bucket hooks give the reference's module for free on one
 * stream; here the per-stage join of mimo_backward_stage cost 0.45 ms of a 4.4 ms step at 4 images per GPU.) */
int mimo_backward_stage_async(mimo_plan* plan, int stage, const float* dout, const float* dloss, float* dx,
                              mimo_stream stream, mimo_stream* ready_stream);
int64_t mimo_plan_encoder_param_floats(const mimo_plan* plan);

/* ---- input gradient only: replaces, for an evaluation, `loss.backward(); data_grad = images.grad.data`
 * (scripts/test/test_nyuv2_depth.py:41-55) — autograd through the whole ensemble member for the sake of d loss / d image.
 * Valid after a mimo_forward with training = 0, no_grad = 0 and perm = NULL (and, if dloss is given, a mimo_loss_forward);
 * dout / dloss as in mimo_backward.  Walks the 8 stages of mimo_backward with the same data-gradient and BatchNorm-backward
 * kernels — after an eval-mode forward the BatchNorm backward is dz = scale * relu'(.) * dy, no per-channel sums, one pass —
 * and launches no weight gradient, no reduction and nothing on the side stream; it writes no byte of the bound grads buffer
 * (which may be NULL) or of the BatchNorm buffers.  The data-gradient weight images are packed once per param_version.
 * dimage [N,Ci,H,W]: gradient w.r.t. the image that repeat_subnetworks (utils.py:51-61) broadcast to the S encoders = the sum
 * of their first-layer data gradients, added in the fixed order s = S-1, S-2, ..., 0 with fp32 adds; accumulate != 0 adds
 * that sum, term by term in the same order, to what dimage holds (the members of an ensemble), 0 overwrites.
 * Bit-identical to mimo_backward's dx summed in that order.  Works on full plans and on inference_only = 2 plans; fp32 and
 * split16 precision (MIMO_ERR_INVALID otherwise). */
int mimo_input_gradient(mimo_plan* plan, const float* dout, const float* dloss, float* dimage, int accumulate,
                        mimo_stream stream);

/* ---- the same for an MC-dropout forward (scripts/test/test_nyuv2_depth.py --monte_carlo_steps): the plan batch N holds
 * `replicas` stochastic passes of the same N / replicas images, stacked pass-major (pass m, image b at row m * N / replicas + b,
 * the layout of EnsembleModule.forward), each row with its own dropout multipliers — drop_masks / elem_masks of the forward, or
 * drawn in the engine (rng_sites).  State checks, stages, kernels and encoder order of mimo_input_gradient; the dropout
 * multipliers of the forward are applied to the gradients where the forward applied them.  dimage [N / replicas,Ci,H,W]: per
 * encoder s = S-1 ... 0 one launch folds the first-layer data gradient and adds its passes in the fixed order
 * m = 0 ... replicas-1 with fp32 adds (no atomics: deterministic); the first encoder assigns unless accumulate != 0.
 * With dloss[s] = k / (M * S_total) for a chunk of k = replicas of M passes this is the chunk's share of
 * d/d image of the mean NLL over all M * S_total outputs (the per-subnetwork loss is a mean over the chunk's N samples).
 * replicas = 1: the bits of mimo_input_gradient.  MIMO_ERR_INVALID: replicas < 1 or N % replicas != 0. */
int mimo_input_gradient_mc(mimo_plan* plan, const float* dout, const float* dloss, float* dimage, int accumulate, int replicas,
                           mimo_stream stream);

/* ---- FGSM: replaces fgsm_attack (scripts/test/test_nyuv2_depth.py:16-24) for all perturbation sizes of a sweep at once.
 * out[k][i] = clamp(image[i] + eps[k] * sign(dimage[i]), lo, hi), i < elems, k < K, with torch.sign's and torch.clamp's
 * arithmetic for every non-NaN gradient (sign(0) = 0; eps = 0 still clamps).  A NaN gradient or image pixel gives a NaN
 * output pixel (torch.sign itself would map a NaN gradient to 0 and hide it).  eps: HOST array [K], eps and K by value into the launch.
 * image and dimage are read once for all K outputs (8 B read + 4 K B written per element).  Asynchronous on the stream. */
int mimo_fgsm_perturb(const float* image, const float* dimage, int64_t elems, const float* eps, int K, float lo, float hi,
                      float* out, mimo_stream stream);

/* ---- PGD (BIM without the random start): the iterated, projected form of the attack above; no reference counterpart.
 * One step for all K perturbation sizes of a sweep in one launch.  x0 [elems] is the clean image; grad and x_adv are
 * [K][elems], the gradient taken at each size's current iterate.  x_adv is updated in place:
 *   v = x_adv[k][i] + alpha[k] * sign(grad[k][i])           (sign as above: sign(0) = 0, a NaN gradient gives NaN)
 *   v = clamp(v, x0[i] - eps[k], x0[i] + eps[k])            (the eps-ball first; each bound is one fp32 rounding)
 *   x_adv[k][i] = clamp(v, lo, hi)                          (then the value range; both clamps pass a NaN)
 * eps[k] = 0 gives clamp(x0, lo, hi) for every non-NaN gradient.  eps, alpha: HOST arrays [K], by value into the launch in
 * slices of 16.  4 + 8 K B read and 4 K B written per element.  MIMO_ERR_INVALID: a null pointer, elems < 1, K < 1, lo > hi,
 * a negative or NaN eps or alpha.  Asynchronous on the stream; no atomics. */
int mimo_pgd_step(const float* x0, const float* grad, float* x_adv, int64_t elems, const float* eps, const float* alpha, int K,
                  float lo, float hi, mimo_stream stream);

/* ---- the random start of PGD for all K sizes from ONE draw: x_adv[k][i] = clamp(x0[i] + eps[k] * r[i], lo, hi), sum and
 * product rounded separately (never fused), r[i] the same for every k.  Quad q = elements 4 q .. 4 q + 3 takes the four
 * words of philox4x32_10(ctr = (lo32(q), hi32(q), lo32(offset) ^ 0xFF000000, hi32(offset)), key = seed), element 4 q + j
 * word j, and r = (2 (w >> 8) + 1 - 2^24) * 2^-24: exact in fp32, symmetric in (-1, 1).  Counter word 2 carries the site
 * number 255 in the dropout draws' layout (rng_offset above; sites are < 56) and differs from the permutation draw's
 * (offset_lo as it is): the three never share a counter within one (seed, offset) block.  (seed, offset): the caller's
 * generator, which it advances by one counter block (4).  eps: HOST array [K]; MIMO_ERR_INVALID as for the step. */
int mimo_pgd_init(const float* x0, int64_t elems, const float* eps, int K, float lo, float hi, uint64_t seed, uint64_t offset,
                  float* x_adv, mimo_stream stream);

/* ---- measurement (no reference counterpart): per-kernel-class device time from HIP events
 * recorded on the launch stream around every 3x3 convolution launch, with the ALGORITHMIC
 * flops (2*9*Cin*Cout*N*H*W, logical channels) and bytes ((Cin+Cout)*N*H*W*4) of those
 * launches.  mimo_plan_profile(plan, 1) resets and arms; reads synchronise on the events. */
enum mimo_prof_kind {
  MIMO_PROF_CONV_FWD = 0,
  MIMO_PROF_CONV_DGRAD = 1,
  MIMO_PROF_CONV_WGRAD = 2,
  MIMO_PROF_BN_RELU_FWD = 3,   /* bandwidth class: BatchNorm + ReLU forward pass (8 B per element) */
  MIMO_PROF_BN_BWD_REDUCE = 4, /* BatchNorm backward pass 1 (8 B per element) */
  MIMO_PROF_BN_BWD_APPLY = 5,  /* BatchNorm backward pass 2 (12 B per element) */
  MIMO_PROF_UPCAT_FWD = 6,     /* bilinear x2 + pad + concat (writes the up-sampled channels) */
  MIMO_PROF_UP_BWD = 7,        /* its gradient gather */
  MIMO_PROF_POOL_BWD = 8,      /* MaxPool2d backward (+ skip-gradient fold) */
  MIMO_PROF_HEAD_FWD = 9,      /* 1x1 head */
  MIMO_PROF_HEAD_BWD = 10,     /* NLL gradient + 1x1 head backward */
  MIMO_PROF_KINDS = 11
};
int mimo_plan_profile(mimo_plan* plan, int enable);
int mimo_plan_profile_read(mimo_plan* plan, int kind, double* total_ms, int64_t* launches, double* flops,
                           double* bytes);
/* Device time of everything launched for the DoubleConv blocks (+ heads) of one resolution tier
 * (0 = full resolution H x W ... 4 = H/16 x W/16), forward and backward separately, since the profile was
 * armed: the denominator of the per-tier HBM fraction of SURVEY 8(d). */
int mimo_plan_profile_read_tier(mimo_plan* plan, int tier, double* forward_ms, double* backward_ms);
/* device time of one kernel class inside one resolution tier (the per-tier kernel table of bench.py) */
int mimo_plan_profile_read_kind_tier(mimo_plan* plan, int kind, int tier, double* ms);

/* ---- optimiser: replaces torch.optim.Adam.step (mimo_unet.py:186-190; L2-in-grad) ------ */
int mimo_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                   float grad_scale, mimo_stream stream);

/* The same step under a loss scaler (the reference trains with Lightning precision="16-mixed" = torch.cuda.amp.GradScaler,
 * scripts/train/train_ndvi.py:71).  step_dev: device float, the optimiser's step count, advanced here unless
 * *found_inf != 0; amp_scale / found_inf: device floats as GradScaler hands them to a fused optimiser (gradients are
 * divided by *amp_scale; the whole update is skipped when *found_inf != 0) or NULL.  No host synchronisation. */
int mimo_adam_step_amp(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, float* step_dev, float grad_scale,
                       const float* amp_scale, const float* found_inf, mimo_stream stream);

/* The same step with gradient clipping: torch.nn.utils.clip_grad_norm_ (clip_mode MIMO_CLIP_NORM, the global L2 norm) or
 * clip_grad_value_ (MIMO_CLIP_VALUE) followed by the Adam update above, without a host synchronisation.  The arguments of
 * mimo_adam_step_amp (step_dev always on the device) plus clip > 0, clip_out (2 device floats) and scratch (device,
 * mimo_grad_clip_scratch_bytes() bytes, 8-byte aligned, owned by the caller, reusable by ordered calls on one stream).
 * With ge = g * s, s = grad_scale (/ *amp_scale when given), formed in fp32:
 *   norm : norm = sqrt(sum ge^2) (squares in fp32, sums in double, a fixed order: two runs give the same bits),
 *          coef = min(1, clip / (norm + 1e-6)); weight decay and the moments see (g * s) * coef.
 *   value: weight decay and the moments see clamp(g * s, -clip, clip); a NaN stays a NaN.
 * clip_out[0] = the norm before clipping (value mode: 0), clip_out[1] = the coefficient applied (value mode: 1; 0 when the
 * norm is not finite), both written whether or not the step is applied.  A norm that is not finite skips the whole step —
 * parameters, moments and step_dev stay untouched, exactly as with *found_inf != 0 (torch would multiply every gradient
 * by NaN instead; clip_out[0] tells what happened).  step_dev advances only when the step is applied.  With coef == 1 the
 * update is bit-identical to mimo_adam_step_amp.  Norm mode: three launches; value mode: two (no reduction). */
enum { MIMO_CLIP_NORM = 1, MIMO_CLIP_VALUE = 2 };
size_t mimo_grad_clip_scratch_bytes(void);
int mimo_adam_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                           float beta1, float beta2, float eps, float weight_decay, float* step_dev, float grad_scale,
                           const float* amp_scale, const float* found_inf, int32_t clip_mode, float clip, float* clip_out,
                           void* scratch, mimo_stream stream);

/* ---- uncertainties: replaces compute_uncertainties (utils.py:76-101) --------------------
 * p1, p2 [N,S,C,HW] contiguous -> mean, aleatoric_var, epistemic_var [N,C,HW]. */
int mimo_uncertainties(const float* p1, const float* p2, int32_t n, int32_t s, int32_t c, int64_t hw,
                       int32_t loss_kind, float* mean, float* aleatoric, float* epistemic, mimo_stream stream);

/* ---- evidential regression head + loss: replaces the tail of EvidentialUnetModel.forward (mimo/models/
 * evidential_unet.py:90-96: mu, softplus(logv), softplus(logalpha) + 1, softplus(logbeta)) and EvidentialLoss.forward
 * (mimo/losses.py:202-247, coeff-free form the reference evaluates) and their autograd backward.
 * logits [N,4,HW] (the S = 1 backbone output), label [N,HW] or NULL, mask [N,HW] or NULL.
 * forward : ev [N,4,HW] = (gamma, v, alpha, beta); loss_map [N,HW] = per-pixel loss (x mask), or NULL.
 * backward: dlogits [N,4,HW] = d_loss [N,HW] (NULL = 0) through the loss  +  d_ev [N,4,HW] (NULL = 0) through the
 *           softplus heads. */
int mimo_evidential_forward(const float* logits, const float* label, const float* mask, int32_t n, int64_t hw, float* ev,
                            float* loss_map, mimo_stream stream);
int mimo_evidential_backward(const float* logits, const float* label, const float* mask, const float* d_ev,
                             const float* d_loss, int32_t n, int64_t hw, float* dlogits, mimo_stream stream);

/* ---- evidential model, evaluation: replaces the per-batch tail of make_predictions in the reference's
 * scripts/test/test_nyuv2_depth_evidential.py:42-65 (test_ndvi_evidential.py has the same lines).
 * mimo_evidential_uncertainties: EvidentialLoss.mode / aleatoric_var / epistemic_var (mimo/losses.py:258-271) straight from
 *   the backbone logits [N,4,HW]: mean = l0, aleatoric_var = beta / (alpha - 1), epistemic_var = beta / (v (alpha - 1)),
 *   each [N,HW], with the head arithmetic of mimo_evidential_forward (alpha = softplus(l2) + 1 rounded, then alpha - 1) in
 *   fp32.  One pass, 16 B read + 12 B written per pixel; 16-byte accesses when hw % 4 == 0 and the pointers are aligned.
 *   Infinities and NaNs (alpha - 1 == 0, v == 0) are written as they come.
 * mimo_evidential_loss_gradient: dlogits [N,4,HW] = d(scale * sum over pixels of loss_map) / d logits — with scale =
 *   1 / (N HW) the backward of `model.loss_fn(out, labels).mean()` (test_nyuv2_depth_evidential.py:44-50) down to the logits.
 *   Bit-identical to mimo_evidential_backward(d_ev = NULL, d_loss = a tensor filled with scale): the same device function,
 *   no weight tensor, no fill launch.  label [N,HW]; mask [N,HW] or NULL as in mimo_evidential_forward.
 * Both are asynchronous on the stream. */
int mimo_evidential_uncertainties(const float* logits, int32_t n, int64_t hw, float* mean, float* aleatoric_var,
                                  float* epistemic_var, mimo_stream stream);
int mimo_evidential_loss_gradient(const float* logits, const float* label, const float* mask, int32_t n, int64_t hw,
                                  float scale, float* dlogits, mimo_stream stream);

/* ---- evidential model, training / validation step: replaces, after the backbone, the tail of
 * EvidentialUnetModel.training_step / validation_step (mimo/models/evidential_unet.py:98-146): the head, EvidentialLoss.forward
 * and `loss.mean()`, `aleatoric_var ** 0.5` / `epistemic_var ** 0.5` (mimo/losses.py:258-271), `y_pred - label`, the two
 * `clip(0, 5).mean()` and compute_regression_metrics (mimo/metrics.py:22-34) — and the backward of that mean.
 * mimo_evidential_step: one pass over logits [N,4,HW], label [N,HW], mask [N,HW] or NULL.  Per pixel, with the head arithmetic
 *   of mimo_evidential_forward (alpha = softplus(l2) + 1 rounded, then alpha - 1): aleatoric_std = sqrt(beta / (alpha - 1)),
 *   epistemic_std = sqrt(beta / (v (alpha - 1))) (NULL: not wanted, not computed), err = l0 - label, each [N,HW]; the
 *   predictions are plane 0 of the logits and are not written.  Non-finite values are written as they come.
 *   scalars: device [8] = mean of the loss map (x mask) over all N HW pixels, masked ones counted (`loss.mean()`), mae, mse,
 *            rmse, r2 (= 1 - SSE / (sum y^2 - (sum y)^2 / n), in double; none of the four looks at the mask),
 *            mean clip(aleatoric_std, 0, 5), mean clip(epistemic_std, 0, 5) (0 when not wanted), element count.  An infinite
 *            std clips to 5; what a NaN does to a scalar is unspecified.
 *   scratch: device doubles [scratch_blocks * 8], scratch_blocks >= 1 (2048 is enough for any size): one partial row per
 *            workgroup, summed in a fixed order by a second one-workgroup kernel — no atomics, the same bits every run.
 *   20 B read (24 with a mask) + 8 B written (12 with epistemic_std) per pixel; 16-byte accesses when hw % 4 == 0 and
 *   every pointer is 16-byte aligned.  n, hw, scratch_blocks >= 1.
 * mimo_evidential_loss_gradient_dev: dlogits [N,4,HW] = d(scale * upstream[0] * sum over pixels of loss_map) / d logits,
 *   upstream: device [1] — the gradient arriving at the mean (1, or a loss scaler's factor), read by the kernel: no host
 *   synchronisation and no [N,HW] tensor filled with it.  Each thread forms s = scale * upstream[0] in one fp32
 *   multiplication: bit-identical to mimo_evidential_loss_gradient(scale = that product), the same device function.
 * Both are asynchronous on the stream. */
int mimo_evidential_step(const float* logits, const float* label, const float* mask, int32_t n, int64_t hw,
                         float* aleatoric_std, float* epistemic_std, float* err, float* scalars, double* scratch,
                         int32_t scratch_blocks, mimo_stream stream);
int mimo_evidential_loss_gradient_dev(const float* logits, const float* label, const float* mask, int32_t n, int64_t hw,
                                      float scale, const float* upstream, float* dlogits, mimo_stream stream);

/* ---- validation epilogue: replaces, after the forward, the tail of MimoUnetModel.validation_step
 * (mimo_unet.py:153-183): compute_uncertainties, sqrt of the variances, calculate_dist_param(log=True) +
 * the combined NLL on the ensemble mean, the error map, compute_regression_metrics (metrics.py:22-34:
 * r2 / mae / mse / rmse) and the two logged uncertainty means — one pass over the logits.
 * out [N,S,2*Ct,HW] logits, label [N,Ct,HW], mask [N,1,HW] or NULL.
 * mean / aleatoric_std / epistemic_std / err: [N,Ct,HW] each.
 * scalars: device [8] = combined NLL, mae, mse, rmse, r2, mean clip(aleatoric_std,0,5),
 *          mean clip(epistemic_std,0,5), element count.
 * scratch: device doubles [scratch_blocks * 8], scratch_blocks >= 1 (1024 is enough for any size). */
int mimo_validation_epilogue(const float* out, const float* label, const float* mask, int32_t n, int32_t s, int32_t ct,
                             int64_t hw, int32_t loss_kind, float eps_min, float eps_max, float* mean,
                             float* aleatoric_std, float* epistemic_std, float* err, float* scalars, double* scratch,
                             int32_t scratch_blocks, mimo_stream stream);

/* ---- loss-buffer step: replaces MimoUnetModel._calculate_train_loss's arithmetic on the [S] loss vector
 * (mimo_unet.py:223-247: weights = loss_buffer.get_weights() read BEFORE loss_buffer.add(loss); loss_buffer.py:43-74:
 * ring mean over ALL rows incl. still-zero ones, softmax(mean / T) * S) — one launch instead of ~9 tensor operations.
 * ring    device [size][S], updated in place: row `index` <- loss (the caller advances its index, loss_buffer.py:52)
 * loss    device [S] (mimo_loss_forward's output); weights / w_over_s: device [S] each = the weights, and weights / S
 *         (the gradient of mean(loss * weights) w.r.t. loss: mimo_backward's dloss); scalars: device [2] =
 *         mean(loss * weights), mean(loss).  1 <= S <= 64. */
int mimo_loss_buffer_step(float* ring, int32_t size, int32_t index, int32_t s, float temperature, const float* loss,
                          float* weights, float* w_over_s, float* scalars, mimo_stream stream);

/* ---- training-step epilogue: replaces, after the fused forward + loss, the no_grad tail of
 * MimoUnetModel.training_step (mimo_unet.py:121-144): the per-subnetwork label gather of apply_input_transform
 * (utils.py:38-48), loss_fn.mode / loss_fn.std (losses.py:166-192), the error map and compute_regression_metrics
 * on the flattened predictions (metrics.py:22-34) — one pass instead of ~20 tensor operations.
 * out [N,S,2*Ct,HW] logits; label [N0,Ct,HW]; perm [S][N] int64 rows of label per (s, n), or NULL (identity, N0 = N).
 * label_t / preds / aleatoric_std / err: [N,S,Ct,HW] each.
 * scalars: device [5] = mae, mse, rmse, r2, element count.  scratch: device doubles [scratch_blocks * 8]. */
int mimo_training_epilogue(const float* out, const float* label, const int64_t* perm, int32_t n, int32_t s, int32_t ct,
                           int64_t hw, int32_t loss_kind, float* label_t, float* preds, float* aleatoric_std, float* err,
                           float* scalars, double* scratch, int32_t scratch_blocks, mimo_stream stream);

/* ---- uncertainty evaluation: replaces the host half of scripts/test/test_nyuv2_depth.py (convert_to_pandas :93-106,
 * compute_metrics :128-130, create_precision_recall_plot :133-144, create_calibration_plot :147-170) and of
 * scripts/test/test_ndvi.py:86-128 — the frame of all test pixels, its sort and the 41 ppf sweeps — by three device
 * passes over an 8-byte record per pixel.  Asynchronous on the stream; no allocation, no synchronisation.
 * workspace: device memory of mimo_eval_workspace_bytes() bytes, 16-byte aligned, zeroed by the caller to reset the
 * running sums; the calls that share a workspace must be issued on ONE stream (its partial rows and the record store are
 * ordered by nothing else); records: the caller's device record store, one uint64 per pixel fed so far
 * (low word: bit pattern of combined_std, high word: |error|; 0xFFFFFFFF in both words marks a skipped pixel). */
size_t mimo_eval_workspace_bytes(void);
/* One batch (make_predictions' clip + `[:, 0]`, test_nyuv2_depth.py:73-74,85-89; convert_to_pandas' two square roots,
 * :97-99; `error`, :129; `below = y_true < ppf`, :149,166).  mean / aleatoric_var / epistemic_var / label
 * [batch,channels,hw] fp32, of which plane `channel` is used; mask [batch,mask_channels,hw] (mask_channels 1 or
 * channels; pixels with 0 are skipped and counted) or NULL.  clip != 0 clamps mean and label to [clip_lo, clip_hi].
 * thresholds: device [num_thresholds <= 64] ascending standard quantiles z_k of the expected confidences; a pixel is
 * "below" at k when label < mean + (sqrt(aleatoric_var) / sqrt 2) z_k in fp32, never when aleatoric_var == 0.
 * records points at the first free slot; batch * hw slots are written. */
int mimo_eval_accumulate(const float* mean, const float* aleatoric_var, const float* epistemic_var, const float* label,
                         const float* mask, int32_t batch, int32_t channels, int32_t channel, int32_t mask_channels,
                         int64_t hw, int32_t clip, float clip_lo, float clip_hi, const float* thresholds,
                         int32_t num_thresholds, uint64_t* records, void* workspace, mimo_stream stream);
/* The cutoffs of `df.sort_values(by='combined_std', ascending=False)` + `(percentiles * N).astype(int)`
 * (test_nyuv2_depth.py:134-137) without a sort: for each of the num_percentiles <= 128 values (device doubles) the exact
 * key of the most uncertain pixel that survives, and how many records with exactly that key survive.
 * num_records < 2^32 (32-bit histogram counters). */
int mimo_eval_select(const uint64_t* records, int64_t num_records, const double* percentiles, int32_t num_percentiles,
                     void* workspace, mimo_stream stream);
/* The `df.iloc[cutoff:]["error"].mean()` rows (test_nyuv2_depth.py:139-142) and `below.mean(axis=1)` (:167) after
 * mimo_eval_select.  out: device doubles [3 * num_percentiles + num_thresholds + 6] = mae | rmse | threshold value of
 * combined_std per cutoff, observed share per threshold, then n, n_masked, n_nonfinite, mae, mse, rmse of all pixels.
 * Records whose key ties with a threshold key contribute their mean error and mean squared error for the number of
 * them that survive. */
int mimo_eval_interval_sums(const uint64_t* records, int64_t num_records, int32_t num_percentiles, int32_t num_thresholds,
                            void* workspace, double* out, mimo_stream stream);
/* ---- sparsification error (Ilg et al. 2018, Poggi et al. 2020): the same curve per uncertainty source and the oracle
 * curve (pixels dropped by their own error), from which the host forms AUSE and AURG.
 * mimo_eval_accumulate with a second store, written at the same slot from the one read of the maps:
 * source_records: one uint64 per pixel (low word: bit pattern of sqrtf(aleatoric_var), high word: of sqrtf(epistemic_var),
 * both with -0 canonicalised to +0).  Records, counters and running sums are those of mimo_eval_accumulate, bit for bit.
 * A skipped pixel has 0xFFFFFFFF in EVERY word of both of its records (written by both entry points), so any of the four
 * words can serve as a key: the later passes step over a slot whose key is that pattern and never read its error. */
int mimo_eval_accumulate_sources(const float* mean, const float* aleatoric_var, const float* epistemic_var,
                                 const float* label, const float* mask, int32_t batch, int32_t channels, int32_t channel,
                                 int32_t mask_channels, int64_t hw, int32_t clip, float clip_lo, float clip_hi,
                                 const float* thresholds, int32_t num_thresholds, uint64_t* records,
                                 uint64_t* source_records, void* workspace, mimo_stream stream);
/* mimo_eval_select over any key word: record i's key is keys[i * key_stride_words], the bit pattern of a non-negative
 * float or 0xFFFFFFFF (skipped).  The four orderings: combined = (uint32*)records, aleatoric = (uint32*)source_records,
 * epistemic = (uint32*)source_records + 1, oracle = (uint32*)records + 1, each with a stride of 2 words.  The workspace must
 * hold the counters of the accumulate passes that wrote the records; every call resets the select state it uses, so the
 * orderings run one after another on one workspace and one stream (select, then interval sums, per ordering). */
int mimo_eval_select_by(const uint32_t* keys, int32_t key_stride_words, int64_t num_records, const double* percentiles,
                        int32_t num_percentiles, void* workspace, mimo_stream stream);
/* mimo_eval_interval_sums after mimo_eval_select_by on the same keys; record i's error is errors[i * error_stride_words]
 * ((uint32*)records + 1, stride 2, in all four orderings).  num_thresholds > 0: out as for mimo_eval_interval_sums;
 * num_thresholds == 0: out is doubles [3 * num_percentiles] = mae | rmse | threshold key only.  One output buffer of the
 * caller holds [3 P + K + 6] of the combined ordering followed by one [3 P] slice per further ordering. */
int mimo_eval_interval_sums_by(const uint32_t* keys, int32_t key_stride_words, const uint32_t* errors,
                               int32_t error_stride_words, int64_t num_records, int32_t num_percentiles,
                               int32_t num_thresholds, void* workspace, double* out, mimo_stream stream);

/* ---- proper scoring rules of the ensemble's mixture predictive: per pixel the equal-weight mixture of the `members`
 * densities an EnsembleModule leaves in HBM (return_raw_predictions) is scored at the label by its probability integral
 * transform (PIT), its negative log-likelihood (natural log, the full density) and its CRPS, in one pass.  Member scale
 * as the loss trains it: theta = clamp(exp(p2), eps_min, eps_max), Laplace b = theta, Gaussian sigma^2 = theta; means and
 * labels are not clipped.  Asynchronous on the stream; no allocation, no synchronisation.
 * workspace: device memory of mimo_score_workspace_bytes() bytes, 16-byte aligned, zeroed by the caller to reset; the
 * calls that share it must be issued on one stream. */
size_t mimo_score_workspace_bytes(void);
/* p1 / p2 [batch,members,channels,hw] fp32 contiguous and label [batch,channels,hw], of which plane `channel` is used;
 * mask [batch,mask_channels,hw] (mask_channels 1 or channels) or NULL.  A pixel with mask == 0 is skipped and counted in
 * n_masked; otherwise one whose label or any member's p1 / p2 is not finite is skipped and counted in n_nonfinite.
 * expected_p: device [num_thresholds <= 64] ascending fp32 thresholds of the PIT histogram: a pixel goes to the first bin k
 * with PIT < expected_p[k], to bin num_thresholds when there is none.  pit_map / nll_map / crps_map: [batch,hw] each or
 * NULL; a skipped pixel gets NaN.  The counters do not depend on which maps are requested; the same sequence of calls gives
 * the same bits (double sums in a fixed order, integer counts).  MIMO_ERR_INVALID with nothing launched: members outside
 * 1 ... 64, num_thresholds outside 1 ... 64, an unknown loss_kind, eps_min <= 0 or eps_max < eps_min or not finite, a
 * null p1 / p2 / label / expected_p / workspace, a pointer that is not 4-byte aligned. */
int mimo_score_accumulate(const float* p1, const float* p2, const float* label, const float* mask, int32_t batch,
                          int32_t members, int32_t channels, int32_t channel, int32_t mask_channels, int64_t hw,
                          int32_t loss_kind, float eps_min, float eps_max, const float* expected_p, int32_t num_thresholds,
                          float* pit_map, float* nll_map, float* crps_map, void* workspace, mimo_stream stream);
/* The same three rules for the evidential model: the posterior predictive of the Normal-Inverse-Gamma heads at a pixel,
 * scored into the same workspace (a mixture call and an evidential call on one workspace add up; mimo_score_finalize
 * serves both).  logits [batch,4,hw] fp32 contiguous; the heads are (mu, v, alpha, beta) = (l0, softplus(l1),
 * softplus(l2) + 1, softplus(l3)) (softplus with threshold 20), v, alpha and beta fp32 values.  The predictive is
 * Student-t with nu = 2 alpha degrees of freedom, location mu and scale sigma = sqrt(beta (1 + v) / (v alpha)).  With
 * z = (y - mu) / sigma and x = nu / (nu + z^2):
 *   PIT   u = F_nu(z) = I_x(nu/2, 1/2) / 2 for z <= 0, 1 - I_x(nu/2, 1/2) / 2 for z > 0 (I the regularised incomplete beta
 *         function; u == 0.5 exactly at z == 0)
 *   NLL   -lgamma(alpha + 1/2) + lgamma(alpha) + ln(nu pi) / 2 + ln sigma + (alpha + 1/2) log1p(z^2 / nu)
 *   CRPS  sigma [ z (2 F_nu(z) - 1) + 2 f_nu(z) (nu + z^2) / (nu - 1)
 *                 - 2 sqrt(nu) / (nu - 1) B(1/2, nu - 1/2) / B(1/2, nu/2)^2 ]        (Jordan, Krueger, Lerch 2019)
 *         f_nu the standard Student-t density; valid for nu > 1, and nu >= 2 here.
 * Evaluated in double from the fp32 heads and rounded once into the fp32 maps; means and labels are not clipped.
 * label [batch,1,hw]; mask [batch,hw] or NULL; maps [batch,hw] or NULL; expected_p and workspace as above.  A pixel with
 * mask == 0 is skipped and counted in n_masked; otherwise one whose label or any of its four logits is not finite, or whose
 * v or beta is 0 (the fp32 softplus has underflowed: l < -103), is skipped and counted in n_nonfinite; alpha == 1 exactly
 * is scored.  A skipped pixel gets NaN in every map.  Workspace word 71 keeps the most iterations the incomplete-beta
 * continued fraction of any pixel took (at most its compile-time cap; a diagnostic, not read by mimo_score_finalize).
 * MIMO_ERR_INVALID with nothing launched: a null logits / label / expected_p / workspace, batch < 1, hw < 1,
 * num_thresholds outside 1 ... 64, a pointer that is not 4-byte aligned. */
int mimo_score_accumulate_evidential(const float* logits, const float* label, const float* mask, int32_t batch, int64_t hw,
                                     const float* expected_p, int32_t num_thresholds, float* pit_map, float* nll_map,
                                     float* crps_map, void* workspace, mimo_stream stream);
/* out: device doubles [num_thresholds + 6] = the share of scored pixels with PIT < expected_p[k] per threshold, then n,
 * n_masked, n_nonfinite, mean NLL, mean CRPS, mean PIT (the shares and the means are NaN at n == 0). */
int mimo_score_finalize(const void* workspace, int32_t num_thresholds, double* out, mimo_stream stream);

/* ---- single-operator entry points (NHWC, channel-padded) used by the parity tests -------
 * They run the same kernels the plan runs.  x [N,H,W,cin_p], w OIHW [cout][cin][3][3]. */
int mimo_op_conv3x3_forward(const float* x, const float* w, const float* bias, float* z, double* stats,
                            int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cin_p, int32_t cout,
                            int32_t cout_p, int32_t precision, mimo_stream stream);
int mimo_op_conv3x3_dgrad(const float* dz, const float* w, float* dx, int32_t n, int32_t h, int32_t wd,
                          int32_t cin, int32_t cin_p, int32_t cout, int32_t cout_p, int32_t precision,
                          mimo_stream stream);
int mimo_op_conv3x3_wgrad(const float* x, const float* dz, float* dw, float* dbias, int32_t n, int32_t h,
                          int32_t wd, int32_t cin, int32_t cin_p, int32_t cout, int32_t cout_p, int32_t precision,
                          mimo_stream stream);
int mimo_op_maxpool2x2(const float* x, float* y, int32_t n, int32_t h, int32_t w, int32_t c_p, mimo_stream stream);
int mimo_op_upsample_cat(const float* skip, const float* low, float* out, int32_t n, int32_t hs, int32_t ws,
                         int32_t cs_p, int32_t hl, int32_t wl, int32_t cl_p, mimo_stream stream);

/* ---- single-operator entry points of the backward element-wise kernels (ew_bn_bwd.hip, ew_head_loss.hip) -------
 * NHWC fp32 tensors whose channel count c_p is a multiple of 8; "ld*" = elements per pixel of the buffer a pointer indexes
 * (a tensor may be a channel slice of a wider buffer; pitches and channel offsets are multiples of 4).  "dxpad" is a
 * gradient on the reflect-padded domain [n, h + 2, w + 2, ldp], as the data-gradient convolution leaves it; fold = the
 * transpose of the 1-pixel reflect padding (utils.py / components.py:17 padding_mode="reflect").
 * precision: MIMO_PREC_FP32 runs the fp32-storage kernels; MIMO_PREC_BF16_MIXED / MIMO_PREC_FP16_MIXED round every
 * activation-like buffer (whole buffers, at their pitch) into bf16 / fp16 copies, run the 16-bit storage kernels on those and
 * widen the outputs again; every other value is treated as fp32 storage.
 * MIMO_ERR_INVALID, with nothing launched: h or w < 2 (no reflect fold), c_p % 8 != 0, a pitch that does not hold its slice,
 * and what each function lists. */
/* da[n,h,w] (ldda) (=|+=) fold(dxpad)[..., choff : choff + c_p] */
int mimo_op_fold_slice(const float* dxpad, int32_t ldp, int32_t choff, float* da, int32_t ldda, int32_t n, int32_t h,
                       int32_t w, int32_t c_p, int32_t accumulate, int32_t precision, mimo_stream stream);
/* MaxPool2d(2) backward (components.py:48): da[n,h,w] (ldda) (=|+=) the gradient fold(dxpad [n, h/2 + 2, w/2 + 2])[...,
 * choff : choff + c_p] routed to the first maximum, in scan order (0,0),(0,1),(1,0),(1,1), of each 2x2 window of a (lda);
 * the last row / column of an odd size receives none.  skip != NULL: + fold(skip [n, h + 2, w + 2] (ldsk))[..., 0 : c_p].
 * The pooled tensor is the folded one: h / 2 and w / 2 >= 2. */
int mimo_op_pool_backward(const float* dxpad, int32_t ldp, int32_t choff, const float* a, int32_t lda, const float* skip,
                          int32_t ldsk, float* da, int32_t ldda, int32_t n, int32_t h, int32_t w, int32_t c_p,
                          int32_t accumulate, int32_t precision, mimo_stream stream);
/* Upsample(x2, bilinear, align_corners=True) + F.pad backward (components.py:78,110-117): da[n,hl,wl] (ldda) (=|+=) the
 * transposed interpolation of fold(dxpad [n, hs + 2, ws + 2])[..., choff : choff + c_p].  hs / 2 == hl and ws / 2 == wl. */
int mimo_op_up_backward(const float* dxpad, int32_t ldp, int32_t choff, float* da, int32_t ldda, int32_t n, int32_t hs,
                        int32_t ws, int32_t hl, int32_t wl, int32_t c_p, int32_t accumulate, int32_t precision,
                        mimo_stream stream);

/* BatchNorm2d + ReLU (+ Dropout2d) backward (components.py:24-29) of one layer, the chain the plan runs: the reduction pass,
 * the column sums, the apply pass and, in eval mode, the column sums of dz.
 *   dy = g * mask[n][c] * [z * scale + shift > 0];   s1 = sum dy;   s2 = sum dy * (z - mean) * invstd
 *   training: dz = scale * (dy - s1 / count - xhat * s2 / count), dgamma = s2, dbeta = s1, dbias = 0 (exactly)
 *   eval:     dz = scale * dy, dbias = sum dz
 * g, the gradient arriving at the activation, comes from `kind`:
 *   0  da [n,h,w] (ldda)
 *   1  fold(dxpad [n, h + 2, w + 2] (ldp))[..., 0 : c_p]   (choff must be 0)
 *   2  mimo_op_pool_backward's result for dxpad / choff / skip / ldsk (+ skoff) with the window's activations re-formed as
 *      relu(fma(z, scale, shift)) * mask — never written
 *   3  mimo_op_head_backward's da for head_* / loss_kind / eps_* with in_scale / in_shift = scale / shift — never written;
 *      head_dw / head_db receive the head's parameter gradients
 * Kinds 2 and 3 exist for fp32 storage and (3) head_co == 2 only: MIMO_ERR_INVALID otherwise. */
typedef struct mimo_op_bn_relu_backward_args {
  int32_t kind, n, h, w, c, c_p; /* c logical channels of c_p */
  int32_t training, split_out, precision;
  const float* da; /* kind 0 */
  int32_t ldda;
  const float* dxpad; /* kinds 1, 2 */
  int32_t ldp, choff;
  const float* skip; /* kind 2, or NULL */
  int32_t ldsk, skoff;
  /* kind 3: w [2][c]; logits out, dout [n][subnetworks][2][h*w]; dloss [subnetworks]; label, mask [n][h*w] (mask or
   * NULL); perm [subnetworks][n] or NULL — the arguments of mimo_loss_forward / mimo_backward */
  const float *head_w, *head_out, *head_dout, *head_dloss, *head_label, *head_mask;
  const int64_t* head_perm;
  int32_t head_co, head_subnetworks, head_s, loss_kind;
  float eps_min, eps_max;
  const float* z; /* the convolution output [n,h,w] (ldz) */
  int32_t ldz;
  const float *scale, *shift, *mean, *invstd; /* [c_p] */
  const float* mask;                          /* Dropout2d multipliers [n][c], or NULL */
  /* outputs (device).  dz [n,h,w,c_p]; split_out = 1 (fp32 storage): the same bytes hold, per pixel and 32-channel chunk,
   * [hi: bf16 x 32 | lo: bf16 x 32] with dz ~= hi + lo (a last chunk of r channels: [hi r | lo r]) */
  float* dz;
  float *dgamma, *dbeta, *dbias; /* [c]; dbias is required in eval mode */
  float *c1, *c2;                /* [c_p]: s1 / count, s2 / count (zeros in eval mode) */
  float *head_dw, *head_db;      /* kind 3: [2][c], [2] */
  float* absmax;                 /* NULL, or absmax_capacity >= 4096 floats: per-workgroup max |dz| */
  int32_t absmax_capacity;
  int32_t* absmax_n; /* host: slots written */
  int32_t* status;   /* host, or NULL: numerics status word (mimo_plan_status bits) */
} mimo_op_bn_relu_backward_args;
int mimo_op_bn_relu_backward(const mimo_op_bn_relu_backward_args* args, mimo_stream stream);

/* 1x1 head + NLL backward (components.py:126, losses.py:151-160) of subnetwork s:
 *   dlogit = dout + dloss[s] / count * mask * dNLL/dlogit   (count = n * (co / 2) * hw; the clamp of exp(log-scale) to
 *            [eps_min, eps_max] acts on the value only, d/dlog keeps the unclamped exp)
 *   da [n, hw, c_p] = W^T dlogit (padding channels zero), dw [co][c] = sum dlogit x a, db [co] = sum dlogit
 * a [n, hw] (lda): the head's input; in_scale / in_shift != NULL: the pre-activation tensor, relu(fma(a, scale, shift)) is
 * applied on the way in.  out, dout [n][subnetworks][co][hw]; label [n][co/2][hw]; mask [n][hw] or NULL; perm
 * [subnetworks][n] or NULL.  dout and / or dloss (with out and label).  c_p <= 256, co even and <= 8. */
typedef struct mimo_op_head_backward_args {
  const float* a;
  int32_t lda;
  const float* w; /* [co][c] */
  int32_t c, c_p, co, n, subnetworks, s;
  int64_t hw;
  const float *out, *dout, *dloss, *label, *mask;
  const int64_t* perm;
  int32_t loss_kind;
  float eps_min, eps_max;
  const float *in_scale, *in_shift;
  int32_t precision;
  float *da, *dw, *db;
} mimo_op_head_backward_args;
int mimo_op_head_backward(const mimo_op_head_backward_args* args, mimo_stream stream);

/* ---- single-operator entry points of the forward element-wise kernels (ew_bn_fwd.hip, ew_resample.hip, ew_dropout.hip, ew_head_loss.hip) -------
 * The conventions of the backward block above: fp32 NHWC tensors at the interface, c_p a multiple of 8, pitches multiples of
 * 4; MIMO_PREC_BF16_MIXED / MIMO_PREC_FP16_MIXED round whole activation-like buffers (at their pitch) into 16-bit copies,
 * run the 16-bit storage kernels and widen the outputs again (an output buffer makes the round trip as a whole: what the
 * kernel leaves unwritten comes back rounded to the storage type, a NaN as a NaN).  Statistics, BatchNorm vectors, Dropout2d
 * multipliers, weights, logits and losses are fp32 in every mode.  An invalid call returns MIMO_ERR_INVALID with nothing
 * launched and nothing written. */

/* BatchNorm2d statistics (components.py:24) from the partial rows [rows][2][cout_pad] of a convolution epilogue (row r: the
 * sums, then the sums of squares, of the channels over that workgroup's pixels; `count` elements per channel in all):
 *   mean = s1 / count, var = max(s2 / count - mean^2, 0), invstd = 1 / sqrt(var + eps), scale = gamma invstd,
 *   shift = beta - mean scale;  running_mean / running_var (in place) move by `momentum` towards mean and the unbiased
 *   variance var count / (count - 1) (var itself when count == 1);  channels [c, c_p) of the four vectors are zeros.
 * route: 1 = the one-launch column sum + finalize (rows <= 2048); 2 = the chunked row sum (at most 64 fp64 chunk rows)
 * followed by the finalize launch (the same status word); 0 = the plan's rule: "rows <= kColsumMaxRows (2048): the one
 * launch; otherwise row sum + finalize".  training = 0: mean / invstd / scale / shift from the running statistics instead
 * (partial, rows, count, route and momentum unused).  status (host, or NULL): bit 1 when a channel sum (eval: a running
 * statistic or its scale) is not finite.
 * Invalid: rows < 1, c < 1, c > c_p, c_p > cout_pad, c_p or cout_pad not a multiple of 8, count < 1, route outside 0..2,
 * route 1 with rows > 2048, a NULL tensor. */
enum mimo_bn_stats_route { MIMO_BN_ROUTE_PLAN = 0, MIMO_BN_ROUTE_ONE_LAUNCH = 1, MIMO_BN_ROUTE_ROWSUM = 2 };
typedef struct mimo_op_bn_stats_args {
  const float* partial;
  int32_t rows, cout_pad, c, c_p, training, route;
  int64_t count;
  const float *gamma, *beta;          /* [c] */
  float *running_mean, *running_var;  /* [c] */
  float momentum, eps;
  float *mean, *invstd, *scale, *shift; /* [c_p] */
  int32_t* status;
} mimo_op_bn_stats_args;
int mimo_op_bn_stats(const mimo_op_bn_stats_args* args, mimo_stream stream);

/* a[n,h,w] (lda) = relu(fma(z (ldz), scale, shift)) * mask[n][c] (mask: Dropout2d multipliers or NULL; channels [c, c_p) of
 * a masked call are zeros).  pool != NULL: the fused kernel, which also writes pool[n, h/2, w/2] (ldpool) = MaxPool2d(2)(a).
 * z_fp32 != 0 in a 16-bit mode: z stays fp32 (the image convolution's output), only a / pool are 16-bit.
 * status (host, or NULL): bit 1 when an element of z is not finite.
 * Invalid: bad dimensions or pitches, c outside [1, c_p], a NULL z / scale / shift / a, pool with h or w < 2. */
typedef struct mimo_op_bn_relu_forward_args {
  const float* z;
  int32_t ldz;
  const float *scale, *shift; /* [c_p] */
  const float* mask;          /* [n][c] or NULL */
  int32_t n, h, w, c, c_p, precision, z_fp32;
  float* a;
  int32_t lda;
  float* pool;
  int32_t ldpool;
  int32_t* status;
} mimo_op_bn_relu_forward_args;
int mimo_op_bn_relu_forward(const mimo_op_bn_relu_forward_args* args, mimo_stream stream);

/* mimo_op_maxpool2x2 with pitches and a storage mode: y[n, h/2, w/2] (ldo) = max over the 2x2 windows of x[n,h,w] (lda) */
int mimo_op_maxpool2x2_ex(const float* x, int32_t lda, float* y, int32_t ldo, int32_t n, int32_t h, int32_t w, int32_t c_p,
                          int32_t precision, mimo_stream stream);
/* mimo_op_upsample_cat with pitches, a storage mode and the producer's BatchNorm + ReLU: out[n,hs,ws,cs_p + cl_p] =
 * cat(skip (lds), zero_pad(bilinear_x2_align_corners(low [n,hl,wl] (ldl)))); lo_scale / lo_shift [cl_p] != NULL: low is a
 * pre-activation tensor and relu(fma(low, lo_scale, lo_shift)) is interpolated.  skip == NULL writes only the up-sampled
 * channels [cs_p, cs_p + cl_p) (with hs == 2 hl and ws == 2 wl: the kernel that works by 2x2 output blocks).
 * Invalid: bad dimensions or pitches, hs < 2 hl or ws < 2 wl, only one of lo_scale / lo_shift. */
int mimo_op_upsample_cat_ex(const float* skip, int32_t lds, const float* low, int32_t ldl, const float* lo_scale,
                            const float* lo_shift, float* out, int32_t n, int32_t hs, int32_t ws, int32_t cs_p, int32_t hl,
                            int32_t wl, int32_t cl_p, int32_t precision, mimo_stream stream);

/* 1x1 head (components.py:126): out[n][s][co'][yx] = bias[co'] + sum_{c' < c} a[n,yx,c'] w[co'][c'] for subnetwork s of
 * out [n][subnetworks][co][hw] (the other subnetworks are left alone).  a [n,hw] (lda >= c rounded up to 8; its padding
 * channels are read and multiplied by zero, so they must be finite); in_scale / in_shift [c rounded up to 8] != NULL: a is
 * the pre-activation tensor, relu(fma(a, in_scale, in_shift)) is applied on the way in.  status (host, or NULL): bit 4 when
 * a logit is not finite.
 * Invalid: c outside [1, 256], co outside [1, 8], n, hw < 1 or n hw >= 2^31, s outside [0, subnetworks), lda too small or
 * not a multiple of 4, only one of in_scale / in_shift, a NULL tensor. */
typedef struct mimo_op_head_forward_args {
  const float* a;
  int32_t lda;
  const float *w, *bias; /* [co][c], [co] */
  int32_t c, co, n, subnetworks, s, hw;
  const float *in_scale, *in_shift;
  int32_t precision;
  float* out;
  int32_t* status;
} mimo_op_head_forward_args;
int mimo_op_head_forward(const mimo_op_head_forward_args* args, mimo_stream stream);

/* loss[s] = mean over n, target channel and pixel of mask * NLL(out[n][s][t] - label[perm[s][n]][t], out[n][s][co/2 + t])
 * (losses.py:151-160; mimo_loss_forward's arithmetic: fp32 terms, fp32 per-thread and per-workgroup sums, fp64 across
 * workgroups).  out [n][subnetworks][co][hw], label [n][co/2][hw], mask [n][hw] or NULL (indexed like the label), perm
 * [subnetworks][n] (device int64, every entry in [0, n)) or NULL.
 * Invalid: co odd or outside [2, 8], n, hw, subnetworks < 1, an unknown loss_kind, a perm entry outside [0, n), a NULL tensor. */
int mimo_op_loss_forward(const float* out, const float* label, const float* mask, const int64_t* perm, int32_t n,
                         int32_t subnetworks, int32_t co, int32_t hw, int32_t loss_kind, float eps_min, float eps_max,
                         float* loss, mimo_stream stream);

/* out[n,h,w,cp] = x[perm[s][n]][s][c'][y][x] for c' < c, zeros in channels [c, cp): the input gather of subnetwork s
 * (utils.py:38-48).  x is addressed as x + image * stride_n + s * stride_s + c' * h * w + yx (strides in elements) and holds
 * x_count elements.  Invalid: c outside [1, cp], cp not a multiple of 4, negative strides, an address beyond x_count, a perm
 * entry outside [0, n). */
int mimo_op_pack_input(const float* x, int64_t x_count, int64_t stride_n, int64_t stride_s, const int64_t* perm, int32_t s,
                       int32_t n, int32_t c, int32_t h, int32_t w, float* out, int32_t cp, mimo_stream stream);
/* dx[n][s][c'][y][x] = fold(dxpad [n, h + 2, w + 2] (ldp))[n][y][x][c'], c' < c, of dx [n][subnetworks][c][h][w] (fp32 in
 * every mode; dxpad in the storage type).  Invalid: h or w < 2, ldp % 4 != 0 or below c rounded up to 4, s outside
 * [0, subnetworks). */
int mimo_op_unpack_dx(const float* dxpad, int32_t ldp, int32_t n, int32_t subnetworks, int32_t s, int32_t c, int32_t h,
                      int32_t w, int32_t precision, float* dx, mimo_stream stream);
/* dimage[n][c'][y][x] (=|+=) fold(dxpad)[n][y][x][c'] (fp32 storage) */
int mimo_op_fold_image_grad(const float* dxpad, int32_t ldp, int32_t n, int32_t c, int32_t h, int32_t w, float* dimage,
                            int32_t accumulate, mimo_stream stream);
/* dimage[b][c'][y][x] (=|+=) sum over m = 0 .. replicas-1, in that order, of fold(dxpad)[m * (n / replicas) + b][y][x][c']:
 * dxpad [n, h + 2, w + 2] (ldp) holds `replicas` passes of n / replicas images, pass-major; dimage [n / replicas][c][h][w].
 * replicas = 1: the bits of mimo_op_fold_image_grad.  Invalid additionally: replicas < 1 or not a divisor of n. */
int mimo_op_fold_image_grad_mc(const float* dxpad, int32_t ldp, int32_t n, int32_t replicas, int32_t c, int32_t h, int32_t w,
                               float* dimage, int32_t accumulate, mimo_stream stream);

/* ---- output monitor: replaces, per log event, the image pipeline of the reference's OutputMonitor callbacks
 * (mimo/tasks/depth/callbacks.py:18-144, mimo/tasks/sen12tp/callbacks.py:12-141): for every panel the first `count`
 * images of a step-output map, torchvision.utils.make_grid and colorize (mimo/visualization.py:9-49) — there ~35 launches,
 * a synchronous copy of the fp32 grid to the host and a matplotlib colormap on the host per panel; here one launch for all
 * panels of the event (two when a panel takes its range from the data), and an RGB uint8 image left on the device.
 *
 * Grid: count == 1: the image itself, Hg = h, Wg = w.  Otherwise xmaps = min(nrow, count), ymaps = ceil(count / xmaps),
 * Hg = ymaps (h + padding) + padding, Wg = xmaps (w + padding) + padding; image k starts at row (k / xmaps)(h + padding) +
 * padding, column (k % xmaps)(w + padding) + padding; every other grid pixel (empty cells of a ragged last row included)
 * has the value 0.
 * Value: src[k, channel, y, x], times mask[k, mc == 1 ? 0 : channel, y, x] when a mask is given, then |.| with flag bit 0.
 * Range: vmin / vmax as given, or with flag bits 1 / 2 the minimum / maximum over the whole grid (its zeros included); a
 * NaN anywhere makes such a bound NaN (torch.min / torch.max) and the panel comes out in the NaN colour.
 * Normalise, each operation rounded to fp32 on its own: vmin != vmax: t = (v - vmin) / (vmax - vmin) (IEEE division);
 * else t = v * 0; u = t * 256.
 * Colour (matplotlib's Colormap.__call__(float32, bytes=True)): NaN: lut[256]; u < 0: lut[0]; u > 255 (256 included):
 * lut[255]; else lut[(int)u].  Output: R, G, B bytes per pixel, [Hg, Wg, 3].
 *
 * mimo_monitor_grids: `panels` is a HOST array and travels in the kernel arguments; src, mask, lut, out and scratch are
 * device memory; scratch (mimo_monitor_scratch_bytes(n_panels) bytes, 4-byte aligned; may be NULL when no panel has flag
 * bit 1 or 2) is owned by the caller and reusable by ordered calls on one stream.  No allocation, no synchronisation.  An
 * image that starts on a 4-byte boundary (out + out_offset) is written in whole dwords, any other in bytes.
 * MIMO_ERR_INVALID with a message and nothing launched: n_panels outside 1 ... 8, count < 1 or > n, channel outside
 * [0, c), a mask with mc not in {1, c}, h or w < 2, nrow < 1, padding < 0, unknown flag bits, a null src / lut / out, a
 * grid of 2^29 pixels or more. */
typedef struct mimo_monitor_panel {
  const float* src;      /* [n, c, h, w] fp32, NCHW contiguous: a step-output map as it is */
  const float* mask;     /* NULL, or [n, mc, h, w] with mc = 1 or c: multiplied in before anything else */
  int32_t n, c, h, w, mc;
  int32_t channel;       /* which of the c channels is drawn */
  int32_t count;         /* images drawn: min(n, max_images), >= 1 */
  int32_t nrow, padding; /* make_grid's: 8 and 2 in the reference */
  int32_t flags;         /* bit 0: |x| before normalising (the depth monitor's error map)
                            bit 1: vmin is the grid minimum; bit 2: vmax is the grid maximum */
  float vmin, vmax;      /* used where the flag bit is clear */
  const uint32_t* lut;   /* device, 257 entries 0x00BBGGRR: 256 colours + the "bad" colour (NaN) */
  int64_t out_offset;    /* byte offset of this panel's [Hg, Wg, 3] uint8 image in `out` */
} mimo_monitor_panel;
enum { MIMO_MONITOR_ABS = 1, MIMO_MONITOR_AUTO_VMIN = 2, MIMO_MONITOR_AUTO_VMAX = 4, MIMO_MONITOR_MAX_PANELS = 8 };
int mimo_monitor_grid_shape(int count, int h, int w, int nrow, int padding, int* hg, int* wg);
size_t mimo_monitor_scratch_bytes(int n_panels);
int mimo_monitor_grids(const mimo_monitor_panel* panels, int n_panels, uint8_t* out, void* scratch, mimo_stream stream);

/* ---- resident data path: a batch gathered on the device from a dataset kept in HBM as the bytes it is stored in.
 * Replaces, per step, the reference's per-sample __getitem__ (mimo/datasets/nyuv2.py:38-53: index through
 * shuffle_permutation, `/ 255.0` in float64, torch.tensor, permute(2, 0, 1), .float()), the DataLoader's collate and the
 * upload of the batch: one launch for all fields (image, label) of the batch.
 *
 * Per field f, batch row b, channel k, pixel (y, x):
 *   i = clamp(index[b], 0, n_samples - 1);  j = remap ? clamp(remap[i], 0, n_samples - 1) : i;
 *   dst_f[b, k, y, x] = lut_f[src_f[j, y, x, k]]
 * The clamps are part of the definition: no address is formed from an index outside the store, whatever the caller passes.
 * The normalisation is the table: (arange(256) / divisor) rounded once to fp32 reproduces the reference's float64 quotient
 * followed by .float() bit for bit; float(i) is the identity (normalize=False).
 *
 * `fields` is a HOST array and travels in the kernel arguments; src, lut, dst, index and remap are device memory.  All
 * fields share n_samples, batch, h and w.  A field whose src is 4-byte aligned, with h * w a multiple of 4, is read in
 * dwords, any other in bytes; a destination quad on a 16-byte boundary is written as one float4, any other as scalars.
 * No allocation, no synchronisation.  MIMO_ERR_INVALID with a message and nothing launched: n_fields outside 1 ... 4, c
 * outside 1 ... 4, a null fields / index / src / lut / dst, a lut or dst that is not 4-byte aligned, batch, h, w or
 * n_samples < 1, batch * h * w * 4 >= 2^31, n_samples * h * w * 4 > 2^62. */
typedef struct mimo_gather_field {
  const uint8_t* src;    /* [n_samples, h, w, c] bytes, contiguous */
  const float* lut;      /* 256 floats */
  float* dst;            /* [batch, c, h, w] fp32, contiguous */
  int32_t c;             /* 1 ... 4 */
  int32_t reserved;
} mimo_gather_field;
enum { MIMO_GATHER_MAX_FIELDS = 4 };
int mimo_dataset_gather(const mimo_gather_field* fields, int n_fields, const int64_t* index, const int64_t* remap,
                        int64_t n_samples, int32_t batch, int32_t h, int32_t w, mimo_stream stream);

/* ---- whole-scene inference: tiles gathered from a scene kept in HBM, and per-tile results stitched back into scene maps.
 * The reference only knows patches (SEN12TP scenes are cut into 256-pixel patches at a stride of 249 by the dataset,
 * scripts/test/test_ndvi.py:152-160, sen12tp_datamodule.py:54-66); the cutting, the overlaps and the seams are these two.
 *
 * Geometry.  Along an axis of length L with patch P and stride s, 1 <= s <= P <= L:
 *   tiles        n = 1 + ceil((L - P) / s)
 *   origins      o_k = min(k s, L - P)            (the last tile is shifted inwards, never padded)
 *   covering     K(p) = {k : o_k <= p < o_k + P}  (a contiguous range, never empty)
 * Tiles of a scene [h, w] are numbered row-major, t = ky nx + kx, T = ny nx, with origin (oy(t), ox(t)) = (o_ky, o_kx).
 *
 * Windows, for i in [0, P):  MIMO_WINDOW_UNIFORM w(i) = 1;  MIMO_WINDOW_LINEAR w(i) = min(i + 1, P - i);
 * MIMO_WINDOW_CROP: weight 1 for the owner of p and 0 for every other tile, the owner being the k in K(p) with the largest
 * linear weight w(p - o_k), ties to the lowest k ("keep the centre of each tile").
 * Normalised 1-D weight (uniform, linear), in fp32:  a_k(p) = w(p - o_k) / sum over ascending j in K(p) of w(p - o_j) — the
 * terms are small integers, the sum is exact, the division is the one correctly rounded operation.  The 2-D weight of tile
 * t at (y, x) is fl(a_ky(y) a_kx(x)).  The normalisation is separable: no weight-sum buffer, no finalising pass.
 *
 * mimo_scene_gather_tiles: scene [c, h, w] fp32 -> dst [n, c, P, P] fp32, both contiguous device memory,
 *   dst[b, k, y, x] = scene[k, oy(t) + y, ox(t) + x],  t = min(t0 + b, T - 1).
 * The clamp is part of the definition: the last, short batch of a scene repeats the last tile and keeps the call shape of
 * all the others.  Quads of a tile row move as one float4 where they lie on a 16-byte boundary (source and destination
 * judged separately), as scalars otherwise.  MIMO_ERR_INVALID with a message and nothing launched: a null or not 4-byte
 * aligned scene / dst, c, h, w, patch, stride or n < 1, patch > h or w, stride > patch, t0 outside [0, T),
 * n * c * P * P >= 2^31, c * h * w > 2^60.
 *
 * mimo_scene_stitch: adds tiles t0 ... t0 + n_valid - 1 into up to 4 scene maps at once.  `fields` is a HOST array and
 * travels in the kernel arguments; field f has a source [n, c_f, P, P] (row b is tile t0 + b; rows >= n_valid are not read)
 * and a destination [c_f, h, w], fp32, contiguous device memory.  For every pixel (y, x) of every channel that at least
 * one tile of the launch covers, with the covering tiles of the launch taken in ascending t:
 *   uniform, linear:  acc = (lowest covering tile overall < t0) ? dst : nothing;
 *                     per tile:  term = fl(a_t v_t);  acc = acc is nothing ? term : fl(acc + term);   dst = acc
 *   crop:             dst = v_owner where the owner is a tile of the launch, untouched otherwise
 * Every multiply and add rounds to nearest on its own (no fused multiply-add).  A pixel whose lowest covering tile lies in
 * the launch is STORED, any other is read, added to and stored: the destination needs no memset, provided the launches of
 * a scene cover 0 ... T - 1 in ascending order on one stream.  The per-pixel order is ascending t whatever the batch
 * size, so the stitched scene is bit-identical for any batching of the same tile values.  Pixels covered by no tile of
 * the launch are not touched.  No allocation, no synchronisation, no atomics.  MIMO_ERR_INVALID with a message and
 * nothing launched: n_fields outside 1 ... 4, a null table / src / dst, a src or dst not 4-byte aligned, c_f outside
 * 1 ... 65535, h, w, patch or stride < 1, patch > h or w, stride > patch, patch > 4096 (the window sums stay exact in
 * fp32), an unknown window, t0 < 0, n_valid < 1, t0 + n_valid > T, h * w >= 2^31,
 * n_valid * c_f * P * P > 2^60. */
enum { MIMO_WINDOW_UNIFORM = 0, MIMO_WINDOW_LINEAR = 1, MIMO_WINDOW_CROP = 2 };
int mimo_scene_gather_tiles(const float* scene, float* dst, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t stride,
                            int32_t t0, int32_t n, mimo_stream stream);
typedef struct mimo_stitch_field {
  const float* src;      /* [n, c, P, P] fp32, contiguous */
  float* dst;            /* [c, h, w] fp32, contiguous */
  int32_t c;             /* 1 ... 65535 */
  int32_t reserved;
} mimo_stitch_field;
enum { MIMO_STITCH_MAX_FIELDS = 4 };
int mimo_scene_stitch(const mimo_stitch_field* fields, int n_fields, int32_t h, int32_t w, int32_t patch, int32_t stride,
                      int32_t window, int32_t t0, int32_t n_valid, mimo_stream stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MIMO_HIP_H */
