// Evaluation of the evidential model on the device, gfx950: the three maps a test loop reads, and the logit gradient of the
// mean loss an FGSM attack starts from.
//
// Replaces (reference): scripts/test/test_nyuv2_depth_evidential.py:42-65 (and the same lines of test_ndvi_evidential.py) —
//   loss = model.loss_fn(out, labels).mean(); loss.backward()                      -> mimo_evidential_loss_gradient
//   EvidentialLoss.mode / aleatoric_var / epistemic_var, mimo/losses.py:258-271    -> mimo_evidential_uncertainties
//
// mimo_evidential_uncertainties: one streaming pass over the backbone logits [N,4,HW].  16 B read and 12 B written per pixel;
// four consecutive pixels per thread and step (one float4 of each logit plane, one float4 store per map) where HW is a
// multiple of 4 and every pointer is 16-byte aligned, one pixel per thread and step otherwise.  Grid-stride, no LDS, no
// atomics.  The arithmetic is the head of evidential_fwd_kernel (nig_head, evidential.h) followed by the reference's three
// formulas in fp32: alpha = softplus(l2) + 1 is rounded first and alpha - 1 is taken of that, as the reference takes it of
// the stored alpha.  Infinities and NaNs (alpha - 1 == 0, v == 0) are written as they come: mimo_eval_accumulate counts and
// skips non-finite pixels.
//
// mimo_evidential_loss_gradient: dlogits = d(scale * sum over pixels of loss_map) / d logits — evidential_bwd_kernel with
// d_ev = NULL and d_loss = scale everywhere, through the same device function (nig_bwd_pixel, evidential.h), without a
// [N,HW] weight tensor or the launch that fills it.
//
// Training / validation step of the same model (reference: mimo/models/evidential_unet.py:98-146, mimo/losses.py:258-271,
// mimo/metrics.py:22-34) —
//   loss.mean(), aleatoric_var ** 0.5, epistemic_var ** 0.5, y_pred - label, the two clip(0, 5).mean() and
//   compute_regression_metrics after the head                                        -> mimo_evidential_step
//   the backward of that mean under any upstream gradient held on the device         -> mimo_evidential_loss_gradient_dev
// mimo_evidential_step: one streaming pass, 20 B read (24 with a mask) and 8 B written per pixel (12 with the epistemic
// map), the same two access widths as mimo_evidential_uncertainties; double sums per thread, an LDS tree per workgroup, one
// partial row per workgroup and a one-workgroup finalize kernel — no atomics.
//
// The head and loss themselves, with their backward (mimo_evidential_forward / mimo_evidential_backward), come first: every
// kernel of this file runs the same device functions of evidential.h.  The sums of the step kernels: block_reduce.h.
#include <algorithm>
#include <cstdint>

#include "block_reduce.h"
#include "common.h"
#include "evidential.h"

namespace mimo {
namespace {

// ---------------------------------------------------------------------------------------
// Evidential regression head + loss (mimo/models/evidential_unet.py:74-96, mimo/losses.py:202-247):
//   (mu, v, alpha, beta) = (l0, softplus(l1), softplus(l2) + 1, softplus(l3))
//   loss = G(alpha) / (v sqrt(beta)) * (2 beta (1 + v) + (2 alpha - 1) v (y - mu)^2) + (y - mu)^2 (2 alpha + v),
//   G(alpha) = Gamma(alpha - 1/2) / (4 Gamma(alpha))
// One pass for the four NIG parameters + the per-pixel loss, one pass for the gradient w.r.t. the logits (analytic:
// dG/dalpha = G (psi(alpha - 1/2) - psi(alpha))) instead of ~40 element-wise tensor operations and their autograd
// nodes.  G is evaluated as exp(lgamma(alpha - 1/2) - lgamma(alpha)) / 4 — the reference exponentiates the two
// lgammas separately, which overflows fp32 (inf / inf = nan) for alpha > 35; this form stays finite there.
// ---------------------------------------------------------------------------------------
// (softplus_f, nig_point and the loss gradient: evidential.h)
__global__ void evidential_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ label,
                                      const float* __restrict__ mask, int64_t total, int64_t hw, float* __restrict__ ev,
                                      float* __restrict__ loss) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / hw, r = i - n * hw;
    const float* l = logits + n * 4 * hw + r;
    const NigPoint q = nig_point(l[0], l[hw], l[2 * hw], l[3 * hw], label ? label[i] : 0.f);
    float* e = ev + n * 4 * hw + r;
    e[0] = q.mu;
    e[hw] = q.v;
    e[2 * hw] = q.alpha;
    e[3 * hw] = q.beta;
    if (loss && label) {
      const float sq = q.d * q.d;
      float v = q.c * q.T + sq * (2.f * q.alpha + q.v);
      if (mask) v *= mask[i];
      loss[i] = v;
    }
  }
}

// dlogits = d_loss * dloss/dlogits (+ d_ev * dev/dlogits): both upstream gradients optional
__global__ void evidential_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ label,
                                      const float* __restrict__ mask, const float* __restrict__ d_ev,
                                      const float* __restrict__ d_loss, int64_t total, int64_t hw, float* __restrict__ dlogits) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    nig_bwd_pixel(logits, label, mask, d_ev, NigUpTensor{d_loss}, i, hw, dlogits);
  }
}

struct NigVars {
  float aleatoric, epistemic;
};
__device__ __forceinline__ NigVars nig_vars(float l1, float l2, float l3) {
  const NigHead h = nig_head(l1, l2, l3);
  const float am1 = h.alpha - 1.f;  // of the rounded alpha
  return NigVars{h.beta / am1, h.beta / (h.v * am1)};
}

// VEC: hw is a multiple of 4 and every pointer is 16-byte aligned (then every plane n * 4 * hw + c * hw is too)
template <bool VEC>
__global__ __launch_bounds__(256) void evidential_uncertainties_kernel(const float* __restrict__ logits, int64_t total, int64_t hw,
                                                                      float* __restrict__ mean, float* __restrict__ aleatoric,
                                                                      float* __restrict__ epistemic) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (VEC) {
    const int64_t quads = total >> 2, hwq = hw >> 2;
    for (int64_t q = first; q < quads; q += stride) {
      const int64_t n = q / hwq, r = (q - n * hwq) << 2;
      const float* l = logits + n * 4 * hw + r;
      const float4 l0 = *reinterpret_cast<const float4*>(l);
      const float4 l1 = *reinterpret_cast<const float4*>(l + hw);
      const float4 l2 = *reinterpret_cast<const float4*>(l + 2 * hw);
      const float4 l3 = *reinterpret_cast<const float4*>(l + 3 * hw);
      const NigVars a = nig_vars(l1.x, l2.x, l3.x), b = nig_vars(l1.y, l2.y, l3.y), c = nig_vars(l1.z, l2.z, l3.z),
                    d = nig_vars(l1.w, l2.w, l3.w);
      reinterpret_cast<float4*>(mean)[q] = l0;
      reinterpret_cast<float4*>(aleatoric)[q] = make_float4(a.aleatoric, b.aleatoric, c.aleatoric, d.aleatoric);
      reinterpret_cast<float4*>(epistemic)[q] = make_float4(a.epistemic, b.epistemic, c.epistemic, d.epistemic);
    }
  } else {
    for (int64_t i = first; i < total; i += stride) {
      const int64_t n = i / hw, r = i - n * hw;
      const float* l = logits + n * 4 * hw + r;
      const NigVars a = nig_vars(l[hw], l[2 * hw], l[3 * hw]);
      mean[i] = l[0];
      aleatoric[i] = a.aleatoric;
      epistemic[i] = a.epistemic;
    }
  }
}

// evidential_bwd_kernel's loop with d_ev = NULL and d_loss[i] = scale
__global__ __launch_bounds__(256) void evidential_loss_gradient_kernel(const float* __restrict__ logits, const float* __restrict__ label,
                                                                      const float* __restrict__ mask, int64_t total, int64_t hw,
                                                                      float scale, float* __restrict__ dlogits) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    nig_bwd_pixel(logits, label, mask, nullptr, NigUpConst{scale}, i, hw, dlogits);
  }
}

// evidential_loss_gradient_kernel with the upstream gradient of the reduced loss read from the device: every thread forms
// s = scale * upstream[0] (one fp32 multiplication) and runs the same device function on NigUpConst{s}
__global__ __launch_bounds__(256) void evidential_loss_gradient_dev_kernel(const float* __restrict__ logits, const float* __restrict__ label,
                                                                          const float* __restrict__ mask, int64_t total, int64_t hw,
                                                                          float scale, const float* __restrict__ upstream,
                                                                          float* __restrict__ dlogits) {
  const float s = scale * upstream[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    nig_bwd_pixel(logits, label, mask, nullptr, NigUpConst{s}, i, hw, dlogits);
  }
}

// ---------------------------------------------------------------------------------------
// Step tail of EvidentialUnetModel.training_step / validation_step (mimo/models/evidential_unet.py:98-146) after the
// backbone: the two standard deviations (losses.py:258-271, sqrt of the variances), the error map, the mean of the masked
// loss map and the sums behind compute_regression_metrics (metrics.py:22-34) and the two clipped uncertainty means — one
// pass over the logits, double accumulators per thread, one partial row per workgroup; a one-workgroup second pass turns
// the rows into the eight scalars in a fixed order (no atomics: the same bits every run).
// ---------------------------------------------------------------------------------------
constexpr int kStepSums = 7;  // loss, err^2, |err|, y, y^2, clip(alea_std), clip(epi_std)

struct NigStep {
  float alea_std, epi_std, err, loss;
};
// m: the pixel's mask value (1 without a mask: the product is then exact); epi_std only when wanted (0 otherwise)
__device__ __forceinline__ NigStep nig_step(float l0, float l1, float l2, float l3, float y, float m, bool masked, bool want_epi) {
  const NigPoint q = nig_point(l0, l1, l2, l3, y);
  const float am1 = q.alpha - 1.f;  // of the rounded alpha, as nig_vars
  const float sq = q.d * q.d;
  NigStep r;
  r.alea_std = sqrtf(q.beta / am1);
  r.epi_std = want_epi ? sqrtf(q.beta / (q.v * am1)) : 0.f;
  r.err = l0 - y;
  r.loss = q.c * q.T + sq * (2.f * q.alpha + q.v);  // evidential_fwd_kernel's expression
  if (masked) r.loss *= m;
  return r;
}
__device__ __forceinline__ float clip05(float x) { return fminf(fmaxf(x, 0.f), 5.f); }  // inf -> 5, as torch.clip
__device__ __forceinline__ void step_accumulate(double (&acc)[kStepSums], const NigStep& r, float y) {
  acc[0] += r.loss;
  acc[1] += (double)r.err * r.err;
  acc[2] += fabsf(r.err);
  acc[3] += y;
  acc[4] += (double)y * y;
  acc[5] += clip05(r.alea_std);
  acc[6] += clip05(r.epi_std);
}

// VEC: hw is a multiple of 4 and every pointer is 16-byte aligned.  epi_std == NULL: not wanted (a uniform branch, so that
// everything else is the same code with and without it).
template <bool VEC>
__global__ __launch_bounds__(256) void evidential_step_kernel(const float* __restrict__ logits, const float* __restrict__ label,
                                                             const float* __restrict__ mask, int64_t total, int64_t hw,
                                                             float* __restrict__ alea_std, float* __restrict__ epi_std,
                                                             float* __restrict__ err, double* __restrict__ partial) {
  const bool masked = mask != nullptr, want_epi = epi_std != nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double acc[kStepSums];
#pragma unroll
  for (int k = 0; k < kStepSums; ++k) acc[k] = 0.0;
  if constexpr (VEC) {
    const int64_t quads = total >> 2, hwq = hw >> 2;
    for (int64_t q = first; q < quads; q += stride) {
      const int64_t n = q / hwq, r = (q - n * hwq) << 2;
      const float* l = logits + n * 4 * hw + r;
      const float4 l0 = *reinterpret_cast<const float4*>(l);
      const float4 l1 = *reinterpret_cast<const float4*>(l + hw);
      const float4 l2 = *reinterpret_cast<const float4*>(l + 2 * hw);
      const float4 l3 = *reinterpret_cast<const float4*>(l + 3 * hw);
      const float4 y = reinterpret_cast<const float4*>(label)[q];
      const float4 m = masked ? reinterpret_cast<const float4*>(mask)[q] : make_float4(1.f, 1.f, 1.f, 1.f);
      const NigStep a = nig_step(l0.x, l1.x, l2.x, l3.x, y.x, m.x, masked, want_epi);
      const NigStep b = nig_step(l0.y, l1.y, l2.y, l3.y, y.y, m.y, masked, want_epi);
      const NigStep c = nig_step(l0.z, l1.z, l2.z, l3.z, y.z, m.z, masked, want_epi);
      const NigStep d = nig_step(l0.w, l1.w, l2.w, l3.w, y.w, m.w, masked, want_epi);
      reinterpret_cast<float4*>(alea_std)[q] = make_float4(a.alea_std, b.alea_std, c.alea_std, d.alea_std);
      if (want_epi) reinterpret_cast<float4*>(epi_std)[q] = make_float4(a.epi_std, b.epi_std, c.epi_std, d.epi_std);
      reinterpret_cast<float4*>(err)[q] = make_float4(a.err, b.err, c.err, d.err);
      step_accumulate(acc, a, y.x);
      step_accumulate(acc, b, y.y);
      step_accumulate(acc, c, y.z);
      step_accumulate(acc, d, y.w);
    }
  } else {
    for (int64_t i = first; i < total; i += stride) {
      const int64_t n = i / hw, r = i - n * hw;
      const float* l = logits + n * 4 * hw + r;
      const float y = label[i];
      const NigStep a = nig_step(l[0], l[hw], l[2 * hw], l[3 * hw], y, masked ? mask[i] : 1.f, masked, want_epi);
      alea_std[i] = a.alea_std;
      if (want_epi) epi_std[i] = a.epi_std;
      err[i] = a.err;
      step_accumulate(acc, a, y);
    }
  }
  const auto red = block_reduce_rows(acc);
  if (threadIdx.x < kStepSums) partial[(size_t)blockIdx.x * 8 + threadIdx.x] = red[threadIdx.x][0];
}

// scalars: write_step_scalars (block_reduce.h); [6] is 0 when the epistemic map was not wanted
__global__ __launch_bounds__(256) void evidential_step_finalize_kernel(const double* __restrict__ partial, int blocks, double count,
                                                                      float* __restrict__ scalars) {
  __shared__ double tot[kStepSums];
  double a[kStepSums];
#pragma unroll
  for (int k = 0; k < kStepSums; ++k) a[k] = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256)  // 256 threads walk the partial rows, then the fixed-order tree
#pragma unroll
    for (int k = 0; k < kStepSums; ++k) a[k] += partial[(size_t)b * 8 + k];
  const auto red = block_reduce_rows(a);
  if (threadIdx.x < kStepSums) tot[threadIdx.x] = red[threadIdx.x][0];
  __syncthreads();
  if (threadIdx.x == 0) write_step_scalars(tot, count, scalars);
}

}  // namespace
}  // namespace mimo

using namespace mimo;

extern "C" int mimo_evidential_forward(const float* logits, const float* label, const float* mask, int32_t n, int64_t hw,
                                       float* ev, float* loss_map, mimo_stream stream) {
  if (!logits || !ev || n < 0 || hw < 0 || (loss_map && !label)) {
    set_error("mimo_evidential_forward: invalid argument");
    return MIMO_ERR_INVALID;
  }
  const int64_t total = (int64_t)n * hw;
  if (total == 0) return MIMO_OK;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);
  hipLaunchKernelGGL(evidential_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, label, mask, total, hw, ev,
                     loss_map);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_evidential_backward(const float* logits, const float* label, const float* mask, const float* d_ev,
                                        const float* d_loss, int32_t n, int64_t hw, float* dlogits, mimo_stream stream) {
  if (!logits || !dlogits || n < 0 || hw < 0 || (d_loss && !label)) {
    set_error("mimo_evidential_backward: invalid argument");
    return MIMO_ERR_INVALID;
  }
  const int64_t total = (int64_t)n * hw;
  if (total == 0) return MIMO_OK;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);
  hipLaunchKernelGGL(evidential_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, label, mask, d_ev, d_loss,
                     total, hw, dlogits);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_evidential_uncertainties(const float* logits, int32_t n, int64_t hw, float* mean, float* aleatoric_var,
                                             float* epistemic_var, mimo_stream stream) {
  if (!logits || !mean || !aleatoric_var || !epistemic_var || n < 0 || hw < 0) {
    set_error("mimo_evidential_uncertainties: invalid argument");
    return MIMO_ERR_INVALID;
  }
  const int64_t total = (int64_t)n * hw;
  if (total == 0) return MIMO_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (hw & 3) == 0 &&
                   (((uintptr_t)logits | (uintptr_t)mean | (uintptr_t)aleatoric_var | (uintptr_t)epistemic_var) & 15) == 0;
  const int64_t units = vec ? total >> 2 : total;
  // grid-stride, 8 workgroups of 256 threads per CU at most (256 CUs), as mimo_fgsm_perturb
  const int blocks = (int)std::min<int64_t>(ceil_div64(units, 256), 2048);
  if (vec)
    hipLaunchKernelGGL(evidential_uncertainties_kernel<true>, dim3(blocks), dim3(256), 0, st, logits, total, hw, mean, aleatoric_var,
                       epistemic_var);
  else
    hipLaunchKernelGGL(evidential_uncertainties_kernel<false>, dim3(blocks), dim3(256), 0, st, logits, total, hw, mean, aleatoric_var,
                       epistemic_var);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_evidential_loss_gradient(const float* logits, const float* label, const float* mask, int32_t n, int64_t hw,
                                             float scale, float* dlogits, mimo_stream stream) {
  if (!logits || !label || !dlogits || n < 0 || hw < 0) {
    set_error("mimo_evidential_loss_gradient: invalid argument");
    return MIMO_ERR_INVALID;
  }
  const int64_t total = (int64_t)n * hw;
  if (total == 0) return MIMO_OK;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);  // mimo_evidential_backward's grid
  hipLaunchKernelGGL(evidential_loss_gradient_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, label, mask, total,
                     hw, scale, dlogits);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_evidential_step(const float* logits, const float* label, const float* mask, int32_t n, int64_t hw,
                                    float* aleatoric_std, float* epistemic_std, float* err, float* scalars, double* scratch,
                                    int32_t scratch_blocks, mimo_stream stream) {
  if (!logits || !label || !aleatoric_std || !err || !scalars || !scratch || n < 1 || hw < 1 || scratch_blocks < 1) {
    set_error("mimo_evidential_step: invalid argument");
    return MIMO_ERR_INVALID;
  }
  const int64_t total = (int64_t)n * hw;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (hw & 3) == 0 && (((uintptr_t)logits | (uintptr_t)label | (uintptr_t)mask | (uintptr_t)aleatoric_std |
                                      (uintptr_t)epistemic_std | (uintptr_t)err) & 15) == 0;  // (NULL counts as aligned)
  const int64_t units = vec ? total >> 2 : total;
  // grid-stride, 8 workgroups of 256 threads per CU at most (256 CUs), as mimo_evidential_uncertainties
  const int blocks = (int)std::min<int64_t>(std::min<int64_t>(ceil_div64(units, 256), 2048), scratch_blocks);
  if (vec)
    hipLaunchKernelGGL(evidential_step_kernel<true>, dim3(blocks), dim3(256), 0, st, logits, label, mask, total, hw, aleatoric_std,
                       epistemic_std, err, scratch);
  else
    hipLaunchKernelGGL(evidential_step_kernel<false>, dim3(blocks), dim3(256), 0, st, logits, label, mask, total, hw, aleatoric_std,
                       epistemic_std, err, scratch);
  MIMO_KERNEL_CHECK();
  hipLaunchKernelGGL(evidential_step_finalize_kernel, dim3(1), dim3(256), 0, st, scratch, blocks, (double)total, scalars);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_evidential_loss_gradient_dev(const float* logits, const float* label, const float* mask, int32_t n, int64_t hw,
                                                 float scale, const float* upstream, float* dlogits, mimo_stream stream) {
  if (!logits || !label || !upstream || !dlogits || n < 0 || hw < 0) {
    set_error("mimo_evidential_loss_gradient_dev: invalid argument");
    return MIMO_ERR_INVALID;
  }
  const int64_t total = (int64_t)n * hw;
  if (total == 0) return MIMO_OK;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);  // mimo_evidential_loss_gradient's grid
  hipLaunchKernelGGL(evidential_loss_gradient_dev_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, label, mask,
                     total, hw, scale, upstream, dlogits);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}
