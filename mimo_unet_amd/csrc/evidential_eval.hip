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
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "evidential.h"

namespace mimo {
namespace {

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

}  // namespace
}  // namespace mimo

using namespace mimo;

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
