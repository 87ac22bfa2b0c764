// The flat-buffer Adam update, written once: adam_kernel (optim.hip) and adam_clipped_kernel (optim_clip/grad_clip.hip)
// differ only in how a raw gradient element becomes the effective gradient, so that with a clipping coefficient of 1
// both give the same bits by construction.
//
// Replaces: torch.optim.Adam.step as configured by mimo/models/mimo_unet.py:186-190
//           (betas .9/.999, eps 1e-8, L2 weight decay folded into the gradient, not AdamW).
//
// Only the per-element update and the bias corrections are shared; the grid-stride loops stay in the two kernels.  hipcc
// optimises a device function on its own before it inlines it, and a helper that reads blockDim / gridDim, or that takes
// the element by reference with the loads and stores around the call, changes adam_kernel's machine code
// (scripts/kernel_isa_diff.py); this pointer form does not.
#pragma once
#include <hip/hip_runtime.h>

namespace mimo {

// 1 - beta^t, the bias correction of optimiser step t (counted on the device: amp_step_kernel / clip_finalize_kernel)
__device__ __forceinline__ float adam_bias_correction(float t, float beta) {
  // as -expm1(t log1p(beta - 1)) (beta - 1 is exact): 1 - powf(beta, t) keeps the rounding of a number near 1 in a result
  // of about t (1 - beta) — 6.7e-6 of the second-moment correction at t = 2, 1.7e-8 in this form
  return -expm1f(t * log1pf(beta - 1.f));
}

// one element, in registers (the 16-byte body) or in memory (the scalar tail); gr = the effective gradient before weight decay
__device__ __forceinline__ void adam_element(float* p, float gr, float* m, float* v, float lr, float beta1, float beta2,
                                             float eps, float wd, float bc1, float bc2_sqrt) {
  if (wd != 0.f) gr = fmaf(wd, *p, gr);
  const float mi = beta1 * *m + (1.f - beta1) * gr;
  const float vi = beta2 * *v + (1.f - beta2) * gr * gr;
  *m = mi;
  *v = vi;
  *p -= (lr / bc1) * (mi / (sqrtf(vi) / bc2_sqrt + eps));
}

}  // namespace mimo
