// Fast-gradient-sign attack on a batch of images, gfx950.
//
// Replaces (reference, relative to /root/reference): fgsm_attack of scripts/test/test_nyuv2_depth.py:16-24 —
//   torch.clamp(image + epsilon * data_grad.sign(), 0, 1)
// — for ALL perturbation sizes of a robustness sweep in one pass.  In eval mode the gradient is taken at the clean image and
// does not depend on epsilon, so image and gradient are read once (8 B per element) and the K perturbed images are written
// (4 K B per element): one float4 of each per thread and step, K float4 stores, no atomics, no reduction.
//
// Arithmetic, element for element torch's for every non-NaN gradient: sign(g) is -1 / 0 / +1; eps * sign(g) is exact, so the
// fused multiply-add the compiler may form rounds like torch's separate add; the clamp passes a NaN image pixel through
// (torch.clamp does), which fminf / fmaxf would not.  eps = 0 still clamps.  One deliberate difference: a NaN gradient gives
// a NaN pixel here, where torch.sign returns 0 and the reference would leave the pixel unattacked without a trace.
#include <algorithm>
#include <cstdint>

#include "common.h"

namespace mimo {
namespace {

constexpr int kFgsmMaxEps = 16;  // perturbation sizes per launch (kernel arguments); longer lists run in slices
struct FgsmEps {
  float v[kFgsmMaxEps];
};

__device__ __forceinline__ float fgsm_sign(float g) { return g > 0.f ? 1.f : (g < 0.f ? -1.f : (g == 0.f ? 0.f : g)); }  // +-0 -> 0, NaN -> NaN
__device__ __forceinline__ float fgsm_one(float x, float sg, float eps, float lo, float hi) {
  const float v = x + eps * sg;
  return v < lo ? lo : (v > hi ? hi : v);  // NaN compares false twice and passes
}

// VEC: elems is a multiple of 4 and every pointer is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void fgsm_perturb_kernel(const float* __restrict__ image, const float* __restrict__ grad,
                                                          int64_t elems, FgsmEps eps, int K, float lo, float hi,
                                                          float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (VEC) {
    const int64_t quads = elems >> 2;
    for (int64_t q = first; q < quads; q += stride) {
      const float4 x = reinterpret_cast<const float4*>(image)[q];
      const float4 g = reinterpret_cast<const float4*>(grad)[q];
      const float4 s = make_float4(fgsm_sign(g.x), fgsm_sign(g.y), fgsm_sign(g.z), fgsm_sign(g.w));
      for (int k = 0; k < K; ++k) {
        const float e = eps.v[k];
        reinterpret_cast<float4*>(out + (int64_t)k * elems)[q] =
            make_float4(fgsm_one(x.x, s.x, e, lo, hi), fgsm_one(x.y, s.y, e, lo, hi), fgsm_one(x.z, s.z, e, lo, hi),
                        fgsm_one(x.w, s.w, e, lo, hi));
      }
    }
  } else {
    for (int64_t i = first; i < elems; i += stride) {
      const float x = image[i], s = fgsm_sign(grad[i]);
      for (int k = 0; k < K; ++k) out[(int64_t)k * elems + i] = fgsm_one(x, s, eps.v[k], lo, hi);
    }
  }
}

}  // namespace
}  // namespace mimo

using namespace mimo;

extern "C" int mimo_fgsm_perturb(const float* image, const float* dimage, int64_t elems, const float* eps, int K, float lo,
                                 float hi, float* out, mimo_stream stream) {
  if (!image || !dimage || !eps || !out || elems < 1 || K < 1) {
    set_error("mimo_fgsm_perturb: bad argument");
    return MIMO_ERR_INVALID;
  }
  if (!(lo <= hi)) {
    set_error("mimo_fgsm_perturb: empty clip range [%g, %g]", lo, hi);
    return MIMO_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (elems & 3) == 0 &&
                   (((uintptr_t)image | (uintptr_t)dimage | (uintptr_t)out) & 15) == 0;  // (then every out + k * elems is aligned too)
  const int64_t units = vec ? elems >> 2 : elems;
  // grid-stride, 8 workgroups of 256 threads per CU at most (256 CUs): enough loads in flight to stream, few enough blocks to launch fast
  const int blocks = (int)std::min<int64_t>(ceil_div64(units, 256), 2048);
  for (int k0 = 0; k0 < K; k0 += kFgsmMaxEps) {
    FgsmEps e = {};
    const int kn = std::min(K - k0, kFgsmMaxEps);
    for (int k = 0; k < kn; ++k) e.v[k] = eps[k0 + k];
    float* dst = out + (int64_t)k0 * elems;
    if (vec)
      hipLaunchKernelGGL(fgsm_perturb_kernel<true>, dim3(blocks), dim3(256), 0, st, image, dimage, elems, e, kn, lo, hi, dst);
    else
      hipLaunchKernelGGL(fgsm_perturb_kernel<false>, dim3(blocks), dim3(256), 0, st, image, dimage, elems, e, kn, lo, hi, dst);
    MIMO_KERNEL_CHECK();
  }
  return MIMO_OK;
}
