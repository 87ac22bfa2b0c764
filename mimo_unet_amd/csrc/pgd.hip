// Iterated, projected sign-gradient attack (PGD; BIM without the random start) on a batch of images, gfx950.
//
// No reference counterpart: the reference's only attack is the single step of fgsm_attack (scripts/test/test_nyuv2_depth.py:16-24,
// csrc/fgsm.hip).  The torch form of one step, per perturbation size,
//   x_adv = clamp(max(min(x_adv + alpha * grad.sign(), x0 + eps), x0 - eps), lo, hi)
// is six full-image launches; here ONE launch serves all K sizes of a robustness sweep.  Unlike FGSM the gradient is taken at
// the current iterate and so differs per size: grad and x_adv are [K, elems], the clean image x0 is read once.
//
// pgd_step_kernel — per element 4 + 8 K B read, 4 K B written; x_adv is updated in place through one pointer.
//   s = sign(grad[k][i])                           fgsm.hip's rule: +-0 -> 0, NaN -> NaN
//   v = x_adv[k][i] + alpha[k] * s                 the product is exact, so a fused multiply-add rounds like the separate add
//   v = clamp(v, x0[i] - eps[k], x0[i] + eps[k])   the eps-ball first; each bound is one fp32 rounding
//   x_adv[k][i] = clamp(v, lo, hi)                 then the value range
// Both clamps are the compare form of fgsm_one: a NaN passes.  eps[k] = 0 gives clamp(x0, lo, hi) whatever the gradient is,
// unless it is NaN.
//
// pgd_init_kernel — the random start of all K sizes from ONE draw: 4 B read, 4 K B written per element.
//   quad q = elements 4 q .. 4 q + 3 takes the four words of
//     philox4x32_10(ctr = (lo32(q), hi32(q), lo32(offset) ^ 0xFF000000, hi32(offset)), key = (lo32(seed), hi32(seed)))
//   element 4 q + j word j.  Counter word 2 is the dropout draws' layout (ew_dropout.hip: lo32(offset) ^ (site << 24), site < 56)
//   with the site number 255 no dropout site can have, and the permutation draw (perm_draw.hip) leaves word 2 = lo32(offset):
//   for the same (seed, offset) block the three never share a counter.
//   r = (2 (w >> 8) + 1 - 2^24) * 2^-24            an odd integer below 2^24 times a power of two: exact, symmetric in (-1, 1)
//   x_adv[k][i] = clamp(fadd(x0[i], fmul(eps[k], r)), lo, hi)      two roundings, never contracted; the same r for every k
// The scalar path walks quads too (one Philox call per quad, its tail quad partly used), so both paths give an element the
// same value.
//
// Both: grid-stride, 256 threads, at most 2048 blocks, float4 when elems % 4 == 0 and every pointer is 16-byte aligned, eps and
// alpha by value in slices of 16, no atomics, no reduction.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "philox.h"

namespace mimo {
namespace {

constexpr int kPgdMaxEps = 16;  // perturbation sizes per launch (kernel arguments); longer lists run in slices
struct PgdSizes {
  float eps[kPgdMaxEps];
  float alpha[kPgdMaxEps];
};

__device__ __forceinline__ float pgd_sign(float g) { return g > 0.f ? 1.f : (g < 0.f ? -1.f : (g == 0.f ? 0.f : g)); }  // +-0 -> 0, NaN -> NaN
__device__ __forceinline__ float pgd_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }  // NaN passes
__device__ __forceinline__ float pgd_one(float x0, float xa, float g, float eps, float alpha, float lo, float hi) {
  const float v = xa + alpha * pgd_sign(g);
  return pgd_clamp(pgd_clamp(v, x0 - eps, x0 + eps), lo, hi);
}

// VEC: elems is a multiple of 4 and every pointer is 16-byte aligned.  x_adv: read and written, so not __restrict__
template <bool VEC>
__global__ __launch_bounds__(256) void pgd_step_kernel(const float* __restrict__ x0, const float* __restrict__ grad, float* x_adv,
                                                      int64_t elems, PgdSizes sz, int K, float lo, float hi) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (VEC) {
    const int64_t quads = elems >> 2;
    for (int64_t q = first; q < quads; q += stride) {
      const float4 x = reinterpret_cast<const float4*>(x0)[q];
      for (int k = 0; k < K; ++k) {
        const float e = sz.eps[k], a = sz.alpha[k];
        const float4 g = reinterpret_cast<const float4*>(grad + (int64_t)k * elems)[q];
        float4* dst = reinterpret_cast<float4*>(x_adv + (int64_t)k * elems) + q;
        const float4 v = *dst;
        *dst = make_float4(pgd_one(x.x, v.x, g.x, e, a, lo, hi), pgd_one(x.y, v.y, g.y, e, a, lo, hi),
                           pgd_one(x.z, v.z, g.z, e, a, lo, hi), pgd_one(x.w, v.w, g.w, e, a, lo, hi));
      }
    }
  } else {
    for (int64_t i = first; i < elems; i += stride) {
      const float x = x0[i];
      for (int k = 0; k < K; ++k) {
        const int64_t at = (int64_t)k * elems + i;
        x_adv[at] = pgd_one(x, x_adv[at], grad[at], sz.eps[k], sz.alpha[k], lo, hi);
      }
    }
  }
}

__device__ __forceinline__ float pgd_unit(unsigned int w) {  // (2 u24 + 1 - 2^24) * 2^-24, exact
  return (float)((int)((w >> 8) << 1) + 1 - (1 << 24)) * 0x1p-24f;
}
__device__ __forceinline__ float pgd_start(float x, float eps, float r, float lo, float hi) {
  // fmul_rn then fadd_rn.  HIP's __fmul_rn / __fadd_rn are inline functions around the plain operators, which hipcc contracts
  // into one v_fma_f32 after inlining them: so the operators themselves, with contraction switched off for this block
#pragma clang fp contract(off)
  const float step = eps * r;
  return pgd_clamp(x + step, lo, hi);
}
__device__ __forceinline__ uint4 pgd_words(int64_t q, uint64_t seed, uint64_t offset) {
  return philox4x32_10(make_uint4((unsigned int)q, (unsigned int)((uint64_t)q >> 32), (unsigned int)offset ^ 0xFF000000u,
                                  (unsigned int)(offset >> 32)),
                       make_uint2((unsigned int)seed, (unsigned int)(seed >> 32)));
}

template <bool VEC>
__global__ __launch_bounds__(256) void pgd_init_kernel(const float* __restrict__ x0, int64_t elems, PgdSizes sz, int K, float lo,
                                                      float hi, uint64_t seed, uint64_t offset, float* __restrict__ x_adv) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t quads = (elems + 3) >> 2;
  for (int64_t q = first; q < quads; q += stride) {
    const uint4 w = pgd_words(q, seed, offset);
    const float r[4] = {pgd_unit(w.x), pgd_unit(w.y), pgd_unit(w.z), pgd_unit(w.w)};
    if constexpr (VEC) {
      const float4 x = reinterpret_cast<const float4*>(x0)[q];
      for (int k = 0; k < K; ++k) {
        const float e = sz.eps[k];
        reinterpret_cast<float4*>(x_adv + (int64_t)k * elems)[q] =
            make_float4(pgd_start(x.x, e, r[0], lo, hi), pgd_start(x.y, e, r[1], lo, hi), pgd_start(x.z, e, r[2], lo, hi),
                        pgd_start(x.w, e, r[3], lo, hi));
      }
    } else {
      const int n = (int)std::min<int64_t>(4, elems - 4 * q);  // the tail quad uses its first n words
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          const float x = x0[4 * q + j];
          for (int k = 0; k < K; ++k) x_adv[(int64_t)k * elems + 4 * q + j] = pgd_start(x, sz.eps[k], r[j], lo, hi);
        }
      }
    }
  }
}

bool pgd_sizes_ok(const float* v, int K) {
  for (int k = 0; k < K; ++k)
    if (!(v[k] >= 0.f)) return false;  // negative or NaN
  return true;
}

int pgd_blocks(int64_t units) { return (int)std::min<int64_t>(ceil_div64(units, 256), 2048); }  // as fgsm.hip

}  // namespace
}  // namespace mimo

using namespace mimo;

extern "C" int mimo_pgd_step(const float* x0, const float* grad, float* x_adv, int64_t elems, const float* eps, const float* alpha,
                             int K, float lo, float hi, mimo_stream stream) {
  if (!x0 || !grad || !x_adv || !eps || !alpha || elems < 1 || K < 1) {
    set_error("mimo_pgd_step: bad argument");
    return MIMO_ERR_INVALID;
  }
  if (!(lo <= hi)) {
    set_error("mimo_pgd_step: empty clip range [%g, %g]", lo, hi);
    return MIMO_ERR_INVALID;
  }
  if (!pgd_sizes_ok(eps, K) || !pgd_sizes_ok(alpha, K)) {
    set_error("mimo_pgd_step: negative or NaN eps / alpha");
    return MIMO_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (elems & 3) == 0 &&
                   (((uintptr_t)x0 | (uintptr_t)grad | (uintptr_t)x_adv) & 15) == 0;  // (then every row k * elems is aligned too)
  const int blocks = pgd_blocks(vec ? elems >> 2 : elems);
  for (int k0 = 0; k0 < K; k0 += kPgdMaxEps) {
    PgdSizes sz = {};
    const int kn = std::min(K - k0, kPgdMaxEps);
    for (int k = 0; k < kn; ++k) {
      sz.eps[k] = eps[k0 + k];
      sz.alpha[k] = alpha[k0 + k];
    }
    const float* g = grad + (int64_t)k0 * elems;
    float* xa = x_adv + (int64_t)k0 * elems;
    if (vec)
      hipLaunchKernelGGL(pgd_step_kernel<true>, dim3(blocks), dim3(256), 0, st, x0, g, xa, elems, sz, kn, lo, hi);
    else
      hipLaunchKernelGGL(pgd_step_kernel<false>, dim3(blocks), dim3(256), 0, st, x0, g, xa, elems, sz, kn, lo, hi);
    MIMO_KERNEL_CHECK();
  }
  return MIMO_OK;
}

extern "C" int mimo_pgd_init(const float* x0, int64_t elems, const float* eps, int K, float lo, float hi, uint64_t seed,
                             uint64_t offset, float* x_adv, mimo_stream stream) {
  if (!x0 || !eps || !x_adv || elems < 1 || K < 1) {
    set_error("mimo_pgd_init: bad argument");
    return MIMO_ERR_INVALID;
  }
  if (!(lo <= hi)) {
    set_error("mimo_pgd_init: empty clip range [%g, %g]", lo, hi);
    return MIMO_ERR_INVALID;
  }
  if (!pgd_sizes_ok(eps, K)) {
    set_error("mimo_pgd_init: negative or NaN eps");
    return MIMO_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (elems & 3) == 0 && (((uintptr_t)x0 | (uintptr_t)x_adv) & 15) == 0;
  const int blocks = pgd_blocks((elems + 3) >> 2);  // one quad per thread and step on both paths
  for (int k0 = 0; k0 < K; k0 += kPgdMaxEps) {
    PgdSizes sz = {};
    const int kn = std::min(K - k0, kPgdMaxEps);
    for (int k = 0; k < kn; ++k) sz.eps[k] = eps[k0 + k];
    float* xa = x_adv + (int64_t)k0 * elems;
    if (vec)
      hipLaunchKernelGGL(pgd_init_kernel<true>, dim3(blocks), dim3(256), 0, st, x0, elems, sz, kn, lo, hi, seed, offset, xa);
    else
      hipLaunchKernelGGL(pgd_init_kernel<false>, dim3(blocks), dim3(256), 0, st, x0, elems, sz, kn, lo, hi, seed, offset, xa);
    MIMO_KERNEL_CHECK();
  }
  return MIMO_OK;
}
