// Device arithmetic of the evidential (Normal-Inverse-Gamma) head and its loss, shared by the training kernels
// (optim.hip: evidential_fwd_kernel / evidential_bwd_kernel) and the evaluation kernels (evidential_eval.hip): one
// definition of the softplus heads, the loss terms and the loss gradient, so that the two paths cannot drift apart.
//
//   (mu, v, alpha, beta) = (l0, softplus(l1), softplus(l2) + 1, softplus(l3))        mimo/models/evidential_unet.py:90-96
//   loss = G(alpha) / (v sqrt(beta)) * (2 beta (1 + v) + (2 alpha - 1) v (y - mu)^2) + (y - mu)^2 (2 alpha + v),
//   G(alpha) = Gamma(alpha - 1/2) / (4 Gamma(alpha))                                  mimo/losses.py:202-247
// The reference exponentiates the two lgammas separately, which overflows fp32 (inf / inf = nan) for alpha > 35; G and
// dG/dalpha come from nig_gamma() below, which stays finite and accurate to a few fp32 roundings for every alpha > 1.
#pragma once
#include <hip/hip_runtime.h>

namespace mimo {

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }  // torch: threshold 20
__device__ __forceinline__ float sigmoid_f(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }
// G(a) = Gamma(a - 1/2) / (4 Gamma(a)) and D(a) = psi(a - 1/2) - psi(a)  (dG/da = G D), a = alpha >= 1.
// Both are differences of nearly equal numbers when formed from lgammaf / a digamma of each argument: lgamma(a) grows like
// a ln a, psi(a) like ln a, while the differences shrink like -ln(a) / 2 and -1 / (2 a).  In fp32 the direct forms measure
// (against fp64) 4e-7 / 6e-7 relative at a = 10, 3e-6 / 7e-5 at 200, 4e-4 / 3e-4 at 1000 and 4e-3 / 1e-2 at 10000.
// Here nothing cancels:
//   a < 8: the recurrences Gamma(x + 1) = x Gamma(x), psi(x + 1) = psi(x) + 1 / x applied to both arguments at once,
//       G(a) = G(a + 1) a / (a - 1/2),   D(a) = D(a + 1) - 1 / (2 (a - 1/2) a)
//     (a - 1/2 is exact in fp32 for a >= 1; every factor is > 1 and every term < 0), at most 7 steps;
//   a >= 8: the asymptotic series of the differences themselves (Stirling's series of lgamma at a - 1/2 and at a, subtracted
//     term by term and expanded in 1 / a):
//       lgamma(a - 1/2) - lgamma(a) = -ln(a) / 2 + P(1 / a),  P(i) = 3/8 i + 1/8 i^2 + 3/64 i^3 + 1/64 i^4 + 3/640 i^5 + 1/384 i^6
//       D(a) = d/da of that = -i (1/2 + 3/8 i + 1/4 i^2 + 9/64 i^3 + 1/16 i^4 + 3/128 i^5 + 1/64 i^6)
//     so G = exp(P) / (4 sqrt(a)): P <= 0.05, the exponential adds one rounding instead of |lgamma| of them.
// Threshold and length, against 40-digit arithmetic (mpmath loggamma / digamma) on a log grid of a in [8, 8e5]: six terms cut
// off at a >= 8 leave |P - exact| <= 1.1e-9 and a relative error of D <= 1.4e-8, both under 2^-24 = 6.0e-8 (five terms:
// 1.1e-8 and 1.2e-7 — too short for D; threshold 6 with six terms: 8.4e-9 and 1.0e-7).
struct NigGamma {
  float G, D;
};
__device__ __forceinline__ NigGamma nig_gamma(float a) {
  float ratio = 1.f, d = 0.f;
  while (a < 8.f) {
    const float lo = a - 0.5f;
    ratio *= a / lo;
    d -= 0.5f / (lo * a);
    a += 1.f;
  }
  const float i = 1.f / a;
  const float P = i * (0.375f + i * (0.125f + i * (3.f / 64.f + i * (1.f / 64.f + i * (3.f / 640.f + i * (1.f / 384.f))))));
  const float D = -i * (0.5f + i * (0.375f + i * (0.25f + i * (9.f / 64.f + i * (1.f / 16.f + i * (3.f / 128.f + i * (1.f / 64.f)))))));
  return NigGamma{0.25f * ratio * expf(P) / sqrtf(a), d + D};
}

// the three softplus heads (alpha is rounded as softplus(l2) + 1: alpha - 1 taken afterwards is the reference's alpha - 1)
struct NigHead {
  float v, alpha, beta;
};
__device__ __forceinline__ NigHead nig_head(float l1, float l2, float l3) {
  NigHead h;
  h.v = softplus_f(l1);
  h.alpha = softplus_f(l2) + 1.f;
  h.beta = softplus_f(l3);
  return h;
}

struct NigPoint {
  float mu, v, alpha, beta, c, T, d, D;  // c = G / (v sqrt(beta)), T = the bracket, d = y - mu, D = psi(alpha - 1/2) - psi(alpha)
};
__device__ __forceinline__ NigPoint nig_point(float l0, float l1, float l2, float l3, float y) {
  NigPoint q;
  const NigHead h = nig_head(l1, l2, l3);
  q.mu = l0;
  q.v = h.v;
  q.alpha = h.alpha;
  q.beta = h.beta;
  q.d = y - q.mu;
  const NigGamma g = nig_gamma(q.alpha);
  q.D = g.D;
  q.c = g.G / (q.v * sqrtf(q.beta));
  q.T = 2.f * q.beta * (1.f + q.v) + (2.f * q.alpha - 1.f) * q.v * q.d * q.d;
  return q;
}

// The upstream gradient of the per-pixel loss: a [N,HW] tensor (NULL = none; evidential_bwd_kernel) or one value for every
// pixel (evidential_loss_gradient_kernel: the mean / sum of the loss map, no tensor and no launch that fills one)
struct NigUpTensor {
  const float* __restrict__ p;
  __device__ __forceinline__ bool on() const { return p != nullptr; }
  __device__ __forceinline__ float at(int64_t i) const { return p[i]; }
};
struct NigUpConst {
  float s;
  __device__ __forceinline__ bool on() const { return true; }
  __device__ __forceinline__ float at(int64_t) const { return s; }
};

// One pixel of the backward: dlogits = d_loss * mask * dloss/dlogits (+ d_ev * dev/dlogits), both upstream gradients optional
// (analytic: dG/dalpha = G (psi(alpha - 1/2) - psi(alpha))).  The ONE definition both backward kernels run.
template <typename Up>
__device__ __forceinline__ void nig_bwd_pixel(const float* __restrict__ logits, const float* __restrict__ label,
                                              const float* __restrict__ mask, const float* __restrict__ d_ev, const Up d_loss,
                                              int64_t i, int64_t hw, float* __restrict__ dlogits) {
  const int64_t n = i / hw, r = i - n * hw;
  const float* l = logits + n * 4 * hw + r;
  const float l1 = l[hw], l2 = l[2 * hw], l3 = l[3 * hw];
  float g_mu = 0.f, g_v = 0.f, g_a = 0.f, g_b = 0.f;
  if (d_loss.on() && label) {
    const NigPoint q = nig_point(l[0], l1, l2, l3, label[i]);
    const float up = d_loss.at(i) * (mask ? mask[i] : 1.f);
    const float sq = q.d * q.d, two_a1 = 2.f * q.alpha - 1.f;
    g_mu = up * (-2.f * q.d) * (q.c * two_a1 * q.v + 2.f * q.alpha + q.v);
    // d(c T)/dv = -c T / v + c (2 beta + (2 alpha - 1) sq) = -2 c beta / v: the (2 alpha - 1) sq terms cancel exactly, and formed
    // separately they left an error of c (2 alpha - 1) sq ulp next to a result of 2 c beta / v (17 % at alpha = 3e3, d = 30)
    g_v = up * (sq - 2.f * q.c * q.beta / q.v);
    g_a = up * (q.c * q.D * q.T + q.c * 2.f * q.v * sq + 2.f * sq);
    g_b = up * (-q.c * q.T / (2.f * q.beta) + 2.f * q.c * (1.f + q.v));
  }
  if (d_ev) {
    const float* e = d_ev + n * 4 * hw + r;
    g_mu += e[0];
    g_v += e[hw];
    g_a += e[2 * hw];
    g_b += e[3 * hw];
  }
  float* o = dlogits + n * 4 * hw + r;
  o[0] = g_mu;
  o[hw] = g_v * sigmoid_f(l1);
  o[2 * hw] = g_a * sigmoid_f(l2);
  o[3 * hw] = g_b * sigmoid_f(l3);
}

}  // namespace mimo
