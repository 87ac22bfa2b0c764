// Device arithmetic of the evidential (Normal-Inverse-Gamma) head and its loss, shared by the training kernels
// (optim.hip: evidential_fwd_kernel / evidential_bwd_kernel) and the evaluation kernels (evidential_eval.hip): one
// definition of the softplus heads, the loss terms and the loss gradient, so that the two paths cannot drift apart.
//
//   (mu, v, alpha, beta) = (l0, softplus(l1), softplus(l2) + 1, softplus(l3))        mimo/models/evidential_unet.py:90-96
//   loss = G(alpha) / (v sqrt(beta)) * (2 beta (1 + v) + (2 alpha - 1) v (y - mu)^2) + (y - mu)^2 (2 alpha + v),
//   G(alpha) = Gamma(alpha - 1/2) / (4 Gamma(alpha))                                  mimo/losses.py:202-247
// G is evaluated as exp(lgamma(alpha - 1/2) - lgamma(alpha)) / 4 — the reference exponentiates the two lgammas
// separately, which overflows fp32 (inf / inf = nan) for alpha > 35; this form stays finite there.
#pragma once
#include <hip/hip_runtime.h>

namespace mimo {

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }  // torch: threshold 20
__device__ __forceinline__ float sigmoid_f(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float digamma_f(float x) {  // x > 0.5 here (alpha > 1)
  float r = 0.f;
  while (x < 6.f) {
    r -= 1.f / x;
    x += 1.f;
  }
  const float i = 1.f / x, i2 = i * i;
  return r + logf(x) - 0.5f * i - i2 * (1.f / 12.f - i2 * (1.f / 120.f - i2 * (1.f / 252.f)));
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
  float mu, v, alpha, beta, c, T, d;  // c = G / (v sqrt(beta)), T = the bracket, d = y - mu
};
__device__ __forceinline__ NigPoint nig_point(float l0, float l1, float l2, float l3, float y) {
  NigPoint q;
  const NigHead h = nig_head(l1, l2, l3);
  q.mu = l0;
  q.v = h.v;
  q.alpha = h.alpha;
  q.beta = h.beta;
  q.d = y - q.mu;
  const float G = 0.25f * expf(lgammaf(q.alpha - 0.5f) - lgammaf(q.alpha));
  q.c = G / (q.v * sqrtf(q.beta));
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
    g_v = up * (-q.c * q.T / q.v + q.c * (2.f * q.beta + two_a1 * sq) + sq);
    g_a = up * (q.c * (digamma_f(q.alpha - 0.5f) - digamma_f(q.alpha)) * q.T + q.c * 2.f * q.v * sq + 2.f * sq);
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
