// Proper scoring rules of the evidential model's predictive on the device (gfx950): per pixel the four logits of the
// Normal-Inverse-Gamma head and the label go in; the probability integral transform, the negative log-likelihood and the CRPS
// of the Student-t posterior predictive come out (student_t.h: the definition, the branch rule of the incomplete beta
// function and its iteration cap).  The heads are csrc/evidential.h's nig_head: (mu, v, alpha, beta) = (l0, softplus(l1),
// softplus(l2) + 1, softplus(l3)) in fp32; everything after them is double, rounded once into the fp32 maps.
//
//   mimo_score_accumulate_evidential   one pass per batch: 20 (+ 4 with a mask) bytes in per pixel, each read once, up to
//                                      12 out; the same workspace, partial rows, fold and finalize as mimo_score_accumulate
//
// A pixel is skipped when mask == 0 (n_masked), or when its label or any of its four logits is not finite, or when v == 0 or
// beta == 0 (the fp32 softplus has underflowed, l < -103: the scale would be infinite or zero) (n_nonfinite): NaN in every
// requested map, no sum, no bin.  alpha == 1 exactly is scored: every formula is finite at nu = 2.  Means and labels are
// not clipped.  The PIT bin and the sums come from the fp32 values the maps get.
//
// The kernel is bound by its double arithmetic, not by its 20 - 36 bytes per pixel: per pixel one log1p, one exponential, two
// logarithms, two short exponentials of the gamma-ratio series, some square roots, and six divisions per iteration of the
// continued fraction (about 12 iterations on average, a wave runs as long as its slowest lane).
#include "../evidential.h"
#include "score_common.h"
#include "student_t.h"

#include <algorithm>

namespace mimo {
namespace score {

struct EvidentialArgs {
  const float *logits, *label, *mask, *pk;
  float *pit, *nll, *crps;
  int B, K;
  int64_t hw;
  u64* part;
};

// VEC: hw % 4 == 0 and every pointer 16-byte aligned -> a float4 of pixels per thread per step (5 (+ 1) 16-byte loads),
// scored one after another; otherwise one pixel per thread with scalar loads.  Each workgroup strides over the batch.
template <bool VEC>
__global__ __launch_bounds__(256) void score_evidential_kernel(EvidentialArgs a) {
  __shared__ float zt[kMaxK + 1];
  __shared__ u32 bins[4 * (kBins + 3)];
  __shared__ double red[3 * 256];
  __shared__ u32 redn[3 * 256];
  __shared__ u32 most;
  constexpr int PPT = VEC ? 4 : 1;
  const int tid = threadIdx.x, wave = tid >> 6;
  if (tid == 0) most = 0u;
  block_prologue(a, zt, bins);
  const int64_t ipi = a.hw / PPT, items = (int64_t)a.B * ipi;  // VEC: hw % 4 == 0
  const float nanv = __uint_as_float(0x7FC00000u);
  Tally t;
  int worst = 0;
  for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < items; q += (int64_t)gridDim.x * 256) {
    const int64_t b = q / ipi, p0 = (q - b * ipi) * PPT;
    const int64_t src = b * 4 * a.hw + p0, dst = b * a.hw + p0;
    float4 l4[4], y4, k4 = make_float4(1.f, 1.f, 1.f, 1.f);
    if (VEC) {
#pragma unroll
      for (int c = 0; c < 4; ++c) l4[c] = *(const float4*)(a.logits + src + c * a.hw);
      y4 = *(const float4*)(a.label + dst);
      if (a.mask) k4 = *(const float4*)(a.mask + dst);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) l4[c].x = a.logits[src + c * a.hw];
      y4.x = a.label[dst];
      if (a.mask) k4.x = a.mask[dst];
    }
    float4 o_pit = make_float4(nanv, nanv, nanv, nanv), o_nll = o_pit, o_crps = o_pit;
#pragma unroll 1
    for (int k = 0; k < PPT; ++k) {
      if (a.mask && pick(k4, k) == 0.f) {
        ++t.nm;
        continue;
      }
      const float y = pick(y4, k), mu = pick(l4[0], k), l1 = pick(l4[1], k), l2 = pick(l4[2], k), l3 = pick(l4[3], k);
      const NigHead h = nig_head(l1, l2, l3);
      // (a NaN or -inf logit gives a NaN or zero head, +inf an infinite one: the logits themselves are tested)
      if (!(isfinite(y) && isfinite(mu) && isfinite(l1) && isfinite(l2) && isfinite(l3) && h.v > 0.f && h.beta > 0.f)) {
        ++t.nf;
        continue;
      }
      float pit, nll, crps;
      int it;
      student_t_scores(mu, h.v, h.alpha, h.beta, y, pit, nll, crps, it);
      worst = it > worst ? it : worst;
      tally_pixel(pit, nll, crps, zt, a.K, bins + wave * (kBins + 3), t);
      put(o_pit, k, pit);
      put(o_nll, k, nll);
      put(o_crps, k, crps);
    }
    if (VEC) {
      if (a.pit) *(float4*)(a.pit + dst) = o_pit;
      if (a.nll) *(float4*)(a.nll + dst) = o_nll;
      if (a.crps) *(float4*)(a.crps + dst) = o_crps;
    } else {
      if (a.pit) a.pit[dst] = o_pit.x;
      if (a.nll) a.nll[dst] = o_nll.x;
      if (a.crps) a.crps[dst] = o_crps.x;
    }
  }
  atomicMax(&most, (u32)worst);
  block_epilogue(a, t, bins, red, redn);  // (its barriers order the atomics before the read below)
  if (tid == kIterWord) a.part[(size_t)blockIdx.x * kAccWords + kIterWord] = most;
}

}  // namespace score
}  // namespace mimo

extern "C" int mimo_score_accumulate_evidential(const float* logits, const float* label, const float* mask, int32_t batch,
                                                int64_t hw, const float* expected_p, int32_t num_thresholds, float* pit_map,
                                                float* nll_map, float* crps_map, void* workspace, mimo_stream stream) {
  using namespace mimo;
  using namespace mimo::score;
  const uintptr_t all = (uintptr_t)logits | (uintptr_t)label | (uintptr_t)mask | (uintptr_t)pit_map | (uintptr_t)nll_map |
                        (uintptr_t)crps_map;
  if (!logits || !label || !expected_p || !workspace || batch < 1 || hw < 1 || num_thresholds < 1 || num_thresholds > kMaxK ||
      (all & 3) || ((uintptr_t)expected_p & 3) || ((uintptr_t)workspace & 15)) {
    set_error("mimo_score_accumulate_evidential: invalid argument (1 <= num_thresholds <= %d)", kMaxK);
    return MIMO_ERR_INVALID;
  }
  Workspace* ws = (Workspace*)workspace;
  const bool vec = (hw % 4 == 0) && (all & 15) == 0;
  EvidentialArgs a{logits, label, mask, expected_p, pit_map, nll_map, crps_map, batch, num_thresholds, hw, &ws->part[0][0]};
  const int blocks = (int)std::min<int64_t>(ceil_div64((int64_t)batch * (vec ? hw / 4 : hw), 256), kBlocks);
  hipLaunchKernelGGL(vec ? score_evidential_kernel<true> : score_evidential_kernel<false>, dim3(blocks), dim3(256), 0,
                     (hipStream_t)stream, a);
  MIMO_KERNEL_CHECK();
  return fold_partials(ws, blocks, kFolded + 1, (hipStream_t)stream);
}
