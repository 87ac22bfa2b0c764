// Gradient clipping fused into the flat Adam step (gfx950, HBM-bound): mimo_adam_step_clipped.
//
// Replaces: torch.nn.utils.clip_grad_norm_ / clip_grad_value_ over the parameter views followed by torch.optim.Adam.step
//           (what Lightning's Trainer(gradient_clip_val=...) runs around the optimiser of mimo/models/mimo_unet.py:186-190).
//
// Lives in a subdirectory because the benchmark never launches it (bench.csrc_hash covers csrc/*.hip, csrc/*.h).  The update
// kernel below and optim.hip's adam_kernel call one per-element update and one bias-correction helper (../adam_update.h):
// they differ only in how a raw gradient element becomes the effective gradient, so that with a coefficient of 1 both give
// the same bits.
//
// Effective gradient ge = g * s, s = grad_scale (/ *amp_scale when given): the factor adam_kernel applies.
//   norm mode : norm = sqrt(sum ge^2), coef = min(1, clip / (norm + 1e-6)), the update sees (g * s) * coef
//   value mode: the update sees clamp(g * s, -clip, clip) (a NaN stays a NaN); no reduction
// Launches (norm mode 3, value mode 2), all ordered on the stream, no atomics, no flags, no "last block":
//   1. grad_sumsq_kernel   <= 2048 workgroups, 16-byte loads, ge and ge^2 in fp32, sums in double: thread, wave (butterfly),
//                          workgroup (LDS tree); one double per workgroup into the scratch row
//   2. clip_finalize_kernel one workgroup folds the row in a fixed order, forms norm and coef in double, rounds each to fp32
//                          once, writes clip_out, decides skip / apply (found_inf, finiteness of the norm), advances step_dev
//                          (amp_step_kernel's job on this route) and leaves {coef, skip} behind the row
//   3. adam_clipped_kernel reads {coef, skip}; the shared update
#include "../adam_update.h"
#include "../common.h"

#include <algorithm>

namespace mimo {
namespace gradclip {

constexpr int kMaxBlocks = 2048;  // workgroups of the sum-of-squares pass == doubles of the partial row
constexpr int kUnroll = 4;        // 16-byte loads in flight per lane

// scratch: double partial[kMaxBlocks], then this record
struct Verdict {
  float coef;
  int32_t skip;
  int32_t pad[2];
};

__device__ __forceinline__ double block_sum(double acc, double* red) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) acc += __shfl_xor(acc, d);
  const int wave = threadIdx.x / kWave, waves = blockDim.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) red[wave] = acc;
  __syncthreads();
  for (int off = waves / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double sq4(const float4 gg, float s) {
  const float e0 = gg.x * s, e1 = gg.y * s, e2 = gg.z * s, e3 = gg.w * s;
  const float q0 = e0 * e0, q1 = e1 * e1, q2 = e2 * e2, q3 = e3 * e3;  // fp32 squares, summed in double
  return ((double)q0 + (double)q1) + ((double)q2 + (double)q3);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, float grad_scale,
                                                         const float* __restrict__ amp_scale, double* __restrict__ partial) {
  __shared__ double red[256 / kWave];
  if (amp_scale) grad_scale /= *amp_scale;
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  double acc = 0.0;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + (kUnroll - 1) * stride < n4; i += kUnroll * stride) {
    float4 gg[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) gg[u] = g4[i + u * stride];  // all issued before the first use
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) acc += sq4(gg[u], grad_scale);
  }
  for (; i < n4; i += stride) acc += sq4(g4[i], grad_scale);
  // tail (n not a multiple of 4)
  for (int64_t t = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    const float e = g[t] * grad_scale;
    const float q = e * e;
    acc += (double)q;
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// blocks == 0: value mode (norm 0, coefficient 1)
__global__ __launch_bounds__(256) void clip_finalize_kernel(const double* __restrict__ partial, int blocks, float clip,
                                                            const float* __restrict__ found_inf, float* __restrict__ step_dev,
                                                            float* __restrict__ clip_out, Verdict* __restrict__ verdict) {
  __shared__ double red[256 / kWave];
  double acc = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) acc += partial[b];
  const double tot = block_sum(acc, red);
  if (threadIdx.x != 0) return;
  float norm = 0.f, coef = 1.f;
  bool skip = found_inf && *found_inf != 0.f;
  if (blocks > 0) {
    const double nd = sqrt(tot);
    norm = (float)nd;
    if (nd - nd == 0.0) {  // finite
      coef = (float)fmin(1.0, (double)clip / (nd + 1e-6));
    } else {  // an inf / nan gradient: nothing is applied
      coef = 0.f;
      skip = true;
    }
  }
  clip_out[0] = norm;
  clip_out[1] = coef;
  verdict->coef = coef;
  verdict->skip = skip ? 1 : 0;
  if (!skip) *step_dev += 1.f;
}

template <int MODE>
__device__ __forceinline__ float clipped(float ge, float c) {
  if (MODE == MIMO_CLIP_NORM) return ge * c;
  return ge < -c ? -c : (ge > c ? c : ge);  // comparisons, not fminf / fmaxf: a NaN stays a NaN (torch.clamp)
}

// adam_kernel (optim.hip) with the clipped gradient; c = the coefficient (norm mode, read from the verdict) or the bound
// (value mode).  Everything after the effective gradient is adam_element (adam_update.h), which adam_kernel calls too.
template <int MODE>
__global__ void adam_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                    float* __restrict__ v, int64_t n, float lr, float beta1, float beta2, float eps, float wd,
                                    float grad_scale, const float* __restrict__ step_dev, const float* __restrict__ amp_scale,
                                    float clip, const Verdict* __restrict__ verdict) {
  if (verdict->skip != 0) return;  // found_inf, or a norm that is not finite: skip this step
  const float c = MODE == MIMO_CLIP_NORM ? verdict->coef : clip;
  const float t = *step_dev;
  const float bc1 = adam_bias_correction(t, beta1);
  const float bc2_sqrt = sqrtf(adam_bias_correction(t, beta2));
  if (amp_scale) grad_scale /= *amp_scale;
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* pa = &pp.x;
    float* ga = &gg.x;
    float* ma = &mm.x;
    float* va = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      adam_element(&pa[j], clipped<MODE>(ga[j] * grad_scale, c), &ma[j], &va[j], lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  // tail (n not a multiple of 4)
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    adam_element(&p[i], clipped<MODE>(g[i] * grad_scale, c), &m[i], &v[i], lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
}

}  // namespace gradclip
}  // namespace mimo

extern "C" size_t mimo_grad_clip_scratch_bytes(void) {
  return sizeof(double) * mimo::gradclip::kMaxBlocks + sizeof(mimo::gradclip::Verdict);
}

extern "C" int mimo_adam_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                      float beta1, float beta2, float eps, float weight_decay, float* step_dev,
                                      float grad_scale, const float* amp_scale, const float* found_inf, int32_t clip_mode,
                                      float clip, float* clip_out, void* scratch, mimo_stream stream) {
  using namespace mimo;
  using namespace mimo::gradclip;
  if (!params || !grads || !exp_avg || !exp_avg_sq || n < 0 || !step_dev || !clip_out || !scratch ||
      ((uintptr_t)scratch & 7) || (clip_mode != MIMO_CLIP_NORM && clip_mode != MIMO_CLIP_VALUE) || !(clip > 0.f)) {
    set_error("mimo_adam_step_clipped: invalid argument (clip_mode 1 = norm or 2 = value, clip > 0, scratch of "
              "mimo_grad_clip_scratch_bytes() bytes, 8-byte aligned)");
    return MIMO_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(scratch);
  Verdict* verdict = reinterpret_cast<Verdict*>(partial + kMaxBlocks);
  const int blocks = (int)std::min<int64_t>(ceil_div64(n / 4 + 1, 256), kMaxBlocks);
  int rows = 0;
  if (clip_mode == MIMO_CLIP_NORM && n > 0) {
    rows = blocks;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, st, grads, n, grad_scale, amp_scale, partial);
    MIMO_KERNEL_CHECK();
  }
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, rows, clip, found_inf, step_dev,
                     clip_out, verdict);
  MIMO_KERNEL_CHECK();
  if (n == 0) return MIMO_OK;
  if (clip_mode == MIMO_CLIP_NORM)
    hipLaunchKernelGGL(adam_clipped_kernel<MIMO_CLIP_NORM>, dim3(blocks), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n,
                       lr, beta1, beta2, eps, weight_decay, grad_scale, (const float*)step_dev, amp_scale, clip,
                       (const Verdict*)verdict);
  else
    hipLaunchKernelGGL(adam_clipped_kernel<MIMO_CLIP_VALUE>, dim3(blocks), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq,
                       n, lr, beta1, beta2, eps, weight_decay, grad_scale, (const float*)step_dev, amp_scale, clip,
                       (const Verdict*)verdict);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}
