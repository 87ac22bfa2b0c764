// The sums of the step-tail kernels (optim.hip, evidential_eval.hip), written once: K double sums per thread folded by a
// workgroup of 256 threads, and the eight scalars of a validation-type step formed from the totals.
//
// The order of the additions is a contract (the same bits every run, and the bits the tests and recorded results hold):
//   - every thread adds its own elements / partial rows in ascending index order (threadIdx.x, + the stride, ...);
//   - the workgroup folds red[k][t] += red[k][t + off] for off = 128, 64, ..., 1, every row k at every level;
//   - no wave butterfly, no atomics.  (grad_clip.hip's block_sum folds a wave first: another order, kept apart.)
//
// block_reduce_rows owns its LDS array instead of taking a reference to the kernel's, and nothing here is `__restrict__`:
// hipcc optimises a device function on its own before it inlines it, a reference would be a flat pointer there, and either
// changes the machine code of the calling kernels (scripts/kernel_isa_diff.py).
#pragma once
#include <hip/hip_runtime.h>

namespace mimo {

constexpr int kReduceThreads = 256;  // blockDim.x of every kernel that calls block_reduce_rows

using ReduceRow = const double[kReduceThreads];

// Returns red with red[k][0] = sum over the workgroup of acc[k], valid for every thread (ends behind a __syncthreads()).
// One LDS array per K; a kernel calls it once.  It holds barriers and a tree wired to 256 threads, and nothing enforces
// either: every thread of the workgroup must reach the call (no early return in front of it), and the kernel must be
// launched with blockDim.x == kReduceThreads.
template <int K>
__device__ __forceinline__ ReduceRow* block_reduce_rows(const double (&acc)[K]) {
  __shared__ double red[K][kReduceThreads];
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int off = kReduceThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
  return red;
}

// The eight scalars of a validation-type step from its totals (compute_regression_metrics, mimo/metrics.py:22-34):
// tot:     [0] loss, [1] err^2, [2] |err|, [3] y, [4] y^2, [5] clip(aleatoric_std), [6] clip(epistemic_std)
// scalars: [0] mean loss, [1] mae, [2] mse, [3] rmse, [4] r2, [5] mean clip(aleatoric_std, 0, 5),
//          [6] mean clip(epistemic_std, 0, 5), [7] element count
__device__ __forceinline__ void write_step_scalars(const double* tot, double count, float* scalars) {
  const double mse = tot[1] / count;
  const double ss_tot = tot[4] - tot[3] * tot[3] / count;
  scalars[0] = (float)(tot[0] / count);
  scalars[1] = (float)(tot[2] / count);
  scalars[2] = (float)mse;
  scalars[3] = (float)sqrt(mse);
  scalars[4] = (float)(1.0 - tot[1] / ss_tot);
  scalars[5] = (float)(tot[5] / count);
  scalars[6] = (float)(tot[6] / count);
  scalars[7] = (float)count;
}

}  // namespace mimo
