// What the scoring kernels share (score_rules.hip: the ensemble's mixture predictive; score_evidential.hip: the evidential
// model's Student-t predictive): the workspace, the per-pixel tally, the workgroup prologue / epilogue that turn a
// workgroup's pixels into one partial row, and the fold of the partial rows into the accumulators.
//
// A pixel that is scored adds its PIT bin, a count and the three fp32 values its maps get; sums are doubles in a FIXED order
// (thread -> workgroup tree -> partial row -> fold over the rows), counts are integer atomics in LDS: the same sequence of
// calls gives the same bits, whichever of the kernels made them.
#pragma once
#include "../common.h"

namespace mimo {
namespace score {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kMaxK = 64;        // PIT thresholds
constexpr int kBins = kMaxK + 1; // bin j = first k with u < p_k; bin K = never below (eval_stats.hip: eval_pixel)
// [0,65) bins, 65 n, 66 n_masked, 67 n_nonfinite, 68 sum NLL, 69 sum CRPS, 70 sum PIT (doubles); 71 the most iterations
// the incomplete-beta continued fraction of any pixel took (score_evidential.hip alone writes and folds it: a diagnostic,
// not a result)
constexpr int kAccWords = 72;
constexpr int kFolded = 71;
constexpr int kIterWord = 71;
constexpr int kBlocks = 1024;    // partial rows = the most workgroups of one launch

// The torch-owned workspace (mimo_score_workspace_bytes; zeroed by the caller at reset).
struct Workspace {
  u64 acc[kAccWords];
  u64 part[kBlocks][kAccWords];
};

__device__ __forceinline__ double as_double(u64 v) { return __longlong_as_double((long long)v); }
__device__ __forceinline__ u64 as_u64(double v) { return (u64)__double_as_longlong(v); }

struct Tally {
  u32 n = 0, nm = 0, nf = 0;
  double nll = 0.0, crps = 0.0, pit = 0.0;
};

// bin and sums of one scored pixel, from the fp32 values its maps get
__device__ __forceinline__ void tally_pixel(float pit, float nll, float crps, const float* __restrict__ zt, int K,
                                            u32* __restrict__ bins, Tally& t) {
  int j = 0;  // first threshold with pit < p_j: lower bound over the table padded to 64 with +inf
#pragma unroll
  for (int step = 32; step > 0; step >>= 1) j += (pit < zt[j + step - 1]) ? 0 : step;
  j += (pit < zt[j]) ? 0 : 1;
  j = j > K ? K : j;
  atomicAdd(&bins[j], 1u);
  ++t.n;
  t.nll += (double)nll;
  t.crps += (double)crps;
  t.pit += (double)pit;
}

__device__ __forceinline__ float pick(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ void put(float4& v, int k, float x) {
  v.x = k == 0 ? x : v.x;
  v.y = k == 1 ? x : v.y;
  v.z = k == 2 ? x : v.z;
  v.w = k == 3 ? x : v.w;
}

// thresholds and per-wave bins in; one partial row per workgroup out (red / redn: 256 entries per quantity).
// A: a kernel's argument block with the thresholds pk [K] and the partial rows part.
template <class A>
__device__ __forceinline__ void block_prologue(const A& a, float* zt, u32* bins) {
  const int tid = threadIdx.x;
  if (tid <= kMaxK) zt[tid] = tid < a.K ? a.pk[tid] : INFINITY;
  for (int i = tid; i < 4 * (kBins + 3); i += 256) bins[i] = 0u;
  __syncthreads();
}

template <class A>
__device__ __forceinline__ void block_epilogue(const A& a, const Tally& t, const u32* bins, double* red, u32* redn) {
  const int tid = threadIdx.x;
  red[tid] = t.nll;
  red[256 + tid] = t.crps;
  red[512 + tid] = t.pit;
  redn[tid] = t.n;
  redn[256 + tid] = t.nm;
  redn[512 + tid] = t.nf;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        red[256 * k + tid] += red[256 * k + tid + off];
        redn[256 * k + tid] += redn[256 * k + tid + off];
      }
    }
    __syncthreads();
  }
  u64* row = a.part + (size_t)blockIdx.x * kAccWords;
  constexpr int W = kBins + 3;
  if (tid < kBins) row[tid] = (u64)bins[tid] + bins[W + tid] + bins[2 * W + tid] + bins[3 * W + tid];
  if (tid >= 65 && tid < 68) row[tid] = redn[256 * (tid - 65)];
  if (tid >= 68 && tid < 71) row[tid] = as_u64(red[256 * (tid - 68)]);
}

// acc[j] += sum over the first `rows` partial rows of column j, j < columns (kFolded; kFolded + 1 takes the larger of
// acc[kIterWord] and the rows' iteration counts as well); rows in a fixed order.  score_rules.hip holds the kernel.
int fold_partials(Workspace* ws, int rows, int columns, hipStream_t stream);

}  // namespace score
}  // namespace mimo
