// Column reductions of per-workgroup partial rows (grid_colsum2, the one-launch machinery the statistics kernels of the other
// operator groups share: ew_device.h).
#include "ew_device.h"

namespace mimo {

// ---------------------------------------------------------------------------------------
// two-level column reduction
// ---------------------------------------------------------------------------------------
__global__ void rowsum_kernel(const float* __restrict__ partial, int rows, int cols, int rows_per_chunk,
                              double* __restrict__ sums) {
  __shared__ double red[256];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const int r0 = blockIdx.y * rows_per_chunk;
  const int r1 = min(rows, r0 + rows_per_chunk);
  double s = 0.0;
  if (col < cols)
    for (int r = r0 + rl; r < r1; r += 4) s += (double)partial[(size_t)r * cols + col];
  red[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0 && col < cols) sums[(size_t)blockIdx.y * cols + col] = red[cl] + red[64 + cl] + red[128 + cl] + red[192 + cl];
}

int rowsum_launch(const float* partial, int rows, int cols, double* sums, int* chunks, hipStream_t s) {
  int nch = ceil_div(rows, 32);
  if (nch > kMaxChunks) nch = kMaxChunks;
  if (nch < 1) nch = 1;
  const int rpc = ceil_div(rows, nch);
  nch = ceil_div(rows, rpc);
  *chunks = nch;
  hipLaunchKernelGGL(rowsum_kernel, dim3(ceil_div(cols, 64), nch), dim3(256), 0, s, partial, rows, cols, rpc, sums);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// out[c] = sum over rows of partial[r][c]  (conv bias gradient)
__global__ __launch_bounds__(kColsumThreads) void colsum_vec_kernel(const float* __restrict__ partial, int rows, int cols,
                                                                    int C, float* __restrict__ out) {
  __shared__ double red[2048];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  double s, unused;
  grid_colsum2(partial, rows, (size_t)cols, c, c, c < C, false, red, &s, &unused);
  if (c < C && threadIdx.x < 64) out[c] = (float)s;
}

int colsum_vec_launch(const float* partial, int rows, int cols, int C, float* out, hipStream_t st) {
  hipLaunchKernelGGL(colsum_vec_kernel, dim3(ceil_div(C, 64)), dim3(kColsumThreads), 0, st, partial, rows, cols, C, out);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

}  // namespace mimo
