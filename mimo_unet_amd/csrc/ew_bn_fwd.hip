// BatchNorm forward: batch / running statistics -> scale / shift, BatchNorm + ReLU (+ Dropout2d, + MaxPool2d) apply.
#include "ew_device.h"

namespace mimo {

// ---------------------------------------------------------------------------------------
// BatchNorm statistics -> scale/shift
// ---------------------------------------------------------------------------------------

// The finalize kernel of the rowsum route runs 256 threads per 64 columns: four groups each add every fourth chunk row (the
// serial walk over up to kMaxChunks rows was most of its ~8 us), the group totals are added in fixed order.  Two columns
// in one walk (sum and sum of squares): one barrier pair.  Every thread of the workgroup must call this; the totals are
// returned to all of them.
__device__ __forceinline__ void chunk_total2(const double* __restrict__ col_a, const double* __restrict__ col_b, size_t stride,
                                             int chunks, bool valid, double* red /*[512]*/, double* ta, double* tb) {
  double sa = 0.0, sb = 0.0;
  if (valid)
    for (int k = threadIdx.x >> 6; k < chunks; k += 4) {
      sa += col_a[(size_t)k * stride];
      sb += col_b[(size_t)k * stride];
    }
  __syncthreads();
  red[threadIdx.x] = sa;
  red[256 + threadIdx.x] = sb;
  __syncthreads();
  const int cl = threadIdx.x & 63;
  *ta = (red[cl] + red[64 + cl]) + (red[128 + cl] + red[192 + cl]);
  *tb = (red[256 + cl] + red[320 + cl]) + (red[384 + cl] + red[448 + cl]);
}

// Channel c < Cp of a training forward from its sum s1 and sum of squares s2 over `count` elements: mean / invstd, the
// scale / shift that BatchNorm + affine apply, the running statistics (pad channels c >= C: zeros).
// status != nullptr: a convolution output that is not finite (an input / weight outside the fp16 range of the split forward, a
// diverged run) shows in its channel sums: recorded for mimo_plan_status instead of surfacing only as NaNs downstream
__device__ __forceinline__ void bn_fwd_finalize_channel(
    int c, int C, double s1, double s2, double count, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ running_mean, float* __restrict__ running_var, float momentum, float eps, float* __restrict__ mean,
    float* __restrict__ invstd, float* __restrict__ scale, float* __restrict__ shift, int* __restrict__ status) {
  if (c >= C) {
    mean[c] = 0.f;
    invstd[c] = 0.f;
    scale[c] = 0.f;
    shift[c] = 0.f;
    return;
  }
  if (status && !(isfinite(s1) && isfinite(s2))) atomicOr(status, kStatusFwdStats);
  const double m = s1 / count;
  double var = s2 / count - m * m;
  var = var > 0.0 ? var : 0.0;
  const double is = 1.0 / sqrt(var + (double)eps);
  const double sc = (double)gamma[c] * is;
  mean[c] = (float)m;
  invstd[c] = (float)is;
  scale[c] = (float)sc;
  shift[c] = (float)((double)beta[c] - m * sc);
  const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
  running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
  running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
}

// second step of the rowsum route (more than kColsumMaxRows partial rows: plan.hip convbn_forward, ops_api.hip); the chunk
// sums carry a partial that is not finite, so the status word is raised here as in bn_fwd_stats_kernel
__global__ void bn_fwd_finalize_kernel(const double* __restrict__ sums, int chunks, int cout_pad, int C, int Cp,
                                       double count, const float* __restrict__ gamma, const float* __restrict__ beta,
                                       float* __restrict__ running_mean, float* __restrict__ running_var,
                                       float momentum, float eps, float* __restrict__ mean, float* __restrict__ invstd,
                                       float* __restrict__ scale, float* __restrict__ shift, int* __restrict__ status) {
  __shared__ double red[512];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int cols = 2 * cout_pad;
  double s1, s2;
  chunk_total2(sums + c, sums + cout_pad + c, cols, chunks, c < C, red, &s1, &s2);
  if (c >= Cp || threadIdx.x >= 64) return;
  bn_fwd_finalize_channel(c, C, s1, s2, count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift,
                          status);
}

// rowsum + bn_fwd_finalize in one launch: partial rows [rows][2][cout_pad] straight from the convolution epilogue
__global__ __launch_bounds__(kColsumThreads) void bn_fwd_stats_kernel(
    const float* __restrict__ partial, int rows, int cout_pad, int C, int Cp, double count, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ running_mean, float* __restrict__ running_var, float momentum,
    float eps, float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ scale, float* __restrict__ shift,
    int* __restrict__ status) {
  __shared__ double red[2048];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  double s1, s2;
  grid_colsum2(partial, rows, (size_t)2 * cout_pad, c, cout_pad + c, c < C, true, red, &s1, &s2);
  if (c >= Cp || threadIdx.x >= 64) return;
  bn_fwd_finalize_channel(c, C, s1, s2, count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift,
                          status);
}

int bn_fwd_stats_launch(const float* partial, int rows, int cout_pad, int C, int Cp, int64_t count, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* mean,
                        float* invstd, float* scale, float* shift, int* status, hipStream_t st) {
  hipLaunchKernelGGL(bn_fwd_stats_kernel, dim3(ceil_div(Cp, 64)), dim3(kColsumThreads), 0, st, partial, rows, cout_pad, C, Cp,
                     (double)count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift, status);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

int bn_fwd_finalize_launch(const double* sums, int chunks, int cout_pad, int C, int Cp, int64_t count,
                           const float* gamma, const float* beta, float* running_mean, float* running_var,
                           float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                           int* status, hipStream_t st) {
  hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3(ceil_div(Cp, 64)), dim3(256), 0, st, sums, chunks, cout_pad, C, Cp,
                     (double)count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift, status);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

__global__ void bn_eval_prepare_kernel(int C, int Cp, const float* __restrict__ gamma, const float* __restrict__ beta,
                                       const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                       float eps, float* __restrict__ mean, float* __restrict__ invstd,
                                       float* __restrict__ scale, float* __restrict__ shift, int* __restrict__ status) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Cp) return;
  if (c >= C) {
    mean[c] = 0.f;
    invstd[c] = 0.f;
    scale[c] = 0.f;
    shift[c] = 0.f;
    return;
  }
  const double m = running_mean[c];
  const double is = 1.0 / sqrt((double)running_var[c] + (double)eps);
  const double sc = (double)gamma[c] * is;
  // running statistics poisoned by an earlier training step (a NaN shift would be dropped by the ReLU's fmaxf: a silently
  // dead channel in eval mode)
  if (status && !(isfinite(m) && isfinite(is) && isfinite(sc))) atomicOr(status, kStatusFwdStats);
  mean[c] = (float)m;
  invstd[c] = (float)is;
  scale[c] = (float)sc;
  shift[c] = (float)((double)beta[c] - m * sc);
}

int bn_eval_prepare_launch(int C, int Cp, const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, float eps, float* mean, float* invstd, float* scale,
                           float* shift, hipStream_t st, int* status) {
  hipLaunchKernelGGL(bn_eval_prepare_kernel, dim3(ceil_div(Cp, 64)), dim3(64), 0, st, C, Cp, gamma, beta,
                     running_mean, running_var, eps, mean, invstd, scale, shift, status);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

template <typename TZ, typename TA>
__global__ void bn_relu_fwd_kernel(const TZ* __restrict__ z, int ldz, TA* __restrict__ a, int lda,
                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                   const float* __restrict__ mask, int C, int Cv, int P, int HW, int* __restrict__ status) {
  const PQ t = pixquad(Cv);
  if (!t.active) return;
  const float4 sc = ld4(scale + 4 * t.q), sh = ld4(shift + 4 * t.q);
  for (int p = t.p; p < P; p += t.pstep) {
    const float4 v = ld4(z + (size_t)p * ldz + 4 * t.q);
    // eval mode (status != nullptr; a training forward sees it in the batch statistics): fmaxf drops a NaN, so a
    // convolution output that is not finite would otherwise vanish here as a silently dead channel
    if (status && !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w))) atomicOr(status, kStatusFwdStats);
    float4 r;
    r.x = fmaxf(fmaf(v.x, sc.x, sh.x), 0.f);
    r.y = fmaxf(fmaf(v.y, sc.y, sh.y), 0.f);
    r.z = fmaxf(fmaf(v.z, sc.z, sh.z), 0.f);
    r.w = fmaxf(fmaf(v.w, sc.w, sh.w), 0.f);
    if (mask) {
      const float4 m = mask4(mask, p / HW, C, 4 * t.q);
      r.x *= m.x;
      r.y *= m.y;
      r.z *= m.z;
      r.w *= m.w;
    }
    st4(a + (size_t)p * lda + 4 * t.q, r);
  }
}

int bn_relu_fwd_launch(const BnReluLayer& L, const float* mask, void* a, int lda, int* status, hipStream_t st) {
  const int Cv = L.Cp / 4;
  const int64_t P = (int64_t)L.N * L.H * L.W;
  MIMO_ST_DISPATCH2(L.dtz, L.dta, TZ, TA,
                    hipLaunchKernelGGL((bn_relu_fwd_kernel<TZ, TA>), pq_grid(Cv, P, kBlocksBnRelu), dim3(256), 0, st,
                                       (const TZ*)L.z, L.ldz, (TA*)a, lda, L.scale, L.shift, mask, L.C, Cv, (int)P, L.H * L.W,
                                       status))
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// BatchNorm + ReLU (+ Dropout2d multipliers) of a tensor whose only spatial consumer is MaxPool2d(2): one thread
// owns a 2x2 window, writes its four activations and their maximum into the pooled tensor — the separate
// pooling pass (a second read of the activation) disappears.  Same arithmetic, bit-identical results.
template <typename TZ, typename TA>
__global__ void bn_relu_pool_fwd_kernel(const TZ* __restrict__ z, int ldz, TA* __restrict__ a, int lda,
                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                        const float* __restrict__ mask, int C, int Cv, int N, int H, int W,
                                        TA* __restrict__ pool, int ldpool, int* __restrict__ status) {
  const PQ t = pixquad(Cv);
  if (!t.active) return;
  const float4 sc = ld4(scale + 4 * t.q), sh = ld4(shift + 4 * t.q);
  const int Hp = H / 2, Wp = W / 2;
  const int P = N * Hp * Wp;
  auto act = [&](float4 v, float4 m) {
    if (status && !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w))) atomicOr(status, kStatusFwdStats);  // as bn_relu_fwd_kernel
    float4 r;
    r.x = fmaxf(fmaf(v.x, sc.x, sh.x), 0.f) * m.x;
    r.y = fmaxf(fmaf(v.y, sc.y, sh.y), 0.f) * m.y;
    r.z = fmaxf(fmaf(v.z, sc.z, sh.z), 0.f) * m.z;
    r.w = fmaxf(fmaf(v.w, sc.w, sh.w), 0.f) * m.w;
    return r;
  };
  PixIter it = pix_iter(t.p, t.pstep, Hp, Wp);
  for (int p = t.p; p < P; p += t.pstep, pix_next(it, Hp, Wp)) {
    const int n = it.n, py = it.y, px = it.x;
    const float4 m = mask ? mask4(mask, n, C, 4 * t.q) : make_float4(1.f, 1.f, 1.f, 1.f);
    const size_t pix = ((size_t)n * H + 2 * py) * W + 2 * px;
    const TZ* zs = z + pix * ldz + 4 * t.q;
    TA* as = a + pix * lda + 4 * t.q;
    const float4 z00 = ld4(zs), z01 = ld4(zs + ldz), z10 = ld4(zs + (size_t)W * ldz), z11 = ld4(zs + (size_t)(W + 1) * ldz);
    const float4 r00 = act(z00, m), r01 = act(z01, m), r10 = act(z10, m), r11 = act(z11, m);
    st4(as, r00);
    st4(as + lda, r01);
    st4(as + (size_t)W * lda, r10);
    st4(as + (size_t)(W + 1) * lda, r11);
    // rounding to the storage type is monotonic: max of the rounded values == rounded max
    st4(pool + (size_t)p * ldpool + 4 * t.q, f4max(f4max(r00, r01), f4max(r10, r11)));
    // odd sizes: the last column / row belongs to no window but is still an activation
    if ((W & 1) && px == Wp - 1) {
      st4(as + 2 * (size_t)lda, act(ld4(zs + 2 * (size_t)ldz), m));
      st4(as + (size_t)(W + 2) * lda, act(ld4(zs + (size_t)(W + 2) * ldz), m));
    }
    if ((H & 1) && py == Hp - 1) {
      st4(as + 2 * (size_t)W * lda, act(ld4(zs + 2 * (size_t)W * ldz), m));
      st4(as + (2 * (size_t)W + 1) * lda, act(ld4(zs + (2 * (size_t)W + 1) * ldz), m));
      if ((W & 1) && px == Wp - 1) st4(as + (2 * (size_t)W + 2) * lda, act(ld4(zs + (2 * (size_t)W + 2) * ldz), m));
    }
  }
}

int bn_relu_pool_fwd_launch(const BnReluLayer& L, const float* mask, void* a, int lda, void* pool, int ldpool, int* status,
                            hipStream_t st) {
  const int Cv = L.Cp / 4;
  MIMO_ST_DISPATCH2(L.dtz, L.dta, TZ, TA,
                    hipLaunchKernelGGL((bn_relu_pool_fwd_kernel<TZ, TA>), pq_grid(Cv, (int64_t)L.N * (L.H / 2) * (L.W / 2), 4096),
                                       dim3(256), 0, st, (const TZ*)L.z, L.ldz, (TA*)a, lda, L.scale, L.shift, mask, L.C, Cv, L.N,
                                       L.H, L.W, (TA*)pool, ldpool, status))
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

}  // namespace mimo
