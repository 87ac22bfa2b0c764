// 1x1 head and the NLL losses, forward and backward (the per-pixel NLL gradient they share with GS_HEAD: ew_device.h).
#include "ew_device.h"

namespace mimo {

// ---------------------------------------------------------------------------------------
// 1x1 head and the NLL losses
// ---------------------------------------------------------------------------------------
// G lanes share a pixel (G = power of two >= channel quads): every lane loads one float4 of the pixel's
// channel row — a wave reads 64 consecutive float4, fully coalesced — multiplies it with its slice of the
// 1x1 weights, and a butterfly of G-lane shuffles completes the Co dot products.  (One thread per pixel
// reading its own 128-byte row touched 64 cache lines per load instruction and ran at 1 TB/s.)
template <int G, int CO, typename T>
__global__ void head_fwd_kernel(const T* __restrict__ a, int lda, const float* __restrict__ w,
                                const float* __restrict__ bias, int C, int Cp, int Co, int N, int S, int s, int HW,
                                float* __restrict__ out, int* __restrict__ status, const float* __restrict__ in_scale,
                                const float* __restrict__ in_shift) {
  // in_scale != nullptr: `a` is the pre-activation tensor of the decoder's last convolution, its BatchNorm + ReLU is applied here
  // CO = compile-time bound of Co (2: one target, 4: the evidential head, 8: the rest); UN pixels per thread and
  // iteration, their loads issued together (one 16-byte load in flight per thread ran at 3.4 TB/s)
  const int g = threadIdx.x % G, pl = threadIdx.x / G;
  constexpr int PPB = 256 / G, UN = 4;
  float wq[CO][4], bs[CO];
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    bs[co] = co < Co ? bias[co] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) wq[co][j] = (co < Co && 4 * g + j < C) ? w[co * C + 4 * g + j] : 0.f;
  }
  const bool has = 4 * g < Cp;
  const bool fin = in_scale != nullptr;
  const float4 isc = (fin && has) ? ld4(in_scale + 4 * g) : f4zero(), ish = (fin && has) ? ld4(in_shift + 4 * g) : f4zero();
  const int64_t P = (int64_t)N * HW, stride = (int64_t)gridDim.x * PPB;
  for (int64_t p0 = (int64_t)blockIdx.x * PPB + pl; p0 < P; p0 += stride * UN) {
    float4 v[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t p = p0 + u * stride;
      v[u] = (has && p < P) ? ld4(a + p * lda + 4 * g) : f4zero();
      if (fin) v[u] = bn_relu4(v[u], isc, ish);  // (lanes without channels: relu(0 * 0 + 0) = 0)
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t p = p0 + u * stride;
      float acc[CO];
#pragma unroll
      for (int co = 0; co < CO; ++co)
        acc[co] = fmaf(v[u].x, wq[co][0], fmaf(v[u].y, wq[co][1], fmaf(v[u].z, wq[co][2], v[u].w * wq[co][3])));
#pragma unroll
      for (int off = 1; off < G; off <<= 1)
#pragma unroll
        for (int co = 0; co < CO; ++co) acc[co] += __shfl_xor(acc[co], off);
      if (p < P) {
        const int n = (int)(p / HW);
        const int yx = (int)(p - (int64_t)n * HW);
#pragma unroll
        for (int co = 0; co < CO; ++co)
          if (co < Co && co % G == g) {
            const float o = acc[co] + bs[co];
            out[(((int64_t)n * S + s) * Co + co) * HW + yx] = o;
            if (status && !isfinite(o)) atomicOr(status, kStatusLogits);
          }
      }
    }
  }
}

int head_fwd_launch(const void* a, int dt, int lda, const float* w, const float* bias, int C, int Co, int N, int S, int s,
                    int HW, float* out, hipStream_t st, int* status, const float* in_scale, const float* in_shift) {
  if (Co > kMaxHeadOut || C > 256) {
    set_error("head: out_channels %d > %d or filter_base_count %d > 256 unsupported", Co, kMaxHeadOut, C);
    return MIMO_ERR_INVALID;
  }
  const int Cp = pad_channels(C), Cv = Cp / 4;
  int G = 2;
  while (G < Cv) G <<= 1;
  const int64_t P = (int64_t)N * HW;
  const int blocks = (int)std::min<int64_t>(ceil_div64(P, (256 / G) * 4), 4096);
#define HEAD_LAUNCH2(GG, CC)                                                                                         \
  MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL((head_fwd_kernel<GG, CC, T>), dim3(blocks), dim3(256), 0, st, (const T*)a, lda, w, bias, \
                                             C, Cp, Co, N, S, s, HW, out, status, in_scale, in_shift))
#define HEAD_LAUNCH(GG)             \
  if (Co <= 2) {                    \
    HEAD_LAUNCH2(GG, 2);            \
  } else if (Co <= 4) {             \
    HEAD_LAUNCH2(GG, 4);            \
  } else {                          \
    HEAD_LAUNCH2(GG, kMaxHeadOut);  \
  }
  switch (G) {
    case 2: HEAD_LAUNCH(2); break;
    case 4: HEAD_LAUNCH(4); break;
    case 8: HEAD_LAUNCH(8); break;
    case 16: HEAD_LAUNCH(16); break;
    case 32: HEAD_LAUNCH(32); break;
    default: HEAD_LAUNCH(64); break;
  }
#undef HEAD_LAUNCH
#undef HEAD_LAUNCH2
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

__global__ void loss_fwd_kernel(const float* __restrict__ out, const float* __restrict__ label,
                                const float* __restrict__ mask, const int64_t* __restrict__ perm, int N, int S, int Co,
                                int HW, int kind, float eps_min, float eps_max, float* __restrict__ partial) {
  __shared__ float red[256];
  const int s = blockIdx.y;
  const int Ct = Co / 2;
  const int64_t total = (int64_t)N * Ct * HW;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int yx = (int)(i % HW);
    const int64_t r = i / HW;
    const int tch = (int)(r % Ct);
    const int n = (int)(r / Ct);
    const int64_t src = perm ? perm[(int64_t)s * N + n] : n;
    const float* o = out + (((int64_t)n * S + s) * Co) * HW + yx;
    const float mu = o[(int64_t)tch * HW], lp = o[(int64_t)(Ct + tch) * HW];
    const float y = label[(src * Ct + tch) * HW + yx];
    float v = nll_value(kind, mu - y, lp, eps_min, eps_max);
    if (mask) v *= mask[src * HW + yx];
    acc += v;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(size_t)s * gridDim.x + blockIdx.x] = red[0];
}

int loss_fwd_launch(const float* out, const float* label, const float* mask, const int64_t* perm, int N, int S, int Co,
                    int HW, int kind, float eps_min, float eps_max, float* partial, int* blocks, hipStream_t st) {
  const int64_t total = (int64_t)N * (Co / 2) * HW;
  const int nb = (int)std::min<int64_t>(ceil_div64(total, 256), 512);
  *blocks = nb;
  hipLaunchKernelGGL(loss_fwd_kernel, dim3(nb, S), dim3(256), 0, st, out, label, mask, perm, N, S, Co, HW, kind, eps_min,
                     eps_max, partial);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

__global__ void loss_finalize_kernel(const float* __restrict__ partial, int S, int blocks, double count,
                                     float* __restrict__ loss_out) {
  __shared__ double red[256];
  const int s = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < blocks; i += blockDim.x) acc += (double)partial[(size_t)s * blocks + i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_out[s] = (float)(red[0] / count);
}

int loss_finalize_launch(const float* partial, int S, int blocks, double count, float* loss_out, hipStream_t st) {
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(S), dim3(256), 0, st, partial, S, blocks, count, loss_out);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// CO = compile-time bound of Co (as in head_fwd_kernel); UN pixels per thread and iteration, loads issued together (the
// grid is capped at kEwMaxBlocks partial rows = 16 waves per CU: one pixel at a time left 16 KB in flight per CU)
template <int CO, typename T>
__global__ void head_bwd_kernel(const T* __restrict__ a, int lda, const float* __restrict__ w, int C, int Cv, int Co,
                                int N, int S, int s, int HW, const float* __restrict__ out,
                                const float* __restrict__ dout, const float* __restrict__ dloss,
                                const float* __restrict__ label, const float* __restrict__ mask,
                                const int64_t* __restrict__ perm, int kind, float eps_min, float eps_max, float inv_count,
                                T* __restrict__ da, float* __restrict__ partial, const float* __restrict__ in_scale,
                                const float* __restrict__ in_shift) {
  __shared__ float4 red[256];
  constexpr int UN = 4;
  const PQ t = pixquad(Cv);
  const bool fin = in_scale != nullptr;
  const float4 isc = (fin && t.active) ? ld4(in_scale + 4 * t.q) : f4zero(), ish = (fin && t.active) ? ld4(in_shift + 4 * t.q) : f4zero();
  const int Cp = 4 * Cv, Ct = Co / 2;
  float4 wq[CO], dwacc[CO];
  float dbacc[CO];
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    wq[co] = f4zero();
    dwacc[co] = f4zero();
    dbacc[co] = 0.f;
    if (co < Co && t.active) {
      const int c0 = 4 * t.q;
      wq[co].x = c0 + 0 < C ? w[co * C + c0 + 0] : 0.f;
      wq[co].y = c0 + 1 < C ? w[co * C + c0 + 1] : 0.f;
      wq[co].z = c0 + 2 < C ? w[co * C + c0 + 2] : 0.f;
      wq[co].w = c0 + 3 < C ? w[co * C + c0 + 3] : 0.f;
    }
  }
  const float coef = dloss ? dloss[s] * inv_count : 0.f;
  if (t.active) {
    const int P = N * HW;
    for (int p0 = t.p; p0 < P; p0 += UN * t.pstep) {
      float dl[UN][CO], mu[UN][CO / 2], lp[UN][CO / 2], y[UN][CO / 2], mk[UN];
      float4 av[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int p = min(p0 + u * t.pstep, P - 1);  // past the end: a valid pixel, results discarded
        const int n = p / HW;
        const int yx = p - n * HW;
        const int64_t obase = (((int64_t)n * S + s) * Co) * HW + yx;
#pragma unroll
        for (int co = 0; co < CO; ++co) dl[u][co] = (dout && co < Co) ? dout[obase + (int64_t)co * HW] : 0.f;
        mk[u] = 1.f;
        if (dloss) {
          const int64_t src = perm ? perm[(int64_t)s * N + n] : n;
          if (mask) mk[u] = mask[src * HW + yx];
#pragma unroll
          for (int tc = 0; tc < CO / 2; ++tc)
            if (tc < Ct) {
              mu[u][tc] = out[obase + (int64_t)tc * HW];
              lp[u][tc] = out[obase + (int64_t)(Ct + tc) * HW];
              y[u][tc] = label[(src * Ct + tc) * HW + yx];
            }
        }
        av[u] = ld4(a + (size_t)p * lda + 4 * t.q);
        if (fin) av[u] = bn_relu4(av[u], isc, ish);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int p = p0 + u * t.pstep;
        if (p >= P) break;
        if (dloss) {
#pragma unroll
          for (int tc = 0; tc < CO / 2; ++tc)
            if (tc < Ct) {
              float gm, gl;
              nll_grad(kind, mu[u][tc] - y[u][tc], lp[u][tc], eps_min, eps_max, &gm, &gl);
#pragma unroll
              for (int co = 0; co < CO; ++co) {  // dl[tc] and dl[Ct + tc], with compile-time register indices
                if (co == tc) dl[u][co] += coef * mk[u] * gm;
                if (co == Ct + tc) dl[u][co] += coef * mk[u] * gl;
              }
            }
        }
        float4 g = f4zero();
#pragma unroll
        for (int co = 0; co < CO; ++co)
          if (co < Co) {
            g.x = fmaf(dl[u][co], wq[co].x, g.x);
            g.y = fmaf(dl[u][co], wq[co].y, g.y);
            g.z = fmaf(dl[u][co], wq[co].z, g.z);
            g.w = fmaf(dl[u][co], wq[co].w, g.w);
            dwacc[co].x = fmaf(dl[u][co], av[u].x, dwacc[co].x);
            dwacc[co].y = fmaf(dl[u][co], av[u].y, dwacc[co].y);
            dwacc[co].z = fmaf(dl[u][co], av[u].z, dwacc[co].z);
            dwacc[co].w = fmaf(dl[u][co], av[u].w, dwacc[co].w);
            dbacc[co] += dl[u][co];
          }
        st4(da + (size_t)p * Cp + 4 * t.q, g);
      }
    }
  }
  // partial row: [Co][Cp] weight gradient followed by [Co] bias gradient (from quad 0 threads)
  float* row = partial + (size_t)blockIdx.x * (Co * Cp + Co);
  for (int co = 0; co < Co; ++co) {
    float4 v = f4zero();
    float b = 0.f;
#pragma unroll
    for (int k = 0; k < CO; ++k)
      if (k == co) {
        v = dwacc[k];
        b = dbacc[k];
      }
    const float4 sw = quad_block_sum(v, t, red);
    if (t.pl == 0 && t.q < Cv) st4(row + co * Cp + 4 * t.q, sw);
    const float4 sb = quad_block_sum(make_float4(b, 0.f, 0.f, 0.f), t, red);
    if (t.pl == 0 && t.q == 0) row[Co * Cp + co] = sb.x;
  }
}

int head_bwd_launch(const void* a, int dt, int lda, const float* w, int C, int Cp, int Co, int N, int S, int s, int HW,
                    const float* out, const float* dout, const float* dloss, const float* label, const float* mask,
                    const int64_t* perm, int kind, float eps_min, float eps_max, void* da, float* partial, int* rows,
                    hipStream_t st, const float* in_scale, const float* in_shift) {
  if (Co > kMaxHeadOut || (Co & 1)) {
    set_error("head: out_channels %d unsupported", Co);
    return MIMO_ERR_INVALID;
  }
  const int Cv = Cp / 4;
  dim3 grid = pq_grid(Cv, (int64_t)N * HW);
  grid.y = 1;  // Cv <= 64 for the head (filter_base_count <= 256)
  *rows = grid.x;
  const float inv_count = 1.f / (float)((double)N * (Co / 2) * HW);
#define HEAD_BWD_LAUNCH(CC)                                                                                              \
  MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL((head_bwd_kernel<CC, T>), grid, dim3(256), 0, st, (const T*)a, lda, w, C, Cv, Co, N, S, s, \
                                             HW, out, dout, dloss, label, mask, perm, kind, eps_min, eps_max, inv_count, (T*)da,  \
                                             partial, in_scale, in_shift))
  if (Co <= 2) {
    HEAD_BWD_LAUNCH(2);
  } else if (Co <= 4) {
    HEAD_BWD_LAUNCH(4);
  } else {
    HEAD_BWD_LAUNCH(kMaxHeadOut);
  }
#undef HEAD_BWD_LAUNCH
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// column sums + finalize in one launch: partial rows [rows][Co*Cp + Co] from head_bwd
__global__ __launch_bounds__(kColsumThreads) void head_bwd_stats_kernel(const float* __restrict__ partial, int rows, int C,
                                                                        int Cp, int Co, float* __restrict__ dw,
                                                                        float* __restrict__ db) {
  __shared__ double red[2048];
  const int cols = Co * Cp + Co;
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  double s, unused;
  grid_colsum2(partial, rows, (size_t)cols, i, i, i < cols, false, red, &s, &unused);
  if (i >= cols || threadIdx.x >= 64) return;
  if (i < Co * Cp) {
    const int co = i / Cp, c = i - co * Cp;
    if (c < C) dw[co * C + c] = (float)s;
  } else {
    db[i - Co * Cp] = (float)s;
  }
}

int head_bwd_stats_launch(const float* partial, int rows, int C, int Cp, int Co, float* dw, float* db, hipStream_t st) {
  hipLaunchKernelGGL(head_bwd_stats_kernel, dim3(ceil_div(Co * Cp + Co, 64)), dim3(kColsumThreads), 0, st, partial, rows, C, Cp,
                     Co, dw, db);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

}  // namespace mimo
