// BatchNorm + ReLU backward (reduce pass, statistics, apply pass; pair-split storage of dz) and, in front of it, the backward
// gathers that feed it from the padded-domain data gradient (pool_bwd, fold_slice, up_bwd).  The gathers are compiled
// in this unit on purpose: up_bwd_kernel is the one caller of pixquad() with xcd_bands set, and a unit without such a
// caller has the argument folded into pixquad before it is inlined, which reorders the scalar prologue of the kernels that
// read gridDim again later (bn_bwd_apply_kernel, split_pairs_kernel): same results, not the same machine code.
#include "ew_device.h"

namespace mimo {

// ---------------------------------------------------------------------------------------
// backward gathers
// ---------------------------------------------------------------------------------------
// MaxPool2d(2) backward (pool_bwd_kernel, GS_POOL)
__device__ __forceinline__ float route_max(float g, float v00, float v01, float v10, float v11, int self) {
  // first maximum in scan order (0,0),(0,1),(1,0),(1,1) receives the gradient (strict '>' update)
  int arg = 0;
  float m = v00;
  if (v01 > m) { m = v01; arg = 1; }
  if (v10 > m) { m = v10; arg = 2; }
  if (v11 > m) { m = v11; arg = 3; }
  return arg == self ? g : 0.f;
}

// One thread owns a 2x2 window: one folded gradient read, the four activations once (not once per
// window member), four stores.  Rows / columns outside every window (odd H or W) receive no pooled gradient.
// skip != nullptr: the tensor is also the skip input of an Up block; that block's padded-domain data gradient
// (channels [0, Cp) of its own buffer, pixel pitch ldsk) is folded and added here, so the skip slice is never
// copied out (da = pool route + skip fold, the same two operands in the same order as the former
// fold_slice + accumulating pool_bwd pair).
template <typename T>
__global__ void pool_bwd_kernel(const T* __restrict__ dxpad, int ldp, int choff, const T* __restrict__ a,
                                int lda, T* __restrict__ da, int ldda, int N, int H, int W, int Cv, int accumulate,
                                const T* __restrict__ skip, int ldsk) {
  const PQ t = pixquad(Cv);
  if (!t.active) return;
  const int Hp = H / 2, Wp = W / 2;
  const int P = N * Hp * Wp;
  PixIter it = pix_iter(t.p, t.pstep, Hp, Wp);
  for (int p = t.p; p < P; p += t.pstep, pix_next(it, Hp, Wp)) {
    const int n = it.n, py = it.y, px = it.x;
    const float4 g = fold_read(dxpad, ldp, n, py, px, Hp, Wp, choff + 4 * t.q);
    const size_t pix = ((size_t)n * H + 2 * py) * W + 2 * px;
    const T* src = a + pix * lda + 4 * t.q;
    const float4 v00 = ld4(src), v01 = ld4(src + lda), v10 = ld4(src + (size_t)W * lda), v11 = ld4(src + (size_t)(W + 1) * lda);
    T* dst = da + pix * ldda + 4 * t.q;
    float4 r[4];
#pragma unroll
    for (int self = 0; self < 4; ++self) {
      r[self].x = route_max(g.x, v00.x, v01.x, v10.x, v11.x, self);
      r[self].y = route_max(g.y, v00.y, v01.y, v10.y, v11.y, self);
      r[self].z = route_max(g.z, v00.z, v01.z, v10.z, v11.z, self);
      r[self].w = route_max(g.w, v00.w, v01.w, v10.w, v11.w, self);
    }
    T* d4[4] = {dst, dst + ldda, dst + (size_t)W * ldda, dst + (size_t)(W + 1) * ldda};
    if (accumulate) {
      float4 o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = ld4(d4[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = f4add(r[j], o[j]);
    }
    if (skip) {
      float4 o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = fold_read(skip, ldsk, n, 2 * py + (j >> 1), 2 * px + (j & 1), H, W, 4 * t.q);
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = f4add(r[j], o[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) st4(d4[j], r[j]);
    if (!accumulate) {  // odd sizes: the last row / column belongs to no window (skip gradient only)
      auto rest = [&](int y, int x) {
        st4(da + (((size_t)n * H + y) * W + x) * ldda + 4 * t.q, skip ? fold_read(skip, ldsk, n, y, x, H, W, 4 * t.q) : f4zero());
      };
      if ((W & 1) && px == Wp - 1) {
        rest(2 * py, W - 1);
        rest(2 * py + 1, W - 1);
      }
      if ((H & 1) && py == Hp - 1) {
        rest(H - 1, 2 * px);
        rest(H - 1, 2 * px + 1);
        if ((W & 1) && px == Wp - 1) rest(H - 1, W - 1);
      }
    } else if (skip) {
      auto rest = [&](int y, int x) {
        T* d = da + (((size_t)n * H + y) * W + x) * ldda + 4 * t.q;
        st4(d, f4add(ld4(d), fold_read(skip, ldsk, n, y, x, H, W, 4 * t.q)));
      };
      if ((W & 1) && px == Wp - 1) {
        rest(2 * py, W - 1);
        rest(2 * py + 1, W - 1);
      }
      if ((H & 1) && py == Hp - 1) {
        rest(H - 1, 2 * px);
        rest(H - 1, 2 * px + 1);
        if ((W & 1) && px == Wp - 1) rest(H - 1, W - 1);
      }
    }
  }
}

int pool_bwd_launch(const void* dxpad, int dt, int ldp, int choff, const void* a, int lda, void* da, int ldda, int N, int H,
                    int W, int Cp, int accumulate, hipStream_t st, const void* skip, int ldsk) {
  const int Cv = Cp / 4;
  MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL(pool_bwd_kernel<T>, pq_grid(Cv, (int64_t)N * (H / 2) * (W / 2), kBlocksPoolBwd), dim3(256),
                                             0, st, (const T*)dxpad, ldp, choff, (const T*)a, lda, (T*)da, ldda, N, H, W, Cv,
                                             accumulate, (const T*)skip, ldsk));
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

template <typename T>
__global__ void fold_slice_kernel(const T* __restrict__ dxpad, int ldp, int choff, T* __restrict__ da, int ldda,
                                  int N, int H, int W, int Cv, int accumulate) {
  const PQ t = pixquad(Cv);
  if (!t.active) return;
  const int P = N * H * W;
  PixIter it = pix_iter(t.p, t.pstep, H, W);
  for (int p = t.p; p < P; p += t.pstep, pix_next(it, H, W)) {
    float4 v = fold_read(dxpad, ldp, it.n, it.y, it.x, H, W, choff + 4 * t.q);
    T* dst = da + (size_t)p * ldda + 4 * t.q;
    if (accumulate) v = f4add(v, ld4(dst));
    st4(dst, v);
  }
}

int fold_slice_launch(const void* dxpad, int dt, int ldp, int choff, void* da, int ldda, int N, int H, int W, int Cp,
                      int accumulate, hipStream_t st) {
  const int Cv = Cp / 4;
  MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL(fold_slice_kernel<T>, pq_grid(Cv, (int64_t)N * H * W, 4096), dim3(256), 0, st,
                                             (const T*)dxpad, ldp, choff, (T*)da, ldda, N, H, W, Cv, accumulate));
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// Input pixel i of an x2 align_corners upsample is read by outputs 2i-1 .. 2i+2 only (2i-2 lands on
// i-2 / i-1 for every size; checked exhaustively for in <= 300 and 512..2048 on the CPU).
// Gradient arriving at low-resolution pixel (n, iy, ix), channel quad q: the transposed interpolation over its 4 x 4
// candidates of the padded-domain data gradient, border folds included.
template <typename T>
__device__ __forceinline__ float4 up_bwd_pixel(const T* __restrict__ dxpad, int ldp, int choff, int q, int n, int iy, int ix,
                                               int H, int W, int h, int w, int padT, int padL) {
    float wy[4], wx[4];
    int cy[4], cx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int oy = 2 * iy - 1 + k, ox = 2 * ix - 1 + k;
      wy[k] = (oy >= 0 && oy < 2 * h) ? lerp_weight(oy, iy, h) : 0.f;
      wx[k] = (ox >= 0 && ox < 2 * w) ? lerp_weight(ox, ix, w) : 0.f;
      cy[k] = min(max(oy, 0), 2 * h - 1) + padT;
      cx[k] = min(max(ox, 0), 2 * w - 1) + padL;
    }
    float4 v = f4zero();
    const T* base = dxpad + (size_t)n * (H + 2) * (W + 2) * ldp + choff + 4 * q;
    // the 16 candidates themselves (padded-domain pixel of image pixel (y, x) = (y + 1, x + 1)): 16 independent loads,
    // weights 0 where the candidate does not read this input (adds an exact zero, same sum as skipping it)
    {
      float4 g[4][4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) g[k][j] = ld4(base + ((size_t)(cy[k] + 1) * (W + 2) + (cx[j] + 1)) * ldp);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float ww = wy[k] * wx[j];
          v.x += ww * g[k][j].x;
          v.y += ww * g[k][j].y;
          v.z += ww * g[k][j].z;
          v.w += ww * g[k][j].w;
        }
    }
    if (!(cy[0] >= 2 && cy[3] <= H - 3 && cx[0] >= 2 && cx[3] <= W - 3)) {
      // Near the border some candidates also receive a reflected pad row / column (transpose of the reflect padding: pad
      // row -1 folds onto row 1, pad row H onto row H - 2; columns alike).  Folding is linear, so instead of folding every
      // candidate (up to 4 dependent loads each, 16 times, in divergent loops: the whole launch waited for these threads —
      // 94 us at 4 images per GPU where the data moves in 15) the pad rows / columns enter as two more rows and columns of
      // the weighted sum, with the weight of the image row / column they fold onto: at most 20 more independent loads.
      float ey[2] = {0.f, 0.f}, ex[2] = {0.f, 0.f};  // weight of pad row -1 / H, pad column -1 / W
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ey[0] += cy[k] == 1 ? wy[k] : 0.f;
        ey[1] += cy[k] == H - 2 ? wy[k] : 0.f;
        ex[0] += cx[k] == 1 ? wx[k] : 0.f;
        ex[1] += cx[k] == W - 2 ? wx[k] : 0.f;
      }
      const int pry[2] = {0, H + 1}, prx[2] = {0, W + 1};  // padded-domain indices of the pad rows / columns
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (ey[e] != 0.f) {  // pad row e against the four candidate columns and the two pad columns
          float4 g[6];
#pragma unroll
          for (int j = 0; j < 4; ++j) g[j] = ld4(base + ((size_t)pry[e] * (W + 2) + (cx[j] + 1)) * ldp);
#pragma unroll
          for (int j = 0; j < 2; ++j) g[4 + j] = ld4(base + ((size_t)pry[e] * (W + 2) + prx[j]) * ldp);
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            const float ww = ey[e] * (j < 4 ? wx[j] : ex[j - 4]);
            v.x += ww * g[j].x;
            v.y += ww * g[j].y;
            v.z += ww * g[j].z;
            v.w += ww * g[j].w;
          }
        }
        if (ex[e] != 0.f) {  // pad column e against the four candidate rows
          float4 g[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) g[k] = ld4(base + ((size_t)(cy[k] + 1) * (W + 2) + prx[e]) * ldp);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float ww = wy[k] * ex[e];
            v.x += ww * g[k].x;
            v.y += ww * g[k].y;
            v.z += ww * g[k].z;
            v.w += ww * g[k].w;
          }
        }
      }
    }
    return v;
}

template <typename T>
__global__ void up_bwd_kernel(const T* __restrict__ dxpad, int ldp, int choff, T* __restrict__ da, int ldda,
                              int N, int H, int W, int h, int w, int padT, int padL, int Cv, int accumulate) {
  const PQ t = pixquad(Cv, true);
  if (!t.active) return;
  const int P = N * h * w;
  PixIter it = pix_iter(t.p, t.pstep, h, w);
  for (int p = t.p; p < P; p += t.pstep, pix_next(it, h, w)) {
    float4 v = up_bwd_pixel(dxpad, ldp, choff, t.q, it.n, it.y, it.x, H, W, h, w, padT, padL);
    T* dst = da + (size_t)p * ldda + 4 * t.q;
    if (accumulate) v = f4add(v, ld4(dst));
    st4(dst, v);
  }
}

// (Round 5 measured the transposed counterpart of upcat_fwd2x2 — one thread per 2 x 2 block of low-resolution pixels, its
// four 4 x 4 candidate windows read as one 6 x 6 window, 36 loads per 4 outputs instead of 64: 0.49 -> 0.52 ms per step,
// slower at 165 registers and three waves per SIMD; profiles/r05/upsampling_2x2.txt.  Not kept.)

int up_bwd_launch(const void* dxpad, int dt, int ldp, int choff, void* da, int ldda, int N, int H, int W, int h, int w,
                  int Cp, int accumulate, hipStream_t st) {
  const int Cv = Cp / 4;
  const int padT = (H - 2 * h) / 2, padL = (W - 2 * w) / 2;
  MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL(up_bwd_kernel<T>, pq_grid(Cv, (int64_t)N * h * w, kBlocksUpBwd), dim3(256), 0, st,
                                             (const T*)dxpad, ldp, choff, (T*)da, ldda, N, H, W, h, w, padT, padL, Cv, accumulate));
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// ---------------------------------------------------------------------------------------
// BatchNorm + ReLU backward
// ---------------------------------------------------------------------------------------
// dy = (gradient arriving at the activation) * dropout mask * [relu input > 0], evaluated on the fly by
// both passes (never stored); the arriving gradient per GradSrc (elementwise.h)
__device__ __forceinline__ float4 relu_gate4(float4 g, float4 v, float4 sc, float4 sh) {
  g.x = fmaf(v.x, sc.x, sh.x) > 0.f ? g.x : 0.f;
  g.y = fmaf(v.y, sc.y, sh.y) > 0.f ? g.y : 0.f;
  g.z = fmaf(v.z, sc.z, sh.z) > 0.f ? g.z : 0.f;
  g.w = fmaf(v.w, sc.w, sh.w) > 0.f ? g.w : 0.f;
  return g;
}

// GS_POOL: one thread owns the 2x2 cell (cy, cx) of image n — as pool_bwd_kernel did: one folded read of the pooled
// gradient, the four pre-activation values once, the window's activations re-formed with bn_relu_pool_fwd_kernel's
// arithmetic, the first maximum in scan order takes the gradient, + the folded skip gradient of each pixel.  Cells of the
// last row / column of an odd-sized image hold one or two pixels and no window.  Returns the valid pixels as a bit mask,
// their pre-activation values in zz[] and their dy (dropout multiplier and ReLU gate applied) in g[].
template <typename TZ, typename TA>
__device__ __forceinline__ int pool_cell4(const GradSrc& s, const TZ* z, int ldz, int n, int cy, int cx, int H, int W, int q,
                                          float4 sc, float4 sh, bool masked, float4 m, float4 zz[4], float4 g[4]) {
  const int Hp = H / 2, Wp = W / 2, y0 = 2 * cy, x0 = 2 * cx;
  const bool win = cy < Hp && cx < Wp;
  const int valid = win ? 15 : ((1 | (x0 + 1 < W ? 2 : 0)) | (y0 + 1 < H ? (4 | (x0 + 1 < W ? 8 : 0)) : 0));
  const TZ* zs = z + (((size_t)n * H + y0) * W + x0) * ldz + 4 * q;
#pragma unroll
  for (int j = 0; j < 4; ++j) zz[j] = (valid >> j) & 1 ? ld4(zs + ((size_t)(j >> 1) * W + (j & 1)) * ldz) : f4zero();
  float4 gp = f4zero();
  if (win) gp = fold_read((const TA*)s.dxpad, s.ldp, n, cy, cx, Hp, Wp, s.choff + 4 * q);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    g[j] = (s.skip && ((valid >> j) & 1)) ? fold_read((const TA*)s.skip, s.ldsk, n, y0 + (j >> 1), x0 + (j & 1), H, W, s.skoff + 4 * q)
                                           : f4zero();
  if (win) {
    auto act = [&](float v, float k, float b, float mm) { return fmaxf(fmaf(v, k, b), 0.f) * mm; };
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // route + skip: pool_bwd_kernel's operands in its order
      g[j].x = route_max(gp.x, act(zz[0].x, sc.x, sh.x, m.x), act(zz[1].x, sc.x, sh.x, m.x), act(zz[2].x, sc.x, sh.x, m.x), act(zz[3].x, sc.x, sh.x, m.x), j) + g[j].x;
      g[j].y = route_max(gp.y, act(zz[0].y, sc.y, sh.y, m.y), act(zz[1].y, sc.y, sh.y, m.y), act(zz[2].y, sc.y, sh.y, m.y), act(zz[3].y, sc.y, sh.y, m.y), j) + g[j].y;
      g[j].z = route_max(gp.z, act(zz[0].z, sc.z, sh.z, m.z), act(zz[1].z, sc.z, sh.z, m.z), act(zz[2].z, sc.z, sh.z, m.z), act(zz[3].z, sc.z, sh.z, m.z), j) + g[j].z;
      g[j].w = route_max(gp.w, act(zz[0].w, sc.w, sh.w, m.w), act(zz[1].w, sc.w, sh.w, m.w), act(zz[2].w, sc.w, sh.w, m.w), act(zz[3].w, sc.w, sh.w, m.w), j) + g[j].w;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (masked) {
      g[j].x *= m.x;
      g[j].y *= m.y;
      g[j].z *= m.z;
      g[j].w *= m.w;
    }
    g[j] = relu_gate4(g[j], zz[j], sc, sh);
  }
  return valid;
}

template <int SRC, typename TZ, typename TA>
__device__ __forceinline__ float4 relu_grad4(const GradSrc& s, const HeadLane& hl, const float* mask, int C, int p,
                                             const PixIter& it, int q, int H, int W, float4 v, float4 sc, float4 sh, float* d0,
                                             float* d1) {
  static_assert(SRC != GS_POOL, "pooled tensors: pool_cell4");
  float4 g;
  const int n = it.n;
  float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
  if (mask) m = mask4(mask, n, C, 4 * q);
  if constexpr (SRC == GS_PLAIN) {
    g = ld4((const TA*)s.da + (size_t)p * s.ldda + 4 * q);
  } else if constexpr (SRC == GS_FOLD) {
    g = fold_read((const TA*)s.dxpad, s.ldp, n, it.y, it.x, H, W, 4 * q);
  } else {
    head_dlogit(s.head, hl, p, d0, d1);
    g = f4zero();
    g.x = fmaf(*d1, hl.w1.x, fmaf(*d0, hl.w0.x, g.x));
    g.y = fmaf(*d1, hl.w1.y, fmaf(*d0, hl.w0.y, g.y));
    g.z = fmaf(*d1, hl.w1.z, fmaf(*d0, hl.w0.z, g.z));
    g.w = fmaf(*d1, hl.w1.w, fmaf(*d0, hl.w0.w, g.w));
  }
  if (mask) {
    g.x *= m.x;
    g.y *= m.y;
    g.z *= m.z;
    g.w *= m.w;
  }
  return relu_gate4(g, v, sc, sh);
}

template <typename TZ, typename TA, int SRC>
__global__ __launch_bounds__(kBnReduceThreads) void bnrelu_bwd_reduce_kernel(
    const GradSrc src, const TZ* __restrict__ z, int ldz,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ mask, int C, int Cv, int N, int H, int W,
    float* __restrict__ partial) {
  __shared__ float4 red[kBnReduceThreads];
  const PQ t = pixquad<kBnReduceThreads>(Cv);
  const int Cp = 4 * Cv;
  float4 a1 = f4zero(), a2 = f4zero();
  float4 hw0 = f4zero(), hw1 = f4zero();  // GS_HEAD: the head's weight gradient (this quad's channels x 2 logits), bias gradient
  float hb0 = 0.f, hb1 = 0.f;
  HeadLane hl = {};
  if constexpr (SRC == GS_HEAD) hl = head_lane(src.head, t.q, t.active);
  if (t.active) {
    const float4 sc = ld4(scale + 4 * t.q), sh = ld4(shift + 4 * t.q), mu = ld4(mean + 4 * t.q), is = ld4(invstd + 4 * t.q);
    if constexpr (SRC == GS_POOL) {
      const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, P = N * Hc * Wc;
      PixIter it = pix_iter(t.p, t.pstep, Hc, Wc);
      for (int p = t.p; p < P; p += t.pstep, pix_next(it, Hc, Wc)) {
        float4 zz[4], g[4];
        const float4 m = mask ? mask4(mask, it.n, C, 4 * t.q) : make_float4(1.f, 1.f, 1.f, 1.f);
        const int valid = pool_cell4<TZ, TA>(src, z, ldz, it.n, it.y, it.x, H, W, t.q, sc, sh, mask != nullptr, m, zz, g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((valid >> j) & 1) {
            a1 = f4add(a1, g[j]);
            a2.x += g[j].x * (zz[j].x - mu.x) * is.x;
            a2.y += g[j].y * (zz[j].y - mu.y) * is.y;
            a2.z += g[j].z * (zz[j].z - mu.z) * is.z;
            a2.w += g[j].w * (zz[j].w - mu.w) * is.w;
          }
      }
    } else {
      const int P = N * H * W;
      PixIter it = pix_iter(t.p, t.pstep, H, W);
      for (int p = t.p; p < P; p += t.pstep, pix_next(it, H, W)) {
        const float4 v = ld4(z + (size_t)p * ldz + 4 * t.q);
        float d0 = 0.f, d1 = 0.f;
        const float4 g = relu_grad4<SRC, TZ, TA>(src, hl, mask, C, p, it, t.q, H, W, v, sc, sh, &d0, &d1);
        a1 = f4add(a1, g);
        a2.x += g.x * (v.x - mu.x) * is.x;
        a2.y += g.y * (v.y - mu.y) * is.y;
        a2.z += g.z * (v.z - mu.z) * is.z;
        a2.w += g.w * (v.w - mu.w) * is.w;
        if constexpr (SRC == GS_HEAD) {  // the head's input is this tensor's activation (no dropout on this path)
          const float4 av = bn_relu4(v, sc, sh);
          hw0.x = fmaf(d0, av.x, hw0.x);
          hw0.y = fmaf(d0, av.y, hw0.y);
          hw0.z = fmaf(d0, av.z, hw0.z);
          hw0.w = fmaf(d0, av.w, hw0.w);
          hw1.x = fmaf(d1, av.x, hw1.x);
          hw1.y = fmaf(d1, av.y, hw1.y);
          hw1.z = fmaf(d1, av.z, hw1.z);
          hw1.w = fmaf(d1, av.w, hw1.w);
          hb0 += d0;
          hb1 += d1;
        }
      }
    }
  }
  const float4 s1 = quad_block_sum(a1, t, red);
  const float4 s2 = quad_block_sum(a2, t, red);
  if (t.pl == 0 && t.q < Cv) {
    float* row = partial + (size_t)blockIdx.x * 2 * Cp;
    st4(row + 4 * t.q, s1);
    st4(row + Cp + 4 * t.q, s2);
  }
  if constexpr (SRC == GS_HEAD) {  // partial row as head_bwd_kernel writes it: [2][Cp] weight gradient, [2] bias gradient
    float* row = src.head.partial + (size_t)blockIdx.x * (2 * Cp + 2);
    const float4 w0 = quad_block_sum(hw0, t, red);
    const float4 w1 = quad_block_sum(hw1, t, red);
    const float4 sb = quad_block_sum(make_float4(hb0, hb1, 0.f, 0.f), t, red);
    if (t.pl == 0 && t.q < Cv) {
      st4(row + 4 * t.q, w0);
      st4(row + Cp + 4 * t.q, w1);
    }
    if (t.pl == 0 && t.q == 0) {
      row[2 * Cp] = sb.x;
      row[2 * Cp + 1] = sb.y;
    }
  }
}

// the fused sources exist for fp32 storage (TZ = TA = float) only
static int check_grad_src(const GradSrc& src, int dta, int dtz) {
  if (src.kind < GS_PLAIN || src.kind > GS_HEAD || (src.kind >= GS_POOL && (dta != ST_F32 || dtz != ST_F32)) ||
      (src.kind == GS_HEAD && src.head.Co != 2)) {
    set_error("BatchNorm backward: gradient source %d unsupported here", src.kind);
    return MIMO_ERR_INVALID;
  }
  return MIMO_OK;
}

int bnrelu_bwd_reduce_launch(const BnReluLayer& L, const GradSrc& src, const float* mask, float* partial, int* rows,
                             hipStream_t st) {
  MIMO_TRY(check_grad_src(src, L.dta, L.dtz));
  const int Cv = L.Cp / 4, N = L.N, H = L.H, W = L.W;
  const int64_t units = src.kind == GS_POOL ? (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) : (int64_t)N * H * W;  // cells / pixels
  // (the fused sources hold more registers: 4 / 5 waves per SIMD = one 1024-thread workgroup per CU, a single round)
  const dim3 grid = pq_grid(Cv, units, src.kind >= GS_POOL ? 256 : kBlocksBnReduce, kBnReduceThreads);
  *rows = grid.x;
#define REDUCE_LAUNCH(TZ, TA, SRC)                                                                                          \
  hipLaunchKernelGGL((bnrelu_bwd_reduce_kernel<TZ, TA, SRC>), grid, dim3(kBnReduceThreads), 0, st, src, (const TZ*)L.z, L.ldz, \
                     L.scale, L.shift, L.mean, L.invstd, mask, L.C, Cv, N, H, W, partial)
  if (src.kind == GS_POOL) {
    REDUCE_LAUNCH(float, float, GS_POOL);
  } else if (src.kind == GS_HEAD) {
    REDUCE_LAUNCH(float, float, GS_HEAD);
  } else if (src.kind == GS_PLAIN) {
    MIMO_ST_DISPATCH2(L.dtz, L.dta, TZ, TA, REDUCE_LAUNCH(TZ, TA, GS_PLAIN))
  } else {
    MIMO_ST_DISPATCH2(L.dtz, L.dta, TZ, TA, REDUCE_LAUNCH(TZ, TA, GS_FOLD))
  }
#undef REDUCE_LAUNCH
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// column sums + finalize in one launch: partial rows [rows][2][Cp] from bnrelu_bwd_reduce
__global__ __launch_bounds__(kColsumThreads) void bn_bwd_stats_kernel(const float* __restrict__ partial, int rows, int C,
                                                                      int Cp, double count, int training,
                                                                      float* __restrict__ c1, float* __restrict__ c2,
                                                                      float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                      float* __restrict__ dbias_zero, int* __restrict__ status) {
  __shared__ double red[2048];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  double s1, s2;
  grid_colsum2(partial, rows, (size_t)2 * Cp, c, Cp + c, c < Cp, true, red, &s1, &s2);
  if (c >= Cp || threadIdx.x >= 64) return;
  if (status && c < C && !(isfinite(s1) && isfinite(s2))) atomicOr(status, kStatusBwdStats);
  c1[c] = training ? (float)(s1 / count) : 0.f;
  c2[c] = training ? (float)(s2 / count) : 0.f;
  if (c < C) {
    if (dgamma) dgamma[c] = (float)s2;
    if (dbeta) dbeta[c] = (float)s1;
    // training-mode BatchNorm removes any per-channel shift of its input: the gradient of the convolution bias
    // in front of it is exactly zero (the reference's autograd produces rounding noise around zero)
    if (dbias_zero) dbias_zero[c] = 0.f;
  }
}

int bn_bwd_stats_launch(const float* partial, int rows, int C, int Cp, int64_t count, int training, float* c1, float* c2,
                        float* dgamma, float* dbeta, float* dbias_zero, int* status, hipStream_t st) {
  hipLaunchKernelGGL(bn_bwd_stats_kernel, dim3(ceil_div(Cp, 64)), dim3(kColsumThreads), 0, st, partial, rows, C, Cp, (double)count,
                     training, c1, c2, dgamma, dbeta, dbias_zero, status);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// Split storage of a gradient tensor for the bf16-pair MFMA kernels (data and weight gradient): per
// pixel, per 32-channel chunk, [hi: 32 bf16 | lo: 32 bf16] with v ~= hi + lo (a last partial chunk of r
// channels is [hi r | lo r]) — the same 4*Cp bytes as fp32, and one contiguous 128-byte line per
// (pixel, chunk), which is exactly the LDS row image of the data-gradient kernel.  The split is the one
// the convolution loaders used to do on every read (hi = RNE(v), lo = RNE(v - hi)).
typedef __bf16 bf16x4_ew __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_split4(float* base, size_t p, int Cp, int q, float4 r) {
  bf16x4_ew hi, lo;
  hi[0] = (__bf16)r.x;
  hi[1] = (__bf16)r.y;
  hi[2] = (__bf16)r.z;
  hi[3] = (__bf16)r.w;
  lo[0] = (__bf16)(r.x - (float)hi[0]);
  lo[1] = (__bf16)(r.y - (float)hi[1]);
  lo[2] = (__bf16)(r.z - (float)hi[2]);
  lo[3] = (__bf16)(r.w - (float)hi[3]);
  const int ch = 4 * q, chunk = ch >> 5, rc = min(32, Cp - 32 * chunk);
  unsigned char* d = reinterpret_cast<unsigned char*>(base) + p * (size_t)Cp * 4 + chunk * 128 + (ch & 31) * 2;
  *reinterpret_cast<bf16x4_ew*>(d) = hi;
  *reinterpret_cast<bf16x4_ew*>(d + 2 * rc) = lo;
}

// max over the workgroup of a non-negative per-thread value -> the workgroup's own slot of `slots` (a plain store, no
// atomic; one barrier at the end of the kernel).  Whoever needs the tensor's maximum reduces the slots (wg_dz_absmax,
// common.h).  Earlier versions kept ONE word per tensor: an atomic max per workgroup (+4 us per launch: ~1800 same-address
// atomics queue), then per wave behind a relaxed load of the word (+25 us: the loads queue too — 4.66 -> 5.25 ms per step
// at 4 images per GPU); per-wave slots cost the consumers 4 x the loads (profiles/r05/wgrad_two_mfma.txt item 5).
__device__ __forceinline__ void block_absmax_store(float* slots, float v) {
  __shared__ float wm[16];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = wm[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) m = fmaxf(m, wm[i]);
    slots[blockIdx.y * gridDim.x + blockIdx.x] = m;
  }
}
__device__ __forceinline__ float absmax4(float m, float4 r) {
  return fmaxf(fmaxf(m, fmaxf(fabsf(r.x), fabsf(r.y))), fmaxf(fabsf(r.z), fabsf(r.w)));
}

__global__ void split_pairs_kernel(const float* __restrict__ src, float* __restrict__ dst, int Cv, int64_t P,
                                   float* __restrict__ absmax) {
  const PQ t = pixquad(Cv);
  float amax = 0.f;
  if (t.active)
    for (int64_t p = t.p; p < P; p += t.pstep) {
      const float4 r = ld4(src + (size_t)p * 4 * Cv + 4 * t.q);
      st_split4(dst, (size_t)p, 4 * Cv, t.q, r);
      amax = absmax4(amax, r);
    }
  if (absmax) block_absmax_store(absmax, amax);
}

int split_pairs_launch(const float* src, float* dst, int64_t P, int Cp, hipStream_t st, float* absmax, int* absmax_n) {
  const dim3 grid = pq_grid(Cp / 4, P, 2048);
  if (absmax && (int)(grid.x * grid.y) > kDzMaxSlots) {
    set_error("split_pairs: %d x %d workgroups exceed the max |dz| slots", (int)grid.x, (int)grid.y);
    return MIMO_ERR_INVALID;
  }
  if (absmax_n) *absmax_n = (int)(grid.x * grid.y);
  hipLaunchKernelGGL(split_pairs_kernel, grid, dim3(256), 0, st, src, dst, Cp / 4, P, absmax);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// (plain / folded sources: held to 72 registers = 7 waves per SIMD, the occupancy round 3's grid scan found best — the
// max |dz| tracking of round 5 had pushed the folded instance to 74 and cost the class 7 %)
constexpr int kApplyMinWaves = 7;
template <typename TZ, typename TA, int SRC>
__global__ __launch_bounds__(256, (SRC == GS_PLAIN || SRC == GS_FOLD) ? kApplyMinWaves : 1) void bn_bwd_apply_kernel(const GradSrc src, const TZ* __restrict__ z, int ldz, const float* __restrict__ scale,
                                    const float* __restrict__ shift, const float* __restrict__ mean,
                                    const float* __restrict__ invstd, const float* __restrict__ mask, int C,
                                    const float* __restrict__ c1, const float* __restrict__ c2, int Cv, int N, int H,
                                    int W, TA* __restrict__ dz, int split_out, float* __restrict__ partial,
                                    float* __restrict__ absmax) {
  __shared__ float4 red[256];
  const PQ t = pixquad(Cv);
  const int Cp = 4 * Cv;
  float4 acc = f4zero();
  float amax = 0.f;  // max |dz| of this thread's elements (absmax != nullptr: the two-MFMA weight gradient scales dz by it)
  HeadLane hl = {};
  if constexpr (SRC == GS_HEAD) hl = head_lane(src.head, t.q, t.active);
  if (t.active) {
    const float4 sc = ld4(scale + 4 * t.q), sh = ld4(shift + 4 * t.q), mu = ld4(mean + 4 * t.q), is = ld4(invstd + 4 * t.q);
    const float4 k1 = ld4(c1 + 4 * t.q), k2 = ld4(c2 + 4 * t.q);
    auto emit = [&](int p, float4 g, float4 v) {
      float4 r;
      r.x = sc.x * (g.x - k1.x - (v.x - mu.x) * is.x * k2.x);
      r.y = sc.y * (g.y - k1.y - (v.y - mu.y) * is.y * k2.y);
      r.z = sc.z * (g.z - k1.z - (v.z - mu.z) * is.z * k2.z);
      r.w = sc.w * (g.w - k1.w - (v.w - mu.w) * is.w * k2.w);
      if (split_out)  // fp32 storage only: bf16 (hi, lo) pair records
        st_split4(reinterpret_cast<float*>(dz), p, Cp, t.q, r);
      else
        st4(dz + (size_t)p * Cp + 4 * t.q, r);
      acc = f4add(acc, r);
      amax = absmax4(amax, r);
    };
    if constexpr (SRC == GS_POOL) {
      const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, P = N * Hc * Wc;
      PixIter it = pix_iter(t.p, t.pstep, Hc, Wc);
      for (int p = t.p; p < P; p += t.pstep, pix_next(it, Hc, Wc)) {
        float4 zz[4], g[4];
        const float4 m = mask ? mask4(mask, it.n, C, 4 * t.q) : make_float4(1.f, 1.f, 1.f, 1.f);
        const int valid = pool_cell4<TZ, TA>(src, z, ldz, it.n, it.y, it.x, H, W, t.q, sc, sh, mask != nullptr, m, zz, g);
        const int p0 = (it.n * H + 2 * it.y) * W + 2 * it.x;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((valid >> j) & 1) emit(p0 + (j >> 1) * W + (j & 1), g[j], zz[j]);
      }
    } else {
      const int P = N * H * W;
      // back to front: the statistics pass in front of this one read the same two tensors front to back, so their LAST
      // part is what the last-level cache still holds
      if (t.p < P) {
        const int p_last = t.p + (P - 1 - t.p) / t.pstep * t.pstep;
        PixIter it = pix_iter(p_last, t.pstep, H, W);
        for (int p = p_last; p >= 0; p -= t.pstep, pix_prev(it, H, W)) {
          const float4 v = ld4(z + (size_t)p * ldz + 4 * t.q);
          float d0, d1;
          emit(p, relu_grad4<SRC, TZ, TA>(src, hl, mask, C, p, it, t.q, H, W, v, sc, sh, &d0, &d1), v);
        }
      }
    }
  }
  if (absmax) block_absmax_store(absmax, amax);
  if (!partial) return;  // training mode: the bias gradient is exactly zero, no column sums wanted
  const float4 s = quad_block_sum(acc, t, red);
  if (t.pl == 0 && t.q < Cv) st4(partial + (size_t)blockIdx.x * Cp + 4 * t.q, s);
}

int bn_bwd_apply_launch(const BnReluLayer& L, const GradSrc& src, const float* mask, const BnBwdApplyOut& out, hipStream_t st) {
  MIMO_TRY(check_grad_src(src, L.dta, L.dtz));
  const int Cv = L.Cp / 4, N = L.N, H = L.H, W = L.W;
  const int64_t units = src.kind == GS_POOL ? (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) : (int64_t)N * H * W;
  const dim3 grid = pq_grid(Cv, units, src.kind == GS_POOL ? 1024 : src.kind == GS_HEAD ? 1280 : kBlocksBnBwd);  // 4 / 5 / 7 per CU
  *out.rows = grid.x;
  if (out.absmax_n) *out.absmax_n = (int)(grid.x * grid.y);  // one slot per workgroup
  if (out.absmax && (int)(grid.x * grid.y) > kDzMaxSlots) {
    set_error("bn_bwd_apply: %d x %d workgroups exceed the max |dz| slots", (int)grid.x, (int)grid.y);
    return MIMO_ERR_INVALID;
  }
  if (out.split_out && L.dta != ST_F32) {
    set_error("bn_bwd_apply: pair-split dz exists for fp32 storage only");
    return MIMO_ERR_INVALID;
  }
  // `done`: recorded when THIS kernel completes, carried by the launch itself (hipExtLaunchKernelGGL stop event) — a separate
  // hipEventRecord behind the kernel costs the stream 2.9-5 us per hand-off (scripts/micro/event_cost.hip), this one ~1
#define APPLY_LAUNCH(TZ, TA, SRC)                                                                                                \
  hipExtLaunchKernelGGL((bn_bwd_apply_kernel<TZ, TA, SRC>), grid, dim3(256), 0, st, nullptr, out.done, 0, src, (const TZ*)L.z, L.ldz, \
                        L.scale, L.shift, L.mean, L.invstd, mask, L.C, out.c1, out.c2, Cv, N, H, W, (TA*)out.dz, out.split_out,  \
                        out.partial, out.absmax)
  if (src.kind == GS_POOL) {
    APPLY_LAUNCH(float, float, GS_POOL);
  } else if (src.kind == GS_HEAD) {
    APPLY_LAUNCH(float, float, GS_HEAD);
  } else if (src.kind == GS_PLAIN) {
    MIMO_ST_DISPATCH2(L.dtz, L.dta, TZ, TA, APPLY_LAUNCH(TZ, TA, GS_PLAIN))
  } else {
    MIMO_ST_DISPATCH2(L.dtz, L.dta, TZ, TA, APPLY_LAUNCH(TZ, TA, GS_FOLD))
  }
#undef APPLY_LAUNCH
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

}  // namespace mimo
