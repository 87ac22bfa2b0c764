// MaxPool2d(2) and bilinear x2 up-sampling + zero pad + concat, forward (their backward gathers: ew_bn_bwd.hip).
#include "ew_device.h"

namespace mimo {

// ---------------------------------------------------------------------------------------
// max pooling 2x2 (floor) and bilinear x2 upsample + zero pad + concat
// ---------------------------------------------------------------------------------------

template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ a, int lda, int N, int H, int W, int Cv,
                                   T* __restrict__ out, int ldo) {
  const PQ t = pixquad(Cv);
  if (!t.active) return;
  const int Ho = H / 2, Wo = W / 2;
  const int P = N * Ho * Wo;
  PixIter it = pix_iter(t.p, t.pstep, Ho, Wo);
  for (int p = t.p; p < P; p += t.pstep, pix_next(it, Ho, Wo)) {
    const int n = it.n, oy = it.y, ox = it.x;
    const T* src = a + (((size_t)n * H + 2 * oy) * W + 2 * ox) * lda + 4 * t.q;
    const float4 v = f4max(f4max(ld4(src), ld4(src + lda)), f4max(ld4(src + (size_t)W * lda), ld4(src + (size_t)(W + 1) * lda)));
    st4(out + (size_t)p * ldo + 4 * t.q, v);
  }
}

int maxpool_fwd_launch(const void* a, int dt, int lda, int N, int H, int W, int Cp, void* out, int ldo, hipStream_t st) {
  const int Cv = Cp / 4;
  const int64_t P = (int64_t)N * (H / 2) * (W / 2);
  MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL(maxpool_fwd_kernel<T>, pq_grid(Cv, P, 4096), dim3(256), 0, st, (const T*)a, lda, N, H,
                                             W, Cv, (T*)out, ldo));
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// lo_scale != nullptr: `low` is the pre-activation tensor of the producing convolution and its BatchNorm + ReLU is applied to
// the four sources of every output pixel here (relu(fma(z, scale, shift)), bn_relu_fwd_kernel's arithmetic, then the same
// interpolation): the activated low-resolution tensor is never written (round 4)

__device__ __forceinline__ float4 sel3(int a, float4 x0, float4 x1, float4 x2) { return a == 1 ? x1 : (a == 0 ? x0 : x2); }
__device__ __forceinline__ float4 blend2(float w0, float4 a, float w1, float4 b) {
  // no fma contraction (here and in the per-pixel kernel's blend): both kernels then round every product and sum alike
#pragma clang fp contract(off)
  return make_float4(w0 * a.x + w1 * b.x, w0 * a.y + w1 * b.y, w0 * a.z + w1 * b.z, w0 * a.w + w1 * b.w);
}
template <typename T>
__global__ void upcat_fwd_kernel(const T* __restrict__ skip, int lds, int csv, const T* __restrict__ low,
                                 int ldl, int clv, int N, int H, int W, int h, int w, int padT, int padL,
                                 T* __restrict__ out, const float* __restrict__ lo_scale,
                                 const float* __restrict__ lo_shift) {
  const int Cv = csv + clv;
  // skip == nullptr: the skip tensor already lives in channels [0, 4*csv) of `out` (its producer writes it
  // there); only the up-sampled part is written, and the threads are mapped over those channels alone
  PQ t = pixquad(skip ? Cv : clv);
  if (!t.active) return;
  if (!skip) t.q += csv;
  const int ldo = 4 * Cv;
  const int P = N * H * W;
  float4 lsc = f4zero(), lsh = f4zero();
  if (lo_scale && t.q >= csv) {
    lsc = ld4(lo_scale + 4 * (t.q - csv));
    lsh = ld4(lo_shift + 4 * (t.q - csv));
  }
  PixIter it = pix_iter(t.p, t.pstep, H, W);
  for (int p = t.p; p < P; p += t.pstep, pix_next(it, H, W)) {
    float4 v;
    if (t.q < csv) {
      v = ld4(skip + (size_t)p * lds + 4 * t.q);
    } else {
      const int n = it.n, y = it.y, x = it.x;
      const int uy = y - padT, ux = x - padL;
      v = f4zero();
      if (uy >= 0 && uy < 2 * h && ux >= 0 && ux < 2 * w) {
        const Lerp ly = lerp_src(uy, h, 2 * h), lx = lerp_src(ux, w, 2 * w);
        const T* b = low + (size_t)n * h * w * ldl + 4 * (t.q - csv);
        float4 v00 = ld4(b + ((size_t)ly.i0 * w + lx.i0) * ldl), v01 = ld4(b + ((size_t)ly.i0 * w + lx.i1) * ldl);
        float4 v10 = ld4(b + ((size_t)ly.i1 * w + lx.i0) * ldl), v11 = ld4(b + ((size_t)ly.i1 * w + lx.i1) * ldl);
        if (lo_scale) {
          v00 = bn_relu4(v00, lsc, lsh);
          v01 = bn_relu4(v01, lsc, lsh);
          v10 = bn_relu4(v10, lsc, lsh);
          v11 = bn_relu4(v11, lsc, lsh);
        }
        v = blend2(ly.l0, blend2(lx.l0, v00, lx.l1, v01), ly.l1, blend2(lx.l0, v10, lx.l1, v11));
      }
    }
    st4(out + (size_t)p * ldo + 4 * t.q, v);
  }
}

// The common geometry — skip tensor already in place (skip == nullptr), output exactly twice the low-resolution size — with
// one thread per 2 x 2 OUTPUT block and channel quad (round 5): the four pixels of a block read sources
// from the 3 x 3 low-resolution neighbourhood of their block only (x2 align_corners: output 2k reads rows k-1 / k, output
// 2k + 1 rows k / k + 1), so 9 loads (and 9 BatchNorm + ReLU evaluations) serve 4 outputs instead of 16.  Which of the three
// rows / columns an output takes is read off the same lerp_src() results as in the per-pixel kernel, and the blend keeps its
// association — horizontal pairs first, then the vertical pair: the same values.
template <typename T>
__global__ __launch_bounds__(256) void upcat_fwd2x2_kernel(int csv, const T* __restrict__ low, int ldl, int clv, int N, int h, int w,
                                    T* __restrict__ out, const float* __restrict__ lo_scale,
                                    const float* __restrict__ lo_shift) {
  PQ t = pixquad(clv);
  if (!t.active) return;
  const int ldo = 4 * (csv + clv), H = 2 * h, W = 2 * w;
  const int P = N * h * w;
  float4 lsc = f4zero(), lsh = f4zero();
  if (lo_scale) {
    lsc = ld4(lo_scale + 4 * t.q);
    lsh = ld4(lo_shift + 4 * t.q);
  }
  PixIter it = pix_iter(t.p, t.pstep, h, w);
  for (int p = t.p; p < P; p += t.pstep, pix_next(it, h, w)) {
    const int n = it.n, by = it.y, bx = it.x;
    const int rr[3] = {max(by - 1, 0), by, min(by + 1, h - 1)}, cc[3] = {max(bx - 1, 0), bx, min(bx + 1, w - 1)};
    const T* b = low + (size_t)n * h * w * ldl + 4 * t.q;
    float4 v[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[a][c] = ld4(b + ((size_t)rr[a] * w + cc[c]) * ldl);
    if (lo_scale) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[a][c] = bn_relu4(v[a][c], lsc, lsh);
    }
    const Lerp ly[2] = {lerp_src(2 * by, h, H), lerp_src(2 * by + 1, h, H)};
    const Lerp lx[2] = {lerp_src(2 * bx, w, W), lerp_src(2 * bx + 1, w, W)};
    // horizontal pairs of every source row, for both output columns
    float4 hx[3][2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j0 = lx[e].i0 - (bx - 1), j1 = lx[e].i1 - (bx - 1);
#pragma unroll
      for (int a = 0; a < 3; ++a)
        hx[a][e] = blend2(lx[e].l0, sel3(j0, v[a][0], v[a][1], v[a][2]), lx[e].l1, sel3(j1, v[a][0], v[a][1], v[a][2]));
    }
    T* o = out + ((size_t)(n * H + 2 * by) * W + 2 * bx) * ldo + 4 * (csv + t.q);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int a0 = ly[d].i0 - (by - 1), a1 = ly[d].i1 - (by - 1);
#pragma unroll
      for (int e = 0; e < 2; ++e)
        st4(o + ((size_t)d * W + e) * ldo,
            blend2(ly[d].l0, sel3(a0, hx[0][e], hx[1][e], hx[2][e]), ly[d].l1, sel3(a1, hx[0][e], hx[1][e], hx[2][e])));
    }
  }
}

int upcat_fwd_launch(const void* skip, int dt, int lds, int csp, const void* low, int ldl, int clp, int N, int H, int W,
                     int h, int w, void* out, hipStream_t st, const float* lo_scale, const float* lo_shift) {
  const int Cv = (csp + clp) / 4;
  const int padT = (H - 2 * h) / 2, padL = (W - 2 * w) / 2;  // F.pad(diff//2, diff - diff//2), components.py:110-115
  if (H < 2 * h || W < 2 * w) {
    set_error("upcat: skip smaller than upsampled input");
    return MIMO_ERR_INVALID;
  }
  if (!skip && H == 2 * h && W == 2 * w) {
    MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL(upcat_fwd2x2_kernel<T>, pq_grid(clp / 4, (int64_t)N * h * w, 4096), dim3(256), 0, st,
                                               csp / 4, (const T*)low, ldl, clp / 4, N, h, w, (T*)out, lo_scale, lo_shift));
    MIMO_KERNEL_CHECK();
    return MIMO_OK;
  }
  MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL(upcat_fwd_kernel<T>, pq_grid(skip ? Cv : clp / 4, (int64_t)N * H * W, 4096), dim3(256), 0,
                                             st, (const T*)skip, lds, csp / 4, (const T*)low, ldl, clp / 4, N, H, W, h, w, padT, padL,
                                             (T*)out, lo_scale, lo_shift));
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

}  // namespace mimo
