// Bandwidth-class kernels of the MIMO U-Net path for gfx950: everything that is not a 3x3
// convolution.  One float4 (4 channels of one pixel) per thread per step, fully coalesced
// NHWC accesses, per-thread register accumulation + LDS block reduction + per-workgroup
// partial rows (deterministic two-level reduction, no float atomics).
//
// This header is the device-side code the operator groups share; it is included by the ew_*.hip files only (the launch
// wrappers they define are declared in elementwise.h, the one host-visible header of the group):
//   ew_reduce.hip ...... rowsum, colsum_vec
//   ew_layout.hip ...... pack_input, unpack_dx, fold_image_grad, fold_image_grad_mc
//   ew_bn_fwd.hip ...... BatchNorm statistics -> scale / shift, BatchNorm + ReLU (+ MaxPool2d) forward
//   ew_resample.hip .... max pooling, bilinear up-sampling + concat (forward)
//   ew_dropout.hip ..... Philox dropout multipliers, the debug delay kernel
//   ew_bn_bwd.hip ...... pool_bwd, fold_slice, up_bwd; BatchNorm + ReLU backward (reduce, statistics, apply), split_pairs
//   ew_head_loss.hip ... 1x1 head and NLL losses, forward and backward
// Everything in here is internal to the translation unit that includes it (anonymous namespace).
//
// Reference operators replaced (paths inside the reference project):
//   BatchNorm2d / ReLU / Dropout2d ........ mimo/models/mimo_components/components.py:24-29
//   MaxPool2d(2) .......................... components.py:48
//   Upsample(bilinear, align_corners) + F.pad + cat ... components.py:78,110-119
//   OutConv 1x1 ........................... components.py:123-129
//   LaplaceNLL / GaussianNLL .............. mimo/losses.py:47-79,132-164
//   apply_input_transform gather .......... mimo/models/utils.py:38-48
#pragma once
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>

#include "elementwise.h"

namespace mimo {
namespace {

// ---------------------------------------------------------------------------------------
// thread mapping: 256 threads = QB channel-quads x PPI pixels; quad fixed per thread
// ---------------------------------------------------------------------------------------
struct PQ {
  int q;       // channel quad handled by this thread
  int ql, pl;  // position inside the workgroup
  int QB, PPI;
  int p, pstep;  // first pixel, pixel stride
  bool active;
};

// xcd_bands: workgroups are dealt round-robin to the 8 XCDs (each with a private L2); give every XCD one
// contiguous band of the pixels in flight, so that gathers which re-read neighbouring rows (bilinear
// backward: every gradient row feeds two input rows) find them in their own L2.
// T = threads per workgroup (256 everywhere but the BatchNorm-backward reduction, which runs 1024)
template <int T = 256>
__device__ __forceinline__ PQ pixquad(int Cv, bool xcd_bands = false) {
  PQ r;
  r.QB = Cv < T ? Cv : T;
  r.PPI = T / r.QB;
  r.ql = threadIdx.x % r.QB;
  r.pl = threadIdx.x / r.QB;
  r.q = blockIdx.y * r.QB + r.ql;
  r.active = r.pl < r.PPI && r.q < Cv;
  int bx = blockIdx.x;
  if (xcd_bands && (gridDim.x & 7) == 0) bx = (bx & 7) * (gridDim.x >> 3) + (bx >> 3);
  r.p = bx * r.PPI + r.pl;
  r.pstep = gridDim.x * r.PPI;
  return r;
}

// Grid caps of the grid-stride kernels, scanned per kernel on the cfg3 step (rocprofv3 kernel trace; 256 CUs):
// the two BatchNorm-backward passes run best with exactly the 7 workgroups per CU their registers allow resident
// (1024 -> 1792 blocks: reduce 1.92 -> 1.63 ms, apply 2.38 -> 2.21 ms per step; 2048 already spills into a second,
// partial round), BatchNorm + ReLU forward with 6 per CU, the 16-tap bilinear backward with many short
// workgroups (4096 -> 16384: 0.67 -> 0.55 ms), the rest at 4096-8192.
constexpr int kBlocksBnRelu = 1536, kBlocksBnBwd = 1792, kBlocksUpBwd = 16384, kBlocksPoolBwd = 8192;
// The BatchNorm-backward REDUCTION runs the same 7168 waves as 448 workgroups of 1024 threads: a quarter of the partial
// rows for the column-sum launch that follows (12.6 -> ~5 us, 24 times per step, at every batch size)
constexpr int kBnReduceThreads = 1024, kBlocksBnReduce = kBlocksBnBwd / 4;
// (Round 6 measured fewer, longer threads on the small tensors of a 4-image step — at least 2 / 4 / 8 pixels per thread, so
// that the 4-6 float4 of channel constants a thread loads are not most of its memory instructions: the BatchNorm-backward
// passes got SLOWER, 0.78 -> 0.80 / 0.91 / 1.10 ms per step; they want the threads.  profiles/r06/exp/ew_min_iters.txt)
static dim3 pq_grid(int Cv, int64_t P, int max_blocks = kEwMaxBlocks, int T = 256) {
  const int QB = Cv < T ? Cv : T;
  const int PPI = T / QB;
  int64_t gx = ceil_div64(P, PPI);
  if (gx > max_blocks) gx = max_blocks;
  if (gx < 1) gx = 1;
  return dim3((unsigned)gx, (unsigned)ceil_div(Cv, QB));
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// 16-bit storage (mimo_precision *_MIXED): four channels = one 8-byte access, arithmetic stays fp32
typedef __bf16 bf16x4_st __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4_st __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const __bf16* p) {
  const bf16x4_st v = *reinterpret_cast<const bf16x4_st*>(p);
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ void st4(__bf16* p, float4 v) {
  bf16x4_st r;
  r[0] = (__bf16)v.x;
  r[1] = (__bf16)v.y;
  r[2] = (__bf16)v.z;
  r[3] = (__bf16)v.w;
  *reinterpret_cast<bf16x4_st*>(p) = r;
}
__device__ __forceinline__ float4 ld4(const _Float16* p) {
  const f16x4_st v = *reinterpret_cast<const f16x4_st*>(p);
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ void st4(_Float16* p, float4 v) {
  f16x4_st r;
  r[0] = (_Float16)v.x;
  r[1] = (_Float16)v.y;
  r[2] = (_Float16)v.z;
  r[3] = (_Float16)v.w;
  *reinterpret_cast<f16x4_st*>(p) = r;
}
// Launch wrappers take untyped pointers plus a StoreType (elementwise.h); BODY sees the element type as T.
#define MIMO_ST_DISPATCH(DT, T, ...) \
  switch (DT) {                      \
    case ST_BF16: {                  \
      typedef __bf16 T;              \
      __VA_ARGS__;                   \
    } break;                         \
    case ST_F16: {                   \
      typedef _Float16 T;            \
      __VA_ARGS__;                   \
    } break;                         \
    default: {                       \
      typedef float T;               \
      __VA_ARGS__;                   \
    } break;                         \
  }
// (z type, activation type) pairs of the BatchNorm kernels: z is fp32 where the convolution that wrote it runs on the
// fp32 kernel family (the 2..4-channel image convolution) even in the 16-bit storage modes
#define MIMO_ST_DISPATCH2(DTZ, DTA, TZ, TA, ...) \
  if ((DTZ) == ST_F32) {                         \
    typedef float TZ;                            \
    MIMO_ST_DISPATCH(DTA, TA, __VA_ARGS__)       \
  } else if ((DTA) == ST_BF16) {                 \
    typedef __bf16 TZ;                           \
    typedef __bf16 TA;                           \
    __VA_ARGS__;                                 \
  } else {                                       \
    typedef _Float16 TZ;                         \
    typedef _Float16 TA;                         \
    __VA_ARGS__;                                 \
  }

__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4max(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// sum the accumulators of the threads that share a channel quad; result valid for pl == 0 (red: one float4 per thread).
// Fixed summation order (deterministic); two levels when many threads share a quad (the 1024-thread reduction).
__device__ __forceinline__ float4 quad_block_sum(float4 v, const PQ& t, float4* red) {
  __syncthreads();
  red[threadIdx.x] = t.active ? v : f4zero();
  __syncthreads();
  float4 s = f4zero();
  if (t.PPI <= 32) {
    if (t.pl == 0)
      for (int j = 0; j < t.PPI; ++j) s = f4add(s, red[j * t.QB + t.ql]);
    return s;
  }
  const bool lead = t.pl < 16 && t.pl < t.PPI;
  if (lead)
    for (int j = t.pl; j < t.PPI; j += 16) s = f4add(s, red[j * t.QB + t.ql]);
  __syncthreads();
  if (lead) red[threadIdx.x] = s;
  __syncthreads();
  s = f4zero();
  if (t.pl == 0)
    for (int j = 0; j < 16 && j < t.PPI; ++j) s = f4add(s, red[j * t.QB + t.ql]);
  return s;
}

// gradient on the reflect-padded domain folded back onto the image (transpose of reflect pad):
// pad row -1 lands on row 1, pad row H on row H-2 (same for columns).
template <typename T>
__device__ __forceinline__ float4 fold_read(const T* dxpad, int ldp, int n, int y, int x, int H, int W, int ch) {
  const T* base = dxpad + (size_t)n * (H + 2) * (W + 2) * ldp + ch;
  float4 s = ld4(base + ((size_t)(y + 1) * (W + 2) + (x + 1)) * ldp);  // interior pixels: this one load
  const bool ya = y == 1, yb = y == H - 2, xa = x == 1, xb = x == W - 2;
  if (ya | yb | xa | xb) {  // rows 1 / H-2 and columns 1 / W-2 also receive the reflected border
    const int ry[3] = {y, -1, H}, rx[3] = {x, -1, W};
    const bool vy[3] = {true, ya, yb}, vx[3] = {true, xa, xb};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (i + j > 0 && vy[i] && vx[j]) s = f4add(s, ld4(base + ((size_t)(ry[i] + 1) * (W + 2) + (rx[j] + 1)) * ldp));
  }
  return s;
}

// (n, y, x) of a pixel index that advances by a fixed stride: two integer divisions once per thread
// instead of two per visited pixel (they cost more VALU than the 48-64 bytes the pixel moves)
struct PixIter {
  int n, y, x, dn, dy, dx;
};
__device__ __forceinline__ PixIter pix_iter(int p0, int pstep, int H, int W) {
  PixIter it;
  const int HW = H * W;
  it.n = p0 / HW;
  int r = p0 - it.n * HW;
  it.y = r / W;
  it.x = r - it.y * W;
  it.dn = pstep / HW;
  r = pstep - it.dn * HW;
  it.dy = r / W;
  it.dx = r - it.dy * W;
  return it;
}
__device__ __forceinline__ void pix_next(PixIter& it, int H, int W) {
  it.x += it.dx;
  it.y += it.dy;
  it.n += it.dn;
  if (it.x >= W) {
    it.x -= W;
    ++it.y;
  }
  if (it.y >= H) {
    it.y -= H;
    ++it.n;
  }
}

__device__ __forceinline__ void pix_prev(PixIter& it, int H, int W) {
  it.x -= it.dx;
  it.y -= it.dy;
  it.n -= it.dn;
  if (it.x < 0) {
    it.x += W;
    --it.y;
  }
  if (it.y < 0) {
    it.y += H;
    --it.n;
  }
}

// ---------------------------------------------------------------------------------------
// column sums of per-workgroup partial rows (colsum_vec and the statistics kernels of BatchNorm forward / backward and of the
// head backward, each in its operator's file)
// ---------------------------------------------------------------------------------------
// ---- one-launch column sums (deterministic): one workgroup of 1024 threads = 64 columns x 16 row groups walks the
// fp32 partial rows of its 64 columns in double, eight independent loads in flight per thread, then runs the
// finalize arithmetic — one launch instead of the rowsum + finalize pair.  (Spreading the rows over several
// workgroups with a last-workgroup ticket was measured SLOWER, 24 vs 13 us: the device-scope fence it needs writes
// back / invalidates the whole L2 on this multi-XCD part.)  Every thread of the workgroup must call grid_colsum2; the
// totals are valid in its first 64 threads.
constexpr int kColsumThreads = 1024;

__device__ __forceinline__ void grid_colsum2(const float* __restrict__ partial, int rows, size_t stride, int col_a, int col_b,
                                             bool valid, bool two, double* red /*[2048]*/, double* ta, double* tb) {
  const int rg = threadIdx.x >> 6;
  double sa = 0.0, sb = 0.0;
  if (valid) {
    const float* pa = partial + col_a;
    const float* pb = partial + col_b;
    int r = rg;
    if (two) {
      for (; r + 48 < rows; r += 64) {
        float a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          a[k] = pa[(size_t)(r + 16 * k) * stride];
          b[k] = pb[(size_t)(r + 16 * k) * stride];
        }
        sa += ((double)a[0] + (double)a[1]) + ((double)a[2] + (double)a[3]);
        sb += ((double)b[0] + (double)b[1]) + ((double)b[2] + (double)b[3]);
      }
    } else {
      for (; r + 112 < rows; r += 128) {
        float a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = pa[(size_t)(r + 16 * k) * stride];
        sa += (((double)a[0] + (double)a[1]) + ((double)a[2] + (double)a[3])) +
              (((double)a[4] + (double)a[5]) + ((double)a[6] + (double)a[7]));
      }
    }
    for (; r < rows; r += 16) {
      sa += (double)pa[(size_t)r * stride];
      if (two) sb += (double)pb[(size_t)r * stride];
    }
  }
  __syncthreads();
  red[threadIdx.x] = sa;
  red[1024 + threadIdx.x] = sb;
  __syncthreads();
  const int cl = threadIdx.x & 63;
  double a = 0.0, b = 0.0;
  if (threadIdx.x < 64) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      a += red[k * 64 + cl];
      b += red[1024 + k * 64 + cl];
    }
  }
  *ta = a;
  *tb = b;
}

// ---------------------------------------------------------------------------------------
// arithmetic that one operator restates from another (the forward of one, the backward of another): defined once
// ---------------------------------------------------------------------------------------
// Dropout2d multipliers [N][C] of channels c0 .. c0 + 3 of sample n (pad channels: 0)
__device__ __forceinline__ float4 mask4(const float* mask, int n, int C, int c0) {
  float4 m;
  const float* mp = mask + (size_t)n * C;
  m.x = c0 + 0 < C ? mp[c0 + 0] : 0.f;
  m.y = c0 + 1 < C ? mp[c0 + 1] : 0.f;
  m.z = c0 + 2 < C ? mp[c0 + 2] : 0.f;
  m.w = c0 + 3 < C ? mp[c0 + 3] : 0.f;
  return m;
}

// relu(fma(z, scale, shift)): bn_relu_fwd_kernel's arithmetic, for the readers that apply their producer's BatchNorm + ReLU
// on the way in (up-sampling, 1x1 head, GS_HEAD)
__device__ __forceinline__ float4 bn_relu4(float4 v, float4 sc, float4 sh) {
  return make_float4(fmaxf(fmaf(v.x, sc.x, sh.x), 0.f), fmaxf(fmaf(v.y, sc.y, sh.y), 0.f), fmaxf(fmaf(v.z, sc.z, sh.z), 0.f),
                     fmaxf(fmaf(v.w, sc.w, sh.w), 0.f));
}

// source index / weight of bilinear align_corners=True interpolation, as torch computes it in
// fp32: src = dst * (in-1)/(out-1); i0 = (int)src; lambda = src - i0; i1 = i0 + (i0 < in-1)
struct Lerp {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lerp lerp_src(int dst, int in, int out) {
  // no fma contraction in here: torch rounds src = scale * dst to fp32 and then subtracts i0 (checked
  // against F.interpolate on the CPU); an fma keeps the exact product and moves lambda by up to an ulp of
  // src (4e-6 at src ~ 50, 2e-6 relative on the output) — and whether the compiler contracts depends on
  // the surrounding code, so it is pinned here
#pragma clang fp contract(off)
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const float src = scale * (float)dst;
  Lerp r;
  r.i0 = min((int)src, in - 1);
  r.l1 = fminf(fmaxf(src - (float)r.i0, 0.f), 1.f);
  r.l0 = 1.f - r.l1;
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  return r;
}

// weight with which output index o (of an x2 align_corners upsample of `in` samples) reads input i
__device__ __forceinline__ float lerp_weight(int o, int i, int in) {
  const Lerp l = lerp_src(o, in, 2 * in);
  return (l.i0 == i ? l.l0 : 0.f) + (l.i1 == i ? l.l1 : 0.f);
}

// value and gradient of the element-wise NLL.  The clamp acts on the value only
// (losses.py:153-155 clamps in place under no_grad), so d/dlog keeps the unclamped exp.
__device__ __forceinline__ float nll_value(int kind, float d, float lp, float eps_min, float eps_max) {
  const float sc = fminf(fmaxf(expf(lp), eps_min), eps_max);
  return kind == MIMO_LOSS_LAPLACE_NLL ? logf(sc) + fabsf(d) / sc : logf(sc) + d * d / sc;
}
__device__ __forceinline__ void nll_grad(int kind, float d, float lp, float eps_min, float eps_max, float* gmu, float* glp) {
  const float e = expf(lp);
  const float sc = fminf(fmaxf(e, eps_min), eps_max);
  if (kind == MIMO_LOSS_LAPLACE_NLL) {
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    *gmu = sgn / sc;
    *glp = (1.f / sc - fabsf(d) / (sc * sc)) * e;
  } else {
    *gmu = 2.f * d / sc;
    *glp = (1.f / sc - d * d / (sc * sc)) * e;
  }
}

// The 1x1 head's per-pixel logit gradient, formed by head_bwd_kernel's arithmetic where the BatchNorm backward of the
// decoder's last convolution takes its arriving gradient straight from the logits and labels (GS_HEAD, elementwise.h)
struct HeadLane {  // GS_HEAD per-thread constants: this channel quad's 1x1 weights, dloss[s] / count
  float4 w0, w1;
  float coef;
};
__device__ __forceinline__ HeadLane head_lane(const HeadGrad& h, int q, bool active) {
  HeadLane l;
  l.w0 = l.w1 = f4zero();
  l.coef = h.dloss ? h.dloss[h.s] * h.inv_count : 0.f;
  if (active) {
    const int c0 = 4 * q;
    float* a0 = reinterpret_cast<float*>(&l.w0);
    float* a1 = reinterpret_cast<float*>(&l.w1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a0[j] = c0 + j < h.C ? h.w[c0 + j] : 0.f;
      a1[j] = c0 + j < h.C ? h.w[h.C + c0 + j] : 0.f;
    }
  }
  return l;
}
// dlogit of pixel p (Co == 2: mean, log-scale), head_bwd_kernel's arithmetic
__device__ __forceinline__ void head_dlogit(const HeadGrad& h, const HeadLane& l, int p, float* d0, float* d1) {
  const int n = p / h.HW;
  const int yx = p - n * h.HW;
  const int64_t obase = (((int64_t)n * h.S + h.s) * 2) * h.HW + yx;
  float a = h.dout ? h.dout[obase] : 0.f, b = h.dout ? h.dout[obase + h.HW] : 0.f;
  if (h.dloss) {
    const int64_t src = h.perm ? h.perm[(int64_t)h.s * h.N + n] : n;
    const float mk = h.mask ? h.mask[src * h.HW + yx] : 1.f;
    const float mu = h.out[obase], lp = h.out[obase + h.HW], y = h.label[src * h.HW + yx];
    float gm, gl;
    nll_grad(h.kind, mu - y, lp, h.eps_min, h.eps_max, &gm, &gl);
    a += l.coef * mk * gm;
    b += l.coef * mk * gl;
  }
  *d0 = a;
  *d1 = b;
}

}  // namespace
}  // namespace mimo
