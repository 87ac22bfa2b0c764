// Proper scoring rules of the ensemble's mixture predictive on the device (gfx950): per pixel the S members' (mu_s, p2_s)
// and the label go in, the probability integral transform, the negative log-likelihood and the CRPS of the equal-weight
// mixture of the S member densities come out; nothing is written but three optional maps and a few counters.
//
//   mimo_score_accumulate   one pass per batch: 8 S + 4 (+ 4 with a mask) bytes in per pixel, each read once; the
//                           S (S + 1) / 2 pair terms of the CRPS from registers (S <= 4, compile-time member counts) or
//                           from a member-major LDS tile of 256 pixels (S <= 64)
//   mimo_score_finalize     observed share below each threshold, the three counts and the three means, on the device
//
// Member scale as the loss trains it: theta = clamp(exp(p2), eps_min, eps_max); Laplace b = theta, Gaussian sigma^2 = theta.
// Means and labels are NOT clipped.  With d = y - mu:
//   PIT   u = mean_s F_s(y)      Laplace d < 0 ? exp(d / b) / 2 : 1 - exp(-d / b) / 2;   Gaussian erfc(-d / (sigma sqrt 2)) / 2
//   NLL   -log mean_s f_s(y)     the full density, by a running-maximum log-sum-exp (finite when every exp underflows),
//                                in double from the unrounded scale
//   CRPS  mean_s a_s - (sum_i c_ii + 2 sum_{i<j} c_ij) / (2 S^2),  a_s = E|X_s - y|,  c_ij = E|X_i - X_j'|
//         Gaussian (Grimit et al. 2006): A(m, s) = 2 s phi(m / s) + m erf(m / (s sqrt 2)); a = A(d, sigma),
//                   c_ij = A(mu_i - mu_j, sqrt(sigma_i^2 + sigma_j^2)), c_ii = 2 sigma / sqrt(pi)
//         Laplace:  a = |d| + b exp(-|d| / b);  c_ii = 3 b / 2;  with D = |mu_i - mu_j|, b_i <= b_j and
//                   x = D (b_i - b_j) / (b_i b_j) <= 0:
//                   c_ij = D + exp(-D / b_i) (b_i^2 + b_i b_j + b_j^2) / (b_i + b_j)
//                            + exp(-D / b_j) b_j^2 D / (b_i (b_i + b_j)) expm1(x) / x            (expm1(x) / x := 1 at x = 0)
//                   — the quotient (b_i^3 e^{-D/b_i} - b_j^3 e^{-D/b_j}) / (b_i^2 - b_j^2) without its cancellation: every
//                   term is positive at any pair of scales.
// Each term of the PIT and of the CRPS is fp32; the sums over members and pairs are carried in double and rounded once.
//
// A pixel is skipped when mask == 0 (n_masked) or when any of its 2 S + 1 inputs is not finite (n_nonfinite): NaN in
// every requested map, no sum, no bin.  The PIT bin is taken from the fp32 value the map gets, the sums add the fp32
// values the maps get: the counters are functions of the maps whether or not the maps are written.
//
// Sums are doubles in a FIXED order (thread -> workgroup tree -> partial row -> fold over the rows), counts are integer
// atomics in LDS: the same sequence of calls gives the same bits.
//
// The workspace, the tally of a scored pixel, the workgroup prologue / epilogue and the fold are score_common.h's, shared
// with the evidential model's Student-t scorer (score_evidential.hip).
#include "score_common.h"

#include <algorithm>
#include <cmath>

namespace mimo {
namespace score {

constexpr int kMaxS = 64;        // members
constexpr int kRegS = 4;         // ... up to which the pair loop runs from registers
constexpr int kTile = 256;       // pixels of an LDS tile = threads of a workgroup

struct Args {
  const float *p1, *p2, *label, *mask, *pk;
  float *pit, *nll, *crps;
  int B, S, C, channel, MC, K;
  int64_t hw;
  double log_lo, log_hi;  // log eps_min, log eps_max
  u64* part;
};

constexpr float kRsqrt2 =0.70710678118654752f;     // 1 / sqrt 2
constexpr float kRsqrt2Pi = 0.39894228040143268f;   // 1 / sqrt(2 pi)
constexpr float kRsqrtPi = 0.56418958354775629f;    // 1 / sqrt pi
constexpr double kHalfLog2Pi = 0.91893853320467274178;  // log(2 pi) / 2
constexpr double kLog2 = 0.69314718055994530942;

// A(m, s) = E|N(m, s^2)|
__device__ __forceinline__ float gauss_abs_mean(float m, float s) {
  const float z = m / s;
  return 2.f * s * (kRsqrt2Pi * expf(-0.5f * z * z)) + m * erff(z * kRsqrt2);
}

// one member at d = y - mu with scale sc (Laplace b; Gaussian sigma^2): F(y), E|X - y|, E|X - X'|
template <int KIND>
__device__ __forceinline__ void member_terms(float d, float sc, float& F, float& a, float& diag) {
  if (KIND == 0) {
    const float ad = fabsf(d), r = ad / sc, e = expf(-r);
    F = d < 0.f ? 0.5f * e : 1.f - 0.5f * e;
    a = ad + sc * e;
    diag = 1.5f * sc;
  } else {
    const float sd = sqrtf(sc), z = d / sd;
    F = 0.5f * erfcf(-z * kRsqrt2);
    a = gauss_abs_mean(d, sd);
    diag = 2.f * sd * kRsqrtPi;
  }
}

// c_ij = E|X_i - X_j'| of two members
template <int KIND>
__device__ __forceinline__ float pair_term(float mi, float si, float mj, float sj) {
  const float D = fabsf(mi - mj);
  if (KIND == 0) {
    const float bi = fminf(si, sj), bj = fmaxf(si, sj), sum = bi + bj;
    const float x = D * (bi - bj) / (bi * bj);
    const float g = x == 0.f ? 1.f : expm1f(x) / x;
    const float t1 = expf(-D / bi) * ((bi * bi + bi * bj + bj * bj) / sum);
    // left to right from the exponential: once it has underflowed the term is 0 whatever the other factors are
    const float t2 = expf(-D / bj) * (bj / sum) * (bj / bi) * D * g;
    return D + t1 + t2;
  } else {
    return gauss_abs_mean(D, sqrtf(si + sj));
  }
}

// registers: NS compile-time members
template <int NS>
struct RegMembers {
  float m[NS], s[NS];
  __device__ __forceinline__ float mu(int i) const { return m[i]; }
  __device__ __forceinline__ float sc(int i) const { return s[i]; }
  __device__ __forceinline__ void set_sc(int i, float v) { s[i] = v; }
};

// one column of the member-major LDS tile: member i of this lane's pixel is kTile floats on
struct LdsMembers {
  const float* m;
  float* s;
  __device__ __forceinline__ float mu(int i) const { return m[i * kTile]; }
  __device__ __forceinline__ float sc(int i) const { return s[i * kTile]; }
  __device__ __forceinline__ void set_sc(int i, float v) { s[i * kTile] = v; }
};

// On entry mem.sc(i) is the member's raw p2; the first loop leaves the scale theta_i there for the pair loop.
// The log-density is carried in double from the unrounded scale: log f is a difference of terms of size |d| / b and log b,
// which an fp32 ulp of either moves by many ulp of a small result; 2 S double exponentials and one logarithm per pixel.
// NS > 0: the member count (loops fully unrolled); NS == 0: S at run time.  log_lo / log_hi: log eps_min / log eps_max.
template <int KIND, int NS, class Mem>
__device__ __forceinline__ void score_pixel(Mem& mem, int S_rt, float y, double log_lo, double log_hi, float& pit, float& nll,
                                            float& crps) {
  const int S = NS ? NS : S_rt;
  constexpr int U = NS ? NS : 1;  // a compile-time member count unrolls fully
  double sF = 0.0, sA = 0.0, sE = 0.0, sC = 0.0, sD = 0.0;
  double mx = -(double)INFINITY;
#pragma unroll U
  for (int i = 0; i < S; ++i) {
    const float mu = mem.mu(i);
    const double pc = fmin(fmax((double)mem.sc(i), log_lo), log_hi), th = exp(pc), dd = (double)y - (double)mu;
    const float sc = (float)th;  // clamp(exp(p2), eps_min, eps_max), correctly rounded
    mem.set_sc(i, sc);
    const double lf = KIND == 0 ? -fabs(dd) / th - (kLog2 + pc) : -0.5 * dd * dd / th - 0.5 * pc - kHalfLog2Pi;
    // running maximum: sE = sum of exp(lf - mx); the one exponential is of -|lf - mx| (0 on the first member: mx = -inf)
    const double e = exp(-fabs(lf - mx));
    sE = lf > mx ? sE * e + 1.0 : sE + e;
    mx = fmax(mx, lf);
    float F, a, diag;
    member_terms<KIND>(y - mu, sc, F, a, diag);
    sF += (double)F;
    sA += (double)a;
    sD += (double)diag;
  }
#pragma unroll U
  for (int i = 0; i < S; ++i) {
    const float mi = mem.mu(i), si = mem.sc(i);
#pragma unroll U
    for (int j = i + 1; j < S; ++j) sC += (double)pair_term<KIND>(mi, si, mem.mu(j), mem.sc(j));
  }
  const double inv = 1.0 / (double)S;
  pit = (float)(sF * inv);
  nll = (float)-(mx + log(sE * inv));
  crps = (float)(sA * inv - (2.0 * sC + sD) * (0.5 * inv * inv));
}

// Registers.  VEC: hw % 4 == 0 and every pointer 16-byte aligned -> a float4 of pixels per thread per step (2 S + 1 (+ 1)
// 16-byte loads), scored one after another; otherwise one pixel per thread with scalar loads.
template <int KIND, int NS, bool VEC>
__global__ __launch_bounds__(256) void score_reg_kernel(Args a) {
  __shared__ float zt[kMaxK + 1];
  __shared__ u32 bins[4 * (kBins + 3)];
  __shared__ double red[3 * 256];
  __shared__ u32 redn[3 * 256];
  constexpr int PPT = VEC ? 4 : 1;
  const int tid = threadIdx.x, wave = tid >> 6;
  block_prologue(a, zt, bins);
  const int64_t ipi = a.hw / PPT, items = (int64_t)a.B * ipi;  // VEC: hw % 4 == 0
  const int64_t mstride = (int64_t)a.C * a.hw;
  const int mch = a.MC == 1 ? 0 : a.channel;
  const float nanv = __uint_as_float(0x7FC00000u);
  Tally t;
  for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < items; q += (int64_t)gridDim.x * 256) {
    const int64_t b = q / ipi, p0 = (q - b * ipi) * PPT;
    const int64_t src = ((int64_t)b * a.S * a.C + a.channel) * a.hw + p0, lsrc = (b * a.C + a.channel) * a.hw + p0;
    const int64_t msrc = (b * a.MC + mch) * a.hw + p0, dst = b * a.hw + p0;
    float4 m4[NS], s4[NS], y4, k4 = make_float4(1.f, 1.f, 1.f, 1.f);
    if (VEC) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        m4[s] = *(const float4*)(a.p1 + src + s * mstride);
        s4[s] = *(const float4*)(a.p2 + src + s * mstride);
      }
      y4 = *(const float4*)(a.label + lsrc);
      if (a.mask) k4 = *(const float4*)(a.mask + msrc);
    } else {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        m4[s].x = a.p1[src + s * mstride];
        s4[s].x = a.p2[src + s * mstride];
      }
      y4.x = a.label[lsrc];
      if (a.mask) k4.x = a.mask[msrc];
    }
    float4 o_pit = make_float4(nanv, nanv, nanv, nanv), o_nll = o_pit, o_crps = o_pit;
#pragma unroll 1
    for (int k = 0; k < PPT; ++k) {
      if (a.mask && pick(k4, k) == 0.f) {
        ++t.nm;
        continue;
      }
      const float y = pick(y4, k);
      RegMembers<NS> mem;
      bool fin = isfinite(y);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const float p = pick(s4[s], k);
        mem.m[s] = pick(m4[s], k);
        mem.s[s] = p;
        fin = fin && isfinite(mem.m[s]) && isfinite(p);
      }
      if (!fin) {
        ++t.nf;
        continue;
      }
      float pit, nll, crps;
      score_pixel<KIND, NS>(mem, NS, y, a.log_lo, a.log_hi, pit, nll, crps);
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
  block_epilogue(a, t, bins, red, redn);
}

// LDS.  A workgroup stages the S x 256 member values of 256 consecutive pixels of one image member-major (tile[.][s][p]:
// consecutive lanes on consecutive banks, for the 16-byte stores of the staging and for the 4-byte reads of the pair loop),
// then each thread scores its own column.  MS: the tile's member capacity, MS >= S; 2 KiB of LDS per member.
template <int KIND, int MS, bool VEC>
__global__ __launch_bounds__(256) void score_lds_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) float tile[2][MS][kTile];
  __shared__ float zt[kMaxK + 1];
  __shared__ u32 bins[4 * (kBins + 3)];
  static_assert(sizeof(float) * 2 * MS * kTile >= 3 * 256 * (sizeof(double) + sizeof(u32)), "the tile doubles as the reduction scratch");
  const int tid = threadIdx.x, wave = tid >> 6;
  block_prologue(a, zt, bins);
  const int S = a.S;
  const int64_t tpi = (a.hw + kTile - 1) / kTile, tiles = (int64_t)a.B * tpi;
  const int64_t mstride = (int64_t)a.C * a.hw;
  const int mch = a.MC == 1 ? 0 : a.channel;
  const float nanv = __uint_as_float(0x7FC00000u);
  Tally t;
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t b = ti / tpi, p0 = (ti - b * tpi) * kTile;
    const int npx = (int)(a.hw - p0 < kTile ? a.hw - p0 : kTile);
    const int64_t src = ((int64_t)b * S * a.C + a.channel) * a.hw + p0;
    __syncthreads();  // the columns of the previous tile have been read
    if (VEC) {        // npx % 4 == 0
      for (int idx = tid; idx < S * (kTile / 4); idx += 256) {
        const int s = idx >> 6, q4 = (idx & 63) << 2;
        if (q4 < npx) {
          *(float4*)&tile[0][s][q4] = *(const float4*)(a.p1 + src + s * mstride + q4);
          *(float4*)&tile[1][s][q4] = *(const float4*)(a.p2 + src + s * mstride + q4);
        }
      }
    } else if (tid < npx) {
      for (int s = 0; s < S; ++s) {
        tile[0][s][tid] = a.p1[src + s * mstride + tid];
        tile[1][s][tid] = a.p2[src + s * mstride + tid];
      }
    }
    __syncthreads();
    if (tid < npx) {
      const int64_t p = p0 + tid;
      float pit = nanv, nll = nanv, crps = nanv;
      if (a.mask && a.mask[(b * a.MC + mch) * a.hw + p] == 0.f) {
        ++t.nm;
      } else {
        const float y = a.label[(b * a.C + a.channel) * a.hw + p];
        bool fin = isfinite(y);
        for (int s = 0; s < S; ++s) fin = fin && isfinite(tile[0][s][tid]) && isfinite(tile[1][s][tid]);
        if (!fin) {
          ++t.nf;
        } else {
          LdsMembers mem{&tile[0][0][tid], &tile[1][0][tid]};  // the raw p2 of this column becomes the scale, in place
          score_pixel<KIND, 0>(mem, S, y, a.log_lo, a.log_hi, pit, nll, crps);
          tally_pixel(pit, nll, crps, zt, a.K, bins + wave * (kBins + 3), t);
        }
      }
      const int64_t dst = b * a.hw + p;
      if (a.pit) a.pit[dst] = pit;
      if (a.nll) a.nll[dst] = nll;
      if (a.crps) a.crps[dst] = crps;
    }
  }
  __syncthreads();
  double* red = (double*)&tile[0][0][0];
  block_epilogue(a, t, bins, red, (u32*)(red + 3 * 256));
}

// acc[j] += sum over the partial rows of column j (one workgroup per column; rows in a fixed order).  Column kIterWord,
// folded only after the evidential kernel, is a running maximum instead.
__global__ __launch_bounds__(256) void score_fold_kernel(const u64* __restrict__ part, int rows, u64* __restrict__ acc) {
  __shared__ u64 ri[256];
  __shared__ double rd[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j == kIterWord) {
    u64 m = 0;
    for (int r = tid; r < rows; r += 256) m = max(m, part[(size_t)r * kAccWords + j]);
    ri[tid] = m;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) ri[tid] = max(ri[tid], ri[tid + off]);
      __syncthreads();
    }
    if (tid == 0) acc[j] = max(acc[j], ri[0]);
    return;
  }
  const bool dbl = j >= 68;
  u64 s = 0;
  double d = 0.0;
  for (int r = tid; r < rows; r += 256) {
    const u64 v = part[(size_t)r * kAccWords + j];
    if (dbl)
      d += as_double(v);
    else
      s += v;
  }
  ri[tid] = s;
  rd[tid] = d;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      ri[tid] += ri[tid + off];
      rd[tid] += rd[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) acc[j] = dbl ? as_u64(as_double(acc[j]) + rd[0]) : acc[j] + ri[0];
}

// out: [0,K) observed share below p_k | n, n_masked, n_nonfinite, mean NLL, mean CRPS, mean PIT
__global__ void score_finalize_kernel(const u64* __restrict__ acc, int K, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const u64 n = acc[65];
  u64 run = 0;
  for (int k = 0; k < K; ++k) {
    run += acc[k];
    out[k] = n ? (double)run / (double)n : nan;
  }
  out[K] = (double)n;
  out[K + 1] = (double)acc[66];
  out[K + 2] = (double)acc[67];
  for (int k = 0; k < 3; ++k) out[K + 3 + k] = n ? as_double(acc[68 + k]) / (double)n : nan;
}

int fold_partials(Workspace* ws, int rows, int columns, hipStream_t stream) {
  hipLaunchKernelGGL(score_fold_kernel, dim3(columns), dim3(256), 0, stream, &ws->part[0][0], rows, ws->acc);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

typedef void (*Kernel)(Args);

template <int KIND, bool VEC>
static Kernel pick_kernel(int S) {
  switch (S) {
    case 1: return score_reg_kernel<KIND, 1, VEC>;
    case 2: return score_reg_kernel<KIND, 2, VEC>;
    case 3: return score_reg_kernel<KIND, 3, VEC>;
    case 4: return score_reg_kernel<KIND, 4, VEC>;
    default: break;
  }
  static_assert(kRegS == 4, "one case per register member count");
  // tile capacities: 16 members 32 KiB, 24 members 48 KiB, 32 members 64 KiB, 64 members 128 KiB
  if (S <= 16) return score_lds_kernel<KIND, 16, VEC>;
  if (S <= 24) return score_lds_kernel<KIND, 24, VEC>;
  if (S <= 32) return score_lds_kernel<KIND, 32, VEC>;
  return score_lds_kernel<KIND, 64, VEC>;
}

}  // namespace score
}  // namespace mimo

extern "C" size_t mimo_score_workspace_bytes(void) { return sizeof(mimo::score::Workspace); }

extern "C" int mimo_score_accumulate(const float* p1, const float* p2, const float* label, const float* mask, int32_t batch,
                                     int32_t members, int32_t channels, int32_t channel, int32_t mask_channels, int64_t hw,
                                     int32_t loss_kind, float eps_min, float eps_max, const float* expected_p,
                                     int32_t num_thresholds, float* pit_map, float* nll_map, float* crps_map, void* workspace,
                                     mimo_stream stream) {
  using namespace mimo;
  using namespace mimo::score;
  const uintptr_t all = (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)label | (uintptr_t)mask | (uintptr_t)pit_map |
                        (uintptr_t)nll_map | (uintptr_t)crps_map;
  if (!p1 || !p2 || !label || !expected_p || !workspace || batch < 1 || members < 1 || members > kMaxS || channels < 1 ||
      channel < 0 || channel >= channels || hw < 1 || num_thresholds < 1 || num_thresholds > kMaxK ||
      (loss_kind != MIMO_LOSS_LAPLACE_NLL && loss_kind != MIMO_LOSS_GAUSSIAN_NLL) || !(eps_min > 0.f) || !(eps_max >= eps_min) ||
      !(eps_max < INFINITY) || (mask && mask_channels != 1 && mask_channels != channels) || (all & 3) ||
      ((uintptr_t)expected_p & 3) || ((uintptr_t)workspace & 15)) {
    set_error("mimo_score_accumulate: invalid argument (1 <= members <= %d, 1 <= num_thresholds <= %d)", kMaxS, kMaxK);
    return MIMO_ERR_INVALID;
  }
  Workspace* ws = (Workspace*)workspace;
  const bool vec = (hw % 4 == 0) && (all & 15) == 0;
  Args a{p1, p2, label, mask, expected_p, pit_map, nll_map, crps_map, batch, members, channels, channel,
         mask ? mask_channels : 1, num_thresholds, hw, std::log((double)eps_min), std::log((double)eps_max), &ws->part[0][0]};
  // workgroups: one per 256 threads' worth of pixels (registers: 256 or 1024 pixels; LDS: one tile of one image)
  const int64_t work = members <= kRegS ? ceil_div64((int64_t)batch * (vec ? hw / 4 : hw), 256) : (int64_t)batch * ceil_div64(hw, kTile);
  const int blocks = (int)std::min<int64_t>(work, kBlocks);
  Kernel kernel = loss_kind == MIMO_LOSS_LAPLACE_NLL ? (vec ? pick_kernel<0, true>(members) : pick_kernel<0, false>(members))
                                                     : (vec ? pick_kernel<1, true>(members) : pick_kernel<1, false>(members));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  MIMO_KERNEL_CHECK();
  return fold_partials(ws, blocks, kFolded, (hipStream_t)stream);
}

extern "C" int mimo_score_finalize(const void* workspace, int32_t num_thresholds, double* out, mimo_stream stream) {
  using namespace mimo;
  using namespace mimo::score;
  if (!workspace || !out || num_thresholds < 1 || num_thresholds > kMaxK || ((uintptr_t)workspace & 15) || ((uintptr_t)out & 7)) {
    set_error("mimo_score_finalize: invalid argument");
    return MIMO_ERR_INVALID;
  }
  hipLaunchKernelGGL(score_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ((const Workspace*)workspace)->acc,
                     num_thresholds, out);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}
