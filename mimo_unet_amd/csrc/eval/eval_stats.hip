// Uncertainty evaluation on the device (gfx950): the sparsification ("precision-recall") and calibration tables of the
// reference's scripts/test/test_nyuv2_depth.py:128-170 / test_ndvi.py:86-128 without moving a pixel to the host.
//
//   mimo_eval_accumulate    one streaming pass per batch: per pixel 16-20 B in, one 8-byte record (bit pattern of
//                           combined_std, |error|) out, a 65-bin calibration counter and the running n / sum e / sum e^2
//   mimo_eval_accumulate_sources  the same pass, which also writes a second 8-byte record per pixel (bit patterns of
//                           aleatoric_std, epistemic_std) from the one read of the maps: 16 B out instead of 8
//   mimo_eval_select_by     exact simultaneous selection of the <= 128 cutoff ranks over ANY strided key word: a count-only
//                           radix select on the key bits, 11 / 11 / 10 bits per pass, integer counters only
//   mimo_eval_interval_sums_by  one more pass: (count, sum e, sum e^2) of every interval between / on the threshold keys,
//                           then the suffix sums, the tie rule and (on request) the calibration shares into an output slice
//   mimo_eval_select / mimo_eval_interval_sums  the two above over the record store's own words (key: low, error: high)
//
// The four orderings of the sparsification error are four key words: combined = low word of the first record, aleatoric /
// epistemic = low / high word of the second record, oracle = the first record's error word as its own key.  They run one
// after another on the one workspace and stream: the select clears its histograms and its per-cutoff state on entry, the
// interval pass overwrites every partial row it later folds, so a run leaves nothing the next one has to undo.
//
// Every sum of floating-point values is formed in a FIXED order (per lane group -> per wave -> per workgroup row -> a
// tree over the rows): no float atomics, so the same records give the same bits.  Counts use integer atomics (LDS inside
// a workgroup, device scope where a histogram crosses workgroups), which are order-independent.
//
// A skipped pixel (mask == 0, or a non-finite value / negative variance) still owns its record slot: EVERY word of its
// records gets the sentinel 0xFFFFFFFF (a NaN pattern no finite standard deviation or error has), so whichever word serves
// as the key, the later passes step over the slot; no pass reads the error of a slot whose key is the sentinel.  (The
// alternative, a separate pointer to the one word that holds the sentinel, costs every ordering a second load.)  The
// record store therefore needs no cross-workgroup prefix and every store of the hot kernel stays coalesced.
//
// Keys are compared as unsigned integers, so a key must be the bit pattern of a non-negative float.  The keys of the
// second record are canonicalised (-0 -> +0: sqrtf(-0.0f) is -0.0f = 0x80000000, above every finite value, and a variance
// of -0.0f passes the >= 0 test); the combined key is stored as sqrtf gives it.
#include "../common.h"

#include <algorithm>

namespace mimo {
namespace eval {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kMaxP = 128;         // cutoffs (percentiles)
constexpr int kMaxK = 64;          // calibration thresholds
constexpr int kBins = kMaxK + 1;   // calibration bins: bin j = "below" from threshold j on; bin K = never below
constexpr int kAccWords = 72;      // [0,65) bins, 65 n, 66 n_masked, 67 n_nonfinite, 68 sum e, 69 sum e^2 (doubles)
constexpr int kAccBlocks = 1024;   // partial rows of the accumulate pass
constexpr int kSlots = 2 * kMaxP + 1;  // intervals: 2 i = strictly between tab[i-1] and tab[i], 2 i + 1 = equal to tab[i]
constexpr int kIntBlocks = 512;    // partial rows of the interval pass
constexpr int kHistBlocks = 2048;
constexpr u32 kSentinel = 0xFFFFFFFFu;
constexpr int kL1 = 2048, kL2 = 2048, kL3 = 1024;  // histogram bins of the three select levels (11 / 11 / 10 bits)

// The torch-owned workspace (mimo_eval_workspace_bytes; zeroed by the caller at reset).
struct Workspace {
  u64 acc[kAccWords];
  u64 part[kAccBlocks][kAccWords];
  // select state, one entry per cutoff
  u64 surv[kMaxP];    // pixels that survive the cutoff: n - trunc(q n)
  u64 resid[kMaxP];   // ascending rank of the largest survivor inside the bucket chosen so far
  u64 eqtot[kMaxP];   // records whose key equals the threshold key
  u64 eqsurv[kMaxP];  // ... and how many of them survive
  u32 prefix[kMaxP];  // key bits decided so far
  u32 next[kMaxP];    // ... one digit longer: written by the resolve workgroups, adopted by the sort kernel
  u32 valid[kMaxP];
  u32 tab[kMaxP];     // sorted (with repeats) prefixes of the valid cutoffs: the next pass's lookup table
  u32 hist1[kL1];
  u32 hist2[kMaxP][kL2];
  u32 hist3[kMaxP][kL3];
  // interval sums: count, sum e, sum e^2
  u64 ipart[kIntBlocks][3][kSlots];
  u64 isum[3][kSlots];
};

__device__ __forceinline__ double as_double(u64 v) { return __longlong_as_double((long long)v); }
__device__ __forceinline__ u64 as_u64(double v) { return (u64)__double_as_longlong(v); }

// ------------------------------------------------------------------------------------------------ accumulate
struct PixelOut {
  u32 key, err;    // first record: combined_std, |error|
  u32 akey, ekey;  // second record (mimo_eval_accumulate_sources): aleatoric_std, epistemic_std
};

// One pixel: clamp, error, the two standard deviations, the calibration bin; what is skipped is only counted.
__device__ __forceinline__ PixelOut eval_pixel(float mu, float av, float ev, float y, float m, bool has_mask, int clip,
                                               float lo, float hi, const float* __restrict__ zt, int K, u32* __restrict__ bins,
                                               u32& n, u32& n_masked, u32& n_nonfinite, double& se, double& se2) {
  PixelOut r{kSentinel, kSentinel, kSentinel, kSentinel};
  if (has_mask && m == 0.f) {
    ++n_masked;
    return r;
  }
  const float var = __fadd_rn(av, ev);  // the sum is formed in fp32 first (test_nyuv2_depth.py:89)
  if (!(isfinite(mu) && isfinite(av) && isfinite(ev) && isfinite(y) && av >= 0.f && ev >= 0.f && isfinite(var))) {
    ++n_nonfinite;
    return r;
  }
  if (clip) {
    mu = fminf(fmaxf(mu, lo), hi);
    y = fminf(fmaxf(y, lo), hi);
  }
  const float e = fabsf(__fsub_rn(y, mu));
  const float astd = sqrtf(av);
  const float s = __fmul_rn(astd, 0.70710678118654752f);  // scale = aleatoric_std / sqrt(2)
  // first threshold j with y < mu + s z_j (monotone in j): lower bound over the table padded to 64 with +inf
  int j = 0;
#pragma unroll
  for (int step = 32; step > 0; step >>= 1) {
    const float t = __fadd_rn(mu, __fmul_rn(s, zt[j + step - 1]));
    j += (y < t) ? 0 : step;
  }
  j += (y < __fadd_rn(mu, __fmul_rn(s, zt[j]))) ? 0 : 1;
  // scale == 0: the reference's ppf is NaN at every p, so the pixel is "not below" in every row
  j = (s == 0.f || j > K) ? K : j;
  atomicAdd(&bins[j], 1u);
  ++n;
  se += (double)e;
  se2 += (double)e * (double)e;
  r.key = __float_as_uint(sqrtf(var));
  r.err = __float_as_uint(e);
  r.akey = __float_as_uint(astd) & 0x7FFFFFFFu;  // -0 -> +0
  r.ekey = __float_as_uint(sqrtf(ev)) & 0x7FFFFFFFu;
  return r;
}

// VEC: hw % 4 == 0 and every pointer 16-byte aligned -> one float4 of pixels per thread per step; otherwise the same
// walk with scalar loads and a bounds test per pixel (the last quad of an image may be partial).  SRC: the second record
// goes to srec at the same slot (rec_vec then covers both stores).
template <bool VEC, bool SRC>
__global__ __launch_bounds__(256) void eval_accumulate_kernel(
    const float* __restrict__ mean, const float* __restrict__ avar, const float* __restrict__ evar,
    const float* __restrict__ label, const float* __restrict__ mask, int B, int C, int channel, int MC, int64_t hw,
    int clip, float lo, float hi, const float* __restrict__ z, int K, uint2* __restrict__ rec, uint2* __restrict__ srec,
    int rec_vec, u64* __restrict__ part) {
  __shared__ float zt[kMaxK + 1];
  __shared__ u32 bins[4][kBins + 3];
  __shared__ double red[2][256];
  __shared__ u32 redn[3][256];
  const int tid = threadIdx.x, wave = tid >> 6;
  if (tid <= kMaxK) zt[tid] = tid < K ? z[tid] : INFINITY;
  for (int i = tid; i < 4 * (kBins + 3); i += 256) (&bins[0][0])[i] = 0u;
  __syncthreads();
  const int64_t qpi = (hw + 3) >> 2, quads = (int64_t)B * qpi;
  const int mch = MC == 1 ? 0 : channel;
  u32 n = 0, nm = 0, nf = 0;
  double se = 0.0, se2 = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < quads; q += (int64_t)gridDim.x * 256) {
    const int64_t b = q / qpi, p0 = (q - b * qpi) << 2;
    const int64_t src = (b * C + channel) * hw + p0, msrc = (b * MC + mch) * hw + p0, dst = b * hw + p0;
    float mu[4], av[4], ev[4], y[4], m[4] = {1.f, 1.f, 1.f, 1.f};
    int cnt = 4;
    if (VEC) {
      *(float4*)mu = *(const float4*)(mean + src);
      *(float4*)av = *(const float4*)(avar + src);
      *(float4*)ev = *(const float4*)(evar + src);
      *(float4*)y = *(const float4*)(label + src);
      if (mask) *(float4*)m = *(const float4*)(mask + msrc);
    } else {
      cnt = (int)(hw - p0 < 4 ? hw - p0 : 4);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) {
          mu[k] = mean[src + k];
          av[k] = avar[src + k];
          ev[k] = evar[src + k];
          y[k] = label[src + k];
          if (mask) m[k] = mask[msrc + k];
        }
    }
    PixelOut o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) o[k] = eval_pixel(mu[k], av[k], ev[k], y[k], m[k], mask != nullptr, clip, lo, hi, zt, K, bins[wave], n, nm, nf, se, se2);
    if (VEC && rec_vec) {  // the record store is 16-byte aligned at dst: two 16-byte stores
      uint4* d = (uint4*)(rec + dst);
      d[0] = make_uint4(o[0].key, o[0].err, o[1].key, o[1].err);
      d[1] = make_uint4(o[2].key, o[2].err, o[3].key, o[3].err);
      if (SRC) {
        uint4* sd = (uint4*)(srec + dst);
        sd[0] = make_uint4(o[0].akey, o[0].ekey, o[1].akey, o[1].ekey);
        sd[1] = make_uint4(o[2].akey, o[2].ekey, o[3].akey, o[3].ekey);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) {
          rec[dst + k] = make_uint2(o[k].key, o[k].err);
          if (SRC) srec[dst + k] = make_uint2(o[k].akey, o[k].ekey);
        }
    }
  }
  // one partial row per workgroup: counts as integers, sums in double, a fixed-order tree
  red[0][tid] = se;
  red[1][tid] = se2;
  redn[0][tid] = n;
  redn[1][tid] = nm;
  redn[2][tid] = nf;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
      redn[0][tid] += redn[0][tid + off];
      redn[1][tid] += redn[1][tid + off];
      redn[2][tid] += redn[2][tid + off];
    }
    __syncthreads();
  }
  u64* row = part + (size_t)blockIdx.x * kAccWords;
  if (tid < kBins) row[tid] = (u64)bins[0][tid] + bins[1][tid] + bins[2][tid] + bins[3][tid];
  if (tid >= 65 && tid < 68) row[tid] = redn[tid - 65][0];
  if (tid == 68 || tid == 69) row[tid] = as_u64(red[tid - 68][0]);
}

// acc[j] += sum over the partial rows of column j (one workgroup per column; rows in a fixed order)
__global__ __launch_bounds__(256) void eval_fold_kernel(const u64* __restrict__ part, int rows, u64* __restrict__ acc) {
  __shared__ u64 ri[256];
  __shared__ double rd[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  const bool dbl = j >= 68;
  u64 a = 0;
  double d = 0.0;
  for (int r = tid; r < rows; r += 256) {
    const u64 v = part[(size_t)r * kAccWords + j];
    if (dbl)
      d += as_double(v);
    else
      a += v;
  }
  ri[tid] = a;
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

// ------------------------------------------------------------------------------------------------ select
// lower bound in a sorted LDS table of n <= 128 entries: first index with tab[i] >= v
__device__ __forceinline__ int lower_bound_u32(const u32* tab, int n, u32 v) {
  int lo = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    const bool lt = tab[lo + half] < v;
    lo = lt ? lo + half + 1 : lo;
    len = lt ? len - half - 1 : half;
  }
  return lo;
}

// One count per lane into dst[idx] (idx < 0: none).  The lanes that share the first active lane's counter add once,
// with their number: a run of identical keys (a clamped variance, a constant map) is then one atomic per wave instead of
// 64 queued on one word.
__device__ __forceinline__ void wave_count(u32* dst, int idx) {
  const u64 act = __ballot(idx >= 0);
  if (!act) return;
  const int first = __ffsll((long long)act) - 1;
  const int i0 = __shfl(idx, first);
  const bool same = idx == i0;
  const u64 m = __ballot(same);
  if (same) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(dst + i0, (u32)__popcll(m));
  } else if (idx >= 0) {
    atomicAdd(dst + idx, 1u);
  }
}

__global__ void eval_select_init_kernel(const u64* __restrict__ acc, const double* __restrict__ pct, int P, Workspace* ws) {
  const int c = threadIdx.x;
  if (c >= kMaxP) return;
  u64 surv = 0;
  if (c < P) {
    const u64 n = acc[65];
    // the cutoff index is the truncation of the float64 product (test_nyuv2_depth.py:137)
    const double prod = pct[c] * (double)n;
    u64 r = prod > 0.0 ? (u64)prod : 0;  // NaN -> 0
    r = r > n ? n : r;
    surv = n - r;
  }
  ws->surv[c] = surv;
  ws->valid[c] = surv > 0;
  ws->resid[c] = surv > 0 ? surv - 1 : 0;
  ws->prefix[c] = 0;
  ws->next[c] = 0;
  ws->eqtot[c] = 0;
  ws->eqsurv[c] = 0;
  ws->tab[c] = 0;
}

// LEVEL 1: every record by its top 11 bits (LDS histogram, flushed with one device-scope add per non-empty bin).
// LEVEL 2 / 3: only records whose upper 11 / 22 bits are in the table the previous level left, by their next 11 / 10 bits.
// Record i's key is keys[i * stride].  WORD 0 / 1: the key is that word of an 8-byte record in a 16-byte aligned store
// `keys` (stride 2): two records per 16-byte load.  WORD < 0: any stride, scalar loads.
template <int LEVEL, int WORD>
__global__ __launch_bounds__(256) void eval_hist_kernel(const u32* __restrict__ keys, int stride, int64_t total, int P,
                                                        Workspace* ws) {
  __shared__ u32 sh[LEVEL == 1 ? kL1 : kMaxP];
  const int tid = threadIdx.x;
  if (LEVEL == 1) {
    for (int i = tid; i < kL1; i += 256) sh[i] = 0u;
  } else if (tid < kMaxP) {
    sh[tid] = tid < P ? ws->tab[tid] : kSentinel;
  }
  __syncthreads();
  const int64_t pairs = (total + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < pairs; q += (int64_t)gridDim.x * 256) {
    u32 key[2] = {kSentinel, kSentinel};
    if (WORD >= 0) {
      const uint2* rec = (const uint2*)keys;
      if (2 * q + 1 < total) {
        const uint4 v = *(const uint4*)(rec + 2 * q);
        key[0] = WORD ? v.y : v.x;
        key[1] = WORD ? v.w : v.z;
      } else {
        const uint2 v = rec[2 * q];
        key[0] = WORD ? v.y : v.x;
      }
    } else {
      key[0] = keys[2 * q * stride];
      if (2 * q + 1 < total) key[1] = keys[(2 * q + 1) * stride];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      int idx = -1;
      if (key[k] != kSentinel) {
        if (LEVEL == 1) {
          idx = (int)(key[k] >> 21);
        } else {
          const u32 parent = LEVEL == 2 ? key[k] >> 21 : key[k] >> 10;
          const int i = lower_bound_u32(sh, P, parent);
          if (i < P && sh[i] == parent) idx = LEVEL == 2 ? i * kL2 + (int)((key[k] >> 10) & 2047u) : i * kL3 + (int)(key[k] & 1023u);
        }
      }
      if (LEVEL == 1) {
        wave_count(sh, idx);
      } else {
        wave_count(LEVEL == 2 ? &ws->hist2[0][0] : &ws->hist3[0][0], idx);
      }
    }
  }
  if (LEVEL == 1) {
    __syncthreads();
    for (int i = tid; i < kL1; i += 256)
      if (sh[i]) atomicAdd(&ws->hist1[i], sh[i]);
  }
}

// Workgroup i scans histogram row i (the first of a run of equal table entries; level 1 has the one row) and moves every
// cutoff whose prefix is that entry one digit down: the bucket that holds its rank, and the rank inside it.
template <int LEVEL>
__global__ __launch_bounds__(256) void eval_resolve_kernel(int P, Workspace* ws) {
  constexpr int NB = LEVEL == 3 ? kL3 : kL2, PER = NB / 256, BITS = LEVEL == 3 ? 10 : 11;
  __shared__ u64 ex[NB + 1];
  __shared__ u64 tsum[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  u32 parent = 0;
  const u32* row = ws->hist1;
  if (LEVEL == 1) {
    if (i != 0) return;
  } else {
    if (i >= P) return;
    parent = ws->tab[i];
    if (parent == kSentinel || (i > 0 && ws->tab[i - 1] == parent)) return;
    row = LEVEL == 2 ? ws->hist2[i] : ws->hist3[i];
  }
  u32 h[PER];
  u64 s = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    h[k] = row[tid * PER + k];
    s += h[k];
  }
  tsum[tid] = s;
  __syncthreads();
  if (tid == 0) {  // 256 serial adds: exclusive scan of the per-thread sums
    u64 run = 0;
    for (int t = 0; t < 256; ++t) {
      const u64 v = tsum[t];
      tsum[t] = run;
      run += v;
    }
    ex[NB] = run;
  }
  __syncthreads();
  u64 run = tsum[tid];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    ex[tid * PER + k] = run;
    run += h[k];
  }
  __syncthreads();
  const int c = tid;
  if (c < P && ws->valid[c] && (LEVEL == 1 || ws->prefix[c] == parent)) {
    const u64 r = ws->resid[c];
    int lo = 0, len = NB;  // last d in [0, NB) with ex[d] <= r
    while (len > 1) {
      const int half = len >> 1;
      const bool le = ex[lo + half] <= r;
      lo = le ? lo + half : lo;
      len = le ? len - half : half;
    }
    // into next[], not prefix[]: the sibling workgroups of this launch still match their cutoffs on prefix[]
    ws->next[c] = LEVEL == 1 ? (u32)lo : ((parent << BITS) | (u32)lo);
    ws->resid[c] = r - ex[lo];
    if (LEVEL == 3) {
      ws->eqtot[c] = ex[lo + 1] - ex[lo];
      ws->eqsurv[c] = r - ex[lo] + 1;
    }
  }
}

// prefix = next (the digit the resolve launch found); tab = the valid cutoffs' prefixes, sorted ascending with repeats
// (rank sort); invalid cutoffs go last as the sentinel
__global__ void eval_sort_kernel(int P, Workspace* ws) {
  __shared__ u32 v[kMaxP];
  const int c = threadIdx.x;
  if (c < kMaxP) {
    const u32 nx = ws->next[c];
    ws->prefix[c] = nx;
    v[c] = (c < P && ws->valid[c]) ? nx : kSentinel;
  }
  __syncthreads();
  if (c >= kMaxP) return;
  int rank = 0;
  for (int j = 0; j < kMaxP; ++j) rank += (v[j] < v[c] || (v[j] == v[c] && j < c)) ? 1 : 0;
  ws->tab[rank] = v[c];
}

// ------------------------------------------------------------------------------------------------ interval sums
// Each record finds its interval among the sorted threshold keys.  Per 64 records a wave groups its lanes by interval
// (one readfirstlane + ballot per distinct interval), every lane sums its group's errors in lane order from an LDS
// staging row, and the group's first lane adds the result to the wave's PRIVATE slot row: plain read-modify-write on
// distinct addresses, a fixed order of additions, no float atomic.
// Record i: key keys[i * kstride], error errors[i * estride].  REC: the two are the words of one 8-byte record at `keys`.
template <bool REC>
__global__ __launch_bounds__(256) void eval_interval_kernel(const u32* __restrict__ keys, int kstride, const u32* __restrict__ errors,
                                                            int estride, int64_t total, int P, Workspace* ws) {
  __shared__ u32 tab[kMaxP];
  __shared__ float stage[4][64];
  __shared__ double sse[4][kSlots], sse2[4][kSlots];
  __shared__ u32 scnt[4][kSlots];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < kMaxP) tab[tid] = tid < P ? ws->tab[tid] : kSentinel;
  for (int i = tid; i < 4 * kSlots; i += 256) {
    (&sse[0][0])[i] = 0.0;
    (&sse2[0][0])[i] = 0.0;
    (&scnt[0][0])[i] = 0u;
  }
  __syncthreads();
  const int64_t steps = (total + 255) / 256;
  for (int64_t st = blockIdx.x; st < steps; st += gridDim.x) {
    const int64_t i = st * 256 + tid;
    int slot = -1;
    float e = 0.f;
    if (i < total) {
      uint2 r;
      if (REC) {
        r = ((const uint2*)keys)[i];
      } else {
        r.x = keys[i * kstride];
        r.y = r.x != kSentinel ? errors[i * estride] : 0u;
      }
      if (r.x != kSentinel) {
        const int lb = lower_bound_u32(tab, P, r.x);
        slot = 2 * lb + ((lb < P && tab[lb] == r.x) ? 1 : 0);
        e = __uint_as_float(r.y);
      }
    }
    stage[wave][lane] = e;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    u64 mine = 0;
    bool done = false;
    while (!done) {  // one trip per distinct interval in the wave
      const int s0 = __builtin_amdgcn_readfirstlane(slot);
      const u64 same = __ballot(slot == s0);  // among the lanes still in the loop: every lane of that interval
      if (slot == s0) {
        mine = same;
        done = true;
      }
    }
    if (slot >= 0) {
      double a = 0.0, a2 = 0.0;
      for (u64 mm = mine; mm; mm &= mm - 1) {
        const float v = stage[wave][__ffsll((long long)mm) - 1];
        a += (double)v;
        a2 += (double)v * (double)v;
      }
      if (lane == __ffsll((long long)mine) - 1) {
        sse[wave][slot] += a;
        sse2[wave][slot] += a2;
        scnt[wave][slot] += (u32)__popcll(mine);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __syncthreads();
  u64* row = &ws->ipart[blockIdx.x][0][0];
  for (int s = tid; s < kSlots; s += 256) {
    row[s] = (u64)scnt[0][s] + scnt[1][s] + scnt[2][s] + scnt[3][s];
    row[kSlots + s] = as_u64(((sse[0][s] + sse[1][s]) + sse[2][s]) + sse[3][s]);
    row[2 * kSlots + s] = as_u64(((sse2[0][s] + sse2[1][s]) + sse2[2][s]) + sse2[3][s]);
  }
}

// isum[k][s] = sum over the workgroup rows (fixed order); grid (kSlots, 3), 64 threads
__global__ void eval_interval_fold_kernel(int rows, Workspace* ws) {
  const int s = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
  u64 a = 0;
  double d = 0.0;
  for (int r = lane; r < rows; r += 64) {
    const u64 v = ws->ipart[r][k][s];
    if (k == 0)
      a += v;
    else
      d += as_double(v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off);
    d += __shfl_xor(d, off);
  }
  if (lane == 0) ws->isum[k][s] = k == 0 ? a : as_u64(d);
}

// out (doubles): [0,P) mae | [P,2P) rmse | [2P,3P) threshold value of the key | and, when K > 0, [3P,3P+K) observed share |
//                n, n_masked, n_nonfinite, mae, mse, rmse of the whole set
__global__ void eval_tables_kernel(int P, int K, Workspace* ws, double* __restrict__ out) {
  __shared__ double cse[kSlots + 1], cse2[kSlots + 1];
  __shared__ u32 tab[kMaxP];
  const int c = threadIdx.x;
  if (c < kMaxP) tab[c] = c < P ? ws->tab[c] : kSentinel;
  if (c == 0) {  // exclusive prefix sums over the <= 257 intervals, ascending
    double a = 0.0, a2 = 0.0;
    for (int s = 0; s < kSlots; ++s) {
      cse[s] = a;
      cse2[s] = a2;
      a += as_double(ws->isum[1][s]);
      a2 += as_double(ws->isum[2][s]);
    }
    cse[kSlots] = a;
    cse2[kSlots] = a2;
  }
  __syncthreads();
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (c < P) {
    double mae = nan, rmse = nan, keyv = nan;
    if (ws->valid[c]) {
      const u32 key = ws->prefix[c];
      const int slot = 2 * lower_bound_u32(tab, P, key) + 1;
      const u64 et = ws->eqtot[c], es = ws->eqsurv[c];
      // a tie group that straddles the cutoff contributes its mean error for the number of its pixels that survive
      const double f = es == et ? 1.0 : (double)es / (double)et;
      const double cnt = (double)ws->surv[c];
      const double s1 = cse[slot] + as_double(ws->isum[1][slot]) * f;
      const double s2 = cse2[slot] + as_double(ws->isum[2][slot]) * f;
      mae = s1 / cnt;
      rmse = sqrt(s2 / cnt);
      keyv = (double)__uint_as_float(key);
    }
    out[c] = mae;
    out[P + c] = rmse;
    out[2 * P + c] = keyv;
  }
  if (c == 0 && K > 0) {
    const u64 n = ws->acc[65];
    u64 run = 0;
    for (int k = 0; k < K; ++k) {
      run += ws->acc[k];
      out[3 * P + k] = n ? (double)run / (double)n : nan;
    }
    double* sc = out + 3 * P + K;
    const double mse = n ? as_double(ws->acc[69]) / (double)n : nan;
    sc[0] = (double)n;
    sc[1] = (double)ws->acc[66];
    sc[2] = (double)ws->acc[67];
    sc[3] = n ? as_double(ws->acc[68]) / (double)n : nan;
    sc[4] = mse;
    sc[5] = sqrt(mse);
  }
}

}  // namespace eval
}  // namespace mimo

extern "C" size_t mimo_eval_workspace_bytes(void) { return sizeof(mimo::eval::Workspace); }

// the accumulate pass of both entry points; source_records == nullptr: the first record only
static int eval_accumulate(const char* what, const float* mean, const float* aleatoric_var, const float* epistemic_var,
                           const float* label, const float* mask, int32_t batch, int32_t channels, int32_t channel,
                           int32_t mask_channels, int64_t hw, int32_t clip, float clip_lo, float clip_hi, const float* thresholds,
                           int32_t num_thresholds, uint64_t* records, uint64_t* source_records, void* workspace,
                           mimo_stream stream) {
  using namespace mimo;
  using namespace mimo::eval;
  if (!mean || !aleatoric_var || !epistemic_var || !label || !thresholds || !records || !workspace || batch < 1 ||
      channels < 1 || channel < 0 || channel >= channels || hw < 1 || num_thresholds < 1 || num_thresholds > kMaxK ||
      (mask && mask_channels != 1 && mask_channels != channels) || ((uintptr_t)records & 7) ||
      ((uintptr_t)source_records & 7) || ((uintptr_t)workspace & 15)) {
    set_error("%s: invalid argument", what);
    return MIMO_ERR_INVALID;
  }
  Workspace* ws = (Workspace*)workspace;
  const uintptr_t al = (uintptr_t)mean | (uintptr_t)aleatoric_var | (uintptr_t)epistemic_var | (uintptr_t)label | (uintptr_t)mask;
  const bool vec = (hw % 4 == 0) && (al & 15) == 0;
  const int rec_vec = (((uintptr_t)records | (uintptr_t)source_records) & 15) == 0;
  const int64_t quads = (int64_t)batch * ((hw + 3) / 4);
  const int blocks = (int)std::min<int64_t>(ceil_div64(quads, 256), kAccBlocks);
  const int mc = mask ? mask_channels : 1;
  auto kernel = source_records ? (vec ? eval_accumulate_kernel<true, true> : eval_accumulate_kernel<false, true>)
                               : (vec ? eval_accumulate_kernel<true, false> : eval_accumulate_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, mean, aleatoric_var, epistemic_var, label, mask,
                     batch, channels, channel, mc, hw, clip, clip_lo, clip_hi, thresholds, num_thresholds, (uint2*)records,
                     (uint2*)source_records, rec_vec, &ws->part[0][0]);
  MIMO_KERNEL_CHECK();
  hipLaunchKernelGGL(eval_fold_kernel, dim3(70), dim3(256), 0, (hipStream_t)stream, &ws->part[0][0], blocks, ws->acc);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_eval_accumulate(const float* mean, const float* aleatoric_var, const float* epistemic_var,
                                    const float* label, const float* mask, int32_t batch, int32_t channels, int32_t channel,
                                    int32_t mask_channels, int64_t hw, int32_t clip, float clip_lo, float clip_hi,
                                    const float* thresholds, int32_t num_thresholds, uint64_t* records, void* workspace,
                                    mimo_stream stream) {
  return eval_accumulate("mimo_eval_accumulate", mean, aleatoric_var, epistemic_var, label, mask, batch, channels, channel,
                         mask_channels, hw, clip, clip_lo, clip_hi, thresholds, num_thresholds, records, nullptr, workspace, stream);
}

extern "C" int mimo_eval_accumulate_sources(const float* mean, const float* aleatoric_var, const float* epistemic_var,
                                            const float* label, const float* mask, int32_t batch, int32_t channels,
                                            int32_t channel, int32_t mask_channels, int64_t hw, int32_t clip, float clip_lo,
                                            float clip_hi, const float* thresholds, int32_t num_thresholds, uint64_t* records,
                                            uint64_t* source_records, void* workspace, mimo_stream stream) {
  if (!source_records) {
    mimo::set_error("mimo_eval_accumulate_sources: invalid argument");
    return MIMO_ERR_INVALID;
  }
  return eval_accumulate("mimo_eval_accumulate_sources", mean, aleatoric_var, epistemic_var, label, mask, batch, channels, channel,
                         mask_channels, hw, clip, clip_lo, clip_hi, thresholds, num_thresholds, records, source_records, workspace,
                         stream);
}

extern "C" int mimo_eval_select_by(const uint32_t* keys, int32_t key_stride_words, int64_t num_records,
                                   const double* percentiles, int32_t num_percentiles, void* workspace, mimo_stream stream) {
  using namespace mimo;
  using namespace mimo::eval;
  if (!keys || key_stride_words < 1 || !percentiles || !workspace || num_records < 1 || num_percentiles < 1 ||
      num_percentiles > kMaxP || num_records >= ((int64_t)1 << 32) || ((uintptr_t)keys & 3) || ((uintptr_t)workspace & 15)) {  // the histogram counters are 32-bit
    set_error("mimo_eval_select_by: invalid argument");
    return MIMO_ERR_INVALID;
  }
  Workspace* ws = (Workspace*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int P = num_percentiles, stride = key_stride_words;
  // a word of an 8-byte record in a 16-byte aligned store: the kernels load whole record pairs from the store's base
  const int word = (int)(((uintptr_t)keys >> 2) & 1);
  const bool pair = stride == 2 && (((uintptr_t)keys - 4 * word) & 15) == 0;
  const u32* base = pair ? keys - word : keys;
  const int blocks = (int)std::min<int64_t>(ceil_div64((num_records + 1) / 2, 256), kHistBlocks);
  auto hist1 = !pair ? eval_hist_kernel<1, -1> : word ? eval_hist_kernel<1, 1> : eval_hist_kernel<1, 0>;
  auto hist2 = !pair ? eval_hist_kernel<2, -1> : word ? eval_hist_kernel<2, 1> : eval_hist_kernel<2, 0>;
  auto hist3 = !pair ? eval_hist_kernel<3, -1> : word ? eval_hist_kernel<3, 1> : eval_hist_kernel<3, 0>;
  MIMO_HIP_CHECK(hipMemsetAsync(ws->hist1, 0, sizeof(ws->hist1) + sizeof(ws->hist2) + sizeof(ws->hist3), s));
  hipLaunchKernelGGL(eval_select_init_kernel, dim3(1), dim3(kMaxP), 0, s, ws->acc, percentiles, P, ws);
  hipLaunchKernelGGL(hist1, dim3(blocks), dim3(256), 0, s, base, stride, num_records, P, ws);
  hipLaunchKernelGGL(eval_resolve_kernel<1>, dim3(1), dim3(256), 0, s, P, ws);
  hipLaunchKernelGGL(eval_sort_kernel, dim3(1), dim3(kMaxP), 0, s, P, ws);
  hipLaunchKernelGGL(hist2, dim3(blocks), dim3(256), 0, s, base, stride, num_records, P, ws);
  hipLaunchKernelGGL(eval_resolve_kernel<2>, dim3(P), dim3(256), 0, s, P, ws);
  hipLaunchKernelGGL(eval_sort_kernel, dim3(1), dim3(kMaxP), 0, s, P, ws);
  hipLaunchKernelGGL(hist3, dim3(blocks), dim3(256), 0, s, base, stride, num_records, P, ws);
  hipLaunchKernelGGL(eval_resolve_kernel<3>, dim3(P), dim3(256), 0, s, P, ws);
  hipLaunchKernelGGL(eval_sort_kernel, dim3(1), dim3(kMaxP), 0, s, P, ws);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_eval_interval_sums_by(const uint32_t* keys, int32_t key_stride_words, const uint32_t* errors,
                                          int32_t error_stride_words, int64_t num_records, int32_t num_percentiles,
                                          int32_t num_thresholds, void* workspace, double* out, mimo_stream stream) {
  using namespace mimo;
  using namespace mimo::eval;
  if (!keys || key_stride_words < 1 || !errors || error_stride_words < 1 || !workspace || !out || num_records < 1 ||
      num_percentiles < 1 || num_percentiles > kMaxP || num_thresholds < 0 || num_thresholds > kMaxK ||
      num_records >= ((int64_t)1 << 32) || (((uintptr_t)keys | (uintptr_t)errors) & 3) || ((uintptr_t)workspace & 15)) {
    set_error("mimo_eval_interval_sums_by: invalid argument");
    return MIMO_ERR_INVALID;
  }
  Workspace* ws = (Workspace*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)std::min<int64_t>(ceil_div64(num_records, 256), kIntBlocks);
  const bool rec = key_stride_words == 2 && error_stride_words == 2 && errors == keys + 1 && ((uintptr_t)keys & 7) == 0;
  hipLaunchKernelGGL(rec ? eval_interval_kernel<true> : eval_interval_kernel<false>, dim3(blocks), dim3(256), 0, s, keys,
                     key_stride_words, errors, error_stride_words, num_records, num_percentiles, ws);
  hipLaunchKernelGGL(eval_interval_fold_kernel, dim3(kSlots, 3), dim3(64), 0, s, blocks, ws);
  hipLaunchKernelGGL(eval_tables_kernel, dim3(1), dim3(kMaxP), 0, s, num_percentiles, num_thresholds, ws, out);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_eval_select(const uint64_t* records, int64_t num_records, const double* percentiles,
                                int32_t num_percentiles, void* workspace, mimo_stream stream) {
  if (!records || ((uintptr_t)records & 15)) {
    mimo::set_error("mimo_eval_select: invalid argument");
    return MIMO_ERR_INVALID;
  }
  return mimo_eval_select_by((const uint32_t*)records, 2, num_records, percentiles, num_percentiles, workspace, stream);
}

extern "C" int mimo_eval_interval_sums(const uint64_t* records, int64_t num_records, int32_t num_percentiles,
                                       int32_t num_thresholds, void* workspace, double* out, mimo_stream stream) {
  if (!records || ((uintptr_t)records & 7) || num_thresholds < 1) {
    mimo::set_error("mimo_eval_interval_sums: invalid argument");
    return MIMO_ERR_INVALID;
  }
  return mimo_eval_interval_sums_by((const uint32_t*)records, 2, (const uint32_t*)records + 1, 2, num_records, num_percentiles,
                                    num_thresholds, workspace, out, stream);
}

