// Single-operator C-ABI entry points (mimo_op_*): thin drivers around the same kernels the
// plan runs, for the per-kernel parity tests.  The convolutions pack their weight image as the plan does: one PackJob
// from pack::make_job (pack_layout.h), written by pack_jobs_kernel.  They allocate temporaries and synchronise —
// test plumbing, never on the timed path.
#include <algorithm>
#include <vector>

#include "elementwise.h"

using namespace mimo;
using pack::is_mixed;
using pack::store_type;

namespace {

// zeroed device temporaries of one call of the entry point `who`.  A failed allocation returns nullptr, is remembered and
// reported by ok(): allocate what a step needs, then MIMO_TRY(t.ok()) before the first use
struct Temp {
  const char* who;
  bool failed = false;
  std::vector<void*> ptrs;
  explicit Temp(const char* who_) : who(who_) {}
  ~Temp() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T>
  T* get(size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
      failed = true;
      return nullptr;
    }
    (void)hipMemset(q, 0, std::max<size_t>(count, 1) * sizeof(T));
    ptrs.push_back(q);
    return static_cast<T*>(q);
  }
  int* ints(const std::vector<int>& v) {
    int* p = get<int>(v.size());
    if (p) (void)hipMemcpy(p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice);
    return p;
  }
  int ok() const {
    if (failed) set_error("%s: allocation failed", who);
    return failed ? MIMO_ERR_HIP : MIMO_OK;
  }
};

std::vector<int> ident_map(int padded, int logical) {
  std::vector<int> m(padded);
  for (int i = 0; i < padded; ++i) m[i] = i < logical ? i : -1;
  return m;
}

__global__ void colsum_naive_kernel(const float* __restrict__ x, int64_t rows, int ld, int C, float* __restrict__ out) {
  const int c = blockIdx.x;
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < rows; r += blockDim.x) s += (double)x[r * ld + c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0 && c < C) out[c] = (float)red[0];
}

__global__ void sums_to_stats_kernel(const double* __restrict__ sums, int chunks, int cout_pad, int cout,
                                     double* __restrict__ stats) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cout) return;
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < chunks; ++k) {
    s1 += sums[(size_t)k * 2 * cout_pad + c];
    s2 += sums[(size_t)k * 2 * cout_pad + cout_pad + c];
  }
  stats[c] = s1;
  stats[cout + c] = s2;
}

// fp32 <-> 16-bit storage conversions, so that the fp32 test interface can drive the 16-bit storage kernels
template <typename T>
__global__ void to16_kernel(const float* __restrict__ s, T* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = (T)s[i];
}
template <typename T>
__global__ void from16_kernel(const T* __restrict__ s, float* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = (float)s[i];
}
int to16(const float* s, void* d, int64_t n, bool f16, hipStream_t st) {
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  if (f16)
    hipLaunchKernelGGL(to16_kernel<_Float16>, dim3(blocks), dim3(256), 0, st, s, (_Float16*)d, n);
  else
    hipLaunchKernelGGL(to16_kernel<__bf16>, dim3(blocks), dim3(256), 0, st, s, (__bf16*)d, n);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}
int from16(const void* s, float* d, int64_t n, bool f16, hipStream_t st) {
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  if (f16)
    hipLaunchKernelGGL(from16_kernel<_Float16>, dim3(blocks), dim3(256), 0, st, (const _Float16*)s, d, n);
  else
    hipLaunchKernelGGL(from16_kernel<__bf16>, dim3(blocks), dim3(256), 0, st, (const __bf16*)s, d, n);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// `count` fp32 elements of `src` as the storage type of `precision`: src itself for fp32 storage, a rounded 16-bit copy otherwise
struct Stored {
  const void* in = nullptr;  // what the kernel reads
  void* out = nullptr;       // what the kernel writes (out16 or dst)
  uint16_t* b16 = nullptr;
  float* dst = nullptr;
  int64_t count = 0;
};
int stage_in(Temp& t, const float* src, int64_t count, int precision, hipStream_t st, Stored* s) {
  s->count = count;
  s->in = src;
  if (!src || !is_mixed(precision)) return MIMO_OK;
  s->b16 = t.get<uint16_t>(count);
  MIMO_TRY(t.ok());
  MIMO_TRY(to16(src, s->b16, count, precision == MIMO_PREC_FP16_MIXED, st));
  s->in = s->b16;
  return MIMO_OK;
}
// an output (read as well when the operator accumulates into it)
int stage_out(Temp& t, float* dst, int64_t count, int precision, hipStream_t st, Stored* s) {
  MIMO_TRY(stage_in(t, dst, count, precision, st, s));
  s->dst = dst;
  s->out = s->b16 ? (void*)s->b16 : (void*)dst;
  return MIMO_OK;
}
int stage_back(const Stored& s, int precision, hipStream_t st) {
  if (s.b16) MIMO_TRY(from16(s.b16, s.dst, s.count, precision == MIMO_PREC_FP16_MIXED, st));
  return MIMO_OK;
}

// The weight image of one convolution launch, written by the plan's packer from a table of one job: w is the bound
// parameter buffer (w_off = 0), the bias lies at its distance from w.  The fp16 kinds get no wmax word: the image keeps
// the fixed 2^8 (ConvLaunch::wmax == nullptr).  bias_dst != nullptr: the bias is copied.
int pack_image(Temp& t, int dir, int precision, const ConvDir& d, const float* w, const float* bias, float* bias_dst, int cout, int cin,
               int cin_p, int cout_p, hipStream_t st, ConvLaunch* a) {
  const int kind = pack::kind(precision, dir, d.split, d.wide != 0);
  const size_t elems = pack::image_elems(kind, d.wide ? d.wide : d.rows, dir == PACK_FWD ? cin_p : cout_p);
  void* img = kind == PK_F32 ? (void*)t.get<float>(elems) : (void*)t.get<uint16_t>(elems);
  const int* rm = t.ints(ident_map(d.rows, dir == PACK_FWD ? cout : cin));
  const int* cm = dir == PACK_FWD ? t.ints(ident_map(cin_p, cin)) : t.ints(ident_map(cout_p, cout));
  PackJob* job_dev = t.get<PackJob>(1);
  MIMO_TRY(t.ok());
  const bool with_bias = bias && bias_dst;
  const PackJob job = pack::make_job(dir, precision, d.split, cout, cin, cin_p, cout_p, d.rows, d.wide, d.pair, rm, cm, img, nullptr, 0,
                                     with_bias ? (int64_t)(((intptr_t)bias - (intptr_t)w) / (intptr_t)sizeof(float)) : 0,
                                     with_bias ? bias_dst : nullptr);
  MIMO_HIP_CHECK(hipMemcpy(job_dev, &job, sizeof(PackJob), hipMemcpyHostToDevice));
  MIMO_TRY(pack_jobs_launch(job_dev, 1, job.total, w, st));
  a->w = kind == PK_F32 ? static_cast<const float*>(img) : nullptr;
  a->wpk = kind == PK_F32 ? nullptr : img;
  return MIMO_OK;
}

// The recipe the plan makes for a layer of this geometry whose input channels lie in order (conv_recipe.h).  An entry point
// has no network to derive sched::wg_side_cus from: its weight gradient is sized for the whole chip (256 CUs), or for the
// MIMO_WGRAD_CUS a plan would honour (wgrad_cus, common.h: the tests run the split counts of the plans' 128 and 192 CUs).
ConvRecipe op_recipe(int precision, int n, int h, int w, int cin, int cin_p, int cout, int cout_p) {
  return conv_recipe(precision, 0, n, h, w, cin, cout, cin_p, cout_p, true, conv_env(wgrad_cus(256)));
}
// tensors are 16-bit where the plan's are: the operands and results of the 16-bit storage kernels
int stored_as(int precision, bool on_16bit_kernels) { return on_16bit_kernels ? precision : (int)MIMO_PREC_FP32; }

}  // namespace

extern "C" {

int mimo_op_conv3x3_forward(const float* x, const float* w, const float* bias, float* z, double* stats, int32_t n,
                            int32_t h, int32_t wd, int32_t cin, int32_t cin_p, int32_t cout, int32_t cout_p,
                            int32_t precision, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  Temp t("mimo_op_conv3x3_forward");
  const ConvRecipe r = op_recipe(precision, n, h, wd, cin, cin_p, cout, cout_p);
  const ConvDir& d = r.fwd;
  float* bp = t.get<float>(d.rows);
  const int rows_cap = std::max(std::max(conv3x3_stat_rows(n, h, wd), conv3x3_ws_stat_rows(n, h, wd)), 2048);
  float* partial = t.get<float>((size_t)rows_cap * 2 * d.rows);
  double* sums = t.get<double>((size_t)kMaxChunks * 2 * d.rows);
  float* kpart = d.kpart ? t.get<float>(d.kpart) : nullptr;  // (the slabs of the K split the plan would use)
  MIMO_TRY(t.ok());
  // 16-bit storage modes: the fp32 tensors of this interface are rounded into 16-bit buffers, the storage-mode kernels
  // run on those, the result is widened again (exact)
  const int sp = stored_as(precision, d.split);
  Stored xs, zs;
  MIMO_TRY(stage_in(t, x, (int64_t)n * h * wd * cin_p, sp, st, &xs));
  MIMO_TRY(stage_out(t, z, (int64_t)n * h * wd * cout_p, sp, st, &zs));
  ConvLaunch a = fill_conv_launch(r, PACK_FWD, n, h, wd, cin_p, cout_p);
  MIMO_TRY(pack_image(t, PACK_FWD, precision, d, w, bias, bp, cout, cin, cin_p, cout_p, st, &a));
  a.x = static_cast<const float*>(xs.in);
  a.y = static_cast<float*>(zs.out);
  a.bias = bp;
  a.stats = stats ? partial : nullptr;
  int rows = 0;
  if (d.split)
    MIMO_TRY(conv3x3_bf16x3_launch_k(a, d.mode, &rows, st, kpart, d.kpart));
  else if (r.thin)
    MIMO_TRY(conv3x3_thin_launch(a, cin, &rows, st));
  else
    MIMO_TRY(conv3x3_launch(a, &rows, st));
  MIMO_TRY(stage_back(zs, sp, st));
  if (stats) {
    int chunks = 0;
    MIMO_TRY(rowsum_launch(partial, rows, 2 * d.rows, sums, &chunks, st));
    hipLaunchKernelGGL(sums_to_stats_kernel, dim3(ceil_div(cout, 64)), dim3(64), 0, st, sums, chunks, d.rows, cout, stats);
    MIMO_KERNEL_CHECK();
  }
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_conv3x3_dgrad(const float* dz, const float* w, float* dx, int32_t n, int32_t h, int32_t wd, int32_t cin,
                          int32_t cin_p, int32_t cout, int32_t cout_p, int32_t precision, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  Temp t("mimo_op_conv3x3_dgrad");
  const ConvRecipe r = op_recipe(precision, n, h, wd, cin, cin_p, cout, cout_p);
  const ConvDir& d = r.dgrad;
  const int64_t ndz = (int64_t)n * h * wd * cout_p, ndx = (int64_t)n * h * wd * cin_p;
  // the padded-domain gradient, in the storage type (sized for fp32), folded in that storage and widened at the end
  float* dxpad = t.get<float>((size_t)n * (h + 2) * (wd + 2) * cin_p);
  // the bf16-pair kernel reads dz in split storage (see elementwise.h split_pairs_launch)
  float* dz_pairs = (d.split && !is_mixed(precision)) ? t.get<float>(ndz) : nullptr;
  float* kpart = d.kpart ? t.get<float>(d.kpart) : nullptr;
  MIMO_TRY(t.ok());
  Stored dzs, dxs;
  MIMO_TRY(stage_in(t, dz, ndz, precision, st, &dzs));
  MIMO_TRY(stage_out(t, dx, ndx, precision, st, &dxs));
  if (dz_pairs) MIMO_TRY(split_pairs_launch(dz, dz_pairs, (int64_t)n * h * wd, cout_p, st));
  ConvLaunch a = fill_conv_launch(r, PACK_DGRAD, n, h, wd, cin_p, cout_p);
  MIMO_TRY(pack_image(t, PACK_DGRAD, precision, d, w, nullptr, nullptr, cout, cin, cin_p, cout_p, st, &a));
  a.x = dz_pairs ? dz_pairs : static_cast<const float*>(dzs.in);
  a.y = dxpad;
  if (d.split)
    MIMO_TRY(conv3x3_bf16x3_launch_k(a, d.mode, nullptr, st, kpart, d.kpart));
  else
    MIMO_TRY(conv3x3_launch(a, nullptr, st));
  MIMO_TRY(fold_slice_launch(dxpad, store_type(precision), cin_p, 0, dxs.out, cin_p, n, h, wd, cin_p, 0, st));
  MIMO_TRY(stage_back(dxs, precision, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_conv3x3_wgrad(const float* x, const float* dz, float* dw, float* dbias, int32_t n, int32_t h, int32_t wd,
                          int32_t cin, int32_t cin_p, int32_t cout, int32_t cout_p, int32_t precision,
                          mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  Temp t("mimo_op_conv3x3_wgrad");
  const ConvRecipe r = op_recipe(precision, n, h, wd, cin, cin_p, cout, cout_p);
  const bool thin = r.wg_thin && wgrad_thin_ok(cin, cout_p, n, h, wd);  // the image convolution's kernel, as in the plan
  WgradLaunch a = fill_wgrad_launch(r, n, h, wd, cin_p, cout_p);
  a.x = x;
  a.dz = dz;
  a.partial = t.get<float>(thin ? wgrad_thin_scratch(cin, cout_p) : (size_t)(a.splits + a.splits / 8 + 2) * 9 * a.cin_pad * a.cout_pad);
  int* cm = t.ints(ident_map(cin_p, cin));
  MIMO_TRY(t.ok());
  if (thin) {
    MIMO_TRY(wgrad_thin_launch(x, cin_p, dz, cout_p, n, h, wd, cin, cout, cout_p, a.partial, dw, st));
  } else if (is_mixed(precision)) {  // dz, and the activations of every layer but the image convolution, as plain 16-bit NHWC tensors
    Stored xs, dzs;
    MIMO_TRY(stage_in(t, x, (int64_t)n * h * wd * cin_p, stored_as(precision, a.store <= 2), st, &xs));
    MIMO_TRY(stage_in(t, dz, (int64_t)n * h * wd * cout_p, precision, st, &dzs));
    a.x = static_cast<const float*>(xs.in);
    a.dz = static_cast<const float*>(dzs.in);
    MIMO_TRY(wgrad_split_launch(a, st));
  } else if (r.wg_split) {  // split storage of dz, as the BatchNorm-backward kernel writes it in the plan
    float* dzs = t.get<float>((size_t)n * h * wd * cout_p);
    // as in the plan: two fp16 MFMAs per product where the recipe has them, with max |dz| next to the split
    float* amax = r.wg_np2 ? t.get<float>(kDzMaxSlots) : nullptr;
    MIMO_TRY(t.ok());
    MIMO_TRY(split_pairs_launch(dz, dzs, (int64_t)n * h * wd, cout_p, st, amax, &a.dz_absmax_n));
    a.dz = dzs;
    a.dz_absmax = amax;
    if (amax) a.np = 2;
    MIMO_TRY(wgrad_split_launch(a, st));
  } else {
    MIMO_TRY(wgrad_launch(a, st));
  }
  if (!thin)
    MIMO_TRY(wgrad_reduce_launch(a.partial, a.splits, a.cin_pad, a.cout_pad, cm, cin_p, cin, cout, dw, st, a.dz_absmax, a.dz_absmax_n));
  if (dbias) {
    hipLaunchKernelGGL(colsum_naive_kernel, dim3(cout), dim3(256), 0, st, dz, (int64_t)n * h * wd, cout_p, cout, dbias);
    MIMO_KERNEL_CHECK();
  }
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_maxpool2x2(const float* x, float* y, int32_t n, int32_t h, int32_t w, int32_t c_p, mimo_stream stream) {
  MIMO_TRY(maxpool_fwd_launch(x, ST_F32, c_p, n, h, w, c_p, y, c_p, (hipStream_t)stream));
  return MIMO_OK;
}

int mimo_op_upsample_cat(const float* skip, const float* low, float* out, int32_t n, int32_t hs, int32_t ws, int32_t cs_p,
                         int32_t hl, int32_t wl, int32_t cl_p, mimo_stream stream) {
  MIMO_TRY(upcat_fwd_launch(skip, ST_F32, cs_p, cs_p, low, cl_p, cl_p, n, hs, ws, hl, wl, out, (hipStream_t)stream));
  return MIMO_OK;
}

}  // extern "C"

// ---- backward element-wise operators (tests/test_ew_bwd_kernels_gpu.py) --------------------------------------------------
// fp32 tensors at the interface; in the 16-bit storage modes whole buffers (every pixel at its full pitch) are rounded into
// 16-bit copies, the storage-mode kernels run on those, and the outputs are widened again (exact).

namespace {

bool bad_dims(const char* who, int n, int h, int w, int c_p) {
  if (n < 1 || h < 2 || w < 2 || c_p < 8 || c_p % 8 != 0 || (int64_t)n * (h + 2) * (w + 2) >= (int64_t)1 << 31) {
    set_error("%s: n %d, %d x %d, c_p %d unsupported (n >= 1, h and w >= 2 for the reflect fold, c_p a multiple of 8)", who, n, h, w, c_p);
    return true;
  }
  return false;
}
// a channel slice [off, off + c_p) of a buffer with `ld` elements per pixel, float4-addressable
bool bad_slice(const char* who, const char* what, int ld, int off, int c_p) {
  if (off < 0 || off % 4 != 0 || ld % 4 != 0 || ld < off + c_p) {
    set_error("%s: %s pitch %d / channel offset %d do not hold %d channels", who, what, ld, off, c_p);
    return true;
  }
  return false;
}
}  // namespace

extern "C" {

int mimo_op_fold_slice(const float* dxpad, int32_t ldp, int32_t choff, float* da, int32_t ldda, int32_t n, int32_t h,
                       int32_t w, int32_t c_p, int32_t accumulate, int32_t precision, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (bad_dims("mimo_op_fold_slice", n, h, w, c_p) || bad_slice("mimo_op_fold_slice", "dxpad", ldp, choff, c_p) ||
      bad_slice("mimo_op_fold_slice", "da", ldda, 0, c_p))
    return MIMO_ERR_INVALID;
  Temp t("mimo_op_fold_slice");
  Stored src, dst;
  MIMO_TRY(stage_in(t, dxpad, (int64_t)n * (h + 2) * (w + 2) * ldp, precision, st, &src));
  MIMO_TRY(stage_out(t, da, (int64_t)n * h * w * ldda, precision, st, &dst));
  MIMO_TRY(fold_slice_launch(src.in, store_type(precision), ldp, choff, dst.out, ldda, n, h, w, c_p, accumulate, st));
  MIMO_TRY(stage_back(dst, precision, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_pool_backward(const float* dxpad, int32_t ldp, int32_t choff, const float* a, int32_t lda, const float* skip,
                          int32_t ldsk, float* da, int32_t ldda, int32_t n, int32_t h, int32_t w, int32_t c_p,
                          int32_t accumulate, int32_t precision, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_pool_backward";
  // (the folded tensor is the pooled one: h / 2 x w / 2 needs two rows and columns)
  if (bad_dims(who, n, h / 2, w / 2, c_p) || bad_dims(who, n, h, w, c_p) || bad_slice(who, "dxpad", ldp, choff, c_p) ||
      bad_slice(who, "a", lda, 0, c_p) || bad_slice(who, "da", ldda, 0, c_p) || (skip && bad_slice(who, "skip", ldsk, 0, c_p)))
    return MIMO_ERR_INVALID;
  Temp t(who);
  Stored src, act, sk, dst;
  MIMO_TRY(stage_in(t, dxpad, (int64_t)n * (h / 2 + 2) * (w / 2 + 2) * ldp, precision, st, &src));
  MIMO_TRY(stage_in(t, a, (int64_t)n * h * w * lda, precision, st, &act));
  MIMO_TRY(stage_in(t, skip, (int64_t)n * (h + 2) * (w + 2) * ldsk, precision, st, &sk));
  MIMO_TRY(stage_out(t, da, (int64_t)n * h * w * ldda, precision, st, &dst));
  MIMO_TRY(pool_bwd_launch(src.in, store_type(precision), ldp, choff, act.in, lda, dst.out, ldda, n, h, w, c_p, accumulate, st,
                           sk.in, ldsk));
  MIMO_TRY(stage_back(dst, precision, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_up_backward(const float* dxpad, int32_t ldp, int32_t choff, float* da, int32_t ldda, int32_t n, int32_t hs,
                        int32_t ws, int32_t hl, int32_t wl, int32_t c_p, int32_t accumulate, int32_t precision,
                        mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_up_backward";
  if (bad_dims(who, n, hs, ws, c_p) || bad_slice(who, "dxpad", ldp, choff, c_p) || bad_slice(who, "da", ldda, 0, c_p))
    return MIMO_ERR_INVALID;
  if (hl < 1 || wl < 1 || hs / 2 != hl || ws / 2 != wl) {
    set_error("%s: %d x %d is not the x2 up-sampling of %d x %d (floor(hs / 2) == hl)", who, hs, ws, hl, wl);
    return MIMO_ERR_INVALID;
  }
  Temp t(who);
  Stored src, dst;
  MIMO_TRY(stage_in(t, dxpad, (int64_t)n * (hs + 2) * (ws + 2) * ldp, precision, st, &src));
  MIMO_TRY(stage_out(t, da, (int64_t)n * hl * wl * ldda, precision, st, &dst));
  MIMO_TRY(up_bwd_launch(src.in, store_type(precision), ldp, choff, dst.out, ldda, n, hs, ws, hl, wl, c_p, accumulate, st));
  MIMO_TRY(stage_back(dst, precision, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_bn_relu_backward(const mimo_op_bn_relu_backward_args* p, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_bn_relu_backward";
  if (!p) {
    set_error("%s: null arguments", who);
    return MIMO_ERR_INVALID;
  }
  const mimo_op_bn_relu_backward_args& a = *p;
  const int prec = a.precision, Cp = a.c_p, N = a.n, H = a.h, W = a.w;
  const bool fused = a.kind == GS_POOL || a.kind == GS_HEAD;
  if (bad_dims(who, N, H, W, Cp) || bad_slice(who, "z", a.ldz, 0, Cp)) return MIMO_ERR_INVALID;
  if (a.kind < GS_PLAIN || a.kind > GS_HEAD || a.c < 1 || a.c > Cp || !a.z || !a.scale || !a.shift || !a.mean || !a.invstd ||
      !a.dz || !a.c1 || !a.c2 || a.absmax_capacity < 0 || (a.absmax && (!a.absmax_n || a.absmax_capacity < kDzMaxSlots))) {
    set_error("%s: kind %d, c %d of %d, a missing tensor, or fewer than %d max |dz| slots", who, a.kind, a.c, Cp, kDzMaxSlots);
    return MIMO_ERR_INVALID;
  }
  if (fused && is_mixed(prec)) {
    set_error("%s: the pooled and head gradient sources exist for fp32 storage only", who);
    return MIMO_ERR_INVALID;
  }
  if (a.split_out && is_mixed(prec)) {
    set_error("%s: pair-split dz exists for fp32 storage only", who);
    return MIMO_ERR_INVALID;
  }
  if (!a.training && !a.dbias) {
    set_error("%s: eval mode returns the bias gradient", who);
    return MIMO_ERR_INVALID;
  }
  GradSrc src;
  src.kind = a.kind;
  Temp t(who);
  Stored gsrc, zs, dzs;
  float* head_partial = nullptr;
  if (a.kind == GS_PLAIN) {
    if (!a.da || bad_slice(who, "da", a.ldda, 0, Cp)) return MIMO_ERR_INVALID;
    MIMO_TRY(stage_in(t, a.da, (int64_t)N * H * W * a.ldda, prec, st, &gsrc));
    src.da = gsrc.in;
    src.ldda = a.ldda;
  } else if (a.kind == GS_FOLD) {  // (the folded source reads channels [0, c_p) of its buffer)
    if (!a.dxpad || a.choff != 0 || bad_slice(who, "dxpad", a.ldp, 0, Cp)) {
      set_error("%s: the folded source needs dxpad with choff 0 and a pitch of at least c_p", who);
      return MIMO_ERR_INVALID;
    }
    MIMO_TRY(stage_in(t, a.dxpad, (int64_t)N * (H + 2) * (W + 2) * a.ldp, prec, st, &gsrc));
    src.dxpad = gsrc.in;
    src.ldp = a.ldp;
  } else if (a.kind == GS_POOL) {
    if (!a.dxpad || bad_dims(who, N, H / 2, W / 2, Cp) || bad_slice(who, "dxpad", a.ldp, a.choff, Cp) ||
        (a.skip && bad_slice(who, "skip", a.ldsk, a.skoff, Cp)))
      return MIMO_ERR_INVALID;
    src.dxpad = a.dxpad;
    src.ldp = a.ldp;
    src.choff = a.choff;
    src.skip = a.skip;
    src.ldsk = a.ldsk;
    src.skoff = a.skoff;
  } else {
    if (a.head_co != 2 || !a.head_w || a.head_subnetworks < 1 || a.head_s < 0 || a.head_s >= a.head_subnetworks ||
        (!a.head_dout && !a.head_dloss) || (a.head_dloss && (!a.head_out || !a.head_label)) || !a.head_dw || !a.head_db ||
        (a.loss_kind != MIMO_LOSS_LAPLACE_NLL && a.loss_kind != MIMO_LOSS_GAUSSIAN_NLL)) {
      set_error("%s: the head source needs 2 logits per pixel, its weights, dout and / or dloss with logits and labels, dw and db", who);
      return MIMO_ERR_INVALID;
    }
    head_partial = t.get<float>((size_t)kBnReduceMaxBlocks * (2 * Cp + 2));
    MIMO_TRY(t.ok());
    HeadGrad& hg = src.head;
    hg.w = a.head_w;
    hg.C = a.c;
    hg.Co = 2;
    hg.N = N;
    hg.S = a.head_subnetworks;
    hg.s = a.head_s;
    hg.HW = H * W;
    hg.out = a.head_out;
    hg.dout = a.head_dout;
    hg.dloss = a.head_dloss;
    hg.label = a.head_label;
    hg.mask = a.head_mask;
    hg.perm = a.head_perm;
    hg.kind = a.loss_kind;
    hg.eps_min = a.eps_min;
    hg.eps_max = a.eps_max;
    hg.inv_count = 1.f / (float)((double)N * H * W);  // head_bwd_launch's: N * (Co / 2) * HW
    hg.partial = head_partial;
  }
  MIMO_TRY(stage_in(t, a.z, (int64_t)N * H * W * a.ldz, prec, st, &zs));
  MIMO_TRY(stage_out(t, a.dz, (int64_t)N * H * W * Cp, prec, st, &dzs));
  // (partial rows: one per workgroup of a BatchNorm-backward grid, <= kBnReduceMaxBlocks = the column-sum kernels' kColsumMaxRows)
  static_assert(kBnReduceMaxBlocks <= kColsumMaxRows, "partial-row capacity");
  float* partial = t.get<float>((size_t)kBnReduceMaxBlocks * 2 * Cp);
  int* status = t.get<int>(1);
  MIMO_TRY(t.ok());
  const int dt = store_type(prec);
  const BnReluLayer L = {zs.in, dt, a.ldz, dt, a.scale, a.shift, a.mean, a.invstd, a.c, Cp, N, H, W};
  int rows = 0;
  MIMO_TRY(bnrelu_bwd_reduce_launch(L, src, a.mask, partial, &rows, st));
  MIMO_TRY(bn_bwd_stats_launch(partial, rows, a.c, Cp, (int64_t)N * H * W, a.training ? 1 : 0, a.c1, a.c2, a.dgamma, a.dbeta,
                               a.training ? a.dbias : nullptr, status, st));
  if (a.kind == GS_HEAD) MIMO_TRY(head_bwd_stats_launch(head_partial, rows, a.c, Cp, 2, a.head_dw, a.head_db, st));
  int absmax_n = 0;
  MIMO_TRY(bn_bwd_apply_launch(L, src, a.mask, BnBwdApplyOut{a.c1, a.c2, dzs.out, a.split_out ? 1 : 0, a.training ? nullptr : partial,
                                                             &rows, a.absmax, &absmax_n, nullptr}, st));
  if (!a.training) MIMO_TRY(colsum_vec_launch(partial, rows, Cp, a.c, a.dbias, st));
  MIMO_TRY(stage_back(dzs, prec, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  if (a.absmax_n) *a.absmax_n = absmax_n;
  if (a.status) MIMO_HIP_CHECK(hipMemcpy(a.status, status, sizeof(int), hipMemcpyDeviceToHost));
  return MIMO_OK;
}

int mimo_op_head_backward(const mimo_op_head_backward_args* p, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_head_backward";
  if (!p) {
    set_error("%s: null arguments", who);
    return MIMO_ERR_INVALID;
  }
  const mimo_op_head_backward_args& a = *p;
  const int Cp = a.c_p;
  // (one workgroup column: the head's channel quads fit one workgroup, filter_base_count <= 256)
  if (a.n < 1 || a.hw < 1 || (int64_t)a.n * a.hw >= (int64_t)1 << 31 || Cp < 8 || Cp % 8 != 0 || Cp > 256 || a.c < 1 || a.c > Cp ||
      bad_slice(who, "a", a.lda, 0, Cp) || a.co < 2 || a.co > kMaxHeadOut || (a.co & 1) || a.subnetworks < 1 || a.s < 0 ||
      a.s >= a.subnetworks || !a.a || !a.w || !a.da || !a.dw || !a.db || (!a.dout && !a.dloss) ||
      (a.dloss && (!a.out || !a.label)) || (!a.in_scale != !a.in_shift) ||
      (a.loss_kind != MIMO_LOSS_LAPLACE_NLL && a.loss_kind != MIMO_LOSS_GAUSSIAN_NLL)) {
    set_error("%s: unsupported geometry or a missing tensor (c_p a multiple of 8 up to 256, an even co <= %d, dout and / or dloss "
              "with logits and labels)", who, kMaxHeadOut);
    return MIMO_ERR_INVALID;
  }
  Temp t(who);
  Stored act, dst;
  MIMO_TRY(stage_in(t, a.a, (int64_t)a.n * a.hw * a.lda, a.precision, st, &act));
  MIMO_TRY(stage_out(t, a.da, (int64_t)a.n * a.hw * Cp, a.precision, st, &dst));
  static_assert(kEwMaxBlocks <= kColsumMaxRows, "partial-row capacity");
  float* partial = t.get<float>((size_t)kEwMaxBlocks * (a.co * Cp + a.co));  // one row per workgroup, head_bwd_launch's grid cap
  MIMO_TRY(t.ok());
  int rows = 0;
  MIMO_TRY(head_bwd_launch(act.in, store_type(a.precision), a.lda, a.w, a.c, Cp, a.co, a.n, a.subnetworks, a.s, (int)a.hw, a.out, a.dout,
                           a.dloss, a.label, a.mask, a.perm, a.loss_kind, a.eps_min, a.eps_max, dst.out, partial, &rows, st,
                           a.in_scale, a.in_shift));
  MIMO_TRY(head_bwd_stats_launch(partial, rows, a.c, Cp, a.co, a.dw, a.db, st));
  MIMO_TRY(stage_back(dst, a.precision, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

}  // extern "C"

// ---- forward element-wise operators (tests/test_ew_fwd_kernels_gpu.py) -----------------------------------------------------
// The conventions of the backward block: fp32 at the interface, whole buffers rounded at their pitch in the 16-bit modes.

namespace {

// dimensions of a forward operator (no reflect fold: one row or column is a tensor)
bool bad_fwd_dims(const char* who, int n, int h, int w, int c_p) {
  if (n < 1 || h < 1 || w < 1 || c_p < 8 || c_p % 8 != 0 || (int64_t)n * h * w >= (int64_t)1 << 31) {
    set_error("%s: n %d, %d x %d, c_p %d unsupported (n, h, w >= 1, n h w < 2^31, c_p a multiple of 8)", who, n, h, w, c_p);
    return true;
  }
  return false;
}
bool bad_precision(const char* who, int precision) {
  if (precision != MIMO_PREC_FP32 && !is_mixed(precision)) {
    set_error("%s: precision %d (fp32, bf16-mixed or 16-mixed storage)", who, precision);
    return true;
  }
  return false;
}
// a device permutation [rows][n]: every entry of row s (all rows: s < 0) in [0, n)
int bad_perm(const char* who, const int64_t* perm, int rows, int s, int n, hipStream_t st, bool* bad) {
  *bad = false;
  if (!perm) return MIMO_OK;
  const int r0 = s < 0 ? 0 : s, nr = s < 0 ? rows : 1;
  std::vector<int64_t> h((size_t)nr * n);
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  MIMO_HIP_CHECK(hipMemcpy(h.data(), perm + (size_t)r0 * n, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int64_t v : h)
    if (v < 0 || v >= n) {
      set_error("%s: permutation entry %lld outside [0, %d)", who, (long long)v, n);
      *bad = true;
      break;
    }
  return MIMO_OK;
}
int read_status(const int* dev, int32_t* host) {
  if (host) MIMO_HIP_CHECK(hipMemcpy(host, dev, sizeof(int), hipMemcpyDeviceToHost));
  return MIMO_OK;
}

}  // namespace

extern "C" {

int mimo_op_bn_stats(const mimo_op_bn_stats_args* p, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_bn_stats";
  if (!p) {
    set_error("%s: null arguments", who);
    return MIMO_ERR_INVALID;
  }
  const mimo_op_bn_stats_args& a = *p;
  if (a.c < 1 || a.c > a.c_p || a.c_p % 8 != 0 || a.cout_pad % 8 != 0 || a.c_p > a.cout_pad || !a.gamma || !a.beta || !a.running_mean ||
      !a.running_var || !a.mean || !a.invstd || !a.scale || !a.shift ||
      (a.training && (!a.partial || a.rows < 1 || a.count < 1 || a.route < MIMO_BN_ROUTE_PLAN || a.route > MIMO_BN_ROUTE_ROWSUM ||
                      (a.route == MIMO_BN_ROUTE_ONE_LAUNCH && a.rows > kColsumMaxRows)))) {
    set_error("%s: c %d of c_p %d of cout_pad %d, rows %d, count %lld, route %d (one launch: rows <= %d) or a missing tensor", who, a.c,
              a.c_p, a.cout_pad, a.rows, (long long)a.count, a.route, kColsumMaxRows);
    return MIMO_ERR_INVALID;
  }
  Temp t(who);
  int* status = t.get<int>(1);
  double* sums = t.get<double>((size_t)kMaxChunks * 2 * a.cout_pad);
  MIMO_TRY(t.ok());
  if (!a.training) {
    MIMO_TRY(bn_eval_prepare_launch(a.c, a.c_p, a.gamma, a.beta, a.running_mean, a.running_var, a.eps, a.mean, a.invstd, a.scale,
                                    a.shift, st, status));
  } else if (a.route == MIMO_BN_ROUTE_ONE_LAUNCH || (a.route == MIMO_BN_ROUTE_PLAN && a.rows <= kColsumMaxRows)) {
    MIMO_TRY(bn_fwd_stats_launch(a.partial, a.rows, a.cout_pad, a.c, a.c_p, a.count, a.gamma, a.beta, a.running_mean, a.running_var,
                                 a.momentum, a.eps, a.mean, a.invstd, a.scale, a.shift, status, st));
  } else {
    int chunks = 0;
    MIMO_TRY(rowsum_launch(a.partial, a.rows, 2 * a.cout_pad, sums, &chunks, st));
    MIMO_TRY(bn_fwd_finalize_launch(sums, chunks, a.cout_pad, a.c, a.c_p, a.count, a.gamma, a.beta, a.running_mean, a.running_var,
                                    a.momentum, a.eps, a.mean, a.invstd, a.scale, a.shift, status, st));
  }
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return read_status(status, a.status);
}

int mimo_op_bn_relu_forward(const mimo_op_bn_relu_forward_args* p, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_bn_relu_forward";
  if (!p) {
    set_error("%s: null arguments", who);
    return MIMO_ERR_INVALID;
  }
  const mimo_op_bn_relu_forward_args& a = *p;
  const int Cp = a.c_p;
  if (bad_fwd_dims(who, a.n, a.h, a.w, Cp) || bad_precision(who, a.precision) || bad_slice(who, "z", a.ldz, 0, Cp) ||
      bad_slice(who, "a", a.lda, 0, Cp))
    return MIMO_ERR_INVALID;
  if (a.c < 1 || a.c > Cp || !a.z || !a.scale || !a.shift || !a.a) {
    set_error("%s: c %d of %d or a missing tensor", who, a.c, Cp);
    return MIMO_ERR_INVALID;
  }
  if (a.pool && (bad_dims(who, a.n, a.h, a.w, Cp) || bad_slice(who, "pool", a.ldpool, 0, Cp))) return MIMO_ERR_INVALID;
  const int prec = a.precision, zprec = a.z_fp32 ? (int)MIMO_PREC_FP32 : prec;
  const int64_t P = (int64_t)a.n * a.h * a.w;
  Temp t(who);
  Stored zs, as, ps;
  int* status = t.get<int>(1);
  MIMO_TRY(t.ok());
  MIMO_TRY(stage_in(t, a.z, P * a.ldz, zprec, st, &zs));
  MIMO_TRY(stage_out(t, a.a, P * a.lda, prec, st, &as));
  // (the forward passes read neither mean nor invstd)
  const BnReluLayer L = {zs.in, store_type(zprec), a.ldz, store_type(prec), a.scale, a.shift, nullptr, nullptr, a.c, Cp, a.n, a.h, a.w};
  if (a.pool) {
    MIMO_TRY(stage_out(t, a.pool, (int64_t)a.n * (a.h / 2) * (a.w / 2) * a.ldpool, prec, st, &ps));
    MIMO_TRY(bn_relu_pool_fwd_launch(L, a.mask, as.out, a.lda, ps.out, a.ldpool, status, st));
    MIMO_TRY(stage_back(ps, prec, st));
  } else {
    MIMO_TRY(bn_relu_fwd_launch(L, a.mask, as.out, a.lda, status, st));
  }
  MIMO_TRY(stage_back(as, prec, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return read_status(status, a.status);
}

int mimo_op_maxpool2x2_ex(const float* x, int32_t lda, float* y, int32_t ldo, int32_t n, int32_t h, int32_t w, int32_t c_p,
                          int32_t precision, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_maxpool2x2_ex";
  if (bad_dims(who, n, h, w, c_p) || bad_precision(who, precision) || bad_slice(who, "x", lda, 0, c_p) ||
      bad_slice(who, "y", ldo, 0, c_p))
    return MIMO_ERR_INVALID;
  if (!x || !y) {
    set_error("%s: a missing tensor", who);
    return MIMO_ERR_INVALID;
  }
  Temp t(who);
  Stored src, dst;
  MIMO_TRY(stage_in(t, x, (int64_t)n * h * w * lda, precision, st, &src));
  MIMO_TRY(stage_out(t, y, (int64_t)n * (h / 2) * (w / 2) * ldo, precision, st, &dst));
  MIMO_TRY(maxpool_fwd_launch(src.in, store_type(precision), lda, n, h, w, c_p, dst.out, ldo, st));
  MIMO_TRY(stage_back(dst, precision, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_upsample_cat_ex(const float* skip, int32_t lds, const float* low, int32_t ldl, const float* lo_scale,
                            const float* lo_shift, float* out, int32_t n, int32_t hs, int32_t ws, int32_t cs_p, int32_t hl,
                            int32_t wl, int32_t cl_p, int32_t precision, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_upsample_cat_ex";
  if (bad_fwd_dims(who, n, hs, ws, cs_p) || bad_fwd_dims(who, n, hl, wl, cl_p) || bad_precision(who, precision) ||
      bad_slice(who, "low", ldl, 0, cl_p) || (skip && bad_slice(who, "skip", lds, 0, cs_p)))
    return MIMO_ERR_INVALID;
  if (hs < 2 * hl || ws < 2 * wl || !low || !out || (!lo_scale != !lo_shift)) {
    set_error("%s: %d x %d is smaller than twice %d x %d, a missing tensor, or only one of lo_scale / lo_shift", who, hs, ws, hl, wl);
    return MIMO_ERR_INVALID;
  }
  Temp t(who);
  Stored sk, lo, dst;
  MIMO_TRY(stage_in(t, skip, (int64_t)n * hs * ws * lds, precision, st, &sk));
  MIMO_TRY(stage_in(t, low, (int64_t)n * hl * wl * ldl, precision, st, &lo));
  MIMO_TRY(stage_out(t, out, (int64_t)n * hs * ws * (cs_p + cl_p), precision, st, &dst));
  MIMO_TRY(upcat_fwd_launch(sk.in, store_type(precision), lds, cs_p, lo.in, ldl, cl_p, n, hs, ws, hl, wl, dst.out, st, lo_scale, lo_shift));
  MIMO_TRY(stage_back(dst, precision, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_head_forward(const mimo_op_head_forward_args* p, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_head_forward";
  if (!p) {
    set_error("%s: null arguments", who);
    return MIMO_ERR_INVALID;
  }
  const mimo_op_head_forward_args& a = *p;
  if (a.c < 1 || a.c > 256 || a.co < 1 || a.co > kMaxHeadOut || a.n < 1 || a.hw < 1 || (int64_t)a.n * a.hw >= (int64_t)1 << 31 ||
      a.subnetworks < 1 || a.s < 0 || a.s >= a.subnetworks || !a.a || !a.w || !a.bias || !a.out || (!a.in_scale != !a.in_shift) ||
      bad_precision(who, a.precision)) {
    set_error("%s: c %d (1..256), co %d (1..%d), n %d, hw %d, subnetwork %d of %d, a missing tensor or only one of in_scale / in_shift",
              who, a.c, a.co, kMaxHeadOut, a.n, a.hw, a.s, a.subnetworks);
    return MIMO_ERR_INVALID;
  }
  if (bad_slice(who, "a", a.lda, 0, pad_channels(a.c))) return MIMO_ERR_INVALID;
  Temp t(who);
  Stored act;
  int* status = t.get<int>(1);
  MIMO_TRY(t.ok());
  MIMO_TRY(stage_in(t, a.a, (int64_t)a.n * a.hw * a.lda, a.precision, st, &act));
  MIMO_TRY(head_fwd_launch(act.in, store_type(a.precision), a.lda, a.w, a.bias, a.c, a.co, a.n, a.subnetworks, a.s, a.hw, a.out, st,
                           status, a.in_scale, a.in_shift));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return read_status(status, a.status);
}

int mimo_op_loss_forward(const float* out, const float* label, const float* mask, const int64_t* perm, int32_t n,
                         int32_t subnetworks, int32_t co, int32_t hw, int32_t loss_kind, float eps_min, float eps_max,
                         float* loss, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_loss_forward";
  if (co < 2 || co > kMaxHeadOut || (co & 1) || n < 1 || hw < 1 || subnetworks < 1 || (int64_t)n * hw >= (int64_t)1 << 31 || !out ||
      !label || !loss || (loss_kind != MIMO_LOSS_LAPLACE_NLL && loss_kind != MIMO_LOSS_GAUSSIAN_NLL)) {
    set_error("%s: co %d (even, 2..%d), n %d, hw %d, %d subnetworks, loss kind %d or a missing tensor", who, co, kMaxHeadOut, n, hw,
              subnetworks, loss_kind);
    return MIMO_ERR_INVALID;
  }
  bool bad = false;
  MIMO_TRY(bad_perm(who, perm, subnetworks, -1, n, st, &bad));
  if (bad) return MIMO_ERR_INVALID;
  Temp t(who);
  float* partial = t.get<float>((size_t)subnetworks * 512);  // loss_fwd_launch's grid cap
  MIMO_TRY(t.ok());
  int blocks = 0;
  MIMO_TRY(loss_fwd_launch(out, label, mask, perm, n, subnetworks, co, hw, loss_kind, eps_min, eps_max, partial, &blocks, st));
  MIMO_TRY(loss_finalize_launch(partial, subnetworks, blocks, (double)n * (co / 2) * hw, loss, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_pack_input(const float* x, int64_t x_count, int64_t stride_n, int64_t stride_s, const int64_t* perm, int32_t s,
                       int32_t n, int32_t c, int32_t h, int32_t w, float* out, int32_t cp, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_pack_input";
  const int64_t hw = (int64_t)h * w;
  if (n < 1 || h < 1 || w < 1 || (int64_t)n * hw >= (int64_t)1 << 31 || c < 1 || c > cp || cp % 4 != 0 || s < 0 || stride_n < 0 ||
      stride_s < 0 || !x || !out || (int64_t)(n - 1) * stride_n + (int64_t)s * stride_s + (int64_t)c * hw > x_count) {
    set_error("%s: n %d, %d x %d, c %d of %d, subnetwork %d, strides %lld / %lld do not fit %lld elements", who, n, h, w, c, cp, s,
              (long long)stride_n, (long long)stride_s, (long long)x_count);
    return MIMO_ERR_INVALID;
  }
  bool bad = false;
  MIMO_TRY(bad_perm(who, perm, s + 1, s, n, st, &bad));
  if (bad) return MIMO_ERR_INVALID;
  MIMO_TRY(pack_input_launch(x, stride_n, stride_s, perm, s, n, c, h, w, out, cp, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_unpack_dx(const float* dxpad, int32_t ldp, int32_t n, int32_t subnetworks, int32_t s, int32_t c, int32_t h,
                      int32_t w, int32_t precision, float* dx, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_unpack_dx";
  if (c < 1 || bad_dims(who, n, h, w, 8) || bad_precision(who, precision) || bad_slice(who, "dxpad", ldp, 0, round_up(c, 4)))
    return MIMO_ERR_INVALID;
  if (subnetworks < 1 || s < 0 || s >= subnetworks || !dxpad || !dx) {
    set_error("%s: subnetwork %d of %d or a missing tensor", who, s, subnetworks);
    return MIMO_ERR_INVALID;
  }
  Temp t(who);
  Stored src;
  MIMO_TRY(stage_in(t, dxpad, (int64_t)n * (h + 2) * (w + 2) * ldp, precision, st, &src));
  MIMO_TRY(unpack_dx_launch(src.in, store_type(precision), ldp, n, subnetworks, s, c, h, w, dx, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_fold_image_grad(const float* dxpad, int32_t ldp, int32_t n, int32_t c, int32_t h, int32_t w, float* dimage,
                            int32_t accumulate, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_fold_image_grad";
  if (c < 1 || bad_dims(who, n, h, w, 8) || bad_slice(who, "dxpad", ldp, 0, round_up(c, 4))) return MIMO_ERR_INVALID;
  if (!dxpad || !dimage) {
    set_error("%s: a missing tensor", who);
    return MIMO_ERR_INVALID;
  }
  MIMO_TRY(fold_image_grad_launch(dxpad, ldp, n, c, h, w, dimage, accumulate, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

int mimo_op_fold_image_grad_mc(const float* dxpad, int32_t ldp, int32_t n, int32_t replicas, int32_t c, int32_t h, int32_t w,
                               float* dimage, int32_t accumulate, mimo_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "mimo_op_fold_image_grad_mc";
  if (c < 1 || bad_dims(who, n, h, w, 8) || bad_slice(who, "dxpad", ldp, 0, round_up(c, 4))) return MIMO_ERR_INVALID;
  if (replicas < 1 || n % replicas != 0) {
    set_error("%s: replicas %d does not divide n %d", who, replicas, n);
    return MIMO_ERR_INVALID;
  }
  if (!dxpad || !dimage) {
    set_error("%s: a missing tensor", who);
    return MIMO_ERR_INVALID;
  }
  MIMO_TRY(fold_image_grad_mc_launch(dxpad, ldp, n / replicas, replicas, c, h, w, dimage, accumulate, st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  return MIMO_OK;
}

}  // extern "C"
