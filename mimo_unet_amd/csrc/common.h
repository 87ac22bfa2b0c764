// Shared host/device helpers of libmimo_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/mimo_hip.h"
#include "conv_launch.h"

namespace mimo {

void set_error(const char* fmt, ...);

#define MIMO_HIP_CHECK(expr)                                                                          \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      ::mimo::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);   \
      return MIMO_ERR_HIP;                                                                            \
    }                                                                                                 \
  } while (0)
#define MIMO_KERNEL_CHECK() MIMO_HIP_CHECK(hipGetLastError())
#define MIMO_TRY(expr)            \
  do {                            \
    int rc_ = (expr);             \
    if (rc_ != MIMO_OK) return rc_; \
  } while (0)

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Channel padding of every NHWC activation tensor (floats per pixel).
static inline int pad_channels(int c) { return round_up(c, 8); }

constexpr int kWave = 64;

static inline int store_bytes(int dt) { return dt == ST_F32 ? 4 : 2; }

// Workgroups are dealt round-robin to the 8 XCDs (each with a private L2) in linear-id order.  This maps a
// linear workgroup id to a "virtual" index such that every XCD owns one CONTIGUOUS range of virtual indices
// (any total, bijective): kernels then decode the virtual index so that workgroups which read the same
// operand tiles (the channel tiles of one pixel tile; neighbouring pixel tiles sharing halo rows) are
// neighbours in virtual order and therefore meet in one L2 instead of eight.
__device__ __forceinline__ int xcd_virtual_index(int linear, int total) {
  return sched::xcd_virtual_index(linear, total);  // tile_sched.h: host-testable
}

// ------------------------------------------------------------------ conv3x3 (conv3x3.hip)
// (ConvLaunch, the "forward-type" 3x3 correlation all of these run: conv_launch.h)
// power-of-two scale of a layer's fp16 weight image from the float bits of its max |w| (tile_sched.h: host-testable)
__host__ __device__ __forceinline__ float w16_scale(unsigned wmax_bits, bool inverse) { return sched::w16_scale(wmax_bits, inverse); }

// K split of a launch by cost (1 = none): few pixel tiles and a long K walk — the 16x16 / 32x32 layers at a few images per
// GPU — finish sooner as wide channel tiles on ksplit x the workgroups plus one reduction pass than as narrow channel tiles
// whose every phase is mostly fixed cost.  MIMO_CONV_KSPLIT: 0 = never, n >= 2 = n wherever the geometry allows (tests).
int conv3x3_ksplit(int mode, int N, int cin_p, int cout_pad, int Ho, int Wo);
// conv3x3_bf16x3_launch with the K split of conv3x3_ksplit when kpart (>= kpart_floats floats of scratch) can hold its
// slabs: the partial launch, then out = bias + sum of the slabs with the BatchNorm partial rows (forward) in one pass
int conv3x3_bf16x3_launch_k(const ConvLaunch& a, int mode, int* rows, hipStream_t stream, float* kpart, size_t kpart_floats);
// 1 when conv3x3_bf16x3_launch(mode) runs this launch on a kernel whose loaders can apply ConvLaunch::in_scale / in_shift
int conv3x3_split_fuses_input(int mode, int wide, int Ho, int Wo);
// returns number of partial-stat rows (spatial blocks) through *rows when stats != nullptr
int conv3x3_launch(const ConvLaunch& a, int* rows, hipStream_t stream);
// plain-FMA kernels for the image convolution (conv_thin.hip; cin = the logical input channels, 1..4, stored in channels
// [0, cin) of x): the forward on the same ConvLaunch (a.w, the inference epilogue, one BatchNorm partial row per workgroup),
// and the weight gradient from an fp32 dz into torch's OIHW layout (partial: wgrad_thin_scratch floats)
int conv3x3_thin_ok(int cin, int cout_p);
int conv3x3_thin_launch(const ConvLaunch& a, int cin, int* rows, hipStream_t stream);
size_t wgrad_thin_scratch(int cin, int cout_p);
int wgrad_thin_ok(int cin, int cout_p, int N, int H, int W);  // the weight gradient too (few channels, many tiles)
int wgrad_thin_launch(const float* x, int ldx, const float* dz, int lddz, int N, int H, int W, int cin, int cout, int cout_p,
                      float* partial, float* dw, hipStream_t stream);
// split 16-bit variant (conv_bf16x3.hip): same ConvLaunch, reads a.wpk instead of a.w.
// mode 0: split16 data gradient (bf16 pairs, pre-split input); 1: split16 forward (fp16 pairs);
// 2: bf16 forward (one MFMA per product); 3: bf16 data gradient
int conv3x3_bf16x3_launch(const ConvLaunch& a, int mode, int* rows, hipStream_t stream);
int conv3x3_wide_stat_rows();
int conv3x3_wide_launch(const ConvLaunch& a, int mode, int* rows, hipStream_t stream);
int conv3x3_pick_nfrag(int cout);            // fragments (of 16 output channels) per workgroup
int conv3x3_cout_pad(int cout);              // packed weight rows for that choice
int conv3x3_stat_rows(int N, int Ho, int Wo);  // spatial workgroups == partial-stat rows
int conv3x3_ws_stat_rows(int N, int Ho, int Wo);  // same for the wave-specialised split kernel (4 rows per tile)

// 256 bytes of zeros in device memory: masked-out tile elements are LOADED from here instead of being
// selected to zero after the load — a select on the loaded value makes the compiler wait for the load
// right where it was issued, which silently removes a register prefetch.
static __device__ __attribute__((aligned(256))) float kZeroPage[64];  // zero-initialised, never written

// the power of two that scales dz in the two-MFMA weight gradient, from the float bits of max |dz| (tile_sched.h: host-testable)
__host__ __device__ __forceinline__ float wg_dz_scale(unsigned absmax_bits, bool inverse) { return sched::wg_dz_scale(absmax_bits, inverse); }
#if defined(__HIPCC__)
// max of the n per-workgroup maxima, computed redundantly by every wave that calls it (n <= kDzMaxSlots floats, L2-resident:
// n / 64 coalesced loads per lane and a butterfly) — no hot word that thousands of waves would queue on
__device__ __forceinline__ float wg_dz_absmax(const float* __restrict__ slots, int n) {
  float m = 0.f;
  for (int i = (int)(threadIdx.x & 63); i < n; i += 64) m = fmaxf(m, slots[i]);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
  return m;
}
#endif
int wgrad_launch(const WgradLaunch& a, hipStream_t stream);

// The switches and the device as conv_recipe (conv_recipe.h) takes them, each read where its kernels read it
bool conv_ws_enabled();
int conv_ksplit_force();
int conv_wide_force();
bool wgrad_ws_enabled();
bool wgrad_np2_enabled();
// (conv3x3_thin_ok queries the device once per process for the plain-FMA kernels' occupancy, whether or not a thin layer follows)
static inline ConvEnv conv_env(int wg_cus) {
  return ConvEnv{conv3x3_thin_ok(1, 8) != 0, conv_ws_enabled(), conv_wide_force(), conv_ksplit_force(), wgrad_ws_enabled(), wgrad_np2_enabled(), wg_cus};
}
// The CUs the weight-gradient launches are sized for (ConvEnv::wg_cus): MIMO_WGRAD_CUS where it holds a value of 8..256, else
// `sized_for` — the plan's sched::wg_side_cus, the whole chip (256) for a per-operator entry point.  Read per plan / call, as
// MIMO_WGRAD_NP is, so that the entry points can run the split counts a plan of any size runs.
static inline int wgrad_cus(int sized_for) {
  const char* e = getenv("MIMO_WGRAD_CUS");
  const int v = e ? atoi(e) : 0;
  return (v >= 8 && v <= 256) ? v : sized_for;
}
// 1 when wgrad_split_launch runs this geometry on a kernel that can apply WgradLaunch::in_scale / in_shift in its loader
int wgrad_split_fuses_input(int cin_p, int cout_p, int store, int np);
// split-bf16 variant (wgrad_split.hip): cin_pad / cout_pad must be multiples of its (CI, CO) tile
int wgrad_split_launch(const WgradLaunch& a, hipStream_t stream);
// extra floats the reduction needs behind the splits*9*cin_pad*cout_pad partial slabs
size_t wgrad_reduce_scratch(int splits, int cin_pad, int cout_pad);
// dW[co][ci][kh][kw] (torch OIHW) = sum over splits of partial[..][tap][cin_map^-1(ci)][co]
// dz_absmax != nullptr: the slabs carry the factor wg_dz_scale(*dz_absmax) (WgradLaunch::np == 2), removed here
int wgrad_reduce_launch(const float* partial, int splits, int cin_pad, int cout_pad, const int* cin_map,
                        int cin_p, int cin, int cout, float* dw, hipStream_t stream, const float* dz_absmax = nullptr,
                        int dz_absmax_n = 0, hipEvent_t done = nullptr);  // done: recorded when the reduction completes

// All weight repacks of a step in ONE launch (a per-layer launch each cost more in dispatch gaps than in work): a device
// table of PackJob records (pack_layout.h: the layouts and the builder of a job), blockIdx.y = job.
int pack_jobs_launch(const PackJob* jobs_dev, int njobs, int max_total, const float* params, hipStream_t stream);
// max |w| of every job with a wmax word (run in front of pack_jobs_launch, on words the caller has zeroed: the maximum of
// THIS pack).  status != nullptr: bit 0 (kStatusFwdStats) is OR-ed in when a maximum is not finite
int wabsmax_jobs_launch(const PackJob* jobs_dev, int njobs, int max_total, const float* params, hipStream_t stream,
                        int* status = nullptr);

}  // namespace mimo
