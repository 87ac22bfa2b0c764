// Colourised image grids of a log event, gfx950.
//
// Replaces, for every panel of a log event in one call, what the reference's OutputMonitor does per panel
// (mimo/tasks/depth/callbacks.py:21-48, mimo/tasks/sen12tp/callbacks.py:15-48): slice the first images of a step-output
// map, torchvision.utils.make_grid (one fill and one copy per image), colorize (mimo/visualization.py:9-49: normalise on
// the device, a synchronous copy of the fp32 grid to the host, a matplotlib colormap there).  Here the source maps are read
// where the step left them (<= 8 B per pixel with a mask) and the coloured [Hg, Wg, 3] uint8 image is written (3 B per
// pixel); what crosses to the host afterwards is the image, at the caller's leisure.
//
// Semantics (include/mimo_hip.h states them in full): make_grid's layout with zeros outside the images, an optional mask
// multiplied in, an optional |x|, the range fixed or taken over the WHOLE grid (torch.min / torch.max: NaN wins), three
// separately rounded fp32 operations t = (v - vmin) / (vmax - vmin), u = t * 256, and matplotlib's lookup rule on u.
//
// Launches: one.  A panel with an automatic bound adds one reduction launch in front: 128 workgroups per panel write their
// (min, max, saw-a-NaN) to the caller's scratch with plain stores, and every workgroup of the colouring launch folds its
// panel's 128 rows itself — no atomics, and min / max of non-NaN values do not depend on the order.
//
// Stores: the image of a panel is one contiguous run of 3 * Hg * Wg bytes, so four pixels that are neighbours in that run
// (neighbours in a row, or the end of one row and the head of the next) are 12 bytes at a multiple of 12: three whole
// dwords whenever the image starts on a dword.  A thread owns such a quad; the last Hg * Wg % 4 pixels of the image, and
// every pixel of an image that does not start on a dword, go out as bytes.
#include <algorithm>
#include <cstdint>

#include "common.h"

namespace mimo {
namespace {

constexpr int kMonMaxPanels = MIMO_MONITOR_MAX_PANELS;
constexpr int kMonThreads = 256;
constexpr int kMonPartials = 128;  // workgroups per panel of the reduction launch == rows the colouring launch folds
constexpr int kLutEntries = 257;   // 256 colours + the colour of a NaN

struct MonPanel {
  const float* src;   // first drawn channel of image 0
  const float* mask;  // likewise, or nullptr
  const uint32_t* lut;
  uint8_t* out;
  int64_t src_stride, mask_stride;  // floats between two images
  uint32_t h, w, hw, count;
  uint32_t xmaps, cell_h, cell_w, pad;  // cell = image + padding; count == 1: xmaps 1, pad 0, cells = the image
  uint32_t wg, npix;                    // grid width, grid pixels (< 2^31)
  int32_t flags, has_zero;              // has_zero: the grid holds pixels outside every image
  float vmin, vmax;
};
struct MonTable {
  MonPanel p[kMonMaxPanels];
};

enum { kMonAbs = MIMO_MONITOR_ABS, kMonAutoMin = MIMO_MONITOR_AUTO_VMIN, kMonAutoMax = MIMO_MONITOR_AUTO_VMAX };

__device__ __forceinline__ float mon_value(const MonPanel& P, uint32_t k, uint32_t r) {
  float v = P.src[(int64_t)k * P.src_stride + r];
  if (P.mask) v = __fmul_rn(v, P.mask[(int64_t)k * P.mask_stride + r]);
  return (P.flags & kMonAbs) ? fabsf(v) : v;
}

// value of grid pixel (y, x): an image pixel, or 0 between the images and in the empty cells of a ragged last row
__device__ __forceinline__ float mon_grid_value(const MonPanel& P, uint32_t y, uint32_t x) {
  const uint32_t ty = y / P.cell_h, ry = y - ty * P.cell_h;
  const uint32_t tx = x / P.cell_w, rx = x - tx * P.cell_w;
  const uint32_t k = ty * P.xmaps + tx;
  if (ry < P.pad || rx < P.pad || tx >= P.xmaps || k >= P.count) return 0.f;
  return mon_value(P, k, (ry - P.pad) * P.w + (rx - P.pad));
}

// colorize's normalisation and Colormap.__call__'s index, every operation rounded on its own
__device__ __forceinline__ uint32_t mon_colour(float v, float vmin, float vmax, const uint32_t* lut) {
  float t;
  if (vmin != vmax)
    t = __fdiv_rn(__fsub_rn(v, vmin), __fsub_rn(vmax, vmin));
  else
    t = __fmul_rn(v, 0.0f);
  const float u = __fmul_rn(t, 256.0f);
  int i;
  if (u != u)
    i = 256;
  else if (u < 0.f)
    i = 0;
  else if (u > 255.f)
    i = 255;  // u == 256 and everything above, +inf included
  else
    i = (int)u;
  return lut[i];
}

// rows of the reduction in scratch: [panel][min | max | nan][kMonPartials]
__device__ __forceinline__ float* mon_rows(float* scratch, int panel) { return scratch + (size_t)panel * 3 * kMonPartials; }

__global__ __launch_bounds__(kMonThreads) void monitor_range_kernel(MonTable tab, float* __restrict__ scratch) {
  const MonPanel& P = tab.p[blockIdx.y];
  if (!(P.flags & (kMonAutoMin | kMonAutoMax))) return;  // the whole workgroup
  float lo = INFINITY, hi = -INFINITY;
  int nan = 0;
  const uint32_t total = P.count * P.hw;
  for (uint32_t i = blockIdx.x * kMonThreads + threadIdx.x; i < total; i += kMonPartials * kMonThreads) {
    const uint32_t k = i / P.hw;
    const float v = mon_value(P, k, i - k * P.hw);
    nan |= v != v;
    lo = v < lo ? v : lo;  // a NaN compares false and is carried by the flag
    hi = v > hi ? v : hi;
  }
  if (P.has_zero && blockIdx.x == 0 && threadIdx.x == 0) {
    lo = 0.f < lo ? 0.f : lo;
    hi = 0.f > hi ? 0.f : hi;
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    lo = fminf(lo, __shfl_xor(lo, d));
    hi = fmaxf(hi, __shfl_xor(hi, d));
    nan |= __shfl_xor(nan, d);
  }
  __shared__ float s_lo[kMonThreads / kWave], s_hi[kMonThreads / kWave];
  __shared__ int s_nan[kMonThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_lo[threadIdx.x / kWave] = lo;
    s_hi[threadIdx.x / kWave] = hi;
    s_nan[threadIdx.x / kWave] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kMonThreads / kWave; ++i) {
      lo = fminf(lo, s_lo[i]);
      hi = fmaxf(hi, s_hi[i]);
      nan |= s_nan[i];
    }
    float* rows = mon_rows(scratch, blockIdx.y);
    rows[blockIdx.x] = lo;
    rows[kMonPartials + blockIdx.x] = hi;
    rows[2 * kMonPartials + blockIdx.x] = nan ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(kMonThreads) void monitor_grid_kernel(MonTable tab, const float* __restrict__ scratch) {
  const MonPanel& P = tab.p[blockIdx.y];
  __shared__ uint32_t s_lut[kLutEntries];
  __shared__ float s_lo[kMonPartials], s_hi[kMonPartials], s_nan[kMonPartials];
  for (int i = threadIdx.x; i < kLutEntries; i += kMonThreads) s_lut[i] = P.lut[i] & 0xFFFFFFu;
  float vmin = P.vmin, vmax = P.vmax;
  if (P.flags & (kMonAutoMin | kMonAutoMax)) {  // the whole workgroup: fold the panel's rows, every workgroup for itself
    static_assert(kMonPartials <= kMonThreads, "one row per thread");
    const float* rows = scratch + (size_t)blockIdx.y * 3 * kMonPartials;
    if (threadIdx.x < kMonPartials) {
      s_lo[threadIdx.x] = rows[threadIdx.x];
      s_hi[threadIdx.x] = rows[kMonPartials + threadIdx.x];
      s_nan[threadIdx.x] = rows[2 * kMonPartials + threadIdx.x];
    }
    __syncthreads();
    for (int off = kMonPartials / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) {
        s_lo[threadIdx.x] = fminf(s_lo[threadIdx.x], s_lo[threadIdx.x + off]);
        s_hi[threadIdx.x] = fmaxf(s_hi[threadIdx.x], s_hi[threadIdx.x + off]);
        s_nan[threadIdx.x] = fmaxf(s_nan[threadIdx.x], s_nan[threadIdx.x + off]);
      }
      __syncthreads();
    }
    const bool nan = s_nan[0] != 0.f;
    if (P.flags & kMonAutoMin) vmin = nan ? NAN : s_lo[0];
    if (P.flags & kMonAutoMax) vmax = nan ? NAN : s_hi[0];
  } else {
    __syncthreads();
  }

  const bool dwords = ((uintptr_t)P.out & 3) == 0;
  const uint32_t quads = dwords ? P.npix >> 2 : 0;
  // quad q: pixels 4 q .. 4 q + 3 of the run, 12 bytes at out + 12 q
  for (uint32_t q = blockIdx.x * kMonThreads + threadIdx.x; q < quads; q += gridDim.x * kMonThreads) {
    uint32_t y = (4 * q) / P.wg, x = 4 * q - y * P.wg;
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = mon_colour(mon_grid_value(P, y, x), vmin, vmax, s_lut);
      if (++x == P.wg) x = 0, ++y;
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(P.out) + 3 * (size_t)q;
    dst[0] = c[0] | (c[1] << 24);          // R0 G0 B0 R1
    dst[1] = (c[1] >> 8) | (c[2] << 16);   // G1 B1 R2 G2
    dst[2] = (c[2] >> 16) | (c[3] << 8);   // B2 R3 G3 B3
  }
  // the pixels no quad covers, one per thread, as bytes
  for (uint32_t p = 4 * quads + blockIdx.x * kMonThreads + threadIdx.x; p < P.npix; p += gridDim.x * kMonThreads) {
    const uint32_t y = p / P.wg, x = p - y * P.wg;
    const uint32_t c = mon_colour(mon_grid_value(P, y, x), vmin, vmax, s_lut);
    uint8_t* dst = P.out + 3 * (size_t)p;
    dst[0] = (uint8_t)c;
    dst[1] = (uint8_t)(c >> 8);
    dst[2] = (uint8_t)(c >> 16);
  }
}

// make_grid's shape (torchvision.utils.make_grid: one image comes back as it is); false: a bad argument or too large
bool mon_shape(int count, int h, int w, int nrow, int padding, int* hg, int* wg, int* xmaps) {
  if (count < 1 || h < 1 || w < 1 || nrow < 1 || padding < 0) return false;
  int64_t H = h, W = w;
  int xm = 1;
  if (count > 1) {
    xm = std::min(nrow, count);
    const int ym = ceil_div(count, xm);
    H = (int64_t)ym * ((int64_t)h + padding) + padding;
    W = (int64_t)xm * ((int64_t)w + padding) + padding;
  }
  if (H * W >= ((int64_t)1 << 31) / 4) return false;  // pixel and byte counts stay 32-bit in the kernels
  *hg = (int)H, *wg = (int)W, *xmaps = xm;
  return true;
}

}  // namespace
}  // namespace mimo

using namespace mimo;

extern "C" int mimo_monitor_grid_shape(int count, int h, int w, int nrow, int padding, int* hg, int* wg) {
  int xm;
  if (!hg || !wg || !mon_shape(count, h, w, nrow, padding, hg, wg, &xm)) {
    set_error("mimo_monitor_grid_shape: count %d, image %d x %d, nrow %d, padding %d: bad argument, or a grid of 2^29 pixels or more",
              count, h, w, nrow, padding);
    return MIMO_ERR_INVALID;
  }
  return MIMO_OK;
}

extern "C" size_t mimo_monitor_scratch_bytes(int n_panels) {
  return (size_t)std::max(0, std::min(n_panels, kMonMaxPanels)) * 3 * kMonPartials * sizeof(float);
}

extern "C" int mimo_monitor_grids(const mimo_monitor_panel* panels, int n_panels, uint8_t* out, void* scratch,
                                  mimo_stream stream) {
  if (n_panels < 1 || n_panels > kMonMaxPanels) {
    set_error("mimo_monitor_grids: %d panels (1 ... %d per call)", n_panels, kMonMaxPanels);
    return MIMO_ERR_INVALID;
  }
  if (!panels || !out) {
    set_error("mimo_monitor_grids: null panel table or output");
    return MIMO_ERR_INVALID;
  }
  MonTable tab = {};
  bool any_auto = false;
  uint32_t max_pix = 0;
  for (int i = 0; i < n_panels; ++i) {
    const mimo_monitor_panel& a = panels[i];
    if (!a.src || !a.lut) {
      set_error("mimo_monitor_grids: panel %d: null source or colour table", i);
      return MIMO_ERR_INVALID;
    }
    if (a.n < 1 || a.c < 1 || a.h < 2 || a.w < 2) {
      set_error("mimo_monitor_grids: panel %d: source [%d, %d, %d, %d] (h and w >= 2: colorize refuses a line)", i, a.n, a.c,
                a.h, a.w);
      return MIMO_ERR_INVALID;
    }
    if (a.count < 1 || a.count > a.n) {
      set_error("mimo_monitor_grids: panel %d: count %d outside 1 ... n = %d", i, a.count, a.n);
      return MIMO_ERR_INVALID;
    }
    if (a.channel < 0 || a.channel >= a.c) {
      set_error("mimo_monitor_grids: panel %d: channel %d outside [0, %d)", i, a.channel, a.c);
      return MIMO_ERR_INVALID;
    }
    if (a.mask && a.mc != 1 && a.mc != a.c) {
      set_error("mimo_monitor_grids: panel %d: mask with %d channels (1 or c = %d)", i, a.mc, a.c);
      return MIMO_ERR_INVALID;
    }
    if (a.nrow < 1) {
      set_error("mimo_monitor_grids: panel %d: nrow %d < 1", i, a.nrow);
      return MIMO_ERR_INVALID;
    }
    if (a.padding < 0) {
      set_error("mimo_monitor_grids: panel %d: padding %d < 0", i, a.padding);
      return MIMO_ERR_INVALID;
    }
    if (a.flags & ~7) {
      set_error("mimo_monitor_grids: panel %d: unknown flag bits 0x%x", i, a.flags);
      return MIMO_ERR_INVALID;
    }
    if (a.out_offset < 0) {
      set_error("mimo_monitor_grids: panel %d: negative out_offset", i);
      return MIMO_ERR_INVALID;
    }
    int hg, wg, xmaps;
    if (!mon_shape(a.count, a.h, a.w, a.nrow, a.padding, &hg, &wg, &xmaps)) {
      set_error("mimo_monitor_grids: panel %d: a grid of 2^29 pixels or more", i);
      return MIMO_ERR_INVALID;
    }
    MonPanel& P = tab.p[i];
    const int64_t hw = (int64_t)a.h * a.w;
    P.src = a.src + (int64_t)a.channel * hw;
    P.src_stride = (int64_t)a.c * hw;
    P.mask = a.mask ? a.mask + (int64_t)(a.mc == 1 ? 0 : a.channel) * hw : nullptr;
    P.mask_stride = (int64_t)a.mc * hw;
    P.lut = a.lut;
    P.out = out + a.out_offset;
    P.h = a.h, P.w = a.w, P.hw = (uint32_t)hw, P.count = a.count;
    const int pad = a.count > 1 ? a.padding : 0;
    P.xmaps = xmaps, P.pad = pad, P.cell_h = a.h + pad, P.cell_w = a.w + pad;
    P.wg = wg, P.npix = (uint32_t)hg * (uint32_t)wg;
    P.flags = a.flags;
    P.has_zero = (int64_t)P.npix > (int64_t)a.count * hw;
    P.vmin = a.vmin, P.vmax = a.vmax;
    any_auto |= (a.flags & (kMonAutoMin | kMonAutoMax)) != 0;
    max_pix = std::max(max_pix, P.npix);
  }
  if (any_auto && (!scratch || ((uintptr_t)scratch & 3))) {
    set_error("mimo_monitor_grids: an automatic range needs mimo_monitor_scratch_bytes() of 4-byte aligned scratch");
    return MIMO_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (any_auto) {
    hipLaunchKernelGGL(monitor_range_kernel, dim3(kMonPartials, n_panels), dim3(kMonThreads), 0, st, tab, (float*)scratch);
    MIMO_KERNEL_CHECK();
  }
  // grid-stride over quads, 2048 workgroups at most over all panels (8 per CU): the ew_*.hip kernels' and fgsm.hip's rule
  const int per_panel = std::max(1, 2048 / n_panels);
  const int blocks = (int)std::min<int64_t>(ceil_div64(ceil_div64(max_pix, 4), kMonThreads), per_panel);
  hipLaunchKernelGGL(monitor_grid_kernel, dim3(blocks, n_panels), dim3(kMonThreads), 0, st, tab, (const float*)scratch);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}
