// Whole-scene inference: the two bandwidth kernels around the forward, gfx950.
//
// The reference only knows patches: SEN12TP scenes are cut into 256-pixel patches at a stride of 249 by the dataset
// (scripts/test/test_ndvi.py:152-160, sen12tp_datamodule.py:54-66) and the seams are the caller's.  Here a scene stays in HBM
// as [C, H, W] fp32, a batch of tiles is one gather launch in front of the forward, and the batch's three result maps are
// added into the three scene maps by one stitch launch behind it.
//
// Geometry (include/mimo_hip.h states it in full; struct SceneAxis below is its only implementation on the device and in
// the argument checks): along an axis of length L with patch P and stride s, n = 1 + ceil((L - P) / s) tiles at the origins
// o_k = min(k s, L - P) — the last tile is shifted inwards, never padded — numbered row-major over the scene, t = ky nx + kx.
//
// Gather: dst[b, c, y, x] = scene[c, oy(t) + y, ox(t) + x] with t = min(t0 + b, T - 1).  The clamp is part of the definition:
// the last, short batch of a scene repeats its last tile and keeps the call shape (one plan, one captured graph).
// A thread owns 4 consecutive pixels of a tile row (the last thread of a row P % 4 of them): one float4 load where the
// source quad lies on a 16-byte boundary, one float4 store where the destination quad does, scalars otherwise.
// Traffic per tile pixel and channel: 4 bytes read, 4 bytes written.
//
// Stitch: output-pixel-centric.  One thread owns one scene pixel of one channel of one field, inside the band of rows the
// launch's tiles t0 ... t0 + n_valid - 1 touch.  It walks the tiles that cover its pixel in ascending t and accumulates
// fl(a_t v_t) with round-to-nearest multiply and add, no contraction; a_t = fl(a_ky(y) a_kx(x)) is the normalised separable
// weight, so no weight-sum buffer and no finalising pass exist.  A pixel whose lowest covering tile overall lies in the
// launch (or a later one) is stored — the first term assigned, the others added — every other pixel is read, added to and
// stored: the destination needs no memset, launches on one stream serialise, and the per-pixel order is ascending t whatever
// the batch size.  `crop` is a pure copy of the owner's value.  Pixels covered by no tile of the launch are not touched.
// Traffic per scene pixel and channel: 4 bytes per covering tile of the launch read, 4 bytes written, and 4 more read
// where an earlier launch has started the sum (the seams between two launches only).
//
// Plain vector loads and stores only: no atomics, no inline assembly.
//
// Lives in a subdirectory because the benchmark never launches it (bench.csrc_hash covers csrc/*.hip, csrc/*.h), as
// data/dataset_gather.hip, eval/eval_stats.hip and optim_clip/grad_clip.hip do.
#include <cstdint>

#include "../common.h"

namespace mimo {
namespace {

constexpr int kSceneThreads = 256;
constexpr int kStitchMaxFields = MIMO_STITCH_MAX_FIELDS;
// linear weights are <= P / 2 and at most P tiles cover a position: their integer sum stays below 2^24 (exact in fp32)
constexpr int kSceneMaxPatch = 4096;

// one axis of the tile grid
struct SceneAxis {
  int32_t len, patch, stride, n;
  __host__ __device__ int32_t origin(int32_t k) const {
    const int64_t o = (int64_t)k * stride;
    return o < len - patch ? (int32_t)o : len - patch;
  }
  // K(p) = {k : o_k <= p < o_k + P} = [lo(p), hi(p)], never empty
  __host__ __device__ int32_t lo(int32_t p) const {
    const int32_t k = p < patch ? 0 : (p - patch) / stride + 1;
    return k < n - 1 ? k : n - 1;
  }
  __host__ __device__ int32_t hi(int32_t p) const { return p >= len - patch ? n - 1 : p / stride; }
};

static SceneAxis make_axis(int32_t len, int32_t patch, int32_t stride) {
  SceneAxis a;
  a.len = len, a.patch = patch, a.stride = stride;
  a.n = 1 + (int32_t)ceil_div64((int64_t)len - patch, stride);
  return a;
}

// One rounding per operation, whatever -ffp-contract says: the toolchain's __fmul_rn / __fadd_rn / __fdiv_rn are plain
// operators compiled under the default contraction mode, so a product and the sum behind it could still fuse into an fma.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;  // correctly rounded: hipcc's default for fp32 division
}

// the `linear` window at offset i of a tile, min(i + 1, P - i)
__device__ __forceinline__ int32_t linear_weight(int32_t i, int32_t patch) { return i + 1 < patch - i ? i + 1 : patch - i; }

// ---------------------------------------------------------------------------------------------------------------- gather
// total = n * c * patch * qpr threads with work, qpr = ceil(patch / 4) quads per tile row
__global__ __launch_bounds__(kSceneThreads) void scene_gather_kernel(const float* __restrict__ scene, float* __restrict__ dst,
                                                                     SceneAxis ay, SceneAxis ax, int32_t c, int32_t t0,
                                                                     uint32_t qpr, uint32_t total) {
  const uint32_t i = blockIdx.x * kSceneThreads + threadIdx.x;
  if (i >= total) return;
  const uint32_t patch = (uint32_t)ax.patch;
  const uint32_t row = i / qpr, x0 = 4 * (i - row * qpr);  // row = (b * c + ch) * patch + y
  const uint32_t plane = row / patch, y = row - plane * patch;
  const uint32_t b = plane / (uint32_t)c, ch = plane - b * (uint32_t)c;
  const uint32_t npx = patch - x0 < 4 ? patch - x0 : 4;
  const int64_t tiles = (int64_t)ay.n * ax.n;
  const int64_t t = (int64_t)t0 + b < tiles ? (int64_t)t0 + b : tiles - 1;
  const int32_t ky = (int32_t)(t / ax.n), kx = (int32_t)(t - (int64_t)ky * ax.n);
  const float* s = scene + ((int64_t)ch * ay.len + ay.origin(ky) + y) * ax.len + ax.origin(kx) + x0;
  float* d = dst + (int64_t)row * patch + x0;  // < n * c * patch * patch < 2^31
  float v[4];
  if (npx == 4 && ((uintptr_t)s & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(s);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = p < (int)npx ? s[p] : 0.f;
  }
  if (npx == 4 && ((uintptr_t)d & 15) == 0) {
    *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (p < (int)npx) d[p] = v[p];
  }
}

// ---------------------------------------------------------------------------------------------------------------- stitch
struct StitchField {
  const float* src;
  float* dst;
  int32_t c;
};
struct StitchTable {
  StitchField f[kStitchMaxFields];
};

// normalised 1-D weight of tile k at position p: w(p - o_k) / sum over ascending j in K(p) of w(p - o_j), one division
__device__ __forceinline__ float axis_weight(const SceneAxis& a, int32_t p, int32_t k, int32_t lo, int32_t hi, int32_t window) {
  if (window == MIMO_WINDOW_UNIFORM) return div_rn(1.f, (float)(hi - lo + 1));
  int32_t sum = 0;
  for (int32_t j = lo; j <= hi; ++j) sum += linear_weight(p - a.origin(j), a.patch);
  return div_rn((float)linear_weight(p - a.origin(k), a.patch), (float)sum);
}

// the owner of p under `crop`: the k in K(p) with the largest linear weight, ties to the lowest k
__device__ __forceinline__ int32_t axis_owner(const SceneAxis& a, int32_t p, int32_t lo, int32_t hi) {
  int32_t best = lo, wbest = linear_weight(p - a.origin(lo), a.patch);
  for (int32_t j = lo + 1; j <= hi; ++j) {
    const int32_t w = linear_weight(p - a.origin(j), a.patch);
    if (w > wbest) best = j, wbest = w;
  }
  return best;
}

// blockIdx.x: pixels of the band [y0, y0 + rows) x [0, W); blockIdx.y: channel; blockIdx.z: field
__global__ __launch_bounds__(kSceneThreads) void scene_stitch_kernel(StitchTable tab, SceneAxis ay, SceneAxis ax, int32_t window,
                                                                     int32_t t0, int32_t n_valid, int32_t y0, uint32_t total) {
  const StitchField& F = tab.f[blockIdx.z];
  const int32_t ch = (int32_t)blockIdx.y;
  const uint32_t i = blockIdx.x * kSceneThreads + threadIdx.x;
  if (i >= total || ch >= F.c) return;
  const uint32_t width = (uint32_t)ax.len;
  const uint32_t r = i / width;
  const int32_t x = (int32_t)(i - r * width), y = y0 + (int32_t)r;
  const int32_t ylo = ay.lo(y), yhi = ay.hi(y), xlo = ax.lo(x), xhi = ax.hi(x);
  const int64_t t1 = (int64_t)t0 + n_valid - 1;  // the launch's last tile
  const int64_t pp = (int64_t)ax.patch * ax.patch;
  float* d = F.dst + ((int64_t)ch * ay.len + y) * width + x;
  if (window == MIMO_WINDOW_CROP) {
    const int32_t ky = axis_owner(ay, y, ylo, yhi), kx = axis_owner(ax, x, xlo, xhi);
    const int64_t t = (int64_t)ky * ax.n + kx;
    if (t < t0 || t > t1) return;
    *d = F.src[((t - t0) * F.c + ch) * pp + (int64_t)(y - ay.origin(ky)) * ax.patch + (x - ax.origin(kx))];
    return;
  }
  bool started = (int64_t)ylo * ax.n + xlo < t0;  // an earlier launch holds the pixel's first terms
  bool touched = false;
  float acc = 0.f;
  for (int32_t ky = ylo; ky <= yhi; ++ky) {
    const int64_t trow = (int64_t)ky * ax.n;
    if (trow + xhi < t0 || trow + xlo > t1) continue;
    const float wy = axis_weight(ay, y, ky, ylo, yhi, window);
    const int64_t srow = (int64_t)(y - ay.origin(ky)) * ax.patch;
    for (int32_t kx = xlo; kx <= xhi; ++kx) {
      const int64_t t = trow + kx;
      if (t < t0 || t > t1) continue;
      if (!touched && started) acc = *d;
      touched = true;
      const float a = mul_rn(wy, axis_weight(ax, x, kx, xlo, xhi, window));
      const float term = mul_rn(a, F.src[((t - t0) * F.c + ch) * pp + srow + (x - ax.origin(kx))]);
      acc = started ? add_rn(acc, term) : term;
      started = true;
    }
  }
  if (touched) *d = acc;
}

// what both entry points ask of the grid; `who` names the caller in the message
static int check_grid(const char* who, int32_t h, int32_t w, int32_t patch, int32_t stride) {
  if (h < 1 || w < 1 || patch < 1 || stride < 1) {
    set_error("%s: scene %d x %d, patch %d, stride %d: all must be >= 1", who, h, w, patch, stride);
    return MIMO_ERR_INVALID;
  }
  if (patch > h || patch > w || stride > patch) {
    set_error("%s: scene %d x %d, patch %d, stride %d: 1 <= stride <= patch <= min(h, w) is needed", who, h, w, patch, stride);
    return MIMO_ERR_INVALID;
  }
  return MIMO_OK;
}

}  // namespace
}  // namespace mimo

using namespace mimo;

extern "C" int mimo_scene_gather_tiles(const float* scene, float* dst, int32_t c, int32_t h, int32_t w, int32_t patch,
                                       int32_t stride, int32_t t0, int32_t n, mimo_stream stream) {
  const char* who = "mimo_scene_gather_tiles";
  if (!scene || !dst) {
    set_error("%s: null scene or destination", who);
    return MIMO_ERR_INVALID;
  }
  if (((uintptr_t)scene & 3) || ((uintptr_t)dst & 3)) {
    set_error("%s: scene and destination hold floats and must be 4-byte aligned", who);
    return MIMO_ERR_INVALID;
  }
  MIMO_TRY(check_grid(who, h, w, patch, stride));
  if (c < 1 || n < 1) {
    set_error("%s: %d channels, %d tiles: both must be >= 1", who, c, n);
    return MIMO_ERR_INVALID;
  }
  // the kernel counts threads and destination elements in 32 bits, tiles and scene offsets in 64
  const int64_t kMaxElems = ((int64_t)1 << 31) - 1, kMaxSceneElems = (int64_t)1 << 60;
  const int64_t pp = (int64_t)patch * patch;  // < 2^62
  if (pp > kMaxElems / c / n) {
    set_error("%s: %d tiles of %d x %d x %d: n * c * patch * patch must stay below 2^31", who, n, c, patch, patch);
    return MIMO_ERR_INVALID;
  }
  if ((int64_t)h * w > kMaxSceneElems / c) {
    set_error("%s: scene %d x %d x %d: c * h * w must stay below 2^60", who, c, h, w);
    return MIMO_ERR_INVALID;
  }
  const SceneAxis ay = make_axis(h, patch, stride), ax = make_axis(w, patch, stride);
  if (t0 < 0 || t0 >= (int64_t)ay.n * ax.n) {
    set_error("%s: first tile %d outside [0, %lld)", who, t0, (long long)ay.n * ax.n);
    return MIMO_ERR_INVALID;
  }
  const uint32_t qpr = (uint32_t)ceil_div(patch, 4);
  const uint32_t total = (uint32_t)((int64_t)n * c * patch * qpr);  // <= n * c * patch * patch < 2^31
  hipLaunchKernelGGL(scene_gather_kernel, dim3((unsigned)ceil_div64(total, kSceneThreads)), dim3(kSceneThreads), 0,
                     (hipStream_t)stream, scene, dst, ay, ax, c, t0, qpr, total);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

extern "C" int mimo_scene_stitch(const mimo_stitch_field* fields, int n_fields, int32_t h, int32_t w, int32_t patch,
                                 int32_t stride, int32_t window, int32_t t0, int32_t n_valid, mimo_stream stream) {
  const char* who = "mimo_scene_stitch";
  if (n_fields < 1 || n_fields > kStitchMaxFields) {
    set_error("%s: %d fields (1 ... %d per call)", who, n_fields, kStitchMaxFields);
    return MIMO_ERR_INVALID;
  }
  if (!fields) {
    set_error("%s: null field table", who);
    return MIMO_ERR_INVALID;
  }
  MIMO_TRY(check_grid(who, h, w, patch, stride));
  if (patch > kSceneMaxPatch) {
    set_error("%s: patch %d: the window sums are exact in fp32 up to a patch of %d", who, patch, kSceneMaxPatch);
    return MIMO_ERR_INVALID;
  }
  if (window != MIMO_WINDOW_UNIFORM && window != MIMO_WINDOW_LINEAR && window != MIMO_WINDOW_CROP) {
    set_error("%s: window %d (0 uniform, 1 linear, 2 crop)", who, window);
    return MIMO_ERR_INVALID;
  }
  const SceneAxis ay = make_axis(h, patch, stride), ax = make_axis(w, patch, stride);
  const int64_t tiles = (int64_t)ay.n * ax.n;
  if (t0 < 0 || n_valid < 1 || (int64_t)t0 + n_valid > tiles) {
    set_error("%s: tiles %d ... %lld outside [0, %lld)", who, t0, (long long)t0 + n_valid - 1, (long long)tiles);
    return MIMO_ERR_INVALID;
  }
  // the kernel counts the pixels of the band in 32 bits, source and scene offsets in 64
  const int64_t kMaxElems = ((int64_t)1 << 31) - 1, kMaxSourceElems = (int64_t)1 << 60;
  if ((int64_t)h * w > kMaxElems) {
    set_error("%s: scene %d x %d: h * w must stay below 2^31", who, h, w);
    return MIMO_ERR_INVALID;
  }
  StitchTable tab = {};
  int32_t c_max = 0;
  for (int i = 0; i < n_fields; ++i) {
    const mimo_stitch_field& a = fields[i];
    if (!a.src || !a.dst) {
      set_error("%s: field %d: null source or destination", who, i);
      return MIMO_ERR_INVALID;
    }
    if (((uintptr_t)a.src & 3) || ((uintptr_t)a.dst & 3)) {
      set_error("%s: field %d: source and destination hold floats and must be 4-byte aligned", who, i);
      return MIMO_ERR_INVALID;
    }
    if (a.c < 1 || a.c > 65535) {
      set_error("%s: field %d: %d channels (1 ... 65535)", who, i, a.c);
      return MIMO_ERR_INVALID;
    }
    if ((int64_t)patch * patch > kMaxSourceElems / a.c / n_valid) {  // (c * h * w < 2^47 with the bounds above)
      set_error("%s: field %d: n_valid * c * patch * patch must stay below 2^60", who, i);
      return MIMO_ERR_INVALID;
    }
    tab.f[i].src = a.src, tab.f[i].dst = a.dst, tab.f[i].c = a.c;
    c_max = a.c > c_max ? a.c : c_max;
  }
  // the band of rows the launch's tiles touch
  const int32_t ky0 = (int32_t)(t0 / ax.n), ky1 = (int32_t)(((int64_t)t0 + n_valid - 1) / ax.n);
  const int32_t y0 = ay.origin(ky0), rows = ay.origin(ky1) + patch - y0;
  const uint32_t total = (uint32_t)((int64_t)rows * w);  // <= h * w < 2^31
  hipLaunchKernelGGL(scene_stitch_kernel, dim3((unsigned)ceil_div64(total, kSceneThreads), c_max, n_fields),
                     dim3(kSceneThreads), 0, (hipStream_t)stream, tab, ay, ax, window, t0, n_valid, y0, total);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}
