// Batches gathered from a byte store that lives in HBM, gfx950.
//
// Replaces, for every field of a batch in one call, what the reference does per SAMPLE on the host
// (mimo/datasets/nyuv2.py:38-53: index the uint8 arrays through shuffle_permutation, `/ 255.0` in float64, torch.tensor,
// permute(2, 0, 1), .float()), the DataLoader's collate to fp32 and the upload of the collated batch.  Here the dataset
// stays on the device as the bytes it is stored in, [n_samples, H, W, c] per field, and a batch is one launch in front of
// the step: gather by index, table lookup, HWC -> NCHW.
//
// Semantics (include/mimo_hip.h states them in full): i = clamp(index[b]), j = remap ? clamp(remap[i]) : i,
// dst_f[b, k, y, x] = lut_f[src_f[j, y, x, k]].  The clamps are part of the definition: no address is ever formed from
// an index outside the store.  The normalisation is the caller's 256-entry table and no arithmetic here, so the result
// carries the caller's rounding (the reference's float64 quotient rounded once) bit for bit.
//
// Traffic per pixel and field: c bytes read, 4 c bytes written — 5 c bytes; the index and remap words are 8 or 16 bytes per
// batch row and workgroup.  Launches: one, blockIdx.y = field.
//
// Table: staged in LDS once per workgroup (256 threads, one entry each), as monitor.hip stages its colour table: the
// lookups of a thread (up to 16) then cost LDS reads and no vector-memory operation.
//
// Work: a thread owns 4 consecutive pixels of one sample (the last thread of a sample h * w % 4 of them when h * w is
// no multiple of 4).  Loads: when h * w % 4 == 0 and the field's base is 4-aligned, every sample and every quad starts on a
// dword, and the quad's 4 c bytes are read as c dwords; otherwise byte by byte.  Stores: one float4 per channel plane
// where the four floats lie on a 16-byte boundary, four scalars otherwise.  Plain vector loads and stores only: no
// atomics, no scratch (the channel count is a template argument, so the per-thread arrays stay in registers), no inline
// assembly.
//
// Lives in a subdirectory because the benchmark never launches it (bench.csrc_hash covers csrc/*.hip, csrc/*.h), as
// eval/eval_stats.hip and optim_clip/grad_clip.hip do.
#include <cstdint>

#include "../common.h"

namespace mimo {
namespace {

constexpr int kGatherThreads = 256;
constexpr int kGatherMaxFields = MIMO_GATHER_MAX_FIELDS;
static_assert(kGatherThreads == 256, "one table entry per thread");

struct GatherField {
  const uint8_t* src;
  const float* lut;
  float* dst;
  int32_t c;
  int32_t dwords;  // the source is read in dwords (4-aligned base, h * w % 4 == 0)
};
struct GatherTable {
  GatherField f[kGatherMaxFields];
};

__device__ __forceinline__ int64_t gather_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// pixels p0 ... p0 + npx - 1 of source sample j into batch row b; npx == 4 on the dword path
template <int C>
__device__ __forceinline__ void gather_quad(const GatherField& F, const float* s_lut, int64_t j, uint32_t b, uint32_t p0,
                                            uint32_t npx, uint32_t hw) {
  const uint8_t* s = F.src + (j * hw + p0) * C;
  float v[C][4];  // [channel][pixel]
  if (F.dwords) {
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(s);
    uint32_t d[C];
#pragma unroll
    for (int m = 0; m < C; ++m) d[m] = s32[m];
#pragma unroll
    for (int n = 0; n < 4 * C; ++n) v[n % C][n / C] = s_lut[(d[n >> 2] >> (8 * (n & 3))) & 0xFFu];
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int k = 0; k < C; ++k) v[k][p] = p < (int)npx ? s_lut[s[p * C + k]] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < C; ++k) {
    float* d = F.dst + ((int64_t)b * C + k) * hw + p0;
    if (npx == 4 && ((uintptr_t)d & 15) == 0) {
      *reinterpret_cast<float4*>(d) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p < (int)npx) d[p] = v[k][p];
    }
  }
}

// total = batch * qps threads with work per field, qps = ceil(h * w / 4) quads per sample
__global__ __launch_bounds__(kGatherThreads) void dataset_gather_kernel(GatherTable tab, const int64_t* __restrict__ index,
                                                                        const int64_t* __restrict__ remap, int64_t n_samples,
                                                                        uint32_t hw, uint32_t qps, uint32_t total) {
  const GatherField& F = tab.f[blockIdx.y];
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = F.lut[threadIdx.x];
  __syncthreads();
  const uint32_t t = blockIdx.x * kGatherThreads + threadIdx.x;
  if (t >= total) return;
  const uint32_t b = t / qps, p0 = 4 * (t - b * qps);
  const uint32_t npx = hw - p0 < 4 ? hw - p0 : 4;
  int64_t j = gather_clamp(index[b], n_samples);
  if (remap) j = gather_clamp(remap[j], n_samples);
  switch (F.c) {  // the same for the whole workgroup
    case 1: gather_quad<1>(F, s_lut, j, b, p0, npx, hw); break;
    case 2: gather_quad<2>(F, s_lut, j, b, p0, npx, hw); break;
    case 3: gather_quad<3>(F, s_lut, j, b, p0, npx, hw); break;
    default: gather_quad<4>(F, s_lut, j, b, p0, npx, hw); break;
  }
}

}  // namespace
}  // namespace mimo

using namespace mimo;

extern "C" int mimo_dataset_gather(const mimo_gather_field* fields, int n_fields, const int64_t* index, const int64_t* remap,
                                   int64_t n_samples, int32_t batch, int32_t h, int32_t w, mimo_stream stream) {
  if (n_fields < 1 || n_fields > kGatherMaxFields) {
    set_error("mimo_dataset_gather: %d fields (1 ... %d per call)", n_fields, kGatherMaxFields);
    return MIMO_ERR_INVALID;
  }
  if (!fields || !index) {
    set_error("mimo_dataset_gather: null field table or index");
    return MIMO_ERR_INVALID;
  }
  if (batch < 1 || h < 1 || w < 1 || n_samples < 1) {
    set_error("mimo_dataset_gather: batch %d, image %d x %d, %lld samples: all must be >= 1", batch, h, w, (long long)n_samples);
    return MIMO_ERR_INVALID;
  }
  // the kernel counts threads, pixels of a sample and elements of a batch in 32 bits and source bytes in 64
  const int64_t hw = (int64_t)h * w;  // < 2^62
  const int64_t kMaxBatchElems = ((int64_t)1 << 31) - 1, kMaxStoreBytes = (int64_t)1 << 62;
  if (hw > kMaxBatchElems / 4 / batch) {  // batch * h * w * 4 channels
    set_error("mimo_dataset_gather: batch %d of %d x %d images: batch * h * w * 4 must stay below 2^31", batch, h, w);
    return MIMO_ERR_INVALID;
  }
  if (n_samples > kMaxStoreBytes / (hw * 4)) {
    set_error("mimo_dataset_gather: %lld samples of %d x %d pixels: n_samples * h * w * 4 must stay below 2^62",
              (long long)n_samples, h, w);
    return MIMO_ERR_INVALID;
  }
  GatherTable tab = {};
  for (int i = 0; i < n_fields; ++i) {
    const mimo_gather_field& a = fields[i];
    if (!a.src || !a.lut || !a.dst) {
      set_error("mimo_dataset_gather: field %d: null source, table or destination", i);
      return MIMO_ERR_INVALID;
    }
    if (a.c < 1 || a.c > 4) {
      set_error("mimo_dataset_gather: field %d: %d channels (1 ... 4)", i, a.c);
      return MIMO_ERR_INVALID;
    }
    if (((uintptr_t)a.lut & 3) || ((uintptr_t)a.dst & 3)) {
      set_error("mimo_dataset_gather: field %d: table and destination hold floats and must be 4-byte aligned", i);
      return MIMO_ERR_INVALID;
    }
    GatherField& F = tab.f[i];
    F.src = a.src, F.lut = a.lut, F.dst = a.dst, F.c = a.c;
    F.dwords = hw % 4 == 0 && ((uintptr_t)a.src & 3) == 0;
  }
  const uint32_t qps = (uint32_t)ceil_div64(hw, 4);
  const uint32_t total = (uint32_t)batch * qps;  // <= batch * h * w < 2^29
  hipLaunchKernelGGL(dataset_gather_kernel, dim3((unsigned)ceil_div64(total, kGatherThreads), n_fields), dim3(kGatherThreads), 0,
                     (hipStream_t)stream, tab, index, remap, n_samples, (uint32_t)hw, qps, total);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}
