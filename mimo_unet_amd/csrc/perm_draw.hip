// The subnetwork permutations of a training step, drawn on the device in one launch, gfx950.
//
// Replaces (paths relative to the reference's root): the draws of apply_input_transform, mimo/models/utils.py:27-36 —
//   main_shuffle = torch.randperm(B).repeat(batch_repetitions); k = int(len * (1 - input_repetition_probability))
//   shuffle_indices[s] = cat(main_shuffle[:k][torch.randperm(k)], main_shuffle[k:])
// — a device randperm (fill, arange, random keys, block sort, duplicate-key fix), S CPU randperms, an upload, an index and a
// concatenation: seven launches in front of the first engine kernel.  Same structure here, from the engine's own generator
// (philox.h, keyed by the (seed, offset) pair of torch's CUDA generator like the dropout multipliers); the VALUES are not the
// reference's generator streams, so the torch route stays for the golden fixtures (models/utils.py).
//
// Definition (restated in numpy by tests/perm_reference.py; M = batch * reps <= 4096, 0 <= k <= M, S <= 64):
//   bits(stream, j) = 64 bits: philox4x32_10(ctr = (j >> 1, stream, offset_lo, offset_hi), key = (seed_lo, seed_hi)), words
//                     (x, y) for even j and (z, w) for odd j, the first word low
//   key(stream, j)  = (bits(stream, j) & ~0xFFF) | j          52 random bits, the index as tie-break: all keys differ
//   argsort(stream, n) = the j of the n keys key(stream, 0..n-1) in ascending key order
//   base = argsort(0, batch); main[i] = base[i mod batch]; sigma_s = argsort(1 + s, k)
//   perm[s][i] = main[sigma_s[i]] for i < k, main[i] for i >= k
// An argsort of independent uniform keys is a uniform random permutation up to ties; with the index in the low 12 bits a
// tie of the upper 52 is broken towards the smaller index (probability ~ n^2 / 2^53 per draw, 2e-9 at n = 4096).
//
// One workgroup per subnetwork and no dependency between them: every workgroup sorts stream 0 itself (the same counters
// give the same `base`), so there is no second launch, no atomic and no flag.  The sort is a bitonic network over 64-bit
// keys in LDS, padded to the next power of two with ~0 (a real key is ~0 only for j = 4095, where nothing is padded); the
// sorted key's low 12 bits ARE the argsort, no payload travels.  LDS: 32 KB of keys + 8 KB for `base`.  Workgroup = half
// the padded length, 64 to 1024 threads: for M <= 64 the whole draw is one wave and the barriers wait for nobody.  The
// network's strides below 32 elements give 2-way conflicts on the 8-byte LDS reads; at the 78 passes of M = 4096 that is
// noise beside the barriers, at a training step's M (4 to 64) the kernel is a handful of passes.  Plain 8-byte vector
// stores, coalesced; no scratch.
#include <cstdint>

#include "common.h"
#include "philox.h"

namespace mimo {
namespace {

constexpr int kPermMaxM = 4096;  // keys in LDS; the index field of a key is 12 bits wide
constexpr int kPermMaxS = 64;

__device__ __forceinline__ uint64_t perm_key(unsigned int j, unsigned int stream, uint64_t seed, uint64_t offset) {
  const uint4 r = philox4x32_10(make_uint4(j >> 1, stream, (unsigned int)offset, (unsigned int)(offset >> 32)),
                                make_uint2((unsigned int)seed, (unsigned int)(seed >> 32)));
  const uint64_t bits = (j & 1u) ? ((uint64_t)r.w << 32) | r.z : ((uint64_t)r.y << 32) | r.x;
  return (bits & ~0xFFFull) | j;
}

// keys[0 .. n) = the n keys of `stream` in ascending order (n >= 1; np = the power of two >= n, keys[n .. np) = ~0)
__device__ void perm_sorted_keys(uint64_t* __restrict__ keys, int n, int np, unsigned int stream, uint64_t seed, uint64_t offset) {
  for (int i = threadIdx.x; i < np; i += blockDim.x) keys[i] = i < n ? perm_key((unsigned int)i, stream, seed, offset) : ~0ull;
  __syncthreads();
  for (int size = 2; size <= np; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (np >> 1); t += blockDim.x) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo | stride;
        const bool ascending = (lo & size) == 0;  // size == np: every pair, lo < np
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a > b) == ascending) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// grid = S workgroups; batch >= 1, M = batch * reps <= kPermMaxM, 0 <= k <= M (checked by the host entry point)
__global__ __launch_bounds__(1024) void draw_permutations_kernel(int64_t* __restrict__ perm, int64_t* __restrict__ main_out,
                                                                 int batch, int M, int k, uint64_t seed, uint64_t offset) {
  __shared__ uint64_t keys[kPermMaxM];
  __shared__ uint16_t base[kPermMaxM];
  const int s = blockIdx.x;
  perm_sorted_keys(keys, batch, pow2_at_least(batch), 0u, seed, offset);
  for (int i = threadIdx.x; i < batch; i += blockDim.x) base[i] = (uint16_t)(keys[i] & 0xFFFu);
  __syncthreads();  // base complete, and every read of keys done before the second draw overwrites them
  if (k > 0) perm_sorted_keys(keys, k, pow2_at_least(k), 1u + (unsigned int)s, seed, offset);
  int64_t* __restrict__ row = perm + (size_t)s * M;
  for (int i = threadIdx.x; i < M; i += blockDim.x) {
    const int src = i < k ? (int)(keys[i] & 0xFFFu) : i;  // src < k <= M
    row[i] = base[src % batch];
    if (main_out && s == 0) main_out[i] = base[i % batch];
  }
}

}  // namespace
}  // namespace mimo

using namespace mimo;

extern "C" int mimo_draw_permutations(int64_t* perm, int64_t* main_out, int32_t batch, int32_t reps, int32_t k, int32_t s,
                                      uint64_t seed, uint64_t offset, mimo_stream stream) {
  if (!perm || batch < 1 || reps < 1) {
    set_error("mimo_draw_permutations: bad argument (perm %p, batch %d, reps %d)", (void*)perm, batch, reps);
    return MIMO_ERR_INVALID;
  }
  const int64_t M = (int64_t)batch * reps;
  if (M > kPermMaxM) {
    set_error("mimo_draw_permutations: batch * reps = %lld exceeds the %d rows one workgroup sorts in LDS", (long long)M, kPermMaxM);
    return MIMO_ERR_INVALID;
  }
  if (s < 1 || s > kPermMaxS) {
    set_error("mimo_draw_permutations: %d subnetworks (1 .. %d)", s, kPermMaxS);
    return MIMO_ERR_INVALID;
  }
  if (k < 0 || k > M) {
    set_error("mimo_draw_permutations: k = %d outside [0, batch * reps = %lld]", k, (long long)M);
    return MIMO_ERR_INVALID;
  }
  int np = 1;
  while (np < M) np <<= 1;
  const int threads = np / 2 < 64 ? 64 : (np / 2 > 1024 ? 1024 : np / 2);
  hipLaunchKernelGGL(draw_permutations_kernel, dim3(s), dim3(threads), 0, (hipStream_t)stream, perm, main_out, batch, (int)M, k,
                     seed, offset);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}
