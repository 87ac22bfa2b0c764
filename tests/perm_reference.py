"""numpy restatement of `mimo_draw_permutations` (include/mimo_hip.h, csrc/perm_draw.hip): the subnetwork permutations of
apply_input_transform (the reference's mimo/models/utils.py:27-36) from a Philox4x32-10 stream.  Holds no device code; the
GPU tests compare the kernel's output with it bit for bit, the CPU tests check the definition itself.

    bits(stream, j) = philox4x32_10(ctr = (j >> 1, stream, offset_lo, offset_hi), key = (seed_lo, seed_hi)):
                      words (x, y) for even j, (z, w) for odd j, the first word low
    key(stream, j)  = (bits & ~0xFFF) | j
    base = argsort(key(0, 0..batch-1)); main[i] = base[i mod batch]; sigma_s = argsort(key(1 + s, 0..k-1))
    perm[s] = main[:k][sigma_s] ++ main[k:]
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
MAX_ROWS, MAX_SUBNETWORKS = 4096, 64


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays (or scalars) of 32-bit counter words held as uint64; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def keys(stream: int, n: int, seed: int, offset: int) -> np.ndarray:
    j = np.arange(n, dtype=np.uint64)
    x, y, z, w = philox4x32_10(j >> np.uint64(1), np.full(n, stream, dtype=np.uint64), np.full(n, offset & 0xFFFFFFFF, dtype=np.uint64),
                               np.full(n, (offset >> 32) & 0xFFFFFFFF, dtype=np.uint64), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    odd = (j & np.uint64(1)) == np.uint64(1)
    bits = np.where(odd, (w << np.uint64(32)) | z, (y << np.uint64(32)) | x)
    return (bits & ~np.uint64(0xFFF)) | j


def argsort_keys(stream: int, n: int, seed: int, offset: int) -> np.ndarray:
    k = keys(stream, n, seed, offset)
    assert len(np.unique(k)) == n  # the index in the low bits makes every key distinct
    return np.argsort(k, kind="stable").astype(np.int64)


def draw_permutations(batch: int, reps: int, k: int, s: int, seed: int, offset: int):
    """(perm [s, batch * reps], main [batch * reps]) as int64 arrays."""
    m = batch * reps
    assert 1 <= batch and 1 <= reps and m <= MAX_ROWS and 0 <= k <= m and 1 <= s <= MAX_SUBNETWORKS
    main = argsort_keys(0, batch, seed, offset)[np.arange(m) % batch]
    perm = np.empty((s, m), dtype=np.int64)
    for sub in range(s):
        perm[sub, :k] = main[:k][argsort_keys(1 + sub, k, seed, offset)]
        perm[sub, k:] = main[k:]
    return perm, main


def head_count(batch: int, reps: int, irp: float) -> int:
    """k as the reference computes it (utils.py:31): int(len(main_shuffle) * (1 - input_repetition_probability))."""
    return int(batch * reps * (1.0 - irp))
