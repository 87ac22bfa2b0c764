"""numpy restatement of the in-engine dropout draws (csrc/ew_dropout.hip, `Plan::make_call` / `forward_impl` and the backward
stages of csrc/plan.hip; MIMO_ENGINE_RNG, on by default).  Holds no device code; the GPU tests (test_dropout_gpu.py) compare
what the kernels drew with it bit for bit, the CPU tests (test_dropout_reference_cpu.py) check the definition itself.

One forward takes one (seed, offset) pair from torch's CUDA generator and advances the offset by 4.

    words(i0, i1, site, seed, offset) = philox4x32_10(ctr = (i0, i1, lo32(offset) ^ ((site << 24) mod 2^32), hi32(offset)),
                                                      key = (lo32(seed), hi32(seed)));  lane j = output word j
    u24  = word >> 8
    keep = float32(u24) * 2^-24 >= float32(p)        (both sides exact in fp32)
         = u24 >= ceil(float32(p) * 2^24)            (the integer form used below: `threshold`)
    multiplier = float32(1) / (float32(1) - float32(p)) where kept, else 0

Sites.  ndc = 3 S + 6 DoubleConv blocks in engine order: in_convs[0..S-1], down1s[0..S-1], down2, down3, down4, up1, up2,
up3, up4s[0..S-1].  A site keeps its positional number whether or not other sites are active.

    Dropout2d site i (the i-th DoubleConv): flat [N][C], C the block's true output channels;
        element 4 q + j takes lane j of words(q, 0, i, ...)
    element-wise site ndc + j (j = 0: center_dropout, 1 + s: final_dropouts[s]): NCHW [N][C][H' W'], Cv = pad8(C) / 4;
        element (n, 4 q + l, r) takes lane l of words(r, n Cv + q, ndc + j, ...); lanes with 4 q + l >= C are unused

Shared randomness.  Within one forward every used multiplier has its own (counter, lane): sites differ in counter word 2
(site < 2^8 sits in bits 24..31, and kMaxSites = 56), elements of one site differ in (i0, i1) or in the lane.  Across
forwards the site number is XORed into bits 24.. of the LOW OFFSET WORD, so offset o at site a and offset o' at site b give
the same word 2 when o' = o ^ ((a ^ b) << 24): the first offset at which a step can reuse a counter block of another step is
FIRST_REUSE_OFFSET = 2^24 (site 1 there repeats site 0 of offset 0).  Below it — 2^22 forwards from a fresh seed — word 2 keeps
the offset's low 24 bits as they are, so any two offsets that differ there, o and o + 4 at any o among them, are disjoint.
"""
import numpy as np

from tests import perm_reference as P

MAX_SITES = 56  # FwdCall::kMaxSites (csrc/plan.hip)
FIRST_REUSE_OFFSET = 1 << 24
_M32 = 0xFFFFFFFF


def counter_word2(site: int, offset: int) -> int:
    return (offset & _M32) ^ ((site << 24) & _M32)


def words(i0, i1, site: int, seed: int, offset: int):
    """The four output words (uint64 arrays holding 32-bit values) for arrays (or scalars) i0, i1, broadcast together."""
    i0, i1 = np.broadcast_arrays(np.asarray(i0, dtype=np.uint64), np.asarray(i1, dtype=np.uint64))
    c2 = np.full(i0.shape, counter_word2(site, offset), dtype=np.uint64)
    c3 = np.full(i0.shape, (offset >> 32) & _M32, dtype=np.uint64)
    return P.philox4x32_10(i0, i1, c2, c3, seed & _M32, (seed >> 32) & _M32)


def u24(word):
    return np.asarray(word, dtype=np.uint64) >> np.uint64(8)


def threshold(p: float) -> int:
    """Smallest u24 that is kept: ceil(float32(p) * 2^24) (the product is exact in float64)."""
    return int(np.ceil(np.float64(np.float32(p)) * 16777216.0))


def keep_float(u, p: float):
    """The keep test as the kernel writes it, in fp32."""
    return np.asarray(u).astype(np.float32) * np.float32(2.0 ** -24) >= np.float32(p)


def keep_int(u, p: float):
    return np.asarray(u, dtype=np.uint64) >= np.uint64(threshold(p))


def kept_value(p: float) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def _multipliers(u, p: float) -> np.ndarray:
    return np.where(keep_int(u, p), kept_value(p), np.float32(0.0)).astype(np.float32)


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def dropout2d_u24(site: int, n: int, c: int, seed: int, offset: int) -> np.ndarray:
    """[N, C] uint64: the 24 uniform bits behind every multiplier of Dropout2d site `site`."""
    count = n * c
    q = np.arange((count + 3) // 4, dtype=np.uint64)
    lanes = np.stack(words(q, 0, site, seed, offset), axis=1)  # [q, lane]
    return u24(lanes).reshape(-1)[:count].reshape(n, c)


def dropout2d_mask(site: int, n: int, c: int, p: float, seed: int, offset: int) -> np.ndarray:
    return _multipliers(dropout2d_u24(site, n, c, seed, offset), p)


def elem_u24(site: int, n: int, c: int, h: int, w: int, seed: int, offset: int) -> np.ndarray:
    """[N, C, H', W'] uint64: the 24 uniform bits behind every multiplier of the element-wise site number `site`."""
    cv, hw = pad8(c) // 4, h * w
    r = np.arange(hw, dtype=np.uint64)[None, :]
    nq = np.arange(n * cv, dtype=np.uint64)[:, None]
    lanes = np.stack(words(r, nq, site, seed, offset), axis=1)  # [n Cv + q, lane, r]
    return u24(lanes).reshape(n, 4 * cv, hw)[:, :c].reshape(n, c, h, w)


def elem_mask(site: int, n: int, c: int, h: int, w: int, p: float, seed: int, offset: int) -> np.ndarray:
    return _multipliers(elem_u24(site, n, c, h, w, seed, offset), p)


def num_double_convs(s: int) -> int:
    return 3 * s + 6


def sites(s: int, f: int, n: int, h: int, w: int, dropout2d=(0.0, 0.0, 0.0), center: float = 0.0, final: float = 0.0):
    """Every dropout site of a model geometry in site order, as dicts {site, kind ("dropout2d" | "center" | "final<s>"),
    shape, p}: the shapes and numbers `engine.Plan.dropout_mask` documents.  dropout2d = (encoder, core, decoder) rates."""
    enc, core, dec = dropout2d
    chans = ([(f, enc)] * s + [(2 * f, enc)] * s
             + [(c * f * s, core) for c in (4, 8, 8, 4, 2, 1)] + [(f, dec)] * s)
    out = [{"site": i, "kind": "dropout2d", "shape": (n, c), "p": float(p)} for i, (c, p) in enumerate(chans)]
    ndc = len(out)
    assert ndc == num_double_convs(s) and ndc + 1 + s <= MAX_SITES
    out.append({"site": ndc, "kind": "center", "shape": (n, 8 * f * s, h // 16, w // 16), "p": float(center)})
    out += [{"site": ndc + 1 + i, "kind": f"final{i}", "shape": (n, f, h, w), "p": float(final)} for i in range(s)]
    return out


def site_u24(site: dict, seed: int, offset: int) -> np.ndarray:
    fn = dropout2d_u24 if site["kind"] == "dropout2d" else elem_u24
    return fn(site["site"], *site["shape"], seed, offset)


def site_mask(site: dict, seed: int, offset: int) -> np.ndarray:
    """The multipliers of one entry of `sites` (fp32, the site's shape)."""
    return _multipliers(site_u24(site, seed, offset), site["p"])


def used_counters(site: dict):
    """(i0, i1, lane) int64 arrays of every multiplier the site uses — what has to be distinct within a counter word 2."""
    if site["kind"] == "dropout2d":
        e = np.arange(site["shape"][0] * site["shape"][1], dtype=np.int64)
        return e // 4, np.zeros_like(e), e % 4
    n, c, h, w = site["shape"]
    cv = pad8(c) // 4
    ni, ci, ri = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(c), np.arange(h * w), indexing="ij"))
    return ri.astype(np.int64), (ni * cv + ci // 4).astype(np.int64), (ci % 4).astype(np.int64)


# The u == p boundary at p = 0.5: an element whose 24 bits are exactly 2^23, so that float32(u24) * 2^-24 == 0.5 and `>=` keeps
# it where `>` would drop it.  Found by `search_boundary()` below (first hit in its order); verified in
# test_dropout_reference_cpu.py, used on the device in test_dropout_gpu.py.
BOUNDARY_SEED = 0x9E3779B97F4A7C15
BOUNDARY_GEOMETRY = dict(s=2, f=6, n=1, h=32, w=32)  # (32 x 32: the smallest image the engine accepts; C = 6 of pad8 = 8)
BOUNDARY_SEARCH_START = 3 << 32
BOUNDARY_OFFSET = (3 << 32) + 4860  # the 1216th offset searched
BOUNDARY_SITE = 14                  # final_dropouts[1]: ndc = 12, + 1 + 1
BOUNDARY_INDEX = (0, 2, 14, 24)     # (n, c, y, x)


def search_boundary(seed: int, s: int, f: int, n: int, h: int, w: int, max_offsets: int, start_offset: int = 0):
    """Offsets start_offset, +4, ... : the first (offset, final site, index) of a final element-wise site whose u24 is
    2^23, or None.  About 2^24 words are needed on average."""
    table = [t for t in sites(s, f, n, h, w, final=0.5) if t["kind"].startswith("final")]
    for k in range(max_offsets):
        offset = start_offset + 4 * k
        for t in table:
            hit = np.argwhere(site_u24(t, seed, offset) == np.uint64(1 << 23))
            if len(hit):
                return offset, t["site"], tuple(int(v) for v in hit[0])
    return None
