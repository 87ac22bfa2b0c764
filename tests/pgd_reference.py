"""numpy fp32 restatement of the PGD kernels (csrc/pgd.hip: `mimo_pgd_step`, `mimo_pgd_init`) and a plain loop with the
chunk rule of `mimo.adversarial.pgd_sweep`.  Holds no device code; the GPU tests (test_pgd_gpu.py) compare the kernels and the
sweep with it bit for bit, the CPU tests (test_pgd_reference_cpu.py) check the definition itself.

    step:   s = sign(g)  (+-0 -> 0, NaN -> NaN);  v = x_adv + alpha * s  (the product is exact: one rounding)
            v = clamp(v, fl(x0 - eps), fl(x0 + eps));  x_adv = clamp(v, lo, hi)        clamp(v, a, b) = a if v < a else b if v > b else v
    start:  quad q = elements 4 q .. 4 q + 3 takes the words of
            philox4x32_10(ctr = (lo32(q), hi32(q), lo32(offset) ^ 0xFF000000, hi32(offset)), key = (lo32(seed), hi32(seed))),
            element 4 q + j word j;  r = (2 (w >> 8) + 1 - 2^24) * 2^-24;  x_adv[k] = clamp(fl(x0 + fl(eps_k * r)), lo, hi)
"""
import numpy as np

from tests import perm_reference as P

_M32 = 0xFFFFFFFF
START_SITE = 0xFF  # the site number of the random start in the dropout draws' counter word 2 (dropout sites are < 56)
F32 = np.float32


def sign(g):
    g = np.asarray(g, dtype=F32)
    return np.where(g > 0, F32(1), np.where(g < 0, F32(-1), np.where(g == 0, F32(0), g))).astype(F32)


def clamp(v, lo, hi):
    """The kernels' compare form: a NaN (and the sign of a zero) passes."""
    v = np.asarray(v, dtype=F32)
    lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(F32)


def pgd_step(x0, grad, x_adv, eps, alpha, lo=0.0, hi=1.0):
    """x0 [*shape]; grad, x_adv [K, *shape]; eps, alpha [K] -> the new x_adv [K, *shape] (a fresh array)."""
    x0, grad, x_adv = (np.asarray(t, dtype=F32) for t in (x0, grad, x_adv))
    out = np.empty_like(x_adv)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(x_adv.shape[0]):
            e, a = F32(eps[k]), F32(alpha[k])
            v = (x_adv[k] + (a * sign(grad[k])).astype(F32)).astype(F32)
            v = clamp(v, (x0 - e).astype(F32), (x0 + e).astype(F32))
            out[k] = clamp(v, F32(lo), F32(hi))
    return out


def start_counter_word2(offset: int) -> int:
    return (offset & _M32) ^ (START_SITE << 24)


def start_counters(elems: int, offset: int):
    """(c0, c1, c2, c3) uint64 arrays, one counter per quad, shared by the vector and the scalar path."""
    q = np.arange((elems + 3) // 4, dtype=np.uint64)
    return (q & np.uint64(_M32), q >> np.uint64(32), np.full(q.shape, start_counter_word2(offset), dtype=np.uint64),
            np.full(q.shape, (offset >> 32) & _M32, dtype=np.uint64))


def start_words(elems: int, seed: int, offset: int) -> np.ndarray:
    """[elems] uint64: the 32-bit word behind every element (the tail quad's unused words dropped)."""
    lanes = np.stack(P.philox4x32_10(*start_counters(elems, offset), seed & _M32, (seed >> 32) & _M32), axis=1)  # [q, lane]
    return lanes.reshape(-1)[:elems]


def unit(word):
    """r = (2 (w >> 8) + 1 - 2^24) * 2^-24 as fp32: exact (an odd integer below 2^24 times a power of two)."""
    t = 2 * (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.int64) + 1 - (1 << 24)
    return t.astype(F32) * F32(2.0 ** -24)


def pgd_init(x0, eps, lo, hi, seed: int, offset: int):
    """[K, *x0.shape]"""
    x0 = np.asarray(x0, dtype=F32)
    r = unit(start_words(x0.size, seed, offset)).reshape(x0.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([clamp((x0 + (F32(e) * r).astype(F32)).astype(F32), F32(lo), F32(hi)) for e in eps])


def step_sizes(eps, steps, step_size=None, rel_step_size=2.5):
    return [float(step_size) if step_size is not None else rel_step_size * float(e) / steps for e in eps]


def level_chunks(levels: int, batch: int, limit: int, mc_dropout: bool = False):
    chunk = 1 if mc_dropout else max(1, limit // batch)
    return [(k0, min(levels, k0 + chunk)) for k0 in range(0, levels, chunk)]


def reference_sweep(gradient_fn, x0, eps, steps, limit, step_size=None, rel_step_size=2.5, lo=0.0, hi=1.0, start=None,
                    mc_dropout=False):
    """{eps: perturbed [B, ...]} of the sweep.  gradient_fn(stacked [Kc * B, ...] float32, levels Kc) -> the gradient of the
    stacked batch, same shape (the caller repeats label and mask).  The levels with eps > 0 are stacked in the order given,
    max(1, limit // B) per call (one with mc_dropout); levels with eps = 0 stay at their start.  start: [K, B, ...] in the
    order of `eps` (the random start), or None for clamp(x0, lo, hi)."""
    x0 = np.asarray(x0, dtype=F32)
    eps = [float(e) for e in eps]
    b = x0.shape[0]
    x_adv = np.stack([clamp(x0, lo, hi)] * len(eps)) if start is None else np.array(start, dtype=F32)
    pos = [k for k, e in enumerate(eps) if e > 0.0]
    alpha = step_sizes(eps, steps, step_size, rel_step_size)
    for _ in range(steps):
        for k0, k1 in level_chunks(len(pos), b, limit, mc_dropout):
            ks = pos[k0:k1]
            stacked = x_adv[ks].reshape((len(ks) * b,) + x0.shape[1:])
            grad = np.asarray(gradient_fn(stacked, len(ks)), dtype=F32).reshape((len(ks),) + x0.shape)
            x_adv[ks] = pgd_step(x0, grad, x_adv[ks], [eps[k] for k in ks], [alpha[k] for k in ks], lo, hi)
    return {e: x_adv[k] for k, e in enumerate(eps)}
