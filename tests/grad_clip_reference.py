"""Reference, input generators and case list for mimo_adam_step_clipped (gradient clipping fused into the flat Adam step):
torch.nn.utils.clip_grad_norm_ / clip_grad_value_ followed by Adam, with the kernel's documented skip rule, in plain torch.

Dtype-generic like tests/scalar_reference.py: on fp32 tensors it is the fp32 torch reference, on the same values in fp64 the
truth.  tests/test_grad_clip_cpu.py pins it to torch's own clipping + torch.optim.Adam, tests/test_grad_clip_gpu.py runs
the kernels against it."""
import math

import numpy as np
import torch

from tests import scalar_reference as R

SIZES = (1, 5, 1027, 2097159)  # 2097159 = one 4-element group + a 3-element tail past a full 2048 x 256 x 4 grid pass
# The sum-of-squares kernel issues four 16-byte loads a lane per trip while four grid strides (2048 x 256 groups of 4 each)
# still fit; below 4 strides + 1 group only its one-load loop runs.  6 strides + 1 group + 3: one four-load trip for every
# lane, two one-load trips, a third for lane 0 of workgroup 0, and the scalar tail — every hand-over in one size.
SUMSQ_STRIDE = 2048 * 256
LOOP_SIZE = 4 * (6 * SUMSQ_STRIDE + 1) + 3  # 12 582 919
NORM_SIZES = SIZES + (LOOP_SIZE,)
STEPS = (1, 2, 1000)
WDS = (0.0, 1e-2)
CLIP_EPS = 1e-6                # torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6)
NORM_SCALE, NORM_AMP = 0.125, 1024.0  # grad_scale / amp_scale of the norm-bound test: the fp32 quotient is exact


def effective_scale(grad_scale, amp_scale=None):
    """s as the kernel forms it: the float argument, divided in fp32 by the loss scale when there is one"""
    s = np.float32(grad_scale)
    if amp_scale is not None:
        s = s / np.float32(amp_scale)
    return float(np.float32(s))


def norm_and_coef(g, s, clip):
    """(norm, coef) of ge = g * s in g's dtype: sqrt(sum ge^2), min(1, clip / (norm + 1e-6))"""
    norm = torch.linalg.vector_norm(g * s)
    coef = torch.clamp(R.f32(clip) / (norm + CLIP_EPS), max=1.0)
    return norm, coef


def clip_reference(p, g, m, v, *, step, mode, clip, wd=0.0, grad_scale=1.0, amp_scale=None, found_inf=0.0, lr=1e-3):
    """One clipped step in the tensors' dtype.  mode "norm": clip_grad_norm_(max_norm = clip); "value": clip_grad_value_.
    Skip rule (the kernel's, not torch's): found_inf != 0 or a norm that is not finite leaves p, m, v untouched.
    Returns p, m, v, norm, coef (value mode: 0 and 1) and `applied`."""
    s = effective_scale(grad_scale, amp_scale)
    ge = g * s
    if mode == "norm":
        norm, coef = norm_and_coef(g, s, clip)
        finite = bool(torch.isfinite(norm))
        gc = ge * coef
    else:
        norm, coef, finite = torch.zeros((), dtype=g.dtype), torch.ones((), dtype=g.dtype), True
        gc = ge.clamp(-R.f32(clip), R.f32(clip))
    if found_inf != 0.0 or not finite:
        return {"p": p.clone(), "m": m.clone(), "v": v.clone(), "norm": norm, "coef": coef, "applied": False}
    out = R.adam_reference(p, gc, m, v, step=step, lr=lr, wd=wd, grad_scale=1.0)
    out.update(norm=norm, coef=coef, applied=True)
    return out


def clip_inputs(n, step):
    """p, g, m, v of tests/scalar_reference.py's Adam tests (g ~ N(0, 1): norm about sqrt(n)) with p carrying g's sign, as m
    does there and for the same reason: clipping 10-fold brings g * coef (~ 0.1) within reach of wd * p (~ 0.01), and where
    the two cancel — to 1 / 137 of either at one element of the n = 1027 draw — the relative error of m = (1 - beta1)(g coef +
    wd p) is the rounding of the clipped gradient times that factor, in the fp32 torch reference as in the kernel: the
    conditioning of the sum, not the arithmetic of either.  With equal signs nothing cancels."""
    p, g, m, v = R.adam_inputs(n, step)
    return torch.sign(g) * p.abs(), g, m, v


OPPOSED_SIZES = (1027, 2097159)  # the bit-identity case on the unsigned draw (p's sign independent of g's)


def norm64(g, grad_scale=1.0, amp_scale=None):
    return float(torch.linalg.vector_norm(g.double() * effective_scale(grad_scale, amp_scale)))


def clip_for(g, factor, grad_scale=1.0, amp_scale=None):
    """the bound factor x the fp64 norm of the effective gradient, as the float the C ABI carries"""
    return R.f32(factor * norm64(g, grad_scale, amp_scale))


ACTIVE, INACTIVE = 0.1, 100.0  # clip / norm: clipping by 10 x, no clipping
VALUE_CLIP = 0.5               # value mode: about 62 % of N(0, 1) draws are clamped


def per_element_cases(n):
    """(step, wd, mode, grad_scale) of the per-element test: every step / weight decay / mode for the small sizes, a diagonal
    for the large one"""
    full = [(step, wd, mode, gs) for step in STEPS for wd in WDS for mode in ("norm", "value") for gs in (1.0, 1.0 / 3.0)]
    if n < 100000:
        return full
    return [(1, 0.0, "norm", 1.0), (2, 1e-2, "value", 1.0 / 3.0), (1000, 1e-2, "norm", 1.0 / 3.0), (1000, 0.0, "value", 1.0)]


def identity_cases(n):
    """(step, wd, amp) of the bit-identity tests; amp: None, or (amp_scale, found_inf = 0)"""
    full = [(step, wd, amp) for step in (1, 1000) for wd in WDS for amp in (None, 1024.0)]
    if n == LOOP_SIZE:
        return [(1000, 1e-2, 1024.0)]
    return full if n < 100000 else [(1, 0.0, None), (1000, 1e-2, 1024.0)]


def all_norm_draws():
    """every (g, grad_scale, amp_scale, clip) the GPU tests clip by norm on random draws"""
    for n in NORM_SIZES:
        for step, wd, mode, gs in per_element_cases(n) if n in SIZES else ():
            if mode == "norm":
                g = clip_inputs(n, step)[1]
                yield g, gs, None, clip_for(g, ACTIVE, gs)
        for step, wd, amp in identity_cases(n):
            g = clip_inputs(n, step)[1]
            gsc = 1.0 if amp is None else amp  # the gradient carries the loss scale, the kernel divides it out
            yield g * gsc, 1.0, amp, clip_for(g * gsc, INACTIVE, 1.0, amp)
            yield g * gsc, 1.0 / 3.0, amp, clip_for(g * gsc, ACTIVE, 1.0 / 3.0, amp)
        g = clip_inputs(n, 1)[1]
        for factor in (ACTIVE, INACTIVE):
            yield g, NORM_SCALE, NORM_AMP, clip_for(g, factor, NORM_SCALE, NORM_AMP)
        g = clip_inputs(n, 2)[1]
        yield g, 1.0 / 3.0, None, clip_for(g, ACTIVE, 1.0 / 3.0)  # the two-runs test
        yield g, 1.0, None, 1.0                                    # the found_inf skip (sizes 5 and 2097159)
    for n in OPPOSED_SIZES:
        g = R.adam_inputs(n, 2)[1]
        yield g, 1.0 / 3.0, None, clip_for(g, ACTIVE, 1.0 / 3.0)  # the opposing-signs identity


def integer_gradients():
    """[(name, g, exact norm)]: every g = 2 with n = 4^k (norm 2 * 2^k; 4^12 = 8 grid strides of the sum-of-squares kernel:
    two four-load trips and nothing else), and g in {0, 3, 4} with a threes and a fours, a = j^2 (sum = 25 j^2, norm 5 j),
    scattered by a fixed permutation (at LOOP_SIZE over the four-load trip, the one-load trips and the tail)"""
    cases = [(f"twos n=4^{k}", torch.full((4 ** k,), 2.0), 2.0 * 2 ** k) for k in (0, 1, 5, 11, 12)]
    for n, j in ((1027, 2), (2097159, 100), (LOOP_SIZE, 500)):
        gen = torch.Generator().manual_seed(n)
        perm = torch.randperm(n, generator=gen)
        ends = torch.tensor([n - 1, n - 4])  # the scalar tail and the last 16-byte group always carry a value
        where = torch.cat([ends, perm[(perm != n - 1) & (perm != n - 4)][: 2 * j * j - 2]])
        g = torch.zeros(n)
        g[where[: j * j]] = 3.0
        g[where[j * j:]] = -4.0
        cases.append((f"0/3/4 n={n}", g, 5.0 * j))
    return cases


NORM_BOUND = 4.0 * 2.0 ** -24
# (derivation: squares in fp32, the sum in double — g * s <= 2^-24, the square <= 1/2 * 2^-24 on the norm, the final rounding
# <= 2^-24: below 2.5 * 2^-24; stated with the test that uses it)
COEF_BOUND = 2.0 * 2.0 ** -24  # the norm's rounding to fp32 (the reported value) and the coefficient's own


def coef_from_reported_norm(norm32, clip):
    return min(1.0, R.f32(clip) / (float(norm32) + CLIP_EPS))


def is_unambiguous(g, grad_scale, amp_scale, clip):
    """no draw sits where fp32 and fp64 could disagree about whether clipping happened"""
    n, c = norm_and_coef(g.double(), effective_scale(grad_scale, amp_scale), clip)
    n, c = float(n), float(c)
    return (c == 1.0 and n <= 0.99 * R.f32(clip)) or c <= 0.999, (n, c)


assert math.isclose(effective_scale(NORM_SCALE, NORM_AMP), NORM_SCALE / NORM_AMP, rel_tol=0.0)
