"""Definition of the mixture scoring rules (PIT, NLL, CRPS of the equal-weight mixture of S Laplace or S Gaussian members)
in numpy, dtype-generic: run in float64 it is the reference, run on the same values in float32 it is the yardstick — the
same formulas with every operation rounded to fp32 — whose distance from the float64 result is what fp32 arithmetic itself
does on that input (the rule of tests/scalar_reference.py).  tests/test_score_reference_cpu.py checks the definition against
numerical integration and scipy; tests/test_score_gpu.py runs score_rules.hip against it.

Layout: mu, p2 [S, N] (member-major), y [N].  erf / erfc come from torch's CPU operators (numpy has none), in either dtype."""
import numpy as np
import torch

LOSSES = ("laplace_nll", "gaussian_nll")
EPS_MIN, EPS_MAX = 1e-5, 1e3


def f32(x):
    """the value a C float argument carries"""
    return float(np.float32(x))


def _erf(x):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy().reshape(np.shape(x))


def _erfc(x):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(x))).numpy().reshape(np.shape(x))


def member_scale(p2, dtype, eps_min=EPS_MIN, eps_max=EPS_MAX):
    """theta = clamp(exp(p2), eps_min, eps_max) with the clamps as the floats the C ABI carries: the Laplace b, the Gaussian
    variance"""
    with np.errstate(over="ignore", under="ignore"):
        return np.clip(np.exp(np.asarray(p2, dtype=dtype)), dtype(f32(eps_min)), dtype(f32(eps_max)))


def gauss_abs_mean(m, s):
    """A(m, s) = E|N(m, s^2)| = 2 s phi(m / s) + m (2 Phi(m / s) - 1)"""
    dt = m.dtype.type
    z = m / s
    with np.errstate(under="ignore"):
        return dt(2) * s * (dt(0.3989422804014327) * np.exp(dt(-0.5) * z * z)) + m * _erf(z * dt(0.7071067811865476))


def laplace_pair(D, si, sj):
    """E|X_i - X_j'| of two Laplace members D = |mu_i - mu_j| apart, without the cancellation of
    (b_i^3 e^{-D/b_i} - b_j^3 e^{-D/b_j}) / (b_i^2 - b_j^2): every term positive at any pair of scales"""
    dt = D.dtype.type
    bi, bj = np.minimum(si, sj), np.maximum(si, sj)
    tot = bi + bj
    with np.errstate(under="ignore", invalid="ignore", divide="ignore", over="ignore"):
        x = D * (bi - bj) / (bi * bj)
        g = np.where(x == 0, dt(1), np.expm1(x) / np.where(x == 0, dt(1), x))
        t1 = np.exp(-D / bi) * ((bi * bi + bi * bj + bj * bj) / tot)
        t2 = np.exp(-D / bj) * (bj / tot) * (bj / bi) * D * g
    return D + t1 + t2


def laplace_pair_quotient(D, bi, bj):
    """the textbook form (float64, b_i != b_j): what laplace_pair restates"""
    return D + (bi ** 3 * np.exp(-D / bi) - bj ** 3 * np.exp(-D / bj)) / (bi ** 2 - bj ** 2)


def member_terms(d, sc, loss):
    """per member at d = y - mu: F(y), log f(y), E|X - y| and E|X - X'|"""
    dt = d.dtype.type
    with np.errstate(under="ignore", over="ignore"):
        if loss == "laplace_nll":
            ad = np.abs(d)
            r = ad / sc
            e = np.exp(-r)
            return np.where(d < 0, dt(0.5) * e, dt(1) - dt(0.5) * e), -r - np.log(dt(2) * sc), ad + sc * e, dt(1.5) * sc
        sd = np.sqrt(sc)
        z = d / sd
        F = dt(0.5) * _erfc(-z * dt(0.7071067811865476))
        lf = dt(-0.5) * z * z - np.log(sd) - dt(0.9189385332046727)
        return F, lf, gauss_abs_mean(d, sd), dt(2) * sd * dt(0.5641895835477563)


def pair_sum(mu, sc, loss):
    """sum over i < j of c_ij, [N]"""
    S = mu.shape[0]
    total = np.zeros(mu.shape[1:], dtype=mu.dtype)
    for i in range(S - 1):
        D = np.abs(mu[i][None] - mu[i + 1:])
        if loss == "laplace_nll":
            c = laplace_pair(D, np.broadcast_to(sc[i][None], D.shape), sc[i + 1:])
        else:
            c = gauss_abs_mean(D, np.sqrt(sc[i][None] + sc[i + 1:]))
        total = total + c.sum(axis=0, dtype=mu.dtype)
    return total


def score(mu, p2, y, loss, dtype=np.float64, eps_min=EPS_MIN, eps_max=EPS_MAX):
    """{"pit", "nll", "crps"} [N] of the mixture in `dtype` (no skip rule: every input finite)"""
    assert loss in LOSSES
    dt = dtype
    mu, y = np.asarray(mu, dtype=dt), np.asarray(y, dtype=dt)
    sc = member_scale(p2, dt, eps_min, eps_max)
    S = mu.shape[0]
    F, lf, a, diag = member_terms(y[None] - mu, sc, loss)
    m = lf.max(axis=0)
    with np.errstate(under="ignore"):
        nll = -(m + np.log(np.exp(lf - m[None]).sum(axis=0, dtype=dt) / dt(S)))
    pit = F.sum(axis=0, dtype=dt) / dt(S)
    crps = a.sum(axis=0, dtype=dt) / dt(S) - (dt(2) * pair_sum(mu, sc, loss) + diag.sum(axis=0, dtype=dt)) / dt(2 * S * S)
    return {"pit": pit, "nll": nll, "crps": crps}


def valid_pixels(mu, p2, y, mask=None):
    """the skip rule: (scored, masked, nonfinite) boolean [N]; mask == 0 first, then any of the 2 S + 1 inputs not finite"""
    masked = np.zeros(np.shape(y), bool) if mask is None else (np.asarray(mask) == 0)
    finite = np.isfinite(y) & np.isfinite(mu).all(axis=0) & np.isfinite(p2).all(axis=0)
    return ~masked & finite, masked, ~masked & ~finite


def pit_bins(pit, expected_p32):
    """counts [K + 1]: bin j = first k with u < p_k over the fp32 thresholds, bin K = never below"""
    p = np.asarray(expected_p32, dtype=np.float32)
    j = np.searchsorted(p, np.asarray(pit, dtype=np.float32), side="right")
    return np.bincount(j, minlength=p.size + 1).astype(np.int64)


def summarize(pit, nll, crps, expected_p, n_masked=0, n_nonfinite=0):
    """what PredictiveScorer.compute() returns, in float64 from per-pixel values of the scored pixels; expected_p float64
    (the thresholds are compared as fp32)"""
    p = np.asarray(expected_p, dtype=np.float64)
    K, n = p.size, int(np.size(pit))
    counts = pit_bins(pit, p.astype(np.float32))
    nan = float("nan")
    observed = np.cumsum(counts)[:K] / n if n else np.full(K, nan)
    mean = lambda v: float(np.asarray(v, dtype=np.float64).sum() / n) if n else nan
    coverage = {float(p[K - 1 - k] - p[k]): float(observed[K - 1 - k] - observed[k]) for k in range(K // 2)
                if abs(p[k] + p[K - 1 - k] - 1.0) <= 1e-12}
    return {"n": n, "n_masked": int(n_masked), "n_nonfinite": int(n_nonfinite), "nll": mean(nll), "crps": mean(crps),
            "pit_mean": mean(pit), "calibration": {"expected": p.copy(), "observed": observed},
            "calibration_error": float(np.mean(np.abs(observed - p))), "coverage": coverage, "counts": counts}


def mixture_cdf(x, mu, sc, loss):
    """F(x) of the mixture at scalar x (float64; mu, sc [S]): the integrand of the CRPS's defining integral"""
    d = np.float64(x) - mu
    if loss == "laplace_nll":
        F = np.where(d < 0, 0.5 * np.exp(-np.abs(d) / sc), 1 - 0.5 * np.exp(-np.abs(d) / sc))
    else:
        F = 0.5 * _erfc(-d / np.sqrt(2 * sc))
    return float(F.mean())


def sample_mixture(rng, mu, sc, loss, n):
    """n draws from the mixture (mu, sc [S] float64)"""
    k = rng.integers(0, mu.size, size=n)
    if loss == "laplace_nll":
        return mu[k] + rng.laplace(0.0, 1.0, size=n) * sc[k]
    return mu[k] + rng.standard_normal(n) * np.sqrt(sc[k])


def random_members(rng, S, N, spread=1.0, log_scale=(-3.0, 0.5)):
    """fp32 (mu, p2, y) of N pixels: means around a common centre, log-scales uniform in `log_scale`, labels within a few
    scales of the means"""
    centre = rng.standard_normal(N)
    mu = (centre[None] + spread * 0.3 * rng.standard_normal((S, N))).astype(np.float32)
    p2 = rng.uniform(log_scale[0], log_scale[1], size=(S, N)).astype(np.float32)
    y = (centre + 0.5 * rng.standard_normal(N)).astype(np.float32)
    return mu, p2, y
