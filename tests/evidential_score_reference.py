"""Definition of the evidential model's scoring rules in numpy float64: PIT, NLL and CRPS of the Student-t posterior
predictive of the Normal-Inverse-Gamma heads (include/mimo_hip.h: mimo_score_accumulate_evidential).

    (mu, v, alpha, beta) = (l0, softplus(l1), softplus(l2) + 1, softplus(l3)),  v, alpha, beta fp32 VALUES
    nu = 2 alpha,  sigma = sqrt(beta (1 + v) / (v alpha)),  z = (y - mu) / sigma

tests/test_evidential_score_reference_cpu.py checks the definition against scipy.stats.t, the CRPS's defining integral
and the Gaussian limit; tests/test_evidential_score_gpu.py runs score_evidential.hip against it.  The incomplete beta
function and the log-gammas come from scipy where it is importable; without it from torch's float64 lgamma and the
bounded continued fraction below, so the GPU test does not need scipy.

Layout: logits [4, N] (channel-major), y [N]."""
import numpy as np
import torch

from tests import scalar_reference as SR

try:
    from scipy import special as _special
except ImportError:  # the GPU test runs without it
    _special = None

CF_CAP = 400       # iterations the reference's continued fraction may take (it stops at convergence)
CF_EPS = 2.0 ** -50
SQRT_PI = 1.7724538509055160273


def softplus64(x):
    """torch's softplus (threshold 20) in float64"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore"):
        return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def heads(logits):
    """(mu, v, alpha, beta) [N] fp32 of logits [4, N] fp32: the softplus evaluated in float64 and rounded to fp32 (alpha as
    the fp32 sum softplus(l2) + 1, csrc/evidential.h: nig_head) — the values the kernel is defined on"""
    l = np.asarray(logits, dtype=np.float32)
    with np.errstate(under="ignore"):
        v = softplus64(l[1]).astype(np.float32)
        alpha = softplus64(l[2]).astype(np.float32) + np.float32(1.0)
        beta = softplus64(l[3]).astype(np.float32)
    return l[0].copy(), v, alpha, beta


def gammaln(x):
    x = np.asarray(x, dtype=np.float64)
    if _special is not None:
        return _special.gammaln(x)
    return torch.lgamma(torch.from_numpy(np.ascontiguousarray(x))).numpy().reshape(x.shape)


def log_beta_half(a):
    """ln B(1/2, a) = ln sqrt(pi) + lgamma(a) - lgamma(a + 1/2)"""
    return np.log(SQRT_PI) + gammaln(a) - gammaln(a + 0.5)


def betainc_cf(a, b, x, log_x, log_1mx, cap=CF_CAP, eps=CF_EPS):
    """I_x(a, b) by the modified Lentz continued fraction (Numerical Recipes betacf), float64, for x < (a + 1) / (a + b + 2);
    log_x = ln x and log_1mx = ln(1 - x) are handed in so that neither is formed by a subtraction.  Bounded: at most `cap`
    iterations, each element stops changing once its last factor is within `eps` of 1.  Returns (I, iterations [N])."""
    a, b, x = (np.asarray(t, dtype=np.float64) for t in (a, b, x))
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = np.ones_like(x)
    d = 1.0 - qab * x / qap
    d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
    h = d.copy()
    live = np.ones(x.shape, bool)
    iters = np.zeros(x.shape, np.int64)
    for m in range(1, cap + 1):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d1 = 1.0 + aa * d
        c1 = 1.0 + aa / c
        d1 = 1.0 / np.where(np.abs(d1) < tiny, tiny, d1)
        c1 = np.where(np.abs(c1) < tiny, tiny, c1)
        h1 = h * d1 * c1
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d2 = 1.0 + aa * d1
        c2 = 1.0 + aa / c1
        d2 = 1.0 / np.where(np.abs(d2) < tiny, tiny, d2)
        c2 = np.where(np.abs(c2) < tiny, tiny, c2)
        de = d2 * c2
        h = np.where(live, h1 * de, h)
        c, d = np.where(live, c2, c), np.where(live, d2, d)
        iters += live
        live = live & ~(np.abs(de - 1.0) < eps)
        if not live.any():
            break
    lnb = gammaln(a) + gammaln(b) - gammaln(a + b)
    with np.errstate(under="ignore", invalid="ignore"):
        front = np.exp(a * log_x + b * log_1mx - lnb) / a
    return np.where(x <= 0.0, 0.0, front * h), iters


def t_tails(nu, z, own=None):
    """(I, J, direct, iterations): I = I_x(nu/2, 1/2) = P(|T| > |z|) and J = I_{1-x}(1/2, nu/2) = P(|T| <= |z|) = 1 - I at
    x = nu / (nu + z^2), each formed without a subtraction: 1 - x is z^2 / (nu + z^2).  `direct` marks where the kernel's
    branch rule x < (a + 1) / (a + 2.5) evaluates I (elsewhere it evaluates J).  own=True forces the reference's own
    continued fraction (which takes the same branch and forms the other tail as the complement); the default uses scipy's
    betainc for both tails where scipy is importable."""
    nu, z = np.asarray(nu, dtype=np.float64), np.asarray(z, dtype=np.float64)
    a, z2 = 0.5 * nu, z * z
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x = np.where(np.isinf(z2), 0.0, nu / (nu + z2))
        xc = np.where(np.isinf(z2), 1.0, z2 / (nu + z2))
        log_x = -np.log1p(z2 / nu)
        log_xc = np.log(xc)
    direct = x < (a + 1.0) / (a + 2.5)
    if own is None:
        own = _special is None
    if not own:  # each tail from the argument that is not rounded next to 1; the other one as its complement
        I_d, J_c = _special.betainc(a, 0.5, x), _special.betainc(0.5, a, xc)
        return np.where(direct, I_d, 1.0 - J_c), np.where(direct, 1.0 - I_d, J_c), direct, np.zeros(z.shape, np.int64)
    half = np.full_like(a, 0.5)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        I_d, it_d = betainc_cf(a, half, np.where(direct, x, 0.5), np.where(direct, log_x, 0.0), np.where(direct, log_xc, 0.0))
        J_c, it_c = betainc_cf(half, a, np.where(direct, 0.0, xc), np.where(direct, 0.0, log_xc), np.where(direct, 0.0, log_x))
    J_c = np.where(xc <= 0.0, 0.0, J_c)
    return np.where(direct, I_d, 1.0 - J_c), np.where(direct, 1.0 - I_d, J_c), direct, np.where(direct, it_d, it_c)


def student_scores(mu, v, alpha, beta, y, own=None, with_iterations=False):
    """{"pit", "nll", "crps"} [N] in float64 of the Student-t predictive (nu = 2 alpha, location mu, scale
    sqrt(beta (1 + v) / (v alpha))) at the label y; no skip rule: every input finite, v > 0, beta > 0.

        PIT   u = I / 2 (z <= 0), 1/2 + J / 2 (z > 0)                       I, J: t_tails
        NLL   -lgamma(alpha + 1/2) + lgamma(alpha) + ln(nu pi) / 2 + ln sigma + (alpha + 1/2) log1p(z^2 / nu)
        CRPS  sigma [ z (2 F - 1) + 2 f (nu + z^2) / (nu - 1) - 2 sqrt(nu) / (nu - 1) B(1/2, nu - 1/2) / B(1/2, nu/2)^2 ]
              (Jordan, Krueger, Lerch 2019), 2 F - 1 = sign(z) J and f the standard t density"""
    mu, v, alpha, beta, y = (np.asarray(t, dtype=np.float64) for t in (mu, v, alpha, beta, y))
    nu = 2.0 * alpha
    sigma = np.sqrt(beta * (1.0 + v) / (v * alpha))
    z = (y - mu) / sigma
    z2 = z * z
    I, J, _, iters = t_tails(nu, z, own)
    pit = np.where(z <= 0.0, 0.5 * I, 0.5 + 0.5 * J)
    pit = np.where(z == 0.0, 0.5, pit)
    lb1 = log_beta_half(alpha)           # ln B(1/2, nu/2)
    lb2 = log_beta_half(nu - 0.5)        # ln B(1/2, nu - 1/2)
    l1p = np.log1p(z2 / nu)
    nll = (lb1 - np.log(SQRT_PI)) + 0.5 * np.log(nu * np.pi) + np.log(sigma) + (alpha + 0.5) * l1p
    with np.errstate(under="ignore"):
        f = np.exp(-(alpha + 0.5) * l1p - 0.5 * np.log(nu) - lb1)
        crps = sigma * (np.abs(z) * J + 2.0 * f * (nu + z2) / (nu - 1.0)
                        - 2.0 * np.sqrt(nu) / (nu - 1.0) * np.exp(lb2 - 2.0 * lb1))
    out = {"pit": pit, "nll": nll, "crps": crps}
    if with_iterations:
        out["iterations"] = iters
    return out


def score_logits(logits, y, own=None):
    """student_scores on heads(logits)"""
    mu, v, alpha, beta = heads(logits)
    return student_scores(mu, v, alpha, beta, y, own)


def valid_pixels(logits, y, mask=None):
    """the skip rule: (scored, masked, nonfinite) boolean [N]; mask == 0 first, then the label or any of the four logits not
    finite, or a head v == 0 or beta == 0 (fp32 softplus underflow: the scale would be infinite or zero)"""
    l = np.asarray(logits, dtype=np.float32)
    masked = np.zeros(np.shape(y), bool) if mask is None else (np.asarray(mask) == 0)
    finite = np.isfinite(y) & np.isfinite(l).all(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        _, v, _, beta = heads(np.where(np.isfinite(l), l, np.float32(0)))
    finite = finite & (v > 0) & (beta > 0)
    return ~masked & finite, masked, ~masked & ~finite


def torch_fn64(mu, head3, y):
    """student_scores as tests/scalar_reference.py's conditioning() calls it: torch tensors mu [N], head3 [N, 3] = (v, alpha,
    beta), y [N] -> {name: float64 tensor [N]}"""
    h = head3.double().numpy()
    r = student_scores(mu.double().numpy(), h[:, 0], h[:, 1], h[:, 2], y.double().numpy())
    return {k: torch.from_numpy(np.ascontiguousarray(r[k])) for k in ("pit", "nll", "crps")}


# floors of the per-element relative error, as tests/test_score_gpu.py sets them for the same three quantities
FLOORS = {"pit": SR.TINY, "nll": SR.frac_floor(SR.FLOOR_SIGNED), "crps": SR.frac_floor(SR.FLOOR_POSITIVE)}


def soft_head_condition(logits, y):
    """{name: the largest COND_MARGIN x conditioning / max(|ref|, floor)} of the three results over the pixels, the conditioning
    being the change of the float64 result when one of v, alpha, beta moves one fp32 ulp (scalar_reference.conditioning)"""
    mu, v, alpha, beta = heads(logits)
    inputs = [torch.from_numpy(mu), torch.from_numpy(np.stack([v, alpha, beta], axis=1)), torch.from_numpy(y)]
    cond = SR.conditioning(torch_fn64, inputs, 1)
    ref = torch_fn64(*[SR.to64(t) for t in inputs])
    out = {}
    for k in ref:
        fl = FLOORS[k](ref[k]) if callable(FLOORS[k]) else FLOORS[k]
        out[k] = float((SR.COND_MARGIN * cond[k] / torch.maximum(ref[k].abs(), torch.as_tensor(fl, dtype=torch.float64))).max())
    return out


# ---- input generators (all fp32) ----------------------------------------------------------------------------------------

def _labels(rng, logits, zmax, tail_df=3.0):
    """labels z sigma away from mu with z heavy-tailed (t_3 scaled) and clipped to +-zmax, rounded to fp32"""
    mu, v, alpha, beta = (t.astype(np.float64) for t in heads(logits))
    sigma = np.sqrt(beta * (1.0 + v) / (v * alpha))
    z = np.clip(rng.standard_t(tail_df, size=mu.size) * (zmax / 6.0), -zmax, zmax)
    z[::11] = rng.uniform(-zmax, zmax, size=z[::11].size)
    return (mu + z * sigma).astype(np.float32)


def exact_head_inputs(rng, N, zmax=30.0):
    """logits [4, N], y [N] whose heads are exact: l1, l3 in (20, 1e3] and l2 in (20, 2e4] a multiple of 2^-8 (softplus
    returns its argument above 20 and l2 + 1 is exact in fp32), log-uniform; labels with |z| up to about zmax"""
    lo = np.log(20.5)
    l1 = np.exp(rng.uniform(lo, np.log(1e3), N)).astype(np.float32)
    l3 = np.exp(rng.uniform(lo, np.log(1e3), N)).astype(np.float32)
    l2 = (np.round(np.exp(rng.uniform(lo, np.log(2e4), N)) * 256.0) / 256.0).astype(np.float32)
    assert np.all((l2.astype(np.float64) + 1.0) == (l2 + np.float32(1)).astype(np.float64)) and l1.min() > 20 and l2.min() > 20
    logits = np.stack([rng.standard_normal(N).astype(np.float32), l1, l2, l3])
    return logits, _labels(rng, logits, zmax)


def soft_head_inputs(rng, N, zmax=8.0, span=9.0):
    """logits [4, N], y [N]: l1, l2, l3 uniform in [-span, span], every 13th l2 = -30 (alpha == 1 exactly); |z| <= zmax"""
    logits = np.stack([rng.standard_normal(N)] + [rng.uniform(-span, span, N) for _ in range(3)]).astype(np.float32)
    logits[2, ::13] = -30.0
    return logits, _labels(rng, logits, zmax)
