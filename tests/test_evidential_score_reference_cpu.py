"""The definition of the evidential model's scoring rules (tests/evidential_score_reference.py) against independent
statements of the same quantities — scipy.stats.t, the CRPS's defining integral, the Gaussian limit, the gamma-ratio
identities the kernel rests on — and the host half of `PredictiveScorer.update_evidential` (no GPU)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import evidential_score_reference as E
from tests import scalar_reference as SR
from tests import score_reference as R
from tests.helpers import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def head_values(rng, gen, n):
    logits, y = gen(rng, n)
    return E.heads(logits) + (y,)


@pytest.mark.parametrize("gen", [E.exact_head_inputs, E.soft_head_inputs])
def test_nll_and_pit_are_scipys_student_t(gen):
    stats = pytest.importorskip("scipy.stats")
    mu, v, alpha, beta, y = (t.astype(np.float64) for t in head_values(np.random.default_rng(3), gen, 20000))
    sigma = np.sqrt(beta * (1 + v) / (v * alpha))
    dist = stats.t(df=2 * alpha, loc=mu, scale=sigma)
    got = E.student_scores(mu, v, alpha, beta, y)
    assert np.allclose(got["nll"], -dist.logpdf(y), rtol=1e-10, atol=1e-10)
    cdf = dist.cdf(y)
    rel = np.abs(got["pit"] - cdf) / np.maximum(cdf, 1e-300)
    report(f"student-t reference vs scipy.stats.t.cdf ({gen.__name__}): worst relative difference {rel.max():.2e}")
    assert rel.max() <= 1e-9  # the lower tail is relative: 1e-190 at z = -30 and nu = 4e4


def test_crps_closed_form_is_the_defining_integral():
    integrate = pytest.importorskip("scipy.integrate")
    stats = pytest.importorskip("scipy.stats")
    for nu in (2.0, 2.5, 7.3, 40.0, 3000.0):
        for z in (-3.0, 0.0, 0.4, 12.0):
            alpha, v, beta = nu / 2, 1.0, nu / 4  # sigma = sqrt(beta 2 / alpha) = 1
            got = float(E.student_scores(np.array([0.0]), np.array([v]), np.array([alpha]), np.array([beta]), np.array([z]))["crps"][0])
            f = lambda x: (stats.t.cdf(x, nu) - (1.0 if x >= z else 0.0)) ** 2
            val = err = 0.0
            for a, b in ((-np.inf, min(z, 0.0)), (min(z, 0.0), max(z, 0.0)), (max(z, 0.0), np.inf)):
                if a < b:
                    q, e = integrate.quad(f, a, b, epsabs=1e-13, epsrel=1e-13, limit=400)
                    val, err = val + q, err + e
            report(f"student-t crps nu={nu} z={z}: closed {got:.15e} quad {val:.15e} diff {abs(got - val):.1e} abserr {err:.1e}")
            assert abs(got - val) <= err + 1e-10 * abs(val)


def test_large_nu_is_the_gaussian_of_one_member():
    """nu = 2e7: the Student-t is the Gaussian N(mu, sigma^2) up to terms of z^4 / (4 nu) in the log-density (1e-6 at
    |z| <= 3; the lgamma difference at alpha = 1e7 is good to 1e-7); against score_reference at S = 1"""
    rng = np.random.default_rng(5)
    n = 2000
    alpha = np.full(n, 1e7)
    var = np.exp(rng.uniform(-3, 1, n))
    mu = rng.standard_normal(n)
    y = mu + rng.uniform(-3, 3, n) * np.sqrt(var)
    v = np.ones(n)
    beta = var * alpha / 2  # sigma^2 = beta 2 / alpha
    got = E.student_scores(mu, v, alpha, beta, y)
    ref = R.score(mu[None], np.log(var)[None], y, "gaussian_nll", eps_min=1e-30, eps_max=1e30)
    for k, tol in (("pit", 1e-6), ("nll", 1e-5), ("crps", 1e-6)):
        d = np.abs(got[k] - ref[k]).max()
        report(f"student-t at nu = 2e7 vs the Gaussian member, {k}: worst difference {d:.2e}")
        assert d <= tol, k


def test_gamma_ratio_identities():
    """B(1/2, nu/2) = 4 sqrt(pi) G(alpha + 1/2) and B(1/2, nu - 1/2) = 4 sqrt(pi) G(2 alpha), G(a) = Gamma(a - 1/2) / (4 Gamma(a))
    (csrc/evidential.h: nig_gamma); and the series the kernel takes G from, against mpmath-free float64 lgammas"""
    special = pytest.importorskip("scipy.special")
    alpha = np.exp(np.linspace(0.0, np.log(3.0e4), 400))
    nu = 2 * alpha
    G = lambda a: np.exp(special.gammaln(a - 0.5) - special.gammaln(a)) / 4
    assert np.allclose(special.beta(0.5, nu / 2), 4 * np.sqrt(np.pi) * G(alpha + 0.5), rtol=1e-10)
    assert np.allclose(np.exp(special.betaln(0.5, nu - 0.5)), 4 * np.sqrt(np.pi) * G(2 * alpha), rtol=1e-10)
    assert np.allclose(E.log_beta_half(alpha), special.betaln(0.5, alpha), rtol=0, atol=1e-10)

    def series(a):  # student_t.h: gamma_half_ratio
        a = a.copy()
        num, den = np.ones_like(a), np.ones_like(a)
        for _ in range(15):
            low = a < 16.0
            num, den, a = np.where(low, num * a, num), np.where(low, den * (a - 0.5), den), np.where(low, a + 1, a)
        i = 1 / a
        P = i * (0.375 + i * (0.125 + i * (3 / 64 + i * (1 / 64 + i * (3 / 640 + i / 384)))))
        return num * np.exp(P) / (den * np.sqrt(a))
    # the series is good to 1e-11 (8.7e-12 against 40-digit arithmetic on [1.5, 6.1e4]); the float64 lgamma difference it is
    # compared with here carries the rounding of two lgammas of size a ln a
    for a in (alpha + 0.5, 2 * alpha):
        rel = np.abs(series(a) / (4 * G(a)) - 1)
        report(f"gamma_half_ratio series against exp(lgamma difference): worst relative difference {rel.max():.2e}")
        assert np.all(rel <= 1e-11 + 4 * np.finfo(np.float64).eps * np.abs(special.gammaln(a)))


def test_own_continued_fraction_against_betainc():
    special = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(7)
    n = 50000
    nu = np.exp(rng.uniform(np.log(2.0), np.log(6.0e4), n))
    z = np.clip(rng.standard_t(3, n) * 10, -1e3, 1e3)
    z[:100] = 0.0
    I, J, direct, it = E.t_tails(nu, z, own=True)
    I_s, J_s, direct_s, _ = E.t_tails(nu, z, own=False)
    assert np.array_equal(direct, direct_s) and direct.any() and (~direct).any()
    for name, a, b in (("upper", I, I_s), ("centre", J, J_s)):
        rel = np.abs(a - b) / np.maximum(b, 1e-300)
        report(f"own continued fraction vs scipy betainc, {name} tail: worst relative difference {rel.max():.2e}; "
               f"iterations at most {int(it.max())}")
        assert rel.max() <= 1e-9
    assert it.max() < E.CF_CAP and np.all(J[:100] == 0) and np.all(I[:100] == 1)
    xt = (nu / 2 + 1) / (nu / 2 + 2.5)  # |z| on either side of the branch limit: where the count peaks
    for s in (0.999, 1.001):
        _, _, _, it = E.t_tails(nu, np.sqrt(nu * (1 - xt) / xt) * s, own=True)
        report(f"own continued fraction at {s} x the branch limit's |z|: iterations at most {int(it.max())}")
        assert it.max() < E.CF_CAP
    a = E.student_scores(np.zeros(n), np.ones(n), nu / 2, nu / 4, z, own=True)
    b = E.student_scores(np.zeros(n), np.ones(n), nu / 2, nu / 4, z, own=False)
    for k in ("pit", "nll", "crps"):
        assert np.allclose(a[k], b[k], rtol=1e-9, atol=1e-300), k
    assert np.all(a["pit"][:100] == 0.5)


def test_heads_and_skip_rule():
    logits = np.zeros((4, 9), np.float32)
    logits[2, 0] = -30.0                  # alpha == 1 exactly: scored
    logits[1, 1] = -120.0                 # v underflows
    logits[3, 2] = -120.0                 # beta underflows
    logits[0, 3] = np.nan
    logits[2, 4] = np.inf
    logits[3, 5] = -np.inf
    logits[2, 8] = 25.0                   # above the threshold: softplus returns its argument
    y = np.zeros(9, np.float32)
    y[6] = np.inf
    mask = np.ones(9, np.float32)
    mask[[5, 7]] = 0                      # masked first
    mu, v, alpha, beta = E.heads(np.where(np.isfinite(logits), logits, 0))
    assert alpha[0] == 1.0 and v[1] == 0.0 and beta[2] == 0.0 and alpha[8] == 26.0 and alpha.dtype == np.float32
    t = torch.nn.functional.softplus(torch.tensor([-9.0, -1.0, 0.0, 3.0, 19.0, 21.0], dtype=torch.float64)).float().numpy()
    assert np.array_equal(E.heads(np.stack([np.zeros(6, np.float32)] + [np.array([-9, -1, 0, 3, 19, 21], np.float32)] * 3))[1], t)
    ok, masked, bad = E.valid_pixels(logits, y, mask)
    assert list(np.flatnonzero(ok)) == [0, 8] and list(np.flatnonzero(masked)) == [5, 7]
    assert list(np.flatnonzero(bad)) == [1, 2, 3, 4, 6]
    r = E.score_logits(logits[:, [0, 8]], y[[0, 8]])
    assert all(np.all(np.isfinite(r[k])) for k in r) and np.all(r["pit"] == 0.5)


def test_soft_head_condition_holds_on_the_reference():
    """What tests/test_evidential_score_gpu.py's soft-head bound rests on, checked without a GPU: COND_MARGIN x the change
    of the float64 result under one fp32 ulp of v, alpha or beta stays below 1e-4 of max(|ref|, floor) for every element of
    the draws that test makes."""
    rng = np.random.default_rng(1)
    logits, y = E.soft_head_inputs(rng, 2 * 64 + 3 * 63 + 2 * 260)
    worst = E.soft_head_condition(logits, y)
    for k, w in worst.items():
        report(f"soft heads, {k}: COND_MARGIN x conditioning at most {w:.2e} of max(|ref|, floor)")
        assert w < 1e-4, k


SYMBOL = "mimo_score_accumulate_evidential"


def test_evidential_score_entry_point_is_declared_exported_and_bound(built_library):
    from mimo_unet_amd import _lib
    header = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    exports = open(os.path.join(ROOT, "mimo_unet_amd", "csrc", "exports.map")).read()
    assert re.search(r"\b%s\(" % SYMBOL, header)
    assert re.search(r"\bmimo_\*", exports) and SYMBOL in exports
    assert SYMBOL in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), SYMBOL)
    assert "score_evidential.hip" in open(os.path.join(ROOT, "Makefile")).read()


def test_host_checks_need_no_gpu():
    from mimo.evaluation import PredictiveScorer, check_evidential_score_shapes
    z = torch.zeros
    assert check_evidential_score_shapes(z(2, 4, 3, 5), z(2, 1, 3, 5), None) == (2, 3, 5)
    assert check_evidential_score_shapes(z(2, 4, 3, 5), z(2, 1, 3, 5), z(2, 3, 5)) == (2, 3, 5)
    assert check_evidential_score_shapes(z(2, 4, 3, 5), z(2, 1, 3, 5), z(2, 1, 3, 5)) == (2, 3, 5)
    for args in ((z(2, 3, 3, 5), z(2, 1, 3, 5), None), (z(4, 3, 5), z(1, 3, 5), None), (z(2, 4, 3, 5), z(2, 3, 5), None),
                 (z(2, 4, 3, 5), z(2, 4, 3, 5), None), (z(2, 4, 3, 5), z(1, 1, 3, 5), None),
                 (z(2, 4, 3, 5), z(2, 1, 3, 5), z(2, 4, 3, 5)), (z(2, 4, 3, 5), z(2, 1, 3, 5), z(2, 5, 3)),
                 (z(2, 4, 3, 5), z(2, 1, 3, 5), z(1, 3, 5))):
        with pytest.raises(ValueError):
            check_evidential_score_shapes(*args)
    # a model that is not evidential is refused before anything of the scorer (or of the model) is touched
    ens = types.SimpleNamespace(loss_fn=None, monte_carlo_steps=2, num_subnetworks=2)
    with pytest.raises(TypeError, match="EvidentialUnetModel"):
        PredictiveScorer.update_from_evidential(None, ens, None, None)
    # a training-mode model is refused by require_eval, shapes before the device
    from mimo.models.evidential_unet import EvidentialUnetModel
    ev = EvidentialUnetModel(in_channels=3, out_channels=4, filter_base_count=4, center_dropout_rate=0.0, final_dropout_rate=0.0,
                             encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0,
                             learning_rate=1e-3, seed=0)
    ev.train()
    with pytest.raises(Exception, match="eval"):
        PredictiveScorer.update_from_evidential(None, ev, z(1, 3, 32, 32), z(1, 1, 32, 32))
    ev.eval()
    for image, label, mask in ((z(1, 2, 32, 32), z(1, 1, 32, 32), None), (z(1, 3, 32, 32), z(1, 32, 32), None),
                               (z(1, 3, 32, 32), z(1, 1, 32, 32), z(1, 2, 32, 32))):
        with pytest.raises(ValueError):
            PredictiveScorer.update_from_evidential(None, ev, image, label, mask)
