"""The definition of the mixture scoring rules (tests/score_reference.py) against independent statements of the same
quantities — the CRPS's defining integral, scipy's densities and distribution functions, known answers, invariants, a
calibration experiment — and the host half of `PredictiveScorer` (no GPU)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import score_reference as R
from tests.helpers import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23


def draw(seed, S, N=1):
    g = np.random.default_rng(seed)
    mu, p2, y = R.random_members(g, S, N)
    return mu.astype(np.float64), p2.astype(np.float64), y.astype(np.float64)


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("S", [1, 2, 5])
def test_crps_closed_form_is_the_defining_integral(loss, S):
    integrate = pytest.importorskip("scipy.integrate")
    for seed in range(4):
        mu, p2, y = draw(100 * S + seed, S)
        sc = R.member_scale(p2, np.float64)
        got = float(R.score(mu, p2, y, loss)["crps"][0])
        m, s, y0 = mu[:, 0], sc[:, 0], float(y[0])
        width = float((s if loss == "laplace_nll" else np.sqrt(s)).max())
        lo, hi = min(m.min(), y0) - 60 * width, max(m.max(), y0) + 60 * width  # the tails beyond: < e^-60 of the integrand
        f = lambda x: (R.mixture_cdf(x, m, s, loss) - (1.0 if x >= y0 else 0.0)) ** 2
        pts = sorted(set([y0] + list(m)))
        val = err = 0.0
        for a, b in zip([lo] + pts, pts + [hi]):  # break points at y and the member means
            v, e = integrate.quad(f, a, b, epsabs=1e-13, epsrel=1e-13, limit=200)
            val, err = val + v, err + e
        report(f"crps {loss} S={S} seed={seed}: closed {got:.15e} quad {val:.15e} diff {abs(got - val):.1e} abserr {err:.1e}")
        assert abs(got - val) <= err + 1e-12 * abs(val)


@pytest.mark.parametrize("loss", R.LOSSES)
def test_nll_and_pit_are_scipy_densities_combined(loss):
    stats = pytest.importorskip("scipy.stats")
    special = pytest.importorskip("scipy.special")
    for S in (1, 3, 7):
        mu, p2, y = draw(7 + S, S, 200)
        sc = R.member_scale(p2, np.float64)
        dist = stats.laplace(loc=mu, scale=sc) if loss == "laplace_nll" else stats.norm(loc=mu, scale=np.sqrt(sc))
        nll = -(special.logsumexp(dist.logpdf(y[None]), axis=0) - np.log(S))
        pit = dist.cdf(y[None]).mean(axis=0)
        got = R.score(mu, p2, y, loss)
        assert np.allclose(got["nll"], nll, rtol=1e-12, atol=1e-12)
        assert np.allclose(got["pit"], pit, rtol=1e-12, atol=1e-15)


def test_known_answers_of_one_member_at_its_mean():
    for b in (1e-3, 0.2, 7.0):
        mu, p2 = np.array([[0.3]]), np.log(np.array([[b]]))
        la = R.score(mu, p2, mu[0], "laplace_nll")
        assert la["pit"][0] == 0.5
        assert abs(la["nll"][0] - np.log(2 * b)) <= 1e-14 * max(1.0, abs(np.log(2 * b)))
        assert abs(la["crps"][0] - b / 4) <= 1e-14 * b
        ga = R.score(mu, p2, mu[0], "gaussian_nll")  # variance b
        sigma = np.sqrt(b)
        assert ga["pit"][0] == 0.5
        assert abs(ga["crps"][0] - sigma * (np.sqrt(2) - 1) / np.sqrt(np.pi)) <= 1e-14 * sigma
        assert abs(ga["nll"][0] - (np.log(sigma) + 0.5 * np.log(2 * np.pi))) <= 1e-14


@pytest.mark.parametrize("loss", R.LOSSES)
def test_invariants(loss):
    mu, p2, y = draw(3, 6, 500)
    base = R.score(mu, p2, y, loss)
    perm = np.random.default_rng(0).permutation(6)
    again = R.score(mu[perm], p2[perm], y, loss)
    one = R.score(mu[:1], p2[:1], y, loss)
    same = R.score(np.repeat(mu[:1], 5, axis=0), np.repeat(p2[:1], 5, axis=0), y, loss)
    for k in ("pit", "nll", "crps"):
        assert np.allclose(base[k], again[k], rtol=1e-12, atol=1e-14), k  # a permutation of the members
        assert np.allclose(one[k], same[k], rtol=1e-12, atol=1e-14), k    # S identical members are one member
    for dt in (np.float64, np.float32):
        for S in (1, 2, 6):
            r = R.score(mu[:S], p2[:S], y, loss, dtype=dt)
            assert np.all(r["crps"] >= 0) and np.all((r["pit"] >= 0) & (r["pit"] <= 1))
    # far tails: the rules stay finite, the PIT saturates
    far = R.score(mu[:3], p2[:3], y + 1e4, loss, dtype=np.float32)
    assert np.all(np.isfinite(far["nll"])) and np.all(far["pit"] == 1) and np.all(np.isfinite(far["crps"]))


def test_laplace_pair_term_in_fp32_near_equal_scales():
    """The fp32 restatement of the pair term stays within 4 fp32 ulp of its float64 value at relative scale differences of 0,
    1 ulp, 1e-6, 1e-3 and 1 (the quotient form loses every digit at the first three); in float64 the form is the quotient
    where that is well conditioned."""
    g = np.random.default_rng(5)
    worst = 0.0
    for rel in (0.0, float(np.finfo(np.float32).eps), 1e-6, 1e-3, 1.0):
        bi = np.exp(g.uniform(-6, 3, size=4000)).astype(np.float32)
        bj = (np.nextafter(bi, np.float32(np.inf)) if rel == float(np.finfo(np.float32).eps) else bi * np.float32(1 + rel)).astype(np.float32)
        D = (bi * np.exp(g.uniform(-8, 3, size=bi.size))).astype(np.float32)
        D[:50] = 0.0
        swap = g.random(bi.size) < 0.5
        si, sj = np.where(swap, bj, bi), np.where(swap, bi, bj)
        lo = R.laplace_pair(D, si, sj)
        hi = R.laplace_pair(D.astype(np.float64), si.astype(np.float64), sj.astype(np.float64))
        assert lo.dtype == np.float32
        e = float(np.max(np.abs(lo.astype(np.float64) - hi) / hi)) / ULP32
        report(f"laplace pair term, relative scale difference {rel:g}: fp32 restatement {e:.2f} ulp from float64")
        worst = max(worst, e)
        assert e <= 4.0
        if rel == 1.0:
            q = R.laplace_pair_quotient(D.astype(np.float64), si.astype(np.float64), sj.astype(np.float64))
            assert np.allclose(hi, q, rtol=1e-12)
        if rel == 0.0:
            b = si.astype(np.float64)
            assert np.allclose(hi, D + np.exp(-D / b) * (3 * b + D) / 2, rtol=1e-14)
    assert np.allclose(R.laplace_pair(np.zeros(3), np.array([0.1, 1.0, 5.0]), np.array([0.1, 1.0, 5.0])), 1.5 * np.array([0.1, 1.0, 5.0]))


@pytest.mark.parametrize("loss", R.LOSSES)
def test_labels_drawn_from_the_mixture_are_calibrated(loss):
    N, S = 200_000, 3
    g = np.random.default_rng(11)
    mu = np.array([-0.4, 0.1, 0.7])
    sc = np.array([0.05, 0.3, 0.12])
    y = R.sample_mixture(g, mu, sc, loss, N)
    r = R.score(np.repeat(mu[:, None], N, axis=1), np.log(np.repeat(sc[:, None], N, axis=1)), y, loss)
    p = np.arange(41) / 40.0
    s = R.summarize(r["pit"], r["nll"], r["crps"], p)
    dev = np.abs(s["calibration"]["observed"] - p)
    report(f"calibration of {N} draws from the {loss} mixture: worst |observed - expected| {dev.max():.2e}, bound {6 * 0.5 / N ** 0.5:.2e}")
    assert np.all(dev <= 6 * 0.5 / np.sqrt(N))
    assert s["n"] == N and abs(s["pit_mean"] - 0.5) <= 6 * (1 / 12) ** 0.5 / np.sqrt(N)
    assert s["calibration_error"] == pytest.approx(dev.mean())
    assert len(s["coverage"]) == 20  # (0, 1), (0.025, 0.975), ... (0.475, 0.525)
    for level, share in s["coverage"].items():
        assert abs(share - level) <= 2 * 6 * 0.5 / np.sqrt(N)


def test_summary_numbers():
    p = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    pit = np.array([0.0, 0.1, 0.25, 0.3, 0.74999, 0.75, 1.0, 0.5], dtype=np.float32)
    s = R.summarize(pit, np.ones(8), 2 * np.ones(8), p, n_masked=3, n_nonfinite=1)
    assert list(s["counts"]) == [0, 2, 2, 2, 1, 1]  # u < p_k strictly; u = 1 is never below
    assert np.array_equal(s["calibration"]["observed"], np.array([0, 2, 4, 6, 7]) / 8)
    assert s["coverage"] == {1.0: 7 / 8, 0.5: 0.5}
    assert (s["n"], s["n_masked"], s["n_nonfinite"], s["nll"], s["crps"]) == (8, 3, 1, 1.0, 2.0)
    from mimo.evaluation import coverage_table
    assert coverage_table(p, s["calibration"]["observed"]) == s["coverage"]
    empty = R.summarize(np.zeros(0, np.float32), np.zeros(0), np.zeros(0), p)
    assert empty["n"] == 0 and np.isnan(empty["nll"]) and np.all(np.isnan(empty["calibration"]["observed"]))


def test_skip_rule():
    mu = np.zeros((2, 6), np.float32)
    p2 = np.zeros((2, 6), np.float32)
    y = np.zeros(6, np.float32)
    mask = np.array([1, 0, 1, 1, 0, 1], np.float32)
    mu[1, 2] = np.nan
    p2[0, 3] = -np.inf
    y[4] = np.inf  # masked first: counted as masked
    y[5] = np.inf
    ok, masked, bad = R.valid_pixels(mu, p2, y, mask)
    assert list(ok) == [True, False, False, False, False, False]
    assert list(masked) == [False, True, False, False, True, False] and list(bad) == [False, False, True, True, False, True]


SYMBOLS = ("mimo_score_workspace_bytes", "mimo_score_accumulate", "mimo_score_finalize")


def test_score_entry_points_are_declared_exported_and_bound(built_library):
    from mimo_unet_amd import _lib
    header = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    exports = open(os.path.join(ROOT, "mimo_unet_amd", "csrc", "exports.map")).read()
    assert re.search(r"\bmimo_\*", exports)
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    ws = lib.mimo_score_workspace_bytes()
    assert ws > 0 and ws % 8 == 0
    assert "score_rules.hip" in open(os.path.join(ROOT, "Makefile")).read()


def test_host_validation_needs_no_gpu():
    from mimo.evaluation import MAX_MEMBERS, PredictiveScorer, check_expected_p, check_score_shapes, mixture_of
    from mimo.losses import LaplaceNLL
    from mimo.models.evidential_unet import EvidentialUnetModel
    from mimo_unet_amd._lib import MimoHipError
    assert np.array_equal(check_expected_p(None), np.arange(41) / 40.0)
    for bad in ([], np.arange(66) / 65.0, [0.5, 0.4], [-0.1, 0.5], [0.5, 1.1], [0.5, float("nan")]):
        with pytest.raises(ValueError):
            check_expected_p(bad)
        with pytest.raises(ValueError):  # before the device is looked for
            PredictiveScorer(expected_p=bad)
    if not torch.cuda.is_available():
        with pytest.raises(MimoHipError):
            PredictiveScorer()
    z5, z4 = torch.zeros(2, 3, 2, 4, 4), torch.zeros(2, 2, 4, 4)
    assert check_score_shapes(z5, z5, z4, None, 1) == (2, 3, 2, 4, 4, 1)
    assert check_score_shapes(z5, z5, z4, torch.zeros(2, 2, 4, 4), 0)[-1] == 2
    for args in ((z4, z4, z4, None, 0), (z5, z5[:, :2], z4, None, 0), (z5, z5, z4[:, :1], None, 0), (z5, z5, z4, None, 2),
                 (z5, z5, z4, torch.zeros(2, 1, 4, 5), 0), (z5, z5, z4, torch.zeros(2, 3, 4, 4), 0),
                 (torch.zeros(1, 65, 1, 2, 2), torch.zeros(1, 65, 1, 2, 2), torch.zeros(1, 1, 2, 2), None, 0)):
        with pytest.raises(ValueError):
            check_score_shapes(*args)
    ens = types.SimpleNamespace(loss_fn=LaplaceNLL(), monte_carlo_steps=8, num_subnetworks=3)
    assert mixture_of(ens) == ("laplace_nll", 1e-5, 1e3, 24)
    ens.monte_carlo_steps = 0
    assert mixture_of(ens)[3] == 3
    ens.monte_carlo_steps, ens.num_subnetworks = 13, 5
    assert 13 * 5 > MAX_MEMBERS
    with pytest.raises(ValueError, match="65"):
        mixture_of(ens)
    ev = EvidentialUnetModel(in_channels=3, out_channels=4, filter_base_count=4, center_dropout_rate=0.0, final_dropout_rate=0.0,
                             encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0,
                             learning_rate=1e-3, seed=0)
    with pytest.raises(NotImplementedError, match="evidential"):
        mixture_of(ev)
    with pytest.raises(NotImplementedError, match="evidential"):
        PredictiveScorer.update_from(None, ev, None, None)  # refused before anything of the scorer is touched


def test_scores_csv_headers(tmp_path):
    from mimo.evaluation import write_scores_csv
    p = np.arange(41) / 40.0
    scores = {"n": 10, "n_masked": 2, "n_nonfinite": 0, "nll": -1.25, "crps": 0.5, "pit_mean": 0.51, "calibration_error": 0.01,
              "calibration": {"expected": p, "observed": p ** 2}}
    a, b = write_scores_csv(scores, str(tmp_path / "out"))
    assert os.path.basename(a) == "scores.csv" and os.path.basename(b) == "calibration_mixture.csv"
    lines = open(a).read().splitlines()
    assert lines[0] == "n,n_masked,n_nonfinite,nll,crps,pit_mean,calibration_error" and lines[1] == "10,2,0,-1.25,0.5,0.51,0.01"
    assert open(b).readline().rstrip("\n") == "Expected Conf.,Observed Conf."
    assert np.array_equal(np.loadtxt(b, delimiter=",", skiprows=1), np.stack([p, p ** 2], axis=1))
