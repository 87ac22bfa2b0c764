"""Host half of the uncertainty evaluator (no GPU): the float64 restatement of the reference's two tables
(tests/eval_reference.py) reproduces the fixture written by the REAL reference (tests/golden/make_eval_golden.py), and the
evaluator's host arithmetic — cutoff indices, standard quantiles, CSV headers — is the reference's."""
import os

import numpy as np
import pytest

from tests import eval_reference as R
from tests.helpers import load_npz, report

PCT = np.arange(100) / 100.0
P41 = np.arange(41) / 40.0
# Distance between the reference's own float32 frame (pandas means of a float32 column) and the float64 restatement,
# relative to the column's maximum, measured on the three data sets of eval_tables.npz when the fixture was generated:
# maps 8.4e-8 / 8.5e-8 (mae / rmse), laplace 1.2e-7 / 7.4e-8, gaussian 1.6e-7 / 7.5e-8.  The largest is recorded; the
# test allows 4 x that — a few float32 roundings of a mean, not a free parameter.
FLOAT32_FRAME_DISTANCE = 1.6e-7


def fixture_maps(fx, name):
    return [fx[f"{name}/{k}"] for k in ("mean", "aleatoric_var", "epistemic_var", "label")]


@pytest.mark.parametrize("name", ["maps", "laplace", "gaussian"])
def test_restatement_reproduces_the_reference_tables(name):
    fx = load_npz("eval_tables.npz")
    cols = R.pixel_columns(*fixture_maps(fx, name))
    n = cols["error"].size
    sp = R.sparsification(cols, PCT)
    cal = R.calibration(cols, fx["z_norm"])
    pr, rc = fx[f"{name}/pr"], fx[f"{name}/cal"]
    assert pr.shape == (100, 3) and rc.shape == (41, 2)
    assert np.array_equal(pr[:, 0], PCT) and np.array_equal(rc[:, 0], P41)
    # calibration: counts match exactly
    assert np.array_equal(rc[:, 1], cal["counts"] / n)
    assert not R.straddling_ties(sp["sorted_desc"], sp["cutoff"])
    for col, key in ((1, "mae"), (2, "rmse")):
        dist = np.abs(pr[:, col] - sp[key]).max() / pr[:, col].max()
        report(f"eval fixture {name}: float32-frame distance of {key}: {dist:.3e}")
        assert dist <= 4 * FLOAT32_FRAME_DISTANCE
    # the conditions the GPU tests rely on
    assert cal["band"].max() <= 1e-4 * n


def test_cutoff_indices_are_the_truncated_float64_product():
    from mimo.evaluation import cutoff_indices
    for n in (1, 99, 100, 101, 10 ** 6 + 7, 2 ** 31 + 5):
        want = np.array([int(np.float64(k / 100.0) * np.float64(n)) for k in range(100)], dtype=np.int64)
        got = cutoff_indices(PCT, n)
        assert got.dtype == np.int64 and np.array_equal(got, want), n
    # where integer arithmetic would differ: 0.29 * 100 = 28.999999999999996
    assert cutoff_indices(PCT, 100)[29] == 28 and cutoff_indices(PCT, 100)[57] == 56


def test_standard_quantiles_match_scipy_to_one_ulp():
    from mimo.evaluation import standard_quantiles
    z = standard_quantiles(P41, "norm")
    try:
        import scipy.stats
        want = scipy.stats.norm.ppf(P41)
        want_laplace = scipy.stats.laplace.ppf(P41)
    except ImportError:
        want, want_laplace = load_npz("eval_tables.npz")["z_norm"], None
    assert z.dtype == np.float64 and z[0] == -np.inf and z[-1] == np.inf and z[20] == 0.0
    assert np.all(np.abs(z[1:-1] - want[1:-1]) <= np.spacing(np.abs(want[1:-1])))
    assert np.array_equal(want, load_npz("eval_tables.npz")["z_norm"]) or want_laplace is None
    zl = standard_quantiles(P41, "laplace")
    assert zl[0] == -np.inf and zl[-1] == np.inf and zl[20] == 0.0 and np.all(np.diff(zl) > 0)
    closed = np.array([np.log(2 * p) if p <= 0.5 else -np.log(2 * (1 - p)) for p in P41[1:-1]])
    assert np.all(np.abs(zl[1:-1] - closed) <= np.spacing(np.abs(closed)))
    if want_laplace is not None:
        assert np.all(np.abs(zl[1:-1] - want_laplace[1:-1]) <= np.spacing(np.abs(want_laplace[1:-1])))
    with pytest.raises(ValueError):
        standard_quantiles(P41, "cauchy")


def test_write_csv_round_trips_the_reference_headers(tmp_path):
    from mimo.evaluation import write_tables_csv
    g = np.random.default_rng(0)
    tables = {"precision_recall": {"percentile": PCT, "mae": g.random(100), "rmse": g.random(100)},
              "calibration": {"expected": P41, "observed": np.sort(g.random(41))}}
    pr_path, cal_path = write_tables_csv(tables, str(tmp_path / "out"))
    assert os.path.basename(pr_path) == "precision_recall.csv" and os.path.basename(cal_path) == "calibration.csv"
    assert open(pr_path).readline().rstrip("\n") == "percentile,mae,rmse"
    assert open(cal_path).readline().rstrip("\n") == "Expected Conf.,Observed Conf."
    pr = np.loadtxt(pr_path, delimiter=",", skiprows=1)
    cal = np.loadtxt(cal_path, delimiter=",", skiprows=1)
    assert np.array_equal(pr, np.stack([PCT, tables["precision_recall"]["mae"], tables["precision_recall"]["rmse"]], axis=1))
    assert np.array_equal(cal, np.stack([P41, tables["calibration"]["observed"]], axis=1))


def test_evaluator_has_no_cpu_path():
    import torch
    from mimo.evaluation import UncertaintyEvaluator
    from mimo_unet_amd._lib import MimoHipError
    if torch.cuda.is_available():
        ev = UncertaintyEvaluator()
        z = torch.zeros(1, 1, 4, 4)
        with pytest.raises(MimoHipError):
            ev.update(z, z, z, z)
    else:
        with pytest.raises(MimoHipError):
            UncertaintyEvaluator()


def test_eval_entry_points_are_declared_and_bound(built_library):
    from mimo_unet_amd import _lib
    lib = _lib.load()
    for name in ("mimo_eval_workspace_bytes", "mimo_eval_accumulate", "mimo_eval_select", "mimo_eval_interval_sums"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.mimo_eval_workspace_bytes() > 0
