"""CPU-side checks of the sparsification error (no GPU needed): `mimo.evaluation.sparsification_areas` against the numpy
restatement (tests/sparsification_reference.py), the properties of the curves it integrates, the validation of source
names and the three new C-ABI symbols.

Bound: both sides are float64 trapezoid sums of the same <= 100 rows; they differ in the grouping of the additions
only -> 1e-12 relative to the area of the curve itself (integral of |curve|), far inside the 1e-9 of the GPU rows."""
import os
import re

import numpy as np
import pytest

from tests import eval_reference as R
from tests import sparsification_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCT = np.arange(100) / 100.0
AREA_TOL = 1e-12
NEW_SYMBOLS = ("mimo_eval_accumulate_sources", "mimo_eval_select_by", "mimo_eval_interval_sums_by")
CASES = [((3, 1, 37, 53), 22), ((5, 2, 32, 48), 23), ((2, 1, 64, 64), 21)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "x".join(map(str, c[0])))
def restated(request):
    shape, seed = request.param
    keys, err, _ = S.source_keys(*R.synthetic_maps(seed, *shape), channel=shape[1] - 1)
    return S.curves(keys, err, PCT)


@pytest.mark.parametrize("normalize", [False, True])
def test_areas_equal_the_restatement(restated, normalize):
    from mimo.evaluation import sparsification_areas
    for name in S.SOURCES:
        for m in ("mae", "rmse"):
            got = sparsification_areas(PCT, restated[name][m], restated["oracle"][m], normalize=normalize)
            want = S.areas(PCT, restated[name][m], restated["oracle"][m], normalize=normalize)
            scale = S.trapezoid(PCT, restated[name][m] / (restated[name][m][0] if normalize else 1.0))
            assert all(isinstance(v, float) for v in got)
            assert abs(got[0] - want[0]) <= AREA_TOL * scale and abs(got[1] - want[1]) <= AREA_TOL * scale, (name, m, got, want)


def test_areas_skip_rows_that_are_not_finite_in_both_curves():
    from mimo.evaluation import sparsification_areas
    x = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    c, o = np.array([4.0, 3.0, 2.0, 1.0, np.nan]), np.array([4.0, 2.0, np.nan, 0.0, np.nan])
    ause, aurg = sparsification_areas(x, c, o)  # rows 0, 1 and 3 remain: x = 0, 0.25, 0.75
    assert ause == pytest.approx(0.25 * (0.0 + 1.0) / 2 + 0.5 * (1.0 + 1.0) / 2, rel=1e-15)
    assert aurg == pytest.approx(0.25 * (0.0 + 1.0) / 2 + 0.5 * (1.0 + 3.0) / 2, rel=1e-15)
    assert (ause, aurg) == pytest.approx(S.areas(x, c, o), rel=1e-15)
    assert all(np.isnan(v) for v in sparsification_areas(x, np.full(5, np.nan), o))
    n_ause, _ = sparsification_areas(x, c, o, normalize=True)
    assert n_ause == pytest.approx(ause / 4.0, rel=1e-15)
    with pytest.raises(ValueError):
        sparsification_areas(x, c[:4], o)


def test_oracle_row_is_at_most_every_source_row(restated):
    """dropping the k pixels with the largest errors leaves the smallest possible sum of errors (and of squares)"""
    for name in S.SOURCES:
        for m in ("mae", "rmse"):
            assert np.all(restated["oracle"][m] <= restated[name][m] * (1 + 1e-12)), (name, m)


def test_ause_of_the_oracle_against_itself_is_zero(restated):
    from mimo.evaluation import sparsification_areas
    for m in ("mae", "rmse"):
        assert sparsification_areas(PCT, restated["oracle"][m], restated["oracle"][m])[0] == 0.0
        assert sparsification_areas(PCT, restated["oracle"][m], restated["oracle"][m], normalize=True)[0] == 0.0


def test_ause_plus_aurg_is_the_area_between_random_removal_and_the_oracle(restated):
    from mimo.evaluation import sparsification_areas
    for name in S.SOURCES:
        for m in ("mae", "rmse"):
            c, o = restated[name][m], restated["oracle"][m]
            ause, aurg = sparsification_areas(PCT, c, o)
            most = S.trapezoid(PCT, c[0] - o)
            assert abs(ause + aurg - most) <= AREA_TOL * S.trapezoid(PCT, c), (name, m)
            assert ause >= -AREA_TOL * most and most > 0


def test_unknown_source_names_raise():
    """before anything touches a GPU: the names are checked first, so the ValueError shows on a host without one"""
    from mimo.evaluation import SOURCES, UncertaintyEvaluator, check_sources
    assert tuple(SOURCES) == S.SOURCES
    assert check_sources(("aleatoric", "combined", "aleatoric")) == ("aleatoric", "combined")
    for bad in (("combined", "total"), ("Aleatoric",), ("",), "std"):
        with pytest.raises(ValueError, match="unknown uncertainty source"):
            check_sources(bad)
        with pytest.raises(ValueError, match="unknown uncertainty source"):
            UncertaintyEvaluator(sources=bad)


def test_new_symbols_are_declared_listed_and_exported(built_library):
    import fnmatch
    import subprocess

    from mimo_unet_amd import _lib
    header = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    vmap = open(os.path.join(ROOT, "mimo_unet_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"([A-Za-z0-9_*?]+)\s*;", vmap.split("global:")[1].split("local:")[0])
    nm = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} is not declared in include/mimo_hip.h"
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns), f"{sym} is not covered by csrc/exports.map"
        assert sym in _lib.EXPORTED_SYMBOLS, f"{sym} is not in _lib.EXPORTED_SYMBOLS"
        assert sym in exported, f"libmimo_hip.so does not export {sym}"
        assert hasattr(lib, sym)
    assert "source_records" in header and "-0 canonicalised" in header  # the layout of the second record
    assert "[3 P] slice per further ordering" in header                  # ... and of the output buffer
