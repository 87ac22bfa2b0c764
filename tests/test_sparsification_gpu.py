"""UncertaintyEvaluator(sources=...) on the GPU against the float64 restatement (tests/sparsification_reference.py): the
sparsification curve per uncertainty source, the oracle curve, AUSE and AURG.

Bounds (those of tests/test_evaluation_gpu.py and its derivation):
* rows: the device and the restatement see bit-identical fp32 keys and errors and both sum in double; only the grouping
  of the additions differs -> 1e-9 relative per row.
* cutoff keys per source: exact (bit for bit).
* areas: float64 arithmetic on those rows -> 1e-9 relative of the restatement's.
Where a test needs that no run of identical keys straddles a cutoff, that is a condition asserted on the restatement
("choose another seed"), not a tolerance.  The oracle ordering needs no such condition: tied records carry one error."""
import time

import numpy as np
import pytest
import torch

from tests import eval_reference as R
from tests import sparsification_reference as S
from tests import test_evaluation_gpu as E
from tests.helpers import report

pytestmark = pytest.mark.gpu

PCT = np.arange(100) / 100.0
ROW_TOL = 1e-9
ALL = ("combined", "aleatoric", "epistemic", "oracle")


def make(sources=ALL, **kw):
    from mimo.evaluation import UncertaintyEvaluator
    return UncertaintyEvaluator(sources=sources, **kw)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def key_bits(a):
    return np.asarray(a).astype(np.float32).view(np.uint32)


def close(got, want, tol=ROW_TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.array_equal(np.isnan(got), np.isnan(want)) and bool(np.all(np.abs(got - want)[~np.isnan(want)] <= tol * np.abs(want)[~np.isnan(want)]))


def same_tables(a, b):
    """two compute() results, bit for bit"""
    assert bits(a["precision_recall"]["mae"]).tolist() == bits(b["precision_recall"]["mae"]).tolist()
    assert bits(a["precision_recall"]["rmse"]).tolist() == bits(b["precision_recall"]["rmse"]).tolist()
    assert np.array_equal(a["calibration"]["observed"], b["calibration"]["observed"]) and np.array_equal(a["cutoff_keys"], b["cutoff_keys"])
    assert (a["n"], a["n_masked"], a["n_nonfinite"], a["mae"], a["mse"]) == (b["n"], b["n_masked"], b["n_nonfinite"], b["mae"], b["mse"])
    assert list(a["sparsification"]) == list(b["sparsification"])
    for name in a["sparsification"]:
        for k in ("mae", "rmse", "cutoff_keys"):
            assert np.array_equal(bits(a["sparsification"][name][k]), bits(b["sparsification"][name][k])), (name, k)
        for k in ("ause", "aurg"):
            assert bits([a[k][name]["mae"], a[k][name]["rmse"]]).tolist() == bits([b[k][name]["mae"], b[k][name]["rmse"]]).tolist()


def check_sources(t, ev, maps, mask=None, channel=0, tag="", tie_rule=(), flat=()):
    """the per-source tables of `t` against the restatement on the same inputs.  `tie_rule`: the sources whose rows are
    held against the evaluator's tie rule (and in which a straddling tie is REQUIRED); every other key source must be
    tie-free at the cutoffs.  `flat`: the sources whose curve is constant (their AURG is 0 up to rounding)."""
    keys, err, cols = S.source_keys(*maps, mask=mask, channel=channel)
    assert (t["n"], t["n_masked"], t["n_nonfinite"]) == (err.size, cols["n_masked"], cols["n_nonfinite"])
    ref = S.curves(keys, err, ev.percentiles)
    assert list(t["sparsification"]) == list(ev.sources) + ([] if "oracle" in ev.sources else ["oracle"])
    rows = {}
    for name, got in t["sparsification"].items():
        sp = ref[name]
        ties = R.straddling_ties(sp["sorted_desc"], sp["cutoff"])
        mae, rmse = sp["mae"], sp["rmse"]
        if name in tie_rule:
            assert ties, f"{tag}: the {name} ordering has no tie that straddles a cutoff — choose another seed"
            mae, rmse = E.tie_rule_rows(S.as_columns(keys[name], err), ev.percentiles)
            free = ~np.isin(sp["cutoff"], ties)  # where no run straddles the cutoff the tie rule IS the plain restatement
            assert close(mae[free], sp["mae"][free]) and close(rmse[free], sp["rmse"][free])
        elif name != "oracle":
            assert not ties, f"{tag}: a tie straddles cutoffs {ties[:5]} of the {name} ordering — choose another seed"
        e_mae = np.nanmax(np.abs(got["mae"] - mae) / mae)
        e_rmse = np.nanmax(np.abs(got["rmse"] - rmse) / rmse)
        report(f"sparsification {tag} {name}: n {err.size}, rows mae {e_mae:.2e} rmse {e_rmse:.2e}, ties at cutoffs {len(ties)}")
        assert close(got["mae"], mae) and close(got["rmse"], rmse), (name, e_mae, e_rmse)
        assert np.array_equal(key_bits(got["cutoff_keys"]), key_bits(sp["cutoff_keys"])), name
        rows[name] = {"mae": mae, "rmse": rmse}
    assert np.array_equal(bits(t["sparsification"]["combined"]["mae"]), bits(t["precision_recall"]["mae"]))
    for name in rows:
        for m in ("mae", "rmse"):
            ause, aurg = S.areas(ev.percentiles, rows[name][m], rows["oracle"][m])
            report(f"sparsification {tag} {name} {m}: AUSE {t['ause'][name][m]:.6e} (restated {ause:.6e}) AURG {t['aurg'][name][m]:.6e} "
                   f"(restated {aurg:.6e})")
            assert abs(t["ause"][name][m] - ause) <= ROW_TOL * abs(ause), (name, m)
            if name in flat:  # a constant curve: both gains are rounding noise around 0, bounded by the rows' own tolerance
                assert abs(t["aurg"][name][m]) <= ROW_TOL * rows[name][m][0] and abs(aurg) <= ROW_TOL * rows[name][m][0]
            else:
                assert abs(t["aurg"][name][m] - aurg) <= ROW_TOL * abs(aurg), (name, m)
    return keys, err, ref


# ------------------------------------------------------------------------------------------ the three geometries
def test_channel_one_of_two_all_sources_vector_path():
    maps = R.synthetic_maps(23, 5, 2, 32, 48)
    ev = make(channel=1)
    E.feed(ev, maps)
    t = ev.compute()
    check_sources(t, ev, maps, channel=1, tag="5x2x32x48 channel 1")
    for name in ("combined", "aleatoric", "epistemic"):  # the oracle curve lies below every source's
        assert np.all(t["sparsification"]["oracle"]["mae"] <= t["sparsification"][name]["mae"] * (1 + ROW_TOL))
        assert np.all(t["sparsification"]["oracle"]["rmse"] <= t["sparsification"][name]["rmse"] * (1 + ROW_TOL))
        assert t["ause"][name]["mae"] > 0 and t["ause"][name]["rmse"] > 0
    assert t["ause"]["oracle"] == {"mae": 0.0, "rmse": 0.0}


def test_odd_size_in_three_updates_equals_one_update():
    """hw = 37 * 53 is odd: the scalar path, with a partial last quad per image and record slots that are only 8-byte
    aligned from the second update on.  (Three images split three ways: one image per update.)"""
    maps = R.synthetic_maps(22, 3, 1, 37, 53)
    one, three = make(), make()
    E.feed(one, maps)
    E.feed(three, maps, splits=[1, 2])
    a, b = one.compute(), three.compute()
    check_sources(b, three, maps, tag="3x1x37x53 in updates of 1 + 1 + 1")
    assert np.array_equal(a["calibration"]["observed"], b["calibration"]["observed"]) and a["n"] == b["n"]
    for name in ALL:  # the same records in the same slots: the same bits
        for k in ("mae", "rmse", "cutoff_keys"):
            assert np.array_equal(bits(a["sparsification"][name][k]), bits(b["sparsification"][name][k])), (name, k)


def test_a_tie_that_straddles_an_aleatoric_cutoff_follows_the_tie_rule():
    maps = R.synthetic_maps(21, 2, 1, 64, 64)
    keys, err, _ = S.source_keys(*maps)
    sp = S.curve(keys["aleatoric"], err, PCT)
    assert len(R.straddling_ties(sp["sorted_desc"], sp["cutoff"])) == 1
    ev = make()
    E.feed(ev, maps)
    check_sources(ev.compute(), ev, maps, tag="2x1x64x64 seed 21", tie_rule=("aleatoric",))


# ------------------------------------------------------------------------------------------ opt-in
def test_default_tables_are_unchanged_by_the_extra_sources():
    maps = R.synthetic_maps(23, 5, 2, 32, 48)
    four, default = make(channel=1), make(sources=("combined",), channel=1)
    E.feed(four, maps, splits=[2])
    E.feed(default, maps, splits=[2])
    a, b = four.compute(), default.compute()
    for k in ("mae", "rmse"):
        assert np.array_equal(a["precision_recall"][k], b["precision_recall"][k])
    assert np.array_equal(a["calibration"]["observed"], b["calibration"]["observed"])
    assert np.array_equal(a["cutoff_keys"], b["cutoff_keys"])
    assert (a["n"], a["mae"], a["mse"], a["rmse"]) == (b["n"], b["mae"], b["mse"], b["rmse"])
    assert "sparsification" not in b and "ause" not in b and "aurg" not in b
    assert default._source_records is None and four._source_records is not None
    only_oracle = make(sources=("combined", "oracle"), channel=1)  # no second store without aleatoric / epistemic
    E.feed(only_oracle, maps, splits=[2])
    c = only_oracle.compute()
    assert only_oracle._source_records is None and list(c["sparsification"]) == ["combined", "oracle"]
    assert np.array_equal(bits(c["sparsification"]["oracle"]["mae"]), bits(a["sparsification"]["oracle"]["mae"]))


# ------------------------------------------------------------------------------------------ skipped pixels
def test_masked_and_nonfinite_pixels_are_stepped_over_in_every_ordering():
    """a skipped slot must not enter the oracle ordering as a pixel with error 0: that would drag its last rows to 0"""
    maps = [a.copy() for a in R.synthetic_maps(24, 2, 1, 32, 32)]
    n = maps[0].size
    mask = (np.random.default_rng(25).permutation(n) % 4 != 0).astype(np.float32).reshape(2, 1, 32, 32)
    flat = [a.reshape(-1) for a in maps]
    kept = np.flatnonzero(mask.reshape(-1) != 0)
    flat[0][kept[3]] = np.nan
    flat[0][kept[400]] = np.nan
    flat[1][kept[77]] = -0.25      # negative variances
    flat[2][kept[900]] = -1e-3
    flat[3][kept[1200]] = np.inf
    ev = make()
    E.feed(ev, maps, mask=mask)
    with pytest.warns(RuntimeWarning, match="5 pixels"):
        t = ev.compute()
    assert (t["n"], t["n_masked"], t["n_nonfinite"]) == (n - n // 4 - 5, n // 4, 5)
    keys, err, _ = check_sources(t, ev, maps, mask=mask, tag="2x1x32x32, 1/4 masked, 5 non-finite")
    last = t["sparsification"]["oracle"]["mae"][-1]  # the 1 % of the kept pixels with the smallest errors
    assert last > 0 and np.sort(err.astype(np.float64))[0] <= last <= np.sort(err.astype(np.float64))[t["n"] - int(0.99 * t["n"])]


# ------------------------------------------------------------------------------------------ an uninformative source
def test_zero_epistemic_variance_gives_the_whole_set_values_and_minus_zero_is_zero():
    maps = list(R.synthetic_maps(26, 2, 1, 32, 32))
    maps[2] = np.zeros_like(maps[2])  # S = 1: no epistemic part
    ev = make()
    E.feed(ev, maps)
    t = ev.compute()
    ep = t["sparsification"]["epistemic"]
    assert np.all(np.abs(ep["mae"] - t["mae"]) <= ROW_TOL * t["mae"]) and np.all(np.abs(ep["rmse"] - t["rmse"]) <= ROW_TOL * t["rmse"])
    assert np.all(ep["cutoff_keys"] == 0.0) and not np.any(np.signbit(ep["cutoff_keys"]))
    for m in ("mae", "rmse"):
        assert abs(t["aurg"]["epistemic"][m]) <= ROW_TOL * ep[m][0]
    check_sources(t, ev, maps, tag="epistemic variance 0", tie_rule=("epistemic",), flat=("epistemic",))
    minus = make()
    maps[2] = np.full_like(maps[2], -0.0)
    assert np.all(np.signbit(maps[2]))
    E.feed(minus, maps)
    same_tables(t, minus.compute())


# ------------------------------------------------------------------------------------------ selection exactness
def hostile_errors(kind):
    g = np.random.default_rng(34)
    shape = (1, 1, 64, 64)
    mean, a_var, e_var, label = (a.copy() for a in R.synthetic_maps(33, *shape))
    if kind == "one-bucket":  # errors in [0.5, 0.6]: every error shares its top 11 bits
        mean = np.full(shape, 0.25, np.float32)
        label = (0.75 + g.uniform(0, 0.1, shape)).astype(np.float32)
    elif kind == "denormal":
        mean = np.zeros(shape, np.float32)
        label = (g.uniform(0, 1, shape) * 1e-40).astype(np.float32)
    elif kind == "half-zero":  # label == mean after the clip
        label.reshape(-1)[::2] = np.clip(mean.reshape(-1)[::2], 0.0, 1.0)
    else:  # fewer pixels than cutoffs
        sl = (slice(None), slice(None), slice(0, 3), slice(0, 19))
        mean, a_var, e_var, label = (np.ascontiguousarray(a[sl]) for a in (mean, a_var, e_var, label))
    return [mean, a_var, e_var, label]


@pytest.mark.parametrize("kind", ["one-bucket", "denormal", "half-zero", "n-below-100"])
def test_oracle_selection_is_exact_on_hostile_error_keys(kind):
    maps = hostile_errors(kind)
    ev = make()
    E.feed(ev, maps)
    t = ev.compute()
    keys, err, _ = S.source_keys(*maps)
    n = err.size
    assert t["n"] == n == (57 if kind == "n-below-100" else 4096)
    if kind == "one-bucket":
        assert np.unique(err.view(np.uint32) >> 21).size == 1 and err.min() >= 0.5
    elif kind == "denormal":
        assert 0 < err.max() < np.finfo(np.float32).tiny and np.unique(err).size > n // 2
    elif kind == "half-zero":
        assert n // 2 <= int((err == 0).sum()) < n // 2 + 8
    kth = n - R.cutoffs(PCT, n) - 1  # ascending rank of the survivor with the largest key
    for name in ALL:  # the key of a rank is defined whatever the ties
        want = np.partition(keys[name], np.unique(kth))[kth]
        assert np.array_equal(key_bits(t["sparsification"][name]["cutoff_keys"]), want.view(np.uint32)), (kind, name)
    sp = S.curve(keys["oracle"], err, PCT)
    got = t["sparsification"]["oracle"]
    assert close(got["mae"], sp["mae"]) and close(got["rmse"], sp["rmse"]), kind
    if kind == "half-zero":
        assert np.all(got["mae"][51:] == 0.0) and got["mae"][49] > 0
    report(f"sparsification oracle selection {kind}: n {n}, {np.unique(err).size} distinct errors, exact")


def test_strided_entry_points_on_contiguous_key_and_error_arrays():
    """the C ABI with a stride of one word (the evaluator itself always passes record words, stride 2): the same records
    in the same slots give the combined table bit for bit"""
    from mimo_unet_amd import _lib as L
    maps = R.synthetic_maps(22, 3, 1, 37, 53)
    ev = make(sources=("combined",))
    E.feed(ev, maps)
    t = ev.compute()
    n, p, k = ev._used, PCT.size, ev.expected_p.size
    words = ev._records[:n].view(torch.int32).view(n, 2)
    keys, errors = words[:, 0].contiguous(), words[:, 1].contiguous()
    out = torch.zeros(3 * p + k + 6, dtype=torch.float64, device=ev.device)
    s = L.current_stream()
    L.check(ev._lib.mimo_eval_select_by(keys.data_ptr(), 1, n, ev._pct_dev.data_ptr(), p, ev._ws.data_ptr(), s))
    L.check(ev._lib.mimo_eval_interval_sums_by(keys.data_ptr(), 1, errors.data_ptr(), 1, n, p, k, ev._ws.data_ptr(), out.data_ptr(), s))
    o = out.cpu().numpy()
    assert np.array_equal(bits(o[:p]), bits(t["precision_recall"]["mae"])) and np.array_equal(bits(o[p: 2 * p]), bits(t["precision_recall"]["rmse"]))
    assert np.array_equal(bits(o[2 * p: 3 * p]), bits(t["cutoff_keys"])) and np.array_equal(o[3 * p: 3 * p + k], t["calibration"]["observed"])


# ------------------------------------------------------------------------------------------ integration
def test_compute_twice_is_bit_identical_and_reset_empties_both_stores():
    maps = R.synthetic_maps(71, 4, 1, 64, 64)
    ev = make()
    E.feed(ev, maps, splits=[1])
    a, b = ev.compute(), ev.compute()
    same_tables(a, b)
    ev.reset()
    assert ev._used == 0
    e = ev.compute()
    assert e["n"] == 0 and e["n_masked"] == 0 and list(e["sparsification"]) == list(ALL)
    for name in ALL:
        assert np.all(np.isnan(e["sparsification"][name]["mae"])) and np.isnan(e["ause"][name]["mae"]) and np.isnan(e["aurg"][name]["rmse"])
    E.feed(ev, maps, splits=[1])
    same_tables(a, ev.compute())


def test_write_csv_with_extra_sources_writes_four_files(tmp_path):
    maps = R.synthetic_maps(22, 3, 1, 37, 53)
    four, default = make(), make(sources=("combined",))
    E.feed(four, maps)
    E.feed(default, maps)
    paths = four.write_csv(str(tmp_path / "four"))
    ref = default.write_csv(str(tmp_path / "default"))
    assert [p.rsplit("/", 1)[1] for p in paths] == ["precision_recall.csv", "calibration.csv", "sparsification.csv", "ause.csv"]
    assert len(ref) == 2 and sorted(f.name for f in (tmp_path / "default").iterdir()) == ["calibration.csv", "precision_recall.csv"]
    for a, b in zip(paths[:2], ref):
        assert open(a, "rb").read() == open(b, "rb").read()
    t = four.compute()
    head = open(paths[2]).readline().strip().split(",")
    assert head == ["percentile"] + [f"{m}_{s}" for s in ALL for m in ("mae", "rmse")]
    table = np.loadtxt(paths[2], delimiter=",", skiprows=1)
    assert table.shape == (100, 9) and np.array_equal(table[:, 0], PCT)
    assert np.array_equal(table[:, 3], t["sparsification"]["aleatoric"]["mae"]) and np.array_equal(table[:, 8], t["sparsification"]["oracle"]["rmse"])
    lines = open(paths[3]).read().splitlines()
    assert lines[0] == "source,ause_mae,ause_rmse,aurg_mae,aurg_rmse" and [ln.split(",")[0] for ln in lines[1:]] == list(ALL)
    assert float(lines[3].split(",")[1]) == t["ause"]["epistemic"]["mae"] and float(lines[2].split(",")[4]) == t["aurg"]["aleatoric"]["rmse"]


def test_update_with_sources_enqueues_without_a_host_synchronisation():
    """16 updates behind a ~0.4 s spin kernel (the pattern of tests/test_evaluation_gpu.py): a blocking call inside
    update(), the growth of the second store included, would find the gate event complete"""
    from tests.test_data_gpu import _sleep_cycles_for
    maps = [torch.from_numpy(a).cuda() for a in R.synthetic_maps(61, 8, 1, 256, 256)]
    ev = make()
    ev.update(*maps)
    ev.compute()
    torch.cuda.synchronize()
    cycles = _sleep_cycles_for(400.0)
    gate = torch.cuda.Event()
    torch.cuda._sleep(cycles)
    gate.record()
    t0 = time.perf_counter()
    blocked = 0
    for _ in range(16):  # grows both stores geometrically on the way: that, too, must not block
        ev.update(*maps)
        blocked += int(gate.query())
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    report(f"sparsification: 16 four-source updates of 8x256x256 enqueued in {host_ms:.1f} ms behind a 400 ms spin kernel; "
           f"found the gate complete: {blocked}")
    assert blocked == 0
    assert ev.compute()["n"] == 17 * 8 * 256 * 256
