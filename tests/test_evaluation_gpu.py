"""UncertaintyEvaluator on the GPU against the float64 restatement of the reference's tables (tests/eval_reference.py)
run live on the host, and against the fixture written by the real reference (tests/golden/eval_tables.npz).

Bounds (derived, not tuned):
* sparsification rows: the device and the restatement see bit-identical fp32 `error` / `combined_std` values and both
  sum in double; only the grouping of the additions differs -> 1e-9 relative per row.  Against the FIXTURE the
  reference's own float32-frame distance (tests/test_evaluation_cpu.py: FLOAT32_FRAME_DISTANCE, x 4) comes on top.
* calibration counts: the device compares `y < mu + s z_k` in fp32, the reference in float64.  For every threshold the
  restatement counts the pixels within delta = 2^-21 (|y| + |mu| + |s z_k|) of the quantile; the device count may differ
  from the exact one by at most that number, and the tests assert that this band holds at most 1e-4 N pixels.
* cutoff keys: exact (bit for bit).
"""
import time
import warnings

import numpy as np
import pytest
import torch

from tests import eval_reference as R
from tests.helpers import load_npz, report
from tests.test_evaluation_cpu import FLOAT32_FRAME_DISTANCE, fixture_maps

pytestmark = pytest.mark.gpu

PCT = np.arange(100) / 100.0
ROW_TOL = 1e-9


def make(**kw):
    from mimo.evaluation import UncertaintyEvaluator
    return UncertaintyEvaluator(**kw)


def feed(ev, maps, mask=None, splits=None):
    """maps: four [B,C,H,W] numpy arrays; splits: batch boundaries of the updates (default: one update)"""
    b = maps[0].shape[0]
    bounds = [0, b] if splits is None else [0] + list(splits) + [b]
    for i0, i1 in zip(bounds[:-1], bounds[1:]):
        ts = [torch.from_numpy(np.ascontiguousarray(a[i0:i1])).cuda() for a in maps]
        m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask[i0:i1])).cuda()
        ev.update(*ts, mask=m)


def device_counts(t):
    return np.rint(t["calibration"]["observed"] * t["n"]).astype(np.int64)


def tie_rule_rows(cols, percentiles):
    """The evaluator's definition where a cutoff falls inside a run of identical combined_std values: the run
    contributes its mean error / mean squared error for the number of its pixels that survive.  Equal to the plain
    restatement wherever no run straddles a cutoff."""
    std, err = cols["combined_std"], cols["error"].astype(np.float64)
    n = std.size
    order = np.argsort(std, kind="stable")  # ascending
    s, e = std[order], err[order]
    c1 = np.concatenate([[0.0], np.cumsum(e)])
    c2 = np.concatenate([[0.0], np.cumsum(e * e)])
    mae, rmse = np.full(len(percentiles), np.nan), np.full(len(percentiles), np.nan)
    for i, r in enumerate(R.cutoffs(percentiles, n)):
        left = n - r
        if left <= 0:
            continue
        key = s[left - 1]
        g0, g1 = np.searchsorted(s, key, "left"), np.searchsorted(s, key, "right")
        f = (left - g0) / (g1 - g0)
        mae[i] = (c1[g0] + (c1[g1] - c1[g0]) * f) / left
        rmse[i] = np.sqrt((c2[g0] + (c2[g1] - c2[g0]) * f) / left)
    return mae, rmse


def check(t, ev, maps, mask=None, clip=(0.0, 1.0), channel=0, tag="", allow_ties=False, check_band=True):
    """tables `t` of evaluator `ev` against the restatement on the same inputs; returns the restated pieces"""
    cols = R.pixel_columns(*maps, mask=mask, clip=clip, channel=channel)
    n = cols["error"].size
    assert (t["n"], t["n_masked"], t["n_nonfinite"]) == (n, cols["n_masked"], cols["n_nonfinite"])
    sp = R.sparsification(cols, ev.percentiles)
    ties = R.straddling_ties(sp["sorted_desc"], sp["cutoff"])
    if allow_ties:
        mae, rmse = tie_rule_rows(cols, ev.percentiles)
        free = ~np.isin(sp["cutoff"], ties)  # where no run straddles the cutoff the tie rule IS the plain restatement
        assert free.sum() >= len(free) // 2
        assert np.all(np.abs(mae[free] - sp["mae"][free]) <= ROW_TOL * sp["mae"][free])
        assert np.all(np.abs(rmse[free] - sp["rmse"][free]) <= ROW_TOL * sp["rmse"][free])
    else:
        assert not ties, f"{tag}: a tie straddles cutoffs {ties[:5]} — choose another seed"
        mae, rmse = sp["mae"], sp["rmse"]
    pr = t["precision_recall"]
    assert np.array_equal(pr["percentile"], ev.percentiles)
    assert np.array_equal(np.isnan(pr["mae"]), np.isnan(mae)) and np.array_equal(np.isnan(pr["rmse"]), np.isnan(rmse))
    e_mae = np.nanmax(np.abs(pr["mae"] - mae) / mae)
    e_rmse = np.nanmax(np.abs(pr["rmse"] - rmse) / rmse)
    assert np.array_equal(t["cutoff_keys"].astype(np.float32).view(np.uint32), sp["cutoff_keys"].astype(np.float32).view(np.uint32))
    e64 = cols["error"].astype(np.float64)
    e_all = max(abs(t["mae"] - e64.mean()) / e64.mean(), abs(t["mse"] - (e64 * e64).mean()) / (e64 * e64).mean())
    # thresholds: the evaluator's own float64 table — pinned to scipy (norm, laplace) and to the closed form by
    # tests/test_evaluation_cpu.py::test_standard_quantiles_match_scipy_to_one_ulp, so this is not circular
    cal = R.calibration(cols, ev.z)
    diff = np.abs(device_counts(t) - cal["counts"])
    report(f"eval {tag}: n {n}, rows mae {e_mae:.2e} rmse {e_rmse:.2e} whole-set {e_all:.2e}; ties at cutoffs {len(ties)}; "
           f"calibration band max {cal['band'].max()} count diff max {diff.max()}")
    assert e_mae <= ROW_TOL and e_rmse <= ROW_TOL and e_all <= ROW_TOL
    assert abs(t["rmse"] - np.sqrt((e64 * e64).mean())) <= ROW_TOL * t["rmse"]
    if check_band:
        assert cal["band"].max() <= 1e-4 * n, f"{tag}: the comparison band is too wide for this input"
    assert np.all(diff <= cal["band"]), (diff, cal["band"])
    assert np.array_equal(t["calibration"]["expected"], ev.expected_p)
    return cols, sp, cal


# ------------------------------------------------------------------------------------------ the fixture
def test_fixture_in_one_update_matches_restatement_and_reference():
    fx = load_npz("eval_tables.npz")
    maps = fixture_maps(fx, "maps")
    ev = make()
    feed(ev, maps)
    t = ev.compute()
    cols, sp, cal = check(t, ev, maps, tag="fixture, one update")
    ref_pr, ref_cal = fx["maps/pr"], fx["maps/cal"]
    for col, key in ((1, "mae"), (2, "rmse")):
        d = np.abs(t["precision_recall"][key] - ref_pr[:, col]).max() / ref_pr[:, col].max()
        report(f"eval fixture vs the reference's table, {key}: {d:.2e}")
        assert d <= 4 * FLOAT32_FRAME_DISTANCE + ROW_TOL
    assert np.all(np.abs(device_counts(t) - np.rint(ref_cal[:, 1] * t["n"])) <= cal["band"])


def test_fixture_in_three_uneven_updates():
    maps = fixture_maps(load_npz("eval_tables.npz"), "maps")
    one, three = make(), make()
    feed(one, maps)
    feed(three, maps, splits=[1, 3])
    a, b = one.compute(), three.compute()
    check(b, three, maps, tag="fixture, updates of 1 + 2 + 1 images")
    assert np.array_equal(a["calibration"]["observed"], b["calibration"]["observed"])  # counts are identical
    assert np.array_equal(a["cutoff_keys"], b["cutoff_keys"]) and a["n"] == b["n"]
    for key in ("mae", "rmse"):
        assert np.all(np.abs(a["precision_recall"][key] - b["precision_recall"][key]) <= ROW_TOL * a["precision_recall"][key])


@pytest.mark.parametrize("name", ["laplace", "gaussian"])
def test_reference_uncertainties_of_a_three_member_pair(name):
    """the maps the reference's own compute_uncertainties made of a (y_pred, log_param) pair with S = 3"""
    fx = load_npz("eval_tables.npz")
    maps = fixture_maps(fx, name)
    ev = make()
    feed(ev, maps)
    t = ev.compute()
    cols, sp, cal = check(t, ev, maps, tag=f"fixture {name} pair")
    for col, key in ((1, "mae"), (2, "rmse")):
        d = np.abs(t["precision_recall"][key] - fx[f"{name}/pr"][:, col]).max() / fx[f"{name}/pr"][:, col].max()
        assert d <= 4 * FLOAT32_FRAME_DISTANCE + ROW_TOL
    assert np.all(np.abs(device_counts(t) - np.rint(fx[f"{name}/cal"][:, 1] * t["n"])) <= cal["band"])


@pytest.mark.parametrize("name,loss", [("laplace", "laplace_nll"), ("gaussian", "gaussian_nll")])
def test_stored_pair_through_mimo_uncertainties_into_the_evaluator(name, loss):
    """(y_pred, log_param) with S = 3 -> mimo_uncertainties -> update, all on the device.  The engine's maps may differ
    from the reference's in the last bits, so the tables are held against the restatement on the engine's own maps (ties
    allowed: 2048 pixels, another rounding); that the maps are the reference's is tests/test_ops_gpu.py's business."""
    from mimo_unet_amd.engine import uncertainties
    fx = load_npz("eval_tables.npz")
    yp = torch.from_numpy(fx[f"{name}/y_pred"]).cuda().clip(min=0, max=1)
    maps = uncertainties(yp.contiguous(), torch.from_numpy(fx[f"{name}/log_param"]).cuda(), loss)
    label = torch.from_numpy(fx[f"{name}/label"]).cuda()
    ev = make()
    ev.update(*maps, label)
    t = ev.compute()
    check(t, ev, [m.cpu().numpy() for m in maps] + [fx[f"{name}/label"]], tag=f"{name} pair via mimo_uncertainties",
          allow_ties=True, check_band=False)
    for col, key in ((1, "mae"), (2, "rmse")):  # and the reference's table of the same pair: the maps agree to fp32 rounding
        d = np.abs(t["precision_recall"][key] - fx[f"{name}/pr"][:, col]).max() / fx[f"{name}/pr"][:, col].max()
        report(f"eval {name} pair via mimo_uncertainties vs the reference's table, {key}: {d:.2e}")


# ------------------------------------------------------------------------------------------ geometries
@pytest.fixture(scope="module")
def benchmark_batches():
    return [R.synthetic_maps(1000 + i, 32, 1, 256, 256) for i in range(8)]


@pytest.mark.parametrize("distribution", ["norm", "laplace"])
def test_benchmark_geometry_eight_updates_of_32x256x256(benchmark_batches, distribution):
    """16.8 M pixels.  float32 standard deviations collide at this count (a few of the 99 cutoffs fall inside a run of
    identical keys, where the reference's unstable sort defines nothing), so the rows are held against the restatement
    WITH the evaluator's tie rule — identical to the plain one at every cutoff that no run straddles."""
    ev = make(distribution=distribution)
    for maps in benchmark_batches:
        feed(ev, maps)
    t = ev.compute()
    allm = [np.concatenate([m[k] for m in benchmark_batches], 0) for k in range(4)]
    check(t, ev, allm, tag=f"8 x 32x1x256x256 {distribution}", allow_ties=True)
    obs = t["calibration"]["observed"]
    assert obs[0] == 0.0 and obs[-1] == 1.0 and np.all(np.diff(obs) >= 0)


@pytest.mark.parametrize("shape,seed", [((4, 1, 256, 256), 11), ((3, 1, 37, 53), 14)], ids=["shard-of-4", "odd-3x37x53"])
def test_shard_and_odd_sizes(shape, seed):
    maps = R.synthetic_maps(seed, *shape)
    ev = make()
    feed(ev, maps)
    check(ev.compute(), ev, maps, tag=f"{shape}")


def test_channel_one_of_two():
    maps = R.synthetic_maps(31, 3, 2, 40, 48)
    ev = make(channel=1)
    feed(ev, maps)
    cols, _, _ = check(ev.compute(), ev, maps, channel=1, tag="channel 1 of 2")
    other = R.pixel_columns(*maps, channel=0)
    assert not np.array_equal(cols["error"], other["error"])


def test_clip_none():
    maps = list(R.synthetic_maps(25, 2, 1, 64, 64))
    maps[0] = (maps[0] * 3.0 - 1.0).astype(np.float32)  # well outside [0, 1]
    maps[3] = (maps[3] * 3.0 - 1.0).astype(np.float32)
    ev, clipped = make(clip=None), make()
    feed(ev, maps)
    feed(clipped, maps)
    t = ev.compute()
    check(t, ev, maps, clip=None, tag="clip=None")
    assert t["mae"] != clipped.compute()["mae"]


def test_zero_scale_pixels_are_never_below():
    """aleatoric_var == 0: scipy's ppf is NaN at every p (scale must be > 0), so the pixel is "not below" in all 41 rows —
    whichever side of the mean its label lies on."""
    maps = [a.copy() for a in R.synthetic_maps(23, 1, 1, 32, 32)]
    mean, a_var, e_var, label = maps
    a_var.reshape(-1)[:200] = 0.0
    label.reshape(-1)[:100] = mean.reshape(-1)[:100].clip(0.2, 0.8) - 0.1  # y < mu
    label.reshape(-1)[100:200] = mean.reshape(-1)[100:200].clip(0.2, 0.8) + 0.1  # y > mu
    ev = make()
    feed(ev, maps)
    t = ev.compute()
    check(t, ev, maps, tag="200 pixels with scale 0", check_band=False)
    assert device_counts(t)[-1] == t["n"] - 200  # p = 1: everything but the zero-scale pixels
    only = make()
    feed(only, [a.reshape(-1)[:200].reshape(1, 1, 10, 20) for a in maps])
    assert np.all(only.compute()["calibration"]["observed"] == 0.0)


# ------------------------------------------------------------------------------------------ selection exactness
def hostile(kind):
    g = np.random.default_rng(31)
    shape = (2, 1, 96, 96)
    mean, _, _, label = R.synthetic_maps(32, *shape)
    e_var = np.zeros(shape, np.float32)
    if kind == "one-bucket":  # std in [0.5, 0.5 + 2^-12]: every key shares its top 11 (in fact 19) bits
        a_var = (0.25 + g.uniform(0, 2.4e-4, shape)).astype(np.float32)
    elif kind == "denormal":  # S = 1: no epistemic part; variances below the smallest normal float
        a_var = (g.uniform(0, 1, shape) * 1e-40).astype(np.float32)
        assert a_var.max() < np.finfo(np.float32).tiny
    elif kind == "thirty-decades":
        a_var = (10.0 ** g.uniform(-30, 0, shape)).astype(np.float32)
    else:  # fewer pixels than cutoffs
        sl = (slice(0, 1), slice(None), slice(0, 7), slice(0, 9))
        return [np.ascontiguousarray(a[sl]) for a in (mean, (10.0 ** g.uniform(-4, 0, shape)).astype(np.float32), e_var, label)]
    return [mean, a_var, e_var, label]


@pytest.mark.parametrize("kind", ["one-bucket", "denormal", "thirty-decades", "n-below-100"])
def test_selection_is_exact_on_hostile_keys(kind):
    maps = hostile(kind)
    ev = make()
    feed(ev, maps)
    t = ev.compute()
    cols = R.pixel_columns(*maps)
    std, n = cols["combined_std"], cols["error"].size
    if kind == "one-bucket":
        assert np.unique(std.view(np.uint32) >> 21).size == 1 and std.min() >= 0.5 and std.max() <= 0.5 + 2.0 ** -12
    kth = n - R.cutoffs(PCT, n) - 1  # ascending rank of the most uncertain survivor
    want = np.partition(std, np.unique(kth))[kth]
    assert np.array_equal(t["cutoff_keys"].astype(np.float32).view(np.uint32), want.view(np.uint32)), kind
    mae, rmse = tie_rule_rows(cols, PCT)
    assert np.all(np.abs(t["precision_recall"]["mae"] - mae) <= ROW_TOL * mae)
    assert np.all(np.abs(t["precision_recall"]["rmse"] - rmse) <= ROW_TOL * rmse)
    report(f"eval selection {kind}: n {n}, {np.unique(std).size} distinct keys, exact")


# ------------------------------------------------------------------------------------------ ties
def test_constant_std_gives_the_whole_set_mae_in_every_row():
    maps = list(R.synthetic_maps(41, 2, 1, 64, 64))
    maps[1] = np.full_like(maps[1], 0.01)
    maps[2] = np.zeros_like(maps[2])
    ev = make()
    feed(ev, maps)
    t = ev.compute()
    assert np.all(np.abs(t["precision_recall"]["mae"] - t["mae"]) <= ROW_TOL * t["mae"])
    assert np.all(np.abs(t["precision_recall"]["rmse"] - t["rmse"]) <= ROW_TOL * t["rmse"])
    assert np.all(t["cutoff_keys"].astype(np.float32) == np.sqrt(np.float32(0.01)))


def test_two_std_values_follow_the_tie_rule_in_closed_form():
    maps = list(R.synthetic_maps(42, 2, 1, 64, 64))
    n = maps[0].size
    big = np.zeros(n, bool)
    big[np.random.default_rng(43).permutation(n)[: (3 * n) // 5]] = True  # 60 % of the pixels carry the larger std
    maps[1] = np.where(big, np.float32(0.04), np.float32(0.01)).reshape(maps[1].shape).astype(np.float32)
    maps[2] = np.zeros_like(maps[2])
    ev = make()
    feed(ev, maps)
    t = ev.compute()
    e = R.pixel_columns(*maps)["error"].astype(np.float64)
    ea, eb, nb = e[~big], e[big], int(big.sum())
    for i, r in enumerate(R.cutoffs(PCT, n)):
        if r < nb:  # the cutoff lies inside the larger-std group: all of A, and nb - r pixels' worth of B's mean
            mae = (ea.sum() + (nb - r) * eb.mean()) / (n - r)
            mse = ((ea * ea).sum() + (nb - r) * (eb * eb).mean()) / (n - r)
        else:
            mae, mse = ea.mean(), (ea * ea).mean()
        assert abs(t["precision_recall"]["mae"][i] - mae) <= ROW_TOL * mae, i
        assert abs(t["precision_recall"]["rmse"][i] - np.sqrt(mse)) <= ROW_TOL * np.sqrt(mse), i


# ------------------------------------------------------------------------------------------ skipped pixels
def test_mask_removes_a_quarter_of_the_pixels():
    maps = R.synthetic_maps(51, 4, 1, 64, 64)
    mask = (np.random.default_rng(52).permutation(maps[0].size) % 4 != 0).astype(np.float32).reshape(4, 1, 64, 64)
    ev = make()
    feed(ev, maps, mask=mask)
    t = ev.compute()
    check(t, ev, maps, mask=mask, tag="mask removes 1/4")
    assert t["n_masked"] == maps[0].size // 4 and t["n"] == maps[0].size - t["n_masked"]


def test_nonfinite_pixels_are_counted_warned_about_and_left_out():
    maps = [a.copy() for a in R.synthetic_maps(57, 2, 1, 64, 64)]
    flat = [a.reshape(-1) for a in maps]
    flat[0][5] = np.nan
    flat[1][77] = np.inf
    flat[2][300] = -1e-3   # negative variance
    flat[3][4000] = -np.inf
    flat[1][5000] = -0.5
    flat[2][6001] = np.nan
    ev = make()
    feed(ev, maps)
    with pytest.warns(RuntimeWarning, match="6 pixels"):
        t = ev.compute()
    assert t["n_nonfinite"] == 6 and np.all(np.isfinite(t["precision_recall"]["mae"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        check(t, ev, maps, tag="6 non-finite pixels")


# ------------------------------------------------------------------------------------------ integration
def test_update_from_an_ensemble_module_equals_update_with_its_host_results():
    from mimo.models.ensemble import EnsembleModule
    from oracle import mimo_oracle as O
    from tests.test_network_gpu import build_model
    passes, B, p = 4, 2, 0.2
    cfg = O.NetConfig(3, 2, 2, 4)
    g = torch.Generator().manual_seed(5)
    model = build_model(cfg, O.init_state(cfg, 3), dropout=(p, p, p))
    specs = O.double_conv_specs(cfg)
    model.model.mask_override = {j: torch.bernoulli(torch.full((passes * B, cout), 1 - p), generator=g) / (1 - p)
                                 for j, (_, _, _, cout) in enumerate(specs)}
    image, label = torch.rand(B, 3, 32, 32, generator=g), torch.rand(B, 1, 32, 32, generator=g)
    ens = EnsembleModule([], models=[model], monte_carlo_steps=passes, keep_on_device=True)
    a = make()
    a.update_from(ens, image.cuda(), label.cuda())
    assert ens.keep_on_device is True
    ens.keep_on_device = False
    host = ens(image.cuda())
    assert all(not t.is_cuda for t in host)
    b = make()
    b.update(*[t.cuda() for t in host], label.cuda())
    ta, tb = a.compute(), b.compute()
    assert ta["n"] == B * 32 * 32 and np.isfinite(ta["mae"])
    for k in ("mae", "rmse"):
        assert np.array_equal(ta["precision_recall"][k], tb["precision_recall"][k])
    assert np.array_equal(ta["calibration"]["observed"], tb["calibration"]["observed"])
    assert np.array_equal(ta["cutoff_keys"], tb["cutoff_keys"])


def test_update_enqueues_without_a_host_synchronisation():
    """16 updates behind a ~0.4 s spin kernel: a blocking call inside update() (a synchronise, an .item(), a pageable
    copy) would return only after the spin kernel, and the gate event recorded behind it would then be complete."""
    from tests.test_data_gpu import _sleep_cycles_for
    maps = [torch.from_numpy(a).cuda() for a in R.synthetic_maps(61, 8, 1, 256, 256)]
    ev = make()
    ev.update(*maps)  # the record store exists (and has room for the growth below) after this
    ev.compute()
    torch.cuda.synchronize()
    cycles = _sleep_cycles_for(400.0)
    gate = torch.cuda.Event()
    torch.cuda._sleep(cycles)
    gate.record()
    t0 = time.perf_counter()
    blocked = 0
    for _ in range(16):  # grows the store geometrically on the way: that, too, must not block
        ev.update(*maps)
        blocked += int(gate.query())
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    report(f"eval: 16 updates of 8x256x256 enqueued in {host_ms:.1f} ms behind a 400 ms spin kernel; found the gate complete: {blocked}")
    assert blocked == 0
    assert ev.compute()["n"] == 17 * 8 * 256 * 256


def test_compute_twice_is_bit_identical_and_reset_empties():
    maps = R.synthetic_maps(71, 4, 1, 128, 128)
    ev = make()
    feed(ev, maps, splits=[1])
    a, b = ev.compute(), ev.compute()
    for k in ("mae", "rmse"):
        assert np.array_equal(a["precision_recall"][k].view(np.uint64), b["precision_recall"][k].view(np.uint64))
    assert np.array_equal(a["calibration"]["observed"], b["calibration"]["observed"]) and np.array_equal(a["cutoff_keys"], b["cutoff_keys"])
    assert (a["n"], a["mae"], a["mse"]) == (b["n"], b["mae"], b["mse"])
    ev.reset()
    e = ev.compute()
    assert e["n"] == 0 and e["n_masked"] == 0 and np.all(np.isnan(e["precision_recall"]["mae"]))
    feed(ev, maps, splits=[1])
    c = ev.compute()
    assert np.array_equal(a["precision_recall"]["mae"].view(np.uint64), c["precision_recall"]["mae"].view(np.uint64))
    assert np.array_equal(a["calibration"]["observed"], c["calibration"]["observed"])


def test_write_csv_from_the_device(tmp_path):
    maps = fixture_maps(load_npz("eval_tables.npz"), "maps")
    ev = make()
    feed(ev, maps)
    pr_path, cal_path = ev.write_csv(str(tmp_path))
    assert open(pr_path).readline().strip() == "percentile,mae,rmse"
    assert open(cal_path).readline().strip() == "Expected Conf.,Observed Conf."
    t = ev.compute()
    assert np.array_equal(np.loadtxt(pr_path, delimiter=",", skiprows=1)[:, 1], t["precision_recall"]["mae"])
