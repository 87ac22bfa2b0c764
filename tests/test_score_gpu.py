"""score_rules.hip on the GPU against the float64 definition of tests/score_reference.py: the three per-pixel maps per
element (bound: the project's rule of tests/scalar_reference.py — 4 x the distance of the SAME formulas in numpy float32 from
float64 on the same fp32 inputs, never below 4 fp32 ulp), special values, the accumulators against the kernel's own maps,
refusals, and `PredictiveScorer` end to end."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from tests import scalar_reference as SR
from tests import score_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 64)  # both sides of the register / LDS switch and of every tile capacity
P41 = np.arange(41) / 40.0
# floors of the per-element relative error (scalar_reference.py): the NLL is a signed sum (its zero crossing is cancellation),
# the CRPS a difference of positive sums, the PIT a mean of positive terms, meaningful down to where fp32 leaves its normal range
FLOORS = {"pit": SR.TINY, "nll": SR.frac_floor(SR.FLOOR_SIGNED), "crps": SR.frac_floor(SR.FLOOR_POSITIVE)}


def lib():
    from mimo_unet_amd import _lib
    return _lib, _lib.load()


def members_tensor(rng, B, S, C, hw):
    """fp32 p1, p2 [B,S,C,hw] and label [B,C,hw] of random mixtures (every channel its own draw)"""
    p1, p2, y = [], [], []
    for _ in range(C):
        m, s, l = R.random_members(rng, S, B * hw)
        p1.append(m.reshape(S, B, hw).transpose(1, 0, 2))
        p2.append(s.reshape(S, B, hw).transpose(1, 0, 2))
        y.append(l.reshape(B, hw))
    return (np.ascontiguousarray(np.stack(p1, axis=2)), np.ascontiguousarray(np.stack(p2, axis=2)),
            np.ascontiguousarray(np.stack(y, axis=1)))


def columns(p1, p2, label, channel):
    """member-major [S, B * hw] columns of one channel and its labels [B * hw], as the reference takes them"""
    B, S, C, hw = p1.shape
    return (p1[:, :, channel].transpose(1, 0, 2).reshape(S, B * hw), p2[:, :, channel].transpose(1, 0, 2).reshape(S, B * hw),
            label[:, channel].reshape(B * hw))


def device_copy(a, offset_floats=0):
    """the array on the device in a buffer that starts `offset_floats` floats after a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset_floats: offset_floats + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def launch(p1, p2, label, mask, channel, loss, expected_p=P41, maps=(True, True, True), offset=0, ws=None,
           eps=(R.EPS_MIN, R.EPS_MAX), members=None, null_input=False):
    """mimo_score_accumulate on numpy inputs; returns (status, [pit, nll, crps] numpy or None, workspace tensor)"""
    L, so = lib()
    B, S, C, hw = p1.shape
    d = [device_copy(t, offset) for t in (p1, p2, label)]
    dm = None if mask is None else device_copy(mask, offset)
    pk = torch.from_numpy(np.asarray(expected_p, dtype=np.float32)).cuda()
    if ws is None:
        ws = torch.zeros(so.mimo_score_workspace_bytes() // 8 + 1, dtype=torch.int64, device="cuda")
    outs = [device_copy(np.full((B, hw), np.nan, np.float32), offset) if m else None for m in maps]
    for o in outs:
        if o is not None:
            o.fill_(float("nan"))
    rc = so.mimo_score_accumulate(None if null_input else d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), L.ptr(dm) or None,
                                  B, S if members is None else members, C, channel, 1 if mask is None else mask.shape[1], hw,
                                  L.LOSS_KINDS[loss], eps[0], eps[1], pk.data_ptr(), pk.numel(),
                                  *[L.ptr(o) or None for o in outs], ws.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    return rc, [None if o is None else o.cpu().numpy().reshape(-1) for o in outs], ws


def acc_of(ws):
    """(bins [65], n, n_masked, n_nonfinite, sums [nll, crps, pit]) of a workspace"""
    words = ws[:71].cpu()
    counts = words[:68].numpy()
    return counts[:65].copy(), int(counts[65]), int(counts[66]), int(counts[67]), words[68:71].view(torch.float64).numpy().copy()


def check_maps(tag, got, p1, p2, label, mask, channel, loss):
    """the three maps per element on the scored pixels, NaN on the skipped ones"""
    mu, lp, y = columns(p1, p2, label, channel)
    B, S, C, hw = p1.shape
    mk = None if mask is None else mask[:, channel if mask.shape[1] > 1 else 0].reshape(-1)
    ok, _, _ = R.valid_pixels(mu, lp, y, mk)
    hi = R.score(mu[:, ok], lp[:, ok], y[ok], loss, np.float64)
    lo = R.score(mu[:, ok], lp[:, ok], y[ok], loss, np.float32)
    for k, g in zip(("pit", "nll", "crps"), got):
        assert np.all(np.isnan(g[~ok])), (tag, k, "a skipped pixel must hold NaN")
        ref = torch.from_numpy(hi[k])
        fl = FLOORS[k](ref) if callable(FLOORS[k]) else FLOORS[k]
        yard = SR.elem_err(torch.from_numpy(lo[k]), ref, fl)[0]
        SR.check("score_rules", f"{tag} {k}", torch.from_numpy(g[ok]), ref, fl, yard)
    return ok


GEOMETRIES = {  # name: (B, C, channel, hw, mask channels or None, pointer offset in floats)
    "aligned": (3, 1, 0, 64, None, 0),
    "odd": (3, 1, 0, 63, None, 0),
    "offset": (2, 1, 0, 64, None, 1),
    "channel": (2, 2, 1, 64, 2, 0),
    "mask1": (2, 2, 0, 68, 1, 0),
    "two_tiles": (2, 1, 0, 260, None, 0),
    "two_tiles_odd": (1, 1, 0, 259, 1, 0),
}


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("S", MEMBERS)
def test_maps_per_element_against_float64(loss, S):
    rng = np.random.default_rng(1000 + S)
    for name, (B, C, channel, hw, mc, offset) in GEOMETRIES.items():
        p1, p2, label = members_tensor(rng, B, S, C, hw)
        mask = None if mc is None else (rng.random((B, mc, hw)) > 0.3).astype(np.float32)
        rc, got, ws = launch(p1, p2, label, mask, channel, loss, offset=offset)
        assert rc == 0, name
        ok = check_maps(f"{loss} S={S} {name}", got, p1, p2, label, mask, channel, loss)
        bins, n, nm, nf, _ = acc_of(ws)
        assert (n, nm, nf) == (int(ok.sum()), int((~ok).sum()), 0) and bins.sum() == n, name


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("vec", [False, True])
def test_one_size_past_the_grid(loss, vec):
    """S = 2 with more pixels than one sweep of the largest grid covers: the grid-stride loop runs a second time.  Scalar
    walk: one pixel per thread, grid x 256 + 262 pixels; float4 walk: four per thread, 4 x grid x 256 + 264."""
    from mimo.evaluation import SCORE_MAX_WORKGROUPS
    hw = 4 * SCORE_MAX_WORKGROUPS * 256 + 264 if vec else SCORE_MAX_WORKGROUPS * 256 + 262
    assert (hw % 4 == 0) == vec
    rng = np.random.default_rng(5)
    p1, p2, label = members_tensor(rng, 1, 2, 1, hw)
    rc, got, ws = launch(p1, p2, label, None, 0, loss)
    assert rc == 0
    check_maps(f"{loss} S=2 hw={hw}", got, p1, p2, label, None, 0, loss)
    assert acc_of(ws)[1] == hw


def special_batch(S, loss):
    """one image of 16 pixels, all members N(0, .) / Laplace(0, .) with log-scale -2 except where planted"""
    rng = np.random.default_rng(9)
    p1 = (0.1 * rng.standard_normal((1, S, 1, 16))).astype(np.float32)
    p2 = np.full((1, S, 1, 16), -2.0, np.float32)
    y = (0.1 * rng.standard_normal((1, 1, 16))).astype(np.float32)
    last = S - 1
    p1[0, last, 0, 0] = np.nan      # 0: a NaN mean
    y[0, 0, 1] = np.inf             # 1: an infinite label
    p2[0, 0, 0, 2] = np.inf         # 2, 3: an infinite log-scale
    p2[0, last, 0, 3] = -np.inf
    p2[0, 0, 0, 4] = 100.0          # 4: clamps to eps_max
    p2[0, last, 0, 5] = -100.0      # 5: clamps to eps_min
    theta = np.float32(np.exp(np.float32(-2.0)))
    width = theta if loss == "laplace_nll" else np.sqrt(theta)
    p1[0, :, 0, 6:8] = 0.25
    y[0, 0, 6] = np.float32(0.25 + 1e3 * width)   # 6, 7: a label 1e3 scales away, above and below
    y[0, 0, 7] = np.float32(0.25 - 1e3 * width)
    # 8: equal scales, distinct means (the batch's default); 9: the label exactly on a member's mean
    y[0, 0, 9] = p1[0, 0, 0, 9]
    p2[0, :, 0, 10] = np.linspace(-2.0, -2.0 + 1e-6, S, dtype=np.float32)  # 10: scales a few ulp apart
    p1[0, :, 0, 11] = p1[0, 0, 0, 11]                                       # 11: identical members
    return p1, p2, y


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("S", [1, 3, 9])
def test_special_values(loss, S):
    p1, p2, label = special_batch(S, loss)
    rc, got, ws = launch(p1, p2, label, None, 0, loss)
    assert rc == 0
    ok = check_maps(f"{loss} S={S} special", got, p1, p2, label, None, 0, loss)
    assert list(np.flatnonzero(~ok)) == [0, 1, 2, 3]
    bins, n, nm, nf, _ = acc_of(ws)
    assert (n, nm, nf) == (12, 0, 4)
    pit, nll, _ = got
    assert pit[6] == 1.0 and pit[7] == 0.0 and np.isfinite(nll[6]) and np.isfinite(nll[7]) and nll[6] > 100
    # PIT = 1 is never below; PIT = 0 is below from p_1 on (not below p_0 = 0)
    assert bins[41] == int((pit[ok] == 1).sum()) >= 1 and bins[0] == 0 and bins[1] == int((pit[ok] < 0.025).sum()) >= 1


def test_accumulators_against_the_kernels_own_maps():
    from mimo.evaluation import PredictiveScorer
    rng = np.random.default_rng(21)
    B, S, C, hw = 3, 5, 1, 33 * 31
    p1, p2, label = members_tensor(rng, B, S, C, hw)
    mask = (rng.random((B, 1, hw)) > 0.2).astype(np.float32)
    p1[1, 2, 0, 17] = np.nan
    label[2, 0, 5] = -np.inf
    mask[1, 0, 17] = mask[2, 0, 5] = 1.0
    t = lambda a: torch.from_numpy(a).cuda().view(*a.shape[:-1], 33, 31)
    tp1, tp2, tl, tm = t(p1), t(p2), t(label), t(mask)
    sc = PredictiveScorer()
    pit, nll, crps = (m.cpu().numpy().reshape(-1) for m in sc.score_maps(tp1, tp2, tl, tm, "gaussian_nll"))
    valid = ~np.isnan(pit)
    assert np.array_equal(valid, ~np.isnan(nll)) and np.array_equal(valid, ~np.isnan(crps))
    bins, n, nm, nf, sums = acc_of(sc._ws)
    want = R.pit_bins(pit[valid], P41.astype(np.float32))
    assert np.array_equal(bins[:42], want) and not bins[42:].any()
    assert (n, nm, nf) == (int(valid.sum()), int((mask == 0).sum()), 2)

    def close(a, m):  # the bound on reordering a double sum of the N values of m
        x = m[valid].astype(np.float64)
        return abs(a - x.sum()) <= x.size * 2.0 ** -52 * np.abs(x).sum()
    assert close(sums[0], nll) and close(sums[1], crps) and close(sums[2], pit)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = sc.compute()
    assert any("non-finite" in str(x.message) for x in w)
    ref = R.summarize(pit[valid], nll[valid], crps[valid], P41, nm, nf)
    assert np.array_equal(res["calibration"]["observed"], ref["calibration"]["observed"])
    assert (res["n"], res["n_masked"], res["n_nonfinite"]) == (n, nm, nf)
    for k in ("nll", "crps", "pit_mean", "calibration_error"):
        assert res[k] == pytest.approx(ref[k], rel=1e-12, abs=1e-15), k
    assert res["coverage"] == pytest.approx(ref["coverage"]) and len(res["coverage"]) == 20
    first_bits = sc._ws[:71].clone(), sc._out.clone()

    # the two halves of the batch in two updates: the same counts, sums within the reordering bound
    halves = PredictiveScorer()
    halves.update(tp1[:1], tp2[:1], tl[:1], tm[:1], "gaussian_nll")
    halves.update(tp1[1:], tp2[1:], tl[1:], tm[1:], "gaussian_nll")
    hb, hn, hnm, hnf, hs = acc_of(halves._ws)
    assert np.array_equal(hb, bins) and (hn, hnm, hnf) == (n, nm, nf)
    assert close(hs[0], nll) and close(hs[1], crps) and close(hs[2], pit)

    # the same calls again: identical bits; without the maps: identical accumulator bits
    again = PredictiveScorer()
    again.score_maps(tp1, tp2, tl, tm, "gaussian_nll")
    again.compute()
    assert torch.equal(again._ws[:71], first_bits[0]) and torch.equal(again._out.view(torch.int64), first_bits[1].view(torch.int64))
    nomaps = PredictiveScorer()
    nomaps.update(tp1, tp2, tl, tm, "gaussian_nll")
    assert torch.equal(nomaps._ws[:71], first_bits[0])

    # reset clears; compute() at n = 0
    sc.reset()
    assert not bool(sc._ws.any())
    empty = sc.compute()
    assert (empty["n"], empty["n_masked"], empty["n_nonfinite"]) == (0, 0, 0) and len(empty["coverage"]) == 20
    assert all(np.isnan(empty[k]) for k in ("nll", "crps", "pit_mean", "calibration_error"))
    assert np.all(np.isnan(empty["calibration"]["observed"]))


def test_refusals_launch_nothing():
    L, so = lib()
    rng = np.random.default_rng(2)
    p1, p2, label = members_tensor(rng, 1, 2, 1, 64)
    for kw in ({"members": 65}, {"members": 0}, {"null_input": True}, {"eps": (0.0, 1e3)}, {"eps": (1.0, 0.5)},
               {"expected_p": np.arange(65) / 64.0}):
        rc, got, ws = launch(p1, p2, label, None, 0, "laplace_nll", **kw)
        assert rc == -1, kw  # MIMO_ERR_INVALID
        assert all(np.all(np.isnan(g)) for g in got) and not bool(ws.any()), kw
        assert b"mimo_score_accumulate" in so.mimo_last_error()
    out = torch.full((47,), float("nan"), dtype=torch.float64, device="cuda")
    assert so.mimo_score_finalize(None, 41, out.data_ptr(), L.current_stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def tiny_models(dropout):
    from mimo.models.mimo_unet import MimoUnetModel
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        models.append(MimoUnetModel(in_channels=3, out_channels=2, num_subnetworks=2, filter_base_count=4, center_dropout_rate=0.0,
                                    final_dropout_rate=0.0, encoder_dropout_rate=dropout, core_dropout_rate=dropout,
                                    decoder_dropout_rate=dropout, loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3,
                                    seed=seed, loss_buffer_size=10, loss_buffer_temperature=0.3).cuda())
    return models


@pytest.mark.parametrize("passes", [0, 3])
def test_update_from_an_ensemble(passes, tmp_path):
    from mimo.evaluation import PredictiveScorer
    from mimo.models.ensemble import EnsembleModule
    ens = EnsembleModule([], monte_carlo_steps=passes, models=tiny_models(0.1 if passes else 0.0), keep_on_device=False)
    g = torch.Generator().manual_seed(3)
    image, label = torch.rand(2, 3, 32, 32, generator=g).cuda(), torch.rand(2, 1, 32, 32, generator=g).cuda()
    a = PredictiveScorer()
    torch.cuda.manual_seed(99)
    a.update_from(ens, image, label)
    assert (ens.keep_on_device, ens.return_raw_predictions) == (False, False)
    ens.return_raw_predictions = True
    torch.cuda.manual_seed(99)
    p1, p2 = ens.forward_on_device(image)
    ens.return_raw_predictions = False
    assert p1.shape == (2, 4 * max(1, passes), 1, 32, 32)
    b = PredictiveScorer()
    b.update(p1, p2, label, None, "laplace_nll", ens.loss_fn.eps_min, ens.loss_fn.eps_max)
    assert torch.equal(a._ws[:71], b._ws[:71])
    res = a.compute()
    assert res["n"] == 2 * 32 * 32 and np.isfinite(res["nll"]) and res["crps"] > 0 and 0 <= res["pit_mean"] <= 1

    class Boom(RuntimeError):
        pass

    def fail(x):
        raise Boom()
    ens.forward_on_device = fail
    with pytest.raises(Boom):
        a.update_from(ens, image, label)
    assert (ens.keep_on_device, ens.return_raw_predictions) == (False, False)

    paths = a.write_csv(str(tmp_path / "csv"), res)
    assert [os.path.basename(p) for p in paths] == ["scores.csv", "calibration_mixture.csv"]
    assert open(paths[0]).readline().rstrip("\n") == "n,n_masked,n_nonfinite,nll,crps,pit_mean,calibration_error"
    assert open(paths[1]).readline().rstrip("\n") == "Expected Conf.,Observed Conf."
    cal = np.loadtxt(paths[1], delimiter=",", skiprows=1)
    assert np.array_equal(cal[:, 0], P41) and np.array_equal(cal[:, 1], res["calibration"]["observed"])


def test_update_from_refuses_before_any_launch():
    from mimo.evaluation import PredictiveScorer
    from mimo.models.ensemble import EnsembleModule
    ens = EnsembleModule([], monte_carlo_steps=17, models=tiny_models(0.1), keep_on_device=True)  # 17 x 4 = 68 members
    called = []
    ens.forward_on_device = lambda x: called.append(1)
    sc = PredictiveScorer()
    with pytest.raises(ValueError, match="68"):
        sc.update_from(ens, torch.zeros(1, 3, 32, 32).cuda(), torch.zeros(1, 1, 32, 32).cuda())
    assert not called and not bool(sc._ws.any())


def test_evaluate_uncertainty_script_scores_synthetic_data(tmp_path):
    out = str(tmp_path / "res")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_uncertainty.py"), "--synthetic_model", "--synthetic", "1",
           "--batch", "2", "--size", "32", "--monte_carlo_steps", "2", "--scores", "--result_dir", out]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    assert res["scores"]["n"] == 2 * 32 * 32 and np.isfinite(res["scores"]["nll"]) and res["scores"]["members"] == 4
    for name in ("scores.csv", "calibration_mixture.csv", "precision_recall.csv", "calibration.csv"):
        assert os.path.exists(os.path.join(out, name)), name
