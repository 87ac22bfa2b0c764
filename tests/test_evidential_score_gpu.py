"""score_evidential.hip on the GPU against the float64 definition of tests/evidential_score_reference.py: the three
per-pixel maps per element, special values, the accumulators against the kernel's own maps, replay, a mixture and an
evidential update in one workspace, the grid stride, refusals, and `PredictiveScorer.update_from_evidential` end to end.

Bounds.  Exact heads (logits above the softplus threshold: the kernel's heads ARE the reference's): 4 fp32 ulp of
max(|ref|, floor) per element (scalar_reference.check with yardstick 0), floors as in tests/test_score_gpu.py.  Soft heads
(the device softplus is within a few ulp of the rounded float64 one): scalar_reference.check_conditioned's bound,
max(COND_MARGIN x the change of the float64 result when one of v, alpha, beta moves one fp32 ulp, 4 ulp of max(|ref|,
floor)); the ranges drawn ([-9, 9] logits, |z| <= 8) keep COND_MARGIN x that change below 1e-4 of max(|ref|, floor)
for every element, which is asserted on the reference before the kernel is looked at (and without a GPU in
tests/test_evidential_score_reference_cpu.py) — the ranges did not have to be narrowed."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from tests import evidential_score_reference as E
from tests import scalar_reference as SR
from tests import score_reference as R
from tests.helpers import report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P41 = np.arange(41) / 40.0
GEOMETRIES = {  # name: (B, hw, pointer offset in floats)
    "aligned": (3, 64, 0),
    "odd": (3, 63, 0),
    "two_blocks": (2, 260, 0),
    "offset": (2, 64, 1),
}


def lib():
    from mimo_unet_amd import _lib
    return _lib, _lib.load()


def device_copy(a, offset_floats=0):
    """the array on the device in a buffer that starts `offset_floats` floats after a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset_floats: offset_floats + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def to_layout(logits, y, B):
    """[4, N] / [N] pixel lists -> logits [B, 4, hw], label [B, 1, hw]"""
    hw = y.size // B
    return np.ascontiguousarray(logits.reshape(4, B, hw).transpose(1, 0, 2)), np.ascontiguousarray(y.reshape(B, 1, hw))


def launch(logits, label, mask=None, expected_p=P41, maps=(True, True, True), offset=0, ws=None, **bad):
    """mimo_score_accumulate_evidential on numpy logits [B,4,hw], label [B,1,hw], mask [B,hw]; returns (status, [pit, nll,
    crps] numpy or None, workspace tensor).  bad: batch= / hw= / null_input= / misalign= for the refusals."""
    L, so = lib()
    B, _, hw = logits.shape
    d = [device_copy(t, offset) for t in (logits, label)]
    dm = None if mask is None else device_copy(mask, offset)
    pk = torch.from_numpy(np.asarray(expected_p, dtype=np.float32)).cuda()
    if ws is None:
        ws = torch.zeros(so.mimo_score_workspace_bytes() // 8 + 1, dtype=torch.int64, device="cuda")
    outs = [device_copy(np.full((B, hw), np.nan, np.float32), offset) if m else None for m in maps]
    p_logits = None if bad.get("null_input") else d[0].data_ptr() + int(bad.get("misalign", 0))
    rc = so.mimo_score_accumulate_evidential(p_logits, d[1].data_ptr(), L.ptr(dm) or None, bad.get("batch", B), bad.get("hw", hw),
                                             pk.data_ptr(), pk.numel(), *[L.ptr(o) or None for o in outs], ws.data_ptr(),
                                             L.current_stream())
    torch.cuda.synchronize()
    return rc, [None if o is None else o.cpu().numpy().reshape(-1) for o in outs], ws


def acc_of(ws):
    """(bins [65], n, n_masked, n_nonfinite, sums [nll, crps, pit]) of a workspace"""
    words = ws[:71].cpu()
    counts = words[:68].numpy()
    return counts[:65].copy(), int(counts[65]), int(counts[66]), int(counts[67]), words[68:71].view(torch.float64).numpy().copy()


def pixel_lists(logits, label, mask):
    B, _, hw = logits.shape
    return logits.transpose(1, 0, 2).reshape(4, B * hw), label.reshape(-1), None if mask is None else mask.reshape(-1)


def floor_of(k, ref):
    fl = E.FLOORS[k]
    return fl(ref) if callable(fl) else fl


def check_counts(tag, ws, ok, masked, bad):
    bins, n, nm, nf, _ = acc_of(ws)
    assert (n, nm, nf) == (int(ok.sum()), int(masked.sum()), int(bad.sum())) and bins.sum() == n, tag


def check_soft(tag, got, logits, y):
    """maps `got` (each [N]) of the pixel list logits [4, N], y [N], every pixel scored, against the float64 reference within
    scalar_reference.check_conditioned's bound; returns the worst error / bound"""
    mu, v, alpha, beta = E.heads(logits)
    inputs = [torch.from_numpy(mu), torch.from_numpy(np.stack([v, alpha, beta], axis=1)), torch.from_numpy(y)]
    cond = SR.conditioning(E.torch_fn64, inputs, 1)
    ref = E.torch_fn64(*[SR.to64(t) for t in inputs])
    everywhere = torch.ones(y.size, dtype=torch.bool)
    worst = 0.0
    for k, g in zip(("pit", "nll", "crps"), got):
        q = SR.check_conditioned("score_evidential", f"{tag} {k}", torch.from_numpy(np.ascontiguousarray(g)), ref[k],
                                 floor_of(k, ref[k]), cond[k], everywhere)
        worst = max(worst, q / SR.COND_MARGIN)
    return worst


def allowed_error(logits, y):
    """({name: float64 reference [N]}, {name: check_conditioned's allowed |error| per element [N]})"""
    mu, v, alpha, beta = E.heads(logits)
    inputs = [torch.from_numpy(mu), torch.from_numpy(np.stack([v, alpha, beta], axis=1)), torch.from_numpy(y)]
    cond = SR.conditioning(E.torch_fn64, inputs, 1)
    ref = E.torch_fn64(*[SR.to64(t) for t in inputs])
    allowed = {k: torch.maximum(SR.COND_MARGIN * cond[k], SR.MARGIN * SR.ULP32 * torch.maximum(
        ref[k].abs(), torch.as_tensor(floor_of(k, ref[k]), dtype=torch.float64))).numpy() for k in ref}
    return {k: v.numpy() for k, v in ref.items()}, allowed


@pytest.fixture(scope="module")
def exact_cases():
    """per geometry, with and without a mask: inputs and the float64 reference, computed once"""
    rng = np.random.default_rng(77)
    cases = {}
    for name, (B, hw, offset) in GEOMETRIES.items():
        for masked in (False, True):
            logits, y = E.exact_head_inputs(rng, B * hw)
            mask = (rng.random((B, hw)) > 0.3).astype(np.float32) if masked else None
            cases[(name, masked)] = (to_layout(logits, y, B) + (mask, offset), E.score_logits(logits, y))
    return cases


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_exact_heads_per_element_against_float64(exact_cases, name, masked):
    (logits, label, mask, offset), ref = exact_cases[(name, masked)]
    rc, got, ws = launch(logits, label, mask, offset=offset)
    assert rc == 0
    ok, mk, bad = E.valid_pixels(*pixel_lists(logits, label, mask))
    assert not bad.any()
    for k, g in zip(("pit", "nll", "crps"), got):
        assert np.all(np.isnan(g[~ok])), (k, "a skipped pixel must hold NaN")
        r = torch.from_numpy(ref[k][ok])
        SR.check("score_evidential", f"exact heads {name} mask={masked} {k}", torch.from_numpy(g[ok]), r, floor_of(k, r), 0.0)
    check_counts(name, ws, ok, mk, bad)


@pytest.mark.parametrize("masked", [False, True])
def test_soft_heads_per_element_against_float64(masked):
    rng = np.random.default_rng(1)
    worst = 0.0
    for name, (B, hw, offset) in GEOMETRIES.items():
        logits, y = E.soft_head_inputs(rng, B * hw)
        assert np.any(E.heads(logits)[2] == 1.0)  # alpha == 1 exactly is among the pixels, and is scored
        for k, w in E.soft_head_condition(logits, y).items():  # the condition the bound rests on, on the reference alone
            assert w < 1e-4, (name, k, w)
        lg, label = to_layout(logits, y, B)
        mask = (rng.random((B, hw)) > 0.3).astype(np.float32) if masked else None
        rc, got, ws = launch(lg, label, mask, offset=offset)
        assert rc == 0
        ok, mk, bad = E.valid_pixels(logits, y, None if mask is None else mask.reshape(-1))
        assert not bad.any()
        for k, g in zip(("pit", "nll", "crps"), got):
            assert np.all(np.isnan(g[~ok])), (name, k)
        worst = max(worst, check_soft(f"soft heads {name} mask={masked}", [g[ok] for g in got], logits[:, ok], y[ok]))
        check_counts(name, ws, ok, mk, bad)
    report(f"[score_evidential] soft heads mask={masked}: worst error / bound {worst:.3f}")


def test_special_values():
    """one launch: non-finite inputs, underflowed heads, a masked pixel, y == mu, |z| ~ 1e6, l2 = 3e4"""
    hw = 24
    logits = np.zeros((1, 4, hw), np.float32)
    logits[0, 0] = np.linspace(-1, 1, hw)
    label = (logits[0, 0] + 0.3).reshape(1, 1, hw).copy()
    mask = np.ones((1, hw), np.float32)
    nonfinite = []
    for i, (c, val) in enumerate([(c, val) for c in range(4) for val in (np.nan, np.inf, -np.inf)]):  # 0 .. 11
        logits[0, c, i] = val
        nonfinite.append(i)
    label[0, 0, 12], label[0, 0, 13], label[0, 0, 14] = np.nan, np.inf, -np.inf
    logits[0, 1, 15] = -120.0   # v == 0
    logits[0, 3, 16] = -120.0   # beta == 0
    nonfinite += [12, 13, 14, 15, 16]
    mask[0, 17] = 0.0
    logits[0, 3, 17] = np.nan   # masked first
    label[0, 0, 18] = logits[0, 0, 18]                       # y == mu
    logits[0, 2, 19] = -30.0                                 # alpha == 1, y == mu
    label[0, 0, 19] = logits[0, 0, 19]
    sigma = np.sqrt(np.log(2.0) * (1 + np.log(2.0)) / (np.log(2.0) * (np.log(2.0) + 1)))  # = 1 at zero logits
    label[0, 0, 20] = np.float32(logits[0, 0, 20] + 1e6 * sigma)    # |z| ~ 1e6 above and below
    label[0, 0, 21] = np.float32(logits[0, 0, 21] - 1e6 * sigma)
    logits[0, 2, 22] = 3.0e4                                  # nu = 6e4 + 2
    logits[0, 2, 23] = 3.0e4
    logits[0, 1, 23], logits[0, 3, 23] = 30.0, 500.0
    label[0, 0, 23] = np.float32(logits[0, 0, 23] - 1e6)
    rc, got, ws = launch(logits, label, mask)
    assert rc == 0
    ok, mk, bad = E.valid_pixels(*pixel_lists(logits, label, mask))
    assert list(np.flatnonzero(bad)) == nonfinite and list(np.flatnonzero(mk)) == [17]
    pit, nll, crps = got
    for g in got:
        assert np.all(np.isnan(g[~ok])) and np.all(np.isfinite(g[ok]))
    check_counts("special", ws, ok, mk, bad)
    assert pit[18] == 0.5 and pit[19] == 0.5
    assert 0.0 <= pit[21] < 1e-6 and 1 - 1e-6 < pit[20] <= 1.0 and 0.0 <= pit[23] <= 1e-30
    assert np.all(crps[ok] > 0) and crps[20] > 1e5 and crps[21] > 1e5
    lg, y, _ = pixel_lists(logits, label, mask)
    check_soft("special values", [g[ok] for g in got], lg[:, ok], y[ok])  # zero logits are soft heads
    bins = acc_of(ws)[0]
    assert bins[41] == int((pit[ok] == 1).sum()) and bins[0] == 0 and not bins[42:].any()


def test_accumulators_replay_and_a_shared_workspace():
    from mimo.evaluation import PredictiveScorer
    rng = np.random.default_rng(21)
    B, h, w = 3, 33, 31
    logits, y = E.soft_head_inputs(rng, B * h * w)
    lg, label = to_layout(logits, y, B)
    mask = (rng.random((B, h * w)) > 0.2).astype(np.float32)
    lg[1, 2, 17] = np.nan
    label[2, 0, 5] = -np.inf
    lg[0, 1, 40] = -120.0
    mask[1, 17] = mask[2, 5] = mask[0, 40] = 1.0
    tl = torch.from_numpy(lg).cuda().view(B, 4, h, w)
    ty = torch.from_numpy(label).cuda().view(B, 1, h, w)
    tm = torch.from_numpy(mask).cuda().view(B, h, w)
    sc = PredictiveScorer()
    pit, nll, crps = (m.cpu().numpy().reshape(-1) for m in sc.score_maps_evidential(tl, ty, tm))
    valid = ~np.isnan(pit)
    assert np.array_equal(valid, ~np.isnan(nll)) and np.array_equal(valid, ~np.isnan(crps))
    bins, n, nm, nf, sums = acc_of(sc._ws)
    want = R.pit_bins(pit[valid], P41.astype(np.float32))
    assert np.array_equal(bins[:42], want) and not bins[42:].any()
    assert (n, nm, nf) == (int(valid.sum()), int((mask == 0).sum()), 3)
    for got, m in zip(sums, (nll, crps, pit)):
        x = m[valid].astype(np.float64)
        assert abs(got - x.sum()) <= 1e-12 * np.abs(x).sum()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = sc.compute()
    assert any("skipped" in str(x.message) for x in caught)
    ref = R.summarize(pit[valid], nll[valid], crps[valid], P41, nm, nf)
    assert np.array_equal(res["calibration"]["observed"], ref["calibration"]["observed"])
    assert (res["n"], res["n_masked"], res["n_nonfinite"]) == (n, nm, nf)
    for k in ("nll", "crps", "pit_mean", "calibration_error"):
        assert res[k] == pytest.approx(ref[k], rel=1e-12, abs=1e-15), k
    first = sc._ws[:72].clone()
    assert 1 <= int(first[71]) <= 160  # the most iterations of the continued fraction any pixel took, within the cap

    # the same calls again, with a [B,1,H,W] mask and without the maps: identical bits
    again = PredictiveScorer()
    again.update_evidential(tl, ty, tm.view(B, 1, h, w))
    assert torch.equal(again._ws[:72], first)
    # two halves in two updates: the same counts, twice the sequence: the same bits
    a, b = PredictiveScorer(), PredictiveScorer()
    for s in (a, b):
        s.update_evidential(tl[:1], ty[:1], tm[:1])
        s.update_evidential(tl[1:], ty[1:], tm[1:])
    assert torch.equal(a._ws, b._ws)
    hb, hn, hnm, hnf, hs = acc_of(a._ws)
    assert np.array_equal(hb, bins) and (hn, hnm, hnf) == (n, nm, nf) and np.allclose(hs, sums, rtol=1e-12, atol=0)

    # a mixture update and an evidential update into one workspace add up
    mu, p2, ym = R.random_members(rng, 3, 2 * 64)
    p1 = torch.from_numpy(mu.reshape(3, 2, 1, 8, 8).transpose(1, 0, 2, 3, 4).copy()).cuda()
    p2 = torch.from_numpy(p2.reshape(3, 2, 1, 8, 8).transpose(1, 0, 2, 3, 4).copy()).cuda()
    ym = torch.from_numpy(ym.reshape(2, 1, 8, 8)).cuda()
    mix = PredictiveScorer()
    mix.update(p1, p2, ym)
    mb, mn, _, _, ms = acc_of(mix._ws)
    both = PredictiveScorer()
    both.update(p1, p2, ym)
    both.update_evidential(tl, ty, tm)
    bb, bn, bnm, bnf, bs = acc_of(both._ws)
    assert np.array_equal(bb, mb + bins) and (bn, bnm, bnf) == (mn + n, nm, nf)
    assert np.allclose(bs, ms + sums, rtol=1e-12, atol=0)
    assert both.compute()["n"] == mn + n


@pytest.mark.parametrize("vec", [False, True])
def test_one_size_past_the_grid(vec):
    """more pixels than one sweep of the largest grid covers: the grid-stride loop runs a second time.  Scalar walk: one pixel
    per thread, grid x 256 + 262 pixels; float4 walk: four per thread, 4 x grid x 256 + 264.  Counts, and the maps on a
    strided sample plus the pixels past the first sweep."""
    from mimo.evaluation import SCORE_MAX_WORKGROUPS
    hw = 4 * SCORE_MAX_WORKGROUPS * 256 + 264 if vec else SCORE_MAX_WORKGROUPS * 256 + 262
    assert (hw % 4 == 0) == vec
    rng = np.random.default_rng(5)
    logits, y = E.soft_head_inputs(rng, hw, zmax=4.0, span=3.0)
    lg, label = to_layout(logits, y, 1)
    rc, got, ws = launch(lg, label, None)
    assert rc == 0
    bins, n, nm, nf, _ = acc_of(ws)
    assert (n, nm, nf) == (hw, 0, 0) and bins.sum() == hw
    pick = np.unique(np.concatenate([np.arange(0, hw, 997), np.arange(hw - 300, hw)]))
    assert all(np.all(np.isfinite(g)) for g in got)
    check_soft(f"hw={hw}, {pick.size} sampled pixels", [g[pick] for g in got], logits[:, pick], y[pick])


def test_refusals_launch_nothing():
    L, so = lib()
    rng = np.random.default_rng(2)
    logits, y = E.soft_head_inputs(rng, 64)
    lg, label = to_layout(logits, y, 1)
    for kw in ({"null_input": True}, {"batch": 0}, {"hw": 0}, {"expected_p": np.arange(65) / 64.0}, {"misalign": 2}):
        rc, got, ws = launch(lg, label, None, **kw)
        assert rc == -1, kw  # MIMO_ERR_INVALID
        assert all(np.all(np.isnan(g)) for g in got) and not bool(ws.any()), kw
        assert b"mimo_score_accumulate_evidential" in so.mimo_last_error()
    ws = torch.zeros(so.mimo_score_workspace_bytes() // 8 + 1, dtype=torch.int64, device="cuda")
    d = device_copy(lg), device_copy(label)
    pk = torch.from_numpy(P41.astype(np.float32)).cuda()
    for args in ((d[0].data_ptr(), d[1].data_ptr(), None, 1, 64, pk.data_ptr(), 0, None, None, None, ws.data_ptr()),
                 (d[0].data_ptr(), d[1].data_ptr(), None, 1, 64, None, 41, None, None, None, ws.data_ptr()),
                 (d[0].data_ptr(), None, None, 1, 64, pk.data_ptr(), 41, None, None, None, ws.data_ptr()),
                 (d[0].data_ptr(), d[1].data_ptr(), None, 1, 64, pk.data_ptr(), 41, None, None, None, None),
                 (d[0].data_ptr(), d[1].data_ptr(), None, 1, 64, pk.data_ptr(), 41, None, None, None, ws.data_ptr() + 8)):
        assert so.mimo_score_accumulate_evidential(*args, L.current_stream()) == -1
    torch.cuda.synchronize()
    assert not bool(ws.any())


def evidential_model(seed=0):
    from mimo.models.evidential_unet import EvidentialUnetModel
    torch.manual_seed(seed)
    return EvidentialUnetModel(in_channels=3, out_channels=4, filter_base_count=4, center_dropout_rate=0.0, final_dropout_rate=0.0,
                               encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0,
                               learning_rate=1e-3, seed=seed).cuda().eval()


def test_update_from_an_evidential_model():
    from mimo.evaluation import PredictiveScorer
    from mimo.models.ensemble import EnsembleModule
    from tests.test_score_gpu import tiny_models
    model = evidential_model()
    g = torch.Generator().manual_seed(3)
    image, label = torch.rand(2, 3, 32, 32, generator=g).cuda(), torch.rand(2, 1, 32, 32, generator=g).cuda()
    mask = (torch.rand(2, 32, 32, generator=g) > 0.25).float().cuda()
    sc = PredictiveScorer()
    sc.update_from_evidential(model, image, label, mask)
    res = sc.compute()
    with torch.no_grad():
        logits = model._logits(image)
    assert logits.shape == (2, 4, 32, 32) and not logits.requires_grad
    lg = logits.cpu().numpy().reshape(2, 4, -1).transpose(1, 0, 2).reshape(4, -1)
    y, mk = label.cpu().numpy().reshape(-1), mask.cpu().numpy().reshape(-1)
    ok, masked, bad = E.valid_pixels(lg, y, mk)
    ref, allowed = allowed_error(lg[:, ok], y[ok])
    assert (res["n"], res["n_masked"], res["n_nonfinite"]) == (int(ok.sum()), int(masked.sum()), 0)
    # a mean of per-pixel values, each within its soft-head bound of the reference: within the mean of those bounds
    for k, name in (("nll", "nll"), ("crps", "crps"), ("pit", "pit_mean")):
        err, bound = abs(res[name] - ref[k].mean()), allowed[k].mean() + 1e-12 * np.abs(ref[k]).mean()
        report(f"[score_evidential] update_from_evidential {name}: got {res[name]:.9e} ref {ref[k].mean():.9e} err {err:.2e} "
               f"bound {bound:.2e}")
        assert err <= bound, name
    # the same accumulator bits from the logits themselves
    direct = PredictiveScorer()
    direct.update_evidential(logits, label, mask)
    assert torch.equal(direct._ws[:72], sc._ws[:72])

    # anything but an evidential model is refused before a launch; a training-mode model too
    ens = EnsembleModule([], monte_carlo_steps=0, models=tiny_models(0.0), keep_on_device=True)
    called = []
    ens.forward_on_device = lambda x: called.append(1)
    fresh = PredictiveScorer()
    with pytest.raises(TypeError, match="EvidentialUnetModel"):
        fresh.update_from_evidential(ens, image, label)
    model.train()
    with pytest.raises(Exception, match="eval"):
        fresh.update_from_evidential(model, image, label)
    model.eval()
    with pytest.raises(ValueError):
        fresh.update_from_evidential(model, image, label[:, 0])
    assert not called and not bool(fresh._ws.any())


def test_evaluate_uncertainty_script_scores_the_evidential_model(tmp_path):
    out = str(tmp_path / "res")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_uncertainty.py"), "--evidential", "--synthetic", "1",
           "--batch", "2", "--size", "32", "--scores", "--result_dir", out]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    assert res["scores"]["n"] == 2 * 32 * 32 and np.isfinite(res["scores"]["nll"]) and res["scores"]["members"] == 1
    assert res["scores"]["crps"] > 0 and 0 <= res["scores"]["pit_mean"] <= 1
    for name in ("scores.csv", "calibration_mixture.csv"):
        assert os.path.exists(os.path.join(out, name)), name
