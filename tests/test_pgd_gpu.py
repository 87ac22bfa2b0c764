"""GPU tests of the PGD kernels (`mimo_pgd_step`, `mimo_pgd_init`: csrc/pgd.hip) and of `mimo.adversarial.pgd_sweep` /
`RobustnessEvaluator(attack="pgd")` on top, in the `split16` and `fp32` precisions.

No reference counterpart (the reference's only attack is the single step of scripts/test/test_nyuv2_depth.py:16-24), so the
yardsticks are definitions: the numpy restatement of the two kernels and the plain loop with the sweep's chunk rule
(tests/pgd_reference.py), driven by `mimo.adversarial.image_gradient` on the very stacked batches the sweep forms, and
`fgsm_sweep` for the one-step case.  Everything is compared bit for bit: no tolerance.  (Where a NaN is expected its
position is compared, not its payload.)  The trajectory of a multi-step attack is deliberately not compared with an fp64
oracle: one sign flip at an undecided pixel compounds, and the gradient itself is held to the oracle by
tests/test_adversarial_gpu.py, tests/test_mc_adversarial_gpu.py and tests/test_evidential_adversarial_gpu.py.

Sizes: 4 k (16-byte path), 4 k + 3 and a view one float into its buffer (scalar path), just above 2048 * 256 * 4 (the
grid-stride loop wraps once), K = 17 (past the 16 sizes one launch takes)."""
import os

import numpy as np
import pytest
import torch

from oracle import mimo_oracle as O
from tests import pgd_reference as G
from tests.helpers import load_npz
from tests.test_adversarial_cpu import CASES, case
from tests.test_adversarial_gpu import _ensemble, _model

pytestmark = pytest.mark.gpu
PRECISIONS = ("split16", "fp32")
INF = float("inf")
#            elems, floats into the buffer, K
SIZES = {"vector": (4 * 1031, 0, 3), "scalar-odd": (4 * 1031 + 3, 0, 3), "scalar-misaligned": (4 * 1031, 1, 3),
         "wrap": (2048 * 256 * 4 + 4 * 77, 0, 1), "k17": (4 * 259, 0, 17)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """bit for bit; a NaN by position"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _dev(a, shift):
    """a on the device, `shift` floats into its buffer (shift = 1: no pointer is 16-byte aligned)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + shift, device="cuda", dtype=torch.float32)
    view = buf[shift:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * shift) % 16
    return view


def _eps(k):
    if k == 1:
        return [0.03]
    return [0.0, 0.02, 0.04][:k] if k <= 3 else [0.0] + [0.005 * j for j in range(1, k)]


def _step_data(elems, k, seed):
    g = np.random.default_rng(seed)
    x0 = g.uniform(-0.1, 1.1, elems).astype(np.float32)
    x0[:4] = [0.0, 1.0, 0.5, np.nan]  # a NaN pixel
    grads = g.standard_normal((3, k, elems)).astype(np.float32)
    grads[:, :, 4:8] = [0.0, -0.0, np.nan, 1e-38]  # +-0, a NaN gradient, a denormal
    return x0, grads


@pytest.mark.parametrize("clip", [(0.1, 0.9), None], ids=["clip", "noclip"])
@pytest.mark.parametrize("size", list(SIZES))
def test_pgd_step_three_in_place_steps_equal_the_restatement(size, clip):
    from mimo_unet_amd.engine import pgd_step
    elems, shift, k = SIZES[size]
    lo, hi = (-INF, INF) if clip is None else clip
    eps = _eps(k)
    alpha = [2.5 * e / 3 if e > 0 else 0.3 for e in eps]  # (eps = 0 with a step: the ball still holds it at x0)
    x0, grads = _step_data(elems, k, 100 + elems % 97 + k)
    start = want = np.stack([G.clamp(x0, lo, hi)] * k)
    x0_d, xa_d = _dev(x0, shift), _dev(want, shift)
    for t in range(3):
        want = G.pgd_step(x0, grads[t], want, eps, alpha, lo, hi)
        ret = pgd_step(x0_d, _dev(grads[t], shift), xa_d, eps, alpha, lo, hi)
        assert ret is xa_d
        got = xa_d.cpu().numpy()
        assert _same(got, want), (size, t)
    assert np.isnan(got[:, 3]).all() and np.isnan(got[:, 6]).all() and not np.isnan(np.delete(got, [3, 6], axis=1)).any()
    if eps[0] == 0.0:  # clamp(x0) but for the NaN gradient
        assert _same(got[0], G.clamp(np.where(np.arange(elems) == 6, np.nan, x0), lo, hi))
    assert (got[-1] != start[-1])[8:].mean() > 0.4  # the attack moved (pixels far outside the clip range cannot)
    assert _same(x0_d.cpu().numpy(), x0)


def test_pgd_kernels_refuse_bad_arguments():
    from mimo_unet_amd import _lib as L
    from mimo_unet_amd.engine import pgd_init, pgd_step
    x0 = torch.rand(64, device="cuda")
    g, xa = torch.randn(1, 64, device="cuda"), x0[None].clone()
    before = xa.clone()
    for eps, alpha, lo, hi in (([-0.01], [0.01], 0.0, 1.0), ([float("nan")], [0.01], 0.0, 1.0), ([0.01], [-0.01], 0.0, 1.0),
                               ([0.01], [float("nan")], 0.0, 1.0), ([0.01], [0.01], 1.0, 0.0)):
        with pytest.raises(L.MimoHipError, match=r"status -1"):  # MIMO_ERR_INVALID
            pgd_step(x0, g, xa, eps, alpha, lo, hi)
    for eps, lo, hi in (([-0.01], 0.0, 1.0), ([float("nan")], 0.0, 1.0), ([0.01], 1.0, 0.0)):
        with pytest.raises(L.MimoHipError, match=r"status -1"):
            pgd_init(x0, eps, lo, hi, 1, 0)
    assert torch.equal(xa, before)
    lib, st = L.load(), L.current_stream()
    e = (L.C.c_float * 1)(0.01)
    assert lib.mimo_pgd_step(None, g.data_ptr(), xa.data_ptr(), 64, e, e, 1, 0.0, 1.0, st) == -1
    assert lib.mimo_pgd_step(x0.data_ptr(), g.data_ptr(), xa.data_ptr(), 0, e, e, 1, 0.0, 1.0, st) == -1
    assert lib.mimo_pgd_init(x0.data_ptr(), 64, e, 0, 0.0, 1.0, 1, 0, xa.data_ptr(), st) == -1


@pytest.mark.parametrize("clip", [(0.0, 1.0), None], ids=["clip", "noclip"])
@pytest.mark.parametrize("size", list(SIZES))
def test_pgd_init_equals_the_restatement(size, clip):
    from mimo_unet_amd.engine import pgd_init
    elems, shift, k = SIZES[size]
    lo, hi = (-INF, INF) if clip is None else clip
    eps = _eps(k)
    seed, offset = 0x9E3779B97F4A7C15, (7 << 32) + 0xFFFFFF00 + 4 * (elems % 5)  # both words of seed and offset in use
    x0 = np.random.default_rng(200 + elems % 89).uniform(-0.1, 1.1, elems).astype(np.float32)
    x0[3] = np.nan
    x0_d = _dev(x0, shift)
    got_d = pgd_init(x0_d, eps, lo, hi, seed, offset)
    got = got_d.cpu().numpy()
    assert _same(got, G.pgd_init(x0, eps, lo, hi, seed, offset)), size
    assert torch.equal(pgd_init(x0_d, eps, lo, hi, seed, offset).view(torch.int32), got_d.view(torch.int32))  # the same draw again
    later = pgd_init(x0_d, eps, lo, hi, seed, offset + 4).cpu().numpy()
    assert (later[-1] != got[-1]).mean() > 0.7 and _same(later, G.pgd_init(x0, eps, lo, hi, seed, offset + 4))
    if eps[0] == 0.0:
        assert _same(got[0], G.clamp(x0, lo, hi))


def test_pgd_init_scalar_and_vector_paths_give_an_element_the_same_value():
    from mimo_unet_amd.engine import pgd_init
    x0 = np.random.default_rng(9).uniform(0, 1, 4 * 300).astype(np.float32)
    whole = pgd_init(_dev(x0, 0), [0.04], 0.0, 1.0, 5, 8).cpu().numpy()
    for elems, shift in ((4 * 300 - 1, 0), (4 * 300 - 3, 0), (4 * 300, 1)):
        part = pgd_init(_dev(x0[:elems], shift), [0.04], 0.0, 1.0, 5, 8).cpu().numpy()
        assert _same(part, whole[:, :elems]), (elems, shift)


# ------------------------------------------------------------------------------------------------ the sweep
def _gradient_fn(ens, label, mask=None, **kw):
    """gradient_fn of `reference_sweep`: `image_gradient` on the stacked batch, label and mask repeated per level"""
    from mimo.adversarial import image_gradient

    def fn(stacked, levels):
        rep = lambda t: None if t is None else t.repeat(levels, *([1] * (t.dim() - 1)))  # noqa: E731
        return image_gradient(ens, torch.from_numpy(stacked).cuda(), rep(label), rep(mask), **kw).cpu().numpy()
    return fn


def _snapshot(ens):
    return [([p.grad for p in m.parameters()], m.model._flat_buffers.clone(), m.model.flat_parameters().clone(),
             [mod.training for mod in m.modules()]) for m in ens.models]


def _assert_untouched(ens, before):
    for m, (grads, buffers, params, flags) in zip(ens.models, before):
        assert all(a is b for a, b in zip(grads, [p.grad for p in m.parameters()]))
        assert torch.equal(m.model._flat_buffers, buffers) and torch.equal(m.model.flat_parameters(), params)
        assert flags == [mod.training for mod in m.modules()]


def _assert_predictions(ens, res):
    """the tuple of a level: the ordinary forward of its perturbed image"""
    want = ens.predict_uncertainties(res[3]) if not hasattr(ens, "models") else tuple(ens(res[3]))
    assert len(res) == 4 and all(torch.equal(a, b) for a, b in zip(res[:3], want))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", CASES)
def test_one_step_of_size_eps_is_fgsm_sweep_bit_for_bit(name, precision, monkeypatch):
    from mimo.adversarial import fgsm_sweep, pgd_sweep
    c = case(load_npz("fgsm.npz"), name)
    ens = _ensemble([_model(c["cfg"], c["state"], c["kind"], precision, monkeypatch)])
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    for eps in (0.02, 0.04, 0.0):
        want = fgsm_sweep(ens, image, label, (eps,), return_perturbed=True)
        got = pgd_sweep(ens, image, label, epsilons=(eps,), steps=1, step_size=eps, return_perturbed=True)
        assert list(got) == [eps] and len(got[eps]) == 4
        for a, b, what in zip(got[eps], want[eps], ("mean", "aleatoric", "epistemic", "perturbed")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (eps, what)
        assert len(pgd_sweep(ens, image, label, epsilons=(eps,), steps=1, step_size=eps)[eps]) == 3
    assert ens.models[0].model.numerics_status() == 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", CASES)
def test_four_step_sweep_equals_the_reference_loop_in_one_and_in_two_chunks(name, precision, monkeypatch):
    from mimo.adversarial import pgd_sweep
    c = case(load_npz("fgsm.npz"), name)
    ens = _ensemble([_model(c["cfg"], c["state"], c["kind"], precision, monkeypatch)])
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    b = image.shape[0]
    eps = (0.0, 0.02, 0.04)
    pgd_sweep(ens, image, label, eps, steps=1)  # (plans, flat buffers)
    before = _snapshot(ens)
    for limit, calls_per_step in ((64, 1), (b, 2)):  # 64 // 3 = 21 levels per launch: one chunk; 3 // 3 = 1: two
        ens.max_samples_per_launch = limit
        assert len(G.level_chunks(2, b, limit)) == calls_per_step
        got = pgd_sweep(ens, image, label, eps, steps=4, return_perturbed=True)
        want = G.reference_sweep(_gradient_fn(ens, label), c["image"], eps, steps=4, limit=limit)
        assert list(got) == list(eps)
        for e in eps:
            pert = got[e][3].cpu().numpy()
            assert _same(pert, want[e]), (limit, e)
            _assert_predictions(ens, got[e])
            # the ball and the range
            assert pert.min() >= 0.0 and pert.max() <= 1.0
            assert (pert >= c["image"] - np.float32(e)).all() and (pert <= c["image"] + np.float32(e)).all()
        assert _same(got[0.0][3].cpu().numpy(), c["image"])  # (the fixture's image lies in [0, 1])
        moved = (got[0.04][3].cpu().numpy() - c["image"])
        assert np.abs(moved).max() > 0.03  # more than one step of 2.5 * 0.04 / 4 = 0.025: the iteration ran
    _assert_untouched(ens, before)
    assert not ens.models[0].training and ens.keep_on_device and not ens.return_raw_predictions
    assert ens.models[0].model.numerics_status() == 0


def test_levels_in_any_order_with_a_mask_and_without_clip(monkeypatch):
    """eps = 0 between two attacked levels, a loss mask, clip=None: the dict keeps the order given, the stacked levels theirs."""
    from mimo.adversarial import pgd_sweep
    c = case(load_npz("fgsm.npz"), "laplace")
    ens = _ensemble([_model(c["cfg"], c["state"], c["kind"], "split16", monkeypatch)])
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    mask = (torch.rand(label.shape, generator=torch.Generator().manual_seed(4)) > 0.3).float().cuda()
    eps = (0.04, 0.0, 0.01)
    got = pgd_sweep(ens, image, label, eps, steps=2, step_size=0.03, mask=mask, clip=None, return_perturbed=True)
    want = G.reference_sweep(_gradient_fn(ens, label, mask), c["image"], eps, steps=2, limit=64, step_size=0.03, lo=-INF, hi=INF)
    assert list(got) == list(eps)
    for e in eps:
        assert _same(got[e][3].cpu().numpy(), want[e]), e
    assert got[0.04][3].max() > 1.0  # nothing clipped


def _generator_state(device):
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    return gen.initial_seed(), gen.get_offset()


def test_random_start_advances_the_generator_by_one_block_and_replays_under_a_seed(monkeypatch):
    from mimo.adversarial import pgd_sweep
    c = case(load_npz("fgsm.npz"), "gaussian")
    ens = _ensemble([_model(c["cfg"], c["state"], c["kind"], "split16", monkeypatch)])
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    eps = (0.0, 0.02, 0.04)
    torch.cuda.manual_seed(4321)
    seed, offset = _generator_state(image.device)
    assert seed == 4321
    a = pgd_sweep(ens, image, label, eps, steps=2, random_start=True, return_perturbed=True)
    assert _generator_state(image.device) == (seed, offset + 4)
    b = pgd_sweep(ens, image, label, eps, steps=2, random_start=True, return_perturbed=True)
    assert _generator_state(image.device) == (seed, offset + 8)
    pgd_sweep(ens, image, label, eps, steps=2)  # no random start: the generator stays
    assert _generator_state(image.device) == (seed, offset + 8)
    torch.cuda.manual_seed(4321)
    r = pgd_sweep(ens, image, label, eps, steps=2, random_start=True, return_perturbed=True)
    for e in eps:
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[e], r[e])), e
    assert not torch.equal(a[0.04][3], b[0.04][3])
    # the start is `pgd_init`'s of that (seed, offset), the rest the plain loop
    start = G.pgd_init(c["image"], eps, 0.0, 1.0, seed, offset)
    want = G.reference_sweep(_gradient_fn(ens, label), c["image"], eps, steps=2, limit=64, start=start)
    for e in eps:
        assert _same(a[e][3].cpu().numpy(), want[e]), e
    assert _same(a[0.0][3].cpu().numpy(), c["image"])


# ------------------------------------------------------------------------------------------------ model kinds
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_member_deep_ensemble(precision, monkeypatch):
    from mimo.adversarial import pgd_sweep
    c = case(load_npz("fgsm.npz"), "laplace")
    cfg_b = O.NetConfig(2, 2, 3, 4)
    ens = _ensemble([_model(c["cfg"], c["state"], "laplace_nll", precision, monkeypatch),
                     _model(cfg_b, O.init_state(cfg_b, 17), "laplace_nll", precision, monkeypatch)])
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    eps = (0.0, 0.02, 0.04)
    got = pgd_sweep(ens, image, label, eps, steps=2, return_perturbed=True)
    want = G.reference_sweep(_gradient_fn(ens, label), c["image"], eps, steps=2, limit=64)
    for e in eps:
        assert _same(got[e][3].cpu().numpy(), want[e]), e
        _assert_predictions(ens, got[e])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mc_dropout_ensemble_with_recorded_masks(precision):
    """Recorded masks (as tests/test_mc_adversarial_gpu.py injects them) in every forward, so the sweep is deterministic: one
    level per gradient call, each over the M masked passes."""
    from mimo.adversarial import pgd_sweep
    from tests import test_mc_adversarial_gpu as MC
    ens = MC._ensemble([MC._model(MC._member_case(2, 500, False), precision)])
    image, label = MC._inputs()
    eps = (0.0, 0.02, 0.04)
    with pytest.raises(NotImplementedError, match="MC-dropout"):
        pgd_sweep(ens, image.cuda(), label.cuda(), eps, steps=2)
    got = pgd_sweep(ens, image.cuda(), label.cuda(), eps, steps=2, return_perturbed=True, mc_dropout=True)
    want = G.reference_sweep(_gradient_fn(ens, label.cuda(), mc_dropout=True), image.numpy(), eps, steps=2, limit=64, mc_dropout=True)
    for e in eps:
        assert _same(got[e][3].cpu().numpy(), want[e]), e
        _assert_predictions(ens, got[e])
    assert got[0.0][0].shape == (MC.B, 1, MC.HW, MC.HW)
    assert (got[0.04][3] != got[0.0][3]).float().mean() > 0.5
    assert ens.models[0].model.numerics_status() == 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bare_evidential_model(precision, monkeypatch):
    from mimo.adversarial import pgd_sweep
    from tests import test_evidential_adversarial_gpu as EV
    from tests.test_evidential_adversarial_cpu import case as ev_case
    c = ev_case(load_npz("evidential_fgsm.npz"), "odd")
    model = EV._model(c, precision, monkeypatch)
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    b = image.shape[0]
    eps = (0.0, 0.02, 0.04)
    for limit in (None, str(b)):  # MIMO_MC_CHUNK_SAMPLES: the default of 64 (one chunk), then B (one level per chunk)
        if limit is not None:
            monkeypatch.setenv("MIMO_MC_CHUNK_SAMPLES", limit)
        got = pgd_sweep(model, image, label, eps, steps=2, return_perturbed=True)
        want = G.reference_sweep(_gradient_fn(model, label), c["image"], eps, steps=2, limit=int(limit or 64))
        for e in eps:
            assert _same(got[e][3].cpu().numpy(), want[e]), (limit, e)
            _assert_predictions(model, got[e])
    assert all(p.grad is None for p in model.parameters()) and not model.training


# ------------------------------------------------------------------------------------------------ the evaluator
def _read(paths):
    return [open(p, "rb").read() for pair in paths.values() for p in pair]


def test_evaluator_pgd_with_one_step_of_size_eps_writes_the_csvs_of_fgsm(tmp_path, monkeypatch):
    from mimo.adversarial import RobustnessEvaluator
    c = case(load_npz("fgsm.npz"), "laplace")
    ens = _ensemble([_model(c["cfg"], c["state"], c["kind"], "split16", monkeypatch)])
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    eps = 0.02
    fgsm = RobustnessEvaluator((eps,), attack="fgsm")
    pgd = RobustnessEvaluator((eps,), attack="pgd", steps=1, step_size=eps)
    assert (pgd.attack, pgd.steps, pgd.step_size, pgd.rel_step_size, pgd.random_start) == ("pgd", 1, eps, 2.5, False)
    many = RobustnessEvaluator((eps,), attack="pgd", steps=4)
    for rob in (fgsm, pgd, many):
        rob.update_from(ens, image, label)
    a, b = fgsm.write_csv(str(tmp_path / "fgsm"), "nyuv2"), pgd.write_csv(str(tmp_path / "pgd"), "nyuv2")
    assert sorted(os.listdir(tmp_path / "pgd")) == sorted(os.listdir(tmp_path / "fgsm")) == ["nyuv2_0.02_calibration.csv",
                                                                                             "nyuv2_0.02_precision_recall.csv"]
    assert _read(a) == _read(b)
    assert _read(many.write_csv(str(tmp_path / "many"), "nyuv2")) != _read(a)  # four steps are another attack


def test_evaluator_defaults_are_the_fgsm_tables(monkeypatch):
    from mimo.adversarial import RobustnessEvaluator, fgsm_sweep
    from mimo.evaluation import UncertaintyEvaluator
    c = case(load_npz("fgsm.npz"), "laplace")
    ens = _ensemble([_model(c["cfg"], c["state"], c["kind"], "split16", monkeypatch)])
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    rob = RobustnessEvaluator()
    assert (rob.attack, rob.epsilons, rob.mc_dropout) == ("fgsm", (0.0, 0.02, 0.04), False)
    rob.update_from(ens, image, label)
    tables = rob.compute()
    sweep = fgsm_sweep(ens, image, label, rob.epsilons)
    for e, (mean, av, ev) in sweep.items():
        plain = UncertaintyEvaluator()
        plain.update(mean, av, ev, label, None)
        want = plain.compute()
        for key in ("precision_recall", "calibration"):
            for col, v in want[key].items():
                assert np.array_equal(tables[e][key][col], v, equal_nan=True), (e, key, col)
        assert tables[e]["n"] == want["n"]
