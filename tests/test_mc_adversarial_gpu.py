"""GPU tests of the FGSM sweep for MC-dropout ensembles: `fold_image_grad_mc_kernel` per operator, `mimo_input_gradient_mc`
through `mimo.adversarial.image_gradient(mc_dropout=True)` against fp64 autograd of the oracle, chunking, two members, the
production generator path, the sweep end to end and `RobustnessEvaluator(mc_dropout=True)`.

Reference semantics at stake: scripts/test/test_nyuv2_depth.py with --monte_carlo_steps M — the mean NLL over the
concatenated axis of all M * S_total outputs (each pass with its own dropout draw) back-propagated to the image.  The masks
are injected on both sides (`mask_override` / `elem_mask_override` here, `masks=` of the oracle), so the gradient GIVEN the
masks is compared; sample (pass m, image i) sits at row m * B + i.

Tolerances: the operator against its fp64 model to 1e-6 of the largest magnitude (an R-term fp32 sum: at most R + 1 adds
on top of the fold's own); whole gradients to TOL of tests/test_adversarial_cpu.py, the one the plain input gradient meets
in both precisions.

Small net throughout (S = 2, f = 4, 32 x 32, B = 2, M = 3): the pass stride (B = 2, R = 3), the pad channel (Ci = 3), a
non-square image and the accumulate path are what the kernel can get wrong, and all of them occur at these shapes."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import mimo_oracle as O
from tests import fgsm_reference as R
from tests import mc_fold_reference as MF
from tests.helpers import rel_err
from tests.test_adversarial_cpu import TOL

pytestmark = pytest.mark.gpu
PRECISIONS = ("fp32", "split16")
P_DROP = 0.2
B, M, HW = 2, 3, 32


# ------------------------------------------------------------------------------------------------ per operator
def _op(name, *args):
    from mimo_unet_amd import _lib as L
    L.check(getattr(L.load(), name)(*args, L.current_stream()), name)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("acc", [0, 1], ids=["assign", "accumulate"])
@pytest.mark.parametrize("hw", [(32, 32), (48, 32)], ids=["32x32", "48x32"])
@pytest.mark.parametrize("C", [2, 3])
def test_fold_image_grad_mc_against_the_fp64_model(C, hw, acc):
    (H, W), Rp, ldp = hw, 3, 4
    g = torch.Generator().manual_seed(7000 + 100 * C + H + acc)
    dxpad = torch.randn(Rp * B, H + 2, W + 2, ldp, generator=g)
    start = torch.randn(B, C, H, W, generator=g)
    want = MF.fold_mc(dxpad.numpy(), Rp, C, start.numpy() if acc else None)
    dimage = start.clone().cuda() if acc else torch.full((B, C, H, W), float("nan"), device="cuda")
    dd = dxpad.cuda()
    _op("mimo_op_fold_image_grad_mc", dd.data_ptr(), ldp, Rp * B, Rp, C, H, W, dimage.data_ptr(), acc)
    got = dimage.cpu().double().numpy()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"fold_image_grad_mc C {C} {H}x{W} acc {acc}: max |err| / max |ref| {err:.3e}")
    assert np.isfinite(got).all() and err <= 1e-6
    # the pass stride: pass-major rows, not image-major — the image-major reading of the same buffer is far off
    wrong = MF.fold(dxpad.numpy())[..., :C].reshape(B, Rp, H, W, C).sum(axis=1).transpose(0, 3, 1, 2)
    assert np.abs(wrong + (start.numpy() if acc else 0) - want).max() > 1e-2 * np.abs(want).max()


@pytest.mark.parametrize("acc", [0, 1], ids=["assign", "accumulate"])
def test_fold_image_grad_mc_with_one_pass_has_the_bits_of_fold_image_grad(acc):
    from mimo_unet_amd import _lib as L
    ldp, N = 4, 3
    for C, (H, W) in ((2, (32, 32)), (3, (48, 32)), (3, (5, 7))):
        g = torch.Generator().manual_seed(7100 + C + H)
        dxpad = torch.randn(N, H + 2, W + 2, ldp, generator=g)
        dxpad[0, 3, 3, :] = -0.0  # an interior pixel that must stay -0 when assigned
        start = torch.randn(N, C, H, W, generator=g)
        outs = []
        for name, extra in (("mimo_op_fold_image_grad", ()), ("mimo_op_fold_image_grad_mc", (1,))):
            dimage = start.clone().cuda() if acc else torch.full((N, C, H, W), float("nan"), device="cuda")
            _op(name, dxpad.cuda().data_ptr(), ldp, N, *extra, C, H, W, dimage.data_ptr(), acc)
            outs.append(dimage)
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), (C, H, W)
    st = L.current_stream()
    buf = torch.zeros(4 * 34 * 34 * 4, device="cuda")
    for replicas in (0, -1, 3):  # 3 does not divide n = 4
        assert L.load().mimo_op_fold_image_grad_mc(buf.data_ptr(), 4, 4, replicas, 3, 32, 32, buf.data_ptr(), 0, st) == -1


# ------------------------------------------------------------------------------------------------ whole gradient
def _state(cfg, seed):
    st = O.init_state(cfg, seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in st:  # running statistics a trained checkpoint would hold
        if k.endswith("running_mean"):
            st[k] = 0.1 * torch.randn(st[k].shape, generator=g)
        elif k.endswith("running_var"):
            st[k] = 0.5 + torch.rand(st[k].shape, generator=g)
    return st


def _draw(shape, g):
    return torch.bernoulli(torch.full(shape, 1.0 - P_DROP), generator=g) / (1.0 - P_DROP)


@functools.lru_cache(maxsize=None)
def _member_case(S, seed, elem, passes=M, ci=3, f=4):
    """(cfg, state, oracle masks for the passes x B stacked batch, mask_override, elem_mask_override) of one member."""
    ce = P_DROP if elem else 0.0
    cfg = O.NetConfig(ci, 2, S, f, P_DROP, P_DROP, P_DROP, ce, ce)
    st = _state(cfg, seed)
    g = torch.Generator().manual_seed(seed + 2)
    n = passes * B
    specs = O.double_conv_specs(cfg)
    omasks = {pref: _draw((n, cout), g) for pref, _, _, cout in specs}
    override = {j: omasks[pref] for j, (pref, _, _, _) in enumerate(specs)}
    elem_override = None
    if elem:
        omasks["core.center_dropout"] = _draw((n, 8 * f * S, HW // 16, HW // 16), g)
        elem_override = {"center": omasks["core.center_dropout"]}
        for s in range(S):
            omasks[f"decoder.final_dropouts.{s}"] = _draw((n, f, HW, HW), g)
            elem_override[f"final{s}"] = omasks[f"decoder.final_dropouts.{s}"]
    return cfg, st, omasks, override, elem_override


@functools.lru_cache(maxsize=None)
def _inputs(ci=3):
    g = torch.Generator().manual_seed(77)
    return torch.rand(B, ci, HW, HW, generator=g), torch.rand(B, 1, HW, HW, generator=g)


def _oracle_gradient(members, passes, kind="laplace_nll"):
    """fp64: d/d image of (1 / (M * S_total)) sum_member sum_m sum_s loss_{m,s}, the passes stacked on the batch axis
    (pass-major) with the recorded masks — a member's loss mean over [M * B, S, 1, H, W] is (1 / (M * S)) sum_m sum_s loss_{m,s}."""
    image, label = _inputs()
    img = image.double().requires_grad_(True)
    s_total = sum(c[0].num_subnetworks for c in members)
    total = 0.0
    for cfg, st, omasks, _, _ in members:
        S = cfg.num_subnetworks
        st64 = {k: (v.double() if v.is_floating_point() else v) for k, v in st.items()}
        x = O.repeat_subnetworks(img.repeat(passes, 1, 1, 1), S)
        out = O.mimo_unet_forward(cfg, st64, x, training=False, mc_dropout=True, masks={k: v.double() for k, v in omasks.items()})
        p1, p2 = O.split_heads(out, cfg.out_channels)
        labels = label.double().repeat(passes, 1, 1, 1)[:, None].repeat(1, S, 1, 1, 1)
        total = total + O.loss_forward(kind, p1, p2, labels) * (S / s_total)
    total.backward()
    return img.grad.detach()


@functools.lru_cache(maxsize=None)
def _oracle_case(elem):
    return _oracle_gradient([_member_case(2, 500, elem)], M)


def _model(case, precision):
    from mimo.models.mimo_unet import MimoUnetModel
    cfg, st, _, override, elem_override = case
    # (the constructor, like the reference's, refuses Dropout2d rates together with center / final rates: in the second case
    # the Dropout2d modules have rate 0 and their multipliers reach the engine through mask_override all the same)
    p2d = 0.0 if elem_override is not None else P_DROP
    m = MimoUnetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, num_subnetworks=cfg.num_subnetworks,
                      filter_base_count=cfg.filter_base_count, center_dropout_rate=cfg.center_dropout_rate,
                      final_dropout_rate=cfg.final_dropout_rate, encoder_dropout_rate=p2d,
                      core_dropout_rate=p2d, decoder_dropout_rate=p2d, loss="laplace_nll",
                      weight_decay=0.0, learning_rate=1e-3, seed=0, loss_buffer_size=10, loss_buffer_temperature=0.3)
    m.load_state_dict({"model." + k: v for k, v in st.items()})
    m.model.set_precision(precision)
    m = m.cuda()
    m.model.mask_override = override
    m.model.elem_mask_override = elem_override
    return m


def _ensemble(models, passes=M):
    from mimo.models.ensemble import EnsembleModule
    return EnsembleModule([], monte_carlo_steps=passes, models=list(models), keep_on_device=True)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("elem", [False, True], ids=["dropout2d", "dropout2d+center+final"])
def test_mc_image_gradient_against_fp64_autograd_of_the_oracle(elem, precision):
    from mimo.adversarial import image_gradient
    case = _member_case(2, 500, elem)
    want = _oracle_case(elem)
    ens = _ensemble([_model(case, precision)])
    image, label = (t.cuda() for t in _inputs())
    got = image_gradient(ens, image, label, mc_dropout=True)
    err = rel_err(got.cpu(), want)
    print(f"MC image gradient [{precision}] elem {elem}: err {err:.3e}, undecided share {R.undecided_share(want.numpy()):.4%}")
    assert got.shape == image.shape and torch.isfinite(got).all()
    assert err <= TOL
    net = ens.models[0].model
    assert net.mask_override is case[3] and net.elem_mask_override is case[4]  # restored
    assert net.numerics_status() == 0
    # every pass counts: the gradient of the first pass alone (what a wrong pass stride or weight would give) is far off
    one = _oracle_gradient([(case[0], case[1], {k: v[:B] for k, v in case[2].items()}, None, None)], 1)
    assert rel_err(one, want) > 20 * TOL


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunked_launches_agree_with_the_unchunked_run_and_repeat_bitwise(precision):
    from mimo.adversarial import image_gradient
    case = _member_case(2, 500, True)
    ens = _ensemble([_model(case, precision)])
    image, label = (t.cuda() for t in _inputs())
    whole = image_gradient(ens, image, label, mc_dropout=True)
    again = image_gradient(ens, image, label, mc_dropout=True)
    assert torch.equal(_bits(whole), _bits(again))
    ens.max_samples_per_launch = 4  # chunks of 2 + 1 passes of B = 2 images
    chunked = image_gradient(ens, image, label, mc_dropout=True)
    chunked_again = image_gradient(ens, image, label, mc_dropout=True)
    assert torch.equal(_bits(chunked), _bits(chunked_again))
    err, err_ref = rel_err(chunked.cpu(), whole.cpu()), rel_err(chunked.cpu(), _oracle_case(True))
    print(f"chunked (2 + 1 passes) vs unchunked [{precision}]: {err:.3e}; chunked vs oracle {err_ref:.3e}")
    assert err <= TOL and err_ref <= TOL
    net = ens.models[0].model
    assert sorted(k[0] for k in net._plans if k[-1] == "input-gradient") == [B, 2 * B, 3 * B]  # one plan per chunk size


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_members_with_two_passes_weigh_one_over_m_s_total(precision):
    from mimo.adversarial import image_gradient
    cases = [_member_case(2, 600, False, 2), _member_case(1, 610, True, 2)]
    want = _oracle_gradient(cases, 2)
    ens = _ensemble([_model(c, precision) for c in cases], passes=2)
    assert ens.num_subnetworks == 3
    image, label = (t.cuda() for t in _inputs())
    got = image_gradient(ens, image, label, mc_dropout=True)
    err = rel_err(got.cpu(), want)
    print(f"two members (S = 2, 1), M = 2 [{precision}]: err {err:.3e}")
    assert err <= TOL


def _snapshot(ens):
    out = []
    for m in ens.models:
        out.append(([p.grad for p in m.parameters()], m.model._flat_buffers.clone(), m.model.flat_parameters().clone(),
                    [mod.training for mod in m.modules()]))
    return out


def _assert_untouched(ens, before):
    for m, (grads, buffers, params, flags) in zip(ens.models, before):
        assert all(a is b for a, b in zip(grads, [p.grad for p in m.parameters()]))
        assert torch.equal(m.model._flat_buffers, buffers) and torch.equal(m.model.flat_parameters(), params)
        assert flags == [mod.training for mod in m.modules()]
        assert not m.model._bn_training() and any(d.training and d.p > 0 for d in m.model._dropout_modules())


@pytest.mark.parametrize("elem", [False, True], ids=["dropout2d", "center+final"])
def test_production_generator_path_draws_fresh_masks_and_replays_under_a_seed(elem):
    from mimo.adversarial import fgsm_sweep, image_gradient
    case = _member_case(2, 500, elem)
    model = _model(case, "split16")
    model.model.mask_override = model.model.elem_mask_override = None
    assert model.model.engine_rng
    ens = _ensemble([model])
    image, label = (t.cuda() for t in _inputs())
    image_gradient(ens, image, label, mc_dropout=True)  # (plans, flat buffers)
    before = _snapshot(ens)
    torch.cuda.manual_seed(1234)
    a = image_gradient(ens, image, label, mc_dropout=True)
    b = image_gradient(ens, image, label, mc_dropout=True)
    torch.cuda.manual_seed(1234)
    c = image_gradient(ens, image, label, mc_dropout=True)
    assert torch.isfinite(a).all() and not torch.equal(a, b)
    assert torch.equal(_bits(a), _bits(c))
    ens.max_samples_per_launch = 4  # every chunk takes its own counter block
    torch.cuda.manual_seed(1234)
    d = image_gradient(ens, image, label, mc_dropout=True)
    torch.cuda.manual_seed(1234)
    e = image_gradient(ens, image, label, mc_dropout=True)
    assert torch.equal(_bits(d), _bits(e)) and torch.isfinite(d).all()
    sweep = fgsm_sweep(ens, image, label, (0.0, 0.02), mc_dropout=True)
    assert all(torch.isfinite(t).all() for r in sweep.values() for t in r)
    _assert_untouched(ens, before)
    assert model.model.numerics_status() == 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mc_sweep_end_to_end_against_the_oracle_on_the_engines_own_perturbed_image(precision):
    """Recorded masks in every forward (gradient and predictions).  The engine's gradient decides the perturbed image: exact
    at every pixel the oracle's gradient decides.  The engine's OWN perturbed image then goes through the oracle, so the
    two networks are never compared on inputs that differ at undecided pixels."""
    from mimo.adversarial import fgsm_sweep
    case = _member_case(2, 500, False)
    cfg, st, omasks = case[0], case[1], case[2]
    want_grad = _oracle_case(False).float().numpy()
    ens = _ensemble([_model(case, precision)])
    image, label = _inputs()
    eps = [0.0, 0.02, 0.04]
    sweep = fgsm_sweep(ens, image.cuda(), label.cuda(), eps, return_perturbed=True, mc_dropout=True)
    assert list(sweep) == eps
    dec = R.decided(want_grad)
    pass_masks = [{k: v[m * B:(m + 1) * B] for k, v in omasks.items()} for m in range(M)]
    for e in eps:
        mean, av, ev, pert = sweep[e]
        pert_np = pert.cpu().numpy()
        diff = pert_np != R.fgsm_attack(image.numpy(), e, want_grad)
        print(f"MC sweep [{precision}] eps {e}: {int(diff.sum())} pixels differ from the oracle's attack, {int((~dec).sum())} undecided of {dec.size}")
        assert not (diff & dec).any()
        want = O.ensemble_forward(cfg, st, torch.from_numpy(pert_np), "laplace_nll", monte_carlo_steps=M, pass_masks=pass_masks)
        errs = {"mean": rel_err(mean.cpu(), want[0]), "aleatoric": rel_err(av.cpu(), want[1]), "epistemic": rel_err(ev.cpu(), want[2])}
        print("   ", errs)
        assert mean.shape == (B, 1, HW, HW) and all(v <= TOL for v in errs.values()), errs
    assert ens.models[0].model.numerics_status() == 0


def test_robustness_evaluator_with_mc_dropout_writes_the_same_file_names(tmp_path):
    from mimo.adversarial import RobustnessEvaluator
    model = _model(_member_case(2, 500, False), "split16")
    model.model.mask_override = None
    ens = _ensemble([model])
    image, label = (t.cuda() for t in _inputs())
    with pytest.raises(NotImplementedError, match="MC-dropout"):
        RobustnessEvaluator().update_from(ens, image, label)
    rob = RobustnessEvaluator(mc_dropout=True)
    rob.update_from(ens, image, label)
    tables = rob.compute()
    assert tables[0.0]["n"] == B * HW * HW
    rob.write_csv(str(tmp_path), "nyuv2", tables)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f"nyuv2_{e}_{k}.csv" for e in ("0.0", "0.02", "0.04") for k in ("precision_recall", "calibration")), names
