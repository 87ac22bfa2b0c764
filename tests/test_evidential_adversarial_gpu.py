"""GPU tests of the evidential model's evaluation path: the uncertainty kernel (`mimo_evidential_uncertainties`), the logit
gradient of the mean loss (`mimo_evidential_loss_gradient`), `EvidentialUnetModel.image_gradient` / `predict_uncertainties`
and the public sweep and evaluators on top, in the `split16` and `fp32` precisions.

Reference semantics at stake: `make_predictions` + `fgsm_attack` of scripts/test/test_nyuv2_depth_evidential.py:16-65 in eval
mode.  tests/golden/evidential_fgsm.npz holds the reference's own numbers (tests/golden/make_evidential_fgsm_golden.py).

Sign rule as in tests/test_adversarial_gpu.py: perturbed images are compared exactly at decided pixels (tests/fgsm_reference.py).

Bit-equality claim: the parent route — autograd through `EvidentialUnetModel` in eval mode, `.mean()` of the fused loss
back-propagated to `image.grad` — hands `mimo_backward` the `dout` that `mimo_evidential_backward` forms from a d_loss tensor
filled with fp32 1 / (B H W) (and a d_ev of zeros, which adds +0 to each term); `image_gradient` hands `mimo_input_gradient`
the `dout` of `mimo_evidential_loss_gradient`, the same device function with that value as a kernel argument.  Both then run
the same data-gradient kernels (tests/test_adversarial_gpu.py asserts that half)."""
import os

import numpy as np
import pytest
import torch

from tests import fgsm_reference as R
from tests.helpers import load_npz, rel_err
from tests.test_evidential_adversarial_cpu import CASES, TOL, case, oracle_uncertainties

pytestmark = pytest.mark.gpu
PRECISIONS = ("split16", "fp32")
HWS = (34 * 34, 33 * 35)  # a multiple of 4 (16-byte path), and not (scalar path)


def _model(c, precision, monkeypatch):
    from mimo.models.evidential_unet import EvidentialUnetModel
    monkeypatch.setenv("MIMO_PRECISION", precision)
    cfg = c["cfg"]
    m = EvidentialUnetModel(in_channels=cfg.in_channels, out_channels=4, filter_base_count=cfg.filter_base_count,
                            center_dropout_rate=0.0, final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
                            decoder_dropout_rate=0.0, weight_decay=0.0, learning_rate=1e-3, seed=0)
    m.load_state_dict({"model." + k: v for k, v in c["state"].items()}, strict=False)
    assert m.model._geom.precision == precision
    return m.cuda().eval()


def _planted_logits(hw, seed):
    """[2,4,hw]: random, plus l2 in {-30, -20, 0, 25} (softplus underflow: alpha - 1 == 0; the threshold at 20) and l1 = -100
    (v == 0), alone and together."""
    g = torch.Generator().manual_seed(seed)
    l = torch.randn(2, 4, hw, generator=g) * 2.0
    for k, v in enumerate((-30.0, -20.0, 0.0, 25.0)):
        l[0, 2, 3 + 5 * k] = v
        l[1, 2, hw - 1 - 7 * k] = v
    l[0, 1, 40], l[1, 1, hw - 2] = -100.0, -100.0
    l[0, 1, 50], l[0, 2, 50] = -100.0, -30.0  # 0 * 0 in the denominator
    l[1, 3, 60], l[1, 2, 60] = -200.0, -30.0  # beta == 0 over alpha - 1 == 0: NaN
    return l.cuda()


@pytest.mark.parametrize("hw", HWS)
def test_uncertainty_kernel_against_the_head_kernel_and_torch_ops(hw):
    from mimo_unet_amd.engine import evidential_head_loss, evidential_uncertainties
    from mimo_unet_amd.losses import EvidentialLoss
    logits = _planted_logits(hw, 7).view(2, 4, hw, 1)
    ev = evidential_head_loss(logits)[0]
    want = (EvidentialLoss.mode(ev), EvidentialLoss.aleatoric_var(ev), EvidentialLoss.epistemic_var(ev))
    got = evidential_uncertainties(logits)
    torch.cuda.synchronize()
    nonfinite = 0
    for name, g, w in zip(("mean", "aleatoric_var", "epistemic_var"), got, want):
        g, w = g[:, 0].cpu(), w.cpu()
        assert g.shape == w.shape == (2, hw, 1)
        fin = torch.isfinite(w)
        assert torch.equal(torch.isfinite(g), fin), name
        assert torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(g[~fin & ~torch.isnan(w)], w[~fin & ~torch.isnan(w)]), name
        rel = float(((g[fin] - w[fin]).abs() / w[fin].abs().clamp_min(1e-30)).max())
        print(f"hw {hw} {name}: max relative difference at finite pixels {rel:.3e}, {int((~fin).sum())} non-finite")
        assert rel <= 1e-6, name  # at most three correctly rounded fp32 operations on identical operands
        nonfinite += int((~fin).sum())
    assert torch.equal(got[0][:, 0], logits[:, 0])
    assert nonfinite >= 8 and torch.isnan(want[1]).any() and torch.isinf(want[1]).any()  # the planted values are there
    # unaligned pointers with hw % 4 == 0: the scalar path, same bits as the 16-byte path
    if hw % 4 == 0:
        flat = torch.empty(2 * 4 * hw + 1, device="cuda")
        shifted = flat[1:].view(2, 4, hw, 1)
        shifted.copy_(logits)
        assert shifted.data_ptr() % 16 != 0
        for a, b in zip(evidential_uncertainties(shifted), got):
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


@pytest.mark.parametrize("with_mask", (False, True), ids=("no-mask", "mask"))
@pytest.mark.parametrize("hw", HWS)
def test_loss_gradient_is_bit_identical_to_the_backward_with_a_filled_d_loss(hw, with_mask):
    from mimo_unet_amd import _lib as L
    from mimo_unet_amd.engine import evidential_loss_gradient
    lib = L.load()
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(2, 4, hw, 1, generator=g) * 1.5).cuda()
    label = torch.rand(2, 1, hw, 1, generator=g).cuda()
    mask = (torch.rand(2, hw, 1, generator=g) > 0.3).float().cuda() if with_mask else None
    scale = float(torch.tensor(1.0) / torch.tensor(float(2 * hw)))
    got = evidential_loss_gradient(logits, label, mask, scale)
    d_loss = torch.full((2, hw), scale, device="cuda")
    want = torch.full_like(logits, float("nan"))
    L.check(lib.mimo_evidential_backward(logits.data_ptr(), label.data_ptr(), L.ptr(mask) or None, None, d_loss.data_ptr(), 2, hw,
                                         want.data_ptr(), L.current_stream()), "mimo_evidential_backward")
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got, want), f"differs by up to {float((got - want).abs().max()):.3e}"
    if with_mask:
        assert (got[:, 0][mask == 0] == 0).all()


def _parent_route(model, image, label, mask=None):
    """What the parent commit offers: autograd through the module in eval mode, `.mean()` of the fused loss -> image.grad."""
    x = image.clone().requires_grad_(True)
    out, loss = model._forward_with_loss(x, label, mask)
    loss.mean().backward()
    return out.detach(), loss.detach().mean(), x.grad.detach()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", CASES)
def test_image_gradient_matches_fixture_and_equals_the_parent_route_bitwise(name, precision, monkeypatch):
    c = case(load_npz("evidential_fgsm.npz"), name)
    model = _model(c, precision, monkeypatch)
    net = model.model
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    net._plan_for(image, None)  # (the flat storage exists from here on)
    net._flat_grads.copy_(torch.arange(net._flat_grads.numel(), device="cuda", dtype=torch.float32).sin())
    grads_before, buffers_before = net._flat_grads.clone(), net._flat_buffers.clone()
    dimage, logits = model.image_gradient(image, label)
    errs = {"logits": rel_err(logits.cpu(), c["logits"]), "dimage": rel_err(dimage.cpu(), c["dimage"])}
    print(name, precision, errs)
    assert all(e <= TOL for e in errs.values()), errs
    assert all(p.grad is None for p in model.parameters())
    assert torch.equal(net._flat_grads, grads_before), "image_gradient wrote the flat gradient buffer"
    assert torch.equal(net._flat_buffers, buffers_before), "image_gradient wrote the BatchNorm buffers"
    assert not dimage.requires_grad and not logits.requires_grad
    # a caller's buffer, and the evaluators' [B,1,H,W] mask against the loss's [B,H,W]
    g = torch.Generator().manual_seed(5)
    mask = (torch.rand(image.shape[0], *image.shape[2:], generator=g) > 0.3).float().cuda()
    mine = torch.full_like(image, float("nan"))
    d3, _ = model.image_gradient(image, label, mask, dimage=mine)
    d4, _ = model.image_gradient(image, label, mask[:, None])
    assert d3 is mine and torch.equal(d3, d4) and not torch.equal(d3, dimage)
    # ---- the parent route on the same network: bit for bit (it writes .grad, so it comes last)
    ev_p, loss_p, dx = _parent_route(model, image, label)
    assert abs(float(loss_p) - float(c["loss"])) <= TOL * abs(float(c["loss"]))
    assert torch.equal(ev_p[:, 0], logits[:, 0])
    assert torch.equal(dimage, dx), f"differs from the autograd route by up to {float((dimage - dx).abs().max()):.3e}"
    _, _, dx_m = _parent_route(model, image, label, mask)
    assert torch.equal(d3, dx_m), f"masked: differs from the autograd route by up to {float((d3 - dx_m).abs().max()):.3e}"
    assert net.numerics_status() == 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", CASES)
def test_sweep_end_to_end_against_the_oracle_on_the_engines_own_perturbed_image(name, precision, monkeypatch):
    """The engine's gradient decides the perturbed image: exact at every decided pixel.  The engine's OWN perturbed image then
    goes through the CPU oracle, so the two networks are never compared on inputs that differ at undecided pixels."""
    from mimo.adversarial import fgsm_sweep
    fx = load_npz("evidential_fgsm.npz")
    c = case(fx, name)
    model = _model(c, precision, monkeypatch)
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    eps = [float(e) for e in fx["epsilons"]]
    sweep = fgsm_sweep(model, image, label, eps, return_perturbed=True)
    assert list(sweep) == eps
    dec = R.decided(c["dimage"])
    for k, e in enumerate(eps):
        mean, av, ev, pert = sweep[e]
        assert mean.shape == av.shape == ev.shape == label.shape and mean.is_cuda
        pert_np = pert.cpu().numpy()
        diff = pert_np != c["perturbed"][k]
        print(f"{name} {precision} eps {e}: {int(diff.sum())} pixels differ from the fixture, all of them undecided "
              f"({int((~dec).sum())} undecided of {dec.size})")
        assert not (diff & dec).any()
        want = oracle_uncertainties(c, pert_np)
        errs = {"mean": rel_err(mean[:, 0].cpu(), want[0]), "aleatoric": rel_err(av[:, 0].cpu(), want[1]),
                "epistemic": rel_err(ev[:, 0].cpu(), want[2])}
        print("   ", errs)
        assert all(v <= TOL for v in errs.values()), errs
    assert len(sweep[eps[0]]) == 4 and len(fgsm_sweep(model, image, label, eps[:1])[eps[0]]) == 3
    assert all(p.grad is None for p in model.parameters()) and not model.training
    assert model.model.numerics_status() == 0


def test_evaluators_take_the_bare_model(tmp_path, monkeypatch):
    from mimo.adversarial import RobustnessEvaluator, fgsm_sweep
    from mimo.evaluation import UncertaintyEvaluator
    c = case(load_npz("evidential_fgsm.npz"), "odd")
    model = _model(c, "split16", monkeypatch)
    g = torch.Generator().manual_seed(3)
    rob = RobustnessEvaluator()
    by_hand = {e: UncertaintyEvaluator() for e in rob.epsilons}
    plain, plain_by_hand = UncertaintyEvaluator(), UncertaintyEvaluator()
    for _ in range(2):
        image = (torch.rand(2, 2, 34, 34, generator=g) * 1.2 - 0.1).cuda()  # some pixels outside [0, 1]: eps = 0 still clamps
        label = torch.rand(2, 1, 34, 34, generator=g).cuda()
        mask = (torch.rand(2, 1, 34, 34, generator=g) > 0.2).float().cuda()
        rob.update_from(model, image, label, mask)
        for e, (mean, av, ev) in fgsm_sweep(model, image, label, rob.epsilons, mask=mask).items():
            by_hand[e].update(mean, av, ev, label, mask)
        plain.update_from(model, image, label)
        plain_by_hand.update(*model.predict_uncertainties(image), label)
    tables = rob.compute()

    def same(a, b):
        for key in ("precision_recall", "calibration"):
            for col, v in b[key].items():
                assert np.array_equal(a[key][col], v, equal_nan=True), (key, col)
        assert a["n"] == b["n"]

    for e in rob.epsilons:
        same(tables[e], by_hand[e].compute())
    same(plain.compute(), plain_by_hand.compute())
    assert plain.compute()["n"] == 2 * 2 * 34 * 34
    assert not np.array_equal(tables[0.04]["precision_recall"]["mae"], tables[0.0]["precision_recall"]["mae"])
    paths = rob.write_csv(str(tmp_path), "nyuv2", tables)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f"nyuv2_{e}_{k}.csv" for e in ("0.0", "0.02", "0.04") for k in ("precision_recall", "calibration")), names
    assert open(paths[0.02][0]).readline().strip() == "percentile,mae,rmse"
    assert open(paths[0.02][1]).readline().strip() == "Expected Conf.,Observed Conf."


def test_an_ensemble_with_an_evidential_member_still_raises(monkeypatch):
    from mimo.adversarial import fgsm_sweep
    from mimo.models.ensemble import EnsembleModule
    c = case(load_npz("evidential_fgsm.npz"), "even")
    model = _model(c, "split16", monkeypatch)
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    with pytest.raises(NotImplementedError, match="evidential"):
        fgsm_sweep(EnsembleModule([], models=[model], keep_on_device=True), image, label, (0.0,))
    with pytest.raises(NotImplementedError, match="eval mode"):
        fgsm_sweep(model.train(), image, label, (0.0,))
