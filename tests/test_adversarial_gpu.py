"""GPU tests of the input-gradient-only backward (`mimo_input_gradient`), the attack kernel (`mimo_fgsm_perturb`) and the
public sweep on top (`mimo.adversarial`), in the `split16` and `fp32` precisions.

Reference semantics at stake: `make_predictions` + `fgsm_attack` of scripts/test/test_nyuv2_depth.py:16-90 in eval mode — the
NLL of the ensemble back-propagated to the image, `clamp(image + eps * sign(grad), 0, 1)`, the prediction on the perturbed
image.  tests/golden/fgsm.npz holds the reference's own numbers (tests/golden/make_fgsm_golden.py).

Sign rule: `sign` is discontinuous, so a pixel counts as DECIDED when |g_ref| >= 1e-3 max|g_ref| (tests/fgsm_reference.py): a
gradient within the project's tolerance TOL = 1e-3 of the reference cannot flip such a pixel.  Perturbed images are compared
exactly at decided pixels; mismatches at undecided pixels are counted and printed, never failed.

Bit-equality claim: `mimo_input_gradient` launches the very per-element kernels `mimo_backward` launches for an eval-mode
forward (bn_bwd_apply with c1 = c2 = 0, the same data-gradient launches, the same GS_HEAD / GS_POOL gradient sources), so its
image gradient equals `mimo_backward`'s dx summed over the subnetworks in the documented order s = S-1 ... 0 bit for bit; no
fusion groups terms differently on this branch, and the 1e-4-of-scale fallback the fusions' section of DESIGN.md would allow
is not used."""
import os

import numpy as np
import pytest
import torch

from oracle import mimo_oracle as O
from tests import fgsm_reference as R
from tests.helpers import load_npz, rel_err
from tests.test_adversarial_cpu import CASES, TOL, case, oracle_gradient

pytestmark = pytest.mark.gpu
PRECISIONS = ("split16", "fp32")


def _model(cfg, state, kind, precision, monkeypatch):
    from mimo.models.mimo_unet import MimoUnetModel
    monkeypatch.setenv("MIMO_PRECISION", precision)
    m = MimoUnetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, num_subnetworks=cfg.num_subnetworks,
                      filter_base_count=cfg.filter_base_count, center_dropout_rate=0.0, final_dropout_rate=0.0,
                      encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, loss=kind, weight_decay=0.0,
                      learning_rate=1e-3, seed=0, loss_buffer_size=10, loss_buffer_temperature=0.3)
    m.load_state_dict({"model." + k: v for k, v in state.items()}, strict=False)
    assert m.model._geom.precision == precision
    return m.cuda().eval()


def _ensemble(models):
    from mimo.models.ensemble import EnsembleModule
    return EnsembleModule([], models=list(models), keep_on_device=True)


def _parent_route(model, image, label, dloss):
    """What the parent commit offers: autograd through the module on [B,S,C,H,W] -> mimo_backward's dx [B,S,C,H,W]."""
    S = model.num_subnetworks
    x5 = image[:, None].repeat(1, S, 1, 1, 1).requires_grad_(True)
    out, loss = model.model.forward_with_loss(x5, label, None, None)
    (loss * dloss).sum().backward()
    return out.detach(), x5.grad.detach()


def _sum_in_engine_order(dx, start=None):
    acc = start
    for s in range(dx.shape[1] - 1, -1, -1):
        acc = dx[:, s].clone() if acc is None else acc + dx[:, s]
    return acc


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", CASES)
def test_image_gradient_matches_fixture_and_equals_the_parent_route_bitwise(name, precision, monkeypatch):
    c = case(load_npz("fgsm.npz"), name)
    model = _model(c["cfg"], c["state"], c["kind"], precision, monkeypatch)
    net, S = model.model, c["cfg"].num_subnetworks
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    dloss = torch.full((S,), 1.0 / S, device="cuda")
    flat_before = None
    dimage = torch.full_like(image, float("nan"))
    with torch.no_grad():
        out, loss = net.image_gradient(image, label, None, dloss, dimage)
    errs = {"logits": rel_err(out.cpu(), c["logits"]), "dimage": rel_err(dimage.cpu(), c["dimage"]),
            "loss": abs(float(loss.mean()) - float(c["loss"])) / abs(float(c["loss"]))}
    print(name, precision, errs)
    assert all(e <= TOL for e in errs.values()), errs
    # ---- the parent route on the same network: bit for bit
    out_p, dx = _parent_route(model, image, label, dloss)
    assert torch.equal(out_p, out)
    errs["dx_sub"] = rel_err(dx.cpu(), c["dx_sub"])
    assert errs["dx_sub"] <= TOL, errs
    want = _sum_in_engine_order(dx)
    assert torch.equal(dimage, want), f"differs from mimo_backward's dx by up to {float((dimage - want).abs().max()):.3e}"
    # ---- accumulate: the same terms in the same order on top of what is there
    start = torch.from_numpy(c["dimage"]).cuda() * 3.0
    acc = start.clone()
    with torch.no_grad():
        net.image_gradient(image, label, None, dloss, acc, accumulate=True)
    assert torch.equal(acc, _sum_in_engine_order(dx, start))
    # ---- plan flavours: the input-gradient-only plan against the full plan
    n, h, w = image.shape[0], image.shape[2], image.shape[3]
    ig_plan = net._plans[(n, h, w, image.device.index, "input-gradient")]
    full = net._plans[(n, h, w, image.device.index, False)]
    assert ig_plan.input_gradient_only and not full.input_gradient_only
    print(f"workspace bytes: full {full.workspace_bytes}, input-gradient-only {ig_plan.workspace_bytes}")
    assert ig_plan.workspace_bytes < full.workspace_bytes
    from mimo_unet_amd._lib import MimoHipError
    with pytest.raises(MimoHipError, match=r"status -3"):  # MIMO_ERR_STATE
        ig_plan.backward(None, dloss, None)
    with pytest.raises(MimoHipError, match=r"status -3"):
        ig_plan.backward(None, dloss, None, stage=0)
    # mimo_input_gradient on the FULL plan, with its gradient buffer bound: same bits, buffer untouched
    grads = net._flat_grads
    grads.copy_(torch.arange(grads.numel(), device="cuda", dtype=torch.float32).sin())
    flat_before = grads.clone()
    out_f, loss_f, dimage_f = torch.empty_like(out), torch.empty_like(loss), torch.full_like(image, float("nan"))
    full.bind(net._flat_params, grads, net._flat_buffers)
    full.forward(image, out_f, training=False, broadcast_subnetworks=True, param_version=net._param_version())
    full.loss_forward(label, None, None, loss_f)
    full.input_gradient(None, dloss, dimage_f)
    assert torch.equal(out_f, out) and torch.equal(dimage_f, dimage)
    assert torch.equal(grads, flat_before)
    # ... and after a forward it is not valid for, it refuses
    full.forward(image, out_f, training=False, broadcast_subnetworks=True, no_grad=True, param_version=net._param_version())
    with pytest.raises(MimoHipError, match=r"status -3"):
        full.input_gradient(None, dloss, dimage_f)
    assert net.numerics_status() == 0


@pytest.mark.parametrize("name", CASES)
def test_fgsm_perturb_equals_the_fixture_exactly(name):
    from mimo_unet_amd.engine import fgsm_perturb
    fx = load_npz("fgsm.npz")
    c = case(fx, name)
    image, grad = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["dimage"]).cuda()
    got = fgsm_perturb(image, grad, list(fx["epsilons"]), 0.0, 1.0).cpu().numpy()  # all three eps in ONE call
    assert got.shape == c["perturbed"].shape and np.array_equal(got, c["perturbed"])
    # the scalar path (element count not a multiple of 4 / unaligned pointers), more eps than one launch takes, other clip range,
    # zero and NaN gradients
    flat_i, flat_g = image.flatten()[1:-2].clone(), grad.flatten()[1:-2].clone()
    flat_g[5], flat_g[6], flat_g[7] = 0.0, -0.0, float("nan")
    eps = [0.01 * k for k in range(19)]
    for img_t, g_t in ((flat_i, flat_g), (image.flatten()[1:-2], grad.flatten()[1:-2]), (image.flatten()[:4096].clone(), flat_g[:4096].clone())):
        got = fgsm_perturb(img_t, g_t, eps, 0.1, 0.9).cpu().numpy()
        for k, e in enumerate(eps):
            want = R.fgsm_attack(img_t.cpu().numpy(), e, g_t.cpu().numpy(), 0.1, 0.9)
            assert np.array_equal(got[k], want, equal_nan=True), (k, e)
    assert np.isnan(got[3][7]) and got[3][5] == got[0][5]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", CASES)
def test_sweep_end_to_end_against_the_oracle_on_the_engines_own_perturbed_image(name, precision, monkeypatch):
    """The engine's gradient decides the perturbed image: exact at every decided pixel.  The engine's OWN perturbed image then
    goes through the CPU oracle, so the two networks are never compared on inputs that differ at undecided pixels."""
    from mimo.adversarial import fgsm_sweep
    fx = load_npz("fgsm.npz")
    c = case(fx, name)
    model = _model(c["cfg"], c["state"], c["kind"], precision, monkeypatch)
    ens = _ensemble([model])
    image, label = torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["label"]).cuda()
    eps = [float(e) for e in fx["epsilons"]]
    sweep = fgsm_sweep(ens, image, label, eps, return_perturbed=True)
    assert list(sweep) == eps
    dec = R.decided(c["dimage"])
    for k, e in enumerate(eps):
        mean, av, ev, pert = sweep[e]
        pert_np = pert.cpu().numpy()
        diff = pert_np != c["perturbed"][k]
        print(f"{name} {precision} eps {e}: {int(diff.sum())} pixels differ from the fixture, all of them undecided "
              f"({int((~dec).sum())} undecided of {dec.size})")
        assert not (diff & dec).any()
        out = O.mimo_unet_forward(c["cfg"], c["state"], O.repeat_subnetworks(torch.from_numpy(pert_np), c["cfg"].num_subnetworks),
                                  training=False)
        p1, p2 = O.split_heads(out, 2)
        ens.return_raw_predictions = True
        g1, g2 = ens(pert)
        ens.return_raw_predictions = False
        want = O.compute_uncertainties(c["kind"], p1, p2)
        errs = {"p1": rel_err(g1.cpu(), p1), "p2": rel_err(g2.cpu(), p2), "mean": rel_err(mean.cpu(), want[0]),
                "aleatoric": rel_err(av.cpu(), want[1]), "epistemic": rel_err(ev.cpu(), want[2])}
        print("   ", errs)
        assert all(v <= TOL for v in errs.values()), errs
    assert model.model.numerics_status() == 0


def _train_case():
    cfg = O.NetConfig(2, 2, 3, 10)
    st = O.init_state(cfg, 91)
    g = torch.Generator().manual_seed(92)
    batches = []
    for _ in range(4):
        image, label = torch.rand(3, 2, 100, 100, generator=g).cuda(), torch.rand(3, 1, 100, 100, generator=g).cuda()
        mask = (torch.rand(3, 1, 100, 100, generator=g) > 0.3).float().cuda()
        batches.append((image, label, mask, O.draw_perms(3, 3, generator=g).cuda()))
    return cfg, st, batches


def _train_run(monkeypatch, env, cfg, st, batches, with_sweeps):
    from mimo.adversarial import fgsm_sweep
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(5)
    model = _model(cfg, st, "laplace_nll", "split16", monkeypatch).train()
    ens = None
    opt = model.configure_optimizers()["optimizer"]
    grads, preds = [], []
    for image, label, mask, perms in batches:
        opt.zero_grad()
        out = model.training_step_with_perms(image, label, mask, perms)
        out["loss"].backward()
        grads.append(model.model.flat_gradients().clone())
        preds.append(out["preds"].clone())
        if with_sweeps:  # between backward and optimiser step: .grad is live, the side stream has just been busy
            net = model.model
            model.eval()
            if ens is None:
                ens = _ensemble([model])
            g0, b0, p0 = net.flat_gradients().clone(), net._flat_buffers.clone(), net.flat_parameters().clone()
            pg = [p.grad for p in model.parameters()]
            sweep = fgsm_sweep(ens, image, label, (0.0, 0.02, 0.04), mask=mask)
            assert all(torch.isfinite(t).all() for r in sweep.values() for t in r)
            assert torch.equal(net.flat_gradients(), g0), "the sweep wrote the flat gradient buffer"
            assert torch.equal(net._flat_buffers, b0), "the sweep wrote the BatchNorm buffers"
            assert torch.equal(net.flat_parameters(), p0)
            assert all(a is b for a, b in zip(pg, [p.grad for p in model.parameters()]))
            assert not model.training and not net._bn_training()  # flags as the caller left them
            model.train()
        opt.step()
    torch.cuda.synchronize()
    assert model.model.numerics_status() == 0
    for k in env:
        monkeypatch.delenv(k)
    return grads, preds, model.model.flat_parameters().clone(), model.model._flat_buffers.clone()


@pytest.mark.parametrize("env", [{"MIMO_WGRAD_STREAM": "0"}, {"MIMO_WGRAD_STREAM": "1"}, {"MIMO_WGRAD_STREAM": "1", "MIMO_TRAIN_GRAPH": "1"},
                                 {"MIMO_WGRAD_STREAM": "1", "MIMO_DEBUG_WGRAD_DELAY_US": "100"}],
                         ids=["one-stream", "side-stream", "train-graph", "late-weight-gradients"])
def test_sweep_touches_nothing_and_training_steps_around_it_keep_their_bits(env, monkeypatch):
    """Four Adam steps with a sweep after every backward against the same steps without: gradient buffer, predictions,
    parameters and BatchNorm buffers bit-identical (in the manner of tests/test_streams_gpu.py), and inside the run the flat
    .grad buffer and the BatchNorm buffers are bit-identical across each sweep."""
    cfg, st, batches = _train_case()
    plain = _train_run(monkeypatch, env, cfg, st, batches, with_sweeps=False)
    mixed = _train_run(monkeypatch, env, cfg, st, batches, with_sweeps=True)
    for name, xs, ys in (("gradient buffer", plain[0], mixed[0]), ("predictions", plain[1], mixed[1])):
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(x, y), f"{name} of step {i} differs by up to {float((x - y).abs().max()):.3e}"
    assert torch.equal(plain[2], mixed[2]) and torch.equal(plain[3], mixed[3])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_member_ensemble_accumulates_with_one_over_s_total(precision, monkeypatch):
    """Members with S = 2 (the fixture's network) and S = 3 (seeded, seeded running statistics): the loss the reference's
    script takes is the mean over the concatenated subnetwork axis, i.e. 1 / 5 on every subnetwork's mean NLL."""
    from mimo.adversarial import image_gradient
    c = case(load_npz("fgsm.npz"), "laplace")
    cfg_b = O.NetConfig(2, 2, 3, 4)
    st_b = O.init_state(cfg_b, 17)
    g = torch.Generator().manual_seed(18)
    for k in st_b:
        if k.endswith("running_mean"):
            st_b[k] = 0.2 * torch.randn(st_b[k].shape, generator=g)
        elif k.endswith("running_var"):
            st_b[k] = 0.5 + torch.rand(st_b[k].shape, generator=g)
    members = [_model(c["cfg"], c["state"], "laplace_nll", precision, monkeypatch), _model(cfg_b, st_b, "laplace_nll", precision, monkeypatch)]
    image, label = torch.from_numpy(c["image"]), torch.from_numpy(c["label"])
    got = image_gradient(_ensemble(members), image.cuda(), label.cuda())
    img = image.clone().requires_grad_(True)
    outs = [O.mimo_unet_forward(cf, st, O.repeat_subnetworks(img, cf.num_subnetworks), training=False)
            for cf, st in ((c["cfg"], c["state"]), (cfg_b, st_b))]
    p1, p2 = torch.cat([o[:, :, :1] for o in outs], 1), torch.cat([o[:, :, 1:] for o in outs], 1)
    O.loss_forward("laplace_nll", p1, p2, label[:, None].repeat(1, 5, 1, 1, 1)).backward()
    err = rel_err(got.cpu(), img.grad)
    print(precision, "two members, image gradient vs oracle:", err, "undecided share", R.undecided_share(img.grad.numpy()))
    assert err <= TOL


def test_robustness_evaluator_tables_and_file_names(tmp_path, monkeypatch):
    from mimo.adversarial import RobustnessEvaluator
    from mimo.evaluation import UncertaintyEvaluator
    c = case(load_npz("fgsm.npz"), "laplace")
    ens = _ensemble([_model(c["cfg"], c["state"], c["kind"], "split16", monkeypatch)])
    g = torch.Generator().manual_seed(3)
    rob, plain = RobustnessEvaluator(), UncertaintyEvaluator()
    assert rob.epsilons == (0.0, 0.02, 0.04)
    for _ in range(2):
        image = (torch.rand(3, 2, 34, 34, generator=g) * 1.2 - 0.1).cuda()  # some pixels outside [0, 1]: eps = 0 still clamps
        label = torch.rand(3, 1, 34, 34, generator=g).cuda()
        rob.update_from(ens, image, label)
        plain.update_from(ens, image.clamp(0, 1), label)
    tables, want = rob.compute(), plain.compute()
    for key in ("precision_recall", "calibration"):
        for col, v in want[key].items():
            assert np.array_equal(tables[0.0][key][col], v, equal_nan=True), (key, col)
    assert tables[0.0]["n"] == want["n"] == 2 * 3 * 34 * 34
    assert not np.array_equal(tables[0.04]["precision_recall"]["mae"], want["precision_recall"]["mae"])
    paths = rob.write_csv(str(tmp_path), "nyuv2", tables)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f"nyuv2_{e}_{k}.csv" for e in ("0.0", "0.02", "0.04") for k in ("precision_recall", "calibration")), names
    assert open(paths[0.02][0]).readline().strip() == "percentile,mae,rmse"
    assert open(paths[0.02][1]).readline().strip() == "Expected Conf.,Observed Conf."


def test_bench_geometry_cfg3_batch_32(monkeypatch):
    """cfg3 (2 -> 1 channels, S = 2, fbc = 30) at batch 32, 256 x 256: finite, the sign of every decided pixel agrees with
    the parent route's gradient (decided on that gradient), no numerics status bits."""
    cfg = O.NetConfig(in_channels=2, out_channels=2, num_subnetworks=2, filter_base_count=30)
    model = _model(cfg, O.init_state(cfg, 1), "laplace_nll", "split16", monkeypatch)
    g = torch.Generator(device="cuda").manual_seed(100)
    image = torch.rand(32, 2, 256, 256, device="cuda", generator=g)
    label = torch.rand(32, 1, 256, 256, device="cuda", generator=g)
    dloss = torch.full((2,), 0.5, device="cuda")
    dimage = torch.empty_like(image)
    with torch.no_grad():
        model.model.image_gradient(image, label, None, dloss, dimage)
    assert torch.isfinite(dimage).all()
    _, dx = _parent_route(model, image, label, dloss)
    ref = _sum_in_engine_order(dx)
    dec = ref.abs() >= R.DECIDED_REL * ref.abs().max()
    flips = int(((torch.sign(dimage) != torch.sign(ref)) & dec).sum())
    print(f"cfg3 batch 32: decided {float(dec.float().mean()):.4%}, sign flips at decided pixels {flips}, "
          f"bitwise equal {bool(torch.equal(dimage, ref))}, max |g| {float(ref.abs().max()):.3e}")
    assert flips == 0
    net = model.model
    for key, plan in net._plans.items():
        print("   plan", key[-1], "workspace bytes", plan.workspace_bytes)
    assert net.numerics_status() == 0
