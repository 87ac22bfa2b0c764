"""mimo_evidential_step and mimo_evidential_loss_gradient_dev — the evidential model's training / validation step tail in one
pass over the logits and its backward under a device-held upstream gradient — against the fp64 reference of
tests/evidential_step_reference.py, by the rules of tests/test_scalar_kernels_gpu.py: maps per element within 4 x the
yardstick (the fp32 torch reference's own distance from fp64), reduced scalars by check_scalar, the loss mean by the mean of
the per-element allowances (conditioning where the fp32 reference has no result: alpha > 35).  Every output starts NaN-filled.
Then EvidentialUnetModel's two steps on the new path against the tensor operations they replace (the switch off)."""
import numpy as np
import pytest
import torch

from tests import evidential_step_reference as S
from tests import scalar_reference as R
from tests.helpers import fp32_acc_bound, report
from tests.test_scalar_kernels_gpu import MIMO_ERR_INVALID, _check_regression_scalars, _L, bits, nans, written

pytestmark = pytest.mark.gpu
GRID_CAP = 2048                      # workgroups of mimo_evidential_step's largest grid (256 threads each)
PAST_A_PASS = GRID_CAP * 256 + 259   # one pixel per thread (odd hw): one full pass and 259 pixels


def _step(lg, y, mk, want_epi=True, blocks=GRID_CAP):
    """mimo_evidential_step on logits [N,4,hw] (CPU tensors; mk may be None): the maps, the scalars, the return code"""
    L = _L()
    lib = L.load()
    N, _, hw = lg.shape
    lgd, yd = lg.cuda().contiguous(), y.cuda().contiguous()
    mkd = None if mk is None else mk.cuda().contiguous()
    o = {"aleatoric_std": nans(N, hw), "epistemic_std": nans(N, hw), "err": nans(N, hw), "scalars": nans(8)}
    scratch = nans(GRID_CAP * 8, dtype=torch.float64)
    L.check(lib.mimo_evidential_step(lgd.data_ptr(), yd.data_ptr(), L.ptr(mkd) or None, N, hw, o["aleatoric_std"].data_ptr(),
                                     o["epistemic_std"].data_ptr() if want_epi else None, o["err"].data_ptr(),
                                     o["scalars"].data_ptr(), scratch.data_ptr(), blocks, L.current_stream()), "mimo_evidential_step")
    torch.cuda.synchronize()
    if not want_epi:
        assert bool(torch.isnan(o["epistemic_std"]).all()), "epistemic_std = NULL must not be written"
        del o["epistemic_std"]
    written(*o.values())
    return {k: v.cpu() for k, v in o.items()}


def _check_step(tag, lg, y, mk, blocks=GRID_CAP, fp32_reference_finite=False):
    """both calls (with and without the epistemic map) against the fp64 reference: three maps, eight scalars"""
    from mimo_unet_amd.engine import EVIDENTIAL_STEP_SCALARS
    yd, ref, bad, cond = S.step_yardstick(lg, y, mk)
    assert (cond is None) == fp32_reference_finite
    got = _step(lg, y, mk, True, blocks)
    fl = lambda k: R._floor_of(S.STEP_FLOORS, k, ref[k])
    for k in ("aleatoric_std", "epistemic_std", "err"):
        R.check("evidential_step", f"{tag} {k}", got[k], ref[k], fl(k), yd[k])
    sc = _check_regression_scalars("evidential_step", tag, got["scalars"], EVIDENTIAL_STEP_SCALARS, ref, yd, S.STEP_FLOORS, y)
    for name, term in (("aleatoric_std_mean", "aleatoric_clip"), ("epistemic_std_mean", "epistemic_clip")):
        R.check_scalar("evidential_step", f"{tag} {name}", sc[name], float(ref[term].mean()), yd[term], R.term_scale(ref[term], fl(term)))
    S.check_loss_mean("evidential_step", tag, sc["loss"], ref["loss"], yd["loss"], bad["loss"], cond)
    assert sc["count"] == float(y.numel())
    if mk is not None:  # the mask reaches the loss and nothing else
        free = _step(lg, y, None, True, blocks)
        for k in ("aleatoric_std", "epistemic_std", "err"):
            assert torch.equal(bits(got[k]), bits(free[k])), k
        assert torch.equal(bits(got["scalars"][1:]), bits(free["scalars"][1:]))
    less = _step(lg, y, mk, False, blocks)
    assert int(bits(less["scalars"])[6]) == 0, "slot 6 must be exactly 0 without the epistemic map"
    keep = [0, 1, 2, 3, 4, 5, 7]
    assert torch.equal(bits(less["scalars"][keep]), bits(got["scalars"][keep])), (less["scalars"], got["scalars"])
    for k in ("aleatoric_std", "err"):
        assert torch.equal(bits(less[k]), bits(got[k])), k
    return got


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("N", [1, 2, 5])
def test_evidential_step_over_the_parameter_sweep(N, masked):
    """R.evidential_sweep (1900 pixels: alpha - 1 in [1e-4, 1e4], v and beta in [1e-3, 1e3], |y - mu| up to 30, every seventh
    pixel masked).  N = 1: hw = 1900, 16-byte accesses; N = 2: hw = 950, one pixel per thread, and a grid capped at 3
    workgroups by scratch_blocks (the grid-stride loop runs again); N = 5: hw = 380, 16-byte accesses across images.  With
    and without a mask, with and without the epistemic map (slot 6 exactly 0, everything else the same bits)."""
    logits, label, mask, _ = R.evidential_sweep()
    lg, y, mk = R.pixels_to_layout(logits, label, mask, N)
    _check_step(f"sweep N={N} {'mask' if masked else 'no mask'}", lg, y, mk if masked else None, blocks=3 if N == 2 else GRID_CAP)


def test_evidential_step_one_element_group_past_a_grid_pass():
    """2048 x 256 + 259 ordinary pixels, one image, odd hw: one full pass of the largest grid and a second, partial one; the
    finalize kernel walks all 2048 partial rows.  The fp32 reference is finite on every pixel."""
    lg, y, mk = R.pixels_to_layout(*R.evidential_ordinary(PAST_A_PASS), 1)
    _check_step(f"{PAST_A_PASS} pixels", lg, y, mk, fp32_reference_finite=True)


def _gradients(lg, y, mk, scale, upstream):
    """(mimo_evidential_loss_gradient_dev with `upstream` on the device, mimo_evidential_loss_gradient with the fp32 product
    formed on the host), both [N,4,hw] on the CPU"""
    L = _L()
    lib = L.load()
    N, _, hw = lg.shape
    lgd, yd, mkd = lg.cuda().contiguous(), y.cuda().contiguous(), (None if mk is None else mk.cuda().contiguous())
    up = torch.tensor([upstream], dtype=torch.float32, device="cuda")
    dev, host = nans(N, 4, hw), nans(N, 4, hw)
    L.check(lib.mimo_evidential_loss_gradient_dev(lgd.data_ptr(), yd.data_ptr(), L.ptr(mkd) or None, N, hw, R.f32(scale), up.data_ptr(),
                                                  dev.data_ptr(), L.current_stream()), "mimo_evidential_loss_gradient_dev")
    product = float(np.float32(scale) * np.float32(upstream))  # one fp32 multiplication
    L.check(lib.mimo_evidential_loss_gradient(lgd.data_ptr(), yd.data_ptr(), L.ptr(mkd) or None, N, hw, product, host.data_ptr(),
                                              L.current_stream()), "mimo_evidential_loss_gradient")
    torch.cuda.synchronize()
    written(dev, host)
    return dev.cpu(), host.cpu()


@pytest.mark.parametrize("layout", ["sweep N=1", "sweep N=2", "past a pass"])
def test_loss_gradient_with_a_device_upstream_is_the_loss_gradient_bit_for_bit(layout):
    """upstream 1, 0.37 and 1024 in a device tensor: the same bits as mimo_evidential_loss_gradient given float32(scale) *
    float32(upstream) from the host; masked pixels exactly zero in all four channels; without a mask too."""
    if layout == "past a pass":
        lg, y, mk = R.pixels_to_layout(*R.evidential_ordinary(PAST_A_PASS), 1)
    else:
        logits, label, mask, _ = R.evidential_sweep()
        lg, y, mk = R.pixels_to_layout(logits, label, mask, int(layout[-1]))
    scale = np.float32(1.0) / np.float32(y.numel())
    for upstream in (1.0, 0.37, 1024.0):
        dev, host = _gradients(lg, y, mk, scale, upstream)
        assert torch.equal(bits(dev), bits(host)), (layout, upstream)
        assert float(dev.permute(0, 2, 1)[mk == 0].abs().max()) == 0.0, "masked pixels must give exactly zero"
        assert float(dev.abs().max()) > 0.0
    dev, host = _gradients(lg, y, None, scale, 0.37)
    assert torch.equal(bits(dev), bits(host))


REQUIRED = ("logits", "label", "aleatoric_std", "err", "scalars", "scratch")


@pytest.mark.parametrize("bad", [dict(null=k) for k in REQUIRED] + [dict(n=0), dict(hw=0), dict(scratch_blocks=0), dict(n=-1)], ids=str)
def test_evidential_step_rejects_invalid_arguments_and_writes_nothing(bad):
    L = _L()
    lib = L.load()
    N, hw = 2, 12
    t = {"logits": torch.randn(N, 4, hw, device="cuda"), "label": torch.randn(N, hw, device="cuda"), "aleatoric_std": nans(N, hw),
         "epistemic_std": nans(N, hw), "err": nans(N, hw), "scalars": nans(8), "scratch": nans(16 * 8, dtype=torch.float64)}
    p = {k: (None if bad.get("null") == k else v.data_ptr()) for k, v in t.items()}
    rc = lib.mimo_evidential_step(p["logits"], p["label"], None, bad.get("n", N), bad.get("hw", hw), p["aleatoric_std"],
                                  p["epistemic_std"], p["err"], p["scalars"], p["scratch"], bad.get("scratch_blocks", 16),
                                  L.current_stream())
    torch.cuda.synchronize()
    assert rc == MIMO_ERR_INVALID and b"mimo_evidential_step" in lib.mimo_last_error()
    for k in ("aleatoric_std", "epistemic_std", "err", "scalars", "scratch"):
        assert bool(torch.isnan(t[k]).all()), k


@pytest.mark.parametrize("null", ["logits", "label", "upstream", "dlogits"])
def test_loss_gradient_dev_rejects_null_pointers_and_writes_nothing(null):
    L = _L()
    lib = L.load()
    N, hw = 2, 12
    t = {"logits": torch.randn(N, 4, hw, device="cuda"), "label": torch.randn(N, hw, device="cuda"),
         "upstream": torch.ones(1, device="cuda"), "dlogits": nans(N, 4, hw)}
    p = {k: (None if k == null else v.data_ptr()) for k, v in t.items()}
    rc = lib.mimo_evidential_loss_gradient_dev(p["logits"], p["label"], None, N, hw, 0.5, p["upstream"], p["dlogits"], L.current_stream())
    torch.cuda.synchronize()
    assert rc == MIMO_ERR_INVALID and bool(torch.isnan(t["dlogits"]).all())


# ---- EvidentialUnetModel -----------------------------------------------------------------------------------------------------

B, H, W = 3, 32, 32


def _models(count):
    from mimo.models.evidential_unet import EvidentialUnetModel
    torch.manual_seed(5)
    out = []
    for _ in range(count):
        m = EvidentialUnetModel(in_channels=3, out_channels=4, filter_base_count=4, center_dropout_rate=0.0, final_dropout_rate=0.0,
                                encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0,
                                learning_rate=1e-3, seed=0)
        if out:
            m.load_state_dict(out[0].state_dict())
        m.model.set_precision("fp32")
        out.append(m.cuda())
    return out


def _batch(masked):
    g = torch.Generator().manual_seed(6)
    image, label = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 1, H, W, generator=g) * 2 - 0.5
    mask = (torch.rand(B, H, W, generator=g) > 0.25).float() if masked else None
    return image, label, mask


def _run_step(m, fused, stage, batch, monkeypatch, loss_factor=None):
    """one training_step + backward (or one eval-mode validation_step) of model `m` with the switch at `fused`: the step's
    dict, the logits the step saw, what it logged, and the gradients"""
    import mimo_unet_amd.models.evidential_unet as EU
    monkeypatch.setattr(EU, "_FUSED_STEP", fused)
    image, label, mask = batch
    x = image.cuda().requires_grad_(stage == "train")
    seen, inner = [], m._logits
    m._logits = lambda t: (seen.append(inner(t)), seen[-1])[1]
    m.logged.clear()
    try:
        if stage == "train":
            m.train()
            out = m.training_step({"image": x, "label": label.cuda(), **({} if mask is None else {"mask": mask.cuda()})}, 0)
            (out["loss"] if loss_factor is None else out["loss"] * loss_factor).backward()
        else:
            m.eval()
            out = m.validation_step({"image": x, "label": label.cuda(), **({} if mask is None else {"mask": mask.cuda()})}, 0)
    finally:
        del m._logits
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()} if stage == "train" else {}
    if stage == "train":
        grads["image"] = x.grad.detach().cpu().clone()
    assert len(seen) == 1
    return {"out": out, "logits": seen[0].detach().float().cpu(), "logged": {k: float(v) for k, v in m.logged.items()}, "grads": grads}


def _compare_paths(stage, on, off, batch):
    image, label, mask = batch
    maps = ["aleatoric_std_map", "err_map"] + (["epistemic_std_map"] if stage == "val" else [])
    assert list(on["out"]) == list(off["out"])
    for k in on["out"]:
        a, b = on["out"][k], off["out"][k]
        assert (a is None and b is None) or tuple(a.shape) == tuple(b.shape), k
    assert tuple(on["out"]["loss"].shape) == () and on["out"]["loss"].requires_grad == (stage == "train")
    assert not any(on["out"][k].requires_grad for k in maps + ["preds"])
    assert torch.equal(bits(on["logits"]), bits(off["logits"])), "the same backbone forward"
    assert torch.equal(bits(on["out"]["preds"]), bits(off["out"]["preds"]))
    lg, y = on["logits"].reshape(B, 4, H * W), label.reshape(B, H * W)
    mk = None if mask is None else mask.reshape(B, H * W)
    yd, ref, bad, cond = S.step_yardstick(lg, y, mk)
    assert cond is None
    fl = lambda k: R._floor_of(S.STEP_FLOORS, k, ref[k])
    for name, r in (("fused", on), ("tensor operations", off)):
        tag = f"{stage}_step ({name})"
        for k in maps:
            rk = k[:-len("_map")]
            R.check("evidential_step", f"{tag} {k}", r["out"][k].reshape(B, H * W), ref[rk], fl(rk), yd[rk])
        lo = r["logged"]
        sc = [lo[f"metric_{stage}/{k}"] for k in ("mae", "mse", "rmse", "r2")] + [float(B * H * W)]
        _check_regression_scalars("evidential_step", tag, sc, ("mae", "mse", "rmse", "r2", "count"), ref, yd, S.STEP_FLOORS, y)
        if stage == "val":
            for key, term in (("metric_val/aleatoric_std_mean", "aleatoric_clip"), ("metric_val/epistemic_std_mean", "epistemic_clip")):
                R.check_scalar("evidential_step", f"{tag} {key}", lo[key], float(ref[term].mean()), yd[term], R.term_scale(ref[term], fl(term)))
            assert lo["val_loss"] == float(r["out"]["loss"])
    assert set(on["logged"]) == set(off["logged"])
    # the loss: the tensor operations sum B H W fp32 terms in fp32, the kernel in double; the terms themselves differ by
    # roundings of single operations (2^-24 each, far inside sqrt(B H W) of them).  Scale: the mean |term|.
    lon, loff = float(on["out"]["loss"].detach()), float(off["out"]["loss"].detach())
    allowed = fp32_acc_bound(B * H * W, 0.0) * float(ref["loss"].abs().mean())
    report(f"[evidential_step] {stage}_step loss: fused {lon:.9e} tensor operations {loff:.9e} fp64 {float(ref['loss'].mean()):.9e} allowed {allowed:.2e}")
    assert abs(lon - loff) <= allowed
    S.check_loss_mean("evidential_step", f"{stage}_step (fused)", lon, ref["loss"], yd["loss"], bad["loss"], cond)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_training_step_on_the_fused_path_matches_the_tensor_operations(masked, monkeypatch):
    """in_channels 3, f = 4, 3 x 32 x 32, fp32, training mode; two models with the same weights, the switch on and off: the same
    keys and shapes, bit-identical predictions, maps and logged metrics within their bounds of the fp64 reference on the
    logits, the loss within the fp32 accumulation bound — and EVERY parameter gradient and the image gradient bit for bit
    (the same device function on the same 1 / (B H W)); with the loss times 1024 every gradient exactly 1024 times that."""
    batch = _batch(masked)
    m_on, m_off, m_scaled = _models(3)
    on, off = _run_step(m_on, True, "train", batch, monkeypatch), _run_step(m_off, False, "train", batch, monkeypatch)
    _compare_paths("train", on, off, batch)
    assert set(on["grads"]) == set(off["grads"]) and len(on["grads"]) > 10
    for k, g in on["grads"].items():
        assert torch.equal(bits(g), bits(off["grads"][k])), k
        assert bool(torch.isfinite(g).all())
    assert float(on["grads"]["image"].abs().max()) > 0.0
    scaled = _run_step(m_scaled, True, "train", batch, monkeypatch, loss_factor=1024.0)
    for k, g in on["grads"].items():
        assert torch.equal(bits(g * 1024.0), bits(scaled["grads"][k])), k


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_validation_step_on_the_fused_path_matches_the_tensor_operations(masked, monkeypatch):
    """the same comparison in eval mode, with the epistemic map, val_loss and the two logged uncertainty means"""
    batch = _batch(masked)
    m_on, m_off = _models(2)
    on, off = _run_step(m_on, True, "val", batch, monkeypatch), _run_step(m_off, False, "val", batch, monkeypatch)
    _compare_paths("val", on, off, batch)


def test_a_four_dimensional_mask_keeps_the_tensor_operations(monkeypatch):
    """a [B,1,H,W] mask (which broadcasts the loss map to [B,B,H,W]) is left to the loss class with the switch on, as
    _forward_with_loss leaves it: the new entry point is not called and the step gives what it gives with the switch off"""
    import mimo_unet_amd.models.evidential_unet as EU
    image, label, mask = _batch(True)
    batch = (image, label, mask[:, None])
    m_on, m_off = _models(2)

    def refuse(*a, **k):
        raise AssertionError("evidential_step called for a [B,1,H,W] mask")
    monkeypatch.setattr(EU, "evidential_step", refuse)
    on, off = _run_step(m_on, True, "train", batch, monkeypatch), _run_step(m_off, False, "train", batch, monkeypatch)
    for k, v in on["out"].items():
        assert torch.equal(v, off["out"][k]), k
    for k, g in on["grads"].items():
        assert torch.equal(bits(g), bits(off["grads"][k])), k


def test_a_label_or_mask_left_on_the_host_never_reaches_the_kernel_as_a_host_pointer():
    """the gate of the model's fused path asks for the whole batch on the GPU, not the image alone (decided before anything
    runs); engine.evidential_step itself moves a host label / mask to the logits' device and gives the same bits"""
    from mimo_unet_amd.engine import evidential_step
    image, label, mask = _batch(True)
    (m,) = _models(1)
    for lb, mk in ((label, mask.cuda()), (label.cuda(), mask), (label, None)):
        assert m._fused_step(image.cuda(), lb, mk, "train") is None
    logits = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(8)).cuda()
    want = evidential_step(logits, label.cuda(), mask.cuda(), True)
    got = evidential_step(logits, label, mask, True)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert a.is_cuda and torch.equal(bits(a), bits(b))


def test_evidential_step_loss_of_every_sweep_pixel_on_its_own():
    """The sweep's loss mean is carried by its largest terms (|y - mu| = 30 at alpha = 1e4: 1e7 per pixel), so a wrong loss on
    a small pixel would hide in it.  Here every pixel's loss is read on its own: one call per pixel with a one-hot mask, whose
    loss slot is float(loss_i / P) — loss_i to one more rounding (2^-24, inside the 4-ulp floor of the bound).  Judged per
    element like the loss map of mimo_evidential_forward: 4 x the yardstick where the fp32 reference is finite, the
    conditioning where it is not.  Both layouts (16-byte accesses, one pixel per thread)."""
    L = _L()
    lib = L.load()
    logits, label, _, _ = R.evidential_sweep()
    P = label.numel()
    for N in (1, 2):
        lg, y, _ = R.pixels_to_layout(logits, label, torch.ones(P), N)
        yd, ref, bad, cond = S.step_yardstick(lg, y, None)
        hw = P // N
        lgd, yd_, mk = lg.cuda().contiguous(), y.cuda().contiguous(), torch.zeros(P, device="cuda")
        alea, err, sc, scratch = nans(N, hw), nans(N, hw), nans(P, 8), nans(GRID_CAP * 8, dtype=torch.float64)
        st = L.current_stream()
        for i in range(P):
            mk[i] = 1.0
            L.check(lib.mimo_evidential_step(lgd.data_ptr(), yd_.data_ptr(), mk.data_ptr(), N, hw, alea.data_ptr(), None, err.data_ptr(),
                                             sc[i].data_ptr(), scratch.data_ptr(), GRID_CAP, st), "mimo_evidential_step")
            mk[i] = 0.0
        torch.cuda.synchronize()
        written(sc)
        loss = (sc[:, 0].double().cpu() * P).reshape(N, hw)
        R.check("evidential_step", f"sweep N={N} per-pixel loss", loss, ref["loss"], R.TINY, yd["loss"], where=~bad["loss"])
        R.check_conditioned("evidential_step", f"sweep N={N} per-pixel loss", loss, ref["loss"], R.TINY, cond, bad["loss"])
