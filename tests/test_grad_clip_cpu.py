"""tests/grad_clip_reference.py against what it stands for (torch's own clipping followed by torch.optim.Adam), the draws of
the GPU tests, FlatAdam's host logic around the clipped step and the Lightning hook of the two model classes — no GPU."""
import pytest
import torch

from tests import grad_clip_reference as G
from tests import scalar_reference as R
from tests.test_host_cpu import _FakeFlatNet


@pytest.mark.parametrize("mode", ["norm", "value"])
@pytest.mark.parametrize("active", [True, False])
@pytest.mark.parametrize("wd", G.WDS)
def test_reference_equals_torch_clipping_followed_by_torch_adam(wd, active, mode):
    """fp64, three steps, a parameter list cut into uneven views of one flat buffer: clip_grad_norm_ / clip_grad_value_ then
    torch.optim.Adam (hyper-parameters as the floats the C ABI carries) against clip_reference, rtol 1e-12"""
    n, cuts = 1027, (0, 1, 8, 300, 301, 1027)
    gen = torch.Generator().manual_seed(5)
    flat = torch.randn(n, generator=gen).double()
    grads = [torch.randn(n, generator=gen).double() for _ in range(3)]
    if mode == "norm":
        clip = G.clip_for(grads[0], G.ACTIVE if active else G.INACTIVE)
    else:
        clip = R.f32(G.VALUE_CLIP if active else 100.0)
    params = [torch.nn.Parameter(flat[a:b].clone()) for a, b in zip(cuts[:-1], cuts[1:])]
    opt = torch.optim.Adam(params, lr=R.f32(1e-3), betas=(R.f32(0.9), R.f32(0.999)), eps=R.f32(1e-8), weight_decay=R.f32(wd))
    st = {"p": flat.clone(), "m": torch.zeros(n, dtype=torch.float64), "v": torch.zeros(n, dtype=torch.float64)}
    for step, g in enumerate(grads, 1):
        for q, (a, b) in zip(params, zip(cuts[:-1], cuts[1:])):
            q.grad = g[a:b].clone()
        if mode == "norm":
            total = torch.nn.utils.clip_grad_norm_(params, clip)
        else:
            torch.nn.utils.clip_grad_value_(params, clip)
        opt.step()
        st = G.clip_reference(st["p"], g, st["m"], st["v"], step=step, mode=mode, clip=clip, wd=wd)
        assert st["applied"]
        if mode == "norm":
            torch.testing.assert_close(st["norm"], total, rtol=1e-12, atol=0.0)
            assert (float(st["coef"]) < 1.0) == active
        torch.testing.assert_close(st["p"], torch.cat([q.detach() for q in params]), rtol=1e-12, atol=0.0)
        for k, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            torch.testing.assert_close(st[k], torch.cat([opt.state[q][key] for q in params]), rtol=1e-12, atol=1e-300)


def test_reference_skip_rule_and_scale():
    p, g, m, v = G.clip_inputs(5, 2)
    for bad, found in ((float("inf"), 0.0), (float("nan"), 0.0), (1.0, 1.0)):
        gb = g.clone()
        gb[3] = bad
        r = G.clip_reference(p, gb, m, v, step=2, mode="norm", clip=1.0, found_inf=found)
        assert not r["applied"] and all(torch.equal(r[k], t) for k, t in (("p", p), ("m", m), ("v", v)))
        assert bool(torch.isfinite(r["norm"])) == (found != 0.0)
    # the loss scale divides out: g * 1024 with amp_scale = 1024 is the plain step
    a = G.clip_reference(p, g * 1024.0, m, v, step=2, mode="norm", clip=0.5, amp_scale=1024.0)
    b = G.clip_reference(p, g, m, v, step=2, mode="norm", clip=0.5)
    assert all(torch.equal(a[k], b[k]) for k in ("p", "m", "v", "norm", "coef"))
    # value mode keeps a NaN a NaN
    gb = g.clone()
    gb[0] = float("nan")
    r = G.clip_reference(p, gb, m, v, step=2, mode="value", clip=0.5)
    assert r["applied"] and bool(torch.isnan(r["p"][0])) and bool(torch.isfinite(r["p"][1:]).all())


def test_the_draws_of_the_gpu_tests_are_unambiguous():
    """coefficient exactly 1 with norm <= 0.99 clip, or <= 0.999: fp32 and fp64 agree about whether clipping happened"""
    count = 0
    for g, gs, amp, clip in G.all_norm_draws():
        ok, (norm, coef) = G.is_unambiguous(g, gs, amp, clip)
        assert ok, (g.numel(), gs, amp, clip, norm, coef)
        count += 1
    assert count >= 40
    for name, g, exact in G.integer_gradients():
        assert float((g.double() ** 2).sum()) == exact * exact, name


# ---- FlatAdam host logic ---------------------------------------------------------------------------------------------------

class _Calls:
    def __init__(self, monkeypatch):
        from mimo_unet_amd import optim as OP
        self.plain, self.amp, self.clipped = [], [], []
        monkeypatch.setattr(OP, "adam_step", lambda p, g, m, v, **kw: self.plain.append(kw))
        monkeypatch.setattr(OP, "adam_step_amp", lambda p, g, m, v, **kw: self.amp.append(kw))
        monkeypatch.setattr(OP, "adam_step_clipped", lambda p, g, m, v, **kw: self.clipped.append(kw))


def test_flat_adam_without_a_clip_setting_takes_the_two_existing_branches(monkeypatch):
    from mimo_unet_amd import optim as OP
    calls = _Calls(monkeypatch)
    opt = OP.FlatAdam(_FakeFlatNet(), lr=1e-2, weight_decay=0.5)
    assert opt.max_grad_norm is None and opt.clip_value is None and opt.last_grad_norm is None and opt.last_clip_coef is None
    opt.reduce_scale = 0.25
    opt.step()
    assert calls.plain == [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.5, step=1, grad_scale=0.25)]
    assert not calls.amp and not calls.clipped and opt._step_dev is None
    opt.grad_scale, opt.found_inf = torch.tensor(1024.0), torch.tensor(0.0)
    opt.step()
    del opt.grad_scale, opt.found_inf
    assert len(calls.plain) == 1 and len(calls.amp) == 1 and not calls.clipped
    kw = calls.amp[0]
    assert set(kw) == {"lr", "betas", "eps", "weight_decay", "step_dev", "reduce_scale", "amp_scale", "found_inf"}
    assert kw["reduce_scale"] == 0.25 and float(kw["amp_scale"]) == 1024.0 and float(kw["found_inf"]) == 0.0
    assert "max_grad_norm" not in opt.state_dict()["param_groups"][0] and set(opt.state_dict()) == {"state", "param_groups", "flat"}


@pytest.mark.parametrize("mode", ["norm", "value"])
def test_flat_adam_hands_the_clipped_step_scaler_and_reduce_scale(monkeypatch, mode):
    from mimo_unet_amd import optim as OP
    calls = _Calls(monkeypatch)
    opt = OP.FlatAdam(_FakeFlatNet(), lr=1e-2, **({"max_grad_norm": 2.5} if mode == "norm" else {"clip_value": 2.5}))
    opt.reduce_scale = 0.125
    opt._step = 7  # seven plain steps before clipping was switched on: the device counter starts there
    opt.grad_scale, opt.found_inf = torch.tensor(512.0), torch.tensor(1.0)
    opt.step()
    del opt.grad_scale, opt.found_inf
    assert not calls.plain and not calls.amp and len(calls.clipped) == 1
    kw = calls.clipped[0]
    assert kw["clip_mode"] == mode and kw["clip"] == 2.5 and kw["reduce_scale"] == 0.125
    assert float(kw["amp_scale"]) == 512.0 and float(kw["found_inf"]) == 1.0
    assert kw["step_dev"] is opt._step_dev and float(kw["step_dev"]) == 7.0 and kw["step_dev"].dtype == torch.float32
    assert kw["clip_out"].shape == (2,) and kw["clip_out"].dtype == torch.float32
    kw["clip_out"].copy_(torch.tensor([30.0, 0.5]))  # what the kernel would leave
    assert float(opt.last_grad_norm) == 30.0 and float(opt.last_clip_coef) == 0.5
    assert opt.last_grad_norm.data_ptr() == kw["clip_out"].data_ptr()  # views, not copies
    # without a scaler the clipped step still runs on the device counter; switching the setting off returns to adam_step_amp
    opt.step()
    assert len(calls.clipped) == 2 and calls.clipped[1]["amp_scale"] is None and calls.clipped[1]["found_inf"] is None
    opt.max_grad_norm = opt.clip_value = None
    opt.step()
    assert len(calls.clipped) == 2 and len(calls.amp) == 1 and not calls.plain
    assert set(opt.state_dict()) == {"state", "param_groups", "flat"}


def test_flat_adam_rejects_both_settings_and_bad_values(monkeypatch):
    from mimo_unet_amd import optim as OP
    calls = _Calls(monkeypatch)
    with pytest.raises(ValueError):
        OP.FlatAdam(_FakeFlatNet(), max_grad_norm=1.0, clip_value=1.0)
    for bad in (0.0, -1.0, float("nan")):
        for name in ("max_grad_norm", "clip_value"):
            with pytest.raises(ValueError):
                OP.FlatAdam(_FakeFlatNet(), **{name: bad})
            opt = OP.FlatAdam(_FakeFlatNet())
            setattr(opt, name, bad)  # plain attributes: checked when the step reads them
            with pytest.raises(ValueError):
                opt.step()
    opt = OP.FlatAdam(_FakeFlatNet(), max_grad_norm=1.0)
    opt.clip_value = 2.0
    with pytest.raises(ValueError):
        opt.step()
    assert not calls.plain and not calls.amp and not calls.clipped


def test_clipped_flat_adam_on_the_reference_follows_torch(monkeypatch):
    """FlatAdam(max_grad_norm) with the engine call replaced by clip_reference: three steps track clip_grad_norm_ + Adam"""
    from mimo_unet_amd import optim as OP

    def fake(p, g, m, v, *, lr, betas, eps, weight_decay, step_dev, reduce_scale, amp_scale, found_inf, clip_mode, clip, clip_out):
        r = G.clip_reference(p, g, m, v, step=int(step_dev.item()) + 1, mode=clip_mode, clip=clip, wd=weight_decay, lr=lr,
                             grad_scale=reduce_scale)
        step_dev += 1
        for k, t in (("p", p), ("m", m), ("v", v)):
            t.copy_(r[k])
        clip_out.copy_(torch.stack([r["norm"], r["coef"]]))

    monkeypatch.setattr(OP, "adam_step_clipped", fake)
    net, ref = _FakeFlatNet(), _FakeFlatNet()
    opt = OP.FlatAdam(net, lr=1e-2, max_grad_norm=0.5)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        gr = torch.randn(10, generator=gen)
        net.grads.copy_(gr)
        ref.a.grad, ref.b.grad = gr[:6].view(2, 3).clone(), gr[6:].clone()
        total = torch.nn.utils.clip_grad_norm_(list(ref.parameters()), 0.5)
        opt.step()
        ropt.step()
        torch.testing.assert_close(opt.last_grad_norm, total, rtol=1e-6, atol=0.0)
    assert opt.step_count == 3
    torch.testing.assert_close(net.flat, ref.flat, rtol=1e-5, atol=1e-7)


# ---- the Lightning hook ----------------------------------------------------------------------------------------------------

def _models():
    from mimo.models.evidential_unet import EvidentialUnetModel
    from mimo.models.mimo_unet import MimoUnetModel
    yield MimoUnetModel(in_channels=2, out_channels=2, num_subnetworks=2, filter_base_count=4, center_dropout_rate=0.0,
                        final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0,
                        loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3, seed=0, loss_buffer_size=10,
                        loss_buffer_temperature=0.3)
    yield EvidentialUnetModel(in_channels=2, out_channels=4, filter_base_count=4, center_dropout_rate=0.0,
                              final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0,
                              weight_decay=0.0, learning_rate=1e-3, seed=0)


class _Wrapper:  # what Lightning hands the hook: a LightningOptimizer around the real one
    def __init__(self, optimizer):
        self.optimizer = optimizer


def test_hook_sets_the_fused_optimizer_and_leaves_others_to_the_base_class():
    from mimo_unet_amd.optim import FlatAdam
    for model in _models():
        assert model.gradient_clip_val is None
        opt = model.configure_optimizers()["optimizer"]
        assert isinstance(opt, FlatAdam)
        grads = []
        for q in model.parameters():
            q.grad = torch.full_like(q, 3.0)
            grads.append(q.grad)
        for algorithm, want in (("norm", (2.0, None)), ("value", (None, 2.0)), (None, (2.0, None))):
            model.configure_gradient_clipping(_Wrapper(opt), gradient_clip_val=2.0, gradient_clip_algorithm=algorithm)
            assert (opt.max_grad_norm, opt.clip_value) == want
        # Lightning calls the hook before every step, with None when the Trainer has no bound: nothing anywhere leaves what
        # the optimiser was given untouched, whichever algorithm the call names; an explicit 0 switches clipping off
        for algorithm in (None, "norm", "value"):
            model.configure_gradient_clipping(opt, gradient_clip_val=None, gradient_clip_algorithm=algorithm)
            assert (opt.max_grad_norm, opt.clip_value) == (2.0, None)
        opt.max_grad_norm, opt.clip_value = None, 1.5  # set on the optimiser by a hand-written loop
        model.configure_gradient_clipping(opt)
        assert (opt.max_grad_norm, opt.clip_value) == (None, 1.5)
        model.configure_gradient_clipping(opt, gradient_clip_val=0.0)
        assert (opt.max_grad_norm, opt.clip_value) == (None, None)
        model.configure_gradient_clipping(opt)
        assert (opt.max_grad_norm, opt.clip_value) == (None, None)
        model.gradient_clip_val = 0.75  # the attribute serves where the Trainer passes nothing
        model.configure_gradient_clipping(opt)
        assert (opt.max_grad_norm, opt.clip_value) == (0.75, None)
        model.configure_gradient_clipping(opt, gradient_clip_val=4.0, gradient_clip_algorithm="value")
        assert (opt.max_grad_norm, opt.clip_value) == (None, 4.0)
        with pytest.raises(ValueError):
            model.configure_gradient_clipping(opt, gradient_clip_val=1.0, gradient_clip_algorithm="agc")
        assert all(q.grad is g and bool((g == 3.0).all()) for q, g in zip(model.parameters(), grads))  # .grad untouched
        # another optimiser goes to the base class's clip_gradients when it has one
        seen = []
        model.use_fused_optimizer = False
        adam = model.configure_optimizers()["optimizer"]
        assert isinstance(adam, torch.optim.Adam)
        from mimo_unet_amd import lightning_compat as LC
        if not LC.HAVE_LIGHTNING:  # (the real clip_gradients needs an attached Trainer)
            model.configure_gradient_clipping(adam, gradient_clip_val=1.0, gradient_clip_algorithm="norm")  # the stand-in has none
            LC.LightningModule.clip_gradients = lambda self, o, gradient_clip_val=None, gradient_clip_algorithm=None: seen.append(
                (o, gradient_clip_val, gradient_clip_algorithm))
            try:
                model.configure_gradient_clipping(adam, gradient_clip_val=1.0, gradient_clip_algorithm="norm")
            finally:
                del LC.LightningModule.clip_gradients
            assert seen == [(adam, 1.0, "norm")]
        assert (opt.max_grad_norm, opt.clip_value) == (None, 4.0) and all(bool((g == 3.0).all()) for g in grads)


def test_grad_norm_is_logged_as_a_copy_however_the_bound_was_set_and_copies_leave_the_optimizer_behind():
    import copy
    import io
    from mimo_unet_amd import lightning_compat as LC
    for model in _models():
        model._log_grad_norm()  # no optimiser yet
        opt = model.configure_optimizers()["optimizer"]
        opt._clip_out = torch.tensor([30.0, 0.5])  # what a clipped step leaves
        if not LC.HAVE_LIGHTNING:  # (the real log() needs an attached Trainer)
            model._log_grad_norm()
            assert "grad_norm" not in model.logged  # clipping by norm is off
            opt.max_grad_norm = 3.0  # set on the optimiser directly: the hook never ran
            model._log_grad_norm()
            opt._clip_out[0] = 7.0  # the next step overwrites the optimiser's scalar, not what was logged
            assert float(model.logged["grad_norm"]) == 30.0
            opt.max_grad_norm, opt.clip_value = None, 3.0  # value mode has no norm
            model.logged.clear()
            model._log_grad_norm()
            assert "grad_norm" not in model.logged
        assert model._flat_adam is opt and copy.deepcopy(model)._flat_adam is None
        buf = io.BytesIO()
        torch.save(model, buf)
        buf.seek(0)
        assert torch.load(buf, weights_only=False)._flat_adam is None and model._flat_adam is opt
        model.use_fused_optimizer = False
        model.configure_optimizers()
        assert model._flat_adam is None  # torch.optim.Adam: Lightning clips it, nothing to log from here


def test_library_binding_declares_the_two_symbols():
    from mimo_unet_amd import _lib
    assert {"mimo_adam_step_clipped", "mimo_grad_clip_scratch_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
