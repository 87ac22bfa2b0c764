"""mimo_adam_step_clipped — global-norm / value clipping fused into the flat Adam step — against tests/grad_clip_reference.py.

Without a measured tolerance: the norm exactly on integer data, within a derived bound on normal draws, bit-identity of two
runs, with mimo_adam_step_amp when clipping is inactive and with mimo_adam_step_amp on a pre-multiplied gradient when it
is active, the coefficient from the reported norm.  Per element against fp64 by the rules of tests/test_scalar_kernels_gpu.py
(4 x the fp32 reference's own distance from fp64, never below 4 ulp).  Every test prints its figures."""
import pytest
import torch

from tests import grad_clip_reference as G
from tests import scalar_reference as R
from tests.helpers import cfg_from_meta, load_npz, report, state_from

pytestmark = pytest.mark.gpu
MIMO_ERR_INVALID = -1
MODES = {"norm": 1, "value": 2}
HYPER = (1e-3, 0.9, 0.999, 1e-8)  # lr, beta1, beta2, eps


def _L():
    from mimo_unet_amd import _lib
    return _lib


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def dev(x):
    return None if x is None else torch.tensor([float(x)], device="cuda")


_scratch = {}


def scratch():
    if "s" not in _scratch:
        nbytes = int(_L().load().mimo_grad_clip_scratch_bytes())
        assert nbytes >= 2048 * 8 + 8
        _scratch["s"] = torch.empty((nbytes + 7) // 8, device="cuda", dtype=torch.float64)
    return _scratch["s"]


def run_clipped(p, g, m, v, *, step, mode, clip, wd=0.0, grad_scale=1.0, amp_scale=None, found_inf=None):
    """mimo_adam_step_clipped on device copies of the CPU tensors -> {p, m, v, step_dev, clip_out} (device tensors)"""
    L = _L()
    o = {"p": p.cuda(), "m": m.cuda(), "v": v.cuda(), "step_dev": torch.tensor([float(step - 1)], device="cuda"),
         "clip_out": torch.full((2,), float("nan"), device="cuda")}
    gd, sc, fi = g.cuda(), dev(amp_scale), dev(found_inf)
    L.check(L.load().mimo_adam_step_clipped(o["p"].data_ptr(), gd.data_ptr(), o["m"].data_ptr(), o["v"].data_ptr(), g.numel(),
                                            *HYPER, wd, o["step_dev"].data_ptr(), grad_scale, L.ptr(sc) or None,
                                            L.ptr(fi) or None, MODES[mode], clip, o["clip_out"].data_ptr(),
                                            scratch().data_ptr(), L.current_stream()), "mimo_adam_step_clipped")
    torch.cuda.synchronize()
    return o


def run_amp(p, g, m, v, *, step, wd=0.0, grad_scale=1.0, amp_scale=None, found_inf=None):
    L = _L()
    o = {"p": p.cuda(), "m": m.cuda(), "v": v.cuda(), "step_dev": torch.tensor([float(step - 1)], device="cuda")}
    gd = g if g.is_cuda else g.cuda()
    sc, fi = dev(amp_scale), dev(found_inf)
    L.check(L.load().mimo_adam_step_amp(o["p"].data_ptr(), gd.data_ptr(), o["m"].data_ptr(), o["v"].data_ptr(), g.numel(),
                                        *HYPER, wd, o["step_dev"].data_ptr(), grad_scale, L.ptr(sc) or None, L.ptr(fi) or None,
                                        L.current_stream()), "mimo_adam_step_amp")
    torch.cuda.synchronize()
    return o


def same_state(a, b, keys=("p", "m", "v", "step_dev")):
    """bit for bit, compared where a's tensors live (no download of the large sizes)"""
    return all(torch.equal(a[k].view(torch.int32), b[k].to(a[k].device).view(torch.int32)) for k in keys)


# ---- the norm -------------------------------------------------------------------------------------------------------------

def test_norm_is_exact_on_integer_data():
    """every g = 2, n = 4^k: the norm is exactly 2 * 2^k; g in {0, 3, -4} with sum g^2 a perfect square: exactly its root
    (squares and their sums are integers below 2^53: no rounding anywhere, whatever the order of the sum)"""
    for name, g, exact in G.integer_gradients():
        z = torch.zeros_like(g)
        o = run_clipped(z, g, z, z, step=1, mode="norm", clip=1e30)
        got = o["clip_out"].cpu()
        report(f"[grad_clip] exact norm {name}: got {float(got[0])!r} want {exact!r} coef {float(got[1])!r}")
        assert float(got[0]) == exact and float(got[1]) == 1.0


@pytest.mark.parametrize("n", G.NORM_SIZES)
def test_norm_within_the_derived_bound_and_coefficient_from_the_reported_norm(n):
    """grad_scale = 0.125, amp_scale = 1024, normal draws.  |norm - norm64| <= 4 * 2^-24 * norm64, derived (squares in fp32,
    the sum in double): rounding of g * s <= 2^-24 on the norm; rounding of the fp32 square <= 2^-24 on the term, 1/2 * 2^-24
    on the norm; the final rounding to fp32 <= 2^-24; the double sum and square root are invisible: below 2.5 * 2^-24 in
    total.  Coefficient: min(1, clip / (norm + 1e-6)) recomputed in double from the REPORTED norm, within 2 * 2^-24 relative
    (the reported norm's rounding and the coefficient's own)."""
    p, g, m, v = G.clip_inputs(n, 1)
    n64 = G.norm64(g, G.NORM_SCALE, G.NORM_AMP)
    for factor in (G.ACTIVE, G.INACTIVE):
        clip = G.clip_for(g, factor, G.NORM_SCALE, G.NORM_AMP)
        o = run_clipped(p, g, m, v, step=1, mode="norm", clip=clip, grad_scale=G.NORM_SCALE, amp_scale=G.NORM_AMP, found_inf=0.0)
        norm, coef = (float(x) for x in o["clip_out"].cpu())
        err = abs(norm - n64) / n64
        want = G.coef_from_reported_norm(norm, clip)
        cerr = abs(coef - want) / want
        report(f"[grad_clip] n={n} clip={factor}x: norm {norm:.9e} fp64 {n64:.9e} rel err {err / 2 ** -24:.3f} x 2^-24 (bound 4); "
               f"coef {coef:.9e} from reported norm {want:.9e} rel err {cerr / 2 ** -24:.3f} x 2^-24 (bound 2)")
        assert err <= G.NORM_BOUND and cerr <= G.COEF_BOUND
        assert (coef == 1.0) == (factor == G.INACTIVE) and float(o["step_dev"]) == 1.0


@pytest.mark.parametrize("n", [1027, 2097159, G.LOOP_SIZE])
def test_two_runs_give_the_same_bits(n):
    p, g, m, v = G.clip_inputs(n, 2)
    clip = G.clip_for(g, G.ACTIVE, 1.0 / 3.0)
    a = run_clipped(p, g, m, v, step=2, mode="norm", clip=clip, wd=1e-2, grad_scale=1.0 / 3.0)
    scratch().fill_(float("nan"))  # nothing may be carried over in the scratch
    b = run_clipped(p, g, m, v, step=2, mode="norm", clip=clip, wd=1e-2, grad_scale=1.0 / 3.0)
    assert same_state(a, b, ("p", "m", "v", "step_dev", "clip_out")) and not torch.equal(bits(a["p"]), bits(p))


# ---- bit-identity with the existing step ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", G.NORM_SIZES)
def test_inactive_clipping_is_bit_identical_to_the_amp_step(n):
    """clip = 100 x norm: coefficient 1, and p, m, v, step_dev equal mimo_adam_step_amp's on copies bit for bit; value mode
    with a bound no element reaches likewise"""
    for step, wd, amp in G.identity_cases(n):
        p, g, m, v = G.clip_inputs(n, step)
        gs = g if amp is None else g * amp
        kw = dict(step=step, wd=wd, grad_scale=1.0, amp_scale=amp, found_inf=None if amp is None else 0.0)
        want = run_amp(p, gs, m, v, **kw)
        got = run_clipped(p, gs, m, v, mode="norm", clip=G.clip_for(gs, G.INACTIVE, 1.0, amp), **kw)
        assert float(got["clip_out"][1]) == 1.0 and float(got["step_dev"]) == float(step)
        assert same_state(got, want), f"norm mode n={n} step={step} wd={wd} amp={amp}"
        got = run_clipped(p, gs, m, v, mode="value", clip=1e30, **kw)
        assert [float(x) for x in got["clip_out"]] == [0.0, 1.0]
        assert same_state(got, want), f"value mode n={n} step={step} wd={wd} amp={amp}"
    report(f"[grad_clip] n={n}: inactive clipping bit-identical to mimo_adam_step_amp over {len(G.identity_cases(n))} cases x 2 modes")


@pytest.mark.parametrize("n", G.NORM_SIZES)
def test_active_clipping_is_bit_identical_to_the_amp_step_on_a_premultiplied_gradient(n):
    """clip = norm / 10: p, m, v equal mimo_adam_step_amp(grad_scale = 1) on the gradient (g * s) * clip_out[1], formed in
    torch fp32 with the same two multiplications (s: the fp32 quotient the kernel uses); value mode: on clamp(g * s)"""
    for step, wd, amp in G.identity_cases(n):
        p, g, m, v = G.clip_inputs(n, step)
        gs_arg = 1.0 / 3.0
        gsc = g if amp is None else g * amp
        s = torch.tensor(G.effective_scale(gs_arg, amp), dtype=torch.float32, device="cuda")
        kw = dict(step=step, wd=wd, grad_scale=gs_arg, amp_scale=amp, found_inf=None if amp is None else 0.0)
        got = run_clipped(p, gsc, m, v, mode="norm", clip=G.clip_for(gsc, G.ACTIVE, gs_arg, amp), **kw)
        coef = got["clip_out"][1]
        assert 0.05 < float(coef) < 0.2
        want = run_amp(p, (gsc.cuda() * s) * coef, m, v, step=step, wd=wd)
        assert same_state(got, want), f"norm mode n={n} step={step} wd={wd} amp={amp}"
        got = run_clipped(p, gsc, m, v, mode="value", clip=R.f32(G.VALUE_CLIP), **kw)
        want = run_amp(p, (gsc.cuda() * s).clamp(-R.f32(G.VALUE_CLIP), R.f32(G.VALUE_CLIP)), m, v, step=step, wd=wd)
        assert same_state(got, want), f"value mode n={n} step={step} wd={wd} amp={amp}"
    report(f"[grad_clip] n={n}: active clipping bit-identical to mimo_adam_step_amp on the pre-multiplied / clamped gradient")


@pytest.mark.parametrize("n", G.OPPOSED_SIZES)
def test_active_clipping_is_bit_identical_where_weight_decay_opposes_the_gradient(n):
    """the unsigned draw of tests/scalar_reference.py (p's sign independent of g's: wd * p opposes the clipped gradient at half
    the elements, and nearly cancels it at some), weight decay 1e-2, clipping 10-fold: identity with mimo_adam_step_amp on
    the pre-multiplied gradient does not depend on the conditioning of that sum, so it needs no tolerance"""
    p, g, m, v = R.adam_inputs(n, 2)
    opposed = int(((p * g) < 0).sum())
    assert 0.4 * n < opposed < 0.6 * n
    gs_arg = 1.0 / 3.0
    s = torch.tensor(G.effective_scale(gs_arg), dtype=torch.float32, device="cuda")
    got = run_clipped(p, g, m, v, step=2, mode="norm", clip=G.clip_for(g, G.ACTIVE, gs_arg), wd=1e-2, grad_scale=gs_arg)
    coef = got["clip_out"][1]
    assert 0.05 < float(coef) < 0.2
    want = run_amp(p, (g.cuda() * s) * coef, m, v, step=2, wd=1e-2)
    assert same_state(got, want)
    got = run_clipped(p, g, m, v, step=2, mode="value", clip=R.f32(G.VALUE_CLIP), wd=1e-2, grad_scale=gs_arg)
    want = run_amp(p, (g.cuda() * s).clamp(-R.f32(G.VALUE_CLIP), R.f32(G.VALUE_CLIP)), m, v, step=2, wd=1e-2)
    assert same_state(got, want)
    report(f"[grad_clip] n={n}: bit-identical with wd * p opposing the clipped gradient at {opposed} elements")


# ---- per element against fp64 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", G.SIZES)
def test_clipped_step_per_element_against_fp64(n):
    """p, m, v after steps 1, 2 and 1000, norm mode clipping 10-fold and value mode, weight decay 0 and 1e-2: 4 x the fp32
    reference's distance from fp64, never below 4 ulp; the worst ratio of each case is printed"""
    worst = {}
    for step, wd, mode, gs in G.per_element_cases(n):
        p, g, m, v = G.clip_inputs(n, step)
        clip = G.clip_for(g, G.ACTIVE, gs) if mode == "norm" else R.f32(G.VALUE_CLIP)
        ref_fn = lambda p_, g_, m_, v_: {k: t for k, t in G.clip_reference(
            p_, g_, m_, v_, step=step, mode=mode, clip=clip, wd=wd, grad_scale=gs).items() if k in ("p", "m", "v")}
        ref = ref_fn(p.double(), g.double(), m.double(), v.double())
        fl = R.adam_floors(p, ref)
        y, _, bad = R.yardstick(ref_fn, [p, g, m, v], fl)
        assert not any(bool(b.any()) for b in bad.values())
        got = run_clipped(p, g, m, v, step=step, mode=mode, clip=clip, wd=wd, grad_scale=gs)
        assert float(got["step_dev"]) == float(step)
        for k in ("p", "m", "v"):
            r = R.check("adam_step_clipped", f"n={n} {mode} wd={wd} gs={gs:.3f} step={step} {k}", got[k], ref[k],
                        R._floor_of(fl, k, ref[k]), y[k])
            worst[(mode, wd)] = max(worst.get((mode, wd), 0.0), r)
    report(f"[grad_clip] n={n}: worst error / yardstick per (mode, weight decay) {worst}")


# ---- skips and invalid arguments -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 2097159])
@pytest.mark.parametrize("what", ["inf", "nan", "found_inf"])
def test_skipped_steps_leave_the_state_untouched(n, what):
    """one inf in g without a scaler, one NaN in g, found_inf = 1 with a finite gradient: p, m, v and step_dev bit-unchanged;
    clip_out written all the same, its norm not finite in the first two"""
    p, g, m, v = G.clip_inputs(n, 2)
    g = g.clone()
    if what != "found_inf":
        g[n - 2] = float(what)
    o = run_clipped(p, g, m, v, step=2, mode="norm", clip=1.0, wd=1e-2, found_inf=1.0 if what == "found_inf" else None)
    norm, coef = (float(x) for x in o["clip_out"].cpu())
    report(f"[grad_clip] skip ({what}) n={n}: clip_out = [{norm}, {coef}]")
    assert same_state(o, {"p": p, "m": m, "v": v, "step_dev": torch.tensor([1.0])}), "a skipped step wrote state"
    if what == "found_inf":
        assert abs(norm - G.norm64(g)) <= G.NORM_BOUND * G.norm64(g)
        assert abs(coef - G.coef_from_reported_norm(norm, 1.0)) <= G.COEF_BOUND * coef
    else:
        assert not torch.isfinite(torch.tensor(norm)) and coef == 0.0
    if what == "inf":  # value mode has no norm: an inf is clamped like any value, as torch does
        o = run_clipped(p, g, m, v, step=2, mode="value", clip=0.5)
        assert float(o["step_dev"]) == 2.0 and bool(torch.isfinite(o["p"]).all())


BAD_ARGS = [dict(p=0), dict(g=0), dict(m=0), dict(v=0), dict(step_dev=0), dict(clip_out=0), dict(scratch=0), dict(n=-1),
            dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan")), dict(mode=0), dict(mode=3)]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=str)
def test_invalid_arguments_are_rejected_and_nothing_is_launched(bad):
    L = _L()
    lib = L.load()
    n = 5
    t = {k: torch.full((n,), 1.5, device="cuda") for k in ("p", "g", "m", "v")}
    t["step_dev"], t["clip_out"] = torch.tensor([3.0], device="cuda"), torch.full((2,), 7.0, device="cuda")
    before = {k: x.clone() for k, x in t.items()}
    a = {k: x.data_ptr() for k, x in t.items()}
    a.update(scratch=scratch().data_ptr(), n=n, clip=1.0, mode=1)
    a.update({k: (None if k in ("p", "g", "m", "v", "step_dev", "clip_out", "scratch") else x) for k, x in bad.items()})
    rc = lib.mimo_adam_step_clipped(a["p"], a["g"], a["m"], a["v"], a["n"], *HYPER, 0.0, a["step_dev"], 1.0, None, None, a["mode"],
                                    a["clip"], a["clip_out"], a["scratch"], L.current_stream())
    torch.cuda.synchronize()
    assert rc == MIMO_ERR_INVALID and b"mimo_adam_step_clipped" in lib.mimo_last_error()
    assert all(torch.equal(bits(t[k]), bits(before[k])) for k in t)


# ---- through the model ---------------------------------------------------------------------------------------------------

def _mini_model(precision):
    from tests.test_network_gpu import build_model
    fx = load_npz("mini_s2_step.npz")
    model = build_model(cfg_from_meta(fx["meta"]), state_from(fx, "init/"), precision=precision, lr=1e-3)
    model.train()
    return model, [torch.from_numpy(fx[f"s0/{k}"]).cuda() for k in ("image", "label", "perms")]


def test_three_clipped_training_steps_through_the_model():
    """mini S = 2 geometry, FlatAdam(max_grad_norm = a tenth of the first step's norm) set through the model's hook:
    last_grad_norm within the derived bound of the fp64 norm of the flat gradient; the parameters after every step bit-identical
    to a second model stepped with the pre-multiplied flat gradient through adam_step_amp; grad_norm logged from the device"""
    from mimo_unet_amd.engine import adam_step_amp
    model, (image, label, perms) = _mini_model("split16")
    twin, _ = _mini_model("split16")
    opt = model.configure_optimizers()["optimizer"]
    m2 = v2 = None
    step2 = torch.zeros(1, device="cuda")
    for it in range(3):
        for mod in (model, twin):
            for q in mod.parameters():
                q.grad = None
            mod.training_step_with_perms(image, label, None, perms)["loss"].backward()
        g = model.model.flat_gradients()
        n64 = float(torch.linalg.vector_norm(g.double()))
        if it == 0:
            assert "grad_norm" not in model.logged
            model.configure_gradient_clipping(opt, gradient_clip_val=n64 / 10.0, gradient_clip_algorithm="norm")
            assert opt.max_grad_norm == n64 / 10.0
        else:
            assert model.logged["grad_norm"].is_cuda and float(model.logged["grad_norm"]) == last_norm
        g_before = g.clone()
        opt.step()
        if it > 0:  # a copy was logged: the step that followed did not change it
            assert float(model.logged["grad_norm"]) == last_norm
        assert torch.equal(bits(g), bits(g_before)), "the step must not write the gradient"
        last_norm, coef = float(opt.last_grad_norm), opt.last_clip_coef
        err = abs(last_norm - n64) / n64
        report(f"[grad_clip] model step {it + 1}: n={g.numel()} norm {last_norm:.9e} fp64 {n64:.9e} rel err {err / 2 ** -24:.3f} x 2^-24 "
               f"coef {float(coef):.6f}")
        assert err <= G.NORM_BOUND
        assert abs(float(coef) - G.coef_from_reported_norm(last_norm, opt.max_grad_norm)) <= G.COEF_BOUND * float(coef)
        assert float(coef) < 1.0 and opt.step_count == it + 1
        p2, g2 = twin.model.flat_parameters(), twin.model.flat_gradients()
        g2.copy_((g * 1.0) * coef)
        if m2 is None:
            m2, v2 = torch.zeros_like(p2), torch.zeros_like(p2)
        adam_step_amp(p2, g2, m2, v2, lr=1e-3, step_dev=step2)
        twin.model.mark_parameters_changed()
        torch.cuda.synchronize()
        assert torch.equal(bits(model.model.flat_parameters()), bits(p2)), f"step {it + 1}: parameters differ from the twin's"
        assert torch.equal(bits(opt._m), bits(m2)) and torch.equal(bits(opt._v), bits(v2))


def test_clipped_training_under_torch_grad_scaler_skips_an_overflow_and_clips_the_next_step():
    """precision "16-mixed" under torch's GradScaler, as test_fp16_mixed_training_under_torch_grad_scaler sets it up, with
    max_grad_norm: three scaled steps clip; a scale of 2^40 overflows fp16 — parameters and step count untouched, scale
    halved; the normal step that follows clips again"""
    model, (image, label, perms) = _mini_model("16-mixed")
    opt = model.configure_optimizers()["optimizer"]
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 12, growth_interval=2)

    def step(sc):
        opt.zero_grad()
        sc.scale(model.training_step_with_perms(image, label, None, perms)["loss"]).backward()
        sc.step(opt)
        sc.update()

    opt.zero_grad()
    model.training_step_with_perms(image, label, None, perms)["loss"].backward()
    n0 = float(torch.linalg.vector_norm(model.model.flat_gradients().double()))
    model.configure_gradient_clipping(opt, gradient_clip_val=n0 / 10.0)
    for it in range(3):
        step(scaler)
        norm, coef = float(opt.last_grad_norm), float(opt.last_clip_coef)
        report(f"[grad_clip] 16-mixed + GradScaler step {it + 1}: unscaled norm {norm:.6e} (first step, unscaled backward: {n0:.6e}) coef {coef:.6f}")
        assert opt.step_count == it + 1 and 0.0 < coef < 1.0
        assert abs(coef - G.coef_from_reported_norm(norm, opt.max_grad_norm)) <= G.COEF_BOUND * coef
        # the loss scale (2^12, then 2^13) was divided out before the norm was taken: step 1 sees the parameters and the batch of
        # the unscaled backward above, so its norm is n0 up to fp16 rounding (a factor 2 is generous); two steps of lr = 1e-3
        # later it is still of n0's order (a factor 16), where the scaled gradient's would be 4096 x n0
        assert n0 / 16.0 < norm < 16.0 * n0 and (it > 0 or n0 / 2.0 < norm < 2.0 * n0)
    assert scaler.get_scale() == 2.0 ** 13
    before, steps_before = model.model.flat_parameters().clone(), opt.step_count
    m_before = opt._m.clone()
    big = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    step(big)
    assert torch.equal(bits(model.model.flat_parameters()), bits(before)) and torch.equal(bits(opt._m), bits(m_before))
    assert opt.step_count == steps_before and big.get_scale() == 2.0 ** 39
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    step(scaler)
    assert opt.step_count == steps_before + 1 and not torch.equal(bits(model.model.flat_parameters()), bits(before))
    assert 0.0 < float(opt.last_clip_coef) < 1.0 and bool(torch.isfinite(opt.last_grad_norm))
