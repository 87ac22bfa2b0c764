"""The plan-free scalar kernels — mimo_loss_buffer_step, mimo_adam_step(_amp), mimo_uncertainties, the validation / training
epilogues and the four evidential entry points — per element against the fp64 references of tests/scalar_reference.py, at
sizes that run every grid-stride loop a second time.  Bounds (scalar_reference.py): elem_err <= 4 x the yardstick (the fp32
torch reference's own distance from fp64 on the same input), never below 4 fp32 ulp; where the fp32 reference is not finite
(evidential, alpha >= 35) 8 x the conditioning of the result under one fp32 ulp of each logit; reduced scalars 4 x the
yardstick of their per-element terms plus the final float conversion.  Every output buffer starts NaN-filled.  Each test
reports its errors, yardsticks and their ratio."""
import pytest
import torch

from tests import scalar_reference as R
from tests.helpers import report
from tests.test_scalar_reference_cpu import TRAINING_SHAPES, UNCERTAINTY_SHAPES, VALIDATION_SHAPES

pytestmark = pytest.mark.gpu
NAN = float("nan")
MIMO_ERR_INVALID = -1
KINDS = ["laplace_nll", "gaussian_nll"]


def _L():
    from mimo_unet_amd import _lib
    return _lib


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def written(*tensors):
    assert all(not bool(torch.isnan(t).any()) for t in tensors), "an output buffer was not fully overwritten"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- loss buffer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", R.LOSS_BUFFER_T)
@pytest.mark.parametrize("size", R.LOSS_BUFFER_SIZES)
@pytest.mark.parametrize("S", R.LOSS_BUFFER_S)
def test_loss_buffer_step_kernel_over_a_wrapping_ring(S, size, T):
    """mimo_loss_buffer_step called directly for 25 successive steps (a ring of 10 wraps twice): weights, weights / S and both
    scalars after every step against the fp64 O.LossBuffer (weights read first, loss added afterwards); the written row equals
    the loss bit for bit, every other row is bit-unchanged.  The yardstick is pooled over the 25 steps (one step of S <= 3
    holds too few elements for a maximum to mean anything); the two scalars are fp32 sums over <= 64 lanes here, so they are
    bounded like per-element outputs, by their own yardstick."""
    L = _L()
    lib = L.load()
    losses = R.loss_buffer_losses(S, size, T)
    y, ref, _ = R.yardstick(lambda l: R.loss_buffer_sequence(l, S, T, size), [losses], R.loss_buffer_floors(losses))
    ring = torch.zeros(size, S, device="cuda")
    got = {k: [] for k in ("weights", "w_over_s", "weighted", "mean")}
    ld = losses.cuda()
    for i in range(R.LOSS_BUFFER_STEPS):
        before = ring.clone()
        w, ws, sc = nans(S), nans(S), nans(2)
        L.check(lib.mimo_loss_buffer_step(ring.data_ptr(), size, i % size, S, T, ld[i].data_ptr(), w.data_ptr(), ws.data_ptr(),
                                          sc.data_ptr(), L.current_stream()), "mimo_loss_buffer_step")
        torch.cuda.synchronize()
        written(w, ws, sc)
        assert torch.equal(bits(ring[i % size]), bits(losses[i])), "the written row must be the loss bit for bit"
        keep = torch.arange(size) != i % size
        assert torch.equal(bits(ring.cpu()[keep]), bits(before.cpu()[keep])), "rows other than `index` must stay untouched"
        assert torch.equal(bits(ring), bits(ref["ring"][i].float()))
        for k, v in (("weights", w), ("w_over_s", ws), ("weighted", sc[0]), ("mean", sc[1])):
            got[k].append(v.cpu())
    fl = R.loss_buffer_floors(losses)
    for k in got:
        R.check("loss_buffer_step", f"S={S} size={size} T={T} {k}", torch.stack(got[k]), ref[k], fl[k], y[k])


@pytest.mark.parametrize("S,size,T", [(3, 10, 0.3), (64, 10, 0.01), (2, 1, 0.3)])
def test_loss_buffer_class_step_gradient_and_index(S, size, T):
    """LossBuffer.step on the model's class over the same sequences: the returned weighted mean, weights and mean, the
    gradient of the weighted mean w.r.t. `loss` through autograd (= weights / S, scaled by the upstream gradient) and the
    index bookkeeping, against the fp64 reference."""
    from mimo.models.mimo_components.loss_buffer import LossBuffer
    losses = R.loss_buffer_losses(S, size, T)
    y, ref, _ = R.yardstick(lambda l: R.loss_buffer_sequence(l, S, T, size), [losses], R.loss_buffer_floors(losses))
    fl = R.loss_buffer_floors(losses)
    lb = LossBuffer(S, T, size)
    got = {k: [] for k in ("weights", "w_over_s", "weighted", "mean")}
    for i in range(R.LOSS_BUFFER_STEPS):
        l = losses[i].cuda().requires_grad_(True)
        res = lb.step(l)
        assert res is not None and lb.index == (i + 1) % size
        total, w, mean = res
        assert not w.requires_grad and not mean.requires_grad
        (total * 3.0).backward()
        for k, v in (("weights", w), ("w_over_s", l.grad / 3.0), ("weighted", total), ("mean", mean)):
            got[k].append(v.detach().cpu())
    assert torch.equal(bits(lb.buffer), bits(ref["ring"][-1].float()))
    for k in got:
        R.check("loss_buffer_step", f"LossBuffer.step S={S} size={size} T={T} {k}", torch.stack(got[k]), ref[k], fl[k], y[k])


def test_loss_buffer_step_declines_what_the_kernel_does_not_cover():
    from mimo.models.mimo_components.loss_buffer import LossBuffer
    assert LossBuffer(65, 0.3, 10).step(torch.zeros(65, device="cuda")) is None       # more than one wave of subnetworks
    assert LossBuffer(3, 0.3, 10).step(torch.zeros(3)) is None                           # a host tensor
    assert LossBuffer(3, 0.3, 0).step(torch.zeros(3, device="cuda")) is None             # a zero-size ring
    lb = LossBuffer(3, 0.3, 10)
    lb.get_weights = lambda: torch.ones(3)
    assert lb.step(torch.zeros(3, device="cuda")) is None and lb.index == 0               # get_weights replaced on the instance
    assert float(lb.buffer.abs().max()) == 0.0


@pytest.mark.parametrize("bad", [dict(S=0), dict(S=65), dict(index=10), dict(T=0.0), dict(T=NAN)], ids=str)
def test_loss_buffer_step_rejects_invalid_arguments_and_writes_nothing(bad):
    L = _L()
    lib = L.load()
    a = dict(S=3, index=2, T=0.3)
    a.update(bad)
    ring = torch.arange(10 * 65, device="cuda", dtype=torch.float32).view(10, 65)
    before = ring.clone()
    loss, w, ws, sc = torch.ones(65, device="cuda"), nans(65), nans(65), nans(2)
    rc = lib.mimo_loss_buffer_step(ring.data_ptr(), 10, a["index"], a["S"], a["T"], loss.data_ptr(), w.data_ptr(), ws.data_ptr(),
                                   sc.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    assert rc == MIMO_ERR_INVALID
    assert bool(torch.isnan(w).all() and torch.isnan(ws).all() and torch.isnan(sc).all()) and torch.equal(bits(ring), bits(before))


def _logged_sequence(fused, monkeypatch):
    """train_loss / train_loss_i / train_weight_i logged by six training steps of a small S = 2 model"""
    import mimo_unet_amd.models.mimo_components.loss_buffer as LB
    from oracle import mimo_oracle as O
    from tests.test_network_gpu import build_model
    monkeypatch.setattr(LB, "_FUSED_STEP", fused)
    cfg = O.NetConfig(in_channels=3, out_channels=2, num_subnetworks=2, filter_base_count=4)
    model = build_model(cfg, O.init_state(cfg, 0), T=0.01)
    model.loss_buffer.buffer_size, model.loss_buffer.buffer = 4, torch.zeros(4, 2)  # wraps within the six steps
    model.train()
    g = torch.Generator().manual_seed(2)
    rows = []
    for _ in range(6):
        image, label = torch.rand(2, 3, 32, 32, generator=g).cuda(), torch.rand(2, 1, 32, 32, generator=g).cuda() * 3
        model.training_step_with_perms(image, label, None, O.draw_perms(2, 2, generator=g).cuda())
        rows.append({k: float(v) for k, v in model.logged.items() if k.startswith(("train_loss", "train_weight"))})
    return rows


def test_fused_loss_buffer_step_logs_what_the_tensor_operations_log(monkeypatch):
    """MimoUnetModel.training_step with the fused kernel against the [S]-sized torch operations it replaces (_FUSED_STEP off):
    the logged train_weight_* and train_loss of both stay within the bound of the fp64 O.LossBuffer fed the logged losses."""
    on, off = _logged_sequence(True, monkeypatch), _logged_sequence(False, monkeypatch)
    losses = torch.tensor([[r["train_loss_0"], r["train_loss_1"]] for r in on])
    assert torch.equal(losses, torch.tensor([[r["train_loss_0"], r["train_loss_1"]] for r in off]))  # the same forward
    y, ref, _ = R.yardstick(lambda l: R.loss_buffer_sequence(l, 2, 0.01, 4), [losses], R.loss_buffer_floors(losses))
    fl = R.loss_buffer_floors(losses)
    for name, rows in (("fused", on), ("tensor operations", off)):
        w = torch.tensor([[r["train_weight_0"], r["train_weight_1"]] for r in rows])
        R.check("loss_buffer_step", f"logged train_weight ({name})", w, ref["weights"], fl["weights"], y["weights"])
        R.check("loss_buffer_step", f"logged train_loss ({name})", torch.tensor([r["train_loss"] for r in rows]), ref["mean"],
                fl["mean"], y["mean"])


# ---- Adam --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_step_and_amp_step_per_element(n):
    """mimo_adam_step and mimo_adam_step_amp (found_inf NULL, 0 and 1; amp_scale NULL and 1024) against O.adam_update in fp64:
    n around the float4 body / scalar tail split and one element group past a grid pass; weight decay 0 and 1e-2, grad_scale 1
    and 1/3, steps 1, 2 and 100000 (the amp variant derives the bias corrections from powf on the device-side counter).  With
    found_inf = 1 state and counter stay bit-unchanged; otherwise step_dev advances by exactly 1."""
    L = _L()
    lib = L.load()
    st = L.current_stream()
    worst = {}
    for wd, gs, step in (R.ADAM_HYPER if n < 100 else R.ADAM_HYPER_LARGE):
        p, g, m, v = R.adam_inputs(n, step)
        ref_fn = lambda p_, g_, m_, v_: R.adam_reference(p_, g_, m_, v_, step=step, wd=wd, grad_scale=gs)
        ref = ref_fn(p.double(), g.double(), m.double(), v.double())
        fl = R.adam_floors(p, ref)
        y, _, bad = R.yardstick(ref_fn, [p, g, m, v], fl)
        assert not any(bool(b.any()) for b in bad.values())
        for variant in ("plain", "amp", "amp found_inf=0 scale=1024", "amp found_inf=1"):
            pd, gd, md, vd = p.cuda(), g.cuda(), m.cuda(), v.cuda()
            args = (pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, wd)
            if variant == "plain":
                L.check(lib.mimo_adam_step(*args, step, gs, st), "mimo_adam_step")
            else:
                step_dev = torch.tensor([float(step - 1)], device="cuda")
                found = None if variant == "amp" else torch.tensor([1.0 if variant.endswith("=1") else 0.0], device="cuda")
                scale = torch.tensor([1024.0], device="cuda") if "scale" in variant else None
                gscale = R.f32(gs) * 1024.0 if scale is not None else gs  # (x 1024 is exact: the kernel divides it out again)
                L.check(lib.mimo_adam_step_amp(*args, step_dev.data_ptr(), gscale, L.ptr(scale) or None, L.ptr(found) or None, st),
                        "mimo_adam_step_amp")
                torch.cuda.synchronize()
                if variant.endswith("=1"):
                    assert float(step_dev) == float(step - 1)
                    assert all(torch.equal(bits(a), bits(b)) for a, b in ((pd, p), (md, m), (vd, v))), "skipped step wrote state"
                    continue
                assert float(step_dev) == float(step), "step_dev must advance by exactly 1"
            torch.cuda.synchronize()
            for k, t in (("p", pd), ("m", md), ("v", vd)):
                name = "adam_step" if variant == "plain" else "adam_step_amp"
                r = R.check(name, f"n={n} wd={wd} gs={gs:.3f} step={step} [{variant}] {k}", t, ref[k], R._floor_of(fl, k, ref[k]), y[k])
                worst[name] = max(worst.get(name, 0.0), r)
    report(f"[adam] n={n}: worst error / yardstick {worst}")


# ---- uncertainties and the epilogues: one element past a grid pass, and Ct = 3 with odd hw ----------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", UNCERTAINTY_SHAPES, ids=str)
def test_uncertainties_per_element(shape, kind):
    L = _L()
    lib = L.load()
    N, S, C, hw = shape
    p1, p2 = R.uncertainty_inputs(N, S, C, hw, 13)
    y, ref, bad = R.yardstick(R.uncertainties_reference(kind), [p1, p2], R.UNCERTAINTY_FLOORS)
    assert not any(bool(b.any()) for b in bad.values())
    a, b = p1.cuda(), p2.cuda()
    outs = {k: nans(N, C, 1, hw) for k in ("mean", "aleatoric_var", "epistemic_var")}
    L.check(lib.mimo_uncertainties(a.data_ptr(), b.data_ptr(), N, S, C, hw, L.LOSS_KINDS[kind], outs["mean"].data_ptr(),
                                   outs["aleatoric_var"].data_ptr(), outs["epistemic_var"].data_ptr(), L.current_stream()))
    torch.cuda.synchronize()
    written(*outs.values())
    for k, t in outs.items():
        R.check("uncertainties", f"{shape} {kind} {k}", t, ref[k], R._floor_of(R.UNCERTAINTY_FLOORS, k, ref[k]), y[k])


def _check_regression_scalars(kernel, tag, sc, names, ref, y, floors, label_t):
    """mae / mse / rmse / r2 / count of an epilogue against the fp64 sums of the fp64 terms"""
    want = R.regression_scalars(ref, label_t)
    fa, fs = R._floor_of(floors, "abs_err", ref["abs_err"]), R._floor_of(floors, "sq_err", ref["sq_err"])
    sa, ss = R.term_scale(ref["abs_err"], fa), R.term_scale(ref["sq_err"], fs)
    got = {k: float(sc[i]) for i, k in enumerate(names)}
    R.check_scalar(kernel, f"{tag} mae", got["mae"], want["mae"], y["abs_err"], sa)
    R.check_scalar(kernel, f"{tag} mse", got["mse"], want["mse"], y["sq_err"], ss)
    R.check_scalar(kernel, f"{tag} rmse", got["rmse"], want["rmse"], y["sq_err"], 0.5 * ss / want["rmse"])  # d sqrt(x) = dx / (2 sqrt x)
    # r2 = 1 - SSE / SS_tot: SS_tot comes from exact inputs in double; SSE carries the terms' error
    R.check_scalar(kernel, f"{tag} r2", got["r2"], want["r2"], y["sq_err"], want["sse_over_ss_tot"] * ss / want["mse"])
    assert got["count"] == want["count"]
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", VALIDATION_SHAPES, ids=str)
def test_validation_epilogue_per_element(shape, kind):
    """N = 1, Ct = 1, hw = 262144 + 259 (one element group past the 1024-workgroup pass; the finalize kernel walks 1024 partial
    rows) and Ct = 3 with hw = 63 (the `r % hw` mask index), clamp-edge logits in the first and last elements, a mask with a
    whole image zero: all four maps per element and all eight scalars."""
    L = _L()
    lib = L.load()
    from mimo_unet_amd.engine import VAL_SCALARS
    N, S, Ct, hw = shape
    out, label, mask = R.validation_inputs(N, S, Ct, hw, 11)
    y, ref, bad = R.yardstick(R.validation_reference(kind), [out, label, mask], R.VALIDATION_FLOORS)
    assert not any(bool(b.any()) for b in bad.values())
    od, ld, md = out.cuda(), label.cuda(), mask.cuda()
    maps = {k: nans(N, Ct, 1, hw) for k in ("mean", "aleatoric_std", "epistemic_std", "err")}
    sc, scratch = nans(8), nans(1024 * 8, dtype=torch.float64)
    L.check(lib.mimo_validation_epilogue(od.data_ptr(), ld.data_ptr(), md.data_ptr(), N, S, Ct, hw, L.LOSS_KINDS[kind], R.EPS_MIN,
                                         R.EPS_MAX, maps["mean"].data_ptr(), maps["aleatoric_std"].data_ptr(),
                                         maps["epistemic_std"].data_ptr(), maps["err"].data_ptr(), sc.data_ptr(), scratch.data_ptr(),
                                         1024, L.current_stream()), "mimo_validation_epilogue")
    torch.cuda.synchronize()
    written(sc, *maps.values())
    fl = lambda k: R._floor_of(R.VALIDATION_FLOORS, k, ref[k])
    for k, t in maps.items():
        R.check("validation_epilogue", f"{shape} {kind} {k}", t, ref[k], fl(k), y[k])
    got = _check_regression_scalars("validation_epilogue", f"{shape} {kind}", sc.cpu(), VAL_SCALARS, ref, y, R.VALIDATION_FLOORS, label)
    for name, term in (("nll_combined", "nll"), ("aleatoric_std_mean", "aleatoric_clip"), ("epistemic_std_mean", "epistemic_clip")):
        R.check_scalar("validation_epilogue", f"{shape} {kind} {name}", got[name], float(ref[term].mean()), y[term],
                       R.term_scale(ref[term], fl(term)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", TRAINING_SHAPES, ids=str)
def test_training_epilogue_per_element(shape, kind):
    """total = 524288 + 262 with S = 3, a permutation and reps = 2 (past the 2048-workgroup pass), and Ct = 3 with
    hw = 63: the gathered labels and predictions bit for bit, std and error map per element, the five scalars."""
    L = _L()
    lib = L.load()
    from mimo_unet_amd.engine import TRAIN_SCALARS
    N0, reps, S, Ct, hw = shape
    N = N0 * reps
    out, label, perms = R.training_inputs(N0, reps, S, Ct, hw, 12)
    y, ref, bad = R.yardstick(R.training_reference(kind), [out, label, perms], R.TRAINING_FLOORS)
    assert not any(bool(b.any()) for b in bad.values())
    od, ld, pd = out.cuda(), label.cuda(), perms.cuda()
    maps = {k: nans(N, S, Ct, 1, hw) for k in ("label_t", "preds", "aleatoric_std", "err")}
    sc, scratch = nans(5), nans(2048 * 8, dtype=torch.float64)
    L.check(lib.mimo_training_epilogue(od.data_ptr(), ld.data_ptr(), pd.data_ptr(), N, S, Ct, hw, L.LOSS_KINDS[kind],
                                       maps["label_t"].data_ptr(), maps["preds"].data_ptr(), maps["aleatoric_std"].data_ptr(),
                                       maps["err"].data_ptr(), sc.data_ptr(), scratch.data_ptr(), 2048, L.current_stream()),
            "mimo_training_epilogue")
    torch.cuda.synchronize()
    written(sc, *maps.values())
    assert torch.equal(bits(maps["label_t"]), bits(ref["label_t"].float())) and torch.equal(bits(maps["preds"]), bits(ref["preds"].float()))
    for k in ("aleatoric_std", "err"):
        R.check("training_epilogue", f"{shape} {kind} {k}", maps[k], ref[k], R._floor_of(R.TRAINING_FLOORS, k, ref[k]), y[k])
    _check_regression_scalars("training_epilogue", f"{shape} {kind}", sc.cpu(), TRAIN_SCALARS, ref, y, R.TRAINING_FLOORS, ref["label_t"])


# ---- evidential --------------------------------------------------------------------------------------------------------------

def _run_evidential(lg, y, mk, d_loss, d_ev):
    """the four entry points on logits [N,4,hw]: NIG parameters, loss map, the three backward variants, the loss gradient for a
    constant upstream gradient (and the backward with that constant as a tensor), the three uncertainty maps"""
    L = _L()
    lib = L.load()
    st = L.current_stream()
    N, _, hw = lg.shape
    lgd, yd, mkd, dl, de = (t.cuda().contiguous() for t in (lg, y, mk, d_loss, d_ev))
    o = {"ev": nans(N, 4, hw), "loss": nans(N, hw), "mean": nans(N, hw), "aleatoric_var": nans(N, hw), "epistemic_var": nans(N, hw)}
    o.update({k: nans(N, 4, hw) for k in ("dlogits_both", "dlogits_loss", "dlogits_ev", "loss_gradient", "dlogits_const")})
    L.check(lib.mimo_evidential_forward(lgd.data_ptr(), yd.data_ptr(), mkd.data_ptr(), N, hw, o["ev"].data_ptr(), o["loss"].data_ptr(), st))
    for key, a, b in (("dlogits_both", de, dl), ("dlogits_loss", None, dl), ("dlogits_ev", de, None)):
        L.check(lib.mimo_evidential_backward(lgd.data_ptr(), yd.data_ptr(), mkd.data_ptr(), L.ptr(a) or None, L.ptr(b) or None, N, hw,
                                             o[key].data_ptr(), st))
    const = torch.full((N, hw), 0.37, device="cuda")
    L.check(lib.mimo_evidential_backward(lgd.data_ptr(), yd.data_ptr(), mkd.data_ptr(), None, const.data_ptr(), N, hw,
                                         o["dlogits_const"].data_ptr(), st))
    L.check(lib.mimo_evidential_loss_gradient(lgd.data_ptr(), yd.data_ptr(), mkd.data_ptr(), N, hw, 0.37, o["loss_gradient"].data_ptr(), st))
    L.check(lib.mimo_evidential_uncertainties(lgd.data_ptr(), N, hw, o["mean"].data_ptr(), o["aleatoric_var"].data_ptr(),
                                              o["epistemic_var"].data_ptr(), st))
    torch.cuda.synchronize()
    written(*o.values())
    return {k: v.cpu() for k, v in o.items()}


def _check_evidential(tag, lg, y, mk, seed=1, only=None):
    g = torch.Generator().manual_seed(seed)
    d_loss, d_ev = torch.rand(y.shape, generator=g) + 0.5, torch.randn(lg.shape, generator=g)
    got = _run_evidential(lg, y, mk, d_loss, d_ev)
    assert torch.equal(bits(got["loss_gradient"]), bits(got["dlogits_const"])), "loss gradient must be the backward, bit for bit"
    assert torch.equal(bits(got["mean"]), bits(lg[:, 0])) and torch.equal(bits(got["ev"][:, 0]), bits(lg[:, 0]))
    off = mk == 0
    assert float(got["loss"][off].abs().max()) == 0.0, "masked pixels must give exactly zero loss"
    for k in ("dlogits_loss", "loss_gradient"):
        assert float(got[k].permute(0, 2, 1)[off].abs().max()) == 0.0, "masked pixels must give exactly zero loss gradient"
    ratios = {}
    const = torch.full_like(d_loss, R.f32(0.37))
    variants = {"dlogits_both": (d_loss, True, True), "dlogits_loss": (d_loss, True, False), "dlogits_ev": (d_loss, False, True),
                "loss_gradient": (const, True, False)}
    for key, (up, use_loss, use_ev) in variants.items():
        if only and key not in only:
            continue
        inputs = [lg, y, mk, up, d_ev]
        fn64 = R.evidential_reference(R.evidential_loss_lgamma_difference, use_loss, use_ev)
        ref = fn64(*[t.double() for t in inputs])
        fl = R.evidential_floors(ref)
        yd, _, bad = R.yardstick(R.evidential_reference(R.evidential_oracle_form, use_loss, use_ev), inputs, fl, fn64=fn64)
        cond = R.conditioning(fn64, inputs, 0) if any(bool(b.any()) for b in bad.values()) else None
        pairs = [(key, "dlogits")]
        if key == "dlogits_both":  # the forward outputs and the variances once
            pairs += [("ev", "ev"), ("loss", "loss"), ("aleatoric_var", "aleatoric_var"), ("epistemic_var", "epistemic_var")]
        for gk, rk in pairs:
            kernel = {"ev": "evidential_forward", "loss": "evidential_forward", "aleatoric_var": "evidential_uncertainties",
                      "epistemic_var": "evidential_uncertainties", "loss_gradient": "evidential_loss_gradient"}.get(gk, "evidential_backward")
            r = R.check(kernel, f"{tag} {gk}", got[gk], ref[rk], fl[rk], yd[rk], where=~bad[rk])
            if cond is not None:
                r = max(r, R.check_conditioned(kernel, f"{tag} {gk}", got[gk], ref[rk], fl[rk], cond[rk], bad[rk]) * R.MARGIN / R.COND_MARGIN)
            ratios[kernel] = max(ratios.get(kernel, 0.0), r)
    report(f"[evidential] {tag}: worst error / bound x {R.MARGIN:g} per kernel {ratios}")


@pytest.mark.parametrize("N", [1, 2])
def test_evidential_kernels_over_the_parameter_sweep(N):
    """1900 pixels, one per combination of alpha - 1 in [1e-4, 1e4], v and beta in [1e-3, 1e3] and |y - mu| in {0, 1e-3, 1, 30},
    logits on both sides of the softplus threshold, every seventh pixel masked: NIG parameters, loss map, dlogits with d_loss
    only, d_ev only and both, the loss gradient (also bit-equal to the backward with a constant-filled d_loss) and the three
    uncertainty maps.  N = 1: hw = 1900 (the 16-byte path of the uncertainties kernel), N = 2: hw = 950 (one pixel per thread).
    Pixels past alpha = 35, where the reference's exp(lgamma) / exp(lgamma) is inf / inf in fp32, are judged by the conditioning
    yardstick — none is dropped."""
    logits, label, mask, _ = R.evidential_sweep()
    _check_evidential(f"sweep N={N}", *R.pixels_to_layout(logits, label, mask, N))


def test_evidential_kernels_one_element_group_past_a_grid_pass():
    """1048576 + 259 pixels of ordinary values (one image, odd hw): the 4096-workgroup pass of the forward / backward / loss-gradient
    kernels and the 2048-workgroup pass of the uncertainties kernel run their loops again"""
    logits, label, mask = R.evidential_ordinary(1048576 + 259)
    _check_evidential("1048835 pixels", *R.pixels_to_layout(logits, label, mask, 1), only=("dlogits_both", "loss_gradient"))
