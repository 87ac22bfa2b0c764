"""The references of tests/scalar_reference.py checked on the CPU: against the host classes (mimo.losses, LossBuffer) and
torch.optim.Adam on ordinary values in fp64 and fp32, the error measures on constructed cases, and — for the exact input
generators tests/test_scalar_kernels_gpu.py uses — that the fp64 reference is finite for every element: nothing is left out."""
import math

import pytest
import torch

from mimo.losses import EvidentialLoss, UncertaintyLoss
from mimo.models.mimo_components.loss_buffer import LossBuffer
from oracle import mimo_oracle as O
from tests import scalar_reference as R

KINDS = ["laplace_nll", "gaussian_nll"]
DTYPES = [torch.float64, torch.float32]
TOL = {torch.float64: 1e-12, torch.float32: 2e-6}


def close(a, b, dtype):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= TOL[dtype] * max(float(b.abs().max()), 1e-30)


def all_finite(d):
    return all(bool(torch.isfinite(v).all()) for v in d.values())


# ---- error measures ----------------------------------------------------------------------------------------------------

def test_elem_err_sees_one_wrong_small_element_and_returns_its_index():
    ref = torch.tensor([[1000.0, 1.0], [1e-3, -2.0]], dtype=torch.float64)
    got = ref.clone()
    got[1, 0] *= 1.01
    e, at = R.elem_err(got, ref, 1e-6)
    assert at == (1, 0) and abs(e - 0.01) < 1e-9
    assert abs(R.elem_err(got, ref, 1.0)[0] - 1e-5) < 1e-12       # under the floor the error is relative to the floor
    got[0, 1] = float("nan")
    assert R.elem_err(got, ref, 1e-6) == (float("inf"), (0, 1))  # an output left NaN is an infinite error
    with pytest.raises(AssertionError):
        R.elem_err(got, got, 1e-6)                                 # a non-finite reference is refused, not skipped


def test_yardstick_is_the_fp32_rounding_of_the_function_and_marks_non_finite_fp32_results():
    x = torch.tensor([0.1, 1.0, 3.0, 40.0])
    errs, hi, bad = R.yardstick(lambda t: {"e": torch.exp(t) / torch.exp(t - 1), "g": torch.exp(torch.lgamma(t * 2))},
                                [x], {"e": R.TINY, "g": R.TINY})
    assert 0 < errs["e"] < 1e-6 and hi["e"].dtype == torch.float64 and not bool(bad["e"].any())
    assert bad["g"].tolist() == [False, False, False, True] and errs["g"] < 1e-5  # exp(lgamma(80)) overflows fp32 only
    assert R.bound(0.0) == 4 * 2.0 ** -23 and R.bound(1e-3) == 4e-3


def test_conditioning_is_the_change_under_one_fp32_ulp_of_each_channel():
    x = torch.tensor([[[1.0], [1000.0]]])  # [N=1, C=2, 1]
    cond = R.conditioning(lambda t: {"s": t[:, 0] * 3 + t[:, 1]}, [x], 0)["s"]
    assert abs(float(cond) - 2.0 ** -14) < 1e-12  # one ulp of 1000 (2^-14) beats three ulp of 1 (3 x 2^-23)


# ---- loss buffer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,size,T", [(3, 10, 0.3), (2, 1, 0.3), (64, 10, 0.3)])
def test_loss_buffer_sequence_matches_the_host_class(S, size, T, dtype):
    losses = R.loss_buffer_losses(S, size, T).to(dtype)
    ref = R.loss_buffer_sequence(losses, S, T, size)
    lb = LossBuffer(S, R.f32(T), size)
    lb.buffer = lb.buffer.to(dtype)
    for i, l in enumerate(losses):
        w = lb.get_weights()                       # read BEFORE the add
        lb.add(l)
        assert close(ref["weights"][i], w, dtype) and close(ref["w_over_s"][i], w / S, dtype)
        assert close(ref["weighted"][i], (l * w).mean(), dtype) and close(ref["mean"][i], l.mean(), dtype)
        assert torch.equal(ref["ring"][i], lb.buffer) and lb.index == (i + 1) % size
    assert float(ref["weights"][0].sub(1).abs().max()) < 1e-6  # an all-zero ring: uniform weights


@pytest.mark.parametrize("S", R.LOSS_BUFFER_S)
@pytest.mark.parametrize("size", R.LOSS_BUFFER_SIZES)
@pytest.mark.parametrize("T", R.LOSS_BUFFER_T)
def test_loss_buffer_inputs_leave_nothing_out(S, size, T):
    losses = R.loss_buffer_losses(S, size, T)
    assert losses.shape == (R.LOSS_BUFFER_STEPS, S) and float(losses.min()) >= -5 and float(losses.max()) <= 40
    errs, hi, bad = R.yardstick(lambda l: R.loss_buffer_sequence(l, S, T, size), [losses], R.loss_buffer_floors(losses))
    assert all_finite(hi) and not any(bool(b.any()) for b in bad.values())
    if S > 1 and T == 0.01 and size == 10:
        assert float((hi["ring"][-1].mean(0) / T).max()) > 1000  # the max-subtraction of the softmax matters
        assert float(losses.min()) < 0


# ---- Adam --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_reference_matches_torch_optim_adam(wd, dtype):
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(1001, generator=g).to(dtype)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=R.f32(1e-3), betas=(R.f32(0.9), R.f32(0.999)), eps=R.f32(1e-8), weight_decay=R.f32(wd))
    st = {"p": p0.clone(), "m": torch.zeros_like(p0), "v": torch.zeros_like(p0)}
    for step in (1, 2, 3):
        grad = torch.randn(1001, generator=g).to(dtype)
        pt.grad = (grad * R.f32(1.0 / 3.0)).clone()
        opt.step()
        st = R.adam_reference(st["p"], grad, st["m"], st["v"], step=step, wd=wd, grad_scale=1.0 / 3.0)
    assert close(st["p"], pt.detach(), dtype)
    assert close(st["m"], opt.state[pt]["exp_avg"], dtype) and close(st["v"], opt.state[pt]["exp_avg_sq"], dtype)


@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_inputs_leave_nothing_out(n):
    for wd, gs, step in (R.ADAM_HYPER if n < 100 else R.ADAM_HYPER_LARGE):
        p, g, m, v = R.adam_inputs(n, step)
        ref = R.adam_reference(p.double(), g.double(), m.double(), v.double(), step=step, wd=wd, grad_scale=gs)
        assert all_finite(ref) and bool((ref["v"] >= 0).all())
        assert bool((torch.sign(m) * torch.sign(g) >= 0).all())  # m carries g's sign: no cancellation in the first moment


# ---- uncertainties and the epilogues ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_validation_and_training_references_match_the_host_loss_classes(kind, dtype):
    crit = UncertaintyLoss.from_name(kind)
    out, label, mask = (t.to(dtype) for t in R.validation_inputs(3, 3, 2, 63, 5))
    ref = R.validation_reference(kind)(out, label, mask)
    p1, p2 = out[:, :, :2], out[:, :, 2:]
    std = crit.std(p1, p2)
    mean, alea = p1.mean(dim=1), (std ** 2).mean(dim=1)
    epi = ((p1 - mean[:, None]) ** 2).sum(dim=1) / 2
    comb = crit.calculate_dist_param(torch.sqrt(alea + epi), log=True)
    nll = crit.forward(mean, comb, label, mask=mask, reduce_mean=False)
    for k, v in (("mean", mean), ("aleatoric_std", alea.sqrt()), ("epistemic_std", epi.sqrt()), ("err", mean - label), ("nll", nll)):
        assert close(ref[k], v, dtype), k
    assert bool((ref["nll"][0] == 0).all())  # image 0 is wholly masked
    u = R.uncertainties_reference(kind)(p1, p2)
    assert close(u["mean"], mean, dtype) and close(u["aleatoric_var"], alea, dtype) and close(u["epistemic_var"], epi, dtype)
    out, label, perms = R.training_inputs(3, 2, 3, 2, 63, 6)
    out, label = out.to(dtype), label.to(dtype)
    tr = R.training_reference(kind)(out, label, perms)
    lt = torch.stack([label[perms[s]] for s in range(3)], dim=1)
    assert torch.equal(tr["label_t"], lt) and close(tr["aleatoric_std"], crit.std(out[:, :, :2], out[:, :, 2:]), dtype)
    assert close(tr["err"], out[:, :, :2] - lt, dtype)
    sc = R.regression_scalars(R.training_reference(kind)(out.double(), label.double(), perms), lt)
    yh, y = out[:, :, :2].double().flatten(), lt.double().flatten()
    assert abs(sc["r2"] - float(1 - ((y - yh) ** 2).sum() / ((y - y.mean()) ** 2).sum())) < 1e-12
    assert abs(sc["rmse"] - float(((yh - y) ** 2).mean().sqrt())) < 1e-12 and sc["count"] == y.numel()


def test_clamp_edges_are_planted_at_both_ends():
    out, _, mask = R.validation_inputs(3, 2, 3, 63, 7)
    first, last = out[0, 0, 3].flatten(), out[2, 1, 5].flatten()
    for t in (first, last):
        assert t[:4].tolist() == pytest.approx(list(R.CLAMP_EDGES)) and t[-4:].tolist() == pytest.approx(list(R.CLAMP_EDGES)[::-1])
    assert abs(math.exp(R.CLAMP_EDGES[1]) - 1e-5) < 1e-11 and abs(math.exp(R.CLAMP_EDGES[2]) - 1e3) < 1e-3
    assert float(mask[0].abs().max()) == 0.0 and 0.0 < float(mask[1:].mean()) < 1.0


# the shapes of the GPU tests (test_scalar_kernels_gpu.py imports them from here)
VALIDATION_SHAPES = [(1, 2, 1, 262144 + 259), (3, 2, 3, 63)]            # N, S, Ct, hw
# (reps = 2 and S = 3 make the total a multiple of 6: 524550 is the first such total past 524288 + 259)
TRAINING_SHAPES = [(5, 2, 3, 1, 17485), (2, 2, 3, 3, 63)]  # N0, reps, S, Ct, hw
UNCERTAINTY_SHAPES = [(1, 2, 1, 1048576 + 259), (3, 2, 3, 63)]          # N, S, C, hw


@pytest.mark.parametrize("kind", KINDS)
def test_epilogue_inputs_leave_nothing_out(kind):
    for N, S, Ct, hw in VALIDATION_SHAPES:
        errs, hi, bad = R.yardstick(R.validation_reference(kind), list(R.validation_inputs(N, S, Ct, hw, 11)), R.VALIDATION_FLOORS)
        assert all_finite(hi) and not any(bool(b.any()) for b in bad.values()), (N, S, Ct, hw)
    for N0, reps, S, Ct, hw in TRAINING_SHAPES:
        out, label, perms = R.training_inputs(N0, reps, S, Ct, hw, 12)
        assert all_finite(R.training_reference(kind)(out.double(), label.double(), perms))
        assert N0 * reps * S * Ct * hw == 524288 + 262 or hw == 63
    for N, S, C, hw in UNCERTAINTY_SHAPES:
        p1, p2 = R.uncertainty_inputs(N, S, C, hw, 13)
        assert all_finite(R.uncertainties_reference(kind)(p1.double(), p2.double()))


# ---- evidential ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_evidential_reference_matches_the_host_class_and_the_oracle_where_they_are_finite(dtype):
    logits, label, mask, am1 = R.evidential_sweep()
    keep = am1 < (100 if dtype == torch.float64 else 20)  # exp(lgamma(alpha)) finite (and fp32-accurate) in this dtype
    lg, y, mk = R.pixels_to_layout(logits[keep].to(dtype), label[keep].to(dtype), mask[keep].to(dtype), 1)
    ev = R.nig_heads(lg)
    ours = R.evidential_loss_lgamma_difference(ev, y, mk)
    host = EvidentialLoss(coeff=1.0)(ev[..., None], y[:, None, :, None], mask=mk[..., None])[..., 0]
    oracle = R.evidential_oracle_form(ev, y, mk)
    tol = 1e-11 if dtype == torch.float64 else 2e-5  # fp32: exp(lgamma) carries |lgamma| ulp (lgamma(21) = 42)
    for other in (host, oracle):
        assert float(((ours - other).abs() / other.abs().clamp_min(1e-30)).max()) < tol
    a_ref, e_ref = EvidentialLoss.aleatoric_var(ev), EvidentialLoss.epistemic_var(ev)
    res = R.evidential_reference(R.evidential_loss_lgamma_difference)(lg, y, mk, torch.ones_like(y), torch.zeros_like(lg))
    assert torch.equal(res["aleatoric_var"], a_ref) and torch.equal(res["epistemic_var"], e_ref)
    # dlogits is the autograd gradient of the host class's loss
    lt = lg.clone().requires_grad_(True)
    EvidentialLoss(coeff=1.0)(R.nig_heads(lt)[..., None], y[:, None, :, None], mask=mk[..., None]).sum().backward()
    scale = lt.grad.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    assert float(((res["dlogits"] - lt.grad).abs() / scale).max()) < (1e-10 if dtype == torch.float64 else 1e-4)


def test_evidential_sweep_covers_the_ranges_and_leaves_nothing_out():
    logits, label, mask, am1 = R.evidential_sweep()
    P = logits.shape[0]
    assert P == 19 * 5 * 5 * 4 and P % 4 == 0 and (P // 2) % 4 != 0  # one layout on the 16-byte path, one off it
    ev = R.nig_heads(logits.double()[None].permute(0, 2, 1))[0]
    d = (label.double() - logits[:, 0].double()).abs()
    assert float((ev[2] - 1).min()) < 1.01e-4 and float((ev[2] - 1).max()) > 0.99e4
    for row in (ev[1], ev[3]):
        assert float(row.min()) < 1.01e-3 and float(row.max()) > 0.99e3
    for target in R.EVIDENTIAL_DIFF:
        assert bool(((d - target).abs() <= 1e-6 * max(target, 1.0) + 2e-7).any()), target
    for c in (1, 2, 3):
        assert bool((logits[:, c] > 20).any()) and bool((logits[:, c] < 20).any())  # both sides of the softplus threshold
    assert 0 < int((mask == 0).sum()) < P // 4
    for N in (1, 2):
        lg, y, mk = R.pixels_to_layout(logits, label, mask, N)
        g = torch.Generator().manual_seed(1)
        d_loss, d_ev = torch.rand(y.shape, generator=g) + 0.5, torch.randn(lg.shape, generator=g)
        fn64 = R.evidential_reference(R.evidential_loss_lgamma_difference)
        errs, hi, bad = R.yardstick(R.evidential_reference(R.evidential_oracle_form), [lg, y, mk, d_loss, d_ev],
                                    R.evidential_floors(fn64(lg.double(), y.double(), mk.double(), d_loss.double(), d_ev.double())),
                                    fn64=fn64)
        assert all_finite(hi)                                            # every pixel has a finite fp64 reference ...
        assert bool(bad["loss"].any()) and not bool(bad["ev"].any())     # ... and those past alpha = 35 have no fp32 one:
        big = (R.pixels_to_layout(am1[:, None].expand(P, 4).float(), am1.float(), mask, N)[1] > 40) & (mk > 0)
        assert bool(bad["loss"][big].all())                              # they go to the conditioning yardstick
        cond = R.conditioning(fn64, [lg, y, mk, d_loss, d_ev], 0)
        assert all_finite(cond)


def test_evidential_ordinary_inputs_have_a_finite_fp32_reference():
    logits, label, mask = R.evidential_ordinary(4096 + 3)
    lg, y, mk = R.pixels_to_layout(logits, label, mask, 1)
    errs, hi, bad = R.yardstick(R.evidential_reference(R.evidential_oracle_form), [lg, y, mk, torch.ones_like(y), torch.zeros_like(lg)],
                                {k: R.TINY for k in ("ev", "loss", "dlogits", "aleatoric_var", "epistemic_var")},
                                fn64=R.evidential_reference(R.evidential_loss_lgamma_difference))
    assert all_finite(hi) and not any(bool(b.any()) for b in bad.values())
