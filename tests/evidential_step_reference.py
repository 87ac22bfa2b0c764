"""Reference of the evidential model's step tail — what EvidentialUnetModel.training_step / validation_step compute after the
backbone (the reference's mimo/models/evidential_unet.py:98-146) and mimo_evidential_step computes in one pass: the
standard-deviation and error maps and the per-element terms of every reduced scalar.  Dtype-generic like the references of
tests/scalar_reference.py: on fp32 tensors it is the reference in fp32 torch on the CPU, on the same values in fp64 the truth.
tests/test_evidential_step_cpu.py pins it to the host classes, tests/test_evidential_step_gpu.py runs the kernels against it."""
import torch

from oracle import mimo_oracle as O
from tests import scalar_reference as R
from tests.helpers import fp32_acc_bound, report


def step_terms(ev, label, mask, loss_form):
    """NIG parameters ev [N,4,...] (gamma, v, alpha, beta), label and mask (or None) of ev[:, 0]'s shape -> the maps and the
    per-element terms.  loss_form(ev, label, mask): one of the two evidential loss forms of scalar_reference.py."""
    alea, epi = O.evidential_vars(ev)
    a_std, e_std, err = alea.sqrt(), epi.sqrt(), ev[:, 0] - label
    return {"aleatoric_std": a_std, "epistemic_std": e_std, "err": err, "loss": loss_form(ev, label, mask),
            "aleatoric_var": alea, "epistemic_var": epi, "abs_err": err.abs(), "sq_err": err * err,
            "aleatoric_clip": a_std.clip(0, 5), "epistemic_clip": e_std.clip(0, 5)}


def step_reference(loss_form):
    """fn(logits [N,4,hw], label [N,hw], mask [N,hw] or None) on the softplus heads of the logits"""
    def fn(logits, label, mask):
        return step_terms(R.nig_heads(logits), label, mask, loss_form)
    return fn


# the standard deviations, variances and their clipped values are quotients and roots of positive numbers; the error map and
# the terms made of it are differences of the signed inputs (the floors the validation epilogue's terms have)
STEP_FLOORS = {"aleatoric_std": R.TINY, "epistemic_std": R.TINY, "aleatoric_var": R.TINY, "epistemic_var": R.TINY, "loss": R.TINY,
               "aleatoric_clip": R.TINY, "epistemic_clip": R.TINY, "err": R.frac_floor(R.FLOOR_SIGNED),
               "abs_err": R.frac_floor(R.FLOOR_SIGNED), "sq_err": R.frac_floor(R.FLOOR_SIGNED)}


def step_yardstick(logits, label, mask):
    """(yardsticks, fp64 reference, elements whose fp32 reference is not finite, conditioning of the loss or None): the fp32
    reference is the oracle's loss form (exp(lgamma) / exp(lgamma): not finite from alpha = 35 on), the fp64 truth the
    lgamma-difference form; where the former has no result the loss is judged by its conditioning under one fp32 ulp of
    each logit."""
    inputs = [logits, label, mask]
    fn64 = step_reference(R.evidential_loss_lgamma_difference)
    y, ref, bad = R.yardstick(step_reference(R.evidential_oracle_form), inputs, STEP_FLOORS, fn64=fn64)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values()), "every pixel needs a finite fp64 reference"
    assert not any(bool(b.any()) for k, b in bad.items() if k != "loss"), "only the loss may lack an fp32 reference"
    cond = R.conditioning(fn64, inputs, 0)["loss"] if bool(bad["loss"].any()) else None
    return y, ref, bad, cond


def loss_mean_allowance(ref_loss, y_loss, bad, cond):
    """What the mean of fp32 per-pixel losses accumulated in double may differ from the fp64 mean by: the mean over pixels of
    the per-element allowance — bound(yardstick) x max(|ref|, floor) where the fp32 reference is finite, COND_MARGIN x the
    conditioning where it is not — plus the final conversion to float.  No pixel is left out."""
    allow = R.bound(y_loss) * torch.maximum(ref_loss.abs(), torch.as_tensor(R.TINY, dtype=torch.float64))
    if cond is not None:
        allow = torch.where(bad, R.COND_MARGIN * cond, allow)
    return float(allow.mean()) + fp32_acc_bound(1, 0.0) * abs(float(ref_loss.mean()))


def check_loss_mean(kernel, tag, got, ref_loss, y_loss, bad, cond):
    want, allowed = float(ref_loss.mean()), loss_mean_allowance(ref_loss, y_loss, bad, cond)
    e = abs(float(got) - want)
    report(f"[{kernel}] scalar {tag} loss: got {float(got):.9e} ref {want:.9e} err {e:.2e} allowed {allowed:.2e} "
           f"({int(bad.sum())} pixels on the conditioning yardstick)")
    assert e <= allowed, (kernel, tag, float(got), want, allowed)
