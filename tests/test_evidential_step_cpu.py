"""tests/evidential_step_reference.py against what it stands for: the host classes EvidentialUnetModel's steps call on the NIG
parameters (EvidentialLoss.forward / mode / aleatoric_var / epistemic_var, compute_regression_metrics, clip(0, 5).mean()), the
golden arrays generated from the reference, and the finiteness of the fp64 truth on every pixel of the parameter sweep."""
import numpy as np
import pytest
import torch

from tests import evidential_step_reference as S
from tests import scalar_reference as R
from tests.helpers import load_npz


def test_step_reference_fp64_matches_the_host_classes():
    """fp64, 4096 ordinary pixels as two images with a mask and without: maps and per-element terms to 1e-12 of the host
    classes' results, the scalars formed from the terms to 1e-12 of compute_regression_metrics / clip(0, 5).mean()."""
    from mimo.losses import EvidentialLoss
    from mimo.metrics import compute_regression_metrics
    logits, label, mask = (t.double() for t in R.pixels_to_layout(*R.evidential_ordinary(4096), 2))
    crit = EvidentialLoss(coeff=1.0)
    ev = R.nig_heads(logits)
    close = lambda a, b: torch.testing.assert_close(torch.as_tensor(a, dtype=torch.float64), b.double(), rtol=1e-12, atol=1e-12)
    for mk in (mask, None):
        for form in (R.evidential_loss_lgamma_difference, R.evidential_oracle_form):  # ordinary alpha: the two forms agree
            got = S.step_reference(form)(logits, label, mk)
            close(got["loss"], crit(ev, label[:, None], mask=mk))
        y_pred = crit.mode(ev)
        close(got["err"], y_pred - label)
        close(got["aleatoric_var"], crit.aleatoric_var(ev))
        close(got["epistemic_var"], crit.epistemic_var(ev))
        close(got["aleatoric_std"], crit.aleatoric_var(ev) ** 0.5)
        close(got["epistemic_std"], crit.epistemic_var(ev) ** 0.5)
        close(got["aleatoric_clip"].mean(), (crit.aleatoric_var(ev) ** 0.5).clip(0, 5).mean())
        close(got["epistemic_clip"].mean(), (crit.epistemic_var(ev) ** 0.5).clip(0, 5).mean())
        want = compute_regression_metrics(y_pred.flatten(), label.flatten())
        sc = R.regression_scalars(got, label)
        for k in ("r2", "mae", "mse", "rmse"):
            close(sc[k], want[k])
        assert sc["count"] == 4096.0


def test_step_reference_fp32_matches_the_golden_arrays():
    """the reference's own aleatoric_var and loss (tests/golden/evidential.npz), at the tolerances
    test_host_cpu.py::test_evidential_loss_class_matches_golden holds the loss class to"""
    fx = load_npz("evidential.npz")
    ev, y, mask = (torch.from_numpy(fx[k]) for k in ("ev", "y", "mask"))
    got = S.step_terms(ev, y[:, 0], mask, R.evidential_oracle_form)
    np.testing.assert_allclose(got["loss"].numpy(), fx["loss"], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(got["aleatoric_var"].numpy(), fx["aleatoric_var"], rtol=1e-6)
    np.testing.assert_allclose(got["epistemic_var"].numpy(), fx["epistemic_var"], rtol=1e-6)


def test_every_sweep_pixel_has_a_finite_fp64_reference():
    """the sweep stays within finite standard deviations (largest epistemic std 1e5) and a finite fp64 loss, with the mask
    and without: no pixel has to be left out of a check"""
    logits, label, mask, _ = R.evidential_sweep()
    for N in (1, 2):
        lg, y, mk = R.pixels_to_layout(logits, label, mask, N)
        for m in (mk, None):
            ref = S.step_reference(R.evidential_loss_lgamma_difference)(lg.double(), y.double(), None if m is None else m.double())
            assert all(bool(torch.isfinite(v).all()) for v in ref.values())
            assert 0.99e5 < float(ref["epistemic_std"].max()) < 1.01e5
            yd, _, bad, cond = S.step_yardstick(lg, y, m)
            assert bool(bad["loss"].any()) and cond is not None and bool(torch.isfinite(cond).all())  # alpha > 35 is in the sweep
            assert np.isfinite(S.loss_mean_allowance(ref["loss"], yd["loss"], bad["loss"], cond))


def test_the_step_switch_and_scalar_names_exist():
    import mimo_unet_amd.models.evidential_unet as EU
    from mimo_unet_amd import _lib
    from mimo_unet_amd.engine import EVIDENTIAL_STEP_SCALARS, VAL_SCALARS
    import os
    assert EU._FUSED_STEP is (os.environ.get("MIMO_EVIDENTIAL_STEP_FUSED", "1") != "0")  # read once at import, default 1
    assert len(EVIDENTIAL_STEP_SCALARS) == 8 and EVIDENTIAL_STEP_SCALARS[1:] == VAL_SCALARS[1:] and EVIDENTIAL_STEP_SCALARS[0] == "loss"
    assert {"mimo_evidential_step", "mimo_evidential_loss_gradient_dev"} <= set(_lib.EXPORTED_SYMBOLS)


def test_a_cpu_batch_keeps_the_tensor_operations_and_their_error(monkeypatch):
    """a batch on the CPU never reaches the new entry point, switch on or off: both steps go the way they went before, which
    ends in the backbone's MimoHipError (the engine has no CPU path) — the same error either way"""
    import mimo_unet_amd.models.evidential_unet as EU
    from mimo.models.evidential_unet import EvidentialUnetModel
    from mimo_unet_amd._lib import MimoHipError

    def refuse(*a, **k):
        raise AssertionError("evidential_step called for a CPU batch")
    monkeypatch.setattr(EU, "evidential_step", refuse)
    m = EvidentialUnetModel(in_channels=3, out_channels=4, filter_base_count=4, center_dropout_rate=0.0, final_dropout_rate=0.0,
                            encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0,
                            learning_rate=1e-3, seed=0)
    g = torch.Generator().manual_seed(7)
    image, label = torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 1, 32, 32, generator=g)
    mask = (torch.rand(2, 32, 32, generator=g) > 0.25).float()
    for batch in ({"image": image, "label": label}, {"image": image, "label": label, "mask": mask}):
        for step, mode in ((m.training_step, m.train), (m.validation_step, m.eval)):
            mode()
            said = {}
            for fused in (True, False):
                monkeypatch.setattr(EU, "_FUSED_STEP", fused)
                assert m._fused_step(image, label, batch.get("mask"), "train") is None
                with pytest.raises(MimoHipError) as e:
                    step(batch, 0)
                said[fused] = str(e.value)
            assert said[True] == said[False]
