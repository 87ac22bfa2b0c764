"""CPU-side checks of the evidential model's FGSM sweep (no GPU needed): the fixture tests/golden/evidential_fgsm.npz (made from
the reference by tests/golden/make_evidential_fgsm_golden.py) against the oracle and against the numpy restatement of the
attack, the conditions the fixture must satisfy, the two new C-ABI symbols, and the refusals of `mimo.adversarial` for a bare
`EvidentialUnetModel`.

Reference semantics at stake: `make_predictions` + `fgsm_attack` of scripts/test/test_nyuv2_depth_evidential.py:16-65 in eval
mode, and `EvidentialLoss.mode / aleatoric_var / epistemic_var` (mimo/losses.py:258-271)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import mimo_oracle as O
from tests import fgsm_reference as R
from tests.helpers import cfg_from_meta, load_npz, rel_err, state_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3  # the project's output tolerance, max|a - b| / max|b|
CASES = ("odd", "even")
MIN_EVIDENCE = 0.1  # lower bound of alpha - 1 and of v at every pixel and eps (make_evidential_fgsm_golden.py)
NEW_SYMBOLS = ("mimo_evidential_uncertainties", "mimo_evidential_loss_gradient")


def case(fx, name):
    c = {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "/")}
    c["cfg"] = cfg_from_meta(c["meta"])
    c["state"] = state_from(c, "state/")
    return c


def oracle_gradient(c):
    """(logits [N,4,H,W], loss, image gradient) of the oracle's eval-mode evidential network with the loss the reference's
    script takes: the mean of the per-pixel evidential loss over all N*H*W pixels."""
    img = torch.from_numpy(c["image"]).clone().requires_grad_(True)
    logits = O.mimo_unet_forward(c["cfg"], c["state"], img[:, None], training=False)[:, 0]
    ev = O.evidential_forward(c["cfg"], c["state"], img, training=False)
    loss = O.evidential_loss(ev, torch.from_numpy(c["label"])).mean()
    loss.backward()
    return logits.detach(), loss.detach(), img.grad.detach()


def oracle_uncertainties(c, image):
    """(mode, aleatoric_var, epistemic_var), each [N,H,W], and the NIG parameters of the oracle on `image` (numpy [N,Ci,H,W])."""
    with torch.no_grad():
        ev = O.evidential_forward(c["cfg"], c["state"], torch.from_numpy(np.ascontiguousarray(image)), training=False)
    av, epv = O.evidential_vars(ev)
    return ev[:, 0], av, epv, ev


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_fixture_logits_and_image_gradient(name):
    c = case(load_npz("evidential_fgsm.npz"), name)
    logits, loss, dimage = oracle_gradient(c)
    errs = {"logits": rel_err(logits, c["logits"]), "dimage": rel_err(dimage, c["dimage"]),
            "loss": abs(float(loss) - float(c["loss"])) / abs(float(c["loss"]))}
    print(name, errs)
    assert all(e <= TOL for e in errs.values()), errs
    # ... and the reference's three maps on its own perturbed images
    for k in range(3):
        mode, av, epv, _ = oracle_uncertainties(c, c["perturbed"][k])
        errs = {"mode": rel_err(mode, c["mode"][k]), "aleatoric": rel_err(av, c["aleatoric_var"][k]),
                "epistemic": rel_err(epv, c["epistemic_var"][k])}
        print("   eps", k, errs)
        assert all(e <= TOL for e in errs.values()), errs


@pytest.mark.parametrize("name", CASES)
def test_numpy_attack_reproduces_the_fixture_perturbed_images_exactly(name):
    fx = load_npz("evidential_fgsm.npz")
    c = case(fx, name)
    assert list(fx["epsilons"]) == [0.0, 0.02, 0.04]
    img = c["image"]
    assert (img == 0).any() and (img == 1).any() and img.min() >= 0 and img.max() <= 1
    for k, eps in enumerate(fx["epsilons"]):
        got = R.fgsm_attack(img, eps, c["dimage"])
        assert got.dtype == np.float32 and np.array_equal(got, c["perturbed"][k]), (name, eps)
    assert np.array_equal(c["perturbed"][0], img)  # eps = 0 on an image inside [0, 1]


@pytest.mark.parametrize("name", CASES)
def test_fixture_satisfies_its_input_conditions(name):
    """Conditions on the inputs, asserted by the generator on the reference's own numbers and here again: few undecided
    pixels (of a gradient that is not all zero), alpha - 1 and v away from zero at every pixel and eps, everything finite."""
    c = case(load_npz("evidential_fgsm.npz"), name)
    n, h, w = c["meta"][4], c["meta"][5], c["meta"][6]
    assert c["logits"].shape == (n, 4, h, w) and c["mode"].shape == (3, n, h, w) and c["dimage"].shape == c["image"].shape
    share = R.undecided_share(c["dimage"])
    print(f"{name}: {share:.4%} of the pixels have |g| < {R.DECIDED_REL:g} max|g| = {np.abs(c['dimage']).max():.3e}")
    assert np.abs(c["dimage"]).max() > 0 and share <= R.MAX_UNDECIDED_SHARE
    for k in range(3):
        # epistemic = aleatoric / v, aleatoric = beta / (alpha - 1): the reference's own maps give v; alpha - 1 from the oracle's
        # parameters on the reference's perturbed image (the fixture stores logits of the clean image only)
        v_ref = c["aleatoric_var"][k] / c["epistemic_var"][k]
        ev = oracle_uncertainties(c, c["perturbed"][k])[3]
        am1, v = float((ev[:, 2] - 1).min()), float(ev[:, 1].min())
        print(f"   eps {k}: min(alpha - 1) {am1:.3f}, min v {v:.3f} (from the reference's maps: {float(v_ref.min()):.3f})")
        assert am1 >= MIN_EVIDENCE and v >= MIN_EVIDENCE and v_ref.min() >= MIN_EVIDENCE
    l = torch.from_numpy(c["logits"])
    assert float(torch.nn.functional.softplus(l[:, 2]).min()) >= MIN_EVIDENCE and float(torch.nn.functional.softplus(l[:, 1]).min()) >= MIN_EVIDENCE
    for k, v in c.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            assert np.isfinite(v).all(), k


def test_new_symbols_are_declared_listed_and_exported(built_library):
    import fnmatch
    import subprocess

    from mimo_unet_amd import _lib
    header = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    vmap = open(os.path.join(ROOT, "mimo_unet_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"([A-Za-z0-9_*?]+)\s*;", vmap.split("global:")[1].split("local:")[0])
    nm = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} is not declared in include/mimo_hip.h"
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns), f"{sym} is not covered by csrc/exports.map"
        assert sym in _lib.EXPORTED_SYMBOLS, f"{sym} is not in _lib.EXPORTED_SYMBOLS"
        assert sym in exported, f"libmimo_hip.so does not export {sym}"
    assert "test_nyuv2_depth_evidential.py:42-65" in header and "losses.py:258-271" in header  # the reference lines they replace


def _evidential(**drop):
    from mimo.models.evidential_unet import EvidentialUnetModel
    kw = dict(center_dropout_rate=0.0, final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
              decoder_dropout_rate=0.0)
    kw.update(drop)
    return EvidentialUnetModel(in_channels=2, out_channels=4, filter_base_count=2, weight_decay=0.0, learning_rate=1e-3, seed=0, **kw)


def test_a_bare_evidential_model_is_accepted_and_cpu_tensors_are_refused_as_such():
    """An eval-mode `EvidentialUnetModel` passes every check of the sweep; what stops it on a CPU-only host is the engine's
    own "runs on an AMD GPU" error — not "the ensemble has no members", which is what it met before it was accepted."""
    from mimo.adversarial import fgsm_sweep, image_gradient
    from mimo_unet_amd._lib import MimoHipError
    model = _evidential().eval()
    image, label = torch.rand(1, 2, 32, 32), torch.rand(1, 1, 32, 32)
    with pytest.raises(MimoHipError):
        fgsm_sweep(model, image, label, (0.0, 0.02))
    with pytest.raises(MimoHipError):
        image_gradient(model, image, label)
    with pytest.raises(MimoHipError):
        model.image_gradient(image, label, mask=torch.ones(1, 1, 32, 32))
    with pytest.raises(MimoHipError):
        model.predict_uncertainties(image)
    with pytest.raises(NotImplementedError, match="negative"):
        fgsm_sweep(model, image, label, (0.0, -0.02))
    with pytest.raises(ValueError, match="label"):
        model.image_gradient(image, torch.rand(1, 32, 32))
    assert all(p.grad is None for p in model.parameters())


def test_training_mode_active_dropout_and_16_bit_storage_are_refused_before_touching_a_gpu(monkeypatch):
    from mimo.adversarial import fgsm_sweep
    from mimo.models.ensemble import EnsembleModule
    image, label = torch.rand(1, 2, 32, 32), torch.rand(1, 1, 32, 32)
    with pytest.raises(NotImplementedError, match="eval mode"):
        fgsm_sweep(_evidential().train(), image, label, (0.0,))
    with pytest.raises(NotImplementedError, match="eval mode"):
        _evidential().train().predict_uncertainties(image)
    dropped = _evidential(encoder_dropout_rate=0.1).eval()
    for d in dropped.model._dropout_modules():
        d.train()  # MC-dropout: the module in eval mode, its dropout layers switched on
    with pytest.raises(NotImplementedError, match="eval mode"):
        fgsm_sweep(dropped, image, label, (0.0,))
    with pytest.raises(NotImplementedError, match="eval mode"):
        dropped.image_gradient(image, label)
    # an ensemble OF evidential models stays refused
    with pytest.raises(NotImplementedError, match="evidential"):
        fgsm_sweep(EnsembleModule([], models=[_evidential().eval()]), image, label, (0.0,))
    monkeypatch.setenv("MIMO_PRECISION", "bf16-mixed")
    stored16 = _evidential().eval()
    assert stored16.model._geom.precision == "bf16-mixed"
    with pytest.raises(NotImplementedError, match="fp32 and split16"):
        fgsm_sweep(stored16, image, label, (0.0,))
    with pytest.raises(NotImplementedError, match="fp32 and split16"):
        stored16.image_gradient(image, label)
