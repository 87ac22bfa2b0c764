"""CPU-side checks of the FGSM robustness sweep (no GPU needed): the fixture tests/golden/fgsm.npz (made from the reference by
tests/golden/make_fgsm_golden.py) against the oracle and against a numpy restatement of the attack, the condition the fixture
must satisfy (share of undecided pixels), the two new C-ABI symbols, and the input validation of `mimo.adversarial`.

Reference semantics at stake: `make_predictions` + `fgsm_attack` of scripts/test/test_nyuv2_depth.py:16-58 in eval mode."""
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
CASES = ("laplace", "gaussian")
NEW_SYMBOLS = ("mimo_input_gradient", "mimo_fgsm_perturb")


def case(fx, name):
    c = {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "/")}
    c["cfg"] = cfg_from_meta(c["meta"])
    c["state"] = state_from(c, "state/")
    c["kind"] = str(c["loss_kind"])
    return c


def oracle_gradient(c, image=None):
    """(logits, per-subnetwork input gradient, image gradient) of the oracle's eval-mode network with the loss the
    reference's script takes: the mean NLL over [N, S, 1, H, W] with the label repeated over the subnetwork axis."""
    cfg = c["cfg"]
    S = cfg.num_subnetworks
    img = torch.from_numpy(c["image"] if image is None else image).clone().requires_grad_(True)
    x5 = O.repeat_subnetworks(img, S)
    x5.retain_grad()
    out = O.mimo_unet_forward(cfg, c["state"], x5, training=False)
    p1, p2 = O.split_heads(out, cfg.out_channels)
    labels = torch.from_numpy(c["label"])[:, None].repeat(1, S, 1, 1, 1)
    O.loss_forward(c["kind"], p1, p2, labels).backward()
    return out.detach(), x5.grad.detach(), img.grad.detach()


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_fixture_logits_and_image_gradient(name):
    c = case(load_npz("fgsm.npz"), name)
    out, dx_sub, dimage = oracle_gradient(c)
    errs = {"logits": rel_err(out, c["logits"]), "dx_sub": rel_err(dx_sub, c["dx_sub"]), "dimage": rel_err(dimage, c["dimage"])}
    print(name, errs)
    assert all(e <= TOL for e in errs.values()), errs
    # the image gradient is the sum of the per-subnetwork gradients (repeat_subnetworks' backward)
    assert rel_err(R.sum_over_subnetworks(c["dx_sub"]), c["dimage"]) <= 1e-6


@pytest.mark.parametrize("name", CASES)
def test_numpy_attack_reproduces_the_fixture_perturbed_images_exactly(name):
    fx = load_npz("fgsm.npz")
    c = case(fx, name)
    assert list(fx["epsilons"]) == [0.0, 0.02, 0.04]
    img = c["image"]
    assert (img == 0).any() and (img == 1).any() and img.min() >= 0 and img.max() <= 1
    for k, eps in enumerate(fx["epsilons"]):
        got = R.fgsm_attack(img, eps, c["dimage"])
        assert got.dtype == np.float32 and np.array_equal(got, c["perturbed"][k]), (name, eps)
    assert np.array_equal(c["perturbed"][0], img)  # eps = 0 on an image inside [0, 1]
    clamped = (c["perturbed"][2] == 0) | (c["perturbed"][2] == 1)
    assert clamped.sum() > (img == 0).sum() // 4  # the clamp acts


def test_numpy_attack_sign_and_clamp_semantics():
    img = np.array([0.5, 0.5, 0.5, 0.99, 0.01, 0.5], dtype=np.float32)
    g = np.array([1e-30, -3.0, 0.0, 2.0, -2.0, np.nan], dtype=np.float32)
    out = R.fgsm_attack(img, 0.04, g)
    want = np.array([np.float32(0.5) + np.float32(0.04), np.float32(0.5) - np.float32(0.04), 0.5, 1.0, 0.0], dtype=np.float32)
    assert np.array_equal(out[:5], want) and np.isnan(out[5])
    t = torch.clamp(torch.from_numpy(img) + 0.04 * torch.from_numpy(g).sign(), 0, 1).numpy()
    assert np.array_equal(out[:5], t[:5])
    # a NaN gradient: torch.sign maps it to 0 (the reference would leave that pixel unattacked, silently); the engine and this
    # restatement let it through as NaN, so that a diverged gradient shows in the perturbed image
    assert t[5] == img[5]


@pytest.mark.parametrize("name", CASES)
def test_fixture_undecided_share_is_within_its_cap(name):
    c = case(load_npz("fgsm.npz"), name)
    share = R.undecided_share(c["dimage"])
    print(f"{name}: {share:.4%} of the pixels have |g| < {R.DECIDED_REL:g} max|g|")
    assert share <= R.MAX_UNDECIDED_SHARE


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
    assert "test_nyuv2_depth.py:41-55" in header and "test_nyuv2_depth.py:16-24" in header  # the reference lines they replace


def _member(S=2, loss="laplace_nll", **drop):
    from mimo.models.mimo_unet import MimoUnetModel
    kw = dict(center_dropout_rate=0.0, final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
              decoder_dropout_rate=0.0)
    kw.update(drop)
    return MimoUnetModel(in_channels=2, out_channels=2, num_subnetworks=S, filter_base_count=2, loss=loss, weight_decay=0.0,
                         learning_rate=1e-3, seed=0, loss_buffer_size=10, loss_buffer_temperature=0.3, **kw)


def test_adversarial_rejects_unsupported_requests_before_touching_a_gpu():
    """MC-dropout, evidential members and negative eps raise NotImplementedError from CPU tensors on a CPU-only host:
    nothing was sent to a GPU (a GPU touch would raise MimoHipError / a CUDA error instead)."""
    from mimo.adversarial import RobustnessEvaluator, fgsm_sweep
    from mimo.models.ensemble import EnsembleModule
    from mimo.models.evidential_unet import EvidentialUnetModel
    image, label = torch.rand(1, 2, 32, 32), torch.rand(1, 1, 32, 32)
    mc = EnsembleModule([], monte_carlo_steps=3, models=[_member(encoder_dropout_rate=0.1)])
    with pytest.raises(NotImplementedError, match="MC-dropout"):
        fgsm_sweep(mc, image, label, (0.0, 0.02))
    ev = EvidentialUnetModel(in_channels=2, out_channels=4, filter_base_count=2, center_dropout_rate=0.0, final_dropout_rate=0.0,
                             encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0,
                             learning_rate=1e-3, seed=0)
    with pytest.raises(NotImplementedError, match="evidential"):
        fgsm_sweep(EnsembleModule([], models=[ev]), image, label, (0.0,))
    plain = EnsembleModule([], models=[_member()])
    with pytest.raises(NotImplementedError, match="negative"):
        fgsm_sweep(plain, image, label, (0.0, -0.02))
    with pytest.raises(NotImplementedError, match="non-negative"):
        RobustnessEvaluator(epsilons=(0.02, -0.01))
