"""CPU-side checks of the FGSM sweep for MC-dropout ensembles (no GPU needed): the two new C-ABI symbols, the opt-in flag
of `mimo.adversarial` (the refusal without it is pinned by tests/test_adversarial_cpu.py), the per-chunk loss weights, and
the fp64 model of `fold_image_grad_mc_kernel` (tests/mc_fold_reference.py) against torch autograd.

Reference semantics at stake: scripts/test/test_nyuv2_depth.py with --monte_carlo_steps M — the mean NLL over the
concatenated axis of all M * S_total outputs, back-propagated to the image."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mc_fold_reference as M
from tests.test_adversarial_cpu import _member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mimo_input_gradient_mc", "mimo_op_fold_image_grad_mc")


def test_new_symbols_are_declared_listed_and_exported(built_library):
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
    # the argument lists ctypes is told about are as long as the declared ones
    for sym in NEW_SYMBOLS:
        decl = re.search(r"\bint\s+" + sym + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[sym][1]), sym


def test_mc_dropout_flag_is_opt_in_and_reaches_the_engine_check():
    """Without the flag: today's NotImplementedError.  With it the request passes validation and fails where every CPU tensor
    fails, at the engine's door (MimoHipError) — nothing else refuses it."""
    from mimo.adversarial import RobustnessEvaluator, fgsm_sweep, image_gradient
    from mimo.models.ensemble import EnsembleModule
    from mimo_unet_amd._lib import MimoHipError
    image, label = torch.rand(1, 2, 32, 32), torch.rand(1, 1, 32, 32)
    mc = EnsembleModule([], monte_carlo_steps=3, models=[_member(encoder_dropout_rate=0.1)])
    with pytest.raises(NotImplementedError, match="MC-dropout"):
        fgsm_sweep(mc, image, label, (0.0, 0.02))
    with pytest.raises(NotImplementedError, match="MC-dropout"):
        image_gradient(mc, image, label)
    with pytest.raises(MimoHipError):
        fgsm_sweep(mc, image, label, (0.0, 0.02), mc_dropout=True)
    with pytest.raises(MimoHipError):
        image_gradient(mc, image, label, mc_dropout=True)
    # (a RobustnessEvaluator cannot be made without a GPU; its flag is off by default like the others)
    import inspect
    for fn in (fgsm_sweep, image_gradient, RobustnessEvaluator.__init__):
        assert inspect.signature(fn).parameters["mc_dropout"].default is False
    # the flag with M = 0 is the plain path: the same engine-door error as without it
    plain = EnsembleModule([], models=[_member()])
    for flag in (False, True):
        with pytest.raises(MimoHipError):
            fgsm_sweep(plain, image, label, (0.0,), mc_dropout=flag)
    # the other refusals hold with the flag set
    with pytest.raises(NotImplementedError, match="negative"):
        fgsm_sweep(mc, image, label, (0.0, -0.02), mc_dropout=True)
    # the model-level entry: BatchNorm in training mode stays refused, passes > 1 needs the flag
    net = _member(encoder_dropout_rate=0.1).model
    net.train()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        net.image_gradient(image, label, None, torch.ones(2), torch.empty_like(image), mc_dropout=True)
    net.eval()
    with pytest.raises(ValueError, match="passes"):
        net.image_gradient(image, label, None, torch.ones(2), torch.empty_like(image), passes=2)


@pytest.mark.parametrize("passes,batch,max_samples", [(3, 2, 4), (4, 2, 64), (1, 2, 2), (5, 1, 2)])
@pytest.mark.parametrize("s_total", [1, 2, 5])
def test_chunk_weights_sum_to_one_over_s_total(passes, batch, max_samples, s_total):
    from mimo_unet_amd.adversarial import _mc_chunk_weights
    chunks = _mc_chunk_weights(passes, batch, max_samples, s_total)
    # the chunks tile [0, passes) in order, each fits the launch limit (or is a single pass), as EnsembleModule.forward forms them
    assert chunks[0][0] == 0 and chunks[-1][1] == passes
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    per_launch = max(1, min(passes, max_samples // batch))
    assert [m1 - m0 for m0, m1, _ in chunks] == [min(per_launch, passes - m0) for m0 in range(0, passes, per_launch)]
    # a chunk of k passes weighs k / (M * S_total): the engine's loss is the mean over the chunk's k * B samples
    for m0, m1, w in chunks:
        assert w == (m1 - m0) / (passes * s_total)
    assert abs(sum(w for _, _, w in chunks) - 1.0 / s_total) <= 4 * np.finfo(np.float64).eps / s_total
    if (passes, batch, max_samples) == (3, 2, 4):
        assert [(m0, m1) for m0, m1, _ in chunks] == [(0, 2), (2, 3)]


@pytest.mark.parametrize("replicas", [1, 3])
@pytest.mark.parametrize("channels", [2, 3])
def test_fold_model_is_the_transpose_of_reflect_pad_and_repeat(channels, replicas):
    B, H, W, ldp = 2, 6, 5, 4
    g = torch.Generator().manual_seed(40 + channels + 10 * replicas)
    dxpad = torch.randn(replicas * B, H + 2, W + 2, ldp, generator=g, dtype=torch.float64)
    start = torch.randn(B, channels, H, W, generator=g, dtype=torch.float64)
    x = torch.zeros(B, channels, H, W, dtype=torch.float64, requires_grad=True)
    y = F.pad(x, (1, 1, 1, 1), mode="reflect").repeat(replicas, 1, 1, 1)  # pass-major: (m, b) at row m * B + b
    (y * dxpad[..., :channels].permute(0, 3, 1, 2)).sum().backward()
    got = M.fold_mc(dxpad.numpy(), replicas, channels)
    assert got.shape == (B, channels, H, W)
    assert np.abs(got - x.grad.numpy()).max() <= 1e-13 * np.abs(x.grad.numpy()).max()
    acc = M.fold_mc(dxpad.numpy(), replicas, channels, start.numpy())
    assert np.abs(acc - (x.grad + start).numpy()).max() <= 1e-13 * np.abs(acc).max()
    if channels < ldp:  # the pad channels never enter
        poisoned = dxpad.clone()
        poisoned[..., channels:] = float("nan")
        assert np.array_equal(M.fold_mc(poisoned.numpy(), replicas, channels), got)
