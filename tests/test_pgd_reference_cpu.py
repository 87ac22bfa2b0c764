"""CPU-side checks of the PGD sweep (no GPU needed): the numpy restatement of `mimo_pgd_step` / `mimo_pgd_init`
(tests/pgd_reference.py) against the usual torch form and against the FGSM restatement, the ball and range invariants, the
random start's arithmetic and its Philox counter layout against the dropout and permutation draws, the two new C-ABI symbols,
and the input validation of `mimo.adversarial.pgd_sweep` / `RobustnessEvaluator(attack=...)`.

No reference counterpart: the reference's only attack is the single step of scripts/test/test_nyuv2_depth.py:16-24."""
import os
import re

import numpy as np
import pytest
import torch

from tests import dropout_reference as D
from tests import fgsm_reference as R
from tests import perm_reference as P
from tests import pgd_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mimo_pgd_step", "mimo_pgd_init")
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _data(seed, n=4096, k=3):
    g = np.random.default_rng(seed)
    x0 = g.uniform(-0.2, 1.2, n).astype(np.float32)
    x0[:8] = [0.0, 1.0, 0.5, 0.25, 1.0, 0.0, 0.75, 0.125]
    x_adv = (x0[None] + g.uniform(-0.05, 0.05, (k, n))).astype(np.float32)
    grad = g.standard_normal((k, n)).astype(np.float32)
    grad[:, 8:16] = [0.0, -0.0, 1e-38, -1e-38, 3.0, -3.0, 0.0, -0.0]  # +-0, denormals, both signs
    return x0, grad, x_adv


def _torch_step(x0, grad, x_adv, eps, alpha, lo, hi):
    x0, grad, x_adv = (torch.from_numpy(t) for t in (x0, grad, x_adv))
    out = []
    for k in range(x_adv.shape[0]):
        v = x_adv[k] + alpha[k] * grad[k].sign()
        out.append(torch.clamp(torch.max(torch.min(v, x0 + eps[k]), x0 - eps[k]), lo, hi))
    return torch.stack(out).numpy()


@pytest.mark.parametrize("clip", [(0.0, 1.0), (0.1, 0.9), (-INF, INF)], ids=["unit", "inner", "inf"])
def test_step_equals_the_usual_torch_form_bit_for_bit(clip):
    eps, alpha = [0.0, 0.02, 0.04], [0.01, 0.005, 0.0125]
    x0, grad, x_adv = _data(1)
    x_adv[0] = x0  # (the eps = 0 level sits on the ball's only point, as in a sweep)
    for _ in range(3):
        want = _torch_step(x0, grad, x_adv, eps, alpha, *clip)
        got = G.pgd_step(x0, grad, x_adv, eps, alpha, *clip)
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
        x_adv = got
        grad = np.roll(grad, 7, axis=1)
    assert (got != x0).any()


def test_step_sign_nan_and_zero_eps_semantics():
    x0 = np.array([0.5, 0.5, 0.5, np.nan, 0.5, 1.5], dtype=np.float32)
    grad = np.array([[0.0, -0.0, np.nan, 1.0, 2.0, -1.0]], dtype=np.float32)
    out = G.pgd_step(x0, grad, x0[None].copy(), [0.04], [0.01], 0.0, 1.0)[0]
    assert out[0] == out[1] == np.float32(0.5)            # +-0 gradient: no move
    assert np.isnan(out[2]) and np.isnan(out[3])          # a NaN gradient and a NaN pixel pass through
    assert out[4] == np.float32(0.5) + np.float32(0.01) and out[5] == np.float32(1.0)
    # eps = 0: clamp(x0, lo, hi) whatever the (non-NaN) gradient and the current iterate are
    x0, g, xa = _data(2)
    out = G.pgd_step(x0, g[:1], xa[:1], [0.0], [0.3], 0.0, 1.0)[0]
    assert np.array_equal(out, G.clamp(x0, 0.0, 1.0))


@pytest.mark.parametrize("eps", [0.0, 0.02, 0.04, 0.3])
def test_one_step_of_size_eps_from_the_clean_image_is_fgsm_bit_for_bit(eps):
    g = np.random.default_rng(3)
    x0 = g.uniform(0.0, 1.0, 4096).astype(np.float32)
    x0[:4] = [0.0, 1.0, 0.0, 1.0]
    grad = g.standard_normal(4096).astype(np.float32)
    grad[4:7] = [0.0, -0.0, np.nan]
    start = G.clamp(x0, 0.0, 1.0)
    assert np.array_equal(_bits(start), _bits(x0))
    got = G.pgd_step(x0, grad[None], start[None], [eps], [eps], 0.0, 1.0)[0]
    want = R.fgsm_attack(x0, eps, grad)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isnan(got[6])


@pytest.mark.parametrize("clip", [(0.0, 1.0), (-INF, INF)], ids=["unit", "inf"])
def test_every_iterate_lies_in_the_ball_and_in_the_range(clip):
    eps, alpha = [0.0, 0.02, 0.04], [0.5, 0.03, 0.003]  # steps larger and smaller than the ball
    x0, grad, _ = _data(4)
    g = np.random.default_rng(5)
    x_adv = np.stack([G.clamp(x0, *clip)] * 3)
    for t in range(7):
        x_adv = G.pgd_step(x0, grad, x_adv, eps, alpha, *clip)
        for k, e in enumerate(eps):
            lower, upper = (x0 - np.float32(e)).astype(np.float32), (x0 + np.float32(e)).astype(np.float32)
            inside = (x0 >= clip[0] - e) & (x0 <= clip[1] + e)  # elsewhere ball and range do not meet: the range wins
            assert (x_adv[k] >= clip[0]).all() and (x_adv[k] <= clip[1]).all()
            assert ((x_adv[k] >= lower) & (x_adv[k] <= upper))[inside].all(), (t, k)
        grad = g.standard_normal(grad.shape).astype(np.float32)


def test_start_unit_is_exact_symmetric_and_inside_the_open_interval():
    g = np.random.default_rng(6)
    w = np.concatenate([g.integers(0, 1 << 32, 100000, dtype=np.uint64), np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint64)])
    r = G.unit(w)
    exact = (2 * (w >> np.uint64(8)).astype(np.int64) + 1 - (1 << 24)).astype(np.float64) / 2.0 ** 24
    assert r.dtype == np.float32 and np.array_equal(r.astype(np.float64), exact)  # no rounding anywhere
    assert (np.abs(r) < 1).all() and (r != 0).all()
    assert r.min() == np.float32(-(1 - 2.0 ** -24)) and r.max() == np.float32(1 - 2.0 ** -24)
    mirror = G.unit(~w & np.uint64(0xFFFFFFFF))
    assert np.array_equal(mirror, -r)
    assert abs(float(r[:100000].mean())) < 0.01 and abs(float((r[:100000] ** 2).mean()) - 1 / 3) < 0.01


def test_start_is_two_roundings_shared_by_the_levels_and_clamped():
    g = np.random.default_rng(7)
    x0 = g.uniform(-0.1, 1.1, 1001).astype(np.float32)
    eps = [0.0, 0.02, 0.04]
    seed, offset = 0x1234567890ABCDEF, (5 << 32) + 8
    out = G.pgd_init(x0, eps, 0.0, 1.0, seed, offset)
    r = G.unit(G.start_words(x0.size, seed, offset))
    for k, e in enumerate(eps):
        prod = (np.float64(np.float32(e)) * r.astype(np.float64)).astype(np.float32)  # one rounding
        want = G.clamp((x0.astype(np.float64) + prod.astype(np.float64)).astype(np.float32), 0.0, 1.0)  # and another
        assert np.array_equal(_bits(out[k]), _bits(want))
        assert (np.abs(out[k].astype(np.float64) - G.clamp(x0, 0, 1)) <= e + 1e-7).all()
    assert np.array_equal(out[0], G.clamp(x0, 0.0, 1.0))
    free = (x0 > 0.05) & (x0 < 0.95)  # nothing is clamped there
    assert (out[2] != x0)[free].mean() > 0.99  # (|eps r| can stay below half an ulp of the pixel)
    # the same r for every level: the displacements are in the ratio of the eps
    d1, d2 = (out[1] - x0)[free].astype(np.float64), (out[2] - x0)[free].astype(np.float64)
    assert np.allclose(d2, 2 * d1, atol=2e-7)
    assert not np.array_equal(G.pgd_init(x0, eps, 0.0, 1.0, seed, offset + 4), out)
    assert not np.array_equal(G.pgd_init(x0, eps, 0.0, 1.0, seed + 1, offset), out)


@pytest.mark.parametrize("elems", [1, 3, 4, 7, 1001])
def test_start_scalar_tail_uses_the_quads_own_counter(elems):
    """Element i takes word i % 4 of quad i // 4 whatever the element count: a buffer cut short (the scalar path's tail quad)
    has the values of the same elements in the longer, vectorisable one."""
    seed, offset = 77, 12
    long_words = G.start_words(1004, seed, offset)
    assert np.array_equal(G.start_words(elems, seed, offset), long_words[:elems])
    c0, c1, c2, c3 = G.start_counters(elems, offset)
    assert len(c0) == (elems + 3) // 4 and np.array_equal(c0, np.arange(len(c0))) and not c1.any()
    one = P.philox4x32_10(c0[-1], c1[-1], c2[-1], c3[-1], seed, 0)
    n = elems - 4 * (len(c0) - 1)
    assert [int(w) for w in one[:n]] == [int(w) for w in long_words[4 * (len(c0) - 1): elems]]


def test_start_counters_are_one_per_quad_with_the_offset_in_words_two_and_three():
    c0, c1, c2, c3 = G.start_counters(4 * 1000 + 2, (9 << 32) + 12)
    assert np.array_equal(c0, np.arange(1001)) and not c1.any()  # (a quad index past 2^32 would carry into word 1)
    assert set(c2.tolist()) == {12 ^ 0xFF000000} and set(c3.tolist()) == {9}


@pytest.mark.parametrize("offset", [0, 4, 8, (1 << 24) - 4, (3 << 32) + 4860, 0xFF000000, 0xFFFFFFFC])
def test_start_shares_no_counter_with_the_dropout_and_permutation_draws_of_its_block(offset):
    word2 = G.start_counter_word2(offset)
    assert word2 == (offset & 0xFFFFFFFF) ^ 0xFF000000
    dropout_word2 = {D.counter_word2(site, offset) for site in range(D.MAX_SITES)}
    assert D.MAX_SITES <= G.START_SITE and word2 not in dropout_word2
    assert word2 != offset & 0xFFFFFFFF  # the permutation draw's word 2 (perm_reference.keys)
    # ... and in full counters, for a geometry's used set: (i0, i1, word 2, word 3) tuples are disjoint
    hi = (offset >> 32) & 0xFFFFFFFF
    c0, c1, c2, c3 = G.start_counters(4 * 32 * 32 * 3, offset)
    mine = set(zip(c0.tolist(), c1.tolist(), c2.tolist(), c3.tolist()))
    theirs = set()
    for site in D.sites(s=2, f=4, n=2, h=32, w=32, dropout2d=(0.1, 0.1, 0.1), center=0.1, final=0.1):
        i0, i1, _ = D.used_counters(site)
        theirs |= {(a, b, D.counter_word2(site["site"], offset), hi) for a, b in zip(i0.tolist(), i1.tolist())}
    for stream in range(1 + 3):
        theirs |= {(j >> 1, stream, offset & 0xFFFFFFFF, hi) for j in range(64)}
    assert theirs and not (mine & theirs)


def test_reference_sweep_applies_the_chunk_rule():
    assert G.level_chunks(2, 5, 64) == [(0, 2)] and G.level_chunks(5, 32, 64) == [(0, 2), (2, 4), (4, 5)]
    assert G.level_chunks(3, 100, 64) == [(0, 1), (1, 2), (2, 3)] and G.level_chunks(3, 2, 64, mc_dropout=True) == [(0, 1), (1, 2), (2, 3)]
    assert G.level_chunks(0, 5, 64) == []
    assert G.step_sizes([0.0, 0.02, 0.04], 10) == [0.0, 2.5 * 0.02 / 10, 2.5 * 0.04 / 10] and G.step_sizes([0.02], 4, 0.01) == [0.01]
    from mimo_unet_amd.adversarial import pgd_level_chunks, pgd_step_sizes
    for levels, batch, limit, mc in ((2, 5, 64, False), (5, 32, 64, False), (3, 100, 64, False), (3, 2, 64, True), (0, 5, 64, False)):
        assert pgd_level_chunks(levels, batch, limit, mc) == G.level_chunks(levels, batch, limit, mc)
    assert list(pgd_step_sizes([0.0, 0.02, 0.04], 10, None, 2.5)) == G.step_sizes([0.0, 0.02, 0.04], 10)
    calls = []
    x0 = np.random.default_rng(8).uniform(0, 1, (2, 3, 4, 4)).astype(np.float32)

    def gradient(stacked, levels):
        calls.append((stacked.shape[0], levels))
        return np.cos(37.0 * stacked)

    out = G.reference_sweep(gradient, x0, (0.02, 0.0, 0.04, 0.06), steps=3, limit=4)
    assert calls == [(4, 2), (2, 1)] * 3  # the three eps > 0 levels, two per call of B = 2; eps = 0 takes no gradient
    assert np.array_equal(out[0.0], x0) and list(out) == [0.02, 0.0, 0.04, 0.06]
    single = G.reference_sweep(gradient, x0, (0.04,), steps=3, limit=64)
    assert np.array_equal(out[0.04], single[0.04])  # per-sample gradient: a level's trajectory does not depend on its neighbours


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
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(CSRC)/pgd.hip" in makefile


def _member(S=2, **drop):
    from mimo.models.mimo_unet import MimoUnetModel
    kw = dict(center_dropout_rate=0.0, final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
              decoder_dropout_rate=0.0)
    kw.update(drop)
    return MimoUnetModel(in_channels=2, out_channels=2, num_subnetworks=S, filter_base_count=2, loss="laplace_nll", weight_decay=0.0,
                         learning_rate=1e-3, seed=0, loss_buffer_size=10, loss_buffer_temperature=0.3, **kw)


def test_pgd_sweep_rejects_bad_requests_before_touching_a_gpu():
    """CPU tensors on a CPU-only host: every refusal is a ValueError / NotImplementedError of the validation, never the
    MimoHipError (or CUDA error) a GPU touch would raise."""
    from mimo.adversarial import RobustnessEvaluator, pgd_sweep
    from mimo.models.ensemble import EnsembleModule
    from mimo.models.evidential_unet import EvidentialUnetModel
    image, label = torch.rand(1, 2, 32, 32), torch.rand(1, 1, 32, 32)
    plain = EnsembleModule([], models=[_member()])
    for kw, match in ((dict(steps=0), "steps"), (dict(steps=-3), "steps"), (dict(steps=2.5), "steps"),
                      (dict(step_size=-0.01), "step_size"), (dict(step_size=float("nan")), "step_size"),
                      (dict(rel_step_size=0.0), "rel_step_size"), (dict(rel_step_size=float("nan")), "rel_step_size")):
        with pytest.raises(ValueError, match=match):
            pgd_sweep(plain, image, label, (0.0, 0.02), **kw)
        with pytest.raises(ValueError, match=match):
            RobustnessEvaluator(attack="pgd", **kw)
    # the refusals of fgsm_sweep, in the same way
    mc = EnsembleModule([], monte_carlo_steps=3, models=[_member(encoder_dropout_rate=0.1)])
    with pytest.raises(NotImplementedError, match="MC-dropout"):
        pgd_sweep(mc, image, label, (0.0, 0.02))
    ev = EvidentialUnetModel(in_channels=2, out_channels=4, filter_base_count=2, center_dropout_rate=0.0, final_dropout_rate=0.0,
                             encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0,
                             learning_rate=1e-3, seed=0)
    with pytest.raises(NotImplementedError, match="evidential"):
        pgd_sweep(EnsembleModule([], models=[ev]), image, label, (0.0,))
    with pytest.raises(NotImplementedError, match="negative"):
        pgd_sweep(plain, image, label, (0.0, -0.02))
    with pytest.raises(ValueError, match="duplicate"):
        pgd_sweep(plain, image, label, (0.02, 0.02))
    with pytest.raises(ValueError, match="no epsilons"):
        pgd_sweep(plain, image, label, ())
    # an unknown attack (a valid one goes on to build its evaluators on the GPU: tests/test_pgd_gpu.py)
    with pytest.raises(ValueError, match="unknown attack"):
        RobustnessEvaluator(attack="cw")
    with pytest.raises(NotImplementedError, match="non-negative"):
        RobustnessEvaluator(epsilons=(0.02, -0.01), attack="pgd")
