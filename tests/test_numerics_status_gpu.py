"""The numerics status word (mimo_plan_status; kStatusFwdStats 1, kStatusBwdStats 2, kStatusLogits 4), one raising site at a
time.  Every site is a single atomicOr behind an isfinite; a rewrite that loses one passes every parity test, so each site
gets a case here that only it can satisfy.

A. The operator entry points that return a status (mimo_op_bn_relu_backward, _bn_stats, _bn_relu_forward, _head_forward): a
   clean run (status 0), then one poisoned element (NaN, +inf, -inf): the exact flag, and every channel the poison cannot
   reach bit-identical to the clean run.
B. A whole plan with ONE dead channel: a NaN in one element of a convolution's bias makes that output channel NaN, the layer's
   own check sees it, the ReLU's fmaxf turns the channel into zeros and everything downstream is finite again — so the logits
   are finite, bit 4 stays clear and exactly the site named in the case's docstring can have raised bit 1.

Every assertion is exact (a flag value, bit-equality with the clean run): no tolerance.

Every raising site in csrc/ (an atomicOr on a status pointer; the convolution epilogues write the literal 1) and the cases
that fail when that atomicOr alone is removed — checked once by building the library without it and running this file:
  ew_bn_bwd.hip    bn_bwd_stats_kernel       test_bn_relu_backward_reports_* (all 16), test_plan_backward_sum_raises_bit_2_*
  ew_bn_fwd.hip    bn_fwd_finalize_channel   test_bn_stats_reports_a_non_finite_partial_on_every_route (all 13: through
                                             bn_fwd_stats_kernel on the one-launch routes, through bn_fwd_finalize_kernel on the
                                             rowsum routes), test_plan_training_forward_batch_statistics,
                                             test_plan_rowsum_route_of_a_training_forward
                   bn_eval_prepare_kernel    test_bn_stats_eval_mode_reports_poisoned_running_statistics,
                                             test_plan_eval_poisoned_running_var
                   bn_relu_fwd_kernel        test_bn_relu_forward_reports_*[*-plain], test_plan_eval_autograd_pass[plain-*]
                   bn_relu_pool_fwd_kernel   test_bn_relu_forward_reports_*[*-pooled], test_plan_eval_autograd_pass[pooled-*]
  ew_head_loss.hip head_fwd_kernel           test_head_forward_reports_a_non_finite_logit (all 24), test_plan_head_weight_raises_bit_4
  conv_bf16x3.hip  conv3x3_ws_kernel         test_plan_folded_epilogue[ws]
                   conv3x3_bf16x3_kernel     test_plan_folded_epilogue[small_image], test_plan_folded_epilogue_under_switches[fallback]
                   wabsmax_jobs_kernel       none: test_plan_infinite_weight reaches it, but no input separates it from the
                                             layer's epilogue (see that test)
  conv_wide.hip    epilogue                  test_plan_folded_epilogue_under_switches[wide]
  conv3x3.hip      epilogue                  test_plan_folded_epilogue[fp32], test_plan_folded_epilogue_under_switches[fallback]
  conv_thin.hip    epilogue                  test_plan_folded_epilogue[thin]
Before bn_fwd_finalize_kernel was given the status pointer, the rowsum cases failed: ...on_every_route[rows{1,17,2048,2049,4100}-
rowsum], [rows{2049,4100}-plan_rule] and test_plan_rowsum_route_of_a_training_forward.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import ew_bwd_reference as E
from tests import ew_fwd_reference as F
from tests.helpers import cfg_from_meta, load_npz, state_from
from tests.test_ew_bwd_kernels_gpu import bits, head_src_to_device, run_bn
from tests.test_ew_fwd_kernels_gpu import EPS, MOM, bn_params, bn_relu_call, bn_stats_call, head_call

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
POISONS = (NAN, INF, -INF)
FWD, BWD, LOGITS = F.STATUS_FWD_STATS, 2, F.STATUS_LOGITS


# ==== A.1 mimo_op_bn_relu_backward =================================================================================================
# The arriving gradient g is multiplied by the Dropout2d multiplier and then SELECTED by the ReLU gate (relu_gate4:
# fmaf(z, scale, shift) > 0 ? g : 0; ew_bwd_reference.bn_relu_bwd: torch.where(gate, dy, 0)) — never multiplied by it.  So a
# non-finite g behind a closed gate contributes an exact 0 to both sums and the status stays 0; behind an open gate it
# reaches s1 = sum dy and s2 = sum dy xhat of its channel, and bn_bwd_stats_kernel raises kStatusBwdStats.
# A non-finite z: the gate is closed for a NaN (a comparison with NaN is false) and for an infinity of the wrong sign, but s2
# adds dy * (z - mean) * invstd = 0 * NaN (or 0 * inf) = NaN: the status is raised whatever the gate — asserted below.
# The kernels are per-channel independent except through the head source: GS_HEAD forms g = dlogit w for EVERY channel of the
# pixel from the same two dlogit values, so a non-finite label / dout element poisons every channel whose gate is open at that
# pixel.  Which channels the poison reaches is taken from the fp64 reference (non-finite dbeta or dgamma), the status follows.

BWD_PIXELS = {(3, 4, 5), (37, 3, 3), (37, 7, 7), (1, 9, 8)}  # (37, 7, 7): the pooled tensor whose pooled size is 3 x 3


def bwd_geometries(kind):
    return [g for g in E.bn_geometries(kind) if g[:3] in BWD_PIXELS]


def z_for(case, c, pre):
    """the stored z that makes channel c's gate argument z * scale + shift about `pre` (+1: open, -1: closed)"""
    v = case["v"]
    return float(E.round_to(torch.tensor((pre - float(v["shift"][c])) / float(v["scale"][c])), case["prec"]))


def prepare_gates(case, flip):
    """Fixes the gates of the elements the poisons go to (part of the case: the clean run sees the same z).  Returns the list
    of (tensor name, index, channels expected non-finite) — one entry per (position, channel) of the issue's list."""
    kind, N, H, W, C = (case[k] for k in ("kind", "N", "H", "W", "C"))
    z, src = case["z"], case["src"]
    first, last = (0, 0, 0), (N - 1, H - 1, W - 1)
    targets = []
    if kind == E.GS_HEAD:  # every channel of the pixel: open at one end, closed at the other
        for pix, open_ in ((first, not flip), (last, flip)):
            for c in range(C):
                z[pix + (c,)] = z_for(case, c, 1.0 if open_ else -1.0)
            n, yx = pix[0], pix[1] * W + pix[2]
            reached = list(range(C)) if open_ else []
            if src["dloss"] is not None:
                m = int(src["perm"][src["s"]][n]) if src["perm"] is not None else n
                targets.append(("label", (m, 0, yx), reached))
            if src["dout"] is not None:
                targets.append(("dout", (n, src["s"], 1, yx), reached))
        return targets
    # (position, channel): open at (first, 0) and (last, C - 1), closed at (first, C - 1) and (last, 0); flip swaps them
    plan = [(first, 0, not flip), (first, C - 1, flip), (last, C - 1, not flip), (last, 0, flip)]
    if C == 1:  # (one channel: one gate per position)
        plan = [plan[0], plan[2]]
    if kind != E.GS_POOL:
        for pix, c, open_ in plan:
            z[pix + (c,)] = z_for(case, c, 1.0 if open_ else -1.0)
            idx = pix + (c,) if kind == E.GS_PLAIN else (pix[0], pix[1] + 1, pix[2] + 1, c)
            targets.append(("da" if kind == E.GS_PLAIN else "dxpad", idx, [c] if open_ else []))
        return targets
    # pooled: the gradient arrives at the FIRST maximum of a window; all four members get the same z, so the first member takes
    # it and its gate is the window's (four pre-activations of -1: four zeros, the first takes the gradient behind a closed gate)
    Hp, Wp = H // 2, W // 2
    for (n, y, x), c, open_ in plan:
        py, px = (0, 0) if (n, y, x) == first else (Hp - 1, Wp - 1)
        z[n, 2 * py:2 * py + 2, 2 * px:2 * px + 2, c] = z_for(case, c, 1.0 if open_ else -1.0)
        targets.append(("dxpad", (n, py + 1, px + 1, src["choff"] + c), [c] if open_ else []))
    if src.get("skip") is not None:  # the skip gradient arrives at its own pixel, the last row / column of an odd size included
        for pix, c, open_ in plan:
            z[pix + (c,)] = z_for(case, c, 1.0 if open_ else -1.0)  # (inside a window: the value the window already holds)
            targets.append(("skip", (pix[0], pix[1] + 1, pix[2] + 1, src["skoff"] + c), [c] if open_ else []))
    return targets


def reference_reach(case):
    """bool [C]: channels whose dbeta or dgamma is not finite in the fp64 reference"""
    kind, C, src, v = case["kind"], case["C"], case["src"], case["v"]
    d = lambda t: t.double() if isinstance(t, torch.Tensor) and t.is_floating_point() else t
    s = {k: d(x) for k, x in src.items()}
    z, mask = case["z"][..., :C].double(), d(case["mask"])
    sc, sh, mu, inv = (v[k][:C].double() for k in ("scale", "shift", "mean", "invstd"))
    r = E.bn_relu_bwd(E.source_gradient(kind, s, z, sc, sh, mask), z, sc, sh, mu, inv, mask, False)
    return ~(torch.isfinite(r["dbeta"]) & torch.isfinite(r["dgamma"]))


def with_poison(case, name, idx, value, in_z=False):
    c2 = dict(case)
    if in_z:
        c2["z"] = case["z"].clone()
        c2["z"][idx] = value
    else:
        c2["src"] = dict(case["src"])
        c2["src"][name] = case["src"][name].clone()
        c2["src"][name][idx] = value
        head_src_to_device(c2)
    return c2


def assert_other_channels_identical(got, clean, reached, C, Cp, kind, what):
    keep = [c for c in range(C) if c not in reached]
    pad = keep + list(range(C, Cp))
    for k in ("dgamma", "dbeta", "dbias"):
        assert torch.equal(bits(got[k][keep]), bits(clean[k][keep])), (what, k)
    for k in ("c1", "c2"):
        assert torch.equal(bits(got[k][pad]), bits(clean[k][pad])), (what, k)
    assert torch.equal(bits(got["dz"][..., pad]), bits(clean["dz"][..., pad])), (what, "dz")


def backward_status_cases(kind, training, prec):
    for i, (N, H, W, C, Cp) in enumerate(bwd_geometries(kind)):
        masked = True if prec != "fp32" else bool(i & 1)
        case = head_src_to_device(E.bn_case(kind, N, H, W, C, Cp, masked, prec=prec, seed=40 + i, variant=i))
        targets = prepare_gates(case, flip=bool(i & 2))
        head_src_to_device(case)
        clean = run_bn(case, training)
        what = f"kind {kind} {N}x{H}x{W} C {C}/{Cp} training {training} {prec}"
        assert clean["status"] == 0, what
        assert not bool(reference_reach(case).any()), what
        for name, idx, reached in targets:
            for value in POISONS:
                bad = with_poison(case, name, idx, value)
                ref = reference_reach(bad).nonzero().flatten().tolist()
                assert ref == reached, (what, name, idx, value, "the reference disagrees with the gate this case set")
                got = run_bn(bad, training)
                assert got["status"] == (BWD if reached else 0), (what, name, idx, value, got["status"])
                for c in reached:
                    assert not bool(torch.isfinite(got["dbeta"][c]) & torch.isfinite(got["dgamma"][c])), (what, name, idx, value, c)
                assert_other_channels_identical(got, clean, reached, C, Cp, kind, (what, name, idx, value))
        # a padding channel of the arriving gradient (scale = shift = 0: its gate is closed, and the status test is c < C)
        if C < Cp and kind != E.GS_HEAD:
            name = {E.GS_PLAIN: "da", E.GS_FOLD: "dxpad", E.GS_POOL: "dxpad"}[kind]
            idx = {E.GS_PLAIN: (0, 0, 0, C), E.GS_FOLD: (0, 1, 1, C), E.GS_POOL: (0, 1, 1, case["src"].get("choff", 0) + C)}[kind]
            got = run_bn(with_poison(case, name, idx, NAN), training)
            assert got["status"] == 0, (what, "padding channel")
            assert_other_channels_identical(got, clean, [], C, Cp, kind, (what, "padding channel"))
        # z itself: 0 * NaN in the second sum, whatever the gate (see above); the other channels untouched
        for pix, c in (((0, 0, 0), 0), ((N - 1, H - 1, W - 1), C - 1)):
            for value in (NAN, INF):
                got = run_bn(with_poison(case, None, pix + (c,), value, in_z=True), training)
                assert got["status"] == BWD, (what, "z", pix, c, value, got["status"])
                assert not bool(torch.isfinite(got["dgamma"][c])), (what, "z", pix, c, value)
                assert_other_channels_identical(got, clean, [c], C, Cp, kind, (what, "z", pix, c, value))
                if kind == E.GS_HEAD:  # the head's weight gradient reads the activation of this tensor: one column
                    keep = [k for k in range(C) if k != c]
                    assert torch.equal(bits(got["head_dw"][:, keep]), bits(clean["head_dw"][:, keep])), (what, "head_dw")
                    assert torch.equal(bits(got["head_db"]), bits(clean["head_db"])), (what, "head_db")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind", [E.GS_PLAIN, E.GS_FOLD, E.GS_POOL, E.GS_HEAD], ids=["plain", "fold", "pool", "head"])
def test_bn_relu_backward_reports_a_non_finite_gradient_behind_an_open_gate(kind, training):
    backward_status_cases(kind, training, "fp32")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("prec", ["bf16-mixed", "16-mixed"])
@pytest.mark.parametrize("kind", [E.GS_PLAIN, E.GS_FOLD], ids=["plain", "fold"])
def test_bn_relu_backward_reports_in_16_bit_storage(kind, prec, training):
    backward_status_cases(kind, training, prec)


# ==== A.2 mimo_op_bn_stats =========================================================================================================

STATS_ROWS = (1, 17, 2048, 2049, 4100)
ROUTE_IDS = {F.ROUTE_ONE: "one_launch", F.ROUTE_ROWSUM: "rowsum", F.ROUTE_PLAN: "plan_rule"}
STATS_CASES = [(rows, route) for rows in STATS_ROWS for route in (F.ROUTE_ONE, F.ROUTE_ROWSUM, F.ROUTE_PLAN)
               if not (route == F.ROUTE_ONE and rows > F.K_COLSUM_MAX_ROWS)]


@pytest.mark.parametrize("rows,route", STATS_CASES, ids=[f"rows{r}-{ROUTE_IDS[k]}" for r, k in STATS_CASES])
def test_bn_stats_reports_a_non_finite_partial_on_every_route(rows, route):
    """One non-finite partial in the LAST row.  rows <= 2048 on the one-launch route and on the plan's rule: bn_fwd_stats_kernel;
    the rowsum route at every row count and the plan's rule beyond 2048 rows: rowsum + bn_fwd_finalize_kernel, which passed no
    status word before this file existed."""
    for j, (C, Cp, cout_pad) in enumerate(F.BN_CHANNELS[:2]):
        g = F.gen(3300 + rows + j)
        part = F.partial_rows(rows, C, cout_pad, g)
        gamma, beta, rm, rv = bn_params(C, g)
        call = lambda p_: bn_stats_call(p_, rows, cout_pad, C, Cp, rows * 64, gamma, beta, rm, rv, MOM, EPS, route)
        clean, status, _ = call(part)
        assert status == 0
        spots = [(0, c, v) for c in (0, C - 1) for v in POISONS] + [(1, C // 2, INF)]  # (1, ...): the sum of squares alone
        for col, c, value in spots:
            bad = part.clone()
            bad[rows - 1, col, c] = value
            got, status, _ = call(bad)
            assert status == FWD, (rows, route, C, col, c, value, status)
            # (an infinite sum of squares alone: invstd = scale = 0 and a finite shift — the running variance shows it)
            assert not all(bool(torch.isfinite(got[k][c])) for k in F.BN_OUTPUTS), (rows, route, c, value)
            keep = [k for k in range(C) if k != c]
            assert all(torch.equal(bits(got[k][keep]), bits(clean[k][keep])) for k in F.BN_OUTPUTS), (rows, route, c, value)
        bad = part.clone()       # a padding channel (c <= column < c_p) and a column beyond c_p: never finalized
        bad[rows - 1, 0, C], bad[rows - 1, 1, Cp] = NAN, INF
        got, status, _ = call(bad)
        assert status == 0, (rows, route, "padding")
        assert all(torch.equal(bits(got[k]), bits(clean[k])) for k in F.BN_OUTPUTS)


def test_bn_stats_eval_mode_reports_poisoned_running_statistics():
    """bn_eval_prepare_kernel: mean, invstd or scale not finite (a NaN / negative running variance, an infinite running mean or
    gamma); the other channels bit for bit."""
    g = F.gen(3400)
    C, Cp, cout_pad = 5, 8, 16
    gamma, beta, rm, rv = bn_params(C, g)
    part = F.partial_rows(1, C, cout_pad, g)
    call = lambda ga, m, v: bn_stats_call(part, 0, cout_pad, C, Cp, 0, ga, beta, m, v, MOM, EPS, F.ROUTE_PLAN, training=0)
    clean, status, _ = call(gamma, rm, rv)
    assert status == 0
    for which, value in ((2, NAN), (2, INF), (2, -1.0), (1, INF), (1, NAN), (0, INF), (0, NAN)):
        for c in (0, C - 1):
            v = [gamma.clone(), rm.clone(), rv.clone()]
            v[which][c] = value
            got, status, _ = call(*v)
            # (an infinite running variance gives invstd = 0, scale = 0: finite, a channel of constant `beta` and no dead one)
            expect = 0 if (which, value) == (2, INF) else FWD
            assert status == expect, (which, value, c, status)
            keep = [k for k in range(C) if k != c]
            assert all(torch.equal(bits(got[k][keep]), bits(clean[k][keep])) for k in ("mean", "invstd", "scale", "shift"))


# ==== A.3 mimo_op_bn_relu_forward ==================================================================================================

FWD_GEOMS = [(2, 5, 7, 5, 8), (1, 9, 8, 13, 16)]   # odd H and odd W; one odd direction, c_p of two quads


@pytest.mark.parametrize("pooled", [False, True], ids=["plain", "pooled"])
@pytest.mark.parametrize("prec,z_fp32", [("fp32", 0), ("bf16-mixed", 0), ("bf16-mixed", 1), ("16-mixed", 0), ("16-mixed", 1)],
                         ids=["fp32", "bf16", "bf16_zfp32", "fp16", "fp16_zfp32"])
def test_bn_relu_forward_reports_a_non_finite_pre_activation(prec, z_fp32, pooled):
    """Eval mode (a status pointer is given).  The poisoned channel has a positive scale: relu(NaN) is dropped to 0 by fmaxf,
    the activation of a dead channel — only the status tells.  Positions: first pixel, and the last row / last column / corner,
    which lie outside every full 2x2 window of the pooled kernel when the size is odd (its three tail branches).
    (These kernels test whole channel quads, padding channels included: a non-finite PADDING channel of z raises the bit as
    well.  The plan's convolutions write zeros there, so nothing is asserted about it.)"""
    for i, geom in enumerate(FWD_GEOMS):
        N, H, W, C, Cp = geom
        c = F.bn_relu_case(200 + i, geom, "fp32" if z_fp32 else prec, bool(i & 1), pooled=pooled)
        c["scale"] = c["scale"].clone()
        c["scale"][[0, C - 1]] = c["scale"][[0, C - 1]].abs()
        a0, pool0, status = bn_relu_call(c, prec, pooled, None, z_fp32)
        assert status == 0
        for pix in ((0, 0, 0), (N - 1, H - 1, W - 1), (0, H - 1, 0), (0, 0, W - 1), (N - 1, H - 1, W - 2), (N - 1, H - 2, W - 1)):
            for ch in (0, C - 1):
                for value in POISONS:
                    z = c["z"].clone()
                    z[pix + (ch,)] = value
                    a, pool, status = bn_relu_call(c, prec, pooled, z, z_fp32)
                    assert status == FWD, (prec, z_fp32, pooled, geom, pix, ch, value, status)
                    keep = [k for k in range(Cp) if k != ch]
                    assert torch.equal(bits(a[..., keep]), bits(a0[..., keep])), (geom, pix, ch, value)
                    if pooled:
                        assert torch.equal(bits(pool[..., keep]), bits(pool0[..., keep])), (geom, pix, ch, value)
                    if value != value:  # the NaN is gone from the output: a silently dead element
                        assert float(a[pix + (ch,)]) == 0.0


# ==== A.4 mimo_op_head_forward =====================================================================================================

@pytest.mark.parametrize("HW", [7, 64])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("prec", ["fp32", "bf16-mixed", "16-mixed"])
def test_head_forward_reports_a_non_finite_logit(prec, fused, S, HW):
    """An activation of 60000 (inside fp16) in channel 0 against a weight of 3e34 in logit 1 only: the product overflows fp32, exactly
    one logit is not finite (fused: channel 0 carries bn_vectors' scale 0.5 / shift -1.5, the activation is 29998.5).  Then,
    unfused, a NaN activation (the logits of one pixel) and a NaN weight (one logit channel)."""
    C, Co, N = 13, 2, 2
    s = S - 1
    c = F.head_case(60 + HW + S, C, Co, N, HW, prec, fused)
    c["w"][1, 0], c["w"][0, 0] = 3e34, 0.5
    clean, status = head_call(c, C, Co, N, S, s, HW, prec, fused)
    assert status == 0 and bool(torch.isfinite(clean[:, s]).all())
    for (n, yx) in ((0, 0), (N - 1, HW - 1)):
        a = c["a"].clone()
        a[n, yx, 0] = 60000.0
        out, status = head_call(c, C, Co, N, S, s, HW, prec, fused, a=a.cuda())
        assert status == LOGITS, (prec, fused, S, HW, n, yx, status)
        bad = ~torch.isfinite(out[:, s].cpu())
        assert int(bad.sum()) == 1 and bool(bad[n, 1, yx])
        same = torch.ones(N, Co, HW, dtype=torch.bool)
        same[n, :, yx] = False  # (logit 0 of the pixel is finite and different: 0.5 x the large activation)
        assert torch.equal(bits(out[:, s])[same], bits(clean[:, s])[same])
        if not fused:  # (fused: the ReLU drops a NaN pre-activation before the head sees it)
            a = c["a"].clone()
            a[n, yx, C - 1] = NAN
            out, status = head_call(c, C, Co, N, S, s, HW, prec, fused, a=a.cuda())
            assert status == LOGITS
            assert bool((~torch.isfinite(out[:, s].cpu()) == ~same).all())
            assert torch.equal(bits(out[:, s])[same], bits(clean[:, s])[same])
    for value in POISONS:
        c2 = dict(c, w=c["w"].clone())
        c2["w"][0, C - 1] = value
        out, status = head_call(c2, C, Co, N, S, s, HW, prec, fused)
        assert status == LOGITS, (prec, fused, value)
        assert torch.equal(bits(out[:, s, 1]), bits(clean[:, s, 1])), "the other logit channel"


# ==== B. one site of a plan at a time ================================================================================================
# The fixture network (mini_s2_step.npz: 2 subnetworks, filter_base_count 4, 3 images of 32 x 32) and where its layers run
# (conv_recipe.h; the layer's padded input channels and image size decide):
#   encoder.in_convs.S.double_conv.0   2 -> 4 at 32 x 32, the packed image: conv_thin.hip (MIMO_CONV_THIN=0: conv3x3.hip)
#   core.down2.conv.double_conv.0      16 -> 32 at 8 x 8: split16 on conv3x3_bf16x3_kernel (fewer than 256 pixels: never
#                                      wave-specialised); its second convolution's output is pooled (down3 reads it)
#   core.up3.conv.double_conv.0        32 -> 16 at 16 x 16: split16 on conv3x3_ws_kernel; MIMO_CONV_WS=0 MIMO_CONV_WIDE=0:
#                                      conv3x3_bf16x3_kernel; MIMO_CONV_WIDE=2: conv_wide.hip; precision fp32: conv3x3.hip
# wabsmax_jobs_kernel (the weight-pack check) reads weights only: a NaN BIAS does not reach it.  bn_eval_prepare_kernel sees
# gamma and the running statistics only.  So a NaN bias reaches exactly the layer's own epilogue / statistics / activation pass.
# (The fp16 range guard looks at the BatchNorm weights and biases alone, which no case here touches: the precision stays.)

UP3, DOWN2, DOWN2_POOLED, IMAGE = ("core.up3.conv.double_conv.0", "core.down2.conv.double_conv.0", "core.down2.conv.double_conv.3",
                                   "encoder.in_convs.0.double_conv.0")


@functools.lru_cache(maxsize=None)
def fixture():
    fx = load_npz("mini_s2_step.npz")
    return fx, cfg_from_meta(fx["meta"])


def fresh_model(precision):
    from tests.test_network_gpu import build_model
    fx, cfg = fixture()
    model = build_model(cfg, state_from(fx, "init/"), precision=precision)
    assert model.model._geom.precision == precision
    return model


def inputs(n=3):
    g = torch.Generator().manual_seed(3)
    image, label = torch.rand(n, 2, 32, 32, generator=g), torch.rand(n, 1, 32, 32, generator=g)
    perms = torch.stack([torch.randperm(n, generator=g) for _ in range(2)])
    return image.cuda(), label.cuda(), perms.cuda()


def forward(model, mode, image, label, perms):
    """the logits [N, S, Co, H, W] of one forward: eval under no_grad (folded epilogue), eval with autograd (separate BatchNorm +
    ReLU pass), training (batch statistics)"""
    if mode == "train":
        model.train()
        out, _ = model.model.forward_with_loss(image, label, None, perms)
        return out
    model.eval()
    x5 = image[:, None].repeat(1, 2, 1, 1, 1)
    if mode == "eval_no_grad":
        with torch.no_grad():
            return torch.cat(model(x5), 2)
    return torch.cat(model(x5), 2)


def poison(model, key, idx, value):
    net = model.model
    t = dict(net.named_parameters()).get(key)
    if t is None:
        t = dict(net.named_buffers())[key]
    with torch.no_grad():
        t[idx] = value
    net.mark_parameters_changed()


def dead_channel_case(precision, mode, key, idx=0, value=NAN, n=3, bit=FWD):
    """clean forward: status 0, finite logits.  Poisoned forward: exactly `bit`, bit 4 clear, the logits all finite (no later
    site can have fired), and the word is cleared by the read."""
    model = fresh_model(precision)
    net = model.model
    args = inputs(n)
    out = forward(model, mode, *args)
    assert bool(torch.isfinite(out).all()) and net.numerics_status() == 0
    poison(model, key, idx, value)
    out = forward(model, mode, *args)
    status = net.numerics_status(clear=False)
    assert status & bit, (precision, mode, key, status)
    assert status == bit and not status & LOGITS, (precision, mode, key, status)
    assert bool(torch.isfinite(out).all()), "a NaN survived the ReLU: a later site could have raised the bit"
    assert net.numerics_status() == bit and net.numerics_status() == 0, "the read clears the word"
    return model


FOLDED = {
    # id: (precision, poisoned bias) — eval forward under no_grad, BatchNorm + ReLU folded into the convolution's epilogue
    "ws": ("split16", UP3 + ".bias"),            # conv_bf16x3.hip conv3x3_ws_kernel, C_EPILOGUE
    "small_image": ("split16", DOWN2 + ".bias"),  # conv_bf16x3.hip conv3x3_bf16x3_kernel (8 x 8: below the 256-pixel rule)
    "fp32": ("fp32", UP3 + ".bias"),             # conv3x3.hip conv3x3_mfma_kernel
    "thin": ("split16", IMAGE + ".bias"),        # conv_thin.hip
}
# the switches are read once per process (test_variants_gpu.py): these run in a child process
SWITCHED = {
    "fallback": ({"MIMO_CONV_WS": "0", "MIMO_CONV_WIDE": "0", "MIMO_CONV_THIN": "0"},
                 [("split16", UP3 + ".bias"),      # conv3x3_bf16x3_kernel at 16 x 16
                  ("split16", IMAGE + ".bias")]),  # the image convolution on conv3x3.hip
    "wide": ({"MIMO_CONV_WIDE": "2"}, [("split16", UP3 + ".bias")]),  # conv_wide.hip
}


@pytest.mark.parametrize("name", sorted(FOLDED))
def test_plan_folded_epilogue(name):
    """Sites reached by the NaN bias: the epilogue of the kernel family named in FOLDED, nothing else."""
    dead_channel_case(FOLDED[name][0], "eval_no_grad", FOLDED[name][1])


def run_switched(name):
    for precision, key in SWITCHED[name][1]:
        dead_channel_case(precision, "eval_no_grad", key)


@pytest.mark.parametrize("name", sorted(SWITCHED))
def test_plan_folded_epilogue_under_switches(name):
    """The same case on the families only a switch reaches (SWITCHED), in a child process that sets it."""
    env = dict(os.environ, **SWITCHED[name][0])
    code = f"from tests.test_numerics_status_gpu import run_switched; run_switched({name!r}); print('switched ok')"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "switched ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("name,key", [("plain", UP3 + ".bias"), ("pooled", DOWN2_POOLED + ".bias")])
def test_plan_eval_autograd_pass(name, key):
    """Eval forward with autograd: the convolution writes z, the separate pass applies BatchNorm + ReLU and tests its input.
    plain: bn_relu_fwd_kernel (the first convolution of up3).  pooled: bn_relu_pool_fwd_kernel (the second convolution of down2,
    whose only spatial reader is down3's MaxPool2d)."""
    dead_channel_case("split16", "eval_autograd", key)


@pytest.mark.parametrize("precision", ["split16", "fp32"])
def test_plan_training_forward_batch_statistics(precision):
    """Training forward: the epilogue's partial sums of the NaN channel reach bn_fwd_stats_kernel -> bn_fwd_finalize_channel (3 x
    16 x 16 pixels: one partial row per tile, far below 2048); the BatchNorm + ReLU passes of a training forward get no status
    pointer.  The channel's scale / shift are NaN and fmaxf drops it in whichever kernel applies them."""
    dead_channel_case(precision, "train", UP3 + ".bias")


def test_plan_rowsum_route_of_a_training_forward():
    """conv3x3_launch (precision fp32) writes one partial row per tile: rows = N * tilesY * tilesX.  pick_tile(32, 32) gives 8 x
    32-pixel tiles (256 pixels, (8 + 2) x (32 + 2) = 340 <= 360 halo pixels): 4 tiles per image, so 513 images of the
    fixture's 32 x 32 leave 2052 > kColsumMaxRows = 2048 rows and convbn_forward takes rowsum_launch + bn_fwd_finalize_launch.
    The poisoned layer is the first convolution of a decoder's up4 block (12 -> 6 at 32 x 32).  The 32 x 32 layers of the
    encoder do not get there: with at most 4 input channels in identity order they all run on conv_thin.hip, whose grid — and
    row count — is capped.  Sites reached: bn_fwd_finalize_kernel -> bn_fwd_finalize_channel.  525 312 pixels: the issue's
    9 x 256 x 256 has 589 824."""
    dead_channel_case("fp32", "train", "decoder.up4s.0.conv.double_conv.0.bias", n=513)


def test_plan_eval_poisoned_running_var():
    """A NaN running variance: bn_eval_prepare_kernel (invstd and scale are NaN).  The folded epilogue tests the convolution's
    output, which is finite, and fmaxf drops the NaN the scale makes of it."""
    dead_channel_case("split16", "eval_no_grad", "core.up3.conv.double_conv.1.running_var")


def test_plan_infinite_weight():
    """One weight of +inf in split16.  wabsmax_jobs_kernel (the weight-pack check) raises the bit — and the fp16 image of that
    weight is (inf, NaN) at any scale, so the output channel is NaN and the layer's epilogue raises it too: the two sites
    cannot be separated by any input (a weight the pack check reports, |w| > 3e38, overflows fp16 at the smallest scale
    2^-100 as well)."""
    dead_channel_case("split16", "eval_no_grad", UP3 + ".weight", idx=(0, 0, 0, 0), value=INF)


def test_plan_backward_sum_raises_bit_2_and_the_epoch_end_check_says_so():
    """A finite training forward, one NaN label: the loss is NaN, the logits are not.  The head's gradient reaches the
    BatchNorm backward of the decoder's last convolution: bn_bwd_stats_kernel, the only site of bit 2."""
    model = fresh_model("split16")
    image, label, perms = inputs()
    model.train()
    out = model.training_step_with_perms(image, label, None, perms)
    out["loss"].backward()
    assert model.model.numerics_status() == 0
    model.on_train_epoch_end()
    model.zero_grad()
    label[1, 0, 5, 7] = NAN
    out = model.training_step_with_perms(image, label, None, perms)
    assert bool(torch.isfinite(out["preds"]).all()) and model.model.numerics_status(clear=False) == 0, "the forward records nothing"
    out["loss"].backward()
    status = model.model.numerics_status(clear=False)
    assert status & BWD and not status & LOGITS, status
    with pytest.raises(FloatingPointError, match="BatchNorm-backward sum was not finite"):
        model.on_train_epoch_end()
    assert model.model.numerics_status() == 0


@pytest.mark.parametrize("mode", ["train", "eval_no_grad"])
def test_plan_head_weight_raises_bit_4(mode):
    """A NaN in one weight of subnetwork 0's 1x1 head: head_fwd_kernel, the only site of bit 4; nothing in front of it is touched."""
    model = fresh_model("split16")
    args = inputs()
    out = forward(model, mode, *args)
    assert bool(torch.isfinite(out).all()) and model.model.numerics_status() == 0
    poison(model, "decoder.outcs.0.conv.weight", (0, 0, 0, 0), NAN)
    out = forward(model, mode, *args)
    status = model.model.numerics_status(clear=False)
    assert status & LOGITS and not status & FWD, status
    assert bool(torch.isnan(out[:, 0, 0]).all()) and bool(torch.isfinite(out[:, 1]).all()) and bool(torch.isfinite(out[:, 0, 1]).all())
    assert model.model.numerics_status() == status and model.model.numerics_status() == 0
