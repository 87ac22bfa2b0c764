"""tests/ew_bwd_reference.py against fp64 autograd through the torch modules the model composes — F.pad(mode="reflect"),
nn.MaxPool2d(2), nn.Upsample(x2, bilinear, align_corners=True) + F.pad + torch.cat, nn.BatchNorm2d (train / eval) + ReLU + a
Dropout2d multiplier, a 1x1 convolution + the host LaplaceNLL / GaussianNLL with a mask — at every geometry the GPU tests
(tests/test_ew_bwd_kernels_gpu.py) run, to fp64 rounding (rtol 1e-12).  Also asserts the properties the generated inputs
must have for the per-element GPU comparison to skip nothing: magnitudes in [2^-20, 2^20], exact-zero gate arguments present,
window members exactly equal or more than 4 ulp apart with ties in every position."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mimo_unet_amd.losses import GaussianNLL, LaplaceNLL
from tests import ew_bwd_reference as E

RTOL = 1e-12


def close(got, ref, what):
    scale = max(float(ref.abs().max()), 1e-300)
    err = float((got - ref).abs().max()) / scale
    assert err <= RTOL, (what, err)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def test_torch_maxpool_tie_rule_on_a_hand_made_window():
    """torch's CPU MaxPool2d tie rule is documented nowhere: pinned here on exact ties.  Expected (scan order, first maximum
    wins): window values -> position that receives the gradient."""
    cases = [([1., 1., 1., 1.], 0), ([0., 2., 2., 1.], 1), ([0., 1., 2., 2.], 2), ([3., 0., 0., 3.], 0), ([0., 0., 0., 0.], 0),
             ([1., 5., 1., 5.], 1), ([-1., -2., -1., -1.], 0)]
    for vals, want in cases:
        a = torch.tensor(vals, dtype=torch.float64).reshape(1, 2, 2, 1)
        assert int(E.first_max(a).reshape(4).nonzero()) == want, vals            # the hand-made expectation: the reference's rule
        x = nchw(a).requires_grad_(True)
        nn.MaxPool2d(2)(x).sum().backward()
        assert int(nhwc(x.grad).reshape(4).nonzero()) == want, ("torch's CPU tie rule differs from scan order", vals)


@pytest.mark.parametrize("N,H,W,Cp", E.fold_pool_geometries() + [E.PAST_GRID_BN], ids=str)
def test_fold_is_the_transpose_of_reflect_padding(N, H, W, Cp):
    g = E.gen(1)
    C = min(Cp, 8)  # (channels are independent: the geometry is what varies)
    dxpad = E.padded_grad(N, H, W, C, g).double()
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    (F.pad(x, (1, 1, 1, 1), mode="reflect") * nchw(dxpad)).sum().backward()
    close(E.fold(dxpad), nhwc(x.grad), "fold")


@pytest.mark.parametrize("N,H0,W0,Cp", E.fold_pool_geometries() + [E.PAST_GRID_POOLED_BN], ids=str)
def test_pool_bwd_against_maxpool_autograd_with_planted_ties(N, H0, W0, Cp):
    H, W = E.pool_size(H0, W0)
    g = E.gen(2)
    C = min(Cp, 8) - 3
    v = E.bn_vectors(C, 8, g)
    mask = E.dropout_mask(N, C, g, True)
    z, _ = E.pooled_preact(N, H, W, C, 8, 8, v, mask, g)
    a32 = E.act32(z[..., :C], v["scale"][:C], v["shift"][:C], mask)
    assert not bool(E.window_gap_violations(a32).any())
    sel = E.first_max(a32)
    win = E.windows(a32)
    ties = (win == win.max(-1, keepdim=True).values).sum(-1)
    if N * (H // 2) * (W // 2) >= 13:  # every planted group was placed: tied maxima of 2, 3 and 4 members, in every position
        tied = (win == win.max(-1, keepdim=True).values) & (ties >= 2).unsqueeze(-1)
        assert {2, 3, 4} <= set(ties.unique().tolist()) and all(bool(tied[..., j].any()) for j in range(4))
        assert all(bool(sel[..., j].any()) for j in range(3))  # (position 3 wins only without a tie)
        assert bool(((win == 0).all(-1)).any()), "an all-zero window"
    gp = torch.randn(N, H // 2, W // 2, C, generator=g, dtype=torch.float64)
    skip = E.padded_grad(N, H, W, C, g).double()
    # torch ties: a distinct tiny bias in scan order makes torch's choice the first maximum whatever its own tie rule is; the
    # bias stays below a quarter of the smallest gap between two distinct members of any window
    x = nchw(a32.double()).requires_grad_(True)
    gaps = (win.double().unsqueeze(-1) - win.double().unsqueeze(-2)).abs()
    step = float(gaps[gaps > 0].min()) / 16 if bool((gaps > 0).any()) else 1e-9
    bias = (step * torch.tensor([[3.0, 2.0], [1.0, 0.0]], dtype=torch.float64)).repeat((H + 1) // 2, (W + 1) // 2)[:H, :W]
    y = nn.MaxPool2d(2)(x + bias)
    (y * nchw(gp)).sum().backward()
    close(E.pool_bwd(gp, a32.double()), nhwc(x.grad), "pool_bwd")
    close(E.pool_bwd(gp, a32.double(), E.fold(skip)), nhwc(x.grad) + E.fold(skip), "pool_bwd + skip")
    assert float(E.pool_bwd(gp, a32.double())[:, 2 * (H // 2):].abs().sum()) == 0 and \
        float(E.pool_bwd(gp, a32.double())[:, :, 2 * (W // 2):].abs().sum()) == 0


@pytest.mark.parametrize("N,H,W,h,w,Cp", E.up_geometries(), ids=str)
def test_up_bwd_against_upsample_pad_cat_autograd(N, H, W, h, w, Cp):
    g = E.gen(3)
    C, choff = 4, 8
    dxpad = E.padded_grad(N, H, W, choff + C + 4, g).double()
    low = torch.randn(N, C, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    skip = torch.randn(N, choff, H, W, generator=g, dtype=torch.float64)
    up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)(low)
    dy, dx = H - up.shape[2], W - up.shape[3]
    cat = torch.cat([skip, F.pad(up, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])], 1)
    (F.pad(cat, (1, 1, 1, 1), mode="reflect") * nchw(dxpad[..., :choff + C])).sum().backward()
    close(E.up_bwd(dxpad, choff, C, h, w), nhwc(low.grad), "up_bwd")


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("N,H,W,Cp", E.fold_pool_geometries() + [E.PAST_GRID_BN], ids=str)
def test_bn_relu_bwd_against_batchnorm_autograd(N, H, W, Cp, masked, training):
    """BatchNorm2d's own statistics are the inputs here (mean / invstd / scale / shift derived from the module in fp64), so
    that autograd's formula and the reference's see the same numbers.  The ReLU enters as a multiplication by E.gate(): the
    kernel decides on z * scale + shift, autograd's ReLU would decide on bn(x), equal only up to rounding.  The decision
    therefore comes from the reference on both sides; that the gate is strict ('>', closed at exactly 0) is asserted on the
    planted zeros by the input-property tests below, not here."""
    g = E.gen(4)
    C = min(Cp, 16) - 3
    zf = E.preact(N, H, W, C, C, C, g, plant_zero_gates=False)
    assert bool(((zf.abs() >= E.LO) & (zf.abs() <= E.HI)).all())
    z = zf.double()
    bn = nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g).double())
        bn.bias.copy_(torch.randn(C, generator=g).double())
        bn.running_mean.copy_(torch.randn(C, generator=g).double() * 0.2)
        bn.running_var.copy_(torch.rand(C, generator=g).double() + 0.5)
    bn.train(training)
    if training:
        mean, var = z.mean((0, 1, 2)), z.var((0, 1, 2), unbiased=False)
    else:
        mean, var = bn.running_mean.clone(), bn.running_var.clone()
    invstd = (var + bn.eps).rsqrt()
    scale = bn.weight.detach() * invstd
    shift = bn.bias.detach() - mean * scale
    mask = E.dropout_mask(N, C, g, masked)
    gr = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    x = nchw(z).requires_grad_(True)
    pre = bn(x)
    # the gate as the kernel takes it: on z * scale + shift (autograd's own ReLU would decide on bn(x), equal up to rounding)
    gt = nchw(E.gate(z, scale, shift).double())
    y = pre * gt
    if mask is not None:
        y = y * mask.double()[:, :, None, None]
    (y * nchw(gr)).sum().backward()
    r = E.bn_relu_bwd(gr, z, scale, shift, mean, invstd, None if mask is None else mask.double(), training)
    close(r["dz"], nhwc(x.grad), "dz")
    close(r["dgamma"], bn.weight.grad, "dgamma")
    close(r["dbeta"], bn.bias.grad, "dbeta")
    if not training:
        close(r["dbias"], x.grad.sum((0, 2, 3)), "dbias")
    else:
        assert float(x.grad.sum((0, 2, 3)).abs().max()) <= 1e-12 * max(float(x.grad.abs().sum()), 1.0)  # exactly zero in exact arithmetic


def test_generated_bn_inputs_have_the_properties_the_gpu_comparison_needs():
    for (N, H, W, Cp) in E.fold_pool_geometries() + [E.PAST_GRID_BN]:
        for C in E.logical_channels(Cp):
            g = E.gen(5)
            v = E.bn_vectors(C, Cp, g)
            z = E.preact(N, H, W, C, Cp, Cp + 8, g)
            for t in (z[..., :C], v["scale"][:C], v["shift"][:C]):
                assert bool(((t.abs() >= E.LO) & (t.abs() <= E.HI)).all())
            assert float(z[..., C:Cp].abs().max() if C < Cp else 0.0) == 0.0 and bool(torch.isnan(z[..., Cp:]).all())
            arg = z[..., :C].double() * v["scale"][:C].double() + v["shift"][:C].double()
            assert bool((arg[..., 0] == 0).any()) and not bool(E.gate(z[..., :C], v["scale"][:C], v["shift"][:C])[arg == 0].any())
            if C > 1:
                assert bool((arg[..., 1] == 0).any())
            # the fp32 fmaf is correctly rounded: its sign is the exact value's sign; emulated here by rounding the fp64 value
            assert bool(((arg.float() > 0) == (arg > 0)).all())


@pytest.mark.parametrize("kind", [E.LAPLACE, E.GAUSSIAN])
@pytest.mark.parametrize("use_dout,use_dloss", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("N,HW,C,Co,fused", [(3, 20, 5, 2, True), (1, 72, 13, 2, False), (37, 9, 8, 2, True), (2, 30, 5, 4, False)])
def test_head_bwd_against_conv1x1_and_host_nll_autograd(N, HW, C, Co, fused, use_dout, use_dloss, kind):
    g = E.gen(6)
    S, s = 3, 1
    hi = E.head_inputs(N, S, Co, HW, g, use_dout, True, True, True)
    e = torch.exp(hi["out"][:, :, Co // 2:])
    assert bool((e < E.EPS_MIN).any()) and bool((e > E.EPS_MAX).any()) and bool(((e > E.EPS_MIN) & (e < E.EPS_MAX)).any())
    w = torch.randn(Co, C, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
    a0 = torch.randn(N, HW, C, generator=g, dtype=torch.float64)
    v = E.bn_vectors(C, C, g)
    sc, sh = (v["scale"].double(), v["shift"].double()) if fused else (None, None)
    x = a0.clone().requires_grad_(True)
    act = (x * sc + sh) * E.gate(a0, sc, sh) if fused else x
    logits = torch.einsum("npc,oc->nop", act, w) + b[None, :, None]     # the 1x1 convolution
    # the loss is evaluated at the recorded logits `out` (the kernel reads them, it does not recompute them): tie them in
    out = hi["out"].double()
    lg = out[:, s] + (logits - logits.detach())
    loss_fn = (LaplaceNLL if kind == E.LAPLACE else GaussianNLL)(E.EPS_MIN, E.EPS_MAX).double()
    Ct = Co // 2
    total = logits.new_zeros(())
    dloss = hi["dloss"].double()
    if use_dloss:
        src = hi["perm"][s]
        total = total + dloss[s] * loss_fn(lg[:, :Ct], lg[:, Ct:], hi["label"].double()[src], mask=hi["mask"].double()[src][:, None, :])
    if use_dout:
        total = total + (logits * hi["dout"].double()[:, s]).sum()
    total.backward()
    r = E.head_bwd(a0, w.detach(), out if use_dloss else None, hi["dout"].double() if use_dout else None,
                   dloss if use_dloss else None, hi["label"].double(), hi["mask"].double(), hi["perm"], s, kind, E.EPS_MIN,
                   E.EPS_MAX, sc, sh)
    da = r["da"] if not fused else r["da"] * sc * E.gate(a0, sc, sh)   # head_bwd stops at the head's input activation
    close(da, x.grad, "da")
    close(r["dw"], w.grad, "dw")
    close(r["db"], b.grad, "db")


def test_decode_split_round_trip():
    for Cp in (8, 24, 64, 72):
        P = 5
        x = torch.randn(P, Cp)
        hi = x.bfloat16()
        lo = (x - hi.float()).bfloat16()
        raw = torch.zeros(P, 2 * Cp, dtype=torch.int16)
        for c0 in range(0, Cp, 32):
            r = min(32, Cp - c0)
            raw[:, 2 * c0:2 * c0 + r] = hi[:, c0:c0 + r].view(torch.int16)
            raw[:, 2 * c0 + r:2 * c0 + 2 * r] = lo[:, c0:c0 + r].view(torch.int16)
        h, l = E.decode_split(raw.view(torch.float32), Cp)
        assert torch.equal(h, hi.float()) and torch.equal(l, lo.float())


def pool_properties(a32, N, H, W, what):
    """what the per-element comparison of a pooled case needs: members of a window exactly equal or more than 4 ulp apart;
    with every planted group placed (13 windows), tied maxima of 2, 3 and 4 members, in every position, and an all-zero window"""
    assert not bool(E.window_gap_violations(a32).any()), what
    if N * (H // 2) * (W // 2) >= 13:
        win = E.windows(a32[..., :1])  # channel 0: guaranteed by construction
        mx = win == win.max(-1, keepdim=True).values
        ties = mx.sum(-1)
        assert {2, 3, 4} <= set(ties.unique().tolist()), what
        assert all(bool((mx & (ties >= 2).unsqueeze(-1))[..., j].any()) for j in range(4)), what
        assert bool((E.windows(a32) == 0).all(-1).any()), what


def test_every_pool_bwd_case_of_the_gpu_test_has_unambiguous_windows():
    """the very draws of test_ew_bwd_kernels_gpu.py::test_pool_backward_kernel (E.pool_case), in fp32 storage; the 16-bit
    cases are these values rounded, where two members that round together are one more exact tie"""
    for (N, H0, W0, Cp) in E.fold_pool_geometries():
        H, W = E.pool_size(H0, W0)
        for i in range(4):
            a, _ = E.pool_case(N, H, W, Cp, i, "fp32")
            pool_properties(a[..., :Cp - 3], N, H, W, (N, H, W, Cp, i))


@pytest.mark.parametrize("masked", [True, False])
def test_every_bn_case_of_the_gpu_test_has_the_input_properties(masked):
    """the very draws of test_bn_relu_backward_kernels (E.bn_case over E.bn_geometries): magnitudes, zero padding channels,
    planted exact-zero gate arguments that close the gate, and for the pooled source unambiguous windows"""
    for kind in (E.GS_PLAIN, E.GS_FOLD, E.GS_POOL, E.GS_HEAD):
        for i, (N, H, W, C, Cp) in enumerate(E.bn_geometries(kind)):
            case = E.bn_case(kind, N, H, W, C, Cp, masked, seed=i, variant=i)
            z, v = case["z"], case["v"]
            for t in (z[..., :C], v["scale"][:C], v["shift"][:C]):
                assert bool(((t.abs() >= E.LO) & (t.abs() <= E.HI)).all())
            assert float(z[..., C:Cp].abs().max() if C < Cp else 0.0) == 0.0
            arg = z[..., :C].double() * v["scale"][:C].double() + v["shift"][:C].double()
            assert bool(((arg.float() > 0) == (arg > 0)).all())
            assert not bool(E.gate(z[..., :C], v["scale"][:C], v["shift"][:C])[arg == 0].any())
            if kind == E.GS_POOL:
                pool_properties(E.act32(z[..., :C], v["scale"][:C], v["shift"][:C], case["mask"]), N, H, W, (kind, N, H, W, C, Cp))
            else:
                assert bool((arg[..., 0] == 0).any()), "a planted exact-zero gate argument"
