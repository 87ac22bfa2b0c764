"""tests/ew_fwd_reference.py against the torch modules the model composes, in fp64 (rtol 1e-12): nn.BatchNorm2d train / eval with
its running-statistics update, F.relu, F.max_pool2d, F.interpolate(align_corners=True) + F.pad + cat, a 1x1 F.conv2d and the
host loss classes.  The fp32 restatement of lerp_src is tied to fp32 F.interpolate on one-hot inputs at every size the cases
use.  On the very draws of tests/test_ew_fwd_kernels_gpu.py: no pre-activation within the per-element bound of 0, no window
maximum decided by less than it, nothing excluded.  And the bounds are tight: perturbed references are rejected by the very
comparison functions the GPU tests call."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

from mimo_unet_amd.losses import GaussianNLL, LaplaceNLL
from tests import ew_bwd_reference as E
from tests import ew_fwd_reference as F
from tests import scalar_reference as R
from tests.test_ew_bwd_kernels_gpu import abs_floor, check_elem, check_sum
from tests.test_ew_bwd_reference_cpu import close, nchw, nhwc


@pytest.mark.parametrize("count_one", [False, True])
def test_bn_stats_against_batchnorm2d_train_and_eval(count_one):
    g = F.gen(1)
    C = 6
    x = torch.randn(1 if count_one else 3, C, 1 if count_one else 5, 1 if count_one else 4, generator=g, dtype=torch.float64)
    bn = nn.BatchNorm2d(C, eps=1e-5, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g).double())
        bn.bias.copy_(torch.randn(C, generator=g).double())
        bn.running_mean.copy_(torch.randn(C, generator=g).double())
        bn.running_var.copy_(torch.rand(C, generator=g).double() + 0.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    rows = x.permute(0, 2, 3, 1).reshape(-1, C)              # one pixel per partial row: [rows][2][C]
    partial = torch.stack([rows, rows * rows], 1)
    count = rows.shape[0]
    r = F.bn_stats(partial, C, count, bn.weight.detach(), bn.bias.detach(), rm, rv, 0.1, 1e-5)
    if not count_one:  # (torch refuses to train on one value per channel; the count == 1 branch is checked by hand below)
        y = bn.train()(x)
        close(nhwc(x) * r["scale"] + r["shift"], nhwc(y.detach()), "train output")
        close(r["running_mean"], bn.running_mean, "running_mean")
        close(r["running_var"], bn.running_var, "running_var (unbiased)")
        close(r["invstd"], (x.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt(), "invstd")
    else:
        assert float(r["var"].abs().max()) == 0.0
        close(r["running_var"], 0.9 * rv, "count == 1: the biased (zero) variance")
        close(r["running_mean"], 0.9 * rm + 0.1 * x.reshape(C), "running_mean")
    e = F.bn_eval(bn.weight.detach(), bn.bias.detach(), rm, rv, 1e-5)
    bn2 = nn.BatchNorm2d(C).double().eval()
    bn2.load_state_dict({**bn.state_dict(), "running_mean": rm, "running_var": rv})
    close(nhwc(x) * e["scale"] + e["shift"], nhwc(bn2(x).detach()), "eval output")


@pytest.mark.parametrize("geom", F.POOL_GEOMETRIES[:5] + F.POOL_GEOMETRIES[6:], ids=str)
def test_activation_and_maxpool_against_relu_and_max_pool2d(geom):
    N, H, W, C, Cp = geom
    C = min(C, 8)
    g = F.gen(2)
    z = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    sc, sh = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    mask = E.dropout_mask(N, C, g, True).double()
    a = E.activation(z, sc, sh, mask)
    close(a, TF.relu(z * sc + sh) * mask[:, None, None, :], "relu(bn) * mask")
    close(F.maxpool(a), nhwc(TF.max_pool2d(nchw(a), 2)), "max_pool2d")


@pytest.mark.parametrize("geom", F.up_geometries(), ids=str)
def test_upsample_cat_against_interpolate_pad_cat(geom):
    N, hs, ws, hl, wl, C, Cp = geom
    C = min(C, 4)
    g = F.gen(3)
    low = torch.randn(N, hl, wl, C, generator=g, dtype=torch.float64)
    skip = torch.randn(N, hs, ws, 3, generator=g, dtype=torch.float64)
    up = TF.interpolate(nchw(low), scale_factor=2, mode="bilinear", align_corners=True)
    dy, dx = hs - up.shape[2], ws - up.shape[3]
    want = torch.cat([nchw(skip), TF.pad(up, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])], 1)
    got = F.upsample_cat(skip, low, hs, ws)
    # the reference interpolates with lerp_src's fp32 weights: 2^-23 of a source index below 2^7 away from the exact ones
    err = float((got - nhwc(want)).abs().max()) / float(want.abs().max())
    assert err <= 2.0 ** -23 * max(hl, wl), err


def test_lerp_src_restatement_reproduces_fp32_interpolate_at_every_size_used():
    sizes = sorted({n for geom in F.up_geometries() for n in geom[3:5]})
    for n in sizes:
        M = F.lerp_matrix32(n, torch.float32)
        eye = torch.eye(n, dtype=torch.float32)  # one-hot rows: column i of the result is the weight every output gives input i
        along_h = TF.interpolate(eye.t().reshape(1, n, n, 1).expand(1, n, n, 2), size=(2 * n, 2), mode="bilinear", align_corners=True)
        assert torch.equal(along_h[0, :, :, 0].t(), M), ("rows", n)
        along_w = TF.interpolate(eye.t().reshape(1, n, 1, n).expand(1, n, 2, n), size=(2, 2 * n), mode="bilinear", align_corners=True)
        assert torch.equal(along_w[0, :, 0, :].t(), M), ("columns", n)


@pytest.mark.parametrize("fused", [False, True])
def test_head_against_conv1x1(fused):
    g = F.gen(4)
    N, HW, C, Co = 3, 20, 13, 4
    a = torch.randn(N, HW, C, generator=g, dtype=torch.float64)
    w, b = torch.randn(Co, C, generator=g, dtype=torch.float64), torch.randn(Co, generator=g, dtype=torch.float64)
    sc, sh = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    x = TF.relu(a * sc + sh) if fused else a
    want = TF.conv2d(x.permute(0, 2, 1).reshape(N, C, HW, 1), w.reshape(Co, C, 1, 1), b).reshape(N, Co, HW)
    close(F.head(a, w, b, *((sc, sh) if fused else ())), want, "head")


@pytest.mark.parametrize("kind", [F.LAPLACE, F.GAUSSIAN])
@pytest.mark.parametrize("use_mask,use_perm", [(False, False), (True, False), (False, True), (True, True)])
def test_loss_against_the_host_loss_classes(kind, use_mask, use_perm):
    out, label, mask, perm = F.loss_case(0, 3, 85, 4, 3, use_mask, use_perm)
    o, l = out.double(), label.double()
    fn = (LaplaceNLL if kind == F.LAPLACE else GaussianNLL)(F.EPS_MIN, F.EPS_MAX).double()
    got = F.loss(o, l, None if mask is None else mask.double(), perm, kind, F.EPS_MIN, F.EPS_MAX)
    for s in range(3):
        src = perm[s] if perm is not None else torch.arange(3)
        want = fn(o[:, s, :2], o[:, s, 2:], l[src], mask=None if mask is None else mask.double()[src][:, None, :])
        close(got[s], want, ("loss", s))


def test_pack_and_unpack_against_plain_indexing():
    g = F.gen(5)
    x = torch.randn(4, 3, 3, 5, 6, generator=g, dtype=torch.float64)
    perm = torch.stack([torch.randperm(4, generator=g) for _ in range(3)])
    out = F.pack_input(x, perm, 1, 8)
    for n in range(4):
        assert torch.equal(out[n, :, :, :3], x[perm[1][n], 1].permute(1, 2, 0)) and float(out[n, :, :, 3:].abs().sum()) == 0
    d = E.padded_grad(2, 5, 6, 8, g).double()
    xin = torch.randn(2, 3, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    (TF.pad(xin, (1, 1, 1, 1), mode="reflect") * nchw(d[..., :3])).sum().backward()
    close(F.unpack_dx(d, 3), xin.grad, "unpack_dx")


# ---- the draws of the GPU tests are unambiguous ---------------------------------------------------------------------------------

def assert_unambiguous(c, pooled, what):
    """no pre-activation within the per-element bound (4 x a yardstick of a few ulp: 16 ulp of |z scale| + |shift| is generous)
    of 0; no two members of a window closer than 4 ulp unless exactly equal"""
    C = c["C"]
    z, sc, sh = c["z"][..., :C], c["scale"][:C], c["shift"][:C]
    pre = F.pre_activation(z, sc, sh)
    mag = (z.double() * sc.double()).abs() + sh.double().abs()
    assert bool((pre.abs() > 16 * 2.0 ** -23 * mag).all()), what
    assert bool(((pre.float() > 0) == (pre > 0)).all()), what
    if pooled and c["H"] >= 2 and c["W"] >= 2:
        assert not bool(E.window_gap_violations(E.act32(z, sc, sh, c["mask"])).any()), what


@pytest.mark.parametrize("prec", ["fp32", "bf16-mixed", "16-mixed"])
def test_every_gate_and_window_of_the_gpu_draws_is_unambiguous(prec):
    for i, geom in enumerate(F.PIXEL_GEOMETRIES):
        for masked in (False, True):
            assert_unambiguous(F.bn_relu_case(i, geom, prec, masked, pooled=False), False, (geom, masked))
    for i, geom in enumerate(F.POOL_GEOMETRIES):
        assert_unambiguous(F.bn_relu_case(100 + i, geom, prec, bool(i & 1)), True, geom)
    for i, geom in enumerate(F.up_geometries()):
        c = F.up_case(i, geom, prec, True)
        assert_unambiguous(dict(C=geom[5], z=c["low"], scale=c["scale"], shift=c["shift"], mask=None, H=1, W=1), False, geom)
    for i, (C, Co, S, N, HW) in enumerate(F.head_cases()):
        c = F.head_case(i, C, Co, N, HW, prec, True)
        assert_unambiguous(dict(C=C, z=c["a"], scale=c["scale"], shift=c["shift"], mask=None, H=1, W=1), False, (C, Co))


# ---- the bounds reject wrong kernels ------------------------------------------------------------------------------------------------

def rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def test_statistics_bound_rejects_a_biased_variance_and_a_dropped_row():
    g = F.gen(10)
    C, rows = 5, 65
    gamma, beta, rm, rv = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g), torch.zeros(C), torch.ones(C)
    for kind, count in (("random", rows * 64), ("integer", rows)):
        part = F.partial_rows(rows, C, 16, g, kind)
        ref = F.bn_stats(part, C, count, gamma, beta, rm, rv, 0.1, 1e-5)
        allowed = F.one_ulp(ref) if kind == "integer" else F.bn_stats_bound(ref, rows, count, 1e-5, gamma, beta, 0.1)
        as_kernel = lambda r: {k: r[k].float() for k in F.BN_OUTPUTS}
        F.check_stats("itself", as_kernel(ref), ref, allowed)
        rejected(lambda: F.check_stats("biased", as_kernel(F.bn_stats(part, C, count, gamma, beta, rm, rv, 0.1, 1e-5, biased=True)), ref, allowed))
        rejected(lambda: F.check_stats("dropped", as_kernel(F.bn_stats(part, C, count, gamma, beta, rm, rv, 0.1, 1e-5, drop_row=rows - 1)), ref, allowed))


def test_per_element_bound_rejects_wrong_interpolation_and_tolerates_reassociation():
    geom = (2, 7, 11, 3, 4, 13, 16)
    c = F.up_case(1, geom, "fp32", False)
    low = c["low"][..., :16]
    fn = lambda l, **kw: {"up": F.upsample_cat(None, l, 7, 11, **kw)}
    fl = abs_floor(fn, [low], "up")
    y, ref, _ = R.yardstick(fn, [low], {"up": fl})
    check = lambda got: check_elem("cpu", "perturbed", got, ref["up"], y["up"], "fp32", fl)
    check(fn(low)["up"])
    # vertical blend first, in fp32: an ulp-level change of association — what the bound is there to tolerate
    check(fn(low, vertical_first=True)["up"])
    rejected(lambda: check(fn(low, clamp_i1=False)["up"]))      # i1 not clamped at the last source row
    shifted = fn(low)["up"].clone()
    shifted[:, :, 8] = shifted[:, :, 7]   # (columns 1..8 hold the up-sampled tensor: asymmetric zero pad of 1 and 2)
    rejected(lambda: check(shifted))


def test_per_element_bound_rejects_a_misplaced_odd_column_a_live_pad_weight_and_a_misapplied_perm():
    c = F.bn_relu_case(107, (2, 6, 7, 13, 16), "fp32", False)
    C = c["C"]
    fn = lambda z, sc, sh: {"a": E.activation(z, sc, sh)}
    inputs = [c["z"][..., :C], c["scale"][:C], c["shift"][:C]]
    fl = abs_floor(fn, inputs, "a")
    y, ref, _ = R.yardstick(fn, inputs, {"a": fl})
    good = fn(*inputs)["a"]
    check_elem("cpu", "itself", good, ref["a"], y["a"], "fp32", fl)
    wrong = good.clone()
    wrong[:, :, -1] = wrong[:, :, -2]    # the last odd column taken from its left neighbour
    rejected(lambda: check_elem("cpu", "odd column", wrong, ref["a"], y["a"], "fp32", fl))
    unwritten = good.clone()
    unwritten[:, -1, -1] = float("nan")  # a pixel of no window left unwritten in a NaN-filled buffer
    rejected(lambda: check_elem("cpu", "unwritten", unwritten, ref["a"], y["a"], "fp32", fl))
    # head: one weight of a padding channel left non-zero (the junk there is ~3.5)
    h = F.head_case(0, 5, 2, 2, 7, "fp32", False)
    hfn = lambda a, w, b: {"out": F.head(a, w, b)}
    hin = [h["a"][..., :5], h["w"], h["bias"]]
    hfl = abs_floor(hfn, hin, "out")
    hy, href, _ = R.yardstick(hfn, hin, {"out": hfl})
    check_elem("cpu", "head itself", hfn(*hin)["out"], href["out"], hy["out"], "fp32", hfl)
    live = hfn(*hin)["out"] + 2.0 ** -12 * h["a"][..., 5][:, None, :]
    rejected(lambda: check_elem("cpu", "live pad weight", live, href["out"], hy["out"], "fp32", hfl))
    # loss: the permutation applied to the output instead of the label
    out, label, mask, perm = F.loss_case(3, 7, 37, 2, 3, True, True)
    assert any(not torch.equal(perm[s][perm[s]], torch.arange(7)) for s in range(3)), "a permutation that is not its own inverse"
    o, l, m = out.double(), label.double(), mask.double()
    ref = F.loss(o, l, m, perm, F.LAPLACE, F.EPS_MIN, F.EPS_MAX)
    absterm = F.loss_absterm(o, l, m, perm, F.LAPLACE, F.EPS_MIN, F.EPS_MAX).mean(1)
    check_sum("cpu", "itself", ref.float(), ref, absterm, F.loss_k(259))
    rejected(lambda: check_sum("cpu", "perm", F.loss(o, l, m, perm, F.LAPLACE, F.EPS_MIN, F.EPS_MAX, perm_on_output=True).float(), ref,
                               absterm, F.loss_k(259)))
