"""The forward element-wise kernels (csrc/ew_bn_fwd.hip, ew_resample.hip, ew_dropout.hip, ew_head_loss.hip), one operator at a time through mimo_op_bn_stats / _bn_relu_forward /
_maxpool2x2_ex / _upsample_cat_ex / _head_forward / _loss_forward / _pack_input / _unpack_dx / _fold_image_grad, against the
fp64 references of tests/ew_fwd_reference.py (proven against the torch modules by tests/test_ew_fwd_reference_cpu.py).

Bounds.  Per-element outputs: check_elem of the backward tests (error <= 4 x the fp32 CPU yardstick, never below 4 fp32 ulp; floor
= the sum of the magnitudes of an element's terms; 16-bit storage: the reference on rounded inputs, rounded to storage, plus one
storage ulp).  Copies, maxima, padding and the fused-versus-unfused identities: bitwise.  Statistics: one ulp on integer
partials, F.bn_stats_bound (derived there) on random ones.  Losses: check_sum with F.loss_k.  Every output buffer starts
NaN-filled; no element is excluded; padding channels of the inputs hold finite non-zero junk unless the contract says zero."""
import ctypes as ct

import pytest
import torch

from tests import ew_bwd_reference as E
from tests import ew_fwd_reference as F
from tests import scalar_reference as R
from tests.helpers import report
from tests.test_ew_bwd_kernels_gpu import MIMO_ERR_INVALID, PRECISIONS, _L, abs_floor, bits, check_elem, check_sum, dev, nans, p

pytestmark = pytest.mark.gpu
NAN = float("nan")
PRECS = list(PRECISIONS)


def run(name, *args):
    L = _L()
    L.check(getattr(L.load(), name)(*args, L.current_stream()), name)


def status_word():
    return ct.c_int32(-1)


# ---- BatchNorm statistics ---------------------------------------------------------------------------------------------------

def bn_stats_call(partial, rows, cout_pad, C, Cp, count, gamma, beta, rm, rv, momentum, eps, route, training=1, expect=0, override=None):
    """override: fields of the argument struct replaced after it is filled (the rejection test: a NULL tensor)"""
    L = _L()
    out = {k: nans(Cp) for k in ("mean", "invstd", "scale", "shift")}
    out["running_mean"], out["running_var"] = rm.clone().cuda(), rv.clone().cuda()
    st = status_word()
    keep = [dev(partial), dev(gamma), dev(beta)]
    a = L.BnStatsArgs(partial=p(keep[0]), rows=rows, cout_pad=cout_pad, c=C, c_p=Cp, training=training, route=route, count=count,
                      gamma=p(keep[1]), beta=p(keep[2]), running_mean=p(out["running_mean"]), running_var=p(out["running_var"]),
                      momentum=momentum, eps=eps, mean=p(out["mean"]), invstd=p(out["invstd"]), scale=p(out["scale"]),
                      shift=p(out["shift"]), status=ct.pointer(st))
    for k, v in (override or {}).items():
        setattr(a, k, v)
    rc = L.load().mimo_op_bn_stats(ct.byref(a), L.current_stream())
    assert rc == expect, (rc, L.load().mimo_last_error())
    torch.cuda.synchronize()
    if rc == 0:
        for k in ("mean", "invstd", "scale", "shift"):
            assert float(out[k][C:].abs().sum()) == 0.0, (k, "padding channels must be zeros")
    return {k: v[:C].cpu() for k, v in out.items()}, st.value, out


def bn_params(C, g):
    return (0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g))


MOM, EPS = F.f32(0.1), F.f32(1e-5)


def routes_for(rows):
    return [r for r in (F.ROUTE_ONE, F.ROUTE_ROWSUM, F.ROUTE_PLAN) if not (r == F.ROUTE_ONE and rows > F.K_COLSUM_MAX_ROWS)]


@pytest.mark.parametrize("kind", ["integer", "random"])
def test_bn_stats_kernels(kind):
    worst = 0.0
    for i, rows in enumerate(F.BN_ROWS_ONE + F.BN_ROWS_TWO):
        C, Cp, cout_pad = F.BN_CHANNELS[i % len(F.BN_CHANNELS)] if rows not in (65, 4097) else F.BN_CHANNELS[1]
        g = F.gen(3000 + i)
        partial = F.partial_rows(rows, C, cout_pad, g, kind)
        count = rows if kind == "integer" else rows * 64
        gamma, beta, rm, rv = bn_params(C, g)
        ref = F.bn_stats(partial, C, count, gamma, beta, rm, rv, MOM, EPS)
        allowed = F.one_ulp(ref) if kind == "integer" else F.bn_stats_bound(ref, rows, count, EPS, gamma, beta, MOM)
        results = {}
        for route in routes_for(rows):
            got, status, _ = bn_stats_call(partial, rows, cout_pad, C, Cp, count, gamma, beta, rm, rv, MOM, EPS, route)
            assert status == 0, "all-finite partials leave the status word 0"
            worst = max(worst, F.check_stats(f"{kind} rows {rows} route {route}", got, ref, allowed))
            results[route] = got
            if kind == "random" and C > 2:  # the constant channel: variance clamps to exactly 0
                want = (1.0 / torch.tensor(EPS, dtype=torch.float64).sqrt()).float()
                assert torch.equal(got["invstd"][2], want), (rows, route, float(got["invstd"][2]))
        if F.ROUTE_ONE in results:  # the two routes against each other: to the bound (both sit within it of the reference)
            for k in F.BN_OUTPUTS:
                d = (results[F.ROUTE_ONE][k].double() - results[F.ROUTE_ROWSUM][k].double()).abs()
                assert bool((d <= 2 * allowed[k]).all()), (rows, k)
            assert all(torch.equal(results[F.ROUTE_PLAN][k], results[F.ROUTE_ONE][k]) for k in F.BN_OUTPUTS), "the plan's rule: one launch"
        else:
            assert all(torch.equal(results[F.ROUTE_PLAN][k], results[F.ROUTE_ROWSUM][k]) for k in F.BN_OUTPUTS), "the plan's rule: row sum"
    report(f"[bn_stats] {kind} WORST err / bound {worst:.3f}")


def test_bn_stats_count_one_inf_channel_and_eval():
    g = F.gen(3100)
    C, Cp, cout_pad = 5, 8, 16
    gamma, beta, rm, rv = bn_params(C, g)
    # count == 1: the running variance takes the biased (zero) variance
    one = F.partial_rows(1, C, cout_pad, g, "integer")
    one[:, 1, :C] = one[:, 0, :C] ** 2
    ref = F.bn_stats(one, C, 1, gamma, beta, rm, rv, MOM, EPS)
    for route in (F.ROUTE_ONE, F.ROUTE_ROWSUM):
        got, status, _ = bn_stats_call(one, 1, cout_pad, C, Cp, 1, gamma, beta, rm, rv, MOM, EPS, route)
        F.check_stats(f"count 1 route {route}", got, ref, F.one_ulp(ref))
        assert status == 0
    # one inf in one channel's partials: the status bit, the other channels untouched
    part = F.partial_rows(17, C, cout_pad, g)
    clean, status, _ = bn_stats_call(part, 17, cout_pad, C, Cp, 17 * 64, gamma, beta, rm, rv, MOM, EPS, F.ROUTE_ONE)
    assert status == 0
    part[5, 0, 3] = float("inf")
    got, status, _ = bn_stats_call(part, 17, cout_pad, C, Cp, 17 * 64, gamma, beta, rm, rv, MOM, EPS, F.ROUTE_ONE)
    assert status == F.STATUS_FWD_STATS
    keep = [c for c in range(C) if c != 3]
    assert all(torch.equal(bits(got[k][keep]), bits(clean[k][keep])) for k in F.BN_OUTPUTS)
    # eval mode: from the running statistics, which stay as they are
    got, status, _ = bn_stats_call(part, 0, cout_pad, C, Cp, 0, gamma, beta, rm, rv, MOM, EPS, F.ROUTE_PLAN, training=0)
    ref = F.bn_eval(gamma, beta, rm, rv, EPS)
    F.check_stats("eval", {k: got[k] for k in ref}, ref, F.one_ulp(ref))
    assert status == 0 and torch.equal(got["running_mean"], rm) and torch.equal(got["running_var"], rv)
    rv2 = rv.clone()
    rv2[1] = float("nan")
    _, status, _ = bn_stats_call(part, 0, cout_pad, C, Cp, 0, gamma, beta, rm, rv2, MOM, EPS, F.ROUTE_PLAN, training=0)
    assert status == F.STATUS_FWD_STATS


# ---- BatchNorm + ReLU (+ pooling), max pooling -------------------------------------------------------------------------------

def bn_relu_call(c, prec, pooled, z=None, z_fp32=0, expect=0, override=None):
    L = _L()
    N, H, W, C, Cp = c["N"], c["H"], c["W"], c["C"], c["Cp"]
    a = nans(N, H, W, c["lda"])
    pool = nans(N, H // 2, W // 2, c["ldpool"]) if pooled else None
    st = status_word()
    keep = [dev(c["z"] if z is None else z), dev(c["scale"]), dev(c["shift"]), dev(c["mask"])]
    args = L.BnReluForwardArgs(z=p(keep[0]), ldz=c["ldz"], scale=p(keep[1]), shift=p(keep[2]), mask=p(keep[3]), n=N, h=H, w=W, c=C, c_p=Cp,
                               precision=PRECISIONS[prec], z_fp32=z_fp32, a=p(a), lda=c["lda"], pool=p(pool), ldpool=c["ldpool"],
                               status=ct.pointer(st))
    for k, v in (override or {}).items():
        setattr(args, k, v)
    rc = L.load().mimo_op_bn_relu_forward(ct.byref(args), L.current_stream())
    assert rc == expect, (rc, L.load().mimo_last_error())
    torch.cuda.synchronize()
    return a, pool, st.value


def bn_relu_reference(c, z):
    C = c["C"]
    mask = c["mask"]
    fn = lambda zz, sc, sh: {"a": E.activation(zz, sc, sh, None if mask is None else mask.to(zz.dtype))}
    inputs = [z[..., :C], c["scale"][:C], c["shift"][:C]]
    fl = abs_floor(fn, inputs, "a")   # |z scale| + |shift| (x the multiplier): the gate of magnitudes is open
    y, ref, _ = R.yardstick(fn, inputs, {"a": fl})
    return ref["a"], y["a"], fl


def maxpool_call(x, lda, N, H, W, Cp, prec, ldo):
    y = nans(N, H // 2, W // 2, ldo)
    xd = dev(x)
    run("mimo_op_maxpool2x2_ex", p(xd), lda, p(y), ldo, N, H, W, Cp, PRECISIONS[prec])
    return y


@pytest.mark.parametrize("prec", PRECS)
def test_bn_relu_forward_kernel(prec):
    worst = 0.0
    for i, geom in enumerate(F.PIXEL_GEOMETRIES):
        for masked in (False, True):
            c = F.bn_relu_case(i, geom, prec, masked, pooled=False)
            variants = [(0, c["z"])] + ([(1, F.bn_relu_case(i, geom, "fp32", masked, pooled=False)["z"])] if prec != "fp32" else [])
            for z_fp32, z in variants:  # (z_fp32: the <float, 16-bit> kernel pair on an unrounded z)
                a, _, status = bn_relu_call(c, prec, False, z, z_fp32)
                C, Cp = c["C"], c["Cp"]
                assert status == 0 and bool(torch.isnan(a[..., Cp:]).all()), "channels beyond c_p were written"
                assert float(a[..., C:Cp].abs().sum()) == 0.0, "padding channels must be zeros"
                ref, y, fl = bn_relu_reference(c, z)
                worst = max(worst, check_elem("bn_relu_fwd", f"{prec} {geom} mask {masked} z_fp32 {z_fp32}", a[..., :C].cpu(), ref, y, prec, fl))
    report(f"[bn_relu_fwd] {prec} WORST err / bound {worst:.3f}")


@pytest.mark.parametrize("prec", PRECS)
def test_bn_relu_pool_kernel_and_its_unfused_chain(prec):
    worst = 0.0
    for i, geom in enumerate(F.POOL_GEOMETRIES):
        masked = bool(i & 1)
        c = F.bn_relu_case(100 + i, geom, prec, masked)
        N, H, W, C, Cp = geom
        a, pool, status = bn_relu_call(c, prec, True)
        assert status == 0 and bool(torch.isnan(a[..., Cp:]).all()) and bool(torch.isnan(pool[..., Cp:]).all())
        assert float(a[..., C:Cp].abs().sum()) == 0.0 and float(pool[..., C:Cp].abs().sum()) == 0.0
        ref, y, fl = bn_relu_reference(c, c["z"])
        worst = max(worst, check_elem("bn_relu_pool_fwd", f"{prec} {geom} mask {masked}", a[..., :C].cpu(), ref, y, prec, fl))
        # the pooled tensor: exactly the maximum of the four activations written
        assert torch.equal(bits(pool[..., :Cp]), bits(F.maxpool(a[..., :Cp].cpu()))), geom
        # Bit-identity with the unfused chain, in every storage type: both round the same fp32 activation to storage, and the
        # maximum of rounded values is the rounded maximum.
        a2, _, _ = bn_relu_call(c, prec, False)
        pool2 = maxpool_call(a2, c["lda"], N, H, W, Cp, prec, c["ldpool"])
        assert torch.equal(bits(a[..., :Cp]), bits(a2[..., :Cp])) and torch.equal(bits(pool[..., :Cp]), bits(pool2[..., :Cp])), geom
    report(f"[bn_relu_pool_fwd] {prec} WORST err / bound {worst:.3f}")


@pytest.mark.parametrize("prec", PRECS)
def test_maxpool_kernel_in_every_storage_type_at_a_pitch(prec):
    for i, geom in enumerate(F.POOL_GEOMETRIES):
        N, H, W, C, Cp = geom
        x = F.pool_input(i, geom, prec)
        y = maxpool_call(x, Cp + 4, N, H, W, Cp, prec, Cp + 12)
        assert bool(torch.isnan(y[..., Cp:]).all())
        assert torch.equal(bits(y[..., :Cp]), bits(F.maxpool(x[..., :Cp]))), geom


# ---- up-sampling + concat ---------------------------------------------------------------------------------------------------------

def upcat_call(c, prec, with_skip, fused, low=None):
    N, hs, ws, hl, wl, Cp, csp = c["N"], c["hs"], c["ws"], c["hl"], c["wl"], c["Cp"], c["csp"]
    out = nans(N, hs, ws, csp + Cp)
    keep = [dev(c["skip"]) if with_skip else None, dev(c["low"]) if low is None else low, dev(c["scale"]), dev(c["shift"])]
    run("mimo_op_upsample_cat_ex", p(keep[0]), c["lds"], p(keep[1]), c["ldl"], p(keep[2]) if fused else None, p(keep[3]) if fused else None,
        p(out), N, hs, ws, csp, hl, wl, Cp, PRECISIONS[prec])
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_upsample_cat_kernels(prec):
    worst = 0.0
    for i, geom in enumerate(F.up_geometries()):
        for fused in (False, True):
            c = F.up_case(i, geom, prec, fused)
            N, hs, ws, hl, wl, C, Cp = geom
            csp = c["csp"]
            sc, sh = (c["scale"], c["shift"]) if fused else (None, None)
            fn = lambda low, *v: {"up": F.upsample_cat(None, low, hs, ws, *v)}
            inputs = [c["low"][..., :Cp]] + ([sc, sh] if fused else [])
            fl = abs_floor(fn, inputs, "up")
            y, ref, _ = R.yardstick(fn, inputs, {"up": fl})
            out = upcat_call(c, prec, True, fused)             # the per-pixel kernel
            assert torch.equal(bits(out[..., :csp]), bits(c["skip"][..., :csp])), "skip channels are copies"
            worst = max(worst, check_elem("upcat_fwd", f"{prec} {geom} fused {fused}", out[..., csp:].cpu(), ref["up"], y["up"], prec, fl))
            border = torch.ones_like(ref["up"], dtype=torch.bool)
            pt, pl = (hs - 2 * hl) // 2, (ws - 2 * wl) // 2
            border[:, pt:pt + 2 * hl, pl:pl + 2 * wl] = False
            assert float(out[..., csp:].cpu()[border].abs().sum()) == 0.0, "the zero padding"
            out2 = upcat_call(c, prec, False, fused)           # skip in place: the 2x2-block kernel when hs == 2 hl, ws == 2 wl
            assert bool(torch.isnan(out2[..., :csp]).all()), "skip == NULL writes only the up-sampled channels"
            assert torch.equal(bits(out2[..., csp:]), bits(out[..., csp:])), ("per-pixel and 2x2-block kernels", geom, fused)
            if fused and prec == "fp32":
                # Bit-identity of the fused BatchNorm + ReLU with the unfused chain.  fp32 storage only: in a 16-bit mode the
                # unfused chain rounds the activation to storage before interpolating and the fused kernel does not.
                bc = dict(N=N, H=hl, W=wl, C=C, Cp=Cp, scale=c["scale"], shift=c["shift"], mask=None, z=c["low"], ldz=c["ldl"], lda=c["ldl"], ldpool=Cp)
                act, _, _ = bn_relu_call(bc, prec, False)
                for with_skip in (True, False):
                    chain = upcat_call(c, prec, with_skip, False, low=act)
                    assert torch.equal(bits(chain[..., csp:]), bits(out[..., csp:])), ("fused lo_scale against its chain", geom, with_skip)
    report(f"[upcat_fwd] {prec} WORST err / bound {worst:.3f}")


# ---- head and loss ---------------------------------------------------------------------------------------------------------------

def head_call(c, C, Co, N, S, s, HW, prec, fused, a=None, lda=None, expect=0, override=None):
    L = _L()
    out = nans(N, S, Co, HW)
    st = status_word()
    keep = [dev(c["a"]) if a is None else a, dev(c["w"]), dev(c["bias"]), dev(c["scale"]), dev(c["shift"])]
    args = L.HeadForwardArgs(a=p(keep[0]), lda=c["lda"] if lda is None else lda, w=p(keep[1]), bias=p(keep[2]), c=C, co=Co, n=N, subnetworks=S, s=s,
                             hw=HW, in_scale=p(keep[3]) if fused else None, in_shift=p(keep[4]) if fused else None,
                             precision=PRECISIONS[prec], out=p(out), status=ct.pointer(st))
    for k, v in (override or {}).items():
        setattr(args, k, v)
    rc = L.load().mimo_op_head_forward(ct.byref(args), L.current_stream())
    assert rc == expect, (rc, L.load().mimo_last_error())
    torch.cuda.synchronize()
    return out, st.value


@pytest.mark.parametrize("prec", PRECS)
def test_head_forward_kernel(prec):
    worst = 0.0
    for i, (C, Co, S, N, HW) in enumerate(F.head_cases()):
        s = S - 1
        for fused in (False, True):
            c = F.head_case(i, C, Co, N, HW, prec, fused)
            v = [c["scale"][:C], c["shift"][:C]] if fused else []
            fn = lambda a, w, b, *sv: {"out": F.head(a, w, b, *sv)}
            inputs = [c["a"][..., :C], c["w"], c["bias"]] + v
            fl = abs_floor(fn, inputs, "out")     # sum |a w| + |bias|
            y, ref, _ = R.yardstick(fn, inputs, {"out": fl})
            out, status = head_call(c, C, Co, N, S, s, HW, prec, fused)
            assert status == 0
            others = [k for k in range(S) if k != s]
            assert bool(torch.isnan(out[:, others]).all()), "another subnetwork's logits were written"
            # (logits are fp32 in every mode: the 16-bit modes round the input only, which the reference sees rounded)
            worst = max(worst, check_elem("head_fwd", f"{prec} C {C} Co {Co} S {S} N {N} HW {HW} fused {fused}", out[:, s].cpu(), ref["out"],
                                          y["out"], "fp32", fl))
            if fused and prec == "fp32":
                # in_scale / in_shift against the unfused chain, bit for bit.  fp32 storage only: a 16-bit chain rounds the activation.
                bc = dict(N=N, H=1, W=HW, C=C, Cp=c["Cp"], scale=c["scale"], shift=c["shift"], mask=None, z=c["a"], ldz=c["lda"], lda=c["lda"], ldpool=c["Cp"])
                act, _, _ = bn_relu_call(bc, prec, False)
                chain, _ = head_call(c, C, Co, N, S, s, HW, prec, False, a=act)
                assert torch.equal(bits(chain[:, s]), bits(out[:, s])), ("fused in_scale against its chain", C, Co)
    report(f"[head_fwd] {prec} WORST err / bound {worst:.3f}")


def test_head_forward_reports_a_non_finite_logit():
    c = F.head_case(0, 5, 2, 2, 7, "fp32", False)
    c["a"][1, 3, 0], c["w"][1, 0] = 3e38, 2.0
    out, status = head_call(c, 5, 2, 2, 1, 0, 7, "fp32", False)
    assert status == F.STATUS_LOGITS
    assert int((~torch.isfinite(out)).sum()) == 1 and bool(torch.isinf(out[1, 0, 1, 3]))


def loss_call(out, label, mask, perm, kind, eps_min, eps_max, expect=0):
    L = _L()
    N, S, Co, HW = out.shape
    loss = nans(S)
    keep = [dev(out), dev(label), dev(mask), dev(perm)]
    rc = L.load().mimo_op_loss_forward(p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), N, S, Co, HW, kind, eps_min, eps_max, p(loss),
                                       L.current_stream())
    assert rc == expect, (rc, L.load().mimo_last_error())
    torch.cuda.synchronize()
    return loss.cpu()


@pytest.mark.parametrize("kind", [F.LAPLACE, F.GAUSSIAN])
def test_loss_forward_kernels(kind):
    worst, i = 0.0, 0
    emin, emax = F.f32(F.EPS_MIN), F.f32(F.EPS_MAX)
    for (N, HW) in F.LOSS_SIZES:
        for use_mask in (False, True):
            for use_perm in (False, True):
                Co = 4 if (N, HW) == (3, 85) and use_mask else 2
                out, label, mask, perm = F.loss_case(i, N, HW, Co, 3, use_mask, use_perm)
                i += 1
                got = loss_call(out, label, mask, perm, kind, emin, emax)
                o64, l64, m64 = out.double(), label.double(), None if mask is None else mask.double()
                ref = F.loss(o64, l64, m64, perm, kind, emin, emax)
                # |term| <= |log sc| + |d|^k / sc: the magnitude of what a thread adds
                absterm = F.loss_absterm(o64, l64, m64, perm, kind, emin, emax)
                count = absterm.shape[1]
                worst = max(worst, check_sum("loss_fwd", f"kind {kind} N {N} HW {HW} mask {use_mask} perm {use_perm}", got, ref,
                                             absterm.sum(1) / count, F.loss_k(count), absterm.amax(1) / count))
    report(f"[loss_fwd] kind {kind} WORST err / bound {worst:.3f}")


@pytest.mark.parametrize("kind", [F.LAPLACE, F.GAUSSIAN])
def test_loss_forward_is_exact_on_integer_terms(kind):
    """eps_min = eps_max = 1: the clamp pins sc to 1 whatever expf returns, logf(1) = 0, the term is |d| or d^2 — integers, for
    both kinds; every fp32 partial sum is an integer below 2^24, the fp64 finalize divides once."""
    for (N, HW) in F.LOSS_SIZES:
        out, label = F.exact_loss_case(N, HW, 3)
        perm = torch.stack([torch.randperm(N, generator=F.gen(s)) for s in range(3)])
        got = loss_call(out, label, None, perm, kind, 1.0, 1.0)
        ref = F.loss(out.double(), label.double(), None, perm, kind, 1.0, 1.0)
        assert torch.equal(got, ref.float()), (kind, N, HW, got, ref)


# ---- layout kernels -----------------------------------------------------------------------------------------------------------------

def test_pack_input_kernel():
    for i, C in enumerate(F.PACK_C):
        for (N, H, W) in ((3, 5, 4), (37, 3, 3), (1, 85, 85)):
            for use_perm in (False, True):
                g = F.gen(9000 + i)
                S, s, cp = 3, 1, 8
                big = torch.randn(N, 2, S, 2, C, H, W, generator=g)   # non-contiguous stride_n / stride_s: a slice of a larger tensor
                x = big[:, 1, :, 0]
                perm = torch.stack([torch.randperm(N, generator=g) for _ in range(S)]) if use_perm else None
                out = nans(N, H, W, cp)
                bd, pd = dev(big), dev(perm)
                first = big[0, 1, 0, 0].data_ptr() - big.data_ptr()
                run("mimo_op_pack_input", bd.data_ptr() + first, big.numel() - first // 4, big.stride(0), big.stride(2), p(pd), s, N, C, H, W,
                    p(out), cp)
                assert torch.equal(bits(out), bits(F.pack_input(x, perm, s, cp))), (C, N, H, W, use_perm)


@pytest.mark.parametrize("prec", PRECS)
def test_unpack_dx_kernel(prec):
    worst = 0.0
    for i, (H, W) in enumerate(F.FOLD_HW):
        for C in (2, 3, 4):
            g = F.gen(9100 + i)
            N, S, s, ldp = 3, 2, 1, 8
            dxpad = F.round_to(E.padded_grad(N, H, W, ldp, g), prec)
            fn = lambda d: {"dx": F.unpack_dx(d, C)}
            fl = abs_floor(fn, [dxpad], "dx")
            y, ref, _ = R.yardstick(fn, [dxpad], {"dx": fl})
            dx = nans(N, S, C, H, W)
            dd = dev(dxpad)
            run("mimo_op_unpack_dx", p(dd), ldp, N, S, s, C, H, W, PRECISIONS[prec], p(dx))
            assert bool(torch.isnan(dx[:, 0]).all())
            # (dx is fp32 in every mode: the 16-bit modes round dxpad only, which the reference sees rounded)
            worst = max(worst, check_elem("unpack_dx", f"{prec} {H}x{W} C {C}", dx[:, s].cpu(), ref["dx"], y["dx"], "fp32", fl))
            if H > 4 and W > 4:  # interior pixels are copies
                assert torch.equal(bits(dx[:, s, :, 2:H - 2, 2:W - 2]), bits(F.unpack_dx(dxpad, C)[:, :, 2:H - 2, 2:W - 2]))
    report(f"[unpack_dx] {prec} WORST err / bound {worst:.3f}")


def test_fold_image_grad_kernel():
    worst = 0.0
    for i, (H, W) in enumerate(F.FOLD_HW):
        for C in (2, 3, 4):
            for acc in (0, 1):
                g = F.gen(9200 + i)
                N, ldp = 3, 8
                dxpad = E.padded_grad(N, H, W, ldp, g)
                prev = torch.randn(N, C, H, W, generator=g)
                fn = lambda d, q: {"dimage": F.unpack_dx(d, C) + (q if acc else 0)}
                fl = abs_floor(fn, [dxpad, prev], "dimage")
                y, ref, _ = R.yardstick(fn, [dxpad, prev], {"dimage": fl})
                dimage = prev.clone().cuda() if acc else nans(N, C, H, W)
                dd = dev(dxpad)
                run("mimo_op_fold_image_grad", p(dd), ldp, N, C, H, W, p(dimage), acc)
                worst = max(worst, check_elem("fold_image_grad", f"{H}x{W} C {C} acc {acc}", dimage.cpu(), ref["dimage"], y["dimage"], "fp32", fl))
    report(f"[fold_image_grad] WORST err / bound {worst:.3f}")


# ---- rejections ---------------------------------------------------------------------------------------------------------------------

def test_invalid_arguments_are_rejected_with_nothing_written():
    L = _L()
    lib = L.load()
    st = L.current_stream()
    g = F.gen(1)
    C, Cp, cout_pad = 5, 8, 16
    gamma, beta, rm, rv = bn_params(C, g)
    part = F.partial_rows(4, C, cout_pad, g)
    assert lib.mimo_op_bn_stats(None, st) == MIMO_ERR_INVALID and lib.mimo_op_bn_relu_forward(None, st) == MIMO_ERR_INVALID
    assert lib.mimo_op_head_forward(None, st) == MIMO_ERR_INVALID
    nulls = [dict(null=k) for k in ("partial", "gamma", "beta", "running_mean", "running_var", "mean", "invstd", "scale", "shift")]
    for kw in [dict(rows=0), dict(C=0), dict(C=9), dict(Cp=12), dict(Cp=24), dict(cout_pad=4), dict(count=0), dict(route=3), dict(route=-1),
               dict(rows=2049, route=F.ROUTE_ONE)] + nulls:
        a = dict(rows=4, cout_pad=cout_pad, C=C, Cp=Cp, count=256, route=F.ROUTE_PLAN)
        a.update(kw)
        _, _, raw = bn_stats_call(part, a["rows"], a["cout_pad"], a["C"], a["Cp"], a["count"], gamma, beta, rm, rv, MOM, EPS, a["route"],
                                  expect=MIMO_ERR_INVALID, override={kw["null"]: None} if "null" in kw else None)
        assert all(bool(torch.isnan(raw[k]).all()) for k in ("mean", "invstd", "scale", "shift")), kw
        assert torch.equal(raw["running_mean"].cpu(), rm) and torch.equal(raw["running_var"].cpu(), rv), kw
    c = F.bn_relu_case(0, (2, 4, 4, 5, 8), "fp32", False)
    for kw, pooled in ((dict(C=9), False), (dict(C=0), False), (dict(ldz=6), False), (dict(lda=4), False), (dict(Cp=12), False),
                       (dict(H=0), False), (dict(ldpool=4), True), (dict(H=1), True)):
        bad = dict(c)
        bad.update(kw)
        if bad["H"] != c["H"]:   # (buffers sized for the valid case)
            a = nans(2, 4, 4, c["lda"])
            pool = nans(2, 2, 2, c["ldpool"])
            keep = [dev(c["z"]), dev(c["scale"]), dev(c["shift"])]
            args = L.BnReluForwardArgs(z=p(keep[0]), ldz=c["ldz"], scale=p(keep[1]), shift=p(keep[2]), mask=None, n=2, h=bad["H"], w=4, c=5, c_p=8,
                                       precision=0, z_fp32=0, a=p(a), lda=c["lda"], pool=p(pool) if pooled else None, ldpool=c["ldpool"], status=None)
            assert lib.mimo_op_bn_relu_forward(ct.byref(args), st) == MIMO_ERR_INVALID, kw
        else:
            a, pool, _ = bn_relu_call(bad, "fp32", pooled, expect=MIMO_ERR_INVALID)
        assert bool(torch.isnan(a).all()) and (pool is None or bool(torch.isnan(pool).all())), kw
    for kw, pooled in ((dict(z=None), False), (dict(scale=None), False), (dict(shift=None), True), (dict(a=None), False), (dict(precision=2), False),
                       (dict(n=0), False), (dict(w=0), False), (dict(w=1), True)):
        a, pool, _ = bn_relu_call(c, "fp32", pooled, expect=MIMO_ERR_INVALID, override=kw)
        assert bool(torch.isnan(a).all()) and (pool is None or bool(torch.isnan(pool).all())), kw
    x, y = torch.randn(2, 4, 4, 8).cuda(), nans(2, 2, 2, 8)
    assert lib.mimo_op_maxpool2x2_ex(None, 8, p(y), 8, 2, 4, 4, 8, 0, st) == MIMO_ERR_INVALID
    assert lib.mimo_op_maxpool2x2_ex(p(x), 8, None, 8, 2, 4, 4, 8, 0, st) == MIMO_ERR_INVALID
    assert lib.mimo_op_maxpool2x2_ex(p(x), 8, p(y), 8, 0, 4, 4, 8, 0, st) == MIMO_ERR_INVALID
    for (lda, ldo, h, cp, prec) in ((4, 8, 4, 8, 0), (8, 6, 4, 8, 0), (8, 8, 1, 8, 0), (8, 8, 4, 12, 0), (8, 8, 4, 8, 2)):
        assert lib.mimo_op_maxpool2x2_ex(p(x), lda, p(y), ldo, 2, h, 4, cp, prec, st) == MIMO_ERR_INVALID
        assert bool(torch.isnan(y).all())
    low, out, vec = torch.randn(2, 2, 2, 8).cuda(), nans(2, 4, 4, 16), torch.ones(8).cuda()
    for (hs, ldl, clp, sc, sh) in ((3, 8, 8, None, None), (4, 4, 8, None, None), (4, 8, 12, None, None), (4, 8, 8, vec, None)):
        assert lib.mimo_op_upsample_cat_ex(None, 8, p(low), ldl, p(sc), p(sh), p(out), 2, hs, 4, 8, 2, 2, clp, 0, st) == MIMO_ERR_INVALID
        assert bool(torch.isnan(out).all())
    assert lib.mimo_op_upsample_cat_ex(None, 8, None, 8, None, None, p(out), 2, 4, 4, 8, 2, 2, 8, 0, st) == MIMO_ERR_INVALID
    assert lib.mimo_op_upsample_cat_ex(None, 8, p(low), 8, None, None, None, 2, 4, 4, 8, 2, 2, 8, 0, st) == MIMO_ERR_INVALID
    for (n, ws, wl, csp, lds, prec) in ((0, 4, 2, 8, 8, 0), (2, 3, 2, 8, 8, 0), (2, 4, 0, 8, 8, 0), (2, 4, 2, 12, 12, 0), (2, 4, 2, 8, 4, 0), (2, 4, 2, 8, 8, 1)):
        assert lib.mimo_op_upsample_cat_ex(p(x), lds, p(low), 8, None, None, p(out), n, 4, ws, csp, 2, wl, 8, prec, st) == MIMO_ERR_INVALID
    assert bool(torch.isnan(out).all())
    hc = F.head_case(0, 5, 2, 2, 7, "fp32", False)
    hv = torch.ones(8).cuda()
    for kw in (dict(a=None), dict(w=None), dict(bias=None), dict(out=None), dict(n=0), dict(hw=0), dict(n=1 << 16, hw=1 << 15), dict(co=0), dict(s=-1),
               dict(subnetworks=0), dict(in_scale=p(hv)), dict(in_shift=p(hv)), dict(precision=1)):
        out_h, _ = head_call(hc, 5, 2, 2, 1, 0, 7, "fp32", False, expect=MIMO_ERR_INVALID, override=kw)
        assert bool(torch.isnan(out_h).all()), kw
    for (C, Co, S, s, lda) in ((0, 2, 1, 0, 16), (257, 2, 1, 0, 264), (5, 9, 1, 0, 16), (5, 2, 1, 1, 16), (5, 2, 1, 0, 4), (5, 2, 1, 0, 10)):
        out, _ = head_call(hc, C, Co, 2, S, s, 7, "fp32", False, lda=lda, expect=MIMO_ERR_INVALID)
        assert bool(torch.isnan(out).all())
    o, lab, _, _ = F.loss_case(0, 2, 7, 2, 3, False, False)
    badperm = torch.tensor([[0, 1], [1, 2], [0, 1]])
    assert bool(torch.isnan(loss_call(o, lab, None, badperm, 0, 1e-5, 1e3, expect=MIMO_ERR_INVALID)).all())
    assert bool(torch.isnan(loss_call(o, lab, None, None, 2, 1e-5, 1e3, expect=MIMO_ERR_INVALID)).all())
    assert bool(torch.isnan(loss_call(torch.randn(2, 3, 3, 7), lab, None, None, 0, 1e-5, 1e3, expect=MIMO_ERR_INVALID)).all())
    od, ld, lossd = o.cuda(), lab.cuda(), nans(3)
    for (po, pl, pz, n, S, co, hw) in ((None, p(ld), p(lossd), 2, 3, 2, 7), (p(od), None, p(lossd), 2, 3, 2, 7), (p(od), p(ld), None, 2, 3, 2, 7),
                                       (p(od), p(ld), p(lossd), 0, 3, 2, 7), (p(od), p(ld), p(lossd), 2, 0, 2, 7), (p(od), p(ld), p(lossd), 2, 3, 2, 0),
                                       (p(od), p(ld), p(lossd), 2, 3, 0, 7), (p(od), p(ld), p(lossd), 2, 3, 10, 7)):
        assert lib.mimo_op_loss_forward(po, pl, None, None, n, S, co, hw, 0, 1e-5, 1e3, pz, st) == MIMO_ERR_INVALID
    assert bool(torch.isnan(lossd).all())
    xin, packed = torch.randn(2, 3, 3, 4, 4).cuda(), nans(2, 4, 4, 8)
    assert lib.mimo_op_pack_input(None, 288, 144, 48, None, 0, 2, 3, 4, 4, p(packed), 8, st) == MIMO_ERR_INVALID
    assert lib.mimo_op_pack_input(p(xin), 288, 144, 48, None, 0, 2, 3, 4, 4, None, 8, st) == MIMO_ERR_INVALID
    for (count, sn, ss, s, c, cp, perm) in ((287, 144, 48, 2, 3, 8, None), (288, -1, 48, 0, 3, 8, None), (288, 144, -1, 0, 3, 8, None),
                                           (288, 144, 48, -1, 3, 8, None), (288, 144, 48, 0, 0, 8, None), (288, 144, 48, 0, 9, 8, None),
                                           (288, 144, 48, 0, 3, 6, None), (288, 144, 48, 0, 3, 8, torch.tensor([[0, 2]]).cuda())):
        assert lib.mimo_op_pack_input(p(xin), count, sn, ss, p(perm), s, 2, c, 4, 4, p(packed), cp, st) == MIMO_ERR_INVALID
        assert bool(torch.isnan(packed).all())
    dxp, dx = torch.randn(2, 6, 6, 8).cuda(), nans(2, 2, 3, 4, 4)
    assert lib.mimo_op_unpack_dx(None, 8, 2, 2, 0, 3, 4, 4, 0, p(dx), st) == MIMO_ERR_INVALID
    assert lib.mimo_op_unpack_dx(p(dxp), 8, 2, 2, 0, 3, 4, 4, 0, None, st) == MIMO_ERR_INVALID
    assert lib.mimo_op_unpack_dx(p(dxp), 8, 2, 2, 0, 3, 4, 4, 2, p(dx), st) == MIMO_ERR_INVALID     # (bf16 is no storage mode)
    assert lib.mimo_op_unpack_dx(p(dxp), 8, 2, 0, 0, 3, 4, 4, 0, p(dx), st) == MIMO_ERR_INVALID
    assert lib.mimo_op_unpack_dx(p(dxp), 8, 0, 2, 0, 3, 4, 4, 0, p(dx), st) == MIMO_ERR_INVALID
    assert lib.mimo_op_fold_image_grad(None, 8, 2, 3, 4, 4, p(dx), 0, st) == MIMO_ERR_INVALID
    assert lib.mimo_op_fold_image_grad(p(dxp), 8, 2, 3, 4, 4, None, 0, st) == MIMO_ERR_INVALID
    for (ldp, s, c, h) in ((6, 0, 3, 4), (4, 0, 5, 4), (8, 2, 3, 4), (8, -1, 3, 4), (8, 0, 3, 1), (8, 0, 0, 4)):
        assert lib.mimo_op_unpack_dx(p(dxp), ldp, 2, 2, s, c, h, 4, 0, p(dx), st) == MIMO_ERR_INVALID
        if s == 0:  # (no subnetwork argument)
            assert lib.mimo_op_fold_image_grad(p(dxp), ldp, 2, c, h, 4, p(dx), 0, st) == MIMO_ERR_INVALID
        assert bool(torch.isnan(dx).all())
