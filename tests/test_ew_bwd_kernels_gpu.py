"""The backward element-wise kernels (csrc/ew_bn_bwd.hip, ew_head_loss.hip), one operator at a time through mimo_op_fold_slice / _pool_backward /
_up_backward / _bn_relu_backward / _head_backward, per element against the fp64 references of tests/ew_bwd_reference.py
(proven against autograd by tests/test_ew_bwd_reference_cpu.py) at the geometries listed there.

Bounds.  Per-element outputs (da, dz): the convention of tests/scalar_reference.py — error <= 4 x the distance of the same
formula in fp32 torch on the CPU from fp64 (the yardstick), never below 4 fp32 ulp; no element is excluded.  Every output
here is a signed sum, whose rounding error scales with the sum of the MAGNITUDES of its terms, not with a result that may
cancel: the floor of an element (error = |got - ref| / max(|ref|, floor)) is that sum — the same reference evaluated on the
magnitudes of its inputs (abs_floor) — so an element that cancels is held to the accuracy its terms allow.  In the 16-bit
storage modes the reference is evaluated on the rounded inputs and rounded to the storage type; a result one fp32 rounding
away from a tie of that rounding lands on the neighbouring 16-bit value, so an element gets one storage ulp of its rounded
reference on top of the fp32 bound.
Per-channel sums: an exact check on small integers (any summation order gives the same integer: a dropped or doubled pixel
cannot hide) and |err| <= 2 k 2^-24 sum |term| on random data, k from the kernels' summation structure (sum_k below).
Every output buffer starts NaN-filled."""
import ctypes as ct

import pytest
import torch

from tests import ew_bwd_reference as E
from tests import scalar_reference as R
from tests.helpers import report

pytestmark = pytest.mark.gpu
NAN = float("nan")
MIMO_ERR_INVALID = -1
PRECISIONS = {"fp32": 0, "bf16-mixed": 3, "16-mixed": 4}
STORAGE_ULP = {"fp32": 0.0, "bf16-mixed": 2.0 ** -7, "16-mixed": 2.0 ** -10}  # largest relative spacing of the storage type
SUBNORMAL_STEP = {"bf16-mixed": 2.0 ** -133, "16-mixed": 2.0 ** -24}
FLOOR = R.frac_floor(R.FLOOR_SIGNED)  # every output here is a sum of signed O(1) inputs
DZ_SLOTS = 4096


def _L():
    from mimo_unet_amd import _lib
    return _lib


def dev(t):
    return None if t is None else t.contiguous().cuda()


def p(t):
    return None if t is None else t.data_ptr()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def abs_floor(fn, inputs, key="da"):
    """the sum of |term| behind every element of fn's output `key`: fn (linear, non-negative weights) on the magnitudes"""
    return fn(*[x.double().abs() if isinstance(x, torch.Tensor) and x.is_floating_point() else x for x in inputs])[key].clamp_min(1e-30)


def check_elem(kernel, name, got, ref64, y, prec="fp32", floor=None):
    """fp32 storage: R.check's measure, max |got - ref| / max(|ref|, floor) <= bound(y).  16-bit storage: the reference is rounded
    as the kernel stores it, and an element may sit one storage ulp of that rounded reference away (a result within the fp32
    bound of a rounding tie lands on the neighbouring 16-bit value; fp16 subnormals are spaced 2^-24) on top of the fp32 bound."""
    assert not bool(torch.isnan(got).any()), (kernel, name, "an expected element was left unwritten")
    fl = torch.as_tensor(FLOOR(ref64) if floor is None else floor, dtype=torch.float64)
    if prec == "fp32":
        e, at = R.elem_err(got, ref64, fl)
        allowed = R.bound(y)
        report(f"[{kernel}] {name}: err {e:.2e} yardstick {y:.2e} ratio to bound {e / allowed:.3f} worst at {at}")
        assert e <= allowed, (kernel, name, e, y, at)
        return e / allowed
    ref = E.round_to(ref64.float(), prec).double()
    allowed = R.bound(y) * torch.maximum(ref64.abs(), fl) + torch.clamp_min(STORAGE_ULP[prec] * ref.abs(), SUBNORMAL_STEP[prec])
    err = (got.double().reshape(ref.shape) - ref).abs()
    assert bool(torch.isfinite(got).all())
    ratio = float((err / allowed).max())
    report(f"[{kernel}] {name}: worst err / (fp32 bound + one storage ulp) {ratio:.3f} yardstick {y:.2e}")
    assert ratio <= 1.0, (kernel, name, ratio, y)
    return ratio


# ---- summation structure of the kernels (ew_bn_bwd.hip) ------------------------------------------------------------------
# A per-channel sum is formed as: each thread adds its n_t terms in sequence (pixels p, p + stride, ...); quad_block_sum adds
# the PPI threads of a workgroup that share a channel quad — in sequence for PPI <= 32, else 16 lanes of PPI / 16 and then those
# 16; the per-workgroup rows are summed in fp64 (grid_colsum2) and converted to float once.  Every fp32 addition errs by at
# most 2^-24 of its result <= 2^-24 sum |term|, so the chain contributes (n_t + block chain) x 2^-24 sum |term|; a term itself
# carries TERM = 4 roundings (mask, (z - mean), x invstd, x g) plus those of its gradient source (K_SRC: a fold adds up to 9
# values, the pooled source adds a folded skip to a folded route, the head forms dlogit in about 12 operations with a 2 ulp
# expf), all relative to the term evaluated on magnitudes; + 2 for the fp64 column sum and the final conversion.
K_SRC = {E.GS_PLAIN: 0, E.GS_FOLD: 8, E.GS_POOL: 18, E.GS_HEAD: 16}
TERM = 4
REDUCE = {"T": 1024, "cap": {E.GS_PLAIN: 448, E.GS_FOLD: 448, E.GS_POOL: 256, E.GS_HEAD: 256}}
APPLY = {"T": 256, "cap": {E.GS_PLAIN: 1792, E.GS_FOLD: 1792, E.GS_POOL: 1024, E.GS_HEAD: 1280}}
HEAD_BWD = {"T": 256, "cap": 1024}


def block_chain(PPI):
    return PPI if PPI <= 32 else -(-PPI // 16) + 16


def grid_of(units, Cp, T, cap):
    """(workgroups along the pixels, pixels per workgroup, terms per thread) of pq_grid / pixquad"""
    Cv = Cp // 4
    QB = min(Cv, T)
    PPI = T // QB
    gx = max(1, min(-(-units // PPI), cap))
    return gx, PPI, -(-units // (gx * PPI))


def sum_k(units, Cp, T, cap, per_unit=1, k_src=0):
    _, PPI, n_t = grid_of(units, Cp, T, cap)
    return n_t * per_unit + block_chain(PPI) + TERM + k_src + 2


def check_sum(kernel, name, got, ref64, absterm, k, largest_term=None):
    """|got - ref| <= 2 k 2^-24 sum |term| per channel; largest_term [C]: the bound must stay below the channel's largest single
    term, so that a dropped pixel of that size cannot pass."""
    assert not bool(torch.isnan(got).any()), (kernel, name, "unwritten")
    allowed = 2.0 * k * 2.0 ** -24 * absterm.double()
    err = (got.detach().cpu().double() - ref64).abs()
    ratio = float((err / allowed.clamp_min(1e-300)).max()) if err.numel() else 0.0
    report(f"[{kernel}] sum {name}: k {k} worst err / bound {ratio:.3f}")
    assert bool((err <= allowed).all()), (kernel, name, ratio)
    if largest_term is not None:
        assert bool((allowed <= largest_term.double())[largest_term > 0].all()), (kernel, name, "bound wider than one term")
    return ratio


# ---- fold_slice / pool_bwd / up_bwd -------------------------------------------------------------------------------------------

def op_variants():
    return [(choff, acc) for choff in (0, 8) for acc in (0, 1)]


@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_fold_slice_kernel(prec):
    L = _L()
    lib = L.load()
    worst = 0.0
    for (N, H, W, Cp) in E.fold_pool_geometries() + [E.PAST_GRID_HEAD]:
        for i, (choff, acc) in enumerate(op_variants()):
            g = E.gen(100 + i)
            ldp, ldda = choff + Cp + 8, Cp + 4
            dxpad = E.round_to(E.padded_grad(N, H, W, ldp, g), prec)
            prev = E.round_to(torch.randn(N, H, W, Cp, generator=g), prec)
            fn = lambda d, q: {"da": E.fold(d)[..., choff:choff + Cp] + (q if acc else 0)}
            fl = abs_floor(fn, [dxpad, prev])
            y, ref, _ = R.yardstick(fn, [dxpad, prev], {"da": fl})
            da = nans(N, H, W, ldda)
            if acc:
                da[..., :Cp] = prev.cuda()
            dxd = dev(dxpad)  # (held in a variable: a temporary's memory may be handed to the next allocation)
            L.check(lib.mimo_op_fold_slice(p(dxd), ldp, choff, p(da), ldda, N, H, W, Cp, acc, PRECISIONS[prec],
                                           L.current_stream()), "mimo_op_fold_slice")
            assert bool(torch.isnan(da[..., Cp:]).all()), "channels outside the slice were written"
            worst = max(worst, check_elem("fold_slice", f"{prec} {N}x{H}x{W}x{Cp} choff {choff} acc {acc}", da[..., :Cp].cpu(),
                                          ref["da"], y["da"], prec, fl))
            if (N, H, W, Cp) == E.PAST_GRID_HEAD:
                break
    report(f"[fold_slice] {prec} WORST err / bound {worst:.3f}")


@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_pool_backward_kernel(prec):
    L = _L()
    lib = L.load()
    worst = 0.0
    for (N, H0, W0, Cp) in E.fold_pool_geometries():
        H, W = E.pool_size(H0, W0)
        for i, (choff, acc) in enumerate(op_variants()):
            for with_skip in (False, True):
                a, g = E.pool_case(N, H, W, Cp, i, prec)
                ldp, lda, ldda, ldsk = choff + Cp + 8, Cp + 4, Cp + 8, Cp + 12
                dxpad = E.round_to(E.padded_grad(N, H // 2, W // 2, ldp, g), prec)
                skip = E.round_to(E.padded_grad(N, H, W, ldsk, g), prec) if with_skip else None
                prev = E.round_to(torch.randn(N, H, W, Cp, generator=g), prec)
                route = E.first_max(a)

                def fn(d, sk, q):
                    r = E.pool_bwd(E.fold(d)[..., choff:choff + Cp], a.to(d.dtype), None, route)
                    if acc:   # the kernel's order: route + previous content, then the skip fold
                        r = r + q
                    return {"da": r if sk is None else r + E.fold(sk)[..., :Cp]}
                fl = abs_floor(fn, [dxpad, skip, prev])
                y, ref, _ = R.yardstick(fn, [dxpad, skip, prev], {"da": fl})
                abuf = nans(N, H, W, lda)
                abuf[..., :Cp] = a.cuda()
                da = nans(N, H, W, ldda)
                if acc:
                    da[..., :Cp] = prev.cuda()
                dxd, skd = dev(dxpad), dev(skip)  # (held in variables: a temporary's memory may be handed to the next allocation)
                L.check(lib.mimo_op_pool_backward(p(dxd), ldp, choff, p(abuf), lda, p(skd), ldsk, p(da), ldda, N, H,
                                                  W, Cp, acc, PRECISIONS[prec], L.current_stream()), "mimo_op_pool_backward")
                assert bool(torch.isnan(da[..., Cp:]).all()), "channels outside the slice were written"
                worst = max(worst, check_elem("pool_bwd", f"{prec} {N}x{H}x{W}x{Cp} choff {choff} acc {acc} skip {with_skip}",
                                              da[..., :Cp].cpu(), ref["da"], y["da"], prec, fl))
    report(f"[pool_bwd] {prec} WORST err / bound {worst:.3f}")


@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_up_backward_kernel(prec):
    L = _L()
    lib = L.load()
    worst = 0.0
    for (N, H, W, h, w, Cp) in E.up_geometries():
        for i, (choff, acc) in enumerate(op_variants()):
            g = E.gen(300 + i)
            ldp, ldda = choff + Cp + 8, Cp + 4
            dxpad = E.round_to(E.padded_grad(N, H, W, ldp, g), prec)
            prev = E.round_to(torch.randn(N, h, w, Cp, generator=g), prec)
            fn = lambda d, q: {"da": E.up_bwd(d, choff, Cp, h, w) + (q if acc else 0)}
            fl = abs_floor(fn, [dxpad, prev])
            y, ref, _ = R.yardstick(fn, [dxpad, prev], {"da": fl})
            da = nans(N, h, w, ldda)
            if acc:
                da[..., :Cp] = prev.cuda()
            dxd = dev(dxpad)
            L.check(lib.mimo_op_up_backward(p(dxd), ldp, choff, p(da), ldda, N, H, W, h, w, Cp, acc, PRECISIONS[prec],
                                            L.current_stream()), "mimo_op_up_backward")
            assert bool(torch.isnan(da[..., Cp:]).all()), "channels outside the slice were written"
            worst = max(worst, check_elem("up_bwd", f"{prec} {N}x{H}x{W}<-{h}x{w}x{Cp} choff {choff} acc {acc}", da[..., :Cp].cpu(),
                                          ref["da"], y["da"], prec, fl))
    report(f"[up_bwd] {prec} WORST err / bound {worst:.3f}")


# ---- BatchNorm + ReLU backward --------------------------------------------------------------------------------------------------

def bn_reference(case, training):
    """(yardsticks, fp64 results, per-channel sums of |term|) of the case"""
    kind, C, src = case["kind"], case["C"], case["src"]
    names = E.SRC_NAMES[kind]
    meta = {k: x for k, x in src.items() if k not in names}

    def fn(z, scale, shift, mean, invstd, mask, *srcs):
        s = dict(meta)
        s.update(zip(names, srcs))
        g = E.source_gradient(kind, s, z, scale, shift, mask).to(z.dtype)
        return E.bn_relu_bwd(g, z, scale, shift, mean, invstd, mask, training)
    v = case["v"]
    inputs = [case["z"][..., :C], v["scale"][:C], v["shift"][:C], v["mean"][:C], v["invstd"][:C], case["mask"]] + [src[k] for k in names]
    i64 = [R.to64(x) for x in inputs]
    s = dict(meta)
    s.update(zip(names, i64[6:]))
    gabs = E.source_gradient(kind, s, i64[0], i64[1], i64[2], i64[5], absolute=True)
    a = E.bn_relu_bwd(gabs, i64[0], i64[1], i64[2], i64[3], i64[4], None if i64[5] is None else i64[5].abs(), False)
    dyabs = a["dz"].abs() / i64[1].abs()                      # |g| |mask| [gate]
    xhat = ((i64[0] - i64[3]) * i64[4]).abs()
    count = dyabs.shape[0] * dyabs.shape[1] * dyabs.shape[2]
    # sum of |term| behind an element of dz = scale (dy - s1 / count - xhat s2 / count)
    dz_floor = a["dz"].abs() + (i64[1].abs() * (dyabs.sum((0, 1, 2)) + xhat * (dyabs * xhat).sum((0, 1, 2))) / count if training else 0.0)
    floors = {k: FLOOR for k in ("dgamma", "dbeta", "c1", "c2", "dbias")}
    floors["dz"] = dz_floor.clamp_min(1e-30)
    y, ref, _ = R.yardstick(fn, inputs, floors)
    absterm = {"dbeta": dyabs.sum((0, 1, 2)), "dgamma": (dyabs * xhat).sum((0, 1, 2)), "dbias": a["dz"].abs().sum((0, 1, 2)),
               "dz_floor": floors["dz"], "dbeta_max": dyabs.amax((0, 1, 2)), "dgamma_max": (dyabs * xhat).amax((0, 1, 2)), "dbias_max": a["dz"].abs().amax((0, 1, 2))}
    if kind == E.GS_HEAD:
        h = E.head_bwd(i64[0].reshape(case["N"], -1, C), s["w"], s["out"], s["dout"], s["dloss"], s["label"], s["mask"], s["perm"],
                       s["s"], s["kind"], s["eps_min"], s["eps_max"], i64[1], i64[2])
        ref["head_dw"], ref["head_db"] = h["dw"], h["db"]
        dla = E.head_dlogit(s["out"], s["dout"], s["dloss"], s["label"], s["mask"], s["perm"], s["s"], s["kind"], s["eps_min"],
                            s["eps_max"], absolute=True)
        act = E.activation(i64[0], i64[1], i64[2]).reshape(case["N"], -1, C).abs()
        absterm["head_dw"] = torch.einsum("nop,npc->oc", dla, act)
        absterm["head_db"] = dla.sum((0, 2))
        absterm["head_dw_max"], absterm["head_db_max"] = head_largest_terms(dla, act)
    return y, ref, absterm


def head_largest_terms(dla, act):
    """largest single |term| of each head dw [Co, C] / db [Co] sum (dla [N, Co, HW], act [N, HW, C] magnitudes)"""
    dw = torch.stack([(dla[:, o, :, None] * act).amax((0, 1)) for o in range(dla.shape[1])])
    return dw, dla.amax((0, 2))


def run_bn(case, training, split_out=0, head_co=2):
    L = _L()
    lib = L.load()
    N, H, W, C, Cp, kind, src, v = (case[k] for k in ("N", "H", "W", "C", "Cp", "kind", "src", "v"))
    keep = {k: dev(x) for k, x in src.items() if isinstance(x, torch.Tensor)}
    keep.update(z=dev(case["z"]), mask=dev(case["mask"]), **{k: dev(x) for k, x in v.items()})
    out = dict(dz=nans(N, H, W, Cp), dgamma=nans(C), dbeta=nans(C), dbias=nans(C), c1=nans(Cp), c2=nans(Cp), head_dw=nans(2, C),
               head_db=nans(2), absmax=nans(DZ_SLOTS))
    a = L.BnReluBackwardArgs()
    a.kind, a.n, a.h, a.w, a.c, a.c_p = kind, N, H, W, C, Cp
    a.training, a.split_out, a.precision = int(training), split_out, PRECISIONS[case["prec"]]
    a.da, a.ldda = p(keep.get("da")), src.get("ldda", 0)
    a.dxpad, a.ldp, a.choff = p(keep.get("dxpad")), src.get("ldp", 0), src.get("choff", 0)
    a.skip, a.ldsk, a.skoff = p(keep.get("skip")), src.get("ldsk", 0), src.get("skoff", 0)
    if kind == E.GS_HEAD:
        a.head_w, a.head_out, a.head_dout, a.head_dloss = p(keep["w"]), p(keep.get("out")), p(keep.get("dout")), p(keep.get("dloss"))
        a.head_label, a.head_mask, a.head_perm = p(keep.get("label")), p(keep.get("mask_")), p(keep.get("perm"))
        a.head_co, a.head_subnetworks, a.head_s, a.loss_kind = head_co, 3, src["s"], src["kind"]
        a.eps_min, a.eps_max = src["eps_min"], src["eps_max"]
    a.z, a.ldz = p(keep["z"]), case["ldz"]
    a.scale, a.shift, a.mean, a.invstd, a.mask = p(keep["scale"]), p(keep["shift"]), p(keep["mean"]), p(keep["invstd"]), p(keep["mask"])
    for k in ("dz", "dgamma", "dbeta", "dbias", "c1", "c2", "head_dw", "head_db", "absmax"):
        setattr(a, k, p(out[k]))
    n_slots, status = ct.c_int32(-1), ct.c_int32(-1)
    a.absmax_capacity, a.absmax_n, a.status = DZ_SLOTS, ct.pointer(n_slots), ct.pointer(status)
    L.check(lib.mimo_op_bn_relu_backward(ct.byref(a), L.current_stream()), "mimo_op_bn_relu_backward")
    out["absmax_n"], out["status"] = n_slots.value, status.value
    return out


def head_src_to_device(case):
    """(the loss mask of the head source is stored under its own key on the device: `mask` is the layer's Dropout2d mask)"""
    if case["kind"] == E.GS_HEAD and case["src"].get("mask") is not None:
        case["src"]["mask_"] = case["src"]["mask"]
    return case


def check_bn(case, training, got, y, ref, absterm, name):
    N, H, W, C, Cp, kind = (case[k] for k in ("N", "H", "W", "C", "Cp", "kind"))
    prec = case["prec"]
    assert got["status"] == 0
    dz = got["dz"].cpu()
    assert float(dz[..., C:].abs().max() if C < Cp else 0.0) == 0.0, "padding channels of dz must be exactly zero"
    r = check_elem("bn_relu_bwd", f"{name} dz", dz[..., :C], ref["dz"], y["dz"], prec, absterm["dz_floor"])
    units = N * ((H + 1) // 2) * ((W + 1) // 2) if kind == E.GS_POOL else N * H * W
    per = 4 if kind == E.GS_POOL else 1
    k = sum_k(units, Cp, REDUCE["T"], REDUCE["cap"][kind], per, K_SRC[kind])
    rs = [check_sum("bn_bwd_stats", f"{name} {q}", got[q], ref[q], absterm[q], k, absterm[q + "_max"]) for q in ("dgamma", "dbeta")]
    count = N * H * W
    for q, s in (("c1", "dbeta"), ("c2", "dgamma")):
        assert float(got[q][C:].abs().max() if C < Cp else 0.0) == 0.0
        if training:
            err = (got[q][:C].cpu().double() - ref[q]).abs()
            assert bool((err <= 2.0 * k * 2.0 ** -24 * absterm[s] / count + 2.0 ** -24 * ref[q].abs()).all()), (name, q)
        else:
            assert float(got[q].abs().max()) == 0.0
    if training:
        assert float(got["dbias"].abs().max()) == 0.0, "the bias gradient in front of a training-mode BatchNorm is exactly zero"
    else:
        kb = sum_k(units, Cp, APPLY["T"], APPLY["cap"][kind], per, K_SRC[kind])
        rs.append(check_sum("bn_bwd_apply", f"{name} dbias", got["dbias"], ref["dbias"], absterm["dbias"], kb, absterm["dbias_max"]))
    if kind == E.GS_HEAD:
        kh = sum_k(units, Cp, REDUCE["T"], REDUCE["cap"][kind], 1, K_SRC[kind])
        rs.append(check_sum("bn_bwd_reduce", f"{name} head dw", got["head_dw"], ref["head_dw"], absterm["head_dw"], kh, absterm["head_dw_max"]))
        rs.append(check_sum("bn_bwd_reduce", f"{name} head db", got["head_db"], ref["head_db"], absterm["head_db"], kh, absterm["head_db_max"]))
    # max over the per-workgroup slots == max |dz| of the returned tensor, exactly
    gx, _, _ = grid_of(units, Cp, APPLY["T"], APPLY["cap"][kind])
    assert got["absmax_n"] == gx * -(-(Cp // 4) // 256)
    if prec == "fp32":
        assert float(got["absmax"][:got["absmax_n"]].max()) == float(got["dz"].abs().max())
    assert bool(torch.isnan(got["absmax"][got["absmax_n"]:]).all())
    return r, max(rs)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("kind", [E.GS_PLAIN, E.GS_FOLD, E.GS_POOL, E.GS_HEAD], ids=["plain", "fold", "pool", "head"])
def test_bn_relu_backward_kernels(kind, masked, training):
    worst = [0.0, 0.0]
    for i, (N, H, W, C, Cp) in enumerate(E.bn_geometries(kind)):
        case = head_src_to_device(E.bn_case(kind, N, H, W, C, Cp, masked, seed=i, variant=i))
        y, ref, absterm = bn_reference(case, training)
        got = run_bn(case, training)
        r = check_bn(case, training, got, y, ref, absterm, f"kind {kind} {N}x{H}x{W} C {C}/{Cp} variant {i % 6}")
        worst = [max(a, b) for a, b in zip(worst, r)]
    report(f"[bn_relu_bwd] kind {kind} mask {masked} training {training} WORST dz err / bound {worst[0]:.3f} sums {worst[1]:.3f}")


@pytest.mark.parametrize("prec", ["bf16-mixed", "16-mixed"])
@pytest.mark.parametrize("kind", [E.GS_PLAIN, E.GS_FOLD], ids=["plain", "fold"])
def test_bn_relu_backward_kernels_in_16_bit_storage(kind, prec):
    """The reference runs on the rounded z and gradient; dz is compared after rounding to the storage type.  (A z rounded to 16
    bits may make a gate argument exactly zero or flip it relative to the fp32 z: both sides see the rounded z.)"""
    worst = 0.0
    for training in (True, False):
        for i, (N, H, W, C, Cp) in enumerate(E.bn_geometries(kind)):
            if (N, H, W) not in ((3, 4, 5), (1, 9, 8), (37, 3, 3), (1, 85, 85)):
                continue
            case = E.bn_case(kind, N, H, W, C, Cp, True, prec=prec, seed=i)
            y, ref, absterm = bn_reference(case, training)
            got = run_bn(case, training)
            r = check_bn(case, training, got, y, ref, absterm, f"{prec} kind {kind} {N}x{H}x{W} C {C}/{Cp} training {training}")
            worst = max(worst, r[0])
    report(f"[bn_relu_bwd] {prec} kind {kind} WORST dz err / bound {worst:.3f}")


@pytest.mark.parametrize("N,H,W,C,Cp", [(1, 85, 85, 253, 256), (37, 3, 3, 5, 8), (3, 5, 4, 21, 24), (2, 9, 8, 64, 64), (3, 4, 5, 35, 40)], ids=str)
def test_bn_relu_backward_split_output_decodes_to_dz(N, H, W, C, Cp):
    """split_out = 1: the bf16 (hi, lo) pair records decode to dz within 2^-16 relative (hi = RNE(v), lo = RNE(v - hi)); the
    sums and the max |dz| slots are those of the plain output, bit for bit."""
    case = E.bn_case(E.GS_FOLD, N, H, W, C, Cp, True, seed=7)
    plain, split = run_bn(case, True), run_bn(case, True, split_out=1)
    hi, lo = E.decode_split(split["dz"].cpu().reshape(-1, Cp), Cp)
    dz = plain["dz"].cpu().reshape(-1, Cp)
    assert torch.equal(hi, dz.bfloat16().float())
    assert bool(((hi.double() + lo.double() - dz.double()).abs() <= 2.0 ** -16 * dz.double().abs()).all())
    for k in ("dgamma", "dbeta", "c1", "c2", "absmax"):
        n = plain["absmax_n"] if k == "absmax" else None
        assert torch.equal(bits(plain[k][:n]), bits(split[k][:n])), k


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind", [E.GS_PLAIN, E.GS_FOLD, E.GS_POOL, E.GS_HEAD], ids=["plain", "fold", "pool", "head"])
@pytest.mark.parametrize("N,H,W,C,Cp", [(1, 85, 85, 253, 256), (37, 5, 4, 5, 8), (3, 9, 8, 17, 24)], ids=str)
def test_per_channel_sums_are_exact_on_small_integers(N, H, W, C, Cp, kind, training):
    """Small-integer g, z and head activations, mean 0, invstd = scale = 1, shift 8 (every gate open), mask of ones: every
    per-channel sum is an integer below 2^24, which fp32 adds exactly in any order."""
    case = head_src_to_device(E.bn_case(kind, N, H, W, C, Cp, True, seed=11, exact=True, variant=1))
    _, ref, _ = bn_reference(case, training)
    got = run_bn(case, training)
    names = ["dgamma", "dbeta"] + ([] if training else ["dbias"]) + (["head_dw", "head_db"] if kind == E.GS_HEAD else [])
    for k in names:
        assert float(ref[k].abs().max()) < 2 ** 24 and bool((ref[k] == ref[k].round()).all())
        assert torch.equal(got[k].cpu().double(), ref[k]), (k, float((got[k].cpu().double() - ref[k]).abs().max()))
    assert got["status"] == 0


# ---- the head ----------------------------------------------------------------------------------------------------------------------

def run_head(N, HW, C, Cp, Co, a, lda, w, hi, s, kind, in_scale=None, in_shift=None, prec="fp32"):
    L = _L()
    lib = L.load()
    keep = {k: dev(x) for k, x in hi.items()}
    keep.update(a=dev(a), w=dev(w), sc=dev(in_scale), sh=dev(in_shift))
    out = dict(da=nans(N, HW, Cp), dw=nans(Co, C), db=nans(Co))
    h = L.HeadBackwardArgs()
    h.a, h.lda, h.w = p(keep["a"]), lda, p(keep["w"])
    h.c, h.c_p, h.co, h.n, h.subnetworks, h.s, h.hw = C, Cp, Co, N, 3, s, HW
    h.out, h.dout, h.dloss, h.label, h.mask, h.perm = (p(keep[k]) for k in ("out", "dout", "dloss", "label", "mask", "perm"))
    h.loss_kind, h.eps_min, h.eps_max = kind, R.f32(E.EPS_MIN), R.f32(E.EPS_MAX)
    h.in_scale, h.in_shift, h.precision = p(keep["sc"]), p(keep["sh"]), PRECISIONS[prec]
    h.da, h.dw, h.db = p(out["da"]), p(out["dw"]), p(out["db"])
    L.check(lib.mimo_op_head_backward(ct.byref(h), L.current_stream()), "mimo_op_head_backward")
    return out


HEAD_GEOMETRIES = [(3, 20, 8), (1, 72, 24), (37, 9, 8), (37, 10, 8), (2, 30, 64), (1, 1440, 256), (1, 129 * 128, 256)]


@pytest.mark.parametrize("kind", [E.LAPLACE, E.GAUSSIAN], ids=["laplace", "gaussian"])
@pytest.mark.parametrize("use_dout,use_dloss", E.HEAD_MODES, ids=["dout", "dloss", "both"])
def test_head_backward_kernel(use_dout, use_dloss, kind):
    """in_scale / in_shift present and absent, perm and mask present and absent, 2 and 4 logits, logits whose exp lies below
    eps_min, above eps_max and inside; the last geometry runs one unrolled group of pixels past kEwMaxBlocks workgroups."""
    worst = [0.0, 0.0]
    for i, (N, HW, Cp) in enumerate(HEAD_GEOMETRIES):
        for C in (E.logical_channels(Cp) if HW <= 72 else (Cp - 3,)):
            g = E.gen(2000 + i)
            Co, fused, extras = (4 if i == 4 else 2), bool(i & 1), i % 3 != 2
            hi = E.head_inputs(N, 3, Co, HW, g, use_dout, use_dloss, extras, extras)
            lda, s = Cp + 4, 1
            a = torch.full((N, HW, lda), NAN)
            a[..., :Cp] = 0.0
            a[..., :C] = E.away_from_zero(torch.randn(N, HW, C, generator=g))
            w = torch.randn(Co, C, generator=g)
            v = E.bn_vectors(C, Cp, g)
            if fused:
                a.view(-1, lda)[0::5, 0] = E.ZERO_GATE_Z[0]
            sc, sh = (v["scale"], v["shift"]) if fused else (None, None)
            meta = dict(perm=hi["perm"])

            def fn(a_, w_, out, dout, dloss, label, mask, sc_, sh_):
                return E.head_bwd(a_, w_, out, dout, dloss, label, mask, meta["perm"], s, kind, R.f32(E.EPS_MIN), R.f32(E.EPS_MAX), sc_, sh_)
            inputs = [a[..., :C], w, hi["out"], hi["dout"], hi["dloss"], hi["label"], hi["mask"], None if sc is None else sc[:C],
                      None if sh is None else sh[:C]]
            i64 = [R.to64(x) for x in inputs]
            dla = E.head_dlogit(i64[2], i64[3], i64[4], i64[5], i64[6], hi["perm"], s, kind, R.f32(E.EPS_MIN), R.f32(E.EPS_MAX), absolute=True)
            fl = torch.einsum("nop,oc->npc", dla, i64[1].abs()).clamp_min(1e-30)  # sum of |term| behind an element of da
            floors = {k: FLOOR for k in ("dlogit", "dw", "db")}
            floors["da"] = fl
            y, ref, _ = R.yardstick(fn, inputs, floors)
            got = run_head(N, HW, C, Cp, Co, a, lda, w, hi, s, kind, sc, sh)
            name = f"{N}x{HW} C {C}/{Cp} Co {Co} fused {fused} perm+mask {extras}"
            da = got["da"].cpu()
            assert float(da[..., C:].abs().max() if C < Cp else 0.0) == 0.0, "padding channels of da must be exactly zero"
            worst[0] = max(worst[0], check_elem("head_bwd", f"{name} da", da[..., :C], ref["da"], y["da"], floor=fl))
            act = (E.activation(i64[0][:, None], i64[7], i64[8])[:, 0] if fused else i64[0]).abs()
            k = sum_k(N * HW, Cp, HEAD_BWD["T"], HEAD_BWD["cap"], 1, K_SRC[E.GS_HEAD])
            dw_max, db_max = head_largest_terms(dla, act)
            worst[1] = max(worst[1], check_sum("head_bwd", f"{name} dw", got["dw"], ref["dw"], torch.einsum("nop,npc->oc", dla, act), k, dw_max),
                           check_sum("head_bwd", f"{name} db", got["db"], ref["db"], dla.sum((0, 2)), k, db_max))
    report(f"[head_bwd] dout {use_dout} dloss {use_dloss} kind {kind} WORST da err / bound {worst[0]:.3f} sums {worst[1]:.3f}")


@pytest.mark.parametrize("fused", [False, True], ids=["activation", "preactivation"])
@pytest.mark.parametrize("N,HW,C,Cp,Co", [(3, 20, 5, 8, 2), (37, 10, 8, 8, 4), (2, 30, 61, 64, 4), (1, 1441, 21, 24, 2),
                                          (1, 129 * 128, 253, 256, 2)], ids=str)
def test_head_backward_sums_are_exact_on_small_integers(N, HW, C, Cp, Co, fused):
    """head_bwd_kernel's own sums (its 4-pixel unrolled loop clamps the tail index to P - 1 and discards the result: where a
    doubled or dropped pixel would arise): integer dout, w and activations (with in_scale = 1, in_shift = 8: a + 8, every gate
    open) make dw, db and da integers below 2^24, equal to the fp64 sums in any order.  Pixel counts that are no multiple of
    the unrolled group, one of them past kEwMaxBlocks workgroups."""
    g = E.gen(2200)
    ints = lambda *shape: torch.randint(-3, 4, shape, generator=g).float()
    hi = dict(out=None, dout=ints(N, 3, Co, HW), dloss=None, label=None, mask=None, perm=None)
    lda, s = Cp + 4, 2
    a = torch.full((N, HW, lda), NAN)
    a[..., :Cp] = 0.0
    a[..., :C] = ints(N, HW, C)
    w = ints(Co, C)
    v = E.bn_vectors(C, Cp, g, exact=True)
    sc, sh = (v["scale"], v["shift"]) if fused else (None, None)
    ref = E.head_bwd(a[..., :C].double(), w.double(), None, hi["dout"].double(), None, None, None, None, s, E.LAPLACE, E.EPS_MIN, E.EPS_MAX,
                     None if sc is None else sc[:C].double(), None if sh is None else sh[:C].double())
    got = run_head(N, HW, C, Cp, Co, a, lda, w, hi, s, E.LAPLACE, sc, sh)
    for k in ("dw", "db", "da"):
        assert float(ref[k].abs().max()) < 2 ** 24 and bool((ref[k] == ref[k].round()).all())
        x = got[k].cpu()[..., :C] if k == "da" else got[k].cpu()
        assert torch.equal(x.double(), ref[k]), (k, float((x.double() - ref[k]).abs().max()))


@pytest.mark.parametrize("prec", ["bf16-mixed", "16-mixed"])
def test_head_backward_kernel_in_16_bit_storage(prec):
    g = E.gen(2100)
    N, HW, C, Cp, Co, s = 3, 20, 21, 24, 2, 1
    hi = E.head_inputs(N, 3, Co, HW, g, True, True, True, True)
    a = torch.zeros(N, HW, Cp)
    a[..., :C] = E.away_from_zero(torch.randn(N, HW, C, generator=g))
    a = E.round_to(a, prec)
    w = torch.randn(Co, C, generator=g)
    fn = lambda a_, w_, out, dout, dloss, label, mask: E.head_bwd(a_, w_, out, dout, dloss, label, mask, hi["perm"], s, E.LAPLACE,
                                                                 R.f32(E.EPS_MIN), R.f32(E.EPS_MAX))
    y, ref, _ = R.yardstick(fn, [a[..., :C], w, hi["out"], hi["dout"], hi["dloss"], hi["label"], hi["mask"]],
                            {k: FLOOR for k in ("dlogit", "da", "dw", "db")})
    got = run_head(N, HW, C, Cp, Co, a, Cp, w, hi, s, E.LAPLACE, prec=prec)
    i64 = [R.to64(x) for x in (a[..., :C], w, hi["out"], hi["dout"], hi["dloss"], hi["label"], hi["mask"])]
    dla = E.head_dlogit(i64[2], i64[3], i64[4], i64[5], i64[6], hi["perm"], s, E.LAPLACE, R.f32(E.EPS_MIN), R.f32(E.EPS_MAX), absolute=True)
    fl = torch.einsum("nop,oc->npc", dla, i64[1].abs()).clamp_min(1e-30)
    check_elem("head_bwd", f"{prec} da", got["da"].cpu()[..., :C], ref["da"], y["da"], prec, fl)
    # (dw / db stay fp32: sums of fp32 products of the rounded activations)
    k = sum_k(N * HW, Cp, HEAD_BWD["T"], HEAD_BWD["cap"], 1, K_SRC[E.GS_HEAD])
    dw_max, db_max = head_largest_terms(dla, i64[0].abs())
    check_sum("head_bwd", f"{prec} dw", got["dw"], ref["dw"], torch.einsum("nop,npc->oc", dla, i64[0].abs()), k, dw_max)
    check_sum("head_bwd", f"{prec} db", got["db"], ref["db"], dla.sum((0, 2)), k, db_max)


# ---- equivalences the plan relies on: compared bit for bit ----------------------------------------------------------------------------

def test_fused_sources_give_the_bits_of_the_unfused_chain():
    """GS_FOLD = fold_slice + GS_PLAIN, GS_POOL = pool_bwd + GS_PLAIN, GS_HEAD = head_bwd + GS_PLAIN for dz.  Eval mode on random
    data (dz = scale * dy: no sums involved); training mode on the exact-integer data, whose sums — and so c1, c2 — are the same
    whatever the order of summation (the fused reductions visit cells / pixels in another order than the plain one)."""
    L = _L()
    lib = L.load()
    for (N, H, W, C, Cp) in [(3, 5, 4, 5, 8), (37, 4, 5, 21, 24), (1, 9, 8, 61, 64), (1, 40, 36, 253, 256)]:
        for training, exact in ((False, False), (True, True)):
            for kind in (E.GS_FOLD, E.GS_POOL, E.GS_HEAD):
                for masked in (True, False):
                    case = head_src_to_device(E.bn_case(kind, N, H, W, C, Cp, masked, seed=21, exact=exact, variant=5))
                    fused = run_bn(case, training)
                    src, da = case["src"], nans(N, H, W, Cp)
                    st = L.current_stream()
                    dxd = dev(src.get("dxpad"))
                    if kind == E.GS_FOLD:
                        L.check(lib.mimo_op_fold_slice(p(dxd), src["ldp"], 0, p(da), Cp, N, H, W, Cp, 0, 0, st))
                    elif kind == E.GS_POOL:
                        a = torch.zeros(N, H, W, Cp)
                        v = case["v"]
                        a[..., :C] = E.act32(case["z"][..., :C], v["scale"][:C], v["shift"][:C], case["mask"])
                        sk = None if src["skip"] is None else src["skip"][..., src["skoff"]:].contiguous()
                        ad, skd = dev(a), dev(sk)
                        L.check(lib.mimo_op_pool_backward(p(dxd), src["ldp"], src["choff"], p(ad), Cp, p(skd),
                                                          src["ldsk"] - src["skoff"], p(da), Cp, N, H, W, Cp, 0, 0, st))
                    else:
                        hi = {k: src.get(k) for k in ("out", "dout", "dloss", "label", "mask", "perm")}
                        da = run_head(N, H * W, C, Cp, 2, case["z"].reshape(N, H * W, -1), case["ldz"], src["w"], hi, src["s"], src["kind"],
                                      case["v"]["scale"], case["v"]["shift"])["da"].reshape(N, H, W, Cp)
                    plain = dict(case, kind=E.GS_PLAIN, src=dict(kind_gs=0, da=da.cpu(), ldda=Cp))
                    unfused = run_bn(plain, training)
                    assert torch.equal(bits(fused["dz"]), bits(unfused["dz"])), (kind, N, H, W, C, Cp, training, masked)


# ---- argument validation: MIMO_ERR_INVALID, nothing launched ---------------------------------------------------------------------------

def test_entry_points_reject_what_the_kernels_do_not_cover():
    L = _L()
    lib = L.load()
    st = L.current_stream()
    buf, out = torch.zeros(1 << 16, device="cuda"), nans(1 << 16)
    bad = []
    for (h, w, cp) in [(1, 4, 8), (4, 1, 8), (4, 4, 12), (4, 4, 0)]:
        bad.append(lib.mimo_op_fold_slice(p(buf), cp + 8, 0, p(out), cp, 1, h, w, cp, 0, 0, st))
        bad.append(lib.mimo_op_up_backward(p(buf), cp + 8, 0, p(out), cp, 1, h, w, h // 2, w // 2, cp, 0, 0, st))
    bad.append(lib.mimo_op_fold_slice(p(buf), 8, 8, p(out), 8, 1, 4, 4, 8, 0, 0, st))             # the slice leaves the pixel
    bad.append(lib.mimo_op_fold_slice(p(buf), 16, 0, p(out), 4, 1, 4, 4, 8, 0, 0, st))
    bad.append(lib.mimo_op_pool_backward(p(buf), 8, 0, p(buf), 8, None, 0, p(out), 8, 1, 3, 4, 8, 0, 0, st))  # pooled 1 x 2
    bad.append(lib.mimo_op_pool_backward(p(buf), 8, 0, p(buf), 8, p(buf), 4, p(out), 8, 1, 4, 4, 8, 0, 0, st))
    bad.append(lib.mimo_op_up_backward(p(buf), 8, 0, p(out), 8, 1, 6, 4, 2, 2, 8, 0, 0, st))      # H / 2 != h
    bad.append(lib.mimo_op_up_backward(p(buf), 8, 0, p(out), 8, 1, 4, 7, 2, 2, 8, 0, 0, st))
    for kind in (E.GS_POOL, E.GS_HEAD):                                                              # fused sources: fp32 storage only
        case = head_src_to_device(E.bn_case(kind, 1, 4, 4, 5, 8, False, seed=1, variant=5))
        for prec in ("bf16-mixed", "16-mixed"):
            with pytest.raises(L.MimoHipError):
                run_bn(dict(case, prec=prec), True)
    assert bad and all(rc == MIMO_ERR_INVALID for rc in bad), bad
    case = head_src_to_device(E.bn_case(E.GS_HEAD, 1, 4, 4, 5, 8, False, seed=1, variant=5))
    with pytest.raises(L.MimoHipError):
        run_bn(case, True, head_co=4)                                                                 # the head source: 2 logits only
    h = L.HeadBackwardArgs()
    h.a, h.w, h.dout, h.da, h.dw, h.db = p(buf), p(buf), p(buf), p(out), p(out), p(out)
    h.lda, h.c, h.c_p, h.co, h.n, h.subnetworks, h.s, h.hw = 8, 5, 8, 3, 1, 1, 0, 4
    assert lib.mimo_op_head_backward(ct.byref(h), st) == MIMO_ERR_INVALID                            # odd co
    h.co, h.c_p = 2, 260
    assert lib.mimo_op_head_backward(ct.byref(h), st) == MIMO_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a rejected call wrote to its output"
