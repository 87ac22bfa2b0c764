"""Plain torch references of the backward element-wise operators (mimo_unet_amd/csrc/ew_bn_bwd.hip, ew_head_loss.hip: fold_slice, pool_bwd,
up_bwd, the BatchNorm + ReLU backward chain with its four gradient sources, head_bwd), the input generators of their tests and
the geometries both test files run: tests/test_ew_bwd_reference_cpu.py proves every function against fp64 autograd through
the torch modules the model composes, tests/test_ew_bwd_kernels_gpu.py runs the kernels against them.

Every function is dtype-generic and a function of the SAME fp32 inputs the kernel sees (scale / shift / mean / invstd are
inputs, never re-derived from z): on fp64 copies it is the truth, on the fp32 tensors it is "the formula in fp32 torch on the
CPU", whose distance from the truth is the yardstick of tests/scalar_reference.py.  Decisions — the ReLU gate and the arg-max of
a pooling window — are not arithmetic: they are always taken on the fp64 value (the window activations rounded to fp32 first),
so a yardstick never contains a flipped decision.  All tensors NHWC."""
import math

import torch

LAPLACE, GAUSSIAN = 0, 1
GS_PLAIN, GS_FOLD, GS_POOL, GS_HEAD = 0, 1, 2, 3


# ---- operators ---------------------------------------------------------------------------------------------------------

def fold(dxpad):
    """Transpose of 1-pixel reflect padding, [N, H+2, W+2, C] -> [N, H, W, C]: pad row -1 folds onto row 1, pad row H onto row
    H-2; columns alike; a corner folds twice (rows first, then the folded pad columns)."""
    H, W = dxpad.shape[1] - 2, dxpad.shape[2] - 2
    assert H >= 2 and W >= 2
    r = dxpad[:, 1:-1].clone()
    r[:, 1] += dxpad[:, 0]
    r[:, H - 2] += dxpad[:, H + 1]
    c = r[:, :, 1:-1].clone()
    c[:, :, 1] += r[:, :, 0]
    c[:, :, W - 2] += r[:, :, W + 1]
    return c


def windows(a):
    """[N, H, W, C] -> [N, H//2, W//2, C, 4], the 2x2 windows in scan order (0,0),(0,1),(1,0),(1,1)"""
    N, H, W, C = a.shape
    Hp, Wp = H // 2, W // 2
    v = a[:, :2 * Hp, :2 * Wp].reshape(N, Hp, 2, Wp, 2, C)
    return v.permute(0, 1, 3, 5, 2, 4).reshape(N, Hp, Wp, C, 4)


def first_max(a):
    """one-hot [N, Hp, Wp, C, 4] (bool) of the FIRST maximum of each window in scan order (route_max's strict '>' update).
    The comparison is made on the values rounded to fp32, as the kernel sees them."""
    v = windows(a.double().float())
    eq = v == v.max(dim=-1, keepdim=True).values
    return eq & (eq.cumsum(-1) == 1)


def unwindow(r, H, W):
    """inverse of windows(): [N, Hp, Wp, C, 4] -> [N, H, W, C], zeros in the last row / column of an odd size"""
    N, Hp, Wp, C, _ = r.shape
    out = r.new_zeros(N, H, W, C)
    out[:, :2 * Hp, :2 * Wp] = r.reshape(N, Hp, Wp, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * Hp, 2 * Wp, C)
    return out


def pool_bwd(g_pooled, a, skip_folded=None, route=None):
    """MaxPool2d(2) backward: g_pooled [N, H//2, W//2, C] goes to the first maximum of each window of a [N, H, W, C]; the odd
    last row / column gets none; + an already folded skip gradient.  route: first_max(a) computed elsewhere."""
    N, H, W, C = a.shape
    sel = first_max(a) if route is None else route
    da = unwindow(torch.where(sel, g_pooled.unsqueeze(-1), g_pooled.new_zeros(())), H, W)
    return da if skip_folded is None else da + skip_folded


def lerp_matrix(n_in, dtype):
    """[2 n_in, n_in]: bilinear x2 align_corners=True interpolation weights (src = o (in - 1) / (out - 1))"""
    n_out = 2 * n_in
    M = torch.zeros(n_out, n_in, dtype=dtype)
    scale = torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=dtype)
    for o in range(n_out):
        src = scale * torch.tensor(float(o), dtype=dtype)
        i0 = min(int(src), n_in - 1)
        l1 = (src - i0).clamp(0, 1)
        M[o, i0] += 1 - l1
        M[o, i0 + (1 if i0 < n_in - 1 else 0)] += l1
    return M


def up_bwd(dxpad, choff, C, h, w):
    """Transpose of Upsample(x2, bilinear, align_corners=True) + F.pad([d // 2, d - d // 2]) applied to
    fold(dxpad)[..., choff : choff + C]: [N, H+2, W+2, ld] -> [N, h, w, C]"""
    g = fold(dxpad)[..., choff:choff + C]
    H, W = g.shape[1], g.shape[2]
    pt, pl = (H - 2 * h) // 2, (W - 2 * w) // 2
    g = g[:, pt:pt + 2 * h, pl:pl + 2 * w]
    return torch.einsum("oi,nopc,pj->nijc", lerp_matrix(h, g.dtype), g, lerp_matrix(w, g.dtype))


def gate(z, scale, shift):
    """[z * scale + shift > 0] on the exact value: the fp64 product of two fp32 numbers is exact and the sum's sign is the exact
    sum's sign (nothing underflows for magnitudes in [2^-20, 2^20]) — the sign of the kernel's correctly rounded fmaf"""
    return (z.double() * scale.double() + shift.double()) > 0


def activation(z, scale, shift, mask=None):
    """relu(z * scale + shift) * mask[n][c] in z's dtype, the ReLU decided by gate()"""
    a = torch.where(gate(z, scale, shift), z * scale + shift, z.new_zeros(()))
    return a if mask is None else a * mask[:, None, None, :]


def bn_relu_bwd(g, z, scale, shift, mean, invstd, mask, training):
    """g, z [N, H, W, C]; the four vectors [C]; mask [N, C] or None.  Returns dz, dgamma, dbeta, c1, c2, dbias and the
    per-channel sums of |term| of s1, s2 and sum dz (the scale of their rounding bounds)."""
    dy = g if mask is None else g * mask[:, None, None, :]
    dy = torch.where(gate(z, scale, shift), dy, dy.new_zeros(()))
    xhat = (z - mean) * invstd
    count = z.shape[0] * z.shape[1] * z.shape[2]
    s1, s2 = dy.sum((0, 1, 2)), (dy * xhat).sum((0, 1, 2))
    if training:
        c1, c2 = s1 / count, s2 / count
        dz = scale * (dy - c1 - xhat * c2)
        dbias = torch.zeros_like(s1)
    else:
        c1 = c2 = torch.zeros_like(s1)
        dz = scale * dy
        dbias = dz.sum((0, 1, 2))
    return {"dz": dz, "dgamma": s2, "dbeta": s1, "c1": c1, "c2": c2, "dbias": dbias}


def nll_grad(kind, d, lp, eps_min, eps_max):
    """closed-form d NLL / d (mean, log-parameter); the clamp acts on the value only, d/dlog keeps the unclamped exp"""
    e = torch.exp(lp)
    sc = e.clamp(eps_min, eps_max)
    if kind == LAPLACE:
        return torch.sign(d) / sc, (1 / sc - d.abs() / (sc * sc)) * e
    return 2 * d / sc, (1 / sc - d * d / (sc * sc)) * e


def head_dlogit(out, dout, dloss, label, mask, perm, s, kind, eps_min, eps_max, absolute=False):
    """dlogit [N, Co, HW] of subnetwork s = dout[:, s] + dloss[s] / count * mask * dNLL (count = N * Co/2 * HW); out, dout
    [N, S, Co, HW]; label [N, Co/2, HW]; mask [N, HW]; perm [S, N] (image n of subnetwork s carries the label of image
    perm[s][n]).  absolute: every term replaced by its magnitude (the scale of a rounding bound)."""
    like = out if out is not None else dout
    N, S, Co, HW = like.shape
    Ct = Co // 2
    dl = like.new_zeros(N, Co, HW)
    if dout is not None:
        dl = dl + (dout[:, s].abs() if absolute else dout[:, s])
    if dloss is not None:
        src = perm[s] if perm is not None else torch.arange(N)
        mu, lp = out[:, s, :Ct], out[:, s, Ct:]
        d = mu - label[src]
        coef = dloss[s] / (N * Ct * HW)
        mk = mask[src][:, None, :] if mask is not None else 1.0
        if absolute:
            e = torch.exp(lp)
            sc = e.clamp(eps_min, eps_max)
            gm = (1 / sc if kind == LAPLACE else 2 * d.abs() / sc)
            gl = (1 / sc + (d.abs() if kind == LAPLACE else d * d) / (sc * sc)) * e
            dl = dl + torch.cat([gm * torch.sign(d).abs() if kind == LAPLACE else gm, gl], 1) * (coef * mk).abs()
        else:
            gm, gl = nll_grad(kind, d, lp, eps_min, eps_max)
            dl = dl + coef * mk * torch.cat([gm, gl], 1)
    return dl


def head_bwd(a, w, out, dout, dloss, label, mask, perm, s, kind, eps_min, eps_max, in_scale=None, in_shift=None):
    """a [N, HW, C] (the head's input, or its pre-activation with in_scale / in_shift [C]); w [Co, C].
    Returns dlogit [N, Co, HW], da [N, HW, C], dw [Co, C], db [Co]."""
    if in_scale is not None:
        a = activation(a[:, None], in_scale, in_shift)[:, 0]
    dl = head_dlogit(out, dout, dloss, label, mask, perm, s, kind, eps_min, eps_max)
    return {"dlogit": dl, "da": torch.einsum("nop,oc->npc", dl, w), "dw": torch.einsum("nop,npc->oc", dl, a), "db": dl.sum((0, 2))}


# ---- the gradient arriving at a BatchNorm + ReLU layer, per source -------------------------------------------------------

def source_gradient(kind, src, z, scale, shift, mask, absolute=False):
    """g [N, H, W, C] for a case's source tensors `src` (dict).  absolute: the same expression with every input replaced by
    its magnitude and every weight by its magnitude — an upper bound of the sum of |term| behind each element."""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    C = z.shape[-1]
    if kind == GS_PLAIN:
        return ab(src["da"][..., :C])
    if kind == GS_FOLD:
        return fold(ab(src["dxpad"]))[..., :C]
    if kind == GS_POOL:
        gp = fold(ab(src["dxpad"]))[..., src["choff"]:src["choff"] + C]
        sk = fold(ab(src["skip"]))[..., src["skoff"]:src["skoff"] + C] if src.get("skip") is not None else None
        return pool_bwd(gp, activation(z.double(), scale.double(), shift.double(), None if mask is None else mask.double()), sk)
    N, H, W, _ = z.shape
    dl = head_dlogit(src["out"], src["dout"], src["dloss"], src["label"], src["mask"], src["perm"], src["s"], src["kind"],
                     src["eps_min"], src["eps_max"], absolute)
    return torch.einsum("nop,oc->npc", dl, ab(src["w"])).reshape(N, H, W, C)


# ---- storage formats -------------------------------------------------------------------------------------------------

def decode_split(raw, Cp):
    """bf16 (hi, lo) pair records of a [P, Cp] fp32-sized buffer (st_split4: per pixel and 32-channel chunk [hi x r | lo x r],
    r = min(32, Cp - 32 chunk)) -> (hi, lo) as fp32 [P, Cp]"""
    P = raw.numel() // Cp
    b = raw.contiguous().view(torch.int16).reshape(P, 2 * Cp).to(torch.int32)
    hi, lo = torch.zeros(P, Cp), torch.zeros(P, Cp)
    for c0 in range(0, Cp, 32):
        r = min(32, Cp - c0)
        for dst, off in ((hi, 2 * c0), (lo, 2 * c0 + r)):
            dst[:, c0:c0 + r] = (b[:, off:off + r] << 16).view(torch.float32)
    return hi, lo


def round_to(t, precision):
    """fp32 values as stored in a storage mode ("fp32", "bf16-mixed", "16-mixed")"""
    return t if precision == "fp32" else t.to(torch.bfloat16 if precision == "bf16-mixed" else torch.float16).float()


# ---- inputs ------------------------------------------------------------------------------------------------------------

LO, HI = 2.0 ** -20, 2.0 ** 20


def gen(seed):
    return torch.Generator().manual_seed(seed)


def away_from_zero(t):
    """magnitudes into [2^-20, 2^20], signs kept"""
    return torch.where(t >= 0, 1.0, -1.0) * t.abs().clamp(LO, HI)


def bn_vectors(C, Cp, g, exact=False):
    """scale, shift, mean, invstd [Cp] (padding channels zero, as the plan leaves them).  Channels 0 and 1 carry power-of-two
    scales so that planted pre-activations make z * scale + shift exactly 0."""
    v = {k: torch.zeros(Cp) for k in ("scale", "shift", "mean", "invstd")}
    if exact:
        v["scale"][:C], v["shift"][:C], v["invstd"][:C] = 1.0, 8.0, 1.0
        return v
    sign = torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    v["scale"][:C] = sign * (0.5 + 1.5 * torch.rand(C, generator=g))
    v["shift"][:C] = away_from_zero(0.5 * torch.randn(C, generator=g))
    v["mean"][:C] = 0.3 * torch.randn(C, generator=g)
    v["invstd"][:C] = 0.5 + torch.rand(C, generator=g)
    v["scale"][0], v["shift"][0] = 0.5, -1.5      # z = 3     -> exactly 0
    if C > 1:
        v["scale"][1], v["shift"][1] = -2.0, 0.25  # z = 0.125 -> exactly 0
    return v


ZERO_GATE_Z = (3.0, 0.125)


def preact(N, H, W, C, Cp, ldz, g, plant_zero_gates=True):
    """z [N, H, W, ldz]: random in channels < C, zero padding channels, NaN beyond Cp (never read).  Every 5th pixel holds the
    value that makes the gate argument of channels 0 / 1 exactly zero."""
    z = torch.full((N, H, W, ldz), float("nan"))
    z[..., :Cp] = 0.0
    z[..., :C] = away_from_zero(torch.randn(N, H, W, C, generator=g))
    if plant_zero_gates:
        flat = z.view(-1, ldz)
        for c, val in enumerate(ZERO_GATE_Z[:min(C, 2)]):
            flat[c::5, c] = val
    return z


def ulp_of(t):
    """fp32 ulp of the binade of |t| (fp32 tensor)"""
    _, e = torch.frexp(t.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(t), e - 24)


def window_gap_violations(a32):
    """bool [N, Hp, Wp, C]: windows in which two members are neither exactly equal nor more than 4 fp32 ulp apart"""
    v = windows(a32)
    bad = torch.zeros(v.shape[:-1], dtype=torch.bool)
    for i in range(4):
        for j in range(i + 1, 4):
            x, y = v[..., i], v[..., j]
            bad |= (x != y) & ((x - y).abs() <= 4 * torch.maximum(ulp_of(x), ulp_of(y)))
    return bad


def act32(z, scale, shift, mask):
    """the window activations the way the issue defines them: formed in fp64, rounded to fp32"""
    return activation(z.double(), scale.double(), shift.double(), None if mask is None else mask.double()).float()


def pooled_preact(N, H, W, C, Cp, ldz, v, mask, g):
    """preact() for a pooled tensor: windows with planted exact ties in every position (duplicated z — pairs, triples and all
    four — ReLU-zeroed members, whole all-zero windows), every other pair of window members more than 4 ulp apart after
    relu(fma) * mask: offending windows are redrawn.  Returns z and the number of redraw rounds."""
    z = preact(N, H, W, C, Cp, ldz, g, plant_zero_gates=False)
    Hp, Wp = H // 2, W // 2
    zc = z[..., :C]
    planted = torch.zeros(N, H, W, C, dtype=torch.bool)
    sc, sh = v["scale"][:C], v["shift"][:C]
    closed = away_from_zero((-1.0 - sh) / sc - torch.sign(sc) * 0.5)  # pre-activation <= -1: ReLU-zeroed
    big = away_from_zero((2.5 - sh) / sc)                             # pre-activation ~ 2.5: the window's maximum in most cases
    lower0 = (1.5 - sh[0]) / sc[0] if float(sc[0]) > 0 else None
    assert lower0 is not None, "channel 0 carries bn_vectors' positive power-of-two scale"
    groups = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1, 2), (1, 2, 3), (0, 1, 2, 3), "zero", "zero03", None, None]
    k = 0
    for n in range(N):
        for py in range(Hp):
            for px in range(Wp):
                grp = groups[k % len(groups)]
                k += 1
                if grp is None:
                    continue
                pos = [(n, 2 * py + (j >> 1), 2 * px + (j & 1)) for j in range(4)]
                if isinstance(grp, str):
                    for j in (range(4) if grp == "zero" else (0, 3)):
                        zc[pos[j]] = closed
                        planted[pos[j]] = True
                else:  # duplicated z: the maximum in ~70 % of the channels, whatever was drawn in the others; in channel 0
                    # always the maximum (the other members are held to a pre-activation <= 1.5), so that tied maxima of 2, 3
                    # and 4 members in every position do not depend on the draw
                    use_big = torch.rand(C, generator=g) < 0.7
                    use_big[0] = True
                    first = torch.where(use_big, big, zc[pos[grp[0]]])
                    for j in range(4):
                        if j in grp:
                            zc[pos[j]] = first
                            planted[pos[j]] = True
                        else:
                            zc[pos[j] + (0,)] = away_from_zero(torch.minimum(zc[pos[j] + (0,)], lower0))
                            planted[pos[j] + (0,)] = True  # (never redrawn above the bound)
    rounds = 0
    while True:
        bad = window_gap_violations(act32(zc, sc, sh, mask))
        if not bool(bad.any()):
            return z, rounds
        rounds += 1
        assert rounds < 50, "window members could not be separated"
        # redraw the drawn members of the offending windows; planted members are equal among themselves by construction
        redraw = unwindow(bad.unsqueeze(-1).expand(*bad.shape, 4).float(), H, W).bool() & ~planted
        zc[:] = torch.where(redraw, away_from_zero(torch.randn(N, H, W, C, generator=g)), zc)


def dropout_mask(N, C, g, on):
    """Dropout2d multipliers [N, C]: 0 or 1 / (1 - p), p = 0.25; channel 0 (the one with the guaranteed ties and the planted
    zero gates) is never dropped"""
    if not on:
        return None
    m = torch.where(torch.rand(N, C, generator=g) < 0.25, 0.0, 1.0 / 0.75)
    m[:, 0] = 1.0 / 0.75
    return m


def padded_grad(N, H, W, ld, g):
    """a gradient on the reflect-padded domain [N, H+2, W+2, ld]"""
    return torch.randn(N, H + 2, W + 2, ld, generator=g)


def head_inputs(N, S, Co, HW, g, use_dout, use_dloss, use_perm, use_mask):
    """logits with exp(log-parameter) below eps_min, above eps_max and inside (channels Co/2 ...: every third pixel each),
    labels, a 0/1 mask, one permutation per subnetwork."""
    Ct = Co // 2
    out = torch.randn(N, S, Co, HW, generator=g)
    lp = torch.randn(N * S * Ct * HW, generator=g)
    lp[0::3] = -13.0 - torch.rand(lp.numel(), generator=g)[0::3]   # exp < eps_min = 1e-5
    lp[1::3] = 7.5 + torch.rand(lp.numel(), generator=g)[1::3]     # exp > eps_max = 1e3
    out[:, :, Ct:] = lp.view(N, S, Ct, HW)
    return {
        "out": out if use_dloss else None,
        "dout": torch.randn(N, S, Co, HW, generator=g) * 1e-3 if use_dout else None,
        "dloss": (0.5 + torch.rand(S, generator=g)) if use_dloss else None,
        "label": torch.randn(N, Ct, HW, generator=g) if use_dloss else None,
        "mask": (torch.rand(N, HW, generator=g) < 0.8).float() if (use_mask and use_dloss) else None,
        "perm": torch.stack([torch.randperm(N, generator=g) for _ in range(S)]) if (use_perm and use_dloss) else None,
    }


EPS_MIN, EPS_MAX = 1e-5, 1e3


# ---- geometries ------------------------------------------------------------------------------------------------------------

CPS = (8, 24, 64, 256)
BORDER_HW = ((2, 2), (2, 3), (3, 2), (3, 3), (4, 5), (5, 4), (6, 7), (9, 8))
BORDER_N = (1, 3)


def logical_channels(Cp):
    return (Cp, Cp - 3, Cp - 7)


def pool_size(H, W):
    """The pooled tensor is the folded one and needs 2 rows and columns: a listed size below 4 is used as the POOLED size of
    an image of mixed parity (2x2 -> 4x4, 2x3 -> 5x6, 3x2 -> 6x5, 3x3 -> 7x7)."""
    return (H, W) if H >= 4 and W >= 4 else (2 * H + (W & 1), 2 * W + (H & 1))


def fold_pool_geometries():
    """(N, H, W, Cp) of the fold_slice / pool_bwd / BatchNorm cases"""
    out = [(N, H, W, 8) for (H, W) in BORDER_HW for N in BORDER_N]
    out += [(3, 4, 5, Cp) for Cp in CPS[1:]] + [(1, 9, 8, Cp) for Cp in CPS[1:]]
    # PixIter: the per-thread pixel stride exceeds one image / is smaller than one row
    out += [(37, 3, 3, 8), (37, 2, 5, 8), (1, 40, 36, 256)]
    return out


def up_geometries():
    """(N, H, W, h, w, Cp): every low-resolution pixel a border pixel, then one interior case.  H // 2 == h leaves
    padT = (H - 2h) // 2 = 0: an odd size pads the bottom row / right column only (F.pad([d // 2, d - d // 2]))."""
    out = []
    for h in (1, 2, 3, 4):
        for w in (1, 2, 3, 4):
            for H in (2 * h, 2 * h + 1):
                for W in (2 * w, 2 * w + 1):
                    out.append((1 if (h + w) & 1 else 3, H, W, h, w, 8))
    out += [(3, 5, 6, 2, 3, Cp) for Cp in CPS[1:]]
    out += [(1, 24, 21, 12, 10, 8), (2, 24, 21, 12, 10, 64), (37, 3, 2, 1, 1, 8), (1, 80, 73, 40, 36, 256)]
    return out


# One element group past a full grid pass (Cp = 256: 64 channel quads, 4 pixels per 256-thread workgroup, 16 per 1024-thread one):
#   BatchNorm reduce, plain / fold: 448 workgroups x 16 pixels = 7168  -> 1 x 85 x 85 = 7225 pixels (apply: 1792 x 4 = 7168 too)
#   head_bwd: kEwMaxBlocks 1024 x 4 pixels x 4 (unrolled) = 16384      -> 1 x 129 x 128 = 16512 pixels (17 MB)
#   fold_slice: 4096 x 4 = 16384 pixels                                -> 1 x 129 x 128
#   pool_bwd: 8192 x 4 = 32768 windows = 131 k pixels; at Cp = 256 the activations alone are 131 k x 1 KB = 134 MB, above the
#             64 MB limit — the cap is not reached (at Cp = 8, 128 windows per workgroup, it would take 1 M windows = 4 M
#             pixels x 32 B = 134 MB as well).  The pooled BatchNorm sources cap at 256 x 16 / 1024 x 4 cells = 4096:
#             1 x 129 x 127 has 65 x 64 = 4160 cells.
#   up_bwd: 16384 x 4 = 65536 low-resolution pixels, 262 k x 1 KB output gradient = 268 MB — not reached.
PAST_GRID_BN = (1, 85, 85, 256)
PAST_GRID_HEAD = (1, 129, 128, 256)
PAST_GRID_POOLED_BN = (1, 129, 127, 256)


# ---- the cases of the GPU tests (built here so that the CPU test asserts the input properties on the very same draws) -----

def f32(x):
    """the value a C float argument carries"""
    return float(torch.tensor(x, dtype=torch.float32))


def pool_case(N, H, W, Cp, i, prec):
    """activations with planted ties (as the forward forms them: relu(fma) * mask, rounded to the storage type — two members
    that round to one 16-bit value are one more exact tie, decided by scan order on both sides), pooled gradient, skip"""
    g = gen(200 + i)
    C = Cp - 3
    v = bn_vectors(C, Cp, g)
    mask = dropout_mask(N, C, g, True)
    z, _ = pooled_preact(N, H, W, C, Cp, Cp, v, mask, g)
    a = torch.zeros(N, H, W, Cp)
    a[..., :C] = act32(z[..., :C], v["scale"][:C], v["shift"][:C], mask)
    return round_to(a, prec), g


HEAD_MODES = [(True, False), (False, True), (True, True)]  # (dout, dloss)
SRC_NAMES = {GS_PLAIN: ["da"], GS_FOLD: ["dxpad"], GS_POOL: ["dxpad", "skip"],
             GS_HEAD: ["w", "out", "dout", "dloss", "label", "mask"]}


def bn_case(kind, N, H, W, C, Cp, masked, prec="fp32", seed=0, exact=False, variant=0):
    """CPU inputs of one BatchNorm-backward case.  exact: small integers, mean 0, invstd = scale = 1, every gate open, mask of
    ones — every per-channel sum an integer below 2^24."""
    g = gen(1000 + seed)
    v = bn_vectors(C, Cp, g, exact)
    mask = (torch.ones(N, C) if exact else dropout_mask(N, C, g, True)) if masked else None
    ldz = Cp + 8 if kind == GS_PLAIN else Cp
    ints = lambda *shape: torch.randint(-3, 4, shape, generator=g).float()
    if kind == GS_POOL and not exact:
        z, _ = pooled_preact(N, H, W, C, Cp, ldz, v, mask, g)
    else:
        z = preact(N, H, W, C, Cp, ldz, g, plant_zero_gates=not exact)
        if exact:  # (distinct integers inside a window would make the arg-max a matter of the draw: fine, both sides see them)
            z[..., :C] = ints(N, H, W, C)
    src = {"kind_gs": kind}
    rnd = (lambda *s: ints(*s)) if exact else (lambda *s: torch.randn(*s, generator=g))
    if kind == GS_PLAIN:
        src.update(da=rnd(N, H, W, Cp + 4), ldda=Cp + 4)
    elif kind == GS_FOLD:
        src.update(dxpad=rnd(N, H + 2, W + 2, Cp + 8), ldp=Cp + 8)
    elif kind == GS_POOL:
        src.update(dxpad=rnd(N, H // 2 + 2, W // 2 + 2, 8 + Cp + 8), ldp=8 + Cp + 8, choff=8,
                   skip=rnd(N, H + 2, W + 2, 4 + Cp + 4) if variant & 1 else None, ldsk=4 + Cp + 4, skoff=4)
    else:
        use_dout, use_dloss = (True, False) if exact else HEAD_MODES[variant % 3]
        hi = head_inputs(N, 3, 2, H * W, g, use_dout, use_dloss, True, True)
        if exact:
            hi["dout"] = ints(N, 3, 2, H * W)
        src.update(hi, w=rnd(2, C), s=1, kind=(variant // 3) % 2, eps_min=f32(EPS_MIN), eps_max=f32(EPS_MAX))
    for k in ("da", "dxpad", "skip"):
        if src.get(k) is not None:
            src[k] = round_to(src[k], prec)
    z = round_to(z, prec)
    return dict(kind=kind, N=N, H=H, W=W, C=C, Cp=Cp, v=v, mask=mask, z=z, ldz=ldz, src=src, prec=prec)


def bn_geometries(kind):
    geoms = fold_pool_geometries() + [PAST_GRID_POOLED_BN if kind == GS_POOL else PAST_GRID_BN]
    out = []
    for (N, H, W, Cp) in geoms:
        if kind == GS_POOL:
            H, W = pool_size(H, W)
        cs = logical_channels(Cp) if (N, H, W) in ((3, 4, 5), (1, 9, 8)) else (Cp - 3,)
        out += [(N, H, W, C, Cp) for C in cs]
    return out
