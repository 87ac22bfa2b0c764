"""Plain torch references of the forward element-wise operators (mimo_unet_amd/csrc/ew_bn_fwd.hip, ew_resample.hip, ew_dropout.hip, ew_head_loss.hip: the BatchNorm statistics,
BatchNorm + ReLU (+ pooling), max pooling, up-sampling + concat, the 1x1 head, the NLL losses and the layout kernels), the input
generators of their tests and the geometries both test files run: tests/test_ew_fwd_reference_cpu.py proves every function
against the torch modules the model composes in fp64, tests/test_ew_fwd_kernels_gpu.py runs the kernels against them.

Conventions of tests/ew_bwd_reference.py, whose round_to, fold, windows, gate, activation and generators are used, not restated:
dtype-generic functions of the SAME fp32 inputs the kernel sees; decisions (the ReLU gate) taken on the fp64 value; NHWC."""
import math

import numpy as np
import torch

from tests import ew_bwd_reference as E
from tests.ew_bwd_reference import EPS_MAX, EPS_MIN, GAUSSIAN, LAPLACE, f32, gen, round_to  # noqa: F401  (re-exported)

K_COLSUM_MAX_ROWS = 2048   # elementwise.h kColsumMaxRows
STATUS_FWD_STATS, STATUS_LOGITS = 1, 4
ROUTE_PLAN, ROUTE_ONE, ROUTE_ROWSUM = 0, 1, 2


# ---- BatchNorm statistics --------------------------------------------------------------------------------------------------

def exact_colsum(x):
    """column sums of a [rows, C] tensor, correctly rounded to fp64 (math.fsum): the reference carries no summation error"""
    return torch.tensor([math.fsum(col) for col in x.double().t().tolist()], dtype=torch.float64)


def bn_stats(partial, C, count, gamma, beta, rm, rv, momentum, eps, biased=False, drop_row=None):
    """bn_fwd_finalize_channel on the column sums of partial [rows][2][cout_pad], in fp64.  momentum / eps: the fp32 values the
    kernel was handed.  biased / drop_row: the perturbations of the CPU test."""
    p = partial.double()
    if drop_row is not None:
        p = torch.cat([p[:drop_row], p[drop_row + 1:]])
    s1, s2 = exact_colsum(p[:, 0, :C]), exact_colsum(p[:, 1, :C])
    m = s1 / count
    var = (s2 / count - m * m).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    sc = gamma.double() * inv
    unb = var if (biased or count == 1) else var * count / (count - 1.0)
    return {"mean": m, "invstd": inv, "scale": sc, "shift": beta.double() - m * sc,
            "running_mean": (1.0 - momentum) * rm.double() + momentum * m,
            "running_var": (1.0 - momentum) * rv.double() + momentum * unb,
            "msq": s2 / count, "var": var, "abs1": exact_colsum(p[:, 0, :C].abs()) / count}


def bn_eval(gamma, beta, rm, rv, eps):
    inv = 1.0 / torch.sqrt(rv.double() + eps)
    sc = gamma.double() * inv
    return {"mean": rm.double(), "invstd": inv, "scale": sc, "shift": beta.double() - rm.double() * sc}


BN_OUTPUTS = ("mean", "invstd", "scale", "shift", "running_mean", "running_var")


def bn_stats_bound(ref, rows, count, eps, gamma, beta, momentum):
    """Per-channel ABSOLUTE error bounds of the statistics kernels against bn_stats (whose column sums are exact).
    The kernel adds the fp32 partials in fp64: a thread's chain of at most rows / 16 terms, a 16-way fold (one-launch route) or
    chunk chains no longer than that (two-launch route) — at most n = rows / 16 + 32 additions on any path, each within u = 2^-53
    of a partial sum <= sum |term|:  d mean <= n u sum |s1 terms| / count,  d msq <= n u msq (its terms are positive).
    var = msq - mean^2 then carries  d var <= d msq + 2 |mean| d mean + 3 u msq  in ABSOLUTE terms, which is the fp64 error
    amplified by the conditioning msq / var when read relative to var; invstd = (var + eps)^-1/2 moves by
    invstd d var / (2 (var + eps)).  Every output is converted to fp32 once: 2^-24 of the magnitudes of its terms."""
    u, c = 2.0 ** -53, 2.0 ** -24
    n = rows / 16 + 32
    m, inv, sc = ref["mean"].abs(), ref["invstd"], ref["scale"].abs()
    dm = n * u * ref["abs1"]
    dvar = n * u * ref["msq"] + 2 * m * dm + 3 * u * ref["msq"]
    dinv = inv * dvar / (2 * (ref["var"] + eps))
    dsc = gamma.double().abs() * dinv
    unb = count / (count - 1.0) if count > 1 else 1.0
    out = {"mean": c * m + dm, "invstd": c * inv + dinv, "scale": c * sc + dsc,
           "shift": c * (beta.double().abs() + m * sc) + m * dsc + sc * dm,
           "running_mean": c * ref["running_mean"].abs() + momentum * dm,
           "running_var": c * ref["running_var"].abs() + momentum * unb * dvar}
    return {k: v.clamp_min(1e-45) for k, v in out.items()}


def check_stats(name, got, ref, allowed):
    """|got - ref| <= allowed per channel for every BatchNorm output; returns the worst ratio.  (The comparison function of the
    statistics tests: the CPU perturbation tests call it too.)"""
    worst = 0.0
    for k in BN_OUTPUTS:
        if k not in got:
            continue
        g = got[k].detach().cpu().double()
        assert bool(torch.isfinite(g).all()), (name, k, "not finite / unwritten")
        ratio = float(((g - ref[k]).abs() / allowed[k]).max())
        assert ratio <= 1.0, (name, k, ratio)
        worst = max(worst, ratio)
    return worst


def one_ulp(ref):
    """{name: one fp32 ulp of the rounded reference}: the bound of the integer-partials test"""
    return {k: E.ulp_of(ref[k].float()).double() for k in BN_OUTPUTS if k in ref}


# ---- pooling / BatchNorm + ReLU ----------------------------------------------------------------------------------------------

def maxpool(a):
    """MaxPool2d(2), floor: [N, H, W, C] -> [N, H//2, W//2, C]"""
    return E.windows(a).max(-1).values


def pre_activation(z, scale, shift):
    return z.double() * scale.double() + shift.double()


# ---- bilinear x2 align_corners up-sampling -----------------------------------------------------------------------------------

def lerp_src32(dst, n_in, n_out, clamp_i1=True):
    """lerp_src of ew_device.h restated in fp32 (numpy scalars round every operation; scale * dst is a separate, rounded
    product as the kernel pins it): (i0, i1, l0, l1)"""
    one = np.float32(1.0)
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    src = np.float32(scale * np.float32(dst))
    i0 = min(int(src), n_in - 1)
    l1 = np.float32(min(max(np.float32(src - np.float32(i0)), np.float32(0.0)), one))
    l0 = np.float32(one - l1)
    i1 = i0 + (1 if (i0 < n_in - 1 or not clamp_i1) else 0)
    return i0, i1, float(l0), float(l1)


def lerp_matrix32(n_in, dtype=torch.float64, clamp_i1=True):
    """[2 n_in, n_in (+ 1 without the clamp)] interpolation matrix whose entries are lerp_src32's fp32 weights"""
    M = torch.zeros(2 * n_in, n_in + (0 if clamp_i1 else 1), dtype=dtype)
    for o in range(2 * n_in):
        i0, i1, l0, l1 = lerp_src32(o, n_in, 2 * n_in, clamp_i1)
        M[o, i0] += l0
        M[o, i1] += l1
    return M


def upsample(low, vertical_first=False, clamp_i1=True):
    """[N, h, w, C] -> [N, 2h, 2w, C]: horizontal pairs first, then the vertical pair (the kernels' association)"""
    My, Mx = lerp_matrix32(low.shape[1], low.dtype, clamp_i1), lerp_matrix32(low.shape[2], low.dtype)
    if not clamp_i1:  # the perturbation: i1 = h reads the row after the last one — not the tensor's; its weight is 0, 0 x inf = NaN
        low = torch.cat([low, torch.full_like(low[:, -1:], float("inf"))], 1)
    if vertical_first:
        return torch.einsum("qp,nopc->noqc", Mx, torch.einsum("oi,nipc->nopc", My, low))
    return torch.einsum("oi,niqc->noqc", My, torch.einsum("qp,nipc->niqc", Mx, low))


def upsample_cat(skip, low, H, W, lo_scale=None, lo_shift=None, **kw):
    """cat(skip, zero_pad(upsample(low))) at H x W (F.pad([d // 2, d - d // 2])); lo_scale: low is a pre-activation"""
    if lo_scale is not None:
        low = E.activation(low, lo_scale, lo_shift)
    up = upsample(low, **kw)
    N, h2, w2, C = up.shape
    pt, pl = (H - h2) // 2, (W - w2) // 2
    out = up.new_zeros(N, H, W, C)
    out[:, pt:pt + h2, pl:pl + w2] = up
    return out if skip is None else torch.cat([skip, out], -1)


# ---- head and loss -----------------------------------------------------------------------------------------------------------

def head(a, w, bias, in_scale=None, in_shift=None):
    """a [N, HW, C], w [Co, C], bias [Co] -> logits [N, Co, HW]"""
    if in_scale is not None:
        a = E.activation(a[:, None], in_scale, in_shift)[:, 0]
    return torch.einsum("npc,oc->nop", a, w) + bias[None, :, None]


def nll_value(kind, d, lp, eps_min, eps_max):
    sc = torch.exp(lp).clamp(eps_min, eps_max)
    return torch.log(sc) + (d.abs() if kind == LAPLACE else d * d) / sc


def loss_terms(out, label, mask, perm, kind, eps_min, eps_max, perm_on_output=False):
    """the un-reduced masked NLL [S, N, Ct, HW] of out [N, S, Co, HW]; image n of subnetwork s carries the label (and mask) of
    image perm[s][n]"""
    N, S, Co, HW = out.shape
    Ct = Co // 2
    rows = []
    for s in range(S):
        src = perm[s] if perm is not None else torch.arange(N)
        o = out[:, s]
        if perm_on_output:  # the perturbation: the permutation applied to the wrong side
            v = nll_value(kind, o[src, :Ct] - label, o[src, Ct:], eps_min, eps_max)
            v = v if mask is None else v * mask[:, None, :]
        else:
            v = nll_value(kind, o[:, :Ct] - label[src], o[:, Ct:], eps_min, eps_max)
            v = v if mask is None else v * mask[src][:, None, :]
        rows.append(v)
    return torch.stack(rows)


def loss(out, label, mask, perm, kind, eps_min, eps_max, **kw):
    t = loss_terms(out, label, mask, perm, kind, eps_min, eps_max, **kw)
    return t.reshape(t.shape[0], -1).mean(1)


def loss_absterm(out, label, mask, perm, kind, eps_min, eps_max):
    """[S, count]: |log sc| + |d|^k / sc (x mask) per element — the magnitude of what a thread adds"""
    Ct = out.shape[2] // 2
    terms = loss_terms(out, label, mask, perm, kind, eps_min, eps_max)
    logpart = loss_terms(torch.cat([out[:, :, :Ct] * 0, out[:, :, Ct:]], 2), label * 0, mask, perm, kind, eps_min, eps_max)
    return (logpart.abs() + (terms - logpart).abs()).reshape(out.shape[1], -1)


def loss_k(total):
    """rounding-error factor of one subnetwork's sum (loss_fwd_kernel / loss_finalize_kernel): each thread adds its n_t terms in
    sequence in fp32, a 256-way fp32 tree adds 8 levels, the <= 512 workgroup sums are added in fp64 and converted once;
    a term carries about 8 roundings (difference, expf and logf at 2 ulp each, clamp, quotient, sum, mask)."""
    blocks = max(1, min(-(-total // 256), 512))
    return -(-total // (blocks * 256)) + 8 + 8 + 2


# ---- layout ------------------------------------------------------------------------------------------------------------------

def pack_input(x, perm, s, cp):
    """x [N, S, C, H, W] -> [N, H, W, cp]: image perm[s][n] of subnetwork s, zero padding channels"""
    N, S, C, H, W = x.shape
    src = perm[s] if perm is not None else torch.arange(N)
    out = x.new_zeros(N, H, W, cp)
    out[..., :C] = x[src, s].permute(0, 2, 3, 1)
    return out


def unpack_dx(dxpad, C):
    """fold(dxpad)[..., :C] as [N, C, H, W]"""
    return E.fold(dxpad)[..., :C].permute(0, 3, 1, 2).contiguous()


# ---- inputs and cases ----------------------------------------------------------------------------------------------------------

def junk(*shape, g):
    """finite non-zero junk for padding channels"""
    return 3.0 + torch.rand(*shape, generator=g)


def partial_rows(rows, C, cout_pad, g, kind="random"):
    """[rows][2][cout_pad] partial sums; columns >= C hold junk (never read).  integer: |value| < 2^12.  random: per-row sums of
    64 samples of a channel with mean mu_c and std sd_c; channel 1: mean 1e3, std 1e-2 (conditioning ~ 1e10); channel 2 constant."""
    p = junk(rows, 2, cout_pad, g=g)
    if kind == "integer":
        p[:, 0, :C] = torch.randint(-31, 32, (rows, C), generator=g).float()      # count = rows: |mean| <= 31, mean^2 <= 961
        p[:, 1, :C] = torch.randint(1024, 4096, (rows, C), generator=g).float()  # msq >= 1024: a positive variance
        return p
    mu = torch.randn(C, generator=g)
    sd = 0.5 + torch.rand(C, generator=g)
    if C > 1:
        mu[1], sd[1] = 1e3, 1e-2
    x = mu + sd * torch.randn(rows, 64, C, generator=g)
    if C > 2:
        x[..., 2] = 0.75  # a constant channel: s2 / count - mean^2 is exactly 0 (0.75, 0.5625 and their multiples are exact)
    p[:, 0, :C] = x.double().sum(1).float()
    p[:, 1, :C] = (x.double() ** 2).sum(1).float()
    if C > 2:
        p[:, 0, 2], p[:, 1, 2] = 0.75 * 64, 0.5625 * 64
    return p


BN_ROWS_ONE = (1, 15, 16, 17, 63, 64, 65, 127, K_COLSUM_MAX_ROWS)
BN_ROWS_TWO = (33, 2047, 2049, 64 * 32 + 1, 4097)
BN_CHANNELS = ((5, 8, 16), (70, 72, 96), (21, 24, 32))  # (c, c_p, cout_pad): c < c_p < cout_pad; 72 > 64: a second workgroup

WIDEST_CP = 960  # 8 x filter_base_count 30 x 4 subnetworks, the widest double convolution of bench.py's configurations
# (N, H, W, C, Cp).  Threads of a 256-thread workgroup: QB = min(Cp / 4, 256) channel quads x PPI = 256 // QB pixels (pixquad).
#   (37, 3, 3, 5, 8)        QB 2, PPI 128: one workgroup spans 14 images (a thread's FIRST pixel lies in a later image)
#   (3, 5, 4, 21, 24)       QB 6, PPI 42: 4 idle threads per workgroup; odd H
#   (2, 9, 8, 64, 64)       QB 16; c == c_p
#   (3, 4, 5, 35, 40)       QB 10, PPI 25: 6 idle threads; odd W
#   (1, 85, 85, 253, 256)   QB 64, PPI 4: 7225 pixels > 1536 x 4 — bn_relu_fwd_kernel's threads take a second pixel; odd H and W
#   (1, 4, 5, 957, 960)     QB 240, PPI 1, 16 idle threads: the widest c_p; with a 960-channel skip the concat has 480 quads: gridDim.y 2
PIXEL_GEOMETRIES = [(37, 3, 3, 5, 8), (3, 5, 4, 21, 24), (2, 9, 8, 64, 64), (3, 4, 5, 35, 40), (1, 85, 85, 253, 256),
                    (1, 4, 5, 957, WIDEST_CP)]
# The kernels that walk pixels with pix_iter / pix_next (bn_relu_pool_fwd, maxpool_fwd, upcat_fwd, upcat_fwd2x2) launch at most 4096
# workgroups: a thread takes a SECOND pixel, and pix_next's result is used, only beyond 4096 x PPI units.  The smallest such shape:
# PPI = 1 needs more than 128 channel quads (c_p 520: QB 130), then 460 images of 6 x 6:
#   pooled / 2x2-block kernels: 460 x 3 x 3 = 4140 units > 4096; stride 4096 = 455 images + 1 unit: dn = 455, dx = 1, so the
#     column carry, the row carry and the image step of pix_next all occur among the 44 threads that go round again
#   per-pixel upcat_fwd (with the 8-channel skip: 132 quads, PPI 1): 460 x 36 = 16560 pixels, four rounds; stride 4096 = 113
#     images + 28 pixels: dn = 113, dy = 4, dx = 4
PAST_GRID_POOLED = (460, 6, 6, 517, 520)
#   (37, 5, 5, 5, 8)        pooled 2 x 2 of an odd size, a workgroup spans images
#   (2, 7, 6, 13, 16), (2, 6, 7, 13, 16)   one odd direction each: the last-row / last-column branch alone (and not the corner)
#   (1, 2, 2, 5, 8)         pooled to 1 x 1
POOL_GEOMETRIES = PIXEL_GEOMETRIES + [(37, 5, 5, 5, 8), (2, 7, 6, 13, 16), (2, 6, 7, 13, 16), (1, 2, 2, 5, 8), PAST_GRID_POOLED]


def up_geometries():
    """(N, hs, ws, hl, wl, C, Cp): every pooled geometry up-sampled back (hs == 2 hl: the 2x2-block kernel when the skip is in
    place, the per-pixel kernel with a skip — PAST_GRID_POOLED takes both beyond their capped grids); then a skip larger by an
    odd amount (2 hl + 1, 2 wl + 3: asymmetric zero padding, per-pixel kernel either way) and hl = 1 / wl = 1 / both (scale = 0 in
    lerp_src)"""
    out = [(N, 2 * (H // 2), 2 * (W // 2), H // 2, W // 2, C, Cp) for (N, H, W, C, Cp) in POOL_GEOMETRIES]
    out += [(2, 2 * 3 + 1, 2 * 4 + 3, 3, 4, 13, 16), (3, 2, 6, 1, 3, 5, 8), (3, 6, 2, 3, 1, 5, 8), (2, 3, 5, 1, 1, 5, 8)]
    return out


def bn_vectors(C, Cp, g):
    """scale / shift [Cp] with zero padding channels (the contract of the statistics kernels)"""
    v = E.bn_vectors(C, Cp, g)
    return v["scale"], v["shift"]


def separated_preact(N, H, W, C, Cp, ldz, scale, shift, mask, g, prec="fp32", pooled=True):
    """z [N, H, W, ldz] (junk in the padding channels and beyond) whose pre-activations stay clear of 0 by more than the
    per-element bound (|fma| >= 2^-10 (|z scale| + |shift|), far above 16 ulp) and whose 2x2 windows hold activations that are
    exactly equal or more than 4 ulp apart: offenders are redrawn, none is excluded.  Returns z rounded to the storage type."""
    z = junk(N, H, W, ldz, g=g)
    zc = round_to(E.away_from_zero(torch.randn(N, H, W, C, generator=g)), prec)
    sc, sh = scale[:C], shift[:C]
    for _ in range(50):
        pre = pre_activation(zc, sc, sh)
        bad = pre.abs() < 2.0 ** -10 * ((zc.double() * sc.double()).abs() + sh.double().abs())
        if pooled and H >= 2 and W >= 2:
            gap = E.window_gap_violations(E.act32(zc, sc, sh, mask))
            bad |= E.unwindow(gap.unsqueeze(-1).expand(*gap.shape, 4).float(), H, W).bool()
        if not bool(bad.any()):
            z[..., :C] = zc
            return z
        zc = torch.where(bad, round_to(E.away_from_zero(torch.randn(N, H, W, C, generator=g)), prec), zc)
    raise AssertionError("pre-activations could not be separated")


def bn_relu_case(i, geom, prec, masked, pooled=True):
    N, H, W, C, Cp = geom
    g = gen(4000 + i)
    scale, shift = bn_vectors(C, Cp, g)
    mask = E.dropout_mask(N, C, g, masked)
    ldz = Cp + 8
    z = separated_preact(N, H, W, C, Cp, ldz, scale, shift, mask, g, prec, pooled)
    return dict(N=N, H=H, W=W, C=C, Cp=Cp, scale=scale, shift=shift, mask=mask, z=z, ldz=ldz, lda=Cp + 4, ldpool=Cp + 12)


def pool_input(i, geom, prec):
    """activations for the stand-alone pooling test: random signs, junk beyond Cp; rounded to storage"""
    N, H, W, C, Cp = geom
    g = gen(5000 + i)
    a = junk(N, H, W, Cp + 4, g=g)
    a[..., :Cp] = torch.randn(N, H, W, Cp, generator=g)
    return round_to(a, prec)


def up_case(i, geom, prec, fused):
    N, hs, ws, hl, wl, C, Cp = geom
    g = gen(6000 + i)
    scale, shift = bn_vectors(C, Cp, g)
    ldl = Cp + 4
    low = separated_preact(N, hl, wl, C, Cp, ldl, scale, shift, None, g, prec, pooled=False)
    csp = Cp if Cp == WIDEST_CP else 8  # (the widest concat buffer: more channel quads than one workgroup column)
    skip = round_to(junk(N, hs, ws, csp + 4, g=g) - 3.5, prec)
    return dict(N=N, hs=hs, ws=ws, hl=hl, wl=wl, C=C, Cp=Cp, csp=csp, lds=csp + 4, ldl=ldl, low=round_to(low, prec), skip=skip,
                scale=scale, shift=shift)


HEAD_C = (5, 8, 13, 21, 61, 100, 253)
HEAD_G = {5: 2, 8: 2, 13: 4, 21: 8, 61: 16, 100: 32, 253: 64}


def head_cases():
    """(C, Co, S, N, HW): every G with every Co once; hw 1 / 7 / 1441; one n hw = (256 / G) 4 blocks + 1"""
    out = []
    for i, C in enumerate(HEAD_C):
        for j, Co in enumerate((2, 4, 8)):
            out.append((C, Co, (1, 3)[(i + j) % 2], (3, 2, 1)[(i + j) % 3], (1, 7, 1441)[(i + j) % 3]))
    out.append((21, 2, 3, 1, (256 // 8) * 4 * 3 + 1))
    out.append((253, 8, 1, 1, (256 // 64) * 4 * 2 + 1))
    return out


def head_case(i, C, Co, N, HW, prec, fused):
    g = gen(7000 + i)
    Cp = -(-C // 8) * 8
    scale, shift = bn_vectors(C, Cp, g)
    lda = Cp + 8
    if fused:
        a = separated_preact(N, 1, HW, C, Cp, lda, scale, shift, None, g, prec, pooled=False)
    else:
        a = junk(N, 1, HW, lda, g=g)
        a[..., :C] = torch.randn(N, 1, HW, C, generator=g)
    return dict(a=round_to(a, prec).reshape(N, HW, lda), lda=lda, Cp=Cp, w=torch.randn(Co, C, generator=g), bias=torch.randn(Co, generator=g),
                scale=scale, shift=shift)


LOSS_SIZES = ((1, 1), (3, 85), (1, 257), (3, 43691))  # (N, HW): N HW = 1, 255, 257 and 131073 = one past 512 x 256


def loss_case(i, N, HW, Co, S, use_mask, use_perm):
    g = gen(8000 + i)
    hi = E.head_inputs(N, S, Co, HW, g, False, True, use_perm, use_mask)
    return hi["out"], hi["label"], hi["mask"], hi["perm"]


def exact_loss_case(N, HW, S):
    """Inputs whose every term is an integer for BOTH kinds, run with eps_min = eps_max = 1: the clamp makes sc == 1 whatever
    the last bits of the device's expf are, logf(1) == 0 exactly, and the term is |d| or d^2 with d an integer, |d| <= 16.
    Sums stay below 2^24, so every fp32 addition is exact in any order."""
    g = gen(8100)
    out = torch.zeros(N, S, 2, HW)
    out[:, :, 0] = torch.randint(-8, 9, (N, S, HW), generator=g).float()
    out[:, :, 1] = torch.randint(-3, 4, (N, S, HW), generator=g).float()
    label = torch.randint(-8, 9, (N, 1, HW), generator=g).float()
    return out, label


PACK_C = (1, 3, 4)
FOLD_HW = ((2, 2), (3, 3), (3, 7), (16, 16))
