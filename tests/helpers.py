"""Shared helpers for the parity tests (test infrastructure)."""
import os

import numpy as np
import torch

from oracle import mimo_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_npz(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def state_from(fx, prefix):
    return {k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in fx.items() if k.startswith(prefix)}


def cfg_from_meta(meta):
    Ci, Co, S, f = (int(v) for v in meta[:4])
    return O.NetConfig(in_channels=Ci, out_channels=Co, num_subnetworks=S, filter_base_count=f)


def rel_err(a, b):
    """max |a-b| / max(|b|) — error relative to the tensor's scale (the fp32
    tolerance the north_star states is 1e-3 on this measure)."""
    a = torch.as_tensor(a, dtype=torch.float64).flatten()
    b = torch.as_tensor(b, dtype=torch.float64).flatten()
    denom = max(float(b.abs().max()), 1e-30)
    return float((a - b).abs().max()) / denom


def rms_rel_err(a, b):
    a = torch.as_tensor(a, dtype=torch.float64).flatten()
    b = torch.as_tensor(b, dtype=torch.float64).flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


AMP_CASES = [("amp_cfg1.npz", "cfg1_step.npz"), ("amp_mini_s2.npz", "mini_s2_step.npz")]
AMP_TAG = {"bf16-mixed": "bf16", "16-mixed": "fp16"}  # precision mode -> prefix inside tests/golden/amp_*.npz


def is_prebn_bias(name):
    """conv bias in front of a BatchNorm: mathematically zero gradient, pure rounding noise on both sides"""
    return "double_conv" in name and name.endswith((".0.bias", ".3.bias"))


def grads_rel_l2(a, b):
    """whole-gradient relative L2 distance sqrt(sum |a-b|^2 / sum |b|^2) over every parameter but the pre-BatchNorm biases"""
    num = den = 0.0
    for k, gb in b.items():
        if is_prebn_bias(k):
            continue
        x, y = torch.as_tensor(a[k]).double(), torch.as_tensor(gb).double()
        num, den = num + float(((x - y) ** 2).sum()), den + float((y ** 2).sum())
    return (num / den) ** 0.5


def amp_reference(amp_name, src_name, mode):
    """One training step of the REFERENCE under torch.autocast (tests/golden/amp_*.npz, make_golden.py::amp_fixture) next
    to the same step of the reference in fp32 (the fixture it was derived from): inputs, both sets of results, and
    `d` = how far the reference's own mixed-precision result sits from its fp32 result on each quantity — the yardstick
    the mixed-precision tolerances are stated in."""
    amp, fx = load_npz(amp_name), load_npz(src_name)
    tag = AMP_TAG[mode]
    sub = lambda pre: {k[len(pre):]: torch.from_numpy(v) for k, v in amp.items() if k.startswith(pre)}
    g16 = sub(f"{tag}/grad/")
    g32 = {k[len("s0/grad/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("s0/grad/")}
    r = {"fx": fx, "cfg": cfg_from_meta(fx["meta"]), "scale": float(amp[f"{tag}/loss_scale"]),
         "image": torch.from_numpy(fx["s0/image"]), "label": torch.from_numpy(fx["s0/label"]),
         "perms": torch.from_numpy(fx["s0/perms"]), "mask": torch.from_numpy(fx["s0/mask"]) if "s0/mask" in fx else None,
         "out16": torch.from_numpy(amp[f"{tag}/out"]), "out32": torch.from_numpy(fx["s0/out"]),
         "eval16": torch.from_numpy(amp[f"{tag}/out_eval"]), "loss16": torch.from_numpy(amp[f"{tag}/loss"]),
         "loss32": torch.from_numpy(fx["s0/loss"]), "total16": float(amp[f"{tag}/total"]), "grads16": g16, "grads32": g32,
         "dx16": torch.from_numpy(amp[f"{tag}/dx"]), "dx32": torch.from_numpy(fx["s0/dx"]), "after16": sub(f"{tag}/after/")}
    r["d_out"] = rel_err(r["out16"], r["out32"])
    r["d_grads"] = grads_rel_l2(g16, g32)
    r["d_dx"] = rel_err(r["dx16"], r["dx32"])
    return r


# Final parameters after a few Adam steps: Adam turns rounding-level gradient differences into sign-level update
# differences, so |ours - reference| per element is bounded by 2 * steps * lr ("budget", two runs with opposite signs), and
# its rms over a tensor measures how many elements flipped.  The reference's OWN fp32 rounding already moves that
# statistic: the oracle run in fp64 against the fp32 fixtures gives rms / budget = 0.121 on cfg1's worst tensor, 0.019 on
# mini_s2's, 0.161 on mini_gauss's (tests/test_oracle_golden.py::test_adam_sign_flip_statistic_of_the_reference_itself pins
# those).  A bound below that would test luck, not parity; one far above it would hide a regression: per
# fixture, ~1.5x the reference's own statistic with a floor for the near-exact fixture — for tensors with >= 256 elements
# (fewer: rms ~ max, one flip).
ADAM_FLIP_RMS = {"cfg1_step.npz": 0.2, "mini_s2_step.npz": 0.08, "mini_gauss_step.npz": 0.25}
# ARITHMETIC-SPECIFIC bounds (DESIGN.md section 4 lists them): split16 since round 5 multiplies the activation of the weight
# gradient as ONE fp16 value (2^-12 per element; dz keeps an fp16 pair; MIMO_WGRAD_NP=3 restores three bf16-pair MFMAs) —
# weight gradients carry 1-4e-4 of their scale in rounding noise instead of 1e-5, so more near-zero gradient elements change
# sign under Adam.  Derived like the fp32 table: ~1.5 x what that arithmetic was observed to do on each fixture
# (profiles/r05/parity_errors.txt: cfg1 0.130, mini_s2 0.126, mini_gauss 0.040), never below the fp32 table's entry.
ADAM_FLIP_RMS_NP2 = {"cfg1_step.npz": 0.2, "mini_s2_step.npz": 0.19, "mini_gauss_step.npz": 0.25}


def wgrad_two_mfma(precision):
    """the plan runs the weight gradient on two fp16 MFMAs per product (the split16 default since round 5)"""
    import os
    return precision == "split16" and os.environ.get("MIMO_WGRAD_NP") != "3"


def adam_flip_bound(fixture, precision):
    return max(ADAM_FLIP_RMS[fixture], ADAM_FLIP_RMS_NP2[fixture]) if wgrad_two_mfma(precision) else ADAM_FLIP_RMS[fixture]


# Per-tensor gradient error against the reference goldens (max |ours - ref| / max |ref|).  The north_star's tolerance is
# 1e-3; the golden checks fail EARLIER, at ~1.3 x what each arithmetic was observed to do, so that the next precision trade
# cannot slide in under the headline tolerance: fp32-MFMA mode observed <= 1.7e-4, three-MFMA split16
# <= 3.6e-4 (a BatchNorm weight gradient of cfg1: the bf16-pair data gradient upstream of it), two-MFMA split16 <= 6.2e-4
# (profiles/r05/parity_errors.txt, profiles/r06/parity_errors.txt).
GOLDEN_GRAD_TOL = {"fp32": 3e-4, "split16-np3": 5e-4, "split16": 8e-4}


def golden_grad_tol(precision):
    if precision == "split16":
        return GOLDEN_GRAD_TOL["split16" if wgrad_two_mfma(precision) else "split16-np3"]
    return GOLDEN_GRAD_TOL.get(precision, 1e-3)


def adam_flip_statistic(ours, ref, budget):
    """rms(|ours - ref|) / budget of one parameter tensor (numpy arrays)"""
    d = np.abs(np.asarray(ours, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float(np.sqrt((d ** 2).mean())) / budget


def free_port():
    """A TCP port that is free right now on 127.0.0.1 (rendezvous of the multi-process tests)."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def report(*parts):
    """Print an observed-error line and, when MIMO_PARITY_LOG names a file, append it there (the GPU run's
    parity_errors.txt that is committed under profiles/)."""
    msg = " ".join(str(p) for p in parts)
    print(msg)
    path = os.environ.get("MIMO_PARITY_LOG")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as fh:
            fh.write(f"{test}: {msg}\n")


# ---- 3 x 3 convolutions: the benchmark's layer table, an fp64 reference, the comparison rules of the operator tests ----

# resolution level (256 >> level) of each DoubleConv, by state_dict prefix (model.py:119-297: four 2x2 poolings down, four
# 2x up-samplings back)
_DOUBLE_CONV_LEVEL = {"encoder.in_convs": 0, "encoder.down1s": 1, "core.down2": 2, "core.down3": 3, "core.down4": 4,
                      "core.up1": 3, "core.up2": 2, "core.up3": 1, "decoder.up4s": 0}
BENCH_GPU_COUNTS = (1, 2, 4, 8)  # strong scaling: the config's batch is the global batch, sharded over 1 / 2 / 4 / 8 GPUs


def pad8(c):
    return (c + 7) // 8 * 8


def conv_cin_pad(c):
    """padded input channels of a convolution as the plan stores them: 4-channel pixels for the image (<= 4 channels),
    8-channel units otherwise"""
    return (c + 3) // 4 * 4 if c <= 4 else pad8(c)


def config_conv_layers(c, n):
    """(N, H, W, Cin, Cout) of every 3 x 3 convolution of bench.CONFIGS entry `c` at `n` images per GPU, distinct"""
    cfg = O.NetConfig(in_channels=c["Ci"], out_channels=c["Co"], num_subnetworks=c["S"], filter_base_count=c["f"])
    out = []
    for prefix, cin, cmid, cout in O.double_conv_specs(cfg):
        level = next(v for k, v in _DOUBLE_CONV_LEVEL.items() if prefix.startswith(k + "."))
        h, w = c["H"] >> level, c["W"] >> level
        for t in ((n, h, w, cin, cmid), (n, h, w, cmid, cout)):
            if t not in out:
                out.append(t)
    return out


def benchmark_shards(c):
    """per-GPU batches bench.py runs config `c` at: its batch, and its strong-scaling shards at 2, 4 and 8 GPUs"""
    return [c["batch"] // g for g in BENCH_GPU_COUNTS]


def benchmark_conv_layers():
    """The distinct (N, H, W, Cin, Cout) of every 3 x 3 convolution the benchmark runs: every config of bench.CONFIGS
    at every per-GPU batch of benchmark_shards, in a fixed order (config, batch, forward order of the layers)."""
    import bench
    out = []
    for c in bench.CONFIGS.values():
        for n in benchmark_shards(c):
            out += [t for t in config_conv_layers(c, n) if t not in out]
    return out


_WGRAD_PROBE = None
WGRAD_RECIPE_FIELDS = ("splits", "ci", "co", "ws", "np2", "tiles", "reduce_blocks", "store", "thin")


def wgrad_probe():
    """libmimo_plan_probe.so (the library's test-only twin, tests/host/plan_probe.hip) with its two host-only entry points
    mimo_test_wgrad_recipe and mimo_test_wg_side_cus"""
    global _WGRAD_PROBE
    if _WGRAD_PROBE is None:
        import ctypes as C
        from mimo_unet_amd import _lib as L
        lib = C.CDLL(os.path.join(os.path.dirname(L.LIB_PATH), "libmimo_plan_probe.so"))
        lib.mimo_test_wgrad_recipe.restype = C.c_int
        lib.mimo_test_wgrad_recipe.argtypes = [C.c_int32] * 9 + [C.POINTER(C.c_int32)]
        lib.mimo_test_wg_side_cus.restype = C.c_int
        lib.mimo_test_wg_side_cus.argtypes = [C.c_int64, C.c_int32]
        _WGRAD_PROBE = lib
    return _WGRAD_PROBE


def wgrad_recipe(precision, layer, wg_cus=0):
    """The weight-gradient launch the library's own conv_recipe makes for layer (N, H, W, Cin, Cout) in `precision` (a key
    of _lib.PRECISIONS; not fp32) at `wg_cus` CUs — 0: at what mimo_op_conv3x3_wgrad runs right now (MIMO_WGRAD_CUS, else
    256) — as a dict of WGRAD_RECIPE_FIELDS; MIMO_WGRAD_NP and the other switches are read as the library reads them."""
    import ctypes as C
    from mimo_unet_amd import _lib as L
    N, H, W, Ci, Co = layer
    out = (C.c_int32 * len(WGRAD_RECIPE_FIELDS))()
    rc = wgrad_probe().mimo_test_wgrad_recipe(L.PRECISIONS[precision], N, H, W, Ci, conv_cin_pad(Ci), Co, pad8(Co), wg_cus, out)
    assert rc == 0, (precision, layer, wg_cus, rc)
    return dict(zip(WGRAD_RECIPE_FIELDS, out))


def plan_wgrad_cus(layer):
    """The distinct CU counts (sched::wg_side_cus) the benchmark's plans size their weight-gradient launches for, over every
    (config, per-GPU batch) of bench.CONFIGS / benchmark_shards whose plan contains `layer`, ascending"""
    import bench
    cus = set()
    for c in bench.CONFIGS.values():
        for n in benchmark_shards(c):
            if layer in config_conv_layers(c, n):
                cus.add(int(wgrad_probe().mimo_test_wg_side_cus(n * c["H"] * c["W"], c["S"] * c["f"])))
    return sorted(cus)


def conv3x3_reference_f64(x, w, b, dz, chunk_elems=1 << 26):
    """Reference of one 3 x 3 reflect-padded convolution (components.py:23,26) in float64, on the inputs' device.

    x [N, H, W, >= Cin] and dz [N, H, W, >= Cout] are NHWC (channels past w's are ignored), w [Cout, Cin, 3, 3], b [Cout].
    Returns float64 z [N, H, W, Cout], dx [N, H, W, Cin], dw, db and the per-channel sums of z and z^2 ("sum", "sumsq").
    The convolution is nine shifted matmuls, one per tap; autograd gives the backward, including the fold of the reflect
    border.  Images are processed in chunks of about `chunk_elems` input / output elements (the sums are accumulated in
    float64 across chunks)."""
    import torch.nn.functional as F
    Co, Ci = w.shape[:2]
    N, H, W = x.shape[:3]
    per_image = H * W * max(Ci, Co)
    step = max(1, chunk_elems // per_image)
    wt = w.detach().double().requires_grad_(True)
    bt = b.detach().double().requires_grad_(True)
    zs, dxs = [], []
    for n0 in range(0, N, step):
        xc = x[n0:n0 + step, ..., :Ci].double().requires_grad_(True)
        xp = F.pad(xc.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1)
        z = bt
        for ky in range(3):
            for kx in range(3):
                z = z + xp[:, ky:ky + H, kx:kx + W, :] @ wt[:, :, ky, kx].t()
        z.backward(dz[n0:n0 + step, ..., :Co].double())
        zs.append(z.detach())
        dxs.append(xc.grad)
    z = torch.cat(zs)
    return {"z": z, "dx": torch.cat(dxs), "dw": wt.grad, "db": bt.grad, "sum": z.sum(dim=(0, 1, 2)),
            "sumsq": (z * z).sum(dim=(0, 1, 2))}


def worst_at(a, b):
    """index (as a tuple) of the largest |a - b|"""
    d = (torch.as_tensor(a, dtype=torch.float64) - torch.as_tensor(b, dtype=torch.float64)).abs()
    return tuple(int(i) for i in np.unravel_index(int(d.argmax()), tuple(d.shape)))


def err_where(a, b):
    """rel_err(a, b) and worst_at(a, b) from one difference"""
    b = torch.as_tensor(b, dtype=torch.float64)
    d = (torch.as_tensor(a, dtype=torch.float64) - b).abs()
    i = int(d.argmax())
    return float(d.flatten()[i]) / max(float(b.abs().max()), 1e-30), tuple(int(k) for k in np.unravel_index(i, tuple(d.shape)))


def conv_tolerances(precision):
    """Per-quantity bounds (max |ours - ref| / max |ref|) of the 3 x 3 convolution operators against a reference of the
    same operation on the same (unrounded) operands; the derivations are in test_ops_gpu.py::test_conv3x3_forward_dgrad_wgrad.
    fp32: accumulation order only.  split16: fp16 / bf16 hi-lo pairs; the two-MFMA weight gradient (one fp16 activation)
    5e-4.  bf16: operands rounded to bf16.  The bias gradient is an fp32 column sum in every mode; the statistics are sums
    of the outputs."""
    tol = {"fp32": 2e-5, "split16": 1e-4, "bf16": 2e-2}[precision]
    stat = 2e-2 if precision == "bf16" else 2e-5
    return {"fwd": tol, "dgrad": tol, "wgrad": 5e-4 if wgrad_two_mfma(precision) else tol, "bgrad": 2e-5, "sum": stat,
            "sumsq": stat}


# quantity -> (key of conv3x3_reference_f64's result, key of the kernel outputs), as check_conv_results compares them
_CONV_QUANTITIES = {"fwd": ("z", "z"), "dgrad": ("dx", "dx"), "wgrad": ("dw", "dw"), "bgrad": ("db", "db"),
                    "sum": ("sum", "stats0"), "sumsq": ("sumsq", "stats1")}


def conv_outputs(z, stats, dx, dw, db, Ci, Co):
    """the kernel results of one forward / data gradient / weight gradient as check_conv_results takes them (any of them
    may be None when that operator was not run)"""
    out = {}
    if z is not None:
        out.update(z_full=z, z=z[..., :Co], stats0=stats[0], stats1=stats[1])
    if dx is not None:
        out.update(dx_full=dx, dx=dx[..., :Ci])
    if dw is not None:
        out.update(dw=dw, db=db)
    return out


def check_conv_results(got, ref, precision, label, tols=None):
    """Compare the outputs of mimo_op_conv3x3_forward / _dgrad / _wgrad (conv_outputs; the output buffers were filled with
    NaN before the calls) with a reference of the same operation (the keys of conv3x3_reference_f64).  Asserts that every
    output was fully overwritten, that the padding channels of z are exactly zero, and the per-quantity bounds
    (conv_tolerances(precision), or `tols`).  The errors and the index of each quantity's worst element — (image, row,
    column, channel) of z / dx, (cout, cin, ky, kx) of dW, the channel of db and of the sums — go through report() after
    `label` (a tuple); they are also returned."""
    tols = tols or conv_tolerances(precision)
    if "z_full" in got:
        Co = got["z"].shape[-1]
        assert bool(torch.isfinite(got["z_full"]).all()), "z not fully written (NaN left in the output)"
        assert bool((got["z_full"][..., Co:] == 0).all()), "padding channels of z must be exactly zero"
    if "dx_full" in got:
        assert bool(torch.isfinite(got["dx_full"]).all()), "dx not fully written (NaN left in the output)"
    if "dw" in got:
        assert bool(torch.isfinite(got["dw"]).all() and torch.isfinite(got["db"]).all()), "dW / db not fully written"
    errs, where = {}, {}
    for q, (rk, gk) in _CONV_QUANTITIES.items():
        if gk not in got:
            continue
        a, r = got[gk], ref[rk].to(got[gk].device)
        if q == "sum" and got["z"].shape[1] * got["z"].shape[2] <= 4:
            errs[q], where[q] = 0.0, ()  # (2 x 2 images: every output sums the same four inputs, sum z cancels)
            continue
        errs[q], where[q] = err_where(a, r)
    report(*label, {q: f"{e:.2e}" for q, e in errs.items()}, "worst at", where)
    bad = {q: e for q, e in errs.items() if not e < tols[q]}
    assert not bad, (bad, {q: where[q] for q in bad})
    return errs, where


STORAGE_TYPES = {"bf16-mixed": (torch.bfloat16, 2.0 ** -7), "16-mixed": (torch.float16, 2.0 ** -10)}  # type, largest relative spacing


def fp32_acc_bound(k, small):
    """Bound (of a tensor's scale) for the fp32 accumulation error of sums of `k` exact products, never below `small`.
    A running fp32 sum adds a rounding error of up to 2^-25 of its partial sum per step: over a chain of k steps a random
    walk of about 2^-24 * sqrt(k / 3) of the partial sums' scale.  Blocked and split accumulations only shorten the chains,
    so 2^-24 * sqrt(k), with k the full reduction length (9 x Cin forward, 9 x Cout data gradient, N x H x W weight
    gradient), bounds them; observed on the benchmark's layers (test_conv3x3_at_benchmark_batches_vs_fp64): 0.25 ... 0.37
    of it on the bf16 forward and data gradient (2.0e-6 at k = 8640, 1.95e-6 at 17280), at most 0.3 of it on the weight
    gradients (2.2e-6 at k = 65536, <= 1.5e-6 at k = 2^20 where the kernels split the pixels into slabs)."""
    return max(small, 2.0 ** -24 * k ** 0.5)


def check_bf16_rounded(got, ref, label, acc_k=None, fp32_ref=None):
    """MIMO_PREC_BF16 kernels compute exactly the convolution of the bf16-rounded operands with fp32 accumulation: z, dx and
    dW against a reference of the same operation on round_bf16(x), round_bf16(w), round_bf16(dz) within 2e-6 of each
    tensor's scale (derived on reduction lengths <= 4096); with `acc_k` ({quantity: reduction length}) within
    fp32_acc_bound(k, 2e-6).  With `fp32_ref` (the reference on the unrounded operands), a forward or weight gradient that
    ran on the plain-FMA fp32 kernels instead (the image layer, conv_thin.hip, taken by the plan in this mode too) passes
    at the fp32 bound 2e-5 against it.  Operators that were not run (conv_outputs) are left out.  Reports (after `label`)
    and returns {quantity: error}, {quantity: worst index}."""
    errs, where, bad = {}, {}, {}
    for q, rk in (("fwd", "z"), ("dgrad", "dx"), ("wgrad", "dw")):
        if rk not in got:
            continue
        r = ref[rk].to(got[rk].device)
        errs[q], where[q] = err_where(got[rk], r)
        if errs[q] < (fp32_acc_bound(acc_k[q], 2e-6) if acc_k else 2e-6):
            continue
        e32 = err_where(got[rk], fp32_ref[rk].to(got[rk].device)) if fp32_ref is not None and q != "dgrad" else None
        if e32 is not None and e32[0] < 2e-5:  # (reported as "<quantity>_fp32": the error against the unrounded operands)
            del errs[q], where[q]
            errs[q + "_fp32"], where[q + "_fp32"] = e32
        else:
            bad[q] = errs[q]
    report(*label, {q: f"{e:.2e}" for q, e in errs.items()}, "worst at", where)
    assert not bad, (bad, {q: where[q] for q in bad})
    return errs, where


def check_storage_rounded(got, ref, mode, label, acc_k=None):
    """The 16-bit STORAGE kernels (bf16-mixed / 16-mixed): products of the rounded operands exact, fp32 accumulation, the
    output rounded ONCE to the storage type.  `ref` is the same operation on the rounded operands, unrounded (keys of
    conv3x3_reference_f64, NHWC).  z and dx must be representable in the storage type; z within one unit in the last place
    of the rounded reference element-wise (and >= 98 % identical); dx interior pixels within one unit element-wise, the two
    border rows / columns (sums of up to four rounded padded-domain values, which may cancel) within two units of the
    tensor's scale; dW (fp32 output) within 5e-6 of its scale; the BatchNorm sums (from the unrounded accumulators) within
    1e-5.  The element-wise forward criterion measures a unit at max(|z|, 1e-3): near zero, the fp32 accumulation error
    of the K = 9 x Cin products can exceed one unit of the value itself (cancellation).  With `acc_k` ({"fwd": K}) the
    floor is max(1e-3, fp32_acc_bound(K, 0) * max|z| / ulp) — the element-wise error stays within the fp32 accumulation
    bound of the tensor's scale there (observed in 16-mixed on the benchmark's layers: up to 1.95 units at the 1e-3 floor
    for K = 2160 ... 8640, all within one unit of the K floor; bf16-mixed, whose unit is 8 x wider, stays within one unit
    at 1e-3).  Outputs of the weight gradient alone (conv_outputs without z and dx): the dW criterion alone.  Reports
    (after `label`) and returns the errors (z and dx in units in the last place) and the worst indices."""
    dt, ulp = STORAGE_TYPES[mode]
    if "z" not in got and "dx" not in got:
        e, at = err_where(got["dw"], ref["dw"].to(got["dw"].device))
        report(*label, f"dW {e:.1e}", "worst at", at)
        assert e < 5e-6, ({"wgrad": e}, at)
        return {"wgrad": e}, {"wgrad": at}
    dev = got["z"].device
    r = lambda t: t.to(dt).double()
    z, dx = got["z"].double(), got["dx"].double()
    zr, dxr = ref["z"].to(dev), ref["dx"].to(dev)
    assert torch.equal(r(z), z) and torch.equal(r(dx), dx), "outputs not representable in the storage type"
    floor = max(1e-3, fp32_acc_bound(acc_k["fwd"], 0.0) * float(zr.abs().max()) / ulp) if acc_k else 1e-3
    ez_all = (z - r(zr)).abs() / zr.abs().clamp_min(floor)
    gref, gmax = r(dxr), float(dxr.abs().max())
    rel = (dx - gref).abs() / dxr.abs().clamp_min(1e-3 * gmax)
    H, W = z.shape[1:3]
    e_int = float(rel[:, 2:-2, 2:-2, :].max()) if H > 4 and W > 4 else 0.0
    errs = {"fwd_ulp": float(ez_all.max()) / ulp, "dgrad_ulp": max(e_int, float((dx - gref).abs().max()) / gmax / 2) / ulp,
            "fwd_identical": float((z == r(zr)).double().mean())}
    where = {"fwd_ulp": worst_at(ez_all, torch.zeros_like(ez_all)), "dgrad_ulp": worst_at(dx, gref)}
    for q, gk, rk in (("wgrad", "dw", "dw"), ("sum", "stats0", "sum"), ("sumsq", "stats1", "sumsq")):
        errs[q], where[q] = err_where(got[gk], ref[rk].to(dev))
    ok = {"fwd_ulp": errs["fwd_ulp"] <= 1.01, "fwd_identical": errs["fwd_identical"] > 0.98,
          "dgrad_ulp": errs["dgrad_ulp"] <= 1.01, "wgrad": errs["wgrad"] < 5e-6, "sum": errs["sum"] < 1e-5,
          "sumsq": errs["sumsq"] < 1e-5}
    report(*label, f"z {errs['fwd_ulp']:.2f} ulp ({100 * errs['fwd_identical']:.2f} % identical), dx {errs['dgrad_ulp']:.2f} ulp, "
           f"dW {errs['wgrad']:.1e}, sums {errs['sum']:.1e} / {errs['sumsq']:.1e}", "worst at", where)
    bad = {q: errs[q] for q, v in ok.items() if not v}
    assert not bad, (bad, {q: where.get(q) for q in bad})
    return errs, where


# ---- the reference training step on any device, and the fp64-anchored gradient rule of the whole-network tests ----

def oracle_state_to(ts, device, dtype):
    """A copy of the oracle's TrainState `ts` with every floating tensor — parameters, BatchNorm buffers, Adam moments and
    the loss buffer's ring — on `device` in `dtype` (num_batches_tracked keeps its integer type).  A `get_weights`
    replaced on the instance (fixed subnetwork weights) is kept, its result moved the same way.  `ts` is not modified."""
    import copy
    mv = lambda t: (t.to(device, dtype) if t.is_floating_point() else t.to(device)).clone()
    out = copy.copy(ts)
    out.st = {k: mv(v) for k, v in ts.st.items()}
    out.exp_avg = {k: mv(v) for k, v in ts.exp_avg.items()}
    out.exp_avg_sq = {k: mv(v) for k, v in ts.exp_avg_sq.items()}
    lb = copy.copy(ts.loss_buffer)
    lb.buffer = mv(ts.loss_buffer.buffer)
    if "get_weights" in vars(ts.loss_buffer):
        lb.get_weights = lambda f=ts.loss_buffer.get_weights: f().to(device, dtype)
    out.loss_buffer = lb
    return out


def reference_train_step(ts, image, label, mask, perms, device="cpu", dtype=torch.float64, **kw):
    """O.train_step (keywords passed on) with every tensor on `device` in `dtype`: runs on oracle_state_to(ts, device,
    dtype) and returns that state (stepped) and the step's results; `ts` itself is not modified.  MIOpen is switched off,
    so on the GPU the reference convolutions are torch's own im2col GEMMs in `dtype`, not an algorithm MIOpen picks (and,
    for float64, one that exists at all).  Pinned to O.train_step on the CPU by tests/test_reference_step_cpu.py."""
    ts = oracle_state_to(ts, device, dtype)
    cast = lambda t: None if t is None else t.to(device, dtype)
    with torch.backends.cudnn.flags(enabled=False):
        res = O.train_step(ts, cast(image), cast(label), cast(mask), perms.to(device), **kw)
    return ts, res


def to_cpu(obj):
    """tensors (also inside dicts) moved to the host"""
    if isinstance(obj, dict):
        return {k: to_cpu(v) for k, v in obj.items()}
    return obj.cpu() if isinstance(obj, torch.Tensor) else obj


def check_grads_vs_fp64(grads, g32, g64, small_net=False):
    """The gradient rule of the whole-network parity tests (test_network_gpu.py::_oracle_vs_hip): ReLU / max-pool
    derivatives are discontinuous, so the gradients are anchored on the fp64 reference and judged against what fp32
    arithmetic itself does on the same problem (the fp32 reference `g32` against `g64`).  Per tensor (the pre-BatchNorm
    biases excluded: mathematically zero), the HIP gradient's relative L2 error must stay within floor + 5 x the larger of
    the fp32 reference's error on that tensor and over all tensors; floor 1e-3 (5e-3 with `small_net`).  Asserts that and
    returns the whole-gradient cosine and relative L2 error (the callers bound those), the worst tensor (name, error,
    fp32-reference error), the fp32 reference's whole-gradient error and how often its arm decided.  All tensors on one
    device."""
    ks = [k for k in g64 if not is_prebn_bias(k)]
    eo_all = (sum(float(((g32[k].double() - g64[k]) ** 2).sum()) for k in ks)
              / sum(float((g64[k] ** 2).sum()) for k in ks)) ** 0.5
    worst, dot, nh, nr, nd = ("", 0.0, 0.0), 0.0, 0.0, 0.0, 0.0
    n_tensors = arm_all = need_all = 0
    floor = 5e-3 if small_net else 1e-3
    for k in ks:
        g, r = grads[k].double(), g64[k]
        eh = float((g - r).norm() / r.norm())
        eo = float((g32[k].double() - r).norm() / r.norm())
        if eh > worst[1]:
            worst = (k, eh, eo)
        assert eh <= floor + 5.0 * max(eo, eo_all), (k, eh, eo, eo_all)
        n_tensors += 1
        arm_all += eo_all > eo               # the whole-gradient arm is the larger of the two for this tensor
        need_all += eh > floor + 5.0 * eo    # ... and the tensor would NOT have passed on its own fp32-reference error
        dot += float((g * r).sum())
        nh += float((g ** 2).sum())
        nr += float((r ** 2).sum())
        nd += float(((g - r) ** 2).sum())
    return {"cos": dot / (nh * nr) ** 0.5, "rel_l2": (nd / nr) ** 0.5, "worst": worst, "eo_all": eo_all,
            "arm_all": arm_all, "need_all": need_all, "n_tensors": n_tensors}
