"""The split weight gradient (wgrad_split.hip and the slab reduction of conv3x3.hip) at the split counts the plans run.

How many pixel slabs a weight-gradient launch writes, how many tiles each workgroup owns and how the reduction walks its
stage-A groups of 16 all follow from sched::wg_pick_splits, which takes the CUs the launch is sized for (ConvEnv::wg_cus).  A
plan sizes it for 128, 192 or 256 CUs (sched::wg_side_cus: every small plan of this suite and every strong-scaling shard of
the benchmark gets 128 or 192), the per-operator entry points for 256 — so the cases of tests/test_ops_gpu.py run other
launches than the plans do.  mimo_op_conv3x3_wgrad honours MIMO_WGRAD_CUS with the plan's rule (wgrad_cus, common.h); these
tests run it at 128, at 192 and unset, on shapes chosen so that each class of launch is reached at a CU count other than
256.  Which class a case reaches is never restated here: every case asserts it from the library's own conv_recipe through
libmimo_plan_probe.so (helpers.wgrad_recipe), so a case cannot silently leave its class when the cost rule changes.

Modes: split16 (two MFMAs per product), split16 under MIMO_WGRAD_NP=3, bf16, bf16-mixed, 16-mixed.  Not fp32: its
sched::wg32_pick_splits does not take the CU count.

The final fan of 16 (>= 512 reduction blocks) with more than 16 splits needs a large layer: >= 512 blocks means >= 32 channel
tiles per slab, which fill a round of workgroups with <= 8 splits, and a further round costs the fixed cost of a workgroup
again — the cost rule goes past 16 splits only where the last round would otherwise stay nearly empty over more than a
thousand pixel tiles.  The smallest such shapes (a host search over channel counts up to 960 and tile counts up to 4096,
cost = pixels x channels): 264 -> 520 channels with 1376 two-row tiles (2 x 86 x 512, 88064 pixels) for the operands stored
in fp32, with 595 four-row tiles (5 x 28 x 544, 76160 pixels) for the 16-bit tensors; both give 17 splits at 128 CUs."""
import pytest
import torch

from tests.helpers import (STORAGE_TYPES, check_bf16_rounded, check_conv_results, check_storage_rounded, conv3x3_reference_f64,
                           conv_cin_pad, conv_tolerances, err_where, pad8, report, wgrad_recipe, wgrad_two_mfma, worst_at)
from tests.test_ops_gpu import _lib, run_conv, to_nhwc

pytestmark = pytest.mark.gpu

F32_STORED = ("split16", "split16-np3", "bf16")  # x and dz reach the kernel as fp32 / pair records: two-row tiles at CI = 64
MIXED = ("bf16-mixed", "16-mixed")  # both operands 16-bit tensors (WgradLaunch::store 1 / 2): four-row tiles
MODES = F32_STORED + MIXED
CUS_SETTINGS = (128, 192, None)  # MIMO_WGRAD_CUS; None: unset (256)


def _even(r, r256, by_cus):
    return 1 < r["splits"] < r["tiles"] and r["tiles"] % r["splits"] == 0


def _uneven(r, r256, by_cus):  # some workgroups own one tile fewer
    return r["splits"] < r["tiles"] and r["tiles"] % r["splits"] != 0


def _differs(r, r256, by_cus):
    return len({v["splits"] for v in by_cus.values()}) > 1


def _single(r, r256, by_cus):
    return r["splits"] == 1 and r256["splits"] > 1


def _fan1_short_group(r, r256, by_cus):  # stage A down to one slab, its last group of 16 not full
    return r["splits"] > 16 and r["splits"] % 16 != 0 and r["reduce_blocks"] < 512


def _fan16_short_group(r, r256, by_cus):  # one stage A, then <= 16 slabs summed by the transposing kernel
    return r["splits"] > 16 and r["splits"] % 16 != 0 and r["reduce_blocks"] >= 512


def _instance(r, r256, by_cus):  # (the CI / CO tile is asserted for every case)
    return True


# (class, (N, H, W, Cin, Cout), the MIMO_WGRAD_CUS the class is reached at, (CI, CO) of the wave-specialised instance, modes)
CASES = [
    (_even, (4, 64, 96, 30, 30), 128, (32, 32), MODES),
    (_even, (3, 40, 72, 90, 45), 128, (32, 48), MODES),
    (_uneven, (3, 68, 96, 30, 30), 128, (32, 32), MODES),
    (_differs, (1, 16, 16, 480, 480), 192, (64, 64), MODES),
    (_differs, (2, 16, 16, 240, 240), 128, (64, 64), F32_STORED),
    (_differs, (2, 32, 16, 240, 240), 192, (64, 64), MODES),
    (_differs, (2, 50, 70, 84, 42), 128, (32, 48), MODES),
    (_single, (1, 8, 8, 960, 480), 128, (64, 64), MODES),
    (_fan1_short_group, (7, 20, 33, 60, 60), 128, (64, 64), MODES),
    (_fan16_short_group, (2, 86, 512, 264, 520), 128, (64, 64), F32_STORED),
    (_fan16_short_group, (5, 28, 544, 264, 520), 128, (64, 64), MIXED),
    (_instance, (3, 40, 72, 60, 45), 128, (64, 48), MODES),
    (_instance, (3, 40, 72, 60, 30), 128, (64, 32), MODES),
    (_instance, (3, 40, 72, 90, 60), 192, (32, 64), MODES),
]
PARAMS = [(c, m) for c in CASES for m in c[4]]
IDS = [f"{c[0].__name__.strip('_')}-{'x'.join(map(str, c[1]))}@{c[2]}-{m}" for c, m in PARAMS]
WS_INSTANCES = {(64, 64), (64, 48), (64, 32), (32, 64), (32, 48), (32, 32)}


def _precision(mode):
    return "split16" if mode == "split16-np3" else mode


def _set_mode(monkeypatch, mode):
    if mode == "split16-np3":
        monkeypatch.setenv("MIMO_WGRAD_NP", "3")


def _set_cus(monkeypatch, setting):
    if setting is None:
        monkeypatch.delenv("MIMO_WGRAD_CUS", raising=False)
    else:
        monkeypatch.setenv("MIMO_WGRAD_CUS", str(setting))


def assert_class(case, mode):
    """The case reaches its class, on its kernel instance, at its CU count — asked of the library's own recipe.  Returns the
    recipes at 128, 192 and 256 CUs."""
    klass, layer, cus, tile, _ = case
    prec = _precision(mode)
    by_cus = {c: wgrad_recipe(prec, layer, c) for c in (128, 192, 256)}
    r = by_cus[cus]
    report("weight-gradient recipe", klass.__name__.strip("_"), mode, layer, {c: (v["splits"], v["tiles"]) for c, v in by_cus.items()},
           "(splits, tiles) at 128 / 192 / 256 CUs; reduction blocks", r["reduce_blocks"])
    assert cus != 256 and r["ws"] == 1 and r["thin"] == 0 and (r["ci"], r["co"]) == tile, (mode, layer, r)
    assert r["store"] == ({"bf16-mixed": 1, "16-mixed": 2}.get(mode, 0)), (mode, layer, r)
    assert r["np2"] == (1 if wgrad_two_mfma(prec) else 0), (mode, layer, r)
    assert 1 <= r["splits"] <= min(r["tiles"], 1024), r
    assert klass(r, by_cus[256], by_cus), (klass.__name__, mode, layer, by_cus)
    return by_cus


def run_wgrad(monkeypatch, mode, layer, setting, x, dz):
    """mimo_op_conv3x3_wgrad under MIMO_WGRAD_CUS = setting into NaN-filled outputs; asserts first that the recipe the entry
    point takes right now is the one of that CU count.  Returns (conv_outputs, recipe)."""
    L = _lib()
    N, H, W, Ci, Co = layer
    prec = _precision(mode)
    _set_cus(monkeypatch, setting)
    ran = wgrad_recipe(prec, layer, 0)
    assert ran == wgrad_recipe(prec, layer, setting or 256), (mode, layer, setting, ran)
    got = run_conv(L.load(), x, None, None, dz, Ci, Co, L.PRECISIONS[prec], fwd=False, dgrad=False)
    return got, ran


@pytest.fixture(scope="module")
def operands():
    """Operands and references, computed once per layer and shared by the modes and tests that follow (the parameters are
    ordered by case); one layer's worth is kept.  get(kind, layer) with kind "random" -> fp32 x, dz (NHWC, padding channels
    zero) and the fp64 reference; ("random", dtype) -> the same rounded to a 16-bit type; "integer" -> integer-valued x in
    {0..3}, dz in {-2..2} and the exact dW / db."""
    cache = {}

    def reference(x, dz, Ci, Co):
        w = torch.zeros(Co, Ci, 3, 3, device="cuda")  # (the weight gradient does not depend on w and b)
        ref = conv3x3_reference_f64(x, w, torch.zeros(Co, device="cuda"), dz)
        return {"dw": ref["dw"], "db": ref["db"]}

    def get(kind, layer):
        if cache and next(iter(cache))[1] != layer:
            cache.clear()
            torch.cuda.empty_cache()
        key = (kind, layer)
        if key in cache:
            return cache[key]
        N, H, W, Ci, Co = layer
        cip, cop = conv_cin_pad(Ci), pad8(Co)
        g = torch.Generator().manual_seed(sum(layer))
        if kind == "random":
            x = to_nhwc(torch.randn(N, Ci, H, W, generator=g), cip)
            dz = to_nhwc(torch.randn(N, Co, H, W, generator=g), cop)
        elif kind == "integer":
            x = to_nhwc(torch.randint(0, 4, (N, Ci, H, W), generator=g).float(), cip)
            dz = to_nhwc(torch.randint(-2, 3, (N, Co, H, W), generator=g).float(), cop)
        else:
            x0, dz0, _ = get("random", layer)
            x, dz = x0.to(kind[1]).float(), dz0.to(kind[1]).float()
        ref = reference(x, dz, Ci, Co)
        if kind == "integer":  # float64 sums of integers below 2^53: exact
            ref = {k: v.round().to(torch.int64) for k, v in ref.items()}
        cache[key] = (x, dz, ref)
        return cache[key]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def test_every_kernel_instance_and_class_is_reached_below_256_cus():
    """Through the library's recipe: in every mode the cases reach all six CI / CO instances of the wave-specialised kernel
    at 128 or 192 CUs — in the 16-bit storage modes on four-row tiles of 16-bit operands (WgradLaunch::store 1 / 2) — and
    every class of launch."""
    for mode in MODES:
        seen, classes = set(), set()
        for case in CASES:
            if mode in case[4]:
                r = wgrad_recipe(_precision(mode), case[1], case[2])
                assert r["ws"] == 1 and case[2] != 256
                seen.add((r["ci"], r["co"]))
                classes.add(case[0])
        assert seen == WS_INSTANCES, (mode, seen)
        assert classes == {_even, _uneven, _differs, _single, _fan1_short_group, _fan16_short_group, _instance}, mode


@pytest.mark.parametrize("case,mode", PARAMS, ids=IDS)
def test_weight_gradient_vs_fp64_at_plan_split_counts(case, mode, operands, monkeypatch):
    """dW and db of mimo_op_conv3x3_wgrad at MIMO_WGRAD_CUS = 128, 192 and unset against conv3x3_reference_f64, each split
    count against the reference (never one against another), under the bounds of the small cases of tests/test_ops_gpu.py:
    split16 conv_tolerances (5e-4 with two MFMAs per product, 1e-4 with three; db 2e-5); bf16 conv_tolerances against the exact
    operands and check_bf16_rounded against the bf16-rounded ones; the storage modes check_storage_rounded (dW 5e-6) against
    the rounded operands they are given, db 2e-5.  acc_k: the reduction length N x H x W, as the benchmark-batch test passes it."""
    _set_mode(monkeypatch, mode)
    assert_class(case, mode)
    layer = case[1]
    N, H, W, Ci, Co = layer
    acc_k = {"wgrad": N * H * W}
    for setting in CUS_SETTINGS:
        label = ("weight gradient at", setting or "unset", "CUs", mode, layer)
        if mode in MIXED:
            x, dz, ref = operands(("random", STORAGE_TYPES[mode][0]), layer)
            got, ran = run_wgrad(monkeypatch, mode, layer, setting, x, dz)
            check_storage_rounded(got, ref, mode, label + (ran["splits"], "splits"), acc_k)
            e, at = err_where(got["db"], ref["db"])
            assert e < conv_tolerances("split16")["bgrad"], ("db", e, at)
        else:
            x, dz, ref = operands("random", layer)
            got, ran = run_wgrad(monkeypatch, mode, layer, setting, x, dz)
            check_conv_results(got, ref, _precision(mode), label + (ran["splits"], "splits"))
            if mode == "bf16":
                rref = operands(("random", torch.bfloat16), layer)[2]
                check_bf16_rounded(got, rref, label + ("rounded operands",), acc_k)
        del got


@pytest.mark.parametrize("case,mode", PARAMS, ids=IDS)
def test_weight_gradient_is_exact_on_small_integers_at_every_split_count(case, mode, operands, monkeypatch):
    """x in {0..3} and dz in {-2..2}, integer-valued: fp16, bf16 and the hi / lo pairs hold them exactly, the two-MFMA
    power-of-two dz scale is exact, and with 6 x N x H x W < 2^24 every product and every partial sum — of a tile, a slab, a
    stage-A group — is an integer fp32 holds exactly, in any order.  dW and db equal the integer reference bit for bit at
    128, at 192 and at 256 CUs, and so one another: one misplaced, dropped or repeated tile or slab changes an integer,
    whatever the tolerance (after test_per_channel_sums_are_exact_on_small_integers)."""
    _set_mode(monkeypatch, mode)
    assert_class(case, mode)
    layer = case[1]
    N, H, W, Ci, Co = layer
    assert 6 * N * H * W < 2 ** 24  # |x dz| <= 6 per pixel: every partial sum stays below 2^24
    x, dz, ref = operands("integer", layer)
    dw_ref, db_ref = ref["dw"].float(), ref["db"].float()
    assert torch.equal(dw_ref.to(torch.int64), ref["dw"]) and float(dw_ref.abs().max()) > 0
    bits = {}
    for setting in CUS_SETTINGS:
        got, ran = run_wgrad(monkeypatch, mode, layer, setting, x, dz)
        dw, db = got["dw"], got["db"]
        if not torch.equal(dw, dw_ref):
            at = worst_at(dw.nan_to_num(nan=float("inf")), dw_ref)
            report("integer weight gradient", mode, layer, "at", setting or "unset", "CUs,", ran["splits"], "splits of", ran["tiles"],
                   "tiles: worst (cout, cin, ky, kx)", at, "got", float(dw[at]), "exact", float(dw_ref[at]),
                   "wrong elements", int((dw != dw_ref).sum()))
        assert torch.equal(dw, dw_ref), (mode, layer, setting, ran)
        assert torch.equal(db, db_ref), (mode, layer, setting)
        bits[setting] = dw.view(torch.int32).clone()
    assert torch.equal(bits[128], bits[None]) and torch.equal(bits[192], bits[None])


@pytest.mark.parametrize("case,mode", PARAMS, ids=IDS)
def test_default_sizing_is_untouched(case, mode, operands, monkeypatch):
    """MIMO_WGRAD_CUS unset, 7 and 300 (outside 8..256): the entry point takes the 256-CU recipe and returns the same dW bit
    for bit in each."""
    _set_mode(monkeypatch, mode)
    layer = case[1]
    prec = _precision(mode)
    x, dz, _ = operands(("random", STORAGE_TYPES[mode][0]) if mode in MIXED else "random", layer)
    want = wgrad_recipe(prec, layer, 256)
    out = {}
    for setting in (None, 7, 300):
        _set_cus(monkeypatch, setting)
        assert wgrad_recipe(prec, layer, 0) == want, (mode, layer, setting)
        L = _lib()
        got = run_conv(L.load(), x, None, None, dz, layer[3], layer[4], L.PRECISIONS[prec], fwd=False, dgrad=False)
        assert bool(torch.isfinite(got["dw"]).all())
        out[setting] = got["dw"].view(torch.int32).clone()
    assert torch.equal(out[7], out[None]) and torch.equal(out[300], out[None])
