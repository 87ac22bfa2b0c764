"""CPU checks of the convolution test infrastructure: the fp64 reference the production-batch operator test compares the
HIP kernels with (pinned to the oracle), and the table of layers that test runs (pinned to bench.CONFIGS and to the
layer list scripts/conv_layer_bench.py times).  No GPU needed."""
import importlib.util
import os

import pytest
import torch

from oracle import mimo_oracle as O
from tests.helpers import (benchmark_conv_layers, benchmark_shards, config_conv_layers, conv3x3_reference_f64, conv_cin_pad,
                           rel_err)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", [(2, 2, 5, 3, 5), (1, 3, 2, 5, 7), (3, 3, 3, 1, 4), (2, 7, 9, 13, 6), (2, 2, 2, 2, 3),
                                  (1, 6, 11, 9, 1)], ids=lambda c: "x".join(map(str, c)))
def test_fp64_reference_matches_the_oracle_convolution(case):
    """conv3x3_reference_f64 (nine shifted matmuls, autograd through F.pad's reflect border) against O.conv3x3_reflect run
    in float64: z, dx (the fold of the reflect border: H or W of 2 and 3, odd channel counts), dW, db and the per-channel
    sums, to rounding of fp64.  NHWC inputs with padding channels (ignored), one image per chunk (the chunked sums)."""
    N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, generator=g).double()  # (fp32 values: the operator test passes fp32 weights)
    b = torch.randn(Co, generator=g).double()
    dz = torch.randn(N, Co, H, W, generator=g, dtype=torch.float64)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    z = O.conv3x3_reflect(xr, wr, br)
    z.backward(dz)
    z = z.detach()
    nhwc = lambda t, cp: torch.cat([t.permute(0, 2, 3, 1), torch.full((N, H, W, cp - t.shape[1]), 1e30, dtype=t.dtype)], -1)
    ref = conv3x3_reference_f64(nhwc(x, conv_cin_pad(Ci) + 4), w.float(), b.float(), nhwc(dz, Co + 3), chunk_elems=1)
    assert all(v.dtype == torch.float64 for v in ref.values())
    assert ref["z"].shape == (N, H, W, Co) and ref["dx"].shape == (N, H, W, Ci)
    errs = {"z": rel_err(ref["z"], z.permute(0, 2, 3, 1)), "dx": rel_err(ref["dx"], xr.grad.permute(0, 2, 3, 1)),
            "dw": rel_err(ref["dw"], wr.grad), "db": rel_err(ref["db"], br.grad),
            "sum": rel_err(ref["sum"], z.sum(dim=(0, 2, 3))), "sumsq": rel_err(ref["sumsq"], (z * z).sum(dim=(0, 2, 3)))}
    assert max(errs.values()) < 1e-12, errs


def _conv_layer_bench_shapes():
    spec = importlib.util.spec_from_file_location("conv_layer_bench", os.path.join(ROOT, "scripts", "conv_layer_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SHAPES


def test_benchmark_conv_layer_table_covers_what_the_benchmark_runs():
    """benchmark_conv_layers() holds every config of bench.CONFIGS at its batch and at its 2 / 4 / 8-GPU strong-scaling
    shards (cfg3 32 / 16 / 8 / 4, cfg2 64 / 32 / 16 / 8, cfg4 16 / 8 / 4 / 2); every shape scripts/conv_layer_bench.py
    times; and the image layer (<= 3 input channels) at N >= 8, the geometry whose weight gradient runs on the plain-FMA
    kernel in the benchmark and in no small operator case."""
    import bench
    table = benchmark_conv_layers()
    assert len(table) == len(set(table)) == 183
    assert {k: benchmark_shards(c) for k, c in bench.CONFIGS.items()} == {"cfg3": [32, 16, 8, 4], "cfg2": [64, 32, 16, 8],
                                                                           "cfg4": [16, 8, 4, 2]}
    for c in bench.CONFIGS.values():
        f, S, Ci = c["f"], c["S"], c["Ci"]
        assert len(config_conv_layers(c, c["batch"])) == 17
        for n in benchmark_shards(c):
            layers = config_conv_layers(c, n)
            assert set(layers) <= set(table)
            # spot checks written out from the model's widths (model.py:119-297): the image layer, the bottleneck, the
            # first convolution after the deepest up-sampling, the decoder's
            for t in ((n, 256, 256, Ci, f), (n, 128, 128, f, 2 * f), (n, 16, 16, 8 * f * S, 8 * f * S),
                      (n, 32, 32, 16 * f * S, 8 * f * S), (n, 256, 256, f * S + f, (f * S + f) // 2)):
                assert t in layers, (c["name"], t)
    missing = [s for s in _conv_layer_bench_shapes() if s not in table]
    assert not missing, missing
    assert any(N >= 8 and Ci <= 3 for N, H, W, Ci, Co in table)
    assert {t for t in table if t[3] <= 3 and t[0] >= 8} >= {(32, 256, 256, 2, 30), (64, 256, 256, 3, 21), (16, 256, 256, 2, 30)}
