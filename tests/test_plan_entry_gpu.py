"""The plan and the per-operator entry point launch a convolution layer the same way: both take the launch from
conv_recipe and fill_conv_launch (mimo_unet_amd/csrc/conv_recipe.h, conv_launch.h), so mimo_op_conv3x3_forward on a layer's
input and weights returns the pre-activation tensor z the plan's own forward wrote, byte for byte.

z never leaves a plan through the C ABI.  libmimo_plan_probe.so (built next to the library from the same objects, with
tests/host/plan_probe.hip compiled together with plan.hip) adds one test-only entry point that copies a layer's input and z
out; the entry point under test is the product library's."""
import ctypes as C
import os

import pytest
import torch

from mimo_unet_amd import _lib as L

PROBE = os.path.join(os.path.dirname(L.LIB_PATH), "libmimo_plan_probe.so")


def _probe():
    lib = C.CDLL(PROBE)
    for name, (res, args) in L._SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.mimo_test_conv_layer.restype = C.c_int
    lib.mimo_test_conv_layer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["split16", "fp32"])
def test_entry_point_forward_is_the_plans_forward_byte_for_byte(precision):
    """S = 2, f = 8 on 2-channel 64 x 64 images, N = 2: the first convolution of encoder.down1s.0 is 8 -> 16 at 32 x 32.  After
    one training forward its input (the pooled encoder output the plan materialised) and its weights go through
    mimo_op_conv3x3_forward; the result equals the plan's z in every byte, padding channels included."""
    probe, lib = _probe(), L.load()
    S, f, N, H, W = 2, 8, 2, 64, 64
    dev = torch.device("cuda", 0)
    st = L.current_stream()
    cfg = L.MimoConfig(2, 2, S, f, N, H, W, 0.0, 0.0, 0.0, 1e-5, 0.1, L.LOSS_KINDS["laplace_nll"], 1e-5, 1e3, 0,
                       L.PRECISIONS[precision], 0, 0.0, 0.0, 0, 0, 0)
    plan = C.c_void_p()
    assert probe.mimo_plan_create(C.byref(cfg), C.byref(plan)) == 0
    try:
        g = torch.Generator().manual_seed(7)
        params = (torch.randn(int(probe.mimo_plan_param_floats(plan)), generator=g) * 0.2).to(dev)
        grads = torch.zeros_like(params)
        buffers = torch.ones(int(probe.mimo_plan_buffer_floats(plan)), device=dev)
        assert probe.mimo_plan_bind(plan, params.data_ptr(), grads.data_ptr(), buffers.data_ptr()) == 0
        x = torch.rand(N, S, 2, H, W, generator=g).to(dev)
        out = torch.empty(N, S, 2, H, W, device=dev)
        args = L.ForwardArgs(x.data_ptr(), x.stride(0), x.stride(1), None, 1, None, out.data_ptr(), None, 0, 0, None, 0, 0, N)
        assert probe.mimo_forward(plan, C.byref(args), st) == 0
        geom, off = (C.c_int32 * 9)(), (C.c_int64 * 2)()
        layer = S  # DoubleConvs in forward order: the S input blocks, then encoder.down1s.0
        assert probe.mimo_test_conv_layer(plan, layer, 0, geom, off, None, None, st) == 0
        n, h, w, cin, cout, cin_p, cout_p, ld_in, dtz = list(geom)
        assert (n, h, w, cin, cout, cin_p, cout_p, ld_in, dtz) == (N, 32, 32, 8, 16, 8, 16, 8, 0)
        xin = torch.full((n, h, w, ld_in), float("nan"), device=dev)
        z_plan = torch.full((n, h, w, cout_p), float("nan"), device=dev)
        assert probe.mimo_test_conv_layer(plan, layer, 0, geom, off, xin.data_ptr(), z_plan.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(xin).all() and torch.isfinite(z_plan).all() and float(z_plan.abs().max()) > 0.0
        wt = params[off[0]:off[0] + cout * cin * 9]
        bias = params[off[1]:off[1] + cout]
        z_op = torch.full((n, h, w, cout_p), float("nan"), device=dev)
        L.check(lib.mimo_op_conv3x3_forward(xin.data_ptr(), wt.data_ptr(), bias.data_ptr(), z_op.data_ptr(), None, n, h, w, cin, cin_p,
                                            cout, cout_p, L.PRECISIONS[precision], st), "conv fwd")
        torch.cuda.synchronize()
        assert torch.equal(z_plan.view(torch.int32), z_op.view(torch.int32))
    finally:
        probe.mimo_plan_destroy(plan)
