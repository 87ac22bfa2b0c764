// Test-only: plan.hip compiled into libmimo_plan_probe.so together with one more entry point, which copies a convolution
// layer's input and pre-activation tensor z out of a plan after a forward.  tests/test_plan_entry_gpu.py holds
// mimo_op_conv3x3_forward to the z the plan's own launch wrote, byte for byte.  Not part of libmimo_hip.so.
#include "../../mimo_unet_amd/csrc/plan.hip"

// Layer `second` (0 / 1) of DoubleConv `dc` (forward order).  geom[9] = N, H, W, Cin, Cout, cin_p, cout_p, pixel pitch of the
// input, StoreType of z; off[2] = float offsets of its weight and bias in the parameter buffer.  in_out / z_out (device,
// nullable): N * H * W * pitch input elements (fp32) and N * H * W * cout_p elements of z are copied there on `stream`.
extern "C" __attribute__((visibility("default"))) int mimo_test_conv_layer(mimo_plan* p, int dc, int second, int32_t* geom, int64_t* off,
                                                                          float* in_out, float* z_out, mimo_stream stream) {
  if (!p || dc < 0 || dc >= (int)p->dcs.size() || !geom || !off) return MIMO_ERR_INVALID;
  const ConvBN& L = second ? p->dcs[dc]->c2 : p->dcs[dc]->c1;
  const int g[9] = {L.N, L.H, L.W, L.Cin, L.Cout, L.cin_p, L.cout_p, L.ld_in, L.r.dtz};
  for (int i = 0; i < 9; ++i) geom[i] = g[i];
  off[0] = L.off_w;
  off[1] = L.off_b;
  const size_t P = (size_t)L.N * L.H * L.W;
  if (in_out) MIMO_HIP_CHECK(hipMemcpyAsync(in_out, L.in, P * L.ld_in * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (z_out) MIMO_HIP_CHECK(hipMemcpyAsync(z_out, L.z, P * L.cout_p * store_bytes(L.r.dtz), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MIMO_OK;
}
