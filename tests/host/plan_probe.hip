// Test-only: plan.hip compiled into libmimo_plan_probe.so together with three more entry points.  Not part of libmimo_hip.so.
//   mimo_test_conv_layer copies a convolution layer's input and pre-activation tensor z out of a plan after a forward:
//     tests/test_plan_entry_gpu.py holds mimo_op_conv3x3_forward to the z the plan's own launch wrote, byte for byte;
//   mimo_test_wgrad_recipe tells which weight-gradient launch the library's own conv_recipe makes for a layer at a CU count:
//     tests/test_wgrad_splits_gpu.py asserts from it that each of its cases runs the class of launch it is there for;
//   mimo_test_wg_side_cus gives the CU count a plan sizes those launches for (tests/helpers.py plan_wgrad_cus).
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

// Host only: the weight-gradient fields of conv_recipe(precision, 0, N, H, W, Cin, Cout, cin_p, cout_p, true, conv_env(cus)) —
// the recipe of a full plan for a layer whose input channels lie in order, as the per-operator entry points take it.  wg_cus
// >= 1: cus = wg_cus, whatever MIMO_WGRAD_CUS says; wg_cus <= 0: cus = wgrad_cus(256), what mimo_op_conv3x3_wgrad runs right
// now.  out[9] = wg_splits, the CI and the CO tile, 1 on the wave-specialised kernel, wg_np2, the pixel tiles the splits
// share, the blocks of the reduction's last kernel (>= 512: final fan 16, else 1), wg_store, 1 where the entry point runs the
// plain-FMA image kernel instead (no splits).  Every switch is read as the library reads it (MIMO_WGRAD_WS, MIMO_WGRAD_NP,
// ...).  fp32 (no split weight gradient): MIMO_ERR_INVALID.
extern "C" __attribute__((visibility("default"))) int mimo_test_wgrad_recipe(int32_t precision, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                                                            int32_t cin_p, int32_t Cout, int32_t cout_p, int32_t wg_cus,
                                                                            int32_t* out) {
  if (!out || N < 1 || H < 2 || W < 2 || Cin < 1 || Cout < 1 || cin_p < Cin || cout_p < Cout) return MIMO_ERR_INVALID;
  const ConvEnv e = conv_env(wg_cus >= 1 ? wg_cus : wgrad_cus(256));
  const ConvRecipe r = conv_recipe(precision, 0, N, H, W, Cin, Cout, cin_p, cout_p, true, e);
  if (!r.wg_split) return MIMO_ERR_INVALID;
  int CI, CO;
  sched::wg_tiles(cin_p, cout_p, e.wgrad_ws, &CI, &CO);
  const bool ws = sched::wg_use_ws(CI, CO, e.wgrad_ws);
  const int tr = ws ? sched::wg_ws_tr(CI, r.wg_store == 1 || r.wg_store == 2) : 4;
  const int v[9] = {r.wg_splits, CI, CO, ws ? 1 : 0, r.wg_np2 ? 1 : 0, sched::wg_num_tiles(N, H, W, tr),
                    sched::cdiv(r.wg_cin_pad, 32) * sched::cdiv(r.wg_cout_pad, 8), r.wg_store,
                    (r.wg_thin && wgrad_thin_ok(Cin, cout_p, N, H, W)) ? 1 : 0};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  return MIMO_OK;
}

// The CUs a plan of `pixels` = N x H x W input pixels and `width` = subnetworks x filter_base_count sizes its weight-gradient
// launches for (what Plan::build() passes to wgrad_cus)
extern "C" __attribute__((visibility("default"))) int mimo_test_wg_side_cus(int64_t pixels, int32_t width) {
  return sched::wg_side_cus((long)pixels, width);
}
