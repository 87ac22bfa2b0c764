// How one 3x3 convolution layer is launched, decided in one place: the kernel family, the packed rows, the wide rows and
// the pair tail of the forward and of the data gradient; the tiling, split count, operand storage and MFMA count of the
// weight gradient; the element type of z.  The plan (once per layer, in build()) and the per-operator entry points
// (ops_api.hip) take every launch from conv_recipe; fill_conv_launch / fill_wgrad_launch (conv_launch.h) turn a recipe into
// the launch structs and pack::make_job reads the same rows, wide and pair.  Pure host arithmetic on tile_sched.h and
// pack_layout.h with no HIP dependency: tests/host/conv_recipe_test.cpp, built with g++ -fsanitize=address,undefined,
// holds it against a table of the decisions of the code it replaced (tests/test_sched_cpu.py).
#pragma once

#include "pack_layout.h"
#include "tile_sched.h"

namespace mimo {

constexpr int kDzMaxSlots = 2048 * 2;  // workgroups of the largest launch that writes dz (<= 2048 x 2)

// What the decisions depend on besides the layer: the kernels' switches and the device (filled by conv_env, common.h)
struct ConvEnv {
  bool thin = true;       // the plain-FMA image kernels exist (conv_thin.hip, MIMO_CONV_THIN)
  bool conv_ws = true;    // wave-specialised 256-pixel convolution kernels (MIMO_CONV_WS)
  int wide_force = 0;     // sched::wide_config's force (MIMO_CONV_WIDE)
  int ksplit_force = -1;  // sched::split_pick_ksplit's force (MIMO_CONV_KSPLIT)
  bool wgrad_ws = true;   // wave-specialised weight-gradient kernels (MIMO_WGRAD_WS)
  bool wgrad_np2 = true;  // ... and their two-MFMA instances (MIMO_WGRAD_NP != 3)
  int wg_cus = 256;       // CUs the weight-gradient launches are sized for (sched::wg_side_cus)
};

struct ConvDir {       // one direction of a layer: PACK_FWD or PACK_DGRAD
  int mode = 0;        // of conv3x3_bf16x3_launch / conv3x3_wide_launch (pack::conv_mode)
  bool split = false;  // runs there; else on the fp32 family (conv3x3.hip, or conv_thin.hip where ConvRecipe::thin)
  int rows = 0;        // packed weight rows of the 256-pixel kernels = entries of the row map
  int wide = 0;        // != 0: the launch runs on conv_wide.hip, value = its packed weight rows
  int pair = 0;        // 1: on the tap-paired instance of the 256-pixel split kernel, the image's last chunk laid out for it
  size_t kpart = 0;    // floats of scratch for the slabs of this launch's K split (0: none)
};

struct ConvRecipe {
  ConvDir fwd, dgrad;
  bool thin = false;  // forward of the image convolution (<= 4 input channels) on the plain-FMA kernels
  int dtz = ST_F32;   // element type of z: the storage type, fp32 where the fp32 kernel family writes it
  bool wg_split = false;  // weight gradient on wgrad_split.hip, else on conv3x3.hip's fp32 kernel
  int wg_cin_pad = 0, wg_cout_pad = 0, wg_splits = 1;
  int wg_store = 0, wg_np = 3;  // WgradLaunch::store, ::np
  bool wg_np2 = false;   // ... np = 2 once the launch that writes dz has left max |dz| for it
  bool wg_thin = false;  // ... on the plain-FMA kernel where wgrad_thin_ok agrees and no data gradient is wanted
};

// k_p: input channels of the launch, store: its stored output channels (forward: cin_p -> cout_p; data gradient: cout_p -> cin_p)
static inline ConvDir conv_dir(int precision, int dir, bool split, int N, int k_p, int store, int rows, int Ho, int Wo, const ConvEnv& e) {
  ConvDir d;
  d.mode = pack::conv_mode(precision, dir);
  d.split = split;
  d.rows = rows;
  if (!split) return d;
  if (precision == MIMO_PREC_SPLIT16 || pack::is_mixed(precision))  // decomposition per layer and direction
    d.wide = sched::wide_config(d.mode, N, k_p, store, Ho, Wo, e.wide_force).rows_pad;
  if (d.wide) return d;
  d.pair = sched::ws_tail_pairs(d.mode, k_p, Ho, Wo, e.conv_ws);
  // K split of the few-tile / long-K launches (split16 only: 1 in every other mode)
  const int ks = sched::split_pick_ksplit(d.mode, N, k_p, rows, Ho, Wo, e.conv_ws, e.ksplit_force);
  d.kpart = sched::ksplit_scratch_floats(ks, N, Ho, Wo, store);
  return d;
}

// cin_p, cout_p: padded channel counts of the layer's input and output tensors; inference_only: mimo_config's (0 full plan,
// 2 input gradient only, 1 no backward); ident_in: logical input channel i lies in padded channel i (the packed image)
static inline ConvRecipe conv_recipe(int precision, int inference_only, int N, int H, int W, int Cin, int Cout, int cin_p,
                                     int cout_p, bool ident_in, const ConvEnv& e) {
  ConvRecipe r;
  const bool mfma16 = precision != MIMO_PREC_FP32, mixed = pack::is_mixed(precision), f16 = precision == MIMO_PREC_FP16_MIXED;
  // split MFMA needs a K chunk of 32 channels; the 2..4-channel image convolution stays on the fp32 kernels (16-bit
  // storage: every layer but the image convolution runs on the 16-bit kernels, whose loaders move 8-channel units)
  const bool fs = mfma16 && cin_p >= (mixed ? 8 : 16);
  r.fwd = conv_dir(precision, PACK_FWD, fs, N, cin_p, cout_p, sched::conv_cout_pad(Cout), H, W, e);
  r.dgrad = conv_dir(precision, PACK_DGRAD, mfma16 && (mixed || cout_p >= 16), N, cout_p, cin_p, sched::conv_cout_pad(cin_p),
                     H + 2, W + 2, e);
  if (inference_only) r.fwd.kpart = 0;  // (the training forward alone is split)
  if (inference_only == 1) r.dgrad.kpart = 0;
  r.dtz = fs ? pack::store_type(precision) : ST_F32;
  r.thin = !fs && ident_in && e.thin && sched::thin_geometry_ok(Cin, cout_p);
  r.wg_thin = r.thin && !mixed;
  r.wg_split = mfma16;
  if (!mfma16) {
    r.wg_cin_pad = sched::rup(cin_p, 32);
    r.wg_cout_pad = sched::rup(cout_p, 32);
    r.wg_splits = sched::wg32_pick_splits(N, H, W, r.wg_cin_pad, r.wg_cout_pad);
    return r;
  }
  int CI, CO;
  sched::wg_tiles(cin_p, cout_p, e.wgrad_ws, &CI, &CO);
  r.wg_cin_pad = sched::rup(cin_p, CI);
  r.wg_cout_pad = sched::rup(cout_p, CO);
  // 16-bit storage: activations and dz plain NHWC 16-bit; the image convolution's input stays fp32
  r.wg_store = !mixed ? 0 : (fs ? (f16 ? 2 : 1) : (f16 ? 4 : 3));
  r.wg_np = (precision == MIMO_PREC_BF16 || mixed) ? 1 : 3;
  r.wg_splits = sched::wg_pick_splits(N, H, W, r.wg_cin_pad, r.wg_cout_pad, CI, CO, e.wgrad_ws, r.wg_store == 1 || r.wg_store == 2, e.wg_cus);
  // two fp16 MFMAs per product: not for the image convolution (raw inputs need not fit fp16: its forward runs on the fp32
  // kernels), and only while the launch that writes dz has a max |dz| slot for each of its workgroups
  // (<= 2048 x ceil(Cp / 1024); wider layers keep the three-MFMA arithmetic)
  r.wg_np2 = precision == MIMO_PREC_SPLIT16 && inference_only == 0 && fs && e.wgrad_np2 && sched::wg_use_ws(CI, CO, e.wgrad_ws) &&
             2048 * sched::cdiv(cout_p / 4, 256) <= kDzMaxSlots;
  return r;
}

}  // namespace mimo
