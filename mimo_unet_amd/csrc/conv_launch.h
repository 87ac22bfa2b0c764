// The launch structs of the 3x3 convolutions and the only code that assigns their geometry fields: fill_conv_launch /
// fill_wgrad_launch, from a layer's recipe (conv_recipe.h).  Plain structs, no HIP dependency: the kernels take them by value
// (common.h includes this header) and tests/host/conv_recipe_test.cpp builds them under g++ -fsanitize=address,undefined.
#pragma once

#include "conv_recipe.h"

namespace mimo {

// "forward-type" 3x3 correlation on the f32 MFMA: y[n,oy,ox,co] = bias[co] +
//   sum_{kh,kw,ci} w[kh,kw][co][ci] * X(n, oy+kh-off, ox+kw-off, ci)
// off == 1: Ho==Hi, X is reflect-padded (forward conv, components.py:23,26)
// off == 2: Ho==Hi+2, X is zero outside the image (transposed conv producing the gradient on
//           the reflect-PADDED domain; consumers fold the border back, see fold_read in ew_device.h)
constexpr int kFinSlack = 32;  // zero floats behind ConvLaunch::in_scale / in_shift (a 32-channel chunk may start at cin_p - 8)
struct ConvLaunch {
  const float* x;
  float* y;
  const float* w;     // fp32 kernel: packed [9][cout_pad][cin_p]
  const void* wpk = nullptr;  // split kernel: packed [chunk][tap][cout_pad][hi 32 | lo 32] fp16/bf16
  const float* bias;  // [cout_pad] or nullptr
  float* stats;       // per-block partial sums [blocks][2][cout_pad] or nullptr
  int N, Hi, Wi, ldx, cin_p;
  int Ho, Wo, ldy, cout_pad, cout_store;
  int off;
  // inference epilogue (all null = plain conv output): y = relu(conv * ep_scale[c] + ep_shift[c]) * ep_mask[n][c]
  // — eval-mode BatchNorm + ReLU (+ Dropout2d multipliers, [N][ep_mask_ld]) folded into the store
  const float* ep_scale = nullptr;
  const float* ep_shift = nullptr;
  const float* ep_mask = nullptr;
  int ep_mask_ld = 0;
  int* status = nullptr;  // with ep_scale: bit 0 is OR-ed in when a convolution output is not finite (the ReLU would drop a NaN)
  int pair = 0;  // split kernel: a.wpk holds the tap-paired image of the last chunk (ConvDir::pair)
  // != 0: a.wpk holds the wide kernel's image — [16-channel chunk][tap][wide rows][hi 16 | lo 16] — and the launch runs
  // on conv_wide.hip (value = packed rows, ConvDir::wide)
  int wide = 0;
  // != nullptr (split16 forward on the wave-specialised kernels only, conv3x3_split_fuses_input): x is the PRE-activation
  // tensor z of the producing convolution and the loaders apply its BatchNorm + ReLU on the way into LDS — relu(z *
  // in_scale[c] + in_shift[c]), bn_relu_fwd_kernel's arithmetic (components.py:24-25 between the two convolutions of a
  // DoubleConv) — so that the activated tensor is never written to HBM
  // Both arrays must be readable (and zero) for kFinSlack floats past cin_p: the loaders read whole 16- / 32-channel chunks
  const float* in_scale = nullptr;
  const float* in_shift = nullptr;
  // fp16 weight images (modes 1 and 6): device word with the float bits of the layer's max |w| the image was packed with
  // (w16_scale); nullptr: the image carries the fixed 2^8 (per-operator entry points)
  const unsigned* wmax = nullptr;
  // > 1 (wave-specialised 256-pixel kernel, split16 modes 0 / 1, cin_p a multiple of 32; conv3x3_ksplit): the K walk over
  // the input channels is split ksplit-fold across workgroups; slab k of y — [ksplit][N][Ho][Wo][ldy] — receives the partial
  // sums of chunk range k (bias, stats and the inference epilogue must be null: conv_ksplit_reduce_launch adds them up)
  int ksplit = 1;
};

struct WgradLaunch {
  const float* x;   // [N,H,W,ldx] activations feeding the conv (reflect-padded on the fly)
  const float* dz;  // [N,H,W,lddz]
  float* partial;   // [splits][9][cin_pad][cout_pad]
  int N, H, W, ldx, lddz;
  int cin_p, cout_p;      // valid channel extents in x / dz (multiples of 4)
  int cin_pad, cout_pad;  // multiples of 32
  int splits;
  // split kernels: MFMAs per product block — 3 (bf16 hi/lo pairs both sides), 1 (bf16 compute), or 2 (round 5,
  // wave-specialised kernel, store 0: the activation as one fp16 value, dz as a scaled fp16 pair; needs dz_absmax)
  int np = 3;
  // np == 2: dz_absmax_n floats whose maximum is max |dz| of this tensor — one per workgroup of the launch that wrote dz
  // (bn_bwd_apply / split_pairs: plain stores, no atomics; kDzMaxSlots is their capacity).  Every workgroup of the weight
  // gradient reduces them itself (wg_dz_absmax: identical result everywhere), scales dz by wg_dz_scale(max) and
  // wgrad_reduce_launch divides the result by it again
  const float* dz_absmax = nullptr;
  int dz_absmax_n = 0;
  // split kernels, operand storage: 0 = activations fp32 + dz pre-split bf16 pair records; 1 / 2 = activations and dz
  // plain NHWC bf16 / fp16 (ldx, lddz in elements); 3 / 4 = activations fp32 (the packed image) + dz plain bf16 / fp16
  int store = 0;
  // != nullptr (split16 wave-specialised kernel only, wgrad_split_fuses_input): x is the PRE-activation tensor z of the
  // producing convolution and the loader applies its BatchNorm + ReLU on the way in — a = relu(z * in_scale[c] +
  // in_shift[c]), the arithmetic of bn_relu_fwd_kernel — so that the activated tensor is never materialised
  const float* in_scale = nullptr;
  const float* in_shift = nullptr;
};

// The launch structs of a layer from its recipe: the only code that assigns their geometry fields.  Zero elsewhere: the
// pointers, the pitches of tensors that are channel slices (ldx, ldy), stats, the epilogue and np = 2 are the caller's.
static inline ConvLaunch fill_conv_launch(const ConvRecipe& r, int dir, int N, int H, int W, int cin_p, int cout_p) {
  const bool fwd = dir == PACK_FWD;
  const ConvDir& d = fwd ? r.fwd : r.dgrad;
  ConvLaunch a{};
  a.N = N;
  a.Hi = H;
  a.Wi = W;
  a.off = fwd ? 1 : 2;  // (the data gradient lands on the reflect-padded domain)
  a.Ho = fwd ? H : H + 2;
  a.Wo = fwd ? W : W + 2;
  a.ldx = a.cin_p = fwd ? cin_p : cout_p;
  a.ldy = a.cout_store = fwd ? cout_p : cin_p;
  a.cout_pad = d.rows;
  a.pair = d.pair;
  a.wide = d.wide;
  return a;
}
static inline WgradLaunch fill_wgrad_launch(const ConvRecipe& r, int N, int H, int W, int cin_p, int cout_p) {
  WgradLaunch g{};
  g.N = N;
  g.H = H;
  g.W = W;
  g.ldx = g.cin_p = cin_p;
  g.lddz = g.cout_p = cout_p;
  g.cin_pad = r.wg_cin_pad;
  g.cout_pad = r.wg_cout_pad;
  g.splits = r.wg_splits;
  g.np = r.wg_np;
  g.store = r.wg_store;
  return g;
}

}  // namespace mimo
