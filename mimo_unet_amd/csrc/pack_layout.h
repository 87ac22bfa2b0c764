// The packed weight images of the 3x3 convolutions, described once: which layout a precision and direction reads, how
// large it is, and the job record that pack_jobs_kernel (conv_bf16x3.hip) writes it from.  The plan (one table for all
// layers) and the per-operator entry points (a table of one job) build their jobs here.  Host-only, no HIP dependency:
// tests/host/pack_layout_test.cpp compiles this header with g++ -fsanitize=address,undefined (tests/test_sched_cpu.py).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/mimo_hip.h"

namespace mimo {

// Element type of the activation-like tensors in HBM (conv outputs, activations and their gradients): fp32, or bf16 /
// fp16 in the 16-bit storage modes MIMO_PREC_BF16_MIXED / MIMO_PREC_FP16_MIXED.  Arithmetic is always fp32.
enum StoreType { ST_F32 = 0, ST_BF16 = 1, ST_F16 = 2 };

// Layout of a packed image (rows = output channels of the launch, cols = its input channels, tap = kh * 3 + kw):
enum PackKind {
  PK_F32 = 0,             // fp32 [tap][rows_pad][cols]
  PK_F16_PAIR = 1,        // fp16 (hi, lo) pairs [32-channel chunk][tap][rows_pad][hi 32 | lo 32]
  PK_BF16_PAIR = 2,       // bf16 pairs, same layout (the single-MFMA modes read hi only)
  PK_WIDE_F16_PAIR = 3,   // conv_wide.hip: fp16 pairs [16-channel chunk][tap][rows_pad][hi 16 | lo 16]
  PK_WIDE_BF16_PAIR = 4,  // ... bf16 pairs
  PK_WIDE_F16 = 5,        // conv_wide.hip, 16-bit storage modes: fp16 single values [32-channel chunk][tap][rows_pad][32]
  PK_WIDE_BF16 = 6,       // ... bf16 single values
};
// The fp16 kinds carry a power-of-two scale: w16_scale(*wmax), or the fixed 2^8 without a wmax word.  Wide kinds: rows
// beyond map_rows are zero.

enum PackDir { PACK_FWD = 0, PACK_DGRAD = 1 };  // PACK_DGRAD: the transposed image (rows = input channels, taps flipped)

// One repack of pack_jobs_kernel (blockIdx.y = job).  Plain C members: the table is copied to the device as bytes.
struct PackJob {
  int64_t w_off, bias_off;  // float offsets into the bound parameter buffer
  void* dst;
  float* bias_dst;
  const int *row_map, *col_map;  // row / column -> logical channel of the OIHW tensor, -1 = zero padding
  int kind, cout, cin, rows_pad, cols, transposed, total, bias_n;  // bias_n > 0: the layer's bias is copied as well
  int pair;  // PK_F16_PAIR / PK_BF16_PAIR: tap-paired image of the last chunk (ConvDir::pair, conv_recipe.h)
  int map_rows;  // entries of row_map (wide kinds: rows_pad may exceed it)
  unsigned* wmax;  // fp16 kinds: max |w| of the layer at this pack, float bits (wabsmax_jobs_launch); image scale = w16_scale
};

namespace pack {

static inline bool is_mixed(int precision) { return precision == MIMO_PREC_BF16_MIXED || precision == MIMO_PREC_FP16_MIXED; }
static inline int store_type(int precision) {
  return precision == MIMO_PREC_BF16_MIXED ? ST_BF16 : precision == MIMO_PREC_FP16_MIXED ? ST_F16 : ST_F32;
}

// mode of conv3x3_bf16x3_launch / conv3x3_wide_launch: forward 1 split16 (fp16 pairs), 2 bf16, 4 bf16-mixed, 6 16-mixed;
// data gradient 0 split16 (bf16 pairs, pre-split input), 3 bf16, 5 bf16-mixed, 7 16-mixed
static inline int conv_mode(int precision, int dir) {
  const bool fwd = dir == PACK_FWD;
  switch (precision) {
    case MIMO_PREC_BF16: return fwd ? 2 : 3;
    case MIMO_PREC_BF16_MIXED: return fwd ? 4 : 5;
    case MIMO_PREC_FP16_MIXED: return fwd ? 6 : 7;
    default: return fwd ? 1 : 0;
  }
}

// split: the launch runs on the 16-bit MFMA kernels (else the fp32 image); wide: on conv_wide.hip
static inline int kind(int precision, int dir, bool split, bool wide) {
  if (!split) return PK_F32;
  if (wide) {
    if (!is_mixed(precision)) return dir == PACK_FWD ? PK_WIDE_F16_PAIR : PK_WIDE_BF16_PAIR;
    return precision == MIMO_PREC_FP16_MIXED ? PK_WIDE_F16 : PK_WIDE_BF16;
  }
  // forward: split16 / 16-mixed multiply fp16 pairs (x 2^8), bf16 / bf16-mixed bf16; data gradient: fp16 in 16-mixed only
  if (dir == PACK_FWD) return (precision == MIMO_PREC_BF16 || precision == MIMO_PREC_BF16_MIXED) ? PK_BF16_PAIR : PK_F16_PAIR;
  return precision == MIMO_PREC_FP16_MIXED ? PK_F16_PAIR : PK_BF16_PAIR;
}
static inline bool kind_is_f16(int k) { return k == PK_F16_PAIR || k == PK_WIDE_F16_PAIR || k == PK_WIDE_F16; }
static inline bool kind_is_pair(int k) { return k >= PK_F16_PAIR && k <= PK_WIDE_BF16_PAIR; }
static inline int kind_chunk(int k) { return k == PK_WIDE_F16_PAIR || k == PK_WIDE_BF16_PAIR ? 16 : 32; }  // channels per chunk

// weights the kernel walks: 9 taps x rows x the columns, padded to whole chunks in the 16-bit layouts
static inline int total(int k, int rows_pad, int cols) {
  return k == PK_F32 ? 9 * rows_pad * cols : (cols + kind_chunk(k) - 1) / kind_chunk(k) * 9 * rows_pad * kind_chunk(k);
}
// elements of the image: floats (PK_F32) or 16-bit values (a pair is two)
static inline size_t image_elems(int k, int rows_pad, int cols) { return (size_t)total(k, rows_pad, cols) * (kind_is_pair(k) ? 2 : 1); }

// The job that packs one layer's image for a direction.  rows: padded output channels of the launch = entries of
// row_map (ConvDir::rows: forward conv3x3_cout_pad(Cout); data gradient conv3x3_cout_pad(cin_p)); wide_rows: ConvDir::wide, 0 =
// none; pair: ConvDir::pair.  bias_dst != nullptr (forward): Cout floats at bias_off are copied there.  wmax is kept
// for the fp16 kinds only.
static inline PackJob make_job(int dir, int precision, bool split, int Cout, int Cin, int cin_p, int cout_p, int rows, int wide_rows,
                               int pair, const int* row_map, const int* col_map, void* dst, unsigned* wmax, int64_t w_off,
                               int64_t bias_off = 0, float* bias_dst = nullptr) {
  PackJob j{};
  j.w_off = w_off;
  j.bias_off = bias_off;
  j.dst = dst;
  j.bias_dst = bias_dst;
  j.bias_n = bias_dst ? Cout : 0;
  j.row_map = row_map;
  j.col_map = col_map;
  j.cout = Cout;
  j.cin = Cin;
  j.transposed = dir == PACK_DGRAD;
  j.cols = dir == PACK_FWD ? cin_p : cout_p;
  j.kind = kind(precision, dir, split, split && wide_rows != 0);
  j.map_rows = rows;
  j.rows_pad = j.kind >= PK_WIDE_F16_PAIR ? wide_rows : rows;
  j.total = total(j.kind, j.rows_pad, j.cols);
  j.pair = (j.kind == PK_F16_PAIR || j.kind == PK_BF16_PAIR) ? pair : 0;
  j.wmax = kind_is_f16(j.kind) ? wmax : nullptr;
  return j;
}

}  // namespace pack
}  // namespace mimo
