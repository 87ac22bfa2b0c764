// Host-only test of mimo_unet_amd/csrc/pack_layout.h, built with -fsanitize=address,undefined by tests/test_sched_cpu.py.
//   * pack::kind / pack::conv_mode against the table below: every (precision, direction, split, wide) the plan produces
//   * pack::make_job over a sweep of layer geometries: total a multiple of 9, image elements = total x 2 for the pair
//     kinds and x 1 otherwise, pair only on the 32-channel pair kinds, map_rows <= rows_pad, the wmax word on the fp16
//     kinds only, and the largest element pack_jobs_kernel's formulas (conv_bf16x3.hip, written out again below) store
//     to for that job lies inside the image
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>

#include "../../mimo_unet_amd/csrc/pack_layout.h"
#include "../../mimo_unet_amd/csrc/tile_sched.h"

using namespace mimo;

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (failures < 20) {                    \
        std::printf("FAIL %s: ", #cond);      \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
      ++failures;                             \
    }                                         \
  } while (0)

struct Row {
  int precision, dir;
  bool split, wide;
  int kind, mode;
};
// split = false is the fp32 image of any precision (the image convolution; every layer of MIMO_PREC_FP32); the wide
// decomposition exists for split16 and the two 16-bit storage modes
static const Row kTable[] = {
    {MIMO_PREC_FP32, PACK_FWD, false, false, PK_F32, 1},
    {MIMO_PREC_FP32, PACK_DGRAD, false, false, PK_F32, 0},
    {MIMO_PREC_SPLIT16, PACK_FWD, false, false, PK_F32, 1},
    {MIMO_PREC_SPLIT16, PACK_FWD, true, false, PK_F16_PAIR, 1},
    {MIMO_PREC_SPLIT16, PACK_FWD, true, true, PK_WIDE_F16_PAIR, 1},
    {MIMO_PREC_SPLIT16, PACK_DGRAD, false, false, PK_F32, 0},
    {MIMO_PREC_SPLIT16, PACK_DGRAD, true, false, PK_BF16_PAIR, 0},
    {MIMO_PREC_SPLIT16, PACK_DGRAD, true, true, PK_WIDE_BF16_PAIR, 0},
    {MIMO_PREC_BF16, PACK_FWD, false, false, PK_F32, 2},
    {MIMO_PREC_BF16, PACK_FWD, true, false, PK_BF16_PAIR, 2},
    {MIMO_PREC_BF16, PACK_DGRAD, false, false, PK_F32, 3},
    {MIMO_PREC_BF16, PACK_DGRAD, true, false, PK_BF16_PAIR, 3},
    {MIMO_PREC_BF16_MIXED, PACK_FWD, false, false, PK_F32, 4},
    {MIMO_PREC_BF16_MIXED, PACK_FWD, true, false, PK_BF16_PAIR, 4},
    {MIMO_PREC_BF16_MIXED, PACK_FWD, true, true, PK_WIDE_BF16, 4},
    {MIMO_PREC_BF16_MIXED, PACK_DGRAD, true, false, PK_BF16_PAIR, 5},
    {MIMO_PREC_BF16_MIXED, PACK_DGRAD, true, true, PK_WIDE_BF16, 5},
    {MIMO_PREC_FP16_MIXED, PACK_FWD, false, false, PK_F32, 6},
    {MIMO_PREC_FP16_MIXED, PACK_FWD, true, false, PK_F16_PAIR, 6},
    {MIMO_PREC_FP16_MIXED, PACK_FWD, true, true, PK_WIDE_F16, 6},
    {MIMO_PREC_FP16_MIXED, PACK_DGRAD, true, false, PK_F16_PAIR, 7},
    {MIMO_PREC_FP16_MIXED, PACK_DGRAD, true, true, PK_WIDE_F16, 7},
};

static void test_table() {
  CHECK(PK_F32 == 0 && PK_F16_PAIR == 1 && PK_BF16_PAIR == 2 && PK_WIDE_F16_PAIR == 3 && PK_WIDE_BF16_PAIR == 4 && PK_WIDE_F16 == 5 &&
            PK_WIDE_BF16 == 6,
        "kind values");
  for (const Row& r : kTable) {
    const int k = pack::kind(r.precision, r.dir, r.split, r.wide), m = pack::conv_mode(r.precision, r.dir);
    CHECK(k == r.kind, "precision %d dir %d split %d wide %d: kind %d, table %d", r.precision, r.dir, r.split, r.wide, k, r.kind);
    CHECK(m == r.mode, "precision %d dir %d: mode %d, table %d", r.precision, r.dir, m, r.mode);
  }
  for (int p = MIMO_PREC_FP32; p <= MIMO_PREC_FP16_MIXED; ++p) {
    const bool mixed = p == MIMO_PREC_BF16_MIXED || p == MIMO_PREC_FP16_MIXED;
    CHECK(pack::is_mixed(p) == mixed, "precision %d", p);
    CHECK(pack::store_type(p) == (p == MIMO_PREC_BF16_MIXED ? ST_BF16 : p == MIMO_PREC_FP16_MIXED ? ST_F16 : ST_F32), "precision %d", p);
  }
}

// pack_jobs_kernel's element formulas: the largest index of j.dst (in elements of the image's type) the job stores to
static size_t max_dst_index(const PackJob& j) {
  const int per_tap = j.total / 9;
  size_t mx = 0;
  for (int i = 0; i < per_tap; ++i) {
    int row, col, k = 0, chunk = 0;
    if (j.kind == PK_F32) {
      col = i % j.cols;
      row = i / j.cols;
    } else {
      const int ck = j.kind == PK_WIDE_F16_PAIR || j.kind == PK_WIDE_BF16_PAIR ? 16 : 32;
      k = i % ck;
      const int rest = i / ck;
      row = rest % j.rows_pad;
      chunk = rest / j.rows_pad;
      col = chunk * ck + k;
    }
    const bool paired = (j.kind == PK_F16_PAIR || j.kind == PK_BF16_PAIR) && j.pair && chunk == (j.cols + 31) / 32 - 1;
    if (paired && k >= 16) continue;
    for (int tap = 0; tap < 9; ++tap) {
      int slot = tap, kk = k;
      if (paired) {  // pair_slot
        const int r = tap / 3, kw = tap - 3 * r;
        slot = r == 2 ? 3 + kw : kw;
        kk = k + (r == 1 ? 16 : 0);
      }
      size_t idx;
      if (j.kind == PK_F32)
        idx = ((size_t)tap * j.rows_pad + row) * j.cols + col;
      else if (j.kind == PK_WIDE_F16 || j.kind == PK_WIDE_BF16)
        idx = (((size_t)chunk * 9 + tap) * j.rows_pad + row) * 32 + k;
      else if (j.kind == PK_WIDE_F16_PAIR || j.kind == PK_WIDE_BF16_PAIR)
        idx = (((size_t)chunk * 9 + tap) * j.rows_pad + row) * 32 + 16 + k;  // the lo half
      else
        idx = (((size_t)chunk * 9 + slot) * j.rows_pad + row) * 64 + 32 + kk;  // the lo half
      if (idx > mx) mx = idx;
    }
  }
  return mx;
}

static void test_jobs() {
  const int chans[] = {4, 8, 16, 24, 40, 48, 96, 256, 960};
  static int row_map, col_map;  // never dereferenced
  static unsigned wmax_word;
  static float image, bias;
  std::set<std::tuple<int, int, int, int>> indexed;  // (kind, rows_pad, cols, pair) whose indices have been walked
  int jobs = 0, wide_jobs = 0;
  for (int precision = MIMO_PREC_FP32; precision <= MIMO_PREC_FP16_MIXED; ++precision)
    for (int dir : {PACK_FWD, PACK_DGRAD})
      for (int cin_p : chans)
        for (int cout_p : chans) {
          // every rows padding of the launch: the forward pads Cout (cout_p - 7 .. cout_p), the data gradient cin_p
          std::set<int> rows_set;
          if (dir == PACK_FWD)
            for (int cout = cout_p > 7 ? cout_p - 7 : 1; cout <= cout_p; ++cout) rows_set.insert(sched::conv_cout_pad(cout));
          else
            rows_set.insert(sched::conv_cout_pad(cin_p));
          const int mode = pack::conv_mode(precision, dir);
          const int cols = dir == PACK_FWD ? cin_p : cout_p, out_ch = dir == PACK_FWD ? cout_p : cin_p;
          const bool can_wide = precision == MIMO_PREC_SPLIT16 || pack::is_mixed(precision);
          const int wide_rows = can_wide ? sched::wide_config(mode, 2, cols, out_ch, 34, 34, 1).rows_pad : 0;
          for (int rows : rows_set)
            for (int split = 0; split <= (precision == MIMO_PREC_FP32 ? 0 : 1); ++split)
              for (int wide : std::set<int>{0, split ? wide_rows : 0})
                for (int pair = 0; pair <= 1; ++pair) {
                  const PackJob j = pack::make_job(dir, precision, split != 0, cout_p, cin_p, cin_p, cout_p, rows, wide, pair, &row_map, &col_map,
                                                   &image, &wmax_word, 12, 34, dir == PACK_FWD ? &bias : nullptr);
                  ++jobs;
                  wide_jobs += wide != 0;
                  const bool pair_kind = j.kind >= PK_F16_PAIR && j.kind <= PK_WIDE_BF16_PAIR;
                  const size_t elems = pack::image_elems(j.kind, j.rows_pad, j.cols);
#define WHERE "precision %d dir %d %d -> %d rows %d wide %d split %d pair %d", precision, dir, cin_p, cout_p, rows, wide, split, pair
                  CHECK(j.kind == pack::kind(precision, dir, split != 0, wide != 0), WHERE);
                  CHECK(j.total > 0 && j.total % 9 == 0 && j.total == pack::total(j.kind, j.rows_pad, j.cols), WHERE);
                  CHECK(elems == (size_t)j.total * (pair_kind ? 2 : 1), WHERE);
                  CHECK(!j.pair || j.kind == PK_F16_PAIR || j.kind == PK_BF16_PAIR, WHERE);
                  CHECK(j.pair == ((j.kind == PK_F16_PAIR || j.kind == PK_BF16_PAIR) ? pair : 0), WHERE);
                  CHECK(j.map_rows == rows && j.map_rows <= j.rows_pad && j.rows_pad == (wide ? wide : rows), WHERE);
                  CHECK(j.transposed == (dir == PACK_DGRAD) && j.cols == cols && j.cout == cout_p && j.cin == cin_p, WHERE);
                  CHECK((j.wmax != nullptr) == (j.kind == PK_F16_PAIR || j.kind == PK_WIDE_F16_PAIR || j.kind == PK_WIDE_F16), WHERE);
                  CHECK(j.bias_n == (dir == PACK_FWD ? cout_p : 0) && j.w_off == 12 && j.bias_off == 34 && j.dst == &image, WHERE);
                  if (indexed.insert(std::make_tuple(j.kind, j.rows_pad, j.cols, j.pair)).second) {
                    const size_t mx = max_dst_index(j);
                    CHECK(mx < elems, WHERE);
                    // ... and the image is no larger than the walk needs, whole chunk rows apart (the paired tail leaves slots unused)
                    CHECK(j.pair || mx + 1 == elems, WHERE);
                  }
#undef WHERE
                }
        }
  CHECK(jobs > 2000 && wide_jobs > 200, "sweep of %d jobs, %d wide", jobs, wide_jobs);
  std::printf("%d jobs (%d wide), %zu distinct images walked\n", jobs, wide_jobs, indexed.size());
}

int main() {
  test_table();
  test_jobs();
  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
