// Host-only test of mimo_unet_amd/csrc/conv_recipe.h, built with -fsanitize=address,undefined by tests/test_sched_cpu.py.
// tests/golden/conv_recipe_parent_table.inc holds, row by row, what the code conv_recipe replaced decided: plan.hip's
// init_convbn, convbn_forward, dgrad_conv and wgrad_issue of the commit before it, evaluated by a program linked against
// that commit's own helper functions (conv3x3_wide_rows, conv3x3_pair_tail, wgrad_split_pick_splits, ...) — every 3 x 3
// convolution of cfg2, cfg3 and cfg4 at the benchmark's batches (64, 32, 16; cfg3 also at 4 images, where the benchmark is
// launch-bound), with the CU count their plans size the weight gradient for, and the CONV_CASES of tests/test_ops_gpu.py
// (256 CUs; the image layers also behind a permuted input map),
// in the five precisions, with the plain-FMA image kernels and the wave-specialised convolution kernels on and off.  A row
// holds for the settings in its `envs` mask (bit 2 x thin + ws): settings that decide the same share a row, and every layer
// and precision has all four.
// For split16, whose K-split scratch and two-MFMA weight gradient depend on it, also as an inference-only and an
// input-gradient-only plan (inference_only 1 / 2).
//   * conv_recipe gives every row's decisions
//   * fill_conv_launch / fill_wgrad_launch (conv_launch.h) put them into the launch structs, with the layer's geometry and
//     nothing else, and the pack job built from the same recipe (pack::make_job, as build() and the entry points call it)
//     carries the pair tail, the wide rows, the rows and the columns of that launch: what the weight image is laid out for is
//     what the kernel is told
//   * the weight gradient's split count (sched::wg_pick_splits through conv_recipe) at the 128, 192 and 256 CUs the plans
//     size it for, on every table geometry at every per-GPU batch of the benchmark's shards and on the cases of
//     tests/test_wgrad_splits_gpu.py: 1 <= splits <= min(tiles, 1024), no split of the strided tile walk without a tile, and
//     the slabs the reduction writes behind them fit the splits + splits / 8 + 2 slabs the plan and the entry points
//     allocate — the last also for every split count 1..1024 with both final fans, whatever the picker picks
#include <cstdio>
#include <initializer_list>

#include "../../mimo_unet_amd/csrc/conv_launch.h"

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

struct DirRow {
  int mode, split, rows, wide, pair;
  size_t kpart;
};
struct Row {
  int precision, envs, inference_only;
  int N, H, W, Cin, Cout, cin_p, ident, wg_cus;
  DirRow fwd, dgrad;
  int thin, dtz;
  int wg_split, wg_cin_pad, wg_cout_pad, wg_splits, wg_store, wg_np, wg_np2, wg_thin;
};
static const Row kTable[] = {
#include "../golden/conv_recipe_parent_table.inc"
};

static void check_dir(const Row& t, int row, int dir, const ConvRecipe& r, const DirRow& want) {
  const char* name = dir == PACK_FWD ? "forward" : "data gradient";
  const ConvDir& d = dir == PACK_FWD ? r.fwd : r.dgrad;
  CHECK(d.mode == want.mode && (int)d.split == want.split && d.rows == want.rows && d.wide == want.wide && d.pair == want.pair &&
            d.kpart == want.kpart,
        "row %d %s: mode %d split %d rows %d wide %d pair %d kpart %zu, the table has %d %d %d %d %d %zu", row, name, d.mode, (int)d.split,
        d.rows, d.wide, d.pair, d.kpart, want.mode, want.split, want.rows, want.wide, want.pair, want.kpart);
  // the launch struct as the plan and the entry points fill it, against the table and against the pack job of the same recipe
  const int cout_p = sched::rup(t.Cout, 8);
  const ConvLaunch a = fill_conv_launch(r, dir, t.N, t.H, t.W, t.cin_p, cout_p);
  const PackJob j = pack::make_job(dir, t.precision, d.split, t.Cout, t.Cin, t.cin_p, cout_p, d.rows, d.wide, d.pair, nullptr, nullptr,
                                   nullptr, nullptr, 0);
  const bool job_wide = j.kind >= PK_WIDE_F16_PAIR;
  CHECK(a.pair == want.pair && a.wide == want.wide && a.cout_pad == want.rows, "row %d %s: the launch has pair %d wide %d rows %d, the table %d %d %d",
        row, name, a.pair, a.wide, a.cout_pad, want.pair, want.wide, want.rows);
  CHECK(j.pair == a.pair && job_wide == (a.wide != 0) && j.rows_pad == (a.wide ? a.wide : a.cout_pad) && j.map_rows == a.cout_pad && j.cols == a.cin_p,
        "row %d %s: the pack job has pair %d kind %d rows %d cols %d, the launch pair %d wide %d rows %d cin_p %d", row, name, j.pair, j.kind,
        j.rows_pad, j.cols, a.pair, a.wide, a.cout_pad, a.cin_p);
  const int ho = dir == PACK_FWD ? t.H : t.H + 2, wo = dir == PACK_FWD ? t.W : t.W + 2;
  CHECK(a.N == t.N && a.Hi == t.H && a.Wi == t.W && a.Ho == ho && a.Wo == wo && a.off == (dir == PACK_FWD ? 1 : 2) &&
            a.cin_p == (dir == PACK_FWD ? t.cin_p : cout_p) && a.cout_store == (dir == PACK_FWD ? cout_p : t.cin_p) && a.ldx == a.cin_p &&
            a.ldy == a.cout_store && a.ksplit == 1 && !a.x && !a.y && !a.w && !a.wpk && !a.bias && !a.stats,
        "row %d %s: launch geometry", row, name);
}

// slabs wgrad_reduce_launch (conv3x3.hip) writes behind the `splits` slabs of the weight-gradient kernel: stage A sums groups
// of 16 into the slabs behind its inputs until <= final_fan slabs are left (16 with >= 512 blocks in the last kernel, else 1)
static int reduce_extra_slabs(int splits, int final_fan) {
  int extra = 0;
  for (int n = splits; n > final_fan;) {
    n = sched::cdiv(n, 16);
    extra += n;
  }
  return extra;
}

static void check_wg_splits(int precision, int N, int H, int W, int Cin, int Cout, int cin_p, long* checked, long* below_256_differs) {
  const int cout_p = sched::rup(Cout, 8);
  int at256 = 0;
  for (const int cus : {256, 192, 128})
    for (const bool ws : {true, false}) {
      ConvEnv e;
      e.wgrad_ws = ws;
      e.wg_cus = cus;
      const ConvRecipe r = conv_recipe(precision, 0, N, H, W, Cin, Cout, cin_p, cout_p, true, e);
      if (!r.wg_split) return;
      int CI, CO;
      sched::wg_tiles(cin_p, cout_p, ws, &CI, &CO);
      const bool s16 = r.wg_store == 1 || r.wg_store == 2;
      const int tiles = sched::wg_num_tiles(N, H, W, sched::wg_use_ws(CI, CO, ws) ? sched::wg_ws_tr(CI, s16) : 4);
      const int s = r.wg_splits;
      CHECK(s >= 1 && s <= tiles && s <= 1024, "prec %d %dx%dx%d %d->%d at %d CUs ws %d: %d splits of %d tiles", precision, N, H, W, Cin, Cout,
            cus, (int)ws, s, tiles);
      if (s < 1) continue;
      // wgrad_split_ws_kernel: split b owns tiles b, b + s, ...: (tiles - 1 - b) / s + 1 of them; the last split the fewest
      CHECK(s - 1 < tiles && (tiles - 1 - (s - 1)) / s + 1 >= 1, "prec %d %dx%dx%d %d->%d at %d CUs: the last of %d splits owns no tile of %d",
            precision, N, H, W, Cin, Cout, cus, s, tiles);
      const int blocks = sched::cdiv(r.wg_cin_pad, 32) * sched::cdiv(r.wg_cout_pad, 8);
      const int extra = reduce_extra_slabs(s, blocks >= 512 ? 16 : 1);
      CHECK(extra <= s / 8 + 2, "prec %d %dx%dx%d %d->%d at %d CUs: %d splits, %d reduction blocks: %d stage-A slabs > %d", precision, N, H, W,
            Cin, Cout, cus, s, blocks, extra, s / 8 + 2);
      ++*checked;
      if (ws && cus == 256) at256 = s;
      if (ws && cus != 256 && s != at256) ++*below_256_differs;
    }
}

static void test_wg_splits() {
  // the sizing rule itself, independent of the picker: every stage-A output of any split count fits splits / 8 + 2 slabs
  for (int s = 1; s <= 1024; ++s) {
    int all_stages = 0;  // ceil(s / 16) + ceil(s / 256) + ... down to one slab
    for (int n = s; n > 1;) {
      n = sched::cdiv(n, 16);
      all_stages += n;
    }
    CHECK(all_stages <= s / 8 + 2 && reduce_extra_slabs(s, 1) == all_stages && reduce_extra_slabs(s, 16) <= all_stages,
          "%d splits: %d / %d stage-A slabs (final fan 1 / 16), %d allocated", s, reduce_extra_slabs(s, 1), reduce_extra_slabs(s, 16), s / 8 + 2);
  }
  long checked = 0, differs = 0;
  const int precisions[] = {MIMO_PREC_SPLIT16, MIMO_PREC_BF16, MIMO_PREC_BF16_MIXED, MIMO_PREC_FP16_MIXED};
  // every geometry of the table (the benchmark's layers and the CONV_CASES) at the table's batch and at every per-GPU batch
  // of the benchmark's shards
  const int rows = (int)(sizeof(kTable) / sizeof(kTable[0]));
  for (int i = 0; i < rows; ++i) {
    const Row& t = kTable[i];
    if (t.precision != MIMO_PREC_SPLIT16 || t.inference_only != 0 || !(t.envs & 8)) continue;  // one row per geometry
    for (const int N : {t.N, 2, 4, 8, 16, 32, 64})
      for (const int p : precisions) check_wg_splits(p, N, t.H, t.W, t.Cin, t.Cout, t.cin_p, &checked, &differs);
  }
  // the cases of tests/test_wgrad_splits_gpu.py
  static const int kCases[][5] = {{4, 64, 96, 30, 30},    {3, 40, 72, 90, 45},   {3, 68, 96, 30, 30},      {1, 16, 16, 480, 480},
                                  {2, 16, 16, 240, 240},  {2, 32, 16, 240, 240}, {2, 50, 70, 84, 42},      {1, 8, 8, 960, 480},
                                  {7, 20, 33, 60, 60},    {2, 86, 512, 264, 520}, {5, 28, 544, 264, 520},  {3, 40, 72, 60, 45},
                                  {3, 40, 72, 60, 30},    {3, 40, 72, 90, 60}};
  for (const auto& c : kCases)
    for (const int p : precisions) check_wg_splits(p, c[0], c[1], c[2], c[3], c[4], sched::rup(c[3], 8), &checked, &differs);
  CHECK(checked > 1000 && differs > 100, "%ld split counts checked, %ld of them other than at 256 CUs", checked, differs);
  std::printf("%ld weight-gradient split counts, %ld of them other than the one at 256 CUs\n", checked, differs);
}

int main() {
  test_wg_splits();
  const int rows = (int)(sizeof(kTable) / sizeof(kTable[0]));
  int thin_rows = 0, wide_rows = 0, pair_rows = 0, ksplit_rows = 0, np2_rows = 0;
  int covered = 0;
  for (int i = 0, n = 4 * rows; i < n; ++i) {
    const Row& t = kTable[i / 4];
    const int bit = i % 4;
    if (!(t.envs >> bit & 1)) continue;
    ++covered;
    ConvEnv e;
    e.thin = (bit & 2) != 0;
    e.conv_ws = (bit & 1) != 0;
    e.wg_cus = t.wg_cus;
    const ConvRecipe r = conv_recipe(t.precision, t.inference_only, t.N, t.H, t.W, t.Cin, t.Cout, t.cin_p, sched::rup(t.Cout, 8), t.ident != 0, e);
    check_dir(t, i / 4, PACK_FWD, r, t.fwd);
    check_dir(t, i / 4, PACK_DGRAD, r, t.dgrad);
    CHECK((int)r.thin == t.thin && r.dtz == t.dtz, "row %d: thin %d dtz %d, the table has %d %d", i / 4, (int)r.thin, r.dtz, t.thin, t.dtz);
    CHECK((int)r.wg_split == t.wg_split && r.wg_cin_pad == t.wg_cin_pad && r.wg_cout_pad == t.wg_cout_pad && r.wg_splits == t.wg_splits &&
              r.wg_store == t.wg_store && (int)r.wg_np2 == t.wg_np2 && (!r.wg_split || r.wg_np == t.wg_np),
          "row %d weight gradient: split %d pads %d x %d splits %d store %d np %d np2 %d, the table has %d %d x %d %d %d %d %d", i / 4,
          (int)r.wg_split, r.wg_cin_pad, r.wg_cout_pad, r.wg_splits, r.wg_store, r.wg_np, (int)r.wg_np2, t.wg_split, t.wg_cin_pad,
          t.wg_cout_pad, t.wg_splits, t.wg_store, t.wg_np, t.wg_np2);
    CHECK((int)r.wg_thin == t.wg_thin, "row %d: wg_thin %d, the table has %d", i / 4, (int)r.wg_thin, t.wg_thin);
    const WgradLaunch g = fill_wgrad_launch(r, t.N, t.H, t.W, t.cin_p, sched::rup(t.Cout, 8));
    CHECK(g.cin_pad == t.wg_cin_pad && g.cout_pad == t.wg_cout_pad && g.splits == t.wg_splits && g.store == t.wg_store &&
              (!r.wg_split || g.np == t.wg_np) && g.N == t.N && g.H == t.H && g.W == t.W && g.cin_p == t.cin_p && g.ldx == t.cin_p &&
              g.cout_p == sched::rup(t.Cout, 8) && g.lddz == g.cout_p && !g.dz_absmax,
          "row %d: weight-gradient launch pads %d x %d splits %d store %d np %d", i / 4, g.cin_pad, g.cout_pad, g.splits, g.store, g.np);
    thin_rows += r.thin;
    wide_rows += (r.fwd.wide != 0) + (r.dgrad.wide != 0);
    pair_rows += r.fwd.pair + r.dgrad.pair;
    ksplit_rows += (r.fwd.kpart != 0) + (r.dgrad.kpart != 0);
    np2_rows += r.wg_np2;
  }
  // the table reaches every decision it is there to pin
  CHECK(covered == 101 * (5 * 4 + 2) && thin_rows > 0 && wide_rows > 0 && pair_rows > 0 && ksplit_rows > 0 && np2_rows > 0,
        "%d decisions: thin %d wide %d pair %d ksplit %d np2 %d", covered, thin_rows, wide_rows, pair_rows, ksplit_rows, np2_rows);
  std::printf("%d decisions: thin %d, wide %d, pair %d, K split %d, two-MFMA weight gradient %d\n", covered, thin_rows, wide_rows, pair_rows,
              ksplit_rows, np2_rows);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
