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
#include <cstdio>

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

int main() {
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
