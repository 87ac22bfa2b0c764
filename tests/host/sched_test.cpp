// Host-only sweep of the schedulers in mimo_unet_amd/csrc/tile_sched.h, built with -fsanitize=address,undefined by
// tests/test_sched_cpu.py (race / memory tooling of the host side).
//   * xcd_virtual_index: a bijection on [0, total) for every grid size 1 .. 4096, every XCD a contiguous range
//   * pick_tile_n: for every H, W in 1 .. 300 and both tile sizes, the tiles cover every pixel exactly once, fit the
//     pixel budget and the LDS halo budget
//   * wide_config / wide_grid_x: geometry invariants for every BASELINE layer at N in {1, 2, 4, 16, 32, 64}
//   * weight-gradient channel tiles / split counts: >= 1, slabs within the plan's scratch formula
//   * conv_cout_pad: covers the channels, multiple of the fragment width
//   * w16_scale / wg_dz_scale (round 5): exact powers of two, reciprocal pairs, scaled maxima inside fp16's range
//   * 256-pixel split convolution (split_config, split_pick_ksplit, ws_tail_pairs, split_fuses_input)
//     and wide_config: equal, field by field, to the launch code they replaced (namespace frozen below) over a sweep of
//     modes, switches, batches, domains and channel counts; grid invariants over the same sweep
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../mimo_unet_amd/csrc/tile_sched.h"

using namespace mimo::sched;

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

static void test_xcd() {
  std::vector<int> seen;
  for (int total = 1; total <= 4096; ++total) {
    seen.assign(total, 0);
    for (int lin = 0; lin < total; ++lin) {
      const int v = xcd_virtual_index(lin, total);
      CHECK(v >= 0 && v < total, "total %d linear %d -> %d", total, lin, v);
      if (v >= 0 && v < total) ++seen[v];
    }
    for (int v = 0; v < total; ++v) CHECK(seen[v] == 1, "total %d: virtual index %d hit %d times", total, v, seen[v]);
    // every XCD (linear % 8) owns one contiguous, increasing range
    for (int k = 0; k < 8 && k < total; ++k) {
      int prev = -1;
      for (int lin = k; lin < total; lin += 8) {
        const int v = xcd_virtual_index(lin, total);
        CHECK(prev < 0 || v == prev + 1, "total %d xcd %d: %d after %d", total, k, v, prev);
        prev = v;
      }
    }
  }
}

static void test_tiles() {
  const int cfgs[3][2] = {{256, 360}, {512, 640}, {128, 180}};
  std::vector<unsigned char> cover;
  for (auto& c : cfgs)
    for (int H = 1; H <= 300; ++H)
      for (int W = 1; W <= 300; ++W) {
        int TR = 0, TC = 0;
        pick_tile_n(H, W, c[0], c[1], &TR, &TC);
        CHECK(TR >= 1 && TC >= 1 && TR * TC <= c[0], "%dx%d npix %d: tile %dx%d", H, W, c[0], TR, TC);
        CHECK((TR + 2) * (TC + 2) <= c[1], "%dx%d: halo %d > %d", H, W, (TR + 2) * (TC + 2), c[1]);
        if (TR < 1 || TC < 1) continue;
        if ((H * 7 + W) % 5 != 0 && !(H <= 40 && W <= 40)) continue;  // full cover check on a fifth of the sizes
        cover.assign((size_t)H * W, 0);
        const int ty = cdiv(H, TR), tx = cdiv(W, TC);
        for (int a = 0; a < ty; ++a)
          for (int b = 0; b < tx; ++b)
            for (int i = 0; i < TR * TC; ++i) {
              const int y = a * TR + i / TC, x = b * TC + i % TC;
              if (y < H && x < W) ++cover[(size_t)y * W + x];
            }
        for (size_t i = 0; i < cover.size(); ++i)
          if (cover[i] != 1) {
            CHECK(false, "%dx%d tile %dx%d: pixel %zu covered %d times", H, W, TR, TC, i, cover[i]);
            break;
          }
      }
}

// ---- The launch rules of conv_bf16x3.hip and wide_config as they stood before they moved into tile_sched.h, written
// out plainly: the split convolution's private dispatch (launch_ws, launch_bf16x3, conv3x3_split_dispatch,
// conv3x3_ksplit, conv3x3_pair_tail, conv3x3_split_fuses_input) with its
// environment switches as arguments, and wide_config with its literals.  Frozen: a deliberate change of a rule changes
// this copy with it.
namespace frozen {
static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

static int pair_tail(int mode, int cin_p, int Ho, int Wo, bool ws_enabled) {
  if (mode < 0 || mode > 1 || !ws_enabled || Ho * Wo < 256) return 0;
  const int tail = cin_p - 32 * (cdiv(cin_p, 32) - 1);
  return tail <= 16 ? 1 : 0;
}
static int fuses_input(int mode, int wide, int Ho, int Wo, bool ws_enabled) {
  return mode == 1 && (wide != 0 || (ws_enabled && Ho * Wo >= 256)) ? 1 : 0;
}

struct Launch {
  bool ws;
  int MF, NF, TR, TC, tilesY, tilesX, gx, coTiles, rows;
};
// launch_ws<NF, MODE, MF>: tile of 64 MF pixels in 360 / 180 LDS rows, grid = gx * coTiles * ksplit
static Launch launch_ws(int NF, int MF, int N, int cout_pad, int Ho, int Wo, int a_ksplit) {
  Launch l;
  l.ws = true, l.MF = MF, l.NF = NF;
  pick_tile_n(Ho, Wo, 64 * MF, MF == 4 ? 360 : 180, &l.TR, &l.TC);
  l.tilesY = cdiv(Ho, l.TR), l.tilesX = cdiv(Wo, l.TC);
  const int numTiles = N * l.tilesY * l.tilesX;
  l.coTiles = cout_pad / (NF * 16);
  const int kWgPerCU = (MF == 2 && NF <= 2) ? 2 : 1;
  const int ksplit = a_ksplit > 1 ? a_ksplit : 1;
  int gx = imax(1, 256 * kWgPerCU / (l.coTiles * ksplit));
  if (gx > numTiles) gx = numTiles;
  const int per = cdiv(numTiles, gx);
  gx = cdiv(numTiles, per);
  l.rows = gx;
  l.gx = gx;
  return l;
}
// launch_bf16x3<MF, NF, MODE>: tile of 128 MF pixels in 640 / 360 LDS rows, grid = (tiles, channel tiles)
static Launch launch_bf16x3(int MF, int NF, int N, int cout_pad, int Ho, int Wo) {
  Launch l;
  l.ws = false, l.MF = MF, l.NF = NF;
  pick_tile_n(Ho, Wo, 8 * MF * 16, MF == 4 ? 640 : 360, &l.TR, &l.TC);
  l.tilesY = cdiv(Ho, l.TR), l.tilesX = cdiv(Wo, l.TC);
  l.rows = N * l.tilesY * l.tilesX;
  l.gx = N * l.tilesY * l.tilesX;
  l.coTiles = cout_pad / (NF * 16);
  return l;
}
static Launch dispatch(int mode, int N, int cout_pad, int Ho, int Wo, int a_ksplit, bool ws_enabled) {
  const int nfr = cout_pad / 16;
  int nf = 4;
  while (nfr % nf != 0) --nf;
  if (ws_enabled && Ho * Wo >= 256) {
    if (a_ksplit <= 1) {
      int TR, TC;
      pick_tile_n(Ho, Wo, 256, 360, &TR, &TC);
      const int numTiles = N * cdiv(Ho, TR) * cdiv(Wo, TC);
      long best = -1;
      for (int c = 4; c >= 1; --c) {
        if (nfr % c) continue;
        const int gx = imax(1, imin(numTiles, 256 / (nfr / c)));
        const long cost = (long)cdiv(numTiles, gx) * (1 + c);
        if (best < 0 || cost < best) best = cost, nf = c;
      }
    }
    const bool mf2 = (mode == 1 || mode == 2 || mode == 4 || mode == 6);
    switch (nf) {
      case 4: return launch_ws(4, 4, N, cout_pad, Ho, Wo, a_ksplit);
      case 3: return launch_ws(3, 4, N, cout_pad, Ho, Wo, a_ksplit);
      case 2: return launch_ws(2, mf2 ? 2 : 4, N, cout_pad, Ho, Wo, a_ksplit);
      default: return launch_ws(1, mf2 ? 2 : 4, N, cout_pad, Ho, Wo, a_ksplit);
    }
  }
  const bool use_big_tile = Ho * Wo >= 1024;
  return launch_bf16x3(use_big_tile && nf >= 3 ? 4 : 2, nf, N, cout_pad, Ho, Wo);
}

static int ksplit(int mode, int N, int cin_p, int cout_pad, int Ho, int Wo, bool ws_enabled, int force) {
  if (force == 0 || (mode != 0 && mode != 1) || !ws_enabled || Ho * Wo < 256 || cin_p % 32 != 0 || cout_pad % 16 != 0) return 1;
  const int nchunks = cin_p / 32;
  if (nchunks < 2) return 1;
  auto legal = [&](int ks) { return ks >= 2 && cdiv(nchunks, ks) * (ks - 1) < nchunks; };
  if (force >= 2) {
    int ks = imin(force, nchunks);
    while (ks >= 2 && !legal(ks)) --ks;
    return ks >= 2 ? ks : 1;
  }
  int TR, TC;
  pick_tile_n(Ho, Wo, 256, 360, &TR, &TC);
  const int numTiles = N * cdiv(Ho, TR) * cdiv(Wo, TC);
  const int nfr = cout_pad / 16;
  long unsplit = -1;
  for (int c = 4; c >= 1; --c) {
    if (nfr % c) continue;
    const int gx = imax(1, imin(numTiles, 256 / (nfr / c)));
    const long cost = (long)cdiv(numTiles, gx) * (1 + c) * nchunks * 3;
    if (unsplit < 0 || cost < unsplit) unsplit = cost;
  }
  int nf = 4;
  while (nfr % nf != 0) --nf;
  const int coTiles = nfr / nf;
  int best = 1;
  long best_cost = -1;
  for (int ks = 2; ks <= 8 && ks <= nchunks; ++ks) {
    if (!legal(ks) || coTiles * ks > 256) continue;
    const int gx = imax(1, imin(numTiles, 256 / (coTiles * ks)));
    const long cost = (long)cdiv(numTiles, gx) * (1 + nf) * cdiv(nchunks, ks) * 3 + 14;
    if (best_cost < 0 || cost < best_cost) best_cost = cost, best = ks;
  }
  return (best_cost >= 0 && best_cost * 100 < unsplit * 85) ? best : 1;
}
static size_t ksplit_scratch(int mode, int N, int cin_p, int cout_pad, int Ho, int Wo, int ldy, bool ws_enabled, int force) {
  const int ks = ksplit(mode, N, cin_p, cout_pad, Ho, Wo, ws_enabled, force);
  return ks > 1 ? (size_t)ks * N * Ho * Wo * ldy : 0;
}
// rows the plan's cap_partial holds for a layer: max(conv3x3_stat_rows, conv3x3_ws_stat_rows)
static int stat_rows(int N, int Ho, int Wo) {
  int TR, TC;
  pick_tile_n(Ho, Wo, 256, 360, &TR, &TC);
  return N * cdiv(Ho, TR) * cdiv(Wo, TC);
}
static int ws_stat_rows() { return 512 * 4; }

static int wide_grid_x(int numTiles, int cotiles) {
  int gx = 256 / cotiles;
  if (gx < 1) gx = 1;
  if (gx > numTiles) gx = numTiles;
  const int per = cdiv(numTiles, gx);
  return cdiv(numTiles, per);
}
static WideCfg wide_config(int mode, int N, int cin_p, int rows, int Ho, int Wo, int force) {
  WideCfg c{0, 0, 0, 0};
  const bool s16 = mode >= 4 && mode <= 7;
  if (force < 0 || !(mode == 0 || mode == 1 || s16) || rows < 1 || cin_p < 16 || Ho < 2 || Wo < 2) return c;
  if (s16 && cin_p % 8 != 0) return c;
  if (mode == 0 && rows % 8 != 0) return c;
  if (int64_t(Ho + 2) * int64_t(Wo + 2) * int64_t(cin_p < rows ? rows : cin_p) * 8 > int64_t(INT32_MAX)) return c;
  int TR, TC;
  pick_tile_n(Ho, Wo, 512, 640, &TR, &TC);
  if ((TR + 2) * (TC + 2) > 640) return c;
  const int tiles = N * cdiv(Ho, TR) * cdiv(Wo, TC);
  const double eff = double(N) * Ho * Wo / (double(tiles) * 512);
  const int r32 = cdiv(rows, 32);
  const int nf = (r32 >= 2 && double(rup(r32, 2)) / r32 <= 1.10 + 1e-9) ? 2 : 1;
  const int cotiles = cdiv(r32, nf);
  if (force == 0) {
    const int k16 = rup(cin_p, s16 ? 32 : 16);
    int TRo, TCo;
    pick_tile_n(Ho, Wo, 256, 360, &TRo, &TCo);
    const double eff_o = double(Ho) * Wo / (double(cdiv(Ho, TRo)) * cdiv(Wo, TCo) * 256);
    const int tail = cin_p - 32 * (cdiv(cin_p, 32) - 1);
    const double k_o = 32.0 * (cdiv(cin_p, 32) - 1) + ((tail <= 16 && !s16) ? 64.0 / 3.0 : 32.0);
    double t_w = double(k16) * (cotiles * nf * 32) / eff * (1.0 + (nf == 2 ? 1.2 : 0.2) / (k16 / (s16 ? 32 : 16)));
    double t_o = (s16 ? 1.45 : 1.15) * k_o * rup(rows, 16) / eff_o;
    {
      const int cu_w = wide_grid_x(tiles, cotiles) * cotiles;
      const int nf_o = conv_pick_nfrag(rows);
      const int cot_o = cdiv(cdiv(rows, 16), nf_o);
      const int tiles_o = N * cdiv(Ho, TRo) * cdiv(Wo, TCo);
      int gx_o = 256 / cot_o > 0 ? 256 / cot_o : 1;
      if (gx_o > tiles_o) gx_o = tiles_o;
      const int cu_o = cdiv(tiles_o, cdiv(tiles_o, gx_o)) * cot_o;
      if (cu_w < 192) t_w *= 256.0 / cu_w;
      if (cu_o < 192) t_o *= 256.0 / cu_o;
    }
    const int gx = 256 / cotiles < tiles ? (256 / cotiles > 0 ? 256 / cotiles : 1) : tiles;
    if (tiles * cotiles < 256 || cdiv(tiles, gx) * (k16 / (s16 ? 32 : 16)) < 8 || t_w >= t_o) return c;
  }
  c.nf = nf;
  c.rows_pad = cotiles * nf * 32;
  c.TR = TR;
  c.TC = TC;
  return c;
}
}  // namespace frozen

static bool same_wide(const WideCfg& a, const WideCfg& b) { return a.nf == b.nf && a.rows_pad == b.rows_pad && a.TR == b.TR && a.TC == b.TC; }

struct Layer {
  int cin, cout, h;
};
static std::vector<Layer> baseline_layers() {
  std::vector<Layer> v;
  // BASELINE configs 2-5 at 256x256: (S, f) = (2, 21), (2, 30), (4, 30), (1, 30); Ci = 3 / 2
  const int sf[4][3] = {{2, 21, 3}, {2, 30, 2}, {4, 30, 2}, {1, 30, 2}};
  for (auto& c : sf) {
    const int S = c[0], f = c[1], Ci = c[2], fs = f * S;
    const Layer l[] = {{Ci, f, 256}, {f, f, 256}, {f, 2 * f, 128}, {2 * f, 2 * f, 128}, {2 * fs, 4 * fs, 64},
                       {4 * fs, 4 * fs, 64}, {4 * fs, 8 * fs, 32}, {8 * fs, 8 * fs, 32}, {8 * fs, 8 * fs, 16},
                       {16 * fs, 8 * fs, 32}, {8 * fs, 4 * fs, 32}, {8 * fs, 4 * fs, 64}, {4 * fs, 2 * fs, 64},
                       {4 * fs, 2 * fs, 128}, {2 * fs, fs, 128}, {f * (S + 1), f * (S + 1) / 2, 256},
                       {f * (S + 1) / 2, f, 256}};
    for (auto& x : l) v.push_back(x);
  }
  return v;
}
static int pad8(int c) { return rup(c, 8); }

static void test_layers() {
  const int batches[6] = {1, 2, 4, 16, 32, 64};
  for (const Layer& L : baseline_layers())
    for (int N : batches) {
      const int cin_p = L.cin <= 4 ? rup(L.cin, 4) : pad8(L.cin), cout_p = pad8(L.cout);
      // --- channel padding of the 256-pixel kernels
      const int cp = conv_cout_pad(L.cout), nf = conv_pick_nfrag(L.cout);
      CHECK(cp >= L.cout && cp % (16 * nf) == 0 && cp < L.cout + 16 * nf, "cout %d: pad %d nfrag %d", L.cout, cp, nf);
      // --- wide convolution: forward (mode 1) and data gradient (mode 0), rule and forced, split16 and 16-bit storage
      const int modes[4] = {1, 0, 4, 5};
      for (int mode : modes)
        for (int force = 0; force <= 1; ++force) {
          const bool fwd = mode == 1 || mode == 4;
          const int K = fwd ? cin_p : cout_p, R = fwd ? cout_p : cin_p, Ho = fwd ? L.h : L.h + 2;
          const WideCfg c = wide_config(mode, N, K, R, Ho, Ho, force);
          CHECK(same_wide(c, frozen::wide_config(mode, N, K, R, Ho, Ho, force)), "wide_config mode %d N %d %d->%d @%d force %d", mode, N, K, R, Ho, force);
          if (c.nf == 0) continue;
          CHECK((c.nf == 1 || c.nf == 2) && c.rows_pad >= R && c.rows_pad % (32 * c.nf) == 0 && c.rows_pad < R + 64,
                "wide rows: %d->%d nf %d rows_pad %d", K, R, c.nf, c.rows_pad);
          CHECK(c.TR * c.TC <= kWideNPix && (c.TR + 2) * (c.TC + 2) <= kWideMaxPix, "wide tile %dx%d", c.TR, c.TC);
          const int tiles = N * cdiv(Ho, c.TR) * cdiv(Ho, c.TC), cot = c.rows_pad / (32 * c.nf);
          const int gx = wide_grid_x(tiles, cot);
          CHECK(gx >= 1 && gx <= tiles && (gx * cot <= 256 || gx == 1), "wide grid: tiles %d cot %d gx %d", tiles, cot, gx);
          // every workgroup column walks ceil or floor(tiles / gx) tiles, at least one
          CHECK((tiles - 1 - (gx - 1)) / gx + 1 >= 1, "wide grid: last column without a tile");
          // the launch recomputes the configuration from (mode, geometry) alone with force = 1: same rows
          const WideCfg c2 = wide_config(mode, N, K, R, Ho, Ho, 1);
          CHECK(c2.rows_pad == c.rows_pad && c2.nf == c.nf, "wide: launch sees %d rows, packer %d", c2.rows_pad, c.rows_pad);
        }
      // --- weight gradient
      for (int ws = 0; ws <= 1; ++ws)
        for (const bool s16 : {false, true}) {  // s16: both operands 16-bit tensors (4-row tiles)
          int CI = 0, CO = 0;
          wg_tiles(cin_p, cout_p, ws != 0, &CI, &CO);
          CHECK((CI == 32 || CI == 48 || CI == 64) && (CO == 32 || CO == 48 || CO == 64), "wg tiles %d %d", CI, CO);
          const int cin_pad = rup(cin_p, CI), cout_pad = rup(cout_p, CO);
          for (const int cus : {256, 192, 128}) {  // launches sized for the whole chip or for a share of it (wg_side_cus)
          const int s = wg_pick_splits(N, L.h, L.h, cin_pad, cout_pad, CI, CO, ws != 0, s16, cus);
          const int tiles = wg_num_tiles(N, L.h, L.h, wg_use_ws(CI, CO, ws != 0) ? wg_ws_tr(CI, s16) : 4);
          CHECK(s >= 1 && s <= 1024 && s <= tiles, "wg splits %d (tiles %d) for %d->%d @%d N %d", s, tiles, L.cin, L.cout, L.h, N);
          // slabs + group-sum levels fit the plan's scratch formula (plan.hip cap_slab: splits + splits / 8 + 2 slabs)
          int extra = 0;
          for (int n = s; n > 1;) {
            n = cdiv(n, 16);
            extra += n;
          }
          CHECK(extra <= s / 8 + 2, "wg reduce levels %d > %d for %d splits", extra, s / 8 + 2, s);
          }
        }
    }
}

// 256-pixel split convolution: every decision equal to the frozen launch code's, and the grid invariants
static void test_split_rules() {
  std::vector<std::pair<int, int>> domains;
  for (int h : {2, 3, 4, 8, 15, 16, 17, 18, 30, 31, 32, 33, 34, 64, 66, 128, 130, 256, 258}) domains.push_back({h, h});
  for (auto d : {std::pair<int, int>{31, 33}, {33, 31}, {15, 17}, {17, 15}, {16, 18}, {8, 32}, {32, 8}, {2, 128}, {128, 2}, {2, 258},
                 {258, 2}, {37, 53}, {39, 55}, {64, 96}, {66, 98}, {32, 34}, {130, 258}})
    domains.push_back(d);
  std::vector<int> cins;
  for (int c : {4, 8, 16, 32, 48, 64, 96, 128, 240, 480})
    for (int d : {0, 4, 8}) cins.push_back(c + d);
  long cases = 0, splits = 0, paired = 0, ws_launches = 0;
  for (int mode = 0; mode <= 7; ++mode)
    for (int ws = 0; ws <= 1; ++ws)
      for (int N : {1, 2, 4, 32})
        for (auto [Ho, Wo] : domains) {
          for (int wide = 0; wide <= 1; ++wide)
            CHECK(split_fuses_input(mode, wide, Ho, Wo, ws != 0) == frozen::fuses_input(mode, wide, Ho, Wo, ws != 0),
                  "fuses_input mode %d wide %d %dx%d ws %d", mode, wide, Ho, Wo, ws);
          for (int cin_p : cins) {
            const int pair = ws_tail_pairs(mode, cin_p, Ho, Wo, ws != 0);
            CHECK(pair == frozen::pair_tail(mode, cin_p, Ho, Wo, ws != 0), "pair mode %d cin_p %d %dx%d ws %d: %d", mode, cin_p, Ho, Wo, ws, pair);
            paired += pair;
            for (int cout_pad = 16; cout_pad <= 512; cout_pad += 16) {
              if (ws == 1)  // (wide_config knows no switch of the split kernel: once per geometry)
                for (int wf = -1; wf <= 1; ++wf)
                  CHECK(same_wide(wide_config(mode, N, cin_p, cout_pad, Ho, Wo, wf), frozen::wide_config(mode, N, cin_p, cout_pad, Ho, Wo, wf)),
                        "wide_config mode %d N %d %d->%d %dx%d force %d", mode, N, cin_p, cout_pad, Ho, Wo, wf);
              for (int force : {-1, 0, 2, 3, 8}) {
                ++cases;
                const int ks = split_pick_ksplit(mode, N, cin_p, cout_pad, Ho, Wo, ws != 0, force);
                CHECK(ks == frozen::ksplit(mode, N, cin_p, cout_pad, Ho, Wo, ws != 0, force), "ksplit mode %d N %d %d->%d %dx%d ws %d force %d: %d",
                      mode, N, cin_p, cout_pad, Ho, Wo, ws, force, ks);
                const int ldy = cout_pad - 8;  // (any pixel pitch: the stored channels of the layer)
                CHECK(ksplit_scratch_floats(ks, N, Ho, Wo, ldy) == frozen::ksplit_scratch(mode, N, cin_p, cout_pad, Ho, Wo, ldy, ws != 0, force),
                      "ksplit scratch mode %d N %d %d->%d %dx%d", mode, N, cin_p, cout_pad, Ho, Wo);
                const SplitCfg c = split_config(mode, N, cin_p, cout_pad, Ho, Wo, ks, ws != 0);
                const frozen::Launch f = frozen::dispatch(mode, N, cout_pad, Ho, Wo, ks, ws != 0);
                CHECK(c.ws == f.ws && c.MF == f.MF && c.NF == f.NF && c.TR == f.TR && c.TC == f.TC && c.tilesY == f.tilesY && c.tilesX == f.tilesX &&
                          c.gx == f.gx && c.coTiles == f.coTiles && c.stat_rows == f.rows && c.pair == pair,
                      "split_config mode %d N %d %d->%d %dx%d ws %d ksplit %d: ws %d MF %d NF %d tile %dx%d gx %d coTiles %d rows %d (frozen: ws %d MF %d "
                      "NF %d tile %dx%d gx %d coTiles %d rows %d)",
                      mode, N, cin_p, cout_pad, Ho, Wo, ws, ks, c.ws, c.MF, c.NF, c.TR, c.TC, c.gx, c.coTiles, c.stat_rows, f.ws, f.MF, f.NF, f.TR, f.TC,
                      f.gx, f.coTiles, f.rows);
                // --- invariants
                const int numTiles = N * c.tilesY * c.tilesX;
                CHECK(c.gx >= 1 && c.gx <= numTiles && (long)c.gx * c.coTiles * ks >= 1, "grid: gx %d of %d tiles, %d channel tiles, ksplit %d", c.gx,
                      numTiles, c.coTiles, ks);
                CHECK(c.coTiles * c.NF * 16 == cout_pad && c.TR * c.TC <= split_npix(c.ws, c.MF) && (c.TR + 2) * (c.TC + 2) <= split_maxpix(c.ws, c.MF),
                      "tile %dx%d, %d x %d channels of %d", c.TR, c.TC, c.coTiles, c.NF * 16, cout_pad);
                if (c.gx >= 1 && c.gx <= numTiles) {  // column v walks tiles v, v + gx, ...: ceil(numTiles / gx) or one fewer, never none
                  const int per = cdiv(numTiles, c.gx), last = (numTiles - 1 - (c.gx - 1)) / c.gx + 1;
                  CHECK((numTiles - 1) / c.gx + 1 == per && (last == per || last == per - 1) && last >= 1, "walk: %d tiles on %d columns", numTiles, c.gx);
                }
                if (ks > 1) {
                  ++splits;
                  CHECK(c.ws && cin_p % 32 == 0 && ksplit_legal(cin_p / 32, ks) && c.coTiles * ks <= 256 && !pair, "ksplit %d of %d chunks, %d channel tiles",
                        ks, cin_p / 32, c.coTiles);
                  // every split has a chunk: the kernel's nck = min(cpk, nchunks - ks' * cpk) >= 1 for the last split
                  CHECK(cin_p / 32 - (ks - 1) * cdiv(cin_p / 32, ks) >= 1, "ksplit %d: the last split is empty", ks);
                }
                CHECK(c.stat_rows <= (c.ws ? kWsStatRows : conv_stat_rows(N, Ho, Wo)), "statistics rows %d > the plan's %d", c.stat_rows,
                      c.ws ? kWsStatRows : conv_stat_rows(N, Ho, Wo));
                ws_launches += c.ws;
              }
            }
          }
        }
  CHECK(kWsStatRows == frozen::ws_stat_rows(), "ws statistics rows %d", kWsStatRows);
  for (auto [Ho, Wo] : domains)
    for (int N : {1, 2, 4, 32}) CHECK(conv_stat_rows(N, Ho, Wo) == frozen::stat_rows(N, Ho, Wo), "conv_stat_rows N %d %dx%d", N, Ho, Wo);
  // the sweep reached every branch
  CHECK(cases > 1000000 && splits > 1000 && paired > 100 && ws_launches > 100000 && ws_launches < cases, "sweep: %ld cases, %ld K splits, %ld paired, %ld ws",
        cases, splits, paired, ws_launches);
  // the wide kernel's grid is the same rule with one workgroup per CU
  for (int tiles = 1; tiles <= 3000; tiles += (tiles < 600 ? 1 : 37))
    for (int cot = 1; cot <= 300; ++cot) CHECK(wide_grid_x(tiles, cot) == frozen::wide_grid_x(tiles, cot), "wide_grid_x(%d, %d)", tiles, cot);
}

// Dispatch decisions the measurements stand on (profiles/r03/conv_layers_ab.txt): a change of the
// cost rule that flips one of these is a deliberate act.  mode 1 = split16 forward, 0 = split16 data gradient
// (rows = padded input channels, domain (H + 2) x (W + 2)), 4 / 5 = bf16-mixed forward / data gradient.
static void test_pinned_decisions() {
  struct D { int mode, N, K, rows, H; bool wide; int nf; };
  const D pins[] = {
      {1, 32, 960, 480, 32, true, 2},   // up1.c1 forward: the largest layer
      {1, 32, 480, 480, 32, true, 2},
      {1, 32, 240, 240, 64, true, 2},
      {1, 32, 32, 30, 256, true, 1},    // 30->30 at 256x256: one 32-channel tile, a chunk per phase
      {1, 32, 48, 30, 256, true, 1},    // 45->30
      {1, 32, 480, 480, 16, false, 0},  // 16x16: the 128-pixel instances fill the chip better
      {1, 32, 96, 45, 256, false, 0},   // 90->45 forward stays on the 256-pixel kernel (64-channel tiles pad 45 -> 64)
      {0, 32, 480, 960, 34, false, 0},  // up1.c1 data gradient: the NF = 4 instance re-reads least
      {0, 32, 32, 32, 258, true, 1},    // 30->30 data gradient
      {1, 4, 32, 30, 256, false, 0},    // 4 images per GPU: two 2-chunk tiles per workgroup do not pay for a persistent kernel
      {1, 4, 240, 240, 64, false, 0},   // ... and 32 pixel tiles x 4 channel tiles leave half the CUs idle
      {0, 32, 240, 480, 66, true, 2},   // up2.c1 data gradient at batch 32: wide
      {0, 4, 240, 480, 66, false, 0},   // ... at 4 images per GPU its 36 x 8 tiles fill 144 workgroups of 2 tiles: the 256-pixel kernel's 230 win (136 -> 104 us)
      {4, 32, 960, 480, 32, true, 2},   // 16-bit storage: the wide kernel takes nearly everything
      {5, 32, 480, 960, 34, true, 2},
  };
  {  // weight-gradient channel tiles (input, output): 32-wide input tiles only where they save >= 20 % of padded work
    struct T { int cin_p, cout_p, CI, CO; };
    const T tiles[] = {{96, 48, 32, 48}, {88, 168, 32, 64}, {48, 32, 64, 32}, {32, 32, 32, 32}, {64, 64, 64, 64},
                       {120, 64, 64, 64}, {480, 480, 64, 64}, {160, 48, 64, 48}};
    for (const T& t : tiles) {
      int CI = 0, CO = 0;
      wg_tiles(t.cin_p, t.cout_p, true, &CI, &CO);
      CHECK(CI == t.CI && CO == t.CO, "pinned weight-gradient tiles for %d x %d: %d x %d (expected %d x %d)", t.cin_p, t.cout_p, CI, CO, t.CI,
            t.CO);
    }
  }
  for (const D& d : pins) {
    const WideCfg c = wide_config(d.mode, d.N, d.K, d.rows, d.H, d.H, 0);
    CHECK((c.nf != 0) == d.wide && (!d.wide || c.nf == d.nf), "pinned decision mode %d N %d %d->%d @%d: nf %d (expected %s nf %d)",
          d.mode, d.N, d.K, d.rows, d.H, c.nf, d.wide ? "wide" : "256-pixel", d.nf);
  }
}

// wide kernel: 32-bit per-unit source offsets - a layer whose image reaches 2 GiB must stay on the 256-pixel kernel
static void test_wide_offset_guard() {
  CHECK(wide_config(1, 1, 32, 32, 1024, 1024, 1).nf != 0, "1024x1024x32 fits 32-bit offsets");
  CHECK(wide_config(1, 1, 128, 128, 2048, 2048, 1).nf == 0, "2048x2048x128 fp32 overflows 32-bit offsets: not wide");
  CHECK(wide_config(1, 1, 32, 32, 4096, 4096, 1).nf == 0, "4096x4096x32 overflows with a 2x pixel pitch: not wide");
  CHECK(wide_config(0, 1, 64, 64, 2048, 2048, 0).nf == 0, "data gradient, same bound");
}

// Power-of-two scales of the fp16 operands (w16_scale, wg_dz_scale): for every exponent and a sweep of mantissas — an exact
// power of two, reciprocal pairs, the scaled maximum inside the band that fp16 represents, and the fixed 2^8 for ordinary weights.
static float bits_to_float(unsigned u) {
  union { unsigned u; float v; } c;
  c.u = u;
  return c.v;
}
static unsigned float_to_bits(float v) {
  union { unsigned u; float v; } c;
  c.v = v;
  return c.u;
}
static void test_scales() {
  for (unsigned e = 1; e <= 254; ++e)
    for (unsigned m = 0; m < (1u << 23); m += 0x1ffffu) {
      const unsigned bits = (e << 23) | m;
      const float x = bits_to_float(bits);
      const float ws = w16_scale(bits, false), wi = w16_scale(bits, true);
      CHECK((float_to_bits(ws) & 0x7fffffu) == 0 && (float_to_bits(wi) & 0x7fffffu) == 0, "w16_scale(%g) not a power of two", x);
      CHECK(ws * wi == 1.0f, "w16_scale(%g): %g * %g != 1", x, ws, wi);
      if (x < 128.f) CHECK(ws == 256.f, "w16_scale(%g) = %g, expected 2^8", x, ws);
      if (x >= 128.f && e <= 127 + 113) CHECK(x * ws >= 8192.f && x * ws < 16384.f, "w16_scale(%g): scaled max %g outside [2^13, 2^14)", x, x * ws);
      CHECK(x * ws < 65504.f || e > 127 + 113, "w16_scale(%g): scaled max %g overflows fp16", x, x * ws);
      const float ds = wg_dz_scale(bits, false), di = wg_dz_scale(bits, true);
      CHECK((float_to_bits(ds) & 0x7fffffu) == 0 && ds * di == 1.0f, "wg_dz_scale(%g): %g, %g", x, ds, di);
      if (e >= 16) CHECK(x * ds >= 16384.f && x * ds < 32768.f, "wg_dz_scale(%g): scaled max %g outside [2^14, 2^15)", x, x * ds);
      if (e < 16) CHECK(x * ds < 32768.f, "wg_dz_scale(%g): scaled max %g", x, x * ds);
    }
  CHECK(wg_dz_scale(0u, false) > 0.f && wg_dz_scale(0u, true) > 0.f, "all-zero dz: finite positive scale");
  CHECK(w16_scale(0u, false) == 256.f, "all-zero weights: 2^8");
  // infinity / NaN maxima: a finite scale (the non-finite values themselves propagate)
  CHECK(wg_dz_scale(0x7f800000u, false) > 0.f && wg_dz_scale(0x7fc00000u, true) > 0.f, "non-finite maximum: finite scale");
}

static void test_side_cus() {
  // the per-GPU batches of cfg3 (S x fbc = 60) under 8-, 4-, 2- and 1-way strong scaling, cfg4 (S = 4: 120) at its 16 images per
  // GPU and cfg2 (2 x 21) at its 64: the measurements the rule stands on (profiles/r05/exp/wgrad_cu_share.txt)
  CHECK(wg_side_cus(4L * 256 * 256, 60) == 128 && wg_side_cus(8L * 256 * 256, 60) == 192 && wg_side_cus(16L * 256 * 256, 60) == 192 &&
            wg_side_cus(32L * 256 * 256, 60) == 256 && wg_side_cus(16L * 256 * 256, 120) == 256 && wg_side_cus(64L * 256 * 256, 42) == 256,
        "wg_side_cus on the measured configurations");
  for (const int width : {8, 42, 60, 120, 512}) {
    int prev = 0;
    for (long px = 1; px < (1L << 34); px = px * 3 / 2 + 1) {  // monotone, 8 <= cus <= 256
      const int c = wg_side_cus(px, width);
      CHECK(c >= 8 && c <= 256 && c >= prev, "wg_side_cus(%ld, %d) = %d", px, width, c);
      prev = c;
    }
  }
}

int main() {
  test_side_cus();
  test_scales();
  test_xcd();
  test_wide_offset_guard();
  test_tiles();
  test_layers();
  test_split_rules();
  test_pinned_decisions();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("sched_test: all checks passed\n");
  return 0;
}
