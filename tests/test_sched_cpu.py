"""Host-side schedulers (mimo_unet_amd/csrc/tile_sched.h: XCD workgroup order, tile shapes, channel-tile widths, split
counts, the wide-convolution dispatch) compiled with g++ -fsanitize=address,undefined and swept over their argument
ranges — the kernels consume exactly these functions (the .hip files include the same header)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_host_test(tmp_path, name):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, "tests", "host", name + ".cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", src, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout


def test_schedulers_under_asan_ubsan(tmp_path):
    _run_host_test(tmp_path, "sched_test")


def test_dz_ring_policy_under_asan_ubsan(tmp_path):
    """mimo_unet_amd/csrc/dz_ring.h: every sequence of layers, joins and rewinds of three trips round the ring, from a clean
    ring and from what an abandoned staged backward leaves — no dz buffer is handed out under a weight gradient that still
    reads it, and the waits are those of the logic the policy replaced (tests/host/dz_ring_test.cpp)."""
    _run_host_test(tmp_path, "dz_ring_test")


def test_graph_replay_policy_under_asan_ubsan(tmp_path):
    """mimo_unet_amd/csrc/graph_replay.h: every sequence of nine training forwards and backwards of two call shapes each,
    calls that are not graphable and drops of the graphs, on a budget of three captures, from a clean plan and from what a drop
    leaves — eager / capture / replay and the captures spent are those of the in-line logic the policy replaced, nothing is
    captured at first sight or replayed under another key, and nothing is graphed once the budget is spent; the eval-mode
    form (capture at first sight, no budget) likewise (tests/host/graph_replay_test.cpp)."""
    _run_host_test(tmp_path, "graph_replay_test")


def test_pack_layout_under_asan_ubsan(tmp_path):
    """mimo_unet_amd/csrc/pack_layout.h: the layout kind and the convolution mode of every (precision, direction, split,
    wide) the plan produces against a written-out table, and over a sweep of layer geometries the job the plan and the
    per-operator entry points build: sizes consistent, every element pack_jobs_kernel's formulas store to inside the
    image (tests/host/pack_layout_test.cpp)."""
    _run_host_test(tmp_path, "pack_layout_test")


def test_conv_recipe_under_asan_ubsan(tmp_path):
    """mimo_unet_amd/csrc/conv_recipe.h: the launch decisions of every convolution of cfg2, cfg3 and cfg4 at the benchmark's
    batches and of the per-operator test geometries, in the five precisions and with the image kernels and the
    wave-specialised kernels on and off, against a table of what the code it replaced decided; the pack job of every
    row carries the pair tail and wide rows its launch gets; and the weight gradient's split count at 128, 192 and 256 CUs
    leaves no split without a tile and its reduction inside the slabs allocated (tests/host/conv_recipe_test.cpp)."""
    _run_host_test(tmp_path, "conv_recipe_test")


def test_kernels_use_the_tested_header():
    """No private copy of a scheduler is left in the .hip sources.  conv_bf16x3.hip reaches the channel-tile width
    (sched::split_pick_nf), the tile shape and the grid through sched::split_config alone: it picks no tile, prices nothing
    and reads its two switches in one place each."""
    csrc = os.path.join(ROOT, "mimo_unet_amd", "csrc")
    for fn, needles in (("conv_bf16x3.hip", ["sched::split_config", "sched::split_pick_ksplit", "sched::ws_tail_pairs", "sched::split_fuses_input",
                                             "sched::ksplit_legal", "sched::ksplit_scratch_floats", "sched::split_maxpix", "sched::kWsStatRows"]), ("conv3x3.hip", ["sched::pick_tile_n", "sched::conv_cout_pad", "sched::conv_stat_rows"]),
                        ("wgrad_split.hip", ["sched::wg_tiles", "sched::wg_pick_splits", "sched::wg_use_ws"]),
                        # the per-layer decisions (pair tail, wide rows, K-split scratch, weight-gradient tiles and splits) are taken in one place
                        ("conv_recipe.h", ["sched::ws_tail_pairs", "sched::wide_config", "sched::split_pick_ksplit", "sched::ksplit_scratch_floats",
                                           "sched::wg_tiles", "sched::wg_pick_splits", "sched::wg32_pick_splits", "sched::thin_geometry_ok"]),
                        ("plan.hip", ["conv_recipe(", "fill_conv_launch", "fill_wgrad_launch", "sched::wg_side_cus", "sched::DzRingPolicy", "sched::GraphReplayPolicy", "pack::make_job", "pack::image_elems"]),
                        ("ops_api.hip", ["conv_recipe(", "fill_conv_launch", "fill_wgrad_launch", "pack::make_job", "pack::image_elems"]),("common.h", ["sched::xcd_virtual_index", "sched::w16_scale", "sched::wg_dz_scale"]),
                        ("conv_wide.hip", ["sched::wide_config", "sched::wide_grid_x"])):
        text = open(os.path.join(csrc, fn)).read()
        for n in needles:
            assert n in text, (fn, n)
    split = open(os.path.join(csrc, "conv_bf16x3.hip")).read()
    for gone in ("pick_tile_n", "use_big_tile", "kKsplitReduceUnits", "kWgPerCU", "(1 + c)", "(1 + nf)", "tail <= 16"):
        assert gone not in split, gone
    assert split.count('getenv("MIMO_CONV_WS")') == 2 and split.count('getenv("MIMO_CONV_KSPLIT")') == 1  # one statement each
    for h in ("tile_sched.h", "conv_recipe.h", "conv_launch.h"):
        header = open(os.path.join(csrc, h)).read()
        assert "getenv" not in header and "hip/" not in header, h
    # ... and nowhere else: the plan and the entry points decide nothing about a convolution launch themselves
    for fn in ("plan.hip", "ops_api.hip"):
        text = open(os.path.join(csrc, fn)).read()
        for gone in ("ws_tail_pairs", "pair_tail", "wide_config", "wide_rows", "wg_tiles", "wgrad_split_tiles", "pick_splits", "pick_ksplit"):
            assert gone not in text, (fn, gone)
