"""Whole-scene tiling without a GPU: proves the numpy restatement (tests/scene_reference.py) that the GPU tests compare
`mimo_scene_gather_tiles` / `mimo_scene_stitch` against bit for bit — the grid, the coverage, reassembly of a field from
its own tiles, agreement with an independent float64 formulation, invariance to the launch size — and checks the declared
interface, the entry points' argument checks (refused before anything touches a device) and the host layer's.

Error model used below.  u = 2^-24.  A normalised 1-D weight is one correctly rounded division of exact integers (1 + d),
the 2-D weight one product of two of them (three roundings in all), a term one more product (four), and a pixel covered by
m = |K_y| |K_x| tiles passes its terms through at most m - 1 additions: every term reaches the result with at most m + 3
factors (1 + d), |d| <= u, so  |result - sum_t a_t v_t| <= gamma(m + 3) sum_t a_t |v_t|,  gamma(k) = k u / (1 - k u)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import scene_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
# (h, w, patch, stride): the GPU test's geometries, and s == 1 on one axis' worth of tiles
GEOMETRIES = [(13, 19, 8, 5), (16, 24, 8, 8), (17, 17, 8, 3), (12, 11, 8, 1), (8, 8, 8, 5)]


def gamma(k):
    return k * U / (1.0 - k * U)


def cover_count(grid):
    """m [h, w] = |K_y(y)| |K_x(x)|"""
    return np.outer([len(k) for k in grid.ky_of], [len(k) for k in grid.kx_of])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("length,patch,stride,count,origins", [
    (8, 8, 5, 1, [0]),                       # L == P: one tile
    (18, 8, 5, 3, [0, 5, 10]),               # (L - P) % s == 0
    (19, 8, 5, 4, [0, 5, 10, 11]),           # a clamped last tile
    (13, 8, 5, 2, [0, 5]),
    (24, 8, 8, 3, [0, 8, 16]),               # s == P
    (25, 8, 8, 4, [0, 8, 16, 17]),           # s == P, clamped
    (11, 8, 1, 4, [0, 1, 2, 3]),             # s == 1
    (2048, 256, 249, 9, [0, 249, 498, 747, 996, 1245, 1494, 1743, 1792]),  # the SEN12TP cut on a 2048-pixel axis
])
def test_tile_counts_and_origins(length, patch, stride, count, origins):
    assert R.axis_tiles(length, patch, stride) == count
    assert R.axis_origins(length, patch, stride) == origins
    assert all(0 <= o <= length - patch for o in origins)  # shifted inwards, never padded
    from mimo_unet_amd.inference import SceneTiler, axis_tiles
    assert axis_tiles(length, patch, stride) == count
    tiler = SceneTiler(length, patch + 3, patch, stride)  # the other axis: two tiles, 0 and 3 (one at s == 1 ... 3)
    nx = R.axis_tiles(patch + 3, patch, stride)
    assert (tiler.ny, tiler.nx, tiler.num_tiles) == (count, nx, count * nx)
    assert tiler.origins() == R.Grid(length, patch + 3, patch, stride).origins()  # row-major: t = ky nx + kx


@pytest.mark.parametrize("length,patch,stride", [(8, 8, 5), (18, 8, 5), (19, 8, 5), (24, 8, 8), (25, 8, 8), (11, 8, 1),
                                                 (17, 8, 3), (64, 32, 25), (57, 32, 25)])
def test_coverage_and_weights(length, patch, stride):
    cover = R.covering(length, patch, stride)
    for p, ks in enumerate(cover):
        assert ks and ks == list(range(ks[0], ks[-1] + 1)), p  # covered, by a contiguous range
    for window in ("uniform", "linear"):
        a = R.axis_weights(length, patch, stride, window)
        assert a.dtype == np.float32
        for p, ks in enumerate(cover):
            assert np.all(a[ks, p] > 0) and np.count_nonzero(a[:, p]) == len(ks)
        # each weight is within u of an exact share: the float64 sum of the fp32 weights is within u of 1 (2 ulp = 4 u)
        assert np.all(np.abs(a.astype(np.float64).sum(axis=0) - 1.0) <= 2 * 2.0 ** -23)
    crop = R.axis_weights(length, patch, stride, "crop")
    assert set(np.unique(crop)) <= {0.0, 1.0} and np.all(crop.sum(axis=0) == 1.0)  # exactly one owner
    origins = R.axis_origins(length, patch, stride)
    for p, (ks, k) in enumerate(zip(cover, R.axis_owner(length, patch, stride))):
        w = {j: R.linear_window(p - origins[j], patch) for j in ks}
        assert crop[k, p] == 1.0 and w[k] == max(w.values()) and all(w[j] < w[k] for j in ks if j < k)


def test_linear_window_is_the_tent():
    assert [R.linear_window(i, 8) for i in range(8)] == [1, 2, 3, 4, 4, 3, 2, 1]
    assert [R.linear_window(i, 5) for i in range(5)] == [1, 2, 3, 2, 1]


# ------------------------------------------------------------------------------------------------- gather and stitch
def _field(c, h, w, seed):
    return np.random.default_rng(seed).standard_normal((c, h, w)).astype(np.float32)


def test_gather_clamps_to_the_last_tile():
    grid = R.Grid(13, 19, 8, 5)
    scene = _field(2, 13, 19, 1)
    tiles = R.gather(scene, grid, 5, 6)  # tiles 5, 6, 7, 7, 7, 7
    assert tiles.shape == (6, 2, 8, 8)
    assert np.array_equal(tiles[0], scene[:, 5:13, 5:13]) and np.array_equal(tiles[2], scene[:, 5:13, 11:19])
    assert all(np.array_equal(tiles[b], tiles[2]) for b in (3, 4, 5))


@pytest.mark.parametrize("h,w,patch,stride", GEOMETRIES)
@pytest.mark.parametrize("window", R.WINDOWS)
def test_reassembly_of_a_field_from_its_own_tiles(h, w, patch, stride, window):
    grid = R.Grid(h, w, patch, stride)
    scene = _field(2, h, w, 2)
    got = R.stitch_scene(R.gather(scene, grid, 0, grid.num_tiles), grid, window, launch=grid.num_tiles)
    assert np.all(np.isfinite(got))  # the NaN pre-fill is gone: every pixel's first term was stored
    m = cover_count(grid)
    assert m.max() == {(13, 19): 6, (16, 24): 1, (17, 17): 9, (12, 11): 20, (8, 8): 1}[h, w]  # up to 20 tiles on a pixel
    if window == "crop" or m.max() == 1:  # a pure copy; s == P (and L == P): no overlap, every weight is 1
        assert np.array_equal(bits(got), bits(scene))
        return
    # all m terms of a pixel are shares of the same value f, of one sign, and the exact shares sum to 1:
    # |result - f| <= gamma(m + 3) |f|  — (m + 3) ulp at most; m == 1 has a == 1 and is exact
    assert np.array_equal(bits(got[:, m == 1]), bits(scene[:, m == 1]))
    err = np.abs(got.astype(np.float64) - scene.astype(np.float64))
    assert np.all(err <= gamma(m + 3)[None] * np.abs(scene.astype(np.float64)))


@pytest.mark.parametrize("h,w,patch,stride", GEOMETRIES)
@pytest.mark.parametrize("window", R.WINDOWS)
def test_restated_stitch_agrees_with_the_float64_formulation(h, w, patch, stride, window):
    """Independent tile values (not cut from one field), against np.add.at of w v and w in float64 and one division."""
    grid = R.Grid(h, w, patch, stride)
    tiles = np.random.default_rng(3).standard_normal((grid.num_tiles, 2, patch, patch)).astype(np.float32)
    got = R.stitch_scene(tiles, grid, window, launch=grid.num_tiles).astype(np.float64)
    want = R.stitch_fp64(tiles, grid, window)
    if window == "crop":
        assert np.array_equal(got, want)  # a pure copy
        return
    # gamma(m + 3) sum_t a_t |v_t| (module docstring), the sum taken by the same float64 formulation over |v|; the float64
    # side's own rounding, about m 2^-53 of that sum, is covered by one more unit in the gamma
    m = cover_count(grid)
    bound = gamma(m + 4)[None] * R.stitch_fp64(np.abs(tiles), grid, window)
    assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("h,w,patch,stride", GEOMETRIES[:4])
@pytest.mark.parametrize("window", R.WINDOWS)
def test_restated_stitch_is_invariant_to_the_launch_size(h, w, patch, stride, window):
    grid = R.Grid(h, w, patch, stride)
    tiles = np.random.default_rng(4).standard_normal((grid.num_tiles, 1, patch, patch)).astype(np.float32)
    whole = R.stitch_scene(tiles, grid, window, launch=grid.num_tiles)
    for launch in (1, 3, grid.nx + 1):
        assert np.array_equal(bits(R.stitch_scene(tiles, grid, window, launch=launch)), bits(whole)), launch


def test_a_launch_touches_only_the_pixels_its_tiles_cover():
    grid = R.Grid(13, 19, 8, 5)
    tiles = np.ones((2, 1, 8, 8), dtype=np.float32)
    for window in R.WINDOWS:
        dst = np.full((1, 13, 19), -7.0, dtype=np.float32)
        R.stitch(dst, tiles, grid, window, 1, 2)  # tiles 1 and 2: rows 0 ... 7, columns 5 ... 17
        touched = dst[0] != -7.0
        assert not touched[8:].any() and not touched[:, :5].any() and not touched[:, 18:].any()
        if window != "crop":
            assert touched[:8, 5:18].all()


# ----------------------------------------------------------------------------------------------------- the interface
def test_entry_points_are_declared_bound_and_refuse_bad_arguments(built_library):
    from mimo_unet_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    for name in ("mimo_scene_gather_tiles", "mimo_scene_stitch"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "typedef struct mimo_stitch_field" in header and "MIMO_WINDOW_CROP = 2" in header
    assert "scene/scene_tiles.hip" in open(os.path.join(ROOT, "Makefile")).read()
    assert C.sizeof(_lib.StitchField) == 24 and _lib.StitchField.dst.offset == 8 and _lib.StitchField.c.offset == 16
    assert _lib.WINDOWS == {"uniform": 0, "linear": 1, "crop": 2}

    # refused before anything touches a device; 64 and 128 stand in for (never dereferenced) device addresses
    def gather(scene=64, dst=128, c=1, h=16, w=16, patch=8, stride=5, t0=0, n=1):
        return lib.mimo_scene_gather_tiles(scene, dst, c, h, w, patch, stride, t0, n, None)

    for what, kw in {"null scene": dict(scene=None), "null dst": dict(dst=None), "odd scene": dict(scene=66),
                     "c 0": dict(c=0), "h 0": dict(h=0), "w < 0": dict(w=-16), "patch 0": dict(patch=0),
                     "stride 0": dict(stride=0), "n 0": dict(n=0), "patch > h": dict(h=7), "patch > w": dict(w=7),
                     "stride > patch": dict(stride=9), "t0 < 0": dict(t0=-1), "t0 == T": dict(t0=9),
                     "2^31 elements": dict(h=4096, w=4096, patch=1024, stride=1024, c=2, n=1024)}.items():
        assert gather(**kw) == -1, what
        assert lib.mimo_last_error().startswith(b"mimo_scene_gather_tiles:"), what

    def stitch(fields=((64, 128, 1),), n_fields=None, h=16, w=16, patch=8, stride=5, window=1, t0=0, n_valid=1, table=True):
        tab = (_lib.StitchField * max(len(fields), 1))(*(_lib.StitchField(s, d, c, 0) for s, d, c in fields))
        return lib.mimo_scene_stitch(tab if table else None, len(fields) if n_fields is None else n_fields, h, w, patch,
                                     stride, window, t0, n_valid, None)

    for what, kw in {"no fields": dict(n_fields=0), "five fields": dict(fields=((64, 128, 1),) * 5),
                     "null table": dict(table=False), "null src": dict(fields=((None, 128, 1),)),
                     "null dst": dict(fields=((64, 128, 1), (64, None, 1))), "odd dst": dict(fields=((64, 130, 1),)),
                     "c 0": dict(fields=((64, 128, 0),)), "c 65536": dict(fields=((64, 128, 65536),)),
                     "h 0": dict(h=0), "patch > w": dict(w=7), "stride > patch": dict(stride=9), "stride 0": dict(stride=0),
                     "window 3": dict(window=3), "window -1": dict(window=-1), "t0 < 0": dict(t0=-1),
                     "n_valid 0": dict(n_valid=0), "past the last tile": dict(t0=8, n_valid=2),
                     "patch 8192": dict(h=8192, w=8192, patch=8192, stride=8192),
                     "2^31 pixels": dict(h=1 << 16, w=1 << 15)}.items():
        assert stitch(**kw) == -1, what
        assert lib.mimo_last_error().startswith(b"mimo_scene_stitch:"), what


# ---------------------------------------------------------------------------------------------------- the host layer
def _evidential():
    from mimo.models.evidential_unet import EvidentialUnetModel
    return EvidentialUnetModel(in_channels=2, out_channels=4, filter_base_count=2, center_dropout_rate=0.0,
                               final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
                               decoder_dropout_rate=0.0, weight_decay=0.0, learning_rate=1e-3, seed=0).eval()


def _member():
    from mimo.models.mimo_unet import MimoUnetModel
    return MimoUnetModel(in_channels=2, out_channels=2, num_subnetworks=2, filter_base_count=2, center_dropout_rate=0.0,
                         final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0,
                         loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3, seed=0, loss_buffer_size=10,
                         loss_buffer_temperature=0.3)


def test_scene_tiler_argument_checks():
    import mimo.inference
    from mimo_unet_amd.inference import SceneTiler
    assert mimo.inference.SceneTiler is SceneTiler
    t = SceneTiler(2048, 2048)  # the defaults: the SEN12TP cut
    assert (t.patch_size, t.stride, t.window, t.num_tiles) == (256, 249, "linear", 81) and t.num_batches(32) == 3
    for bad in (dict(height=31), dict(width=31), dict(stride=0), dict(stride=33), dict(stride=-1), dict(window="hann"),
                dict(patch_size=0)):
        kw = dict(height=57, width=64, patch_size=32, stride=25, window="linear")
        kw.update(bad)
        with pytest.raises(ValueError):
            SceneTiler(**kw)
    t = SceneTiler(57, 64, 32, 25, "crop")
    with pytest.raises(ValueError):
        t.gather(torch.zeros(3, 57, 64), 0, 4)  # a host tensor
    with pytest.raises(ValueError):
        t.stitch([], 0, 1)


def test_predict_scene_argument_checks():
    from mimo.inference import predict_scene
    from mimo.models.ensemble import EnsembleModule
    from mimo_unet_amd._lib import MimoHipError
    ens, ev = EnsembleModule([], models=[_member()]), _evidential()
    scene = torch.zeros(2, 40, 48)
    kw = dict(patch_size=32, stride=25, batch_size=4)
    for model in (ens, ev):
        for bad in (dict(patch_size=41), dict(patch_size=48), dict(stride=0), dict(stride=33), dict(window="hann"),
                    dict(batch_size=0)):
            with pytest.raises(ValueError):
                predict_scene(model, scene, **{**kw, **bad})
        with pytest.raises(ValueError, match="channels"):
            predict_scene(model, torch.zeros(3, 40, 48), **kw)
        with pytest.raises(ValueError):
            predict_scene(model, torch.zeros(1, 2, 40, 48), **kw)
        with pytest.raises(MimoHipError):  # every check passed: what stops a host model is the engine's own error
            predict_scene(model, scene, **kw)
    with pytest.raises(ValueError, match="return_raw_predictions"):
        predict_scene(EnsembleModule([], models=[_member()], return_raw_predictions=True), scene, **kw)
    with pytest.raises(TypeError):
        predict_scene(_member(), scene, **kw)


def test_ensemble_forward_returns_what_its_device_body_returns(monkeypatch):
    """`forward` is `forward_on_device` plus the move to the host that `keep_on_device` switches off."""
    from mimo.models.ensemble import EnsembleModule
    ens = EnsembleModule([], models=[_member()])
    marker = tuple(torch.full((1,), float(i)) for i in range(3))
    monkeypatch.setattr(ens, "forward_on_device", lambda x: marker)
    out = ens(torch.zeros(1, 2, 32, 32))
    assert all(torch.equal(a, b) for a, b in zip(out, marker))
    ens.keep_on_device = True
    assert ens(torch.zeros(1, 2, 32, 32)) is marker
