"""Whole-scene inference on the GPU: `mimo_scene_gather_tiles` and `mimo_scene_stitch` bit for bit against their numpy
restatement (tests/scene_reference.py, proved in tests/test_scene_reference_cpu.py) for all three windows, their argument
checks, and `predict_scene` end to end against the restated stitch of the model's own tile results.

Kernel shapes, the smallest at which each path can go wrong:
  P 8,  s 5, 2 x 13 x 19   clamped last tile on both axes, odd row length (no source quad on 16 bytes after row 0), 6 tiles on a pixel
  P 8,  s 8, 1 x 16 x 24   no overlap: every weight is 1
  P 8,  s 3, 1 x 17 x 17   three tiles per axis on a pixel (nine in all)
  P 32, s 25, 4 x 57 x 64  float4 loads (ox = 0, 32) and scalar loads (ox = 25) into float4 stores, more than one workgroup;
                           once more with the destination one float into its allocation (scalar stores)
  P 6,  s 4, 1 x 9 x 11    a patch that is no multiple of 4: a tail of 2 pixels per tile row
Launch sizes 1, 3, T and T + 2: the clamp of the gather and `n_valid` of the stitch; the rows behind `n_valid` hold NaN, the
destinations are pre-filled with NaN (the first-write rule) between guard floats."""
import functools

import numpy as np
import pytest
import torch

from tests import scene_reference as R

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.0
CASES = {
    # name: (patch, stride, (c, h, w), destination shift of the gather in floats)
    "p8_s5_2x13x19_clamped_scalar": (8, 5, (2, 13, 19), 0),
    "p8_s8_1x16x24_no_overlap": (8, 8, (1, 16, 24), 0),
    "p8_s3_1x17x17_nine_tiles_on_a_pixel": (8, 3, (1, 17, 17), 0),
    "p32_s25_4x57x64_float4": (32, 25, (4, 57, 64), 0),
    "p32_s25_4x57x64_scalar_stores": (32, 25, (4, 57, 64), 1),
    "p6_s4_1x9x11_row_tail": (6, 4, (1, 9, 11), 0),
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Guarded:
    """`numel` floats between guard floats (optionally `shift` floats further into the allocation), filled with `fill`."""

    def __init__(self, shape, fill, shift=0):
        self.shape, self.numel, self.first = tuple(shape), int(np.prod(shape)), GUARD + shift
        self.buf = torch.full((self.first + self.numel + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.view = self.buf[self.first:self.first + self.numel].view(self.shape)
        self.view.fill_(fill)
        self.ptr = self.buf.data_ptr() + 4 * self.first

    def out(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        b = self.buf.cpu()
        return bool((b[:self.first] == SENTINEL).all() and (b[self.first + self.numel:] == SENTINEL).all())


def _gather(scene_ptr, dst_ptr, c, h, w, patch, stride, t0, n):
    from mimo_unet_amd import _lib
    rc = _lib.load().mimo_scene_gather_tiles(scene_ptr, dst_ptr, c, h, w, patch, stride, t0, n, _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def _stitch(fields, h, w, patch, stride, window, t0, n_valid, n_fields=None):
    """fields: (source pointer, destination pointer, channels)"""
    from mimo_unet_amd import _lib
    table = (_lib.StitchField * max(len(fields), 1))(*(_lib.StitchField(s, d, c, 0) for s, d, c in fields))
    rc = _lib.load().mimo_scene_stitch(table, len(fields) if n_fields is None else n_fields, h, w, patch, stride,
                                       window if isinstance(window, int) else _lib.WINDOWS[window], t0, n_valid,
                                       _lib.current_stream())
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def _case(name):
    """(grid, scene, tile values of two fields with c and 1 channels): computed once, never written"""
    patch, stride, (c, h, w), _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    grid = R.Grid(h, w, patch, stride)
    scene = rng.standard_normal((c, h, w)).astype(np.float32)
    values = [rng.standard_normal((grid.num_tiles, k, patch, patch)).astype(np.float32) for k in (c, 1)]
    return grid, scene, values


@functools.lru_cache(maxsize=None)
def _stitched(name, window):
    grid, _, values = _case(name)
    return [R.stitch_scene(v, grid, window, launch=grid.num_tiles) for v in values]


@pytest.mark.parametrize("name", list(CASES))
def test_gather_equals_the_definition(name):
    patch, stride, (c, h, w), shift = CASES[name]
    grid, scene, _ = _case(name)
    T = grid.num_tiles
    scene_dev = _dev(scene)
    for n in (1, 3, T, T + 2):
        for t0 in range(0, T, n):
            dst = _Guarded((n, c, patch, patch), np.nan, shift)
            assert _gather(scene_dev.data_ptr(), dst.ptr, c, h, w, patch, stride, t0, n) == 0
            want = R.gather(scene, grid, t0, n)
            assert np.array_equal(_bits(dst.out()), _bits(want)), (name, n, t0)
            assert dst.guards_intact(), (name, n, t0)
    # the clamp: a launch that overruns T repeats the last tile
    oy, ox = grid.origin(T - 1)
    assert np.array_equal(R.gather(scene, grid, 0, T + 2)[-1], scene[:, oy:oy + patch, ox:ox + patch])


@pytest.mark.parametrize("window", R.WINDOWS)
@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[3] == 0])
def test_stitch_equals_the_restatement_for_every_launch_size(name, window):
    patch, stride, (c, h, w), _ = CASES[name]
    grid, _, values = _case(name)
    T = grid.num_tiles
    want = _stitched(name, window)
    results = []
    for n in (1, 3, T, T + 2):
        maps = [_Guarded((k, h, w), np.nan) for k in (c, 1)]
        for t0 in range(0, T, n):
            n_valid = min(n, T - t0)
            sources = []
            for v in values:  # a batch of n rows: the tiles of the launch, then NaN the kernel must not read
                batch = np.full((n,) + v.shape[1:], np.nan, dtype=np.float32)
                batch[:n_valid] = v[t0:t0 + n_valid]
                sources.append(_dev(batch))
            fields = [(s.data_ptr(), m.ptr, k) for s, m, k in zip(sources, maps, (c, 1))]
            assert _stitch(fields, h, w, patch, stride, window, t0, n_valid) == 0
        got = [m.out() for m in maps]
        for g, wnt, m in zip(got, want, maps):
            assert np.all(np.isfinite(g)), (name, window, n)  # the first-write rule: no NaN of the pre-fill is left
            assert np.array_equal(_bits(g), _bits(wnt)), (name, window, n)
            assert m.guards_intact(), (name, window, n)
        results.append(got)
    for other in results[1:]:  # whatever the batching: the same bits
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(results[0], other))


def test_a_launch_leaves_the_other_pixels_alone():
    patch, stride, (c, h, w), _ = CASES["p8_s5_2x13x19_clamped_scalar"]
    grid, _, values = _case("p8_s5_2x13x19_clamped_scalar")
    for window in R.WINDOWS:
        dst = _Guarded((c, h, w), SENTINEL)
        want = np.full((c, h, w), SENTINEL, dtype=np.float32)
        # tiles 1 and 2 alone: rows 0 ... 7, columns 5 ... 17; the first terms of columns 5 ... 7 (tile 0) are "already
        # there" as the sentinel, which the restatement adds to in the same way
        src = _dev(values[0][1:3])
        assert _stitch([(src.data_ptr(), dst.ptr, c)], h, w, patch, stride, window, 1, 2) == 0
        R.stitch(want, values[0][1:3], grid, window, 1, 2)
        got = dst.out()
        assert np.array_equal(_bits(got), _bits(want)), window
        assert np.all(got[:, 8:] == SENTINEL) and np.all(got[:, :, :5] == SENTINEL) and np.all(got[:, :, 18:] == SENTINEL)
        assert dst.guards_intact()


def test_refused_arguments_launch_nothing():
    from mimo_unet_amd import _lib
    c, h, w, patch, stride, n = 2, 13, 19, 8, 5, 3
    scene = _dev(np.zeros((c, h, w), dtype=np.float32))
    lib = _lib.load()

    def gather_refused(what, **kw):
        dst = _Guarded((n, c, patch, patch), SENTINEL)
        args = dict(scene_ptr=scene.data_ptr(), dst_ptr=dst.ptr, c=c, h=h, w=w, patch=patch, stride=stride, t0=0, n=n)
        args.update(kw)
        assert _gather(**args) != 0, what
        assert lib.mimo_last_error().startswith(b"mimo_scene_gather_tiles:"), what
        assert bool((dst.buf == SENTINEL).all()), what

    good = _Guarded((n, c, patch, patch), SENTINEL)
    assert _gather(scene.data_ptr(), good.ptr, c, h, w, patch, stride, 0, n) == 0 and bool((good.view == 0).all())
    for what, kw in {"null scene": dict(scene_ptr=None), "scene off by 2 bytes": dict(scene_ptr=scene.data_ptr() + 2),
                     "c 0": dict(c=0), "h < patch": dict(h=7), "w < patch": dict(w=7), "w 0": dict(w=0),
                     "patch 0": dict(patch=0), "stride 0": dict(stride=0), "stride > patch": dict(stride=9),
                     "n 0": dict(n=0), "t0 < 0": dict(t0=-1), "t0 == T": dict(t0=8),
                     "2^31 destination elements": dict(n=1 << 26)}.items():
        gather_refused(what, **kw)
    assert _gather(scene.data_ptr(), None, c, h, w, patch, stride, 0, n) != 0

    src = _dev(np.ones((n, c, patch, patch), dtype=np.float32))

    def stitch_refused(what, fields=None, **kw):
        dst = _Guarded((c, h, w), SENTINEL)
        args = dict(h=h, w=w, patch=patch, stride=stride, window="linear", t0=0, n_valid=n)
        args.update(kw)
        assert _stitch(fields(dst) if fields else [(src.data_ptr(), dst.ptr, c)], **args) != 0, what
        assert lib.mimo_last_error().startswith(b"mimo_scene_stitch:"), what
        assert bool((dst.buf == SENTINEL).all()), what

    good = _Guarded((c, h, w), SENTINEL)
    assert _stitch([(src.data_ptr(), good.ptr, c)], h, w, patch, stride, "linear", 0, n) == 0 and good.guards_intact()
    assert not bool((good.view == SENTINEL).all())
    for what, kw in {"no fields": dict(n_fields=0), "h < patch": dict(h=7), "w < patch": dict(w=7), "stride 0": dict(stride=0),
                     "stride > patch": dict(stride=9), "window 3": dict(window=3), "t0 < 0": dict(t0=-1),
                     "n_valid 0": dict(n_valid=0), "past the last tile": dict(t0=6, n_valid=3)}.items():
        stitch_refused(what, **kw)
    stitch_refused("five fields", fields=lambda d: [(src.data_ptr(), d.ptr, c)] * 5)
    stitch_refused("null source", fields=lambda d: [(None, d.ptr, c)])
    stitch_refused("destination off by 2 bytes", fields=lambda d: [(src.data_ptr(), d.ptr + 2, c)])
    stitch_refused("c 0", fields=lambda d: [(src.data_ptr(), d.ptr, 0)])
    stitch_refused("a null destination in the second field", fields=lambda d: [(src.data_ptr(), d.ptr, c), (src.data_ptr(), None, c)])


# ------------------------------------------------------------------------------------------------------------ end to end
P, S, BATCH = 32, 25, 4
SCENE = (3, 57, 64)  # 2 x 3 = 6 tiles: batches of tiles 0 ... 3 and 4, 5, 5, 5


def _mimo_member(dropout=0.0):
    from oracle import mimo_oracle as O
    from tests.test_network_gpu import build_model
    cfg = O.NetConfig(3, 2, 2, 4)
    return cfg, build_model(cfg, O.init_state(cfg, 3), dropout=(dropout,) * 3).eval()


def _evidential():
    from mimo.models.evidential_unet import EvidentialUnetModel
    torch.manual_seed(7)
    return EvidentialUnetModel(in_channels=3, out_channels=4, filter_base_count=4, center_dropout_rate=0.0,
                               final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
                               decoder_dropout_rate=0.0, weight_decay=0.0, learning_rate=1e-3, seed=0).cuda().eval()


def _deep():
    from mimo.models.ensemble import EnsembleModule
    return EnsembleModule([], models=[_mimo_member()[1]])  # keep_on_device=False: predict_scene stays on the device anyway


def _mc(passes=3, p=0.2):
    from mimo.models.ensemble import EnsembleModule
    from oracle import mimo_oracle as O
    cfg, model = _mimo_member(dropout=p)
    g = torch.Generator().manual_seed(5)
    # recorded Dropout2d masks for passes x BATCH samples: every batch of the scene draws the same ones
    model.model.mask_override = {j: torch.bernoulli(torch.full((passes * BATCH, cout), 1 - p), generator=g) / (1 - p)
                                 for j, (_, _, _, cout) in enumerate(O.double_conv_specs(cfg))}
    return EnsembleModule([], models=[model], monte_carlo_steps=passes, keep_on_device=True)


def _tiles_call(model, tiles):
    """the model's own (mean, aleatoric_var, epistemic_var) of a batch of tiles, on the device"""
    if hasattr(model, "predict_uncertainties"):
        return model.predict_uncertainties(tiles)
    return tuple(t.cuda() for t in model(tiles))


def _compare(got, want, spread, tag):
    """Bit for bit where the engine's forward repeated itself bit for bit on one batch, else within four times the
    measured run-to-run spread."""
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.shape == w.shape and np.all(np.isfinite(g)), (tag, k)
        diff = float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max())
        print(f"{tag} map {k}: run-to-run spread {spread[k]:.3e}, max |predict_scene - restatement| {diff:.3e}")
        if spread[k] == 0.0:
            assert np.array_equal(_bits(g), _bits(w)), (tag, k, diff)
        else:
            assert diff <= 4 * spread[k], (tag, k, diff, spread[k])


@pytest.mark.parametrize("kind", ["deep", "evidential", "mc_dropout"])
def test_predict_scene_equals_the_restated_stitch_of_the_model_s_tiles(kind):
    from mimo.inference import predict_scene
    model = {"deep": _deep, "evidential": _evidential, "mc_dropout": _mc}[kind]()
    scene = torch.rand(SCENE, generator=torch.Generator().manual_seed(1)).cuda()
    grid = R.Grid(SCENE[1], SCENE[2], P, S)
    T = grid.num_tiles
    assert T == 6
    # the route a user writes: tiles sliced by torch into the same padded batches of 4
    batches = []
    for t0 in range(0, T, BATCH):
        origins = [grid.origin(min(t0 + b, T - 1)) for b in range(BATCH)]
        batches.append(torch.stack([scene[:, oy:oy + P, ox:ox + P] for oy, ox in origins]).contiguous())
    first, again = _tiles_call(model, batches[0]), _tiles_call(model, batches[0])
    spread = [float((a.double() - b.double()).abs().max()) for a, b in zip(first, again)]
    per_map = [[] for _ in range(3)]
    for t0, tiles in zip(range(0, T, BATCH), batches):
        for k, r in enumerate(_tiles_call(model, tiles)):
            per_map[k].append(r[:min(BATCH, T - t0)].cpu().numpy())
    values = [np.concatenate(v) for v in per_map]  # [T, C_out, P, P]
    for window in ("linear", "crop") if kind == "deep" else ("linear",):
        want = [R.stitch_scene(v, grid, window, launch=BATCH) for v in values]
        got = predict_scene(model, scene, patch_size=P, stride=S, batch_size=BATCH, window=window)
        assert all(g.is_cuda and tuple(g.shape) == (1, SCENE[1], SCENE[2]) for g in got)
        _compare(got, want, spread, f"{kind}/{window}")
    if kind == "deep":  # a host scene is uploaded once, and the batching leaves the bits alone given the same tile values
        host = predict_scene(model, scene.cpu(), patch_size=P, stride=S, batch_size=BATCH)
        assert all(torch.equal(a, b) for a, b in zip(host, predict_scene(model, scene, patch_size=P, stride=S, batch_size=BATCH)))


@pytest.mark.parametrize("kind", ["deep", "evidential"])
def test_a_scene_of_one_patch_is_the_model_s_own_result(kind):
    """batch_size=1: the call shape of `model(scene[None])`, hence the same plan."""
    from mimo.inference import predict_scene
    model = {"deep": _deep, "evidential": _evidential}[kind]()
    scene = torch.rand(3, P, P, generator=torch.Generator().manual_seed(2)).cuda()
    first, again = _tiles_call(model, scene[None]), _tiles_call(model, scene[None])
    spread = [float((a.double() - b.double()).abs().max()) for a, b in zip(first, again)]
    want = [t[0].cpu().numpy() for t in first]
    for window in R.WINDOWS:
        got = predict_scene(model, scene, patch_size=P, stride=S, batch_size=1, window=window)
        _compare(got, want, spread, f"one patch/{kind}/{window}")
