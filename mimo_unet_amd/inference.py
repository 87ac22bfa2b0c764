"""Whole-scene inference: hand the model one scene, get one map of prediction, aleatoric variance and epistemic variance.

The reference only knows patches: SEN12TP scenes are cut into 256-pixel patches at a stride of 249 by the dataset
(``scripts/test/test_ndvi.py:152-160``, ``sen12tp_datamodule.py:54-66``), `EnsembleModule.forward` and
`EvidentialUnetModel.predict_uncertainties` return tiles, and the cutting, the batching, the 7-pixel overlaps and the seams
are left to user code.  Here the scene stays in HBM and a batch is three launches: `mimo_scene_gather_tiles`, the model's
forward, `mimo_scene_stitch` for all three maps (``csrc/scene/scene_tiles.hip``; ``include/mimo_hip.h`` states the geometry,
the windows and the operation order in full).  Every batch, the last included, has `batch_size` rows — the gather repeats
the last tile, the stitch leaves the repeats out — so a scene runs on one inference plan and one captured graph.  No host
synchronisation, no index tensors, no weight-sum buffer and no finalising pass."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from . import _lib as L

WINDOWS = tuple(L.WINDOWS)


def axis_tiles(length: int, patch: int, stride: int) -> int:
    """n = 1 + ceil((L - P) / s) tiles along an axis of length L"""
    return 1 + -(-(length - patch) // stride)


class SceneTiler:
    """The tile grid of a ``[*, height, width]`` scene and the launches over it.

    Along each axis ``n = 1 + ceil((L - P) / s)`` tiles at ``o_k = min(k s, L - P)`` (the last tile is shifted inwards, never
    padded), numbered row-major.  Holds the tile buffers of `gather` (one per call shape, reused from batch to batch: a
    captured forward keeps reading the same address) and hands out the scene maps `stitch` adds into."""

    def __init__(self, height: int, width: int, patch_size: int = 256, stride: int = 249, window: str = "linear") -> None:
        height, width, patch_size, stride = int(height), int(width), int(patch_size), int(stride)
        if patch_size < 1:
            raise ValueError(f"SceneTiler: patch_size {patch_size} must be >= 1")
        if height < patch_size or width < patch_size:
            raise ValueError(f"SceneTiler: a {height} x {width} scene is smaller than the {patch_size}-pixel patch")
        if not 1 <= stride <= patch_size:
            raise ValueError(f"SceneTiler: stride {stride} outside [1, patch_size = {patch_size}]")
        if window not in L.WINDOWS:
            raise ValueError(f"SceneTiler: unknown window {window!r} (one of {', '.join(WINDOWS)})")
        self.height, self.width, self.patch_size, self.stride, self.window = height, width, patch_size, stride, window
        self.ny, self.nx = axis_tiles(height, patch_size, stride), axis_tiles(width, patch_size, stride)
        self.num_tiles = self.ny * self.nx
        self._tiles = {}  # (batch, channels, device) -> [batch, channels, P, P]

    def origins(self) -> List[Tuple[int, int]]:
        """(oy, ox) of tiles 0 ... num_tiles - 1"""
        oy = [min(k * self.stride, self.height - self.patch_size) for k in range(self.ny)]
        ox = [min(k * self.stride, self.width - self.patch_size) for k in range(self.nx)]
        return [(y, x) for y in oy for x in ox]

    def num_batches(self, batch_size: int) -> int:
        return -(-self.num_tiles // batch_size)

    def _require_scene(self, t: torch.Tensor, what: str) -> None:
        if (t.dim() != 3 or tuple(t.shape[1:]) != (self.height, self.width) or t.dtype != torch.float32 or not t.is_cuda
                or not t.is_contiguous()):
            raise ValueError(f"{what}: a contiguous fp32 [C, {self.height}, {self.width}] device tensor is needed, got "
                             f"{t.dtype} {list(t.shape)} on {t.device}")

    def scene_buffer(self, channels: int, device) -> torch.Tensor:
        """An uninitialised ``[channels, height, width]`` map: `stitch` stores a pixel's first term, so no memset is needed
        when the launches of a scene cover tiles 0 ... num_tiles - 1 in ascending order."""
        return torch.empty(channels, self.height, self.width, dtype=torch.float32, device=device)

    def gather(self, scene: torch.Tensor, t0: int, batch_size: int) -> torch.Tensor:
        """Tiles ``min(t0 + b, num_tiles - 1)``, b = 0 ... batch_size - 1, as ``[batch_size, C, P, P]``: one launch on the
        current stream into this tiler's buffer for the call shape (overwritten by the next `gather` of that shape)."""
        self._require_scene(scene, "SceneTiler.gather")
        if batch_size < 1 or not 0 <= t0 < self.num_tiles:
            raise ValueError(f"SceneTiler.gather: batch_size {batch_size}, first tile {t0} of {self.num_tiles}")
        c, p = int(scene.shape[0]), self.patch_size
        key = (int(batch_size), c, scene.device)
        tiles = self._tiles.get(key)
        if tiles is None:
            tiles = self._tiles[key] = torch.empty(batch_size, c, p, p, dtype=torch.float32, device=scene.device)
        with torch.cuda.device(scene.device):
            L.check(L.load().mimo_scene_gather_tiles(scene.data_ptr(), tiles.data_ptr(), c, self.height, self.width, p,
                                                     self.stride, t0, batch_size, L.current_stream()),
                    "mimo_scene_gather_tiles")
        return tiles

    def stitch(self, fields: Sequence[Tuple[torch.Tensor, torch.Tensor]], t0: int, n_valid: int) -> None:
        """Adds tiles t0 ... t0 + n_valid - 1 into the scene maps, one launch for up to four ``(tiles [n, c, P, P], scene
        [c, H, W])`` pairs; row b of `tiles` is tile t0 + b, rows from n_valid on are left out."""
        if not 1 <= len(fields) <= 4:
            raise ValueError(f"SceneTiler.stitch: {len(fields)} fields (1 ... 4 per launch)")
        p = self.patch_size
        for src, dst in fields:
            self._require_scene(dst, "SceneTiler.stitch")
            if (src.dim() != 4 or tuple(src.shape[1:]) != (dst.shape[0], p, p) or src.shape[0] < n_valid
                    or src.dtype != torch.float32 or src.device != dst.device or not src.is_contiguous()):
                raise ValueError(f"SceneTiler.stitch: a contiguous fp32 [n >= {n_valid}, {dst.shape[0]}, {p}, {p}] tensor on "
                                 f"{dst.device} is needed, got {src.dtype} {list(src.shape)} on {src.device}")
        table = (L.StitchField * len(fields))(*(L.StitchField(src.data_ptr(), dst.data_ptr(), int(dst.shape[0]), 0)
                                                for src, dst in fields))
        with torch.cuda.device(fields[0][1].device):
            L.check(L.load().mimo_scene_stitch(table, len(fields), self.height, self.width, p, self.stride,
                                               L.WINDOWS[self.window], t0, n_valid, L.current_stream()), "mimo_scene_stitch")


def _tile_predictor(model):
    """(in_channels, tiles [B,C,P,P] -> three [B,C_out,P,P] device tensors) of an `EnsembleModule` or a bare
    `EvidentialUnetModel`"""
    from .models.ensemble import EnsembleModule
    from .models.evidential_unet import EvidentialUnetModel
    if isinstance(model, EvidentialUnetModel):
        return model.in_channels, model.predict_uncertainties
    if isinstance(model, EnsembleModule):
        if model.return_raw_predictions:
            raise ValueError("predict_scene stitches (mean, aleatoric_var, epistemic_var); an EnsembleModule with "
                             "return_raw_predictions=True returns the subnetworks' raw parameters")
        return model.models[0].in_channels, model.forward_on_device
    raise TypeError(f"predict_scene takes an EnsembleModule or an EvidentialUnetModel, got {type(model).__name__}")


def predict_scene(model, scene: torch.Tensor, *, patch_size: int = 256, stride: int = 249, batch_size: int = 32,
                  window: str = "linear"):
    """scene ``[C_in, H, W]`` fp32 -> ``(mean, aleatoric_var, epistemic_var)``, each ``[C_out, H, W]`` on the device.

    model: an `EnsembleModule` (deep or MC-dropout, either setting of `keep_on_device`) or a bare `EvidentialUnetModel`
    in eval mode, on the device.  A host scene is uploaded once.  Each batch is one gather launch, the model's forward and
    one stitch launch for all three maps; overlaps are blended with `window` ("linear": a tent that favours tile centres,
    "uniform": the plain mean, "crop": each pixel from the tile whose centre is nearest).  The stitched maps are
    bit-identical for any `batch_size` given the same tile results."""
    if scene.dim() != 3:
        raise ValueError(f"predict_scene: scene must be [C_in, H, W], got {list(scene.shape)}")
    if int(batch_size) < 1:
        raise ValueError(f"predict_scene: batch_size {batch_size} must be >= 1")
    tiler = SceneTiler(scene.shape[1], scene.shape[2], patch_size, stride, window)
    in_channels, predict = _tile_predictor(model)
    if scene.shape[0] != in_channels:
        raise ValueError(f"predict_scene: the scene has {scene.shape[0]} channels, the model takes {in_channels}")
    if not scene.is_cuda:
        device = next(iter(model.parameters())).device if not hasattr(model, "models") else model.device
        if device.type != "cuda":
            raise L.MimoHipError("predict_scene runs on an AMD GPU through libmimo_hip.so; move the model to cuda")
        scene = scene.to(device)
    scene = scene.detach().contiguous().float()
    batch_size = int(batch_size)
    maps = None
    for t0 in range(0, tiler.num_tiles, batch_size):
        results = predict(tiler.gather(scene, t0, batch_size))
        if maps is None:
            maps = [tiler.scene_buffer(r.shape[1], scene.device) for r in results]
        tiler.stitch([(r.contiguous(), m) for r, m in zip(results, maps)], t0, min(batch_size, tiler.num_tiles - t0))
    return tuple(maps)
