"""numpy restatement of the whole-scene tiling (include/mimo_hip.h, "whole-scene inference"): the tile grid, the three
windows, the normalised fp32 weights, `mimo_scene_gather_tiles` and `mimo_scene_stitch` with the kernel's operation order.

Nothing here is shared with the library or with mimo_unet_amd/inference.py: the covering ranges are found by testing every
tile against the definition o_k <= p < o_k + P, not by the closed forms the kernel uses.

Every fp32 operation is one numpy operation on float32 operands (numpy rounds each to nearest and never fuses), so the
restatement defines every bit of the stitched scene."""
import numpy as np

WINDOWS = ("uniform", "linear", "crop")
F32 = np.float32


def axis_tiles(length, patch, stride):
    """n = 1 + ceil((L - P) / s)"""
    assert 1 <= stride <= patch <= length, (length, patch, stride)
    return 1 + -(-(length - patch) // stride)


def axis_origins(length, patch, stride):
    """o_k = min(k s, L - P): the last tile is shifted inwards"""
    return [min(k * stride, length - patch) for k in range(axis_tiles(length, patch, stride))]


def covering(length, patch, stride):
    """per position p the ascending list K(p) = [k : o_k <= p < o_k + P]"""
    origins = axis_origins(length, patch, stride)
    return [[k for k, o in enumerate(origins) if o <= p < o + patch] for p in range(length)]


def linear_window(i, patch):
    return min(i + 1, patch - i)


def axis_owner(length, patch, stride):
    """per position the k in K(p) with the largest linear weight, ties to the lowest k"""
    origins = axis_origins(length, patch, stride)
    owners = []
    for p, ks in enumerate(covering(length, patch, stride)):
        weights = [linear_window(p - origins[k], patch) for k in ks]
        owners.append(ks[weights.index(max(weights))])  # index(): the first, i.e. the lowest k
    return owners


def axis_weights(length, patch, stride, window):
    """a [n, L] float32: the normalised 1-D weight of tile k at position p, 0 where the tile does not cover p.
    uniform / linear: w(p - o_k) / sum over ascending j in K(p) of w(p - o_j) — an exact integer sum, one fp32 division.
    crop: 1 for the owner, 0 otherwise."""
    assert window in WINDOWS, window
    origins = axis_origins(length, patch, stride)
    a = np.zeros((len(origins), length), dtype=F32)
    if window == "crop":
        for p, k in enumerate(axis_owner(length, patch, stride)):
            a[k, p] = 1.0
        return a
    for p, ks in enumerate(covering(length, patch, stride)):
        w = [1 if window == "uniform" else linear_window(p - origins[k], patch) for k in ks]
        total = 0
        for v in w:  # ascending j; small integers, exact
            total += v
        assert total < 1 << 24
        for k, v in zip(ks, w):
            a[k, p] = F32(v) / F32(total)
    return a


class Grid:
    """The tile grid of a scene [h, w]: tiles numbered row-major, t = ky nx + kx."""

    def __init__(self, h, w, patch, stride):
        self.h, self.w, self.patch, self.stride = h, w, patch, stride
        self.oy, self.ox = axis_origins(h, patch, stride), axis_origins(w, patch, stride)
        self.ny, self.nx = len(self.oy), len(self.ox)
        self.num_tiles = self.ny * self.nx
        self.ky_of, self.kx_of = covering(h, patch, stride), covering(w, patch, stride)
        self._weights = {}

    def weights(self, window):
        """(a_y [ny, h], a_x [nx, w]) of `axis_weights`, computed once per window"""
        if window not in self._weights:
            self._weights[window] = (axis_weights(self.h, self.patch, self.stride, window),
                                     axis_weights(self.w, self.patch, self.stride, window))
        return self._weights[window]

    def origin(self, t):
        return self.oy[t // self.nx], self.ox[t % self.nx]

    def origins(self):
        return [self.origin(t) for t in range(self.num_tiles)]


def gather(scene, grid, t0, n):
    """dst[b, c, y, x] = scene[c, oy(t) + y, ox(t) + x] with t = min(t0 + b, T - 1)"""
    P = grid.patch
    out = np.empty((n, scene.shape[0], P, P), dtype=scene.dtype)
    for b in range(n):
        oy, ox = grid.origin(min(t0 + b, grid.num_tiles - 1))
        out[b] = scene[:, oy:oy + P, ox:ox + P]
    return out


def stitch(dst, tiles, grid, window, t0, n_valid):
    """One launch: adds tiles t0 ... t0 + n_valid - 1 (rows 0 ... n_valid - 1 of `tiles` [n, c, P, P]) into dst [c, h, w]
    in place, pixel by pixel in ascending t.  A pixel whose lowest covering tile overall is >= t0 is stored (the first
    term assigned), any other is read and added to; pixels no tile of the launch covers are not touched."""
    assert 0 <= t0 and 1 <= n_valid and t0 + n_valid <= grid.num_tiles and n_valid <= tiles.shape[0]
    assert dst.dtype == F32 and tiles.dtype == F32
    ay, ax = grid.weights(window)
    t1 = t0 + n_valid - 1
    rows = sorted({y for t in range(t0, t1 + 1) for y in range(grid.origin(t)[0], grid.origin(t)[0] + grid.patch)})
    for y in rows:
        for x in range(grid.w):
            kys, kxs = grid.ky_of[y], grid.kx_of[x]
            started = kys[0] * grid.nx + kxs[0] < t0  # an earlier launch holds the pixel's first terms
            for ky in kys:  # ky outer, kx inner: ascending t
                for kx in kxs:
                    t = ky * grid.nx + kx
                    if not t0 <= t <= t1:
                        continue
                    v = tiles[t - t0, :, y - grid.oy[ky], x - grid.ox[kx]]  # all channels
                    if window == "crop":
                        if ay[ky, y] == 1.0 and ax[kx, x] == 1.0:
                            dst[:, y, x] = v  # a pure copy of the owner's value
                        continue
                    term = (ay[ky, y] * ax[kx, x]) * v  # fl(fl(a_ky a_kx) v): float32 operands, one rounding each
                    dst[:, y, x] = dst[:, y, x] + term if started else term
                    started = True
    return dst


def stitch_scene(tiles, grid, window, launch, fill=np.nan):
    """All T tiles [T, c, P, P] stitched in launches of `launch` tiles into a destination pre-filled with `fill`."""
    dst = np.full((tiles.shape[1], grid.h, grid.w), fill, dtype=F32)
    for t0 in range(0, grid.num_tiles, launch):
        n_valid = min(launch, grid.num_tiles - t0)
        stitch(dst, tiles[t0:t0 + n_valid], grid, window, t0, n_valid)
    return dst


def stitch_fp64(tiles, grid, window):
    """An independent formulation in float64: np.add.at of w v and of w over all tiles, then one division; the window is
    the UN-normalised 2-D product w(y) w(x) (crop: the 0 / 1 ownership product)."""
    P = grid.patch
    num = np.zeros((tiles.shape[1], grid.h, grid.w))
    den = np.zeros((grid.h, grid.w))
    if window == "crop":
        own_y, own_x = axis_owner(grid.h, P, grid.stride), axis_owner(grid.w, P, grid.stride)
    for t in range(grid.num_tiles):
        ky, kx = divmod(t, grid.nx)
        oy, ox = grid.origin(t)
        if window == "uniform":
            wy = wx = np.ones(P)
        elif window == "linear":
            wy = wx = np.array([linear_window(i, P) for i in range(P)], dtype=np.float64)
        else:
            wy = np.array([1.0 if own_y[oy + i] == ky else 0.0 for i in range(P)])
            wx = np.array([1.0 if own_x[ox + i] == kx else 0.0 for i in range(P)])
        w2 = np.outer(wy, wx)
        yy, xx = np.meshgrid(np.arange(oy, oy + P), np.arange(ox, ox + P), indexing="ij")
        np.add.at(den, (yy, xx), w2)
        for c in range(tiles.shape[1]):
            np.add.at(num[c], (yy, xx), w2 * tiles[t, c].astype(np.float64))
    return num / den
