"""Independent float64 numpy restatement of the per-source sparsification curves, the oracle curve and their areas
(AUSE, Ilg et al. 2018; AURG, Poggi et al. 2020).  It shares no code with mimo_unet_amd/evaluation.py and builds on
tests/eval_reference.py: per source a stable descending argsort of the float32 key, then suffix means of the float32
error at `(percentiles * N).astype(int)`, everything after the keys in float64.

The four keys of a kept pixel: combined = sqrt(aleatoric_var + epistemic_var) (float32 sum first), aleatoric =
sqrt(aleatoric_var), epistemic = sqrt(epistemic_var), oracle = the pixel's own |error|."""
import numpy as np

from tests import eval_reference as R

SOURCES = ("combined", "aleatoric", "epistemic", "oracle")


def source_keys(mean, aleatoric_var, epistemic_var, label, mask=None, clip=(0.0, 1.0), channel=0):
    """[B,C,H,W] float32 maps -> ({source: float32 key per kept pixel}, float32 error per kept pixel, eval_reference's
    columns).  The kept pixels are eval_reference.pixel_columns' (mask != 0, everything finite, variances >= 0)."""
    cols = R.pixel_columns(mean, aleatoric_var, epistemic_var, label, mask=mask, clip=clip, channel=channel)
    pick = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32)[:, channel]).reshape(-1)
    mu, av, ev, y = pick(mean), pick(aleatoric_var), pick(epistemic_var), pick(label)
    with np.errstate(all="ignore"):
        keep = np.isfinite(mu) & np.isfinite(av) & np.isfinite(ev) & np.isfinite(y) & (av >= 0) & (ev >= 0) & np.isfinite(av + ev)
    if mask is not None:
        m = np.asarray(mask, dtype=np.float32)
        keep &= m[:, 0 if m.shape[1] == 1 else channel].reshape(-1) != 0
    assert int(keep.sum()) == cols["error"].size
    # |.|: the square root of a variance of -0.0 is -0.0, which is the key 0 like +0.0
    keys = {"combined": cols["combined_std"], "aleatoric": np.abs(np.sqrt(av[keep])), "epistemic": np.abs(np.sqrt(ev[keep])),
            "oracle": cols["error"]}
    assert np.array_equal(keys["aleatoric"], np.abs(cols["aleatoric_std"]))
    assert all(k.dtype == np.float32 for k in keys.values())
    return keys, cols["error"], cols


def as_columns(key, error):
    """a key in the place eval_reference.sparsification (and the tie rule of tests/test_evaluation_gpu.py) sorts by"""
    return {"combined_std": key, "error": error}


def curve(key, error, percentiles):
    """eval_reference.sparsification with `key` as the ordering: mae, rmse, cutoff, cutoff_keys, sorted_desc"""
    return R.sparsification(as_columns(key, error), percentiles)


def curves(keys, error, percentiles):
    return {name: curve(key, error, percentiles) for name, key in keys.items()}


def trapezoid(x, y):
    total = 0.0
    for i in range(len(x) - 1):
        total += (float(x[i + 1]) - float(x[i])) * (float(y[i]) + float(y[i + 1])) / 2.0
    return total


def areas(percentiles, rows, oracle_rows, normalize=False):
    """(AUSE, AURG): trapezoid rule over the rows where both curves are finite.  AUSE = area between the curve and the
    oracle; AURG = area between the random-removal curve (the constant whole-set value, row 0) and the curve."""
    x, c, o = (np.asarray(a, dtype=np.float64) for a in (percentiles, rows, oracle_rows))
    ok = np.isfinite(c) & np.isfinite(o)
    x, c, o = x[ok], c[ok], o[ok]
    if normalize:
        c, o = c / c[0], o / o[0]
    return trapezoid(x, c - o), trapezoid(x, c[0] - c)
