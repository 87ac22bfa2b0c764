"""Independent float64 numpy restatement of the reference's two evaluation tables (scripts/test/test_nyuv2_depth.py:
93-170): a stable argsort and suffix means for `precision_recall.csv`, `y < ppf` for `calibration.csv`.  It shares no
code with mimo_unet_amd/evaluation.py: the standard quantiles are passed in by the caller.

The per-pixel quantities are formed the way the reference's frame holds them — float32 clamp, float32 `error`, float32
square roots (numpy on float32 arrays) — and everything after that is float64."""
import numpy as np


def pixel_columns(mean, aleatoric_var, epistemic_var, label, mask=None, clip=(0.0, 1.0), channel=0):
    """[B,C,H,W] float32 maps -> dict of flat float32 columns of the kept pixels + the skip counts."""
    pick = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32)[:, channel]).reshape(-1)
    mu, av, ev, y = pick(mean), pick(aleatoric_var), pick(epistemic_var), pick(label)
    keep = np.ones(mu.shape, dtype=bool)
    if mask is not None:
        m = np.asarray(mask, dtype=np.float32)
        keep = (m[:, 0 if m.shape[1] == 1 else channel].reshape(-1) != 0)
    with np.errstate(all="ignore"):
        var = av + ev  # float32 sum first
        finite = np.isfinite(mu) & np.isfinite(av) & np.isfinite(ev) & np.isfinite(y) & (av >= 0) & (ev >= 0) & np.isfinite(var)
    n_masked = int((~keep).sum())
    n_nonfinite = int((keep & ~finite).sum())
    keep &= finite
    mu, av, var, y = mu[keep], av[keep], var[keep], y[keep]
    if clip is not None:
        mu, y = np.clip(mu, np.float32(clip[0]), np.float32(clip[1])), np.clip(y, np.float32(clip[0]), np.float32(clip[1]))
    return {"y_pred": mu, "y_true": y, "error": np.abs(y - mu), "aleatoric_std": np.sqrt(av), "combined_std": np.sqrt(var),
            "n_masked": n_masked, "n_nonfinite": n_nonfinite}


def cutoffs(percentiles, n):
    return (np.asarray(percentiles, dtype=np.float64) * n).astype(int)


def sparsification(cols, percentiles):
    """mae / rmse of the pixels left after dropping the int(q N) most uncertain ones; also the descending-sorted
    combined_std (float32) for tie checks."""
    std, err = cols["combined_std"], cols["error"]
    n = std.size
    order = np.argsort(-std.astype(np.float64), kind="stable")
    e = err[order].astype(np.float64)
    suf = np.concatenate([np.cumsum(e[::-1])[::-1], [0.0]])
    suf2 = np.concatenate([np.cumsum((e * e)[::-1])[::-1], [0.0]])
    cut = cutoffs(percentiles, n)
    left = (n - cut).astype(np.float64)
    with np.errstate(all="ignore"):
        mae, rmse = suf[cut] / left, np.sqrt(suf2[cut] / left)
    keys = np.where(cut < n, std[order][np.minimum(cut, n - 1)], np.nan)  # the most uncertain survivor
    return {"mae": mae, "rmse": rmse, "cutoff": cut, "cutoff_keys": keys.astype(np.float64), "sorted_desc": std[order]}


def straddling_ties(sorted_desc, cut):
    """cutoffs that fall inside a run of identical combined_std values (where pandas' unstable sort leaves the
    reference's row undefined)"""
    n = sorted_desc.size
    return [int(c) for c in cut if 0 < c < n and sorted_desc[c - 1] == sorted_desc[c]]


def calibration(cols, z):
    """observed counts per threshold in float64 (`y_true < loc + scale * z`, scale = aleatoric_std / sqrt 2; NaN for
    scale == 0 as scipy's ppf gives) and the number of pixels within the fp32 comparison band of each quantile."""
    y, mu = cols["y_true"].astype(np.float64), cols["y_pred"].astype(np.float64)
    s = cols["aleatoric_std"].astype(np.float64) / np.sqrt(2.0)
    counts, band = np.zeros(len(z), dtype=np.int64), np.zeros(len(z), dtype=np.int64)
    with np.errstate(all="ignore"):
        for k, zk in enumerate(np.asarray(z, dtype=np.float64)):
            ppf = np.where(s > 0, mu + s * zk, np.nan)
            counts[k] = int((y < ppf).sum())
            delta = 2.0 ** -21 * (np.abs(y) + np.abs(mu) + np.abs(s * zk))
            band[k] = int((np.abs(y - ppf) <= delta).sum()) if np.isfinite(zk) else 0
    return {"counts": counts, "band": band, "observed": counts / max(y.size, 1)}


def synthetic_maps(seed, b, c, h, w, noise="laplace"):
    """Seeded float32 maps shaped like an ensemble's output on a regression task in [0, 1]: a label, an aleatoric
    standard deviation spread over a decade, a mean that misses the label by noise of that scale, a small epistemic part."""
    g = np.random.default_rng(seed)
    shape = (b, c, h, w)
    label = g.uniform(0.1, 0.9, shape)
    a_std = np.exp(g.uniform(np.log(0.02), np.log(0.2), shape))
    eps = g.laplace(0.0, 1.0 / np.sqrt(2.0), shape) if noise == "laplace" else g.normal(0.0, 1.0, shape)
    mean = label + a_std * eps * g.uniform(0.5, 1.5, shape)
    e_var = (0.3 * a_std * g.normal(0.0, 1.0, shape)) ** 2
    f = lambda a: a.astype(np.float32)
    return f(mean), f(a_std ** 2), f(e_var), f(label)
