"""Generate tests/golden/eval_tables.npz from the REAL reference's evaluation code.

    python tests/golden/make_eval_golden.py --reference /path/to/MIMO-Unet

Loads the reference's scripts/test/test_nyuv2_depth.py as a module and calls its own `compute_uncertainties`,
`convert_to_pandas`, `compute_metrics`, `create_precision_recall_plot` and `create_calibration_plot` (with
scipy.stats.norm, as its main() does) on seeded inputs.  The script's two package imports need `lightning` and `h5py`;
the functions used here touch neither, so empty stand-in modules carrying the two imported names are registered first.
Needs pandas, scipy and tqdm.  Only arrays are stored: nothing of the reference's text enters the repository.

Stored per data set `<name>/`: the four float32 maps fed to the evaluator (mean, aleatoric_var, epistemic_var, label),
for the two (y_pred, log_param) pairs also those, and the reference's tables `pr` [100,3] (percentile, mae, rmse) and
`cal` [41,2] (expected, observed); `z_norm`: scipy.stats.norm.ppf of the 41 expected confidences."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import eval_reference as R  # noqa: E402


def load_reference(ref):
    for name, attr in (("mimo.models.ensemble", "EnsembleModule"), ("mimo.datasets.nyuv2", "NYUv2DepthDataset")):
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
        setattr(sys.modules[name], attr, type(attr, (), {}))
    mods = {}
    for key, rel in (("test_nyuv2_depth", "scripts/test/test_nyuv2_depth.py"), ("reference_losses", "mimo/losses.py")):
        spec = importlib.util.spec_from_file_location(key, os.path.join(ref, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[key] = mod  # create_calibration_plot pickles compute_ppf for its process pool
        spec.loader.exec_module(mod)
        mods[key] = mod
    return mods["test_nyuv2_depth"], mods["reference_losses"]


def reference_tables(T, mean, a_var, e_var, label):
    """make_predictions' tail (test_nyuv2_depth.py:73-90) + main()'s table block (:215-234) on [B,1,H,W] maps"""
    import scipy.stats
    t = lambda a: torch.from_numpy(a)
    y_pred, y_true = t(mean).clip(min=0, max=1)[:, 0], t(label).clip(min=0, max=1)[:, 0]
    av, ev = t(a_var)[:, 0], t(e_var)[:, 0]
    df = T.compute_metrics(T.convert_to_pandas(y_pred, y_true, av, ev, av + ev))
    pr = T.create_precision_recall_plot(df)
    cal = T.create_calibration_plot(df, scipy.stats.norm, processes=1)
    return pr.to_numpy(dtype=np.float64), cal.to_numpy(dtype=np.float64)


def suitable(maps, z):
    """the conditions the GPU tests assert of their inputs: no tie straddles a cutoff, thin comparison bands"""
    cols = R.pixel_columns(*maps)
    sp = R.sparsification(cols, np.arange(100) / 100.0)
    cal = R.calibration(cols, z)
    return not R.straddling_ties(sp["sorted_desc"], sp["cutoff"]) and cal["band"].max() <= 1e-4 * cols["error"].size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MIMO_REFERENCE"), required="MIMO_REFERENCE" not in os.environ)
    args = ap.parse_args()
    import scipy.stats
    T, losses = load_reference(args.reference)
    z = scipy.stats.norm.ppf(np.arange(41) / 40.0)
    out = {"z_norm": z}

    seed = 0
    while not suitable(R.synthetic_maps(seed, 4, 1, 64, 64), z):
        seed += 1
    maps = R.synthetic_maps(seed, 4, 1, 64, 64)
    out["maps/seed"] = np.int64(seed)
    for k, a in zip(("mean", "aleatoric_var", "epistemic_var", "label"), maps):
        out[f"maps/{k}"] = a
    out["maps/pr"], out["maps/cal"] = reference_tables(T, *maps)

    # (y_pred, log_param) pairs with S = 3: the four maps come from the reference's own compute_uncertainties
    for name, crit in (("laplace", losses.LaplaceNLL()), ("gaussian", losses.GaussianNLL())):
        seed = 100
        while True:
            g = np.random.default_rng(seed)
            label = g.uniform(0.1, 0.9, (2, 1, 32, 32)).astype(np.float32)
            y_pred = (label[:, None] + 0.05 * g.normal(size=(2, 3, 1, 32, 32))).astype(np.float32)
            log_param = g.uniform(-4.0, -2.0, (2, 3, 1, 32, 32)).astype(np.float32)
            yp = torch.from_numpy(y_pred).clip(min=0, max=1)
            av, ev = T.compute_uncertainties(crit, y_preds=yp, log_params=torch.from_numpy(log_param))
            maps = (yp.mean(axis=1).numpy(), av.numpy(), ev.numpy(), label)
            if suitable(maps, z):
                break
            seed += 1
        out[f"{name}/seed"] = np.int64(seed)
        out[f"{name}/y_pred"], out[f"{name}/log_param"] = y_pred, log_param
        for k, a in zip(("mean", "aleatoric_var", "epistemic_var", "label"), maps):
            out[f"{name}/{k}"] = np.ascontiguousarray(a, dtype=np.float32)
        out[f"{name}/pr"], out[f"{name}/cal"] = reference_tables(T, *maps)

    path = os.path.join(HERE, "eval_tables.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: int(v) for k, v in out.items() if k.endswith("seed")})


if __name__ == "__main__":
    main()
