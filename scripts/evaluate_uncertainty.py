"""Uncertainty evaluation of an ensemble on the GPU: precision_recall.csv + calibration.csv (the second half of the
reference's scripts/test/test_nyuv2_depth.py / test_ndvi.py), with HIP-event timings of the device route and the time
of the host route (the same tables from `.cpu()` copies: numpy argsort + 41 quantile sweeps) next to it.

    python scripts/evaluate_uncertainty.py --synthetic 8 --result_dir out            # seeded maps, no network
    python scripts/evaluate_uncertainty.py --synthetic_model --synthetic 2 --monte_carlo_steps 4 --result_dir out
    python scripts/evaluate_uncertainty.py --model_checkpoint_paths a.ckpt b.ckpt --batch_dir batches/ --result_dir out
    python scripts/evaluate_uncertainty.py --evidential --synthetic 2 --result_dir out   # a seeded EvidentialUnetModel
    python scripts/evaluate_uncertainty.py --evidential --model_checkpoint_paths ev.ckpt --batch_dir batches/ --result_dir out
    python scripts/evaluate_uncertainty.py --synthetic 8 --sources combined aleatoric epistemic --result_dir out
    python scripts/evaluate_uncertainty.py --synthetic_model --synthetic 2 --monte_carlo_steps 4 --scores --result_dir out
    python scripts/evaluate_uncertainty.py --evidential --synthetic 2 --scores --result_dir out

--scores: the proper scoring rules of the mixture predictive too (NLL, CRPS, PIT calibration of the equal-weight mixture of every
member density: `PredictiveScorer`), written to scores.csv and calibration_mixture.csv.  With a model the members are the
ensemble's raw outputs; with --synthetic alone three seeded Laplace members per pixel; with --evidential the one network's
Student-t posterior predictive (`PredictiveScorer.update_from_evidential`, reported with members = 1) under the same rules.

--sources: the sparsification curve per uncertainty source and the oracle curve (sparsification.csv), AUSE / AURG (ause.csv).

--evidential: ONE `EvidentialUnetModel` (one checkpoint, or a seeded network) fed through `predict_uncertainties`, as the
reference's scripts/test/test_nyuv2_depth_evidential.py / test_ndvi_evidential.py drive the model itself.

--batch_dir: `*.npy` files holding one dict each ({"image": [B,C,H,W], "label": [B,1,H,W], optional "mask"}), saved with
np.save(..., allow_pickle=True).  --synthetic N without a model feeds N seeded batches of (mean, aleatoric_var,
epistemic_var, label) maps of --batch x 1 x --size x --size straight into the evaluator."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimo.evaluation import PredictiveScorer, UncertaintyEvaluator  # noqa: E402


def seeded_maps(seed, b, size, device):
    g = torch.Generator(device=device).manual_seed(seed)
    shape = (b, 1, size, size)
    label = torch.rand(shape, generator=g, device=device) * 0.8 + 0.1
    a_std = torch.exp(torch.rand(shape, generator=g, device=device) * 2.3026 - 3.912)  # 0.02 .. 0.2
    mean = label + a_std * torch.randn(shape, generator=g, device=device)
    e_var = (0.3 * a_std * torch.randn(shape, generator=g, device=device)) ** 2
    return mean, a_std ** 2, e_var, label


def seeded_members(seed, b, size, device, members=3):
    """raw member outputs (p1, p2) [b, members, 1, size, size] around seeded_maps' mean and scale, and its label"""
    mean, a_var, _, label = seeded_maps(seed, b, size, device)
    g = torch.Generator(device=device).manual_seed(10_000 + seed)
    shape = (b, members, 1, size, size)
    scale = a_var.sqrt()[:, None] / 2 ** 0.5
    p1 = mean[:, None] + 0.3 * scale * torch.randn(shape, generator=g, device=device)
    p2 = torch.log(scale) + 0.2 * torch.randn(shape, generator=g, device=device)
    return p1, p2, label


def host_tables(batches, z, percentiles, clip=(0.0, 1.0)):
    """the reference's recipe on host copies, in numpy: what the device route replaces (batches: mean, aleatoric_var,
    epistemic_var, label, mask-or-None; masked pixels are dropped first)"""
    keep = np.concatenate([np.ones(b[0][:, 0].numel(), bool) if b[4] is None else (b[4].cpu().numpy()[:, 0].reshape(-1) != 0)
                           for b in batches])
    mu, av, ev, y = (np.concatenate([b[k].cpu().numpy()[:, 0].reshape(-1) for b in batches])[keep] for k in range(4))
    mu, y = np.clip(mu, *clip), np.clip(y, *clip)
    err, a_std, c_std = np.abs(y - mu), np.sqrt(av), np.sqrt(av + ev)
    e = err[np.argsort(-c_std, kind="stable")].astype(np.float64)
    suf, suf2 = np.cumsum(e[::-1])[::-1], np.cumsum((e * e)[::-1])[::-1]
    cut = (percentiles * e.size).astype(int)
    mae, rmse = suf[cut] / (e.size - cut), np.sqrt(suf2[cut] / (e.size - cut))
    s = a_std.astype(np.float64) / np.sqrt(2.0)
    with np.errstate(invalid="ignore"):
        obs = np.array([(y < mu + s * zk).mean() for zk in z])
    return mae, rmse, obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_checkpoint_paths", nargs="*", default=[])
    ap.add_argument("--synthetic_model", action="store_true", help="a seeded MIMO U-Net instead of checkpoints")
    ap.add_argument("--evidential", action="store_true", help="one EvidentialUnetModel instead of an ensemble")
    ap.add_argument("--monte_carlo_steps", type=int, default=0)
    ap.add_argument("--batch_dir")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--distribution", default="norm", choices=["norm", "laplace"])
    ap.add_argument("--sources", nargs="+", default=["combined"], choices=["combined", "aleatoric", "epistemic", "oracle"],
                    help="orderings of the sparsification curve; any beyond 'combined' adds the oracle, AUSE and AURG")
    ap.add_argument("--scores", action="store_true", help="NLL, CRPS and PIT calibration of the mixture predictive")
    ap.add_argument("--result_dir", required=True)
    ap.add_argument("--no_host_route", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    ensemble = None
    if args.evidential:
        from mimo.models.evidential_unet import EvidentialUnetModel
        if len(args.model_checkpoint_paths) > 1 or args.monte_carlo_steps:
            ap.error("--evidential takes one checkpoint and no --monte_carlo_steps")
        if args.model_checkpoint_paths:
            ensemble = EvidentialUnetModel.load_from_checkpoint(args.model_checkpoint_paths[0])
        else:
            torch.manual_seed(0)
            ensemble = EvidentialUnetModel(in_channels=3, out_channels=4, filter_base_count=8, center_dropout_rate=0.0,
                                           final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
                                           decoder_dropout_rate=0.0, weight_decay=0.0, learning_rate=1e-3, seed=0)
        ensemble = ensemble.to(dev).eval()
    elif args.model_checkpoint_paths or args.synthetic_model:
        from mimo.models.ensemble import EnsembleModule
        models = None
        if args.synthetic_model:
            from mimo.models.mimo_unet import MimoUnetModel
            torch.manual_seed(0)
            models = [MimoUnetModel(in_channels=3, out_channels=2, num_subnetworks=2, filter_base_count=8, center_dropout_rate=0.0,
                                    final_dropout_rate=0.0, encoder_dropout_rate=0.1, core_dropout_rate=0.1,
                                    decoder_dropout_rate=0.1, loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3, seed=0,
                                    loss_buffer_size=10, loss_buffer_temperature=0.3).cuda()]
        ensemble = EnsembleModule(args.model_checkpoint_paths, monte_carlo_steps=args.monte_carlo_steps, models=models,
                                  keep_on_device=True).to(dev)

    ev = UncertaintyEvaluator(distribution=args.distribution, sources=args.sources)
    scorer = PredictiveScorer() if args.scores else None
    kept, update_ms, masked = [], [], False
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed_update(maps, mask=None):
        e0.record()
        ev.update(*maps, mask=mask)
        e1.record()
        e1.synchronize()
        update_ms.append(e0.elapsed_time(e1))
        if not args.no_host_route:
            kept.append(tuple(t[:, :1] for t in maps) + (None if mask is None else mask[:, :1],))

    if ensemble is not None:
        if args.batch_dir:
            batches = [np.load(f, allow_pickle=True).item() for f in sorted(glob.glob(os.path.join(args.batch_dir, "*.npy")))]
        else:
            g = torch.Generator().manual_seed(1)
            batches = [{"image": torch.rand(args.batch, 3, args.size, args.size, generator=g),
                        "label": torch.rand(args.batch, 1, args.size, args.size, generator=g)} for _ in range(max(1, args.synthetic))]
        for b in batches:
            image, label = (torch.as_tensor(b[k]).to(dev) for k in ("image", "label"))
            mask = torch.as_tensor(b["mask"]).to(dev) if b.get("mask") is not None else None
            masked = masked or mask is not None
            if scorer is not None and args.evidential:  # a second forward; the Student-t predictive of the one network
                scorer.update_from_evidential(ensemble, image, label, mask)
            elif scorer is not None:  # a second forward: the evaluator's maps and the raw members are two return modes
                scorer.update_from(ensemble, image, label, mask)
            if args.no_host_route:
                ev.update_from(ensemble, image, label, mask)  # the three-line form of INTEGRATION.md
            else:  # the same two steps apart, to time the update alone and to keep the maps for the host route
                maps = ensemble.predict_uncertainties(image) if args.evidential else ensemble(image)
                timed_update(tuple(maps) + (label,), mask)
    else:
        if args.synthetic < 1:
            ap.error("give checkpoints, --synthetic_model or --synthetic N")
        ev.update(*seeded_maps(999, args.batch, args.size, dev))  # first call: allocations, code load
        ev.reset()
        for i in range(args.synthetic):
            timed_update(seeded_maps(i, args.batch, args.size, dev))
            if scorer is not None:
                scorer.update(*seeded_members(i, args.batch, args.size, dev))

    ev.compute()  # first call
    compute_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0.record()
        tables = ev.compute()
        e1.record()
        e1.synchronize()
        compute_ms.append(e0.elapsed_time(e1))
    ev.write_csv(args.result_dir, tables)

    pixels = args.batch * args.size * args.size
    res = {"n": tables["n"], "pixels_per_update": pixels, "compute_ms": [round(v, 3) for v in compute_ms], "mae": tables["mae"],
           "rmse": tables["rmse"]}
    if update_ms:
        # HIP events around one update(): the accumulate pass AND its 70-workgroup fold launch.  Bytes of the pass: four
        # fp32 maps in (five with a mask), one 8-byte record out (two with aleatoric / epistemic among the sources).
        records = 16 if {"aleatoric", "epistemic"} & set(args.sources) else 8
        res.update(update_ms_median=float(np.median(update_ms)), update_ms_min=float(np.min(update_ms)),
                   bytes_per_pixel=(20 if masked else 16) + records)
        res["update_GBps_at_min"] = res["bytes_per_pixel"] * pixels / (res["update_ms_min"] * 1e-3) / 1e9
    if scorer is not None:
        scores = scorer.compute()
        scorer.write_csv(args.result_dir, scores)
        members = 3 if ensemble is None else 1 if args.evidential else max(1, args.monte_carlo_steps) * ensemble.num_subnetworks
        res["scores"] = {k: scores[k] for k in ("n", "nll", "crps", "pit_mean", "calibration_error")}
        res["scores"].update(members=members, coverage_90=min(scores["coverage"].items(), key=lambda kv: abs(kv[0] - 0.9))[1])
    if "ause" in tables:
        res.update(ause=tables["ause"], aurg=tables["aurg"])
    if kept:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mae, rmse, obs = host_tables(kept, ev.z, ev.percentiles)
        res["host_route_s"] = time.perf_counter() - t0
        res["host_vs_device_mae_max_rel"] = float(np.nanmax(np.abs(mae - tables["precision_recall"]["mae"]) / mae))
        res["host_vs_device_observed_max_abs"] = float(np.abs(obs - tables["calibration"]["observed"]).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
