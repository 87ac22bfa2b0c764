"""Timings of `PredictiveScorer` on the GPU, next to a torch restatement of the same formulas on the same device:

    python scripts/measure_scores.py            # writes profiles/scores/summary.txt

`update` and `compute` at 5 x 256^2 and 32 x 256^2 pixels, both losses, S_total = 3 (one MIMO model), 12 (four checkpoints)
and 24 (8 MC passes x 3).  Each figure is the median (and the minimum) of --reps calls between HIP events after --warmup
calls of the same shape; the two routes alternate inside one process.  The torch route forms the [B,S,S,H,W] pair
broadcast in chunks of images that keep one temporary under --chunk_mb.  For S_total = 3 the achieved bytes per second of
`update` (8 S + 4 bytes per pixel over the time of the call: the pass and its fold launch) stand next to those of
`UncertaintyEvaluator.update` (16 bytes in, 8 out) at the same pixel count.  No GPU: the script fails."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimo.evaluation import PredictiveScorer, UncertaintyEvaluator  # noqa: E402

EPS_MIN, EPS_MAX = 1e-5, 1e3


def gauss_abs_mean(m, s):
    z = m / s
    return 2 * s * (0.3989422804014327 * torch.exp(-0.5 * z * z)) + m * torch.erf(z * 0.7071067811865476)


def torch_scores(p1, p2, y, loss):
    """sums of (nll, crps, pit) over the pixels of p1 / p2 [b,S,H,W], y [b,H,W]: the kernel's formulas in fp32 torch"""
    S = p1.shape[1]
    th = torch.exp(p2).clamp(EPS_MIN, EPS_MAX)
    d = y[:, None] - p1
    if loss == "laplace_nll":
        ad = d.abs()
        e = torch.exp(-ad / th)
        F = torch.where(d < 0, 0.5 * e, 1 - 0.5 * e)
        lf = -ad / th - torch.log(2 * th)
        a = ad + th * e
        D = (p1[:, :, None] - p1[:, None]).abs()
        bi, bj = torch.minimum(th[:, :, None], th[:, None]), torch.maximum(th[:, :, None], th[:, None])
        x = D * (bi - bj) / (bi * bj)
        g = torch.where(x == 0, torch.ones_like(x), torch.expm1(x) / torch.where(x == 0, torch.ones_like(x), x))
        c = D + torch.exp(-D / bi) * ((bi * bi + bi * bj + bj * bj) / (bi + bj)) + torch.exp(-D / bj) * (bj / (bi + bj)) * (bj / bi) * D * g
    else:
        sd = th.sqrt()
        z = d / sd
        F = 0.5 * torch.erfc(-z * 0.7071067811865476)
        lf = -0.5 * z * z - torch.log(sd) - 0.9189385332046727
        a = gauss_abs_mean(d, sd)
        c = gauss_abs_mean((p1[:, :, None] - p1[:, None]).abs(), (th[:, :, None] + th[:, None]).sqrt())
    nll = -(torch.logsumexp(lf, dim=1) - math.log(S))
    crps = a.mean(dim=1) - c.sum(dim=(1, 2)) / (2 * S * S)  # the full S x S sum: the diagonal is c_ii
    return torch.stack([nll.double().sum(), crps.double().sum(), F.mean(dim=1).double().sum()])


def torch_route(p1, p2, y, loss, chunk):
    tot = torch.zeros(3, dtype=torch.float64, device=p1.device)
    for b0 in range(0, p1.shape[0], chunk):
        tot += torch_scores(p1[b0:b0 + chunk, :, 0], p2[b0:b0 + chunk, :, 0], y[b0:b0 + chunk, 0], loss)
    return tot


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "scores", "summary.txt"))
    ap.add_argument("--batches", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--members", type=int, nargs="+", default=[3, 12, 24])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk_mb", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_scores.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"PredictiveScorer on {torch.cuda.get_device_name(0)}: HIP-event times in ms, median (min) of {args.reps} calls after "
             f"{args.warmup} warm-up calls; {args.size} x {args.size} images, one channel, no mask",
             "torch: the same formulas in fp32 torch on the same GPU ([B,S,S,H,W] broadcast in image chunks); "
             "ratio = torch median / update median", "",
             f"{'loss':12s} {'B':>3s} {'S':>3s} {'update':>16s} {'compute':>16s} {'torch':>18s} {'ratio':>7s} {'GB/s':>7s} {'max rel diff of the means':>26s}"]
    eval_lines = []
    for loss in ("laplace_nll", "gaussian_nll"):
        for B in args.batches:
            for S in args.members:
                g = torch.Generator(device=dev).manual_seed(1000 * B + S)
                shape = (B, S, 1, args.size, args.size)
                centre = torch.randn((B, 1, 1, args.size, args.size), generator=g, device=dev)
                p1 = centre + 0.3 * torch.randn(shape, generator=g, device=dev)
                p2 = torch.rand(shape, generator=g, device=dev) * 3.5 - 3.0
                y = centre[:, 0] + 0.5 * torch.randn((B, 1, args.size, args.size), generator=g, device=dev)
                sc = PredictiveScorer()
                upd = timed(lambda: sc.update(p1, p2, y, None, loss), args.warmup, args.reps)
                cmp_ = timed(sc.compute, args.warmup, args.reps)
                sc.reset()
                sc.update(p1, p2, y, None, loss)
                res = sc.compute()
                pair_bytes = 4 * S * S * args.size * args.size
                chunk = max(1, min(B, (args.chunk_mb << 20) // pair_bytes))
                tor = timed(lambda: torch_route(p1, p2, y, loss, chunk), max(1, args.warmup // 2), max(3, args.reps // 4))
                means = (torch_route(p1, p2, y, loss, chunk) / res["n"]).cpu().numpy()
                ours = np.array([res["nll"], res["crps"], res["pit_mean"]])
                diff = float(np.max(np.abs(means - ours) / np.abs(ours)))
                pixels = B * args.size * args.size
                gbps = (8 * S + 4) * pixels / (upd[1] * 1e-3) / 1e9
                lines.append(f"{loss:12s} {B:3d} {S:3d} {upd[0]:8.3f} ({upd[1]:6.3f}) {cmp_[0]:8.3f} ({cmp_[1]:6.3f}) "
                             f"{tor[0]:9.3f} ({tor[1]:7.3f}) {tor[0] / upd[0]:7.1f} {gbps:7.0f} {diff:26.2e}")
                print(lines[-1], flush=True)
                if S == 3 and loss == "laplace_nll":
                    ev = UncertaintyEvaluator()
                    maps = (p1[:, 0], torch.exp(p2[:, 0]) ** 2, torch.exp(p2[:, 1]) ** 2 * 0.1, y)

                    def feed():
                        ev.reset()
                        ev.update(*maps)
                    et = timed(feed, args.warmup, args.reps)
                    eval_lines.append(f"B={B:2d} S=3: score update {(8 * S + 4)} B/pixel at min time {gbps:6.0f} GB/s; "
                                      f"mimo_eval_accumulate (UncertaintyEvaluator.update, 24 B/pixel, with a workspace reset) "
                                      f"{et[0]:.3f} ({et[1]:.3f}) ms = {24 * pixels / (et[1] * 1e-3) / 1e9:6.0f} GB/s")
                del p1, p2, y, centre
                torch.cuda.empty_cache()
    lines += ["", "achieved bytes per second, S_total = 3 (whole call between events: the pass and its fold launch):"] + eval_lines
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(eval_lines))


if __name__ == "__main__":
    main()
