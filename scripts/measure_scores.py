"""Timings of `PredictiveScorer` on the GPU, next to a torch restatement of the same formulas on the same device:

    python scripts/measure_scores.py            # writes profiles/scores/summary.txt
    python scripts/measure_scores.py --evidential   # adds the evidential model's section to it

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


EVIDENTIAL_MARK = "PredictiveScorer.update_evidential"


def evidential_leg(args, dev):
    """`update_evidential` at --evidential_batch x size^2 next to `update` at S = 1 (the same 1-member traffic: the
    bandwidth yardstick) and next to the route a user had before: the logits copied to the host and the three quantities
    from scipy.stats.t.  Replaces the section of --out that starts at EVIDENTIAL_MARK (or appends one)."""
    import time
    B, size = args.evidential_batch, args.size
    g = torch.Generator(device=dev).manual_seed(77)
    logits = torch.randn((B, 4, size, size), generator=g, device=dev) * 1.5
    logits[:, 2] = torch.rand((B, size, size), generator=g, device=dev) * 12.0 - 3.0  # alpha from 1.05 to 10
    label = logits[:, :1] + torch.randn((B, 1, size, size), generator=g, device=dev) * 1.5
    pixels = B * size * size
    sc = PredictiveScorer()
    upd = timed(lambda: sc.update_evidential(logits, label), args.warmup, args.reps)
    sc.reset()
    sc.update_evidential(logits, label)
    res = sc.compute()
    worst_iterations = int(sc._ws[71])
    mix = PredictiveScorer()
    p1, p2 = logits[:, None, :1].contiguous(), logits[:, None, 1:2].contiguous()
    one = timed(lambda: mix.update(p1, p2, label, None, "laplace_nll"), args.warmup, args.reps)
    lines = [f"{EVIDENTIAL_MARK} on {torch.cuda.get_device_name(0)}: the Student-t predictive of the evidential model, {B} x {size} x "
             f"{size} pixels, no mask, no maps; HIP-event times in ms, median (min) of {args.reps} calls after {args.warmup} warm-up calls",
             f"update_evidential (20 B/pixel)         {upd[0]:8.3f} ({upd[1]:6.3f})  = {20 * pixels / (upd[1] * 1e-3) / 1e9:6.0f} GB/s at the min",
             f"update, Laplace, S = 1 (12 B/pixel)    {one[0]:8.3f} ({one[1]:6.3f})  = {12 * pixels / (one[1] * 1e-3) / 1e9:6.0f} GB/s at the min",
             f"update_evidential / update at S = 1: {upd[0] / one[0]:.1f} x (double-precision arithmetic, not traffic: at the "
             f"S = 1 kernel's bytes per second its 20 B/pixel would take {20 * pixels / (12 * pixels / one[1]):.3f} ms)",
             f"most continued-fraction iterations of any pixel: {worst_iterations} (cap 160); n = {res['n']}, mean nll {res['nll']:.6f}, "
             f"mean crps {res['crps']:.6f}, mean pit {res['pit_mean']:.6f}"]
    try:
        from scipy import stats
    except ImportError:
        lines.append("host route (scipy.stats.t): scipy is not importable here: not measured")
    else:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        l, y = logits.cpu().numpy().astype(np.float64), label.cpu().numpy()[:, 0].astype(np.float64)
        sp = lambda x: np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))
        mu, v, alpha, beta = l[:, 0], sp(l[:, 1]), sp(l[:, 2]) + 1, sp(l[:, 3])
        nu, sigma = 2 * alpha, np.sqrt(beta * (1 + v) / (v * alpha))
        z = (y - mu) / sigma
        F, f = stats.t.cdf(z, nu), stats.t.pdf(z, nu)
        from scipy.special import gammaln
        lb1 = np.log(np.pi) / 2 + gammaln(alpha) - gammaln(alpha + 0.5)
        lb2 = np.log(np.pi) / 2 + gammaln(nu - 0.5) - gammaln(nu)
        nll = -(stats.t.logpdf(z, nu) - np.log(sigma))
        crps = sigma * (z * (2 * F - 1) + 2 * f * (nu + z * z) / (nu - 1) - 2 * np.sqrt(nu) / (nu - 1) * np.exp(lb2 - 2 * lb1))
        host_s = time.perf_counter() - t0
        diff = max(abs(nll.mean() - res["nll"]) / abs(res["nll"]), abs(crps.mean() - res["crps"]) / abs(res["crps"]),
                   abs(F.mean() - res["pit_mean"]) / abs(res["pit_mean"]))
        lines.append(f"host route (logits to the host, scipy.stats.t cdf / pdf / logpdf in float64, one call each): {host_s * 1e3:.0f} ms "
                     f"= {host_s * 1e3 / upd[0]:.0f} x update_evidential; max rel diff of the three means {diff:.2e}")
    print("\n".join(lines), flush=True)
    old = open(args.out).read().splitlines() if os.path.exists(args.out) else []
    keep = next((i for i, line in enumerate(old) if line.startswith(EVIDENTIAL_MARK)), len(old))
    old = old[:keep]
    while old and not old[-1].strip():
        old.pop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(old + ([""] if old else []) + lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evidential", action="store_true", help="only the evidential leg: appended to --out")
    ap.add_argument("--evidential_batch", type=int, default=32)
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
    if args.evidential:
        evidential_leg(args, dev)
        return
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
