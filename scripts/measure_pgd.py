"""Times `mimo.adversarial.pgd_sweep` against the same attack written in torch on the public API the code base had before it,
and `mimo_pgd_step` alone against its byte count.  Needs an MI355X; prints one JSON line per batch size and, with --out, writes
them to a file.

    python scripts/measure_pgd.py --batches 5 32 --out profiles/pgd/measure_pgd.json

The torch route (`torch_route` below), per step and PER eps: `image_gradient` at that level's iterate, then `sign`, `mul`/`add`,
`min`, `max` and `clamp` as torch launches; at the end the ensemble forward per eps, as in `pgd_sweep`.  `pgd_sweep` stacks the
levels on the batch axis for the gradient (max(1, 64 // B) levels per call) and moves all of them with one `mimo_pgd_step` launch.

Method: both routes are warmed up on the timed shapes (plans, code objects), then timed in alternating pairs (drift hits both
alike) with device events around each whole sweep; median, minimum and maximum over --repeats pairs are reported.  The two
routes are compared on their perturbed images as well (share of pixels whose bits differ).  They are close, not equal: the
gradient of a stacked batch of another size runs other launch recipes (other summation orders) and carries the factor 1 / Kc,
so a pixel whose gradient is within rounding of zero can take the other sign, and later steps build on it.
`pgd_step` alone: --step_launches back-to-back launches between two events after a warm-up, so the figure includes the launch
gaps of a dependent chain; bytes = elems * (4 + 8 K + 4 K).  At batch 5 the whole working set (39 MB at K = 3) stays in the
256 MiB Infinity Cache, so that rate is a cache rate, not an HBM rate; at batch 32 it is 252 MB per launch.

The network is BASELINE's cfg3 geometry (S = 2, fbc = 30, 256 x 256) with seeded weights and --channels input channels."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimo.adversarial import image_gradient, pgd_sweep  # noqa: E402


def torch_route(ensemble, image, label, epsilons, steps, rel_step_size=2.5, return_perturbed=False):
    out = {}
    for eps in epsilons:
        alpha = rel_step_size * eps / steps
        x = image.clamp(0, 1)
        if eps > 0:
            upper, lower = image + eps, image - eps
            for _ in range(steps):
                grad = image_gradient(ensemble, x, label)
                x = x + alpha * grad.sign()
                x = torch.max(torch.min(x, upper), lower)
                x = x.clamp(0, 1)
        res = tuple(ensemble(x))
        out[eps] = res + (x,) if return_perturbed else res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--fbc", type=int, default=30)
    ap.add_argument("--epsilons", type=float, nargs="+", default=[0.01, 0.02, 0.04])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step_launches", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_pgd.py: no GPU is visible; nothing is measured on a CPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from mimo.models.ensemble import EnsembleModule
    from mimo.models.mimo_unet import MimoUnetModel
    from mimo_unet_amd.engine import pgd_step
    torch.manual_seed(0)
    member = MimoUnetModel(in_channels=args.channels, out_channels=2, num_subnetworks=2, filter_base_count=args.fbc,
                           center_dropout_rate=0.0, final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
                           decoder_dropout_rate=0.0, loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3, seed=0,
                           loss_buffer_size=10, loss_buffer_temperature=0.3).cuda()
    ensemble = EnsembleModule([], models=[member], keep_on_device=True).to(dev)
    eps = tuple(args.epsilons)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        return res, e0.elapsed_time(e1)

    def spread(ms):
        return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "repeats": len(ms)}

    lines = []
    for batch in args.batches:
        g = torch.Generator().manual_seed(batch)
        image = torch.rand(batch, args.channels, args.size, args.size, generator=g).to(dev)
        label = torch.rand(batch, 1, args.size, args.size, generator=g).to(dev)
        routes = {"pgd_sweep": lambda: pgd_sweep(ensemble, image, label, eps, steps=args.steps, return_perturbed=True),
                  "torch_route": lambda: torch_route(ensemble, image, label, eps, args.steps, return_perturbed=True)}
        for _ in range(2):
            for fn in routes.values():
                fn()
        ms = {k: [] for k in routes}
        res = {}
        for i in range(args.repeats):
            for k in (("pgd_sweep", "torch_route") if i % 2 == 0 else ("torch_route", "pgd_sweep")):
                res[k], t = timed(routes[k])
                ms[k].append(t)
        differ = {str(e): float((res["pgd_sweep"][e][3] != res["torch_route"][e][3]).float().mean()) for e in eps}
        mean_diff = {str(e): float((res["pgd_sweep"][e][0] - res["torch_route"][e][0]).abs().max() / res["torch_route"][e][0].abs().max())
                     for e in eps}
        # ---- the step kernel alone
        k = len(eps)
        alpha = [2.5 * e / args.steps for e in eps]
        x_adv = image[None].repeat(k, 1, 1, 1, 1)
        grad = torch.randn(x_adv.shape, device=dev)
        for _ in range(20):
            pgd_step(image, grad, x_adv, eps, alpha)
        _, chain = timed(lambda: [pgd_step(image, grad, x_adv, eps, alpha) for _ in range(args.step_launches)])
        step_us = 1e3 * chain / args.step_launches
        nbytes = image.numel() * (4 + 8 * k + 4 * k)
        levels = max(1, ensemble.max_samples_per_launch // batch)
        line = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "batch": batch, "channels": args.channels,
                "size": args.size, "fbc": args.fbc, "epsilons": list(eps), "steps": args.steps, "levels_per_gradient_call": levels,
                "pgd_sweep": spread(ms["pgd_sweep"]), "torch_route": spread(ms["torch_route"]),
                "speedup_median": float(np.median(ms["torch_route"]) / np.median(ms["pgd_sweep"])),
                "perturbed_pixels_that_differ": differ, "max_mean_difference_over_max_mean": mean_diff,
                "pgd_step": {"K": k, "elems": image.numel(), "bytes": nbytes, "launches": args.step_launches,
                             "us_per_launch_in_a_chain": step_us, "TB_per_s": nbytes / (step_us * 1e-6) / 1e12}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
