"""FGSM robustness sweep of an ensemble on the GPU (the first half of the reference's scripts/test/test_nyuv2_depth.py:
make_predictions per noise level + the two tables), with the time of the sweep per batch and, with --compare, the time of
the route the code base offered before `mimo.adversarial`: per eps, autograd through `MimoUnetModel` with the torch-side
loss, `x.grad`, the torch expression of the attack, then the ensemble forward.

    python scripts/evaluate_robustness.py --synthetic 4 --result_dir out                      # seeded model and batches
    python scripts/evaluate_robustness.py --synthetic 4 --compare --result_dir out            # + the older route, alternating
    python scripts/evaluate_robustness.py --model_checkpoint_paths a.ckpt b.ckpt --batch_dir batches/ --result_dir out
    python scripts/evaluate_robustness.py --evidential --synthetic 4 --compare --result_dir out   # a bare EvidentialUnetModel
    python scripts/evaluate_robustness.py --evidential --model_checkpoint_paths ev.ckpt --batch_dir batches/ --result_dir out
    python scripts/evaluate_robustness.py --synthetic 8 --monte_carlo_steps 8 --compare --result_dir out   # MC-dropout ensemble
    python scripts/evaluate_robustness.py --synthetic 4 --attack pgd --pgd_steps 10 --result_dir out       # PGD instead of FGSM

--attack pgd: the iterated, projected attack (`pgd_sweep`) with --pgd_steps steps of --pgd_step_size (default 2.5 * eps / steps)
and, with --pgd_random_start, a random start from the engine's generator; the tables and their file names are the same.  The
older route is the FGSM one, so --compare is not offered with it (scripts/measure_pgd.py times PGD against its torch form).

--monte_carlo_steps N (the reference's flag): an MC-dropout ensemble of N passes per member, attacked through
`fgsm_sweep(..., mc_dropout=True)` — one gradient over the N masked passes, then the MC forward per eps.  The synthetic member
is then BASELINE's cfg5 (S = 1, Dropout2d p = 0.1 at encoder, core and decoder sites; --channels 3 --batch 2 are its geometry,
the defaults stay those of cfg3).  The older route's MC leg: per eps, per member and per pass one autograd backward through
`MimoUnetModel` with the dropout modules on, `x.grad` summed in torch.  The two routes draw different masks, so their
predictions are not compared.  The line `fold_image_grad_mc: ...` gives the bytes one launch of the new kernel moves at this
geometry (its time comes from a kernel trace of a run without --compare).

--evidential: the reference's scripts/test/test_nyuv2_depth_evidential.py — ONE `EvidentialUnetModel` (one checkpoint, or a
seeded fbc = --fbc network) instead of an ensemble; the older route is then autograd through the model, `.mean()` of its loss.

--batch_dir: `*.npy` files holding one dict each ({"image": [B,C,H,W], "label": [B,1,H,W], optional "mask"}), saved with
np.save(..., allow_pickle=True).  --synthetic N: N seeded batches of --batch x --channels x --size x --size (defaults: the
benchmark geometry cfg3, 32 x 2 x 256 x 256) through a seeded S = 2, fbc = --fbc network."""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimo.adversarial import RobustnessEvaluator, fgsm_sweep, pgd_sweep  # noqa: E402


def older_route(ensemble, image, label, epsilons, mask=None):
    """Per eps (the reference's loop, test_nyuv2_depth.py:38-61): gradient of the NLL w.r.t. the image through every member under
    autograd (the whole training backward runs for it), sign / mul / add / clamp as torch launches, the ensemble forward."""
    out = {}
    s_total = ensemble.num_subnetworks
    for eps in epsilons:
        grad = torch.zeros_like(image)
        for model in ensemble.models:
            S = model.num_subnetworks
            x5 = image[:, None].repeat(1, S, 1, 1, 1).requires_grad_(True)
            p1, p2 = model(x5)
            labels = label[:, None].repeat(1, S, 1, 1, 1)
            raw = model.loss_fn.forward(p1, p2, labels, reduce_mean=False, mask=None if mask is None else mask[:, None])
            (raw.mean() * (S / s_total)).backward()
            grad += x5.grad.sum(dim=1)
        perturbed = torch.clamp(image + eps * grad.sign(), 0, 1)
        out[eps] = ensemble(perturbed)
    return out


def older_route_mc(ensemble, image, label, epsilons, mask=None):
    """The MC-dropout form of `older_route`: per eps, per member and per pass one autograd backward through the member with its
    dropout modules on (BatchNorm in eval mode), the passes' `x.grad` summed in torch with the weight 1 / (M * S_total)."""
    out = {}
    s_total, passes = ensemble.num_subnetworks, ensemble.monte_carlo_steps
    for eps in epsilons:
        grad = torch.zeros_like(image)
        for model in ensemble.models:
            S = model.num_subnetworks
            labels = label[:, None].repeat(1, S, 1, 1, 1)
            for _ in range(passes):
                x5 = image[:, None].repeat(1, S, 1, 1, 1).requires_grad_(True)
                p1, p2 = model(x5)
                raw = model.loss_fn.forward(p1, p2, labels, reduce_mean=False, mask=None if mask is None else mask[:, None])
                (raw.mean() * (S / (passes * s_total))).backward()
                grad += x5.grad.sum(dim=1)
            model.zero_grad()
        perturbed = torch.clamp(image + eps * grad.sign(), 0, 1)
        out[eps] = ensemble(perturbed)
    return out


def older_route_evidential(model, image, label, epsilons, mask=None):
    """Per eps (the reference's loop, test_nyuv2_depth_evidential.py:39-65): autograd through the model to the image (the whole
    training backward runs for it), the torch expression of the attack, the model again, the head kernel's parameters through
    `loss_fn.mode / aleatoric_var / epistemic_var` as three torch launches."""
    out = {}
    m3 = None if mask is None else mask.reshape(mask.shape[0], *mask.shape[-2:])
    for eps in epsilons:
        x = image.clone().requires_grad_(True)
        _, loss = model._forward_with_loss(x, label, m3)
        model.zero_grad()
        loss.mean().backward()
        perturbed = torch.clamp(image + eps * x.grad.sign(), 0, 1)
        with torch.no_grad():
            ev = model(perturbed)
            out[eps] = tuple(f(ev).unsqueeze(1) for f in (model.loss_fn.mode, model.loss_fn.aleatoric_var, model.loss_fn.epistemic_var))
    model.zero_grad()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_checkpoint_paths", nargs="*", default=[])
    ap.add_argument("--batch_dir")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--fbc", type=int, default=30)
    ap.add_argument("--members", type=int, default=1, help="seeded members of the synthetic ensemble")
    ap.add_argument("--epsilons", type=float, nargs="+", default=[0.0, 0.02, 0.04])
    ap.add_argument("--name", default="synthetic")
    ap.add_argument("--evidential", action="store_true", help="one EvidentialUnetModel instead of an ensemble")
    ap.add_argument("--monte_carlo_steps", type=int, default=0, metavar="N",
                    help="MC-dropout ensemble of N passes per member (fgsm_sweep(mc_dropout=True))")
    ap.add_argument("--compare", action="store_true", help="also time the autograd route, in alternating pairs")
    ap.add_argument("--attack", choices=("fgsm", "pgd"), default="fgsm")
    ap.add_argument("--pgd_steps", type=int, default=10)
    ap.add_argument("--pgd_step_size", type=float, default=None, help="default: 2.5 * eps / pgd_steps per level")
    ap.add_argument("--pgd_random_start", action="store_true")
    ap.add_argument("--result_dir", required=True)
    args = ap.parse_args()
    mc = args.monte_carlo_steps
    if mc < 0 or (mc > 0 and args.evidential):
        ap.error("--monte_carlo_steps: a positive number of passes, and not with --evidential (the reference's evidential "
                 "scripts have no MC mode)")
    if args.attack == "pgd" and args.compare:
        ap.error("--compare times the FGSM autograd route: not with --attack pgd")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from mimo.models.ensemble import EnsembleModule
    models = None
    if args.evidential:
        from mimo.models.evidential_unet import EvidentialUnetModel
        if len(args.model_checkpoint_paths) > 1:
            ap.error("--evidential takes one checkpoint")
        if args.model_checkpoint_paths:
            ensemble = EvidentialUnetModel.load_from_checkpoint(args.model_checkpoint_paths[0])
        else:
            if args.synthetic < 1:
                ap.error("give a checkpoint or --synthetic N")
            torch.manual_seed(0)
            ensemble = EvidentialUnetModel(in_channels=args.channels, out_channels=4, filter_base_count=args.fbc,
                                           center_dropout_rate=0.0, final_dropout_rate=0.0, encoder_dropout_rate=0.0,
                                           core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0, learning_rate=1e-3,
                                           seed=0)
        ensemble = ensemble.to(dev).eval()
    elif not args.model_checkpoint_paths:
        if args.synthetic < 1:
            ap.error("give checkpoints or --synthetic N")
        from mimo.models.mimo_unet import MimoUnetModel
        models = []
        for i in range(args.members):
            torch.manual_seed(i)
            p = 0.1 if mc > 0 else 0.0
            models.append(MimoUnetModel(in_channels=args.channels, out_channels=2, num_subnetworks=1 if mc > 0 else 2,
                                        filter_base_count=args.fbc,
                                        center_dropout_rate=0.0, final_dropout_rate=0.0, encoder_dropout_rate=p,
                                        core_dropout_rate=p, decoder_dropout_rate=p, loss="laplace_nll", weight_decay=0.0,
                                        learning_rate=1e-3, seed=i, loss_buffer_size=10, loss_buffer_temperature=0.3).cuda())
    if not args.evidential:
        ensemble = EnsembleModule(args.model_checkpoint_paths, monte_carlo_steps=mc, models=models, keep_on_device=True).to(dev)
    older = older_route_evidential if args.evidential else (older_route_mc if mc > 0 else older_route)
    if args.batch_dir:
        batches = [np.load(f, allow_pickle=True).item() for f in sorted(glob.glob(os.path.join(args.batch_dir, "*.npy")))]
    else:
        g = torch.Generator().manual_seed(1)
        batches = [{"image": torch.rand(args.batch, args.channels, args.size, args.size, generator=g),
                    "label": torch.rand(args.batch, 1, args.size, args.size, generator=g)} for _ in range(args.synthetic)]
    eps = tuple(args.epsilons)
    rob = RobustnessEvaluator(eps, mc_dropout=mc > 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        return res, e0.elapsed_time(e1)

    first = {k: torch.as_tensor(batches[0][k]).to(dev) for k in ("image", "label")}
    sweep = fgsm_sweep if mc == 0 else (lambda *a, **k: fgsm_sweep(*a, mc_dropout=True, **k))
    if args.attack == "pgd":
        def sweep(*a, **k):
            return pgd_sweep(*a, steps=args.pgd_steps, step_size=args.pgd_step_size, random_start=args.pgd_random_start,
                             mc_dropout=mc > 0, **k)
    sweep(ensemble, first["image"], first["label"], eps)  # first calls: plans, code load
    if args.compare:
        older(ensemble, first["image"], first["label"], eps)
    new_ms, old_ms, agree = [], [], []
    for i, b in enumerate(batches):
        image, label = (torch.as_tensor(b[k]).to(dev) for k in ("image", "label"))
        mask = torch.as_tensor(b["mask"]).to(dev) if b.get("mask") is not None else None
        order = ("new", "old") if i % 2 == 0 else ("old", "new")  # alternating pairs: drift hits both routes alike
        res = {}
        for which in order if args.compare else ("new",):
            if which == "new":
                res["new"], ms = timed(lambda: sweep(ensemble, image, label, eps, mask=mask))
                new_ms.append(ms)
            else:
                res["old"], ms = timed(lambda: older(ensemble, image, label, eps, mask=mask))
                old_ms.append(ms)
        if args.compare and mc == 0:  # the two routes' predictions differ only where a gradient's sign is within rounding of zero
            e = eps[-1]
            a, c = res["new"][e][0], res["old"][e][0]
            agree.append(float((a - c).abs().max() / c.abs().max()))
        line = f"batch {i}: sweep {new_ms[-1]:.3f} ms"
        if args.compare:
            line += f", autograd route {old_ms[-1]:.3f} ms"
        if agree:
            line += f", max |mean difference| / max |mean| at eps {eps[-1]}: {agree[-1]:.2e}"
        print(line, flush=True)
        for e, (mean, av, ev) in res["new"].items():
            rob.evaluators[e].update(mean, av, ev, label, mask)
    tables = rob.compute()
    rob.write_csv(args.result_dir, args.name, tables)
    out = {"model": "evidential" if args.evidential else "ensemble", "epsilons": list(eps), "batches": len(batches), "pixels_per_batch": int(batches[0]["image"].shape[0]) * args.size * args.size
           if not args.batch_dir else None, "sweep_ms_median": float(np.median(new_ms)), "sweep_ms_min": float(np.min(new_ms)),
           "mae_per_eps": {str(e): tables[e]["mae"] for e in eps}}
    if args.attack == "pgd":
        out.update(attack="pgd", pgd_steps=args.pgd_steps, pgd_step_size=args.pgd_step_size, pgd_random_start=args.pgd_random_start)
    if mc > 0:
        # what one launch of fold_image_grad_mc_kernel moves: R * 4 * Ci_p read, 4 * Ci written (+ 4 * Ci read when accumulating)
        # per pixel of the B images, at the chunk the gradient runs in
        from mimo_unet_amd.adversarial import _mc_chunk_weights
        b, ci = int(batches[0]["image"].shape[0]), int(batches[0]["image"].shape[1])
        m0, m1, _ = _mc_chunk_weights(mc, b, ensemble.max_samples_per_launch, ensemble.num_subnetworks)[0]
        pix = b * int(batches[0]["image"].shape[-2]) * int(batches[0]["image"].shape[-1])
        cip = (ci + 3) // 4 * 4
        out.update(monte_carlo_steps=mc, passes_per_launch=m1 - m0,
                   fold_image_grad_mc_bytes={"assign": pix * ((m1 - m0) * 4 * cip + 4 * ci),
                                             "accumulate": pix * ((m1 - m0) * 4 * cip + 8 * ci)})
        print(f"fold_image_grad_mc: B {b}, R {m1 - m0}, Ci {ci} (padded {cip}): {out['fold_image_grad_mc_bytes']} bytes per launch")
    if old_ms:
        out.update(autograd_route_ms_median=float(np.median(old_ms)), autograd_route_ms_min=float(np.min(old_ms)),
                   speedup_median=float(np.median(old_ms) / np.median(new_ms)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
