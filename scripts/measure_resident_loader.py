"""What feeding a training loop costs on one GPU, at cfg2's geometry (bench.py: 3 -> 1 channels, S = 2, fbc = 21, batch 64) with
synthetic uint8 data at NYUv2's 128 x 160 and at 256 x 256.

Two routes, the same MimoUnetModel training loop (zero_grad, training_step, backward, step) over each:
  (a) dataloader  DataLoader(NYUv2DepthDataset.from_arrays(...), num_workers=12, pin_memory=True, shuffle, drop_last)
                  under mimo_unet_amd.data.DevicePrefetcher — per-sample __getitem__ on the host, collate, one upload per
                  tensor and step
  (b) resident    mimo_unet_amd.data.ResidentLoader over a ResidentDataset of the same arrays — one mimo_dataset_gather
                  launch per step on the training stream
Per route and size: images/s of --repeats timed loops of --steps steps (a host clock around a loop that ends in a
synchronise; an untimed loop of --warmup steps first).  For the gather alone: HIP events around 200 back-to-back gather
calls (the span holds the host's per-call work, so it is an upper bound on the launch's device time) and the GB/s that
time means for the launch's 5 c bytes per pixel and field.

Every leg (one route at one size) runs in a process of its own under its own time limit; after a leg that does not end
cleanly no further leg is started.  Writes profiles/resident_data/summary.txt (--out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"128x160": (128, 160), "256x256": (256, 256)}
BATCH, CHANNELS, WORKERS = 64, 3, 12


def leg(args):
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("measure_resident_loader.py needs a GPU: a timing taken anywhere else says nothing")
    import bench
    from mimo_unet_amd.data import DevicePrefetcher, ResidentDataset, ResidentLoader
    from mimo_unet_amd.datasets.nyuv2 import NYUv2DepthDataset

    h, w = SIZES[args.size]
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    n = BATCH * args.steps
    image = rng.randint(0, 256, size=(n, h, w, CHANNELS), dtype=np.uint8)
    # a label the image predicts (its channel mean), so that the loss stays finite over the run
    depth = image.mean(axis=3, keepdims=True).astype(np.uint8)
    ds = NYUv2DepthDataset.from_arrays(image, depth)
    if args.leg == "dataloader":
        host = torch.utils.data.DataLoader(ds, batch_size=BATCH, num_workers=WORKERS, pin_memory=True, shuffle=True,
                                           drop_last=True, persistent_workers=True)
        loader = DevicePrefetcher(host, "cuda", depth=2)
    else:
        store = ResidentDataset(*ds.resident_fields())
        loader = ResidentLoader(store, BATCH, shuffle=True, drop_last=True)

    model = bench.make_model(dict(bench.CONFIGS["cfg2"], H=h, W=w)).cuda().train()
    opt = model.configure_optimizers()["optimizer"]

    def epoch(limit):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        for i, batch in enumerate(loader):
            if i >= limit:
                break
            opt.zero_grad()
            model.training_step(batch, i)["loss"].backward()
            opt.step()
            steps += 1
        torch.cuda.synchronize()
        return steps * BATCH / (time.perf_counter() - t0)

    epoch(args.warmup)
    res = {"leg": args.leg, "size": args.size, "batch": BATCH, "steps": args.steps,
           "precision": os.environ.get("MIMO_PRECISION", "split16"),
           "images_per_s": [round(epoch(args.steps), 1) for _ in range(args.repeats)]}
    if args.leg == "resident":
        index = torch.arange(BATCH, device="cuda") * 3 % n
        for _ in range(10):
            store.gather(index)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        calls = 200
        a.record()
        for _ in range(calls):
            store.gather(index)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) / calls * 1e3
        nbytes = 5 * (CHANNELS + 1) * BATCH * h * w  # c read + 4 c written per pixel, image and label
        res.update(gather_call_us_upper_bound=round(us, 1), gather_bytes=nbytes, gather_gb_per_s=round(nbytes / us / 1e3, 1),
                   store_mib=round(store.nbytes / 2**20, 1))
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds one leg may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_data", "summary.txt"))
    ap.add_argument("--leg", choices=("dataloader", "resident"), help="run one leg in this process (used by the driver)")
    ap.add_argument("--size", choices=tuple(SIZES))
    args = ap.parse_args()
    if args.leg:
        return leg(args)

    results, failed = [], None
    for size in SIZES:
        for name in ("dataloader", "resident"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--size", size, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
            except subprocess.TimeoutExpired:
                failed = f"{name} {size}: no result within {args.leg_timeout} s"
                break
            lines = [ln[4:] for ln in out.stdout.splitlines() if ln.startswith("LEG ")]
            if out.returncode != 0 or not lines:
                failed = f"{name} {size}: exit status {out.returncode}\n{out.stderr[-2000:]}"
                break
            results.append(json.loads(lines[-1]))
            print(lines[-1], flush=True)
        if failed:
            break

    text = [f"Feeding a cfg2-geometry training loop (3 -> 1 ch, S = 2, fbc = 21, batch {BATCH}), one MI355X, synthetic uint8 data,",
            f"{args.repeats} timed loops of {args.steps} steps per leg after {args.warmup} warm-up steps; images/s per loop.",
            f"(a) dataloader: DataLoader(num_workers={WORKERS}, pin_memory=True) under DevicePrefetcher   (b) resident: ResidentLoader", ""]
    by = {(r["size"], r["leg"]): r for r in results}
    for size in SIZES:
        a, b = by.get((size, "dataloader")), by.get((size, "resident"))
        if not a or not b:
            continue
        spread = max(a["images_per_s"]) - min(a["images_per_s"])
        floor = min(a["images_per_s"]) - spread
        verdict = "holds" if min(b["images_per_s"]) >= floor else "FAILS"
        text += [f"{size}, precision {a['precision']}:",
                 f"  (a) dataloader  {a['images_per_s']}  spread {spread:.1f}",
                 f"  (b) resident    {b['images_per_s']}",
                 f"  acceptance (b) >= min(a) - spread(a) = {floor:.1f}: {verdict}",
                 f"  gather call: <= {b['gather_call_us_upper_bound']} us for {b['gather_bytes']} bytes (5 c per pixel and field, c = 3 + 1)"
                 f" = {b['gather_gb_per_s']} GB/s; store {b['store_mib']} MiB", ""]
    if failed:
        text += ["NOT MEASURED (the run stopped here): " + failed, ""]
    text += [json.dumps(r) for r in results]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
