"""Time `UncertaintyEvaluator.update` and `.compute` for one set of sources, in one process: one timed loop each, at the
geometry of tests/test_evaluation_gpu.py::test_benchmark_geometry_eight_updates_of_32x256x256 (8 updates of 32 x 1 x 256²
= 16.8 M pixels).  Prints one JSON line.

    python scripts/measure_sparsification.py                                              # the default evaluator
    python scripts/measure_sparsification.py --sources combined aleatoric epistemic      # + oracle: four orderings
    python scripts/measure_sparsification.py --tree ../parent_checkout                   # another checkout's package

To compare two commits, run the legs alternately and several times each; the spread between the runs of one leg is the
yardstick for a difference between two.  Both loops end in a device synchronise; the update loop includes the reset of
the workspace (one small memset per 8 updates, the same in every leg)."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="root of the checkout whose package is measured")
    ap.add_argument("--sources", nargs="*", default=None, help="omit for the default evaluator (works on any commit)")
    ap.add_argument("--updates", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--update_loops", type=int, default=500, help="timed passes of --updates updates")
    ap.add_argument("--compute_loops", type=int, default=200)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    from mimo.evaluation import UncertaintyEvaluator
    from scripts.evaluate_uncertainty import seeded_maps

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ev = UncertaintyEvaluator() if args.sources is None else UncertaintyEvaluator(sources=args.sources)
    batches = [seeded_maps(i, args.batch, args.size, dev) for i in range(args.updates)]
    for _ in range(2):  # allocations of both stores, code load
        ev.reset()
        for maps in batches:
            ev.update(*maps)
        first = ev.compute()
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    for _ in range(args.update_loops):
        ev.reset()
        for maps in batches:
            ev.update(*maps)
    torch.cuda.synchronize()
    update_ms = (time.perf_counter() - t0) * 1e3 / (args.update_loops * args.updates)

    t0 = time.perf_counter()
    for _ in range(args.compute_loops):
        tables = ev.compute()  # ends in the one device-to-host copy, which synchronises
    torch.cuda.synchronize()
    compute_ms = (time.perf_counter() - t0) * 1e3 / args.compute_loops

    same = all((tables["precision_recall"][k] == first["precision_recall"][k]).all() for k in ("mae", "rmse"))
    pixels = args.batch * args.size * args.size
    stores = 2 if getattr(ev, "_source_records", None) is not None else 1
    print(json.dumps({
        "label": args.label, "sources": args.sources or ["combined"], "orderings": len(getattr(ev, "_orderings", ("combined",))),
        "n": tables["n"], "pixels_per_update": pixels, "update_ms": round(update_ms, 5), "compute_ms": round(compute_ms, 4),
        "bytes_per_pixel": 16 + 8 * stores, "update_GBps": round((16 + 8 * stores) * pixels / (update_ms * 1e-3) / 1e9, 1),
        "update_loops": args.update_loops, "compute_loops": args.compute_loops, "tables_repeat_bit_for_bit": bool(same),
        "mae": tables["mae"], "row50_mae": float(tables["precision_recall"]["mae"][50]),
        "ause_mae": {k: v["mae"] for k, v in tables.get("ause", {}).items()},
    }))


if __name__ == "__main__":
    main()
