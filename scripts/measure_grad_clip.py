"""HIP-event times of the clipped flat Adam step on one GPU (the table of DESIGN.md section 3).

At n = 15 060 000 (cfg3's parameter count) and 60 100 000 (cfg4's), every variant warmed up, repeated --repeats times in
alternation, back-to-back calls on preallocated buffers:
  amp_step      (a) mimo_adam_step_amp
  clipped_norm  (b) mimo_adam_step_clipped, norm mode (clip = a tenth of the norm: the coefficient is applied)
  unfused       (c) torch.nn.utils.clip_grad_norm_ over cfg3's real parameter views of the flat gradient, then (a); at cfg3's
                    size only
  sum_read      (d) torch.sum over the gradient: what one more read of it costs
The check is (b) - (a) against (d), from the same run: the clipped step should cost about one more read of the gradient plus
one small launch; more than 2 x (d) means the reduction does not stream.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SIZES = {"cfg3": 15_060_000, "cfg4": 60_100_000}


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # microseconds


def cfg3_shapes():
    from mimo.models.mimo_components.model import MimoUNet
    net = MimoUNet(in_channels=2, out_channels=2, num_subnetworks=2, filter_base_count=30)
    return [tuple(q.shape) for q in net.parameters()]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_grad_clip.py needs a GPU: a timing taken anywhere else says nothing")
    from mimo_unet_amd import _lib as L

    lib, st, dev = L.load(), L.current_stream(), "cuda"
    scratch = torch.empty((int(lib.mimo_grad_clip_scratch_bytes()) + 7) // 8, device=dev, dtype=torch.float64)
    shapes = cfg3_shapes()
    total = sum(int(torch.Size(s).numel()) for s in shapes)
    res = {"cfg3_parameter_views": len(shapes), "cfg3_parameters": total, "iters": args.iters, "sizes": {}}
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    for name, n in SIZES.items():
        gen = torch.Generator(device=dev).manual_seed(1)
        p, g = torch.randn(n, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen)
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        step_dev, clip_out = torch.zeros(1, device=dev), torch.zeros(2, device=dev)
        clip = float(torch.linalg.vector_norm(g.double())) / 10.0
        ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n)

        def amp_step():
            L.check(lib.mimo_adam_step_amp(*ptrs, *hyper, step_dev.data_ptr(), 1.0, None, None, st), "mimo_adam_step_amp")

        def clipped_norm():
            L.check(lib.mimo_adam_step_clipped(*ptrs, *hyper, step_dev.data_ptr(), 1.0, None, None, 1, clip, clip_out.data_ptr(),
                                               scratch.data_ptr(), st), "mimo_adam_step_clipped")

        variants = {"amp_step": amp_step, "clipped_norm": clipped_norm, "sum_read": lambda: torch.sum(g)}
        if name == "cfg3":
            gbuf = torch.randn(max(n, total), device=dev, generator=gen)
            views, off = [], 0
            for s in shapes:
                k = int(torch.Size(s).numel())
                q = torch.empty(s, device=dev)
                q.grad = gbuf[off: off + k].view(s)
                views.append(q)
                off += k

            def unfused():
                torch.nn.utils.clip_grad_norm_(views, clip)
                amp_step()
            variants["unfused"] = unfused
        us = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                us[k].append(round(timed(fn, args.iters), 2))
        best = {k: min(x) for k, x in us.items()}
        res["sizes"][name] = {"n": n, "us": us, "clipped_minus_amp_us": round(best["clipped_norm"] - best["amp_step"], 2),
                              "sum_read_us": best["sum_read"],
                              "extra_over_read": round((best["clipped_norm"] - best["amp_step"]) / best["sum_read"], 3),
                              "last_norm": float(clip_out[0]), "last_coef": float(clip_out[1])}
        del p, g, m, v
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
