"""HIP-event times of the evidential model's step tail on one GPU (the figures of DESIGN.md section 3).

Two groups, both at --batch x --size x --size pixels, every variant warmed up, repeated --repeats times in alternation:
  kernels_us  each C entry point alone, back-to-back calls on preallocated buffers: mimo_evidential_step (training /
              validation outputs, with / without a mask), mimo_evidential_loss_gradient_dev, and the kernels of the tensor
              path (mimo_evidential_forward, mimo_evidential_backward with a filled d_loss, mimo_evidential_loss_gradient);
  tails_us    the whole tail of EvidentialUnetModel.training_step (+ backward down to the logits) and validation_step after
              the backbone — the backbone is replaced by a fixed logits leaf — with MIMO_EVIDENTIAL_STEP_FUSED on and off;
              host work included.
Run from a checkout without the fused step (an earlier commit), only the entries that exist there are measured: that is how
the tensor path is timed on the commit before the feature.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_evidential_step.py needs a GPU: a timing taken anywhere else says nothing")
    import mimo_unet_amd.models.evidential_unet as EU
    from mimo.models.evidential_unet import EvidentialUnetModel
    from mimo_unet_amd import _lib as L

    B, H, W = args.batch, args.size, args.size
    hw, dev = H * W, "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    logits = torch.randn(B, 4, H, W, device=dev, generator=g)
    label = (logits[:, 0:1] + torch.randn(B, 1, H, W, device=dev, generator=g)).contiguous()
    mask = (torch.rand(B, H, W, device=dev, generator=g) > 0.2).float()
    lib, st = L.load(), L.current_stream()
    has_step = hasattr(EU, "_FUSED_STEP")
    res = {"shape": [B, H, W], "fused_step_present": has_step}

    alea, epi, err = (torch.empty(B, 1, H, W, device=dev) for _ in range(3))
    sc, scratch = torch.empty(8, device=dev), torch.empty(2048 * 8, device=dev, dtype=torch.float64)
    dl, up = torch.empty_like(logits), torch.ones(1, device=dev)
    ev, lm = torch.empty_like(logits), torch.empty(B, H, W, device=dev)
    dloss = torch.full((B, H, W), 1.0 / (B * hw), device=dev)
    lg, lb, mk = logits.data_ptr(), label.data_ptr(), mask.data_ptr()
    kernels = {
        "evidential_forward": lambda: lib.mimo_evidential_forward(lg, lb, mk, B, hw, ev.data_ptr(), lm.data_ptr(), st),
        "evidential_backward": lambda: lib.mimo_evidential_backward(lg, lb, mk, None, dloss.data_ptr(), B, hw, dl.data_ptr(), st),
        "loss_gradient": lambda: lib.mimo_evidential_loss_gradient(lg, lb, mk, B, hw, 1.0 / (B * hw), dl.data_ptr(), st),
    }
    if has_step:
        def step(want_epi, m):
            return lambda: lib.mimo_evidential_step(lg, lb, m, B, hw, alea.data_ptr(), epi.data_ptr() if want_epi else None,
                                                    err.data_ptr(), sc.data_ptr(), scratch.data_ptr(), 2048, st)
        kernels.update({"step_train_mask": step(False, mk), "step_val_mask": step(True, mk), "step_train_nomask": step(False, None),
                        "step_val_nomask": step(True, None),
                        "loss_gradient_dev": lambda: lib.mimo_evidential_loss_gradient_dev(lg, lb, mk, B, hw, 1.0 / (B * hw),
                                                                                           up.data_ptr(), dl.data_ptr(), st)})
    res["kernels_us"] = {k: [] for k in kernels}
    for _ in range(args.repeats):
        for k, fn in kernels.items():
            res["kernels_us"][k].append(round(timed(fn, 200), 2))

    m = EvidentialUnetModel(in_channels=3, out_channels=4, filter_base_count=4, center_dropout_rate=0.0, final_dropout_rate=0.0,
                            encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0, weight_decay=0.0,
                            learning_rate=1e-3, seed=0).cuda()
    leaf = logits.clone().requires_grad_(True)
    m._logits = lambda x: leaf  # the backbone's output, fixed
    batch = {"image": torch.zeros(B, 3, H, W, device=dev), "label": label, "mask": mask}

    def train_tail():
        leaf.grad = None
        m.training_step(batch, 0)["loss"].backward()

    def val_tail():
        m.validation_step(batch, 0)

    variants = [("fused", True), ("tensor_ops", False)] if has_step else [("tensor_ops", False)]
    res["tails_us"] = {f"{s}_{name}": [] for s in ("train", "val") for name, _ in variants}
    for stage, tail, mode in (("train", train_tail, m.train), ("val", val_tail, m.eval)):
        mode()
        for _ in range(args.repeats):
            for name, fused in variants:
                if has_step:
                    EU._FUSED_STEP = fused
                res["tails_us"][f"{stage}_{name}"].append(round(timed(tail, 30), 1))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
