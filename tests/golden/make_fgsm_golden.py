"""Generate tests/golden/fgsm.npz from the REAL reference.

    python tests/golden/make_fgsm_golden.py --reference /path/to/MIMO-Unet

Imports the reference's `MimoUNet` and losses and loads `fgsm_attack` from its scripts/test/test_nyuv2_depth.py (whose two
package imports need `lightning` and `h5py`: empty stand-in modules carrying the two imported names are registered first,
as make_eval_golden.py does).  Drives them as `make_predictions` does (test_nyuv2_depth.py:38-58): labels repeated over the
subnetwork axis, `loss_fn(y_pred, log_param, labels)`, backward to the image, fgsm_attack per noise level.  Only arrays are
stored: nothing of the reference's text enters the repository.

Two eval-mode cases, each after a few training steps (non-trivial BatchNorm running statistics):
  laplace  : S = 2, 2 -> 1 channels, f = 2, 3 x 34 x 34 (not a multiple of 16: 17 x 17 at 1/2 resolution, odd)
  gaussian : S = 3, 3 -> 1 channels, f = 1, 3 x 32 x 32
Images lie in [0, 1] with about 3 % of the pixels exactly 0 and 3 % exactly 1, so that the clamp acts.
Stored per case `<name>/`: meta, state/*, image, label, logits [N,S,2,H,W], dx_sub [N,S,Ci,H,W] (per-subnetwork input
gradient), dimage [N,Ci,H,W], perturbed [3,N,Ci,H,W] for eps = 0, 0.02, 0.04, and the seed that was used.

The sign of a gradient is discontinuous: a pixel is decided when |g| >= 1e-3 max|g| (tests/fgsm_reference.py).  The share of
undecided pixels of a case must be at most 2 % — asserted HERE on the reference's own gradient (seeds are tried in order
until a case satisfies it) and again by tests/test_adversarial_cpu.py."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EPSILONS = (0.0, 0.02, 0.04)  # test_nyuv2_depth.py:192
CASES = {"laplace": dict(loss="laplace_nll", S=2, Ci=2, f=2, N=3, H=34, W=34),
         "gaussian": dict(loss="gaussian_nll", S=3, Ci=3, f=1, N=3, H=32, W=32)}


def load_fgsm_reference():
    spec = importlib.util.spec_from_file_location("fgsm_reference", os.path.join(ROOT, "tests", "fgsm_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref):
    sys.dont_write_bytecode = True
    sys.path = [p for p in sys.path if os.path.abspath(p or ".") != ROOT]
    sys.path.insert(0, ref)
    from mimo.losses import GaussianNLL, LaplaceNLL
    from mimo.models.mimo_components.model import MimoUNet
    from mimo.models.utils import repeat_subnetworks
    import mimo
    assert os.path.abspath(mimo.__file__).startswith(os.path.abspath(ref))
    # the test script imports two package modules that need lightning / h5py; fgsm_attack touches neither
    for name, attr in (("mimo.models.ensemble", "EnsembleModule"), ("mimo.datasets.nyuv2", "NYUv2DepthDataset")):
        if name not in sys.modules:
            parts = name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
            setattr(sys.modules[name], attr, type(attr, (), {}))
    spec = importlib.util.spec_from_file_location("test_nyuv2_depth", os.path.join(ref, "scripts/test/test_nyuv2_depth.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return MimoUNet, {"laplace_nll": LaplaceNLL, "gaussian_nll": GaussianNLL}, repeat_subnetworks, script.fgsm_attack


def make_case(c, seed, MimoUNet, losses, repeat_subnetworks, fgsm_attack):
    import torch
    S, Ci, f, N, H, W = c["S"], c["Ci"], c["f"], c["N"], c["H"], c["W"]
    torch.manual_seed(seed)
    net = MimoUNet(in_channels=Ci, out_channels=2, num_subnetworks=S, filter_base_count=f)
    crit = losses[c["loss"]]()
    g = torch.Generator().manual_seed(seed + 1)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    net.train()
    for _ in range(4):  # running statistics and parameters away from their initial values
        x = torch.rand(N, S, Ci, H, W, generator=g)
        y = torch.rand(N, S, 1, H, W, generator=g)
        out = net(x)
        opt.zero_grad()
        crit(out[:, :, :1], out[:, :, 1:], y).backward()
        opt.step()
    net.eval()
    image = torch.rand(N, Ci, H, W, generator=g)
    u = torch.rand(N, Ci, H, W, generator=g)
    image = torch.where(u < 0.03, torch.zeros_like(image), torch.where(u > 0.97, torch.ones_like(image), image))
    label = torch.rand(N, 1, H, W, generator=g)
    # make_predictions, test_nyuv2_depth.py:38-58 (the ensemble's member forward is repeat_subnetworks + the network)
    labels = label.unsqueeze(1).repeat(1, S, 1, 1, 1)
    image.requires_grad = True
    x5 = repeat_subnetworks(image, num_subnetworks=S)
    x5.retain_grad()
    out = net(x5)
    y_pred, log_param = out[:, :, :1], out[:, :, 1:]
    loss = crit(y_pred, log_param, labels)
    net.zero_grad()
    loss.backward()
    data_grad = image.grad.data
    fx = {"meta": np.array([Ci, 2, S, f, N, H, W]), "loss_kind": np.array(c["loss"]), "seed": np.int64(seed),
          "image": image.detach().numpy().copy(), "label": label.numpy().copy(), "logits": out.detach().numpy().copy(),
          "loss": loss.detach().numpy().copy(), "dx_sub": x5.grad.numpy().copy(), "dimage": data_grad.numpy().copy(),
          "perturbed": np.stack([fgsm_attack(image, e, data_grad).detach().numpy() for e in EPSILONS])}
    for k, v in net.state_dict().items():
        if not k.endswith("num_batches_tracked"):
            fx["state/" + k] = v.detach().numpy().copy()
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MIMO_REFERENCE"), required="MIMO_REFERENCE" not in os.environ)
    args = ap.parse_args()
    R = load_fgsm_reference()
    ref = load_reference(args.reference)
    import torch
    torch.set_num_threads(4)
    torch.use_deterministic_algorithms(True)
    out = {"epsilons": np.array(EPSILONS, dtype=np.float64)}
    for name, c in CASES.items():
        seed = 0
        while True:
            fx = make_case(c, seed, *ref)
            share = R.undecided_share(fx["dimage"])
            img = fx["image"]
            ok = share <= R.MAX_UNDECIDED_SHARE and (img == 0).any() and (img == 1).any() and np.isfinite(fx["dimage"]).all()
            print(f"{name}: seed {seed}: undecided share {share:.4%} at {R.DECIDED_REL:g} of max|g| = {np.abs(fx['dimage']).max():.3e}"
                  f"{'' if ok else '  (rejected)'}")
            if ok:
                break
            seed += 1
            assert seed < 50, "no suitable seed"
        assert share <= R.MAX_UNDECIDED_SHARE
        for k, v in fx.items():
            out[f"{name}/{k}"] = v
    path = os.path.join(HERE, "fgsm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
