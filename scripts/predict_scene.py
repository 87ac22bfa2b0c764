"""One whole scene through a trained model: y_preds.npy, aleatoric_vars.npy and epistemic_vars.npy (the names the
reference's scripts/test/test_ndvi.py writes per batch of patches), each [C_out, H, W] for the scene [C_in, H, W] in
--scene x.npy.  The scene is cut into --patch_size tiles at --stride on the device, run in batches of --batch_size and
stitched with --window (mimo.inference.predict_scene); nothing is clipped or rescaled.

    python scripts/predict_scene.py --model_checkpoint_paths a.ckpt b.ckpt --scene scene.npy --result_dir out
    python scripts/predict_scene.py --model_checkpoint_paths a.ckpt --monte_carlo_steps 10 --scene scene.npy --result_dir out
    python scripts/predict_scene.py --evidential --model_checkpoint_paths ev.ckpt --scene scene.npy --result_dir out
    python scripts/predict_scene.py --synthetic_model --scene scene.npy --result_dir out     # a seeded network, no checkpoint

--evidential: ONE `EvidentialUnetModel` fed through `predict_uncertainties`; otherwise an `EnsembleModule` over the
checkpoints (a deep ensemble, or MC dropout with --monte_carlo_steps)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimo.inference import SceneTiler, predict_scene  # noqa: E402


def load_model(args, in_channels, device):
    kw = dict(center_dropout_rate=0.0, final_dropout_rate=0.0, weight_decay=0.0, learning_rate=1e-3, seed=0)
    rate = 0.1 if args.monte_carlo_steps else 0.0
    kw.update(encoder_dropout_rate=rate, core_dropout_rate=rate, decoder_dropout_rate=rate)
    if args.evidential:
        from mimo.models.evidential_unet import EvidentialUnetModel
        if args.synthetic_model:
            torch.manual_seed(0)
            model = EvidentialUnetModel(in_channels=in_channels, out_channels=4, filter_base_count=8, **kw)
        else:
            model = EvidentialUnetModel.load_from_checkpoint(args.model_checkpoint_paths[0])
        return model.to(device).eval()
    from mimo.models.ensemble import EnsembleModule
    models = None
    if args.synthetic_model:
        from mimo.models.mimo_unet import MimoUnetModel
        torch.manual_seed(0)
        models = [MimoUnetModel(in_channels=in_channels, out_channels=2, num_subnetworks=2, filter_base_count=8,
                                loss="laplace_nll", loss_buffer_size=10, loss_buffer_temperature=0.3, **kw)]
    return EnsembleModule(args.model_checkpoint_paths, monte_carlo_steps=args.monte_carlo_steps, models=models,
                          keep_on_device=True).to(device)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model_checkpoint_paths", nargs="*", default=[])
    ap.add_argument("--synthetic_model", action="store_true", help="a seeded network instead of checkpoints")
    ap.add_argument("--scene", required=True, help=".npy file holding a [C_in, H, W] array")
    ap.add_argument("--result_dir", required=True)
    ap.add_argument("--monte_carlo_steps", type=int, default=0)
    ap.add_argument("--evidential", action="store_true", help="one EvidentialUnetModel instead of an ensemble")
    ap.add_argument("--patch_size", type=int, default=256)
    ap.add_argument("--stride", type=int, default=249)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--window", default="linear", choices=["uniform", "linear", "crop"])
    args = ap.parse_args()
    if bool(args.model_checkpoint_paths) == args.synthetic_model:
        ap.error("give --model_checkpoint_paths or --synthetic_model")
    if args.evidential and (len(args.model_checkpoint_paths) > 1 or args.monte_carlo_steps):
        ap.error("--evidential takes one checkpoint and no --monte_carlo_steps")
    scene = np.load(args.scene)
    if scene.ndim != 3:
        ap.error(f"--scene must hold a [C_in, H, W] array, got {list(scene.shape)}")
    tiler = SceneTiler(scene.shape[1], scene.shape[2], args.patch_size, args.stride, args.window)  # argument errors first
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    model = load_model(args, scene.shape[0], device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    scene_dev = torch.from_numpy(np.ascontiguousarray(scene, dtype=np.float32)).to(device)
    a.record()
    maps = predict_scene(model, scene_dev, patch_size=args.patch_size, stride=args.stride, batch_size=args.batch_size,
                         window=args.window)
    b.record()
    torch.cuda.synchronize()
    os.makedirs(args.result_dir, exist_ok=True)
    for name, t in zip(("y_preds", "aleatoric_vars", "epistemic_vars"), maps):
        np.save(os.path.join(args.result_dir, name + ".npy"), t.cpu().numpy())
    print(json.dumps({"scene": list(scene.shape), "tiles": tiler.num_tiles, "grid": [tiler.ny, tiler.nx],
                      "batches": tiler.num_batches(args.batch_size), "window": args.window,
                      "first_call_ms": round(a.elapsed_time(b), 3), "result_dir": args.result_dir}))


if __name__ == "__main__":
    main()
