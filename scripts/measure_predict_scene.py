"""What whole-scene inference costs on one GPU: a synthetic 2 x 2048 x 2048 scene cut into 256-pixel tiles at a stride of
249 (9 x 9 = 81 tiles), cfg3's network (bench.py) in eval mode as a one-member `EnsembleModule`, batches of 32 tiles.

Reports, from --repeats timed runs after --warmup untimed ones, all timed with device events:
  engine      mimo.inference.predict_scene: scene milliseconds and tiles per second
  launches    the span of one `SceneTiler.gather` call and of one `SceneTiler.stitch` call (three maps, 32 tiles) taken
              over --calls back-to-back calls between two events — an upper bound on the device time, the host's per-call
              work lies inside the span — next to one batch's forward, and their share of it
  torch_route the same scene through the route a user writes today, restated in torch here: the tiles from an unfolded
              view indexed at the origins, the same model calls (the last batch short: 17 tiles), then
              `index_put_(accumulate=True)` of w v and of w over all tiles and one division per map; the index tensors and
              the window are built once outside the timed span
and the largest difference between the two routes' maps.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out, ms = None, []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(round(a.elapsed_time(b), 3))
    return out, ms


def span_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) / calls * 1e3, 2)


class TorchRoute:
    """Cut, batch, accumulate and divide with torch operators."""

    def __init__(self, tiler, scene, batch_size):
        p, dev = tiler.patch_size, scene.device
        origins = torch.tensor(tiler.origins(), device=dev)  # [T, 2]
        self.oy, self.ox, self.batch_size, self.tiles_total = origins[:, 0], origins[:, 1], batch_size, tiler.num_tiles
        ramp = torch.arange(p, device=dev)
        self.yy = (self.oy[:, None, None] + ramp[None, :, None]).expand(-1, p, p).contiguous()
        self.xx = (self.ox[:, None, None] + ramp[None, None, :]).expand(-1, p, p).contiguous()
        w1 = torch.minimum(ramp + 1, p - ramp).float() if tiler.window == "linear" else torch.ones(p, device=dev)
        self.w2 = (w1[:, None] * w1[None, :])[None].expand(tiler.num_tiles, p, p).contiguous()
        self.shape = (tiler.height, tiler.width)

    def __call__(self, model, scene):
        p = self.w2.shape[-1]
        tiles = scene.unfold(1, p, 1).unfold(2, p, 1)[:, self.oy, self.ox].permute(1, 0, 2, 3).contiguous()  # [T, C, P, P]
        results = [model(tiles[t0:t0 + self.batch_size]) for t0 in range(0, self.tiles_total, self.batch_size)]
        den = torch.zeros(self.shape, device=scene.device).index_put_((self.yy, self.xx), self.w2, accumulate=True)
        maps = []
        for k in range(3):
            v = torch.cat([r[k] for r in results])[:, 0]  # [T, P, P]
            num = torch.zeros(self.shape, device=scene.device).index_put_((self.yy, self.xx), self.w2 * v, accumulate=True)
            maps.append((num / den)[None])
        return tuple(maps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--patch_size", type=int, default=256)
    ap.add_argument("--stride", type=int, default=249)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--window", default="linear", choices=["uniform", "linear"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_scene", "measure_predict_scene.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_predict_scene.py needs a GPU: a timing taken anywhere else says nothing")
    import bench
    from mimo.inference import SceneTiler, predict_scene
    from mimo.models.ensemble import EnsembleModule

    c = bench.CONFIGS["cfg3"]
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    model = EnsembleModule([], models=[bench.make_model(c).cuda().eval()], keep_on_device=True)
    scene = torch.rand(c["Ci"], args.size, args.size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    kw = dict(patch_size=args.patch_size, stride=args.stride, batch_size=args.batch_size, window=args.window)
    tiler = SceneTiler(args.size, args.size, args.patch_size, args.stride, args.window)
    route = TorchRoute(tiler, scene, args.batch_size)

    def engine():
        return predict_scene(model, scene, **kw)

    def torch_route():
        return route(model, scene)

    for _ in range(args.warmup):
        engine()
        torch_route()
    got, engine_ms = timed(engine, args.repeats)
    want, torch_ms = timed(torch_route, args.repeats)
    diff = [float((a - b).abs().max()) for a, b in zip(got, want)]

    # the launches on their own, and one batch's forward
    tiles = tiler.gather(scene, 0, args.batch_size)
    results = model(tiles)
    maps = [tiler.scene_buffer(r.shape[1], scene.device) for r in results]
    n_valid = min(args.batch_size, tiler.num_tiles)
    fields = [(r, m) for r, m in zip(results, maps)]
    gather_us = span_us(lambda: tiler.gather(scene, 0, args.batch_size), args.calls)
    stitch_us = span_us(lambda: tiler.stitch(fields, 0, n_valid), args.calls)
    forward_us = span_us(lambda: model(tiles), 10)
    p, ci = args.patch_size, c["Ci"]
    res = {
        "what": f"predict_scene: {ci} x {args.size} x {args.size} scene, patch {p}, stride {args.stride}, {tiler.num_tiles} tiles, "
                f"batches of {args.batch_size}, window {args.window}, cfg3 network in eval mode",
        "tiles": tiler.num_tiles, "batches": tiler.num_batches(args.batch_size), "repeats": args.repeats,
        "engine_scene_ms": engine_ms, "engine_tiles_per_s": [round(tiler.num_tiles / (ms * 1e-3), 1) for ms in engine_ms],
        "torch_route_scene_ms": torch_ms, "torch_route_tiles_per_s": [round(tiler.num_tiles / (ms * 1e-3), 1) for ms in torch_ms],
        "max_abs_difference_between_routes": diff,
        "gather_call_us_upper_bound": gather_us, "stitch_call_us_upper_bound": stitch_us, "batch_forward_us": forward_us,
        "gather_plus_stitch_share_of_forward": round((gather_us + stitch_us) / forward_us, 5),
        "gather_call_bytes": 2 * 4 * args.batch_size * ci * p * p,
        # nominal, per map: every tile pixel of the launch read once and as many bytes again written; the pixels actually
        # written are fewer by the overlaps (47.4 MB in all, not 50.3, for tiles 0 ... 31 of the default scene)
        "stitch_call_bytes_nominal": 3 * 2 * 4 * n_valid * p * p,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
