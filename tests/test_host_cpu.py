"""CPU-side checks of the host mirror and of the C-ABI library (no GPU needed): interface
parity with the reference's module surface, golden-pinned host arithmetic, exported symbols,
and the data-parallel plumbing over gloo with world_size 2."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import free_port, load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(built_library):
    from mimo_unet_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    declared = set(re.findall(r"\b(mimo_[a-z0-9_]+)\s*\(", header))
    declared -= {"mimo_plan"}  # typedef
    assert len(declared) >= 20
    for name in sorted(declared):
        assert hasattr(lib, name), f"libmimo_hip.so does not export {name}"
    assert set(_lib.EXPORTED_SYMBOLS) <= declared
    assert lib.mimo_version() >= 1


def test_library_dynamic_symbol_table_is_exactly_the_c_abi(built_library):
    """-fvisibility=hidden + the linker version script (csrc/exports.map): `nm -D` shows the functions declared in
    include/mimo_hip.h and nothing else — no C++ internals, device stubs, kernel handles or libstdc++ instantiations."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    declared = set(re.findall(r"\b(mimo_[a-z0-9_]+)\s*\(", header)) - {"mimo_plan"}
    assert exported == declared, (sorted(exported - declared)[:10], sorted(declared - exported)[:10])


def test_no_cpu_execution_path():
    from mimo.models.mimo_components.model import MimoUNet
    from mimo_unet_amd._lib import MimoHipError
    net = MimoUNet(3, 2, 1, 4)
    with pytest.raises(MimoHipError):
        net(torch.zeros(1, 1, 3, 32, 32))


def test_seeded_init_and_state_dict_match_reference():
    from mimo.models.mimo_components.model import MimoUNet
    for name in ("cfg1_step.npz", "mini_s2_step.npz"):
        fx = load_npz(name)
        Ci, Co, S, f = (int(v) for v in fx["meta"][:4])
        torch.manual_seed(1 if name.startswith("cfg1") else 2)
        net = MimoUNet(Ci, Co, S, f)
        sd = net.state_dict()
        ref = {k[len("init/"):]: v for k, v in fx.items() if k.startswith("init/")}
        assert list(sd.keys()) == list(ref.keys())  # same names, same order as the reference's state_dict
        for k, v in ref.items():
            assert np.array_equal(sd[k].numpy(), v), k


def test_constructor_contract():
    from mimo.models.mimo_components.model import MimoUNet
    with pytest.raises(ValueError):
        MimoUNet(3, 2, 2, 4, encoder_dropout_rate=0.1, center_dropout_rate=0.1)
    net = MimoUNet(3, 2, 2, 4, encoder_dropout_rate=0.1, core_dropout_rate=0.1, decoder_dropout_rate=0.1)
    drops = [m for m in net.modules() if m.__class__.__name__.startswith("Dropout")]
    assert len(drops) == len(net.double_convs()) + 1 + 2  # + center_dropout + S final_dropouts


def test_transient_state_is_complete_on_fresh_copied_and_unpickled_models():
    """Everything the engine derives from the module tree is declared once (`_TRANSIENT`): a fresh, a deep-copied and an
    unpickled model have every one of these attributes at its empty value, and a pickle carries none of them."""
    import copy
    import pickle
    from mimo.models.mimo_components.model import MimoUNet
    fresh = MimoUNet(3, 2, 2, 4)
    assert {"_plans", "_evicted_status", "_mask_plan", "grad_sync", "grad_ready_hook", "_inference_keep", "_flat_params",
            "_dc_cache"} <= set(MimoUNet._TRANSIENT)
    fresh.double_convs()  # fills the cached module lists
    fresh._evicted_status, fresh.grad_sync, fresh._inference_keep = 5, object(), (torch.zeros(1),)
    assert not set(fresh.__getstate__()) & set(MimoUNet._TRANSIENT)
    assert "_geom" in fresh.__getstate__() and "_plan_cache_size" in fresh.__getstate__()
    for net in (MimoUNet(3, 2, 2, 4), copy.deepcopy(fresh), pickle.loads(pickle.dumps(fresh))):
        assert all(name in net.__dict__ for name in MimoUNet._TRANSIENT)
        assert len(net._plans) == 0 and net._evicted_status == 0
        assert net._mask_plan is None and net.grad_sync is None and net._inference_keep is None and net._dc_cache is None
        assert net.numerics_status() == 0  # (no plan: nothing touches the device)
        assert [k for k, _ in net.named_parameters()] == [k for k, _ in fresh.named_parameters()]


def test_loss_classes_match_reference_golden():
    from mimo.losses import GaussianNLL, LaplaceNLL, UncertaintyLoss
    fx = load_npz("losses.npz")
    mu, y, ls, mask = (torch.from_numpy(fx[k]) for k in ("mu", "y", "ls", "mask"))
    for kind, crit in (("laplace", LaplaceNLL()), ("gaussian", GaussianNLL())):
        a, b = mu.clone().requires_grad_(True), ls.clone().requires_grad_(True)
        raw = crit.forward(a, b, y, reduce_mean=False, mask=mask)
        raw.sum().backward()
        np.testing.assert_allclose(raw.detach().numpy(), fx[kind + "/raw"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(a.grad.numpy(), fx[kind + "/dmu"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(b.grad.numpy(), fx[kind + "/dls"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(crit.forward(mu, ls, y).numpy(), fx[kind + "/mean"], rtol=1e-6)
        np.testing.assert_allclose(crit.std(mu, ls).numpy(), fx[kind + "/std"], rtol=1e-6)
        np.testing.assert_allclose(crit.calculate_dist_param(crit.std(mu, ls), log=True).numpy(),
                                   fx[kind + "/dist_param_log"], rtol=1e-5, atol=1e-6)
        assert crit.num_distribution_params == 2 and crit.mode(mu, ls) is mu
    assert isinstance(UncertaintyLoss.from_name("laplace_nll"), LaplaceNLL)
    with pytest.raises(ValueError):
        UncertaintyLoss.from_name("huber")


def test_loss_buffer_matches_reference_golden():
    from mimo.models.mimo_components.loss_buffer import LossBuffer
    fx = load_npz("losses.npz")
    lb = LossBuffer(subnetworks=3, temperature=0.3, buffer_size=10)
    for i, row in enumerate(torch.from_numpy(fx["lossbuf/seq"])):
        np.testing.assert_allclose(lb.get_weights().numpy(), fx["lossbuf/weights"][i], rtol=1e-6)
        lb.add(row)
    np.testing.assert_allclose(lb.buffer.numpy(), fx["lossbuf/final"])
    lb0 = LossBuffer(subnetworks=2, temperature=1.0, buffer_size=0)
    lb0.add(torch.ones(2))
    np.testing.assert_allclose(lb0.get_weights().numpy(), fx["lossbuf/size0_weights"])


def test_permutation_draw_replays_reference():
    from mimo.models.utils import apply_input_transform, flatten_subnetwork_dimension, repeat_subnetworks
    from mimo_unet_amd.models.utils import draw_subnetwork_permutations
    fx = load_npz("mini_s2_step.npz")
    torch.manual_seed(1000 + 2)
    perms = draw_subnetwork_permutations(3, 2)
    assert np.array_equal(perms.numpy(), fx["s0/perms"])  # same RNG consumption as utils.py:27-36
    img = torch.from_numpy(fx["s0/image"])
    torch.manual_seed(1000 + 2)
    xt, yt, mt = apply_input_transform(img, torch.from_numpy(fx["s0/label"]), None, num_subnetworks=2)
    assert torch.equal(xt, torch.stack([img[perms[s]] for s in range(2)], 1)) and mt is None
    assert repeat_subnetworks(img, 4).shape == (3, 4, 2, 32, 32)
    assert flatten_subnetwork_dimension(xt).shape == (6, 2, 32, 32)
    torch.manual_seed(0)
    p = draw_subnetwork_permutations(4, 3, input_repetition_probability=0.5, batch_repetitions=2)
    assert p.shape == (3, 8) and torch.equal(p[0, 4:], p[1, 4:]) and torch.equal(p[0, 4:], p[2, 4:])


def test_lightning_surface_and_checkpoint_roundtrip(tmp_path):
    from mimo.models.mimo_unet import MimoUnetModel
    parser = MimoUnetModel.add_model_specific_args(argparse.ArgumentParser())
    a = parser.parse_args([])
    assert (a.num_subnetworks, a.filter_base_count, a.loss, a.learning_rate, a.loss_buffer_size,
            a.loss_buffer_temperature, a.scheduler_step_size, a.scheduler_gamma) == (3, 32, "laplace_nll", 1e-3, 10, 1.0, 20, 0.5)
    kw = dict(in_channels=3, out_channels=2, num_subnetworks=2, filter_base_count=4, center_dropout_rate=0.0,
              final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0,
              loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3, seed=1, loss_buffer_size=10,
              loss_buffer_temperature=0.3)
    m = MimoUnetModel(**kw)
    assert m.hparams["trainable_params"] == sum(p.numel() for p in m.model.parameters())
    assert m.hparams["loss"] == "laplace_nll" and m.compile() is m
    cfgd = m.configure_optimizers()
    assert set(cfgd) == {"optimizer", "lr_scheduler", "monitor"} and cfgd["monitor"] == "val_loss"
    assert isinstance(cfgd["lr_scheduler"], torch.optim.lr_scheduler.StepLR)
    path = os.path.join(tmp_path, "m.ckpt")
    ck = m.checkpoint_dict() if hasattr(m, "checkpoint_dict") else {"state_dict": m.state_dict(), "hyper_parameters": dict(m.hparams)}
    ck["state_dict"] = {k.replace("model.", "model._orig_mod.", 1): v for k, v in ck["state_dict"].items()}  # compiled-reference ckpt
    torch.save(ck, path)
    m2 = MimoUnetModel.load_from_checkpoint(path)
    for (k1, v1), (k2, v2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)


def _ddp_worker(rank, world, port, q):
    import torch.distributed as dist
    from mimo_unet_amd.ddp import FlatGradientAllReducer, shard_batch
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(7)
    full = {"image": torch.rand(8, 2, 4, 4, generator=g), "label": torch.rand(8, 1, 4, 4, generator=g), "mask": None}
    shard = shard_batch(full, rank, world)
    # stand-in per-rank "gradient": a deterministic function of the shard, 1000 floats
    flat = torch.cat([shard["image"].flatten(), shard["label"].flatten()]).repeat(7)[:1000].clone()
    local = flat.clone()
    red = FlatGradientAllReducer(bucket_bytes=256 * 4, min_bucket_bytes=200 * 4)  # buckets of <= 256 floats
    # announced like the engine does: adjacent ranges from the tail to the head; small ones are merged
    red.start(flat, 900, 1000)   # held (100 < 200)
    red.start(flat, 850, 900)    # merged: 150, still held
    red.start(flat, 500, 850)    # merged: [500, 1000) -> issued as 256 + 244
    red.start(flat, 0, 500)      # issued as 256 + 244
    assert red.issued == [(500, 756), (756, 1000), (0, 256), (256, 500)], red.issued
    red.finish()
    # no_sync(): announcements inside are dropped (gradient accumulation), the reducer stays idle
    with red.no_sync():
        red.start(flat, 0, 1000)
    assert not red.busy and red.issued == []
    # BatchNorm running buffers: per rank while training, rank 0's at a checkpoint (ddp.broadcast_buffers)
    from mimo_unet_amd.ddp import broadcast_buffers
    bn = torch.nn.BatchNorm2d(3)
    bn.running_mean.fill_(float(rank + 1))
    broadcast_buffers(bn)
    assert float(bn.running_mean[0]) == 1.0 and int(bn.num_batches_tracked) == 0
    q.put((rank, local.numpy(), flat.clone().numpy(), red.scale, shard["image"].shape[0]))  # by value
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_allreduce_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res = [(r, torch.from_numpy(a), torch.from_numpy(b), c, d) for r, a, b, c, d in res]
    (_, l0, r0, s0, n0), (_, l1, r1, s1, n1) = res
    assert n0 == n1 == 4 and s0 == s1 == 0.5
    assert torch.allclose(r0, l0 + l1) and torch.equal(r0, r1)          # every rank holds the sum
    assert torch.allclose(r0 * s0, (l0 + l1) / 2)                        # optimiser sees the mean of the shard grads


def _rs_worker(rank, world, port, q):
    import torch.distributed as dist
    from mimo_unet_amd.ddp import FlatGradientAllReducer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(40 + rank)
    local = torch.randn(1003, generator=g)  # 1003: no bucket divides evenly over 2 or 3 ranks
    out = {}
    for algo in FlatGradientAllReducer.ALGORITHMS:
        flat = local.clone()
        red = FlatGradientAllReducer(bucket_bytes=300 * 4, min_bucket_bytes=100 * 4, algorithm=algo)
        for b, e in ((800, 1003), (750, 800), (301, 750), (0, 301)):  # tail to head, like the backward announces them
            red.start(flat, b, e)
        red.finish()
        assert not red.busy and len(red.last_issued) >= 4
        out[algo] = flat.numpy()
    q.put((rank, local.numpy(), out["all_reduce"], out["reduce_scatter"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_reduce_scatter_all_gather_reducer_equals_all_reduce_gloo(world):
    """VERDICT r5 item 6b / SURVEY §5: the bucketed exchange as in-place reduce-scatter + all-gather (the direct form for the
    fully connected xGMI topology) leaves the same sums on every rank as `dist.all_reduce` — bit-identical across ranks, and
    bit-identical to the all-reduce at two ranks (a + b has one order); buckets that do not divide by the world size send
    their remainder as a small all-reduce."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_rs_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    total = sum(torch.from_numpy(l).double() for _, l, _, _ in res)
    for _, _, ar, rs in res:
        ar, rs = torch.from_numpy(ar), torch.from_numpy(rs)
        assert torch.equal(rs, torch.from_numpy(res[0][3]))  # every rank holds the same bits
        assert torch.allclose(rs.double(), total, rtol=1e-6, atol=1e-6)
        if world == 2:
            assert torch.equal(rs, ar)
        else:
            assert torch.allclose(rs, ar, rtol=1e-6, atol=1e-6)


def test_evidential_loss_class_matches_golden():
    """mimo.losses.EvidentialLoss (host mirror) on the reference's golden NIG parameters."""
    from mimo.losses import EvidentialLoss
    from tests.helpers import load_npz
    fx = load_npz("evidential.npz")
    crit = EvidentialLoss(coeff=1.0)
    ev, y, mask = (torch.from_numpy(fx[k]) for k in ("ev", "y", "mask"))
    np.testing.assert_allclose(crit(ev, y, mask=mask).numpy(), fx["loss"], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(crit.aleatoric_var(ev).numpy(), fx["aleatoric_var"], rtol=1e-6)
    np.testing.assert_allclose(crit.epistemic_var(ev).numpy(), fx["epistemic_var"], rtol=1e-6)
    np.testing.assert_allclose(crit(torch.from_numpy(fx["ext/ev"]), torch.from_numpy(fx["ext/y"])).numpy(), fx["ext/loss"],
                               rtol=1e-5)
    assert torch.equal(crit.mode(ev), ev[:, 0]) and crit.num_distribution_params == 4
    assert float(crit(ev, y, reduce_mean=True)) == float(crit(ev, y).mean())


def test_alias_package_resolves_unmirrored_submodules_from_the_reference(tmp_path):
    """scripts/train/train_ndvi.py:10-13 imports mimo.models.* (mirrored here) and mimo.tasks / mimo.datasets (not):
    with the repo first and the reference second on PYTHONPATH both resolve, each from its own tree.  The reference
    checkout is stood in for by a tree of the same layout (an empty mimo/__init__.py, its own mimo.models / mimo.losses,
    which must lose to ours, and the unmirrored mimo.regularization / mimo.visualization, which must be found there)."""
    import subprocess
    import sys
    ref = tmp_path / "reference"
    for rel in ("mimo/__init__.py", "mimo/models/__init__.py"):
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text("")
    for rel in ("mimo/models/mimo_unet.py", "mimo/models/ensemble.py", "mimo/losses.py", "mimo/regularization.py",
                "mimo/visualization.py"):
        (ref / rel).write_text("TREE = 'reference'\n")
    code = ("import mimo.models.mimo_unet as a, mimo.models.ensemble as e, mimo.losses as l\n"
            "import mimo.regularization as r, mimo.visualization as v\n"
            "print(a.__file__); print(e.__file__); print(l.__file__); print(r.__file__); print(v.__file__)\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + str(ref), PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    files = out.stdout.split()
    assert all(f.startswith(ROOT + os.sep) for f in files[:3]), files
    assert all(f.startswith(str(ref) + os.sep) for f in files[3:]), files


class _FakeFlatNet(torch.nn.Module):
    """Two parameters that are views of one flat buffer, like MimoUNet after _ensure_flat."""

    def __init__(self):
        super().__init__()
        self.flat = torch.arange(10, dtype=torch.float32) / 10
        self.grads = torch.zeros(10)
        self.a = torch.nn.Parameter(torch.zeros(2, 3))
        self.b = torch.nn.Parameter(torch.zeros(4))
        self.a.data = self.flat[0:6].view(2, 3)
        self.b.data = self.flat[6:10]

    def flat_parameters(self):
        return self.flat

    def flat_gradients(self):
        return self.grads


def _torch_adam_step(p, g, m, v, *, lr, betas, eps, weight_decay, step, grad_scale):
    g = g * grad_scale + weight_decay * p
    m.mul_(betas[0]).add_(g, alpha=1 - betas[0])
    v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
    p.sub_(lr * (m / (1 - betas[0] ** step)) / ((v / (1 - betas[1] ** step)).sqrt() + eps))


def test_flat_adam_state_roundtrip_and_reference_adam_state(monkeypatch):
    """FlatAdam.load_state_dict: own checkpoints survive a CPU-mapped save/load (no silent re-zeroing of the
    moments), a reference torch.optim.Adam state_dict is scattered into the flat layout, the caller's dict is
    left alone, and a wrong-sized state is an error."""
    import copy
    import io

    from mimo_unet_amd import optim as OP
    monkeypatch.setattr(OP, "adam_step", _torch_adam_step)
    g = torch.Generator().manual_seed(0)
    grads = [torch.randn(10, generator=g) for _ in range(4)]

    def run(net, opt, gs):
        for gr in gs:
            net.grads.copy_(gr)
            opt.step()

    net = _FakeFlatNet()
    opt = OP.FlatAdam(net, lr=1e-2)
    run(net, opt, grads[:2])
    buf = io.BytesIO()
    torch.save({"opt": opt.state_dict(), "flat": net.flat.clone()}, buf)
    run(net, opt, grads[2:])
    want = net.flat.clone()
    # resume from the checkpoint
    ck = torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=False)
    net2 = _FakeFlatNet()
    net2.flat.copy_(ck["flat"])
    opt2 = OP.FlatAdam(net2, lr=1e-2)
    before = copy.deepcopy({k: v for k, v in ck["opt"].items() if k != "flat"})
    opt2.load_state_dict(ck["opt"])
    assert "flat" in ck["opt"] and {k: v for k, v in ck["opt"].items() if k != "flat"} == before  # not mutated
    run(net2, opt2, grads[2:])
    assert torch.equal(net2.flat, want)
    # a reference torch.optim.Adam checkpoint (per-parameter state)
    net3 = _FakeFlatNet()
    ref = torch.optim.Adam(net3.parameters(), lr=1e-2)
    for gr in grads[:2]:
        net3.a.grad, net3.b.grad = gr[:6].view(2, 3).clone(), gr[6:].clone()
        ref.step()
    net4 = _FakeFlatNet()
    net4.flat.copy_(net3.flat)
    opt4 = OP.FlatAdam(net4, lr=1e-2)
    opt4.load_state_dict(ref.state_dict())
    for gr in grads[2:]:
        net3.a.grad, net3.b.grad = gr[:6].view(2, 3).clone(), gr[6:].clone()
        ref.step()
    run(net4, opt4, grads[2:])
    assert opt4._step == 4
    torch.testing.assert_close(net4.flat, net3.flat, rtol=1e-6, atol=1e-7)
    # wrong architecture
    bad = opt.state_dict()
    bad["flat"] = {"step": 1, "exp_avg": torch.zeros(7), "exp_avg_sq": torch.zeros(7)}
    with pytest.raises(ValueError):
        opt2.load_state_dict(bad)


def test_logging_without_a_trainer_and_parameter_version_tracks_loads():
    from mimo.models.mimo_unet import MimoUnetModel
    m = MimoUnetModel(in_channels=3, out_channels=2, num_subnetworks=2, filter_base_count=4, center_dropout_rate=0.0,
                      final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0, decoder_dropout_rate=0.0,
                      loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3, seed=0, loss_buffer_size=10,
                      loss_buffer_temperature=0.3)
    assert m._batch_size() is None
    m._log("x", torch.tensor(1.0))
    assert float(m.logged["x"]) == 1.0

    class DM:
        batch_size = 7

    class TR:
        datamodule = DM()

    m.trainer = TR()
    assert m._batch_size() == 7
    # every load_state_dict through the net invalidates the inference cache key
    e0 = m.model._param_epoch
    m.load_state_dict(m.state_dict())
    assert m.model._param_epoch > e0


def test_bench_multi_gpu_request_without_gpus_fails_cleanly():
    """`bench.py --gpus 2` is self-launching; on a box without two GPUs it must say so (before any GPU call) instead of
    silently running one rank."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIMO_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs present: the multi-rank run itself is covered by the gpu tests")
    assert r.returncode != 0 and "GPU(s) visible" in (r.stderr + r.stdout)


def test_bench_counts_gpus_without_touching_hip(tmp_path, monkeypatch):
    """The parent of a self-launched N-rank run counts GPUs from the KFD topology in sysfs and the *_VISIBLE_DEVICES
    variables — no torch.cuda / HIP call before it forks."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    nodes = tmp_path / "kfd" / "topology" / "nodes"
    for i, simd in enumerate([0, 0, 1024, 1024, 1024, 1024]):  # two CPU nodes, four GPUs
        (nodes / str(i)).mkdir(parents=True)
        (nodes / str(i) / "properties").write_text(f"cpu_cores_count {64 if simd == 0 else 0}\nsimd_count {simd}\n")
    for v in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    assert bench.visible_gpu_count(str(nodes)) == 4
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,2")
    assert bench.visible_gpu_count(str(nodes)) == 2
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "1")
    assert bench.visible_gpu_count(str(nodes)) == 1
    # no KFD sysfs tree (masked in a container, or no driver): "sysfs does not say" — the ranks' own device check decides
    assert bench.visible_gpu_count(str(tmp_path / "nothing" / "topology" / "nodes")) is None
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src[src.index("def spawn_ranks"):src.index("def main")]
    assert "torch.cuda" not in body.split('"""')[2]  # the spawning parent makes no torch.cuda call


def test_bench_reports_counter_traffic_only_for_the_running_kernel_sources(tmp_path, monkeypatch):
    """`roofline.traffic` comes from a committed rocprofv3 counter summary; it must be the summary of THIS
    build.  pmc_traffic.json carries the content hash of mimo_unet_amd/csrc/*.{hip,h} it was collected on; another hash (or
    none, as in the round-3 file) gives (None, reason) and bench.py prints traffic: null."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    h = bench.csrc_hash()
    assert len(h) == 16 and h == bench.csrc_hash()
    final = tmp_path / "profiles" / "r99" / "final"
    final.mkdir(parents=True)
    # the hash is computed over the real sources: keep ROOT for it, redirect only the profile lookup
    real_root = bench.ROOT
    monkeypatch.setattr(bench, "csrc_hash", lambda: h)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    (final / "pmc_traffic.json").write_text(json.dumps({"csrc_hash": "0" * 16, "step_bytes": 1, "classes": {}}))
    pt, why = bench.pmc_traffic()
    assert pt is None and "other kernel sources" in why
    (final / "pmc_traffic.json").write_text(json.dumps({"step_bytes": 1, "classes": {}}))  # no hash at all (round-3 file)
    assert bench.pmc_traffic()[0] is None
    (final / "pmc_traffic.json").write_text(json.dumps({"csrc_hash": h, "step_bytes": 7, "classes": {}}))
    pt, src = bench.pmc_traffic()
    assert pt["step_bytes"] == 7 and src.endswith("pmc_traffic.json")
    monkeypatch.setattr(bench, "ROOT", real_root)
    # the committed summary of this round belongs to the committed sources
    pt, src = bench.pmc_traffic()
    if pt is None:
        # kernel sources edited since the last counter collection: bench.py then reports traffic = null with this reason
        # (never a stale figure); the round's final profile run (scripts/collect_profiles.sh) makes them agree again
        assert "other kernel sources" in src, src
        pytest.skip("committed counter summary is stale against the kernel sources: " + src)
    assert "profiles/r0" in src, src


def test_bench_algorithmic_byte_model_matches_survey_table():
    """SURVEY 8(d) contract figures: cfg3 = 525.3 / 188.7 / 94.4 / 47.2 / 5.9 MB per image and tier (861.5 total),
    194.8 GFLOP per image; cfg2 605.0 MB, 95.4 GFLOP."""
    import bench
    tiers, total = bench.algorithmic_bytes_per_image(bench.CONFIGS["cfg3"])
    assert [round(t / 1e6, 1) for t in tiers] == [525.3, 188.7, 94.4, 47.2, 5.9] and round(total / 1e6, 1) == 861.5
    flops = 3 * sum(2 * ci * co * k * k * h * w for _, ci, co, h, w, k in bench.conv_layers(bench.CONFIGS["cfg3"]))
    assert round(flops / 1e9, 1) == 194.8
    assert round(bench.algorithmic_bytes_per_image(bench.CONFIGS["cfg2"])[1] / 1e6, 1) == 605.0


def test_bench_dump_outputs_caps_and_samples_deterministically(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy per array, whole up to its cap, else the same seeded sample of its elements every run;
    the caps keep the files below 64 MB in all."""
    import bench
    assert 4 * sum(bench.DUMP_CAPS.values()) < 64e6
    monkeypatch.setitem(bench.DUMP_CAPS, "preds", 10)
    preds = torch.arange(24, dtype=torch.float64).view(2, 3, 4)
    loss = torch.tensor(1.5, dtype=torch.float16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"preds": preds, "loss": loss})
    a, b = np.load(tmp_path / "a" / "preds.npy"), np.load(tmp_path / "b" / "preds.npy")
    assert a.dtype == np.float32 and a.shape == (10,) and np.array_equal(a, b)
    assert len(set(a.tolist())) == 10 and set(a.tolist()) <= set(range(24)) and np.all(np.diff(a) > 0)
    lo = np.load(tmp_path / "a" / "loss.npy")
    assert lo.dtype == np.float32 and lo.shape == () and float(lo) == 1.5
    bench.dump_outputs(str(tmp_path / "c"), {"preds": preds[0, :2]})  # 8 elements: whole, shape kept
    assert np.array_equal(np.load(tmp_path / "c" / "preds.npy"), preds[0, :2].numpy().astype(np.float32))


def test_flat_adam_follows_the_grad_scaler_protocol_for_fused_optimizers(monkeypatch):
    """torch.amp.GradScaler hands a fused optimiser (`_step_supports_amp_scaling`) two tensor attributes around step():
    `grad_scale` (divide the gradients by it) and `found_inf` (skip the step when non-zero) and deletes them afterwards.
    FlatAdam forwards them to the device-side kernel, keeps its own multiplier under another name (`reduce_scale`) and
    counts steps on the device so that a skipped step does not advance the bias correction."""
    from mimo_unet_amd import optim as OP
    calls = []

    def fake_amp(p, g, m, v, *, lr, betas, eps, weight_decay, step_dev, reduce_scale, amp_scale, found_inf):
        calls.append((None if amp_scale is None else float(amp_scale), None if found_inf is None else float(found_inf)))
        if found_inf is not None and float(found_inf) != 0:
            return
        step_dev += 1
        gs = g * reduce_scale / (1.0 if amp_scale is None else float(amp_scale))
        _torch_adam_step(p, gs, m, v, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, step=int(step_dev.item()), grad_scale=1.0)

    monkeypatch.setattr(OP, "adam_step", _torch_adam_step)
    monkeypatch.setattr(OP, "adam_step_amp", fake_amp)
    net, ref = _FakeFlatNet(), _FakeFlatNet()
    opt, ropt = OP.FlatAdam(net, lr=1e-2), OP.FlatAdam(ref, lr=1e-2)
    assert opt._step_supports_amp_scaling and opt.reduce_scale == 1.0 and not hasattr(opt, "grad_scale")
    g = torch.Generator().manual_seed(1)
    grads = [torch.randn(10, generator=g) for _ in range(3)]
    # scaled step, overflow step (skipped), scaled step  ==  two plain steps on the unscaled gradients
    for i, (gr, inf) in enumerate(((grads[0], 0.0), (grads[1], 1.0), (grads[2], 0.0))):
        net.grads.copy_(gr * 1024.0)
        opt.grad_scale, opt.found_inf = torch.tensor(1024.0), torch.tensor(inf)   # what GradScaler.step() sets ...
        opt.step()
        del opt.grad_scale, opt.found_inf                                          # ... and removes
    for gr in (grads[0], grads[2]):
        ref.grads.copy_(gr)
        ropt.step()
    assert opt.step_count == 2 and calls == [(1024.0, 0.0), (1024.0, 1.0), (1024.0, 0.0)]
    torch.testing.assert_close(net.flat, ref.flat, rtol=1e-6, atol=1e-7)
    # once the device counter exists, a plain step keeps using it
    net.grads.copy_(grads[1])
    opt.step()
    assert opt.step_count == 3 and calls[-1] == (None, None)
    assert opt.state_dict()["flat"]["step"] == 3


def test_oracle_mixed_precision_emulation_inserts_the_storage_roundings():
    """O.conv_operands("bf16-mixed" | "16-mixed"): operands and stored tensors rounded like the engine's 16-bit storage
    modes — eval forward deviates from fp32 at the level of the type (and fp16 less than bf16), a training step runs,
    updates the running statistics from the UNROUNDED conv output and stays within mixed-precision distance of fp32."""
    from oracle import mimo_oracle as O
    cfg = O.NetConfig(3, 2, 2, 4)
    st = O.init_state(cfg, 0)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 2, 3, 32, 32, generator=g)
    with torch.no_grad():
        ref = O.mimo_unet_forward(cfg, st, x, training=False)
        errs = {}
        for kind in ("bf16", "bf16-mixed", "16-mixed"):
            with O.conv_operands(kind):
                out = O.mimo_unet_forward(cfg, st, x, training=False)
            errs[kind] = float((out - ref).abs().max() / ref.abs().max())
    assert 1e-6 < errs["16-mixed"] < errs["bf16-mixed"] < 2e-2 and errs["16-mixed"] < 2e-3
    img, lab = torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 1, 32, 32, generator=g)
    perms = O.draw_perms(2, 2, generator=g)
    res = {}
    for kind in ("fp32", "16-mixed"):
        ts = O.TrainState(cfg=cfg, st={k: v.clone() for k, v in st.items()}, loss_buffer=O.LossBuffer(2, 0.3, 10))
        with O.conv_operands(kind):
            r = O.train_step(ts, img, lab, None, perms, apply_optimizer=False)
        res[kind] = (float(r["total"]), ts.st["core.down2.conv.double_conv.1.running_mean"].clone(),
                     torch.cat([v.flatten() for k, v in sorted(r["grads"].items())]))
    assert abs(res["16-mixed"][0] - res["fp32"][0]) < 5e-3 * abs(res["fp32"][0])
    torch.testing.assert_close(res["16-mixed"][1], res["fp32"][1], rtol=5e-3, atol=5e-4)
    cos = torch.nn.functional.cosine_similarity(res["16-mixed"][2], res["fp32"][2], dim=0).item()
    assert cos > 0.97
    assert O._STORE16 is None and O._CONV_OPERANDS == "fp32"  # context managers restored the defaults


def test_every_environment_switch_is_documented():
    """README.md's switch table is the interface of the A/B switches: every MIMO_* variable the library, the host mirror or
    bench.py reads is listed there, and nothing is listed that no code reads."""
    import glob
    import re
    code = set()
    for f in glob.glob(os.path.join(ROOT, "mimo_unet_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "mimo_unet_amd", "csrc", "*.h")):
        code |= set(re.findall(r'getenv\("(MIMO_[A-Z0-9_]+)"\)', open(f).read()))
    for f in glob.glob(os.path.join(ROOT, "mimo_unet_amd", "**", "*.py"), recursive=True) + [os.path.join(ROOT, "bench.py")]:
        code |= set(re.findall(r'environ[^\n]*?"(MIMO_[A-Z0-9_]+)"', open(f).read()))
    doc = set(re.findall(r"`(MIMO_[A-Z0-9_]+)`", open(os.path.join(ROOT, "README.md")).read()))
    test_only = {"MIMO_PARITY_LOG"}  # read by tests/helpers.py only
    assert code - doc == set(), sorted(code - doc)
    assert doc - code - test_only == set(), sorted(doc - code - test_only)
