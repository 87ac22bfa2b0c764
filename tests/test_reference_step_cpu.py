"""CPU pin of the device reference of a training step (tests/helpers.py::reference_train_step), which the benchmark-batch
tests run on the GPU in float64 and float32: run on the CPU it must reproduce O.train_step — the oracle the golden vectors
pin — step after step, including the optimiser and the loss buffer.  No GPU needed."""
import pytest
import torch

from oracle import mimo_oracle as O
from tests.helpers import cfg_from_meta, load_npz, reference_train_step, rel_err, state_from


def _fixture_state(fx, dtype):
    cfg = cfg_from_meta(fx["meta"])
    st = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state_from(fx, "init/").items()}
    return O.TrainState(cfg=cfg, st=st, loss_kind=str(fx["loss_kind"]), lr=float(fx["lr"]), weight_decay=float(fx["wd"]),
                        loss_buffer=O.LossBuffer(cfg.num_subnetworks, float(fx["temperature"]), 10))


def _close(a, b, what):
    if a.dtype == torch.int64:
        assert torch.equal(a, b), what
    else:
        assert rel_err(a, b) < 1e-12, (what, rel_err(a, b))


@pytest.mark.parametrize("name", ["cfg1_step.npz", "mini_s2_step.npz", "mini_gauss_step.npz"])
def test_reference_train_step_reproduces_the_oracle_on_the_cpu(name):
    """Every step of the fixture in float64: the helper (which works on a moved copy of the state and hands the stepped
    copy back) against O.train_step stepping its own state in place — outputs, per-subnetwork losses, weights, total,
    input and parameter gradients, then parameters, BatchNorm buffers, Adam moments and the loss-buffer ring — within
    1e-12 of each tensor's scale."""
    fx = load_npz(name)
    dt = torch.float64
    ts_o, ts_h = _fixture_state(fx, dt), _fixture_state(fx, dt)
    ts_o.loss_buffer.buffer = ts_o.loss_buffer.buffer.to(dt)  # (the helper keeps the ring in the reference's dtype too)
    for it in range(int(fx["meta"][8])):
        t = lambda k: torch.from_numpy(fx[k]) if k in fx else None
        batch = (t(f"s{it}/image"), t(f"s{it}/label"), t(f"s{it}/mask"), t(f"s{it}/perms"))
        r_o = O.train_step(ts_o, *(None if b is None else b.to(dt) if b.is_floating_point() else b for b in batch),
                           want_input_grad=(it == 0))
        ts_h, r_h = reference_train_step(ts_h, *batch, device="cpu", dtype=dt, want_input_grad=(it == 0))
        for k in ("out", "loss", "weights", "total") + (("dx",) if it == 0 else ()):
            assert r_h[k].dtype == dt, k
            _close(r_h[k], r_o[k], (it, k))
        for k, g in r_o["grads"].items():
            _close(r_h["grads"][k], g, (it, "grad", k))
        assert ts_h.step == ts_o.step == it + 1
        for k, v in ts_o.st.items():
            _close(ts_h.st[k], v, (it, k))
        for k in ts_o.exp_avg:
            _close(ts_h.exp_avg[k], ts_o.exp_avg[k], (it, "exp_avg", k))
            _close(ts_h.exp_avg_sq[k], ts_o.exp_avg_sq[k], (it, "exp_avg_sq", k))
        _close(ts_h.loss_buffer.buffer, ts_o.loss_buffer.buffer, (it, "loss buffer"))
        assert ts_h.loss_buffer.index == ts_o.loss_buffer.index


def test_reference_train_step_leaves_its_input_state_alone_and_keeps_fixed_weights():
    """The helper steps a copy: the caller's state (parameters, BatchNorm buffers, counters, ring) is unchanged, and a
    get_weights replaced on the caller's loss buffer (the fixed weights of the parity tests) is honoured, cast to the
    reference's dtype.  The float32 run on the CPU is O.train_step in float32, bit for bit."""
    fx = load_npz("mini_s2_step.npz")
    ts = _fixture_state(fx, torch.float32)
    lb_w = torch.tensor([0.7, 1.3])
    ts.loss_buffer.get_weights = lambda: lb_w
    snap = {k: v.clone() for k, v in ts.st.items()}
    batch = [torch.from_numpy(fx[k]) for k in ("s0/image", "s0/label", "s0/mask", "s0/perms")]
    ts64, r64 = reference_train_step(ts, *batch, device="cpu", dtype=torch.float64)
    assert all(torch.equal(snap[k], v) for k, v in ts.st.items()) and ts.step == 0 and ts.exp_avg == {}
    assert ts.loss_buffer.index == 0 and not bool(ts.loss_buffer.buffer.any())
    assert r64["weights"].dtype == torch.float64 and torch.equal(r64["weights"], lb_w.double())
    nbt = [k for k in ts.st if k.endswith("num_batches_tracked")]
    assert ts64.step == 1 and all(int(ts64.st[k]) == int(ts.st[k]) + 1 for k in nbt)
    ts32, r32 = reference_train_step(ts, *batch, device="cpu", dtype=torch.float32)
    ref = _fixture_state(fx, torch.float32)
    ref.loss_buffer.get_weights = lambda: lb_w
    r_o = O.train_step(ref, *batch)
    assert torch.equal(r32["out"], r_o["out"]) and torch.equal(r32["total"], r_o["total"])
    assert all(torch.equal(r32["grads"][k], g) for k, g in r_o["grads"].items())
    assert all(torch.equal(ts32.st[k], v) for k, v in ref.st.items())
