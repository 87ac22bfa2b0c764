"""Whole training steps at the benchmark's own batches against a float64 reference on the device.

bench.py times a cfg3 step at batch 32 (per-GPU shards 16 / 8 / 4), cfg2 at 64 and cfg4 at 16.  The grid-stride kernels
are capped in workgroups, so how many pixels each thread sums in fp32, and how many partial rows the column sums walk,
grow with the batch: the BatchNorm statistics, BN + ReLU (+ pool), up-sampling + concat, the head and loss, the
BatchNorm-backward passes and FlatAdam are checked here at those batches.  Each case builds the benchmark's model
(bench.make_model after torch.manual_seed(1)) and batch (CUDA generator seeded 100, torch.rand image and label, rank 0's
rows of the global batch) and compares one step with oracle.mimo_oracle.train_step run on the GPU in float64 (the truth)
and in float32 (the yardstick: what fp32 arithmetic itself does), tests/helpers.py::reference_train_step.  The Adam
update is teacher-forced: fp64 Adam applied to the HIP's own gradients, which separates the kernel from gradient noise."""
import math

import pytest
import torch

import bench
from oracle import mimo_oracle as O
from tests.helpers import check_grads_vs_fp64, is_prebn_bias, reference_train_step, report
from tests.test_configs_gpu import BF16_GRAD_COS, BF16_TRAIN_OUT

pytestmark = pytest.mark.gpu
TOL = 1e-3  # outputs, losses and BatchNorm buffers (max |a - b| / max |b|), as in test_network_gpu.py::_oracle_vs_hip
ULP = 2.0 ** -23  # fp32 spacing relative to a value (an upper bound of one unit in the last place)


def _cfg(name):
    c = bench.CONFIGS[name]
    return c, O.NetConfig(c["Ci"], c["Co"], c["S"], c["f"])


def _bench_model(name, precision):
    c, _ = _cfg(name)
    torch.manual_seed(1)
    model = bench.make_model(c).cuda()
    model.model.set_precision(precision)
    model.train()
    return model, model.configure_optimizers()["optimizer"]


def _bench_batch(name, n, seed=7):
    """bench.py's strong-scaling batch: the global batch from a CUDA generator seeded 100, rank 0's first `n` rows; the
    subnetwork permutations from a seeded CPU generator"""
    c, _ = _cfg(name)
    g = torch.Generator(device="cuda").manual_seed(100)
    image = torch.rand(c["batch"], c["Ci"], c["H"], c["W"], device="cuda", generator=g)
    label = torch.rand(c["batch"], 1, c["H"], c["W"], device="cuda", generator=g)
    perms = O.draw_perms(n, c["S"], generator=torch.Generator().manual_seed(seed))
    return image[:n].contiguous(), label[:n].contiguous(), perms.cuda()


def _ref_state(model, cfg):
    """the oracle's TrainState holding the model's current parameters, BatchNorm buffers and loss-buffer ring"""
    st = {k[len("model."):]: v.detach().clone() for k, v in model.state_dict().items()}
    lb = model.loss_buffer
    ts = O.TrainState(cfg=cfg, st=st, loss_buffer=O.LossBuffer(cfg.num_subnetworks, lb.temperature, lb.buffer_size))
    ts.loss_buffer.buffer = lb.buffer.detach().clone().cuda()
    ts.loss_buffer.index = lb.index
    return ts


def _err(a, b):
    b = b.double()
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# Adam's hyper-parameters as the kernels receive them (float arguments of mimo_adam_step / _amp): the reference below runs
# in float64 on THESE values.  1 - beta2 in fp32 is 0.00099998713, 1.3e-5 away from 0.001: 27 times the 4-unit bound on v
# against a reference with the decimal 0.999.  torch's own fused fp32 Adam keeps its betas in fp32 the same way.
_F32 = lambda x: float(torch.tensor(x, dtype=torch.float32))


def _adam_ref(p0, g, m0, v0, step, lr):
    pd, md, vd, gd = p0.double(), m0.double(), v0.double(), g.double()
    O.adam_update(pd, gd, md, vd, step, _F32(lr), beta1=_F32(0.9), beta2=_F32(0.999), eps=_F32(1e-8))
    return pd, md, vd


def _adam_check(p0, g, m0, v0, p, m, v, step, lr, label, ref=None):
    """An Adam update of flat buffers (p0, m0, v0 -> p, m, v, fp32) against torch.optim.Adam's rule in float64 on the same
    gradient g (_adam_ref).  The kernel evaluates m, v and the update m / (sqrt(v) / sqrt(bc2) + eps) * lr / bc1 in fp32
    from exact inputs: a few roundings of each, so m and v within 4 units of their own terms' scale, and p within 4 units
    of p plus 1e-5 of lr (the update is at most ~lr; its relative error a few units, far below 1e-5)."""
    pd, md, vd = ref if ref is not None else _adam_ref(p0, g, m0, v0, step, lr)
    b1, b2 = _F32(0.9), _F32(0.999)
    gd = g.double()
    bp = 4 * ULP * pd.abs() + lr * 1e-5
    bm = 4 * ULP * (b1 * m0.double().abs() + (1 - b1) * gd.abs()) + 1e-38
    bv = 4 * ULP * (b2 * v0.double() + (1 - b2) * gd * gd) + 1e-38
    out = {}
    for q, got, r_, bnd in (("p", p, pd, bp), ("m", m, md, bm), ("v", v, vd, bv)):
        r = (got.double() - r_).abs() / bnd
        i = int(r.argmax())
        out[q] = (float(r.flatten()[i]), i)
    report(*label, f"Adam t={step} over {p0.numel()} elements ({p0.numel() % 4} in the tail loop): worst |error| / bound "
           + ", ".join(f"{q} {e:.2f} at {i}" for q, (e, i) in out.items()))
    bad = {q: v for q, v in out.items() if not v[0] <= 1.0}
    assert not bad, bad
    return out


def _adam_tail_check(model, p0, g, m0, v0, step, lr, label, amp_scale=None):
    """FlatAdam's buffer is padded per tensor to whole float4 (cfg3: 15 063 580 elements for 15 063 514 parameters), so the
    network's own step never runs the kernel's tail loop.  Here mimo_adam_step runs on copies of the first n elements, n
    just below the network's parameter count with n % 4 = 3 and non-zero gradients on the last three (not padding), so
    those go through the tail loop; same reference and bounds.  amp_scale: the same through mimo_adam_step_amp (the
    gradients scaled by amp_scale and unscaled by the kernel, the step counter on the device, found_inf = 0)."""
    from mimo_unet_amd.engine import adam_step, adam_step_amp
    n = sum(t.numel() for t in model.parameters()) // 4 * 4 - 1
    nz = (g[: n + 1] != 0).cpu()
    while not bool(nz[n - 3:n].all()):
        n -= 4
    p, m, v = p0[:n].clone(), m0[:n].clone(), v0[:n].clone()
    if amp_scale is None:
        adam_step(p, g[:n].clone(), m, v, lr=lr, step=step)
        what = "mimo_adam_step"
    else:
        step_dev = torch.full((1,), float(step - 1), device=p.device)
        adam_step_amp(p, g[:n] * amp_scale, m, v, lr=lr, step_dev=step_dev, amp_scale=torch.full((1,), float(amp_scale),
                      device=p.device), found_inf=torch.zeros(1, device=p.device))
        assert float(step_dev) == step
        what = "mimo_adam_step_amp"
    ref = tuple(t[:n] for t in _adam_ref(p0, g, m0, v0, step, lr))
    _adam_check(p0[:n], g[:n], m0[:n], v0[:n], p, m, v, step, lr, label + (f"{what}, unpadded length",), ref=ref)
    tail = slice(n - n % 4, n)
    assert bool((p[tail] != p0[tail]).all()), "the tail elements were not updated"


def _step_and_compare(model, opt, cfg, image, label, perms, label_str, *, amp_scale=None, grad_rule=True,
                      ref_operands=None, bounds=None):
    """One training step of the HIP model on (image, label, perms) against the fp64 and fp32 references started from the
    model's own state; then opt.step() checked by _adam_check.  amp_scale: backward on amp_scale * loss and the step through
    mimo_adam_step_amp (grad_scale = amp_scale, found_inf = 0, the device step counter).  ref_operands: run the references
    under O.conv_operands(kind) (the bf16-operand oracle), bounds: that mode's {"out", "loss", "buf", "cos"}.  Returns the
    HIP results and the references for callers that compare more."""
    N, S, half = image.shape[0], cfg.num_subnetworks, cfg.out_channels // 2
    ts = _ref_state(model, cfg)
    refs = {}
    for dt in (torch.float64, torch.float32):
        if ref_operands is None:
            refs[dt] = reference_train_step(ts, image, label, None, perms, device="cuda", dtype=dt, apply_optimizer=False)
        else:
            with O.conv_operands(ref_operands):
                refs[dt] = reference_train_step(ts, image, label, None, perms, device="cuda", dtype=dt, apply_optimizer=False)
    (ts64, r64), (ts32, r32) = refs[torch.float64], refs[torch.float32]
    opt.zero_grad()
    out = model.training_step_with_perms(image, label, None, perms)
    (out["loss"] if amp_scale is None else out["loss"] * amp_scale).backward()
    net = model.model
    p0, g = net.flat_parameters().detach().clone(), net.flat_gradients().detach().clone()
    if amp_scale is not None:
        g = g / amp_scale  # (exact: a power of two)
    m0 = opt._m.clone() if opt._m is not None else torch.zeros_like(p0)
    v0 = opt._v.clone() if opt._v is not None else torch.zeros_like(p0)
    # forward: predictions, log-scales, per-subnetwork losses (the ring row this step wrote) and the total
    preds = out["preds"].view(N, S, half, *image.shape[2:])
    log_scale = torch.log(out["aleatoric_std_map"].view(N, S, half, *image.shape[2:]).double() / math.sqrt(2.0))
    lb = model.loss_buffer
    loss_row = lb.buffer[(lb.index - 1) % lb.buffer_size]
    errs, yard = {}, {}
    for q, got, k, sl in (("preds", preds, "out", slice(0, half)), ("log_scale", log_scale, "out", slice(half, None)),
                          ("subnet_losses", loss_row, "loss", None), ("total", out["loss"].detach(), "total", None)):
        r, r_32 = (r64[k], r32[k]) if sl is None else (r64[k][:, :, sl], r32[k][:, :, sl])
        errs[q], yard[q] = _err(got, r), _err(r_32, r)
    # BatchNorm running statistics after the step, per layer
    sd = model.state_dict()
    bn = {k: (_err(sd["model." + k], v), _err(ts32.st[k], v)) for k, v in ts64.st.items() if "running" in k}
    wbn = max(bn, key=lambda k: bn[k][0])
    b = bounds or {"out": TOL, "loss": TOL, "buf": TOL}
    report(*label_str, "vs fp64 (fp32 yardstick): " + ", ".join(f"{q} {errs[q]:.2e} ({yard[q]:.2e})" for q in errs)
           + f"; BN buffers worst {wbn} {bn[wbn][0]:.2e} ({bn[wbn][1]:.2e})")
    assert errs["preds"] < b["out"] and errs["log_scale"] < b["out"], errs
    assert errs["subnet_losses"] < b["loss"] and errs["total"] < b["loss"], errs
    assert bn[wbn][0] < b["buf"], (wbn, bn[wbn])
    # gradients
    grads = {k[len("model."):]: p.grad.detach() for k, p in model.named_parameters()}
    if amp_scale is not None:
        grads = {k: v / amp_scale for k, v in grads.items()}
    if grad_rule:
        try:
            gc = check_grads_vs_fp64(grads, r32["grads"], r64["grads"])
        except AssertionError as e:
            report(*label_str, "gradient rule failed:", e)
            raise
        gtxt = (f"grads: cos {gc['cos']:.7f} rel-L2 {gc['rel_l2']:.2e}, worst tensor {gc['worst'][0]} {gc['worst'][1]:.2e} "
                f"(fp32 reference {gc['worst'][2]:.2e}, over all tensors {gc['eo_all']:.2e}; {gc['need_all']} of "
                f"{gc['n_tensors']} needed the whole-gradient arm)")
    else:
        dot = n1 = n2 = 0.0
        for k, r in r64["grads"].items():
            if is_prebn_bias(k):
                continue
            a = grads[k].double()
            dot, n1, n2 = dot + float((a * r).sum()), n1 + float((a * a).sum()), n2 + float((r * r).sum())
        gc = {"cos": dot / (n1 * n2) ** 0.5}
        gtxt = f"grads: cosine {gc['cos']:.5f} vs the {ref_operands}-operand reference"
    report(*label_str, gtxt)
    if grad_rule:
        assert gc["cos"] > 0.9999 and gc["rel_l2"] < 2e-2, gc
    else:
        assert gc["cos"] > b["cos"], gc
    # the optimiser, teacher-forced on the HIP's gradients
    if amp_scale is None:
        opt.step()
        t = opt.step_count
    else:
        opt.grad_scale = torch.full((1,), float(amp_scale), device="cuda")
        opt.found_inf = torch.zeros(1, device="cuda")
        opt.step()
        del opt.grad_scale, opt.found_inf
        t = opt.step_count  # (the device counter)
    lr = float(opt.param_groups[0]["lr"])
    _adam_check(p0, g, m0, v0, net.flat_parameters(), opt._m, opt._v, t, lr, label_str)
    _adam_tail_check(model, p0, g, m0, v0, t, lr, label_str, amp_scale)
    return {"model_sd": {k: v.detach().clone() for k, v in sd.items()}, "r64": r64, "ts64": ts64, "r32": r32, "errs": errs,
            "gc": gc}


def _free(*label):
    """report the device memory peak since the last call (the fp64 reference dominates it), release the cache"""
    torch.cuda.synchronize()
    report(*label, f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.empty_cache()


CASES = [  # (config, per-GPU batch, precision, MIMO_WGRAD_NP)
    ("cfg3", 32, "split16", None),
    ("cfg3", 32, "split16", "3"),
    ("cfg3", 32, "fp32", None),
    ("cfg3", 8, "split16", None),
    ("cfg2", 64, "split16", None),
    ("cfg4", 16, "split16", None),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-N{c[1]}-{c[2]}" + (f"-np{c[3]}" if c[3] else ""))
def test_training_step_at_a_benchmark_batch_vs_fp64(case, monkeypatch):
    name, n, precision, np_env = case
    if np_env is None:
        monkeypatch.delenv("MIMO_WGRAD_NP", raising=False)
    else:
        monkeypatch.setenv("MIMO_WGRAD_NP", np_env)  # read when the plan is built (the first step)
    _, cfg = _cfg(name)
    model, opt = _bench_model(name, precision)
    image, label, perms = _bench_batch(name, n)
    _step_and_compare(model, opt, cfg, image, label, perms, (name, f"N={n}", precision, f"np={np_env or 2}"))
    del model, opt
    _free(name, f"N={n}", precision)


def test_cfg4_bf16_training_step_at_its_batch_vs_the_bf16_operand_reference():
    """cfg4 at 16 in bf16 (its bench arithmetic) against the oracle that rounds the convolution operands the same way
    (O.conv_operands("bf16"), as test_configs_gpu.py::test_cfg4_geometry_bf16_vs_oracle), with that test's bounds: the
    training-mode outputs (BF16_TRAIN_OUT), the gradient's direction (BF16_GRAD_COS) and the losses (2e-2, its bound on the
    total loss of the same mode, there against the fp32 oracle, which sits further from this arithmetic than the
    bf16-operand reference here).  The BatchNorm buffers are statistics of the same training-mode outputs: their bound.
    Adam teacher-forced as in every case."""
    _, cfg = _cfg("cfg4")
    model, opt = _bench_model("cfg4", "bf16")
    image, label, perms = _bench_batch("cfg4", 16)
    _step_and_compare(model, opt, cfg, image, label, perms, ("cfg4", "N=16", "bf16"), grad_rule=False, ref_operands="bf16",
                      bounds={"out": BF16_TRAIN_OUT, "loss": 2e-2, "buf": BF16_TRAIN_OUT, "cos": BF16_GRAD_COS})
    del model, opt
    _free("cfg4", "N=16", "bf16")


@pytest.mark.parametrize("amp", [False, True], ids=["flat_adam", "adam_amp"])
def test_three_teacher_forced_steps_cfg3_at_32(amp, monkeypatch):
    """Three steps at cfg3's batch, each against fp64 started from the HIP's state after the previous one (parameters,
    BatchNorm buffers, the loss-buffer ring): non-uniform subnetwork weights from step 2 on, Adam's bias corrections at
    t = 2 and 3 on the moments the kernel itself wrote, running statistics accumulating.  amp: the same through
    mimo_adam_step_amp (loss scaled by 2^10, gradients unscaled by the kernel, the step counter on the device), then one
    more step with found_inf = 1, which must leave parameters and both moments bit-unchanged and not count."""
    monkeypatch.delenv("MIMO_WGRAD_NP", raising=False)
    _, cfg = _cfg("cfg3")
    model, opt = _bench_model("cfg3", "split16")
    image, label, _ = _bench_batch("cfg3", 32)
    weights = []
    for k in range(3):
        perms = O.draw_perms(32, cfg.num_subnetworks, generator=torch.Generator().manual_seed(7 + k))
        res = _step_and_compare(model, opt, cfg, image, label, perms.cuda(), ("cfg3", "N=32", "split16", f"step {k + 1}",
                                "amp" if amp else "flat"), amp_scale=1024.0 if amp else None)
        weights.append(res["r64"]["weights"])
        del res
        _free("cfg3", "N=32", f"step {k + 1}")
    assert opt.step_count == 3
    report("cfg3", "N=32", "amp" if amp else "flat", "subnetwork weights of steps 1-3:", [w.tolist() for w in weights])
    assert not bool((weights[2] == weights[2][0]).all()), weights  # the ring's losses made them non-uniform
    if amp:
        opt.zero_grad()
        out = model.training_step_with_perms(image, label, None, perms.cuda())
        (out["loss"] * 1024.0).backward()
        net = model.model
        before = [t.detach().clone() for t in (net.flat_parameters(), opt._m, opt._v)]
        opt.grad_scale = torch.full((1,), 1024.0, device="cuda")
        opt.found_inf = torch.ones(1, device="cuda")
        opt.step()
        del opt.grad_scale, opt.found_inf
        after = (net.flat_parameters(), opt._m, opt._v)
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "a step with found_inf = 1 changed the state"
        assert opt.step_count == 3
    del model, opt
    _free("cfg3", "N=32", "found_inf step")


def _prebn_std(model, cfg, image, perms):
    """per-channel std of every pre-BatchNorm convolution output in an fp64 training-mode forward with the conv biases
    set to zero (the biases cannot change anything downstream of a training-mode BatchNorm): {conv prefix: [C]}"""
    st = {k[len("model."):]: v.detach().double().clone() for k, v in model.state_dict().items()
          if v.is_floating_point()}
    for k in st:
        if is_prebn_bias(k):
            st[k].zero_()
    sig, orig = {}, O.conv_bn_relu

    def rec(x, st_, conv, bn, training):
        z = O.conv3x3_reflect(x, st_[conv + ".weight"], None)
        sig[conv] = z.std(dim=(0, 2, 3), unbiased=False)
        return orig(x, st_, conv, bn, training)

    O.conv_bn_relu = rec
    try:
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
            O.mimo_unet_forward(cfg, st, O.apply_perms(image.double(), perms), training=True)
    finally:
        O.conv_bn_relu = orig
    return sig


@pytest.mark.parametrize("shift,k", [(s, k) for s in ("bias", "image") for k in (10, 100)])
def test_batchnorm_with_large_channel_means_cfg3_at_32(shift, k, monkeypatch):
    """Training-mode BatchNorm removes a per-channel shift of its input exactly, so shifting changes nothing but the
    running means — and exposes statistics that cancel (a variance taken as E[z^2] - E[z]^2 loses k^2 of its precision
    when a channel's mean is k times its spread).  "bias": every pre-BatchNorm convolution bias set to k * sigma_c (sigma_c:
    the channel's std in a bias-free fp64 forward); "image": k * std(image) added to the image (reflect padding keeps it
    constant; the first BatchNorm removes it).

    At k, against fp64: predictions, log-scales, losses and running variances within the k = 0 bounds (TOL); the running
    means within the k = 0 bound of their k = 0 scale plus 16 fp32 units of the shifted value.  These are the checks the
    statistics themselves decide.  The gradients follow the whole-network rule with torch's fp32 reference on the SAME
    shifted inputs as the yardstick, not the k = 0 one: a shifted convolution output is an fp32 value of about k sigma,
    whose rounding (k * 2^-24 of sigma) moves the normalised values and flips ReLU decisions near zero in every fp32
    implementation.  torch's fp32 step shows it: its worst gradient tensor is 6.5e-3 from fp64 at k = 0 and 2.2e-2 at
    k = 100; the HIP step's is 6.1e-2 / 7.1e-2 (bias / image), inside 1e-3 + 5 x 2.2e-2, while its predictions stay within
    6.7e-4 / 9.4e-4 and its running variances within 1e-5 of fp64.  The k = 0 fp32 yardstick is reported next to it."""
    monkeypatch.delenv("MIMO_WGRAD_NP", raising=False)
    _, cfg = _cfg("cfg3")
    image0, label, perms = _bench_batch("cfg3", 32)
    model, opt = _bench_model("cfg3", "split16")
    res0 = _step_and_compare(model, opt, cfg, image0, label, perms, ("cfg3", "N=32", "split16", f"{shift} shift k=0"))
    g32_0 = res0["r32"]["grads"]
    base = {q: float(v.abs().max()) for q, v in res0["ts64"].st.items() if q.endswith("running_mean")}
    del model, opt, res0
    _free("cfg3", "N=32", f"{shift} shift k=0")
    model, opt = _bench_model("cfg3", "split16")
    image = image0
    if shift == "bias":
        sig = _prebn_std(model, cfg, image0, perms)
        sd = model.state_dict()
        for conv, s in sig.items():
            sd["model." + conv + ".bias"].copy_((k * s).float())
        model.load_state_dict(sd)
    else:
        image = image0 + k * float(image0.std())
    label_k = ("cfg3", "N=32", "split16", f"{shift} shift k={k:g}")
    res = _step_and_compare(model, opt, cfg, image, label, perms, label_k)
    g64 = res["r64"]["grads"]
    e0 = {q: float((g32_0[q].double() - r).norm() / r.norm()) for q, r in g64.items() if not is_prebn_bias(q)}
    w0 = max(e0, key=e0.get)
    report(*label_k, f"k = 0 fp32 yardstick against this fp64 step: worst tensor {w0} {e0[w0]:.2e}")
    worst = ("", 0.0)
    for q, ref in res["ts64"].st.items():
        if not q.endswith("running_mean"):
            continue
        e = float((res["model_sd"]["model." + q].double() - ref).abs().max())
        bound = TOL * base[q] + 16 * 2.0 ** -24 * float(ref.abs().max())
        if e / bound > worst[1]:
            worst = (q, e / bound)
    report(*label_k, f"running_mean worst |error| / bound {worst[1]:.3f} ({worst[0]})")
    assert worst[1] <= 1.0, worst
    del model, opt, res
    _free(*label_k)
