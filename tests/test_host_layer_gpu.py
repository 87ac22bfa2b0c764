"""The Python host layer of the engine on the device: a plan's autograd bookkeeping (`engine.Plan`), what survives a plan
that `MimoUNet` drops, and the tensors an eval-mode call outside autograd keeps alive.  Smallest geometry the engine
accepts: S=2, f=4, batch 2, 32x32."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CI, CO, S, F, N, H, W = 3, 2, 2, 4, 2, 32, 32


def _net():
    from mimo_unet_amd.models.mimo_components.model import MimoUNet
    torch.manual_seed(11)
    return MimoUNet(CI, CO, S, F).cuda()


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


# ------------------------------------------------------------------------------------------------ Plan bookkeeping
def test_plan_bookkeeping_fields_exist_from_construction_and_only_their_methods_change_them():
    from mimo_unet_amd.engine import NetGeometry, Plan
    plan = Plan(NetGeometry(CI, CO, S, F), N, H, W, torch.device("cuda", 0))
    assert plan.generation == 0 and plan.pending is None
    params, buffers = torch.zeros(plan.param_floats, device="cuda"), torch.zeros(plan.buffer_floats, device="cuda")
    out = torch.empty(N, S, CO, H, W, device="cuda")
    plan.bind(params, torch.zeros_like(params), buffers)
    plan.forward(_rand(N, S, CI, H, W), out, training=False)
    plan.status()
    assert plan.generation == 0 and plan.pending is None  # the engine calls leave them alone
    assert plan.begin_graph() == 1 and (plan.generation, plan.pending) == (1, 1)
    plan.note_eval_call()
    assert (plan.generation, plan.pending) == (2, 1)  # the generation only
    plan.release(2)
    assert (plan.generation, plan.pending) == (2, 1)  # not the generation that is pending: left alone
    plan.release(1)
    assert (plan.generation, plan.pending) == (2, None)
    assert plan.begin_graph() == 3 and (plan.generation, plan.pending) == (3, 3)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ status survives a drop
@pytest.mark.parametrize("how", ["set_loss", "to", "set_precision"])
def test_numerics_status_survives_every_way_a_plan_is_dropped(how):
    """A non-finite input makes a training forward record "BatchNorm batch statistic not finite" on its plan; every call
    that drops the plans hands the bit on to `numerics_status()`, which reports it once."""
    net = _net().train()
    x = _rand(N, S, CI, H, W)
    x[0, 0, 0, 5, 5] = float("nan")
    net(x)
    bits = net.numerics_status(clear=False)
    print(f"{how}: status word of the live plan {bits}")
    assert bits & 1 and len(net._plans) == 1
    {"set_loss": lambda: net.set_loss("gaussian_nll"), "to": lambda: net.to("cuda"),
     "set_precision": lambda: net.set_precision("fp32")}[how]()
    assert len(net._plans) == 0 and net._evicted_status == bits
    assert net.numerics_status() == bits and net.numerics_status() == 0 and net._evicted_status == 0


# ------------------------------------------------------------------------------------------------ _inference_keep
def _kept_pointers(obj, found=None):
    found = set() if found is None else found
    if isinstance(obj, torch.Tensor):
        found.add(obj.data_ptr())
    elif isinstance(obj, dict):
        _kept_pointers(list(obj.values()), found)
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            _kept_pointers(o, found)
    return found


def _injected_masks(net, rows):
    d2 = torch.ones(rows, F, device="cuda")  # Dropout2d multipliers of the first DoubleConv
    center = torch.ones(rows, 8 * F * S, H // 16, W // 16, device="cuda")
    net.mask_override, net.elem_mask_override = {0: d2}, {"center": center}
    return [d2, center]


def test_inference_keep_holds_what_the_plan_points_at_on_each_eval_mode_route():
    net = _net().eval()
    # the inference forward (eval mode under no_grad) with injected masks
    x = _rand(N, S, CI, H, W)
    handed = [x] + _injected_masks(net, N)
    with torch.no_grad():
        out = net(x)
    assert {t.data_ptr() for t in handed + [out]} <= _kept_pointers(net._inference_keep)
    # image_gradient, MC-dropout route with injected masks: masks, label, loss mask, dloss, logits
    image, label, lmask = _rand(N, CI, H, W, seed=1), _rand(N, 1, H, W, seed=2), torch.ones(N, 1, H, W, device="cuda")
    dloss, dimage = torch.full((S,), 0.5, device="cuda"), torch.empty(N, CI, H, W, device="cuda")
    handed = [image, label, lmask, dloss] + _injected_masks(net, N)
    out, _ = net.image_gradient(image, label, lmask, dloss, dimage, mc_dropout=True)
    assert {t.data_ptr() for t in handed + [out]} <= _kept_pointers(net._inference_keep)
    # ... and the plain route
    net.mask_override = net.elem_mask_override = None
    out, _ = net.image_gradient(image, label, lmask, dloss, dimage)
    assert {t.data_ptr() for t in (image, label, lmask, dloss, out)} <= _kept_pointers(net._inference_keep)
    # image_gradient_from_dout: image, logits and the dout the caller made from them
    made = []
    out = net.image_gradient_from_dout(image, lambda logits: made.append(torch.ones_like(logits)) or made[0], dimage)
    assert {t.data_ptr() for t in (image, out, made[0])} <= _kept_pointers(net._inference_keep)
    torch.cuda.synchronize()
    assert torch.isfinite(dimage).all() and net.numerics_status() == 0
