"""The dropout multipliers drawn inside the engine (MIMO_ENGINE_RNG, csrc/ew_dropout.hip) against their numpy restatement
(tests/dropout_reference.py) bit for bit: every site's mask as `Plan.dropout_mask` reads it back, and — without the read-back
kernel — whole forwards and backwards against the same call handed the restatement's masks through `mask_override` /
`elem_mask_override`.  Geometries are chosen for the tails (N C = 2 mod 4, C = 6 of pad8 = 8, C = 1), the grid-stride
wrap of both element-wise kernels, the low offset word wrapping between two steps, and an element with u == p exactly."""
import numpy as np
import pytest
import torch

from oracle import mimo_oracle as O
from tests import dropout_reference as D
from tests.test_network_gpu import build_model

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x9E3779B97F4A7C15, (3 << 32) | 0xFFFFFFF8  # both halves of both words in use; the low word wraps at the next step
RATES = dict(dropout2d=(0.1, 0.3, 0.5), center=0.2, final=0.05)  # one rate per group
# (S, f, N, H, W).  The first: Dropout2d counts N C = 18, 36, ... = 2 mod 4, element-wise C = 6 (second lane group half used),
# 3 x 4 center.  The second: the smallest center the engine builds, 2 x 2 at 32 x 32 (a one-pixel center, 16 x 16, is refused:
# test_a_one_pixel_center_is_refused).  The third: one subnetwork, five images.
GEOMETRIES = [(2, 6, 3, 50, 70), (3, 8, 1, 32, 32), (1, 8, 5, 32, 48)]


def _generator():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _set_generator(seed=SEED, offset=OFFSET):
    torch.manual_seed(seed)
    _generator().set_offset(offset)
    assert _generator().initial_seed() & (2 ** 64 - 1) == seed and _generator().get_offset() == offset


def _model(s, f, *, dropout2d=(0.0, 0.0, 0.0), center=0.0, final=0.0, precision="split16", ci=3):
    """The network tests' model.  Its constructor (like the reference's) refuses Dropout2d together with the element-wise
    sites; the engine takes both, so the element-wise rates are set behind it: on the modules that say which sites are
    active, and on the geometry the plans are built from."""
    from mimo_unet_amd.engine import NetGeometry
    cfg = O.NetConfig(ci, 2, s, f)
    model = build_model(cfg, O.init_state(cfg, 11), dropout=dropout2d, precision=precision)
    net = model.model
    net.core.center_dropout.p = center
    for d in net.decoder.final_dropouts:
        d.p = final
    net._geom = NetGeometry(**{**net._geom.__dict__, "center_dropout_rate": center, "final_dropout_rate": final})
    net._drop_plans()
    assert net.engine_rng
    return model


def _inputs(s, n, h, w, ci=3, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, s, ci, h, w, generator=g).cuda(), torch.rand(n, s, 1, h, w, generator=g).cuda()


def _plan(net):
    return list(net._plans.values())[-1]  # the plan used last (least recently used first)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_masks(plan, table, seed, offset):
    """Every active site of `table` as the plan reads it back == the restatement: keep pattern and kept value, bit for bit.
    (HIP's fp32 divide is correctly rounded and the build has no fast-math flag: the kept value is the definition's.)"""
    checked = 0
    for t in table:
        if t["p"] <= 0.0:
            continue
        got, want = plan.dropout_mask(t["site"]).cpu().numpy(), D.site_mask(t, seed, offset)
        assert got.shape == want.shape == t["shape"] and got.dtype == np.float32
        assert np.array_equal(got != 0, want != 0), f"keep pattern of site {t['site']} ({t['kind']})"
        assert np.array_equal(_bits(got), _bits(want)), f"kept value of site {t['site']} ({t['kind']})"
        checked += 1
    return checked


def _inject(net, table, seed, offset):
    """The restatement's masks of every active site through the recorded-mask arguments."""
    active = [t for t in table if t["p"] > 0.0]
    net.mask_override = {t["site"]: torch.from_numpy(D.site_mask(t, seed, offset)).cuda() for t in active if t["kind"] == "dropout2d"}
    net.elem_mask_override = {t["kind"]: torch.from_numpy(D.site_mask(t, seed, offset)).cuda() for t in active
                              if t["kind"] != "dropout2d"}


def _release(net):
    net.mask_override = net.elem_mask_override = None


# ------------------------------------------------------------------------------------------------ a. every site
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "S{}-f{}-N{}-{}x{}".format(*g))
def test_masks_equal_the_restatement_at_every_site(geom):
    s, f, n, h, w = geom
    table = D.sites(s, f, n, h, w, **RATES)
    model = _model(s, f, **RATES).train()
    x, _ = _inputs(s, n, h, w)
    _set_generator()
    with torch.no_grad():
        model.model(x)
    assert _generator().get_offset() == OFFSET + 4
    plan = _plan(model.model)
    assert plan.num_double_convs == D.num_double_convs(s) and plan.double_conv_channels == [t["shape"][1] for t in table[:3 * s + 6]]
    assert _check_masks(plan, table, SEED, OFFSET) == len(table) == 4 * s + 7
    # the next forward draws at the next offset: the low word has wrapped, the high word carried
    with torch.no_grad():
        model.model(x)
    assert _generator().get_offset() == OFFSET + 8 == (4 << 32) | 0
    assert _check_masks(plan, table, SEED, OFFSET + 4) == len(table)


def test_a_one_pixel_center_is_refused():
    """16 x 16 would give a 1 x 1 center; the reflect padding of its convolutions needs two pixels, and the plan says so."""
    from mimo_unet_amd._lib import MimoHipError
    model = _model(3, 8, **RATES).train()
    with pytest.raises(MimoHipError, match="too small"), torch.no_grad():
        model.model(_inputs(3, 1, 16, 16)[0])


# ------------------------------------------------------------------------------------------------ b. partial activation
def test_active_sites_keep_their_positional_number_and_inactive_ones_are_refused():
    from mimo_unet_amd._lib import MimoHipError
    s, f, n, h, w = GEOMETRIES[0]
    rates = dict(dropout2d=(0.3, 0.0, 0.2), center=0.0, final=0.05)
    table = D.sites(s, f, n, h, w, **rates)
    model = _model(s, f, **rates).train()
    _set_generator()
    with torch.no_grad():
        model.model(_inputs(s, n, h, w)[0])
    plan = _plan(model.model)
    active = [t["site"] for t in table if t["p"] > 0.0]
    assert active == [0, 1, 2, 3, 10, 11, 13, 14]  # encoders, decoders, final: the core (4..9) and the center (12) are off
    assert _check_masks(plan, table, SEED, OFFSET) == len(active)
    for t in table:
        if t["p"] <= 0.0:
            with pytest.raises(MimoHipError, match=r"status -3.*(had no mask|was not drawn by the engine) in the last forward"):
                plan.dropout_mask(t["site"])


# ------------------------------------------------------------------------------------------------ c. forward and backward
def _step(model, x, y):
    model.zero_grad()
    xg = x.clone().requires_grad_(True)
    p1, p2 = model(xg)
    loss = model.loss_fn.forward(p1, p2, y, reduce_mean=False).mean()
    (loss * 256.0).backward()  # (a power of two: keeps the fp16 gradients of "16-mixed" away from underflow)
    return p1.detach().clone(), p2.detach().clone(), xg.grad.clone(), model.model.flat_gradients().clone()


@pytest.mark.parametrize("precision", ["fp32", "split16", "bf16", "bf16-mixed", "16-mixed"])
def test_forward_and_backward_used_the_definition(precision):
    """A step that draws == the same step handed the restatement's masks: outputs, input gradient and flat gradient bit for
    bit.  The element-wise sites' forward and backward regenerate their multipliers in `elem_mask_mul_kernel<T>` (T = float,
    __bf16, _Float16 over the five modes); the read-back kernel is not involved."""
    s, f, n, h, w = GEOMETRIES[0]
    table = D.sites(s, f, n, h, w, **RATES)
    model = _model(s, f, precision=precision, **RATES).train()
    x, y = _inputs(s, n, h, w)
    _set_generator()
    drawn = _step(model, x, y)
    assert _generator().get_offset() == OFFSET + 4
    _inject(model.model, table, SEED, OFFSET)
    given = _step(model, x, y)
    assert _generator().get_offset() == OFFSET + 4  # nothing was drawn
    _release(model.model)
    assert all(bool(torch.isfinite(t).all()) for t in drawn) and float(drawn[2].abs().max()) > 0 and float(drawn[3].abs().max()) > 0
    for name, a, b in zip(("p1", "p2", "input gradient", "flat gradient"), drawn, given):
        assert torch.equal(a, b), f"{precision}: {name} differs in {int((a != b).sum())} of {a.numel()}"
    # and the masks matter: the masks of another offset give another step
    _inject(model.model, table, SEED, OFFSET + 4)
    other = _step(model, x, y)
    _release(model.model)
    assert not torch.equal(other[0], drawn[0]) and not torch.equal(other[3], drawn[3])


# ------------------------------------------------------------------------------------------------ d. grid-stride loops
def test_grid_stride_loops_of_both_element_wise_kernels():
    """N H W = 17 x 256 x 256 = 1 114 112 > 4096 x 256 threads: `elem_mask_mul_kernel` (one thread per pixel) and
    `elem_dropout_mask_kernel` (one per pixel and lane group, Cv = 2) both go round their loops.  f = 1: one channel of a
    padded eight, so seven lanes of every pixel's two counters are unused.  Forward only."""
    s, f, n, h, w = 1, 1, 17, 256, 256
    assert n * h * w > 4096 * 256
    table = D.sites(s, f, n, h, w, final=0.3)
    model = _model(s, f, final=0.3).train()
    x, _ = _inputs(s, n, h, w)
    _set_generator()
    with torch.no_grad():
        drawn = model.model(x).clone()
    assert _check_masks(_plan(model.model), table, SEED, OFFSET) == 1
    _inject(model.model, table, SEED, OFFSET)
    with torch.no_grad():
        given = model.model(x).clone()
    _release(model.model)
    assert bool(torch.isfinite(drawn).all()) and torch.equal(drawn, given)


# ------------------------------------------------------------------------------------------------ e. captured training graph
def test_graphed_training_steps_draw_fresh_masks(monkeypatch):
    """MIMO_TRAIN_GRAPH=1 (read per plan): the first step of a call shape runs eagerly, the second is captured and replayed,
    the later ones replay.  Each step's Dropout2d masks are the restatement's at its own offset — the draw stays in front of
    the graph — across the low offset word's wrap, and the generator advances by 4 per step."""
    monkeypatch.setenv("MIMO_TRAIN_GRAPH", "1")
    s, f, n, h, w = 2, 4, 4, 32, 32
    table = D.sites(s, f, n, h, w, dropout2d=RATES["dropout2d"])
    model = _model(s, f, dropout2d=RATES["dropout2d"], ci=2).train()
    opt = model.configure_optimizers()["optimizer"]
    g = torch.Generator().manual_seed(53)
    perms = torch.arange(n)[None].repeat(s, 1).cuda()
    _set_generator()
    masks = []
    for step in range(4):
        image, label = torch.rand(n, 2, h, w, generator=g).cuda(), torch.rand(n, 1, h, w, generator=g).cuda()
        opt.zero_grad()
        out = model.training_step_with_perms(image, label, None, perms)
        out["loss"].backward()
        opt.step()
        assert _generator().get_offset() == OFFSET + 4 * (step + 1)
        assert _check_masks(_plan(model.model), table, SEED, OFFSET + 4 * step) == 3 * s + 6, f"step {step}"
        masks.append(torch.cat([_plan(model.model).dropout_mask(t["site"]).flatten() for t in table if t["p"] > 0.0]))
        assert bool(torch.isfinite(out["loss"]))
    assert all(not torch.equal(masks[i], masks[j]) for i in range(4) for j in range(i))
    assert model.model.numerics_status() == 0


# ------------------------------------------------------------------------------------------------ f. MC-dropout inference
@pytest.mark.parametrize("kind", ["dropout2d", "elementwise"])
def test_mc_dropout_inference_route(kind):
    """`EnsembleModule.forward`: BatchNorm in eval mode, the dropout modules in training mode, torch.no_grad(), the passes
    stacked on the batch axis.  Three calls: with Dropout2d only, the first derives the packed weights eagerly, the second
    captures the eval graph, the third replays it (the element-wise sites stay off the graph)."""
    from mimo.models.ensemble import EnsembleModule
    s, f, b, h, w, passes = 2, 6, 2, 32, 48, 2
    rates = dict(dropout2d=RATES["dropout2d"]) if kind == "dropout2d" else dict(center=RATES["center"], final=RATES["final"])
    table = D.sites(s, f, passes * b, h, w, **rates)
    model = _model(s, f, **rates)
    ens = EnsembleModule([], monte_carlo_steps=passes, return_raw_predictions=True, models=[model], keep_on_device=True)
    assert not model.model._bn_training() and any(d.training and d.p > 0 for d in model.model._dropout_modules())
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(4)).cuda()
    _set_generator()
    drawn = []
    for call in range(3):
        drawn.append(tuple(t.clone() for t in ens(x)))
        assert _generator().get_offset() == OFFSET + 4 * (call + 1)
        assert _check_masks(_plan(model.model), table, SEED, OFFSET + 4 * call) == sum(t["p"] > 0 for t in table)
    assert not torch.equal(drawn[0][0], drawn[1][0]) and not torch.equal(drawn[1][0], drawn[2][0])
    for call in range(3):
        _inject(model.model, table, SEED, OFFSET + 4 * call)
        given = ens(x)
        _release(model.model)
        assert _generator().get_offset() == OFFSET + 12
        assert all(torch.equal(a, c) for a, c in zip(drawn[call], given)), f"call {call}"


# ------------------------------------------------------------------------------------------------ g. u == p
def test_an_element_with_u_equal_to_p_is_kept():
    """The committed constants of dropout_reference.py: at p = 0.5 the element's 24 bits are exactly 2^23, u == p, and
    `u >= p` keeps it."""
    g = D.BOUNDARY_GEOMETRY
    table = D.sites(g["s"], g["f"], g["n"], g["h"], g["w"], final=0.5)
    model = _model(g["s"], g["f"], final=0.5).train()
    _set_generator(D.BOUNDARY_SEED, D.BOUNDARY_OFFSET)
    with torch.no_grad():
        model.model(_inputs(g["s"], g["n"], g["h"], g["w"])[0])
    plan = _plan(model.model)
    assert float(plan.dropout_mask(D.BOUNDARY_SITE)[D.BOUNDARY_INDEX]) == 2.0
    assert _check_masks(plan, table, D.BOUNDARY_SEED, D.BOUNDARY_OFFSET) == g["s"]
