"""The subnetwork permutations drawn inside the engine (`mimo_draw_permutations`, MIMO_ENGINE_PERM / `engine_perm`): the
kernel against its numpy restatement (tests/perm_reference.py) bit for bit at the sizes where a padded bitonic sort, the
`j mod batch` tiling and the k boundary can go wrong; the structure of apply_input_transform (the reference's
mimo/models/utils.py:27-36) independently of the restatement; the generator protocol; and a training step that draws its
own permutations against the same step handed those permutations."""
import os

import numpy as np
import pytest
import torch

from oracle import mimo_oracle as O
from tests import perm_reference as R

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x9E3779B97F4A7C15, (3 << 32) | 0xFFFFFFF8  # both halves of both words in use

# (batch, reps, k, S): the issue's list with k = int(batch * reps * (1 - irp)), then k = 1 and a non-power-of-two M just
# above one wave (as one batch, and as 13 x 5 with the boundary inside a repetition)
CASES = [(b, r, R.head_count(b, r, irp), s) for b, r, irp, s in
         [(1, 1, 0.0, 1), (2, 1, 0.0, 2), (4, 1, 0.0, 2), (5, 3, 0.5, 3), (4, 2, 1.0, 2), (7, 1, 0.9, 2), (8, 1, 0.2, 4),
          (64, 1, 0.0, 2), (33, 2, 0.3, 2), (4096, 1, 0.0, 2)]] + [(5, 1, 1, 3), (65, 1, 65, 2), (13, 5, 40, 64)]
assert CASES[4] == (4, 2, 0, 2) and CASES[5] == (7, 1, 0, 2) and CASES[3] == (5, 3, 7, 3)  # the two k = 0 cases are k = 0


def _draw(batch, reps, k, s, seed=SEED, offset=OFFSET):
    from mimo_unet_amd.engine import draw_permutations
    perm, main = draw_permutations(batch, reps, k, s, seed, offset, torch.device("cuda"), want_main=True)
    return perm.cpu().numpy(), main.cpu().numpy()


@pytest.fixture(scope="module")
def drawn():
    """Every case once: (kernel perm, kernel main, reference perm, reference main)."""
    return {c: _draw(*c) + R.draw_permutations(*c, SEED, OFFSET) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b{}-r{}-k{}-S{}".format(*c))
def test_kernel_equals_the_restatement(case, drawn):
    perm, main, rperm, rmain = drawn[case]
    assert perm.dtype == np.int64 and perm.shape == (case[3], case[0] * case[1])
    assert np.array_equal(main, rmain)
    assert np.array_equal(perm, rperm)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b{}-r{}-k{}-S{}".format(*c))
def test_structure_of_the_input_transform(case, drawn):
    """Without the restatement: `main` is a permutation of the batch tiled `reps` times, every row re-orders the first k
    entries of `main` and shares its tail."""
    batch, reps, k, _ = case
    perm, main = drawn[case][:2]
    assert np.array_equal(np.sort(main[:batch]), np.arange(batch))
    assert np.array_equal(main, np.tile(main[:batch], reps))
    for row in perm:
        assert np.array_equal(np.sort(row[:k]), np.sort(main[:k]))
        assert np.array_equal(row[k:], main[k:])
    if k >= 16:  # 16! orders: equal rows, or an unshuffled head, would be a bug, not a coincidence
        assert not np.array_equal(perm[0, :k], main[:k])
        assert len({row[:k].tobytes() for row in perm}) == len(perm)


@pytest.mark.parametrize("batch,reps,s", [(4097, 1, 2), (17, 241, 2), (4, 1, 65)])
def test_sizes_beyond_one_workgroup_are_refused_and_write_nothing(batch, reps, s):
    from mimo_unet_amd import _lib as L
    from mimo_unet_amd.engine import draw_permutations
    with pytest.raises(L.MimoHipError):
        draw_permutations(batch, reps, batch * reps, s, 1, 0, torch.device("cuda"))
    lib = L.load()
    m = batch * reps
    perm = torch.full((s, m), -7, device="cuda", dtype=torch.int64)
    main = torch.full((m,), -7, device="cuda", dtype=torch.int64)
    rc = lib.mimo_draw_permutations(perm.data_ptr(), main.data_ptr(), batch, reps, m, s, 1, 0, L.current_stream())
    torch.cuda.synchronize()
    assert rc != 0 and lib.mimo_last_error()
    assert bool((perm == -7).all()) and bool((main == -7).all())
    assert lib.mimo_draw_permutations(perm.data_ptr(), None, 4, 1, 5, 1, 1, 0, L.current_stream()) != 0  # k > M


def _offset():
    return torch.cuda.default_generators[torch.cuda.current_device()].get_offset()


def test_generator_protocol():
    from mimo_unet_amd.models.utils import draw_subnetwork_permutations
    torch.manual_seed(31)
    cpu_state, start = torch.get_rng_state(), _offset()
    a = draw_subnetwork_permutations(16, 3, 0.25, 2, device="cuda", engine=True)
    assert _offset() == start + 4
    b = draw_subnetwork_permutations(16, 3, 0.25, 2, device="cuda", engine=True)
    assert _offset() == start + 8 and not torch.equal(a, b)
    assert torch.equal(cpu_state, torch.get_rng_state())  # no CPU randperm behind the draw
    torch.manual_seed(31)
    assert torch.equal(a, draw_subnetwork_permutations(16, 3, 0.25, 2, device="cuda", engine=True))
    # and it is the entry point's draw for the generator's (seed, offset)
    ref, _ = R.draw_permutations(16, 2, R.head_count(16, 2, 0.25), 3, 31, start)
    assert np.array_equal(a.cpu().numpy(), ref)
    from mimo_unet_amd._lib import MimoHipError
    with pytest.raises(MimoHipError):
        draw_subnetwork_permutations(4097, 2, device="cuda", engine=True)
    assert _offset() == start + 4  # a refused size consumes nothing


CFG = O.NetConfig(in_channels=2, out_channels=2, num_subnetworks=2, filter_base_count=4)


def _model(state, *, reps=1, irp=0.0, encoder_dropout=0.0):
    from mimo.models.mimo_unet import MimoUnetModel
    m = MimoUnetModel(in_channels=2, out_channels=2, num_subnetworks=2, filter_base_count=4, center_dropout_rate=0.0,
                      final_dropout_rate=0.0, encoder_dropout_rate=encoder_dropout, core_dropout_rate=0.0,
                      decoder_dropout_rate=0.0, loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3, seed=0,
                      loss_buffer_size=10, loss_buffer_temperature=0.3, input_repetition_probability=irp,
                      batch_repetitions=reps)
    m.load_state_dict({"model." + k: v for k, v in state.items()})
    return m.cuda().train()


def _batches(steps):
    g = torch.Generator().manual_seed(53)
    return [{"image": torch.rand(4, 2, 32, 32, generator=g).cuda(), "label": torch.rand(4, 1, 32, 32, generator=g).cuda()}
            for _ in range(steps)]


def _steps(model, batches, perms=None):
    """One Adam step per batch; `perms`: handed to training_step_with_perms, else training_step draws.  Returns per step
    (loss, logged values, generator offset after the step) and the parameters after the last step."""
    opt = model.configure_optimizers()["optimizer"]
    trace = []
    for i, b in enumerate(batches):
        opt.zero_grad()
        out = (model.training_step(b, i) if perms is None else
               model.training_step_with_perms(b["image"], b["label"], None, perms[i]))
        out["loss"].backward()
        opt.step()
        trace.append((out["loss"].detach().clone(), {k: torch.as_tensor(v).clone() for k, v in model.logged.items()}, _offset()))
    torch.cuda.synchronize()
    assert model.model.numerics_status() == 0
    return trace, model.model.flat_parameters().clone()


def _same_run(a, b):
    assert len(a[0]) == len(b[0])
    for i, ((la, ga, _), (lb, gb, _)) in enumerate(zip(a[0], b[0])):
        assert torch.equal(la, lb), f"loss of step {i}: {la.item()} != {lb.item()}"
        assert ga.keys() == gb.keys() and len(ga) >= 9
        for k in ga:
            assert torch.equal(ga[k], gb[k]), f"logged {k} of step {i}"
    assert torch.equal(a[1], b[1]), "parameters after the last Adam step"


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "train-graph"])
@pytest.mark.parametrize("reps,irp", [(1, 0.0), (2, 0.5)])
def test_step_that_draws_equals_step_given_the_draw(reps, irp, graph, monkeypatch):
    """training_step with engine_perm against training_step_with_perms on the permutations the same generator state
    gives: loss, logged values and parameters after Adam, bit for bit; with MIMO_TRAIN_GRAPH=1 (read per plan) the
    drawing model's second and later calls replay the captured step, which stages perm into the plan's own buffer."""
    from mimo_unet_amd.models.utils import draw_subnetwork_permutations
    steps = 4 if graph else 3
    state, batches = O.init_state(CFG, 17), _batches(steps)
    torch.manual_seed(71)
    start = _offset()
    perms = [draw_subnetwork_permutations(4, 2, irp, reps, device="cuda", engine=True) for _ in range(steps)]
    assert perms[0].shape == (2, 4 * reps) and not torch.equal(perms[0], perms[1])
    model_b = _model(state, reps=reps, irp=irp)
    given = _steps(model_b, batches, perms)
    if graph:
        monkeypatch.setenv("MIMO_TRAIN_GRAPH", "1")
    model_a = _model(state, reps=reps, irp=irp)
    model_a.engine_perm = True
    torch.manual_seed(71)
    drawing = _steps(model_a, batches)
    assert [t[2] for t in drawing[0]] == [start + 4 * (i + 1) for i in range(steps)]
    _same_run(drawing, given)


def test_dropout_and_permutations_take_one_counter_block_each():
    """Encoder Dropout2d drawn in the engine as well: per step the permutations take the block at the generator's offset,
    the dropout multipliers the next one; one seed gives one run."""
    state, batches = O.init_state(CFG, 17), _batches(2)
    runs = []
    for _ in range(2):
        model = _model(state, encoder_dropout=0.3)
        model.engine_perm = True
        assert model.model.engine_rng
        torch.manual_seed(5)
        start = _offset()
        runs.append(_steps(model, batches))
        assert [t[2] for t in runs[-1][0]] == [start + 8, start + 16]
    _same_run(runs[0], runs[1])


def test_default_is_the_torch_route():
    from mimo_unet_amd.models.utils import draw_subnetwork_permutations
    model = _model(O.init_state(CFG, 17))
    if "MIMO_ENGINE_PERM" not in os.environ:
        assert model.engine_perm is False
    model.engine_perm = False  # (a no-op unless the suite itself runs under the switch)
    batch = _batches(1)[0]
    torch.manual_seed(9)
    start = _offset()
    want = draw_subnetwork_permutations(4, 2, 0.0, 1, device="cuda")
    torch_route, cpu_state = _offset() - start, torch.get_rng_state()
    torch.manual_seed(9)
    start = _offset()
    out = model.training_step(batch, 0)
    assert _offset() - start == torch_route and torch.equal(cpu_state, torch.get_rng_state())
    # and those permutations are what the step used: the same step, given them
    other = _model(O.init_state(CFG, 17))
    assert torch.equal(out["loss"], other.training_step_with_perms(batch["image"], batch["label"], None, want)["loss"])
