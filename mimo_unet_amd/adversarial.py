"""FGSM robustness sweep of an `EnsembleModule`, on the GPU: the first half of the reference's
``scripts/test/test_nyuv2_depth.py`` (``fgsm_attack`` :16-24, ``make_predictions`` :26-90, driven per noise level at
:190-205).

The reference, per noise level, runs the ensemble under autograd, back-propagates the NLL through every member to the
image, forms ``clamp(image + eps * sign(grad), 0, 1)`` and predicts again.  In eval mode the gradient is taken at the clean
image and does not depend on eps, so here ONE gradient serves the whole sweep:

* per member one eval-mode forward with its graph kept, the loss, and `mimo_input_gradient` — the data-gradient chain
  only (no weight gradient, no reduction, no `.grad` write), accumulated over the members into one image gradient;
* one `mimo_fgsm_perturb` launch that reads image and gradient once and writes the perturbed image of every eps;
* the ordinary no-grad ensemble forward per eps.

    sweep = fgsm_sweep(ensemble, image, label, (0.0, 0.02, 0.04))     # {eps: (mean, aleatoric_var, epistemic_var)}

    rob = RobustnessEvaluator()                                        # the two tables per noise level
    for batch in loader:
        rob.update_from(ensemble, batch["image"].cuda(), batch["label"].cuda())
    rob.write_csv(result_dir, "nyuv2")

A bare `EvidentialUnetModel` is accepted wherever an ensemble is (the reference's scripts/test/test_nyuv2_depth_evidential.py
and test_ndvi_evidential.py drive the model itself, :42-65): `EvidentialUnetModel.image_gradient` — the eval-mode forward, the
logit gradient of `loss_fn(out, labels).mean()` in one kernel, `mimo_input_gradient` with that `dout` — then the same one
`mimo_fgsm_perturb` launch and `predict_uncertainties` per eps.

MC-dropout ensembles (`monte_carlo_steps = M > 0`, the reference's ``--monte_carlo_steps``) are opt-in: without
`mc_dropout=True` they are refused as before — the reference draws fresh dropout masks in each of its forwards, so a sweep has
no bit parity to be held to.  The gradient GIVEN the masks is deterministic, and that is what `mc_dropout=True` computes:

* the loss of the reference's script is the mean NLL over the concatenated axis of all M * S_total outputs, each pass with
  its own mask draw; the gradient here is

      d/d image of (1 / (M * S_total)) * sum_member sum_m sum_s loss_{m,s}

  taken ONCE at the clean image, with one draw of M mask sets per member, and it serves every eps of the sweep.  The
  reference redraws per eps; the draw does not depend on eps, so each eps's result has the same distribution either way;
* per member the M passes are stacked on the batch axis, pass-major as in `EnsembleModule.forward`, in chunks of
  `ensemble.max_samples_per_launch // B` passes: one masked eval-mode forward, the loss, and `mimo_input_gradient_mc`, whose
  first-layer fold sums the chunk's passes in a fixed order (no atomics: two calls with the same masks give the same bits).
  A chunk of k passes gets dloss[s] = k / (M * S_total) — the engine's per-subnetwork loss is already the mean over the
  chunk's k * B samples.  The first chunk of member 0 assigns, every other chunk accumulates;
* the masks come from the engine's generator (keyed by torch's CUDA generator: `torch.cuda.manual_seed` replays a
  gradient), or from `mask_override` / `elem_mask_override` with rows for all M * B samples, sliced per chunk;
* the perturbed predictions per eps are the ordinary MC forward of the ensemble, with fresh masks;
* BatchNorm uses its running statistics throughout.

Still refused: an `EvidentialUnetModel` with active dropout (the reference's evidential scripts have no MC mode), and the
precisions other than fp32 / split16.

`pgd_sweep` is the iterated, projected form of the same attack (PGD; BIM without its random start), which the reference does
not have: per step one `image_gradient` call on the perturbation levels stacked on the batch axis and one `mimo_pgd_step`
launch for all of them (csrc/pgd.hip), an optional random start from the engine's generator (`mimo_pgd_init`), then the same
predictions.  `RobustnessEvaluator(attack="pgd")` routes through it; the defaults run `fgsm_sweep` as before.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from .evaluation import UncertaintyEvaluator, write_tables_csv

DEFAULT_EPSILONS = (0.0, 0.02, 0.04)  # test_nyuv2_depth.py:192


def _is_evidential(model) -> bool:
    from .models.evidential_unet import EvidentialUnetModel
    return isinstance(model, EvidentialUnetModel)


def _validate_epsilons(epsilons: Sequence[float]) -> Tuple[float, ...]:
    eps = tuple(float(e) for e in epsilons)
    if not eps:
        raise ValueError("fgsm_sweep: no epsilons")
    if any(not e >= 0.0 for e in eps):
        raise NotImplementedError(f"fgsm_sweep: negative (or NaN) epsilons are not supported: {eps}")
    if len(set(eps)) != len(eps):
        raise ValueError(f"fgsm_sweep: duplicate epsilons {eps}")
    return eps


def _validate(ensemble, epsilons: Sequence[float], mc_dropout: bool = False) -> Tuple[float, ...]:
    """Everything that can be refused is refused here, before anything touches the GPU."""
    if _is_evidential(ensemble):  # the model itself, not an ensemble of it
        ensemble.require_eval("fgsm_sweep")
        ensemble.model._require_gradient_precision("fgsm_sweep: the input gradient is")
        return _validate_epsilons(epsilons)
    if getattr(ensemble, "monte_carlo_steps", 0) > 0 and not mc_dropout:
        raise NotImplementedError("fgsm_sweep: MC-dropout ensembles (monte_carlo_steps > 0) are not supported: the reference "
                                  "draws fresh dropout masks in each of its forwards, there is nothing to be in parity with")
    from .models.mimo_unet import MimoUnetModel
    models = list(getattr(ensemble, "models", []))
    if not models:
        raise ValueError("fgsm_sweep: the ensemble has no members")
    for m in models:
        if not isinstance(m, MimoUnetModel):
            raise NotImplementedError(f"fgsm_sweep: members must be MimoUnetModel (Laplace / Gaussian NLL heads), not "
                                      f"{type(m).__name__}: an evidential model is not supported as a member, pass the "
                                      f"EvidentialUnetModel itself")
    return _validate_epsilons(epsilons)


def _mc_chunk_weights(passes: int, batch: int, max_samples_per_launch: int, s_total: int):
    """[(m0, m1, weight)]: the passes [m0, m1) of each launch — chunks of `max_samples_per_launch // batch` passes, as
    `EnsembleModule.forward` forms them — and the dloss entry of the chunk, (m1 - m0) / (passes * s_total): the engine's
    per-subnetwork loss is the mean over the chunk's (m1 - m0) * batch samples, the wanted one the mean over passes * batch.
    The weights of a subnetwork sum to 1 / s_total over the chunks."""
    chunk = max(1, min(passes, max_samples_per_launch // max(batch, 1)))
    return [(m0, min(passes, m0 + chunk), (min(passes, m0 + chunk) - m0) / (passes * s_total)) for m0 in range(0, passes, chunk)]


def image_gradient(ensemble, image: torch.Tensor, label: torch.Tensor, mask: Optional[torch.Tensor] = None,
                   mc_dropout: bool = False) -> torch.Tensor:
    """d loss / d image [B,C,H,W] of `loss_fn(y_pred, log_param, labels)` as the reference's script forms it
    (test_nyuv2_depth.py:44-55): the mean NLL over the concatenated subnetwork axis of ALL members, i.e. a weight of
    1 / S_total on every subnetwork's mean loss.  Members are summed in list order (member 0 assigns, the others add).
    A bare `EvidentialUnetModel`: the gradient of `loss_fn(out, labels).mean()` (`EvidentialUnetModel.image_gradient`).
    mc_dropout=True with an ensemble of `monte_carlo_steps = M > 0`: the mean over the M * S_total outputs of M masked passes
    per member (module docstring); with M = 0 the flag changes nothing."""
    _validate(ensemble, (0.0,), mc_dropout)
    if _is_evidential(ensemble):
        return ensemble.image_gradient(image, label, mask)[0]
    if not image.is_cuda:
        from . import _lib as L
        raise L.MimoHipError("fgsm_sweep runs on an AMD GPU through libmimo_hip.so; move the ensemble and its inputs to cuda")
    s_total = ensemble.num_subnetworks
    image = image.detach().contiguous().float()
    label = label.detach().to(image.device)
    mask = None if mask is None else mask.detach().to(image.device)
    dimage = torch.empty_like(image)
    passes = getattr(ensemble, "monte_carlo_steps", 0) if mc_dropout else 0
    with torch.no_grad():
        if passes > 0:
            _mc_image_gradient(ensemble, image, label, mask, dimage, passes, s_total)
            return dimage
        for i, model in enumerate(ensemble.models):
            dloss = torch.full((model.num_subnetworks,), 1.0 / s_total, device=image.device, dtype=torch.float32)
            model.model.image_gradient(image, label, mask, dloss, dimage, accumulate=i > 0)
    return dimage


def _mc_image_gradient(ensemble, image, label, mask, dimage, passes: int, s_total: int) -> None:
    b = image.shape[0]
    chunks = _mc_chunk_weights(passes, b, ensemble.max_samples_per_launch, s_total)
    first = True
    for model in ensemble.models:
        net = model.model
        # tests: recorded masks for all passes x B samples, sliced per launch as EnsembleModule.forward slices them
        recorded, recorded_elem = net.mask_override, net.elem_mask_override
        try:
            for m0, m1, weight in chunks:
                if recorded is not None:
                    net.mask_override = {j: t[m0 * b: m1 * b] for j, t in recorded.items()}
                if recorded_elem is not None:
                    net.elem_mask_override = {k: t[m0 * b: m1 * b] for k, t in recorded_elem.items()}
                dloss = torch.full((model.num_subnetworks,), weight, device=image.device, dtype=torch.float32)
                net.image_gradient(image, label, mask, dloss, dimage, accumulate=not first, passes=m1 - m0, mc_dropout=True)
                first = False
        finally:
            net.mask_override, net.elem_mask_override = recorded, recorded_elem


def fgsm_sweep(ensemble, image: torch.Tensor, label: torch.Tensor, epsilons: Sequence[float] = DEFAULT_EPSILONS,
               mask: Optional[torch.Tensor] = None, clip: Optional[Tuple[float, float]] = (0.0, 1.0),
               return_perturbed: bool = False, mc_dropout: bool = False) -> Dict[float, tuple]:
    """{eps: (mean, aleatoric_var, epistemic_var)} [B,Ct,H,W] on the device, for the image attacked with each eps
    (eps = 0 is the clamped clean image, as in the reference).  `ensemble`: an `EnsembleModule` or a bare `EvidentialUnetModel`.  image [B,C,H,W], label [B,Ct,H,W], mask [B,1,H,W] or None
    (weights the loss the gradient is taken of).  clip: the range the perturbed image is clamped to; None = no clamp.
    return_perturbed: the tuples get the perturbed image [B,C,H,W] as a fourth entry.
    mc_dropout: accept an MC-dropout ensemble (`monte_carlo_steps > 0`): one gradient over its masked passes at the clean
    image, then the ordinary MC forward per eps with fresh masks (module docstring).
    The members' `.grad`, BatchNorm buffers and train / eval flags are left as they were."""
    eps = _validate(ensemble, epsilons, mc_dropout)
    from .engine import fgsm_perturb
    dimage = image_gradient(ensemble, image, label, mask, mc_dropout=mc_dropout)
    lo, hi = (float("-inf"), float("inf")) if clip is None else (float(clip[0]), float(clip[1]))
    perturbed = fgsm_perturb(image.detach(), dimage, eps, lo, hi)
    return _predict_levels(ensemble, [(e, perturbed[k]) for k, e in enumerate(eps)], return_perturbed)


def _predict_levels(ensemble, levels, return_perturbed: bool) -> Dict[float, tuple]:
    """The tail of a sweep: levels = [(eps, perturbed image)] -> {eps: (mean, aleatoric_var, epistemic_var[, perturbed])}"""
    if _is_evidential(ensemble):
        out = {}
        for e, x in levels:
            res = ensemble.predict_uncertainties(x)
            out[e] = res + (x,) if return_perturbed else res
        return out
    keep, raw = ensemble.keep_on_device, ensemble.return_raw_predictions
    ensemble.keep_on_device, ensemble.return_raw_predictions = True, False
    out = {}
    try:
        for e, x in levels:
            res = tuple(ensemble(x))
            out[e] = res + (x,) if return_perturbed else res
    finally:
        ensemble.keep_on_device, ensemble.return_raw_predictions = keep, raw
    return out


def _validate_pgd(steps, step_size, rel_step_size) -> Tuple[int, Optional[float], float]:
    if isinstance(steps, bool) or int(steps) != steps or steps < 1:
        raise ValueError(f"pgd_sweep: steps must be an integer >= 1, got {steps!r}")
    if step_size is not None and not float(step_size) >= 0.0:
        raise ValueError(f"pgd_sweep: step_size must be None or a non-negative number, got {step_size!r}")
    if not float(rel_step_size) > 0.0:
        raise ValueError(f"pgd_sweep: rel_step_size must be positive, got {rel_step_size!r}")
    return int(steps), None if step_size is None else float(step_size), float(rel_step_size)


def pgd_step_sizes(eps: Sequence[float], steps: int, step_size: Optional[float], rel_step_size: float) -> Tuple[float, ...]:
    """alpha_k: `step_size` for every level if it is given, else rel_step_size * eps_k / steps in Python floats (cast to fp32
    once, where the launch takes them)."""
    return tuple(float(step_size) if step_size is not None else rel_step_size * e / steps for e in eps)


def pgd_level_chunks(levels: int, batch: int, limit: int, mc_dropout: bool = False):
    """[(k0, k1)]: the eps > 0 levels [k0, k1) of each gradient launch — max(1, limit // batch) levels stacked on the batch
    axis, one level with mc_dropout=True (the passes already fill the launch)."""
    chunk = 1 if mc_dropout else max(1, int(limit) // max(int(batch), 1))
    return [(k0, min(levels, k0 + chunk)) for k0 in range(0, levels, chunk)]


def _samples_per_launch(ensemble) -> int:
    if _is_evidential(ensemble):  # the bare model has no such attribute: EnsembleModule's default
        return max(1, int(os.environ.get("MIMO_MC_CHUNK_SAMPLES", "64")))
    return int(ensemble.max_samples_per_launch)


def _clamp_compare(x: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """clamp in the kernels' compare form (a NaN and the sign of a zero pass), once per sweep"""
    if lo == float("-inf") and hi == float("inf"):
        return x
    return torch.where(x < lo, torch.full_like(x, lo), torch.where(x > hi, torch.full_like(x, hi), x))


def pgd_sweep(ensemble, image: torch.Tensor, label: torch.Tensor, epsilons: Sequence[float] = DEFAULT_EPSILONS, steps: int = 10,
              step_size: Optional[float] = None, rel_step_size: float = 2.5, random_start: bool = False,
              mask: Optional[torch.Tensor] = None, clip: Optional[Tuple[float, float]] = (0.0, 1.0),
              return_perturbed: bool = False, mc_dropout: bool = False) -> Dict[float, tuple]:
    """`fgsm_sweep`'s dict for the iterated, projected sign-gradient attack (PGD; BIM with random_start=False): per level
    eps_k, `steps` times

        x_adv_k = clamp(clamp(x_adv_k + alpha_k * sign(d loss / d image at x_adv_k), image - eps_k, image + eps_k), *clip)

    Same model kinds, refusals and untouched members as `fgsm_sweep`; no reference counterpart (its only attack is FGSM).
    alpha_k: `step_size`, or rel_step_size * eps_k / steps.  Start: clamp(image, *clip); with random_start=True
    clamp(image + eps_k * r, *clip), r uniform in (-1, 1) from the engine's generator (`engine.pgd_init`: one draw shared by
    the levels, keyed by torch's CUDA generator of the image's device, whose offset advances by 4 — `torch.cuda.manual_seed`
    replays a sweep).
    Per step the levels with eps > 0 are stacked on the batch axis, in the order given, in chunks of
    max(1, limit // B) levels (limit = `ensemble.max_samples_per_launch`; for a bare evidential model its default,
    MIMO_MC_CHUNK_SAMPLES or 64): ONE `image_gradient` call per chunk on [Kc * B, C, H, W] — label and mask are repeated once
    per sweep — and one `mimo_pgd_step` launch per chunk.  The stacked loss is a mean over the Kc * B samples, so each level's
    gradient carries a factor 1 / Kc: a positive factor changes no sign, and only the sign is used.  With mc_dropout=True a
    chunk holds one level (the passes already fill the launch) and every step draws fresh masks from the engine's generator:
    the attack ascends an expectation over masks.  Levels with eps = 0 take no gradient: they stay at their start.
    Afterwards every level is predicted exactly as in `fgsm_sweep`."""
    eps = _validate(ensemble, epsilons, mc_dropout)
    steps, step_size, rel_step_size = _validate_pgd(steps, step_size, rel_step_size)
    if not image.is_cuda:
        from . import _lib as L
        raise L.MimoHipError("pgd_sweep runs on an AMD GPU through libmimo_hip.so; move the ensemble and its inputs to cuda")
    from .engine import pgd_init, pgd_step
    lo, hi = (float("-inf"), float("inf")) if clip is None else (float(clip[0]), float(clip[1]))
    x0 = image.detach().contiguous().float()
    b = x0.shape[0]
    # attacked levels first, in the order given, so that every chunk is one contiguous [Kc * B, C, H, W] block of x_adv
    order = [k for k, e in enumerate(eps) if e > 0.0] + [k for k, e in enumerate(eps) if e == 0.0]
    kp = sum(1 for e in eps if e > 0.0)
    eps_o = [eps[k] for k in order]
    alpha_o = pgd_step_sizes(eps_o, steps, step_size, rel_step_size)
    with torch.no_grad():
        if random_start:
            index = x0.device.index if x0.device.index is not None else torch.cuda.current_device()
            gen = torch.cuda.default_generators[index]
            seed, offset = gen.initial_seed(), gen.get_offset()
            x_adv = pgd_init(x0, eps_o, lo, hi, seed, offset)
            gen.set_offset(offset + 4)  # after the launch, one counter block, as `_engine_permutations` does
        else:
            x_adv = _clamp_compare(x0, lo, hi).unsqueeze(0).repeat(len(eps), *([1] * x0.dim()))
        chunks = pgd_level_chunks(kp, b, _samples_per_launch(ensemble), mc_dropout)
        if chunks:
            most = max(k1 - k0 for k0, k1 in chunks)
            label_r = label.detach().to(x0.device).repeat(most, *([1] * (label.dim() - 1)))
            mask_r = None if mask is None else mask.detach().to(x0.device).repeat(most, *([1] * (mask.dim() - 1)))
        for _ in range(steps):
            for k0, k1 in chunks:
                n = (k1 - k0) * b
                stacked = x_adv[k0:k1].view(n, *x0.shape[1:])
                grad = image_gradient(ensemble, stacked, label_r[:n], None if mask_r is None else mask_r[:n], mc_dropout=mc_dropout)
                pgd_step(x0, grad.view(k1 - k0, *x0.shape), x_adv[k0:k1], eps_o[k0:k1], alpha_o[k0:k1], lo, hi)
    perturbed = {eps[k]: x_adv[j] for j, k in enumerate(order)}
    return _predict_levels(ensemble, [(e, perturbed[e]) for e in eps], return_perturbed)


ATTACKS = ("fgsm", "pgd")


class RobustnessEvaluator:
    """One `UncertaintyEvaluator` per noise level, fed by `fgsm_sweep`: the sparsification and calibration tables of
    test_nyuv2_depth.py:215-234 for every eps of its sweep (:192).  `evaluator_kwargs` go to every UncertaintyEvaluator.
    mc_dropout: handed to `fgsm_sweep` (MC-dropout ensembles).
    attack="pgd": fed by `pgd_sweep(steps, step_size, rel_step_size, random_start)` instead; the default "fgsm" ignores the four."""

    def __init__(self, epsilons: Sequence[float] = DEFAULT_EPSILONS, mc_dropout: bool = False, attack: str = "fgsm",
                 steps: int = 10, step_size: Optional[float] = None, rel_step_size: float = 2.5, random_start: bool = False,
                 **evaluator_kwargs):
        self.epsilons = tuple(float(e) for e in epsilons)
        self.mc_dropout = bool(mc_dropout)
        if not self.epsilons or any(not e >= 0.0 for e in self.epsilons):
            raise NotImplementedError(f"RobustnessEvaluator: epsilons must be non-negative, got {self.epsilons}")
        if len(set(self.epsilons)) != len(self.epsilons):
            raise ValueError(f"RobustnessEvaluator: duplicate epsilons {self.epsilons}")
        if attack not in ATTACKS:
            raise ValueError(f"RobustnessEvaluator: unknown attack {attack!r}, one of {ATTACKS}")
        self.attack = attack
        self.steps, self.step_size, self.rel_step_size = ((steps, step_size, rel_step_size) if attack == "fgsm" else
                                                          _validate_pgd(steps, step_size, rel_step_size))
        self.random_start = bool(random_start)
        self.evaluators = {e: UncertaintyEvaluator(**evaluator_kwargs) for e in self.epsilons}

    def reset(self) -> None:
        for ev in self.evaluators.values():
            ev.reset()

    def update_from(self, ensemble, image, label, mask=None) -> None:
        if self.attack == "pgd":
            sweep = pgd_sweep(ensemble, image, label, self.epsilons, steps=self.steps, step_size=self.step_size,
                              rel_step_size=self.rel_step_size, random_start=self.random_start, mask=mask,
                              mc_dropout=self.mc_dropout)
        else:
            sweep = fgsm_sweep(ensemble, image, label, self.epsilons, mask=mask, mc_dropout=self.mc_dropout)
        for e, (mean, av, ev) in sweep.items():
            self.evaluators[e].update(mean, av, ev, label.to(mean.device), None if mask is None else mask.to(mean.device))

    def compute(self) -> Dict[float, dict]:
        return {e: ev.compute() for e, ev in self.evaluators.items()}

    def write_csv(self, directory: str, name: str, tables: Optional[Dict[float, dict]] = None):
        """`{name}_{eps}_precision_recall.csv` and `{name}_{eps}_calibration.csv` per noise level (test_nyuv2_depth.py:229,234;
        eps formatted as Python prints the float: 0.0, 0.02, 0.04)."""
        tables = self.compute() if tables is None else tables
        os.makedirs(directory, exist_ok=True)
        paths = {}
        for e in self.epsilons:
            tmp = os.path.join(directory, f".{name}_{e}")
            a, b = write_tables_csv(tables[e], tmp)
            pa, pb = (os.path.join(directory, f"{name}_{e}_{kind}.csv") for kind in ("precision_recall", "calibration"))
            os.replace(a, pa)
            os.replace(b, pb)
            os.rmdir(tmp)
            paths[e] = (pa, pb)
        return paths
