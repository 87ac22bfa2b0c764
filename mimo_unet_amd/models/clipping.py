"""Lightning's gradient-clipping hook for the two model classes.

Lightning clips before `optimizer.step()`, when the gradients of a fused optimiser under a loss scaler are still scaled (its
mixed-precision plugin refuses the combination); `FlatAdam` clips inside its step instead, so the hook only hands it the
bound."""
from ..optim import FlatAdam


class FlatAdamClipping:
    """`gradient_clip_val`: the bound used when the Trainer passes none (hand-written loops call the hook once with the
    optimiser, or set `max_grad_norm` / `clip_value` on the optimiser themselves).  `_flat_adam`: the `FlatAdam` that
    `configure_optimizers` built, for logging its norm; copies and pickles of the model leave it behind."""
    gradient_clip_val = None
    _flat_adam = None

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_flat_adam", None)
        return state

    def configure_gradient_clipping(self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None):
        opt = getattr(optimizer, "optimizer", optimizer)  # Lightning hands over a LightningOptimizer wrapper
        if gradient_clip_val is None:
            gradient_clip_val = self.gradient_clip_val
        if isinstance(opt, FlatAdam):
            algorithm = getattr(gradient_clip_algorithm, "value", gradient_clip_algorithm)  # str or Lightning's enum
            if algorithm not in (None, "norm", "value"):
                raise ValueError(f"gradient_clip_algorithm: 'norm' or 'value', got {gradient_clip_algorithm!r}")
            # Lightning calls the hook before every step, with None when the Trainer was given no bound: what the optimiser
            # was built with, or was given since, then stands.  An explicit 0 switches clipping off, as in Lightning.
            if gradient_clip_val is not None:
                bound = gradient_clip_val if gradient_clip_val != 0 else None
                opt.max_grad_norm, opt.clip_value = (None, bound) if algorithm == "value" else (bound, None)
                opt._clip_setting()
            return
        clip_gradients = getattr(super(), "clip_gradients", None)
        if clip_gradients is not None:
            clip_gradients(optimizer, gradient_clip_val=gradient_clip_val, gradient_clip_algorithm=gradient_clip_algorithm)

    def _log_grad_norm(self) -> None:
        """`grad_norm`: the norm before clipping of the last optimiser step clipped by norm (the step before this
        training_step), however the bound reached the optimiser; nothing before the first such step or without clipping by
        norm.  A copy made on the device, no host synchronisation: the value logged does not change when the next step
        overwrites the optimiser's own scalar."""
        opt = self._flat_adam
        if opt is not None and opt.max_grad_norm is not None and opt.last_grad_norm is not None:
            self._log("grad_norm", opt.last_grad_norm.clone())
