"""The depth task's callbacks under the reference's import path (mimo/tasks/depth/callbacks.py:12-144):
`OutputMonitor` is the one-kernel image logger of `mimo.monitor` (its defaults are the depth task's), and
`WandbMetricsDefiner` declares the summary of the validation metrics to wandb — nothing when `wandb` is absent."""
from mimo.monitor import OutputMonitor  # noqa: F401
from mimo_unet_amd.lightning_compat import Callback

try:
    import wandb
except ImportError:
    wandb = None


class WandbMetricsDefiner(Callback):
    SUMMARIES = {"metric_val/r2": "max", "metric_val/mae": "min", "metric_val/mse": "min"}

    def on_fit_start(self, trainer, pl_module) -> None:
        if wandb is None:
            return
        for name, summary in self.SUMMARIES.items():
            wandb.define_metric(name, summary=summary)
