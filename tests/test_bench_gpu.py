"""bench.py's plain run: the timed pass and the line only (everything else behind --full), and --dump-outputs writing what
the last timed step returned, from the same inputs every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = {"loss", "preds", "aleatoric_std_map", "err_map", "label", "params"}


def _plain_run(dump_dir, steps=3, warmup=1, batch=4):
    env = {k: v for k, v in os.environ.items() if k not in ("MIMO_PARITY_LOG", "RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--batch", str(batch), "--dump-outputs", str(dump_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_run_times_the_headline_alone_and_dumps_its_last_step(tmp_path):
    lines = [_plain_run(tmp_path / d) for d in ("a", "b")]
    for line in lines:
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "images/s" and line["higher_is_better"] is True
        assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 4) < 0.01 * 4  # images/s x s/step = batch
        # nothing beyond the timed pass: no strict pass, no kernel-class pass, no enqueue probe, no CPU baseline
        assert line["value_strict"] is None and "roofline" not in line and "cpu_baseline" not in line
        assert line["config"]["host_enqueue_ms_per_step"] is None
    a, b = ({n: np.load(tmp_path / d / (n + ".npy")) for n in DUMPED} for d in ("a", "b"))
    assert set(os.listdir(tmp_path / "a")) == {n + ".npy" for n in DUMPED}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64e6
    assert all(v.dtype == np.float32 for v in a.values())
    # cfg3 at batch 4: [S * batch, 1, 256, 256] per-pixel maps; the loss is the line's final_loss
    assert a["preds"].shape == a["label"].shape == (8, 1, 256, 256) and a["params"].shape == (1 << 21,)  # params: a sample
    assert abs(float(a["loss"]) - lines[0]["config"]["final_loss"]) < 1e-4 * max(1.0, abs(float(a["loss"])))
    # same arguments, same inputs: the gathered labels (image, label and permutations are all seeded) are identical, and
    # the step computed from them agrees (Adam moves a parameter by at most lr = 1e-3 per step, 4 steps here)
    assert np.array_equal(a["label"], b["label"])
    assert rel_err(a["preds"], b["preds"]) < 1e-2 and rel_err(a["loss"], b["loss"]) < 1e-3
    assert float(np.abs(a["params"] - b["params"]).max()) <= 2 * 4 * 1e-3
