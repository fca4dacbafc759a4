"""bench.py as the benchmark driver calls it (GPU): a plain run prints only the headline line (no roofline / CPU-baseline passes),
--steps sets the number of timed steps, and --dump-outputs writes what the last timed step computed, the same in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(outdir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(outdir)] + list(extra), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_reproducible_outputs(gpu_lib, tmp_path):
    a = _bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["value"] > 0 and a["dtype"] == "bf16"
    assert abs(a["value"] - 8 * 1e3 / a["ms_per_step"]) <= 1e-2 * a["value"] + 0.1
    assert "roofline" not in a and "cpu_baseline" not in a and "kernels" not in a
    names = sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".npy"))
    assert {"loss.npy", "topk_hits.npy", "loss_per_sample.npy", "params.npy", "grads.npy"} <= set(names), names
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    for f in names:
        x = np.load(tmp_path / "a" / f)
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all(), f
    assert np.load(tmp_path / "a" / "loss_per_sample.npy").shape == (8,)
    # the same arguments: the same inputs, and (the step is bit-reproducible) the same outputs
    _bench(tmp_path / "b")
    for f in names:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
