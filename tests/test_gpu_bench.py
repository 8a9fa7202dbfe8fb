"""-m gpu: bench.py's plain run on a small configuration — the headline line only, `--steps` timed steps, and
`--dump-outputs` writing what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "7", "--warmup", "4", "--batch", "512", "--max-vocab", "20000",
           "--data-batches", "3", "--no-tunable", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 7 and out["warmup"] == 4 and out["n_gpus"] == 1 and out["unit"] == "examples/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["ms_per_step"] > 0
    assert abs(out["value"] - 512 * 1e3 / out["ms_per_step"]) <= 5e-3 * out["value"]
    for extra in ("kernels", "roofline", "models", "optimizer_state_sweep", "cpu_baseline", "host_fed", "box"):
        assert extra not in out, extra                                 # (--full only)
    names = os.listdir(out_dir)
    assert "loss.npy" in names and any(n.endswith("embedding_weights.npy") for n in names) and len(names) > 10
    assert sum(os.path.getsize(out_dir / n) for n in names) < 64 << 20
    loss = np.load(out_dir / "loss.npy")
    assert loss.dtype == np.float64 and abs(float(loss[0]) - out["final_loss"]) <= 1e-6
    for n in names:
        a = np.load(out_dir / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
