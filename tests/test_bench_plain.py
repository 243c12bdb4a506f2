"""bench.py without --full: one result line carrying the headline fields and none of what --full adds, exactly --steps
timed steps, and --dump-outputs writing the last timed step's loss and grid gradients (float32, under 64 MB)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_step_outputs(tmp_path):
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["unit"] == "point-samples/s" and rec["higher_is_better"]
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    n_points = rec["config"]["points_per_gpu"]
    assert abs(rec["value"] * rec["ms_per_step"] * 1e-3 - n_points) <= 1e-6 * n_points
    assert not set(rec) & {"roofline", "kernels_us", "extras", "cpu_baseline", "without_settle_phase"}

    names = sorted(os.listdir(dump))
    assert names == ["grad_level0.npy", "grad_level1.npy", "grad_level2_sample.npy", "loss.npy"], names
    assert sum(os.path.getsize(dump / n) for n in names) <= 64 << 20
    arrays = {n[:-4]: np.load(dump / n) for n in names}
    for name, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert arrays["loss"].shape == (2,) and arrays["loss"][0] > 0
    assert arrays["grad_level0"].shape == (1, 8, 32, 32, 32) and arrays["grad_level1"].shape == (1, 8, 64, 64, 64)
    for name in ("grad_level0", "grad_level1", "grad_level2_sample"):
        assert np.abs(arrays[name]).max() > 0, name
