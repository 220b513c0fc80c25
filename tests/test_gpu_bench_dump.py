"""A plain bench.py run (no --full) on the GPU: it times exactly --steps steps once, skips the CPU
baseline, and --dump-outputs writes the closed loop's last-step outputs — the arrays a caller of
batched.ClosedLoop reads back after the same warm-up and timed steps, bit for bit (same seeded
workload, Philox noise keyed by the global instance id, every instance solved on its own)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARMUP, STEPS = 256, 2, 4   # one launch each; 256 instances = 256 wavefronts of the lean loop


def test_plain_run_times_steps_once_and_dumps_last_step(tmp_path):
    from drone_attitude_control_amd.batched import ClosedLoop

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "force",
                          "--batch", str(B), "--steps", str(STEPS), "--warmup", str(WARMUP),
                          "--dump-outputs", str(tmp_path / "dump")],
                         cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["dtype"] == "f64"
    assert line["timing"]["regions"] == 1 and len(line["timing"]["region_ms"]) == 1
    assert line["closed_loop"]["instance_steps"] == B * (WARMUP + STEPS)
    assert line["cpu_baseline"] is None
    assert line["ms_per_step"] > 0
    assert math.isclose(line["value"], B / (line["ms_per_step"] * 1e-3), rel_tol=1e-9)

    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == ["instance.npy", "instance_stats.npy", "state.npy"]
    got = {f[:-4]: np.load(tmp_path / "dump" / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["instance"], np.arange(B))

    loop = ClosedLoop("force", B, seed=42)
    loop.run(WARMUP)
    loop.run(STEPS)
    assert got["state"].shape == (B, 4) and np.array_equal(got["state"], loop.state())
    assert got["instance_stats"].shape == (B, 4) and np.array_equal(got["instance_stats"], loop.instance_stats())
    assert np.all(got["instance_stats"][:, 3] == WARMUP + STEPS)
