"""GPU: a plain `python bench.py` run (no --full) measures the headline alone.  It sets up, warms up, times the steps, writes
--dump-outputs and prints the line; the fields only --full measures (roofline, HBM kernel classes, other configs, CPU
baselines) stay null."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_alone(tmp_path):
    out = tmp_path / "dump"
    proc = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                           "--dump-outputs", str(out)], cwd=REPO, capture_output=True, text=True, timeout=900)
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert proc.returncode == 0 and len(lines) == 1, (proc.returncode, proc.stdout[-2000:], proc.stderr[-4000:])
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"] == "bf16"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["unit"] == "clips/s"
    assert d["config"]["launch_probe"] is not None           # the launch mode is still chosen by measurement
    assert d["roofline"] is None and d["hbm_kernels"] is None and d["other_configs"] is None and d["cpu_baseline"] is None
    cost = np.load(out / "cost.npy")
    assert cost.size == 1 and np.isfinite(cost).all()
    assert np.isfinite(np.load(out / "grad_sample.npy")).all()
