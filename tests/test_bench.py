"""bench.py end to end at its own shape: a plain run prints the headline line and nothing that takes runs of its own
(`roofline`, `cpu_baseline`: those come with --full)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_line_only():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(16 * 1e3 / out["ms_per_step"], rel=1e-9)   # batch 16 per step, one GPU
    assert out["config"]["final_loss"] > 0
    assert "roofline" not in out and "cpu_baseline" not in out
