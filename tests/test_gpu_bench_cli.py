"""bench.py's command line on a small C2 call (256 sets, 3 timed steps): a plain run prints the headline figures only
and --dump-outputs writes the per-job results of the last timed step; --full adds the roofline, the isolated-call
latency, the parity leg and the CPU baseline to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SETS, STEPS = 256, 3
SMALL = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--sets", str(SETS), "--inflight", "2"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "p50_batch_latency_ms", "parity", "cpu_baseline")


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_headline_and_dump(tmp_path):
    d = run_bench("--dump-outputs", str(tmp_path / "dump"))
    assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_ONLY), sorted(d)
    assert d["steps"] == STEPS and d["unit"] == "sets/s" and d["higher_is_better"] is True
    # value = sets of the timed steps / their time, ms_per_step = that time / steps (both rounded in the line)
    assert d["value"] * d["ms_per_step"] / 1e3 == pytest.approx(SETS, rel=1e-2)
    assert os.listdir(tmp_path / "dump") == ["job_results.npy"]
    res = np.load(tmp_path / "dump" / "job_results.npy")
    assert res.dtype == np.float32 and np.array_equal(res, np.ones(SETS, np.float32))  # one valid job per set


def test_full_run_adds_the_other_legs():
    d = run_bench("--full")
    assert all(k in d for k in HEADLINE + FULL_ONLY), sorted(d)
    assert d["parity"]["jobs"] == SETS and d["parity"]["mismatches"] == 0
    assert d["cpu_baseline"]["results_match_gpu"] is True
    assert d["roofline"]["launches_timed"] >= 1 and d["p50_batch_latency_ms"] > 0
