"""GPU: bench.py end to end on a small C4 graph.  A plain run prints the headline line and writes --dump-outputs; the legs
that take runs of their own (roofline, parity, CPU baselines, kNN, training, partitioned driver) come only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--nodes", "20000", "--edges", "400000", "--knn-n", "4096"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY = {"median_ms_per_step", "hidden_conv_edges_per_sec", "roofline", "partitioned_path_n1", "knn", "train",
             "cpu_baseline", "cpu_baseline_torch", "parity"}


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_is_the_headline_alone(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert HEADLINE <= set(line) and not FULL_ONLY & set(line), sorted(line)
    assert line["metric"] == "aggregated_edges_per_sec_ktgnn_fwd" and line["unit"] == "edges/s" and line["higher_is_better"]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    for name in ("base", "target", "target_hat"):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.shape == (20000, 2) and np.isfinite(a).all()


def test_full_run_adds_the_other_legs():
    line = _bench("--full")
    assert HEADLINE | FULL_ONLY <= set(line), sorted(FULL_ONLY - set(line))
    assert line["parity"]["within_1e-5"]
    assert line["train"]["steps"] == 5
