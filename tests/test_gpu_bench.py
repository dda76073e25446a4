"""bench.py --gpus 1 on the GPU at a small grid: a plain run prints the headline line alone (and the --dump-outputs files), --full the
whole line with its checks and baselines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FULL_ONLY = ("roofline", "gpu_state", "y_placement", "cpu_baseline", "bitexact_vs_reference_cpu", "vendor_baseline", "other_configs")


def run_bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--grid", "48", *argv],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, f"rc {r.returncode}, {len(lines)} JSON lines:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    d = run_bench("--dump-outputs", str(tmp_path))
    assert d["metric"] == "SpMV GFLOP/s (SELL-32-512 dp; achieved HBM GB/s in roofline)" and d["unit"] == "GFLOP/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == 5 and d["warmup"] == 2
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["config"]["n_rows"] == 48 ** 3
    assert not [k for k in FULL_ONLY if k in d]
    y, rows = np.load(tmp_path / "y.npy"), np.load(tmp_path / "y_rows.npy")
    assert y.shape == (48 ** 3,) and np.array_equal(rows, np.arange(48 ** 3)) and np.all(np.isfinite(y))


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_the_baselines():
    d = run_bench("--full", "--no-traffic", "--no-vendor-baseline", "--other-configs", "", "--cpu-seconds", "0.5")
    assert d["value"] > 0 and d["bitexact_vs_reference_cpu"] is True and d["cpu_baseline"]["value"] > 0
    assert d["roofline"]["kernel_ms"] > 0 and d["roofline"]["stream_same_run_GBs"]["read"] > 0
    assert "idle_before_timing" in d["gpu_state"] and "kernel_ms_per_output_vector" in d["y_placement"]
