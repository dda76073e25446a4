"""bench.py --dump-outputs on the CPU: y is written in the original row order, a larger y as a fixed seeded sample within the size
limit, and the same inputs give the same files.  The GPU run of the flagship path itself is bench.py's own business."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT


def _perm(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


def test_whole_y_in_original_row_order(tmp_path):
    n, pad = 1000, 24
    o2n = _perm(n + pad, 1)[:n]                   # old_to_new: original row -> SELL row (padding slots are never named)
    y_orig = np.random.default_rng(2).standard_normal(n)
    y = torch.full((n + pad,), np.nan, dtype=torch.float64)
    y[torch.from_numpy(o2n).long()] = torch.from_numpy(y_orig)
    bench.dump_outputs(str(tmp_path), y, o2n, n)
    got, rows = np.load(tmp_path / "y.npy"), np.load(tmp_path / "y_rows.npy")
    assert got.dtype == np.float64 and rows.dtype == np.float64
    assert np.array_equal(got, y_orig) and np.array_equal(rows, np.arange(n))


def test_large_y_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    n = 5000
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 16 * n - 8)        # the whole y and its row numbers do not fit
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ROWS", 600)
    o2n = _perm(n, 3)
    y = torch.from_numpy(np.random.default_rng(4).standard_normal(n))
    y_orig = y.numpy()[o2n]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), y, o2n, n)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["y.npy", "y_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 2 * 8 * 600 + 2 * 128
    rows = np.load(tmp_path / "a" / "y_rows.npy")
    assert rows.size == 600 and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert np.array_equal(np.load(tmp_path / "a" / "y.npy"), y_orig[rows.astype(np.int64)])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "out"]])
def test_rejected_arguments(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "error" in r.stderr
