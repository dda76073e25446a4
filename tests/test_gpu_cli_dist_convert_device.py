"""`uspmv ... -convert device | device_stable` in multi-rank runs (host/uspmv_dist.cpp): the rank's block generated in HBM
(or the host block uploaded), the object from uspmv_dist_create_from_arrays_ex, the self-check against the block in HBM.  Every run: 3
timed steps, -check_y 1, the JSON line, x the ramp, y dumped; the dumped y must equal the -convert host run's byte for byte."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, mtx_path

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "ultimate-spmv_amd", "uspmv")
COMMON = ["-bench_steps", "3", "-bench_warmup", "1", "-check_y", "1", "-json", "-"]
SCS = ["scs", "-c", "32", "-s", "512"]
GEN = "gen:16x16x24"


def _env(tmp_path, tag, **kw):
    env = dict(os.environ, USPMV_DIST_X="ramp", USPMV_DUMP_Y=str(tmp_path / tag), USPMV_ID_DIR=str(tmp_path), USPMV_JOB_ID=f"{tag}{os.getpid()}",
               USPMV_HC_TIMEOUT="120", OMP_NUM_THREADS=os.environ.get("USPMV_TEST_OMP", "4"), OMP_WAIT_POLICY="passive", **kw)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "USPMV_LOOPBACK", "USPMV_LOOPBACK_RANK", "USPMV_EXCHANGE", "USPMV_DEVICE_BLOCK"):
        if k not in kw:
            env.pop(k, None)
    return env


def _report(out):
    lines = [ln for ln in out.splitlines() if ln.startswith('{"gflops"')]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def loopback(tmp_path, tag, rank, args, P=3):
    """one loopback rank; returns (report, stdout, y bytes)"""
    r = subprocess.run([EXE] + args + COMMON, cwd=tmp_path, env=_env(tmp_path, tag, USPMV_LOOPBACK=str(P), USPMV_LOOPBACK_RANK=str(rank)),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return _report(r.stdout), r.stdout, open(tmp_path / f"{tag}.{rank}", "rb").read()


def real_ranks(tmp_path, tag, args, world=3):
    """`world` rank processes sharing the GPU over the host-staged exchange; returns (rank 0's report, rank 0's stdout, [y bytes per rank])"""
    procs = []
    for rank in range(world):
        env = _env(tmp_path, tag, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", USPMV_EXCHANGE="host")
        procs.append(subprocess.Popen([EXE] + args + COMMON, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=180)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
    return _report(outs[0]), outs[0], [open(tmp_path / f"{tag}.{rank}", "rb").read() for rank in range(world)]


def checked(rep, route):
    assert rep["y_checked"] is True and rep["y_mismatches"] == 0, rep
    assert rep["setup"]["route"] == route and rep["setup"]["block_s"] >= 0 and rep["setup"]["object_s"] > 0, rep["setup"]


@pytest.mark.parametrize("rank", (0, 1, 2))
@pytest.mark.parametrize("prec", ("-dp", "-sp"))
def test_loopback_generated_block_gives_the_host_routes_y(tmp_path, prec, rank):
    base = [GEN] + SCS + [prec, "-seg_rows", "-comm_halos", "1"]
    rep_h, _, y_h = loopback(tmp_path, "h", rank, base + ["-convert", "host"])
    rep_d, out_d, y_d = loopback(tmp_path, "d", rank, base + ["-convert", "device"])
    rep_s, out_s, y_s = loopback(tmp_path, "s", rank, base + ["-convert", "device_stable"])
    checked(rep_h, "host"); checked(rep_d, "device_generated"); checked(rep_s, "device_generated")
    assert len(y_h) == 2048 * (8 if prec == "-dp" else 4) and y_d == y_h and y_s == y_h, (prec, rank)
    assert rep_d["y_checksum_rank0"] == rep_h["y_checksum_rank0"]
    # same keys as the host route's line, and the same numbers where the route cannot matter
    assert rep_d.keys() == rep_h.keys() and rep_d["rank0"].keys() == rep_h["rank0"].keys()
    for k in ("n_local", "n_halo", "n_send", "interior", "boundary", "tiles", "n_elements", "n_chunks", "n_rows_padded", "algorithmic_bytes"):
        assert rep_d["rank0"][k] == rep_h["rank0"][k], k
    assert "block generated on the device; the reference's tie order" in out_d
    assert "block generated on the device; stable tie order" in out_s


def test_uploaded_source_ap_decades(tmp_path):
    """gen: with decades 4 under -ap[dp_sp]: the host generator (pow) and an upload; algorithmic_bytes counts the sp part from the handle"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    t1 = float(np.quantile(np.abs(np.asarray(pkg.gen_stencil27(16, 16, 24, dof=1, magnitude_decades=4.0).arrays()[2])), 0.7))
    base = [GEN + ":1:4"] + SCS + ["-ap[dp_sp]", "-ap_threshold_1", repr(t1), "-seg_rows", "-comm_halos", "1"]
    for rank in (0, 1):
        rep_h, _, y_h = loopback(tmp_path, f"h{rank}", rank, base + ["-convert", "host"])
        rep_d, out_d, y_d = loopback(tmp_path, f"d{rank}", rank, base + ["-convert", "device"])
        checked(rep_h, "host"); checked(rep_d, "device_uploaded")
        assert y_d == y_h and len(y_h) == 2048 * 8
        assert rep_d["data_type"] == "ap[dp_sp]" and rep_d["rank0"]["algorithmic_bytes"] == rep_h["rank0"]["algorithmic_bytes"]
        assert "host block uploaded" in out_d


def test_uploaded_source_rand_x(tmp_path):
    base = [GEN] + SCS + ["-dp", "-rand_x", "1", "-seg_rows", "-comm_halos", "1"]
    rep_h, _, y_h = loopback(tmp_path, "h", 1, base + ["-convert", "host"])
    rep_d, _, y_d = loopback(tmp_path, "d", 1, base + ["-convert", "device"])
    checked(rep_h, "host"); checked(rep_d, "device_uploaded")
    assert y_d == y_h and len(y_h) == 2048 * 8


def test_uploaded_source_mtx_three_real_ranks(tmp_path):
    base = [mtx_path("bcsstk13")] + SCS + ["-dp", "-seg_nnz", "-comm_halos", "1"]
    rep_h, _, ys_h = real_ranks(tmp_path, "h", base + ["-convert", "host"])
    rep_d, out_d, ys_d = real_ranks(tmp_path, "d", base + ["-convert", "device"])
    checked(rep_h, "host"); checked(rep_d, "device_uploaded")
    assert ys_d == ys_h and sum(len(y) for y in ys_h) == 2003 * 8 and "host block uploaded" in out_d
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".uspmvcoo")], "block files must be gone"


def test_generated_source_unequal_blocks_three_real_ranks(tmp_path):
    base = [GEN] + SCS + ["-dp", "-seg_nnz", "-comm_halos", "1"]
    rep_h, _, ys_h = real_ranks(tmp_path, "h", base + ["-convert", "host"])
    rep_d, _, ys_d = real_ranks(tmp_path, "d", base + ["-convert", "device"])
    checked(rep_h, "host"); checked(rep_d, "device_generated")
    assert len({len(y) for y in ys_h}) > 1, "seg-nnz blocks of the stencil are unequal"
    assert ys_d == ys_h and sum(len(y) for y in ys_h) == 16 * 16 * 24 * 8
    assert [r["n_local"] for r in rep_d["per_rank"]] == [r["n_local"] for r in rep_h["per_rank"]]


def test_auto_all_takes_the_uploaded_source_and_says_so(tmp_path):
    rep, out, _ = loopback(tmp_path, "a", 0, [GEN] + SCS + ["-dp", "-seg_rows", "-comm_halos", "1", "-step_form", "auto_all", "-convert", "device"])
    checked(rep, "device_uploaded")
    assert "host block uploaded" in out and "block generated on the device" not in out


def test_single_rank_ap_convert_device_is_still_refused(tmp_path):
    r = subprocess.run([EXE, GEN] + SCS + ["-ap[dp_sp]", "-ap_threshold_1", "0.5", "-convert", "device"], cwd=tmp_path, env=_env(tmp_path, "x"),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-convert device needs a one-precision run (-dp or -sp)." in r.stderr
