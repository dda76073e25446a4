"""`uspmv gen:... -convert device | device_stable -equilibrate 1` in multi-rank runs (host/uspmv_dist.cpp): the rank's block
is generated in HBM and scaled there by uspmv_equilibrate_device -- its local rows, global columns, as the host route scales its block
with uspmv_coo_equilibrate -- and the self-check runs against the scaled arrays.  The dumped y must equal the -convert host run's byte for
byte.  The loopback harness is that of tests/test_gpu_cli_dist_convert_device.py."""
import subprocess

import pytest

from test_gpu_cli_dist_convert_device import COMMON, EXE, GEN, SCS, _env, _report, checked, loopback

pytestmark = pytest.mark.gpu
RANK = 1


@pytest.mark.parametrize("prec", ("-dp", "-sp"))
def test_loopback_block_scaled_on_the_device_gives_the_host_routes_y(tmp_path, prec):
    base = [GEN] + SCS + [prec, "-seg_rows", "-comm_halos", "1", "-equilibrate", "1"]
    rep_h, _, y_h = loopback(tmp_path, "h", RANK, base + ["-convert", "host"])
    rep_d, out_d, y_d = loopback(tmp_path, "d", RANK, base + ["-convert", "device"])
    rep_s, out_s, y_s = loopback(tmp_path, "s", RANK, base + ["-convert", "device_stable"])
    checked(rep_h, "host"); checked(rep_d, "device_generated"); checked(rep_s, "device_generated")
    assert len(y_h) == 2048 * (8 if prec == "-dp" else 4) and y_d == y_h and y_s == y_h, prec
    assert rep_d["y_checksum_rank0"] == rep_h["y_checksum_rank0"] == rep_s["y_checksum_rank0"]
    assert "block generated on the device" in out_d and "block generated on the device" in out_s
    if prec == "-dp":
        # USPMV_DEVICE_BLOCK=upload still forces the uploaded source: the host block, scaled on the host
        tag = "f"
        r = subprocess.run([EXE] + base + ["-convert", "device"] + COMMON, cwd=tmp_path,
                           env=_env(tmp_path, tag, USPMV_LOOPBACK="3", USPMV_LOOPBACK_RANK=str(RANK), USPMV_DEVICE_BLOCK="upload"),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        checked(_report(r.stdout), "device_uploaded")
        assert "host block uploaded" in r.stdout and open(tmp_path / f"{tag}.{RANK}", "rb").read() == y_h
