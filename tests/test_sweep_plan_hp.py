"""Column-window sweep plan for the adaptive-precision splits with an fp16 part (ultimate-spmv_amd/host/sweep_plan.cpp with two or three
structs) checked on the host: tests/cpp/sweep_plan_hp_emulate.cpp replays the plan the way scs_spmv_sweep_ap_hp consumes it and compares
with every part's slot-ordered chain, composed as the kernels compose them, bit for bit -- ap[dp_hp], ap[sp_hp], ap[dp_sp_hp]; several
C / sigma / window / tile shapes; rows with > 255 entries of one part in a window and a row with unsorted columns (their tiles go to the
rest list); empty parts, rows empty in some parts only; +-0, +-inf, NaN, hp values that overflow binary16, an explicit +0 on a row's last
column.  It also requires the one-struct and the dp+sp plan to come out byte for byte in the layout they had before the third part
existed (restated in the harness), and repeats on the three-part planner the coverage tests/test_gpu_sweep_ap_hp.py relies on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_plan_hp_replay_matches_part_chains(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "sweep_plan_hp_emulate")
    # -ffp-contract=off: the float products of ap[sp_hp] must be rounded before they are added, as __fmul_rn does on the device
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(libdir, "host"),
                           os.path.join(ROOT, "tests", "cpp", "sweep_plan_hp_emulate.cpp"), "-o", exe, "-L" + libdir, "-luspmv",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-6000:] + out.stderr[-2000:]
