"""Block-vector column-window sweep plan (ultimate-spmv_amd/host/sweep_plan.cpp: uspmv_build_block_sweep_plan) checked on the host:
tests/cpp/block_sweep_plan_emulate.cpp replays the plan the way scs_spmmv_sweep consumes it (per-wave stream offsets, windows ascending,
rounds in batches of four with the ballot arithmetic, padding once per column) and compares every accumulator with the reference's
slot-ordered FMA chain, bit for bit, in double and float: a partial last wave, a tile without windows, a count byte of 255, the shapes the
planner declines, special values in X.  The program also corrupts one plan and fails unless its replay notices."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_sweep_plan_replay_matches_fma_chain(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "block_sweep_plan_emulate")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(libdir, "host"),
                           os.path.join(ROOT, "tests", "cpp", "block_sweep_plan_emulate.cpp"), "-o", exe, "-L" + libdir, "-luspmv",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
    assert "corrupted plan" in out.stdout and "-> caught" in out.stdout and "NOT CAUGHT" not in out.stdout, out.stdout
