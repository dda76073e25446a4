"""The block (SpMMV) plan's host planner without a GPU: row orders (ties undone, balls, flat patches) are chunk-length-preserving
permutations whose copies keep every row's slots in order; phases tile a tile's slot groups, respect the 8-group / 256-row limits and
their one-list-per-phase indices decode to the entries' columns; flat patches + dynamic-programming cuts stage at most 0.8 of the
rows of the ties-undone / greedy plan on a 3-dof mesh and never more than the ties-undone plan elsewhere (tests/helpers/block_plan_check.cpp).
The same invariants hold for the planner's other two forms: 512-row phases, and lists of 128-byte LINES (16 doubles / 32 floats) whose
indices decode as (line << shift) | row-in-line; the shapes the GPU tests run those kernels on keep the properties they are chosen for."""
import os
import subprocess

from conftest import ROOT, mtx_path

PKG = os.path.join(ROOT, "ultimate-spmv_amd")


def test_block_plan_row_orders_and_phase_cuts(tmp_path):
    exe = str(tmp_path / "block_plan_check")
    srcs = [os.path.join(ROOT, "tests", "helpers", "block_plan_check.cpp")] + [os.path.join(PKG, "host", f) for f in
            ("mtx_io.cpp", "scs_convert.cpp", "gen_matrix.cpp", "tlc_plan.cpp", "debug.cpp")]
    cmd = ["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host")] + srcs + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    r = subprocess.run([exe, mtx_path("bcsstk13"), mtx_path("impcol_e"), mtx_path("FDM-2d-16")], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:] + r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("all ok") and r.stdout.count("ok ") >= 9 * 9
    # 12 cases (band11, the small 3-dof mesh at sigma = 1 and the small 2-dof mesh at C = 64 added): per case 3 row orders x 3 cuts in the
    # 256-row form and again with 512-row phases, the line-list form (16 doubles) per row order and once on the F32 struct (32 floats)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert len(lines) == 12 * (9 + 9 + 3 + 1)
    assert sum(" cap=512 " in ln for ln in lines) == 12 * 9
    assert sum(" shift=4 " in ln for ln in lines) == 12 * 3 and sum(" f32 shift=5 " in ln for ln in lines) == 12
