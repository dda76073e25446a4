"""The non-square matrices of tests/test_gpu_nonsquare.py on the host.  The non-square gates: the additive chunk records are for square
matrices (csrc/tlc_planner.hip additive_eligible, host/tlc_plan.cpp), so uspmv_additive_plan_probe must keep nothing on any struct the GPU
file multiplies with, whatever "tlc_additive" says.  And the planners' answers the GPU file asserts on the device -- every line and
element plan stages every tile, the sweep takes every tile or declines as sweeps() says, x_len_min is 1 + the highest column over ALL
parts -- come from tests/cpp/nonsquare_plan_check.cpp, which runs the host planners on the same structs."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_nonsquare as ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("block", "halo", "thin", "tall")


@pytest.fixture(scope="module")
def mats(pkg):
    out = {}
    for name in NAMES:
        gen, n, nc, _ = ns.MATRICES[name]
        out[name] = gen(pkg)
        I, J, _ = out[name].arrays()
        assert (out[name].n_rows, out[name].n_cols) == (n, nc) and n != nc
        assert np.all(np.diff(np.asarray(I)) >= 0) and int(np.asarray(J).max()) < nc
    return out


def _kept_nothing(pkg, s, tag):
    for additive in (1, 2):
        old = pkg.get_tuning("tlc_additive")
        pkg.set_tuning(tlc_additive=additive)
        try:
            st, _ = pkg.additive_plan_probe(s, decode=False)
        finally:
            pkg.set_tuning(tlc_additive=old)
        assert st["kept"] == 0 and st["n_additive"] == 0 and st["n_chunks"] == 0 and st["tiles_with_records"] == 0, (tag, additive, st)


@pytest.mark.parametrize("name", NAMES)
def test_no_additive_records_on_a_nonsquare_struct(pkg, mats, name):
    m = mats[name]
    structs = 0
    for C, sigma in ns.CSIG:
        for code in (pkg.F64, pkg.F32):
            s = pkg.convert_to_scs(m, C, sigma, code)
            pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"].copy())
            assert s.n_rows != s.n_cols
            _kept_nothing(pkg, s, (name, C, sigma, code)); structs += 1
        if name in ("block", "halo") and (C, sigma) != (16, 16):
            ds, ss = ns._pair_structs(pkg, m, C, sigma, th=ns.TH_PAIR)
            parts = [ds, ss]
            for kind in ("dp_hp", "sp_hp", "dp_sp_hp"):
                built = ns._build(pkg, m, kind, C, sigma, *ns.TH_HP)
                assert built is not None, (name, kind, C, sigma, "a conversion was refused")
                parts += [q for q in built[0] if q is not None and q.dtype != pkg.F16]      # (the records are for dp and sp structs)
            for q in parts:
                assert q.nnz > 0
                _kept_nothing(pkg, q, (name, C, sigma, "part", q.dtype)); structs += 1
    assert structs == (8 + 3 * 6 if name in ("block", "halo") else 8)


def _facts(line):
    head, *rest = line.split()
    kv = dict(f.split("=") for f in rest if "=" in f)
    return head, [f for f in rest if "=" not in f], kv


def _checker(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "nonsquare_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(libdir, "host"),
                           os.path.join(ROOT, "tests", "cpp", "nonsquare_plan_check.cpp"), "-o", exe, "-L" + libdir, "-luspmv",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_which_shapes_keep_the_line_plan(pkg, mats, tmp_path):
    """LINE_PLAN of the GPU file: the block planner's line plan under "spmmv_xline" is turned down on the scattered shapes and kept, in dp
    and sp, on the mesh row block -- whose x rows (8097, odd) lie beyond the padded rows like the others'"""
    exe = _checker(pkg, tmp_path)
    made = dict(mats)
    gen, n, nc, n_pad = ns.MATRICES["mesh"]
    made["mesh"] = gen(pkg)
    assert (made["mesh"].n_rows, made["mesh"].n_cols) == (n, nc)
    kept = 0
    for (name, C, sigma), want in ns.LINE_PLAN.items():
        coo = str(tmp_path / (name + ".coo"))
        made[name].save(coo)
        out = subprocess.run([exe, coo, str(C), str(sigma), "0", "0,0"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
        facts = [_facts(ln) for ln in out.stdout.strip().splitlines()[:-1]]
        assert [f[0] for f in facts] == ["struct", "struct"] and [f[1][0] for f in facts] == ["f64", "f32"]
        assert tuple(int(f[2]["line_plan"]) for f in facts) == want, (name, C, sigma, out.stdout)
        assert all(f[2]["phased"] == "1" for f in facts)
        if name == "mesh":
            assert all(int(f[2]["x_rows"]) == ns.MESH_X_ROWS > int(f[2]["n_pad"]) == n_pad for f in facts)
        kept += sum(want)
    assert kept == 4


@pytest.mark.parametrize("name", NAMES)
def test_host_planners_on_nonsquare(pkg, mats, tmp_path, name):
    exe = _checker(pkg, tmp_path)
    coo = str(tmp_path / (name + ".coo"))
    mats[name].save(coo)
    _, n, nc, n_pad = ns.MATRICES[name]
    split = name in ("block", "halo")
    lines_seen = 0
    for C, sigma in ns.CSIG:
        out = subprocess.run([exe, coo, str(C), str(sigma), repr(ns.TH_PAIR) if split else "0", "%r,%r" % ns.TH_HP], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
        lines = out.stdout.strip().splitlines()[:-1]
        assert [ln.split()[0] for ln in lines] == ["struct", "struct"] + (["dp_sp", "dp_hp", "sp_hp", "dp_sp_hp"] if split else [])
        for ln in lines:
            head, flags, kv = _facts(ln)
            tag = (name, C, sigma, ln)
            assert "refused" not in flags, tag
            assert int(kv["n_pad"]) == n_pad, tag
            x_rows = int(kv["x_rows"])
            if name == "block":
                assert x_rows == ns.BLOCK_X_ROWS and x_rows > n_pad and x_rows % 2 == 1 and x_rows % 4 != 0, tag
            elif name in ("halo", "thin"):
                assert x_rows == nc, tag
            else:
                assert x_rows <= 512 < n_pad, tag
            for wlog, rows in ns.SWEEP_SHAPES:
                nt = -(-n_pad // rows)
                assert kv["sweep%d" % wlog] == ("all:%d" if ns.sweeps(name, sigma, wlog) else "none:%d") % nt, tag
            if head == "struct":
                assert int(kv["parked"]) == (7 if name == "halo" and sigma >= 64 else 0), tag
                for rows in (256, 512, 1024):
                    nt = -(-n_pad // rows)
                    assert kv["line%d" % rows] == "%d/%d" % (nt, nt), tag
                assert kv["elem"] == "%d/%d" % (-(-n_pad // 256), -(-n_pad // 256)), tag
                for wlog in (9, 11):
                    assert kv["bsweep%d" % wlog] == "all:%d" % -(-n_pad // 1024), tag
                if C in (32, 64):
                    assert kv["phased"] == "1", tag
                assert kv["additive"] == "0/0", tag
            else:
                assert all(int(v) > 0 for v in kv["nnz"].split(",")), tag
                assert kv["line512"] == "%d/%d" % (-(-n_pad // 512), -(-n_pad // 512)), tag
                if name == "block":      # the first part alone refers to fewer x rows than the split: x_len must come from all parts
                    assert int(kv["x_rows_first"]) == ns.BLOCK_X_ROWS_FIRST < x_rows, tag
            lines_seen += 1
    assert lines_seen == 4 * (6 if split else 2)
