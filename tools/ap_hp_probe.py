#!/usr/bin/env python3
"""ap[dp_sp] against ap[dp_sp_hp] (uspmv_spmv_ap / uspmv_spmv_ap_hp) on stencils with magnitude decades and the same t1, the two forms
timed alternately; and, on a wide-irregular banded matrix (the planners fall through to the column-window sweep), ap[dp_sp] against
ap[dp_sp_hp] and ap[dp_hp] at the same t1, alternating as well.

Per form it prints one JSON line: the plan kind the handles ended on (none | tlc | sweep), kernel time (median of the rounds, each the
mean of --reps back-to-back launches between two events), the bytes per non-zero the kernel streams (line plan: values + local indices
of every part incl. padding slots, chunk arrays, the staged x lines, y; sweep: the compacted entry streams, the count bytes, the staged
windows, the padding columns, y), that traffic over the kernel time over 8 TB/s (the streamed-bytes fraction) and the hp share of the
non-zeros.

    python tools/ap_hp_probe.py --matrix stencil74 --matrix stencil253 --matrix banded [--reps 50 --rounds 5]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

HBM = 8e12


def _build(pkg, parts, dtypes, C=32, sigma=512):
    structs = [None] * len(parts)
    s0 = pkg.convert_to_scs(parts[0], C, sigma, dtypes[0])
    perm = s0.arrays()["old_to_new_idx"].copy()
    structs[0] = s0
    for k in range(1, len(parts)):
        if parts[k] is not None:
            structs[k] = pkg.convert_to_scs(parts[k], C, sigma, dtypes[k], fixed_permutation=perm)
    for s in structs:
        if s is not None:
            pkg.permute_scs_cols(s, perm)
    return structs


def _bytes(structs, hand, planned):
    vs = {0: 8, 1: 4, 2: 2}
    b = 0
    for s in structs:
        if s is None:
            continue
        b += s.n_elements * (vs[s.dtype] + (2 if planned else 4)) + 8 * s.n_chunks
    b += 8 * structs[0].n_rows_padded                                   # y
    if planned:
        p = hand[0].plan_download()
        b += 128 * len(p["tile_lines"]) + 4 * len(p["tile_line_ptr"])   # staged x lines (128-byte double lines)
    else:
        b += 8 * structs[0].n_rows_padded                               # x read at least once
    return b


def _sweep_bytes(structs, info):
    """what the sweep kernels stream: sizeof(value) + 2 bytes per stored entry, one count byte per (row, window, part), every window of
    every tile once, the padding column and the wave offsets per part, y"""
    vs = {0: 8, 1: 4, 2: 2}
    parts = [s for s in structs if s is not None]
    rows, wlog, cnt_bytes, tiles = info["tile_rows"], info["wlog"], info["cnt_bytes"], info["sweep"]
    b = sum(s.nnz * (vs[s.dtype] + 2) for s in parts)
    b += len(parts) * (cnt_bytes + 4 * tiles * rows + 4 * tiles * rows // 64)
    b += (cnt_bytes // rows) * (1 << wlog) * vs[parts[0].dtype]           # windows staged: sum over the tiles of their window count
    b += 8 * structs[0].n_rows_padded + 24 * tiles
    return b


def _optimize_verbose(fn):
    """fn() with USPMV_VERBOSE set and the library's stderr captured: the fields of the sweep planner's report line, if it wrote one"""
    sys.stderr.flush()
    old_env, saved = os.environ.get("USPMV_VERBOSE"), os.dup(2)
    os.environ["USPMV_VERBOSE"] = "1"
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            if old_env is None:
                del os.environ["USPMV_VERBOSE"]
        tmp.seek(0)
        lines = [ln for ln in tmp.read().decode(errors="replace").splitlines() if "] sweep plan" in ln]
    if not lines:
        return None
    return {k: int(v) for k, v in (kv.split("=") for kv in lines[-1].split() if "=" in kv) if v.lstrip("-").isdigit()}


def _time(t, fn, reps):
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    fn(); fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", action="append", default=[])
    ap.add_argument("--decades", type=float, default=8.0)
    ap.add_argument("--q1", type=float, default=0.8, help="t1 = this quantile of |v| (the same t1 for both forms)")
    ap.add_argument("--q2", type=float, default=0.4, help="t2 = this quantile of |v| (ap[dp_sp_hp])")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--forms", default="", help="comma-separated subset of dp_sp,dp_sp_hp,dp_hp (default: all the matrix has)")
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    t.cuda.set_device(0)
    for name in a.matrix or ["stencil74"]:
        if name == "stencil74":
            m = pkg.gen_stencil27(74, 74, 74, 5, magnitude_decades=a.decades)
        elif name == "stencil253":
            m = pkg.gen_stencil27(253, 253, 253, 1, magnitude_decades=a.decades)
        elif name == "banded":
            m = pkg.gen_banded_random(500000, 140, 50000, magnitude_decades=10.0)
        else:
            raise SystemExit(f"unknown matrix {name}")
        v = np.abs(np.asarray(m.arrays()[2]))
        t1, t2 = float(np.quantile(v, a.q1)), float(np.quantile(v, a.q2))
        del v
        nnz = m.nnz
        forms = {}
        want = [f for f in a.forms.split(",") if f] or ["dp_sp", "dp_sp_hp"] + (["dp_hp"] if name == "banded" else [])
        if "dp_sp" in want:
            dp, sp = pkg.partition_precisions(m, t1)
            st = _build(pkg, [dp, sp], [pkg.F64, pkg.F32])
            del dp, sp
            hd = [pkg.DeviceMatrix(s) for s in st]
            info = _optimize_verbose(lambda: pkg.optimize_ap(hd[0], hd[1], st[0], st[1]))
            x = t.ones(st[0].n_rows_padded, dtype=t.float64, device="cuda"); y = t.zeros_like(x)
            forms["dp_sp"] = (st, hd, lambda hd=hd, x=x, y=y: pkg.spmv_ap(hd[0], hd[1], x, y), hd[0].plan_info()[0], 0, info)
        for kind in [f for f in want if f != "dp_sp"]:
            hi, mid, hp = pkg.partition_precisions_hp(m, kind, t1, t2)
            st = _build(pkg, [hi, mid, hp], [pkg.F64, pkg.F32, pkg.F16])
            hp_nnz = hp.nnz
            del hi, mid, hp
            hh = [pkg.DeviceMatrix(s) if s is not None else None for s in st]
            info = _optimize_verbose(lambda: pkg.optimize_ap_hp(hh[0], hh[1], hh[2], *st))
            x = t.ones(st[0].n_rows_padded, dtype=t.float64, device="cuda"); y = t.zeros_like(x)
            forms[kind] = (st, hh, lambda hh=hh, x=x, y=y: pkg.spmv_ap_hp(hh[0], hh[1], hh[2], x, y), hh[0].plan_info()[0], hp_nnz, info)
        del m
        times = {k: [] for k in forms}
        for _ in range(a.rounds):                                        # the forms alternate, round by round
            for k, f in forms.items():
                times[k].append(_time(t, f[2], a.reps))
        for k, (st, hand, _, plan_kind, hpn, info) in forms.items():
            ms = float(np.median(times[k]))
            b = _sweep_bytes(st, info) if plan_kind == 2 and info else _bytes(st, hand, plan_kind == 1)
            print(json.dumps(dict(matrix=name, form=k, plan=("none", "tlc", "sweep")[plan_kind], plan_kind=plan_kind, sweep_plan=info if plan_kind == 2 else None,
                                  nnz=nnz, t1=t1, t2=t2 if k == "dp_sp_hp" else None,
                                  ms=round(ms, 4), ms_rounds=[round(v, 4) for v in times[k]], bytes_per_nnz=round(b / nnz, 3),
                                  streamed_bytes_fraction=round(b / (ms * 1e-3) / HBM, 3), hp_share=round(hpn / nnz, 3),
                                  part_elements=[s.n_elements if s is not None else 0 for s in st])), flush=True)
        del forms
        t.cuda.synchronize()
        t.cuda.empty_cache()


if __name__ == "__main__":
    main()
