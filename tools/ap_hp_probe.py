#!/usr/bin/env python3
"""ap[dp_sp] against ap[dp_sp_hp] (uspmv_spmv_ap / uspmv_spmv_ap_hp) on stencils with magnitude decades and the same t1, the two forms
timed alternately; and the planless lane-per-row ap[dp_sp_hp] kernel on a wide-irregular banded matrix (no sweep plan for hp parts).

Per form it prints one JSON line: kernel time (median of the rounds, each the mean of --reps back-to-back launches between two events),
the bytes per non-zero the kernel streams (values + local indices of every part incl. padding slots, chunk arrays, the staged x lines,
y), that traffic over the kernel time over 8 TB/s (the streamed-bytes fraction) and the hp share of the non-zeros.

    python tools/ap_hp_probe.py --matrix stencil74 --matrix stencil253 --matrix banded [--reps 50 --rounds 5]
"""
import argparse
import json
import os
import sys

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
        if name != "banded":
            dp, sp = pkg.partition_precisions(m, t1)
            st = _build(pkg, [dp, sp], [pkg.F64, pkg.F32])
            del dp, sp
            hd = [pkg.DeviceMatrix(s) for s in st]
            nt, ns = pkg.optimize_ap(hd[0], hd[1], st[0], st[1])
            x = t.ones(st[0].n_rows_padded, dtype=t.float64, device="cuda"); y = t.zeros_like(x)
            forms["dp_sp"] = (st, hd, lambda hd=hd, x=x, y=y: pkg.spmv_ap(hd[0], hd[1], x, y), hd[0].plan_info()[0] == 1, 0, x, y)
        hi, mid, hp = pkg.partition_precisions_hp(m, "dp_sp_hp", t1, t2)
        st = _build(pkg, [hi, mid, hp], [pkg.F64, pkg.F32, pkg.F16])
        hp_nnz = hp.nnz
        del hi, mid, hp
        hh = [pkg.DeviceMatrix(s) for s in st]
        nt, ns = pkg.optimize_ap_hp(hh[0], hh[1], hh[2], *st)
        x = t.ones(st[0].n_rows_padded, dtype=t.float64, device="cuda"); y = t.zeros_like(x)
        forms["dp_sp_hp"] = (st, hh, lambda hh=hh, x=x, y=y: pkg.spmv_ap_hp(hh[0], hh[1], hh[2], x, y), hh[0].plan_info()[0] == 1, hp_nnz, x, y)
        del m
        times = {k: [] for k in forms}
        for _ in range(a.rounds):                                        # the forms alternate, round by round
            for k, f in forms.items():
                times[k].append(_time(t, f[2], a.reps))
        for k, (st, hand, _, planned, hpn, _, _) in forms.items():
            ms = float(np.median(times[k]))
            b = _bytes(st, hand, planned)
            print(json.dumps(dict(matrix=name, form=k, plan="tlc" if planned else "none", nnz=nnz, t1=t1, t2=t2 if k == "dp_sp_hp" else None,
                                  ms=round(ms, 4), ms_rounds=[round(v, 4) for v in times[k]], bytes_per_nnz=round(b / nnz, 3),
                                  streamed_bytes_fraction=round(b / (ms * 1e-3) / HBM, 3), hp_share=round(hpn / nnz, 3),
                                  part_elements=[s.n_elements if s is not None else 0 for s in st])), flush=True)
        del forms
        t.cuda.synchronize()
        t.cuda.empty_cache()


if __name__ == "__main__":
    main()
