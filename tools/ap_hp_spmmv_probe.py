#!/usr/bin/env python3
"""Adaptive-precision SpMMV with an fp16 part (uspmv_spmmv_ap_hp) against what a caller had before it, alternated in one process on the
same handles:

  (a) spmmv_ap_hp of the split, width b
  (g) the same with tuning "tlc" 0: the generic lane-per-row kernel
  (b) b calls of spmv_ap_hp on the same (planned) handles                 -- the matrix streamed b times
  (c) spmmv_ap of the ap[dp_sp] pair at the same t1, on its own default plan  -- reported only, decides nothing
  (a) once more in every round: the A/A spread of this run

Matrix: stencil74 (27-point, 5 dof on 74^3 nodes, magnitudes over 8 decades, SELL-32-512); t1 / t2 the 0.8 / 0.4 quantiles of |v|.  The
hp handles are planned with optimize_ap_hp(..., spmmv_ap_hp_plan_lines(b, dtype)).  Every figure is the median over --rounds of the mean
of --reps back-to-back calls between two events (two untimed calls first).

Per (kind, b, layout) one JSON line: the times, the ratios, the spread, whether (a) is ahead of (b) and of (g) by more than the spread,
the path uspmv_spmmv_ap_hp_path reports, and the bytes the staged kernel streams (values + 16-bit indices of every part and pass, chunk
arrays, every tile's lines of X rows once per vector, Y) over the time over 8 TB/s.

    python tools/ap_hp_spmmv_probe.py [--kind dp_hp --kind dp_sp_hp --b 4 --b 8 --layout rowwise --reps 100 --rounds 3 --out probe.jsonl]

--sweep: the block sweep kernel over the parts' shared column-window sweep plan (path 3) instead, on the banded-random matrix of DESIGN
5.6 (500 000 x 140 over +-50 000 columns, 10 decades, SELL-32-512, t1 / t2 the 0.7 / 0.35 quantiles), see sweep_vs_generic.

    python tools/ap_hp_spmmv_probe.py --sweep [--kind sp_hp --b 2 --layout rowwise --reps 200 --rounds 3 --out probe.jsonl]
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
    structs[0] = pkg.convert_to_scs(parts[0], C, sigma, dtypes[0])
    perm = structs[0].arrays()["old_to_new_idx"].copy()
    for k in range(1, len(parts)):
        if parts[k] is not None:
            structs[k] = pkg.convert_to_scs(parts[k], C, sigma, dtypes[k], fixed_permutation=perm)
    for s in structs:
        if s is not None:
            pkg.permute_scs_cols(s, perm)
    return structs


def _time(t, fn, reps):
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    fn(); fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def sweep_vs_generic(pkg, t, a, out):
    """(a) spmmv_ap_hp, (g) the same call under tuning "sweep" 0 -- the generic lane-per-row kernel, what ran before the block sweep
    kernel existed --, (b) b x spmv_ap_hp on these handles, (b0) b x spmv_ap_hp on default-planned handles (the single-vector kernel at
    its best), (a) once more for the A/A spread; alternated on the same handles in every round.  Plans: every window at which
    uspmv_spmmv_ap_hp_sweep_vectors names more vectors of this b per pass than at the next wider one, from the widest that holds two,
    built on the device (the arrays of the host planner, tests/test_gpu_sweep_ap_hp.py).  --tile-rows: the plan's rows per tile (0: the
    planner's default)."""
    m = pkg.gen_banded_random(500000, 140, 50000, magnitude_decades=10.0)
    v = np.abs(np.asarray(m.arrays()[2]))
    v = v[(v > 0) & np.isfinite(v)]
    t1, t2 = float(np.quantile(v, 0.7)), float(np.quantile(v, 0.35))
    del v
    nnz = m.nnz
    vs = {pkg.F64: 8, pkg.F32: 4, pkg.F16: 2}
    for kind in a.kind or ["dp_hp", "sp_hp", "dp_sp_hp"]:
        hi, mid, hp = pkg.partition_precisions_hp(m, kind, t1, t2)
        xdt = pkg.F32 if kind == "sp_hp" else pkg.F64
        st = _build(pkg, [hi, mid, hp], [xdt, pkg.F32, pkg.F16])
        del hi, mid, hp
        n = st[0].n_rows_padded
        tdt = t.float32 if kind == "sp_hp" else t.float64
        H0 = [pkg.DeviceMatrix(s) if s is not None else None for s in st]
        pkg.optimize_device_ap_hp(H0[0], H0[1], H0[2])
        for b in a.b or [2, 4, 8, 16]:
            windows = [w for w in range(8, 16) if pkg.spmmv_ap_hp_sweep_vectors(b, w, xdt) > pkg.spmmv_ap_hp_sweep_vectors(b, w + 1, xdt)]
            X = t.ones(b * n, dtype=tdt, device="cuda"); Y = t.zeros_like(X)
            alg = sum(s.n_elements * (vs[s.dtype] + 4) + 8 * s.n_chunks for s in st if s is not None) + 2 * vs[xdt] * b * n
            for wlog in sorted(windows, reverse=True):
                H = [pkg.DeviceMatrix(s) if s is not None else None for s in st]
                tiles, swept = pkg.optimize_sweep_device_ap_hp(H[0], H[1], H[2], wlog, a.tile_rows)
                meta = H[0].sweep_plan_digest()[1]
                for layout in a.layout or ["rowwise", "colwise"]:
                    lay = pkg.ROWWISE if layout == "rowwise" else pkg.COLWISE
                    path, vec = pkg.spmmv_ap_hp_path(H[0], H[1], H[2], b, n, lay)
                    fa = lambda: pkg.spmmv_ap_hp(H[0], H[1], H[2], X, Y, b, n, lay)           # noqa: E731
                    fb = lambda: [pkg.spmv_ap_hp(H[0], H[1], H[2], X, Y) for _ in range(b)]   # noqa: E731
                    fb0 = lambda: [pkg.spmv_ap_hp(H0[0], H0[1], H0[2], X, Y) for _ in range(b)]   # noqa: E731
                    ta, tg, tb, tb0, ta2 = [], [], [], [], []
                    for _ in range(a.rounds):
                        ta.append(_time(t, fa, a.reps))
                        pkg.set_tuning(sweep=0)
                        try:
                            path_g = pkg.spmmv_ap_hp_path(H[0], H[1], H[2], b, n, lay)[0]
                            tg.append(_time(t, fa, a.reps))
                        finally:
                            pkg.set_tuning(sweep=1)
                        tb.append(_time(t, fb, max(1, a.reps // b)))
                        tb0.append(_time(t, fb0, max(1, a.reps // b)))
                        ta2.append(_time(t, fa, a.reps))
                    ms_a, ms_g, ms_b, ms_b0 = (float(np.median(q)) for q in (ta, tg, tb, tb0))
                    spread = max(ta + ta2) - min(ta + ta2)
                    rec = dict(matrix="banded500k", config="sweep_vs_generic", kind=kind, b=b, layout=layout, nnz=nnz, n_rows_padded=n, t1=t1,
                               t2=t2 if kind == "dp_sp_hp" else None, part_elements=[s.n_elements if s is not None else 0 for s in st],
                               wlog=int(meta[2]), tile_rows=int(meta[1]), tiles=tiles, tiles_swept=swept, path=path, vectors_per_pass=vec,
                               passes=b // vec if vec else 0, kernel=("generic", "gather", "staged", "sweep")[path], path_sweep_off=path_g,
                               reps=a.reps, rounds=a.rounds, ms_a_spmmv_ap_hp=round(ms_a, 4), ms_g_sweep_off=round(ms_g, 4),
                               ms_b_times_spmv_ap_hp=round(ms_b, 4), ms_b0_times_spmv_ap_hp_default_plan=round(ms_b0, 4),
                               ms_a_again=round(float(np.median(ta2)), 4), aa_spread_ms=round(spread, 4), g_over_a=round(ms_g / ms_a, 3),
                               b_over_a=round(ms_b / ms_a, 3), b0_over_a=round(ms_b0 / ms_a, 3),
                               a_ahead_of_g_by_more_than_spread=bool(ms_g - ms_a > spread), a_ahead_of_b_by_more_than_spread=bool(ms_b - ms_a > spread),
                               a_ahead_of_b0_by_more_than_spread=bool(ms_b0 - ms_a > spread), algorithmic_bytes=alg,
                               algorithmic_bytes_over_time_over_8TBs=round(alg / (ms_a * 1e-3) / HBM, 3),
                               ms_rounds=dict(a=[round(q, 4) for q in ta], g=[round(q, 4) for q in tg], b=[round(q, 4) for q in tb],
                                              b0=[round(q, 4) for q in tb0], a_again=[round(q, 4) for q in ta2]))
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out: out.write(line + "\n"); out.flush()
                del H
            del X, Y
            t.cuda.synchronize()
            t.cuda.empty_cache()
        del st, H0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", action="append", default=[])
    ap.add_argument("--b", type=int, action="append", default=[])
    ap.add_argument("--layout", action="append", default=[])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-pair", action="store_true", help="skip (c), the ap[dp_sp] pair")
    ap.add_argument("--sweep", action="store_true", help="only: the block sweep kernel over the shared sweep plan against the generic kernel and "
                                                         "b x spmv_ap_hp on the same handles (sweep_vs_generic, banded-random 500 k x 140)")
    ap.add_argument("--tile-rows", type=int, default=0, help="--sweep: rows per tile of the plans (0: the planner's default)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    t.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None
    if a.sweep:
        sweep_vs_generic(pkg, t, a, out)
        if out: out.close()
        return
    m = pkg.gen_stencil27(74, 74, 74, 5, magnitude_decades=8.0)
    v = np.abs(np.asarray(m.arrays()[2]))
    t1, t2 = float(np.quantile(v, 0.8)), float(np.quantile(v, 0.4))
    del v
    nnz = m.nnz
    pair = None
    if not a.no_pair:
        dp, sp = pkg.partition_precisions(m, t1)
        ps = _build(pkg, [dp, sp], [pkg.F64, pkg.F32])
        del dp, sp
        pair = [pkg.DeviceMatrix(s) for s in ps]
        pkg.optimize_ap(pair[0], pair[1], ps[0], ps[1])
    vs = {pkg.F64: 8, pkg.F32: 4, pkg.F16: 2}
    for kind in a.kind or ["dp_hp", "sp_hp", "dp_sp_hp"]:
        hi, mid, hp = pkg.partition_precisions_hp(m, kind, t1, t2)
        hp_share = hp.nnz / nnz
        xdt = pkg.F32 if kind == "sp_hp" else pkg.F64
        st = _build(pkg, [hi, mid, hp], [xdt, pkg.F32, pkg.F16])
        del hi, mid, hp
        n = st[0].n_rows_padded
        tdt = t.float32 if kind == "sp_hp" else t.float64
        for b in a.b or [2, 4, 8, 16]:
            H = [pkg.DeviceMatrix(s) if s is not None else None for s in st]
            budget = pkg.spmmv_ap_hp_plan_lines(b, xdt)
            tiles, staged = pkg.optimize_ap_hp(H[0], H[1], H[2], *st, budget)
            plan_kind = H[0].plan_info()[0]
            plan = H[0].plan_download() if plan_kind == 1 else None
            X = t.ones(b * n, dtype=tdt, device="cuda"); Y = t.zeros_like(X)
            Xd = t.ones(b * n, dtype=t.float64, device="cuda") if pair else None
            Yd = t.zeros_like(Xd) if pair else None
            for layout in a.layout or ["rowwise", "colwise"]:
                lay = pkg.ROWWISE if layout == "rowwise" else pkg.COLWISE
                path, vec = pkg.spmmv_ap_hp_path(H[0], H[1], H[2], b, n, lay)
                fa = lambda: pkg.spmmv_ap_hp(H[0], H[1], H[2], X, Y, b, n, lay)          # noqa: E731
                fb = lambda: [pkg.spmv_ap_hp(H[0], H[1], H[2], X, Y) for _ in range(b)]  # noqa: E731
                fc = (lambda: pkg.spmmv_ap(pair[0], pair[1], Xd, Yd, b, n, lay)) if pair else None   # noqa: E731
                ta, tg, tb, tc, ta2 = [], [], [], [], []
                for _ in range(a.rounds):
                    ta.append(_time(t, fa, a.reps))
                    pkg.set_tuning(tlc=0)
                    try:
                        tg.append(_time(t, fa, a.reps))
                    finally:
                        pkg.set_tuning(tlc=1)
                    tb.append(_time(t, fb, max(1, a.reps // b)))
                    if fc: tc.append(_time(t, fc, a.reps))
                    ta2.append(_time(t, fa, a.reps))
                ms_a, ms_g, ms_b = (float(np.median(q)) for q in (ta, tg, tb))
                ms_c = float(np.median(tc)) if tc else None
                spread = max(ta + ta2) - min(ta + ta2)
                passes = b // vec if vec else 0
                streamed = None
                if path == 2:
                    streamed = sum(s.n_elements * (vs[s.dtype] + 2) * passes + 12 * s.n_chunks for s in st if s is not None) + vs[xdt] * b * n
                    streamed += 16 * vs[xdt] * b * len(plan["tile_lines"]) + 4 * len(plan["tile_line_ptr"])
                rec = dict(matrix="stencil74", kind=kind, b=b, layout=layout, nnz=nnz, n_rows_padded=n, hp_share=round(hp_share, 3), t1=t1,
                           t2=t2 if kind == "dp_sp_hp" else None, part_elements=[s.n_elements if s is not None else 0 for s in st],
                           line_budget=budget, plan_kind=plan_kind, tiles=tiles, tiles_staged=staged,
                           max_lines_used=plan["max_lines_used"] if plan else 0, path=path, vectors_per_pass=vec,
                           kernel=("generic", "gather", "staged", "sweep")[path], reps=a.reps, rounds=a.rounds,
                           ms_a_spmmv_ap_hp=round(ms_a, 4), ms_g_tlc_off=round(ms_g, 4), ms_b_times_spmv_ap_hp=round(ms_b, 4),
                           ms_c_spmmv_ap_pair=round(ms_c, 4) if ms_c else "not measured", ms_a_again=round(float(np.median(ta2)), 4),
                           aa_spread_ms=round(spread, 4), b_over_a=round(ms_b / ms_a, 3), g_over_a=round(ms_g / ms_a, 3),
                           c_over_a=round(ms_c / ms_a, 3) if ms_c else "not measured",
                           a_ahead_of_b_by_more_than_spread=bool(ms_b - ms_a > spread), a_ahead_of_g_by_more_than_spread=bool(ms_g - ms_a > spread),
                           streamed_bytes=streamed,
                           streamed_bytes_over_time_over_8TBs=round(streamed / (ms_a * 1e-3) / HBM, 3) if streamed else None,
                           ms_rounds=dict(a=[round(q, 4) for q in ta], g=[round(q, 4) for q in tg], b=[round(q, 4) for q in tb],
                                          c=[round(q, 4) for q in tc], a_again=[round(q, 4) for q in ta2]))
                line = json.dumps(rec)
                print(line, flush=True)
                if out: out.write(line + "\n"); out.flush()
            del H, X, Y, Xd, Yd
            t.cuda.synchronize()
            t.cuda.empty_cache()
        del st
    if out: out.close()


if __name__ == "__main__":
    main()
