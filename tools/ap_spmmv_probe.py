#!/usr/bin/env python3
"""Adaptive-precision SpMMV (uspmv_spmmv_ap) against what a caller had before it, alternated in one process on the same handles:

  (a) spmmv_ap of the pair, width b
  (b) b calls of spmv_ap on the same (planned) pair                      -- the matrix streamed b times
  (c) spmmv of the UNSPLIT dp matrix with the block plan DeviceMatrix(s, block_tlc=b) gives it
  (d) (a) once more in every round: the A/A spread of this run

Matrices: stencil74 (27-point, 5 dof on 74^3 nodes), stencil111 (3 dof on 111^3), banded (500 000 rows, 140 entries per row over a
+-50 000 band); magnitudes over 10 decades, threshold 1e-3, SELL-32-512.  Layouts: rowwise, colwise, colwise with X prepared
(uspmv_spmmv_x_prepared).  Every figure is the median over --rounds of the mean of --reps back-to-back launches between two HIP
events (uspmv_time_launches, two untimed launches first).

Per (matrix, b, layout) one JSON line: the times, the ratios b/a and c/a, the spread, whether (a) beats (b) by more than the spread,
the algorithmic bytes  n_el_dp * 12 + n_el_sp * 8 + 16 * n_chunks + 8 * b * (n_cols + n_rows_padded)  and the bytes the launch
really moves through HBM at least (the same plus the re-layout pass of a column-major X that is not prepared), each over the kernel
time over 8 TB/s as a fraction of its own name, and the X bytes the gathers request from the caches (8 * b per stored entry).

    python tools/ap_spmmv_probe.py --matrix stencil74 --b 4 --b 8 [--reps 200 --rounds 3 --no-unsplit --out probe.jsonl]
    python tools/ap_spmmv_probe.py --matrix banded --sweep [--out probe.jsonl]      # sweep_vs_gather: see that function
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


def _matrix(pkg, name):
    if name == "stencil74":
        return pkg.gen_stencil27(74, 74, 74, 5, magnitude_decades=10.0)
    if name == "stencil111":
        return pkg.gen_stencil27(111, 111, 111, 3, magnitude_decades=10.0)
    if name == "banded":
        return pkg.gen_banded_random(500000, 140, 50000, magnitude_decades=10.0)
    raise SystemExit(f"unknown matrix {name}")


def staged_vs_gather(pkg, B, t, a, name, b, ds, ss, X, Y, n, alg, out):
    """the staged kernel over the pair's shared plan against the gather kernel, alternated on the SAME handles (tuning "tlc" 1 / 0), the
    pair planned with the line budget spmmv_ap_plan_lines(b) at 256 and 512 rows per tile"""
    for tile_rows in (256, 512):
        Pd, Ps = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
        pkg.set_tuning(tlc_tile_rows=tile_rows)
        try:
            tiles, staged = pkg.optimize_ap(Pd, Ps, ds, ss, pkg.spmmv_ap_plan_lines(b))
        finally:
            pkg.set_tuning(tlc_tile_rows=0)
        kind = Pd.plan_info()[0]
        if kind != 1:
            rec = dict(matrix=name, b=b, config="staged_vs_gather", tile_rows=tile_rows, result="not measured", why=f"no shared line plan on the pair (plan kind {kind})")
            print(json.dumps(rec), flush=True)
            if out: out.write(json.dumps(rec) + "\n"); out.flush()
            continue
        for layout in ("rowwise", "colwise_prepared"):
            lay = pkg.ROWWISE if layout == "rowwise" else pkg.COLWISE
            if layout == "colwise_prepared": pkg.spmmv_x_prepared(Pd, X, b, n)
            ts, tg, ts2, tv = [], [], [], []
            for _ in range(a.rounds):
                ts.append(B.time_launches(7, a.reps, A=Pd, B=Ps, x=X, y=Y, b=b, ld=n, layout=lay))
                pkg.set_tuning(tlc=0)
                try:
                    tg.append(B.time_launches(7, a.reps, A=Pd, B=Ps, x=X, y=Y, b=b, ld=n, layout=lay))
                finally:
                    pkg.set_tuning(tlc=1)
                ts2.append(B.time_launches(7, a.reps, A=Pd, B=Ps, x=X, y=Y, b=b, ld=n, layout=lay))
                tv.append(b * B.time_launches(4, a.reps, A=Pd, B=Ps, x=X, y=Y))
            if layout == "colwise_prepared": pkg.spmmv_x_release(Pd)
            ms_s, ms_g, ms_v = float(np.median(ts)), float(np.median(tg)), float(np.median(tv))
            spread = max(ts + ts2) - min(ts + ts2)
            streamed = ds.n_elements * 10 + ss.n_elements * 6 + 24 * ds.n_chunks + 8 * b * n      # values + 16-bit indices, chunk arrays, Y ...
            p = Pd.plan_download()
            streamed += 128 * b * len(p["tile_lines"]) + 4 * len(p["tile_line_ptr"])               # ... and every tile's lines of X rows once
            rec = dict(matrix=name, b=b, config="staged_vs_gather", tile_rows=tile_rows, layout=layout, line_budget=pkg.spmmv_ap_plan_lines(b), max_lines_used=p["max_lines_used"],
                       tiles=tiles, tiles_staged=staged, ms_staged=round(ms_s, 4), ms_gather=round(ms_g, 4), ms_staged_again=round(float(np.median(ts2)), 4),
                       aa_spread_ms=round(spread, 4), gather_over_staged=round(ms_g / ms_s, 3), staged_faster_by_more_than_spread=bool(ms_g - ms_s > spread),
                       ms_b_times_spmv_ap=round(ms_v, 4), speedup_over_b_spmv_ap=round(ms_v / ms_s, 3), beats_b_spmv_ap_by_more_than_spread=bool(ms_v - ms_s > spread),
                       algorithmic_bytes=alg, streamed_bytes=streamed,
                       algorithmic_bytes_over_time_over_8TBs=round(alg / (ms_s * 1e-3) / HBM, 3),
                       streamed_bytes_over_time_over_8TBs=round(streamed / (ms_s * 1e-3) / HBM, 3),
                       ms_rounds=dict(staged=[round(v, 4) for v in ts], gather=[round(v, 4) for v in tg], staged_again=[round(v, 4) for v in ts2]))
            print(json.dumps(rec), flush=True)
            if out: out.write(json.dumps(rec) + "\n"); out.flush()
        del Pd, Ps


def sweep_vs_gather(pkg, B, t, a, name, widths, ds, ss, n, n_cols, out):
    """the block sweep kernel over the pair's column-window sweep plan against the gather kernel and against b x spmv_ap, alternated
    on the SAME handles (tuning "sweep" 1 / 0): (a) spmmv_ap, (g) spmmv_ap with "sweep" 0, (b) b x spmv_ap, (a) once more.  Plans: what
    uspmv_dmat_optimize_ap installs by default (windows of 2^14 doubles: one vector fills the LDS, the block kernel does not apply and
    (a) is (g)); the same planned for two LDS buffers (2^13); and every narrower window at which uspmv_spmmv_ap_sweep_vectors names
    more vectors of this b per pass.  (b0): b x spmv_ap on the DEFAULT plan, the single-vector kernel at its best, measured in the same rounds."""
    D0, S0 = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
    pkg.optimize_ap(D0, S0, ds, ss)
    if D0.plan_info()[0] != 2:
        rec = dict(matrix=name, config="sweep_vs_gather", result="not measured", why=f"optimize_ap installs plan kind {D0.plan_info()[0]}, not the sweep")
        print(json.dumps(rec), flush=True)
        if out: out.write(json.dumps(rec) + "\n"); out.flush()
        return
    for b in widths:
        plans = [("default", 0, 1), ("default, planned for two buffers", 0, 2)]
        for w in (12, 11):          # every narrower window that puts more vectors into a pass, down to the one that takes the most
            if pkg.spmmv_ap_sweep_vectors(b, w) > pkg.spmmv_ap_sweep_vectors(b, w + 1): plans.append((f"wlog {w}", w, 1))
        X = t.ones(b * n, dtype=t.float64, device="cuda"); Y = t.zeros_like(X)
        alg = ds.n_elements * 12 + ss.n_elements * 8 + 16 * ds.n_chunks + 8 * b * (n_cols + n)
        for plan_name, wlog_arg, plan_nbuf in plans:
            Pd, Ps = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
            pkg.set_tuning(sweep_nbuf=plan_nbuf)
            try:
                if wlog_arg: pkg.optimize_sweep_ap(Pd, Ps, ds, ss, wlog_arg, 0)
                else: pkg.optimize_ap(Pd, Ps, ds, ss)
            finally:
                pkg.set_tuning(sweep_nbuf=1)
            meta = Pd.sweep_plan_digest()[1]
            tile_rows, wlog, tiles, swept = int(meta[1]), int(meta[2]), int(meta[4]), int(meta[3])
            for layout in ("rowwise", "colwise"):
                lay = pkg.ROWWISE if layout == "rowwise" else pkg.COLWISE
                path, vec = pkg.spmmv_ap_path(Pd, Ps, b, n, lay)
                ta, tg, tb, tb0, ta2 = [], [], [], [], []
                for _ in range(a.rounds):
                    ta.append(B.time_launches(7, a.reps, A=Pd, B=Ps, x=X, y=Y, b=b, ld=n, layout=lay))
                    pkg.set_tuning(sweep=0)
                    try:
                        tg.append(B.time_launches(7, a.reps, A=Pd, B=Ps, x=X, y=Y, b=b, ld=n, layout=lay))
                    finally:
                        pkg.set_tuning(sweep=1)
                    tb.append(b * B.time_launches(4, a.reps, A=Pd, B=Ps, x=X, y=Y))
                    tb0.append(b * B.time_launches(4, a.reps, A=D0, B=S0, x=X, y=Y))
                    ta2.append(B.time_launches(7, a.reps, A=Pd, B=Ps, x=X, y=Y, b=b, ld=n, layout=lay))
                ms_a, ms_g, ms_b, ms_b0 = (float(np.median(v)) for v in (ta, tg, tb, tb0))
                spread = max(ta + ta2) - min(ta + ta2)
                rec = dict(matrix=name, config="sweep_vs_gather", b=b, layout=layout, plan=plan_name, wlog=wlog, tile_rows=tile_rows, tiles=tiles, tiles_swept=swept,
                           path=path, vectors_per_pass=vec, kernel=("generic", "gather", "staged", "sweep")[path], reps=a.reps, rounds=a.rounds,
                           ms_a_spmmv_ap=round(ms_a, 4), ms_g_spmmv_ap_sweep_off=round(ms_g, 4), ms_b_times_spmv_ap=round(ms_b, 4),
                           ms_b0_times_spmv_ap_default_plan=round(ms_b0, 4), ms_a_again=round(float(np.median(ta2)), 4), aa_spread_ms=round(spread, 4),
                           g_over_a=round(ms_g / ms_a, 3), b_over_a=round(ms_b / ms_a, 3), b0_over_a=round(ms_b0 / ms_a, 3),
                           a_ahead_of_g_by_more_than_spread=bool(ms_g - ms_a > spread), a_ahead_of_b_by_more_than_spread=bool(ms_b - ms_a > spread),
                           a_ahead_of_b0_by_more_than_spread=bool(ms_b0 - ms_a > spread),
                           algorithmic_bytes=alg, algorithmic_bytes_over_time_over_8TBs=round(alg / (ms_a * 1e-3) / HBM, 3),
                           ms_rounds=dict(a=[round(v, 4) for v in ta], g=[round(v, 4) for v in tg], b=[round(v, 4) for v in tb], b0=[round(v, 4) for v in tb0],
                                          a_again=[round(v, 4) for v in ta2]))
                print(json.dumps(rec), flush=True)
                if out: out.write(json.dumps(rec) + "\n"); out.flush()
            del Pd, Ps
        del X, Y
        t.cuda.synchronize()
        t.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", action="append", default=[])
    ap.add_argument("--b", type=int, action="append", default=[])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-unsplit", action="store_true", help="skip (c), the block plan of the unsplit matrix")
    ap.add_argument("--staged", action="store_true", help="also: the staged kernel over the shared plan against the gather kernel on the same handles")
    ap.add_argument("--sweep", action="store_true", help="only: the block sweep kernel over the pair's sweep plan against the gather kernel and b x spmv_ap "
                                                         "on the same handles (sweep_vs_gather; --matrix banded)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    from ultimate_spmv_amd import binding as B
    t.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None
    widths = a.b or [2, 4, 8, 16]
    for name in a.matrix or ["stencil74"]:
        m = _matrix(pkg, name)
        nnz, n_cols = m.nnz, m.n_cols
        dp, sp = pkg.partition_precisions(m, 1e-3)
        ds = pkg.convert_to_scs(dp, 32, 512, pkg.F64)
        perm = ds.arrays()["old_to_new_idx"].copy()
        ss = pkg.convert_to_scs(sp, 32, 512, pkg.F32, fixed_permutation=perm)
        del dp, sp
        pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
        if a.sweep:
            del m
            sweep_vs_gather(pkg, B, t, a, name, widths, ds, ss, ds.n_rows_padded, n_cols, out)
            del ds, ss
            continue
        Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
        pkg.optimize_ap(Ad, As, ds, ss)
        plan_kind = Ad.plan_info()[0]
        lines_used = Ad.plan_download()["max_lines_used"] if plan_kind == 1 else 0
        n = ds.n_rows_padded
        su = None
        if not a.no_unsplit:
            su = pkg.convert_to_scs(m, 32, 512, pkg.F64)
            pkg.permute_scs_cols(su, su.arrays()["old_to_new_idx"])
        del m
        for b in widths:
            Au = None
            if su is not None:
                try:
                    Au = pkg.DeviceMatrix(su, block_tlc=b)
                except pkg.UspmvError as e:                      # (a width the block planner does not take: (c) stays "not measured")
                    print(f"# {name} b={b}: no block plan for the unsplit matrix: {e}", file=sys.stderr, flush=True)
            X = t.ones(b * n, dtype=t.float64, device="cuda"); Y = t.zeros_like(X)
            alg = ds.n_elements * 12 + ss.n_elements * 8 + 16 * ds.n_chunks + 8 * b * (n_cols + n)
            for layout in ("rowwise", "colwise", "colwise_prepared"):
                lay = pkg.ROWWISE if layout == "rowwise" else pkg.COLWISE
                if layout == "colwise_prepared": pkg.spmmv_x_prepared(Ad, X, b, n)
                if layout == "colwise_prepared" and Au is not None: pkg.spmmv_x_prepared(Au, X, b, n)
                ta, tb, tc, td = [], [], [], []
                for _ in range(a.rounds):
                    ta.append(B.time_launches(7, a.reps, A=Ad, B=As, x=X, y=Y, b=b, ld=n, layout=lay))
                    tb.append(b * B.time_launches(4, a.reps, A=Ad, B=As, x=X, y=Y))
                    if Au is not None: tc.append(B.time_launches(5, a.reps, A=Au, x=X, y=Y, b=b, ld=n, layout=lay))
                    td.append(B.time_launches(7, a.reps, A=Ad, B=As, x=X, y=Y, b=b, ld=n, layout=lay))
                if layout == "colwise_prepared":
                    pkg.spmmv_x_release(Ad)
                    if Au is not None: pkg.spmmv_x_release(Au)
                ms_a, ms_b = float(np.median(ta)), float(np.median(tb))
                ms_c = float(np.median(tc)) if tc else None
                spread = max(ta + td) - min(ta + td)
                streamed = alg + (16 * b * n if layout == "colwise" else 0)
                rec = dict(matrix=name, b=b, layout=layout, nnz=nnz, n_rows_padded=n, elements_dp=ds.n_elements, elements_sp=ss.n_elements,
                           single_vector_plan=("none", "tlc", "sweep")[plan_kind], max_lines_used=lines_used,
                           kernel="staged" if plan_kind == 1 and lines_used <= pkg.spmmv_ap_plan_lines(b) else "gather", reps=a.reps, rounds=a.rounds,
                           ms_spmmv_ap=round(ms_a, 4), ms_b_times_spmv_ap=round(ms_b, 4), ms_spmmv_unsplit_dp=round(ms_c, 4) if ms_c else "not measured",
                           ms_spmmv_ap_again=round(float(np.median(td)), 4), aa_spread_ms=round(spread, 4),
                           speedup_over_b_spmv_ap=round(ms_b / ms_a, 3), unsplit_dp_over_spmmv_ap=round(ms_c / ms_a, 3) if ms_c else "not measured",
                           beats_b_spmv_ap_by_more_than_spread=bool(ms_b - ms_a > spread),
                           algorithmic_bytes=alg, hbm_bytes_at_least=streamed, gathered_x_bytes=8 * b * (ds.n_elements + ss.n_elements),
                           algorithmic_bytes_over_time_over_8TBs=round(alg / (ms_a * 1e-3) / HBM, 3),
                           hbm_bytes_at_least_over_time_over_8TBs=round(streamed / (ms_a * 1e-3) / HBM, 3),
                           ms_rounds=dict(a=[round(v, 4) for v in ta], b=[round(v, 4) for v in tb], c=[round(v, 4) for v in tc], d=[round(v, 4) for v in td]))
                line = json.dumps(rec)
                print(line, flush=True)
                if out: out.write(line + "\n"); out.flush()
            if a.staged and pkg.spmmv_ap_plan_lines(b) > 0:
                staged_vs_gather(pkg, B, t, a, name, b, ds, ss, X, Y, n, alg, out)
            del Au, X, Y
            t.cuda.synchronize()
            t.cuda.empty_cache()
        del Ad, As, ds, ss, su
    if out: out.close()


if __name__ == "__main__":
    main()
