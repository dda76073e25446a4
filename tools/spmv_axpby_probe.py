#!/usr/bin/env python3
"""What the fused update y = alpha A x + beta z (uspmv_spmv_axpby) costs and saves, as JSON lines.

Per configuration -- `stencil` (27-point, --grid^3, the line plan), `elem` (27-point x 3 dof with its nodes renumbered inside blocks: the
element plan on dealt rows), `sweep` (banded-random --n-sweep x 140: the column-window sweep) -- and precision, four legs:
  a  uspmv_spmv alone                                   b  fused residual form (alpha = -1, beta = 1, no dots)
  c  fused with both dots                               d  c's results from uspmv_spmv + torch ops (axpby, two dots, no host sync)
plus a2, the same as a, which gives the A/A spread of the run.  The legs ALTERNATE inside one process: every round times each leg once
(--steps calls between two events, after --warmup), the figure of a leg is the median over --rounds.  `cg` times --cg-iters CG
iterations on the stencil both ways: fused (one call per iteration gives q = A p and <p,q>) and composed (uspmv_spmv + torch.dot).

--ap dp_sp,dp_hp,sp_hp,dp_sp_hp runs the same legs on an adaptive-precision split of each configuration's matrix instead (DESIGN.md 5.13;
thresholds at the 0.7 / 0.35 quantiles of |v|, as in tools/ap_numbering_probe.py; the planner's own choice lines -> elements -> sweep):
a is uspmv_spmv_ap[_hp] alone, b and c uspmv_spmv_ap[_hp]_axpby, d the plain call plus torch ops; `cg` runs on the ap[dp_sp] pair only.

  python tools/spmv_axpby_probe.py --configs stencil,elem,sweep,cg --out profiles/spmv_axpby/probe.jsonl
  python tools/spmv_axpby_probe.py --ap dp_sp,dp_hp,sp_hp,dp_sp_hp --configs stencil,elem,sweep,cg --out profiles/spmv_ap_axpby/probe.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def renumbered(pkg, g, dof, Kb):
    base = pkg.gen_stencil27(g, g, g, dof=dof)
    I0, J0, V0 = (np.array(v) for v in base.arrays())
    n = base.n_rows
    rng = np.random.default_rng(7)
    pn = np.arange(n // dof, dtype=np.int64)
    for s0 in range(0, pn.size, Kb):
        seg = pn[s0:s0 + Kb].copy(); rng.shuffle(seg); pn[s0:s0 + Kb] = seg
    I1 = (pn[I0 // dof] * dof + I0 % dof).astype(np.int32); J1 = (pn[J0 // dof] * dof + J0 % dof).astype(np.int32)
    o = np.lexsort((J1, I1))
    return pkg.Coo.from_arrays(n, n, I1[o], J1[o], V0[o])


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="stencil,elem,sweep,cg")
    ap.add_argument("--precisions", default="dp,sp")
    ap.add_argument("--grid", type=int, default=253)
    ap.add_argument("--grid-elem", type=int, default=80)
    ap.add_argument("--n-sweep", type=int, default=500000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cg-iters", type=int, default=50)
    ap.add_argument("--ap", default="", help="comma-separated kinds of adaptive-precision splits to run instead of the one-precision handles")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    def handle(coo, dtype):
        s = pkg.convert_to_scs(coo, 32, 512, dtype)
        pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"])
        return s, pkg.DeviceMatrix(s, "cuda:0", tlc=True)

    def split(coo, kind):
        """the handles [first, mid | None, last] of one split with its planner's plan, and the first part's struct"""
        a = np.abs(np.asarray(coo.arrays()[2])); a = a[a > 0]
        t1, t2 = float(np.quantile(a, 0.7)), float(np.quantile(a, 0.35))
        if kind in ("dp_hp", "sp_hp"):
            t1 = min(t1, 6e4)                                # (what goes to binary16 stays under its largest finite value)
        t2 = min(t2, 6e4)
        if kind == "dp_sp":
            hi, lo = pkg.partition_precisions(coo, t1); mid = None
        else:
            hi, mid, lo = pkg.partition_precisions_hp(coo, kind, t1, t2)
        sh = pkg.convert_to_scs(hi, 32, 512, pkg.F32 if kind == "sp_hp" else pkg.F64)
        perm = sh.arrays()["old_to_new_idx"].copy()
        sm = pkg.convert_to_scs(mid, 32, 512, pkg.F32, fixed_permutation=perm) if mid is not None else None
        sl = pkg.convert_to_scs(lo, 32, 512, pkg.F32 if kind == "dp_sp" else pkg.F16, fixed_permutation=perm)
        ss = [sh, sm, sl]
        for st in ss:
            if st is not None:
                pkg.permute_scs_cols(st, perm)
        hs = [pkg.DeviceMatrix(st, "cuda:0") if st is not None else None for st in ss]
        if kind == "dp_sp":
            pkg.optimize_ap(hs[0], hs[2], sh, sl)
        else:
            pkg.optimize_ap_hp(hs[0], hs[1], hs[2], sh, sm, sl)
        return sh, hs, [st.nnz if st is not None else None for st in ss]

    kinds = [k for k in args.ap.split(",") if k]
    for cfg in [c for c in args.configs.split(",") if c]:
        if cfg in ("stencil", "cg"):
            coo = pkg.gen_stencil27(args.grid, args.grid, args.grid)
        elif cfg == "elem":
            coo = renumbered(pkg, args.grid_elem, 3, 20000)
        elif cfg == "sweep":
            coo = pkg.gen_banded_random(args.n_sweep, 140, 50000, magnitude_decades=10.0)
        else:
            raise SystemExit(f"unknown configuration {cfg!r}")
        for prec in (kinds if kinds else args.precisions.split(",")):
            if kinds and cfg == "cg" and prec != "dp_sp":
                continue
            if kinds:
                td = torch.float32 if prec == "sp_hp" else torch.float64
                s, hs, part_nnz = split(coo, prec)
                A = hs[0]
                if prec == "dp_sp":
                    spmv = lambda x_, y_: pkg.spmv_ap(hs[0], hs[2], x_, y_)
                    axpby = lambda x_, y_, *a_, **kw: pkg.spmv_ap_axpby(hs[0], hs[2], x_, y_, *a_, **kw)
                    reserve, path_of = (lambda: pkg.ap_axpby_reserve(hs[0], hs[2])), (lambda x_: pkg.spmv_ap_axpby_path(hs[0], hs[2], x_))
                else:
                    spmv = lambda x_, y_: pkg.spmv_ap_hp(hs[0], hs[1], hs[2], x_, y_)
                    axpby = lambda x_, y_, *a_, **kw: pkg.spmv_ap_hp_axpby(hs[0], hs[1], hs[2], x_, y_, *a_, **kw)
                    reserve, path_of = (lambda: pkg.ap_hp_axpby_reserve(*hs)), (lambda x_: pkg.spmv_ap_hp_axpby_path(hs[0], hs[1], hs[2], x_))
            else:
                dtype, td = (pkg.F64, torch.float64) if prec == "dp" else (pkg.F32, torch.float32)
                s, A = handle(coo, dtype)
                hs, part_nnz = None, None
                spmv = lambda x_, y_: pkg.spmv(A, x_, y_)
                axpby = lambda x_, y_, *a_, **kw: pkg.spmv_axpby(A, x_, y_, *a_, **kw)
                reserve, path_of = A.axpby_reserve, (lambda x_: pkg.spmv_axpby_path(A, x_))
            n, npad = s.n_rows, s.n_rows_padded
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.rand(npad, dtype=td, device="cuda", generator=g)
            b = torch.rand(npad, dtype=td, device="cuda", generator=g)
            w = torch.rand(npad, dtype=td, device="cuda", generator=g)
            y = torch.zeros(npad, dtype=td, device="cuda")
            dots = torch.zeros(2, dtype=torch.float64, device="cuda")
            reserve()
            base = {"config": cfg, "precision": prec, "n_rows": n, "nnz": s.nnz if not kinds else sum(v for v in part_nnz if v), "plan_kind": A.plan_info()[0],
                    "granularity": A.plan_granularity(), "rows_dealt": int(A.plan_rows_dealt()), "path": path_of(x)}
            if kinds:
                base["part_nnz"] = part_nnz
            if cfg == "cg":
                d1, acc = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")

                def cg(fused):
                    # the memory traffic of CG's inner loop, without the host round trip for the step lengths (fixed ones: this times the passes)
                    p, r, q, xx = x.clone(), b.clone(), y, torch.zeros_like(x)
                    for _ in range(args.cg_iters):
                        if fused:
                            axpby(p, q, 1.0, 0.0, w=p, dots=d1, n_dot_rows=n)        # q = A p, <q,q>, <p,q>
                        else:
                            spmv(p, q)
                            acc.copy_(torch.dot(p[:n].double(), q[:n].double()).reshape(1))
                        xx.add_(p, alpha=1e-3); r.add_(q, alpha=-1e-3)
                        acc.copy_(torch.dot(r[:n].double(), r[:n].double()).reshape(1))
                        p.mul_(0.5).add_(r)
                legs = {"cg_fused": lambda: cg(True), "cg_composed": lambda: cg(False), "cg_composed_2": lambda: cg(False)}
                steps, warm = 1, 1
            else:
                def leg_d():
                    spmv(x, y)
                    y.mul_(-1.0).add_(b)
                    dots[0:1].copy_(torch.dot(y[:n].double(), y[:n].double()).reshape(1))
                    dots[1:2].copy_(torch.dot(w[:n].double(), y[:n].double()).reshape(1))
                legs = {"a": lambda: spmv(x, y), "b": lambda: axpby(x, y, -1.0, 1.0, z=b),
                        "c": lambda: axpby(x, y, -1.0, 1.0, z=b, w=w, dots=dots, n_dot_rows=n), "d": leg_d,
                        "a2": lambda: spmv(x, y)}
                steps, warm = args.steps, args.warmup
            times = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    times[k].append(timed(torch, fn, steps, warm))
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = dict(base, ms={k: round(v, 5) for k, v in med.items()}, ms_min={k: round(min(v), 5) for k, v in times.items()},
                       rounds=args.rounds, steps=steps)
            if cfg == "cg":
                rec["aa_spread"] = round(abs(med["cg_composed"] - med["cg_composed_2"]) / med["cg_composed"], 4)
                rec["fused_over_composed"] = round(med["cg_fused"] / med["cg_composed"], 4)
            else:
                rec["aa_spread"] = round(abs(med["a"] - med["a2"]) / med["a"], 4)
                rec["fused_over_composed"] = round(med["c"] / med["d"], 4)
                rec["fused_dots_over_spmv"] = round(med["c"] / med["a"], 4)
                rec["fused_residual_over_spmv"] = round(med["b"] / med["a"], 4)
            emit(rec)
            del A, hs, s, x, b, w, y
            torch.cuda.empty_cache()
        del coo


if __name__ == "__main__":
    main()
