#!/usr/bin/env python3
"""Equilibrated adaptive-precision set-up when the matrix is already in HBM as COO arrays, timed in one process:

  equilibration     uspmv_equilibrate_device, HIP events around the whole call (the two memsets of the vectors, the flag word and its
                    read-back are inside: an upper bound of the three kernels' time; their own times come from a rocprofv3 --kernel-trace
                    --stats run of this probe with --no-host).  Bytes: 52 per entry (row pass 12, column pass 16, scaling 24), the gathers
                    of row_max / col_max not counted; that traffic over the call's time as a fraction of what uspmv_stream_copy reaches
                    in the same run.  The atomics the column pass issues after its skip are counted by a diagnostic instantiation of the
                    same kernel (uspmv_equilibrate_device_count_atomics).
  partition         uspmv_partition_precisions_device_eq on the scaled arrays against uspmv_partition_precisions_device on the same arrays
                    (thresholds that split alike), runs interleaved.
  whole route       (a) host: D2H copy of I, J, V -> uspmv_coo_equilibrate_scales -> uspmv_partition_precisions_eq -> uspmv_convert_to_scs of
                    every part (the others with the first part's permutation) -> uspmv_permute_scs_cols -> upload -> device plan;
                    (b) device: uspmv_equilibrate_device -> uspmv_convert_to_scs_device_ap_from_arrays_eq -> the same device plan.
                    Medians of --runs runs of wall time, the device synchronised before the clock is read.

Per (matrix, kind) one JSON line is printed and appended to profiles/ap_equilibrated/probe.jsonl.

    python tools/ap_equilibrate_probe.py --matrix banded --matrix stencil74 [--runs 3] [--kinds dp_sp,dp_sp_hp] [--no-host]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tools.ap_device_setup_probe import _plan, stream_copy_rate  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ap_equilibrated", "probe.jsonl")
EQ_BYTES_PER_ENTRY = 52
PARTITION_BYTES_PER_ENTRY = 48


def host_route(pkg, t, dev, n_rows, n_cols, kind, t1, t2):
    I, J, V = (a.cpu().numpy() for a in dev)
    m = pkg.Coo.from_arrays(n_rows, n_cols, I, J, V)
    del I, J, V
    r, c = m.equilibrate_scales()
    parts = pkg.partition_precisions_eq(m, kind, t1, t2, r, c)
    del m
    dts = [pkg.F64, pkg.F32, pkg.F32 if kind == "dp_sp" else pkg.F16]
    s0 = pkg.convert_to_scs(parts[0], 32, 512, dts[0])
    perm = s0.arrays()["old_to_new_idx"].copy()
    structs = [s0] + [pkg.convert_to_scs(p, 32, 512, dt, fixed_permutation=perm) if p is not None else None for p, dt in zip(parts[1:], dts[1:])]
    del parts
    for s in structs:
        if s is not None:
            pkg.permute_scs_cols(s, perm)
    hand = [pkg.DeviceMatrix(s) if s is not None else None for s in structs]
    plan = _plan(pkg, kind, hand)
    t.cuda.synchronize()
    return hand, plan


def device_route(pkg, t, dev, n_rows, n_cols, kind, t1, t2):
    Vs, r, c = pkg.equilibrate_device(*dev, n_rows, n_cols)
    _, hand, _, _, cnt = pkg.convert_ap_device_from_arrays_eq(dev[0], dev[1], Vs, n_rows, n_cols, 32, 512, kind, t1, t2, r, c, want_layout=False)
    plan = _plan(pkg, kind, hand)
    t.cuda.synchronize()
    return hand, plan, cnt


def timed(t, fn):
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", action="append", default=[])
    ap.add_argument("--kinds", default="dp_sp,dp_sp_hp")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip route (a): for a kernel-trace run of the device side alone")
    ap.add_argument("--out", default=OUT, help="the JSON lines are appended here ('' for none)")
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    t.cuda.set_device(0)
    copy_rate = stream_copy_rate(pkg, t)
    for name in a.matrix or ["banded"]:
        if name == "banded":
            m = pkg.gen_banded_random(500000, 140, 50000, magnitude_decades=10.0)
        elif name == "stencil74":
            m = pkg.gen_stencil27(74, 74, 74, 5, magnitude_decades=8.0)
        else:
            raise SystemExit(f"unknown matrix {name}")
        n_rows, n_cols, nnz = m.n_rows, m.n_cols, m.nnz
        dev = tuple(t.from_numpy(np.array(x)).cuda() for x in m.arrays())
        del m
        gc.collect()
        # equilibration: warm-up, then the runs; the atomics of the column pass on the unscaled values
        Vs, r, c = pkg.equilibrate_device(*dev, n_rows, n_cols)
        eq_ms = [timed(t, lambda: pkg.equilibrate_device(*dev, n_rows, n_cols, out=Vs))[0] for _ in range(max(a.runs, 5))]
        n_atomics = pkg.equilibrate_device_count_atomics(*dev, n_rows, n_cols, r)
        # thresholds of the scaled matrix (quantiles of |v| c r, so that t / (c r) splits 20 / 40 / 40) and of the unscaled partition on the
        # same arrays (quantiles of |v|)
        q = (Vs.abs() * c[dev[1].long()] * r[dev[0].long()]).cpu().numpy()
        t1, t2 = float(np.quantile(q, 0.8)), float(np.quantile(q, 0.4))
        v = Vs.abs().cpu().numpy()
        u1, u2 = float(np.quantile(v, 0.8)), float(np.quantile(v, 0.4))
        del q, v
        sdev = (dev[0], dev[1], Vs)
        ems = float(np.median(eq_ms))
        for kind in a.kinds.split(","):
            part_eq_ms, part_ms, host_s, dev_s = [], [], [], []
            cnt = plan_d = plan_h = None
            pkg.partition_precisions_device_eq(*sdev, n_rows, n_cols, kind, t1, t2, r, c)       # warm-up of both
            pkg.partition_precisions_device(*sdev, n_rows, n_cols, kind, u1, u2)
            for run in range(max(a.runs, 5)):                                                    # interleaved A / B
                part_eq_ms.append(timed(t, lambda: pkg.partition_precisions_device_eq(*sdev, n_rows, n_cols, kind, t1, t2, r, c))[0])
                part_ms.append(timed(t, lambda: pkg.partition_precisions_device(*sdev, n_rows, n_cols, kind, u1, u2))[0])
                gc.collect(); t.cuda.empty_cache()
            for run in range(a.runs):
                if not a.no_host:
                    t.cuda.synchronize(); c0 = time.perf_counter()
                    hand, plan_h = host_route(pkg, t, dev, n_rows, n_cols, kind, t1, t2)
                    host_s.append(time.perf_counter() - c0)
                    del hand
                    gc.collect()
                t.cuda.synchronize(); c0 = time.perf_counter()
                hand, plan_d, cnt = device_route(pkg, t, dev, n_rows, n_cols, kind, t1, t2)
                dev_s.append(time.perf_counter() - c0)
                del hand
                gc.collect(); t.cuda.empty_cache()
                print(f"# {name} {kind} run {run}: host {host_s[-1] if host_s else float('nan'):.3f} s, device {dev_s[-1]:.4f} s", file=sys.stderr, flush=True)
            pe, pu = float(np.median(part_eq_ms)), float(np.median(part_ms))
            rec = dict(matrix=name, kind=kind, n_rows=n_rows, nnz=nnz, t1=t1, t2=t2 if kind == "dp_sp_hp" else None, part_nnz=cnt, runs=a.runs,
                       stream_copy_bytes_per_s=round(copy_rate / 1e12, 3) * 1e12,
                       equilibrate_call_ms=round(ems, 4), equilibrate_call_runs=[round(x, 4) for x in eq_ms], equilibrate_bytes=EQ_BYTES_PER_ENTRY * nnz,
                       equilibrate_call_fraction_of_stream_copy=round(EQ_BYTES_PER_ENTRY * nnz / (ems * 1e-3) / copy_rate, 3),
                       column_atomics_issued=n_atomics, column_atomics_per_entry=round(n_atomics / nnz, 6),
                       partition_eq_call_ms=round(pe, 4), partition_eq_call_runs=[round(x, 4) for x in part_eq_ms],
                       partition_call_ms=round(pu, 4), partition_call_runs=[round(x, 4) for x in part_ms],
                       partition_eq_call_fraction_of_stream_copy=round(PARTITION_BYTES_PER_ENTRY * nnz / (pe * 1e-3) / copy_rate, 3),
                       partition_call_fraction_of_stream_copy=round(PARTITION_BYTES_PER_ENTRY * nnz / (pu * 1e-3) / copy_rate, 3),
                       host_route_s=round(float(np.median(host_s)), 4) if host_s else None, host_route_runs=[round(x, 4) for x in host_s],
                       device_route_s=round(float(np.median(dev_s)), 5), device_route_runs=[round(x, 5) for x in dev_s],
                       plan_tiles_staged_host=plan_h, plan_tiles_staged_device=plan_d)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        del dev, sdev, Vs, r, c
        gc.collect(); t.cuda.empty_cache()


if __name__ == "__main__":
    main()
