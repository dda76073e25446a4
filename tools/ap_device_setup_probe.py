#!/usr/bin/env python3
"""Adaptive-precision set-up when the matrix is already in HBM as COO arrays: the route through the host against the set-up on the device,
timed in one process, for ap[dp_sp] and ap[dp_sp_hp].

  (a) host route     D2H copy of I, J, V -> uspmv_partition_precisions[_hp] -> uspmv_convert_to_scs of every part (the others with the first
                     part's permutation) -> uspmv_permute_scs_cols -> upload -> device plan (uspmv_dmat_optimize_device_ap[_hp])
  (b) device route   uspmv_convert_to_scs_device_ap_from_arrays -> the same device plan

Each is the median of --runs runs of wall time, the device synchronised before the clock is read; of route (b) the one-call set-up
(partition + conversions) is also timed by itself, the rest being the device planner both routes share.  Per (matrix, kind) one JSON line is
printed and appended to profiles/ap_device_setup/probe.jsonl.  Also in the line: the partition alone (uspmv_partition_precisions_device,
HIP events around the whole call, so the allocations of the parts, the scan and the two small read-backs are inside: an upper bound of the
three kernels' time; their own times come from a rocprofv3 --kernel-trace --stats run of this probe), the bytes its two passes move (48
per entry: 16 read by the counting pass, 16 read and 16 written by the scatter) and that traffic over the call's time as a fraction of
the rate uspmv_stream_copy reaches in the same run.

    python tools/ap_device_setup_probe.py --matrix banded --matrix stencil74 [--runs 5] [--kinds dp_sp,dp_sp_hp] [--no-host]
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

OUT = os.path.join(ROOT, "profiles", "ap_device_setup", "probe.jsonl")
PARTITION_BYTES_PER_ENTRY = 48


def _plan(pkg, kind, hand):
    if kind == "dp_sp":
        return pkg.optimize_device_ap(hand[0], hand[2])
    return pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2])


def host_route(pkg, t, dev, n_rows, n_cols, kind, t1, t2):
    I, J, V = (a.cpu().numpy() for a in dev)
    m = pkg.Coo.from_arrays(n_rows, n_cols, I, J, V)
    del I, J, V
    if kind == "dp_sp":
        dp, sp = pkg.partition_precisions(m, t1)
        parts, dts = [dp, None, sp], [pkg.F64, pkg.F32, pkg.F32]
    else:
        parts, dts = list(pkg.partition_precisions_hp(m, kind, t1, t2)), [pkg.F64, pkg.F32, pkg.F16]
    del m
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
    c0 = time.perf_counter()
    _, hand, _, _, cnt = pkg.convert_ap_device_from_arrays(*dev, n_rows, n_cols, 32, 512, kind, t1, t2, want_layout=False)
    t.cuda.synchronize()
    convert_s = time.perf_counter() - c0                   # partition + conversions; the rest of the route is the device planner
    plan = _plan(pkg, kind, hand)
    t.cuda.synchronize()
    return hand, plan, cnt, convert_s


def stream_copy_rate(pkg, t, n=1 << 27):
    a = t.empty(n, dtype=t.float64, device="cuda"); b = t.ones(n, dtype=t.float64, device="cuda")
    st = t.cuda.current_stream().cuda_stream
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    rates = []
    for _ in range(5):
        e0.record()
        for _ in range(5):
            rc = pkg.lib().uspmv_stream_copy(a.data_ptr(), b.data_ptr(), n, st)
            assert rc == 0
        e1.record(); e1.synchronize()
        rates.append(5 * 16.0 * n / (e0.elapsed_time(e1) * 1e-3))
    return float(np.median(rates))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", action="append", default=[])
    ap.add_argument("--kinds", default="dp_sp,dp_sp_hp")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip route (a): for a kernel-trace run of the device route alone")
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
        I, J, V = m.arrays()
        v = np.abs(np.asarray(V))
        t1, t2 = float(np.quantile(v, 0.8)), float(np.quantile(v, 0.4))
        del v
        dev = tuple(t.from_numpy(np.array(x)).cuda() for x in (I, J, V))
        del I, J, V, m
        for kind in a.kinds.split(","):
            host_s, dev_s, conv_s, part_ms = [], [], [], []
            cnt = plan_d = plan_h = None
            for run in range(a.runs):
                if not a.no_host:
                    t.cuda.synchronize(); c0 = time.perf_counter()
                    hand, plan_h = host_route(pkg, t, dev, n_rows, n_cols, kind, t1, t2)
                    host_s.append(time.perf_counter() - c0)
                    del hand
                    gc.collect()
                t.cuda.synchronize(); c0 = time.perf_counter()
                hand, plan_d, cnt, cs = device_route(pkg, t, dev, n_rows, n_cols, kind, t1, t2)
                dev_s.append(time.perf_counter() - c0); conv_s.append(cs)
                del hand
                e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
                e0.record()
                parts = pkg.partition_precisions_device(*dev, n_rows, n_cols, kind, t1, t2)
                e1.record(); e1.synchronize()
                part_ms.append(e0.elapsed_time(e1))
                del parts
                gc.collect(); t.cuda.empty_cache()
                print(f"# {name} {kind} run {run}: host {host_s[-1] if host_s else float('nan'):.3f} s, device {dev_s[-1]:.4f} s (set-up call {conv_s[-1]:.4f} s), partition call {part_ms[-1]:.3f} ms",
                      file=sys.stderr, flush=True)
            pms = float(np.median(part_ms))
            rec = dict(matrix=name, kind=kind, n_rows=n_rows, nnz=nnz, t1=t1, t2=t2 if kind == "dp_sp_hp" else None, part_nnz=cnt, runs=a.runs,
                       host_route_s=round(float(np.median(host_s)), 4) if host_s else None, host_route_runs=[round(x, 4) for x in host_s],
                       device_route_s=round(float(np.median(dev_s)), 5), device_route_runs=[round(x, 5) for x in dev_s],
                       device_setup_call_s=round(float(np.median(conv_s)), 5), device_setup_call_runs=[round(x, 5) for x in conv_s],
                       plan_tiles_staged_host=plan_h, plan_tiles_staged_device=plan_d,
                       partition_call_ms=round(pms, 4), partition_call_runs=[round(x, 4) for x in part_ms],
                       partition_bytes=PARTITION_BYTES_PER_ENTRY * nnz, stream_copy_bytes_per_s=round(copy_rate / 1e12, 3) * 1e12,
                       partition_call_fraction_of_stream_copy=round(PARTITION_BYTES_PER_ENTRY * nnz / (pms * 1e-3) / copy_rate, 3))
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        del dev
        gc.collect(); t.cuda.empty_cache()


if __name__ == "__main__":
    main()
