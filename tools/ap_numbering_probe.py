#!/usr/bin/env python3
"""Adaptive-precision SpMV when x is numbered differently from the rows: the shared plan over single x elements against what the split runs
without it.  The matrices are those of tools/numbering_probe.py with NUMBERING_COLS_ONLY=1 -- the 27-point x 3 dof stencil on g^3 nodes with
the COLUMNS' nodes renumbered at random inside consecutive blocks of K nodes, SELL-32-512 -- split at quantiles of |v| into the parts of
ap[dp_sp], ap[dp_sp_hp], ap[dp_hp] and ap[sp_hp].

Per (K, kind), one JSON line: which plan every handle got under "tlc_elem" 2 (the element plan wherever the policy admits it), 1 (the
default) and 0 (lines, then the sweep: what the planners did before the element plan existed for splits); the SpMV of the handles planned
under 2 and under 0 timed in turn in one process (HIP events around REPS launches, ROUNDS alternating rounds after a warm-up; min, median
and the spread (max - min) / min of each side); the fraction of the 8 TB/s roofline in algorithmic bytes (every stored entry its value and a
4-byte column index, 8 bytes per chunk and part, x once, y once); both y bit-identical to the planless lane-per-row kernels; and the set-up
time of the host and of the device planner under either setting.

usage: ap_numbering_probe.py [g = 80] [K,K,... = 1000,5000,20000] [kind,kind,... = dp_sp,dp_sp_hp,dp_hp,sp_hp]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge
pkg = ge.load_package()
torch.cuda.set_device(0)
g = int(sys.argv[1]) if len(sys.argv) > 1 else 80
Ks = [int(k) for k in (sys.argv[2] if len(sys.argv) > 2 else "1000,5000,20000").split(",")]
kinds = (sys.argv[3] if len(sys.argv) > 3 else "dp_sp,dp_sp_hp,dp_hp,sp_hp").split(",")
REPS, ROUNDS = int(os.environ.get("AP_PROBE_REPS", "40")), int(os.environ.get("AP_PROBE_ROUNDS", "5"))
dof, C_, sigma = 3, 32, 512
VAL_BYTES = {pkg.F64: 8, pkg.F32: 4, pkg.F16: 2}

base = pkg.gen_stencil27(g, g, g, dof=dof)
I0, J0, V0 = (np.array(a) for a in base.arrays())
n = base.n_rows
del base
absv = np.abs(V0)
T1, T2 = float(np.quantile(absv, 0.7)), float(np.quantile(absv, 0.35))      # 30 % / 35 % / 35 % of the entries (two parts: 30 % / 70 %)
del absv
rng = np.random.default_rng(7)


def split(m, kind):
    if kind == "dp_sp":
        hi, lo = pkg.partition_precisions(m, T1)
        mid = None
    else:
        hi, mid, lo = pkg.partition_precisions_hp(m, kind, T1, T2)
    sh = pkg.convert_to_scs(hi, C_, sigma, pkg.F32 if kind == "sp_hp" else pkg.F64)
    perm = sh.arrays()["old_to_new_idx"].copy()
    sm = pkg.convert_to_scs(mid, C_, sigma, pkg.F32, fixed_permutation=perm) if mid is not None else None
    sl = pkg.convert_to_scs(lo, C_, sigma, pkg.F32 if kind == "dp_sp" else pkg.F16, fixed_permutation=perm)
    return [sh, sm, sl]


def planned(kind, structs, elem, device):
    """handles planned under "tlc_elem" = elem by the host or the device planner; (handles, set-up ms)"""
    hand = [pkg.DeviceMatrix(s) if s is not None else None for s in structs]
    torch.cuda.synchronize()
    pkg.set_tuning(tlc_elem=elem)
    try:
        t0 = time.perf_counter()
        if kind == "dp_sp":
            pkg.optimize_device_ap(hand[0], hand[2]) if device else pkg.optimize_ap(hand[0], hand[2], structs[0], structs[2])
        elif device:
            pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2])
        else:
            pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
        torch.cuda.synchronize()
        return hand, (time.perf_counter() - t0) * 1e3
    finally:
        pkg.set_tuning(tlc_elem=1)


def launch(kind, hand, x, y):
    if kind == "dp_sp":
        pkg.spmv_ap(hand[0], hand[2], x, y)
    else:
        pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y)


def timed(kind, hand, x, y):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        launch(kind, hand, x, y)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def plan_of(hand):
    names = {0: "none", 1: "tlc", 2: "sweep"}
    return [dict(plan=names[h.plan_info()[0]], tiles=h.plan_info()[1], planned=h.plan_info()[2], elements_per_list_entry=h.plan_granularity())
            for h in hand if h is not None]


def stats(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), spread=round((max(v) - min(v)) / min(v), 4))


for K in Ks:
    nn = n // dof
    p = np.arange(nn, dtype=np.int64)
    for s0 in range(0, nn, K):
        seg = p[s0:s0 + K].copy(); rng.shuffle(seg); p[s0:s0 + K] = seg
    pcol = (p[J0 // dof] * dof + J0 % dof).astype(np.int32)
    o = np.lexsort((pcol, I0))
    m = pkg.Coo.from_arrays(n, n, I0[o], pcol[o], V0[o])
    del pcol, o
    for kind in kinds:
        structs = split(m, kind)
        parts = [s for s in structs if s is not None]
        npad, nch = parts[0].n_rows_padded, parts[0].n_chunks
        xdt = torch.float32 if kind == "sp_hp" else torch.float64
        xb = 4 if kind == "sp_hp" else 8
        x = torch.rand(max(npad, n), dtype=xdt, device="cuda")
        ys = [torch.zeros(npad, dtype=xdt, device="cuda") for _ in range(3)]
        pkg.set_tuning(tlc=0, sweep=0)                      # the yardstick: planless lane-per-row kernels
        try:
            launch(kind, [pkg.DeviceMatrix(s) if s is not None else None for s in structs], x, ys[2])
            torch.cuda.synchronize()
        finally:
            pkg.set_tuning(tlc=1, sweep=1)
        He, host_ms_e = planned(kind, structs, 2, False)
        H0, host_ms_0 = planned(kind, structs, 0, False)
        H1, _ = planned(kind, structs, 1, False)
        De, dev_ms_e = planned(kind, structs, 2, True)
        D0, dev_ms_0 = planned(kind, structs, 0, True)
        launch(kind, He, x, ys[0]); launch(kind, H0, x, ys[1]); torch.cuda.synchronize()
        same = bool(torch.equal(ys[0], ys[2])) and bool(torch.equal(ys[1], ys[2]))
        launch(kind, De, x, ys[0]); torch.cuda.synchronize()
        same_dev = bool(torch.equal(ys[0], ys[2]))
        for _ in range(2):                                  # warm-up of both sides
            timed(kind, He, x, ys[0]); timed(kind, H0, x, ys[1])
        te, t0 = [], []
        for _ in range(ROUNDS):                             # alternating A/B
            te.append(timed(kind, He, x, ys[0])); t0.append(timed(kind, H0, x, ys[1]))
        byts = sum(s.n_elements * (VAL_BYTES[s.dtype] + 4) + 8 * nch for s in parts) + xb * n + xb * npad
        fr = lambda ms: round(byts / ms / 1e6 / 8000, 3)
        print(json.dumps(dict(g=g, K=K, kind=kind, n=n, nnz=int(sum(s.nnz for s in parts)), algorithmic_bytes=int(byts),
                              plan_tlc_elem_2=plan_of(He), plan_tlc_elem_1=plan_of(H1), plan_tlc_elem_0=plan_of(H0),
                              device_plan_tlc_elem_2=plan_of(De), device_plan_tlc_elem_0=plan_of(D0),
                              bitexact=same, bitexact_device_planned=same_dev,
                              ms_tlc_elem_2=stats(te), ms_tlc_elem_0=stats(t0), frac_tlc_elem_2=fr(min(te)), frac_tlc_elem_0=fr(min(t0)),
                              speedup_min=round(min(t0) / min(te), 3), speedup_median=round(statistics.median(t0) / statistics.median(te), 3),
                              setup_ms=dict(host_tlc_elem_2=round(host_ms_e, 1), host_tlc_elem_0=round(host_ms_0, 1),
                                            device_tlc_elem_2=round(dev_ms_e, 1), device_tlc_elem_0=round(dev_ms_0, 1)))), flush=True)
        del He, H0, H1, De, D0, structs, parts, x, ys
    del m
