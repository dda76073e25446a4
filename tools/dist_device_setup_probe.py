#!/usr/bin/env python3
"""Set-up of one rank's block of the distributed object by its two routes, on ONE GPU in loopback (peer-store exchange: no communicator
is made, so the time is the set-up's own):

  host    DistNative(local_coo, ...)                    uspmv_dist_create_from_coo / _ap_from_coo / _ap_hp_from_coo: every O(nnz) step on the host
  device  DistNative.from_device_arrays(d_I, d_J, d_V)  uspmv_dist_create_from_arrays: every O(nnz) step on the device

Per block one JSON line: wall time of each route as the median of --reps creations after one untimed creation (the block's COO arrays
exist before the clock starts: on the host for the host route, in HBM for the device route), the wall time of the two new calls alone
(uspmv_halo_discover_device on freshly converted handles, uspmv_dmat_chunk_classes_device over the parts), and the device memory the device
route holds at its peak beyond what the finished object keeps -- sampled from hipMemGetInfo every millisecond while the call runs, so
a lower bound.  Both objects pass uspmv_dist_check.

Blocks: 304  block 3 of 8 (seg-rows) of gen:304x304x304, dp
        ap   block 1 of 4 of the 74 x 74 x 296 x 5 dof stencil with 10 decades (the 74^3 x 5 block of DESIGN.md 6.7), as ap[dp_sp] at
             threshold 1e-3 and as ap[dp_sp_hp] at the 0.7 / 0.35 quantiles of |v|

    python tools/dist_device_setup_probe.py [--blocks 304,ap --reps 3 --out profiles/dist_device_setup/probe.jsonl]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def block(pkg, shape, dof, dec, P, rank):
    counts = pkg.gen_stencil27_row_counts(*shape, dof)
    wsa = pkg.seg_from_row_counts(counts, "seg-rows", P)
    return wsa, pkg.gen_stencil27(*shape, dof, magnitude_decades=dec, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))


class PeakUsed:
    """device memory in use, sampled while a call runs"""

    def __init__(self, t):
        self.t, self.peak, self.stop = t, 0, False

    def used(self):
        free, total = self.t.cuda.mem_get_info()
        return total - free

    def __enter__(self):
        self.base = self.peak = self.used()
        self.thread = threading.Thread(target=self.poll, daemon=True)
        self.thread.start()
        return self

    def poll(self):
        while not self.stop:
            self.peak = max(self.peak, self.used())
            time.sleep(0.001)

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()
        self.end = self.used()


def timed(t, make, reps):
    """median wall seconds of `make` (one untimed call first); the last object made"""
    ts, d = [], None
    for k in range(reps + 1):
        if d is not None:
            d.close()
        t.cuda.synchronize()
        t0 = time.perf_counter()
        d = make()
        t.cuda.synchronize()
        if k:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(x, 4) for x in ts], d


def probe(pkg, t, name, wsa, loc, n_cols, rank, P, kw, reps, out):
    C, sigma = 32, 512
    base = dict(comm_rank=0, comm_size=1, exchange="peer", **kw)
    I, J, V = loc.arrays()
    dev = [t.from_numpy(np.array(a)).cuda() for a in (I, J, V)]
    host_s, host_all, dh = timed(t, lambda: pkg.DistNative(loc, wsa, C, sigma, rank, P, None, **base), reps)
    dev_s, dev_all, dd = timed(t, lambda: pkg.DistNative.from_device_arrays(*dev, n_cols, wsa, C, sigma, rank, P, None, **base), reps)
    same = (dh.n_halo, dh.n_send, dh.n_interior, dh.n_boundary, dh.use_tiles) == (dd.n_halo, dd.n_send, dd.n_interior, dd.n_boundary, dd.use_tiles)
    bad = []
    for d in (dh, dd):
        x, y = d.new_x(np.zeros(d.n_local)), d.new_y()
        bad.append(d.check(loc, x, y)[0])
    rec = dict(block=name, kind=kw.get("ap_kind") or ("dp_sp" if "ap_threshold" in kw else "dp"), rows=loc.n_rows, nnz=loc.nnz, n_halo=dd.n_halo,
               units="tiles" if dd.use_tiles else "chunks", host_setup_s=round(host_s, 4), host_setup_all_s=host_all, device_setup_s=round(dev_s, 4),
               device_setup_all_s=dev_all, host_over_device=round(host_s / dev_s, 2), same_meta=same, check_mismatches=bad)
    dh.close(); dd.close()
    # peak device memory of one more creation by the device route, beyond what the object keeps
    t.cuda.synchronize()
    with PeakUsed(t) as mem:
        dd = pkg.DistNative.from_device_arrays(*dev, n_cols, wsa, C, sigma, rank, P, None, **base)
        t.cuda.synchronize()
    rec.update(object_bytes=mem.end - mem.base, peak_extra_bytes_sampled=mem.peak - mem.end,
               table_bytes=8 * max(int(wsa[-1]), n_cols))
    dd.close()
    # the two new calls alone, on handles converted for them
    kind = rec["kind"]
    nl = loc.n_rows
    if kind == "dp":
        parts = [dev]
        dts = [pkg.F64]
    else:
        parts = [p for p in pkg.partition_precisions_device(*dev, nl, n_cols, kind, kw["ap_threshold"], kw.get("ap_threshold_2", 0.0)) if p is not None]
        dts = [pkg.F64, pkg.F32] if kind == "dp_sp" else [pkg.F64, pkg.F32, pkg.F16]
    halo_s, cls_s = [], []
    for k in range(reps + 1):
        _, A0, o2n, _ = pkg.convert_to_scs_device_from_arrays(*parts[0], nl, n_cols, C, sigma, dts[0], permute_cols=False, want_layout=False)
        As = [A0] + [pkg.convert_to_scs_device_from_arrays(*p, nl, n_cols, C, sigma, dt, fixed_permutation=o2n, permute_cols=False, want_layout=False)[1]
                     for p, dt in zip(parts[1:], dts[1:])]
        t.cuda.synchronize()
        t0 = time.perf_counter()
        pkg.halo_discover_device(As, n_cols, wsa, rank, P, o2n)
        t1 = time.perf_counter()
        for A in As:
            A.chunk_classes_device(nl)
        t2 = time.perf_counter()
        if k:
            halo_s.append(t1 - t0); cls_s.append(t2 - t1)
        del As, A0
    rec.update(halo_discover_device_s=round(float(np.median(halo_s)), 5), chunk_classes_device_s=round(float(np.median(cls_s)), 5))
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n"); out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="304,ap")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_device_setup", "probe.jsonl"))
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    t.cuda.set_device(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as out:
        for b in a.blocks.split(","):
            if b == "304":
                wsa, loc = block(pkg, (304, 304, 304), 1, 0.0, 8, 3)
                probe(pkg, t, "gen:304x304x304 block 3 of 8", wsa, loc, 304 ** 3, 3, 8, dict(), a.reps, out)
            elif b in ("ap", "ap_dp_sp", "ap_dp_sp_hp"):
                wsa, loc = block(pkg, (74, 74, 296), 5, 10.0, 4, 1)
                n_cols = 74 * 74 * 296 * 5
                v = np.abs(np.asarray(loc.arrays()[2])[::16])
                name = "gen:74x74x296:5:10 block 1 of 4"
                if b != "ap_dp_sp_hp":
                    probe(pkg, t, name, wsa, loc, n_cols, 1, 4, dict(ap_threshold=1e-3), a.reps, out)
                if b != "ap_dp_sp":
                    probe(pkg, t, name, wsa, loc, n_cols, 1, 4,
                          dict(ap_kind="dp_sp_hp", ap_threshold=float(np.quantile(v, 0.7)), ap_threshold_2=float(np.quantile(v, 0.35))), a.reps, out)
            else:
                raise SystemExit(f"unknown block {b!r}")
            del loc


if __name__ == "__main__":
    main()
