#!/usr/bin/env python3
"""The distributed adaptive-precision BLOCK step (uspmv_dist_spmmv_ap) on ONE GPU in loopback, against what a caller had before it.

The protocol of tools/dist_ap_probe.py.  Matrix: 27-point stencil, 5 dof, magnitudes over 10 decades, threshold 1e-3, SELL-32-512;
block 1 of P = 4 of 74 x 74 x 296 nodes (seg-rows): the 74^3 x 5 matrix (2 026 120 rows).  Per (b, layout) the arms are alternated in
one process, each round = `steps` eager steps between two HIP events on the object's stream after 3 untimed steps of the same arm:

  (a) uspmv_dist_spmmv_ap in its default form (overlap, "pad_split" 1)
  (b) uspmv_dist_spmmv_ap with "overlap" 0 (the exchange, then uspmv_spmmv_ap on the block)
  (c) b x uspmv_dist_spmv on the same ap object, one column after the other -- what a caller did before the block step existed
  (d) uspmv_dist_spmmv on the one-precision dp object of the same block, in its default form

All exchanges bulkvec.  One JSON line per (b, layout): medians and spreads (max - min over the rounds) in ms per block step, which
kernel the tile lists take (uspmv_spmmv_ap_tiles_path), and whether (a) is ahead of each other arm by more than twice that arm's spread.
--arms c runs arm (c) alone: it uses nothing newer than the single-vector ap step, so it also runs on a checkout that has no block step.
Loopback exchanges are RCCL self send / recv on one GPU, not links: N > 1 GPUs stay unmeasured, and no default follows from these numbers.

    python tools/dist_ap_spmmv_probe.py [--rounds 5 --steps 20 --b 4 8 --arms abcd --out profiles/dist_ap_spmmv/probe.jsonl]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

THR = 1e-3
COL, ROW = 0, 1


def block(pkg, shape, dof, dec, P, rank):
    counts = pkg.gen_stencil27_row_counts(*shape, dof)
    wsa = pkg.seg_from_row_counts(counts, "seg-rows", P)
    return wsa, pkg.gen_stencil27(*shape, dof, magnitude_decades=dec, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=74, help="the block is nodes^3 x 5 dof (74: the size the README quotes)")
    ap.add_argument("--b", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--arms", default="abcd")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    assert t.cuda.is_available(), "dist_ap_spmmv_probe needs a GPU"
    t.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None
    P, rank, C, sigma, dof, dec = 4, 1, 32, 512, 5, 10.0
    shape = (a.nodes, a.nodes, a.nodes * P)
    t0 = time.perf_counter()
    wsa, loc = block(pkg, shape, dof, dec, P, rank)
    nl = int(wsa[rank + 1] - wsa[rank])
    d_ap = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_threshold=THR)
    d_dp = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1) if "d" in a.arms else None
    setup_s = time.perf_counter() - t0
    xo = 1.0 + 1e-3 * (np.arange(nl) % 1000)
    bad_ap = d_ap.check(loc, d_ap.new_x(xo), d_ap.new_y())[0]
    ld = d_ap.padded_vec_size
    pair = (SimpleNamespace(h=d_ap._A), SimpleNamespace(h=d_ap._A_sp))

    def timed(d, fn):
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        fn(3); d.synchronize()
        e0.record(d.stream); fn(a.steps); e1.record(d.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for b in a.b:
        cols = [xo * (1.0 + (v % 8) / 8.0) for v in range(b)]
        for layout in (COL, ROW):
            X = d_ap.new_X(cols, b, layout)
            Y = t.zeros(b * ld, dtype=t.float64, device="cuda")
            xs = [d_ap.new_x(c) for c in cols]
            ys = [d_ap.new_y() for _ in cols]
            if d_dp is not None:
                assert d_dp.padded_vec_size == ld
                Xd = d_dp.new_X(cols, b, layout)
                Yd = t.zeros(b * ld, dtype=t.float64, device="cuda")

            def arm_a(n):
                d_ap.set_option("overlap", 1)
                for _ in range(n):
                    d_ap.spmmv_ap(X, Y, b, layout)

            def arm_b(n):
                d_ap.set_option("overlap", 0)
                for _ in range(n):
                    d_ap.spmmv_ap(X, Y, b, layout)
                d_ap.set_option("overlap", 1)

            def arm_c(n):
                for _ in range(n):
                    for x, y in zip(xs, ys):
                        d_ap.spmv(x, y)

            def arm_d(n):
                for _ in range(n):
                    d_dp.spmmv(Xd, Yd, b, layout)

            arms = dict(a=(d_ap, arm_a), b=(d_ap, arm_b), c=(d_ap, arm_c), d=(d_dp, arm_d))
            ms = {k: [] for k in a.arms}
            for _ in range(a.rounds):
                for k in a.arms:
                    ms[k].append(timed(*arms[k]))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
            rec = dict(config="block step", label=a.label, matrix="gen:%dx%dx%d:%d:%g block %d of %d" % (*shape, dof, dec, rank, P), threshold_1=THR, C=C,
                       sigma=sigma, n_local=nl, n_halo=d_ap.n_halo, b=b, layout="row-wise" if layout == ROW else "column-wise", mode="bulkvec",
                       rounds=a.rounds, steps=a.steps, timing="HIP events on the object's stream around eager steps; ms per block step",
                       self_check_mismatches_ap=bad_ap, ms={k: round(v, 4) for k, v in med.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                       ms_rounds={k: [round(v, 4) for v in vs] for k, vs in ms.items()}, setup_s=round(setup_s, 1))
            if hasattr(pkg, "spmmv_ap_tiles_path") and d_ap.use_tiles:
                rec["tiles_path"] = list(pkg.spmmv_ap_tiles_path(pair[0], pair[1], b, ld, layout))
            if "a" in med:
                rec["a_ahead_by_more_than_twice_the_spreads"] = {k: bool(med[k] - med["a"] > 2 * max(spread[k], spread["a"])) for k in med if k != "a"}
                rec["a_behind_by_more_than_twice_the_spreads"] = {k: bool(med["a"] - med[k] > 2 * max(spread[k], spread["a"])) for k in med if k != "a"}
            if "a" in med or "b" in med:
                rec["steps_counted"] = d_ap.spmmv_info()
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()
            del X, Y, xs, ys
    d_ap.close()
    if d_dp is not None:
        d_dp.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
