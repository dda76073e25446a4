#!/usr/bin/env python3
"""The distributed BLOCK step of the adaptive-precision kinds with an fp16 part (uspmv_dist_spmmv_ap_hp) on ONE GPU in loopback, against
what a caller had before it.

The protocol of tools/dist_ap_spmmv_probe.py and the thresholds of tools/dist_ap_probe.py --kind.  Matrix: 27-point stencil, 5 dof,
magnitudes over 10 decades, SELL-32-512; block 1 of P = 4 of 74 x 74 x 296 nodes (seg-rows): the 74^3 x 5 matrix (2 026 120 rows);
thresholds at the 0.7 / 0.35 quantiles of |v| of every 16th entry of the block.  Per (kind, b, layout) the arms are alternated in one
process, each round = `steps` eager steps between two HIP events on the object's stream after 3 untimed steps of the same arm:

  (a) uspmv_dist_spmmv_ap_hp in its default form (overlap, "pad_split" 1)
  (b) uspmv_dist_spmmv_ap_hp with "overlap" 0 (the exchange, then uspmv_spmmv_ap_hp on the block)
  (c) b x uspmv_dist_spmv on the same object, one column after the other -- what a caller did before the block step existed
  (d) uspmv_dist_spmmv_ap on the ap[dp_sp] object of the same block at the upper threshold, in its default form
  (e) arm (a) under tuning "tlc" 0: the same lists forced to the lane-per-row kernel -- on a block whose padded_vec_size leaves the
      columns off the 16-byte grid, (e) against (a) column-wise is what the narrow-piece staging buys

All exchanges bulkvec.  One JSON line per (kind, b, layout): medians and spreads (max - min over the rounds) in ms per block step, which
kernel the tile lists take in every arm (uspmv_spmmv_ap_hp_tiles_path / uspmv_spmmv_ap_tiles_path), and whether (a) is ahead of or behind
each other arm by more than twice the larger spread.
--arms c runs arm (c) alone: it uses nothing newer than the single-vector step, so it also runs on a checkout that has no block step.
Loopback exchanges are RCCL self send / recv on one GPU, not links: N > 1 GPUs stay unmeasured, and no default follows from these numbers.

    python tools/dist_ap_hp_spmmv_probe.py [--kind dp_sp_hp sp_hp --rounds 5 --steps 20 --b 4 8 --arms abcde
                                            --out profiles/dist_ap_hp_spmmv/probe.jsonl]
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

COL, ROW = 0, 1


def block(pkg, shape, dof, dec, P, rank):
    counts = pkg.gen_stencil27_row_counts(*shape, dof)
    wsa = pkg.seg_from_row_counts(counts, "seg-rows", P)
    return wsa, pkg.gen_stencil27(*shape, dof, magnitude_decades=dec, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", nargs="+", default=["dp_sp_hp", "sp_hp"], choices=("dp_hp", "sp_hp", "dp_sp_hp"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=74, help="the block is nodes^3 x 5 dof (74: the size the README quotes)")
    ap.add_argument("--b", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--arms", default="abcde")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    assert t.cuda.is_available(), "dist_ap_hp_spmmv_probe needs a GPU"
    t.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None
    P, rank, C, sigma, dof, dec = 4, 1, 32, 512, 5, 10.0
    shape = (a.nodes, a.nodes, a.nodes * P)
    wsa, loc = block(pkg, shape, dof, dec, P, rank)
    nl = int(wsa[rank + 1] - wsa[rank])
    av = np.abs(np.asarray(loc.arrays()[2])[::16])
    t1, t2 = float(np.quantile(av, 0.7)), float(np.quantile(av, 0.35))
    mk = dict(comm_rank=0, comm_size=1)
    xo = 1.0 + 1e-3 * (np.arange(nl) % 1000)
    d_ap = None
    if "d" in a.arms:
        d_ap = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), ap_threshold=t1, **mk)
        pair = (SimpleNamespace(h=d_ap._A), SimpleNamespace(h=d_ap._A_sp))

    def timed(d, fn):
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        fn(3); d.synchronize()
        e0.record(d.stream); fn(a.steps); e1.record(d.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for kind in a.kind:
        t0 = time.perf_counter()
        d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), ap_kind=kind, ap_threshold=t1, ap_threshold_2=t2, **mk)
        setup_s = time.perf_counter() - t0
        bad = d.check(loc, d.new_x(xo), d.new_y())[0]
        ld, size = d.padded_vec_size, 4 if kind == "sp_hp" else 8
        for b in a.b:
            cols = [xo * (1.0 + (v % 8) / 8.0) for v in range(b)]
            for layout in (COL, ROW):
                X = d.new_X(cols, b, layout)
                Y = t.zeros(b * ld, dtype=d.tdtype, device="cuda")
                xs = [d.new_x(c) for c in cols]
                ys = [d.new_y() for _ in cols]
                if d_ap is not None:
                    assert d_ap.padded_vec_size == ld
                    Xp = d_ap.new_X(cols, b, layout)
                    Yp = t.zeros(b * ld, dtype=t.float64, device="cuda")

                def arm_a(n):
                    for _ in range(n):
                        d.spmmv_ap_hp(X, Y, b, layout)

                def arm_b(n):
                    d.set_option("overlap", 0)
                    for _ in range(n):
                        d.spmmv_ap_hp(X, Y, b, layout)
                    d.set_option("overlap", 1)

                def arm_c(n):
                    for _ in range(n):
                        for x, y in zip(xs, ys):
                            d.spmv(x, y)

                def arm_d(n):
                    for _ in range(n):
                        d_ap.spmmv_ap(Xp, Yp, b, layout)

                def arm_e(n):
                    pkg.set_tuning(tlc=0)
                    try:
                        for _ in range(n):
                            d.spmmv_ap_hp(X, Y, b, layout)
                    finally:
                        pkg.set_tuning(tlc=1)

                arms = dict(a=(d, arm_a), b=(d, arm_b), c=(d, arm_c), d=(d_ap, arm_d), e=(d, arm_e))
                ms = {k: [] for k in a.arms}
                for _ in range(a.rounds):
                    for k in a.arms:
                        ms[k].append(timed(*arms[k]))
                med = {k: float(np.median(v)) for k, v in ms.items()}
                spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
                rec = dict(config="block step hp", kind="ap[%s]" % kind, label=a.label, matrix="gen:%dx%dx%d:%d:%g block %d of %d" % (*shape, dof, dec, rank, P),
                           threshold_1=t1, threshold_2=t2, thresholds="0.7 / 0.35 quantiles of |v| over every 16th entry of the block", C=C, sigma=sigma,
                           n_local=nl, n_halo=d.n_halo, padded_vec_size=ld, column_bytes_mod_16=(ld * size) % 16, b=b,
                           layout="row-wise" if layout == ROW else "column-wise", mode="bulkvec", rounds=a.rounds, steps=a.steps,
                           timing="HIP events on the object's stream around eager steps; ms per block step", self_check_mismatches=bad,
                           ms={k: round(v, 4) for k, v in med.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                           ms_rounds={k: [round(v, 4) for v in vs] for k, vs in ms.items()}, setup_s=round(setup_s, 1), census=d.pad_info(),
                           lists=dict(tiles=d.use_tiles, interior=d.n_interior, boundary=d.n_boundary))
                if hasattr(d, "spmmv_ap_hp_tiles_path") and d.use_tiles:
                    paths = {k: list(d.spmmv_ap_hp_tiles_path(b, layout)) for k in a.arms if k in "ab"}
                    if "c" in a.arms:
                        paths["c"] = "single-vector lists (uspmv_spmv_ap_hp_tiles)"
                    if "e" in a.arms:
                        pkg.set_tuning(tlc=0)
                        paths["e"] = list(d.spmmv_ap_hp_tiles_path(b, layout))
                        pkg.set_tuning(tlc=1)
                    if d_ap is not None and d_ap.use_tiles:
                        paths["d"] = list(pkg.spmmv_ap_tiles_path(pair[0], pair[1], b, ld, layout))
                    rec["tiles_path"] = paths
                if "a" in med:
                    rec["a_ahead_by_more_than_twice_the_spreads"] = {k: bool(med[k] - med["a"] > 2 * max(spread[k], spread["a"])) for k in med if k != "a"}
                    rec["a_behind_by_more_than_twice_the_spreads"] = {k: bool(med["a"] - med[k] > 2 * max(spread[k], spread["a"])) for k in med if k != "a"}
                    rec["steps_counted"] = d.spmmv_info()
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n"); out.flush()
                del X, Y, xs, ys
        d.close()
    if d_ap is not None:
        d_ap.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
