#!/usr/bin/env python3
"""The distributed adaptive-precision step (uspmv_dist_create_ap_from_coo) on ONE GPU in loopback, against what a caller had before it.

Matrix: 27-point stencil, 5 dof, magnitudes over 10 decades, threshold 1e-3, SELL-32-512; block 1 of P = 4 of 74 x 74 x 296 nodes
(seg-rows), so that the block is the 74^3 x 5 matrix (2 026 120 rows) the README quotes.  Three arms, alternated in one process, each
round = 60 steps replayed from the captured hipGraph between two HIP events on the object's stream, after 10 untimed steps of the
same form (a change of form drops the graph: the capture happens in the warm-up):

  (a) the ap object, overlap with "pad_split" 1 (its default)
  (b) the ap object, plain (exchange, then the whole matrix)
  (c) the one-precision dp object on the same block in its default form (overlap, "pad_split" 0)
  (s) uspmv_spmv_ap on the ap object's pair, no object, no exchange

One JSON line: medians and spreads (max - min over the rounds) in ms per step, whether (a) is ahead of (b) and of (c) by more than
twice the compared arm's spread, and the tile census.  --census prints the census alone (interior / padding-only / real boundary
tiles per rank; what runs before the exchange with "pad_split" 0 and 1) for the loopback test matrices and the probe block.
Loopback exchanges are RCCL self send / recv on one GPU, not links: N > 1 GPUs stay unmeasured.

--kind dp_hp | sp_hp | dp_sp_hp measures the object of a kind with an fp16 part (uspmv_dist_create_ap_hp_from_coo) on the same block instead,
thresholds at the 0.7 / 0.35 quantiles of |v| (of every 16th entry of the block), four arms alternated the same way:

  (a) the hp object in its default form (overlap, "pad_split" 1)
  (b) the hp object plain
  (c) the ap[dp_sp] object at threshold = the 0.7 quantile in its default form
  (d) uspmv_spmv_ap_hp on the hp object's handles, no object, no exchange

    python tools/dist_ap_probe.py [--rounds 5 --steps 60 --out profiles/dist_ap/probe.jsonl]
    python tools/dist_ap_probe.py --census [--out ...]
    python tools/dist_ap_probe.py --kind dp_sp_hp [--out profiles/dist_ap_hp/probe.jsonl]
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


def block(pkg, shape, dof, dec, P, rank):
    counts = pkg.gen_stencil27_row_counts(*shape, dof)
    wsa = pkg.seg_from_row_counts(counts, "seg-rows", P)
    return wsa, pkg.gen_stencil27(*shape, dof, magnitude_decades=dec, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))


def census(d):
    """tiles (chunks without tile lists) by class, and how many run before the exchange has completed with "pad_split" 0 / 1"""
    info = d.pad_info()
    pad = info["pad_tiles"]
    return dict(units="tiles" if d.use_tiles else "chunks", total=d.n_interior + d.n_boundary, interior=d.n_interior, padding_only=pad,
                real_boundary=d.n_boundary - pad, before_exchange_pad_split_0=d.n_interior, before_exchange_pad_split_1=d.n_interior + pad)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n"); out.flush()


def run_census(pkg, out):
    for shape, dof, dec, P, C, sigma in (((24, 24, 24), 1, 6.0, 2, 32, 512), ((16, 16, 40), 1, 6.0, 4, 32, 512)):
        for rank in range(P):
            wsa, loc = block(pkg, shape, dof, dec, P, rank)
            for kind, thr in (("ap[dp_sp]", THR), ("dp", None)):
                d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_threshold=thr)
                emit(dict(config="census", matrix="gen:%dx%dx%d:%d:%g" % (*shape, dof, dec), P=P, rank=rank, kind=kind, **census(d)), out)
                d.close()


def run_hp(pkg, t, a, out):
    """the four arms of --kind (see the module text)"""
    P, rank, C, sigma, dof, dec = 4, 1, 32, 512, 5, 10.0
    shape = (a.nodes, a.nodes, a.nodes * P)
    t0 = time.perf_counter()
    wsa, loc = block(pkg, shape, dof, dec, P, rank)
    nl = int(wsa[rank + 1] - wsa[rank])
    av = np.abs(np.asarray(loc.arrays()[2])[::16])
    t1, t2 = float(np.quantile(av, 0.7)), float(np.quantile(av, 0.35))
    del av
    mk = dict(comm_rank=0, comm_size=1)
    d_hp = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), ap_kind=a.kind, ap_threshold=t1, ap_threshold_2=t2, **mk)
    d_ap = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), ap_threshold=t1, **mk)
    setup_s = time.perf_counter() - t0
    xo = 1.0 + 1e-3 * (np.arange(nl) % 1000)
    bad = {k: d.check(loc, d.new_x(xo), d.new_y(), use_graph=True)[0] for k, d in (("hp", d_hp), ("ap", d_ap))}
    vec = {id(d): (d.new_x(xo), d.new_y()) for d in (d_hp, d_ap)}
    hand = [SimpleNamespace(h=h) if h is not None else None for h in (d_hp._A, d_hp._A_mid, d_hp._A_hp)]

    def timed(d, fn):
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record(d.stream); fn(a.steps); e1.record(d.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def arm_object(d, overlap, pad):
        x, y = vec[id(d)]
        d.set_option("overlap", overlap); d.set_option("pad_split", pad)
        d.run(x, y, 10, use_graph=True); d.synchronize()           # warm-up of this form (and its capture)
        return timed(d, lambda n: d.run(x, y, n, use_graph=True))

    def arm_kernel():
        x, y = vec[id(d_hp)]
        lib, xp, yp, st = pkg.lib(), x.data_ptr(), y.data_ptr(), d_hp.stream.cuda_stream
        hm = hand[1].h if hand[1] is not None else None

        def launch(n):
            for _ in range(n):
                assert lib.uspmv_spmv_ap_hp(hand[0].h, hm, hand[2].h, xp, yp, st) == 0
        launch(10); d_hp.synchronize()
        return timed(d_hp, launch)

    ms = dict(a=[], b=[], c=[], d=[])
    for _ in range(a.rounds):
        ms["a"].append(arm_object(d_hp, 1, 1))
        ms["b"].append(arm_object(d_hp, 0, 1))
        ms["c"].append(arm_object(d_ap, 1, 1))
        ms["d"].append(arm_kernel())
    d_hp._refresh(); d_ap._refresh()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(max(v) - min(v)) for k, v in ms.items()}

    def real(x, y):                                                 # x ahead of y by more than twice the larger spread
        return bool(med[y] - med[x] > 2 * max(spread[x], spread[y]))

    el = dict(hi=d_hp.scs.n_elements, mid=d_hp.scs_mid.n_elements if d_hp.scs_mid is not None else 0, hp=d_hp.scs_hp.n_elements)
    nz = dict(hi=d_hp.scs.nnz, mid=d_hp.scs_mid.nnz if d_hp.scs_mid is not None else 0, hp=d_hp.scs_hp.nnz)
    rec = dict(config="step_hp", kind="ap[%s]" % a.kind, matrix="gen:%dx%dx%d:%d:%g block %d of %d" % (*shape, dof, dec, rank, P), threshold_1=t1, threshold_2=t2,
               thresholds="0.7 / 0.35 quantiles of |v| over every 16th entry of the block", C=C, sigma=sigma, n_local=nl, n_halo=d_hp.n_halo, nnz=loc.nnz,
               nnz_parts=nz, elements_parts=el, elements_ap_dp_sp=dict(dp=d_ap.scs.n_elements, sp=d_ap.scs_sp.n_elements), rounds=a.rounds, steps=a.steps,
               timing="HIP events on the object's stream around the replays of one captured graph (arm d: around the launches); ms per step",
               graph_replay=dict(hp=d_hp.graph_captured, ap=d_ap.graph_captured), self_check_mismatches=bad,
               ms_a_hp_overlap_pad_split=round(med["a"], 4), ms_b_hp_plain=round(med["b"], 4), ms_c_ap_dp_sp_default=round(med["c"], 4),
               ms_d_spmv_ap_hp_no_exchange=round(med["d"], 4), spread_ms={k: round(v, 4) for k, v in spread.items()},
               rule="a difference is real when it exceeds twice the larger of the two spreads",
               a_ahead_of_b=real("a", "b"), b_ahead_of_a=real("b", "a"), a_ahead_of_c=real("a", "c"), c_ahead_of_a=real("c", "a"),
               b_ahead_of_c=real("b", "c"), c_ahead_of_b=real("c", "b"),
               census_hp=census(d_hp), census_ap=census(d_ap), setup_s=round(setup_s, 1),
               ms_rounds={k: [round(v, 4) for v in vs] for k, vs in ms.items()})
    emit(rec, out)
    d_hp.close(); d_ap.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--nodes", type=int, default=74, help="the block is nodes^3 x 5 dof (74: the size the README quotes)")
    ap.add_argument("--census", action="store_true")
    ap.add_argument("--kind", default="dp_sp", choices=("dp_sp", "dp_hp", "sp_hp", "dp_sp_hp"), help="dp_sp: the ap[dp_sp] arms; else the fp16 kind's four arms")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    assert t.cuda.is_available(), "dist_ap_probe needs a GPU"
    t.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None
    if a.census:
        run_census(pkg, out)
        return
    if a.kind != "dp_sp":
        run_hp(pkg, t, a, out)
        if out:
            out.close()
        return
    P, rank, C, sigma, dof, dec = 4, 1, 32, 512, 5, 10.0
    shape = (a.nodes, a.nodes, a.nodes * P)
    t0 = time.perf_counter()
    wsa, loc = block(pkg, shape, dof, dec, P, rank)
    nl = int(wsa[rank + 1] - wsa[rank])
    d_ap = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_threshold=THR)
    d_dp = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1)
    setup_s = time.perf_counter() - t0
    xo = 1.0 + 1e-3 * (np.arange(nl) % 1000)
    vec = {id(d): (d.new_x(xo), d.new_y()) for d in (d_ap, d_dp)}
    bad_ap = d_ap.check(loc, *vec[id(d_ap)], use_graph=True)[0]
    bad_dp = d_dp.check(loc, *vec[id(d_dp)], use_graph=True)[0]
    vec = {id(d): (d.new_x(xo), d.new_y()) for d in (d_ap, d_dp)}
    pair = (SimpleNamespace(h=d_ap._A), SimpleNamespace(h=d_ap._A_sp))

    def timed(d, fn):
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record(d.stream); fn(a.steps); e1.record(d.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def arm_object(d, overlap, pad):
        x, y = vec[id(d)]
        d.set_option("overlap", overlap); d.set_option("pad_split", pad)
        d.run(x, y, 10, use_graph=True); d.synchronize()           # warm-up of this form (and its capture)
        return timed(d, lambda n: d.run(x, y, n, use_graph=True))

    def arm_kernel():
        x, y = vec[id(d_ap)]
        launch = lambda n: [pkg.spmv_ap(pair[0], pair[1], x, y, stream=d_ap.stream) for _ in range(n)]  # noqa: E731
        launch(10); d_ap.synchronize()
        return timed(d_ap, launch)

    ms = dict(a=[], b=[], c=[], s=[])
    for _ in range(a.rounds):
        ms["a"].append(arm_object(d_ap, 1, 1))
        ms["b"].append(arm_object(d_ap, 0, 1))
        ms["c"].append(arm_object(d_dp, 1, 0))
        ms["s"].append(arm_kernel())
    d_ap._refresh(); d_dp._refresh()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
    el_dp, el_sp = d_ap.scs.n_elements, d_ap.scs_sp.n_elements
    rec = dict(config="step", matrix="gen:%dx%dx%d:%d:%g block %d of %d" % (*shape, dof, dec, rank, P), threshold_1=THR, C=C, sigma=sigma, n_local=nl,
               n_halo=d_ap.n_halo, nnz=loc.nnz, elements_dp=el_dp, elements_sp=el_sp, elements_one_precision=d_dp.scs.n_elements,
               rounds=a.rounds, steps=a.steps, timing="HIP events on the object's stream around the replays of one captured graph; ms per step",
               graph_replay=dict(ap=d_ap.graph_captured, dp=d_dp.graph_captured), self_check_mismatches=dict(ap=bad_ap, dp=bad_dp),
               ms_a_ap_overlap_pad_split=round(med["a"], 4), ms_b_ap_plain=round(med["b"], 4), ms_c_dp_default=round(med["c"], 4),
               ms_s_spmv_ap_no_exchange=round(med["s"], 4), spread_ms={k: round(v, 4) for k, v in spread.items()},
               a_ahead_of_b_by_more_than_twice_b_spread=bool(med["b"] - med["a"] > 2 * spread["b"]),
               a_ahead_of_c_by_more_than_twice_c_spread=bool(med["c"] - med["a"] > 2 * spread["c"]),
               a_behind_b_by_more_than_twice_b_spread=bool(med["a"] - med["b"] > 2 * spread["b"]),
               census_ap=census(d_ap), census_dp=census(d_dp), setup_s=round(setup_s, 1),
               ms_rounds={k: [round(v, 4) for v in vs] for k, vs in ms.items()})
    emit(rec, out)
    d_ap.close(); d_dp.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
