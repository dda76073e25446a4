#!/usr/bin/env python3
"""The SpMV planner's route table: every public planner entry (optimize / optimize_device, optimize_ap / optimize_device_ap,
optimize_ap_hp / optimize_device_ap_hp for ap[dp_hp], ap[sp_hp], ap[dp_sp_hp]) against the smallest matrices that reach each route of
csrc/tlc_planner.hip -- the line plan, the line plan on grown tiles, the plan over single x elements, the column-window sweep -- one JSON
record per (matrix, kind, planner): what the entry returned, what the handles carry afterwards and a sha1 over the plan's arrays.

  planner_routes.py record OUT.json            try each route's ladder of sizes, keep the smallest that meets the conditions below, write the table
  planner_routes.py check TABLE.json           recompute every record of a table and compare (tests/test_gpu_planner_routes.py does the same)
  planner_routes.py times TABLE.json LABEL N   wall time of every entry on the table's matrices, N repetitions: one JSON line per case on stdout

Conditions a recorded table meets: every entry has a record on lines, on elements and on the sweep; one record has tile_rows > 256; the host
and the device record of one case carry equal hashes.  All matrices stay below 2^20 padded rows, so no tile size is measured."""
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KINDS = ("one", "dp_sp", "dp_hp", "sp_hp", "dp_sp_hp")
PLANNERS = ("host", "device")
ROUTES = ("lines", "grow", "elements", "sweep", "dropped")
# per route: the sizes tried when recording, smallest first (what they mean: coo_of)
LADDERS = {"lines": [16], "grow": [4096, 8192, 16384], "elements": [[24, 1000], [24, 2000], [24, 4000], [24, 8000], [32, 8000], [40, 8000]], "sweep": [6000, 10000, 16000, 30000, 60000],
           "dropped": [100000, 200000, 400000]}
C_SIGMA = (32, 512)


def scrambled_columns(pkg, g, dof, K, seed=3):
    """27-point x dof stencil on g^3 nodes, the columns' nodes renumbered at random inside consecutive blocks of K nodes (the generator of
    tests/test_gpu_ap_elem_plan.py)"""
    base = pkg.gen_stencil27(g, g, g, dof=dof)
    I, J, V = (np.array(a) for a in base.arrays())
    n = base.n_rows
    nn = n // dof
    rng = np.random.default_rng(seed)
    p = np.arange(nn, dtype=np.int64)
    for s0 in range(0, nn, K):
        seg = p[s0:s0 + K].copy(); rng.shuffle(seg); p[s0:s0 + K] = seg
    J2 = (p[J // dof] * dof + J % dof).astype(np.int32)
    o = np.lexsort((J2, I))
    return pkg.Coo.from_arrays(n, n, I[o], J2[o], V[o])


def coo_of(pkg, route, size):
    if route == "lines":
        return pkg.gen_stencil27(size, size, size, magnitude_decades=4.0)
    if route == "grow":          # 30 per row over +-2000 columns: 256-row tiles need more than 250 lines
        return pkg.gen_banded_random(size, 30, 2000, magnitude_decades=4.0)
    if route == "elements":
        return scrambled_columns(pkg, size[0], 3, size[1])           # size: (nodes per edge, nodes per renumbered block)
    if route == "sweep":         # the wide banded-random matrix of tests/test_gpu_sweep.py
        return pkg.gen_banded_random(size, 60, 5000, magnitude_decades=4.0)
    return partly_regular(pkg, size)


def partly_regular(pkg, n_cols, g=20, n_rows=20000, per_row=8, seed=7):
    """The first two fifths of the rows are the 27-point stencil on g^3 nodes (their tiles stage on the line plan and would sweep), the others
    hold per_row entries anywhere in n_cols columns: too many lines for the line plan, an entry per listed element (the element plan does not
    pay), and more x to stage per entry than the sweep allows.  A split with an fp16 part drops its line plan there (ap_hp_plan_worth)."""
    I, J, V = (np.array(a) for a in pkg.gen_stencil27(g, g, g).arrays())
    rng = np.random.default_rng(seed)
    rows = np.arange(g ** 3, n_rows, dtype=np.int32)
    J2 = np.sort(rng.integers(0, n_cols, (rows.size, per_row)), axis=1)
    keep = np.ones(J2.shape, bool)
    keep[:, 1:] = J2[:, 1:] != J2[:, :-1]                   # (a column once per row)
    I2 = np.repeat(rows, per_row).reshape(J2.shape)[keep]
    V2 = rng.uniform(0.5, 1.0, I2.size) * 10.0 ** rng.uniform(-2.0, 2.0, I2.size)
    return pkg.Coo.from_arrays(n_rows, n_cols, np.concatenate([I, I2]).astype(np.int32), np.concatenate([J, J2[keep]]).astype(np.int32),
                               np.concatenate([V, V2]))


_STRUCTS = {}


def structs_of(pkg, route, size, kind):
    """(first, mid | None, last) host structs of one split in one row order (kind "one": the dp struct alone), built once per process"""
    size_key = tuple(size) if isinstance(size, list) else size
    key = (route, size_key, kind)
    if key in _STRUCTS:
        return _STRUCTS[key]
    if (route, size_key) not in _STRUCTS:
        _STRUCTS[(route, size_key)] = coo_of(pkg, route, size)
    m = _STRUCTS[(route, size_key)]
    C, sigma = C_SIGMA
    a = np.abs(np.asarray(m.arrays()[2]))
    a = a[a > 0]
    t1, t2 = float(np.quantile(a, 0.7)), min(float(np.quantile(a, 0.35)), 6e4)
    if kind in ("dp_hp", "sp_hp"):
        t1 = min(t1, 6e4)
    if kind == "one":
        parts = (m, None, None)
    elif kind == "dp_sp":
        hi, lo = pkg.partition_precisions(m, t1)
        parts = (hi, None, lo)
    else:
        parts = pkg.partition_precisions_hp(m, kind, t1, t2)
    dts = {"one": (pkg.F64, None, None), "dp_sp": (pkg.F64, None, pkg.F32), "dp_hp": (pkg.F64, None, pkg.F16),
           "sp_hp": (pkg.F32, None, pkg.F16), "dp_sp_hp": (pkg.F64, pkg.F32, pkg.F16)}[kind]
    first = pkg.convert_to_scs(parts[0], C, sigma, dts[0])
    perm = first.arrays()["old_to_new_idx"].copy()
    ss = [first] + [pkg.convert_to_scs(p, C, sigma, dt, fixed_permutation=perm) if p is not None else None for p, dt in zip(parts[1:], dts[1:])]
    if route not in ("elements", "dropped"):                # (the scattered columns keep a numbering of their own; "dropped" is not square)
        for s in ss:
            if s is not None:
                pkg.permute_scs_cols(s, perm)
    _STRUCTS[key] = tuple(ss)
    return _STRUCTS[key]


def plan(pkg, kind, planner, ss, hand):
    """calls the entry of (kind, planner) on fresh handles; returns (n_tiles, n_staged)"""
    if kind == "one":
        return hand[0].optimize(ss[0]) if planner == "host" else hand[0].optimize_device()
    if kind == "dp_sp":
        return pkg.optimize_ap(hand[0], hand[2], ss[0], ss[2]) if planner == "host" else pkg.optimize_device_ap(hand[0], hand[2])
    return pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *ss) if planner == "host" else pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2])


def tuning_of(route, kind):
    """an ap[dp_sp] pair below 2^20 padded rows takes the element plan only under "tlc_elem" 2"""
    return dict(tlc_elem=2) if route == "elements" and kind == "dp_sp" else {}


def planned(pkg, route, kind, planner, ss):
    hand = [pkg.DeviceMatrix(s) if s is not None else None for s in ss]
    tuning = tuning_of(route, kind)
    if tuning:
        pkg.set_tuning(**tuning)
    try:
        t0 = time.perf_counter()
        ret = plan(pkg, kind, planner, ss, hand)
        dt = time.perf_counter() - t0
    finally:
        if tuning:
            pkg.set_tuning(tlc_elem=1)
    return hand, ret, dt


def _tile_rows(pkg, A):
    tr = ctypes.c_int()
    rc = pkg.lib().uspmv_dmat_tile_rows(A.h, ctypes.byref(tr))
    assert rc == 0, rc
    return tr.value


def record(pkg, route, size, kind, planner):
    ss = structs_of(pkg, route, size, kind)
    hand, ret, _ = planned(pkg, route, kind, planner, ss)
    live = [h for h in hand if h is not None]
    info = [list(h.plan_info()) for h in live]
    sha = hashlib.sha1()
    if info[0][0] == 2:
        d, meta = live[0].sweep_plan_digest()
        sha.update(np.asarray(d + meta, np.uint64).tobytes())
        for k in range(len(live)):
            d, n = live[0].sweep_plan_digest_part(k)
            sha.update(np.asarray(d + [n], np.uint64).tobytes())
    else:
        for k, h in enumerate(live):
            p = h.plan_download()
            if p is None:
                continue
            # (the line list lives with the first part; the further parts hold their local indices only)
            for name in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16") if k == 0 else ("c16_ptrs", "col16"):
                sha.update(np.ascontiguousarray(p[name]).tobytes())
            sha.update(np.int64(p["max_lines_used"]).tobytes())
    return dict(case=f"{route}/{kind}/{planner}", plan_info=info, returned=list(ret), tile_rows=[_tile_rows(pkg, h) for h in live],
                granularity=[h.plan_granularity() for h in live], index_bits=[h.index_bits() for h in live], sha1=sha.hexdigest())


def route_reached(route, recs):
    """does this size show the route on every entry, the host and the device planner agreeing?"""
    by = {r["case"]: r for r in recs}
    for kind in KINDS:
        h, d = by[f"{route}/{kind}/host"], by[f"{route}/{kind}/device"]
        if h["sha1"] != d["sha1"] or h["plan_info"] != d["plan_info"]:
            return False
        for r in (h, d):
            kinds, gran = {i[0] for i in r["plan_info"]}, set(r["granularity"])
            ok = {"lines": kinds == {1} and gran == {16}, "grow": kinds == {1} and gran == {16} and (kind != "one" or r["tile_rows"][0] > 256),
                  "elements": kinds == {1} and gran == {1}, "sweep": kinds == {2},
                  # (some but under half of the tiles staged, and a split with an fp16 part ends without a plan)
                  "dropped": not kind.endswith("_hp") or (kinds == {0} and 0 < 2 * r["returned"][1] < r["returned"][0])}[route]
            if not ok:
                return False
    return True


def cases(table):
    return [(route, table["sizes"][route], kind, planner) for route in ROUTES if route in table["sizes"] for kind in KINDS for planner in PLANNERS]


def main(argv):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.lib()
    assert torch.cuda.is_available(), "the planners need a GPU"
    torch.cuda.set_device(0)
    mode = argv[1]
    if mode == "record":
        table = dict(sizes={}, records=[])
        for route in ROUTES:
            for size in LADDERS[route]:
                recs = [record(pkg, route, size, kind, planner) for kind in KINDS for planner in PLANNERS]
                ok = route_reached(route, recs)
                print(f"{route} at {size}: {'reached' if ok else 'not reached'}", file=sys.stderr, flush=True)
                if not ok:
                    for r in recs:
                        print("   ", json.dumps(r), file=sys.stderr, flush=True)
                    continue
                table["sizes"][route] = size
                table["records"] += recs
                break
            else:
                if route != "dropped":                      # (the one route the table may lack)
                    raise SystemExit(f"no size of {LADDERS[route]} reaches '{route}' on every entry")
        assert any(max(r["tile_rows"]) > 256 for r in table["records"])
        with open(argv[2], "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
    elif mode == "check":
        with open(argv[2]) as f:
            table = json.load(f)
        want = {r["case"]: r for r in table["records"]}
        bad = 0
        for route, size, kind, planner in cases(table):
            got = record(pkg, route, size, kind, planner)
            if got != want[got["case"]]:
                bad += 1
                print("DIFFERS", json.dumps(got), "recorded", json.dumps(want[got["case"]]), flush=True)
        print(f"{len(want)} records, {bad} differ")
        return 1 if bad else 0
    elif mode == "times":
        with open(argv[2]) as f:
            table = json.load(f)
        label, reps = argv[3], int(argv[4])
        for route, size, kind, planner in cases(table):
            ss = structs_of(pkg, route, size, kind)
            secs = []
            for _ in range(reps + 1):                      # (the first call of an entry is a warm-up: kernels load lazily)
                torch.cuda.synchronize()
                _, _, dt = planned(pkg, route, kind, planner, ss)
                secs.append(round(dt, 6))
            print(json.dumps(dict(commit=label, case=f"{route}/{kind}/{planner}", seconds=secs[1:])), flush=True)
    else:
        raise SystemExit(__doc__)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
