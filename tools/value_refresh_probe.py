"""Numeric refresh against the re-set-up it replaces, on the GPU.  Three handles, every one from COO arrays in HBM:

  stencil253   27-point 253^3 dp stencil, the default plan (uspmv_dmat_optimize_device)
  mesh111x3    111^3 nodes x 3 dof, the b = 8 block plan (uspmv_dmat_optimize_block_device)
  banded       banded-random 500 k x 140, its column-window sweep plan (uspmv_dmat_optimize_sweep_device)

and per handle, in one process, alternating, warmed, HIP events around calls that end in a synchronise:

  (a) uspmv_dmat_update_values_from_arrays with and without check_pattern -- placement + refresh of the plans
  (b) uspmv_dmat_values_changed alone
  (c) what a caller had before from the same device arrays: uspmv_convert_to_scs_device_from_arrays + the same planner call
  (d) uspmv_stream_copy, the rate yardstick of the same run

(a) is also reported as bytes over time against (d), the bytes counted from the shapes: 12 read per entry (4 of the row index, 8 of the
value), sizeof(VT) written per slot, 4 more read per slot under check_pattern (the stored column; the 4 of J per entry are not counted).  The plans' own refresh (b) is inside (a)'s time and not in its bytes.  One JSON line per handle, printed and
appended to profiles/value_refresh/probe.jsonl ("placement": which placement kernel the library under test has; the lines that say
"entries" were measured on a build with one thread per COO entry behind a memset, the form that was not kept).  --setups 0 leaves
route (c) out: for a kernel-trace run of the refresh alone."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "value_refresh", "probe.jsonl")


def timed(t, fn):
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1), r


def stream_copy_ms(pkg, t, a, b):
    st = t.cuda.current_stream().cuda_stream
    ms, _ = timed(t, lambda: [pkg.lib().uspmv_stream_copy(a.data_ptr(), b.data_ptr(), a.numel(), st) for _ in range(5)])
    return ms / 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--handles", default="stencil253,mesh111x3,banded")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--setups", type=int, default=2, help="rounds that also time route (c)")
    ap.add_argument("--out", default=OUT, help="the JSON lines are appended here ('' for none)")
    a = ap.parse_args()
    import torch as t
    pkg = ge.load_package()
    t.cuda.set_device(0)
    n_copy = 1 << 27
    ca, cb = t.empty(n_copy, dtype=t.float64, device="cuda"), t.ones(n_copy, dtype=t.float64, device="cuda")
    form = "slots"
    for name in a.handles.split(","):
        if name == "stencil253":
            I, J, V = pkg.gen_stencil27_device(253, 253, 253)
            n, plan, plan_name = 253 ** 3, (lambda A: A.optimize_device()), "optimize_device"
        elif name == "mesh111x3":
            I, J, V = pkg.gen_stencil27_device(111, 111, 111, dof=3)
            n, plan, plan_name = 3 * 111 ** 3, (lambda A: A.optimize_block_device(8)), "optimize_block_device(8)"
        elif name == "banded":
            m = pkg.gen_banded_random(500000, 140, 50000)
            I, J, V = (t.from_numpy(np.array(x)).cuda() for x in m.arrays())
            n, plan, plan_name = m.n_rows, (lambda A: A.optimize_sweep_device()), "optimize_sweep_device"
            del m
        else:
            raise SystemExit(f"unknown handle {name}")
        nnz = int(I.numel())
        V1 = V * 1.5

        def setup():
            _, A, o2n, _ = pkg.convert_to_scs_device_from_arrays(I, J, V, n, n, 32, 512, pkg.F64, want_layout=False)
            return A, o2n, plan(A)

        A, o2n, planned = setup()
        t.cuda.synchronize()
        rows = dict(a_check=[], a_nocheck=[], b=[], c=[], d=[])
        actions = None
        for r in range(a.rounds + 1):                        # round 0 warms
            ms_c, (Ac, _, _) = timed(t, setup) if a.setups and r <= a.setups else (None, (None, None, None))
            del Ac
            ms_ac, actions = timed(t, lambda: A.update_values_from_coo(I, J, V1 if r % 2 else V, row_pos=o2n, col_perm=o2n, check=True))
            ms_an, _ = timed(t, lambda: A.update_values_from_coo(I, J, V if r % 2 else V1, row_pos=o2n, col_perm=o2n, check=False))
            ms_b, _ = timed(t, lambda: A.values_changed())
            ms_d = stream_copy_ms(pkg, t, ca, cb)
            if r:
                for k, v in (("a_check", ms_ac), ("a_nocheck", ms_an), ("b", ms_b), ("c", ms_c), ("d", ms_d)):
                    if v is not None:
                        rows[k].append(v)
        med = {k: float(np.median(v)) if v else float("nan") for k, v in rows.items()}
        copy_rate = 16.0 * n_copy / (med["d"] * 1e-3)
        ne = A.n_elements
        bytes_nocheck, bytes_check = 12 * nnz + 8 * ne, 12 * nnz + 12 * ne
        line = dict(handle=name, placement=form, n_rows=n, nnz=nnz, n_elements=ne, planner=plan_name, planned=list(planned), plan_kind=A.plan_info()[0],
                    block_plan=A.block_plan_info()["phased_plan"], actions=actions, rounds=a.rounds,
                    update_check_ms=round(med["a_check"], 4), update_nocheck_ms=round(med["a_nocheck"], 4), values_changed_ms=round(med["b"], 4),
                    resetup_ms=round(med["c"], 2) if rows["c"] else None, stream_copy_GBs=round(copy_rate / 1e9, 1),
                    update_check_GBs=round(bytes_check / (med["a_check"] * 1e-3) / 1e9, 1), update_nocheck_GBs=round(bytes_nocheck / (med["a_nocheck"] * 1e-3) / 1e9, 1),
                    update_check_frac_of_copy=round(bytes_check / (med["a_check"] * 1e-3) / copy_rate, 3),
                    update_nocheck_frac_of_copy=round(bytes_nocheck / (med["a_nocheck"] * 1e-3) / copy_rate, 3),
                    resetup_over_update_check=round(med["c"] / med["a_check"], 1) if rows["c"] else None,
                    resetup_over_update_check_plus_values_changed=round(med["c"] / (med["a_check"] + med["b"]), 1) if rows["c"] else None,
                    spread_ms={k: [round(min(v), 4), round(max(v), 4)] for k, v in rows.items() if v})
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del A, I, J, V, V1, o2n
        t.cuda.empty_cache()


if __name__ == "__main__":
    main()
