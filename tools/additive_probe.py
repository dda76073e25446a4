#!/usr/bin/env python3
"""The tile-local-column kernel over its local indices against the additive chunk records (`tlc_additive`), alternating between two
handles of one matrix in one process, per matrix class: kernel ms (median and min of the rounds), whether the byte rule keeps the records,
the share of additive chunks, bits compared with the local-index result and with the gather kernel."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch as t
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from ultimate_spmv_amd import binding as B
    t.cuda.set_device(0)
    classes = {
        "stencil27_253": lambda: pkg.gen_stencil27(253, 253, 253),
        "stencil27_304": lambda: pkg.gen_stencil27(304, 304, 304),
        "stencil27_111_dof3": lambda: pkg.gen_stencil27(111, 111, 111, dof=3),
        "kkt_200": lambda: pkg.gen_kkt(200),
    }
    for name, gen in classes.items():
        if args.only and name not in args.only.split(","):
            continue
        coo = gen()
        s = pkg.convert_to_scs(coo, 32, 512, pkg.F64)
        a = s.arrays(); pkg.permute_scs_cols(s, a["old_to_new_idx"])
        x = t.rand(s.n_rows_padded, dtype=t.float64, device="cuda"); y = t.zeros_like(x)
        rule, _ = pkg.additive_plan_probe(s, decode=False)            # the byte rule's verdict (at 256 rows per tile)
        pkg.set_tuning(tlc_additive=2)
        stage = pkg.additive_plan_probe2(s)                           # W of the 2-byte map, the tagged line lists
        pkg.set_tuning(tlc_additive=1)
        H = {}
        for v in (0, 1):
            pkg.set_tuning(tlc_additive=2 if v else 0)
            H[v] = pkg.DeviceMatrix(s, tlc=True)
        pkg.set_tuning(tlc_additive=1)
        A0 = pkg.DeviceMatrix(s)                                  # gather kernel
        yg = t.zeros_like(x); pkg.spmv(A0, x, yg); del A0
        ys = {}
        for v in (0, 1):
            y.fill_(-1.0); pkg.spmv(H[v], x, y); ys[v] = y.clone()
        for v in (0, 1): B.time_launches(0, 20, A=H[v], x=x, y=y)
        ms = {0: [], 1: []}
        for _ in range(args.rounds):
            for v in (0, 1): ms[v].append(B.time_launches(0, args.reps, A=H[v], x=x, y=y))
        for v in (0, 1):
            m = sorted(ms[v])[len(ms[v]) // 2]
            n_add, n_ch = H[v].additive_chunks()
            print(json.dumps(dict(matrix=name, n=s.n_rows, nnz=s.nnz, additive=v, tile_rows=H[v].tile_rows, kernel_ms_median=round(m, 5), kernel_ms_min=round(min(ms[v]), 5),
                                  rounds=[round(q, 5) for q in ms[v]], additive_chunks=n_add, chunks_with_records=n_ch, chunks=s.n_chunks, index_bits=H[v].index_bits(),
                                  rule_keeps=bool(rule["kept"]), map_block=stage["W"], list_entries=stage["list_entries"], lines_listed_again=stage["lines_listed_again"], new_bytes=rule["new_bytes"], replaced_bytes=rule["replaced_bytes"], lds_elements=rule["max_elems"],
                                  same_as_local_indices=bool(t.equal(ys[v], ys[0])), same_as_gather=bool(t.equal(ys[v], yg)))), flush=True)
        del H, coo, s


if __name__ == "__main__":
    main()
