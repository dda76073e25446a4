#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/random_vs_reference.npz: what the GENUINE reference (oracle/_ref, built by
oracle/Makefile where the reference sources are present) computes for the randomised inputs of tests/test_random_vs_reference.py.

    python oracle/make_golden_random.py

The inputs are made by the test module's own functions, so test and fixture cannot drift apart unseen: their SHA-1 is stored next
to the reference's outputs.  Where the original cross-check fed the reference with what the product produced (the SELL arrays of the
kernel cases, the file the product's writer rewrote), the product is run here too.  Small results are stored whole, larger ones as
"dtype|size|SHA-1 of the bytes" under <key>#sha1 (tests/test_random_vs_reference.py::same); the kernels' y and Y always whole."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge  # noqa: E402
import test_random_vs_reference as T  # noqa: E402
from oracle import refshim as R  # noqa: E402

OUT = T.FIXTURE
SCS_KEYS = T.SCS_KEYS
SHA_ABOVE = 2048          # elements


def put(out, key, a):
    a = np.ascontiguousarray(a)
    if a.size > SHA_ABOVE:
        out[key + "#sha1"] = f"{a.dtype.str}|{a.size}|{T.sha(a)}"
    else:
        out[key] = a


def convert_goldens(pkg, out):
    for seed, n, C, sigma in T.CASES:
        n_cols, I, J, V = T.convert_case(seed, n)
        p = f"convert/{seed}/"
        out[p + "inputs"] = T.sha(I, J, V)
        rm = R.RefMtx.from_coo(n, n_cols, I, J, V)
        for dt in ("f64", "f32"):
            r = R.convert_to_scs(rm, C, sigma, dt)
            ra = r.arrays()
            out[p + dt + "/meta"] = np.array([r.n_chunks, r.n_elements, r.n_rows_padded], np.int64)
            for k in SCS_KEYS:
                put(out, p + dt + "/" + k, ra[k])
            written = ra["old_to_new_idx"][ra["old_to_new_idx"] < n]
            put(out, p + dt + "/new_to_old_idx_written", ra["new_to_old_idx"][written])
        th = float(np.median(np.abs(V)))
        rdp, rsp, (sI, sJ, sV) = R.partition_precisions_dpsp(rm, th)
        for k, a in zip(("dp/I", "dp/J", "dp/V", "sp/I", "sp/J", "sp/V"), rdp.arrays() + (sI, sJ, sV)):
            put(out, p + k, a)
        # the ap[dp_sp] sp struct, only where the test reaches it (the product decides, as in the test: a permutation that moves a row
        # into a padding slot, or a non-empty row on a shorter chunk, would overrun the reference)
        m = pkg.Coo.from_arrays(n, n_cols, I, J, V)
        dp, sp = pkg.partition_precisions(m, th)
        if dp.nnz and sp.nnz and n >= C:
            perm = pkg.convert_to_scs(dp, C, sigma, pkg.F64).arrays()["old_to_new_idx"].copy()
            if np.all(perm < n):
                try:
                    pkg.convert_to_scs(sp, C, sigma, pkg.F32, fixed_permutation=perm)
                except pkg.UspmvError:
                    continue
                rds = R.convert_to_scs(rdp, C, sigma, "f64")
                rss = R.convert_to_scs(rsp, C, sigma, "f32", fixed_perm=rds.arrays()["old_to_new_idx"])
                for k in SCS_KEYS:
                    put(out, p + "ap_sp/" + k, rss.arrays()[k])


def equilibrate_goldens(pkg, out):
    for name in T.EQUILIBRATE:
        m = T.equilibrate_case(pkg, name)
        I, J, V = [a.copy() for a in m.arrays()]
        p = f"equilibrate/{name}/"
        out[p + "inputs"] = T.sha(I, J, V)
        rm = R.RefMtx.from_coo(m.n_rows, m.n_cols, I, J, V)
        rm.equilibrate()
        put(out, p + "values", rm.arrays()[2])


def kernel_goldens(pkg, out):
    for seed, n, C, sigma in T.CASES[3:]:
        inputs, structs = T.kernel_case(pkg, seed, n, C, sigma)
        p = f"kernels/{seed}/"
        out[p + "inputs"] = T.sha(*inputs)
        for dt, kind, s, xp in structs:
            a = s.arrays()
            out[p + dt + "/scs"] = T.sha(*(a[k] for k in SCS_KEYS), xp)
            out[p + dt + "/y"] = R.spmv_scs(kind, C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
            X, b, ld = T.kernel_block_x(s, xp)
            Y = R.spmmv_scs_general(C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, b, ld, 0)
            out[p + dt + "/Y"] = Y.reshape(b, ld)[:, :s.n_rows_padded].copy()


def partition_goldens(out):
    for seed, n, P, method, C, sigma in T.PARTITION:
        I, J, V = T.partition_case(seed, n)
        p = f"partition/{seed}/"
        out[p + "inputs"] = T.sha(I, J, V)
        rm = R.RefMtx.from_coo(n, n, I, J, V, "mpi")
        wsa = R.seg_work_sharing_arr(rm, method, P)
        put(out, p + "wsa", wsa)
        for r in range(P):
            if wsa[r + 1] == wsa[r]:
                continue
            q = f"{p}{r}/"
            loc = R.seg_local_mtx(rm, wsa, r)
            for k, a in zip("IJV", loc.arrays()):
                put(out, q + k, a)
            rs = R.convert_to_scs(loc, C, sigma, "f64")
            nh, recv, cum = R.collect_local_needed_heri(rs, wsa, r, P)
            out[q + "n_halo"] = np.array(nh, np.int64)
            put(out, q + "recv_counts_cumsum", cum)
            for o in range(P):
                put(out, f"{q}recv_idxs/{o}", recv[o])
            put(out, q + "col_idxs", rs.arrays()["col_idxs"])


def read_mtx_goldens(pkg, out):
    def coo(key, path):
        r = R.RefMtx.read(path)
        I, J, V = r.arrays()
        out[key + "/dims"] = np.array([r.n_rows, r.nnz], np.int64)
        put(out, key + "/I", I); put(out, key + "/J", J); put(out, key + "/V", V.view(np.uint64))      # (values: bit for bit)

    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "spellings.mtx")
        T.write_spellings_mtx(p)
        coo("read_mtx/spellings", p)
        p = os.path.join(d, "big_sym.mtx")
        T.write_big_symmetric_mtx(p)
        coo("read_mtx/big_symmetric", p)
        q = os.path.join(d, "rewritten.mtx")
        pkg.read_mtx(p).write_mtx(q, symmetric=False)          # (the file the test rewrites through the product's writer)
        coo("read_mtx/big_rewritten", q)


def main():
    for v in ("colwise", "mpi"):
        if not R.available(v):
            raise SystemExit(f"oracle/_ref ({v}) is not built: run `make -C oracle` where the reference sources are present")
    pkg = ge.load_package()
    out = {}
    convert_goldens(pkg, out)
    equilibrate_goldens(pkg, out)
    kernel_goldens(pkg, out)
    partition_goldens(out)
    read_mtx_goldens(pkg, out)
    out = {k: np.asarray(v) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
