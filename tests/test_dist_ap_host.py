"""Host side of the distributed adaptive-precision (ap[dp_sp]) step: the one halo of a dp + sp pair (uspmv_halo_discover_ap) against the
oracle's collect_local_needed_heri on the concatenated column arrays, the host reference of the self-check
(uspmv_dist_check_reference_ap) against the oracle's whole-matrix ap product, and the new symbols of the C ABI.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, make_x, mtx_path

NEW_SYMBOLS = ("uspmv_spmv_ap_tiles", "uspmv_spmv_ap_chunks", "uspmv_halo_discover_ap", "uspmv_dist_create_ap_from_coo",
               "uspmv_dist_create_ap_from_coo_ex", "uspmv_dist_check_reference_ap", "uspmv_dist_parts_ap")


def ap_pair(pkg, coo, C, sigma, threshold):
    """the host set-up of a pair up to (not including) the column steps: partition -> dp struct -> sp struct with dp's permutation"""
    coo_dp, coo_sp = pkg.partition_precisions(coo, threshold)
    s_dp = pkg.convert_to_scs(coo_dp, C, sigma, pkg.F64)
    s_sp = pkg.convert_to_scs(coo_sp, C, sigma, pkg.F32, fixed_permutation=s_dp.arrays()["old_to_new_idx"].copy())
    return s_dp, s_sp, coo_dp, coo_sp


def whole_matrix_ap_reference(pkg, orc, coo, C, sigma, threshold, x_global):
    """y (original order) of the oracle's scs_ap_impl_cpu on the WHOLE matrix, set up the host way"""
    s_dp, s_sp, coo_dp, coo_sp = ap_pair(pkg, coo, C, sigma, threshold)
    o2n = s_dp.arrays()["old_to_new_idx"].copy()
    pkg.permute_scs_cols(s_dp, o2n)
    pkg.permute_scs_cols(s_sp, o2n)
    a, b = s_dp.arrays(), s_sp.arrays()
    xp = np.zeros(s_dp.n_rows_padded)
    xp[:coo.n_rows] = pkg.apply_permutation(np.ascontiguousarray(x_global, np.float64), a["new_to_old_idx"])
    with np.errstate(invalid="ignore"):
        y = orc.spmv_scs_ap_adv(C, s_dp.n_chunks, (a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"]),
                                (b["chunk_ptrs"], b["chunk_lengths"], b["col_idxs"], b["values"]), xp)
    return pkg.apply_permutation(y, a["old_to_new_idx"]), coo_dp.nnz, coo_sp.nnz


@pytest.mark.parametrize("name,P,method,C,sigma", [("bcsstk13", 4, "seg-nnz", 32, 512), ("impcol_e", 2, "seg-rows", 8, 16)])
def test_halo_of_the_pair_is_the_oracles_halo_of_the_concatenated_columns(pkg, orc, name, P, method, C, sigma):
    coo = pkg.read_mtx(mtx_path(name))
    wsa = pkg.seg_work_sharing_arr(coo, method, P)
    for rank in range(P):
        loc = pkg.seg_local_coo(coo, wsa, rank)
        s_dp, s_sp, coo_dp, coo_sp = ap_pair(pkg, loc, C, sigma, 1.0)
        assert coo_dp.nnz > 0 and coo_sp.nnz > 0, (name, rank)
        n_dp = s_dp.n_elements
        both = np.concatenate([s_dp.arrays()["col_idxs"], s_sp.arrays()["col_idxs"]]).astype(np.int32)
        n_halo, recv, cum = orc.collect_local_needed_heri(both, wsa, rank, P, coo.n_cols)
        h = pkg.halo_discover_ap(s_dp, s_sp, wsa, rank, P)
        assert h.n_halo == n_halo and h.n_local == wsa[rank + 1] - wsa[rank]
        assert np.array_equal(h.recv_counts_cumsum, cum)
        for p in range(P):
            assert np.array_equal(h.recv_idxs_of(p), recv[p]), (name, rank, p)
        assert np.array_equal(s_dp.arrays()["col_idxs"], both[:n_dp]) and np.array_equal(s_sp.arrays()["col_idxs"], both[n_dp:])
        if rank > 0:                      # both parts' padding asks for global column 0: one slot, one number
            assert n_halo > 0


def test_halo_of_a_pair_with_different_chunk_counts_is_refused(pkg):
    coo = pkg.read_mtx(mtx_path("impcol_e"))
    wsa = pkg.seg_work_sharing_arr(coo, "seg-rows", 2)
    loc = pkg.seg_local_coo(coo, wsa, 0)
    s_dp, s_sp, _, coo_sp = ap_pair(pkg, loc, 8, 16, 1.0)
    other = pkg.convert_to_scs(coo_sp, 4, 16, pkg.F32)
    assert other.n_chunks != s_dp.n_chunks
    before = s_dp.arrays()["col_idxs"].copy()
    with pytest.raises(pkg.UspmvError, match="share C, n_chunks"):
        pkg.halo_discover_ap(s_dp, other, wsa, 0, 2)
    assert np.array_equal(s_dp.arrays()["col_idxs"], before)     # refused before anything was rewritten
    with pytest.raises(pkg.UspmvError):
        pkg.halo_discover_ap(s_dp, s_dp, wsa, 0, 2)              # one struct twice is no pair


def test_dist_check_reference_ap_is_the_oracles_whole_matrix_product(pkg, orc):
    shape, P, C, sigma, thr = (24, 24, 24), 2, 32, 512, 1e-3
    coo = pkg.gen_stencil27(*shape, magnitude_decades=6.0)
    n = coo.n_rows
    wsa = pkg.seg_work_sharing_arr(coo, "seg-rows", P)
    y_ref, n_dp, n_sp = whole_matrix_ap_reference(pkg, orc, coo, C, sigma, thr, make_x(n))
    assert n_dp > 0 and n_sp > 0                                  # the split is not vacuous
    y0, n_dp0, n_sp0 = whole_matrix_ap_reference(pkg, orc, coo, C, sigma, 0.0, make_x(n))
    assert n_sp0 == 0 and n_dp0 == coo.nnz and not np.array_equal(y0, y_ref)
    for rank in range(P):
        loc = pkg.seg_local_coo(coo, wsa, rank)
        rows = slice(int(wsa[rank]), int(wsa[rank + 1]))
        assert np.array_equal(pkg.dist_check_reference_ap(loc, wsa, rank, P, thr), y_ref[rows]), rank
        got0 = pkg.dist_check_reference_ap(loc, wsa, rank, P, 0.0)
        assert np.array_equal(got0, y0[rows]) and np.array_equal(got0, pkg.dist_check_reference(loc, wsa, rank, P, pkg.F64))
    with pytest.raises(pkg.UspmvError):
        pkg.dist_check_reference_ap(loc, wsa, P, P, thr)


def test_new_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "uspmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(uspmv_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(pkg.library_path())
    from ultimate_spmv_amd import binding
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name) and name in binding._SIGS, name
