"""Host side of the distributed step of the adaptive-precision kinds with an fp16 part (ap[dp_hp], ap[sp_hp], ap[dp_sp_hp]): the one halo
of the two or three parts (uspmv_halo_discover_ap_hp) against the oracle's collect_local_needed_heri on the concatenated column arrays,
the host reference of the self-check (uspmv_dist_check_reference_ap_hp) against the oracle's whole-matrix product composed part by part
(_oracle of test_gpu_ap_hp.py), and the new symbols of the C ABI.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, make_x, mtx_path
from test_gpu_ap_hp import KINDS, _build, _oracle, _same

NEW_SYMBOLS = ("uspmv_spmv_ap_hp_tiles", "uspmv_spmv_ap_hp_chunks", "uspmv_halo_discover_ap_hp", "uspmv_dist_create_ap_hp_from_coo",
               "uspmv_dist_create_ap_hp_from_coo_ex", "uspmv_dist_check_reference_ap_hp", "uspmv_dist_parts_ap_hp")
DEC, T1, T2 = 6.0, 2.4, 0.016            # gen_stencil27(magnitude_decades=6): |v| in 1e-4 .. 100; 30 % hi, 35 % mid, 35 % hp
# (matrix, P, seg method, C, sigma, (t1, t2)): every block is accepted by the host route with all parts non-empty
MTX_CASES = [("bcsstk13", 4, "seg-nnz", 32, 512, (1.0, 0.01)), ("impcol_e", 2, "seg-rows", 8, 16, (1.0, 0.0315967))]


def hp_parts(pkg, coo, kind, C, sigma, t1, t2):
    """the host set-up of a split up to (not including) the column steps: partition -> hi struct -> the other parts with hi's permutation.
    ((hi, mid | None, hp) structs, (hi, mid | None, hp) COO parts)"""
    hi, mid, hp = pkg.partition_precisions_hp(coo, kind, t1, t2)
    sh = pkg.convert_to_scs(hi, C, sigma, pkg.F32 if kind == "sp_hp" else pkg.F64)
    perm = sh.arrays()["old_to_new_idx"].copy()
    sm = pkg.convert_to_scs(mid, C, sigma, pkg.F32, fixed_permutation=perm) if mid is not None else None
    sq = pkg.convert_to_scs(hp, C, sigma, pkg.F16, fixed_permutation=perm)
    return (sh, sm, sq), (hi, mid, hp)


def assert_parts_not_vacuous(coos, kind):
    """every part has entries, and the hp part holds normal binary16 numbers that really round (no overflow, no subnormal)"""
    hi, mid, hp = coos
    assert hi.nnz > 0 and hp.nnz > 0 and (mid is None) == (kind != "dp_sp_hp") and (mid is None or mid.nnz > 0), kind
    return hi.nnz, 0 if mid is None else mid.nnz, hp.nnz


def whole_matrix_ap_hp_reference(pkg, orc, coo, kind, C, sigma, t1, t2, x_global):
    """y (original order, float32 for sp_hp) of the oracle's part-by-part composition on the WHOLE matrix, set up the host way"""
    b = _build(pkg, coo, kind, C, sigma, t1, t2)
    assert b is not None
    structs, _ = b
    a = structs[0].arrays()
    xp = np.zeros(structs[0].n_rows_padded)
    xp[:coo.n_rows] = pkg.apply_permutation(np.ascontiguousarray(x_global, np.float64), a["new_to_old_idx"])
    if kind == "sp_hp":
        xp = xp.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.ascontiguousarray(_oracle(orc, kind, structs, xp))
    nnz = tuple(0 if s is None else s.nnz for s in structs)
    assert nnz[0] > 0 and nnz[2] > 0 and (kind != "dp_sp_hp" or nnz[1] > 0), (kind, nnz)
    return pkg.apply_permutation(y, a["old_to_new_idx"]), nnz


def test_stencil_inputs_split_into_three_real_parts(pkg):
    """the inputs the GPU tests rely on: at (T1, T2) the stencil's entries go 30 / 35 / 35 % to hi / mid / hp, and the hp values are normal
    binary16 numbers that differ from the double they were rounded from"""
    coo = pkg.gen_stencil27(24, 24, 24, magnitude_decades=DEC)
    v = np.abs(np.asarray(coo.arrays()[2]))
    hi, mid, hp = pkg.partition_precisions_hp(coo, "dp_sp_hp", T1, T2)
    fr = np.array([hi.nnz, mid.nnz, hp.nnz]) / coo.nnz
    assert np.all(np.abs(fr - (0.30, 0.35, 0.35)) < 0.02), fr
    small = v[v < T2]
    q = np.abs(np.asarray(hp.arrays()[2]))
    assert len(small) == hp.nnz and np.isfinite(q).all() and q.min() >= 2.0 ** -14 and q.max() < 65504
    assert (np.sort(q) != np.sort(small)).mean() > 0.9        # rounded for real


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,P,method,C,sigma,thr", MTX_CASES)
def test_halo_of_the_parts_is_the_oracles_halo_of_the_concatenated_columns(pkg, orc, kind, name, P, method, C, sigma, thr):
    coo = pkg.read_mtx(mtx_path(name))
    wsa = pkg.seg_work_sharing_arr(coo, method, P)
    for rank in range(P):
        loc = pkg.seg_local_coo(coo, wsa, rank)
        structs, coos = hp_parts(pkg, loc, kind, C, sigma, *thr)
        assert_parts_not_vacuous(coos, kind)
        assert np.isfinite(np.asarray(coos[2].arrays()[2])).all(), (name, rank)          # no hp infinity
        parts = [s for s in structs if s is not None]
        sizes = np.cumsum([0] + [s.n_elements for s in parts])
        cat = np.concatenate([s.arrays()["col_idxs"] for s in parts]).astype(np.int32)
        n_halo, recv, cum = orc.collect_local_needed_heri(cat, wsa, rank, P, coo.n_cols)   # rewrites `cat` to the local + halo numbering
        h = pkg.halo_discover_ap_hp(structs[0], structs[1], structs[2], wsa, rank, P)
        assert h.n_halo == n_halo and h.n_local == wsa[rank + 1] - wsa[rank]
        assert np.array_equal(h.recv_counts_cumsum, cum)
        for p in range(P):
            assert np.array_equal(h.recv_idxs_of(p), recv[p]), (name, kind, rank, p)
        for k, s in enumerate(parts):                          # every struct rewritten against the one numbering
            assert np.array_equal(s.arrays()["col_idxs"], cat[sizes[k]:sizes[k + 1]]), (name, kind, rank, k)
        if rank > 0:                                           # all parts' padding asks for global column 0: one slot, one number
            assert n_halo > 0


def test_halo_of_parts_that_do_not_belong_together_is_refused(pkg):
    coo = pkg.read_mtx(mtx_path("impcol_e"))
    wsa = pkg.seg_work_sharing_arr(coo, "seg-rows", 2)
    loc = pkg.seg_local_coo(coo, wsa, 0)
    (sh, sm, sq), (_, mid, hp) = hp_parts(pkg, loc, "dp_sp_hp", 8, 16, 1.0, 0.0315967)
    other_hp = pkg.convert_to_scs(hp, 4, 16, pkg.F16)
    other_mid = pkg.convert_to_scs(mid, 4, 16, pkg.F32)
    assert other_hp.n_chunks != sh.n_chunks
    before = [s.arrays()["col_idxs"].copy() for s in (sh, sm, sq)]
    with pytest.raises(pkg.UspmvError, match="share C, n_chunks"):
        pkg.halo_discover_ap_hp(sh, sm, other_hp, wsa, 0, 2)
    with pytest.raises(pkg.UspmvError, match="share C, n_chunks"):
        pkg.halo_discover_ap_hp(sh, other_mid, sq, wsa, 0, 2)
    with pytest.raises(pkg.UspmvError, match="share C, n_chunks"):
        pkg.halo_discover_ap_hp(sh, None, other_hp, wsa, 0, 2)
    for twice in ((sh, sh, sq), (sh, sm, sh), (sh, sq, sq), (sh, None, sh)):
        with pytest.raises(pkg.UspmvError, match="one struct"):
            pkg.halo_discover_ap_hp(*twice, wsa, 0, 2)
    for s, b in zip((sh, sm, sq), before):                     # refused before anything was rewritten
        assert np.array_equal(s.arrays()["col_idxs"], b)
    assert pkg.halo_discover_ap_hp(sh, sm, sq, wsa, 0, 2).n_local == wsa[1] - wsa[0]     # and the real triple still goes through


@pytest.mark.parametrize("kind", KINDS)
def test_dist_check_reference_ap_hp_is_the_oracles_whole_matrix_composition(pkg, orc, kind):
    shape, P, C, sigma = (24, 24, 24), 2, 32, 512
    coo = pkg.gen_stencil27(*shape, magnitude_decades=DEC)
    n = coo.n_rows
    wsa = pkg.seg_work_sharing_arr(coo, "seg-rows", P)
    y_ref, nnz = whole_matrix_ap_hp_reference(pkg, orc, coo, kind, C, sigma, T1, T2, make_x(n))
    assert y_ref.dtype == (np.float32 if kind == "sp_hp" else np.float64) and not np.isnan(y_ref).any()
    for rank in range(P):
        loc = pkg.seg_local_coo(coo, wsa, rank)
        rows = slice(int(wsa[rank]), int(wsa[rank + 1]))
        got = pkg.dist_check_reference_ap_hp(loc, wsa, rank, P, kind, T1, T2)
        assert got.dtype == y_ref.dtype and _same(got, y_ref[rows]), (kind, rank)
        if kind != "sp_hp":                                    # nothing below the thresholds: the one-precision reference
            got0 = pkg.dist_check_reference_ap_hp(loc, wsa, rank, P, kind, 0.0, 0.0)
            assert np.array_equal(got0, pkg.dist_check_reference(loc, wsa, rank, P, pkg.F64)) and not np.array_equal(got0, got)
    with pytest.raises(pkg.UspmvError):
        pkg.dist_check_reference_ap_hp(loc, wsa, P, P, kind, T1, T2)
    with pytest.raises(pkg.UspmvError):
        pkg.dist_check_reference_ap_hp(loc, wsa, 0, P, pkg.AP_DP_SP, T1, T2)


def test_new_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "uspmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(uspmv_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(pkg.library_path())
    from ultimate_spmv_amd import binding
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name) and name in binding._SIGS, name
    for name in ("spmv_ap_hp_tiles", "spmv_ap_hp_chunks", "halo_discover_ap_hp", "dist_check_reference_ap_hp"):
        assert callable(getattr(pkg, name)), name
