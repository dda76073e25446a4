"""Equilibrated adaptive precision on the device: uspmv_equilibrate_device (csrc/equilibrate_kernels.hip) against
uspmv_coo_equilibrate_scales, uspmv_partition_precisions_device_eq against uspmv_partition_precisions_eq, and the one-call set-up
uspmv_convert_to_scs_device_ap_from_arrays_eq against the host route (equilibrate_scales -> partition_precisions_eq -> convert_to_scs with
the first part's permutation -> permute_scs_cols -> upload).  Every comparison is on bits.  The shapes are the smallest at which each
mechanism of the kernels can break: a lane holds two neighbouring entries, a wave 128, a workgroup 512 (equilibration) or 1024 (partition)."""
import numpy as np
import pytest

from test_ap_equilibrated_host import (CASES, KINDS, assert_parts, case_arrays, np_partition_eq, quantile_thresholds, rect_case, refused_cases,
                                       same_bits)
from test_gpu_ap_device_setup import _plan, _tup, _xp, _y, big_random, bits, host_structs, same_handles
from test_gpu_ap_hp import _oracle as hp_oracle, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


def up(t, a, offset=False):
    """device copy; offset: starting at an odd element, so that the kernels' 16-byte loads are not aligned"""
    a = np.ascontiguousarray(a)
    return t.from_numpy(np.concatenate([a[:1], a])).cuda()[1:] if offset and a.size else t.from_numpy(a.copy()).cuda()


def short_rows(rng, nnz, n_cols=97):
    """nnz entries as rows of 1 .. 3 entries"""
    lens = []
    while sum(lens) < nnz:
        lens.append(min(int(rng.integers(1, 4)), nnz - sum(lens)))
    n_rows = max(len(lens), 1)
    I = np.repeat(np.arange(len(lens)), lens).astype(np.int32)
    J = rng.integers(0, n_cols, nnz).astype(np.int32)
    V = rng.standard_normal(nnz) * 10.0 ** rng.uniform(-5, 3, nnz)
    return n_rows, n_cols, I, J, V


def check_equilibrate(pkg, t, case, in_place=False, offset=False):
    n_rows, n_cols, I, J, V = case
    m = pkg.Coo.from_arrays(n_rows, n_cols, I, J, V)
    r, c = m.equilibrate_scales()
    want = m.arrays()[2]
    dI, dJ, dV = up(t, I, offset), up(t, J, offset), up(t, V, offset)
    out, dr, dc = pkg.equilibrate_device(dI, dJ, dV, n_rows, n_cols, out=dV if in_place else None)
    assert V.size == 0 or (out.data_ptr() == dV.data_ptr()) == in_place
    assert same_bits(out.cpu().numpy(), want), "scaled values"
    assert same_bits(dr.cpu().numpy(), r), "row_max"
    assert same_bits(dc.cpu().numpy(), c), "col_max"
    if not in_place:
        assert same_bits(dV.cpu().numpy(), V), "the input is left alone"
    return (dI, dJ, out, dr, dc), (m, r, c)


# ------------------------------------------------------------------------------------------------ equilibrate_device
@pytest.mark.parametrize("nnz", (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049))
def test_equilibrate_sizes_around_the_wave_and_the_workgroup(pkg, t, nnz):
    case = short_rows(np.random.default_rng(100 + nnz), nnz)
    check_equilibrate(pkg, t, case)
    check_equilibrate(pkg, t, case, in_place=True)
    check_equilibrate(pkg, t, case, offset=True)                      # the unaligned, non-vector load path
    check_equilibrate(pkg, t, case, in_place=True, offset=True)


def test_equilibrate_long_row_across_workgroups(pkg, t):
    """one row of 2 500 entries (entries 400 .. 2899) among short ones: a run across six workgroups of 512 entries, its maximum in turn
    in every one of them"""
    rng = np.random.default_rng(7)
    for peak in (400, 600, 1100, 1700, 2200, 2899):
        n_rows, n_cols, I, J, V = short_rows(rng, 400, n_cols=3001)
        I2 = np.concatenate([I, np.full(2500, n_rows), I[:50] + n_rows + 1]).astype(np.int32)
        J2 = np.concatenate([J, np.arange(2500), J[:50]]).astype(np.int32)
        V2 = np.concatenate([V, rng.standard_normal(2500), V[:50]])
        V2[peak] = 1e4
        case = (int(I2.max()) + 1, n_cols, I2, J2, V2)
        check_equilibrate(pkg, t, case)
        check_equilibrate(pkg, t, case, offset=True)


def test_equilibrate_one_entry_rows_and_one_column(pkg, t):
    rng = np.random.default_rng(8)
    n = 3000
    V = rng.standard_normal(n) * 10.0 ** rng.uniform(-5, 3, n)
    k = np.arange(n, dtype=np.int32)
    check_equilibrate(pkg, t, (n, n, k, ((k * 7) % n).astype(np.int32), V))                   # 64 runs per wave
    # every candidate of the column pass to one address: row-scaled, each is 1.0, so only the first to arrive sets a record
    check_equilibrate(pkg, t, (n, 1, k, np.zeros(n, np.int32), V))
    # ... and with rows of several entries the candidates differ: ascending magnitudes, every one a record when taken in order
    n_rows, _, I, _, _ = short_rows(rng, n)
    Vasc = np.sort(np.abs(V)) * np.where(k % 2 == 0, 1.0, -1.0)
    check_equilibrate(pkg, t, (n_rows, 1, I, np.zeros(n, np.int32), Vasc))
    check_equilibrate(pkg, t, (n_rows, 1, I, np.zeros(n, np.int32), Vasc[::-1].copy()))
    # a single row holding everything, and empty rows between the runs
    check_equilibrate(pkg, t, (1, n, np.zeros(n, np.int32), k, V))
    check_equilibrate(pkg, t, (5 * n_rows, 1, (I * 5).astype(np.int32), np.zeros(n, np.int32), V))


@pytest.mark.parametrize("name", CASES + ("stencil_decades",))
def test_equilibrate_matrices(pkg, t, name):
    if name == "stencil_decades":
        m = pkg.gen_stencil27(9, 11, 13, magnitude_decades=6.0)
        case = (m.n_rows, m.n_cols) + tuple(a.copy() for a in m.arrays())
    else:
        case = case_arrays(pkg, name)
    (_, _, _, dr, dc), _ = check_equilibrate(pkg, t, case)
    if name.startswith("rect"):
        assert (dr == 0).any() and (dc == 0).any()                    # empty rows and columns
    check_equilibrate(pkg, t, case, in_place=True)


def test_equilibrate_refusals_leave_the_output_alone(pkg, t):
    cases = dict(refused_cases())
    n_rows, n_cols, I, J, V = rect_case(37, 53, 3753)
    swapped = I.copy(); swapped[[10, 40]] = swapped[[40, 10]]
    assert np.any(np.diff(swapped) < 0)
    cases["unsorted"] = (n_rows, n_cols, swapped, J, V)
    far = J.copy(); far[V.size // 2] = n_cols
    cases["column_out_of_range"] = (n_rows, n_cols, I, far, V)
    neg = I.copy(); neg[0] = -1
    cases["row_out_of_range"] = (n_rows, n_cols, neg, J, V)
    status = dict(unsorted=3)
    for what, (n_rows, n_cols, I, J, V) in cases.items():
        dI, dJ, dV = up(t, I), up(t, J), up(t, V)
        out = t.full_like(dV, 7.0)
        with pytest.raises(pkg.UspmvError) as e:
            pkg.equilibrate_device(dI, dJ, dV, n_rows, n_cols, out=out)
        assert e.value.status == status.get(what, 1), what
        assert bool((out == 7.0).all()), what
        keep = dV.clone()
        with pytest.raises(pkg.UspmvError):
            pkg.equilibrate_device(dI, dJ, dV, n_rows, n_cols, out=dV)
        assert same_bits(dV.cpu().numpy(), keep.cpu().numpy()), what
    # an explicit zero whose column has other entries is no refusal (the rare second look at the columns comes back clean)
    n_rows, n_cols, I, J, V = rect_case(37, 53, 3753)
    k = np.flatnonzero((np.bincount(I)[I] >= 2) & (np.bincount(J)[J] >= 2))[0]       # neither its row nor its column is left all zero
    V[k] = 0.0
    check_equilibrate(pkg, t, (n_rows, n_cols, I, J, V))


# ------------------------------------------------------------------------------------------------ partition_precisions_device_eq
def partition_cases(pkg):
    out = [(name, case_arrays(pkg, name)) for name in CASES + ("pow2",)]
    for name, m in (("stencil_decades", pkg.gen_stencil27(9, 11, 13, magnitude_decades=6.0)), ("random2000", big_random(pkg))):
        out.append((name, (m.n_rows, m.n_cols) + tuple(a.copy() for a in m.arrays())))
    return out


@pytest.fixture(scope="module")
def scaled(pkg, t):
    """name -> (device I, J, scaled V, row_max, col_max), (host Coo scaled, r, c, I, J, V scaled): equilibrated once, on both sides"""
    out = {}
    for name, case in partition_cases(pkg):
        dev, (m, r, c) = check_equilibrate(pkg, t, case)
        out[name] = (dev, (m, r, c, case[2], case[3], m.arrays()[2].copy()))
    return out


def case_thresholds(name, kind, I, J, V, r, c):
    return (1.0, 2.0 ** -4) if name == "pow2" else quantile_thresholds(kind, I, J, V, r, c)


def dev_parts(got):
    return [None if g is None else tuple(a.cpu().numpy() for a in g) for g in got]


@pytest.mark.parametrize("kind", KINDS)
def test_partition_device_eq(pkg, t, scaled, kind):
    for name, ((dI, dJ, dV, dr, dc), (m, r, c, I, J, V)) in scaled.items():
        t1, t2 = case_thresholds(name, kind, I, J, V, r, c)
        part, stored, (av, T1, T2) = np_partition_eq(kind, I, J, V, r, c, t1, t2)
        if name == "pow2":
            assert np.count_nonzero(av == T1) > 0 and np.count_nonzero(av == T2) > 0
        got = dev_parts(pkg.partition_precisions_device_eq(dI, dJ, dV, m.n_rows, m.n_cols, kind, t1, t2, dr, dc))
        want = [None if q is None else tuple(a.copy() for a in q.arrays()) for q in pkg.partition_precisions_eq(m, kind, t1, t2, r, c)]
        assert_parts(got, kind, I, J, V, part, stored, f"{name} {kind} (restatement)")
        for p in range(3):
            assert (got[p] is None) == (want[p] is None)
            if got[p] is not None:
                assert np.array_equal(got[p][0], want[p][0]) and np.array_equal(got[p][1], want[p][1]) and same_bits(got[p][2], want[p][2]), (name, kind, p)
    # offset arrays: the non-vector load path of both passes
    (dI, dJ, dV, dr, dc), (m, r, c, I, J, V) = scaled["impcol_e"]
    t1, t2 = case_thresholds("impcol_e", kind, I, J, V, r, c)
    part, stored, _ = np_partition_eq(kind, I, J, V, r, c, t1, t2)
    got = dev_parts(pkg.partition_precisions_device_eq(up(t, I, True), up(t, J, True), up(t, V, True), m.n_rows, m.n_cols, kind, t1, t2, dr, dc))
    assert_parts(got, kind, I, J, V, part, stored, f"offset {kind}")


@pytest.mark.parametrize("kind", ("dp_hp", "sp_hp", "dp_sp_hp"))
def test_partition_device_eq_nan_goes_to_lo(pkg, t, scaled, kind):
    """a NaN falls through to the plain else; the hp part's value goes through the integer rounding routine, the same text on both sides"""
    (dI, dJ, dV, dr, dc), (m, r, c, I, J, V) = scaled["rect_37x53"]
    V = V.copy()
    k = V.size // 2
    V[k] = np.nan
    t1, t2 = quantile_thresholds(kind, I, J, V, r, c)
    mh = pkg.Coo.from_arrays(m.n_rows, m.n_cols, I, J, V)
    want = pkg.partition_precisions_eq(mh, kind, t1, t2, r, c)
    got = dev_parts(pkg.partition_precisions_device_eq(dI, dJ, up(t, V), m.n_rows, m.n_cols, kind, t1, t2, dr, dc))
    assert np.count_nonzero(np.isnan(got[2][2])) == 1 and not np.isnan(got[0][2]).any()
    for p in range(3):
        if want[p] is not None:
            wI, wJ, wV = want[p].arrays()
            assert np.array_equal(got[p][0], wI) and np.array_equal(got[p][1], wJ) and same_bits(got[p][2], wV), (kind, p)


def test_partition_device_eq_checks_its_indices(pkg, t, scaled):
    (dI, dJ, dV, dr, dc), (m, r, c, I, J, V) = scaled["rect_37x53"]
    far = J.copy(); far[3] = m.n_cols + 1000000
    with pytest.raises(pkg.UspmvError, match="column index"):
        pkg.partition_precisions_device_eq(dI, up(t, far), dV, m.n_rows, m.n_cols, "dp_sp", 1.0, 0.0, dr, dc)
    neg = I.copy(); neg[0] = -5
    with pytest.raises(pkg.UspmvError, match="row index"):
        pkg.partition_precisions_device_eq(up(t, neg), dJ, dV, m.n_rows, m.n_cols, "dp_hp", 1.0, 0.0, dr, dc)


# ------------------------------------------------------------------------------------------------ the one-call set-up
@pytest.mark.parametrize("kind", KINDS)
def test_one_call_eq_equals_the_host_route(pkg, orc, t, scaled, kind):
    compared = ran = 0
    for name in ("bcsstk13", "stencil_decades", "rect_37x53"):
        (dI, dJ, dV, dr, dc), (m, r, c, I, J, V) = scaled[name]
        t1, t2 = case_thresholds(name, kind, I, J, V, r, c)
        parts = pkg.partition_precisions_eq(m, kind, t1, t2, r, c)
        for C, sigma in ((1, 1), (32, 512), (5, 7), (64, 128)):
            structs = host_structs(pkg, parts, kind, C, sigma)
            if structs is None:                           # where the host route refuses, the device route refuses alike
                with pytest.raises(pkg.UspmvError, match="padded slot"):
                    pkg.convert_ap_device_from_arrays_eq(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, kind, t1, t2, dr, dc)
                continue
            lay, hand, o2n, n2o, cnt = pkg.convert_ap_device_from_arrays_eq(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, kind, t1, t2, dr, dc)
            assert cnt == [p.nnz if p is not None else 0 for p in parts], (name, C, sigma)
            same_handles(pkg, structs, hand, (name, kind, C, sigma))
            a, la = structs[0].arrays(), lay.arrays()
            assert (lay.C, lay.sigma, lay.n_rows, lay.n_cols, lay.n_rows_padded, lay.n_chunks, lay.n_elements, lay.nnz, lay.dtype) == \
                   (C, sigma, m.n_rows, m.n_cols, structs[0].n_rows_padded, structs[0].n_chunks, structs[0].n_elements, parts[0].nnz, structs[0].dtype)
            for k in ("chunk_ptrs", "chunk_lengths", "old_to_new_idx", "new_to_old_idx"):
                assert np.array_equal(la[k], a[k]), (name, C, sigma, k)
            assert np.array_equal(o2n.cpu().numpy(), a["old_to_new_idx"]) and np.array_equal(n2o.cpu().numpy(), a["new_to_old_idx"])
            compared += 1
            if m.n_rows != m.n_cols:
                continue
            xp = _xp(structs, kind, m.n_rows)
            if kind == "dp_sp":
                want = orc.spmv_scs_ap_adv(C, structs[0].n_chunks, _tup(structs[0].arrays(), np.float64), _tup(structs[2].arrays(), np.float32), xp)
            else:
                want = hp_oracle(orc, kind, (structs[0], structs[1], structs[2]), xp)
            for planned in (False, True):
                if planned:
                    _plan(pkg, kind, hand)
                assert _same(_y(pkg, t, kind, hand, xp), want), (name, C, sigma, planned)
            ran += 1
    assert compared >= 8 and ran >= 6, (compared, ran)


def test_one_call_eq_with_null_vectors_is_the_unscaled_function(pkg, t, scaled):
    """the existing function is the same body with both pointers NULL: asked through the _eq symbol, it gives the unscaled handles"""
    import ctypes as C
    (dI, dJ, dV, dr, dc), (m, r, c, I, J, V) = scaled["impcol_e"]
    t1 = float(np.quantile(np.abs(V), 0.6))
    _, want, _, _, cnt_w = pkg.convert_ap_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, 32, 512, "dp_sp", t1)
    hh, hm, hl = C.c_void_p(), C.c_void_p(), C.c_void_p()
    cnt = (C.c_int64 * 3)()
    rc = pkg.lib().uspmv_convert_to_scs_device_ap_from_arrays_eq(dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), m.n_rows, m.n_cols, V.size, 32, 512,
                                                                pkg.AP_DP_SP, t1, 0.0, None, None, pkg.SORT_HOST, None, None, None, None, cnt,
                                                                C.byref(hh), C.byref(hm), C.byref(hl))
    assert rc == 0 and list(cnt) == cnt_w and not hm.value
    try:
        for h, w in ((hh, want[0]), (hl, want[2])):
            cp = np.empty(w.n_chunks + 1, np.int32); cl = np.empty(w.n_chunks, np.int32); ci = np.empty(w.n_elements, np.int32)
            va = np.empty(w.n_elements, np.float64 if w.dtype == pkg.F64 else np.float32)
            assert pkg.lib().uspmv_dmat_download(h, cp.ctypes.data, cl.ctypes.data, ci.ctypes.data, va.ctypes.data) == 0
            d = pkg.dmat_download(w)
            assert np.array_equal(cp, d["chunk_ptrs"]) and np.array_equal(cl, d["chunk_lengths"]) and np.array_equal(ci, d["col_idxs"])
            assert np.array_equal(bits(va), bits(d["values"]))
    finally:
        pkg.lib().uspmv_dmat_free(hh); pkg.lib().uspmv_dmat_free(hl)
