"""Numeric refresh (new values on an unchanged pattern, plans kept), the part that needs no device: the entry points are declared in
include/uspmv.h, exported by libuspmv.so and bound by the package; their refusals come with their texts and before the device check;
Scs.update_values -- the host twin of uspmv_dmat_update_values_from_arrays -- equals a conversion of the new values under the old
struct's permutation bit for bit, and leaves the struct alone when it refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, mtx_path

INVALID, UNSUPPORTED, NO_DEVICE = 1, 3, 5
NEW = ("uspmv_dmat_values_changed", "uspmv_dmat_update_values", "uspmv_dmat_update_values_from_arrays", "uspmv_scs_update_values",
       "uspmv_raw_plan_cache_values_changed")


def new_values(I, V0):
    """V1 of the tests: every value scaled by a factor in [1.25, 1.75) that depends on its position, every third negated; then the last
    entry of every fifth row +0.0 and the first entry of every eleventh row -0.0 (stripped tails appear, signed zeros are kept).  I: the
    row indices, sorted."""
    k = np.arange(V0.size, dtype=np.uint64)
    V1 = V0 * (1.25 + ((k * np.uint64(2654435761)) % np.uint64(1024)).astype(np.float64) / 2048.0)
    V1[::3] = -V1[::3]
    first = np.flatnonzero(np.r_[True, I[1:] != I[:-1]])
    last = np.r_[first[1:], I.size] - 1
    V1[last[I[last] % 5 == 0]] = 0.0
    V1[first[I[first] % 11 == 0]] = -0.0
    assert np.isfinite(V1).all()
    return V1


def bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def test_symbols_declared_exported_bound(pkg):
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(uspmv_[a-z0-9_]+)\s*\(", hdr))
    from ultimate_spmv_amd import binding
    L = C.CDLL(pkg.library_path())
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in binding._SIGS, name
    for name, value in (("COPIES", 1), ("RECHUNKED", 2), ("SWEEP_REBUILT", 4), ("BLOCK_SWEEP_DROPPED", 8)):
        assert re.search(rf"USPMV_REFRESH_{name}\s*=\s*{value}\b", hdr) and getattr(pkg, "REFRESH_" + name) == value
    for m in ("values_changed", "update_values", "update_values_from_coo"):
        assert callable(getattr(pkg.DeviceMatrix, m))
    assert callable(pkg.Scs.update_values) and callable(pkg.raw_plan_cache_values_changed)
    with open(os.path.join(ROOT, "include", "uspmv_interface.hpp")) as f:
        text = f.read()
    assert "values_changed(void *stream" in text and "update_values_from_device_coo(" in text


def _wrapped(L, dtype):
    """a handle around HOST memory: every call on it below is refused before the arrays are read"""
    cp = np.array([0, 4], np.int32); cl = np.array([2], np.int32); ci = np.zeros(4, np.int32)
    va = np.ones(4, {0: np.float64, 1: np.float32, 2: np.uint16}[dtype])
    h = C.c_void_p()
    assert L.uspmv_dmat_wrap(2, 1, 4, dtype, cp.ctypes.data, cl.ctypes.data, ci.ctypes.data, va.ctypes.data, C.byref(h)) == 0
    return h, (cp, cl, ci, va)


def test_refusals_come_before_the_device_check(pkg):
    L = pkg.lib()
    err = lambda: L.uspmv_last_error().decode()
    I = np.zeros(4, np.int32); J = np.zeros(4, np.int32); V = np.ones(4)
    p = lambda a: None if a is None else a.ctypes.data
    acts = C.c_int(77)
    from_arrays = lambda h, dst, I=I, J=J, V=V, check=1: L.uspmv_dmat_update_values_from_arrays(h, p(I), p(J), p(V), 2, 4, None, None, check, dst, None, C.byref(acts))
    # NULL arguments
    assert L.uspmv_dmat_values_changed(None, None, C.byref(acts)) == INVALID and "NULL" in err() and acts.value == 0
    assert L.uspmv_dmat_update_values(None, p(V), None, None) == INVALID and "NULL" in err()
    assert from_arrays(None, None) == INVALID and "NULL" in err()
    assert L.uspmv_raw_plan_cache_values_changed(None, None, None) == INVALID and "NULL" in err()
    h, keep = _wrapped(L, pkg.F64)
    try:
        assert L.uspmv_dmat_update_values(h, None, None, None) == INVALID and "NULL" in err()
        assert from_arrays(h, p(keep[3]), I=None) == INVALID and "NULL" in err()
        assert from_arrays(h, p(keep[3]), V=None) == INVALID and "NULL" in err()
        assert from_arrays(h, p(keep[3]), J=None) == INVALID and "NULL" in err()
        # a wrapped handle: its caller writes the array
        assert L.uspmv_dmat_update_values(h, p(V), None, C.byref(acts)) == INVALID
        assert "write the value array and call uspmv_dmat_values_changed" in err()
        assert from_arrays(h, None) == INVALID and "uspmv_dmat_values_changed" in err() and "d_values_dst" in err()
        assert from_arrays(h, p(V)) == INVALID and "d_values_dst is not the value array of the handle" in err()
        # the handle's shape
        assert L.uspmv_dmat_update_values_from_arrays(h, p(I), p(J), p(V), 3, 4, None, None, 1, p(keep[3]), None, None) == INVALID and "chunks" in err()
        assert L.uspmv_dmat_update_values_from_arrays(h, p(I), p(J), p(V), 0, 4, None, None, 1, p(keep[3]), None, None) == INVALID and "no rows" in err()
        assert np.array_equal(keep[3], np.ones(4))
        # valid arguments reach the device check (no array is read before it)
        if pkg.device_count() == 0:
            assert L.uspmv_dmat_values_changed(h, None, C.byref(acts)) == NO_DEVICE
            assert from_arrays(h, p(keep[3])) == NO_DEVICE
    finally:
        L.uspmv_dmat_free(h)
    # an fp16 handle: the hp part of an adaptive-precision split
    h, keep = _wrapped(L, pkg.F16)
    try:
        for rc in (L.uspmv_dmat_values_changed(h, None, None), L.uspmv_dmat_update_values(h, p(V), None, None), from_arrays(h, p(keep[3]))):
            assert rc == UNSUPPORTED
        assert "fp16 handle" in err() and "uspmv_convert_to_scs_device_ap_from_arrays" in err()
    finally:
        L.uspmv_dmat_free(h)
    # no cached plan holds this pointer: nothing to do, whether or not there is a device
    n = C.c_int(5)
    assert L.uspmv_raw_plan_cache_values_changed(p(V), None, C.byref(n)) == 0 and n.value == 0


def _coo(pkg, name):
    return pkg.gen_stencil27(9, 11, 13) if name == "stencil27" else pkg.read_mtx(mtx_path(name))


def _struct_arrays(s):
    a = s.arrays()
    return [np.array(a[k]) for k in ("chunk_ptrs", "chunk_lengths", "col_idxs", "values")]


@pytest.mark.parametrize("dtype", ["dp", "sp"])
@pytest.mark.parametrize("Cs", [(1, 1), (4, 8), (32, 512)])
@pytest.mark.parametrize("name", ["FDM-2d-16", "impcol_e", "bcsstk13", "stencil27"])
def test_scs_update_values(pkg, name, Cs, dtype):
    Cc, sigma = Cs
    dt = pkg.F64 if dtype == "dp" else pkg.F32
    m0 = _coo(pkg, name)
    I, J, V0 = [np.array(a) for a in m0.arrays()]
    assert (np.diff(I) >= 0).all()
    s = pkg.convert_to_scs(m0, Cc, sigma, dt)
    o2n = np.array(s.arrays()["old_to_new_idx"])
    pkg.permute_scs_cols(s, o2n)
    before = _struct_arrays(s)
    V1 = new_values(I, V0)

    def fresh(V):
        """the conversion of the new values under the old struct's permutation (the permutations of such a struct are the identity,
        as in the reference: they are not compared)"""
        f = pkg.convert_to_scs(pkg.Coo.from_arrays(m0.n_rows, m0.n_cols, I, J, V), Cc, sigma, dt, fixed_permutation=o2n)
        pkg.permute_scs_cols(f, o2n)
        return _struct_arrays(f)

    for V in (V1, V0):                                         # there and back: stripped tails appear and disappear
        s.update_values(pkg.Coo.from_arrays(m0.n_rows, m0.n_cols, I, J, V), col_perm=o2n, check=True)
        for got, want in zip(_struct_arrays(s), fresh(V)):
            assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want))
        assert np.array_equal(np.array(s.arrays()["old_to_new_idx"]), o2n)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(_struct_arrays(s), before))

    # ---- refusals; the struct is unchanged after each
    lens = np.bincount(I, minlength=m0.n_rows)
    r = int(np.argmax(lens))                                   # the longest row fills its chunk: one entry more overruns it
    k = int(np.searchsorted(I, r, side="right"))
    bad = []
    bad.append((pkg.Coo.from_arrays(m0.n_rows, m0.n_cols, np.insert(I, k, r), np.insert(J, k, J[k - 1]), np.insert(V1, k, 1.0)), INVALID, "more entries than the chunk"))
    pair = int(np.flatnonzero((I[1:] == I[:-1]) & (J[1:] != J[:-1]))[0])
    Js = J.copy(); Js[[pair, pair + 1]] = Js[[pair + 1, pair]]
    bad.append((pkg.Coo.from_arrays(m0.n_rows, m0.n_cols, I, Js, V1), INVALID, f"entry {pair}: its column differs"))
    cut = int(np.flatnonzero(I[1:] != I[:-1])[0])              # the last entry of the first row and the first of the next
    Iu = I.copy(); Iu[[cut, cut + 1]] = Iu[[cut + 1, cut]]
    bad.append((pkg.Coo.from_arrays(m0.n_rows, m0.n_cols, Iu, J, V1), UNSUPPORTED, "sorted by row"))
    neg = pkg.Coo.from_arrays(m0.n_rows, m0.n_cols, I, J, V1)
    neg.arrays()[0][0] = -1                                    # (uspmv_coo_create refuses such an index: written behind its back)
    bad.append((neg, INVALID, "a row index lies outside [0, n_rows)"))
    for coo, status, text in bad:
        with pytest.raises(pkg.UspmvError) as e:
            s.update_values(coo, col_perm=o2n, check=True)
        assert e.value.status == status and text in str(e.value), (text, str(e.value))
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(_struct_arrays(s), before))
    # without the pattern check the swapped pair goes through: the values follow the COO order
    s.update_values(pkg.Coo.from_arrays(m0.n_rows, m0.n_cols, I, Js, V1), check=False)
    assert np.array_equal(bits(_struct_arrays(s)[3]), bits(fresh(V1)[3]))
