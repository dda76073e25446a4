"""The C ABI around the sweep path of adaptive-precision SpMMV (uspmv_spmmv_ap_path, uspmv_spmmv_ap_sweep_vectors): declared in
include/uspmv.h, exported by libuspmv.so, bound by the package, refusing bad arguments with a status code and a uspmv_last_error text
before any device is needed; and the pure function's values."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _header():
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        return f.read()


def test_declared_in_the_header_exported_and_bound(pkg):
    h = _header()
    assert re.search(r"\bint\s+uspmv_spmmv_ap_path\s*\(\s*const uspmv_dmat_t \*dp,\s*const uspmv_dmat_t \*sp,\s*int b,\s*int64_t ld,\s*int layout,"
                     r"\s*int \*path,\s*int \*vectors_per_pass\s*\)\s*;", h)
    assert re.search(r"\bint\s+uspmv_spmmv_ap_sweep_vectors\s*\(\s*int b,\s*int wlog,\s*int \*vectors\s*\)\s*;", h)
    L = pkg.lib()
    assert L.uspmv_spmmv_ap_path is not None and L.uspmv_spmmv_ap_sweep_vectors is not None
    assert callable(pkg.spmmv_ap_path) and callable(pkg.spmmv_ap_sweep_vectors)
    with open(os.path.join(ROOT, "include", "uspmv_interface.hpp")) as f:
        hpp = f.read()
    assert "uspmv_spmmv_ap_path(" in hpp and "uspmv_spmmv_ap_sweep_vectors(" in hpp


def test_path_refuses_null_handles_and_bad_arguments_without_a_device(pkg):
    L = pkg.lib()
    path, vec = C.c_int(-1), C.c_int(-1)
    for b, lay in ((4, pkg.COLWISE), (4, pkg.ROWWISE), (0, pkg.ROWWISE), (-2, pkg.COLWISE), (4, 7)):
        rc = L.uspmv_spmmv_ap_path(None, None, b, 0, lay, C.byref(path), C.byref(vec))
        assert rc != 0
        assert b"uspmv_spmmv_ap_path" in L.uspmv_last_error()
        assert (path.value, vec.value) == (-1, -1)            # nothing reported on a refusal


def test_sweep_vectors_arguments(pkg):
    L = pkg.lib()
    n = C.c_int(-1)
    for b, wlog in ((0, 12), (-3, 12), (4, 7), (4, 17), (4, -1)):
        assert L.uspmv_spmmv_ap_sweep_vectors(b, wlog, C.byref(n)) != 0
        assert b"uspmv_spmmv_ap_sweep_vectors" in L.uspmv_last_error()
    assert L.uspmv_spmmv_ap_sweep_vectors(4, 12, None) != 0
    assert b"uspmv_spmmv_ap_sweep_vectors" in L.uspmv_last_error()
    with pytest.raises(pkg.UspmvError):
        pkg.spmmv_ap_sweep_vectors(0, 12)
    with pytest.raises(pkg.UspmvError):
        pkg.spmmv_ap_sweep_vectors(4, 7)


def test_sweep_vectors_values(pkg):
    L = pkg.lib()
    n = C.c_int(-1)
    for b in (1, 2, 3, 4, 8, 16, 17):
        for wlog in range(8, 17):
            assert L.uspmv_spmmv_ap_sweep_vectors(b, wlog, C.byref(n)) == 0
            v = n.value
            assert v == 0 or v in (2, 4, 8)
            if v:
                # whole passes over the b vectors, and one window of v vectors (2^wlog doubles each) within the 160 KiB of a gfx950 workgroup
                assert v <= b and b % v == 0 and (8 << wlog) * v <= 160 * 1024
                # ... and the largest such
                assert all(not (w <= b and b % w == 0 and (8 << wlog) * w <= 160 * 1024) for w in (2, 4, 8) if w > v)
            if b not in (2, 4, 8, 16) or wlog >= 14: assert v == 0
            else: assert v >= 2
            assert pkg.spmmv_ap_sweep_vectors(b, wlog) == v
    # the default pair plan's windows (2^13 doubles) serve two vectors per pass, 2^12 four, 2^11 eight
    assert [pkg.spmmv_ap_sweep_vectors(16, w) for w in (13, 12, 11)] == [2, 4, 8]
