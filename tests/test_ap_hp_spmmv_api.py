"""The C ABI of adaptive-precision SpMMV with an fp16 part (uspmv_spmmv_ap_hp, uspmv_spmmv_ap_hp_path, uspmv_spmmv_ap_hp_plan_lines):
declared in include/uspmv.h, exported by libuspmv.so, and refusing bad arguments with a status code and a uspmv_last_error text that
begins with the function's name, before any device is needed."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HANDLES = r"\s*const uspmv_dmat_t \*hi,\s*const uspmv_dmat_t \*mid,\s*const uspmv_dmat_t \*hp,"


def _header():
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        return f.read()


def test_declared_in_the_header_and_exported(pkg):
    h = _header()
    assert re.search(r"\bint\s+uspmv_spmmv_ap_hp\s*\(" + HANDLES + r"\s*const void \*d_X,\s*void \*d_Y,\s*int b,\s*int64_t ld,\s*int layout,"
                     r"\s*void \*stream\s*\)\s*;", h)
    assert re.search(r"\bint\s+uspmv_spmmv_ap_hp_path\s*\(" + HANDLES + r"\s*int b,\s*int64_t ld,\s*int layout,\s*int \*path,"
                     r"\s*int \*vectors_per_pass\s*\)\s*;", h)
    assert re.search(r"\bint\s+uspmv_spmmv_ap_hp_plan_lines\s*\(\s*int b,\s*int x_dtype,\s*int \*max_lines\s*\)\s*;", h)
    L = pkg.lib()
    assert L.uspmv_spmmv_ap_hp is not None and L.uspmv_spmmv_ap_hp_path is not None and L.uspmv_spmmv_ap_hp_plan_lines is not None
    assert callable(pkg.spmmv_ap_hp) and callable(pkg.spmmv_ap_hp_path) and callable(pkg.spmmv_ap_hp_plan_lines)


def test_null_handles_are_refused_without_a_device(pkg):
    L = pkg.lib()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    path, vec = C.c_int(-1), C.c_int(-1)
    for lay in (pkg.COLWISE, pkg.ROWWISE):
        assert L.uspmv_spmmv_ap_hp(None, None, None, p, p, 4, 0, lay, None) != 0
        assert L.uspmv_last_error().startswith(b"uspmv_spmmv_ap_hp:")
        assert L.uspmv_spmmv_ap_hp_path(None, None, None, 4, 0, lay, C.byref(path), C.byref(vec)) != 0
        assert L.uspmv_last_error().startswith(b"uspmv_spmmv_ap_hp_path:")
    assert (path.value, vec.value) == (-1, -1)


def test_plan_lines_values(pkg):
    """two vectors of the fullest tile (16 X rows per line) in the 160 KiB of LDS: 640 lines of doubles, 1280 of floats, at the widths
    that have a staged kernel; 0 at every other"""
    L = pkg.lib()
    n = C.c_int(-1)
    for dtype, size, want in ((pkg.F64, 8, 640), (pkg.F32, 4, 1280)):
        for b in (1, 2, 3, 4, 5, 8, 13, 16, 17, 32):
            assert L.uspmv_spmmv_ap_hp_plan_lines(b, dtype, C.byref(n)) == 0
            assert n.value == (want if b in (2, 4, 8, 16) else 0), (dtype, b, n.value)
            assert n.value <= 160 * 1024 // (32 * size)
            assert pkg.spmmv_ap_hp_plan_lines(b, dtype) == n.value


def test_plan_lines_refusals(pkg):
    L = pkg.lib()
    n = C.c_int(-1)
    for b in (0, -3):
        assert L.uspmv_spmmv_ap_hp_plan_lines(b, pkg.F64, C.byref(n)) != 0
        assert L.uspmv_last_error().startswith(b"uspmv_spmmv_ap_hp_plan_lines:")
    for dtype in (pkg.F16, 3, -1):
        assert L.uspmv_spmmv_ap_hp_plan_lines(4, dtype, C.byref(n)) != 0
        assert L.uspmv_last_error().startswith(b"uspmv_spmmv_ap_hp_plan_lines:")
    assert L.uspmv_spmmv_ap_hp_plan_lines(4, pkg.F64, None) != 0
    assert L.uspmv_last_error().startswith(b"uspmv_spmmv_ap_hp_plan_lines:")
    assert n.value == -1
    with pytest.raises(pkg.UspmvError):
        pkg.spmmv_ap_hp_plan_lines(0, pkg.F64)
    with pytest.raises(pkg.UspmvError):
        pkg.spmmv_ap_hp_plan_lines(4, pkg.F16)
