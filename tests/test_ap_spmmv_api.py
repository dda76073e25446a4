"""The C ABI of adaptive-precision SpMMV (uspmv_spmmv_ap, uspmv_spmmv_ap_plan_lines): declared in include/uspmv.h, exported by
libuspmv.so, and refusing bad arguments with a status code and a uspmv_last_error text before any device is needed."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _header():
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        return f.read()


def test_declared_in_the_header_and_exported(pkg):
    h = _header()
    assert re.search(r"\bint\s+uspmv_spmmv_ap\s*\(\s*const uspmv_dmat_t \*dp,\s*const uspmv_dmat_t \*sp,\s*const void \*d_X,\s*void \*d_Y,\s*int b,"
                     r"\s*int64_t ld,\s*int layout,\s*void \*stream\s*\)\s*;", h)
    assert re.search(r"\bint\s+uspmv_spmmv_ap_plan_lines\s*\(\s*int b,\s*int \*max_lines\s*\)\s*;", h)
    L = pkg.lib()
    assert L.uspmv_spmmv_ap is not None and L.uspmv_spmmv_ap_plan_lines is not None
    assert callable(pkg.spmmv_ap) and callable(pkg.spmmv_ap_plan_lines)


def test_null_handles_are_refused_without_a_device(pkg):
    L = pkg.lib()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    for lay in (pkg.COLWISE, pkg.ROWWISE):
        rc = L.uspmv_spmmv_ap(None, None, p, p, 4, 0, lay, None)
        assert rc != 0
        assert b"uspmv_spmmv_ap" in L.uspmv_last_error()


def test_plan_lines_arguments(pkg):
    L = pkg.lib()
    n = C.c_int(-1)
    for b in (0, -3):
        assert L.uspmv_spmmv_ap_plan_lines(b, C.byref(n)) != 0
        assert b"uspmv_spmmv_ap_plan_lines" in L.uspmv_last_error()
    assert L.uspmv_spmmv_ap_plan_lines(4, None) != 0
    assert b"uspmv_spmmv_ap_plan_lines" in L.uspmv_last_error()
    for b in (1, 2, 3, 4, 8, 16, 17):
        assert L.uspmv_spmmv_ap_plan_lines(b, C.byref(n)) == 0
        # a staged tile holds max_lines * 16 X rows of at least two doubles (two vectors per pass at the least) in LDS: never beyond
        # the 160 KiB a gfx950 workgroup can have; widths without a B-specialised kernel have no staged kernel either
        assert 0 <= n.value and n.value * 128 * 2 <= 160 * 1024
        if b not in (2, 4, 8, 16): assert n.value == 0
        assert pkg.spmmv_ap_plan_lines(b) == n.value
    with pytest.raises(pkg.UspmvError):
        pkg.spmmv_ap_plan_lines(0)
