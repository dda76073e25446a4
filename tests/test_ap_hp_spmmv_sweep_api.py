"""The C ABI around the sweep path of adaptive-precision SpMMV with an fp16 part (uspmv_spmmv_ap_hp_sweep_vectors): declared in
include/uspmv.h, exported by libuspmv.so, bound by the package, refusing bad arguments with USPMV_ERR_INVALID and a uspmv_last_error
text under its own name before any device is needed; and the pure function's whole table against the rule restated here."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

LDS = 160 * 1024                    # what a gfx950 workgroup can have
WIDTHS = (1, 2, 3, 4, 8, 16, 32)
NAME = b"uspmv_spmmv_ap_hp_sweep_vectors"
ERR_INVALID = 1                     # USPMV_ERR_INVALID


def _rule(b, wlog, x_bytes):
    """the largest of {8, 4, 2} that is at most b, divides b and fits one window of 2^wlog X elements per vector; only for the widths
    with a specialised kernel"""
    if b not in (2, 4, 8, 16):
        return 0
    for bs in (8, 4, 2):
        if bs <= b and b % bs == 0 and (x_bytes << wlog) * bs <= LDS:
            return bs
    return 0


def test_declared_in_the_header_exported_and_bound(pkg):
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+uspmv_spmmv_ap_hp_sweep_vectors\s*\(\s*int b,\s*int wlog,\s*int x_dtype,\s*int \*vectors\s*\)\s*;", h)
    assert pkg.lib().uspmv_spmmv_ap_hp_sweep_vectors is not None
    assert callable(pkg.spmmv_ap_hp_sweep_vectors)


def test_the_whole_table(pkg):
    L = pkg.lib()
    n = C.c_int(-1)
    for dtype, x_bytes in ((pkg.F64, 8), (pkg.F32, 4)):
        for b in WIDTHS:
            for wlog in range(8, 17):
                assert L.uspmv_spmmv_ap_hp_sweep_vectors(b, wlog, dtype, C.byref(n)) == 0
                assert n.value == _rule(b, wlog, x_bytes), (dtype, b, wlog, n.value)
                assert pkg.spmmv_ap_hp_sweep_vectors(b, wlog, dtype) == n.value
    # the rows of the table as the header states them: vectors per pass at b = 16 for windows of 2^11 .. 2^15 elements
    assert [pkg.spmmv_ap_hp_sweep_vectors(16, w, pkg.F64) for w in (11, 12, 13, 14, 15)] == [8, 4, 2, 0, 0]
    assert [pkg.spmmv_ap_hp_sweep_vectors(16, w, pkg.F32) for w in (11, 12, 13, 14, 15)] == [8, 8, 4, 2, 0]
    # the planner's default windows under "sweep_nbuf" 1 -- 2^14 doubles, 2^15 floats -- hold one vector: no block kernel at any width
    for b in WIDTHS:
        assert pkg.spmmv_ap_hp_sweep_vectors(b, 14, pkg.F64) == 0 and pkg.spmmv_ap_hp_sweep_vectors(b, 15, pkg.F32) == 0


def test_refusals(pkg):
    L = pkg.lib()
    n = C.c_int(-1)
    bad = [(0, 12, pkg.F64), (-3, 12, pkg.F32), (4, 7, pkg.F64), (4, 17, pkg.F64), (4, -1, pkg.F32), (4, 12, pkg.F16), (4, 12, 99), (4, 12, -1)]
    for b, wlog, dtype in bad:
        assert L.uspmv_spmmv_ap_hp_sweep_vectors(b, wlog, dtype, C.byref(n)) == ERR_INVALID, (b, wlog, dtype)
        assert L.uspmv_last_error().startswith(NAME), (b, wlog, dtype)
        assert n.value == -1                                   # nothing reported on a refusal
    assert L.uspmv_spmmv_ap_hp_sweep_vectors(4, 12, pkg.F64, None) == ERR_INVALID
    assert L.uspmv_last_error().startswith(NAME)
    for args in ((0, 12, pkg.F64), (4, 7, pkg.F32), (4, 12, pkg.F16)):
        with pytest.raises(pkg.UspmvError):
            pkg.spmmv_ap_hp_sweep_vectors(*args)
