"""The public surface around the shared element plan of the adaptive-precision kinds, as far as it can be checked without a device: the
planners and the plan queries are declared in include/uspmv.h, exported by libuspmv.so and bound by the package; the header names the
fallback order lines -> elements -> sweep for all four planners; uspmv_dmat_plan_granularity answers 0 on a handle without a plan (a
part of a split that was never planned); and the planners refuse bad handles before any device is needed."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

ERR_INVALID = 1                     # USPMV_ERR_INVALID
PLANNERS = ("uspmv_dmat_optimize_ap", "uspmv_dmat_optimize_ap_hp", "uspmv_dmat_optimize_device_ap", "uspmv_dmat_optimize_device_ap_hp")


def _header():
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        return f.read()


def test_declared_exported_and_bound(pkg):
    h = _header()
    L = pkg.lib()
    for name in PLANNERS + ("uspmv_dmat_plan_granularity", "uspmv_dmat_plan_download", "uspmv_spmv_ap_tiles", "uspmv_spmv_ap_hp_tiles",
                            "uspmv_spmmv_ap_path", "uspmv_spmmv_ap_hp_path", "uspmv_spmmv_ap_tiles_path", "uspmv_spmmv_ap_hp_tiles_path"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
        assert getattr(L, name) is not None
    for wrapper in ("optimize_ap", "optimize_ap_hp", "optimize_device_ap", "optimize_device_ap_hp", "spmv_ap_tiles", "spmv_ap_hp_tiles",
                    "spmmv_ap_path", "spmmv_ap_hp_path", "spmmv_ap_tiles_path", "spmmv_ap_hp_tiles_path"):
        assert callable(getattr(pkg, wrapper)), wrapper
    assert callable(pkg.DeviceMatrix.plan_granularity) and callable(pkg.DeviceMatrix.plan_download)


def test_the_header_names_the_fallback_order(pkg):
    """the comment in front of each of the four planners says lines -> elements -> sweep"""
    h = _header()
    for name in PLANNERS:
        at = re.search(r"\bint\s+" + name + r"\s*\(", h).start()
        comment = h[h.rfind("/*", 0, at):at]
        assert re.search(r"lines\s*->\s*elements\s*->\s*sweep", comment), name


def test_tuning_keys_of_the_policy(pkg):
    assert pkg.get_tuning("tlc_elem") == 1 and pkg.get_tuning("tlc_elem_cap") == 4096
    pkg.set_tuning(tlc_elem=2)
    try:
        assert pkg.get_tuning("tlc_elem") == 2
    finally:
        pkg.set_tuning(tlc_elem=1)


def test_granularity_of_a_part_without_a_plan_is_zero(pkg):
    """uspmv_dmat_wrap needs no device (the arrays are never read here): a handle fresh from it carries no plan"""
    L = pkg.lib()
    cp = np.zeros(3, np.int32); cl = np.zeros(2, np.int32); ci = np.zeros(1, np.int32)
    for dtype, va in ((pkg.F64, np.zeros(1, np.float64)), (pkg.F32, np.zeros(1, np.float32)), (pkg.F16, np.zeros(1, np.float16))):
        h = C.c_void_p()
        assert L.uspmv_dmat_wrap(32, 2, 0, dtype, cp.ctypes.data_as(C.c_void_p), cl.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                 va.ctypes.data_as(C.c_void_p), C.byref(h)) == 0
        try:
            g = C.c_int(-1)
            assert L.uspmv_dmat_plan_granularity(h, C.byref(g)) == 0 and g.value == 0
            k, a, b = C.c_int(-1), C.c_int64(-1), C.c_int64(-1)
            assert L.uspmv_dmat_plan_info(h, C.byref(k), C.byref(a), C.byref(b)) == 0 and (k.value, a.value, b.value) == (0, 0, 0)
            assert L.uspmv_dmat_plan_granularity(h, None) == ERR_INVALID
        finally:
            L.uspmv_dmat_free(h)
    g = C.c_int(-1)
    assert L.uspmv_dmat_plan_granularity(None, C.byref(g)) == ERR_INVALID and g.value == -1


def test_planners_refuse_null_handles_before_any_device(pkg):
    L = pkg.lib()
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert L.uspmv_dmat_optimize_device_ap(None, None, 0, C.byref(a), C.byref(b)) == ERR_INVALID
    assert L.uspmv_dmat_optimize_device_ap_hp(None, None, None, 0, C.byref(a), C.byref(b)) == ERR_INVALID
    assert L.uspmv_dmat_optimize_ap(None, None, None, None, 0, C.byref(a), C.byref(b)) == ERR_INVALID
    assert L.uspmv_dmat_optimize_ap_hp(None, None, None, None, None, None, 0, C.byref(a), C.byref(b)) == ERR_INVALID
    assert (a.value, b.value) == (-1, -1)
