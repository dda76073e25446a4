"""y = alpha A x + beta z with two dot products (uspmv_spmv_axpby), the part that needs no device: the three entry points are declared in
include/uspmv.h, exported by libuspmv.so and bound by the package, and every refusal comes back with its status and a message that
names the function before a device is looked for.  (The refusal of a part of an adaptive-precision split needs a plan, hence a device:
tests/test_gpu_spmv_axpby.py.)"""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

INVALID, UNSUPPORTED, NO_DEVICE = 1, 3, 5
NEW = ("uspmv_spmv_axpby", "uspmv_spmv_axpby_path", "uspmv_spmv_axpby_reserve")


def test_symbols_declared_exported_bound(pkg):
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        raw = f.read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(uspmv_[a-z0-9_]+)\s*\(", hdr))
    from ultimate_spmv_amd import binding
    L = C.CDLL(pkg.library_path())
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in binding._SIGS, name
    # the struct as the header lays it out: two doubles, three pointers, one int64
    m = re.search(r"typedef struct \{(.*?)\} uspmv_axpby_t;", hdr, flags=re.S)
    assert m, "uspmv_axpby_t is not declared"
    fields = [re.split(r"[\s*]+", d.strip())[-1] for part in m.group(1).split(";") for d in part.split(",") if d.strip()]
    assert fields == ["alpha", "beta", "d_z", "d_w", "d_dots", "n_dot_rows"], fields
    assert [f[0] for f in pkg.AxpbyOp._fields_] == fields and C.sizeof(pkg.AxpbyOp) == 48
    assert callable(pkg.spmv_axpby) and callable(pkg.spmv_axpby_path) and callable(pkg.DeviceMatrix.axpby_reserve)
    with open(os.path.join(ROOT, "include", "uspmv_interface.hpp")) as f:
        text = f.read()
    assert "spmv_axpby(" in text and "spmv_axpby_path(" in text and "axpby_reserve(" in text
    # uspmv_spmv itself is untouched
    assert "int uspmv_spmv(const uspmv_dmat_t *A, const void *d_x, void *d_y, void *stream);" in raw


def _wrapped(L, dtype, n_chunks=3, C_=2):
    """a handle around HOST memory (n_chunks chunks of C_ rows, two slots each): every call below is refused before the arrays are read"""
    ne = n_chunks * C_ * 2
    cp = (np.arange(n_chunks + 1) * C_ * 2).astype(np.int32); cl = np.full(n_chunks, 2, np.int32); ci = np.zeros(ne, np.int32)
    va = np.ones(ne, {0: np.float64, 1: np.float32, 2: np.uint16}[dtype])
    h = C.c_void_p()
    assert L.uspmv_dmat_wrap(C_, n_chunks, ne, dtype, cp.ctypes.data, cl.ctypes.data, ci.ctypes.data, va.ctypes.data, C.byref(h)) == 0
    return h, (cp, cl, ci, va)


def test_refusals_come_before_the_device_check(pkg):
    L = pkg.lib()
    err = lambda: L.uspmv_last_error().decode()
    Op = pkg.AxpbyOp
    n = 6                                                    # rows y may be written: 3 chunks of 2
    for dtype, np_t in ((pkg.F64, np.float64), (pkg.F32, np.float32)):
        es = np.dtype(np_t).itemsize
        x = np.ones(n, np_t); y = np.full(2 * n, 9.0, np_t); z = np.ones(n, np_t); dots = np.full(2, 7.0)
        p = lambda a, off=0: a.ctypes.data + off * es
        call = lambda h, x_, y_, op: L.uspmv_spmv_axpby(h, x_, y_, None if op is None else C.byref(op), None)
        good = lambda **kw: Op(**{**dict(alpha=1.0, beta=0.0, d_z=None, d_w=None, d_dots=None, n_dot_rows=n), **kw})
        assert call(None, p(x), p(y), good()) == INVALID and "uspmv_spmv_axpby: NULL matrix" in err()
        h, keep = _wrapped(L, dtype)
        try:
            who = "uspmv_spmv_axpby: "
            assert call(h, p(x), p(y), None) == INVALID and who in err() and "NULL op" in err()
            assert call(h, None, p(y), good()) == INVALID and who in err() and "NULL vector" in err()
            assert call(h, p(x), None, good()) == INVALID and who in err() and "NULL vector" in err()
            # beta != 0 needs z (a NaN beta is non-zero and simply propagates -- it is the NULL that is refused)
            for beta in (1.0, -2.5, float("nan"), float("inf")):
                assert call(h, p(x), p(y), good(beta=beta)) == INVALID and who in err() and "d_z" in err(), beta
            # z overlapping y partially, from either side, by one element and by all but one; exactly equal is allowed
            for off in (1, n - 1):
                assert call(h, p(x), p(y, off), good(beta=1.0, d_z=p(y))) == INVALID and who in err() and "overlaps" in err(), off
                assert call(h, p(x), p(y), good(beta=1.0, d_z=p(y, off))) == INVALID and who in err() and "overlaps" in err(), off
            # n_dot_rows outside [0, rows y may be written]
            for bad in (-1, n + 1, 1 << 40):
                assert call(h, p(x), p(y), good(n_dot_rows=bad, d_dots=p(dots))) == INVALID and who in err() and "n_dot_rows" in err(), bad
            # what passes every check reaches the device check: in place, z behind y, NULL z with beta == 0, non-finite alpha, both ends of n_dot_rows
            if pkg.device_count() == 0:
                for op, yy in ((good(beta=1.0, d_z=p(y)), p(y)), (good(beta=1.0, d_z=p(y, n)), p(y)), (good(alpha=float("nan")), p(y)),
                               (good(beta=0.0, d_z=None, n_dot_rows=0, d_dots=p(dots)), p(y)), (good(beta=0.0, d_z=p(y, 1)), p(y)),
                               (good(n_dot_rows=n, d_dots=p(dots), d_w=p(z)), p(y))):
                    assert call(h, p(x), yy, op) == NO_DEVICE, err()
                assert L.uspmv_spmv_axpby_reserve(h) == NO_DEVICE
            # nothing was written by any of it
            assert (y == 9.0).all() and (dots == 7.0).all() and (keep[3] == 1).all()
            # the path query: same handle checks, needs no device at all
            path = C.c_int(-1)
            assert L.uspmv_spmv_axpby_path(None, p(x), C.byref(path)) == INVALID and "uspmv_spmv_axpby_path: NULL matrix" in err()
            assert L.uspmv_spmv_axpby_path(h, None, C.byref(path)) == INVALID and "uspmv_spmv_axpby_path: " in err() and "NULL" in err()
            assert L.uspmv_spmv_axpby_path(h, p(x), None) == INVALID and "uspmv_spmv_axpby_path: " in err() and "NULL" in err()
            assert L.uspmv_spmv_axpby_path(h, p(x), C.byref(path)) == 0 and path.value == 1          # default tuning, no plan: the fused rows kernel
            pkg.set_tuning(unroll=4)
            try:
                assert L.uspmv_spmv_axpby_path(h, p(x), C.byref(path)) == 0 and path.value == 2      # no fused instantiation for that unroll
            finally:
                pkg.set_tuning(unroll=8)
            assert L.uspmv_spmv_axpby_reserve(None) == INVALID and "uspmv_spmv_axpby_reserve: NULL matrix" in err()
        finally:
            L.uspmv_dmat_free(h)
    # an fp16 handle: all three, in uspmv_spmv's words
    h, keep = _wrapped(L, pkg.F16)
    try:
        x = np.ones(n); y = np.ones(n); path = C.c_int(-1)
        op = Op(1.0, 0.0, None, None, None, n)
        for name, rc in (("uspmv_spmv_axpby", L.uspmv_spmv_axpby(h, x.ctypes.data, y.ctypes.data, C.byref(op), None)),
                         ("uspmv_spmv_axpby_path", L.uspmv_spmv_axpby_path(h, x.ctypes.data, C.byref(path))),
                         ("uspmv_spmv_axpby_reserve", L.uspmv_spmv_axpby_reserve(h))):
            assert rc == UNSUPPORTED, name
        assert "uspmv_spmv_axpby_reserve: fp16 handle" in err() and "uspmv_spmv_ap_hp" in err()
    finally:
        L.uspmv_dmat_free(h)
