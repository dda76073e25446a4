"""y = alpha A x + beta z with two dot products on the parts of an adaptive-precision split (uspmv_spmv_ap_axpby, uspmv_spmv_ap_hp_axpby),
the part that needs no device: the six entry points are declared in include/uspmv.h, exported by libuspmv.so and bound by the package
with the documented signatures, the header states the contract, and every refusal comes back with its status and a message that names
the function before a device is looked for.  In the manner of tests/test_spmv_axpby_api.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from conftest import ROOT
from test_spmv_axpby_api import _wrapped

INVALID, NO_DEVICE = 1, 5
NEW = ("uspmv_spmv_ap_axpby", "uspmv_spmv_ap_axpby_path", "uspmv_spmv_ap_axpby_reserve",
       "uspmv_spmv_ap_hp_axpby", "uspmv_spmv_ap_hp_axpby_path", "uspmv_spmv_ap_hp_axpby_reserve")
TAIL = ["x", "y", "alpha", "beta", "z", "w", "dots", "n_dot_rows", "stream"]


def test_symbols_declared_exported_bound(pkg):
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        raw = f.read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(uspmv_[a-z0-9_]+)\s*\(", hdr))
    from ultimate_spmv_amd import binding
    L = C.CDLL(pkg.library_path())
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in binding._SIGS, name
    flat = re.sub(r"\s+", " ", hdr)
    for decl in ("int uspmv_spmv_ap_axpby(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, double *d_y, const uspmv_axpby_t *op, void *stream);",
                 "int uspmv_spmv_ap_axpby_path(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const void *d_x, int *path);",
                 "int uspmv_spmv_ap_axpby_reserve(uspmv_dmat_t *dp, const uspmv_dmat_t *sp);",
                 "int uspmv_spmv_ap_hp_axpby(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, void *d_y, "
                 "const uspmv_axpby_t *op, void *stream);",
                 "int uspmv_spmv_ap_hp_axpby_path(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, int *path);",
                 "int uspmv_spmv_ap_hp_axpby_reserve(uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp);"):
        assert decl in flat, decl
    # the plain entry points are untouched
    assert "int uspmv_spmv_ap(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, double *d_y, void *stream);" in raw
    assert "int uspmv_spmv_ap_hp(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, void *d_y, void *stream);" in raw


def test_binding_signatures(pkg):
    def names(f):
        return list(inspect.signature(f).parameters)
    sig = inspect.signature(pkg.spmv_ap_axpby)
    assert names(pkg.spmv_ap_axpby) == ["A_dp", "A_sp"] + TAIL
    assert names(pkg.spmv_ap_hp_axpby) == ["A_hi", "A_mid", "A_hp"] + TAIL
    for f in (pkg.spmv_ap_axpby, pkg.spmv_ap_hp_axpby):
        p = inspect.signature(f).parameters
        assert (p["alpha"].default, p["beta"].default) == (1.0, 0.0)
        assert all(p[k].default is None for k in ("z", "w", "dots", "n_dot_rows", "stream"))
    assert sig.parameters["x"].default is inspect.Parameter.empty
    assert names(pkg.spmv_ap_axpby_path) == ["A_dp", "A_sp", "x"] and names(pkg.spmv_ap_hp_axpby_path) == ["A_hi", "A_mid", "A_hp", "x"]
    assert names(pkg.ap_axpby_reserve) == ["A_dp", "A_sp"] and names(pkg.ap_hp_axpby_reserve) == ["A_hi", "A_mid", "A_hp"]
    with open(os.path.join(ROOT, "include", "uspmv_interface.hpp")) as f:
        text = f.read()
    ap = text[text.index("class DeviceApScs"):]
    ap = ap[:ap.index("\n};")]
    for member in ("void spmv_axpby(", "int spmv_axpby_path(", "void axpby_reserve("):
        assert member in ap, member
    for name in NEW:
        assert name + "(" in ap, name


def test_the_header_states_the_contract():
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        raw = f.read()
    i = raw.index("int uspmv_spmv_ap_axpby(")
    comment = re.sub(r"\s*\n \* ", " ", raw[raw.rindex("/*", 0, i):i])
    for phrase in ("DESIGN.md 5.13", "dp + sp", "hi + hp", "(hi + mid) + hp", "(float)(sp + hp)", "converted ONCE", "never an FMA",
                   "bit for bit", "d_z may be d_y", "no floating-point atomics", "no host synchronisation", "logical id",
                   "slots behind the first's", "bitwise reproducible", "FIRST handle", "capturing", "_reserve", "USPMV_ERR_INVALID",
                   "n_dot_rows", "uspmv_spmv_ap_generic", "\"nontemporal\" 0", "\"unroll\" < 8", "\"sweep_unroll\" < 8", "\"sweep_pair\" != 2",
                   "16-byte grid"):
        assert phrase in comment, phrase


def test_refusals_come_before_the_device_check(pkg):
    """handles around host memory: every call below is refused (or answered) before the arrays are read"""
    L = pkg.lib()
    err = lambda: L.uspmv_last_error().decode()
    Op = pkg.AxpbyOp
    n = 6                                                    # rows y may be written: 3 chunks of 2
    dp, k1 = _wrapped(L, pkg.F64); sp, k2 = _wrapped(L, pkg.F32); hp, k3 = _wrapped(L, pkg.F16)
    sp4, k4 = _wrapped(L, pkg.F32, n_chunks=4); hp4, k5 = _wrapped(L, pkg.F16, n_chunks=4); spc, k6 = _wrapped(L, pkg.F32, C_=4)
    keep = (k1, k2, k3, k4, k5, k6)
    try:
        families = {
            # name: (call(handles..., x, y, op), good handles, np type, refused handle sets with the text of the plain call)
            "uspmv_spmv_ap_axpby": (
                lambda hs, x_, y_, op: L.uspmv_spmv_ap_axpby(hs[0], hs[1], x_, y_, None if op is None else C.byref(op), None),
                lambda hs, x_, path: L.uspmv_spmv_ap_axpby_path(hs[0], hs[1], x_, path),
                lambda hs: L.uspmv_spmv_ap_axpby_reserve(hs[0], hs[1]),
                (dp, sp), np.float64,
                [((None, sp), "NULL matrix"), ((dp, None), "NULL matrix"), ((dp, dp), "expects a double and a float struct"),
                 ((sp, dp), "expects a double and a float struct"), ((dp, hp), "expects a double and a float struct"),
                 ((dp, sp4), "must share C and n_chunks"), ((dp, spc), "must share C and n_chunks")]),
            "uspmv_spmv_ap_hp_axpby": (
                lambda hs, x_, y_, op: L.uspmv_spmv_ap_hp_axpby(hs[0], hs[1], hs[2], x_, y_, None if op is None else C.byref(op), None),
                lambda hs, x_, path: L.uspmv_spmv_ap_hp_axpby_path(hs[0], hs[1], hs[2], x_, path),
                lambda hs: L.uspmv_spmv_ap_hp_axpby_reserve(hs[0], hs[1], hs[2]),
                (dp, sp, hp), np.float64,
                [((None, None, hp), "NULL matrix"), ((dp, None, None), "NULL matrix"), ((dp, None, sp), "the parts must be"),
                 ((dp, dp, hp), "the parts must be"), ((sp, sp, hp), "the parts must be"), ((hp, None, hp), "the parts must be"),
                 ((dp, None, hp4), "must share C and n_chunks"), ((dp, sp4, hp), "must share C and n_chunks")]),
        }
        for who, (call, path_of, reserve, hs, np_t, bad_handles) in families.items():
            es = np.dtype(np_t).itemsize
            x = np.ones(n, np_t); y = np.full(2 * n, 9.0, np_t); z = np.ones(n, np_t); dots = np.full(2, 7.0)
            p = lambda a, off=0: a.ctypes.data + off * es
            good = lambda **kw: Op(**{**dict(alpha=1.0, beta=0.0, d_z=None, d_w=None, d_dots=None, n_dot_rows=n), **kw})
            path = C.c_int(-1)
            for bad, text in bad_handles:
                assert call(bad, p(x), p(y), good()) == INVALID and who + ": " in err() and text in err(), (who, text, err())
                assert path_of(bad, p(x), C.byref(path)) == INVALID and who + "_path: " in err() and text in err(), (who, text, err())
                assert reserve(bad) == INVALID and who + "_reserve: " in err() and text in err(), (who, text, err())
            assert call(hs, p(x), p(y), None) == INVALID and who + ": " in err() and "NULL op" in err()
            assert call(hs, None, p(y), good()) == INVALID and who + ": " in err() and "NULL vector" in err()
            assert call(hs, p(x), None, good()) == INVALID and who + ": " in err() and "NULL vector" in err()
            for beta in (1.0, -2.5, float("nan")):
                assert call(hs, p(x), p(y), good(beta=beta)) == INVALID and who + ": " in err() and "d_z" in err(), beta
            for off in (1, n - 1):
                assert call(hs, p(x), p(y, off), good(beta=1.0, d_z=p(y))) == INVALID and who + ": " in err() and "overlaps" in err(), off
                assert call(hs, p(x), p(y), good(beta=1.0, d_z=p(y, off))) == INVALID and who + ": " in err() and "overlaps" in err(), off
            for badn in (-1, n + 1, 1 << 40):
                assert call(hs, p(x), p(y), good(n_dot_rows=badn, d_dots=p(dots))) == INVALID and who + ": " in err() and "n_dot_rows" in err(), badn
            if pkg.device_count() == 0:
                for op in (good(beta=1.0, d_z=p(y)), good(beta=1.0, d_z=p(y, n)), good(beta=0.0, d_z=None, n_dot_rows=0, d_dots=p(dots)),
                           good(n_dot_rows=n, d_dots=p(dots), d_w=p(z))):
                    assert call(hs, p(x), p(y), op) == NO_DEVICE, err()
                assert reserve(hs) == NO_DEVICE
            assert (y == 9.0).all() and (dots == 7.0).all()
            # the path query needs no device: no plan, default tuning -> the fused lane-per-row kernel
            assert path_of(hs, None, C.byref(path)) == INVALID and who + "_path: " in err() and "NULL" in err()
            assert path_of(hs, p(x), None) == INVALID and who + "_path: " in err() and "NULL" in err()
            assert path_of(hs, p(x), C.byref(path)) == 0 and path.value == 1
            pkg.set_tuning(unroll=4)
            try:   # the pair's lane-per-row kernel fuses at unroll 8 only; the kinds with an fp16 part do not consult "unroll"
                assert path_of(hs, p(x), C.byref(path)) == 0 and path.value == (2 if who == "uspmv_spmv_ap_axpby" else 1)
            finally:
                pkg.set_tuning(unroll=8)
            pkg.set_tuning(nontemporal=0)
            try:
                assert path_of(hs, p(x), C.byref(path)) == 0 and path.value == 2
            finally:
                pkg.set_tuning(nontemporal=1)
        # ap[sp_hp]: float vectors, same checks on the element size of the overlap test
        x = np.ones(n, np.float32); y = np.full(2 * n, 9.0, np.float32)
        op = Op(1.0, 1.0, y.ctypes.data + 4, None, None, n)
        assert L.uspmv_spmv_ap_hp_axpby(sp, None, hp, x.ctypes.data, y.ctypes.data, C.byref(op), None) == INVALID and "overlaps" in err()
        assert (y == 9.0).all() and all((k[3] == 1).all() for k in keep[:2])
    finally:
        for h in (dp, sp, hp, sp4, hp4, spc):
            L.uspmv_dmat_free(h)
