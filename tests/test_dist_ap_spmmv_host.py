"""Host side of the distributed ap[dp_sp] block step: the four new symbols of the C ABI (uspmv_spmmv_ap_tiles / _chunks / _tiles_path,
uspmv_dist_spmmv_ap) are declared, exported and bound, and refuse NULL handles and bad scalar arguments before any HIP call.  No GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = ("uspmv_spmmv_ap_tiles", "uspmv_spmmv_ap_chunks", "uspmv_spmmv_ap_tiles_path", "uspmv_dist_spmmv_ap")
INVALID = 1                                    # USPMV_ERR_INVALID
COLWISE, ROWWISE = 0, 1


@pytest.fixture(scope="module")
def L(pkg):
    lib = C.CDLL(pkg.library_path())
    lib.uspmv_last_error.restype = C.c_char_p
    i64, vp = C.c_int64, C.c_void_p
    lib.uspmv_spmmv_ap_tiles.argtypes = lib.uspmv_spmmv_ap_chunks.argtypes = [vp, vp, vp, i64, vp, vp, C.c_int, i64, C.c_int, vp]
    lib.uspmv_spmmv_ap_tiles_path.argtypes = [vp, vp, C.c_int, i64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.uspmv_dist_spmmv_ap.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    return lib


def test_new_symbols_are_declared_exported_and_bound(pkg, L):
    hdr = open(os.path.join(ROOT, "include", "uspmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(uspmv_[a-z0-9_]+)\s*\(", hdr))
    from ultimate_spmv_amd import binding
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name) and name in binding._SIGS, name
    for name in ("spmmv_ap_tiles", "spmmv_ap_chunks", "spmmv_ap_tiles_path"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.DistNative.spmmv_ap)
    # the signatures of the issue, argument for argument
    flat = re.sub(r"\s+", " ", hdr)
    for fn in ("uspmv_spmmv_ap_tiles", "uspmv_spmmv_ap_chunks"):
        ids = "d_tile_ids" if fn.endswith("tiles") else "d_chunk_ids"
        assert re.search(rf"int {fn} ?\( ?const uspmv_dmat_t \*dp, const uspmv_dmat_t \*sp, const int32_t \*{ids}, int64_t n_ids, const void \*d_X, "
                         r"void \*d_Y, int b, int64_t ld, int layout, void \*stream ?\)", flat), fn
    assert re.search(r"int uspmv_spmmv_ap_tiles_path ?\( ?const uspmv_dmat_t \*dp, const uspmv_dmat_t \*sp, int b, int64_t ld, int layout, int \*path, "
                     r"int \*vectors_per_pass ?\)", flat)
    assert re.search(r"int uspmv_dist_spmmv_ap ?\( ?uspmv_dist_t \*d, void \*d_X, void \*d_Y, int b, int layout, int mode, int comm_halos, void \*stream ?\)", flat)


def _refused(L, rc, name, text=None):
    assert rc == INVALID, (name, rc)
    msg = L.uspmv_last_error()
    assert name.encode() in msg and (text is None or text.encode() in msg), msg


def test_list_forms_refuse_null_handles_and_bad_scalars_without_a_device(pkg, L):
    buf = (C.c_double * 8)()
    ids = (C.c_int32 * 4)()
    p, q = C.cast(buf, C.c_void_p), C.cast(ids, C.c_void_p)
    path, vec = C.c_int(7), C.c_int(7)
    for lay in (COLWISE, ROWWISE):
        for fn in ("uspmv_spmmv_ap_tiles", "uspmv_spmmv_ap_chunks"):
            _refused(L, getattr(L, fn)(None, None, q, 4, p, p, 4, 0, lay, None), fn)
            _refused(L, getattr(L, fn)(None, None, None, 0, p, p, 4, 0, lay, None), fn)       # (an empty list still checks its handles)
            for b in (0, -3):
                _refused(L, getattr(L, fn)(None, None, q, 4, p, p, b, 0, lay, None), fn, f"b={b}")
        _refused(L, L.uspmv_spmmv_ap_tiles_path(None, None, 4, 0, lay, C.byref(path), C.byref(vec)), "uspmv_spmmv_ap_tiles_path")
        _refused(L, L.uspmv_spmmv_ap_tiles_path(None, None, 0, 0, lay, C.byref(path), C.byref(vec)), "uspmv_spmmv_ap_tiles_path", "b=0")
    for fn in ("uspmv_spmmv_ap_tiles", "uspmv_spmmv_ap_chunks"):
        _refused(L, getattr(L, fn)(None, None, q, 4, p, p, 4, 0, 2, None), fn, "unknown layout 2")
    _refused(L, L.uspmv_spmmv_ap_tiles_path(None, None, 4, 0, -1, C.byref(path), C.byref(vec)), "uspmv_spmmv_ap_tiles_path", "unknown layout -1")
    assert (path.value, vec.value) == (7, 7)                                                  # (a refused query writes nothing)


def test_dist_spmmv_ap_refuses_null_and_bad_scalars_without_a_device(pkg, L):
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    fn = "uspmv_dist_spmmv_ap"
    _refused(L, L.uspmv_dist_spmmv_ap(None, p, p, 4, COLWISE, 0, 1, None), fn, "NULL argument")
    for b in (0, -1):
        _refused(L, L.uspmv_dist_spmmv_ap(None, p, p, b, COLWISE, 0, 1, None), fn, f"b={b}")
    _refused(L, L.uspmv_dist_spmmv_ap(None, p, p, 4, 2, 0, 1, None), fn, "unknown layout 2")
    for mode in (3, -1):
        _refused(L, L.uspmv_dist_spmmv_ap(None, p, p, 4, ROWWISE, mode, 1, None), fn, f"unknown mode {mode}")
