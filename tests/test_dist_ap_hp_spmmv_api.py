"""The C ABI of the block-vector step of the adaptive-precision kinds with an fp16 part across ranks (uspmv_spmmv_ap_hp_tiles,
uspmv_spmmv_ap_hp_chunks, uspmv_spmmv_ap_hp_tiles_path, uspmv_dist_spmmv_ap_hp): declared in include/uspmv.h, exported by libuspmv.so with
the ctypes signatures the binding declares, reachable through the package, and refusing bad arguments with a status code and a
uspmv_last_error text that begins with the function's name, before any device is needed."""
import ctypes as C
import os
import re

from conftest import ROOT

HANDLES = r"\s*const uspmv_dmat_t \*hi,\s*const uspmv_dmat_t \*mid,\s*const uspmv_dmat_t \*hp,"
BLOCK = r"\s*const void \*d_X,\s*void \*d_Y,\s*int b,\s*int64_t ld,\s*int layout,\s*void \*stream\s*\)\s*;"
NEW_SYMBOLS = ("uspmv_spmmv_ap_hp_tiles", "uspmv_spmmv_ap_hp_chunks", "uspmv_spmmv_ap_hp_tiles_path", "uspmv_dist_spmmv_ap_hp")


def _header():
    with open(os.path.join(ROOT, "include", "uspmv.h")) as f:
        return f.read()


def test_declared_in_the_header(pkg):
    h = _header()
    assert re.search(r"\bint\s+uspmv_spmmv_ap_hp_tiles\s*\(" + HANDLES + r"\s*const int32_t \*d_tile_ids,\s*int64_t n_ids," + BLOCK, h)
    assert re.search(r"\bint\s+uspmv_spmmv_ap_hp_chunks\s*\(" + HANDLES + r"\s*const int32_t \*d_chunk_ids,\s*int64_t n_ids," + BLOCK, h)
    assert re.search(r"\bint\s+uspmv_spmmv_ap_hp_tiles_path\s*\(" + HANDLES + r"\s*int b,\s*int64_t ld,\s*int layout,\s*int \*path,"
                     r"\s*int \*vectors_per_pass\s*\)\s*;", h)
    assert re.search(r"\bint\s+uspmv_dist_spmmv_ap_hp\s*\(\s*uspmv_dist_t \*d,\s*void \*d_X,\s*void \*d_Y,\s*int b,\s*int layout,\s*int mode,"
                     r"\s*int comm_halos,\s*void \*stream\s*\)\s*;", h)


def test_exported_with_the_declared_ctypes_signatures(pkg):
    from ultimate_spmv_amd import binding as B
    L = pkg.lib()
    vp, i64, ci, pi = C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int)
    want = {"uspmv_spmmv_ap_hp_tiles": [vp, vp, vp, vp, i64, vp, vp, ci, i64, ci, vp],
            "uspmv_spmmv_ap_hp_chunks": [vp, vp, vp, vp, i64, vp, vp, ci, i64, ci, vp],
            "uspmv_spmmv_ap_hp_tiles_path": [vp, vp, vp, ci, i64, ci, pi, pi],
            "uspmv_dist_spmmv_ap_hp": [vp, vp, vp, ci, ci, ci, ci, vp]}
    assert set(want) == set(NEW_SYMBOLS)
    for name, args in want.items():
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == args, name
        assert B._SIGS[name] == (C.c_int, args), name
    # the twins they mirror keep the same argument lists behind the handles
    assert list(L.uspmv_spmmv_ap_tiles.argtypes)[2:] == want["uspmv_spmmv_ap_hp_tiles"][3:]
    assert list(L.uspmv_dist_spmmv_ap.argtypes) == want["uspmv_dist_spmmv_ap_hp"]


def test_the_package_exports_the_python_names(pkg):
    assert callable(pkg.spmmv_ap_hp_tiles) and callable(pkg.spmmv_ap_hp_chunks) and callable(pkg.spmmv_ap_hp_tiles_path)
    assert callable(pkg.DistNative.spmmv_ap_hp) and callable(pkg.DistNative.spmmv_ap_hp_tiles_path) and callable(pkg.DistNative.new_X)


def test_null_arguments_are_refused_without_a_device(pkg):
    L = pkg.lib()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    path, vec = C.c_int(-1), C.c_int(-1)
    for lay in (pkg.COLWISE, pkg.ROWWISE):
        assert L.uspmv_spmmv_ap_hp_tiles(None, None, None, None, 0, p, p, 4, 0, lay, None) != 0
        assert L.uspmv_last_error().startswith(b"uspmv_spmmv_ap_hp_tiles:")
        assert L.uspmv_spmmv_ap_hp_chunks(None, None, None, None, 0, p, p, 4, 0, lay, None) != 0
        assert L.uspmv_last_error().startswith(b"uspmv_spmmv_ap_hp_chunks:")
        assert L.uspmv_spmmv_ap_hp_tiles_path(None, None, None, 4, 0, lay, C.byref(path), C.byref(vec)) != 0
        assert L.uspmv_last_error().startswith(b"uspmv_spmmv_ap_hp_tiles_path:")
    assert (path.value, vec.value) == (-1, -1)
    assert L.uspmv_dist_spmmv_ap_hp(None, p, p, 4, pkg.COLWISE, 0, 1, None) == 1          # USPMV_ERR_INVALID
    assert L.uspmv_last_error().startswith(b"uspmv_dist_spmmv_ap_hp: NULL argument")
    for b, lay, mode, text in ((0, pkg.COLWISE, 0, b"b=0"), (4, 2, 0, b"unknown layout 2"), (4, pkg.COLWISE, 3, b"unknown mode 3")):
        assert L.uspmv_dist_spmmv_ap_hp(None, p, p, b, lay, mode, 1, None) == 1
        assert L.uspmv_last_error() == b"uspmv_dist_spmmv_ap_hp: " + text
