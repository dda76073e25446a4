"""uspmv_gen_stencil27_device and uspmv_dist_check_arrays, the part that needs no device: the symbols are declared,
exported and bound, and the refusals come with the host generator's codes before the first HIP call."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

INVALID, UNSUPPORTED, OVERFLOW = 1, 3, 4
NEW = ("uspmv_gen_stencil27_device", "uspmv_dist_check_arrays")


def test_new_symbols_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "uspmv.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    from ultimate_spmv_amd import binding
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert re.search(r"\sT\s+%s$" % name, exported, re.M), name
        assert name in binding._SIGS, name
        assert getattr(pkg.lib(), name).argtypes is not None
    assert callable(pkg.gen_stencil27_device) and callable(pkg.DistNative.check_arrays)


def _gen(L, nx, ny, nz, dof, dec, rb, re_, out):
    return L.uspmv_gen_stencil27_device(nx, ny, nz, dof, 0x5EED, dec, rb, re_, None, out)


def test_generator_refuses_like_the_host_function_before_any_hip_call(pkg):
    """every case is also put to uspmv_gen_stencil27: same status (the decades case apart, which only the device generator refuses)"""
    L = pkg.lib()
    err = lambda: L.uspmv_last_error().decode()
    h = C.c_void_p()
    n = 4 * 3 * 2
    cases = [((4, 3, 2, 1, 0.0, 0, n, None), INVALID, "bad argument"),
             ((0, 3, 2, 1, 0.0, 0, n, C.byref(h)), INVALID, "bad argument"),
             ((4, 3, 2, 1, 0.0, 5, 5, C.byref(h)), INVALID, "bad row range"),
             ((4, 3, 2, 1, 0.0, 7, 5, C.byref(h)), INVALID, "bad row range"),
             ((4, 3, 2, 1, 0.0, 0, n + 1, C.byref(h)), INVALID, "bad row range"),
             ((1300, 1300, 1300, 1, 0.0, 0, 1000, C.byref(h)), OVERFLOW, "rows exceed int32")]
    for args, status, text in cases:
        assert _gen(L, *args) == status, args
        assert text in err() and "uspmv_gen_stencil27_device" in err(), (args, err())
        assert not h.value
        hh = C.c_void_p()
        host_out = None if args[-1] is None else C.byref(hh)
        assert L.uspmv_gen_stencil27(*args[:4], 0x5EED, *args[4:7], host_out) == status, args
    assert _gen(L, 4, 3, 2, 1, 4.0, 0, n, C.byref(h)) == UNSUPPORTED
    assert "magnitude_decades" in err() and not h.value


def test_check_arrays_refuses_a_null_object(pkg):
    L = pkg.lib()
    assert L.uspmv_dist_check_arrays(None, None, None, None, 0, None, None, None, 0, None, None, None) == INVALID
    assert "uspmv_dist_check_arrays" in L.uspmv_last_error().decode()
