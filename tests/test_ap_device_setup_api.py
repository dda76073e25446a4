"""Adaptive-precision set-up from device-resident COO arrays, the part that needs no device: the argument refusals of
uspmv_partition_precisions_device / uspmv_convert_to_scs_device_ap_from_arrays come before the device check, and the rounding text the
partition kernels compile (ultimate-spmv_amd/host/uspmv_f16_round.hpp) is compiled with g++ into tests/cpp/f16_round_check.cpp and compared
with numpy's float64 -> float16, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INVALID, UNSUPPORTED, NO_DEVICE = 1, 3, 5


def _partition(L, I, J, V, n_rows, n_cols, nnz, kind, parts):
    p = lambda a: None if a is None else a.ctypes.data
    return L.uspmv_partition_precisions_device(p(I), p(J), p(V), n_rows, n_cols, nnz, kind, 1.0, 0.5, None, parts)


def _one_call(L, I, J, V, n_rows, n_cols, nnz, Cc, sigma, kind, sort, hi, mid, lo):
    p = lambda a: None if a is None else a.ctypes.data
    ref = lambda h: None if h is None else C.byref(h)
    return L.uspmv_convert_to_scs_device_ap_from_arrays(p(I), p(J), p(V), n_rows, n_cols, nnz, Cc, sigma, kind, 1.0, 0.5, sort, None, None, None, None,
                                                        None, ref(hi), ref(mid), ref(lo))


def test_refusals_come_before_the_device_check(pkg):
    L = pkg.lib()
    err = lambda: L.uspmv_last_error().decode()
    I = np.zeros(4, np.int32); J = np.zeros(4, np.int32); V = np.ones(4)        # host arrays: every call below is refused before they are read
    parts = (C.c_void_p * 3)()
    assert L.uspmv_partition_precisions_device(None, None, None, 4, 4, 0, pkg.AP_DP_SP, 1.0, 0.0, None, None) == INVALID
    for a, b, c in ((None, J, V), (I, None, V), (I, J, None)):
        assert _partition(L, a, b, c, 4, 4, 4, pkg.AP_DP_SP, parts) == INVALID and "bad argument" in err()
    assert _partition(L, I, J, V, 4, 4, -1, pkg.AP_DP_SP, parts) == INVALID
    for kind in (-1, 4, 99):
        assert _partition(L, I, J, V, 4, 4, 4, kind, parts) == INVALID and f"unknown kind {kind}" in err()
    assert _partition(L, I, J, V, 0, 4, 4, pkg.AP_DP_HP, parts) == INVALID and "no rows" in err()
    assert all(not h for h in parts)

    hi, mid, lo = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok = dict(n_rows=4, n_cols=4, nnz=4, Cc=2, sigma=2, kind=pkg.AP_DP_SP_HP, sort=pkg.SORT_HOST, hi=hi, mid=mid, lo=lo)
    for change, text in ((dict(I=None), "bad argument"), (dict(J=None), "bad argument"), (dict(V=None), "bad argument"), (dict(kind=5), "unknown kind 5"),
                         (dict(n_rows=0), "no rows"), (dict(Cc=0), "C and sigma"), (dict(sigma=0), "C and sigma"), (dict(sort=2), "unknown sort mode 2"),
                         (dict(hi=None), "NULL output"), (dict(lo=None), "NULL output"), (dict(mid=None), "NULL output")):
        kw = dict(ok, I=I, J=J, V=V); kw.update(change)
        assert _one_call(L, **kw) == INVALID and text in err(), change
    for kind in (pkg.AP_DP_SP, pkg.AP_DP_HP, pkg.AP_SP_HP):                      # the two-part kinds have no mid part to return
        kw = dict(ok, I=I, J=J, V=V, kind=kind, mid=None, Cc=0)
        assert _one_call(L, **kw) == INVALID and "C and sigma" in err()
    assert not hi.value and not mid.value and not lo.value


def test_valid_arguments_reach_the_device_check(pkg):
    """An empty matrix (no array is read): USPMV_ERR_NO_DEVICE where there is no GPU, an empty set of parts / handles where there is one.
    The plain conversion takes USPMV_F16 now and still refuses an unknown dtype."""
    L = pkg.lib()
    have = pkg.device_count() > 0
    parts = (C.c_void_p * 3)()
    rc = _partition(L, None, None, None, 4, 4, 0, pkg.AP_DP_SP_HP, parts)
    assert rc == (0 if have else NO_DEVICE), L.uspmv_last_error()
    for h in parts:
        if h:
            L.uspmv_dcoo_free(h)
    hi, mid, lo = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = _one_call(L, None, None, None, 4, 4, 0, 2, 2, pkg.AP_DP_SP_HP, pkg.SORT_HOST, hi, mid, lo)
    assert rc == (0 if have else NO_DEVICE), L.uspmv_last_error()
    for h in (hi, mid, lo):
        if h.value:
            L.uspmv_dmat_free(h)
    out = C.c_void_p()
    plain = lambda dtype: L.uspmv_convert_to_scs_device_from_arrays(None, None, None, 4, 4, 0, 2, 2, dtype, None, 1, pkg.SORT_HOST, None, None, None, None, C.byref(out))
    assert plain(7) == INVALID and "unknown dtype 7" in L.uspmv_last_error().decode()
    rc = plain(pkg.F16)
    assert rc == (0 if have else NO_DEVICE), L.uspmv_last_error()
    if out.value:
        L.uspmv_dmat_free(out)


def _patterns():
    rng = np.random.default_rng(16)
    halves = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float64)       # every half value, widened (NaNs with their payloads)
    fin = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)          # 0 .. 65504: neighbours a < b
    mid = (fin[:-1] + fin[1:]) / 2                                                        # exact in double: the half-way points
    mid = np.concatenate([mid, [65520.0]])                                                # ... and the one between 65504 and "65536"
    ties = np.concatenate([mid, np.nextafter(mid, 0.0), np.nextafter(mid, np.inf)])
    named = np.array([1 + 2.0 ** -11 + 2.0 ** -30, 2.0 ** -25, np.nextafter(2.0 ** -25, 0.0), np.nextafter(2.0 ** -25, 1.0), 65504.0,
                      np.nextafter(65520.0, 0.0), 65520.0, 65536.0, 0.0, np.inf, 2.0 ** -24, 2.0 ** -14, 5e-324, 2.2250738585072014e-308, 1e-40, 1e-46,
                      1e39, 1e300])
    nans = np.array([0x7FF0000000000001, 0x7FF8000000000000, 0x7FF4000000000000, 0x7FF00000000003FF, 0x7FF0040000000000, 0x7FF0020000000000,
                     0x7FFFFFFFFFFFFFFF, 0x7FF8000000000001, 0x7FF0000080000000], dtype=np.uint64)
    vals = np.concatenate([halves, ties, -ties, named, -named]).view(np.uint64)
    return np.concatenate([rng.integers(0, 2 ** 64, 10 ** 6, dtype=np.uint64), vals, nans, nans | np.uint64(1 << 63)])


def test_rounding_header_equals_numpy_bit_for_bit(pkg, tmp_path):
    exe = str(tmp_path / "f16_round_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "ultimate-spmv_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "f16_round_check.cpp"), "-o", exe])
    pat = _patterns()
    fin, fh, fw = (str(tmp_path / n) for n in ("in.bin", "half.bin", "wide.bin"))
    pat.tofile(fin)
    out = subprocess.run([exe, fin, fh, fw], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == f"{pat.size} OK", out.stdout + out.stderr
    with np.errstate(over="ignore", invalid="ignore"):
        want = pat.view(np.float64).astype(np.float16)
    got = np.fromfile(fh, np.uint16)
    bad = np.flatnonzero(got != want.view(np.uint16))
    assert bad.size == 0, [(hex(int(pat[k])), hex(int(got[k])), hex(int(want.view(np.uint16)[k]))) for k in bad[:8]]
    assert np.array_equal(np.fromfile(fw, np.uint64), want.astype(np.float64).view(np.uint64))
    # the example checked by hand: one rounding gives 0x3C01, the path through float 0x3C00
    k = int(np.flatnonzero(pat == np.array([1 + 2.0 ** -11 + 2.0 ** -30]).view(np.uint64)[0])[0])
    assert got[k] == 0x3C01 and np.float32(1 + 2.0 ** -11 + 2.0 ** -30).astype(np.float16).view(np.uint16) == 0x3C00
    # ... and the library's own routine (the same text, compiled into libuspmv.so) through the host partition
    v = pat[:4096].view(np.float64)
    v = v[np.isfinite(v)]
    m = pkg.Coo.from_arrays(v.size, 1, np.arange(v.size), np.zeros(v.size), v)
    _, _, hp = pkg.partition_precisions_hp(m, "dp_hp", np.inf)
    with np.errstate(over="ignore"):
        assert np.array_equal(np.array(hp.arrays()[2]).view(np.uint64), v.astype(np.float16).astype(np.float64).view(np.uint64))
