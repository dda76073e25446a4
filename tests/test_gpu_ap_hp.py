"""Adaptive precision with an fp16 part on the MI355X (uspmv_spmv_ap_hp): ap[dp_hp], ap[sp_hp], ap[dp_sp_hp] against the pinned oracle,
composed part by part, bit for bit -- planless (lane per row), with the host-built and the device-built shared plan (equal array for
array), on handles made by uspmv_dmat_wrap, for C in {1, 2, 8, 10, 32, 64, 128} and several sigma.  The reference's own GPU path stops
at "not yet implemented" (code/classes_structs.hpp:553-600), and interface.hpp does not compile as shipped, so the yardstick is the
oracle:
  ap[dp_hp]     spmv_scs_ap_adv with the hp values as float32 (exact)
  ap[dp_sp_hp]  spmv_scs of every part with its values widened to float64, then (d + s) + h
  ap[sp_hp]     spmv_scs_ap with an empty dp part, once per part (float x), then float32(sp + hp)
test_oracle_composition proves the composition on two-part inputs first."""
import gc
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_x, mtx_path

MATS = ["FDM-2d-16", "impcol_e", "matrix1", "myBigMat", "mySymmMat", "matrix_band_klein", "bcsstk13"]
CS = (1, 2, 8, 10, 32, 64, 128)
KINDS = ("dp_hp", "sp_hp", "dp_sp_hp")


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    yield torch


def _thresholds(m):
    a = np.abs(np.asarray(m.arrays()[2]))
    a = a[a > 0]
    return float(np.quantile(a, 0.7)), float(np.quantile(a, 0.35))


def _build(pkg, m, kind, C, sigma, t1, t2):
    """(structs hi, mid | None, hp), permutation; None when the hi part's permutation parks a non-empty row of another part on a padded
    slot (the reference overruns its chunk there, uspmv_convert_to_scs refuses)."""
    hi, mid, hp = pkg.partition_precisions_hp(m, kind, t1, t2)
    sh = pkg.convert_to_scs(hi, C, sigma, pkg.F32 if kind == "sp_hp" else pkg.F64)
    perm = sh.arrays()["old_to_new_idx"].copy()
    try:
        sm = pkg.convert_to_scs(mid, C, sigma, pkg.F32, fixed_permutation=perm) if mid is not None else None
        sq = pkg.convert_to_scs(hp, C, sigma, pkg.F16, fixed_permutation=perm)
    except pkg.UspmvError:
        return None
    for s in (sh, sm, sq):
        if s is not None:
            pkg.permute_scs_cols(s, perm)
    return (sh, sm, sq), perm


def _t(a, dt):
    return (a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"].astype(dt))


def _empty(nc):
    return (np.zeros(nc + 1, np.int32), np.zeros(nc, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))


def _oracle(orc, kind, structs, xp):
    sh, sm, sq = structs
    C, nc = sh.C, sh.n_chunks
    h, q = sh.arrays(), sq.arrays()
    if kind == "dp_hp":
        return orc.spmv_scs_ap_adv(C, nc, _t(h, np.float64), _t(q, np.float32), xp)
    if kind == "dp_sp_hp":
        d = orc.spmv_scs(C, nc, *_t(h, np.float64), xp)
        s = orc.spmv_scs(C, nc, *_t(sm.arrays(), np.float64), xp)
        hh = orc.spmv_scs(C, nc, *_t(q, np.float64), xp)
        return (d + s) + hh
    xs = xp.astype(np.float32)
    a = orc.spmv_scs_ap(C, nc, _empty(nc), _t(h, np.float32), xs.astype(np.float64), xs)
    b = orc.spmv_scs_ap(C, nc, _empty(nc), _t(q, np.float32), xs.astype(np.float64), xs)
    return (a + b).astype(np.float32)


def _x(structs, perm, kind, n):
    sh = structs[0]
    xp = np.zeros(sh.n_rows_padded)
    xp[:n] = make_x(n)[sh.arrays()["new_to_old_idx"]]
    return xp.astype(np.float32) if kind == "sp_hp" else xp


def _same(got, want):
    """bit for bit, except that a NaN equals any NaN (the sign and payload of a NaN made by inf - inf differ between CPU and GPU; an hp part
    whose values overflow binary16 to +-inf makes such rows)"""
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return np.array_equal(got[~nan].view(u), want[~nan].view(u))


def _run(pkg, t, hand, kind, xp):
    x = t.from_numpy(xp).cuda()
    y = t.full((hand[0].n_rows_padded,), 7.0, dtype=x.dtype, device="cuda")
    pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y)
    return y.cpu().numpy()


def _handles(pkg, structs):
    return [pkg.DeviceMatrix(s) if s is not None else None for s in structs]   # uspmv_dmat_wrap around torch-owned arrays


def _plans(hand):
    return [h.plan_download() if h is not None else None for h in hand]


def _same_plans(p, q):
    for part, (a, b) in enumerate(zip(p, q)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        # the line list lives with the first part; the others hold their local indices only
        for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16") if part == 0 else ("c16_ptrs", "col16"):
            assert np.array_equal(a[k], b[k]), (part, k)


def test_oracle_composition(pkg, orc):
    """The composed yardsticks reproduce the pinned two-part kernels on two-part inputs (no GPU needed)."""
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    dp, sp = pkg.partition_precisions(m, 1e3)
    sd = pkg.convert_to_scs(dp, 32, 64, pkg.F64)
    perm = sd.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, 32, 64, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(sd, perm); pkg.permute_scs_cols(ss, perm)
    d, s = sd.arrays(), ss.arrays()
    nc = sd.n_chunks
    xp = np.zeros(sd.n_rows_padded); xp[:m.n_rows] = make_x(m.n_rows)[d["new_to_old_idx"]]
    xs = xp.astype(np.float32)
    # chains in double, parts added afterwards: spmv_scs per part == spmv_scs_ap_adv
    y_adv = orc.spmv_scs_ap_adv(32, nc, _t(d, np.float64), _t(s, np.float32), xp)
    y_cmp = orc.spmv_scs(32, nc, *_t(d, np.float64), xp) + orc.spmv_scs(32, nc, *_t(s, np.float64), xp)
    assert np.array_equal(y_adv, y_cmp)
    # float products: spmv_scs_ap with an empty dp part, once per part, then added == spmv_scs_ap of the pair
    y_ap = orc.spmv_scs_ap(32, nc, _t(d, np.float64), _t(s, np.float32), xp, xs)
    y_c2 = orc.spmv_scs_ap(32, nc, _t(d, np.float64), _empty(nc), xp, xs) + orc.spmv_scs_ap(32, nc, _empty(nc), _t(s, np.float32), xp, xs)
    assert np.array_equal(y_ap, y_c2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_kinds_against_oracle(pkg, orc, torch_cuda, kind):
    t = torch_cuda
    ran = planned = 0
    for name in MATS:
        m = pkg.read_mtx(mtx_path(name))
        t1, t2 = _thresholds(m)
        for C in CS:
            for sigma in (1, 4 * C if C < 64 else 128):
                b = _build(pkg, m, kind, C, sigma, t1, t2)
                if b is None:
                    continue
                structs, perm = b
                xp = _x(structs, perm, kind, m.n_rows)
                want = _oracle(orc, kind, structs, xp)
                hand = _handles(pkg, structs)
                assert hand[0].plan_info()[0] == 0
                got = _run(pkg, t, hand, kind, xp)
                assert _same(got, want), (name, C, sigma, "planless")
                nt, ns = pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
                got = _run(pkg, t, hand, kind, xp)
                assert _same(got, want), (name, C, sigma, "host plan")
                ph = _plans(hand)
                kinds = [h.plan_info()[0] for h in hand if h is not None]
                assert len(set(kinds)) == 1 and kinds[0] == (1 if ns > 0 and ns * 2 >= nt else 0), (name, C, sigma, kinds, nt, ns)
                planned += kinds[0]
                hd = _handles(pkg, structs)
                ntd, nsd = pkg.optimize_device_ap_hp(hd[0], hd[1], hd[2])
                got = _run(pkg, t, hd, kind, xp)
                assert _same(got, want), (name, C, sigma, "device plan")
                if (ntd, nsd) == (nt, ns):
                    _same_plans(ph, _plans(hd))
                ran += 1
    assert ran >= len(MATS) * len(CS) and planned > 0, (ran, planned)


@pytest.mark.gpu
def test_empty_parts_and_rows(pkg, orc, torch_cuda):
    """A part without entries, and rows that are empty in some parts but not in others."""
    t = torch_cuda
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    a = np.abs(np.asarray(m.arrays()[2]))
    for kind in KINDS:
        for t1, t2 in ((0.0, 0.0), (np.inf, np.inf), (np.inf, 0.0), (float(a.max()), float(np.median(a)))):
            b = _build(pkg, m, kind, 32, 64, t1, t2)
            assert b is not None
            structs, perm = b
            xp = _x(structs, perm, kind, m.n_rows)
            want = _oracle(orc, kind, structs, xp)
            for how in ("none", "host", "device"):
                hand = _handles(pkg, structs)
                if how == "host":
                    pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
                elif how == "device":
                    pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2])
                assert _same(_run(pkg, t, hand, kind, xp), want), (kind, t1, t2, how)


@pytest.mark.gpu
def test_fp16_handle_refuses_one_precision_spmv(pkg, torch_cuda):
    t = torch_cuda
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    s = pkg.convert_to_scs(m, 32, 64, pkg.F16)
    A = pkg.DeviceMatrix(s)
    assert A.torch_dtype == t.float16
    d = pkg.dmat_download(A)
    assert np.array_equal(d["values"].view(np.uint16), s.arrays()["values"].view(np.uint16))
    x = t.ones(s.n_rows_padded, dtype=t.float16, device="cuda"); y = t.zeros_like(x)
    for f in (lambda: pkg.spmv(A, x, y), lambda: A.optimize(s), lambda: A.optimize_device(),
              lambda: pkg.spmmv(A, x, y, 1, s.n_rows_padded)):
        with pytest.raises(pkg.UspmvError) as e:
            f()
        assert e.value.status == 3                                            # USPMV_ERR_UNSUPPORTED
    with pytest.raises(pkg.UspmvError):
        pkg.convert_to_scs_device(m, 32, 64, pkg.F16)                         # no device-side conversion of hp parts


@pytest.mark.gpu
def test_fullsize_stencil_dp_sp_hp(pkg, orc, torch_cuda):
    """74^3 x 5 dof, magnitudes over 8 decades, thresholds that put about half of the non-zeros in hp."""
    t = torch_cuda
    m = pkg.gen_stencil27(74, 74, 74, 5, magnitude_decades=8.0)
    a = np.abs(np.asarray(m.arrays()[2]))
    t1, t2 = float(np.quantile(a, 0.8)), float(np.quantile(a, 0.5))
    structs, perm = _build(pkg, m, "dp_sp_hp", 32, 512, t1, t2)
    assert structs[2].nnz >= 0.45 * m.nnz
    xp = _x(structs, perm, "dp_sp_hp", m.n_rows)
    want = _oracle(orc, "dp_sp_hp", structs, xp)
    hand = _handles(pkg, structs)
    nt, ns = pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
    assert ns == nt and hand[0].plan_info()[0] == 1
    assert _same(_run(pkg, t, hand, "dp_sp_hp", xp), want)
    hd = _handles(pkg, structs)
    assert pkg.optimize_device_ap_hp(hd[0], hd[1], hd[2]) == (nt, ns)
    assert _same(_run(pkg, t, hd, "dp_sp_hp", xp), want)
    _same_plans(_plans(hand), _plans(hd))


@pytest.mark.gpu
def test_plan_family_create_free_loop(pkg, torch_cuda):
    t = torch_cuda
    m = pkg.gen_stencil27(40, 40, 40)
    structs, perm = _build(pkg, m, "dp_sp_hp", 32, 512, 1.0, 0.1)
    x = t.ones(structs[0].n_rows_padded, dtype=t.float64, device="cuda"); y = t.zeros_like(x)

    def cycle():
        for how in ("host", "device"):
            hand = _handles(pkg, structs)
            for _ in range(2):                         # re-planned in place: the second plan replaces the first
                if how == "host":
                    pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
                else:
                    pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2])
                pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y)
            del hand
        gc.collect()
        t.cuda.synchronize()
        t.cuda.empty_cache()

    cycle()
    free0, _ = t.cuda.mem_get_info()
    for _ in range(5):
        cycle()
    free1, _ = t.cuda.mem_get_info()
    assert free0 - free1 <= 2 << 20, f"{(free0 - free1) / 2**20:.1f} MiB of device memory lost over five cycles"


LAUNCHER_SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>
#include <hip/hip_runtime_api.h>
#include "uspmv_launchers.hpp"

typedef long ST;
// MultiPrecFuncPtr with HAVE_HALF_MATH, the __CUDACC__ form (code/classes_structs.hpp:301-333)
using MultiPrecFuncPtr = std::function<void(bool, const ST *, const ST *, const int *, const int *, const int *, const double *, double *, double *,
                                            const ST *, const ST *, const int *, const int *, const int *, const float *, float *, float *,
                                            const ST *, const ST *, const int *, const int *, const int *, const _Float16 *, _Float16 *, _Float16 *,
                                            const ST, const int *)>;

static std::vector<char> slurp(const std::string &p) {
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<char> b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
    fclose(f);
    return b;
}
static void *to_dev(const std::vector<char> &b) {
    void *d = nullptr;
    if (hipMalloc(&d, b.size() ? b.size() : 4) != hipSuccess) exit(3);
    if (b.size() && hipMemcpy(d, b.data(), b.size(), hipMemcpyHostToDevice) != hipSuccess) exit(3);
    return d;
}
template <typename T> static T *dev(const std::string &p) { return (T *)to_dev(slurp(p)); }
template <typename T> static T *dev_scalar(T v) { std::vector<char> b(sizeof(T)); memcpy(b.data(), &v, sizeof(T)); return (T *)to_dev(b); }
static void dump(const std::string &p, const void *d, size_t bytes) {
    std::vector<char> h(bytes);
    if (uspmv_stream_synchronize(nullptr) != USPMV_OK || hipMemcpy(h.data(), d, bytes, hipMemcpyDeviceToHost) != hipSuccess) exit(4);
    FILE *f = fopen(p.c_str(), "wb"); fwrite(h.data(), 1, bytes, f); fclose(f);
}

int main(int argc, char **argv) {
    const std::string d = std::string(argv[1]) + "/", kind = argv[2];
    const long C = atol(argv[3]), nc = atol(argv[4]);
    const size_t n = (size_t)(C * nc);
    const ST *dC = dev_scalar<ST>(C), *dN = dev_scalar<ST>(nc);
    int *h_cp = dev<int>(d + "h_cp"), *h_cl = dev<int>(d + "h_cl"), *h_ci = dev<int>(d + "h_ci");
    int *q_cp = dev<int>(d + "q_cp"), *q_cl = dev<int>(d + "q_cl"), *q_ci = dev<int>(d + "q_ci");
    const _Float16 *q_va = dev<_Float16>(d + "q_va");
    int *m_cp = nullptr, *m_cl = nullptr, *m_ci = nullptr;
    const float *m_va = nullptr;
    if (kind == "dp_sp_hp") { m_cp = dev<int>(d + "m_cp"); m_cl = dev<int>(d + "m_cl"); m_ci = dev<int>(d + "m_ci"); m_va = dev<float>(d + "m_va"); }
    int rank = 0;
    MultiPrecFuncPtr f;
    if (kind == "dp_hp") f = uspmv_launchers::spmv_hip_ap_dp_hp_scs_launcher<int>;
    else if (kind == "sp_hp") f = uspmv_launchers::spmv_hip_ap_sp_hp_scs_launcher<int>;
    else f = uspmv_launchers::spmv_hip_ap_dp_sp_hp_scs_launcher<int>;
    const bool sp = kind == "sp_hp";
    const void *va = sp ? (const void *)dev<float>(d + "h_va") : (const void *)dev<double>(d + "h_va");
    void *x = sp ? (void *)dev<float>(d + "x") : (void *)dev<double>(d + "x"), *y = nullptr;
    if (hipMalloc(&y, (sp ? 4 : 8) * n) != hipSuccess) exit(3);
    for (int rep = 0; rep < 2; ++rep) {          // the second call runs on the cached handles and their device-built plan
        if (hipMemset(y, 0xff, (sp ? 4 : 8) * n) != hipSuccess) exit(3);
        if (sp)
            f(false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dC, dN, h_cp, h_cl, h_ci, (const float *)va,
              (float *)x, (float *)y, dC, dN, q_cp, q_cl, q_ci, q_va, nullptr, nullptr, (ST)((n + 255) / 256), &rank);
        else
            f(false, dC, dN, h_cp, h_cl, h_ci, (const double *)va, (double *)x, (double *)y, dC, dN, m_cp, m_cl, m_ci, m_va, nullptr, nullptr,
              dC, dN, q_cp, q_cl, q_ci, q_va, nullptr, nullptr, (ST)((n + 255) / 256), &rank);
        dump(d + "y" + std::to_string(rep), y, (sp ? 4 : 8) * n);
    }
    uspmv_launchers::release();
    printf("OK\n");
    return 0;
}
'''


@pytest.mark.gpu
def test_half_math_launchers(tmp_path, pkg, orc):
    """include/uspmv_launchers.hpp with -DHAVE_HALF_MATH: the three launchers convert to MultiPrecFuncPtr of that shape and reproduce
    the oracle bit for bit (C = 32: device-built plan; C = 10: lane per row)."""
    src = tmp_path / "l.cpp"
    src.write_text("#include <cstring>\n" + LAUNCHER_SRC)
    exe = str(tmp_path / "l")
    libdir = os.path.join(ROOT, "ultimate-spmv_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-DHAVE_HALF_MATH", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", libdir, "-luspmv", f"-Wl,-rpath,{libdir}"])
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    t1, t2 = _thresholds(m)
    d = str(tmp_path)

    def dump(name, arr):
        np.ascontiguousarray(arr).tofile(os.path.join(d, name))

    for kind in KINDS:
        for C in (32, 10):
            structs, perm = _build(pkg, m, kind, C, C, t1, t2)
            xp = _x(structs, perm, kind, m.n_rows)
            for tag, s in zip("hmq", structs):
                if s is None:
                    continue
                a = s.arrays()
                dump(tag + "_cp", a["chunk_ptrs"]); dump(tag + "_cl", a["chunk_lengths"]); dump(tag + "_ci", a["col_idxs"])
                dump(tag + "_va", a["values"])
            dump("x", xp)
            r = subprocess.run([exe, d, kind, str(C), str(structs[0].n_chunks)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (kind, C, r.stdout, r.stderr)
            want = _oracle(orc, kind, structs, xp)
            for rep in range(2):
                got = np.fromfile(os.path.join(d, f"y{rep}"), want.dtype)
                assert _same(got, want), (kind, C, rep)
