"""Column-window sweep for adaptive precision with an fp16 part (csrc/sweep_ap_hp_kernels.hip; plans: host/sweep_plan.cpp and
csrc/sweep_plan_kernels.hip with two or three parts): ap[dp_hp], ap[sp_hp], ap[dp_sp_hp] on banded-random matrices whose rows are too
wide for the shared line plan, against the pinned oracle composed part by part (the helpers of tests/test_gpu_ap_hp.py), bit for bit.
The matrices have a multiple of 128 rows, so no row slot is padded and no conversion is declined: every test counts its cases."""
import gc
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_x

pytestmark = pytest.mark.gpu

KINDS = ("dp_hp", "sp_hp", "dp_sp_hp")
DEFAULTS = dict(sweep=1, sweep_nbuf=1, sweep_unroll=8, sweep_pair=2, sweep_wlog=0, sweep_tile_rows=0, sweep_max_stage=0, tlc=1)


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    pkg.set_tuning(**DEFAULTS)
    yield torch
    pkg.set_tuning(**DEFAULTS)


@pytest.fixture(scope="module")
def banded(pkg):
    """51 200 x 70 over +-6 000 columns, magnitudes over 10 decades; t1 / t2: 30 % of the entries in hi, 70 % in hp or 35 % + 35 %"""
    m = pkg.gen_banded_random(51200, 70, 6000, magnitude_decades=10.0)
    return m, _thresholds(m)


def _thresholds(m, q1=0.7, q2=0.35):
    a = np.abs(np.asarray(m.arrays()[2]))
    a = a[(a > 0) & np.isfinite(a)]
    return float(np.quantile(a, q1)), float(np.quantile(a, q2))


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


def _x(structs, perm, kind, n, special=False):
    sh = structs[0]
    xp = np.zeros(sh.n_rows_padded)
    xp[:n] = make_x(n)[sh.arrays()["new_to_old_idx"]]
    if special:
        xp[0] = -np.inf; xp[3] = -0.0; xp[17] = np.nan
    return xp.astype(np.float32) if kind == "sp_hp" else xp


def _same(got, want):
    """bit for bit, except that a NaN equals any NaN (the sign and payload of a NaN made by inf - inf differ between CPU and GPU; an hp part
    whose values overflow binary16 to +-inf makes such rows)"""
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return np.array_equal(got[~nan].view(u), want[~nan].view(u))


def _run(pkg, t, hand, kind, xp, x=None):
    if x is None:
        x = t.from_numpy(xp).cuda()
    y = t.full((hand[0].n_rows_padded,), 7.0, dtype=x.dtype, device="cuda")
    pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y)
    return y.cpu().numpy()


def _handles(pkg, structs):
    return [pkg.DeviceMatrix(s) if s is not None else None for s in structs]   # uspmv_dmat_wrap around torch-owned arrays


def _kinds(hand):
    return [h.plan_info()[0] for h in hand if h is not None]


def _digests(hand):
    """the shared arrays of the plan and every part's, as digests"""
    n_parts = sum(h is not None for h in hand)
    d, meta = hand[0].sweep_plan_digest()
    parts = [hand[0].sweep_plan_digest_part(p) for p in range(3)]
    # the whole-plan digest carries parts 0 and 1 at [4:9] and [10:15], their stream lengths in meta[6] and meta[7]
    assert d[4:9] == parts[0][0] and d[10:15] == parts[1][0], (d, parts)
    assert meta[6] == parts[0][1] and meta[7] == parts[1][1], (meta, parts)
    return d[:5] + d[9:10], meta[:6], parts, n_parts


def _same_sweep_plans(a, b):
    da, db = _digests(a), _digests(b)
    assert da == db, (da, db)
    n_parts = da[3]
    for p in range(3):                       # every part the split has holds a stream; a part it has not is all zeros
        dig, n_vals = da[2][p]
        assert (any(dig) and n_vals >= 0) if p < n_parts else (not any(dig) and n_vals == 0), (p, n_parts, dig, n_vals)


def test_optimize_falls_through_to_the_sweep(pkg, orc, torch_cuda, banded):
    """planless, optimize_ap_hp, optimize_device_ap_hp on fresh wrapped handles: the line plan stages fewer than half of the tiles, so both
    planners end on the sweep (kind 2 on every part, every tile covered) with equal arrays; y equals the oracle each time."""
    t = torch_cuda
    m, (t1, t2) = banded
    cases = 0
    for kind in KINDS:
        for C in (8, 32, 64):
            for sigma in (1, 128):
                b = _build(pkg, m, kind, C, sigma, t1, t2)
                assert b is not None, (kind, C, sigma)
                structs, perm = b
                xp = _x(structs, perm, kind, m.n_rows)
                want = _oracle(orc, kind, structs, xp)
                hand = _handles(pkg, structs)
                assert _kinds(hand)[0] == 0
                assert _same(_run(pkg, t, hand, kind, xp), want), (kind, C, sigma, "planless")
                nt, ns = pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
                assert ns * 2 < nt, (kind, C, sigma, nt, ns)                       # (n_tiles / n_staged: the line plan's outcome)
                assert set(_kinds(hand)) == {2}, (kind, C, sigma, _kinds(hand))
                for h in hand:
                    if h is not None:
                        k, a, n = h.plan_info()
                        assert a == n and n > 0, (kind, C, sigma, a, n)
                assert _same(_run(pkg, t, hand, kind, xp), want), (kind, C, sigma, "host plan")
                hd = _handles(pkg, structs)
                ntd, nsd = pkg.optimize_device_ap_hp(hd[0], hd[1], hd[2])
                assert nsd * 2 < ntd, (kind, C, sigma, ntd, nsd)
                assert set(_kinds(hd)) == {2}, (kind, C, sigma, _kinds(hd))
                assert _same(_run(pkg, t, hd, kind, xp), want), (kind, C, sigma, "device plan")
                _same_sweep_plans(hand, hd)
                cases += 1
    assert cases == 18


def test_explicit_entry_points_and_tunings(pkg, orc, torch_cuda, banded):
    """non-default windows and tiles (2048 and 4096 rows: 2 and 4 rows per lane) through both explicit entry points, and every
    sweep_pair / sweep_unroll / sweep_nbuf form: the same bits every time"""
    t = torch_cuda
    m, (t1, t2) = banded
    cases = 0
    for kind in KINDS:
        for C, sigma in ((32, 512), (64, 64)):
            b = _build(pkg, m, kind, C, sigma, t1, t2)
            assert b is not None
            structs, perm = b
            for special in (False, True):
                xp = _x(structs, perm, kind, m.n_rows, special)
                want = _oracle(orc, kind, structs, xp)
                x = t.from_numpy(xp).cuda()
                hand, hd = _handles(pkg, structs), _handles(pkg, structs)
                for wlog, rows in ((11, 256), (12, 1024), (12, 2048), (13, 4096), (0, 0)):
                    if special and rows not in (1024, 4096):
                        continue
                    nt, ns = pkg.optimize_sweep_ap_hp(hand[0], hand[1], hand[2], *structs, wlog, rows)
                    assert ns == nt and set(_kinds(hand)) == {2}, (kind, C, sigma, wlog, rows, nt, ns)
                    assert pkg.optimize_sweep_device_ap_hp(hd[0], hd[1], hd[2], wlog, rows) == (nt, ns)
                    _same_sweep_plans(hand, hd)
                    for pair in (0, 1, 2):
                        for un in (4, 8):
                            for nbuf in (1, 2):
                                pkg.set_tuning(sweep_pair=pair, sweep_unroll=un, sweep_nbuf=nbuf)
                                for hs in (hand, hd) if (pair, un, nbuf) == (2, 8, 1) else (hand,):
                                    assert _same(_run(pkg, t, hs, kind, xp, x), want), (kind, C, sigma, special, wlog, rows, pair, un, nbuf)
                    pkg.set_tuning(**DEFAULTS)
                    cases += 1
    assert cases == 3 * 2 * (5 + 2)


def _edit(pkg, m, fn):
    I, J, v = (np.array(a) for a in m.arrays())
    fn(I, J, v)
    return pkg.Coo.from_arrays(m.n_rows, m.n_cols, I, J, v)


def test_partial_coverage_runs_the_chunk_list_kernel(pkg, orc, torch_cuda):
    """tiles that do not qualify -- more than 255 entries of one part in a window (the rows at the matrix' edge, whose band is cut in
    half), a row with unsorted columns -- run on the chunk-list form of the lane-per-row kernel inside the same call"""
    t = torch_cuda
    cases = 0
    wide = pkg.gen_banded_random(5120, 400, 2400, magnitude_decades=10.0)

    def swap(I, J, v):
        e = np.flatnonzero(I == 3000)
        J[e[0]], J[e[-1]] = J[e[-1]], J[e[0]]
        v[e[0]] = v[e[-1]] = 0.5 * np.abs(v[v != 0]).min()       # both into the hp part, whatever the thresholds
    unsorted = _edit(pkg, pkg.gen_banded_random(8192, 40, 3000, magnitude_decades=10.0), swap)
    for name, m, q, wlog in (("wide", wide, (0.02, 0.01), 11), ("unsorted", unsorted, (0.7, 0.35), 9)):
        t1, t2 = _thresholds(m, *q)
        for kind in KINDS:
            structs, perm = _build(pkg, m, kind, 32, 1, t1, t2)
            xp = _x(structs, perm, kind, m.n_rows)
            want = _oracle(orc, kind, structs, xp)
            hand, hd = _handles(pkg, structs), _handles(pkg, structs)
            pkg.set_tuning(sweep_max_stage=1 << 20)
            nt, ns = pkg.optimize_sweep_ap_hp(hand[0], hand[1], hand[2], *structs, wlog, 256)
            assert 0 < ns < nt, (name, kind, nt, ns)
            assert pkg.optimize_sweep_device_ap_hp(hd[0], hd[1], hd[2], wlog, 256) == (nt, ns)
            pkg.set_tuning(**DEFAULTS)
            _same_sweep_plans(hand, hd)
            assert hand[0].sweep_plan_digest()[1][5] > 0                                   # chunks left to the lane-per-row kernel
            for hs in (hand, hd):
                assert _same(_run(pkg, t, hs, kind, xp), want), (name, kind)
            cases += 1
    assert cases == 6


def test_special_values(pkg, orc, torch_cuda):
    """+-0, +-inf, NaN (ap[dp_sp_hp]: the other kinds' split refuses it), hp values that overflow binary16 to +-inf, an explicit +0 on a
    row's last column (stripped like the padding it cannot be told from, applied once), against a special x"""
    t = torch_cuda
    base = pkg.gen_banded_random(20480, 40, 3000, magnitude_decades=10.0)
    cases = 0
    for kind in KINDS:
        def special(I, J, v):
            e = np.arange(len(v))
            last = np.flatnonzero(np.r_[I[1:] != I[:-1], True])
            v[e % 97 == 1] = -0.0
            v[e % 97 == 2] = 0.0
            v[e % 1009 == 3] = np.inf
            v[e % 1009 == 4] = -np.inf
            v[e % 211 == 5] = 7e4
            v[e % 211 == 6] = -7e4
            v[e % 13 == 7] = 3e5 + (e[e % 13 == 7] % 1000)
            v[e % 13 == 8] = 2e6 + (e[e % 13 == 8] % 1000) / 3.0
            if kind == "dp_sp_hp":
                v[e % 1013 == 9] = np.nan
            v[last[I[last] % 3 == 0]] = 0.0
        m = _edit(pkg, base, special)
        for C, sigma, wlog, rows in ((32, 512, 10, 1024), (64, 128, 9, 2048), (8, 1, 11, 256)):
            b = _build(pkg, m, kind, C, sigma, 1e6, 1e5)      # 7e4 lands in the hp part of every kind and overflows binary16 there
            assert b is not None
            structs, perm = b
            assert np.isinf(structs[2].arrays()["values"].view(np.float16)).any()
            xp = _x(structs, perm, kind, m.n_rows, special=True)
            want = _oracle(orc, kind, structs, xp)
            assert np.isnan(want).any() and np.isinf(want).any()
            hand, hd = _handles(pkg, structs), _handles(pkg, structs)
            y0 = _run(pkg, t, hand, kind, xp)
            assert _same(y0, want), (kind, C, sigma, "planless")
            nt, ns = pkg.optimize_sweep_ap_hp(hand[0], hand[1], hand[2], *structs, wlog, rows)
            assert ns == nt
            assert pkg.optimize_sweep_device_ap_hp(hd[0], hd[1], hd[2], wlog, rows) == (nt, ns)
            _same_sweep_plans(hand, hd)
            for pair in (0, 2):
                pkg.set_tuning(sweep_pair=pair)
                for hs in (hand, hd):
                    assert _same(_run(pkg, t, hs, kind, xp), want), (kind, C, sigma, pair)
            pkg.set_tuning(**DEFAULTS)
            cases += 1
    assert cases == 9


def test_fallbacks_sweep_off_and_unaligned_x(pkg, orc, torch_cuda, banded):
    """set_tuning(sweep=0) at call time and an x that is not 16-byte aligned: the same handles give the same bits without the sweep"""
    t = torch_cuda
    m, (t1, t2) = banded
    cases = 0
    for kind in KINDS:
        structs, perm = _build(pkg, m, kind, 32, 128, t1, t2)
        xp = _x(structs, perm, kind, m.n_rows)
        want = _oracle(orc, kind, structs, xp)
        hand = _handles(pkg, structs)
        pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
        assert set(_kinds(hand)) == {2}
        assert _same(_run(pkg, t, hand, kind, xp), want)
        pkg.set_tuning(sweep=0)
        assert _same(_run(pkg, t, hand, kind, xp), want), (kind, "sweep off")
        pkg.set_tuning(sweep=1)
        buf = t.zeros(len(xp) + 4, dtype=t.from_numpy(xp).dtype, device="cuda")
        xu = buf[1:1 + len(xp)]
        xu.copy_(t.from_numpy(xp))
        assert xu.data_ptr() % 16 != 0
        assert _same(_run(pkg, t, hand, kind, xp, xu), want), (kind, "unaligned x")
        cases += 1
    assert cases == 3


def test_fullsize_banded_dp_sp_hp(pkg, orc, torch_cuda):
    """The HV15R-class matrix of DESIGN 5.6: 500 000 x 140 over +-50 000 columns, 10 decades, t1 / t2 at the 0.8 / 0.4 quantiles."""
    t = torch_cuda
    m = pkg.gen_banded_random(500000, 140, 50000, magnitude_decades=10.0)
    t1, t2 = _thresholds(m, 0.8, 0.4)
    b = _build(pkg, m, "dp_sp_hp", 32, 512, t1, t2)
    assert b is not None
    structs, perm = b
    xp = _x(structs, perm, "dp_sp_hp", m.n_rows)
    want = _oracle(orc, "dp_sp_hp", structs, xp)
    hand = _handles(pkg, structs)
    nt, ns = pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
    assert ns * 2 < nt and set(_kinds(hand)) == {2}
    k, a, n = hand[0].plan_info()
    assert a == n
    assert _same(_run(pkg, t, hand, "dp_sp_hp", xp), want)
    hd = _handles(pkg, structs)
    ntd, nsd = pkg.optimize_device_ap_hp(hd[0], hd[1], hd[2])
    assert nsd * 2 < ntd and set(_kinds(hd)) == {2}
    assert _same(_run(pkg, t, hd, "dp_sp_hp", xp), want)
    _same_sweep_plans(hand, hd)


def test_sweep_plan_create_free_loop(pkg, torch_cuda, banded):
    t = torch_cuda
    m, (t1, t2) = banded
    structs, perm = _build(pkg, m, "dp_sp_hp", 32, 512, t1, t2)
    x = t.ones(structs[0].n_rows_padded, dtype=t.float64, device="cuda"); y = t.zeros_like(x)

    def cycle():
        for how in ("host", "device", "host explicit", "device explicit"):
            hand = _handles(pkg, structs)
            for rep in range(2):                       # re-planned in place: the second plan replaces the first
                if how == "host":
                    pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *structs)
                elif how == "device":
                    pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2])
                elif how == "host explicit":
                    pkg.optimize_sweep_ap_hp(hand[0], hand[1], hand[2], *structs, 12, 1024 << rep)
                else:
                    pkg.optimize_sweep_device_ap_hp(hand[0], hand[1], hand[2], 12, 1024 << rep)
                assert set(_kinds(hand)) == {2}
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


# the HAVE_HALF_MATH launcher program of tests/test_gpu_ap_hp.py
LAUNCHER_SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
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


def test_half_math_launchers_reach_the_sweep(tmp_path, pkg, orc, banded):
    """The launchers of include/uspmv_launchers.hpp plan through uspmv_dmat_optimize_device_ap_hp: on a banded matrix that is the sweep
    (the device builder reports its plan under USPMV_VERBOSE), and y of both calls equals the oracle."""
    src = tmp_path / "l.cpp"
    src.write_text(LAUNCHER_SRC)
    exe = str(tmp_path / "l")
    libdir = os.path.join(ROOT, "ultimate-spmv_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-DHAVE_HALF_MATH", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", libdir, "-luspmv", f"-Wl,-rpath,{libdir}"])
    m, (t1, t2) = banded
    d = str(tmp_path)

    def dump(name, arr):
        np.ascontiguousarray(arr).tofile(os.path.join(d, name))

    cases = 0
    for kind in KINDS:
        structs, perm = _build(pkg, m, kind, 32, 32, t1, t2)
        xp = _x(structs, perm, kind, m.n_rows)
        for tag, s in zip("hmq", structs):
            if s is None:
                continue
            a = s.arrays()
            dump(tag + "_cp", a["chunk_ptrs"]); dump(tag + "_cl", a["chunk_lengths"]); dump(tag + "_ci", a["col_idxs"])
            dump(tag + "_va", a["values"])
        dump("x", xp)
        r = subprocess.run([exe, d, kind, "32", str(structs[0].n_chunks)], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, USPMV_VERBOSE="1"))
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (kind, r.stdout, r.stderr)
        lines = [ln for ln in r.stderr.splitlines() if "sweep plan (device builder)" in ln]
        assert lines, (kind, r.stderr)
        f = dict(kv.split("=") for kv in lines[-1].split() if "=" in kv)
        assert int(f["sweep"]) == int(f["tiles"]) > 0, (kind, lines[-1])
        want = _oracle(orc, kind, structs, xp)
        for rep in range(2):
            got = np.fromfile(os.path.join(d, f"y{rep}"), want.dtype)
            assert _same(got, want), (kind, rep)
        cases += 1
    assert cases == 3
