"""Adaptive-precision set-up from device-resident COO arrays: uspmv_partition_precisions_device (csrc/ap_partition_kernels.hip) against
uspmv_partition_precisions[_hp], and uspmv_convert_to_scs_device_ap_from_arrays against the host route (partition -> convert_to_scs, the
other parts with the first part's permutation as fixed permutation -> permute_scs_cols of every part with the first part's old_to_new ->
upload), for ap[dp_sp], ap[dp_hp], ap[sp_hp] and ap[dp_sp_hp].  Everything is compared bit for bit: the parts' I, J and V (V as uint64),
the handles' arrays (fp16 values as uint16), the layout and the permutations, and y of spmv_ap / spmv_ap_hp on the device-built handles
against the oracle and against the host-built handles."""
import gc

import numpy as np
import pytest

from conftest import make_x
from test_gpu_ap_hp import _oracle as hp_oracle, _same
from test_gpu_convert_device import matrices as convert_matrices

pytestmark = pytest.mark.gpu
KINDS = ("dp_sp", "dp_hp", "sp_hp", "dp_sp_hp")
CSIG = ((1, 1), (4, 4), (16, 512), (32, 512), (32, 1), (5, 7), (64, 128))
# the partition's own constants: a workgroup takes PER_WG entries and writes one count per part, the scan works in blocks of SCAN_BLOCK
PER_WG, SCAN_BLOCK = 1024, 1024
PAD_REFUSED = dict(n=17, C=8, sigma=32, sp_only=3)      # found on the CPU with the host path: see test_padded_slot_refusal


@pytest.fixture(scope="module")
def t(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


def big_random(pkg):
    """2 000 rows of 160 .. 192 entries: 3 * ceil(nnz / PER_WG) counts must exceed one scan block, i.e. nnz > 341 * 1024 = 349 184, which
    a mean row length of 176 gives (352 000 +- 1 000); magnitudes over eight decades"""
    rng = np.random.default_rng(11)
    n = 2000
    I = np.repeat(np.arange(n), rng.integers(160, 193, n))
    V = rng.standard_normal(I.size) * 10.0 ** rng.uniform(-6, 2, I.size)
    m = pkg.Coo.from_arrays(n, n, I, rng.integers(0, n, I.size), V)
    assert 3 * -(-m.nnz // PER_WG) > SCAN_BLOCK, m.nnz
    return m


@pytest.fixture(scope="module")
def mats(pkg):
    names = ["FDM-2d-16", "impcol_e", "bcsstk13", "matrix1", "matrix_band_klein", "ragged300", "stencil", "stencil_decades", "random2000"]
    return list(zip(names, convert_matrices(pkg) + [pkg.gen_stencil27(9, 11, 13, magnitude_decades=6.0), big_random(pkg)]))


def dev_coo(t, m):
    I, J, V = m.arrays()
    return t.from_numpy(np.array(I)).cuda(), t.from_numpy(np.array(J)).cuda(), t.from_numpy(np.array(V)).cuda()


def thresholds(m, kind):
    """(t1, t2, balanced).  Matrices with many magnitudes: quantiles that give the hi part 40 % of the entries of a two-part kind, every
    part a third of a three-part kind.  FDM-2d-16 and matrix_band_klein hold two and three magnitudes: no threshold balances them, theirs
    are the largest and the smallest magnitude themselves (values exactly equal to t1 and t2)."""
    a = np.abs(np.asarray(m.arrays()[2]))
    u = np.unique(a)
    if u.size < 50:
        return float(u[-1]), float(u[0]), False
    if kind == "dp_sp_hp":
        return float(np.quantile(a, 2 / 3)), float(np.quantile(a, 1 / 3)), True
    return float(np.quantile(a, 0.6)), 0.0, True


def host_parts(pkg, m, kind, t1, t2):
    if kind == "dp_sp":
        dp, sp = pkg.partition_precisions(m, t1)
        return [dp, None, sp]
    return list(pkg.partition_precisions_hp(m, kind, t1, t2))


def same_parts(pkg, t, m, kind, t1, t2, dev=None):
    want = host_parts(pkg, m, kind, t1, t2)
    dI, dJ, dV = dev if dev is not None else dev_coo(t, m)
    got = pkg.partition_precisions_device(dI, dJ, dV, m.n_rows, m.n_cols, kind, t1, t2)
    assert len(got) == 3
    for p, (w, g) in enumerate(zip(want, got)):
        assert (w is None) == (g is None), (kind, p)
        if w is None:
            continue
        wI, wJ, wV = (np.array(a) for a in w.arrays())
        gI, gJ, gV = (a.cpu().numpy() for a in g)
        assert gI.size == w.nnz, (kind, p, gI.size, w.nnz)
        assert np.array_equal(gI, wI) and np.array_equal(gJ, wJ), (kind, p)
        assert np.array_equal(gV.view(np.uint64), wV.view(np.uint64)), (kind, p)
    return want, got


def part_dtypes(pkg, kind):
    return [pkg.F32 if kind == "sp_hp" else pkg.F64, pkg.F32, pkg.F32 if kind == "dp_sp" else pkg.F16]


def host_structs(pkg, parts, kind, C, sigma):
    """the host route; None where it refuses (the first part's ordering parks a non-empty row of another part on a padded slot)"""
    dts = part_dtypes(pkg, kind)
    s0 = pkg.convert_to_scs(parts[0], C, sigma, dts[0])
    perm = s0.arrays()["old_to_new_idx"].copy()
    try:
        rest = [pkg.convert_to_scs(p, C, sigma, dt, fixed_permutation=perm) if p is not None else None for p, dt in zip(parts[1:], dts[1:])]
    except pkg.UspmvError as e:
        assert "padded slot" in str(e)
        return None
    structs = [s0] + rest
    for s in structs:
        if s is not None:
            pkg.permute_scs_cols(s, perm)
    return structs


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_handles(pkg, structs, hand, tag):
    for p, (s, A) in enumerate(zip(structs, hand)):
        assert (s is None) == (A is None), (tag, p)
        if s is None:
            continue
        a, d = s.arrays(), pkg.dmat_download(A)
        assert (A.C, A.n_chunks, A.n_elements, A.dtype) == (s.C, s.n_chunks, s.n_elements, s.dtype), (tag, p)
        for k in ("chunk_ptrs", "chunk_lengths", "col_idxs"):
            assert np.array_equal(d[k], a[k]), (tag, p, k)
        assert d["values"].dtype == a["values"].dtype and np.array_equal(bits(d["values"]), bits(a["values"])), (tag, p, "values")


@pytest.mark.parametrize("kind", KINDS)
def test_parts_equal_the_host_partition(pkg, t, mats, kind):
    for name, m in mats:
        t1, t2, balanced = thresholds(m, kind)
        want, _ = same_parts(pkg, t, m, kind, t1, t2)
        if balanced:
            fr = [w.nnz / m.nnz for w in want if w is not None]
            if kind == "dp_sp_hp":
                assert all(0.25 <= f <= 0.5 for f in fr), (name, fr)
            else:                                         # two parts cannot both stay under a half: the hi part does
                assert 0.25 <= fr[0] <= 0.5, (name, fr)


SPECIAL = np.array([1.0, -1.0, 2.0 ** -10, -2.0 ** -10, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), np.nextafter(2.0 ** -10, 0.0), 0.0, -0.0,
                    np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072009e-308, 1e-40, -1e-40, 1e-46, -1e-46, 1e39, -1e39, 1e300, -1e300,
                    1 + 2.0 ** -11 + 2.0 ** -30, -(1 + 2.0 ** -11 + 2.0 ** -30), 2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -25,
                    np.nextafter(2.0 ** -25, 1.0), np.nextafter(2.0 ** -25, 0.0), -2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 65504.0,
                    np.nextafter(65520.0, 0.0), 65520.0, -65520.0, 2.0 ** -14, np.nextafter(2.0 ** -14, 0.0), 0.1, 3.0, 1e-3])


def test_extreme_thresholds_and_special_values(pkg, t, mats):
    m = dict(mats)["stencil_decades"]
    dev = dev_coo(t, m)
    for kind in KINDS:
        want, _ = same_parts(pkg, t, m, kind, 0.0, 0.0, dev)                       # everything in the first part
        assert want[0].nnz == m.nnz and want[2].nnz == 0
        for t2 in (np.inf, 0.0):
            want, _ = same_parts(pkg, t, m, kind, np.inf, t2, dev)                 # the first part empty
            assert want[0].nnz == 0
    n = SPECIAL.size
    forms = [pkg.Coo.from_arrays(1, n, np.zeros(n), np.arange(n), SPECIAL), pkg.Coo.from_arrays(n, n, np.arange(n), (np.arange(n) * 7) % n, SPECIAL)]
    for m in forms:
        dev = dev_coo(t, m)
        for kind in KINDS:
            for t1, t2 in ((1.0, 2.0 ** -10), (np.inf, np.inf), (np.inf, 0.0), (0.0, 0.0), (1e-45, 1e-47)):
                _, got = same_parts(pkg, t, m, kind, t1, t2, dev)
                if t1 == np.inf and t2 == np.inf and kind != "dp_sp":
                    # the hp part against numpy itself: every finite value, rounded once (1 + 2^-11 + 2^-30 -> 0x3C01, half subnormals kept)
                    v = SPECIAL[np.isfinite(SPECIAL)]
                    with np.errstate(over="ignore"):
                        h = v.astype(np.float16)
                    assert np.array_equal(got[2][2].cpu().numpy().view(np.uint64), h.astype(np.float64).view(np.uint64))
                    assert h[np.flatnonzero(v == 1 + 2.0 ** -11 + 2.0 ** -30)[0]].view(np.uint16) == 0x3C01
                if t1 == np.inf and kind == "dp_sp":
                    v = SPECIAL[np.isfinite(SPECIAL)]
                    with np.errstate(over="ignore"):                               # float subnormals kept, 1e-46 -> 0, 1e39 and 1e300 -> inf
                        assert np.array_equal(got[2][2].cpu().numpy().view(np.uint64), v.astype(np.float32).astype(np.float64).view(np.uint64))


def test_sizes_around_the_wave_and_the_workgroup(pkg, t):
    rng = np.random.default_rng(5)
    for nnz in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        V = rng.standard_normal(nnz) * 10.0 ** rng.uniform(-4, 1, nnz)
        for m in (pkg.Coo.from_arrays(1, nnz, np.zeros(nnz), np.arange(nnz), V), pkg.Coo.from_arrays(nnz, nnz, np.arange(nnz), rng.integers(0, nnz, nnz), V)):
            dev = dev_coo(t, m)
            for kind in KINDS:
                same_parts(pkg, t, m, kind, 1e-1, 1e-3, dev)
    # arrays that start at an odd element: the kernels' 16-byte loads need the 8-byte loads instead
    m = pkg.Coo.from_arrays(1, 1025, np.zeros(1025), np.arange(1025), rng.standard_normal(1025))
    I, J, V = (np.array(a) for a in m.arrays())
    pad = lambda a: t.from_numpy(np.concatenate([a[:1], a])).cuda()[1:]
    for kind in KINDS:
        same_parts(pkg, t, m, kind, 0.5, 0.1, (pad(I), pad(J), pad(V)))


def test_class_patterns(pkg, t):
    """which part an entry goes to, laid out against the kernels' units: alternating classes, whole workgroups of one class, one foreign
    entry in the first and the last lane of a wave (a lane holds two neighbouring entries, a wave 128, a round 512, a workgroup 1024)"""
    nnz = 3 * PER_WG - 72
    k = np.arange(nnz)
    cls_value = np.array([4.0, 0.5, 0.001])                                       # t1 = 1, t2 = 0.1: hi, mid, lo
    patterns = [k % 2 * 2, k % 3, (k // PER_WG) % 3, 2 - (k // PER_WG) % 3, (k // 64) % 3, (k // 128) % 2 * 2]
    for base, other in ((0, 2), (2, 0), (1, 0)):
        for where in (0, 1, 63, 64, 126, 127, 128, 511, 512, 1022, 1023, 1024, nnz - 1):
            c = np.full(nnz, base); c[where] = other
            patterns.append(c)
    for c in patterns:
        V = cls_value[c] * (1.0 + 1e-6 * k) * np.where(k % 5 == 0, -1.0, 1.0)      # every entry its own value: a wrong order shows
        for m in (pkg.Coo.from_arrays(1, nnz, np.zeros(nnz), k, V), pkg.Coo.from_arrays(nnz, nnz, k, (k * 13) % nnz, V)):
            dev = dev_coo(t, m)
            for kind in KINDS:
                same_parts(pkg, t, m, kind, 1.0, 0.1, dev)


@pytest.mark.parametrize("kind", KINDS)
def test_handles_equal_the_host_route(pkg, t, mats, kind):
    compared = refused = 0
    for name, m in mats:
        t1, t2, _ = thresholds(m, kind)
        parts = host_parts(pkg, m, kind, t1, t2)
        dI, dJ, dV = dev_coo(t, m)
        for C, sigma in CSIG:
            structs = host_structs(pkg, parts, kind, C, sigma)
            if structs is None:                           # where the host route refuses, the device route refuses alike
                with pytest.raises(pkg.UspmvError, match="padded slot"):
                    pkg.convert_ap_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, kind, t1, t2)
                refused += 1
                continue
            lay, hand, o2n, n2o, cnt = pkg.convert_ap_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, kind, t1, t2)
            assert cnt == [p.nnz if p is not None else 0 for p in parts], (name, C, sigma)
            same_handles(pkg, structs, hand, (name, kind, C, sigma))
            a, la = structs[0].arrays(), lay.arrays()
            assert (lay.C, lay.sigma, lay.n_rows, lay.n_cols, lay.n_rows_padded, lay.n_chunks, lay.n_elements, lay.nnz, lay.dtype) == \
                   (C, sigma, m.n_rows, m.n_cols, structs[0].n_rows_padded, structs[0].n_chunks, structs[0].n_elements, parts[0].nnz, structs[0].dtype)
            for k in ("chunk_ptrs", "chunk_lengths", "old_to_new_idx", "new_to_old_idx"):
                assert np.array_equal(la[k], a[k]), (name, C, sigma, k)
            assert np.array_equal(o2n.cpu().numpy(), a["old_to_new_idx"]) and np.array_equal(n2o.cpu().numpy(), a["new_to_old_idx"])
            compared += 1
    assert compared >= 6 * len(CSIG), (compared, refused)


def test_empty_first_part_takes_the_tie_order_of_all_zero_counts(pkg, t, mats):
    m = dict(mats)["bcsstk13"]
    dI, dJ, dV = dev_coo(t, m)
    for kind in KINDS:
        parts = host_parts(pkg, m, kind, np.inf, 0.0)
        assert parts[0].nnz == 0
        for C, sigma in ((32, 512), (4, 4)):
            structs = host_structs(pkg, parts, kind, C, sigma)
            if structs is None:
                with pytest.raises(pkg.UspmvError, match="padded slot"):
                    pkg.convert_ap_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, kind, np.inf, 0.0)
                continue
            lay, hand, o2n, _, _ = pkg.convert_ap_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, kind, np.inf, 0.0)
            same_handles(pkg, structs, hand, (kind, C, sigma))
            assert np.array_equal(o2n.cpu().numpy(), structs[0].arrays()["old_to_new_idx"])


def _tup(a, dt):
    return (a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"].astype(dt))


def _y(pkg, t, kind, hand, xp, x_sp=None):
    x = t.from_numpy(xp).cuda()
    y = t.full((hand[0].n_rows_padded,), 7.0, dtype=x.dtype, device="cuda")
    if kind == "dp_sp":
        pkg.spmv_ap(hand[0], hand[2], x, y, x_sp=None if x_sp is None else t.from_numpy(x_sp).cuda())
    else:
        pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y)
    return y.cpu().numpy()


def _plan(pkg, kind, hand):
    if kind == "dp_sp":
        pkg.optimize_device_ap(hand[0], hand[2])
    else:
        pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2])


def _xp(structs, kind, n):
    xp = np.zeros(structs[0].n_rows_padded)
    xp[:n] = make_x(n)[structs[0].arrays()["new_to_old_idx"]]
    return xp.astype(np.float32) if kind == "sp_hp" else xp


@pytest.mark.parametrize("kind", KINDS)
def test_results_equal_the_oracle_and_the_host_built_handles(pkg, orc, t, mats, kind):
    ran = 0
    for name, m in mats:
        if m.n_rows != m.n_cols:
            continue
        t1, t2, _ = thresholds(m, kind)
        parts = host_parts(pkg, m, kind, t1, t2)
        dI, dJ, dV = dev_coo(t, m)
        for C, sigma in ((32, 512), (16, 512), (4, 4), (64, 128)):
            structs = host_structs(pkg, parts, kind, C, sigma)
            if structs is None:
                continue
            _, hand, _, _, _ = pkg.convert_ap_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, kind, t1, t2, want_layout=False)
            host_hand = [pkg.DeviceMatrix(s) if s is not None else None for s in structs]
            xp = _xp(structs, kind, m.n_rows)
            if kind == "dp_sp":
                d, s = structs[0].arrays(), structs[2].arrays()
                want = orc.spmv_scs_ap_adv(C, structs[0].n_chunks, _tup(d, np.float64), _tup(s, np.float32), xp)
            else:
                want = hp_oracle(orc, kind, (structs[0], structs[1], structs[2]), xp)
            for planned in (False, True):
                if planned:
                    _plan(pkg, kind, hand); _plan(pkg, kind, host_hand)
                got, got_host = _y(pkg, t, kind, hand, xp), _y(pkg, t, kind, host_hand, xp)
                assert _same(got, want), (name, C, sigma, planned)
                assert np.array_equal(bits(got), bits(got_host)), (name, C, sigma, planned)
                if kind == "dp_sp":                       # the variant with a float copy of x: spmv_scs_ap
                    xs = xp.astype(np.float32)
                    want_g = orc.spmv_scs_ap(C, structs[0].n_chunks, _tup(d, np.float64), _tup(s, np.float32), xp, xs)
                    assert np.array_equal(_y(pkg, t, kind, hand, xp, xs), want_g), (name, C, sigma, planned, "generic")
            ran += 1
    assert ran >= 12, ran


def test_block_vectors_on_the_device_built_handles(pkg, t, mats):
    m = dict(mats)["stencil_decades"]
    dI, dJ, dV = dev_coo(t, m)
    for kind, b in (("dp_sp", 4), ("dp_sp_hp", 2)):
        t1, t2, _ = thresholds(m, kind)
        _, hand, o2n, _, _ = pkg.convert_ap_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, 32, 512, kind, t1, t2, want_layout=False)
        _plan(pkg, kind, hand)
        n = hand[0].n_rows_padded
        cols = [np.zeros(n) for _ in range(b)]
        for v in range(b):
            cols[v][o2n.cpu().numpy()] = make_x(m.n_rows) * (1.0 + v / 8.0)
        X = t.from_numpy(np.concatenate(cols)).cuda()
        Y = t.full((b * n,), 3.0, dtype=t.float64, device="cuda")
        if kind == "dp_sp":
            pkg.spmmv_ap(hand[0], hand[2], X, Y, b, n, pkg.COLWISE)
        else:
            pkg.spmmv_ap_hp(hand[0], hand[1], hand[2], X, Y, b, n, pkg.COLWISE)
        Y = Y.cpu().numpy()
        for v in range(b):
            assert np.array_equal(bits(Y[v * n:(v + 1) * n]), bits(_y(pkg, t, kind, hand, cols[v]))), (kind, v)


@pytest.mark.parametrize("kind", KINDS)
def test_device_stable_ordering(pkg, t, mats, kind):
    """USPMV_SORT_DEVICE_STABLE: rows of equal length keep their original order, so the first part's chunk arrays equal the host route's
    and y in ORIGINAL row order equals the host route's bit for bit (a row's entry order never changes); the other parts follow the first
    part's permutation, whatever its tie order is."""
    for name in ("impcol_e", "bcsstk13", "ragged300", "stencil_decades"):
        m = dict(mats)[name]
        t1, t2, _ = thresholds(m, kind)
        parts = host_parts(pkg, m, kind, t1, t2)
        dI, dJ, dV = dev_coo(t, m)
        for C, sigma in ((4, 4), (16, 512), (32, 512), (64, 128)):
            lay, hand, o2n, n2o, _ = pkg.convert_ap_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, kind, t1, t2, sort=pkg.SORT_DEVICE_STABLE)
            p = o2n.cpu().numpy()
            assert np.unique(p).size == m.n_rows and p.min() >= 0 and p.max() < m.n_rows
            s0 = pkg.convert_to_scs(parts[0], C, sigma, part_dtypes(pkg, kind)[0])
            a, d = s0.arrays(), pkg.dmat_download(hand[0])
            assert np.array_equal(d["chunk_lengths"], a["chunk_lengths"]) and np.array_equal(d["chunk_ptrs"], a["chunk_ptrs"]), (name, C, sigma)
            assert np.array_equal(lay.arrays()["old_to_new_idx"], p)
            structs = host_structs(pkg, parts, kind, C, sigma)
            if structs is None:
                continue
            x = make_x(m.n_rows)
            xd = np.zeros(hand[0].n_rows_padded); xd[p] = x
            xh = np.zeros(structs[0].n_rows_padded); xh[structs[0].arrays()["old_to_new_idx"]] = x
            if kind == "sp_hp":
                xd, xh = xd.astype(np.float32), xh.astype(np.float32)
            host_hand = [pkg.DeviceMatrix(s) if s is not None else None for s in structs]
            y_dev = _y(pkg, t, kind, hand, xd)[p]
            y_host = _y(pkg, t, kind, host_hand, xh)[structs[0].arrays()["old_to_new_idx"]]
            assert np.array_equal(bits(y_dev), bits(y_host)), (name, C, sigma)


def test_nan_is_refused_by_the_two_part_kinds_and_lands_in_hp_of_the_three_part_kind(pkg, t, mats):
    m = dict(mats)["impcol_e"]
    I, J, V = (np.array(a) for a in m.arrays())
    V = V.copy()
    first = 1100
    V[first] = np.nan; V[first + 77] = -np.nan; V[5] = 0.25
    dev = tuple(t.from_numpy(a).cuda() for a in (I, J, V))
    good = dev_coo(t, m)
    for kind in ("dp_sp", "dp_hp", "sp_hp"):
        for call in (lambda: pkg.partition_precisions_device(*dev, m.n_rows, m.n_cols, kind, 1.0),
                     lambda: pkg.convert_ap_device_from_arrays(*dev, m.n_rows, m.n_cols, 32, 64, kind, 1.0)):
            with pytest.raises(pkg.UspmvError, match=f"element {first} fits neither struct") as e:
                call()
            assert e.value.status == 1
        same_parts(pkg, t, m, kind, 1.0, 0.0, good)                               # a following valid call works
    bad = pkg.Coo.from_arrays(m.n_rows, m.n_cols, I, J, V)
    _, got = same_parts(pkg, t, bad, "dp_sp_hp", 1.0, 0.1, dev)
    hp_v = got[2][2].cpu().numpy()
    nan_bits = np.array([np.nan, -np.nan]).astype(np.float16).astype(np.float64).view(np.uint64)
    assert np.array_equal(hp_v[np.isnan(hp_v)].view(np.uint64), nan_bits)
    parts = host_parts(pkg, bad, "dp_sp_hp", 1.0, 0.1)
    structs = host_structs(pkg, parts, "dp_sp_hp", 32, 64)
    _, hand, _, _, _ = pkg.convert_ap_device_from_arrays(*dev, m.n_rows, m.n_cols, 32, 64, "dp_sp_hp", 1.0, 0.1)
    same_handles(pkg, structs, hand, "nan in hp")


def test_bad_indices_are_refused_before_anything_is_built(pkg, t):
    n = 40
    I0 = np.repeat(np.arange(n, dtype=np.int32), 3); J0 = (np.arange(I0.size, dtype=np.int32) * 7) % n
    V = t.from_numpy(np.linspace(0.01, 3.0, I0.size)).cuda()
    cases = []
    for what, pos, val, text, status in (("I", 0, -1, "row index", 1), ("I", 50, -7, "row index", 1), ("I", I0.size - 1, n, "row index", 1),
                                         ("I", 60, 5, "sorted by row", 3), ("J", 3, -1, "column index", 1), ("J", 100, n, "column index", 1),
                                         ("J", I0.size - 1, 1 << 30, "column index", 1)):
        I, J = I0.copy(), J0.copy()
        (I if what == "I" else J)[pos] = val
        cases.append((t.from_numpy(I).cuda(), t.from_numpy(J).cuda(), text, status))
    for kind in KINDS:
        for dI, dJ, text, status in cases:
            for call in (lambda: pkg.partition_precisions_device(dI, dJ, V, n, n, kind, 1.0, 0.1),
                         lambda: pkg.convert_ap_device_from_arrays(dI, dJ, V, n, n, 8, 16, kind, 1.0, 0.1)):
                with pytest.raises(pkg.UspmvError, match=text) as e:
                    call()
                assert e.value.status == status, (kind, text)
    dI, dJ = t.from_numpy(I0).cuda(), t.from_numpy(J0).cuda()
    with pytest.raises(pkg.UspmvError, match="8192"):
        big = t.arange(20000, dtype=t.int32, device="cuda")
        pkg.convert_ap_device_from_arrays(big, big, t.ones(20000, dtype=t.float64, device="cuda"), 20000, 20000, 32, 16384, "dp_sp", 1.0,
                                          sort=pkg.SORT_DEVICE_STABLE)
    lay, hand, _, _, cnt = pkg.convert_ap_device_from_arrays(dI, dJ, V, n, n, 8, 16, "dp_sp_hp", 1.0, 0.1)      # a following valid call works
    assert sum(cnt) == I0.size and all(h is not None for h in hand)


def test_padded_slot_refusal(pkg, t):
    """17 rows, C = 8, sigma = 32: the last three rows have no dp entry, and the unstable sort of the dp part's counts sends them behind
    n_rows (positions 23, 22, 21), where their sp entries would overrun a chunk of length 0 -- found with the host route, which refuses;
    the device route refuses with the same text, and takes the matrix once the ordering is the stable one."""
    c = PAD_REFUSED
    n = c["n"]
    I = np.arange(n); J = np.zeros(n, np.int64); V = np.where(I < n - c["sp_only"], 2.0, 0.25)
    m = pkg.Coo.from_arrays(n, n, I, J, V)
    dp, sp = pkg.partition_precisions(m, 1.0)
    perm = pkg.convert_to_scs(dp, c["C"], c["sigma"], pkg.F64).arrays()["old_to_new_idx"].copy()
    assert perm.max() >= n
    with pytest.raises(pkg.UspmvError, match="fixed_permutation maps a non-empty row onto a padded slot") as host:
        pkg.convert_to_scs(sp, c["C"], c["sigma"], pkg.F32, fixed_permutation=perm)
    dev = dev_coo(t, m)
    for kind in KINDS:
        with pytest.raises(pkg.UspmvError, match="fixed_permutation maps a non-empty row onto a padded slot") as e:
            pkg.convert_ap_device_from_arrays(*dev, n, n, c["C"], c["sigma"], kind, 1.0, 0.1)
        assert e.value.status == host.value.status
        assert str(e.value).split("fixed_permutation", 1)[1] == str(host.value).split("fixed_permutation", 1)[1]
        _, hand, _, _, cnt = pkg.convert_ap_device_from_arrays(*dev, n, n, c["C"], c["sigma"], kind, 1.0, 0.1, sort=pkg.SORT_DEVICE_STABLE)
        assert cnt[0] == n - c["sp_only"] and sum(cnt) == n


def test_f16_in_the_plain_conversion(pkg, t, mats):
    for name in ("impcol_e", "ragged300", "stencil_decades"):
        m = dict(mats)[name]
        dI, dJ, dV = dev_coo(t, m)
        for C, sigma in ((32, 512), (5, 7), (1, 1)):
            for permute in (True, False):
                s = pkg.convert_to_scs(m, C, sigma, pkg.F16)
                if permute:
                    pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"])
                lay, A, o2n, _ = pkg.convert_to_scs_device_from_arrays(dI, dJ, dV, m.n_rows, m.n_cols, C, sigma, pkg.F16, permute_cols=permute)
                assert lay.dtype == pkg.F16 and A.dtype == pkg.F16
                same_handles(pkg, [s], [A], (name, C, sigma, permute))
                assert np.array_equal(o2n.cpu().numpy(), s.arrays()["old_to_new_idx"])
    v = t.from_numpy(SPECIAL).cuda()                      # one rounding, overflow, subnormals: the scatter kernel's own conversion
    k = t.arange(SPECIAL.size, dtype=t.int32, device="cuda")
    m = pkg.Coo.from_arrays(SPECIAL.size, SPECIAL.size, np.arange(SPECIAL.size), np.arange(SPECIAL.size), SPECIAL)
    _, A, _, _ = pkg.convert_to_scs_device_from_arrays(k, k, v, SPECIAL.size, SPECIAL.size, 4, 1, pkg.F16)
    same_handles(pkg, [pkg.convert_to_scs(m, 4, 1, pkg.F16)], [A], "special")


def test_no_device_memory_is_lost(pkg, t, mats):
    m = dict(mats)["random2000"]
    dev = dev_coo(t, m)
    I, J, V = (np.array(a) for a in m.arrays())
    V = V.copy(); V[1234] = np.nan
    nan_dev = (dev[0], dev[1], t.from_numpy(V).cuda())
    n_pad = -(-m.n_rows // 32) * 32
    x = t.ones(n_pad, dtype=t.float64, device="cuda"); y = t.zeros_like(x)

    def cycle():
        for kind in ("dp_sp", "dp_sp_hp"):
            lay, hand, o2n, n2o, _ = pkg.convert_ap_device_from_arrays(*dev, m.n_rows, m.n_cols, 32, 512, kind, 1e-1, 1e-3)
            _plan(pkg, kind, hand)
            if kind == "dp_sp":
                pkg.spmv_ap(hand[0], hand[2], x, y)
            else:
                pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y)
            assert hand[0].n_rows_padded == n_pad
            del lay, hand, o2n, n2o
            parts = pkg.partition_precisions_device(*dev, m.n_rows, m.n_cols, kind, 1e-1, 1e-3)
            del parts
        with pytest.raises(pkg.UspmvError):               # a refused call releases what it had built
            pkg.convert_ap_device_from_arrays(*nan_dev, m.n_rows, m.n_cols, 32, 512, "dp_sp", 1e-1)
        gc.collect()
        t.cuda.synchronize()
        t.cuda.empty_cache()

    cycle()
    free0, _ = t.cuda.mem_get_info()
    for _ in range(20):
        cycle()
    free1, _ = t.cuda.mem_get_info()
    assert free0 - free1 <= 2 << 20, f"{(free0 - free1) / 2**20:.1f} MiB of device memory lost over twenty rounds"
