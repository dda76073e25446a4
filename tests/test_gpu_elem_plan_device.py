"""The tile-local-column plan over single x ELEMENTS built on the device (uspmv_dmat_optimize_device: plan_count_elems / plan_write_elems of
csrc/plan_kernels.hip, the policy of csrc/tlc_planner.hip elements_take_over): equal to the host planner's element plan array for array, on
handles that never had a host struct as well, and a fallback only -- caps, gates, line budgets and ap pairs keep what they had."""
import numpy as np
import pytest

from conftest import make_x

pytestmark = pytest.mark.gpu

PLAN_KEYS = ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16")


@pytest.fixture(scope="module")
def t(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch


def scrambled_columns(pkg, g, dof, K, seed=3, rows_too=False):
    """27-point x dof stencil on g^3 nodes with the COLUMNS' nodes renumbered at random inside consecutive blocks of K nodes (rows keep their order
    unless rows_too: then the permutation is symmetric)."""
    base = pkg.gen_stencil27(g, g, g, dof=dof)
    I, J, V = (np.array(a) for a in base.arrays())
    n = base.n_rows
    nn = n // dof
    rng = np.random.default_rng(seed)
    p = np.arange(nn, dtype=np.int64)
    for s0 in range(0, nn, K):
        seg = p[s0:s0 + K].copy(); rng.shuffle(seg); p[s0:s0 + K] = seg
    J2 = (p[J // dof] * dof + J % dof).astype(np.int32)
    I2 = (p[I // dof] * dof + I % dof).astype(np.int32) if rows_too else I
    o = np.lexsort((J2, I2))
    return pkg.Coo.from_arrays(n, n, I2[o], J2[o], V[o])


@pytest.fixture(scope="module")
def scattered(pkg):
    return scrambled_columns(pkg, 40, 3, 8000)       # <= 1 512 distinct columns per 256-row tile, in up to 13 windows of 4 096


@pytest.fixture(scope="module")
def scattered_wide(pkg):
    return scrambled_columns(pkg, 48, 3, 30000)      # <= 1 656 distinct columns per tile, in a median of 22 windows: no bitmap holds them


def _struct(pkg, orc, m, C, sigma, dt):
    """(struct, arrays, x, oracle y) in the struct's own column numbering (no column permutation, as tests/test_gpu_elem_plan.py)"""
    s = pkg.convert_to_scs(m, C, sigma, pkg.F64 if dt == "f64" else pkg.F32)
    a = s.arrays()
    x = np.zeros(max(s.n_rows_padded, s.n_cols), a["values"].dtype)
    x[:s.n_cols] = make_x(s.n_cols).astype(a["values"].dtype)
    want = orc.spmv_scs(C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], x)
    return s, a, x, want


def _y(pkg, t, A, s, x):
    dx = t.from_numpy(x).cuda()
    dy = t.full((s.n_rows_padded,), -3.0, dtype=dx.dtype, device="cuda")
    pkg.spmv(A, dx, dy)
    return dy.cpu().numpy()


def _host_and_device(pkg, s):
    Ah = pkg.DeviceMatrix(s); Ah.optimize(s)
    Ad = pkg.DeviceMatrix(s); Ad.optimize_device()
    return Ah, Ad


def _assert_equal_element_plans(pkg, t, Ah, Ad, s, x, want, tag):
    assert Ah.plan_granularity() == 1 and Ad.plan_granularity() == 1, (tag, Ah.plan_granularity(), Ad.plan_granularity())
    assert (Ad.tlc_tiles, Ad.tlc_staged) == (Ah.tlc_tiles, Ah.tlc_staged), tag
    assert Ad.index_bits() == Ah.index_bits(), tag
    ph, pd = Ah.plan_download(), Ad.plan_download()
    assert ph is not None and pd is not None, tag
    for k in PLAN_KEYS:
        assert np.array_equal(ph[k], pd[k]), (tag, k)
    assert ph["max_lines_used"] == pd["max_lines_used"], tag
    for H in (Ah, Ad):
        assert np.array_equal(_y(pkg, t, H, s, x)[:s.n_rows_padded], want[:s.n_rows_padded]), tag
    ids = t.tensor([1, 3, 0], dtype=t.int32, device="cuda")
    dx = t.from_numpy(x).cuda()
    assert Ad.tlc_tiles >= 4 and Ad.tile_rows == Ah.tile_rows == 256
    for H in (Ah, Ad):
        dy = t.full((s.n_rows_padded,), -3.0, dtype=dx.dtype, device="cuda")
        pkg.spmv_tiles(H, ids, dx, dy)
        got = dy.cpu().numpy()
        R = H.tile_rows
        for tile in (0, 1, 3):
            assert np.array_equal(got[tile * R:(tile + 1) * R], want[tile * R:(tile + 1) * R]), (tag, tile)
        assert np.all(got[2 * R:3 * R] == -3.0) and np.all(got[4 * R:] == -3.0), tag
    return ph


@pytest.mark.parametrize("C,sigma,dt", [(32, 512, "f64"), (32, 1, "f32"), (64, 128, "f64")])
def test_device_element_plan_equals_the_host_plan(pkg, orc, t, scattered, C, sigma, dt):
    s, a, x, want = _struct(pkg, orc, scattered, C, sigma, dt)
    Ah, Ad = _host_and_device(pkg, s)
    _assert_equal_element_plans(pkg, t, Ah, Ad, s, x, want, (C, sigma, dt))


def test_device_element_plan_on_the_rechunked_path(pkg, orc, t, scattered):
    """C = 16: both planners run on an internal C = 32 re-chunking (the device one builds it on the device) and reach the element plan there"""
    s, a, x, want = _struct(pkg, orc, scattered, 16, 64, "f64")
    Ah, Ad = _host_and_device(pkg, s)
    assert Ad.plan_info() == Ah.plan_info()
    assert Ah.plan_granularity() == 1 and Ad.plan_granularity() == 1
    assert (Ad.tlc_tiles, Ad.tlc_staged) == (Ah.tlc_tiles, Ah.tlc_staged)
    for H in (Ah, Ad):
        assert np.array_equal(_y(pkg, t, H, s, x)[:s.n_rows_padded], want[:s.n_rows_padded])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_tiles_no_window_bitmap_can_hold(pkg, orc, t, scattered_wide, dt):
    s, a, x, want = _struct(pkg, orc, scattered_wide, 32, 512, dt)
    Ah, Ad = _host_and_device(pkg, s)
    ph = Ah.plan_download()
    assert Ah.plan_granularity() == 1 and ph is not None
    lp, tl = ph["tile_line_ptr"], ph["tile_lines"]
    windows = np.array([len(np.unique(tl[lp[k]:lp[k + 1]] >> 12)) for k in range(len(lp) - 1)])
    assert np.count_nonzero(windows > 16) * 2 >= len(windows), (np.count_nonzero(windows > 16), len(windows))   # (precondition on the input)
    _assert_equal_element_plans(pkg, t, Ah, Ad, s, x, want, ("wide", dt))


def test_handles_that_never_had_a_host_struct(pkg, orc, t, scattered):
    m = scattered
    lay, A = pkg.convert_to_scs_device(m, 32, 512, pkg.F64)
    nt, ns = A.optimize_device()
    assert A.plan_granularity() == 1 and nt > 0 and ns == nt, (A.plan_granularity(), nt, ns)
    s = pkg.convert_to_scs(m, 32, 512, pkg.F64)                 # the same conversion on the host: columns permuted, x permuted
    a = s.arrays(); pkg.permute_scs_cols(s, a["old_to_new_idx"]); a = s.arrays()
    xp = np.zeros(s.n_rows_padded)
    xp[:s.n_rows] = pkg.apply_permutation(make_x(s.n_rows), a["new_to_old_idx"])
    want = orc.spmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
    got = _y(pkg, t, A, s, xp)
    assert np.array_equal(got, want)
    # ... and in the caller's row order
    assert np.array_equal(pkg.apply_permutation(got[:s.n_rows].copy(), a["old_to_new_idx"]), pkg.apply_permutation(want[:s.n_rows].copy(), a["old_to_new_idx"]))


def test_raw_arrays_through_the_plan_cache(pkg, orc, t, scattered):
    s, a, x, want = _struct(pkg, orc, scattered, 32, 512, "f64")
    A = pkg.DeviceMatrix(s)          # torch-owned device arrays = what a host application would pass
    dx = t.from_numpy(x).cuda()
    try:
        pkg.set_tuning(raw_plan_cache=1)
        for rep in range(2):
            dy = t.full((s.n_rows_padded,), -5.0, dtype=t.float64, device="cuda")
            pkg.uspmv_scs_gpu(s.C, s.n_chunks, A.chunk_ptrs, A.chunk_lengths, A.col_idxs, A.values, dx, dy)
            assert np.array_equal(dy.cpu().numpy(), want[:s.n_rows_padded]), rep
    finally:
        pkg.set_tuning(raw_plan_cache=0)
        pkg.lib().uspmv_raw_plan_cache_clear()


@pytest.mark.parametrize("C,sigma,dt,most", [(32, 1, "f32", 16384), (32, 512, "f64", 8192)])
def test_large_caps(pkg, orc, t, scattered, C, sigma, dt, most):
    """tlc_elem_cap 16384: float takes it whole, double is clipped to 8 192 (64 KiB of the value type); the count pass then runs on its largest set"""
    s, a, x, want = _struct(pkg, orc, scattered, C, sigma, dt)
    pkg.set_tuning(tlc_elem_cap=16384, tlc_elem=2)
    try:
        Ah, Ad = _host_and_device(pkg, s)
    finally:
        pkg.set_tuning(tlc_elem_cap=4096, tlc_elem=1)
    ph = _assert_equal_element_plans(pkg, t, Ah, Ad, s, x, want, ("cap", dt))
    assert ph["max_lines_used"] <= most


def test_the_fallback_stays_a_fallback(pkg, orc, t, scattered):
    s, a, x, want = _struct(pkg, orc, scattered, 32, 512, "f64")
    pkg.set_tuning(tlc_elem_cap=1100)                         # the tiles list more elements than that: the other plans answer
    try:
        A = pkg.DeviceMatrix(s); A.optimize_device()
    finally:
        pkg.set_tuning(tlc_elem_cap=4096)
    assert A.plan_granularity() != 1
    assert np.array_equal(_y(pkg, t, A, s, x)[:s.n_rows_padded], want[:s.n_rows_padded])
    pkg.set_tuning(tlc_elem=0)
    try:
        A = pkg.DeviceMatrix(s); A.optimize_device()
    finally:
        pkg.set_tuning(tlc_elem=1)
    assert A.plan_granularity() != 1
    A = pkg.DeviceMatrix(s); A.optimize_device(max_lines=40)   # a caller with a line budget of its own keeps the line plan
    assert A.plan_granularity() != 1


def test_regular_numbering_keeps_the_line_plan_unless_forced(pkg, orc, t):
    s = pkg.convert_to_scs(pkg.gen_stencil27(16, 16, 16, dof=3), 32, 512, pkg.F64)
    a = s.arrays(); pkg.permute_scs_cols(s, a["old_to_new_idx"]); a = s.arrays()
    A = pkg.DeviceMatrix(s); A.optimize_device()
    assert A.plan_granularity() == 16 and A.tlc_staged == A.tlc_tiles
    pkg.set_tuning(tlc_elem=2)
    try:
        Ah, Ad = _host_and_device(pkg, s)
    finally:
        pkg.set_tuning(tlc_elem=1)
    assert Ah.plan_granularity() == 1 and Ad.plan_granularity() == 1
    assert (Ad.tlc_tiles, Ad.tlc_staged) == (Ah.tlc_tiles, Ah.tlc_staged)
    ph, pd = Ah.plan_download(), Ad.plan_download()
    for k in PLAN_KEYS:
        assert np.array_equal(ph[k], pd[k]), k
    assert ph["max_lines_used"] == pd["max_lines_used"]
    x = np.zeros(s.n_rows_padded); x[:s.n_rows] = make_x(s.n_rows)
    want = orc.spmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], x)
    for H in (A, Ad):
        assert np.array_equal(_y(pkg, t, H, s, x), want)


def test_ap_pair_keeps_lines_then_sweep(pkg, orc, t, scattered):
    dp, sp = pkg.partition_precisions(scattered, 0.5)
    assert dp.nnz > 0 and sp.nnz > 0
    ds = pkg.convert_to_scs(dp, 32, 512, pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, 32, 512, pkg.F32, fixed_permutation=perm)
    da, sa = ds.arrays(), ss.arrays()
    Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
    pkg.optimize_device_ap(Ad, As)
    assert Ad.plan_granularity() != 1 and As.plan_granularity() != 1
    x = np.zeros(max(ds.n_rows_padded, ds.n_cols)); x[:ds.n_cols] = make_x(ds.n_cols)
    y = t.full((ds.n_rows_padded,), -3.0, dtype=t.float64, device="cuda")
    pkg.spmv_ap(Ad, As, t.from_numpy(x).cuda(), y)
    want = orc.spmv_scs_ap_adv(32, ds.n_chunks, (da["chunk_ptrs"], da["chunk_lengths"], da["col_idxs"], da["values"]),
                               (sa["chunk_ptrs"], sa["chunk_lengths"], sa["col_idxs"], sa["values"]), x)
    assert np.array_equal(y.cpu().numpy(), want)


def test_no_device_memory_is_lost_over_replanning(pkg, t, scattered):
    import gc
    s = pkg.convert_to_scs(scattered, 32, 512, pkg.F64)
    A = pkg.DeviceMatrix(s)

    def round_():
        A.optimize_device()
        assert A.plan_granularity() == 1
        pkg.set_tuning(tlc_elem=0)
        try:
            A.optimize_device()
        finally:
            pkg.set_tuning(tlc_elem=1)
        assert A.plan_granularity() != 1
        gc.collect(); t.cuda.synchronize()

    round_()
    free0, _ = t.cuda.mem_get_info()
    for _ in range(5):
        round_()
    free1, _ = t.cuda.mem_get_info()
    assert free0 - free1 == 0, f"{(free0 - free1) / 2**20:.2f} MiB of device memory lost over five re-planning rounds"
