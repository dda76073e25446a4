"""The phased SpMMV kernel scs_spmmv_quadph (csrc/spmmv_phased.hip; 64-byte X rows: dp b = 8, sp b = 16) on the arms and tuning keys that no
other file runs: the plan over original X-row numbering behind the permuting re-layout ("spmmv_unscramble", xmode 3), a handle planned
again without its optional (unscrambled / line) plan, non-temporal
column-major stores ("spmmv_ycol_nt") in every X mode and in the streamed kernels, 512-row phases ("spmmv_phase_rows": two-byte indices, the
MAXP = 8 instantiation with 32 KB of LDS), no phased plan at all ("spmmv_phased" 0: kernel 6 answers), the brick row order ("spmmv_reorder" 3),
the line-staged form (XM = 2) where the last line of a column crosses the leading dimension, and the block remap of remap_block
(uspmv_device.hpp) with small groups and a stagger, on grids with full super-blocks and a remainder.

Reference: the oracle's spmmv_scs / spmv_scs on the host struct's arrays (same slot order, fused multiply-add).  The contract is bit
equality; there is no tolerance in this file.  Y is filled with a sentinel before every product and carries a guard zone behind its end; in
column-major Y with ld > n_rows_padded the rows between the columns must keep the sentinel.

Every case first NAMES the arm that answered -- DeviceMatrix.spmmv_last_path() and block_plan_info() -- and only then compares bits, so a handle
that lost its plan (the launcher then falls through to kernel 6, 4 or 3, with the same bits) fails here.  Nothing is skipped.

Tuning is process-global: tuning() reads every key it is about to set (the library defaults of BASE, which pin the arm, and the case's own)
and puts the values back in `finally`.

The shape facts (phases per tile, rows per phase, which line plans the planner keeps) come from the host planner
(tests/helpers/block_plan_check.cpp checks the same planner forms on the CPU) and are re-asserted here through block_plan_info()."""
import contextlib

import numpy as np
import pytest

from conftest import make_x

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7.0, 64
# library defaults of every key that decides which SpMMV / SpMV arm runs (csrc/uspmv_device.hpp, struct Tuning)
BASE = dict(nontemporal=1, xcd_remap=256, xcd_stagger=0, ablate=0, tlc=1, sweep=1, sweep_remap=8, tlc_tile_rows=0, spmmv_variant=0, spmmv_unroll=0,
            spmmv_lds_kb=0, spmmv_tile_rows=0, spmmv_reorder=4, spmmv_brick_stride=0, spmmv_brick_lines=4, spmmv_phase_dp=24, spmmv_stream=0,
            spmmv_stream_waves=4, spmmv_stream_xcd=1, spmmv_stream_depth=1, spmmv_phased=1, spmmv_phase_rows=256, spmmv_xcol=0, spmmv_ycol_nt=0,
            spmmv_xline=0, spmmv_unscramble=0, spmmv_idx8=1, spmmv_list_plan=0, block_plan_device=1)
# name: (generator, its arguments, keywords, C, sigma)
SHAPES = {
    "band11": ("gen_banded_random", (1000, 11, 900), {}, 32, 1),          # 16 tiles, every chunk L = 11: two full groups and a tail of 3
    "mesh3": ("gen_stencil27", (12, 11, 10), dict(dof=3), 32, 512),       # L from 36 to 81, partial last groups, up to 6 phases per tile
    "mesh3-s1": ("gen_stencil27", (12, 11, 10), dict(dof=3), 32, 1),      # sigma = 1: no permutation; the dp line plan is kept
    "mesh2": ("gen_stencil27", (9, 30, 11), dict(dof=2), 64, 128),        # C = 64
    "band40": ("gen_banded_random", (3000, 40, 1500), {}, 32, 512),       # 47 tiles, 10 phases per tile
    "thin3-s1": ("gen_stencil27", (5, 5, 40), dict(dof=3), 32, 1),        # sigma = 1, thin mesh: the sp line plan (32 rows per line) is kept too
    "stencil1": ("gen_stencil27", (24, 20, 18), {}, 32, 512),
}
DTYPES = ("f64", "f32")


@pytest.fixture(scope="module")
def t(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


@contextlib.contextmanager
def tuning(pkg, **kw):
    keys = dict(BASE, **kw)
    old = {k: pkg.get_tuning(k) for k in keys}
    try:
        pkg.set_tuning(**keys)
        yield
    finally:
        pkg.set_tuning(**old)


class Case:
    """One struct, its permuted x and the oracle's products of the block vectors built from it (computed once, read-only)."""

    def __init__(self, pkg, orc, m, C, sigma, dt):
        self.pkg, self.orc, self.C = pkg, orc, C
        self.dtype = pkg.F64 if dt == "f64" else pkg.F32
        self.b = 8 if dt == "f64" else 16
        s = pkg.convert_to_scs(m, C, sigma, self.dtype)
        a = s.arrays(); pkg.permute_scs_cols(s, a["old_to_new_idx"]); a = s.arrays()
        self.s, self.a, self.n = s, a, s.n_rows_padded
        self.uint = np.uint64 if dt == "f64" else np.uint32
        xp = np.zeros(max(s.n_rows_padded, m.n_cols), a["values"].dtype)
        xp[:s.n_rows] = pkg.apply_permutation(make_x(s.n_rows).astype(xp.dtype), a["new_to_old_idx"])
        xp[s.n_rows:m.n_cols] = make_x(m.n_cols - s.n_rows).astype(xp.dtype) * xp.dtype.type(0.5)      # (rectangular: columns beyond the rows)
        self.xp = xp
        self._ref = {}

    def lds(self):
        return (self.n, self.n + 24)

    def block(self, ld, rowwise):
        """X like block() of tests/test_gpu_spmmv_stream.py: column v = xp * (1 + v/8)"""
        xp, b = self.xp, self.b
        X = np.zeros(b * ld, xp.dtype)
        for v in range(b):
            col = xp * xp.dtype.type(1.0 + v / 8.0)
            if rowwise:
                X[v::b] = col
            else:
                X[v * ld:v * ld + xp.size] = col
        return X

    def oracle(self, X, ld, rowwise):
        a = self.a
        Yo = self.orc.spmmv_scs(self.C, self.s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, self.b, ld, rowwise)
        Yo.setflags(write=False)
        return Yo

    def ref(self, ld, rowwise):
        if (ld, rowwise) not in self._ref:
            X = self.block(ld, rowwise)
            X.setflags(write=False)
            self._ref[(ld, rowwise)] = (X, self.oracle(X, ld, rowwise))
        return self._ref[(ld, rowwise)]


@pytest.fixture(scope="module")
def cases(pkg, orc, t):
    mats, cache = {}, {}

    def get(name, dt):
        gen, args, kw, C, sigma = SHAPES[name]
        if (gen, args) not in mats:
            mats[(gen, args)] = getattr(pkg, gen)(*args, **kw)
        if (name, dt) not in cache:
            cache[(name, dt)] = Case(pkg, orc, mats[(gen, args)], C, sigma, dt)
        return cache[(name, dt)]
    return get


def product(t, K, A, dX, ld, rowwise):
    """one uspmv_spmmv into a sentinel-filled Y with a guard zone; returns (Y on the host, (kernel, x_pass))"""
    dY = t.full((K.b * ld + GUARD,), SENTINEL, dtype=dX.dtype, device="cuda")
    K.pkg.spmmv(A, dX, dY, K.b, ld, K.pkg.ROWWISE if rowwise else K.pkg.COLWISE)
    t.cuda.synchronize()
    return dY.cpu().numpy(), A.spmmv_last_path()


def same_bits(K, got, Yo, ld, rowwise, tag, nan_ok=False):
    """the n_rows_padded rows of every column bit for bit; every other element of Y still the sentinel"""
    n, b = K.n, K.b
    assert np.all(got[b * ld:] == SENTINEL), tag
    if rowwise:
        g, o = got[:n * b], Yo[:n * b]
        assert np.all(got[n * b:b * ld] == SENTINEL), tag
    else:
        g, o = got[:b * ld].reshape(b, ld)[:, :n], Yo.reshape(b, ld)[:, :n]
        assert np.all(got[:b * ld].reshape(b, ld)[:, n:] == SENTINEL), tag      # guard rows between the columns
    g, o = np.ascontiguousarray(g), np.ascontiguousarray(o)
    if nan_ok:
        assert np.array_equal(np.isnan(g), np.isnan(o)), tag
        keep = ~np.isnan(o)
        assert np.array_equal(g[keep].view(K.uint), o[keep].view(K.uint)), tag
    else:
        assert not np.isnan(o).any(), tag
        bad = np.flatnonzero(g.view(K.uint).ravel() != o.view(K.uint).ravel())
        assert bad.size == 0, tag + (bad.size, bad[:8].tolist())


def run(t, K, A, rowwise, ld, expect, tag, dX=None):
    """the product of the case's X; asserts the arm that answered FIRST, then the bits"""
    X, Yo = K.ref(ld, rowwise)
    if dX is None:
        dX = t.from_numpy(np.array(X)).cuda()              # (a writable copy: the cached X is read-only)
    got, path = product(t, K, A, dX, ld, rowwise)
    assert path == expect, tag + (path, expect)
    same_bits(K, got, Yo, ld, rowwise, tag)
    return dX


def run_all(t, K, A, row_path, col_path, tag):
    run(t, K, A, True, K.n, row_path, tag + ("rowwise",))
    for ld in K.lds():
        run(t, K, A, False, ld, col_path, tag + ("colwise", ld))


# ------------------------------------------------------------------------------------------------ 1. the default kernel is kernel 8
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["band11", "mesh3", "mesh3-s1", "mesh2", "band40"])
def test_default_handles_run_the_phased_kernel(pkg, t, cases, name, dt):
    K = cases(name, dt)
    with tuning(pkg):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert A.spmmv_last_path() == (0, 0)
        assert info["phased_plan"] == 1 and info["idx8"] == 1 and 0 < info["max_rows"] <= 256 and info["device_built"] == 0, info
        assert info["tiles"] == (K.n + 63) // 64 and info["phases"] >= info["tiles"], info
        run_all(t, K, A, (8, 0), (8, 1), (name, dt, "host plan"))
        D = pkg.DeviceMatrix(K.s)
        D.optimize_block_device(K.b)
        dinfo = D.block_plan_info()
        assert dinfo["phased_plan"] == 1 and dinfo["idx8"] == 1 and dinfo["device_built"] == 1 and dinfo["tiles"] == info["tiles"], dinfo
        run_all(t, K, D, (8, 0), (8, 1), (name, dt, "device plan"))
    with tuning(pkg, spmmv_idx8=0):                      # two-byte indices on 256-row phases: still kernel 8
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 1 and info["idx8"] == 0 and info["max_rows"] <= 256, info
        run_all(t, K, A, (8, 0), (8, 1), (name, dt, "idx8=0"))


# ------------------------------------------------------------------------------------------------ 2. spmmv_unscramble
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["mesh3", "mesh2", "band40"])
def test_unscrambled_plan_behind_the_permuting_relayout(pkg, t, cases, name, dt):
    K = cases(name, dt)
    with tuning(pkg, spmmv_unscramble=1):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 1 and info["idx8"] == 1, info
        for ld in K.lds():
            tag = (name, dt, ld)
            dX = run(t, K, A, False, ld, (8, 3), tag + ("fresh",))
            pkg.spmmv_x_prepared(A, dX, K.b, ld)
            for rep in range(3):
                run(t, K, A, False, ld, (8, 2), tag + ("prepared", rep), dX=dX)
            run(t, K, A, True, K.n, (8, 0), tag + ("rowwise between",))        # (row-major X never goes through the workspace)
            run(t, K, A, False, ld, (8, 2), tag + ("prepared after rowwise",), dX=dX)
            pkg.spmmv_x_release(A)
            run(t, K, A, False, ld, (8, 3), tag + ("released",), dX=dX)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("why,name,tune,device", [("sigma 1", "mesh3-s1", {}, False), ("device-built plan", "mesh3", {}, True),
                                                   ("idx8 0", "mesh3", dict(spmmv_idx8=0), False), ("512-row phases", "mesh3", dict(spmmv_phase_rows=512), False)])
def test_unscrambled_plan_is_absent_where_it_cannot_be_built(pkg, t, cases, why, name, tune, device, dt):
    """no permutation (sigma = 1), no permutation KNOWN (plan from the device arrays), or phases / indices the xmode 3 launch is not compiled
    for: the plain re-layout and the plain plan answer, x_pass 1"""
    K = cases(name, dt)
    with tuning(pkg, spmmv_unscramble=1, **tune):
        if device:
            A = pkg.DeviceMatrix(K.s)
            A.optimize_block_device(K.b)
        else:
            A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 1 and info["device_built"] == int(device), info
        run_all(t, K, A, (8, 0), (8, 1), (why, name, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_unscrambled_plan_special_values(pkg, t, cases, dt):
    """+-Inf, NaN and -0.0 scattered in X; then one NaN alone at permuted position 0, the column every padding entry multiplies (0 * NaN
    reaches every row of a chunk that is padded, as in the reference)"""
    K = cases("mesh3", dt)
    ld = K.n + 24
    rng = np.random.default_rng(11)
    Xs = K.block(ld, False)
    live = np.concatenate([v * ld + np.arange(K.s.n_rows) for v in range(K.b)])
    sp = rng.choice(live, 200, replace=False)
    Xs[sp[:50]] = np.inf; Xs[sp[50:100]] = -np.inf; Xs[sp[100:150]] = np.nan; Xs[sp[150:]] = -0.0
    X0 = K.block(ld, False)
    X0[0] = np.nan                                      # column 0 of the block vector, permuted row 0
    with tuning(pkg, spmmv_unscramble=1):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        for what, X in (("scattered", Xs), ("NaN at 0", X0)):
            Yo = K.oracle(X, ld, False)
            assert np.isnan(Yo).any() and not np.isnan(Yo).all()
            got, path = product(t, K, A, t.from_numpy(X).cuda(), ld, False)
            assert path == (8, 3), (what, dt, path)
            same_bits(K, got, Yo, ld, False, (what, dt), nan_ok=True)


@pytest.mark.parametrize("name,dt,key,col_path", [("mesh3", "f64", "spmmv_unscramble", (8, 3)), ("mesh3", "f32", "spmmv_unscramble", (8, 3)),
                                                  ("mesh3-s1", "f64", "spmmv_xline", (8, 0))])
def test_replanning_a_handle_drops_the_optional_plans(pkg, t, cases, name, dt, key, col_path):
    """a handle that carries the unscrambled or the line plan is planned again without the key: the second uspmv_dmat_optimize_block must
    release the optional plan with everything else (block_plan_reset, the one release path of the plans' phase lists), so that the key set
    again at LAUNCH time finds no such plan and the plain re-layout over the new phased plan answers"""
    K = cases(name, dt)
    A = pkg.DeviceMatrix(K.s)
    with tuning(pkg, **{key: 1}):
        A.optimize_block(K.s, K.b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 1 and info["line_plan"] == int(key == "spmmv_xline"), info
        run_all(t, K, A, (8, 0), col_path, (name, dt, key, "first plan"))
    with tuning(pkg):
        A.optimize_block(K.s, K.b)
    with tuning(pkg, **{key: 1}):
        info = A.block_plan_info()
        assert info["phased_plan"] == 1 and info["line_plan"] == 0 and info["line_phases"] == 0, info
        run_all(t, K, A, (8, 0), (8, 1), (name, dt, key, "planned again"))


# ------------------------------------------------------------------------------------------------ 3. spmmv_ycol_nt
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("dt", DTYPES)
def test_nontemporal_column_major_stores(pkg, t, cases, dt, nt):
    """"spmmv_ycol_nt" 1 over column-major Y in every X mode of the phased kernel and in the streamed kernels, with and without
    "nontemporal" (without it the plain-store instantiation must answer and the key change nothing)"""
    K = cases("mesh3", dt)
    with tuning(pkg, spmmv_ycol_nt=1, nontemporal=nt):                              # re-layout pass, X mode 0
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        assert A.block_plan_info()["phased_plan"] == 1
        run_all(t, K, A, (8, 0), (8, 1), ("relayout", dt, nt))
    with tuning(pkg, spmmv_ycol_nt=1, nontemporal=nt, spmmv_unscramble=1):          # X mode 3
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        run_all(t, K, A, (8, 0), (8, 3), ("unscrambled", dt, nt))
    # X mode 2: the line plan.  dp lines hold 16 rows and mesh3 at sigma = 1 keeps its plan; sp lines hold 32 rows, 43 of its phases would
    # need more than 8 of them and the planner turns that plan down (asserted: the re-layout path answers) -- the thin mesh keeps it
    L = cases("mesh3-s1", dt)
    with tuning(pkg, spmmv_ycol_nt=1, nontemporal=nt, spmmv_xline=1):
        A = pkg.DeviceMatrix(L.s, block_tlc=L.b)
        info = A.block_plan_info()
        if dt == "f64":
            assert info["line_plan"] == 1 and info["line_phases"] >= info["tiles"], info
            run_all(t, L, A, (8, 0), (8, 0), ("lines", dt, nt))
        else:
            assert info["line_plan"] == 0 and info["phased_plan"] == 1, info
            run_all(t, L, A, (8, 0), (8, 1), ("lines turned down", dt, nt))
        T = cases("thin3-s1", dt)
        A = pkg.DeviceMatrix(T.s, block_tlc=T.b)
        info = A.block_plan_info()
        assert info["line_plan"] == 1 and info["line_phases"] > info["tiles"], info
        run_all(t, T, A, (8, 0), (8, 0), ("lines, thin mesh", dt, nt))
    for depth, waves in ((1, 4), (2, 4), (1, 5)):                                    # the streamed kernels (waves 5: its own instantiation)
        with tuning(pkg, spmmv_ycol_nt=1, nontemporal=nt, spmmv_stream=4, spmmv_stream_depth=depth, spmmv_stream_waves=waves):
            A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
            info = A.block_plan_info()
            assert info["stream_grid"] > 0 and info["stream_descriptors"] >= info["phases"], info
            run_all(t, K, A, (10, 0), (10, 1), ("stream", depth, waves, dt, nt))


# ------------------------------------------------------------------------------------------------ 4. spmmv_phase_rows = 512
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,phase_dp", [("band11", 24), ("mesh3", 24), ("mesh2", 0)])
def test_512_row_phases(pkg, t, cases, name, phase_dp, dt):
    """some phase lists more than 256 rows: two-byte indices and the MAXP = 8 instantiation (32 KB of LDS; column-major X through
    registers: two list entries per thread).  The streamed kernel is compiled for one-byte indices only and must decline.
    mesh2 under the default cuts ("spmmv_phase_dp" 24: least staged rows + 24 per phase) stays at 236 rows per phase, which is the
    MAXP = 4 kernel again; filled to the brim ("spmmv_phase_dp" 0, what the device-side builder does) its longest phase lists 304."""
    K = cases(name, dt)
    with tuning(pkg, spmmv_phase_rows=512, spmmv_phase_dp=phase_dp):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 1 and 256 < info["max_rows"] <= 512 and info["idx8"] == 0, info
        run_all(t, K, A, (8, 0), (8, 1), (name, dt))
    with tuning(pkg, spmmv_phase_rows=512, spmmv_xcol=1):
        for ld in K.lds():
            run(t, K, A, False, ld, (8, 0), (name, dt, "xcol", ld))
    with tuning(pkg, spmmv_phase_rows=512, spmmv_phase_dp=phase_dp, spmmv_stream=4):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert info["max_rows"] > 256 and info["stream_grid"] == 0, info
        run_all(t, K, A, (8, 0), (8, 1), (name, dt, "stream declined"))


# ------------------------------------------------------------------------------------------------ 5. spmmv_phased = 0
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["band11", "mesh3", "mesh2"])
def test_without_a_phased_plan_kernel_6_answers(pkg, t, cases, name, dt):
    K = cases(name, dt)
    with tuning(pkg, spmmv_phased=0):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 0 and info["list_plan"] == 1, info
        run_all(t, K, A, (6, 0), (6, 1), (name, dt))


# ------------------------------------------------------------------------------------------------ 6. spmmv_reorder = 3
@pytest.mark.parametrize("name,dt,stride,lines", [("mesh3", "f64", 36, 1), ("mesh3", "f64", 36, 4), ("mesh3", "f32", 36, 1), ("mesh3", "f32", 36, 4),
                                                   ("stencil1", "f64", 24, 4)])
def test_brick_row_order(pkg, t, cases, name, dt, stride, lines):
    """tiles = flat bricks of `lines` mesh lines of `stride` = nx * dof rows in original numbering (uspmv_scs_reorder_bricks)"""
    K = cases(name, dt)
    with tuning(pkg, spmmv_reorder=3, spmmv_brick_stride=stride, spmmv_brick_lines=lines):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 1 and info["tiles"] == (K.n + 63) // 64, info
        run_all(t, K, A, (8, 0), (8, 1), (name, dt, stride, lines))


# ------------------------------------------------------------------------------------------------ 7. a line that crosses ld
def test_line_plan_at_the_end_of_a_column(pkg, orc, t):
    """A rectangular matrix (1019 rows, 1025 columns; convert_to_scs and the planner take it: confirmed on the CPU) whose rows all refer
    to the last six columns.  ld = 1026 (n_cols rounded up to even, >= n_rows_padded = 1024): the last listed line of every column,
    X rows 1024..1039, crosses ld after its first 16-byte piece -- the branch of the line staging that must neither copy the next
    column's elements nor, in the last column, read behind X.  X[1025] of every column is never referred to and holds a poison."""
    n, nc = 1019, 1025
    I = np.repeat(np.arange(n), 7)
    J = np.empty((n, 7), np.int64)
    J[:, :6] = np.arange(n)[:, None] + np.arange(6)[None, :]
    J[:, 6] = nc - 1 - np.arange(n) % 6
    V = 1.0 + 0.01 * ((np.arange(n * 7) * 7) % 13)
    m = pkg.Coo.from_arrays(n, nc, I, J.ravel(), V)
    K = Case(pkg, orc, m, 32, 1, "f64")
    ld = nc + 1
    assert K.n == 1024 and ld % 2 == 0 and ld >= K.n and (ld - 1024) * 8 < 128
    X = K.block(ld, False)
    X.reshape(K.b, ld)[:, nc:] = 1e300
    Yo = K.oracle(X, ld, False)
    with tuning(pkg, spmmv_xline=1):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 1 and info["line_plan"] == 1, info
        got, path = product(t, K, A, t.from_numpy(X).cuda(), ld, False)
        assert path == (8, 0), path
        same_bits(K, got, Yo, ld, False, ("rectangular",))
    assert np.abs(Yo).max() < 1e6                           # (the poison is in no product)


# ------------------------------------------------------------------------------------------------ 8. xcd_remap / xcd_stagger
def test_xcd_remap_and_stagger_share_a_word(pkg):
    old = pkg.get_tuning("xcd_remap"), pkg.get_tuning("xcd_stagger")
    try:
        pkg.set_tuning(xcd_remap=3)
        assert (pkg.get_tuning("xcd_remap"), pkg.get_tuning("xcd_stagger")) == (3, old[1])
        pkg.set_tuning(xcd_stagger=5)
        assert (pkg.get_tuning("xcd_remap"), pkg.get_tuning("xcd_stagger")) == (3, 5)
        pkg.set_tuning(xcd_remap=65536)
        assert (pkg.get_tuning("xcd_remap"), pkg.get_tuning("xcd_stagger")) == (65536, 5)
        pkg.set_tuning(xcd_stagger=2047)
        assert (pkg.get_tuning("xcd_remap"), pkg.get_tuning("xcd_stagger")) == (65536, 2047)
        for bad in (dict(xcd_stagger=2048), dict(xcd_stagger=-1), dict(xcd_remap=65537)):
            with pytest.raises(pkg.UspmvError):
                pkg.set_tuning(**bad)
            assert (pkg.get_tuning("xcd_remap"), pkg.get_tuning("xcd_stagger")) == (65536, 2047)
        pkg.set_tuning(xcd_remap=0)
        assert (pkg.get_tuning("xcd_remap"), pkg.get_tuning("xcd_stagger")) == (0, 2047)
    finally:
        pkg.set_tuning(xcd_remap=old[0], xcd_stagger=old[1])
    assert (pkg.get_tuning("xcd_remap"), pkg.get_tuning("xcd_stagger")) == old


REMAPS = [(G, S) for G in (2, 3, 5) for S in (0, 1, 3, 2047)] + [(1, 0), (1, 3)]


def full_and_rest(grid, G):
    """a grid this file remaps: at least 16 blocks, no multiple of 8 (nor of 8G), at least one full super-block of 8G blocks and a rest"""
    return grid >= 16 and grid % 8 != 0 and (G == 1 or (grid // (8 * G) >= 1 and grid % (8 * G) != 0))


@pytest.mark.parametrize("dt", DTYPES)
def test_block_remap_phased_spmmv(pkg, t, cases, dt):
    K = cases("band40", dt)
    with tuning(pkg):
        A = pkg.DeviceMatrix(K.s, block_tlc=K.b)
        tiles = A.block_plan_info()["tiles"]
        assert tiles == 47
        dX = None
        for G, S in REMAPS:
            assert full_and_rest(tiles, G)
            pkg.set_tuning(xcd_remap=G, xcd_stagger=S)
            dX = run(t, K, A, True, K.n, (8, 0), (dt, G, S), dX=dX)


def test_block_remap_spmv_on_tile_and_sweep_plans(pkg, orc, t):
    """spmv on a tile-local-column handle (256-row tiles) and on a column-window sweep handle (256-row tiles).  The matrix is the ragged
    generator of tests/test_gpu_sweep_ragged.py at 10999 rows: 43 tiles, so that G = 5 has a full super-block (40) and a rest as well.
    The sweep kernel takes its remap mode from "sweep_remap" (groups only; it has no key for the stagger bits), so that key follows G."""
    m = pkg.gen_banded_random(10999, 23, 700, seed=7, magnitude_decades=10.0)
    s = pkg.convert_to_scs(m, 32, 512, pkg.F64)
    a = s.arrays(); pkg.permute_scs_cols(s, a["old_to_new_idx"]); a = s.arrays()
    xp = np.zeros(s.n_rows_padded)
    xp[:s.n_rows] = pkg.apply_permutation(make_x(s.n_rows), a["new_to_old_idx"])
    yo = orc.spmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
    assert s.n_rows % 256 != 0 and s.n_rows_padded == 11008 and not np.any(yo[:s.n_rows] == SENTINEL)
    with tuning(pkg, tlc_tile_rows=256):
        T = pkg.DeviceMatrix(s, tlc=True)
        kind, tiles, planned = T.plan_info()
        assert kind == 1 and tiles == planned == 43 and T.tile_rows == 256, (kind, tiles, planned, T.tile_rows)
        W = pkg.DeviceMatrix(s)
        nt, nsw = W.optimize_sweep(s, 9, 256)
        assert W.plan_info()[0] == 2 and nt == nsw == 43, (W.plan_info(), nt, nsw)
        dx = t.from_numpy(xp).cuda()
        for G, S in REMAPS:
            assert full_and_rest(43, G)
            pkg.set_tuning(xcd_remap=G, xcd_stagger=S, sweep_remap=G)
            for what, A in (("tile plan", T), ("sweep plan", W)):
                y = t.full((s.n_rows_padded + GUARD,), SENTINEL, dtype=t.float64, device="cuda")
                pkg.spmv(A, dx, y)
                t.cuda.synchronize()
                got = y.cpu().numpy()
                assert np.all(got[s.n_rows_padded:] == SENTINEL), (what, G, S)
                assert not np.any(got[:s.n_rows] == SENTINEL), (what, G, S, np.flatnonzero(got[:s.n_rows] == SENTINEL)[:8].tolist())
                assert np.array_equal(got[:s.n_rows_padded].view(np.uint64), yo.view(np.uint64)), (what, G, S)
