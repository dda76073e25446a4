"""The block-vector column-window sweep kernel (csrc/spmmv_sweep.hip) in the forms tests/test_gpu_spmmv_sweep.py leaves out: two LDS
buffers ("sweep_nbuf" 2: the toggle cb ^ 1, window s + 1 staged while s is consumed), "nontemporal" 0, "sweep_remap" other than 8, a tile
without windows (S == 0), a last tile whose last wave is partial, a count byte of 255 (not a multiple of the batch of four rounds),
special values in column-major X, in float and under two buffers -- and every way the launcher declines a call (windows narrower than one
wave instruction per column, ld or pointers off the 16-byte grid, another block width, a plan that a declined re-plan removed), where
another kernel must give the same bits.  Every case compares with the oracle bit for bit, checks that nothing of Y beyond the matrix rows
is written, and asserts through DeviceMatrix.spmmv_last_path() that the sweep kernel (9) did, or did not, answer.  The shapes were checked
against the host planner (tests/cpp/block_sweep_plan_emulate.cpp replays the same ones)."""
import numpy as np
import pytest

from test_gpu_spmmv_sweep import block, prep

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
TAIL = 40            # elements allocated behind Y (and X): must keep the sentinel
TUNING = dict(spmmv_variant=0, sweep_nbuf=1, nontemporal=1, sweep_remap=8, sweep_max_stage=0)     # the defaults, restored by every test


@pytest.fixture(scope="module")
def t(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch


def shape_a(pkg):
    return pkg.gen_stencil27(15, 11, 7)                       # 1155 rows


def _coo(pkg, n, rows):
    I = np.concatenate([np.full(len(r), i, np.int32) for i, r in enumerate(rows)])
    J = np.concatenate([np.asarray(r, np.int32) for r in rows])
    V = 0.5 + ((I.astype(np.int64) * 7 + J.astype(np.int64) * 3) % 29) / 16.0
    return pkg.Coo.from_arrays(n, n, I, J, V)


def shape_h(pkg):
    """3500 rows of {i-3 .. i+3}; rows 1024..2047 and every row with i % 7 == 3 emptied: the second 1024-row tile has no window at all"""
    n = 3500
    rows = [[] if (1024 <= i < 2048 or i % 7 == 3) else list(range(max(i - 3, 0), min(i + 3, n - 1) + 1)) for i in range(n)]
    return _coo(pkg, n, rows)


def shape_d(pkg, wide):
    """2048 rows: row 5 has `wide` entries in columns 0 .. wide-1, every other row the diagonal and column i + 300"""
    n = 2048
    rows = [list(range(wide)) if i == 5 else [i] + ([i + 300] if i + 300 < n else []) for i in range(n)]
    return _coo(pkg, n, rows)


def shape_band(pkg):
    return pkg.gen_banded_random(5000, 40, 700, magnitude_decades=4.0)


def shape_stencil3(pkg):
    return pkg.gen_stencil27(14, 13, 12, dof=3)


class Case:
    """One struct on the device with its oracle results (computed once per (X, layout, ld) and shared by the forms)."""

    def __init__(self, pkg, orc, m, C, sigma, dt):
        self.pkg, self.orc, self.C = pkg, orc, C
        self.dtype = pkg.F64 if dt == "f64" else pkg.F32
        self.b = 8 if dt == "f64" else 16
        self.vw = 2 if dt == "f64" else 4                 # elements per 16 bytes
        self.s, self.a, self.xp = prep(pkg, m, C, sigma, self.dtype)
        self.n = self.s.n_rows_padded
        self.A = pkg.DeviceMatrix(self.s)
        self._ref = {}

    def plan(self, wlog, tile_rows, b=None):
        return self.A.optimize_block_sweep(self.s, self.b if b is None else b, wlog=wlog, tile_rows=tile_rows)

    def oracle(self, X, b, ld, rowwise, key=None):
        if key is not None and (key, b, ld, rowwise) in self._ref:
            return self._ref[(key, b, ld, rowwise)]
        a = self.a
        Yo = self.orc.spmmv_scs(self.C, self.s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, b, ld, rowwise)
        Yo.setflags(write=False)
        if key is not None:
            self._ref[(key, b, ld, rowwise)] = Yo
        return Yo

    def run(self, t, rowwise, ld, X=None, key="plain", b=None, nan_equal=False, x_off=0, y_off=0):
        """One product into a sentinel-filled Y; returns spmmv_last_path().  x_off / y_off: elements by which X / Y are moved off their
        allocation (a view into a larger tensor)."""
        pkg, b, n = self.pkg, self.b if b is None else b, self.n
        if X is None:
            X = block(self.xp, b, ld, rowwise)
        else:
            key = key if key != "plain" else None
        Yo = self.oracle(X, b, ld, rowwise, key)
        hX = np.full(x_off + X.size + TAIL, SENTINEL, X.dtype); hX[x_off:x_off + X.size] = X
        dXa = t.from_numpy(hX).cuda()
        dYa = t.full((y_off + b * ld + TAIL,), SENTINEL, dtype=dXa.dtype, device="cuda")
        dX, dY = dXa[x_off:x_off + X.size], dYa[y_off:y_off + b * ld]
        pkg.spmmv(self.A, dX, dY, b, ld, pkg.ROWWISE if rowwise else pkg.COLWISE)
        t.cuda.synchronize()
        path = self.A.spmmv_last_path()
        all_y = dYa.cpu().numpy()
        got = all_y[y_off:y_off + b * ld]
        what = (rowwise, ld, b, path)
        assert np.all(all_y[:y_off] == SENTINEL) and np.all(all_y[y_off + b * ld:] == SENTINEL), what      # nothing around Y is touched
        if rowwise:
            same(got[:n * b], Yo[:n * b], nan_equal, what)
            assert np.all(got[n * b:] == SENTINEL), what
        else:
            for v in range(b):
                same(got[v * ld:v * ld + n], Yo[v * ld:v * ld + n], nan_equal, what + (v,))
                assert np.all(got[v * ld + n:(v + 1) * ld] == SENTINEL), what + (v,)                     # rows n_rows_padded..ld are left alone
        return path


def same(got, want, nan_equal, what):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    if nan_equal:
        both = np.isnan(got) & np.isnan(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        assert np.array_equal(got[~both].view(u), want[~both].view(u)), what
    else:
        assert not np.isnan(want).any(), what
        assert np.array_equal(got.view(u), want.view(u)), what


def xcol_sweeps(case, wlog):
    """Column-major X is staged by wave instructions of 64 pieces of 16 bytes per column: a window narrower than that keeps the re-layout path."""
    return (1 << wlog) >= 64 * case.vw


def all_forms(case, t, wlog):
    """Both layouts x sweep_nbuf x nontemporal x (column-major) ld; the sweep must answer wherever the window is wide enough."""
    pkg, n = case.pkg, case.n
    for nbuf in (1, 2):
        for nt in (0, 1):
            pkg.set_tuning(sweep_nbuf=nbuf, nontemporal=nt)
            assert case.run(t, True, n) == (9, 0), (nbuf, nt)
            for ld in (n, n + 24):
                path = case.run(t, False, ld)
                if xcol_sweeps(case, wlog):
                    assert path == (9, 0), (nbuf, nt, ld, path)
                else:
                    assert path[0] != 9, (nbuf, nt, ld, path)


SHAPES = [("A", shape_a, 32, 64, 6, 6), ("A", shape_a, 32, 64, 7, 7), ("A", shape_a, 32, 64, 8, 8), ("A", shape_a, 8, 1, 7, 7),
          ("H", shape_h, 16, 1, 7, 8), ("H", shape_h, 32, 1, 7, 8), ("H", shape_h, 64, 1, 7, 8), ("band", shape_band, 32, 64, 7, 7)]


@pytest.mark.parametrize("name,gen,C,sigma,wlog64,wlog32", SHAPES)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sweep_forms(pkg, orc, t, name, gen, C, sigma, wlog64, wlog32, dt):
    """A: n_rows_padded 1184 (C = 8: 1160) = 18.5 waves, the last tile 160 rows with a half wave.  H: a tile with S == 0, 0..10 windows per
    tile.  band: 14-20 windows per tile, the longest buffer alternation under sweep_nbuf 2."""
    case = Case(pkg, orc, gen(pkg), C, sigma, dt)
    if name == "A":
        assert case.n == (1184 if C == 32 else 1160)          # the last wave of the last tile is partial
    wlog = wlog64 if dt == "f64" else wlog32
    try:
        nt, ns = case.plan(wlog, 1024)
        assert nt > 0 and nt == ns, (nt, ns)
        pkg.set_tuning(spmmv_variant=9)
        all_forms(case, t, wlog)
    finally:
        pkg.set_tuning(**TUNING)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sweep_remap_values(pkg, orc, t, dt):
    """Shape A at wlog 7 with the tile -> workgroup map off, of one tile per group, and the default eight."""
    case = Case(pkg, orc, shape_a(pkg), 32, 64, dt)
    try:
        nt, ns = case.plan(7, 1024)
        assert nt == 2 and ns == 2
        pkg.set_tuning(spmmv_variant=9)
        for remap in (0, 1, 8):
            for nbuf in (1, 2):
                pkg.set_tuning(sweep_remap=remap, sweep_nbuf=nbuf)
                assert case.run(t, True, case.n) == (9, 0), (remap, nbuf)
                path = case.run(t, False, case.n + 24)
                assert (path == (9, 0)) if xcol_sweeps(case, 7) else (path[0] != 9), (remap, nbuf, path)
    finally:
        pkg.set_tuning(**TUNING)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sweep_count_byte_255(pkg, orc, t, dt):
    """Shape D: one row with 255 entries in one window -- the count byte's maximum, 63 batches of four rounds and one of three, run by a
    single lane while 63 lanes sit the rounds out.  The default staging limit declines the shape (24 bytes per non-zero), and so does a
    256th entry whatever the limit; both must leave the handle without a plan and with the right bits."""
    case = Case(pkg, orc, shape_d(pkg, 255), 32, 1, dt)
    wide = Case(pkg, orc, shape_d(pkg, 256), 32, 1, dt)
    try:
        pkg.set_tuning(spmmv_variant=9)
        nt, ns = case.plan(8, 1024)
        assert nt == 2 and ns != nt
        assert case.run(t, True, case.n) == (3, 0)
        assert case.run(t, False, case.n + 24) == (3, 1)
        pkg.set_tuning(sweep_max_stage=4096)
        nt, ns = case.plan(8, 1024)
        assert (nt, ns) == (2, 2)
        all_forms(case, t, 8)
        nt, ns = wide.plan(8, 1024)
        assert nt == 2 and ns != nt
        for nbuf in (1, 2):
            pkg.set_tuning(sweep_nbuf=nbuf)
            assert wide.run(t, True, wide.n)[0] != 9
            assert wide.run(t, False, wide.n)[0] != 9
    finally:
        pkg.set_tuning(**TUNING)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sweep_two_buffers_four_rows_per_lane(pkg, orc, t, dt):
    """4096-row tiles (four rows per lane) at wlog 10: two buffers of 64 KiB fit."""
    case = Case(pkg, orc, shape_stencil3(pkg), 32, 1, dt)
    try:
        nt, ns = case.plan(10, 4096)
        assert nt == 2 and ns == 2
        pkg.set_tuning(spmmv_variant=9, sweep_nbuf=2)
        assert case.run(t, True, case.n) == (9, 0)
        for ld in (case.n, case.n + 24):
            assert case.run(t, False, ld) == (9, 0)
    finally:
        pkg.set_tuning(**TUNING)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sweep_two_buffers_asked_one_fits(pkg, orc, t, dt):
    """wlog 11: a window is 128 KiB, two do not fit the LDS, the launcher runs one buffer whatever sweep_nbuf asks."""
    case = Case(pkg, orc, shape_stencil3(pkg), 32, 512, dt)
    try:
        nt, ns = case.plan(11, 1024)
        assert nt == 7 and ns == 7
        pkg.set_tuning(spmmv_variant=9, sweep_nbuf=2)
        assert case.run(t, True, case.n) == (9, 0)
        for ld in (case.n, case.n + 24):
            assert case.run(t, False, ld) == (9, 0)
    finally:
        pkg.set_tuning(**TUNING)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sweep_declines_and_another_kernel_answers(pkg, orc, t, dt):
    """Every reason for which launch_bsw / launch_spmmv_sweep turn a call down on a handle that carries the plan: the gather kernel (3)
    answers after a re-layout pass (x_pass 1), or -- X or Y off the 16-byte grid -- the generic kernel (1) on X as passed."""
    case = Case(pkg, orc, shape_a(pkg), 32, 64, dt)
    n, vw = case.n, case.vw
    narrow = 6 if dt == "f64" else 7                          # 2^narrow < 64 * vw rows: narrower than one wave instruction per column
    try:
        pkg.set_tuning(spmmv_variant=9)
        for nbuf in (1, 2):
            pkg.set_tuning(sweep_nbuf=nbuf)
            nt, ns = case.plan(narrow, 1024)
            assert nt == 2 and ns == 2
            assert case.run(t, False, n) == (3, 1)
            assert case.run(t, True, n) == (9, 0)                 # the same handle, row-major: the sweep
            nt, ns = case.plan(8, 1024)
            assert nt == 2 and ns == 2
            assert case.run(t, False, n) == (9, 0)
            # ld off the 16-byte grid: odd for double, ld % 4 == 2 for float
            ld = n + 1 if dt == "f64" else n + 2
            assert ld % vw != 0 and (dt == "f64" or ld % 4 == 2)
            assert case.run(t, False, ld) == (3, 1)
            # X, then Y, one element off a 16-byte boundary
            for rowwise in (True, False):
                assert case.run(t, rowwise, n, x_off=1) == (1, 0)
                assert case.run(t, rowwise, n, y_off=1) == (1, 0)
                assert case.run(t, rowwise, n) == (9, 0)
        if dt == "f64":
            # b = 4 on a handle planned for b = 8
            assert case.run(t, True, n, b=4) == (3, 0)
            assert case.run(t, False, n, b=4) == (3, 1)
            assert case.run(t, True, n) == (9, 0)
    finally:
        pkg.set_tuning(**TUNING)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sweep_declined_replan_removes_the_plan(pkg, orc, t, dt):
    """A handle that carried a plan and is planned again with a shape the planner declines (sigma 512, wlog 8, 2048-row tiles) has none."""
    case = Case(pkg, orc, shape_stencil3(pkg), 32, 512, dt)
    try:
        pkg.set_tuning(spmmv_variant=9)
        nt, ns = case.plan(9, 1024)
        assert nt == 7 and ns == 7
        assert case.run(t, True, case.n) == (9, 0)
        nt, ns = case.plan(8, 2048)
        assert nt == 4 and ns == 0
        assert case.run(t, True, case.n) == (3, 0)
        assert case.run(t, False, case.n + 24) == (3, 1)
    finally:
        pkg.set_tuning(**TUNING)


@pytest.mark.parametrize("name,gen,C,sigma,wlog64,wlog32", [("A", shape_a, 32, 64, 8, 8), ("H", shape_h, 32, 1, 7, 8)])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sweep_special_values_both_layouts(pkg, orc, t, name, gen, C, sigma, wlog64, wlog32, dt):
    """+-inf, NaN and -0.0 in 200 places of X and a non-finite X row at the padding column: a lane that sits a round out discards its
    product also when the X row it happens to read is NaN, or lies in the part of a window past ld that was never staged."""
    case = Case(pkg, orc, gen(pkg), C, sigma, dt)
    b, n, a = case.b, case.n, case.a
    wlog = wlog64 if dt == "f64" else wlog32
    rng = np.random.default_rng(5)
    pad_col = int(a["col_idxs"][a["chunk_ptrs"][0] + (a["chunk_lengths"][0] - 1) * C + C - 1])
    pad_row = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, -1.0, 5e-324] * (b // 8), case.xp.dtype)
    try:
        nt, ns = case.plan(wlog, 1024)
        assert nt > 0 and nt == ns
        pkg.set_tuning(spmmv_variant=9)
        for rowwise in (True, False):
            X = block(case.xp, b, n, rowwise)
            sp = rng.choice(X.size, 200, replace=False)
            X[sp[:50]] = np.inf; X[sp[50:100]] = -np.inf; X[sp[100:150]] = np.nan; X[sp[150:]] = -0.0
            if rowwise:
                X[pad_col * b:(pad_col + 1) * b] = pad_row
            else:
                X[pad_col::n] = pad_row
            for nbuf in (1, 2):
                pkg.set_tuning(sweep_nbuf=nbuf)
                assert case.run(t, rowwise, n, X=X, key=("special", rowwise), nan_equal=True) == (9, 0), (rowwise, nbuf)
    finally:
        pkg.set_tuning(**TUNING)
