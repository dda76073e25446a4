"""Every single-GPU kernel family on NON-SQUARE matrices.  The other GPU files build square matrices, where the x rows a matrix refers
to never exceed its padded rows; here they do, or the matrix has far fewer columns than rows:

  block  rows 4001 .. 7001 of gen_banded_random(9999, 23, 700, seed 7): 3001 x 9999, n_rows_padded 3008 (no multiple of any tile), x rows up
         to 7695 (odd, = 3 mod 4, no multiple of any window) -- x windows, lines and elements far beyond the padded rows
  halo   3001 x 4238: a band of +-60 inside the rows and one to three columns in [3001, 4238) on two rows of three; some late rows are empty,
         so that at sigma >= 64 the reference's tie order parks real rows on padded slots and permuted columns alias halo column numbers
  thin   the same generator at 1019 x 1024: n_cols == n_rows_padded != n_rows
  tall   3001 x 257, three columns per row: x far shorter than y
  mesh   rows 5001 .. 8001 of gen_stencil27(5, 5, 120, dof 3): 3001 x 9000, x rows up to 8097 -- the one shape here whose columns come in runs,
         so that the block planner keeps its LINE plan (on the others the lines would stage more than twice the rows and it turns them down)

x is built directly in the struct's column numbering (1 + the highest column of any part elements, scaled differently below and above
n_rows) and the device tensor holds exactly that many elements: nothing behind the contract's x_len may be needed.  Block vectors have
ld >= x rows > n_rows_padded, so thousands of Y rows per column lie between the rows a call writes and ld.  Y is pre-filled with 9.0 and
carries a 64-element guard; everything outside the written rows must still be 9.0.  Comparison is bitwise against the oracle on the
struct's own arrays, a NaN equal to any NaN in the same place; there is no tolerance in this file.  Every test asserts its preconditions
and the plan, kernel or path that answered before it looks at a product, and counts its cases; nothing is skipped.

What the planners make of these shapes -- which plans stage or sweep every tile, which the planner declines -- is computed on the host by
tests/cpp/nonsquare_plan_check.cpp and compared with sweeps() below in tests/test_nonsquare_host.py, which also holds the non-square
gates: no additive chunk records on any of these structs."""
import contextlib

import numpy as np
import pytest

from conftest import make_x
from test_gpu_ap_device_setup import KINDS, bits, dev_coo, host_parts, host_structs, part_dtypes, same_handles, same_parts
from test_gpu_ap_hp_spmmv import _bs_rule
from test_gpu_ap_hp_spmmv_sweep import DEFAULTS, GUARD, _build, _oracle, _same
from test_gpu_ap_spmmv_sweep import _pair_structs
from test_gpu_sweep_ap_hp import _same_sweep_plans
from test_gpu_sweep_ragged import GATHER, SWEEP, _expected_path

pytestmark = pytest.mark.gpu
CSIG = ((32, 512), (8, 64), (64, 1), (16, 16))
SWEEP_SHAPES = ((8, 256), (10, 1024), (13, 4096))        # (log2 of the window, rows per tile)
TH_PAIR, TH_HP = 1e-1, (1.0, 1e-2)                        # the splits' thresholds: ap[dp_sp]; the kinds with an fp16 part
FILL = 9.0
# (matrix, C, sigma, kind) whose host route refuses: the first part's tie order parks a row that is empty there, but not in another part, on a
# padded slot -- as the reference would overrun its chunk
HOST_REFUSES = {("tall", 8, 64, "dp_sp_hp")}


# ------------------------------------------------------------------------------------------------ the matrices
def _values(I, J):
    i, j = I.astype(np.int64), J.astype(np.int64)
    return (1.0 + ((i * 7 + j * 3) % 29) / 16.0) * 10.0 ** (((i * 5 + j * 11) % 9) - 6) * np.where((i + j) % 5 == 0, -1.0, 1.0)


def halo_matrix(pkg, n, n_cols):
    """n x n_cols: row i holds {i - 60, i - 17, i - 3, i, i + 5, i + 29, i + 60} inside [0, n) and, unless i % 3 == 2, one to three columns
    in [n, n_cols); rows i >= 2600 with i % 7 == 3 are empty.  Magnitudes over nine decades.  Entries sorted by row, then column."""
    I, J = [], []
    for i in range(n):
        if i >= 2600 and i % 7 == 3:
            continue
        cols = {c for c in (i - 60, i - 17, i - 3, i, i + 5, i + 29, i + 60) if 0 <= c < n}
        if i % 3 != 2:
            for k in range(1 + (i * 7) % 3):
                cols.add(n + (i * 131 + k * 389) % (n_cols - n))
        cols = sorted(cols)
        I += [i] * len(cols); J += cols
    I, J = np.asarray(I, np.int32), np.asarray(J, np.int32)
    return pkg.Coo.from_arrays(n, n_cols, I, J, _values(I, J))


def tall_matrix(pkg, n=3001, n_cols=257):
    i = np.arange(n, dtype=np.int64)
    cols = np.sort(np.stack([(i * 37) % n_cols, (i * 101 + 13) % n_cols, (i * 211 + 91) % n_cols], 1), 1)
    keep = np.ones_like(cols, bool); keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    I, J = np.repeat(i, 3).reshape(n, 3)[keep].astype(np.int32), cols[keep].astype(np.int32)
    return pkg.Coo.from_arrays(n, n_cols, I, J, _values(I, J))


MATRICES = {   # name: (builder, rows, columns, n_rows_padded)
    "block": (lambda pkg: pkg.gen_banded_random(9999, 23, 700, seed=7, magnitude_decades=10.0, row_begin=4001, row_end=7002), 3001, 9999, 3008),
    "halo": (lambda pkg: halo_matrix(pkg, 3001, 4238), 3001, 4238, 3008),
    "thin": (lambda pkg: halo_matrix(pkg, 1019, 1024), 1019, 1024, 1024),
    "tall": (tall_matrix, 3001, 257, 3008),
    "mesh": (lambda pkg: pkg.gen_stencil27(5, 5, 120, dof=3, row_begin=5001, row_end=8002), 3001, 9000, 3008),
}
MESH_X_ROWS = 8097
# (matrix, C, sigma): does uspmv_dmat_optimize_block keep the line plan under "spmmv_xline" 1, in (dp, sp)?  From the host planner
# (tests/cpp/nonsquare_plan_check.cpp, held against this table in tests/test_nonsquare_host.py)
LINE_PLAN = {("block", 32, 512): (0, 0), ("block", 64, 1): (0, 0), ("halo", 32, 512): (0, 0), ("mesh", 32, 1): (1, 1), ("mesh", 64, 1): (1, 1)}
LDS_BYTES = 160 * 1024                                    # of a workgroup


def lds_vectors(b, wlog, itemsize):
    """vectors per pass of the block sweep kernels: the largest of {8, 4, 2} that is at most b, divides b and fits the LDS with one window"""
    for bs in (8, 4, 2):
        if bs <= b and b % bs == 0 and (itemsize << wlog) * bs <= LDS_BYTES:
            return bs
    return 0
BLOCK_X_ROWS, BLOCK_X_ROWS_FIRST = 7695, 7683             # the row block: x rows of all parts together / of the first part of a split alone


def sweeps(name, sigma, wlog):
    """does the sweep planner take every tile (True) or decline the matrix (False)?  The sigma sort permutes the columns below n_rows;
    under sigma = 512 the windows of 2^8 columns of a row then no longer ascend.  The row block has no column below its n_rows."""
    return name == "block" or not (sigma == 512 and wlog == 8)


@pytest.fixture(scope="module")
def t(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    pkg.set_tuning(**DEFAULTS)
    yield torch
    pkg.set_tuning(**DEFAULTS)


@pytest.fixture(scope="module")
def mats(pkg):
    cache = {}

    def get(name):
        if name not in cache:
            gen, n, nc, _ = MATRICES[name]
            cache[name] = gen(pkg)
            assert (cache[name].n_rows, cache[name].n_cols) == (n, nc) and n != nc
        return cache[name]
    return get


@contextlib.contextmanager
def tuned(pkg, **kw):
    old = {k: pkg.get_tuning(k) for k in kw}
    try:
        pkg.set_tuning(**kw)
        yield
    finally:
        pkg.set_tuning(**old)


def _x(x_rows, n_rows, dtype):
    """x over the struct's column numbering: make_x, the elements from n_rows on at half the scale"""
    xp = make_x(x_rows)
    xp[n_rows:] *= 0.5
    return xp.astype(dtype)


def _check(got, want, tag):
    """`want` holds FILL wherever the call must not write: one comparison covers the products, the rows up to ld and the guard"""
    assert got.shape == want.shape
    if not _same(got, want):
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{tag}: {len(bad)} of {got.size} elements differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}")


def _block_x(cols, b, ld, rowwise, fill=0.0):
    """b columns laid out with leading dimension ld; the rows behind a column's elements hold `fill`"""
    X = np.full(b * ld, fill, cols[0].dtype)
    for v in range(b):
        if rowwise: X[v:cols[v].size * b:b] = cols[v]
        else: X[v * ld:v * ld + cols[v].size] = cols[v]
    return X


def _block_want(ycols, b, ld, rowwise):
    n = ycols[0].size
    want = np.full(b * ld + GUARD, FILL, ycols[0].dtype)
    for v in range(b):
        if rowwise: want[v:n * b:b] = ycols[v]
        else: want[v * ld:v * ld + n] = ycols[v]
    return want


# ------------------------------------------------------------------------------------------------ one struct in dp or sp
class Rect:
    """One struct of one matrix, columns permuted with its own permutation; x of exactly x_rows elements and the oracle's y"""

    def __init__(self, pkg, orc, name, m, C, sigma, dt):
        self.pkg, self.orc, self.name, self.C, self.sigma = pkg, orc, name, C, sigma
        self.code, self.np_dtype = (pkg.F64, np.float64) if dt == "f64" else (pkg.F32, np.float32)
        s = pkg.convert_to_scs(m, C, sigma, self.code)
        self.perm = s.arrays()["old_to_new_idx"].copy()
        pkg.permute_scs_cols(s, self.perm)
        self.s, self.a, self.n, self.n_rows = s, s.arrays(), s.n_rows_padded, m.n_rows
        self.x_rows = 1 + int(self.a["col_idxs"].max())
        self.xp = _x(self.x_rows, m.n_rows, self.np_dtype)
        self.want = np.concatenate([self.spmv_oracle(self.xp), np.full(GUARD, FILL, self.np_dtype)])
        self._case = {}

    def spmv_oracle(self, x):
        a = self.a
        return self.orc.spmv_scs(self.C, self.s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], x)

    def preconditions(self):
        _, n, nc, n_pad = MATRICES[self.name]
        assert self.s.n_rows == n != nc and self.n == n_pad and self.s.nnz > 0
        if self.name == "block":
            xr = self.x_rows
            assert xr == BLOCK_X_ROWS > self.n and xr % 2 == 1 and xr % 4 != 0
            for wlog, rows in SWEEP_SHAPES:
                assert xr % (1 << wlog) != 0 and self.n % rows != 0
        elif self.name == "halo":
            assert self.x_rows == nc > self.n
            assert int((self.perm >= n).sum()) == (7 if self.sigma >= 64 else 0)     # real rows parked on padded slots
        elif self.name == "thin":
            assert self.x_rows == nc == self.n
        elif self.name == "mesh":
            assert self.x_rows == MESH_X_ROWS > self.n and self.x_rows % 2 == 1 and self.x_rows % 4 != 0
        else:
            assert self.x_rows <= 512 < self.n

    def spmv(self, t, A, tag, want=None):
        dx = t.from_numpy(self.xp).cuda()
        assert dx.numel() == self.x_rows
        y = t.full((self.n + GUARD,), FILL, dtype=A.torch_dtype, device="cuda")
        self.pkg.spmv(A, dx, y)
        _check(y.cpu().numpy(), self.want if want is None else want, (self.name, self.C, self.sigma, self.np_dtype.__name__) + tuple(tag))

    def split2_want(self):
        """what "spmv_variant" 1 (scs_spmv_split2: two lanes per row) computes, restated through the oracle: the chain over the even slots
        of a row, the chain over its odd slots, one addition -- not the sequential chain, but as exactly defined, so bits are compared"""
        a, C, y = self.a, self.C, []
        cp, cl = a["chunk_ptrs"].astype(np.int64), a["chunk_lengths"].astype(np.int64)
        for h in (0, 1):
            T = (cl + 1 - h) >> 1
            idx = np.concatenate([cp[c] + ((2 * np.arange(T[c]) + h) * C)[:, None] + np.arange(C)[None, :] for c in range(len(cl))]).ravel()
            ptr = np.concatenate([[0], np.cumsum(T * C)]).astype(np.int32)
            y.append(self.orc.spmv_scs(C, self.s.n_chunks, ptr, T.astype(np.int32), a["col_idxs"][idx], a["values"][idx], self.xp))
        return np.concatenate([y[0] + y[1], np.full(GUARD, FILL, self.np_dtype)])

    def lds(self):
        return (self.x_rows, self.x_rows + 1, self.x_rows + 24)

    def case(self, b, rowwise, ld):
        """(X of b * ld elements, expected Y of b * ld + GUARD): column v = xp * (1 + v / 8)"""
        key = (b, rowwise, ld)
        if key not in self._case:
            a = self.a
            cols = [(self.xp * self.np_dtype(1.0 + v / 8.0)).astype(self.np_dtype) for v in range(b)]
            X = _block_x(cols, b, ld, rowwise)
            Yo = self.orc.spmmv_scs(self.C, self.s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, b, ld, rowwise)
            n = self.n
            ycols = [Yo[v:n * b:b] if rowwise else Yo[v * ld:v * ld + n] for v in range(b)]
            self._case[key] = (X, _block_want(ycols, b, ld, rowwise), cols)
        return self._case[key]

    def spmmv(self, t, A, b, rowwise, ld, tag, dX=None):
        """one product; returns (spmmv_last_path(), the device X)"""
        X, want, _ = self.case(b, rowwise, ld)
        if dX is None:
            dX = t.from_numpy(X).cuda()
        assert dX.numel() == b * ld and ld >= self.x_rows
        dY = t.full((b * ld + GUARD,), FILL, dtype=A.torch_dtype, device="cuda")
        self.pkg.spmmv(A, dX, dY, b, ld, self.pkg.ROWWISE if rowwise else self.pkg.COLWISE)
        t.cuda.synchronize()
        path = A.spmmv_last_path()
        _check(dY.cpu().numpy(), want, (self.name, self.C, self.sigma, b, "rowwise" if rowwise else "colwise", ld, path) + tuple(tag))
        return path, dX


@pytest.fixture(scope="module")
def rects(pkg, orc, t, mats):
    cache = {}

    def get(name, C, sigma, dt):
        if (name, C, sigma, dt) not in cache:
            cache[(name, C, sigma, dt)] = Rect(pkg, orc, name, mats(name), C, sigma, dt)
        return cache[(name, C, sigma, dt)]
    return get


def _line_plan(A, D):
    """host- and device-built plan of one struct: the same plan, every tile staged, and never an additive chunk record"""
    assert A.plan_info() == D.plan_info(), (A.plan_info(), D.plan_info())
    kind, tiles, planned = A.plan_info()
    assert kind == 1 and tiles == planned > 0, (kind, tiles, planned)
    assert A.additive_chunks() == (0, 0) and D.additive_chunks() == (0, 0)


# ------------------------------------------------------------------------------------------------ 1. SpMV, one precision
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("C,sigma", CSIG)
@pytest.mark.parametrize("name", ["block", "halo", "tall"])
def test_spmv_every_plan(pkg, t, rects, name, C, sigma, dt):
    """plain upload (at C = 32 also the software-pipelined kernel and the two-lanes-per-row kernel, the latter against its own two chains
    restated through the oracle: Rect.split2_want), the default plan from the host and from the device, the same under
    "tlc_additive" 2 (records must never be installed on a non-square struct), 16-bit and 12-bit local indices, the element plan
    ("tlc_elem" 2: on the caller's rows -- the dealing by the matrix graph is for square matrices), and the column-window sweep at three
    shapes from the host and from the device: kind 2 with every tile sweeping and equal digests, or -- where sweeps() says the planner
    declines -- no plan and the gather kernel's bits"""
    R = rects(name, C, sigma, dt)
    R.preconditions()
    s, cases = R.s, 0
    R.spmv(t, pkg.DeviceMatrix(s), ("upload",)); cases += 1
    if C == 32:
        with tuned(pkg, spmv_variant=2):
            R.spmv(t, pkg.DeviceMatrix(s), ("upload, spmv_variant", 2)); cases += 1
        with tuned(pkg, spmv_variant=1):
            R.spmv(t, pkg.DeviceMatrix(s), ("upload, spmv_variant", 1), want=R.split2_want()); cases += 1
    for additive in (pkg.get_tuning("tlc_additive"), 2):
        with tuned(pkg, tlc_additive=additive):
            A = pkg.DeviceMatrix(s); A.optimize(s)
            D = pkg.DeviceMatrix(s); D.optimize_device()
            _line_plan(A, D)
            assert A.plan_granularity() == D.plan_granularity() == 16 and not A.plan_rows_dealt()
            R.spmv(t, A, ("host plan, tlc_additive", additive)); R.spmv(t, D, ("device plan, tlc_additive", additive)); cases += 2
    for i12 in (0, 2):
        with tuned(pkg, tlc_idx12=i12):
            A = pkg.DeviceMatrix(s); A.optimize(s)
            D = pkg.DeviceMatrix(s); D.optimize_device()
        _line_plan(A, D)
        assert A.index_bits() == D.index_bits() and A.index_bits() in ((16,) if i12 == 0 else (12, 16)), (i12, A.index_bits(), D.index_bits())
        R.spmv(t, A, ("host plan, tlc_idx12", i12)); R.spmv(t, D, ("device plan, tlc_idx12", i12)); cases += 2
    with tuned(pkg, tlc_elem=2):
        A = pkg.DeviceMatrix(s); A.optimize(s)
        D = pkg.DeviceMatrix(s); D.optimize_device()
    _line_plan(A, D)
    assert A.plan_granularity() == D.plan_granularity() == 1, (A.plan_granularity(), D.plan_granularity())
    assert not A.plan_rows_dealt() and not D.plan_rows_dealt()
    R.spmv(t, A, ("host element plan",)); R.spmv(t, D, ("device element plan",)); cases += 2
    assert 256 % C == 0
    for wlog, rows in SWEEP_SHAPES:
        A, D = pkg.DeviceMatrix(s), pkg.DeviceMatrix(s)
        with tuned(pkg, sweep_max_stage=1 << 20):
            got = A.optimize_sweep(s, wlog, rows), D.optimize_sweep_device(None, wlog, rows)
        nt = -(-R.n // rows)
        if sweeps(name, sigma, wlog):
            assert got == ((nt, nt), (nt, nt)), (wlog, rows, got)
            assert A.plan_info() == D.plan_info() == (2, nt, nt)
            assert A.sweep_plan_digest() == D.sweep_plan_digest()
            assert A.sweep_plan_digest()[1][1:3] == [rows, wlog]
        else:
            assert got == ((nt, 0), (nt, 0)), (wlog, rows, got)
            assert A.plan_info()[0] == D.plan_info()[0] == 0
        R.spmv(t, A, ("host sweep plan", wlog, rows)); R.spmv(t, D, ("device sweep plan", wlog, rows)); cases += 2
    assert cases == 17 + (2 if C == 32 else 0)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("C,sigma", CSIG)
def test_thin_halo_has_no_additive_records(pkg, t, rects, C, sigma, dt):
    """n_cols == n_rows_padded but != n_rows: the default plan and the plan under "tlc_additive" 2 carry no records"""
    R = rects("thin", C, sigma, dt)
    R.preconditions()
    cases = 0
    R.spmv(t, pkg.DeviceMatrix(R.s), ("upload",))
    for additive in (pkg.get_tuning("tlc_additive"), 2):
        with tuned(pkg, tlc_additive=additive):
            A = pkg.DeviceMatrix(R.s); A.optimize(R.s)
            D = pkg.DeviceMatrix(R.s); D.optimize_device()
            _line_plan(A, D)
            R.spmv(t, A, ("host plan, tlc_additive", additive)); R.spmv(t, D, ("device plan, tlc_additive", additive)); cases += 2
    assert cases == 4


# ------------------------------------------------------------------------------------------------ 2. the declined sweep
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_declined_sweep_leaves_no_plan(pkg, t, rects, dt):
    """halo matrix, C = 32, sigma = 512, windows of 2^8: uspmv_dmat_optimize_sweep[_device] does not raise on a matrix whose tiles do not
    qualify -- it returns (tiles, 0) and leaves the handle WITHOUT a plan, also one that carried a sweep plan before (the builders drop it
    before they look at the matrix); the gather kernel then answers with the oracle's bits"""
    R = rects("halo", 32, 512, dt)
    R.preconditions()
    assert not sweeps("halo", 512, 8) and sweeps("halo", 512, 10)
    cases = 0
    with tuned(pkg, sweep_max_stage=1 << 20):
        for device in (False, True):
            A = pkg.DeviceMatrix(R.s)
            plan = (lambda w, r: A.optimize_sweep_device(None, w, r)) if device else (lambda w, r: A.optimize_sweep(R.s, w, r))
            assert plan(10, 1024) == (3, 3) and A.plan_info() == (2, 3, 3)
            R.spmv(t, A, ("sweep plan", device))
            assert plan(8, 256) == (12, 0)
            assert A.plan_info()[0] == 0
            R.spmv(t, A, ("declined", device)); cases += 1
    assert cases == 2


# ------------------------------------------------------------------------------------------------ 3. SpMMV, one precision
def _block_sweeps(b, itemsize, wlog, rowwise, ld):
    """the block window sweep's launcher takes row-major X always, column-major X in whole 16-byte pieces per column and windows of at
    least one wave instruction per column"""
    vw = 16 // itemsize
    return rowwise or (ld % vw == 0 and (1 << wlog) >= 64 * vw)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,C,sigma", [("block", 32, 512), ("block", 64, 1), ("halo", 32, 512)])
def test_spmmv_every_handle(pkg, t, rects, name, C, sigma, dt):
    """64-byte X rows (dp b = 8, sp b = 16) and a generic width (3, 5), both layouts, ld in {x rows, + 1, + 24} -- all of them > the
    padded rows, because X needs them: no plan (gather kernel 3), host and device block plans (phased kernel 8), the plan streamed with
    prefetch depth 1 and 2 (kernel 10, C = 32), "spmmv_xcol" (kernel 8 on the caller's column-major X: x_pass 0), "spmmv_xline" (on these
    shapes the planner turns the line plan down -- LINE_PLAN -- and the re-layout pass answers; the line arm itself runs in
    test_line_plan_beyond_the_padded_rows), the block window sweep at two windows (kernel 9); the generic width runs kernel 1 on every
    handle.  The device builder's plan equals the host planner's, asked for the same plan, array for array (digests).  Column-major X
    re-laid out once (uspmv_spmmv_x_prepared) gives the same bits with x_pass 2.  A poison in the X rows x_rows .. ld - 1 of an ld the
    sweep kernel takes changes nothing."""
    R = rects(name, C, sigma, dt)
    R.preconditions()
    s, size = R.s, R.np_dtype().itemsize
    wide, odd = 64 // size, 3 if dt == "f64" else 5
    vw = 16 // size
    shapes = [(rw, ld) for ld in R.lds() for rw in (1, 0)]
    assert all(ld > R.n for _, ld in shapes)
    if name == "block":
        assert R.x_rows % vw != 0                                  # column-major columns start off the 16-byte grid at ld = x rows
    cases = 0

    def grid(A, b, expect, tag, prepared=False):
        nonlocal cases
        for rw, ld in shapes:
            path, dX = R.spmmv(t, A, b, rw, ld, tag)
            assert path == expect(rw, ld), (tag, b, rw, ld, path, expect(rw, ld))
            if prepared and not rw and path[1] == 1:
                pkg.spmmv_x_prepared(A, dX, b, ld)
                p2, _ = R.spmmv(t, A, b, rw, ld, tag + ("prepared",), dX=dX)
                pkg.spmmv_x_release(A)
                assert p2 == (path[0], 2), (tag, b, ld, p2)
            cases += 1

    # ---- no plan
    N = pkg.DeviceMatrix(s)
    assert N.spmmv_last_path() == (0, 0)
    grid(N, wide, lambda rw, ld: (3, 0 if rw else 1), ("no plan",), prepared=True)
    grid(N, odd, lambda rw, ld: (1, 0), ("no plan",))
    # ---- block plans
    A = pkg.DeviceMatrix(s); A.optimize_block(s, wide)
    D = pkg.DeviceMatrix(s); D.optimize_block_device(wide)
    ia, idv = A.block_plan_info(), D.block_plan_info()
    assert ia["phased_plan"] == idv["phased_plan"] == 1 and ia["tiles"] == idv["tiles"] == -(-R.n // 64), (ia, idv)
    assert (ia["device_built"], idv["device_built"]) == (0, 1)
    for what, H in (("host block plan", A), ("device block plan", D)):
        grid(H, wide, lambda rw, ld: (8, 0 if rw else 1), (what,), prepared=True)
    # ---- the device builder against the host planner asked for the same plan (ties undone, phases filled to the brim): every array
    with tuned(pkg, spmmv_reorder=1, spmmv_phase_dp=0):
        built = {}
        for dev in (0, 1):
            with tuned(pkg, block_plan_device=dev):
                H = pkg.DeviceMatrix(s); H.optimize_block_device(wide)
            info = H.block_plan_info()
            assert info["phased_plan"] == 1 and info["device_built"] == dev and info["tiles"] == -(-R.n // 64), (dev, info)
            info.pop("device_built")
            built[dev] = (H.block_plan_digest(), info)
            grid(H, wide, lambda rw, ld: (8, 0 if rw else 1), ("optimize_block_device, block_plan_device", dev))
        assert built[0][1] == built[1][1], (built[0][1], built[1][1])
        assert built[0][0] == built[1][0], [k for k in range(8) if built[0][0][k] != built[1][0][k]]
    Ao = pkg.DeviceMatrix(s); Ao.optimize_block(s, odd)
    Do = pkg.DeviceMatrix(s); Do.optimize_block_device(odd)
    for what, H in (("host block plan", Ao), ("device block plan", Do)):
        grid(H, odd, lambda rw, ld: (1, 0), (what,))
    # ---- the plan walked as a stream
    for depth in (1, 2):
        with tuned(pkg, spmmv_stream=4, spmmv_stream_depth=depth):
            S4 = pkg.DeviceMatrix(s); S4.optimize_block(s, wide)
            info = S4.block_plan_info()
            if C == 32:
                assert info["stream_grid"] > 0 and info["stream_descriptors"] >= info["phases"], info
            else:
                assert info["stream_grid"] == 0, info                                   # (the streamed kernel is written for C = 32)
            k = 10 if C == 32 else 8
            grid(S4, wide, lambda rw, ld: (k, 0 if rw else 1), ("streamed, depth", depth))
    # ---- column-major X staged by the phased kernel itself
    with tuned(pkg, spmmv_xline=1):
        L = pkg.DeviceMatrix(s); L.optimize_block(s, wide)
        info = L.block_plan_info()
        # scattered columns: the lines would stage more than twice the rows, the planner keeps the row plan and the re-layout pass answers
        assert info["line_plan"] == LINE_PLAN[(name, C, sigma)][dt == "f32"] == 0 and info["phased_plan"] == 1, info
        grid(L, wide, lambda rw, ld: (8, 0 if rw else 1), ("spmmv_xline, line plan turned down",))
    with tuned(pkg, spmmv_xcol=1):
        grid(A, wide, lambda rw, ld: (8, 0), ("spmmv_xcol",))
    # ---- the block window sweep
    for wlog in (9, 11):
        W = pkg.DeviceMatrix(s)
        with tuned(pkg, sweep_max_stage=1 << 20):
            nt, nsw = W.optimize_block_sweep(s, wide, wlog, 1024)
        assert nt == nsw == -(-R.n // 1024), (wlog, nt, nsw)
        grid(W, wide, lambda rw, ld: (9, 0) if _block_sweeps(wide, size, wlog, rw, ld) else (3, 1), ("block sweep", wlog))
    # ---- a poison behind the x rows of every column
    # (an ld in whole 16-byte pieces for dp and sp, so that the sweep kernel -- W: windows of 2^11 rows -- stages the poisoned rows itself)
    ld = -(-R.x_rows // 4) * 4 + 24
    assert ld % vw == 0 and _block_sweeps(wide, size, 11, 0, ld)
    X, want, cols = R.case(wide, 0, ld)
    poison = 1e300 if dt == "f64" else 1e30
    Xp = _block_x(cols, wide, ld, False, fill=poison)
    assert int((Xp == R.np_dtype(poison)).sum()) == (ld - R.x_rows) * wide >= 24 * wide
    for what, H, k in (("no plan", N, (3, 1)), ("host block plan", A, (8, 1)), ("block sweep", W, (9, 0))):
        dY = t.full((wide * ld + GUARD,), FILL, dtype=H.torch_dtype, device="cuda")
        pkg.spmmv(H, t.from_numpy(Xp).cuda(), dY, wide, ld, pkg.COLWISE)
        assert H.spmmv_last_path() == k, (what, H.spmmv_last_path(), k)
        _check(dY.cpu().numpy(), want, (name, C, dt, "poisoned X", what))
        cases += 1
    assert cases == 6 * 14 + 3


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("C", [32, 64])
def test_line_plan_beyond_the_padded_rows(pkg, t, rects, C, dt):
    """"spmmv_xline" 1 on the mesh row block at sigma = 1, where the planner KEEPS the line plan (asserted): the phased kernel stages
    column-major X by 128-byte lines of columns that are 8097 rows long and more -- lines far beyond the padded rows, the last line of a
    column cut by x rows -- wherever ld leaves the columns in whole 16-byte pieces (kernel 8, x_pass 0); other ld go through the
    re-layout pass (x_pass 1), row-major X is staged by rows.  A poison behind the x rows of every column changes nothing."""
    R = rects("mesh", C, 1, dt)
    R.preconditions()
    size = R.np_dtype().itemsize
    wide, vw = 64 // size, 16 // size
    lds = R.lds() + (-(-R.x_rows // 4) * 4 + 24,)
    cases = lined = 0
    with tuned(pkg, spmmv_xline=1):
        L = pkg.DeviceMatrix(R.s); L.optimize_block(R.s, wide)
        info = L.block_plan_info()
        assert info["line_plan"] == LINE_PLAN[("mesh", C, 1)][dt == "f32"] == 1 and info["phased_plan"] == 1, info
        assert info["line_phases"] >= info["tiles"] == -(-R.n // 64) and info["line_rows_staged"] > 0, info
        for ld in lds:
            for rw in (1, 0):
                want = (8, 0 if rw or ld % vw == 0 else 1)
                path, _ = R.spmmv(t, L, wide, rw, ld, ("line plan",))
                assert path == want, (rw, ld, path, want)
                lined += (not rw) and want == (8, 0); cases += 1
        ld = lds[-1]
        X, want, cols = R.case(wide, 0, ld)
        poison = 1e300 if dt == "f64" else 1e30
        Xp = _block_x(cols, wide, ld, False, fill=poison)
        assert int((Xp == R.np_dtype(poison)).sum()) == (ld - R.x_rows) * wide
        dY = t.full((wide * ld + GUARD,), FILL, dtype=L.torch_dtype, device="cuda")
        pkg.spmmv(L, t.from_numpy(Xp).cuda(), dY, wide, ld, pkg.COLWISE)
        assert L.spmmv_last_path() == (8, 0)
        _check(dY.cpu().numpy(), want, ("mesh", C, dt, "poisoned X, line plan")); cases += 1
    assert cases == 9 and lined == (2 if dt == "f64" else 1)


# ------------------------------------------------------------------------------------------------ 4, 5. adaptive precision
class RectSplit:
    """One split of one matrix -- structs (hi, mid | None, lo), columns permuted with the first part's permutation -- with x of exactly
    x_rows elements (1 + the highest column of ANY part), 8 columns of X (column v = xp * (1 + v / 8)) and the oracle's columns of Y"""

    def __init__(self, pkg, orc, name, m, kind, C, sigma):
        self.pkg, self.orc, self.name, self.kind, self.C, self.sigma = pkg, orc, name, kind, C, sigma
        if kind == "dp_sp":
            ds, ss = _pair_structs(pkg, m, C, sigma, th=TH_PAIR)
            self.structs = (ds, None, ss)
        else:
            built = _build(pkg, m, kind, C, sigma, *TH_HP)
            assert built is not None, (name, kind, C, sigma, "a conversion was refused")
            self.structs = built[0]
        sh = self.structs[0]
        self.n, self.n_rows = sh.n_rows_padded, m.n_rows
        self.dtype = np.float32 if kind == "sp_hp" else np.float64
        self.x_dtype = pkg.F32 if kind == "sp_hp" else pkg.F64
        self.x_rows_part = [1 + int(s.arrays()["col_idxs"].max()) for s in self.structs if s is not None]
        self.x_rows = max(self.x_rows_part)
        self.xp = _x(self.x_rows, m.n_rows, self.dtype)
        self.xcols = [(self.xp * self.dtype(1.0 + v / 8.0)).astype(self.dtype) for v in range(8)]
        self.ycols = [self.oracle(x) for x in self.xcols]
        self._case = {}

    def oracle(self, x):
        if self.kind != "dp_sp":
            return _oracle(self.orc, self.kind, self.structs, x)
        parts = tuple((q["chunk_ptrs"], q["chunk_lengths"], q["col_idxs"], q["values"]) for q in (self.structs[0].arrays(), self.structs[2].arrays()))
        return self.orc.spmv_scs_ap_adv(self.C, self.structs[0].n_chunks, parts[0], parts[1], x)

    def preconditions(self):
        _, n, nc, n_pad = MATRICES[self.name]
        for s in self.structs:
            assert s is None or (s.nnz > 0 and s.n_elements > 0 and s.n_rows_padded == n_pad and s.n_rows == n != nc), (self.kind, "an empty part")
        assert (self.structs[1] is not None) == (self.kind == "dp_sp_hp")
        xr = self.x_rows
        if self.name == "block":
            # a planner that took x_len from the first part alone would pass every square test
            assert xr == BLOCK_X_ROWS and self.x_rows_part[0] == BLOCK_X_ROWS_FIRST < xr
            assert xr > self.n and xr % 2 == 1 and xr % 4 != 0
            for wlog, rows in SWEEP_SHAPES:
                assert xr % (1 << wlog) != 0 and self.n % rows != 0
        else:
            assert xr == nc > self.n

    def handles(self):
        return [self.pkg.DeviceMatrix(s) if s is not None else None for s in self.structs]

    def shapes(self):
        return [(rw, ld) for ld in (self.x_rows, self.x_rows + 1, self.x_rows + 24) for rw in (1, 0)]

    def case(self, b, rowwise, ld):
        key = (b, rowwise, ld)
        if key not in self._case:
            self._case[key] = (_block_x(self.xcols[:b], b, ld, rowwise), _block_want(self.ycols[:b], b, ld, rowwise))
        return self._case[key]

    def spmv(self, t, hand, tag, v=0):
        pkg = self.pkg
        dx = t.from_numpy(self.xcols[v]).cuda()
        assert dx.numel() == self.x_rows
        y = t.full((self.n + GUARD,), FILL, dtype=hand[0].torch_dtype, device="cuda")
        if self.kind == "dp_sp": pkg.spmv_ap(hand[0], hand[2], dx, y)
        else: pkg.spmv_ap_hp(hand[0], hand[1], hand[2], dx, y)
        want = np.concatenate([self.ycols[v], np.full(GUARD, FILL, self.dtype)])
        _check(y.cpu().numpy(), want, (self.name, self.kind, self.C, self.sigma) + tuple(tag))

    def path(self, hand, b, ld, rowwise):
        pkg, lay = self.pkg, self.pkg.ROWWISE if rowwise else self.pkg.COLWISE
        if self.kind == "dp_sp": return pkg.spmmv_ap_path(hand[0], hand[2], b, ld, lay)
        return pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, lay)

    def spmmv(self, t, hand, b, rowwise, ld, tag):
        pkg, lay = self.pkg, self.pkg.ROWWISE if rowwise else self.pkg.COLWISE
        X, want = self.case(b, rowwise, ld)
        dX = t.from_numpy(X).cuda()
        assert dX.numel() == b * ld and ld >= self.x_rows
        dY = t.full((b * ld + GUARD,), FILL, dtype=hand[0].torch_dtype, device="cuda")
        if self.kind == "dp_sp": pkg.spmmv_ap(hand[0], hand[2], dX, dY, b, ld, lay)
        else: pkg.spmmv_ap_hp(hand[0], hand[1], hand[2], dX, dY, b, ld, lay)
        _check(dY.cpu().numpy(), want, (self.name, self.kind, self.C, self.sigma, b, "rowwise" if rowwise else "colwise", ld) + tuple(tag))

    def vectors(self, b, wlog):
        if self.kind == "dp_sp": return self.pkg.spmmv_ap_sweep_vectors(b, wlog)
        return self.pkg.spmmv_ap_hp_sweep_vectors(b, wlog, self.x_dtype)

    def aligned(self, rowwise, ld):
        """column-major X in whole 16-byte pieces per column (what the staged and the sweep kernels stage by)"""
        return bool(rowwise) or (ld * np.dtype(self.dtype).itemsize) % 16 == 0

    def plan_tiles(self, hand, device):
        """the shared tile-local-column plan; returns the lines of its fullest tile"""
        pkg = self.pkg
        if self.kind == "dp_sp":
            nt, ns = pkg.optimize_device_ap(hand[0], hand[2]) if device else pkg.optimize_ap(hand[0], hand[2], self.structs[0], self.structs[2])
        else:
            nt, ns = pkg.optimize_device_ap_hp(*hand) if device else pkg.optimize_ap_hp(*hand, *self.structs)
        assert nt == ns > 0, (self.kind, device, nt, ns)
        assert [h.plan_info() for h in hand if h is not None] == [(1, nt, ns)] * (3 if hand[1] is not None else 2)
        return hand[0].plan_download()["max_lines_used"]

    def plan_sweep(self, hand, wlog, rows, device):
        """the shared sweep plan under "sweep_max_stage" 1 << 20; returns (tiles, sweep tiles)"""
        pkg = self.pkg
        with tuned(pkg, sweep_max_stage=1 << 20):
            if self.kind == "dp_sp":
                if device: return hand[0].optimize_sweep_device(hand[2], wlog, rows)
                return pkg.optimize_sweep_ap(hand[0], hand[2], self.structs[0], self.structs[2], wlog, rows)
            if device: return pkg.optimize_sweep_device_ap_hp(*hand, wlog, rows)
            return pkg.optimize_sweep_ap_hp(*hand, *self.structs, wlog, rows)

    def tile_path(self, lines, b, rowwise, ld):
        """(path, vectors) on the shared line plan: the staged kernel; the pair reaches it through the re-layout pass whatever ld is, the
        kinds with an fp16 part stage the caller's columns and want them in 16-byte pieces"""
        bs = _bs_rule(lines, np.dtype(self.dtype).itemsize, b)
        if self.kind == "dp_sp":
            return (2, bs)
        return (2, bs) if bs and self.aligned(rowwise, ld) else (0, 0)

    def sweep_path(self, b, wlog, rowwise, ld):
        if self.aligned(rowwise, ld):
            return _expected_path(self.pkg, self, b, wlog, rowwise)
        return (GATHER, 0) if self.kind == "dp_sp" else (0, 0)


@pytest.fixture(scope="module")
def splits(pkg, orc, t, mats):
    cache = {}

    def get(name, kind, C, sigma):
        if (name, kind, C, sigma) not in cache:
            cache[(name, kind, C, sigma)] = RectSplit(pkg, orc, name, mats(name), kind, C, sigma)
        return cache[(name, kind, C, sigma)]
    return get


@pytest.mark.parametrize("C,sigma", CSIG[:3])
@pytest.mark.parametrize("name", ["block", "halo"])
@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_precision_every_plan(pkg, t, splits, kind, name, C, sigma):
    """ap[dp_sp] and the three kinds with an fp16 part: the single-vector product plain, on the shared line plan and on the shared sweep
    plan at three shapes, each from the host and from the device (equal plans); the block product at b in {2, 4, 8}, both layouts,
    ld in {x rows, + 1, + 24}, on the host's line plan and on the host's sweep plans, with the path the dispatch names asserted first:
    staged (2), sweep (3), and where a column-major ld leaves the columns off 16 bytes or the window leaves no room for two vectors the
    pair's gather kernel (1) or the generic kernel (0)"""
    S = splits(name, kind, C, sigma)
    S.preconditions()
    cases, swept, staged = 0, 0, 0
    S.spmv(t, S.handles(), ("plain",)); cases += 1
    # ---- the shared line plan
    H, D = S.handles(), S.handles()
    lines = S.plan_tiles(H, False)
    assert S.plan_tiles(D, True) == lines
    assert [h.plan_info() for h in H if h is not None] == [h.plan_info() for h in D if h is not None]
    for v in (0, 3):
        S.spmv(t, H, ("host line plan", v), v); S.spmv(t, D, ("device line plan", v), v)
    cases += 2
    for b in (2, 4, 8):
        assert _bs_rule(lines, np.dtype(S.dtype).itemsize, b) >= 2, (lines, b)      # (two vectors of the fullest tile fit: the staged kernel applies)
        for rw, ld in S.shapes():
            want = S.tile_path(lines, b, rw, ld)
            assert S.path(H, b, ld, rw) == want, ("line plan", b, rw, ld, S.path(H, b, ld, rw), want)
            S.spmmv(t, H, b, rw, ld, ("line plan", lines))
            staged += want[0] == 2; cases += 1
    S.spmmv(t, D, 4, 0, S.x_rows + 1, ("device line plan", lines)); cases += 1
    # ---- the shared sweep plan
    for wlog, rows in SWEEP_SHAPES:
        H, D = S.handles(), S.handles()
        got = S.plan_sweep(H, wlog, rows, False), S.plan_sweep(D, wlog, rows, True)
        nt = -(-S.n // rows)
        if not sweeps(name, sigma, wlog):
            assert got == ((nt, 0), (nt, 0)), (wlog, rows, got)
            assert all(h.plan_info()[0] == 0 for h in H + D if h is not None)
            S.spmv(t, H, ("declined sweep", wlog)); S.spmmv(t, H, 4, 0, S.x_rows + 1, ("declined sweep", wlog)); cases += 1
            continue
        assert got == ((nt, nt), (nt, nt)), (wlog, rows, got)
        assert all(h.plan_info() == (2, nt, nt) for h in H + D if h is not None)
        _same_sweep_plans(H, D)
        assert H[0].sweep_plan_digest()[1][1:3] == [rows, wlog]
        assert S.path(H, 1, S.x_rows, 0) == (SWEEP, 1)
        for v in (0, 5):
            S.spmv(t, H, ("host sweep plan", wlog, v), v); S.spmv(t, D, ("device sweep plan", wlog, v), v)
        cases += 1
        for b in (2, 4, 8):
            vec = lds_vectors(b, wlog, np.dtype(S.dtype).itemsize)
            assert vec >= 2 and S.vectors(b, wlog) == vec, (b, wlog, vec, S.vectors(b, wlog))
            for rw, ld in S.shapes():
                want = S.sweep_path(b, wlog, rw, ld)
                assert S.path(H, b, ld, rw) == want, ("sweep plan", wlog, b, rw, ld, S.path(H, b, ld, rw), want)
                S.spmmv(t, H, b, rw, ld, ("sweep plan", wlog, rows))
                swept += want[0] == SWEEP; cases += 1
        S.spmmv(t, D, 4, 0, S.x_rows + 1, ("device sweep plan", wlog)); cases += 1
    n_sweeps = sum(sweeps(name, sigma, w) for w, _ in SWEEP_SHAPES)
    assert cases == 1 + 2 + 18 + 1 + n_sweeps * 20 + (3 - n_sweeps)
    # how often the kernels under test must have answered, from the shapes alone: of the 6 (layout, ld) 3 are row-major and the
    # column-major ones count where ld leaves whole 16-byte pieces; the pair's staged kernel takes every ld (re-layout pass), its sweep
    # kernel leaves row-major X in more than two passes to the gather kernel (b = 8 at two vectors per pass: windows of 2^13 doubles)
    ok = 3 + sum(S.aligned(0, ld) for ld in (S.x_rows, S.x_rows + 1, S.x_rows + 24))
    assert ok == {("block", 8): 4, ("block", 4): 4, ("halo", 8): 5, ("halo", 4): 3}[(name, np.dtype(S.dtype).itemsize)]
    assert staged == (18 if kind == "dp_sp" else 3 * ok), (staged, ok)
    want_swept = sum(3 * ok - (3 if kind == "dp_sp" and wlog == 13 else 0) for wlog, _ in SWEEP_SHAPES if sweeps(name, sigma, wlog))
    assert swept == want_swept, (swept, want_swept)


# ------------------------------------------------------------------------------------------------ 6. set-up on the device
@pytest.mark.parametrize("C,sigma", [(32, 512), (8, 64)])
@pytest.mark.parametrize("name", ["block", "halo", "tall"])
def test_device_setup_equals_the_host_route(pkg, orc, t, mats, rects, name, C, sigma):
    """uspmv_convert_to_scs_device, the conversion from device-resident COO arrays (the reference's tie order with and without the column
    permutation, the stable device ordering), uspmv_partition_precisions_device and the one-call adaptive-precision set-up for all four
    kinds: arrays, permutations and counts bit-identical to the host route, the columns >= n_rows untouched by the column permutation,
    and one planned product each against the oracle"""
    m, R = mats(name), rects(name, C, sigma, "f64")
    R.preconditions()
    n, nc, a, cases = m.n_rows, m.n_cols, R.a, 0

    def same_arrays(A, want, tag):
        d = pkg.dmat_download(A)
        for k in ("chunk_ptrs", "chunk_lengths", "col_idxs"):
            assert np.array_equal(d[k], want[k]), (name, C, sigma, tag, k)
        assert np.array_equal(bits(d["values"]), bits(want["values"])), (name, C, sigma, tag)
        return d

    lay, A = pkg.convert_to_scs_device(m, C, sigma, pkg.F64)
    assert np.array_equal(lay.arrays()["old_to_new_idx"], R.perm)
    same_arrays(A, a, "convert_to_scs_device")
    A.optimize_device()
    assert A.plan_info()[0] == 1
    R.spmv(t, A, ("convert_to_scs_device + device plan",)); cases += 1

    dI, dJ, dV = dev_coo(t, m)
    assert np.all(np.diff(np.asarray(m.arrays()[0])) >= 0)
    lay, A, o2n, n2o = pkg.convert_to_scs_device_from_arrays(dI, dJ, dV, n, nc, C, sigma, pkg.F64)
    assert np.array_equal(o2n.cpu().numpy(), R.perm) and np.array_equal(n2o.cpu().numpy(), a["new_to_old_idx"])
    d1 = same_arrays(A, a, "from arrays")
    A.optimize_device()
    assert A.plan_info()[0] == 1
    R.spmv(t, A, ("from arrays + device plan",)); cases += 1
    # without the column permutation: the host struct before permute_scs_cols; the permutation moves the columns < n_rows and no other
    s0 = pkg.convert_to_scs(m, C, sigma, pkg.F64)
    lay, A0, o2n0, _ = pkg.convert_to_scs_device_from_arrays(dI, dJ, dV, n, nc, C, sigma, pkg.F64, permute_cols=False)
    assert np.array_equal(o2n0.cpu().numpy(), R.perm)
    d0 = same_arrays(A0, s0.arrays(), "from arrays, permute_cols False")
    c0, c1 = d0["col_idxs"], d1["col_idxs"]
    beyond = c0 >= n
    assert beyond.any() == (nc > n) and np.array_equal(c1[beyond], c0[beyond])
    assert np.array_equal(c1[~beyond], R.perm[c0[~beyond]])
    x0 = _x(1 + int(c0.max()), n, np.float64)
    want0 = np.concatenate([orc.spmv_scs(C, s0.n_chunks, d0["chunk_ptrs"], d0["chunk_lengths"], c0, d0["values"], x0), np.full(GUARD, FILL)])
    A0.optimize_device()
    y = t.full((R.n + GUARD,), FILL, dtype=t.float64, device="cuda")
    pkg.spmv(A0, t.from_numpy(x0).cuda(), y)
    _check(y.cpu().numpy(), want0, (name, C, sigma, "permute_cols False")); cases += 1
    # the stable device ordering: another tie order, the same chunk layout; its product against the oracle on its own arrays
    lay7, A7, o2n7, n2o7 = pkg.convert_to_scs_device_from_arrays(dI, dJ, dV, n, nc, C, sigma, pkg.F64, sort=pkg.SORT_DEVICE_STABLE)
    d7 = pkg.dmat_download(A7)
    assert np.array_equal(d7["chunk_ptrs"], a["chunk_ptrs"]) and np.array_equal(d7["chunk_lengths"], a["chunk_lengths"])
    beyond7 = d7["col_idxs"] >= max(n, R.n)
    assert np.array_equal(np.sort(d7["col_idxs"][beyond7]), np.sort(c0[c0 >= max(n, R.n)]))
    x7 = _x(1 + int(d7["col_idxs"].max()), n, np.float64)
    want7 = np.concatenate([orc.spmv_scs(C, s0.n_chunks, d7["chunk_ptrs"], d7["chunk_lengths"], d7["col_idxs"], d7["values"], x7), np.full(GUARD, FILL)])
    A7.optimize_device()
    y = t.full((R.n + GUARD,), FILL, dtype=t.float64, device="cuda")
    pkg.spmv(A7, t.from_numpy(x7).cuda(), y)
    _check(y.cpu().numpy(), want7, (name, C, sigma, "stable device ordering")); cases += 1

    # ---- adaptive precision
    for kind in KINDS:
        t1, t2 = (TH_PAIR, 0.0) if kind == "dp_sp" else TH_HP
        if name == "tall":                                          # (its values span the same decades)
            assert np.abs(np.asarray(m.arrays()[2])).min() < t1 < np.abs(np.asarray(m.arrays()[2])).max()
        same_parts(pkg, t, m, kind, t1, t2, (dI, dJ, dV))
        structs = host_structs(pkg, host_parts(pkg, m, kind, t1, t2), kind, C, sigma)
        assert (structs is None) == ((name, C, sigma, kind) in HOST_REFUSES), (name, kind, C, sigma)
        if structs is None:
            # the reference's tie order parks a row without a dp entry behind n_rows, where its sp entries would overrun a chunk of length
            # 0: the host route refuses (found on the CPU); the device route must refuse in the same words, and take the stable ordering
            with pytest.raises(pkg.UspmvError, match="fixed_permutation maps a non-empty row onto a padded slot"):
                pkg.convert_ap_device_from_arrays(dI, dJ, dV, n, nc, C, sigma, kind, t1, t2)
            _, hand, _, _, cnt = pkg.convert_ap_device_from_arrays(dI, dJ, dV, n, nc, C, sigma, kind, t1, t2, sort=pkg.SORT_DEVICE_STABLE)
            assert cnt == [p.nnz for p in host_parts(pkg, m, kind, t1, t2)] and all(c > 0 for c in cnt)
            down = [pkg.dmat_download(h) for h in hand]
            x = _x(max(1 + int(d["col_idxs"].max()) for d in down), n, np.float64)
            ch = [orc.spmv_scs(C, hand[0].n_chunks, d["chunk_ptrs"], d["chunk_lengths"], d["col_idxs"], d["values"].astype(np.float64), x) for d in down]
            nt, ns = pkg.optimize_device_ap_hp(*hand)
            assert nt == ns > 0
            y = t.full((R.n + GUARD,), FILL, dtype=t.float64, device="cuda")
            pkg.spmv_ap_hp(hand[0], hand[1], hand[2], t.from_numpy(x).cuda(), y)
            _check(y.cpu().numpy(), np.concatenate([(ch[0] + ch[1]) + ch[2], np.full(GUARD, FILL)]), (name, kind, C, sigma, "stable ordering"))
            cases += 1
            continue
        lay, hand, o2n, n2o, cnt = pkg.convert_ap_device_from_arrays(dI, dJ, dV, n, nc, C, sigma, kind, t1, t2)
        same_handles(pkg, structs, hand, (name, kind, C, sigma))
        assert cnt == [s.nnz if s is not None else 0 for s in structs] and all(c > 0 for c, s in zip(cnt, structs) if s is not None)
        h0 = structs[0].arrays()
        assert np.array_equal(o2n.cpu().numpy(), h0["old_to_new_idx"]) and np.array_equal(n2o.cpu().numpy(), h0["new_to_old_idx"])
        for s, s_one in zip(structs, host_structs_unpermuted(pkg, host_parts(pkg, m, kind, t1, t2), kind, C, sigma)):
            if s is not None:
                u, p = s_one.arrays()["col_idxs"], s.arrays()["col_idxs"]
                assert np.array_equal(p[u >= n], u[u >= n]) and (u >= n).any() == (nc > n)
        x_rows = max(1 + int(s.arrays()["col_idxs"].max()) for s in structs if s is not None)
        dtype = np.float32 if kind == "sp_hp" else np.float64
        x = _x(x_rows, n, dtype)
        if kind == "dp_sp":
            parts = tuple((q["chunk_ptrs"], q["chunk_lengths"], q["col_idxs"], q["values"]) for q in (structs[0].arrays(), structs[2].arrays()))
            want = orc.spmv_scs_ap_adv(C, structs[0].n_chunks, parts[0], parts[1], x)
            nt, ns = pkg.optimize_device_ap(hand[0], hand[2])
        else:
            want = _oracle(orc, kind, tuple(structs), x)
            nt, ns = pkg.optimize_device_ap_hp(*hand)
        assert nt == ns > 0 and all(h.plan_info() == (1, nt, ns) for h in hand if h is not None)
        y = t.full((R.n + GUARD,), FILL, dtype=hand[0].torch_dtype, device="cuda")
        dx = t.from_numpy(x).cuda()
        assert dx.numel() == x_rows
        if kind == "dp_sp": pkg.spmv_ap(hand[0], hand[2], dx, y)
        else: pkg.spmv_ap_hp(hand[0], hand[1], hand[2], dx, y)
        _check(y.cpu().numpy(), np.concatenate([want, np.full(GUARD, FILL, dtype)]), (name, kind, C, sigma, "device set-up + device plan"))
        cases += 1
    assert cases == 8


def host_structs_unpermuted(pkg, parts, kind, C, sigma):
    """the structs of host_structs() before permute_scs_cols"""
    dts = part_dtypes(pkg, kind)
    s0 = pkg.convert_to_scs(parts[0], C, sigma, dts[0])
    perm = s0.arrays()["old_to_new_idx"].copy()
    return [s0] + [pkg.convert_to_scs(p, C, sigma, dt, fixed_permutation=perm) if p is not None else None for p, dt in zip(parts[1:], dts[1:])]
