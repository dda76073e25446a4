"""SpMMV of the fp16 adaptive-precision kinds on the parts' shared column-window sweep plan (csrc/ap_hp_spmmv_sweep.hip,
scs_spmmv_ap_hp_sweep): b in {2, 4, 8, 16} right-hand sides walk the plan's compacted streams once per pass.  The contract is the
project's usual one -- same bits: column v of Y is what the oracle composed part by part (the helpers of tests/test_gpu_sweep_ap_hp.py)
and uspmv_spmv_ap_hp give for column v of X, for every kind, every plan shape (rows per lane 1, 2 and 4; 8, 4 and 2 vectors per pass;
one and several passes; one and two LDS buffers), both layouts, a padded leading dimension, partial coverage (rest chunks),
device-built plans and special values.  No tolerance anywhere; a NaN equals any NaN in the same place.  uspmv_spmmv_ap_hp_path must
say which kernel ran.

The matrix, gen_banded_random(16384, 40, 1500), has a multiple of 128 rows, so no row slot is padded and no conversion is declined:
every test counts its cases.  Its band spans about 3000 columns: several windows per tile at wlog 8-11, two at 12, one at 13-14."""
import numpy as np
import pytest

from conftest import block_x, make_x

pytestmark = pytest.mark.gpu
KINDS = ("dp_hp", "sp_hp", "dp_sp_hp")
SHAPES = ((32, 512), (64, 64))
GUARD = 64
WIDTHS = (2, 4, 8, 16)
SWEEP = 3
# (wlog, tile rows): threads 256 / rows per lane 1, 1024 / 1, 1024 / 2, 1024 / 4, and the default tile on the widest window that holds two
# double vectors; (14, 0) is that window for float X
PLANS = ((11, 256), (12, 1024), (12, 2048), (12, 4096), (13, 0), (14, 0))
DEFAULTS = dict(nontemporal=1, spmmv_variant=0, tlc=1, sweep=1, sweep_nbuf=1, sweep_unroll=8, sweep_pair=2, sweep_remap=8, sweep_threads=0,
                sweep_wlog=0, sweep_tile_rows=0, sweep_max_stage=0, tlc_tile_rows=0)


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert pkg.device_count() >= 1
    torch.cuda.set_device(0)
    pkg.set_tuning(**DEFAULTS)
    yield torch
    pkg.set_tuning(**DEFAULTS)


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


def _same(got, want):
    """bit for bit, except that a NaN equals any NaN (the sign and payload of a NaN made by inf - inf differ between CPU and GPU; an hp part
    whose values overflow binary16 to +-inf makes such rows)"""
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return np.array_equal(got[~nan].view(u), want[~nan].view(u))


class BlockSplit:
    """One split of one matrix, its X of n_oracle columns (column v = xp * (1 + v / 8), what conftest.block_x lays out) and the oracle's
    columns of Y, computed once; the expected Y of every (b, layout, ld) is kept."""

    def __init__(self, pkg, orc, m, kind, C, sigma, n_oracle=16):
        t1, t2 = _thresholds(m)
        b = _build(pkg, m, kind, C, sigma, t1, t2)
        assert b is not None, (kind, C, sigma)
        self.structs, _ = b
        sh = self.structs[0]
        self.pkg, self.kind, self.C, self.n = pkg, kind, C, sh.n_rows_padded
        self.dtype = np.float32 if kind == "sp_hp" else np.float64
        self.x_dtype = pkg.F32 if kind == "sp_hp" else pkg.F64
        xp = np.zeros(self.n)
        xp[:m.n_rows] = make_x(m.n_rows)[sh.arrays()["new_to_old_idx"]]
        self.xp = xp.astype(self.dtype)
        self.xcols = [(self.xp * self.dtype(1.0 + v / 8.0)).astype(self.dtype) for v in range(n_oracle)]      # column v of block_x
        self.ycols = [_oracle(orc, kind, self.structs, x) for x in self.xcols]
        self._case = {}

    def handles(self):
        return [self.pkg.DeviceMatrix(s) if s is not None else None for s in self.structs]

    def shapes(self):
        return [(1, self.n), (0, self.n), (0, self.n + 32)]

    def case(self, b, rowwise, ld):
        """(X, expected Y with 9.0 wherever the call must not write), both of b * ld + GUARD elements"""
        key = (b, rowwise, ld)
        if key not in self._case:
            n = self.n
            X = np.concatenate([block_x(self.xp, n, b, ld, rowwise), np.zeros(GUARD, self.dtype)])
            want = np.full(b * ld + GUARD, 9.0, self.dtype)
            for v in range(b):
                if rowwise: want[v:n * b:b] = self.ycols[v]
                else: want[v * ld:v * ld + n] = self.ycols[v]
            self._case[key] = (X, want)
        return self._case[key]

    def run(self, t, hand, b, rowwise, ld, offset=0, tag=""):
        """one call into a Y filled with 9.0 (+ guard zone); `offset` elements into freshly allocated buffers"""
        X, want = self.case(b, rowwise, ld)
        td = hand[0].torch_dtype
        dXb = t.zeros(len(X) + offset, dtype=td, device="cuda"); dX = dXb[offset:]; dX.copy_(t.from_numpy(X))
        dYb = t.full((len(want) + offset,), 9.0, dtype=td, device="cuda"); dY = dYb[offset:]
        if offset: assert dX.data_ptr() % 16 != 0 and dY.data_ptr() % 16 != 0
        self.pkg.spmmv_ap_hp(hand[0], hand[1], hand[2], dX, dY, b, ld, self.pkg.ROWWISE if rowwise else self.pkg.COLWISE)
        got = dY.cpu().numpy()
        if not _same(got, want):
            bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
            raise AssertionError(f"{self.kind} C={self.C} b={b} rowwise={rowwise} ld={ld} {tag}: {len(bad)} elements differ, first at "
                                 f"{bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}")
        if offset: assert float(dYb[0]) == 9.0
        return dX, dY


@pytest.fixture(scope="module")
def splits(pkg, orc, torch_cuda):
    m = pkg.gen_banded_random(16384, 40, 1500, magnitude_decades=10.0)
    cache = {}

    def get(kind, C, sigma):
        if (kind, C, sigma) not in cache:
            cache[(kind, C, sigma)] = BlockSplit(pkg, orc, m, kind, C, sigma)
            assert cache[(kind, C, sigma)].n == 16384
        return cache[(kind, C, sigma)]
    return get


def _plan(pkg, S, hand, wlog, rows, device=False):
    """install the parts' shared sweep plan (every tile sweeping, kind 2 on every part); returns the log2 of its window"""
    pkg.set_tuning(sweep_max_stage=1 << 20)          # (the stage-cost heuristic would decline so small a matrix at the wide windows)
    try:
        if device: nt_, nsw = pkg.optimize_sweep_device_ap_hp(hand[0], hand[1], hand[2], wlog, rows)
        else: nt_, nsw = pkg.optimize_sweep_ap_hp(hand[0], hand[1], hand[2], *S.structs, wlog, rows)
    finally:
        pkg.set_tuning(sweep_max_stage=0)
    assert nsw == nt_ > 0, (wlog, rows, nt_, nsw)
    assert [h.plan_info()[0] for h in hand if h is not None] == [2] * (3 if hand[1] is not None else 2)
    meta = hand[0].sweep_plan_digest()[1]
    assert meta[0] == 1 and (wlog == 0 or meta[2] == wlog) and (rows == 0 or meta[1] == rows), meta
    return int(meta[2])


def _expected_path(pkg, S, b, wlog, rowwise):
    """(path, vectors) of sweep-planned parts at a B-specialised width: the sweep kernel wherever two vectors of a window fit LDS, in one
    pass or several; else the generic kernel"""
    vec = pkg.spmmv_ap_hp_sweep_vectors(b, wlog, S.x_dtype)
    return (SWEEP, vec) if vec else (0, 0)


def _layout(pkg, rowwise):
    return pkg.ROWWISE if rowwise else pkg.COLWISE


def _bits(t, S):
    return t.int32 if S.kind == "sp_hp" else t.int64


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: f"wlog{p[0]}_rows{p[1]}")
@pytest.mark.parametrize("C,sigma", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_grid_bitexact(pkg, torch_cuda, splits, kind, C, sigma, plan):
    """every width x layout x leading dimension on every plan shape: path 3 with the vectors per pass uspmv_spmmv_ap_hp_sweep_vectors
    names (mandatory wherever that is b), the oracle's bits in every written element, 9.0 everywhere else (padded ld, guard zone); and
    column v = uspmv_spmv_ap_hp of column v on the same handles.  Both buffer counts and both load / store forms everywhere, their full
    product on the (12, 2048) plan."""
    t = torch_cuda
    S = splits(kind, C, sigma)
    if plan == (14, 0) and kind != "sp_hp":
        # 2^14 doubles: one vector fills the LDS, the block kernel stands back at every width -- checked without the grid
        hand = S.handles()
        assert _plan(pkg, S, hand, 14, 0) == 14
        for b in WIDTHS:
            for rowwise, ld in S.shapes():
                assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, _layout(pkg, rowwise)) == (0, 0)
        S.run(t, hand, 4, 1, S.n, tag="wlog 14, path 0")
        return
    hand = S.handles()
    wlog = _plan(pkg, S, hand, *plan)
    assert wlog == plan[0]
    full = plan == (12, 2048)
    bits = _bits(t, S)
    try:
        # the single-vector product of the 16 columns on these handles (its own sweep kernel): pinned to the oracle here
        ysp = []
        for v in range(16):
            y = t.full((S.n,), -3.0, dtype=hand[0].torch_dtype, device="cuda")
            pkg.spmv_ap_hp(hand[0], hand[1], hand[2], t.from_numpy(S.xcols[v]).cuda(), y)
            assert _same(y.cpu().numpy(), S.ycols[v]), ("spmv_ap_hp", v)
            ysp.append(y)
        k = cases = 0
        for b in WIDTHS:
            for rowwise, ld in S.shapes():
                path, vec = pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, _layout(pkg, rowwise))
                assert (path, vec) == _expected_path(pkg, S, b, wlog, rowwise), (b, rowwise, ld, wlog, path, vec)
                if pkg.spmmv_ap_hp_sweep_vectors(b, wlog, S.x_dtype) == b: assert (path, vec) == (SWEEP, b)      # single pass: mandatory
                combos = [(nb, nt) for nb in (1, 2) for nt in (1, 0)] if full else [((1, 1), (2, 0), (2, 1), (1, 0))[k % 4], ((2, 0), (1, 1), (1, 0), (2, 1))[k % 4]]
                k += 1
                for nbuf, nt in combos:
                    pkg.set_tuning(sweep_nbuf=nbuf, nontemporal=nt)
                    dX, dY = S.run(t, hand, b, rowwise, ld, tag=f"plan={plan} nbuf={nbuf} nt={nt}")
                for v in range(b):
                    ycol = dY[v:S.n * b:b] if rowwise else dY[v * ld:v * ld + S.n]
                    assert t.equal(ysp[v].view(bits), ycol.contiguous().view(bits)), (b, rowwise, ld, v)
                cases += 1
        assert cases == 12
    finally:
        pkg.set_tuning(sweep_nbuf=1, nontemporal=1)


@pytest.mark.parametrize("kind", KINDS)
def test_the_switches(pkg, torch_cuda, splits, kind):
    """"sweep" 0 and "spmmv_variant" 1 report (0, 0) on the same handles and give the same bits; widths without a specialised kernel stay
    on the generic kernel; a view one element off 16-byte alignment gives the same bits with its surroundings untouched; a column-major ld
    whose columns are not 16-byte aligned does not report the sweep; handles planned with the default window report (0, 0) for every b,
    and b = 1 reports the single-vector sweep"""
    t = torch_cuda
    S = splits(kind, 32, 512)
    hand = S.handles()
    wlog = _plan(pkg, S, hand, 12, 2048)
    try:
        for b in (2, 8):
            for rowwise, ld in S.shapes():
                lay = _layout(pkg, rowwise)
                assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, lay) == _expected_path(pkg, S, b, wlog, rowwise)
                assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, lay)[0] == SWEEP
                for key in ("sweep", "spmmv_variant"):
                    pkg.set_tuning(**{key: 1 - DEFAULTS[key]})
                    assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, lay) == (0, 0), key
                    S.run(t, hand, b, rowwise, ld, tag=f"{key} flipped")
                    pkg.set_tuning(**{key: DEFAULTS[key]})
                S.run(t, hand, b, rowwise, ld, tag="switches back")
                S.run(t, hand, b, rowwise, ld, offset=1, tag="one element off")
    finally:
        pkg.set_tuning(**DEFAULTS)
    for b in (3, 5):
        for rowwise, ld in S.shapes():
            assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, _layout(pkg, rowwise)) == (0, 0)
            S.run(t, hand, b, rowwise, ld, tag="generic width")
    assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], 1, S.n, pkg.COLWISE) == (SWEEP, 1)
    # column-major with a leading dimension that leaves the columns off 16 bytes: the sweep kernel stands back; row-major does not mind
    odd = S.n + (33 if kind != "sp_hp" else 34)
    assert (odd * S.dtype().itemsize) % 16 != 0
    assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], 4, odd, pkg.COLWISE)[0] != SWEEP
    assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], 4, odd, pkg.ROWWISE) == (SWEEP, 4)
    S.run(t, hand, 4, 0, S.n + 32, tag="even ld")
    # the planner's default window under "sweep_nbuf" 1: one vector fills the LDS
    hd = S.handles()
    wdef = _plan(pkg, S, hd, 0, 0)
    assert wdef == (15 if kind == "sp_hp" else 14)
    for b in (2, 3, 4, 8, 16):
        for rowwise, ld in S.shapes():
            assert pkg.spmmv_ap_hp_path(hd[0], hd[1], hd[2], b, ld, _layout(pkg, rowwise)) == (0, 0)
    assert pkg.spmmv_ap_hp_path(hd[0], hd[1], hd[2], 1, S.n, pkg.ROWWISE) == (SWEEP, 1)
    S.run(t, hd, 2, 1, S.n, tag="default window")


@pytest.mark.parametrize("kind", ("dp_sp_hp", "sp_hp"))
def test_partial_coverage_runs_the_rest_chunks(pkg, orc, torch_cuda, kind):
    """one 256-row tile whose rows list their entries in DESCENDING column order (windows not ascending: the planner leaves it to the
    rest chunks), every other tile sweeps: sweep kernel + lane-per-row kernel over the rest chunks together give the oracle's Y"""
    t = torch_cuda
    n = 4096
    I, J, V = (a.copy() for a in pkg.gen_banded_random(n, 40, 1500, magnitude_decades=10.0).arrays())
    order = np.lexsort((J, I))                                    # rows ascending, columns ascending within a row
    I, J, V = I[order], J[order], V[order]
    sel = np.flatnonzero((I >= 512) & (I < 768))
    rev = sel[np.lexsort((-J[sel].astype(np.int64), I[sel]))]     # ... descending within the rows of tile 2
    J[sel], V[sel] = J[rev], V[rev]
    coo = pkg.Coo.from_arrays(n, n, I, J, V)
    S = BlockSplit(pkg, orc, coo, kind, 32, 1, n_oracle=8)
    assert S.n == n
    hand = S.handles()
    pkg.set_tuning(sweep_max_stage=1 << 20)
    try:
        n_tiles, n_sweep = pkg.optimize_sweep_ap_hp(hand[0], hand[1], hand[2], *S.structs, 8, 256)
    finally:
        pkg.set_tuning(sweep_max_stage=0)
    assert 0 < n_sweep < n_tiles == n // 256, (n_tiles, n_sweep)
    assert hand[0].sweep_plan_digest()[1][5] > 0                  # chunks left to the lane-per-row kernel
    cases = 0
    for b in (2, 8):
        for rowwise, ld in S.shapes():
            assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, _layout(pkg, rowwise)) == (SWEEP, b)    # (windows of 2^8 elements: one pass)
            for nt in (1, 0):
                pkg.set_tuning(nontemporal=nt)
                try:
                    S.run(t, hand, b, rowwise, ld, tag=f"partial coverage {n_sweep}/{n_tiles} nt={nt}")
                finally:
                    pkg.set_tuning(nontemporal=1)
            cases += 1
    assert cases == 6


@pytest.mark.parametrize("kind", KINDS)
def test_device_built_plan(pkg, torch_cuda, splits, kind):
    """the plan built on the device from the handles' own arrays (no host struct involved) runs the same kernel to the same bits"""
    S = splits(kind, 32, 512)
    hand = S.handles()
    assert _plan(pkg, S, hand, 12, 1024, device=True) == 12
    cases = 0
    for b in WIDTHS:
        for rowwise, ld in S.shapes():
            assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, _layout(pkg, rowwise)) == _expected_path(pkg, S, b, 12, rowwise)
            S.run(torch_cuda, hand, b, rowwise, ld, tag="device-built plan")
            cases += 1
    assert cases == 12


@pytest.mark.parametrize("kind", KINDS)
def test_special_values(pkg, torch_cuda, splits, kind):
    """X columns with NaN, +-Inf, -0.0 and denormals, other places in every column: NaN in the same places as per-column
    uspmv_spmv_ap_hp, every other element bitwise"""
    t = torch_cuda
    S = splits(kind, 32, 512)
    n, b = S.n, 8
    tiny, dmin = (np.float32(1e-45), np.float32(1.1754944e-38) / 4) if kind == "sp_hp" else (5e-324, 2.2250738585072014e-308 / 4.0)
    cols = np.empty((b, n), S.dtype)
    for v in range(b):
        x = S.xcols[v].copy()
        x[0 + v] = -np.inf; x[3 + 2 * v] = -0.0; x[100 + 7 * v] = np.inf; x[1000 + 13 * v] = np.nan; x[2000 + v:2000 + v + 40] = tiny * (v + 1)
        x[n // 2 + 31 * v] = -dmin
        cols[v] = x
    cases = 0
    for wlog, rows in ((12, 2048), (11, 256), (13, 0)):
        hand = S.handles()
        _plan(pkg, S, hand, wlog, rows)
        ref = np.empty((b, n), S.dtype)
        for v in range(b):
            y = t.zeros(n, dtype=hand[0].torch_dtype, device="cuda")
            pkg.spmv_ap_hp(hand[0], hand[1], hand[2], t.from_numpy(cols[v]).cuda(), y)
            ref[v] = y.cpu().numpy()
        assert np.isnan(ref).any() and np.isinf(ref).any()
        for bb in (2, 8):
            for rowwise in (1, 0):
                X = np.ascontiguousarray(cols[:bb].T).reshape(-1) if rowwise else cols[:bb].reshape(-1)
                dY = t.full((bb * n,), 9.0, dtype=hand[0].torch_dtype, device="cuda")
                assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], bb, n, _layout(pkg, rowwise)) == _expected_path(pkg, S, bb, wlog, rowwise)
                pkg.spmmv_ap_hp(hand[0], hand[1], hand[2], t.from_numpy(X).cuda(), dY, bb, n, _layout(pkg, rowwise))
                got = dY.cpu().numpy()
                got = np.ascontiguousarray(got.reshape(n, bb).T) if rowwise else got.reshape(bb, n)
                assert _same(got, ref[:bb]), (wlog, rows, bb, rowwise)
                cases += 1
    assert cases == 12


def test_no_workspace_no_growth(pkg, torch_cuda, splits):
    """column-major X is staged straight from the caller's array: 200 calls alternating b = 2 and 4 leave free device memory where it
    was after the first two"""
    t = torch_cuda
    S = splits("dp_sp_hp", 32, 512)
    hand = S.handles()
    _plan(pkg, S, hand, 12, 2048)
    X = t.ones(4 * S.n, dtype=t.float64, device="cuda"); Y = t.zeros_like(X)
    for b in (4, 2):
        assert pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, S.n, pkg.COLWISE)[0] == SWEEP
        pkg.spmmv_ap_hp(hand[0], hand[1], hand[2], X, Y, b, S.n, pkg.COLWISE)
    t.cuda.synchronize()
    free0, _ = t.cuda.mem_get_info()
    for k in range(200):
        pkg.spmmv_ap_hp(hand[0], hand[1], hand[2], X, Y, 2 if k % 2 == 0 else 4, S.n, pkg.COLWISE)
    t.cuda.synchronize()
    free1, _ = t.cuda.mem_get_info()
    assert free0 == free1, f"{free0 - free1} bytes of device memory gone over 200 calls"
