"""The adaptive-precision sweep kernels on RAGGED matrices: scs_spmv_sweep_ap_hp (csrc/sweep_ap_hp_kernels.hip), scs_spmmv_ap_hp_sweep
(csrc/ap_hp_spmmv_sweep.hip), scs_spmmv_ap_sweep (csrc/ap_spmmv_sweep.hip) and the chunk-list form of scs_spmmv_ap_rows over rest chunks
that end on the matrix's padded last chunk.  The other sweep files run them on friendly sizes only (rows = padded rows = a multiple of
every tile, window and DMA piece), where the tail branches of the staging code, the row slots beyond n_rows_padded in the last tile and a
chunk list with the last chunk never execute.  Here every matrix has an odd number of referenced X rows that is no multiple of a 16-byte
piece or of the window, and a partial last tile -- each test ASSERTS that before it looks at a product, so a change of the generator
cannot turn this file back into a friendly-size test.

All four kinds: ap[dp_sp] against the oracle's spmv_scs_ap_adv, the fp16 kinds against the oracle composed part by part (the helpers of
tests/test_gpu_ap_hp_spmmv_sweep.py), column by column.  Same bits, no tolerance; a NaN equals any NaN in the same place.  Y is pre-filled
with 9.0 and carries a 64-element guard zone: nothing outside the written elements may change.  No case is skipped: every test counts its
cases.

One thing is the dispatch's own and not a property of these shapes: uspmv_spmmv_ap keeps the gather kernel for ROW-MAJOR X in more than
two passes, so the pair reports path 1 there (shape B at b = 16, shape C at b = 8 and 16); those cases are asserted as
such and still pinned to the oracle."""
import numpy as np
import pytest

from conftest import make_x
from test_gpu_ap_hp_spmmv_sweep import DEFAULTS, GUARD, WIDTHS, BlockSplit, _oracle, _plan, _same, _thresholds
from test_gpu_ap_spmmv_sweep import _pair_structs
from test_gpu_sweep_ap_hp import _same_sweep_plans

pytestmark = pytest.mark.gpu
KINDS = ("dp_sp", "dp_hp", "sp_hp", "dp_sp_hp")
GATHER, SWEEP = 1, 3
SEED = 7                                     # gen_banded_random(n, nnz_per_row, band, seed=7, magnitude_decades=10.0): tests/cpp/sweep_plan_hp_emulate.cpp
MATRICES = {9999: (9999, 23, 700), 7777: (7777, 31, 900), 5001: (5001, 40, 1500)}
# id: (rows of the matrix, C, sigma, wlog, tile rows, n_rows_padded)
SHAPES = {
    "A": (9999, 8, 64, 8, 512, 10000),       # many windows; 512 threads; 8 vectors per pass
    "B": (7777, 32, 512, 12, 1024, 7808),    # double X: 4 vectors per pass, several passes at b = 8, 16
    "C": (9999, 32, 1, 13, 4096, 10016),     # 4 rows per lane walked in row groups; double X: 2 vectors per pass, float X: 4
    "D": (7777, 64, 128, 13, 2048, 7808),    # C = 64; 2 rows per lane
    "E": (7777, 32, 512, 14, 1024, 7808),    # float X at 2 vectors per pass: two rows per piece at b = 2, through registers from b = 4 on
    "F": (5001, 16, 1, 11, 256, 5008),       # 256-thread workgroups; C = 16
    # 4 rows per lane under 8 and 4 vectors per pass: the row-group loop with double X as well (4 groups of 1 row and 2 of 2 rows for the
    # fp16 kinds, 2 of 2 rows for the pair), which shape C reaches with float X only -- double X runs 2 vectors per pass there, 4 rows at a time
    "G": (9999, 32, 1, 11, 4096, 10016),
}


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert pkg.device_count() >= 1
    torch.cuda.set_device(0)
    pkg.set_tuning(**DEFAULTS)
    yield torch
    pkg.set_tuning(**DEFAULTS)


class PairSplit(BlockSplit):
    """BlockSplit for the ap[dp_sp] pair, split at the median of |value|: structs (dp, None, sp), double X"""

    def __init__(self, pkg, orc, m, C, sigma, n_oracle=16):
        ds, ss = _pair_structs(pkg, m, C, sigma, th=_thresholds(m, 0.5, 0.5)[0])
        self.structs = (ds, None, ss)
        self.pkg, self.kind, self.C, self.n = pkg, "dp_sp", C, ds.n_rows_padded
        self.dtype, self.x_dtype = np.float64, pkg.F64
        xp = np.zeros(self.n)
        xp[:m.n_rows] = make_x(m.n_rows)[ds.arrays()["new_to_old_idx"]]
        self.xp = xp
        self.xcols = [xp * (1.0 + v / 8.0) for v in range(n_oracle)]
        self.ycols = [_oracle_of(orc, self, x) for x in self.xcols]
        self._case = {}


def _split(pkg, orc, m, kind, C, sigma, n_oracle=16):
    return PairSplit(pkg, orc, m, C, sigma, n_oracle) if kind == "dp_sp" else BlockSplit(pkg, orc, m, kind, C, sigma, n_oracle)


def _oracle_of(orc, S, x):
    if S.kind != "dp_sp":
        return _oracle(orc, S.kind, S.structs, x)
    parts = tuple((q["chunk_ptrs"], q["chunk_lengths"], q["col_idxs"], q["values"]) for q in (S.structs[0].arrays(), S.structs[2].arrays()))
    return orc.spmv_scs_ap_adv(S.C, S.structs[0].n_chunks, parts[0], parts[1], x)


@pytest.fixture(scope="module")
def splits(pkg, orc, torch_cuda):
    mats, cache = {}, {}

    def get(kind, shape):
        rows, C, sigma = SHAPES[shape][:3]
        if rows not in mats:
            mats[rows] = pkg.gen_banded_random(*MATRICES[rows], seed=SEED, magnitude_decades=10.0)
        if (kind, rows, C, sigma) not in cache:
            cache[(kind, rows, C, sigma)] = _split(pkg, orc, mats[rows], kind, C, sigma)
        return cache[(kind, rows, C, sigma)]
    return get


def _layout(pkg, rowwise):
    return pkg.ROWWISE if rowwise else pkg.COLWISE


def _spmmv(pkg, S, hand, X, Y, b, ld, rowwise):
    if S.kind == "dp_sp": pkg.spmmv_ap(hand[0], hand[2], X, Y, b, ld, _layout(pkg, rowwise))
    else: pkg.spmmv_ap_hp(hand[0], hand[1], hand[2], X, Y, b, ld, _layout(pkg, rowwise))


def _spmv(pkg, S, hand, x, y):
    if S.kind == "dp_sp": pkg.spmv_ap(hand[0], hand[2], x, y)
    else: pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y)


def _path(pkg, S, hand, b, ld, rowwise):
    if S.kind == "dp_sp": return pkg.spmmv_ap_path(hand[0], hand[2], b, ld, _layout(pkg, rowwise))
    return pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, _layout(pkg, rowwise))


def _vectors(pkg, S, b, wlog):
    return pkg.spmmv_ap_sweep_vectors(b, wlog) if S.kind == "dp_sp" else pkg.spmmv_ap_hp_sweep_vectors(b, wlog, S.x_dtype)


def _expected_path(pkg, S, b, wlog, rowwise):
    """(path, vectors) of sweep-planned parts at a B-specialised width: the sweep kernel wherever two vectors of a window fit LDS; where
    they do not, the fp16 kinds' generic kernel and the pair's gather kernel, which the pair also keeps for row-major X in more than two
    passes"""
    vec = _vectors(pkg, S, b, wlog)
    if S.kind != "dp_sp":
        return (SWEEP, vec) if vec else (0, 0)
    return (SWEEP, vec) if vec and (not rowwise or b // vec <= 2) else (GATHER, 0)


def _install(pkg, S, hand, wlog, rows, device=False):
    """install the parts' shared sweep plan (sweep_max_stage 1 << 20), assert that every tile sweeps with kind 2 on every part; returns
    the log2 of its window"""
    if S.kind != "dp_sp":
        return _plan(pkg, S, hand, wlog, rows, device)
    pkg.set_tuning(sweep_max_stage=1 << 20)
    try:
        if device: nt_, nsw = hand[0].optimize_sweep_device(hand[2], wlog, rows)
        else: nt_, nsw = pkg.optimize_sweep_ap(hand[0], hand[2], S.structs[0], S.structs[2], wlog, rows)
    finally:
        pkg.set_tuning(sweep_max_stage=0)
    assert nsw == nt_ > 0, (wlog, rows, nt_, nsw)
    assert [hand[0].plan_info()[0], hand[2].plan_info()[0]] == [2, 2]
    meta = hand[0].sweep_plan_digest()[1]
    assert meta[0] == 1 and meta[2] == wlog and meta[1] == rows, meta
    return int(meta[2])


def _x_rows(S):
    """X rows the matrix references: 1 + the highest column index of any part (padding entries included)"""
    return 1 + max(int(s.arrays()["col_idxs"].max()) for s in S.structs if s is not None)


def _ragged(S, wlog, rows, n_pad):
    """the conditions under which the tail branches run; returns the number of referenced X rows"""
    for s in S.structs:
        assert s is None or (s.nnz > 0 and s.n_elements > 0), (S.kind, "an empty part")
    assert (S.structs[1] is not None) == (S.kind == "dp_sp_hp")
    assert S.n == n_pad and all(s.n_rows_padded == n_pad for s in S.structs if s is not None), (S.n, n_pad)
    assert n_pad % rows != 0, "the last tile must be partial"
    xr = _x_rows(S)
    piece = 16 // np.dtype(S.dtype).itemsize
    assert xr % 2 == 1 and xr % piece != 0 and xr % (1 << wlog) != 0 and xr < n_pad, (xr, piece, wlog, n_pad)
    return xr


def _run(t, pkg, S, hand, X, want, b, rowwise, ld, tag=""):
    """one call on X into a Y filled with 9.0 (b * ld + GUARD elements, as X and want): the oracle's bits where the call must write,
    9.0 everywhere else"""
    assert len(X) == len(want) == b * ld + GUARD
    dX = t.from_numpy(X).cuda()
    dY = t.full((len(want),), 9.0, dtype=hand[0].torch_dtype, device="cuda")
    _spmmv(pkg, S, hand, dX, dY, b, ld, rowwise)
    got = dY.cpu().numpy()
    if not _same(got, want):
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{S.kind} C={S.C} b={b} rowwise={rowwise} ld={ld} {tag}: {len(bad)} elements differ, first at "
                             f"{bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}")
    return dY


def _bits(t, S):
    return t.int32 if S.kind == "sp_hp" else t.int64


GRID = [(k, s) for k in KINDS for s in "ABCDEFG"]


@pytest.mark.parametrize("kind,shape", GRID, ids=[f"{k}-{s}" for k, s in GRID])
def test_grid_bitexact(pkg, torch_cuda, splits, kind, shape):
    """every width x layout x leading dimension on every ragged shape: the path and the vectors per pass that the dispatch names (the
    sweep wherever two vectors of a window fit LDS), the oracle's bits in every written element, 9.0 everywhere else; and column v = the
    single-vector product of column v on the same handles (its own sweep kernel), itself pinned to the oracle -- on shape B under every
    sweep_pair / sweep_nbuf form.  Two of the buffer-count x load / store forms per case, their full product on shape B.  Shape E is
    ap[sp_hp]'s (float X at two vectors per pass); for double X one vector of 2^14 rows fills the LDS and the block kernel stands back."""
    t = torch_cuda
    _, C, sigma, wlog, rows, n_pad = SHAPES[shape]
    S = splits(kind, shape)
    _ragged(S, wlog, rows, n_pad)
    hand = S.handles()
    assert _install(pkg, S, hand, wlog, rows) == wlog
    if shape == "E" and kind != "sp_hp":
        cases = 0
        for b in WIDTHS:
            for rowwise, ld in S.shapes():
                assert _vectors(pkg, S, b, wlog) == 0
                assert _path(pkg, S, hand, b, ld, rowwise) == ((GATHER, 0) if kind == "dp_sp" else (0, 0))
                cases += 1
        assert cases == 12
        _run(t, pkg, S, hand, *S.case(4, 1, S.n), 4, 1, S.n, tag="wlog 14, no sweep")
        return
    full = shape == "B"
    bits = _bits(t, S)
    try:
        if kind != "dp_sp": assert _path(pkg, S, hand, 1, S.n, 0) == (SWEEP, 1)
        forms = [(pair, nbuf) for pair in (0, 1, 2) for nbuf in (1, 2)] if full else [(DEFAULTS["sweep_pair"], DEFAULTS["sweep_nbuf"])]
        ysp = []
        for v in range(16):
            x = t.from_numpy(S.xcols[v]).cuda()
            for pair, nbuf in forms:
                pkg.set_tuning(sweep_pair=pair, sweep_nbuf=nbuf)
                y = t.full((S.n,), -3.0, dtype=hand[0].torch_dtype, device="cuda")
                _spmv(pkg, S, hand, x, y)
                assert _same(y.cpu().numpy(), S.ycols[v]), ("single vector", v, pair, nbuf)
            ysp.append(y)
        pkg.set_tuning(sweep_pair=DEFAULTS["sweep_pair"], sweep_nbuf=DEFAULTS["sweep_nbuf"])
        k = cases = swept = 0
        for b in WIDTHS:
            for rowwise, ld in S.shapes():
                path, vec = _path(pkg, S, hand, b, ld, rowwise)
                assert (path, vec) == _expected_path(pkg, S, b, wlog, rowwise), (b, rowwise, ld, wlog, path, vec)
                assert _vectors(pkg, S, b, wlog) >= 2
                if kind != "dp_sp" or not rowwise or b // _vectors(pkg, S, b, wlog) <= 2:
                    assert (path, vec) == (SWEEP, _vectors(pkg, S, b, wlog))
                    swept += 1
                combos = [(nb, nt) for nb in (1, 2) for nt in (1, 0)] if full else [((1, 1), (2, 0), (2, 1), (1, 0))[k % 4], ((2, 0), (1, 1), (1, 0), (2, 1))[k % 4]]
                k += 1
                X, want = S.case(b, rowwise, ld)
                for nbuf, nt in combos:
                    pkg.set_tuning(sweep_nbuf=nbuf, nontemporal=nt)
                    dY = _run(t, pkg, S, hand, X, want, b, rowwise, ld, tag=f"shape {shape} nbuf={nbuf} nt={nt}")
                for v in range(b):
                    ycol = dY[v:S.n * b:b] if rowwise else dY[v * ld:v * ld + S.n]
                    assert t.equal(ysp[v].view(bits), ycol.contiguous().view(bits)), (b, rowwise, ld, v)
                cases += 1
        assert cases == 12
        # (the pair's row-major X in more than two passes stays on the gather kernel: b = 16 at 4 vectors per pass, b = 8, 16 at 2)
        assert swept == 12 - (0 if kind != "dp_sp" else {12: 1, 13: 2}.get(wlog, 0)), (swept, wlog)
    finally:
        pkg.set_tuning(**DEFAULTS)


@pytest.mark.parametrize("shape", ("A", "C"))
@pytest.mark.parametrize("kind", KINDS)
def test_unreferenced_x_is_unread_in_effect(pkg, orc, torch_cuda, splits, kind, shape):
    """X with NaN in every element the matrix does not reference -- rows xr ... n_pad - 1 of every column, the ld padding of a
    column-major X, the guard zone -- gives the bits of the clean X.  The oracle, fed the same poisoned columns, says so first (its
    padding entries point at a referenced column): the input is fair.  A kernel that stages the tail correctly but consumes a stale or
    out-of-range window element -- the index of a lane that sits a round out -- fails here."""
    t = torch_cuda
    _, C, sigma, wlog, rows, n_pad = SHAPES[shape]
    S = splits(kind, shape)
    xr = _ragged(S, wlog, rows, n_pad)
    for v in range(8):
        xpois = S.xcols[v].copy()
        xpois[xr:] = np.nan
        assert np.isnan(xpois).sum() == S.n - xr > 0
        ypois = _oracle_of(orc, S, xpois)
        u = {4: np.uint32, 8: np.uint64}[ypois.dtype.itemsize]
        assert np.array_equal(ypois.view(u), S.ycols[v].view(u)), ("the oracle reads an unreferenced X row", v)
    hand = S.handles()
    assert _install(pkg, S, hand, wlog, rows) == wlog
    cases = 0
    try:
        for b in (2, 8):
            for rowwise, ld in S.shapes():
                assert _path(pkg, S, hand, b, ld, rowwise) == _expected_path(pkg, S, b, wlog, rowwise)
                X, want = S.case(b, rowwise, ld)
                X = X.copy()
                if rowwise:
                    X[xr * b:] = np.nan
                else:
                    for v in range(b): X[v * ld + xr:(v + 1) * ld] = np.nan
                    X[b * ld:] = np.nan
                assert np.isnan(X).sum() == b * (ld - xr) + GUARD
                for nbuf in (1, 2):
                    pkg.set_tuning(sweep_nbuf=nbuf)
                    _run(t, pkg, S, hand, X, want, b, rowwise, ld, tag=f"shape {shape} poisoned X nbuf={nbuf}")
                cases += 1
        assert cases == 6
    finally:
        pkg.set_tuning(**DEFAULTS)


@pytest.mark.parametrize("kind", ("dp_sp", "sp_hp", "dp_sp_hp"))
def test_rest_chunks_at_the_ragged_end(pkg, orc, torch_cuda, kind):
    """the 9 999-row matrix at C = 32, sigma = 1, windows of 2^8, 256-row tiles, the rows of the LAST tile (>= 9 984) listing their
    entries in descending column order: the planner leaves that tile to the lane-per-row kernel, whose chunk-id list then ends with the
    matrix's padded last chunk; sweep kernel + rest chunks together give the oracle's Y"""
    t = torch_cuda
    n, wlog, rows, n_pad = 9999, 8, 256, 10016
    I, J, V = (a.copy() for a in pkg.gen_banded_random(*MATRICES[n], seed=SEED, magnitude_decades=10.0).arrays())
    order = np.lexsort((J, I))                                    # rows ascending, columns ascending within a row
    I, J, V = I[order], J[order], V[order]
    last = (n_pad // rows) * rows
    assert last == 9984 < n
    sel = np.flatnonzero(I >= last)
    rev = sel[np.lexsort((-J[sel].astype(np.int64), I[sel]))]     # ... descending within the rows of the last tile
    J[sel], V[sel] = J[rev], V[rev]
    S = _split(pkg, orc, pkg.Coo.from_arrays(n, n, I, J, V), kind, 32, 1, n_oracle=8)
    _ragged(S, wlog, rows, n_pad)
    hand = S.handles()
    pkg.set_tuning(sweep_max_stage=1 << 20)
    try:
        if kind == "dp_sp": n_tiles, n_sweep = pkg.optimize_sweep_ap(hand[0], hand[2], S.structs[0], S.structs[2], wlog, rows)
        else: n_tiles, n_sweep = pkg.optimize_sweep_ap_hp(hand[0], hand[1], hand[2], *S.structs, wlog, rows)
    finally:
        pkg.set_tuning(sweep_max_stage=0)
    assert 0 < n_sweep < n_tiles == -(-n_pad // rows), (n_tiles, n_sweep)
    assert hand[0].sweep_plan_digest()[1][5] > 0                  # chunks left to the lane-per-row kernel
    cases = 0
    try:
        for b in (2, 8):
            for rowwise, ld in S.shapes():
                assert _path(pkg, S, hand, b, ld, rowwise) == (SWEEP, b)                  # (windows of 2^8 elements: one pass)
                X, want = S.case(b, rowwise, ld)
                for nt in (1, 0):
                    pkg.set_tuning(nontemporal=nt)
                    _run(t, pkg, S, hand, X, want, b, rowwise, ld, tag=f"rest chunks at the end {n_sweep}/{n_tiles} nt={nt}")
                cases += 1
        assert cases == 6
    finally:
        pkg.set_tuning(**DEFAULTS)


@pytest.mark.parametrize("shape", ("A", "C"))
@pytest.mark.parametrize("kind", KINDS)
def test_device_built_plan(pkg, torch_cuda, splits, kind, shape):
    """the plan built on the device from the handles' own arrays (csrc/sweep_plan_kernels.hip has the same partial last tile) equals the
    host planner's array for array and gives the oracle's bits at b = 1 and 4"""
    t = torch_cuda
    _, C, sigma, wlog, rows, n_pad = SHAPES[shape]
    S = splits(kind, shape)
    _ragged(S, wlog, rows, n_pad)
    host, hand = S.handles(), S.handles()
    assert _install(pkg, S, host, wlog, rows) == wlog
    assert _install(pkg, S, hand, wlog, rows, device=True) == wlog
    _same_sweep_plans(host, hand)
    cases = 0
    for v in range(4):
        y = t.full((S.n,), -3.0, dtype=hand[0].torch_dtype, device="cuda")
        _spmv(pkg, S, hand, t.from_numpy(S.xcols[v]).cuda(), y)
        assert _same(y.cpu().numpy(), S.ycols[v]), ("single vector, device-built plan", v)
    cases += 1
    for rowwise, ld in S.shapes():
        assert _path(pkg, S, hand, 4, ld, rowwise) == _expected_path(pkg, S, 4, wlog, rowwise)
        assert _path(pkg, S, hand, 4, ld, rowwise)[0] == SWEEP
        _run(t, pkg, S, hand, *S.case(4, rowwise, ld), 4, rowwise, ld, tag=f"shape {shape}, device-built plan")
        cases += 1
    assert cases == 4
