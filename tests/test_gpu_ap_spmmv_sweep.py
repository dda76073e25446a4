"""ap[dp_sp] SpMMV on the pair's column-window sweep plan (csrc/ap_spmmv_sweep.hip, scs_spmmv_ap_sweep): b in {2, 4, 8, 16} right-hand
sides walk the plan's compacted dp and sp streams once per pass.  The contract is the project's usual one -- same bits: column v of Y is
what scs_ap_impl_cpu<C> (the oracle's spmv_scs_ap_adv) and uspmv_spmv_ap give for column v of X, for every plan shape (rows per lane 1,
2 and 4; 8, 4 and 2 vectors per pass; one and several passes; one and two LDS buffers), both layouts, a padded leading dimension,
partial coverage (rest chunks), device-built plans and special values.  No tolerance anywhere; NaN: same places, sign left to the
hardware.  uspmv_spmmv_ap_path must say which kernel ran."""
import numpy as np
import pytest

from conftest import block_x, make_x

pytestmark = pytest.mark.gpu
GUARD = 64
WIDTHS = (2, 4, 8, 16)
# (wlog, tile rows, "sweep_nbuf" while planning).  (0, 0): the planner's defaults -- its window is what the LDS buffers of the single-vector
# kernel leave: 2^13 doubles when planned for two buffers, 2^14 (one vector fills the LDS: the block kernel stands back) for one
PLANS = ((11, 256, 1), (12, 1024, 1), (12, 2048, 1), (12, 4096, 1), (0, 0, 2), (0, 0, 1))
GATHER, STAGED, SWEEP = 1, 2, 3


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert pkg.device_count() >= 1
    torch.cuda.set_device(0)
    yield torch
    pkg.set_tuning(nontemporal=1, spmmv_variant=0, tlc=1, sweep=1, sweep_nbuf=1, sweep_unroll=8, sweep_remap=8, sweep_wlog=0, sweep_tile_rows=0,
                   sweep_max_stage=0, tlc_tile_rows=0)


def _pair_structs(pkg, coo, C, sigma, th=1e-3):
    """the ap[dp_sp] pair of `coo` as test_gpu_sweep.py builds it: one row permutation, columns permuted with it"""
    dp, sp = pkg.partition_precisions(coo, th)
    assert dp.nnz > 0 and sp.nnz > 0
    ds = pkg.convert_to_scs(dp, C, sigma, pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, C, sigma, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
    return ds, ss


class BlockPair:
    """A pair, its X of 16 columns (column v = xp * (1 + v / 8), what conftest.block_x lays out) and the oracle's 16 columns of Y, computed
    once; X and the expected Y of every (b, layout, ld) are kept on the device."""

    def __init__(self, pkg, orc, t, coo, C, sigma, n_oracle=16):
        self.pkg, self.t, self.C = pkg, t, C
        self.ds, self.ss = _pair_structs(pkg, coo, C, sigma)
        da, sa = self.ds.arrays(), self.ss.arrays()
        self.n = self.ds.n_rows_padded
        self.xp = np.zeros(self.n)
        self.xp[:self.ds.n_rows] = pkg.apply_permutation(make_x(self.ds.n_rows), da["new_to_old_idx"])
        parts = tuple((q["chunk_ptrs"], q["chunk_lengths"], q["col_idxs"], q["values"]) for q in (da, sa))
        self.ycols = [orc.spmv_scs_ap_adv(C, self.ds.n_chunks, parts[0], parts[1], self.xp * (1.0 + v / 8.0)) for v in range(n_oracle)]
        self._case = {}

    def handles(self):
        return self.pkg.DeviceMatrix(self.ds), self.pkg.DeviceMatrix(self.ss)

    def shapes(self):
        return [(1, self.n), (0, self.n), (0, self.n + 32)]

    def case(self, b, rowwise, ld):
        """(X, expected Y with 9.0 wherever the kernel must not write) on the device, Y of b * ld + GUARD elements"""
        key = (b, rowwise, ld)
        if key not in self._case:
            n = self.n
            X = block_x(self.xp, n, b, ld, rowwise)
            want = np.full(b * ld + GUARD, 9.0)
            for v in range(b):
                if rowwise: want[v:n * b:b] = self.ycols[v]
                else: want[v * ld:v * ld + n] = self.ycols[v]
            self._case[key] = (self.t.from_numpy(X).cuda(), self.t.from_numpy(want).cuda())
        return self._case[key]

    def run(self, Ad, As, b, rowwise, ld, tag=""):
        t = self.t
        dX, want = self.case(b, rowwise, ld)
        dY = t.full((b * ld + GUARD,), 9.0, dtype=t.float64, device="cuda")
        self.pkg.spmmv_ap(Ad, As, dX, dY, b, ld, self.pkg.ROWWISE if rowwise else self.pkg.COLWISE)
        if not t.equal(dY, want):
            got, w = dY.cpu().numpy(), want.cpu().numpy()
            bad = np.flatnonzero(got != w)
            raise AssertionError(f"b={b} rowwise={rowwise} ld={ld} {tag}: {len(bad)} elements differ, first at {bad[0]}: {got[bad[0]]!r} != {w[bad[0]]!r}")
        return dX, dY


@pytest.fixture(scope="module")
def pairs(pkg, orc, torch_cuda):
    coo = pkg.gen_banded_random(50000, 70, 6000, magnitude_decades=10.0)
    cache = {}

    def get(C, sigma):
        if (C, sigma) not in cache:
            cache[(C, sigma)] = BlockPair(pkg, orc, torch_cuda, coo, C, sigma)
        return cache[(C, sigma)]
    return get


def _plan(pkg, P, Ad, As, wlog, rows, plan_nbuf=1):
    """install the pair's sweep plan; returns the log2 of its window"""
    pkg.set_tuning(sweep_nbuf=plan_nbuf)
    try:
        nt_, nsw = pkg.optimize_sweep_ap(Ad, As, P.ds, P.ss, wlog, rows)
    finally:
        pkg.set_tuning(sweep_nbuf=1)
    assert nsw == nt_ > 0 and Ad.plan_info()[0] == 2
    meta = Ad.sweep_plan_digest()[1]
    assert meta[0] == 1 and (wlog == 0 or meta[2] == wlog) and (rows == 0 or meta[1] == rows)
    return int(meta[2])


def _expected_path(pkg, b, wlog, rowwise):
    """(path, vectors) of a sweep-planned pair at a B-specialised width: the sweep kernel wherever two vectors of a window fit LDS, except
    for row-major X in more than two passes, which measured behind the gather kernel and keeps it"""
    vec = pkg.spmmv_ap_sweep_vectors(b, wlog)
    return (SWEEP, vec) if vec and (not rowwise or b // vec <= 2) else (GATHER, 0)


def _layout(pkg, rowwise):
    return pkg.ROWWISE if rowwise else pkg.COLWISE


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: f"wlog{p[0]}_rows{p[1]}_nbuf{p[2]}")
@pytest.mark.parametrize("C,sigma", [(32, 512), (64, 64)])
def test_grid_bitexact(pkg, torch_cuda, pairs, C, sigma, plan):
    """every width x layout x leading dimension on every plan shape: path 3 with the vectors per pass uspmv_spmmv_ap_sweep_vectors names
    (windows of 2^14 doubles: no two vectors fit, path 1), the oracle's bits in every written element, 9.0 everywhere else (padded ld,
    guard zone); and column v = uspmv_spmv_ap of column v on the same handles.  Both buffer counts and both load / store forms
    everywhere, their full product on the (12, 2048) plan."""
    t = torch_cuda
    P = pairs(C, sigma)
    wlog, rows, plan_nbuf = plan
    Ad, As = P.handles()
    wlog = _plan(pkg, P, Ad, As, wlog, rows, plan_nbuf)
    assert wlog == (plan[0] or (13 if plan_nbuf == 2 else 14))
    full = plan[:2] == (12, 2048)
    try:
        # the single-vector product of the 16 columns on these handles (its own sweep kernel): pinned to the oracle here
        ysp = []
        for v in range(16):
            y = t.full((P.n,), -3.0, dtype=t.float64, device="cuda")
            pkg.spmv_ap(Ad, As, t.from_numpy(P.xp * (1.0 + v / 8.0)).cuda(), y)
            assert np.array_equal(y.cpu().numpy(), P.ycols[v]), ("spmv_ap", v)
            ysp.append(y)
        k = 0
        for b in WIDTHS:
            for rowwise, ld in P.shapes():
                path, vec = pkg.spmmv_ap_path(Ad, As, b, ld, _layout(pkg, rowwise))
                assert (path, vec) == _expected_path(pkg, b, wlog, rowwise), (b, rowwise, ld, wlog, path, vec)
                if wlog <= 13 and (not rowwise or b <= 2 * pkg.spmmv_ap_sweep_vectors(b, wlog)): assert path == SWEEP
                if wlog >= 14: assert path == GATHER
                combos = [(nb, nt) for nb in (1, 2) for nt in (1, 0)] if full else [((1, 1), (2, 0), (2, 1), (1, 0))[k % 4], ((2, 0), (1, 1), (1, 0), (2, 1))[k % 4]]
                k += 1
                for nbuf, nt in combos:
                    pkg.set_tuning(sweep_nbuf=nbuf, nontemporal=nt)
                    dX, dY = P.run(Ad, As, b, rowwise, ld, tag=f"plan={plan} nbuf={nbuf} nt={nt}")
                for v in range(b):
                    assert t.equal(ysp[v], dY[v:P.n * b:b] if rowwise else dY[v * ld:v * ld + P.n]), (b, rowwise, ld, v)
    finally:
        pkg.set_tuning(sweep_nbuf=1, nontemporal=1)


def test_the_switch(pkg, torch_cuda, pairs):
    """tuning "sweep" 0: the same handles report the gather kernel and give the same bits"""
    P = pairs(32, 512)
    Ad, As = P.handles()
    _plan(pkg, P, Ad, As, 13, 0)
    try:
        assert pkg.spmmv_ap_path(Ad, As, 2, P.n, pkg.ROWWISE) == (SWEEP, 2) and pkg.spmmv_ap_path(Ad, As, 8, P.n, pkg.COLWISE) == (SWEEP, 2)
        for b in (2, 8):
            for rowwise, ld in P.shapes():
                lay = _layout(pkg, rowwise)
                assert pkg.spmmv_ap_path(Ad, As, b, ld, lay) == _expected_path(pkg, b, 13, rowwise)
                pkg.set_tuning(sweep=0)
                assert pkg.spmmv_ap_path(Ad, As, b, ld, lay) == (GATHER, 0)
                P.run(Ad, As, b, rowwise, ld, tag="sweep=0")
                pkg.set_tuning(sweep=1)
                P.run(Ad, As, b, rowwise, ld, tag="sweep=1")
    finally:
        pkg.set_tuning(sweep=1)


def test_other_paths_keep_their_place(pkg, orc, torch_cuda, pairs):
    """widths without a specialised kernel stay on the generic kernel (path 0) on a sweep-planned pair, and so does an 8-byte-aligned view
    (which uspmv_spmmv_ap_path, asked about aligned vectors, cannot see: checked by its bits and its untouched surroundings); a pair with
    the shared line plan still reports the staged kernel"""
    t = torch_cuda
    P = pairs(32, 512)
    Ad, As = P.handles()
    _plan(pkg, P, Ad, As, 12, 2048)
    for b in (3, 5):
        for rowwise, ld in P.shapes():
            assert pkg.spmmv_ap_path(Ad, As, b, ld, _layout(pkg, rowwise)) == (0, 0)
            P.run(Ad, As, b, rowwise, ld, tag="generic width")
    pkg.set_tuning(spmmv_variant=1)
    try:
        assert pkg.spmmv_ap_path(Ad, As, 4, P.n, pkg.ROWWISE) == (0, 0)
    finally:
        pkg.set_tuning(spmmv_variant=0)
    for b in (2, 8):
        for rowwise, ld in P.shapes():
            dX, want = P.case(b, rowwise, ld)
            dXb = t.zeros(dX.numel() + 1, dtype=t.float64, device="cuda"); dXo = dXb[1:]; dXo.copy_(dX)
            dYb = t.full((want.numel() + 1,), 9.0, dtype=t.float64, device="cuda"); dYo = dYb[1:]
            assert dXo.data_ptr() % 16 == 8 and dYo.data_ptr() % 16 == 8
            pkg.spmmv_ap(Ad, As, dXo, dYo, b, ld, _layout(pkg, rowwise))
            assert t.equal(dYo, want) and float(dYb[0]) == 9.0, (b, rowwise, ld)
    # column-major with an odd leading dimension: no 16-byte pieces of a column, the sweep kernel stands back
    assert pkg.spmmv_ap_path(Ad, As, 4, P.n + 33, pkg.COLWISE)[0] != SWEEP
    assert pkg.spmmv_ap_path(Ad, As, 4, P.n + 33, pkg.ROWWISE) == (SWEEP, 4)
    # the stencil pair of test_staged_kernel_over_the_shared_plan
    ds, ss = _pair_structs(pkg, pkg.gen_stencil27(24, 24, 24, dof=1, magnitude_decades=10.0), 32, 512)
    Sd, Ss = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
    pkg.optimize_ap(Sd, Ss, ds, ss, pkg.spmmv_ap_plan_lines(4))
    assert Sd.plan_info()[0] == 1
    for lay in (pkg.ROWWISE, pkg.COLWISE):
        path, vec = pkg.spmmv_ap_path(Sd, Ss, 4, ds.n_rows_padded, lay)
        assert path == STAGED and vec in (2, 4), (path, vec)


def _same_but_nan_sign(got, ref):
    return np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~np.isnan(got)], ref[~np.isnan(ref)])


def test_special_values(pkg, torch_cuda, pairs):
    """X columns with NaN, +-Inf, -0.0 and denormals, other places in every column: NaN in the same places as per-column uspmv_spmv_ap,
    every other element bitwise"""
    t = torch_cuda
    P = pairs(32, 512)
    n, b = P.n, 8
    cols = np.empty((b, n))
    for v in range(b):
        x = P.xp * (1.0 + v / 8.0)
        x[0 + v] = -np.inf; x[3 + 2 * v] = -0.0; x[100 + 7 * v] = np.inf; x[1000 + 13 * v] = np.nan; x[2000 + v:2000 + v + 40] = 5e-324 * (v + 1)
        x[n // 2 + 31 * v] = -2.2250738585072014e-308 / 4.0
        cols[v] = x
    for wlog, rows in ((12, 2048), (11, 256), (13, 0)):
        Ad, As = P.handles()
        _plan(pkg, P, Ad, As, wlog, rows)
        ref = np.empty((b, n))
        for v in range(b):
            y = t.zeros(n, dtype=t.float64, device="cuda")
            pkg.spmv_ap(Ad, As, t.from_numpy(cols[v]).cuda(), y)
            ref[v] = y.cpu().numpy()
        assert np.isnan(ref).any() and np.isinf(ref).any()
        for bb in (2, 8):
            for rowwise in (1, 0):
                X = np.ascontiguousarray(cols[:bb].T).reshape(-1) if rowwise else cols[:bb].reshape(-1)
                dY = t.full((bb * n,), 9.0, dtype=t.float64, device="cuda")
                assert pkg.spmmv_ap_path(Ad, As, bb, n, _layout(pkg, rowwise)) == _expected_path(pkg, bb, wlog, rowwise)
                pkg.spmmv_ap(Ad, As, t.from_numpy(X).cuda(), dY, bb, n, _layout(pkg, rowwise))
                got = dY.cpu().numpy()
                got = got.reshape(n, bb).T if rowwise else got.reshape(bb, n)
                assert _same_but_nan_sign(got, ref[:bb]), (wlog, rows, bb, rowwise)


def test_partial_coverage_runs_the_rest_chunks(pkg, orc, torch_cuda):
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
    pkg.set_tuning(sweep_max_stage=1 << 20)
    try:
        P = BlockPair(pkg, orc, t, coo, 32, 1, n_oracle=8)
        assert P.n == n
        Ad, As = P.handles()
        n_tiles, n_sweep = pkg.optimize_sweep_ap(Ad, As, P.ds, P.ss, 8, 256)
    finally:
        pkg.set_tuning(sweep_max_stage=0)
    assert 0 < n_sweep < n_tiles == n // 256, (n_tiles, n_sweep)
    for b in (2, 8):
        for rowwise, ld in P.shapes():
            assert pkg.spmmv_ap_path(Ad, As, b, ld, _layout(pkg, rowwise)) == (SWEEP, b)          # (windows of 2^8 doubles: one pass)
            for nt in (1, 0):
                pkg.set_tuning(nontemporal=nt)
                try:
                    P.run(Ad, As, b, rowwise, ld, tag=f"partial coverage {n_sweep}/{n_tiles} nt={nt}")
                finally:
                    pkg.set_tuning(nontemporal=1)


def test_device_built_plan(pkg, torch_cuda, pairs):
    """the plan built on the device from the handles' own arrays (no host struct involved) runs the same kernel to the same bits"""
    P = pairs(32, 512)
    Ad, As = P.handles()
    nt_, nsw = Ad.optimize_sweep_device(As, 12, 1024)
    assert nsw == nt_ > 0
    for b in WIDTHS:
        for rowwise, ld in P.shapes():
            assert pkg.spmmv_ap_path(Ad, As, b, ld, _layout(pkg, rowwise)) == _expected_path(pkg, b, 12, rowwise)
            P.run(Ad, As, b, rowwise, ld, tag="device-built plan")


def test_no_workspace_no_growth(pkg, torch_cuda, pairs):
    """column-major X is staged straight from the caller's array: 200 calls alternating b = 2 and 4 leave free device memory where it
    was after the first two, and uspmv_spmmv_x_prepared / _release around a call change nothing"""
    t = torch_cuda
    P = pairs(32, 512)
    Ad, As = P.handles()
    _plan(pkg, P, Ad, As, 12, 2048)
    X = t.ones(4 * P.n, dtype=t.float64, device="cuda"); Y = t.zeros_like(X)
    for b in (4, 2):
        assert pkg.spmmv_ap_path(Ad, As, b, P.n, pkg.COLWISE)[0] == SWEEP
        pkg.spmmv_ap(Ad, As, X, Y, b, P.n, pkg.COLWISE)
    t.cuda.synchronize()
    free0, _ = t.cuda.mem_get_info()
    for k in range(200):
        pkg.spmmv_ap(Ad, As, X, Y, 2 if k % 2 == 0 else 4, P.n, pkg.COLWISE)
    t.cuda.synchronize()
    free1, _ = t.cuda.mem_get_info()
    assert free0 == free1, f"{free0 - free1} bytes of device memory gone over 200 calls"
    b, ld = 4, P.n + 32
    dX, want = P.case(b, 0, ld)
    pkg.spmmv_x_prepared(Ad, dX, b, ld)
    P.run(Ad, As, b, 0, ld, tag="prepared")
    pkg.spmmv_x_release(Ad)
    P.run(Ad, As, b, 0, ld, tag="released")


def test_default_chain_at_a_size_a_user_runs(pkg, orc, torch_cuda):
    """uspmv_dmat_optimize_ap on wide irregular rows installs the sweep plan (kind 2) with the single-vector kernel's window: under the
    default "sweep_nbuf" 1 that is 2^14 doubles, one vector fills the LDS and uspmv_spmmv_ap_sweep_vectors says 0 -- the block product
    keeps the gather kernel there; planned for two buffers (2^13 doubles), or through uspmv_dmat_optimize_sweep_ap with the window that
    uspmv_spmmv_ap_sweep_vectors names for b, it runs the sweep kernel.  Y = per-column uspmv_spmv_ap on the same handles, columns 0 and
    b - 1 = the oracle."""
    t = torch_cuda
    ds, ss = _pair_structs(pkg, pkg.gen_banded_random(120000, 140, 50000, magnitude_decades=10.0), 32, 512)
    da, sa = ds.arrays(), ss.arrays()
    n = ds.n_rows_padded
    xp = np.zeros(n); xp[:ds.n_rows] = pkg.apply_permutation(make_x(ds.n_rows), da["new_to_old_idx"])
    parts = tuple((q["chunk_ptrs"], q["chunk_lengths"], q["col_idxs"], q["values"]) for q in (da, sa))
    cols = t.stack([t.from_numpy(xp * (1.0 + v / 8.0)) for v in range(8)]).cuda()        # [8, n]: row v = column v of X
    y_or = {v: orc.spmv_scs_ap_adv(32, ds.n_chunks, parts[0], parts[1], cols[v].cpu().numpy()) for v in (0, 1, 7)}
    for how in ("optimize_ap", "optimize_ap, two buffers", "optimize_sweep_ap"):
        for b in (2, 8):
            Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
            if how == "optimize_sweep_ap":
                wlog = max(w for w in range(8, 17) if pkg.spmmv_ap_sweep_vectors(b, w) == b)   # all b vectors in one pass: 13 for 2, 11 for 8
                assert wlog == {2: 13, 8: 11}[b]
                pkg.optimize_sweep_ap(Ad, As, ds, ss, wlog, 0)
            else:
                pkg.set_tuning(sweep_nbuf=2 if "two" in how else 1)
                try:
                    pkg.optimize_ap(Ad, As, ds, ss)
                finally:
                    pkg.set_tuning(sweep_nbuf=1)
            kind, tiles, planned = Ad.plan_info()
            assert kind == 2 and planned == tiles > 0, (how, kind, tiles, planned)
            wlog = int(Ad.sweep_plan_digest()[1][2])
            assert wlog == {"optimize_ap": 14, "optimize_ap, two buffers": 13}.get(how, wlog)
            ycols = t.zeros((b, n), dtype=t.float64, device="cuda")
            for v in range(b):
                pkg.spmv_ap(Ad, As, cols[v], ycols[v])
            for v in (0, b - 1):
                assert np.array_equal(ycols[v].cpu().numpy(), y_or[v]), (how, b, v)
            for lay in (pkg.ROWWISE, pkg.COLWISE):
                assert pkg.spmmv_ap_path(Ad, As, b, n, lay) == _expected_path(pkg, b, wlog, lay == pkg.ROWWISE), (how, b, lay, wlog)
                if how == "optimize_sweep_ap": assert pkg.spmmv_ap_path(Ad, As, b, n, lay) == (SWEEP, b)
                dX = (cols[:b].t().contiguous() if lay == pkg.ROWWISE else cols[:b].contiguous()).reshape(-1)
                want = (ycols.t().contiguous() if lay == pkg.ROWWISE else ycols).reshape(-1)
                dY = t.full((b * n,), 9.0, dtype=t.float64, device="cuda")
                pkg.spmmv_ap(Ad, As, dX, dY, b, n, lay)
                assert t.equal(dY, want), (how, b, lay)
