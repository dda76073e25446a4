"""Adaptive-precision SpMMV (uspmv_spmmv_ap, csrc/ap_spmmv_kernels.hip): an ap[dp_sp] pair times a block of b vectors.  The contract is
bit-exactness per column: column v of Y is what scs_ap_impl_cpu<C> (the oracle's spmv_scs_ap_adv) gives for column v of X -- for every C,
both layouts, every kernel the dispatch can take and every plan the handles may carry.  No tolerance anywhere."""
import os

import numpy as np
import pytest

from conftest import block_x, golden, make_x, mtx_path

pytestmark = pytest.mark.gpu
SCALE = float(os.environ.get("USPMV_FULL_SCALE", "1.0"))
NAMES = ["bcsstk13", "impcol_e", "FDM-2d-16", "matrix1"]
WIDTHS = (1, 2, 3, 4, 5, 8, 13, 16)
GUARD = 64


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert pkg.device_count() >= 1
    torch.cuda.set_device(0)
    yield torch
    pkg.set_tuning(unroll=8, nontemporal=1, xcd_remap=256, block=256, spmmv_unroll=0, spmmv_variant=0, tlc=1, sweep=1, tlc_tile_rows=0)


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a)).cuda()


class Pair:
    """One golden ap[dp_sp] pair, built as test_ap_golden_bitexact builds it, with the oracle's Y per (b, layout, ld) computed once."""

    def __init__(self, pkg, orc, name):
        a = golden("ap.npz")
        p = name + "_"
        m = pkg.read_mtx(mtx_path(name))
        dp, sp = pkg.partition_precisions(m, float(a[p + "th"]))
        self.C, sg = int(a[p + "C"]), int(a[p + "sigma"])
        self.ds = pkg.convert_to_scs(dp, self.C, sg, pkg.F64)
        perm = self.ds.arrays()["old_to_new_idx"].copy()
        self.ss = pkg.convert_to_scs(sp, self.C, sg, pkg.F32, fixed_permutation=perm)
        pkg.permute_scs_cols(self.ds, perm); pkg.permute_scs_cols(self.ss, perm)
        self.n = self.ds.n_rows_padded
        self.xp = np.zeros(self.n); xg = a[p + "x_perm"]; self.xp[:min(self.n, len(xg))] = xg[:self.n]
        self.nnz = (dp.nnz, sp.nnz)
        self.orc, self.name, self._want = orc, name, {}
        da, sa = self.ds.arrays(), self.ss.arrays()
        self.parts = tuple((q["chunk_ptrs"].copy(), q["chunk_lengths"].copy(), q["col_idxs"].copy(), q["values"].copy()) for q in (da, sa))

    def handles(self, pkg):
        return pkg.DeviceMatrix(self.ds), pkg.DeviceMatrix(self.ss)

    def case(self, b, rowwise, ld):
        """(X, expected Y with 9.0 wherever the kernel must not write), both of b * ld + GUARD elements"""
        key = (b, rowwise, ld)
        if key not in self._want:
            n = self.n
            X = block_x(self.xp, n, b, ld, rowwise)
            want = np.full(b * ld + GUARD, 9.0)
            for v in range(b):
                xcol = np.ascontiguousarray(X[v:n * b:b] if rowwise else X[v * ld:v * ld + n])
                ycol = self.orc.spmv_scs_ap_adv(self.C, self.ds.n_chunks, self.parts[0], self.parts[1], xcol)
                if rowwise: want[v:n * b:b] = ycol
                else: want[v * ld:v * ld + n] = ycol
            self._want[key] = (X, want)
        return self._want[key]

    def shapes(self, b):
        return [(1, self.n), (0, self.n), (0, self.n + 32)]


@pytest.fixture(scope="module")
def pairs(pkg, orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Pair(pkg, orc, name)
        return cache[name]
    return get


def _run(pkg, t, P, Ad, As, b, rowwise, ld, offset=0, tag=""):
    """one call into a Y filled with 9.0 (+ guard zone); `offset` doubles into freshly allocated buffers (8-byte-aligned views)"""
    X, want = P.case(b, rowwise, ld)
    dXb = t.zeros(len(X) + offset, dtype=t.float64, device="cuda"); dX = dXb[offset:]; dX.copy_(_dev(t, X))
    dYb = t.full((len(want) + offset,), 9.0, dtype=t.float64, device="cuda"); dY = dYb[offset:]
    assert dX.data_ptr() % 16 == (8 * offset) % 16
    pkg.spmmv_ap(Ad, As, dX, dY, b, ld, pkg.ROWWISE if rowwise else pkg.COLWISE)
    got = dY.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{P.name} b={b} rowwise={rowwise} ld={ld} {tag}: {len(bad)} elements differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}")
    if offset: assert float(dYb[0]) == 9.0
    return dX, dY


def _grid(pkg, t, P, Ad, As, widths=WIDTHS, offset=0, tag=""):
    for b in widths:
        for rowwise, ld in P.shapes(b):
            _run(pkg, t, P, Ad, As, b, rowwise, ld, offset, tag)


@pytest.mark.parametrize("name", NAMES)
def test_golden_grid_bitexact(pkg, torch_cuda, pairs, name):
    """every width, both layouts, a padded leading dimension: written elements equal the oracle's, everything else of Y keeps its 9.0;
    and column v equals uspmv_spmv_ap on column v"""
    t = torch_cuda
    P = pairs(name)
    expect_nnz = {"bcsstk13": (67043, 16840), "impcol_e": (483, 825), "FDM-2d-16": (256, 960)}
    if name in expect_nnz: assert P.nnz == expect_nnz[name]
    else: assert P.nnz[0] > 0 and P.nnz[1] == 0           # matrix1: empty sp part, C = 10
    Ad, As = P.handles(pkg)
    for b in WIDTHS:
        for rowwise, ld in P.shapes(b):
            dX, dY = _run(pkg, t, P, Ad, As, b, rowwise, ld)
            for v in range(b):
                xcol = (dX[v:P.n * b:b] if rowwise else dX[v * ld:v * ld + P.n]).contiguous()
                ycol = t.full((P.n,), -3.0, dtype=t.float64, device="cuda")
                pkg.spmv_ap(Ad, As, xcol, ycol)
                assert t.equal(ycol, dY[v:P.n * b:b] if rowwise else dY[v * ld:v * ld + P.n]), (name, b, rowwise, ld, v)


@pytest.mark.parametrize("name", ["bcsstk13", "impcol_e"])
def test_every_kernel_same_bits(pkg, torch_cuda, pairs, name):
    t = torch_cuda
    P = pairs(name)
    Ad, As = P.handles(pkg)
    try:
        pkg.set_tuning(spmmv_variant=1)                          # the generic kernel for every width
        _grid(pkg, t, P, Ad, As, tag="variant 1")
        pkg.set_tuning(spmmv_variant=0)
        for nt in (0, 1):
            for xcd in (0, 1, 3):
                pkg.set_tuning(nontemporal=nt, xcd_remap=xcd)
                _grid(pkg, t, P, Ad, As, tag=f"nt={nt} xcd={xcd}")
        pkg.set_tuning(nontemporal=1, xcd_remap=256)
        for u in (1, 2, 4, 8):                                   # slots per batch of the row-major kernel
            pkg.set_tuning(spmmv_unroll=u)
            _grid(pkg, t, P, Ad, As, widths=(2, 4, 8, 16), tag=f"unroll={u}")
        pkg.set_tuning(spmmv_unroll=0)
        for block in (64, 1024):
            pkg.set_tuning(block=block)
            _grid(pkg, t, P, Ad, As, widths=(3, 4, 16), tag=f"block={block}")
        pkg.set_tuning(block=256)
        _grid(pkg, t, P, Ad, As, offset=1, tag="8-byte offset")     # X and Y not 16-byte aligned: the fallback
    finally:
        pkg.set_tuning(nontemporal=1, xcd_remap=256, spmmv_variant=0, spmmv_unroll=0, block=256)


@pytest.mark.parametrize("name", ["bcsstk13", "impcol_e"])
def test_planned_handles_same_bits(pkg, torch_cuda, pairs, name):
    """whatever plan the pair carries -- shared tile-local-column plan at any line budget and tile size, host- or device-built, switched
    off by tuning -- the block product keeps its bits (and the single-vector product its plan)"""
    t = torch_cuda
    P = pairs(name)
    try:
        for tile_rows in (256, 1024):
            for b in (2, 4, 8):
                for max_lines in sorted({0, 2, pkg.spmmv_ap_plan_lines(b)}):      # 2: mixed staged and gather tiles
                    Ad, As = P.handles(pkg)
                    pkg.set_tuning(tlc_tile_rows=tile_rows)
                    pkg.optimize_ap(Ad, As, P.ds, P.ss, max_lines)
                    pkg.set_tuning(tlc_tile_rows=0)
                    _grid(pkg, t, P, Ad, As, widths=(1, b, b + 1), tag=f"optimize_ap max_lines={max_lines} tile_rows={tile_rows}")
        Ad, As = P.handles(pkg)
        pkg.optimize_device_ap(Ad, As)
        _grid(pkg, t, P, Ad, As, tag="optimize_device_ap")
        pkg.set_tuning(tlc=0)
        _grid(pkg, t, P, Ad, As, tag="planned, tlc=0")
    finally:
        pkg.set_tuning(tlc=1, tlc_tile_rows=0)


def test_staged_kernel_over_the_shared_plan(pkg, orc, torch_cuda):
    """a stencil whose every tile fits the line budget of width 4: the pair planned with spmmv_ap_plan_lines(4) runs the kernel that
    stages the tile's X rows in LDS (scs_spmmv_ap_tlc) -- same bits; widths 2, 8 and 16 as well, at tile sizes whose line counts take
    them through one and through several passes over the vectors"""
    t = torch_cuda
    coo = pkg.gen_stencil27(24, 24, 24, dof=1, magnitude_decades=10.0)
    dp, sp = pkg.partition_precisions(coo, 1e-3)
    assert dp.nnz > 0 and sp.nnz > 0
    ds = pkg.convert_to_scs(dp, 32, 512, pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, 32, 512, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
    da, sa = ds.arrays(), ss.arrays()
    parts = tuple((q["chunk_ptrs"], q["chunk_lengths"], q["col_idxs"], q["values"]) for q in (da, sa))
    n = ds.n_rows_padded
    xp = np.zeros(n); xp[:ds.n_rows] = pkg.apply_permutation(make_x(ds.n_rows), da["new_to_old_idx"])
    for b in (4, 2, 8, 16):
        budget = pkg.spmmv_ap_plan_lines(b)
        assert budget > 0 and budget * 128 * 2 <= 160 * 1024
        for tile_rows in (0, 256, 1024):
            Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
            pkg.set_tuning(tlc_tile_rows=tile_rows)
            try:
                pkg.optimize_ap(Ad, As, ds, ss, budget)
            finally:
                pkg.set_tuning(tlc_tile_rows=0)
            kind, tiles, planned = Ad.plan_info()
            if b == 4 and tile_rows == 0:
                assert kind == 1 and planned == tiles > 0, (kind, tiles, planned)
                assert Ad.plan_download()["max_lines_used"] <= budget
            for rowwise, ld in ((1, n), (0, n), (0, n + 32)):
                X = block_x(xp, n, b, ld, rowwise)
                want = np.full(b * ld + GUARD, 9.0)
                for v in range(b):
                    xcol = np.ascontiguousarray(X[v:n * b:b] if rowwise else X[v * ld:v * ld + n])
                    ycol = orc.spmv_scs_ap_adv(32, ds.n_chunks, parts[0], parts[1], xcol)
                    if rowwise: want[v:n * b:b] = ycol
                    else: want[v * ld:v * ld + n] = ycol
                for nt in (1, 0):
                    pkg.set_tuning(nontemporal=nt)
                    try:
                        dY = t.full((len(want),), 9.0, dtype=t.float64, device="cuda")
                        pkg.spmmv_ap(Ad, As, _dev(t, X), dY, b, ld, pkg.ROWWISE if rowwise else pkg.COLWISE)
                    finally:
                        pkg.set_tuning(nontemporal=1)
                    assert np.array_equal(dY.cpu().numpy(), want), (b, tile_rows, rowwise, ld, nt, kind, tiles, planned)


# uspmv_spmmv_ap_path of the impcol_e pair planned with spmmv_ap_plan_lines(b), under ("tlc" 1, "tlc" 0, "spmmv_variant" 1): the staged, the
# gather and the lane-per-row kernel.  The matrix yields the shared line plan (plan_info kind 1) at C = 8 as well as at C = 32, and the
# commit before the pair moved to the shared kernels reports the same 2, 1, 0 at both (with 2 and 8 vectors per pass at b = 2 and 16).
SHARED_KERNEL_PATHS = (2, 1, 0)


@pytest.mark.parametrize("C", [8, 32])
def test_pair_on_the_shared_block_kernels(pkg, torch_cuda, C):
    """ap[dp_sp] runs the lane-per-row and the staged kernel that every ap kind shares (csrc/ap_hp_spmmv_kernels.hip, last part float):
    impcol_e (225 rows) at C = 8 and C = 32, b = 2 and b = 16, both layouts, the pair planned with spmmv_ap_plan_lines(b).  Under "tlc" 1,
    "tlc" 0 and "spmmv_variant" 1 every column of Y is bitwise uspmv_spmv_ap of that column of X, and uspmv_spmmv_ap_path reports
    2, 1 and 0 (SHARED_KERNEL_PATHS)."""
    t = torch_cuda
    a = golden("ap.npz")
    m = pkg.read_mtx(mtx_path("impcol_e"))
    assert m.n_rows == 225
    dp, sp = pkg.partition_precisions(m, float(a["impcol_e_th"]))
    assert dp.nnz > 0 and sp.nnz > 0
    ds = pkg.convert_to_scs(dp, C, int(a["impcol_e_sigma"]), pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, C, int(a["impcol_e_sigma"]), pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
    n = ds.n_rows_padded
    xp = np.zeros(n); xp[:ds.n_rows] = pkg.apply_permutation(make_x(ds.n_rows), ds.arrays()["new_to_old_idx"])
    tunings = (dict(tlc=1), dict(tlc=0), dict(spmmv_variant=1))
    try:
        for b in (2, 16):
            Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
            pkg.optimize_ap(Ad, As, ds, ss, pkg.spmmv_ap_plan_lines(b))
            assert Ad.plan_info()[0] == 1                             # the shared line plan
            for rowwise, ld in ((1, n), (0, n), (0, n + 32)):
                lay = pkg.ROWWISE if rowwise else pkg.COLWISE
                dX = _dev(t, block_x(xp, n, b, ld, rowwise))
                want = t.full((b * ld + GUARD,), 9.0, dtype=t.float64, device="cuda")
                for v in range(b):                                     # the single-vector product of every column, once
                    xcol = (dX[v:n * b:b] if rowwise else dX[v * ld:v * ld + n]).contiguous()
                    ycol = t.full((n,), -3.0, dtype=t.float64, device="cuda")
                    pkg.spmv_ap(Ad, As, xcol, ycol)
                    if rowwise: want[v:n * b:b] = ycol
                    else: want[v * ld:v * ld + n] = ycol
                for tune, path in zip(tunings, SHARED_KERNEL_PATHS):
                    pkg.set_tuning(tlc=1, spmmv_variant=0)
                    pkg.set_tuning(**tune)
                    got_path = pkg.spmmv_ap_path(Ad, As, b, ld, lay)[0]
                    assert got_path == path, (C, b, rowwise, ld, tune, got_path)
                    dY = t.full((b * ld + GUARD,), 9.0, dtype=t.float64, device="cuda")
                    pkg.spmmv_ap(Ad, As, dX, dY, b, ld, lay)
                    assert t.equal(dY, want), (C, b, rowwise, ld, tune)
    finally:
        pkg.set_tuning(tlc=1, spmmv_variant=0)


def test_prepared_x(pkg, torch_cuda, pairs):
    """uspmv_spmmv_x_prepared on the dp handle: the re-layout once, then calls that skip it; a new X needs a new call; release returns
    to the per-call pass"""
    t = torch_cuda
    P = pairs("bcsstk13")
    Ad, As = P.handles(pkg)
    b, ld = 8, P.n + 32
    X, want = P.case(b, 0, ld)
    dX = _dev(t, X)
    pkg.spmmv_x_prepared(Ad, dX, b, ld)
    for _ in range(2):
        dY = t.full((len(want),), 9.0, dtype=t.float64, device="cuda")
        pkg.spmmv_ap(Ad, As, dX, dY, b, ld, pkg.COLWISE)
        assert np.array_equal(dY.cpu().numpy(), want)
    dX.mul_(2.0)                                                  # X written in place: prepare again
    pkg.spmmv_x_prepared(Ad, dX, b, ld)
    dY = t.full((len(want),), 9.0, dtype=t.float64, device="cuda")
    pkg.spmmv_ap(Ad, As, dX, dY, b, ld, pkg.COLWISE)
    mask = np.full(len(want), False)
    for v in range(b): mask[v * ld:v * ld + P.n] = True
    want2 = np.where(mask, 2.0 * want, 9.0)                      # (a power of two: exact)
    assert np.array_equal(dY.cpu().numpy(), want2)
    # another width in between overwrites the workspace and ends the preparation by itself
    X4, want4 = P.case(4, 0, P.n)
    dY4 = t.full((len(want4),), 9.0, dtype=t.float64, device="cuda")
    pkg.spmmv_ap(Ad, As, _dev(t, X4), dY4, 4, P.n, pkg.COLWISE)
    assert np.array_equal(dY4.cpu().numpy(), want4)
    dY.fill_(9.0)
    pkg.spmmv_ap(Ad, As, dX, dY, b, ld, pkg.COLWISE)
    assert np.array_equal(dY.cpu().numpy(), want2)
    pkg.spmmv_x_prepared(Ad, dX, b, ld)
    pkg.spmmv_x_release(Ad)
    dX.mul_(0.5)                                                  # released: the per-call path sees the new contents
    dY.fill_(9.0)
    pkg.spmmv_ap(Ad, As, dX, dY, b, ld, pkg.COLWISE)
    assert np.array_equal(dY.cpu().numpy(), want)


def test_refusals(pkg, torch_cuda, pairs):
    t = torch_cuda
    P, Q = pairs("bcsstk13"), pairs("impcol_e")
    Ad, As = P.handles(pkg)
    Qd, Qs = Q.handles(pkg)
    assert Q.ds.n_chunks != P.ds.n_chunks and Q.C == P.C
    X = t.ones(4 * P.n, dtype=t.float64, device="cuda"); Y = t.zeros_like(X)
    with pytest.raises(pkg.UspmvError): pkg.spmmv_ap(As, Ad, X, Y, 4, P.n)                 # swapped handles
    with pytest.raises(pkg.UspmvError): pkg.spmmv_ap(Ad, As, X, Y, 0, P.n)
    with pytest.raises(pkg.UspmvError): pkg.spmmv_ap(Ad, As, X, Y, 4, P.n, 7)              # unknown layout
    with pytest.raises(pkg.UspmvError): pkg.spmmv_ap(Ad, As, X, Y, 4, P.n - 1, pkg.COLWISE)
    pkg.spmmv_ap(Ad, As, X, Y, 4, P.n - 1, pkg.ROWWISE)                                    # (ld is ignored for rowwise)
    with pytest.raises(pkg.UspmvError): pkg.spmmv_ap(Ad, Qs, X, Y, 4, P.n)                 # different n_chunks
    assert t.all(t.isfinite(Y))


def test_workspace_is_allocated_once(pkg, torch_cuda, pairs):
    """200 column-major calls alternating b = 4 and b = 8 on one pair: free device memory stays where it was after the first two"""
    t = torch_cuda
    P = pairs("bcsstk13")
    Ad, As = P.handles(pkg)
    X = t.ones(8 * P.n, dtype=t.float64, device="cuda"); Y = t.zeros_like(X)
    for b in (8, 4):
        pkg.spmmv_ap(Ad, As, X, Y, b, P.n, pkg.COLWISE)
    t.cuda.synchronize()
    free0, _ = t.cuda.mem_get_info()
    for k in range(200):
        pkg.spmmv_ap(Ad, As, X, Y, 4 if k % 2 == 0 else 8, P.n, pkg.COLWISE)
    t.cuda.synchronize()
    free1, _ = t.cuda.mem_get_info()
    assert free0 == free1, f"{free0 - free1} bytes of device memory gone over 200 calls"


def _full_size_case(pkg, orc, t, coo, tag, want_kind):
    dp, sp = pkg.partition_precisions(coo, 1e-3)
    assert dp.nnz > 0 and sp.nnz > 0
    ds = pkg.convert_to_scs(dp, 32, 512, pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, 32, 512, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
    da, sa = ds.arrays(), ss.arrays()
    Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
    pkg.optimize_ap(Ad, As, ds, ss)
    kind, tiles, planned = Ad.plan_info()
    assert kind == want_kind, (tag, kind, tiles, planned)
    b, n = 8, ds.n_rows_padded
    xp = np.zeros(n); xp[:ds.n_rows] = pkg.apply_permutation(make_x(ds.n_rows), da["new_to_old_idx"])
    print(f"\n[{tag}] n={ds.n_rows} dp nnz={dp.nnz} sp nnz={sp.nnz} plan kind {kind}: {planned}/{tiles} tiles", flush=True)
    cols = t.stack([t.from_numpy(xp * (1.0 + v / 8.0)) for v in range(b)]).cuda()        # [b, n]: row v = column v of X
    ycols = t.zeros_like(cols)
    for v in range(b):
        pkg.spmv_ap(Ad, As, cols[v], ycols[v])           # pinned to the oracle at this size by test_gpu_fullsize.py
    for v in (0, 7):
        y_or = orc.spmv_scs_ap_adv(32, ds.n_chunks, (da["chunk_ptrs"], da["chunk_lengths"], da["col_idxs"], da["values"]),
                                   (sa["chunk_ptrs"], sa["chunk_lengths"], sa["col_idxs"], sa["values"]), cols[v].cpu().numpy())
        assert np.array_equal(ycols[v].cpu().numpy(), y_or), (tag, "column", v)
    for lay in (pkg.ROWWISE, pkg.COLWISE):
        dX = (cols.t().contiguous() if lay == pkg.ROWWISE else cols).reshape(-1)
        want = (ycols.t().contiguous() if lay == pkg.ROWWISE else ycols).reshape(-1)
        dY = t.full((b * n,), 9.0, dtype=t.float64, device="cuda")
        pkg.spmmv_ap(Ad, As, dX, dY, b, n, lay)
        assert t.equal(dY, want), (tag, "layout", lay)
        dY2 = t.full((b * n,), 9.0, dtype=t.float64, device="cuda")
        pkg.spmmv_ap(Ad, As, 2.0 * dX, dY2, b, n, lay)
        assert t.equal(dY2, 2.0 * dY), (tag, "linearity", lay)


def test_full_size_config4_stencil(pkg, orc, torch_cuda):
    """config 4's regular stand-in (5 dof on 74^3 nodes, 10 decades, threshold 1e-3, SELL-32-512), b = 8, on the shared plan
    uspmv_dmat_optimize_ap installs"""
    g = max(6, int(74 * SCALE))
    _full_size_case(pkg, orc, torch_cuda, pkg.gen_stencil27(g, g, g, dof=5, magnitude_decades=10.0), "ap spmmv cfg4", 1)


def test_full_size_config4b_banded_random(pkg, orc, torch_cuda):
    """the banded-random matrix of config 4b: the pair carries the column-window sweep plan, which does not apply to block vectors and
    is ignored"""
    n = max(200000, int(2017169 * SCALE ** 3))
    _full_size_case(pkg, orc, torch_cuda, pkg.gen_banded_random(n, 140, 50000, magnitude_decades=10.0), "ap spmmv cfg4b", 2)
