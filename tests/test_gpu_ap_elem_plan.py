"""The shared tile-local-column plan over single x ELEMENTS for the four adaptive-precision kinds (ap[dp_sp], ap[dp_hp], ap[sp_hp],
ap[dp_sp_hp]): the planners' fallback order lines -> elements -> sweep (csrc/tlc_planner.hip: elements_take_over, the policy one-precision
handles have), the host and the device planner equal array for array (csrc/plan_kernels.hip), and the ELEM staging arm of
scs_spmv_ap_tlc / scs_spmv_ap_hp_tlc (csrc/ap_kernels.hip).  Every y is compared bit for bit with the oracle's ap result for the same
structs, composed as tests/test_gpu_ap_hp.py composes it:
  ap[dp_sp], ap[dp_hp]  spmv_scs_ap_adv (the second part's values as float32: exact)
  ap[dp_sp_hp]          spmv_scs of every part with its values widened to float64, then (d + s) + h
  ap[sp_hp]             spmv_scs_ap with an empty dp part, once per part (float x), then float32(sp + hp)
The kinds with an fp16 part fall to the element plan by themselves ("tlc_elem" 1).  An ap[dp_sp] pair does so from 2^20 padded rows on
(its own test below) and under "tlc_elem" 2 at every size: tests/test_gpu_elem_plan_device.py::test_ap_pair_keeps_lines_then_sweep pins
the ap[dp_sp] pair of the scattered matrix used here (192 000 rows) to lines -> sweep at the default setting, so the
ap[dp_sp] cases on that matrix set the key around the planner call."""
import numpy as np
import pytest

from conftest import make_x, mtx_path

pytestmark = pytest.mark.gpu

KINDS = ("dp_sp", "dp_hp", "sp_hp", "dp_sp_hp")


@pytest.fixture(scope="module")
def t(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch


def scrambled_columns(pkg, g, dof, K, seed=3):
    """27-point x dof stencil on g^3 nodes with the COLUMNS' nodes renumbered at random inside consecutive blocks of K nodes (the generator
    of tests/test_gpu_elem_plan.py)."""
    base = pkg.gen_stencil27(g, g, g, dof=dof)
    I, J, V = (np.array(a) for a in base.arrays())
    n = base.n_rows
    nn = n // dof
    rng = np.random.default_rng(seed)
    p = np.arange(nn, dtype=np.int64)
    for s0 in range(0, nn, K):
        seg = p[s0:s0 + K].copy(); rng.shuffle(seg); p[s0:s0 + K] = seg
    J2 = (p[J // dof] * dof + J % dof).astype(np.int32)
    o = np.lexsort((J2, I))
    return pkg.Coo.from_arrays(n, n, I[o], J2[o], V[o])


def _quantiles(m, kind):
    """(t1, t2): quantiles of |v| that leave every part non-empty; the boundary below which values go to binary16 stays under its largest
    finite value, so no part overflows to inf (bcsstk13 reaches 1e12)."""
    a = np.abs(np.asarray(m.arrays()[2]))
    a = a[a > 0]
    t1, t2 = float(np.quantile(a, 0.7)), float(np.quantile(a, 0.35))
    if kind in ("dp_hp", "sp_hp"):
        t1 = min(t1, 6e4)
    t2 = min(t2, 6e4)
    return t1, t2


class Split:
    """The structs of one split (first, mid | None, last) in one row order, x in the structs' column numbering and the oracle's y."""

    def __init__(self, pkg, orc, m, kind, C, sigma, t1, t2, permute_cols):
        self.kind, self.C = kind, C
        if kind == "dp_sp":
            hi, lo = pkg.partition_precisions(m, t1)
            mid = None
        else:
            hi, mid, lo = pkg.partition_precisions_hp(m, kind, t1, t2)
        self.nnz = (hi.nnz, mid.nnz if mid is not None else None, lo.nnz)
        sh = pkg.convert_to_scs(hi, C, sigma, pkg.F32 if kind == "sp_hp" else pkg.F64)
        perm = sh.arrays()["old_to_new_idx"].copy()
        sm = pkg.convert_to_scs(mid, C, sigma, pkg.F32, fixed_permutation=perm) if mid is not None else None
        sl = pkg.convert_to_scs(lo, C, sigma, pkg.F32 if kind == "dp_sp" else pkg.F16, fixed_permutation=perm)
        self.structs = (sh, sm, sl)
        xdt = np.float32 if kind == "sp_hp" else np.float64
        if permute_cols:                                   # square: columns in the rows' order, x permuted alike
            for s in self.structs:
                if s is not None:
                    pkg.permute_scs_cols(s, perm)
            x = np.zeros(sh.n_rows_padded)
            x[:m.n_rows] = make_x(m.n_rows)[sh.arrays()["new_to_old_idx"]]
        else:                                              # x in a numbering of its own
            x = np.zeros(max(sh.n_rows_padded, m.n_cols))
            x[:m.n_cols] = make_x(m.n_cols)
        self.x = x.astype(xdt)
        self.n_pad = sh.n_rows_padded
        self.want = self._oracle(orc)

    def _oracle(self, orc):
        def tup(s, dt):
            a = s.arrays()
            return (a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"].astype(dt))
        sh, sm, sl = self.structs
        C, nc, x = sh.C, sh.n_chunks, self.x
        if self.kind in ("dp_sp", "dp_hp"):
            return orc.spmv_scs_ap_adv(C, nc, tup(sh, np.float64), tup(sl, np.float32), x)
        if self.kind == "dp_sp_hp":
            return (orc.spmv_scs(C, nc, *tup(sh, np.float64), x) + orc.spmv_scs(C, nc, *tup(sm, np.float64), x)) + orc.spmv_scs(C, nc, *tup(sl, np.float64), x)
        empty = (np.zeros(nc + 1, np.int32), np.zeros(nc, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))
        a = orc.spmv_scs_ap(C, nc, empty, tup(sh, np.float32), x.astype(np.float64), x)
        b = orc.spmv_scs_ap(C, nc, empty, tup(sl, np.float32), x.astype(np.float64), x)
        return (a + b).astype(np.float32)

    # ---- device side
    def handles(self, pkg):
        return [pkg.DeviceMatrix(s) if s is not None else None for s in self.structs]

    def plan_host(self, pkg, hand, **tuning):
        return _planned(pkg, tuning, lambda: pkg.optimize_ap(hand[0], hand[2], self.structs[0], self.structs[2]) if self.kind == "dp_sp"
                        else pkg.optimize_ap_hp(hand[0], hand[1], hand[2], *self.structs))

    def plan_device(self, pkg, hand, **tuning):
        return _planned(pkg, tuning, lambda: pkg.optimize_device_ap(hand[0], hand[2]) if self.kind == "dp_sp"
                        else pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2]))

    def forced(self):
        """the tuning under which a split of the 192 000-row scattered matrix falls to the element plan"""
        return dict(tlc_elem=2) if self.kind == "dp_sp" else {}

    def y(self, pkg, t, hand, tiles=None):
        x = t.from_numpy(self.x).cuda()
        y = t.full((self.n_pad,), -3.0, dtype=x.dtype, device="cuda")
        if self.kind == "dp_sp":
            pkg.spmv_ap(hand[0], hand[2], x, y) if tiles is None else pkg.spmv_ap_tiles(hand[0], hand[2], tiles, x, y)
        else:
            pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y) if tiles is None else pkg.spmv_ap_hp_tiles(hand[0], hand[1], hand[2], tiles, x, y)
        return y.cpu().numpy()


DEFAULTS = dict(tlc_elem=1, tlc_elem_cap=4096)


def _planned(pkg, tuning, call):
    pkg.set_tuning(**tuning) if tuning else None
    try:
        return call()
    finally:
        if tuning:
            pkg.set_tuning(**{k: DEFAULTS[k] for k in tuning})


def _same(got, want):
    """bit for bit; a NaN equals any NaN, as in tests/test_gpu_ap_hp.py (sign and payload of an inf - inf differ between CPU and GPU: the
    split whose binary16 part holds all of bcsstk13 has such rows)"""
    nan = np.isnan(want)
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return got.dtype == want.dtype and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(u), want[~nan].view(u))


def _gran(hand):
    return [h.plan_granularity() for h in hand if h is not None]


def _plans_equal(a_hand, b_hand):
    for part, (a, b) in enumerate((a, b) for a, b in zip(a_hand, b_hand) if a is not None):
        pa, pb = a.plan_download(), b.plan_download()
        assert pa is not None and pb is not None, part
        # (the element list lives with the first part; the further parts hold their local indices only)
        for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16") if part == 0 else ("c16_ptrs", "col16"):
            assert np.array_equal(pa[k], pb[k]), (part, k)
        assert pa["max_lines_used"] == pb["max_lines_used"], part


@pytest.fixture(scope="module")
def scattered(pkg):
    return scrambled_columns(pkg, 40, 3, 8000)       # <= 1 512 distinct columns per 256-row tile, on ~2 000 lines: no line plan stages it


_SPLITS = {}


def _scattered_split(pkg, orc, scattered, kind, C, sigma):
    """one split of the scattered matrix per (kind, C, sigma), built once for the module (structs, x, oracle y: read only)"""
    key = (kind, C, sigma)
    if key not in _SPLITS:
        t1, t2 = _quantiles(scattered, kind)
        sp = Split(pkg, orc, scattered, kind, C, sigma, t1, t2, permute_cols=False)
        assert all(n is None or n > 0 for n in sp.nnz), sp.nnz          # the quantiles leave every part non-empty
        _SPLITS[key] = sp
    return _SPLITS[key]


# ---- 1. scattered columns, host planner -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C,sigma", [("dp_sp", 32, 512), ("dp_sp", 64, 128), ("dp_sp", 32, 1), ("dp_hp", 32, 512), ("sp_hp", 32, 512),
                                          ("dp_sp_hp", 32, 512)])
def test_scattered_columns_host_planner(pkg, orc, t, scattered, kind, C, sigma):
    sp = _scattered_split(pkg, orc, scattered, kind, C, sigma)
    hand = sp.handles(pkg)
    nt, ns = sp.plan_host(pkg, hand, **sp.forced())
    assert _gran(hand) == [1] * len(_gran(hand)), (kind, _gran(hand))
    assert nt > 0 and ns == nt, (nt, ns)
    assert all(h.plan_info() == (1, nt, nt) for h in hand if h is not None)
    assert _same(sp.y(pkg, t, hand), sp.want)
    ids = t.tensor([1, 3, 0], dtype=t.int32, device="cuda")
    got = sp.y(pkg, t, hand, tiles=ids)
    for tile in (0, 1, 3):
        assert _same(got[tile * 256:(tile + 1) * 256], sp.want[tile * 256:(tile + 1) * 256]), tile
    assert np.all(got[2 * 256:3 * 256] == -3.0) and np.all(got[4 * 256:] == -3.0)       # the sentinel survives outside the list


# ---- 2. device planner ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C,sigma", [("dp_sp", 32, 512), ("dp_sp", 64, 128), ("dp_hp", 32, 512), ("sp_hp", 32, 512), ("dp_sp_hp", 32, 512)])
def test_device_planner_equals_the_host_planner(pkg, orc, t, scattered, kind, C, sigma):
    sp = _scattered_split(pkg, orc, scattered, kind, C, sigma)
    hh, hd = sp.handles(pkg), sp.handles(pkg)
    res_h = sp.plan_host(pkg, hh, **sp.forced())
    res_d = sp.plan_device(pkg, hd, **sp.forced())
    assert _gran(hd) == [1] * len(_gran(hd)) and _gran(hh) == _gran(hd), (kind, _gran(hh), _gran(hd))
    assert res_d == res_h and res_d[0] == res_d[1] > 0
    _plans_equal(hh, hd)
    assert _same(sp.y(pkg, t, hd), sp.want)
    ids = t.tensor([1, 3, 0], dtype=t.int32, device="cuda")
    got = sp.y(pkg, t, hd, tiles=ids)
    for tile in (0, 1, 3):
        assert _same(got[tile * 256:(tile + 1) * 256], sp.want[tile * 256:(tile + 1) * 256]), tile
    assert np.all(got[2 * 256:3 * 256] == -3.0)


def test_device_planner_on_handles_set_up_on_the_device(pkg, orc, t, scattered):
    """ap[dp_sp_hp] handles that never had a host struct (uspmv_convert_to_scs_device_ap_from_arrays): element plan, the host conversion's bits"""
    I, J, V = (np.array(a) for a in scattered.arrays())
    t1, t2 = _quantiles(scattered, "dp_sp_hp")
    dI, dJ, dV = (t.from_numpy(np.ascontiguousarray(a)).cuda() for a in (I, J, V))
    _, hand, _, _, part_nnz = pkg.convert_ap_device_from_arrays(dI, dJ, dV, scattered.n_rows, scattered.n_cols, 32, 512, "dp_sp_hp", t1, t2)
    assert all(c > 0 for c in part_nnz)
    pkg.optimize_device_ap_hp(hand[0], hand[1], hand[2])
    assert _gran(hand) == [1, 1, 1], _gran(hand)
    # the same conversion on the host: columns permuted by the set-up, x permuted alike
    sp = Split(pkg, orc, scattered, "dp_sp_hp", 32, 512, t1, t2, permute_cols=True)
    assert _same(sp.y(pkg, t, hand), sp.want)


# ---- the ap[dp_sp] pair by itself: from 2^20 padded rows on ------------------------------------------------------------------------------
def _grouped_scattered(pkg, n_rows, K=40000, per_row=16, rows_per_group=5, seed=5):
    """rows i of a group of five share 16 columns, the columns renumbered at random inside blocks of K: a 256-row tile lists 832 distinct
    columns (4.9 entries per element) on more x lines than a line plan may list -- the smallest entry count at which a pair of 2^20 rows
    meets the element plan's conditions"""
    n_groups = (n_rows + rows_per_group - 1) // rows_per_group
    n_cols = n_groups * per_row
    rng = np.random.default_rng(seed)
    q = np.arange(n_cols, dtype=np.int32)
    for s0 in range(0, n_cols, K):
        rng.shuffle(q[s0:s0 + K])
    rows = np.arange(n_rows, dtype=np.int64)
    J = q[((rows // rows_per_group) * per_row)[:, None] + np.arange(per_row)[None, :]]
    J.sort(axis=1)
    I = np.repeat(rows.astype(np.int32), per_row)
    V = rng.uniform(-1.0, 1.0, I.size)
    V[np.abs(V) < 1e-3] = 0.5
    return pkg.Coo.from_arrays(n_rows, n_cols, I, np.ascontiguousarray(J.reshape(-1)), V)


@pytest.mark.parametrize("log2_rows,by_itself", [(20, True), (19, False)])
def test_ap_dp_sp_pair_takes_the_element_plan_by_itself_from_2_20_rows(pkg, orc, t, log2_rows, by_itself):
    """the size rule of the pair's default (csrc/tlc_planner.hip ap_elements_by_default), either side of it, both planners, no tuning key"""
    m = _grouped_scattered(pkg, 1 << log2_rows)
    sp = Split(pkg, orc, m, "dp_sp", 32, 1, 0.5, 0.0, permute_cols=False)
    assert sp.n_pad == 1 << log2_rows and all(n is None or n > 0 for n in sp.nnz)
    hh, hd = sp.handles(pkg), sp.handles(pkg)
    sp.plan_host(pkg, hh)
    sp.plan_device(pkg, hd)
    assert _gran(hh) == _gran(hd)
    if by_itself:
        assert _gran(hh) == [1, 1] and all(h.plan_info()[0] == 1 and h.plan_info()[1] == h.plan_info()[2] for h in hh if h is not None), (_gran(hh), hh[0].plan_info())
        _plans_equal(hh, hd)
    else:
        assert 1 not in _gran(hh), _gran(hh)
    for hand in (hh, hd):
        assert _same(sp.y(pkg, t, hand), sp.want)


# ---- 3. the cap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dp_sp", "dp_sp_hp"])
def test_tiles_over_the_cap_keep_the_other_plans(pkg, orc, t, scattered, kind):
    sp = _scattered_split(pkg, orc, scattered, kind, 32, 512)
    for plan in (sp.plan_host, sp.plan_device):
        hand = sp.handles(pkg)
        try:
            plan(pkg, hand, tlc_elem_cap=1100, **sp.forced())        # the tiles list more elements than that
        finally:
            pkg.set_tuning(**DEFAULTS)
        assert 1 not in _gran(hand), _gran(hand)
        assert _same(sp.y(pkg, t, hand), sp.want)


# ---- 4. a regular numbering keeps its line plan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_regular_numbering_keeps_the_line_plan_unless_forced(pkg, orc, t, kind):
    m = pkg.gen_stencil27(16, 16, 16, dof=3)
    sp = Split(pkg, orc, m, kind, 32, 512, *_quantiles(m, kind), permute_cols=True)
    for plan in (sp.plan_host, sp.plan_device):
        hand = sp.handles(pkg)
        nt, ns = plan(pkg, hand)
        assert _gran(hand) == [16] * len(_gran(hand)) and ns == nt
        assert _same(sp.y(pkg, t, hand), sp.want)
        forced = sp.handles(pkg)
        plan(pkg, forced, tlc_elem=2)
        assert _gran(forced) == [1] * len(_gran(forced))
        assert _same(sp.y(pkg, t, forced), sp.want)


# ---- 5. edges, forced --------------------------------------------------------------------------------------------------------------------
def _forced_both_planners(pkg, t, sp, want_elem=True):
    hh, hd = sp.handles(pkg), sp.handles(pkg)
    sp.plan_host(pkg, hh, tlc_elem=2)
    sp.plan_device(pkg, hd, tlc_elem=2)
    assert _gran(hh) == _gran(hd)
    if want_elem:
        assert _gran(hh) == [1] * len(_gran(hh)), (sp.kind, _gran(hh))
        _plans_equal(hh, hd)
    for hand in (hh, hd):
        assert _same(sp.y(pkg, t, hand), sp.want), sp.kind


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,C,sigma", [("bcsstk13", 32, 1), ("bcsstk13", 64, 1), ("impcol_e", 32, 1), ("impcol_e", 16, 1)])
def test_golden_matrices_ragged_tiles(pkg, orc, t, kind, name, C, sigma):
    """bcsstk13: 2003 rows -- the last tile is partial, n no multiple of 16; impcol_e: 225 rows -- one partial tile"""
    m = pkg.read_mtx(mtx_path(name))
    sp = Split(pkg, orc, m, kind, C, sigma, *_quantiles(m, kind), permute_cols=True)
    assert all(n is None or n > 0 for n in sp.nnz) and np.all(np.isfinite(sp.want))
    _forced_both_planners(pkg, t, sp)


def _wide(pkg, n_rows=700, n_cols=1531, per_row=9, seed=11):
    rng = np.random.default_rng(seed)
    I = np.repeat(np.arange(n_rows, dtype=np.int32), per_row)
    J = np.concatenate([np.sort(rng.choice(n_cols, per_row, replace=False)) for _ in range(n_rows)]).astype(np.int32)
    J[-1] = n_cols - 1                                       # the last column is referenced (by the last row, its largest column)
    V = rng.uniform(-1.0, 1.0, I.size)
    V[np.abs(V) < 1e-3] = 0.5
    return pkg.Coo.from_arrays(n_rows, n_cols, I, J, V)


@pytest.mark.parametrize("kind", KINDS)
def test_more_columns_than_rows(pkg, orc, t, kind):
    m = _wide(pkg)
    assert int(np.asarray(m.arrays()[1]).max()) == m.n_cols - 1
    sp = Split(pkg, orc, m, kind, 32, 64, *_quantiles(m, kind), permute_cols=False)
    _forced_both_planners(pkg, t, sp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["first_empty", "last_empty"])
def test_a_split_with_an_empty_part(pkg, orc, t, kind, which):
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    big = 10.0 * float(np.abs(np.asarray(m.arrays()[2])).max())
    # a threshold above every |v| empties the first part, one below every |v| the last (ap[dp_sp_hp]: the mid part goes with the side that empties)
    t1, t2 = (big, big) if which == "first_empty" else (0.0, 0.0)
    sp = Split(pkg, orc, m, kind, 32, 1, t1, t2, permute_cols=True)
    assert (sp.nnz[0] == 0) if which == "first_empty" else (sp.nnz[2] == 0), sp.nnz
    _forced_both_planners(pkg, t, sp)


# ---- 6. block vectors on handles that carry the element plan -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_block_vectors_take_a_non_staged_path(pkg, orc, t, scattered, kind):
    sp = _scattered_split(pkg, orc, scattered, kind, 32, 512)
    hand = sp.handles(pkg)
    sp.plan_host(pkg, hand, **sp.forced())
    assert _gran(hand) == [1] * len(_gran(hand))
    y1 = sp.y(pkg, t, hand)
    assert _same(y1, sp.want)
    n, ld = sp.n_pad, len(sp.x)
    ids = t.tensor([1, 3, 0], dtype=t.int32, device="cuda")
    for b in (2, 4):
        for layout in (pkg.COLWISE, pkg.ROWWISE):
            X = np.zeros((b, ld), sp.x.dtype)
            for v in range(b):
                X[v] = sp.x * (1.0 if v == 0 else 0.0)          # column 0 carries x; the others zeros
            Xl = X if layout == pkg.COLWISE else np.ascontiguousarray(X.T)
            dX = t.from_numpy(np.ascontiguousarray(Xl).reshape(-1)).cuda()
            dY = t.full((b * ld,), -3.0, dtype=dX.dtype, device="cuda")
            if kind == "dp_sp":
                path, _ = pkg.spmmv_ap_path(hand[0], hand[2], b, ld, layout)
                tpath, _ = pkg.spmmv_ap_tiles_path(hand[0], hand[2], b, ld, layout)
                pkg.spmmv_ap(hand[0], hand[2], dX, dY, b, ld, layout)
            else:
                path, _ = pkg.spmmv_ap_hp_path(hand[0], hand[1], hand[2], b, ld, layout)
                tpath, _ = pkg.spmmv_ap_hp_tiles_path(hand[0], hand[1], hand[2], b, ld, layout)
                pkg.spmmv_ap_hp(hand[0], hand[1], hand[2], dX, dY, b, ld, layout)
            assert path in (0, 1) and tpath == 0, (kind, b, layout, path, tpath)      # neither staged (2) nor sweep (3)
            Y = dY.cpu().numpy()
            Y = Y.reshape(b, ld) if layout == pkg.COLWISE else Y.reshape(ld, b).T
            assert _same(np.ascontiguousarray(Y[0, :n]), y1), (kind, b, layout)
            assert np.all(Y[1:, :n] == 0.0)
            # ... and over a list of tiles
            dY2 = t.full((b * ld,), -3.0, dtype=dX.dtype, device="cuda")
            if kind == "dp_sp":
                pkg.spmmv_ap_tiles(hand[0], hand[2], ids, dX, dY2, b, ld, layout)
            else:
                pkg.spmmv_ap_hp_tiles(hand[0], hand[1], hand[2], ids, dX, dY2, b, ld, layout)
            Y2 = dY2.cpu().numpy()
            Y2 = Y2.reshape(b, ld) if layout == pkg.COLWISE else Y2.reshape(ld, b).T
            for tile in (0, 1, 3):
                assert _same(np.ascontiguousarray(Y2[0, tile * 256:(tile + 1) * 256]), y1[tile * 256:(tile + 1) * 256]), (kind, b, layout, tile)
            assert np.all(Y2[:, 2 * 256:3 * 256] == -3.0)
