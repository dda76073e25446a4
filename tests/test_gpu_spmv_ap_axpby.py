"""uspmv_spmv_ap_axpby / uspmv_spmv_ap_hp_axpby on the device: y = alpha A x + beta z, <y,y> and <w,y> on the parts of an adaptive-precision
split, bit for bit against the numpy restatement of tests/test_gpu_spmv_axpby.py -- t is what the pre-existing uspmv_spmv_ap[_hp] stores
on the same handles (held against the oracle's composition first), then rn(alpha t) and rn(rn(alpha t) + rn(beta z)) in the type of
x and y: float64, float32 for ap[sp_hp].  Every case first asserts which plan is installed and which path answers, then runs the checks
of that file's everything(): (1, 0) against the plain call and nothing beyond its rows, the residual, an in-place call, beta = 0 with a
NaN and a NULL z, the dots with 1e300 in the padding rows of z and w, their reproducibility and their distance to math.fsum within
2 n 2^-53 sum|p q| (any summation order plus one rounding per product), no w, n_dot_rows = 0.

Shapes: 3 001 rows (3 008 padded: the last workgroup and the last tile have rowless lanes) or bcsstk13's 2 003."""
import numpy as np
import pytest

from conftest import mtx_path
from test_gpu_ap_elem_plan import Split, _quantiles, scrambled_columns
from test_gpu_nonsquare import MATRICES
from test_gpu_spmv_axpby import FILL, GUARD, Setup, bits, check, everything, mixed_sweep_matrix, restate, same, tuned

pytestmark = pytest.mark.gpu
KINDS = ("dp_sp", "dp_hp", "sp_hp", "dp_sp_hp")


@pytest.fixture(scope="module")
def t():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


def tail_mixed_matrix(pkg, n=3001):
    """mixed_sweep_matrix's band, the rows from 2 048 on listing their columns in DESCENDING order: tiles of 512 or 1 024 rows sweep in
    front of that row and stay with the rest chunks behind it"""
    I, J = [], []
    for i in range(n):
        cols = sorted(c for c in (i - 300, i - 5, i, i + 7, i + 290) if 0 <= c < n)
        if i >= 2048:
            cols = cols[::-1]
        I += [i] * len(cols); J += cols
    I, J = np.asarray(I, np.int32), np.asarray(J, np.int32)
    V = (1.0 + ((I.astype(np.int64) * 7 + J * 3) % 29) / 16.0) * np.where((I + J) % 5 == 0, -1.0, 1.0)
    return pkg.Coo.from_arrays(n, n, I, J, V)


MATS = {   # name: (builder, square -- columns permuted with the rows, x in the rows' order)
    "block": (MATRICES["block"][0], False), "halo": (MATRICES["halo"][0], False),
    "bcsstk13": (lambda pkg: pkg.read_mtx(mtx_path("bcsstk13")), True),
    "scrambled": (lambda pkg: scrambled_columns(pkg, 10, 3, 500), True),
    "mixed": (mixed_sweep_matrix, True), "tail": (tail_mixed_matrix, True),
}
_CACHE = {}


def split_of(pkg, orc, mat, kind, C, sigma, thresholds=None):
    """one split per (matrix, kind, C, sigma, thresholds), built once for the module: structs, x and the oracle's y are read only"""
    key = (mat, kind, C, sigma, thresholds)
    if key not in _CACHE:
        if mat not in _CACHE:
            _CACHE[mat] = MATS[mat][0](pkg)
        m = _CACHE[mat]
        t1, t2 = thresholds if thresholds is not None else _quantiles(m, kind)
        sp = Split(pkg, orc, m, kind, C, sigma, t1, t2, permute_cols=MATS[mat][1])
        if thresholds is None:
            assert all(n is None or n > 0 for n in sp.nnz), sp.nnz
        _CACHE[key] = sp
    return _CACHE[key]


# ---- the two families behind one set of calls
def plain(pkg, sp, hand, x, y, stream=None):
    return pkg.spmv_ap(hand[0], hand[2], x, y, stream=stream) if sp.kind == "dp_sp" else pkg.spmv_ap_hp(hand[0], hand[1], hand[2], x, y, stream=stream)


def fused(pkg, sp, hand, x, y, *a, **kw):
    return pkg.spmv_ap_axpby(hand[0], hand[2], x, y, *a, **kw) if sp.kind == "dp_sp" else pkg.spmv_ap_hp_axpby(hand[0], hand[1], hand[2], x, y, *a, **kw)


def path_of(pkg, sp, hand, x):
    return pkg.spmv_ap_axpby_path(hand[0], hand[2], x) if sp.kind == "dp_sp" else pkg.spmv_ap_hp_axpby_path(hand[0], hand[1], hand[2], x)


def reserve(pkg, sp, hand):
    return pkg.ap_axpby_reserve(hand[0], hand[2]) if sp.kind == "dp_sp" else pkg.ap_hp_axpby_reserve(hand[0], hand[1], hand[2])


def plan_lines(pkg, sp, hand, max_lines=0):
    s = sp.structs
    if sp.kind == "dp_sp":
        return pkg.optimize_ap(hand[0], hand[2], s[0], s[2], max_lines)
    return pkg.optimize_ap_hp(hand[0], hand[1], hand[2], s[0], s[1], s[2], max_lines)


def plan_sweep(pkg, sp, hand, wlog, tile_rows):
    s = sp.structs
    with tuned(pkg, sweep_max_stage=1 << 20):
        if sp.kind == "dp_sp":
            return pkg.optimize_sweep_ap(hand[0], hand[2], s[0], s[2], wlog, tile_rows)
        return pkg.optimize_sweep_ap_hp(hand[0], hand[1], hand[2], s[0], s[1], s[2], wlog, tile_rows)


def live(hand):
    return [h for h in hand if h is not None]


def assert_plan(hand, kind, gran=None):
    for h in live(hand):
        assert h.plan_info()[0] == kind, (kind, h.plan_info())
        if gran is not None:
            assert h.plan_granularity() == gran, (gran, h.plan_granularity())


class ApSetup(Setup):
    """Setup of tests/test_gpu_spmv_axpby.py on the handles of a split: x, the t of uspmv_spmv_ap[_hp] and the rows it writes, computed
    once (and held against the oracle's composition); vec() and want() are that class's."""

    def __init__(self, pkg, t, sp, hand, tag, path=1, x=None):
        self.pkg, self.t, self.tag, self.sp, self.hand = pkg, t, tag, sp, hand
        self.np_t = sp.x.dtype.type
        self.n, self.npad = sp.structs[0].n_rows, sp.n_pad
        self.x = t.from_numpy(sp.x).cuda() if x is None else x
        self.tdt = self.x.dtype
        assert path_of(pkg, sp, hand, self.x) == path, (tag, path_of(pkg, sp, hand, self.x))
        ya, yb = (self._plain_spmv(f) for f in (FILL, 5.0))
        self.written = ~((ya == FILL) & (yb == 5.0))
        assert self.written[:self.npad].all() and not self.written[self.npad:].any(), tag
        check(ya[self.written], yb[self.written], (tag, "the plain call twice"))
        self.tv = ya.copy()
        check(ya[:self.npad], sp.want, (tag, "the plain call against the oracle's composition"))

    def _plain_spmv(self, fill):
        y = self.t.full((self.npad + GUARD,), fill, dtype=self.tdt, device="cuda")
        plain(self.pkg, self.sp, self.hand, self.x, y)
        self.t.cuda.synchronize()
        return y.cpu().numpy()

    def run(self, alpha, beta, z=None, w=None, dots=False, n_dot=None, in_place=False):
        t = self.t
        y0 = np.full(self.npad + GUARD, FILL, self.np_t)
        if in_place:
            y0[self.written] = z[self.written]
        y = t.from_numpy(y0).cuda()
        dz = y if in_place else (None if z is None else t.from_numpy(z).cuda())
        dw = None if w is None else t.from_numpy(w).cuda()
        d = t.full((2,), 7.0, dtype=t.float64, device="cuda") if dots else None
        fused(self.pkg, self.sp, self.hand, self.x, y, alpha, beta, z=dz, w=dw, dots=d, n_dot_rows=n_dot)
        t.cuda.synchronize()
        return y.cpu().numpy(), (None if d is None else d.cpu().numpy())


# ---- every fused kernel of the default tuning ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mat,C,sigma", [("block", 32, 512), ("halo", 10, 20)])
def test_no_plan_lane_per_row(pkg, orc, t, kind, mat, C, sigma):
    """C = 32: the CT = 32 lane-per-row kernels on a non-square matrix, x in its own numbering; C = 10: run-time C, 3 010 padded rows on
    workgroups of 256 threads -- lanes past the last chunk"""
    sp = split_of(pkg, orc, mat, kind, C, sigma)
    hand = sp.handles(pkg)
    assert_plan(hand, 0, 0)
    everything(ApSetup(pkg, t, sp, hand, ("no plan", kind, C)))


@pytest.mark.parametrize("kind,C,sigma", [(k, 32, 512) for k in KINDS] + [("dp_sp", 16, 1), ("dp_hp", 16, 1)])
def test_shared_line_plan(pkg, orc, t, kind, C, sigma):
    """C = 32 and C = 16: the CT = 32 and CT = 0 tile kernels, every tile staged.  (C = 16 runs unsorted: at sigma = 64 the first part's
    ordering parks rows it has no entry in behind n_rows, and uspmv_convert_to_scs refuses the other parts under that permutation.)"""
    sp = split_of(pkg, orc, "halo", kind, C, sigma)
    hand = sp.handles(pkg)
    with tuned(pkg, tlc_elem=0, sweep=0):                  # (plan time only: the line plan whatever it stages)
        nt, ns = plan_lines(pkg, sp, hand)
    assert nt > 1 and ns == nt, (nt, ns)
    assert_plan(hand, 1, 16)
    everything(ApSetup(pkg, t, sp, hand, ("lines", kind, C)))


@pytest.mark.parametrize("kind", ["dp_sp", "dp_sp_hp"])
def test_line_plan_under_a_budget_at_the_median_tile(pkg, orc, t, kind):
    """tiles without a line list (nl == 0, the wide-footprint branch with global gathers) next to staged ones, one launch, one epilogue"""
    sp = split_of(pkg, orc, "bcsstk13", kind, 32, 512)
    hand = sp.handles(pkg)
    with tuned(pkg, tlc_elem=0, sweep=0):
        plan_lines(pkg, sp, hand)
        nl = np.diff(hand[0].plan_download()["tile_line_ptr"])
        budget = int(np.sort(nl[nl > 0])[int((nl > 0).sum()) // 2])       # the median staged tile still stages, the fuller ones do not
        assert 0 < budget < nl.max(), nl
        plan_lines(pkg, sp, hand, budget)
    assert_plan(hand, 1, 16)
    nl = np.diff(hand[0].plan_download()["tile_line_ptr"])
    assert (nl == 0).any() and (nl > 0).any(), nl
    everything(ApSetup(pkg, t, sp, hand, ("budget", kind)))


@pytest.mark.parametrize("kind", KINDS)
def test_shared_element_plan(pkg, orc, t, kind):
    sp = split_of(pkg, orc, "scrambled", kind, 32, 512)
    hand = sp.handles(pkg)
    nt, ns = sp.plan_host(pkg, hand, tlc_elem=2)
    assert nt > 1 and ns == nt, (nt, ns)
    assert_plan(hand, 1, 1)
    everything(ApSetup(pkg, t, sp, hand, ("elements", kind)))


def _sweep_case(pkg, orc, t, kind, mat="mixed", tile_rows=256, **launch_tuning):
    sp = split_of(pkg, orc, mat, kind, 32, 1)
    hand = sp.handles(pkg)
    nt, ns = plan_sweep(pkg, sp, hand, 8, tile_rows)
    assert nt == -(-sp.n_pad // tile_rows) and 0 < ns < nt, (nt, ns)       # some tiles sweep, the others are rest chunks: two launches, one slot range
    assert_plan(hand, 2)
    assert hand[0].plan_info() == (2, nt, ns)
    with tuned(pkg, **launch_tuning):
        everything(ApSetup(pkg, t, sp, hand, ("sweep + rest", kind, tile_rows, launch_tuning)))


@pytest.mark.parametrize("kind", KINDS)
def test_sweep_tiles_and_rest_chunks(pkg, orc, t, kind):
    _sweep_case(pkg, orc, t, kind)


def test_sweep_with_two_window_buffers(pkg, orc, t):
    _sweep_case(pkg, orc, t, "dp_sp_hp", sweep_nbuf=2)


@pytest.mark.parametrize("kind,tile_rows,rows_per_lane", [("dp_sp", 512, 2), ("dp_hp", 512, 2), ("dp_hp", 1024, 4), ("dp_sp_hp", 1024, 4)])
def test_sweep_with_several_rows_per_lane(pkg, orc, t, kind, tile_rows, rows_per_lane):
    """tiles of 512 / 1 024 rows on workgroups of 256 threads ("sweep_threads"): two / four rows per lane -- the plan info's tile count
    says which tile size was installed.  (Four rows per lane is what a matrix of 1.5 M rows gets by default.)"""
    assert tile_rows // 256 == rows_per_lane
    _sweep_case(pkg, orc, t, kind, mat="tail", tile_rows=tile_rows, sweep_threads=256)


@pytest.mark.parametrize("which", ["first_empty", "last_empty"])
def test_a_split_with_an_empty_part(pkg, orc, t, which):
    m = _CACHE.setdefault("bcsstk13", MATS["bcsstk13"][0](pkg))
    big = 10.0 * float(np.abs(np.asarray(m.arrays()[2])).max())
    sp = split_of(pkg, orc, "bcsstk13", "dp_sp", 32, 1, thresholds=(big, big) if which == "first_empty" else (0.0, 0.0))
    assert (sp.nnz[0] == 0) if which == "first_empty" else (sp.nnz[2] == 0), sp.nnz
    hand = sp.handles(pkg)
    with tuned(pkg, tlc_elem=0, sweep=0):
        nt, ns = plan_lines(pkg, sp, hand)
    assert ns > 0
    assert_plan(hand, 1, 16)
    everything(ApSetup(pkg, t, sp, hand, ("empty part", which)))


def test_x_off_the_16_byte_grid_leaves_the_plan_and_stays_fused(pkg, orc, t):
    sp = split_of(pkg, orc, "halo", "dp_sp", 32, 512)
    hand = sp.handles(pkg)
    with tuned(pkg, tlc_elem=0, sweep=0):
        plan_lines(pkg, sp, hand)
    assert_plan(hand, 1, 16)
    xo = t.zeros(sp.x.size + 1, dtype=t.float64, device="cuda")[1:]
    xo.copy_(t.from_numpy(sp.x))
    assert xo.data_ptr() % 16 == 8
    everything(ApSetup(pkg, t, sp, hand, ("x off the grid",), path=1, x=xo))
    with tuned(pkg, unroll=4):
        assert path_of(pkg, sp, hand, xo) == 2               # (the pair's lane-per-row kernel fuses at the default unroll only)


# ---- path 2 --------------------------------------------------------------------------------------------------------------------------------
def test_path_2_pair_under_unroll_4(pkg, orc, t):
    sp = split_of(pkg, orc, "block", "dp_sp", 32, 512)
    hand = sp.handles(pkg)
    with tuned(pkg, unroll=4):
        everything(ApSetup(pkg, t, sp, hand, ("path 2", "unroll=4"), path=2))
    hp = split_of(pkg, orc, "block", "dp_hp", 32, 512)
    hh = hp.handles(pkg)
    with tuned(pkg, unroll=4):
        assert path_of(pkg, hp, hh, t.from_numpy(hp.x).cuda()) == 1      # the kinds with an fp16 part do not consult "unroll"


@pytest.mark.parametrize("kind", ["dp_sp", "sp_hp"])
def test_path_2_without_the_non_temporal_stream(pkg, orc, t, kind):
    sp = split_of(pkg, orc, "halo", kind, 32, 512)
    hand = sp.handles(pkg)
    with tuned(pkg, tlc_elem=0, sweep=0):
        plan_lines(pkg, sp, hand)
    assert_plan(hand, 1, 16)
    with tuned(pkg, nontemporal=0):
        everything(ApSetup(pkg, t, sp, hand, ("path 2", "nontemporal=0", kind), path=2))


def test_path_2_on_a_sweep_plan(pkg, orc, t):
    for knob in (dict(sweep_unroll=4), dict(sweep_pair=1)):
        _sweep_case_path2(pkg, orc, t, "dp_hp", knob)


def _sweep_case_path2(pkg, orc, t, kind, knob):
    sp = split_of(pkg, orc, "mixed", kind, 32, 1)
    hand = sp.handles(pkg)
    nt, ns = plan_sweep(pkg, sp, hand, 8, 256)
    assert 0 < ns < nt
    with tuned(pkg, **knob):
        S = ApSetup(pkg, t, sp, hand, ("path 2", knob), path=2)
        b = S.vec(1)
        y, _ = S.run(0.37, -2.5, z=b, in_place=True)
        check(y, S.want(0.37, -2.5, b), (S.tag, "in place"))


# ---- a recurrence ----------------------------------------------------------------------------------------------------------------------------
def test_chebyshev_recurrence_in_place(pkg, orc, t):
    """ten steps of y <- 2a A x - y in place with both dots, x and y swapping: after every step y equals the numpy restatement of that
    step (t from the plain call on the step's x) bit for bit, and a second run reproduces every dot bit for bit"""
    sp = split_of(pkg, orc, "mixed", "dp_sp", 32, 512)
    hand = sp.handles(pkg)
    with tuned(pkg, tlc_elem=0, sweep=0):
        nt, ns = plan_lines(pkg, sp, hand)
    assert ns == nt
    assert_plan(hand, 1, 16)
    n, npad, a = sp.structs[0].n_rows, sp.n_pad, 0.05
    assert sp.x.size == npad
    x0 = sp.x.copy()
    y0 = np.where(np.arange(npad) < n, np.cos(np.arange(npad) * 0.37), 0.0)
    assert path_of(pkg, sp, hand, t.from_numpy(x0).cuda()) == 1

    def ten_steps(verify):
        x, y = t.from_numpy(x0).cuda(), t.from_numpy(y0).cuda()
        d = t.zeros(2, dtype=t.float64, device="cuda")
        tt = t.empty(npad, dtype=t.float64, device="cuda")
        out = []
        for step in range(10):
            if verify:
                plain(pkg, sp, hand, x, tt)
                want = restate(tt.cpu().numpy(), 2.0 * a, -1.0, y.cpu().numpy())
            fused(pkg, sp, hand, x, y, 2.0 * a, -1.0, z=y, w=x, dots=d, n_dot_rows=n)
            t.cuda.synchronize()
            if verify:
                check(y.cpu().numpy(), want, ("recurrence", step))
            out.append(d.cpu().numpy().copy())
            x, y = y, x
        return out

    first, second = ten_steps(True), ten_steps(False)
    for step, (p, q) in enumerate(zip(first, second)):
        assert np.array_equal(bits(p), bits(q)), (step, p, q)
        assert np.isfinite(p).all() and p[0] > 0.0, (step, p)


# ---- refusals, stream capture ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_y_alone(pkg, orc, t):
    sp = split_of(pkg, orc, "halo", "dp_sp", 32, 512)
    sp16 = split_of(pkg, orc, "halo", "dp_sp", 16, 1)
    hp = split_of(pkg, orc, "halo", "dp_hp", 32, 512)
    hand, hand16, hh = sp.handles(pkg), sp16.handles(pkg), hp.handles(pkg)
    x = t.from_numpy(sp.x).cuda()
    y = t.full((sp.n_pad + GUARD,), FILL, dtype=t.float64, device="cuda")
    z = t.ones(sp.n_pad + GUARD, dtype=t.float64, device="cuda")
    d = t.full((2,), 7.0, dtype=t.float64, device="cuda")
    pair, trio = "uspmv_spmv_ap_axpby: ", "uspmv_spmv_ap_hp_axpby: "
    with pytest.raises(pkg.UspmvError, match=pair + ".*share C and n_chunks"):
        pkg.spmv_ap_axpby(hand[0], hand16[2], x, y)
    with pytest.raises(pkg.UspmvError, match=pair + ".*expects a double and a float struct"):
        pkg.spmv_ap_axpby(hand[0], hand[0], x, y)                      # a one-precision handle in place of the sp part
    with pytest.raises(pkg.UspmvError, match=trio + ".*the parts must be"):
        pkg.spmv_ap_hp_axpby(hh[0], None, hand[2], x, y)
    with pytest.raises(pkg.UspmvError, match=trio + ".*share C and n_chunks"):
        pkg.spmv_ap_hp_axpby(hand16[0], None, hh[2], x, y)
    for call, who, hs in ((pkg.spmv_ap_axpby, pair, (hand[0], hand[2])), (pkg.spmv_ap_hp_axpby, trio, (hh[0], None, hh[2]))):
        with pytest.raises(pkg.UspmvError, match=who + ".*d_z") as e:
            call(*hs, x, y, 1.0, 1.0, z=None)
        assert e.value.status == 1
        for bad in (-1, sp.n_pad + 1):
            with pytest.raises(pkg.UspmvError, match=who + ".*n_dot_rows"):
                call(*hs, x, y, 1.0, 1.0, z=z, dots=d, n_dot_rows=bad)
        with pytest.raises(pkg.UspmvError, match=who + ".*overlaps"):
            call(*hs, x, y, 1.0, 1.0, z=y[1:])
    t.cuda.synchronize()
    assert bool((y == FILL).all()) and bool((d == 7.0).all())


@pytest.mark.parametrize("kind", ["dp_sp", "dp_sp_hp"])
def test_stream_capture_needs_the_reserve_and_replays_to_the_same_bits(pkg, orc, t, kind):
    sp = split_of(pkg, orc, "halo", kind, 32, 512)

    def planned():
        hand = sp.handles(pkg)
        with tuned(pkg, tlc_elem=0, sweep=0):
            plan_lines(pkg, sp, hand)
        assert_plan(hand, 1, 16)
        return hand
    S = ApSetup(pkg, t, sp, planned(), ("capture", kind))
    z, w = S.vec(2, pad=1e300), S.vec(3, pad=1e300)
    y_eager, d_eager = S.run(0.37, -2.5, z=z, w=w, dots=True, n_dot=S.n)
    hand = planned()                                       # fresh handles: no workspace yet
    dz, dw = t.from_numpy(z).cuda(), t.from_numpy(w).cuda()
    y = t.full((S.npad + GUARD,), FILL, dtype=t.float64, device="cuda")
    d = t.full((2,), 7.0, dtype=t.float64, device="cuda")
    scratch = t.zeros(8, device="cuda")
    name = "uspmv_spmv_ap_axpby_reserve" if kind == "dp_sp" else "uspmv_spmv_ap_hp_axpby_reserve"
    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g):
        scratch.add_(1.0)
        with pytest.raises(pkg.UspmvError, match=name) as e:
            fused(pkg, sp, hand, S.x, y, 0.37, -2.5, z=dz, w=dw, dots=d, n_dot_rows=S.n)
        assert e.value.status == 1
    reserve(pkg, sp, hand)
    g2 = t.cuda.CUDAGraph()
    with t.cuda.graph(g2):
        fused(pkg, sp, hand, S.x, y, 0.37, -2.5, z=dz, w=dw, dots=d, n_dot_rows=S.n)
    for _ in range(2):
        y.fill_(FILL); d.fill_(7.0)
        g2.replay()
        t.cuda.synchronize()
        check(y.cpu().numpy(), y_eager, "graph replay, y")
        assert np.array_equal(bits(d.cpu().numpy()), bits(d_eager)), (d.cpu().numpy(), d_eager)
    assert same(y.cpu().numpy(), y_eager)
