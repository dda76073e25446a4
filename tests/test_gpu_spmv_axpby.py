"""uspmv_spmv_axpby on the device: y = alpha A x + beta z, <y,y> and <w,y>, bit for bit against a numpy restatement -- t from the
oracle's spmv_scs (the slot-ordered FMA chain uspmv_spmv stores), then rn(alpha t) and rn(rn(alpha t) + rn(beta z)) in the handle's
dtype.  A NaN equals any NaN in the same place.  Every case first asserts which plan and which path answered.

Rows a call does not own: every comparison is against a vector that holds FILL wherever uspmv_spmv itself leaves y alone (found by two
runs of uspmv_spmv over two fills), guard included.  The csr kernel (C = 1 as crs) has no canonical summation order, so its t is what
uspmv_spmv stores, as the entry point's contract words it; every other case also holds uspmv_spmv's y against the oracle."""
import contextlib
import math

import numpy as np
import pytest

from conftest import make_x, mtx_path
from test_gpu_elem_plan import scrambled_columns
from test_gpu_nonsquare import MATRICES

pytestmark = pytest.mark.gpu
FILL, GUARD = 9.0, 64


@pytest.fixture(scope="module")
def t():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


@contextlib.contextmanager
def tuned(pkg, **kw):
    old = {k: pkg.get_tuning(k) for k in kw}
    try:
        pkg.set_tuning(**kw)
        yield
    finally:
        pkg.set_tuning(**old)


def bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same(got, want):
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def check(got, want, tag):
    assert got.shape == want.shape, tag
    if not same(got, want):
        bad = np.flatnonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{tag}: {len(bad)} of {got.size} elements differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}")


def restate(tv, alpha, beta, z):
    """the contract in numpy: every operation below rounds once, in the dtype of tv"""
    ty = tv.dtype.type
    with np.errstate(all="ignore"):
        v = ty(alpha) * tv
        if ty(beta) != 0:
            v = v + ty(beta) * z
    return v


def mixed_sweep_matrix(pkg, n=3001):
    """banded, columns ascending inside a row -- except in every third 256-row tile, whose rows list their columns in DESCENDING order:
    those tiles visit the windows of x backwards, do not qualify for the sweep and stay with the rest chunks"""
    I, J = [], []
    for i in range(n):
        cols = sorted(c for c in (i - 300, i - 5, i, i + 7, i + 290) if 0 <= c < n)
        if (i // 256) % 3 == 1:
            cols = cols[::-1]
        I += [i] * len(cols); J += cols
    I, J = np.asarray(I, np.int32), np.asarray(J, np.int32)
    V = (1.0 + ((I.astype(np.int64) * 7 + J * 3) % 29) / 16.0) * np.where((I + J) % 5 == 0, -1.0, 1.0)
    return pkg.Coo.from_arrays(n, n, I, J, V)


def struct(pkg, coo, C, sigma, dt, permute=True):
    s = pkg.convert_to_scs(coo, C, sigma, pkg.F64 if dt == "f64" else pkg.F32)
    if permute and coo.n_rows == coo.n_cols:
        pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"])
    return s


# name -> (matrix, C, sigma, handle builder, what must have answered); the builders run under the default tuning unless they say otherwise
def _plain(pkg, s): return pkg.DeviceMatrix(s)
def _crs(pkg, s): return pkg.DeviceMatrix(s, crs=True)
def _planned(pkg, s):
    A = pkg.DeviceMatrix(s); A.optimize(s); return A
def _idx(bits_):
    def build(pkg, s):
        with tuned(pkg, tlc_idx12=2 if bits_ == 12 else 0):
            return _planned(pkg, s)
    return build
def _elem(pkg, s):
    with tuned(pkg, tlc_elem=2):
        return _planned(pkg, s)
def _dealt(pkg, s): return pkg.DeviceMatrix(s, tlc=True)
def _additive(pkg, s):
    with tuned(pkg, tlc_additive=2):
        return pkg.DeviceMatrix(s, tlc=True)
def _sweep(pkg, s):
    A = pkg.DeviceMatrix(s)
    with tuned(pkg, sweep_max_stage=1 << 20):
        nt, ns = A.optimize_sweep(s, 8, 256)
    assert 0 < ns < nt, (nt, ns)                       # some tiles sweep, the others are rest chunks
    return A


MATS = {
    "bcsstk13": lambda pkg: pkg.read_mtx(mtx_path("bcsstk13")),
    "block": MATRICES["block"][0], "halo": MATRICES["halo"][0],
    "stencil": lambda pkg: pkg.gen_stencil27(37, 11, 6),
    "scrambled": lambda pkg: scrambled_columns(pkg, 40, 3, 8000, rows_too=True),
    "mixed": mixed_sweep_matrix,
}
CASES = {
    "crs C=1":            ("bcsstk13", 1, 1, _crs, dict(kind=0)),
    "rechunked C=8":      ("block", 8, 64, _planned, dict(kind=1)),
    "no plan C=10":       ("halo", 10, 20, _plain, dict(kind=0)),
    "no plan C=32":       ("block", 32, 512, _plain, dict(kind=0)),
    "no plan C=64":       ("bcsstk13", 64, 128, _plain, dict(kind=0)),
    "lines 16-bit":       ("halo", 32, 512, _idx(16), dict(kind=1, gran=16, index_bits=16)),
    "lines 12-bit":       ("block", 32, 512, _idx(12), dict(kind=1, gran=16, index_bits=12)),
    "elements":           ("halo", 32, 512, _elem, dict(kind=1, gran=1, dealt=False)),
    "elements dealt":     ("scrambled", 32, 512, _dealt, dict(kind=1, gran=1, dealt=True)),
    "additive":           ("stencil", 32, 512, _additive, dict(kind=1, gran=16, additive=True)),
    "sweep + rest":       ("mixed", 32, 1, _sweep, dict(kind=2)),
}


@pytest.fixture(scope="module")
def mats(pkg):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = MATS[name](pkg)
        return cache[name]
    return get


class Setup:
    """one handle with its x, its t and the rows uspmv_spmv writes -- computed once, shared by everything a case checks"""

    def __init__(self, pkg, orc, t, mats, case, dt, path=1):
        mat, C, sigma, build, expect = CASES[case]
        self.pkg, self.t, self.tag = pkg, t, (case, dt)
        s = self.s = struct(pkg, mats(mat), C, sigma, dt)
        a = s.arrays()
        self.np_t = a["values"].dtype.type
        self.n, self.npad = s.n_rows, s.n_rows_padded
        x_rows = max(s.n_cols, self.npad)
        xp = make_x(x_rows); xp[self.n:] *= 0.5
        self.xp = xp.astype(self.np_t)
        self.A = A = build(pkg, s)
        # which plan answered
        assert A.plan_info()[0] == expect["kind"], (self.tag, A.plan_info())
        if "gran" in expect: assert A.plan_granularity() == expect["gran"], (self.tag, A.plan_granularity())
        if "index_bits" in expect: assert A.index_bits() == expect["index_bits"], (self.tag, A.index_bits())
        if "dealt" in expect: assert bool(A.plan_rows_dealt()) == expect["dealt"], self.tag
        if expect.get("additive"): assert A.additive_chunks()[1] > 0, (self.tag, A.additive_chunks())
        self.x = t.from_numpy(self.xp).cuda()
        assert pkg.spmv_axpby_path(A, self.x) == path, (self.tag, pkg.spmv_axpby_path(A, self.x))
        # uspmv_spmv over two fills: its t and the rows it owns
        ya, yb = (self._plain_spmv(f) for f in (FILL, 5.0))
        self.written = ~((ya == FILL) & (yb == 5.0))
        assert self.written[:self.n].all() and not self.written[self.npad:].any(), self.tag
        check(ya[self.written], yb[self.written], (self.tag, "uspmv_spmv twice"))
        self.tv = ya.copy()
        if not A_is_crs(build):
            want = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], self.xp[:max(s.n_cols, self.npad)])
            check(ya[:self.n], np.asarray(want)[:self.n], (self.tag, "uspmv_spmv against the oracle"))

    def _plain_spmv(self, fill):
        y = self.t.full((self.npad + GUARD,), fill, dtype=self.A.torch_dtype, device="cuda")
        self.pkg.spmv(self.A, self.x, y)
        self.t.cuda.synchronize()
        return y.cpu().numpy()

    def vec(self, seed, pad=None):
        """a vector in y's row order over the padded rows + guard: values of both signs over a few decades; pad: what the padding rows and the guard hold"""
        rng = np.random.default_rng(seed)
        v = (rng.standard_normal(self.npad + GUARD) * 10.0 ** rng.integers(-3, 3, self.npad + GUARD)).astype(self.np_t)
        if pad is not None:
            with np.errstate(over="ignore"):
                v[self.n:] = self.np_t(pad)
        return v

    def run(self, alpha, beta, z=None, w=None, dots=False, n_dot=None, in_place=False):
        """one call on a FILL-ed y (in place: y starts as z on the rows the call owns); returns y, dots"""
        t, pkg = self.t, self.pkg
        y0 = np.full(self.npad + GUARD, FILL, self.np_t)
        if in_place:
            y0[self.written] = z[self.written]
        y = t.from_numpy(y0).cuda()
        dz = y if in_place else (None if z is None else t.from_numpy(z).cuda())
        dw = None if w is None else t.from_numpy(w).cuda()
        d = t.full((2,), 7.0, dtype=t.float64, device="cuda") if dots else None
        pkg.spmv_axpby(self.A, self.x, y, alpha, beta, z=dz, w=dw, dots=d, n_dot_rows=n_dot)
        t.cuda.synchronize()
        return y.cpu().numpy(), (None if d is None else d.cpu().numpy())

    def want(self, alpha, beta, z):
        zz = np.zeros_like(self.tv) if z is None else z
        return np.where(self.written, restate(self.tv, alpha, beta, zz), self.np_t(FILL))


def A_is_crs(build):
    return build is _crs


def everything(S):
    """the checks every case runs"""
    tag = S.tag
    b, nan = S.vec(1), np.full(S.npad + GUARD, np.nan, S.np_t)
    # alpha = 1, beta = 0: uspmv_spmv's y, bit for bit, and nothing beyond it
    y, _ = S.run(1.0, 0.0)
    check(y, np.where(S.written, S.tv, S.np_t(FILL)), (tag, "(1, 0) against uspmv_spmv"))
    # the residual b - A x
    y, _ = S.run(-1.0, 1.0, z=b)
    check(y, S.want(-1.0, 1.0, b), (tag, "(-1, 1), z = b"))
    # in place
    y, _ = S.run(0.37, -2.5, z=b, in_place=True)
    check(y, S.want(0.37, -2.5, b), (tag, "(0.37, -2.5) in place"))
    # beta = 0: z is never read
    for z in (nan, None):
        y, _ = S.run(0.37, 0.0, z=z)
        check(y, S.want(0.37, 0.0, None), (tag, "beta = 0, z", "NaN" if z is not None else None))
    # dots over the caller's rows: the padding rows of z and w hold 1e300 (inf in float), a kernel that includes them cannot pass
    z, w = S.vec(2, pad=1e300), S.vec(3, pad=1e300)
    y, d = S.run(0.37, -2.5, z=z, w=w, dots=True, n_dot=S.n)
    want = S.want(0.37, -2.5, z)
    check(y, want, (tag, "with dots"))
    y2, d2 = S.run(0.37, -2.5, z=z, w=w, dots=True, n_dot=S.n)
    assert np.array_equal(bits(d), bits(d2)) and same(y, y2), (tag, "two calls", d, d2)
    yd, wd = want[:S.n].astype(np.float64), w[:S.n].astype(np.float64)
    for k, (p, q) in enumerate(((yd, yd), (wd, yd))):
        prod = p * q
        ref, mag = math.fsum(prod), math.fsum(np.abs(prod))
        bound = 2.0 * S.n * 2.0 ** -53 * mag               # any summation order plus one rounding per product
        print(f"{tag} dots[{k}] = {d[k]!r}, fsum = {ref!r}, |diff| = {abs(d[k] - ref):.3e}, bound = {bound:.3e}")
        assert abs(d[k] - ref) <= bound, (tag, k, d[k], ref, bound)
    # no w: dots[1] = 0, dots[0] as before
    _, d3 = S.run(0.37, -2.5, z=z, dots=True, n_dot=S.n)
    assert d3[1] == 0.0 and bits(d3)[0] == bits(d)[0], (tag, d3, d)
    # n_dot_rows = 0: both sums empty
    _, d4 = S.run(0.37, -2.5, z=z, w=w, dots=True, n_dot=0)
    assert d4[0] == 0.0 and d4[1] == 0.0, (tag, d4)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_in_every_default_kernel(pkg, orc, t, mats, case, dt):
    everything(Setup(pkg, orc, t, mats, case, dt, path=1))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_non_default_unroll_takes_path_2_and_still_matches(pkg, orc, t, mats, dt):
    with tuned(pkg, unroll=4):
        everything(Setup(pkg, orc, t, mats, "no plan C=32", dt, path=2))


def test_x_off_the_16_byte_grid_leaves_the_plan_and_stays_fused(pkg, orc, t, mats):
    """uspmv_spmv leaves the plan for such an x and launches scs_spmv_rows, which has a fused form: path 1 by the launcher's own
    conditions, another grid, the same y"""
    S = Setup(pkg, orc, t, mats, "lines 16-bit", "f64", path=1)
    xo = t.zeros(S.xp.size + 1, dtype=t.float64, device="cuda")[1:]
    xo.copy_(S.x)
    assert xo.data_ptr() % 16 == 8 and pkg.spmv_axpby_path(S.A, xo) == 1
    S.x = xo
    everything(S)
    with tuned(pkg, unroll=2):
        assert pkg.spmv_axpby_path(S.A, xo) == 2               # (the rows kernel fuses at the default unroll only)


def test_a_part_of_an_adaptive_precision_split_is_refused(pkg, t, mats):
    m = mats("bcsstk13")
    dp, sp = pkg.partition_precisions(m, 1.0)
    s_dp = pkg.convert_to_scs(dp, 32, 512, pkg.F64)
    perm = s_dp.arrays()["old_to_new_idx"]
    s_sp = pkg.convert_to_scs(sp, 32, 512, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(s_dp, perm); pkg.permute_scs_cols(s_sp, perm)
    A_dp, A_sp = pkg.DeviceMatrix(s_dp), pkg.DeviceMatrix(s_sp)
    pkg.optimize_ap(A_dp, A_sp, s_dp, s_sp)
    assert A_dp.plan_info()[0] != 0
    x = t.ones(s_dp.n_rows_padded, dtype=t.float64, device="cuda")
    y = t.full((s_dp.n_rows_padded,), FILL, dtype=t.float64, device="cuda")
    with pytest.raises(pkg.UspmvError, match="uspmv_spmv_axpby: .*adaptive-precision split") as e:
        pkg.spmv_axpby(A_dp, x, y)
    assert e.value.status == 3
    with pytest.raises(pkg.UspmvError, match="uspmv_spmv_axpby_path: .*adaptive-precision split"):
        pkg.spmv_axpby_path(A_dp, x)
    with pytest.raises(pkg.UspmvError, match="uspmv_spmv_axpby_reserve: .*adaptive-precision split"):
        A_dp.axpby_reserve()
    t.cuda.synchronize()
    assert bool((y == FILL).all())


def test_stream_capture_needs_the_reserve_and_replays_to_the_same_bits(pkg, orc, t, mats):
    S = Setup(pkg, orc, t, mats, "lines 16-bit", "f64", path=1)
    z, w = S.vec(2, pad=1e300), S.vec(3, pad=1e300)
    y_eager, d_eager = S.run(0.37, -2.5, z=z, w=w, dots=True, n_dot=S.n)
    A = _idx(16)(pkg, S.s)                                 # a fresh handle: no workspace yet
    dz, dw = t.from_numpy(z).cuda(), t.from_numpy(w).cuda()
    y = t.full((S.npad + GUARD,), FILL, dtype=t.float64, device="cuda")
    d = t.full((2,), 7.0, dtype=t.float64, device="cuda")
    scratch = t.zeros(8, device="cuda")
    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g):
        scratch.add_(1.0)
        with pytest.raises(pkg.UspmvError, match="uspmv_spmv_axpby_reserve") as e:
            pkg.spmv_axpby(A, S.x, y, 0.37, -2.5, z=dz, w=dw, dots=d, n_dot_rows=S.n)
        assert e.value.status == 1
    A.axpby_reserve()
    g2 = t.cuda.CUDAGraph()
    with t.cuda.graph(g2):
        pkg.spmv_axpby(A, S.x, y, 0.37, -2.5, z=dz, w=dw, dots=d, n_dot_rows=S.n)
    for _ in range(2):
        y.fill_(FILL); d.fill_(7.0)
        g2.replay()
        t.cuda.synchronize()
        check(y.cpu().numpy(), y_eager, "graph replay, y")
        assert np.array_equal(bits(d.cpu().numpy()), bits(d_eager)), (d.cpu().numpy(), d_eager)
