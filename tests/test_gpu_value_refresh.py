"""Numeric refresh on the device: new values on an unchanged pattern, plans kept (uspmv_dmat_values_changed, uspmv_dmat_update_values,
uspmv_dmat_update_values_from_arrays, uspmv_raw_plan_cache_values_changed; csrc/refresh_kernels.hip).

Every case goes V0 -> V1 -> V0 (new_values of tests/test_value_refresh_host.py: stripped tails appear and disappear, signed zeros are
kept), first asserts the path it is about -- which plan the handle carries, which kernel answered, which actions the refresh reported --
and then compares (i) y or Y with the oracle on the host struct of the new values, (ii) with a fresh handle built from the new values by
the same planner calls, (iii) the handle's arrays / plan digests with the fresh handle's.  Bit equality throughout: all values are
finite."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from conftest import make_x, mtx_path
from test_gpu_elem_plan import scrambled_columns
from test_gpu_spmmv_phased_arms import BASE, SHAPES
from test_value_refresh_host import bits, new_values

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def t(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


@contextlib.contextmanager
def tuning(pkg, **kw):
    old = {k: pkg.get_tuning(k) for k in kw}
    try:
        pkg.set_tuning(**kw)
        yield
    finally:
        pkg.set_tuning(**old)


class Mat:
    """A pattern with its two sets of values: the COO arrays on the host and in HBM, per (C, sigma, dtype) the host structs (columns
    permuted), x and the oracle's y, computed once and left unchanged."""

    def __init__(self, pkg, orc, t, coo):
        self.pkg, self.orc, self.t = pkg, orc, t
        self.n_rows, self.n_cols = coo.n_rows, coo.n_cols
        self.I, self.J, V0 = [np.array(a) for a in coo.arrays()]
        self.V = [V0, new_values(self.I, V0)]
        self.dI, self.dJ = t.from_numpy(self.I).cuda(), t.from_numpy(self.J).cuda()
        self.dV = [t.from_numpy(v).cuda() for v in self.V]
        self._s = {}

    def coo(self, k):
        return self.pkg.Coo.from_arrays(self.n_rows, self.n_cols, self.I, self.J, self.V[k])

    def struct(self, k, Cc, sigma, dtype):
        """(host struct of values k, its arrays, x, the oracle's y)"""
        key = (k, Cc, sigma, dtype)
        if key not in self._s:
            pkg = self.pkg
            s = pkg.convert_to_scs(self.coo(k), Cc, sigma, dtype)
            pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"].copy())
            a = s.arrays()
            xp = np.zeros(max(s.n_rows_padded, s.n_cols), s.np_dtype)
            xp[:s.n_rows] = pkg.apply_permutation(make_x(s.n_rows, s.np_dtype), a["new_to_old_idx"])
            y = self.orc.spmv_scs(Cc, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
            xp.setflags(write=False); y.setflags(write=False)
            self._s[key] = (s, a, xp, y)
        return self._s[key]


@pytest.fixture(scope="module")
def mats(pkg, orc, t):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "stencil27":
                coo = pkg.gen_stencil27(9, 11, 13)
            elif name == "banded":
                coo = pkg.gen_banded_random(60000, 60, 5000)
            elif name == "mesh3big":
                coo = pkg.gen_stencil27(14, 13, 12, dof=3)
            elif name == "dealt":
                coo = scrambled_columns(pkg, 40, 3, 8000, rows_too=True)
            elif name in SHAPES:
                gen, args, kw, _, _ = SHAPES[name]
                coo = getattr(pkg, gen)(*args, **kw)
            else:
                coo = pkg.read_mtx(mtx_path(name))
            cache[name] = Mat(pkg, orc, t, coo)
        return cache[name]
    return get


def spmv(pkg, t, A, xp):
    y = t.full((A.n_rows_padded,), -7.0, dtype=A.torch_dtype, device="cuda")
    pkg.spmv(A, t.from_numpy(xp).cuda(), y)
    t.cuda.synchronize()
    return y.cpu().numpy()


def same_arrays(pkg, A, F):
    a, f = pkg.dmat_download(A), pkg.dmat_download(F)
    return all(np.array_equal(bits(a[k]), bits(f[k])) for k in ("chunk_ptrs", "chunk_lengths", "col_idxs", "values"))


def same_plan(A, F):
    a, f = A.plan_download(), F.plan_download()
    if a is None or f is None:
        return a is None and f is None
    return all(np.array_equal(a[k], f[k]) for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16")) and a["max_lines_used"] == f["max_lines_used"]


# ------------------------------------------------------------------------------------------ no plan, line plan: nothing but the array
@pytest.mark.parametrize("dt", ["dp", "sp"])
@pytest.mark.parametrize("Cs", [(1, 1), (10, 20), (32, 512)])
@pytest.mark.parametrize("name", ["bcsstk13", "stencil27"])
def test_planless_and_line_plan(pkg, t, mats, name, Cs, dt):
    # The CRS kernel behind the crs flag sums a row over several lanes: it has no order to be bit-exact with and is held to a tolerance
    # elsewhere (tests/test_gpu_parity.py).  With one lane per row ("csr_lanes" 1) it walks the row as the oracle does, so the comparison
    # of this file -- bit equality -- applies to it as to every other kernel.
    with tuning(pkg, csr_lanes=1 if Cs[0] == 1 else pkg.get_tuning("csr_lanes")):
        _planless_and_line_plan(pkg, t, mats(name), Cs, dt)


def _planless_and_line_plan(pkg, t, M, Cs, dt):
    Cc, sigma = Cs
    dtype = pkg.F64 if dt == "dp" else pkg.F32
    crs = Cc == 1
    line = Cc == 32                                          # the line plan of uspmv_dmat_optimize[_device]; the other two stay without a plan
    s0, a0, xp, _ = M.struct(0, Cc, sigma, dtype)

    def path(A):
        kind = A.plan_info()[0]
        if line:
            assert kind == 1 and A.plan_granularity() == 16 and not A.plan_rows_dealt(), (kind, A.plan_granularity())
        else:
            assert kind == 0

    def fresh(k):
        s = M.struct(k, Cc, sigma, dtype)[0]
        F = pkg.DeviceMatrix(s, crs=crs)
        if line:
            F.optimize_device()
        return F

    # route 1: a handle that owns its arrays, from the device conversion; route 2: torch arrays wrapped; route 3: written in place
    _, A1, o2n, _ = pkg.convert_to_scs_device_from_arrays(M.dI, M.dJ, M.dV[0], M.n_rows, M.n_cols, Cc, sigma, dtype)
    if crs:
        assert pkg.lib().uspmv_dmat_set_crs(A1.h, 1) == 0
    A2, A3 = pkg.DeviceMatrix(s0, crs=crs), pkg.DeviceMatrix(s0, crs=crs)
    if line:
        A1.optimize_device(); A2.optimize_device(); A3.optimize(s0)
    assert np.array_equal(o2n.cpu().numpy(), a0["old_to_new_idx"])
    for k in (1, 0):
        s, a, _, want = M.struct(k, Cc, sigma, dtype)
        F = fresh(k)
        yF = spmv(pkg, t, F, xp)
        assert np.array_equal(bits(yF), bits(want))
        for route, A in ((1, A1), (2, A2), (3, A3)):
            path(A)
            if route == 3:
                A.values.copy_(t.from_numpy(a["values"]).cuda())
                acts = A.values_changed()
            else:
                acts = A.update_values_from_coo(M.dI, M.dJ, M.dV[k], row_pos=o2n, col_perm=o2n, check=True)
            assert acts == 0, (route, acts)
            path(A)
            y = spmv(pkg, t, A, xp)
            assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(y), bits(yF)), (route, k)
            assert same_arrays(pkg, A, F) and (route == 3 or same_plan(A, F)), (route, k)     # (route 3 was planned from the host struct)
    # a handle that owns its arrays also takes them in its own layout
    acts = A1.update_values(np.array(M.struct(1, Cc, sigma, dtype)[1]["values"]))
    assert acts == 0 and np.array_equal(bits(spmv(pkg, t, A1, xp)), bits(M.struct(1, Cc, sigma, dtype)[3]))


# ------------------------------------------------------------------------------------------ narrow chunks: the internal C = 32 copy
@pytest.mark.parametrize("dt", ["dp", "sp"])
@pytest.mark.parametrize("name,Cs", [("stencil27", (1, 1)), ("stencil27", (4, 512)), ("stencil27", (16, 512)), ("bcsstk13", (4, 512)), ("bcsstk13", (16, 512))])
def test_narrow_chunks_rechunked(pkg, t, mats, name, Cs, dt):
    M = mats(name)
    Cc, sigma = Cs
    dtype = pkg.F64 if dt == "dp" else pkg.F32
    crs = Cc == 1
    s0, a0, xp, _ = M.struct(0, Cc, sigma, dtype)
    o2n = t.from_numpy(np.array(a0["old_to_new_idx"])).cuda()

    def rechunked(A):
        """the SpMV kernels read a value array that is not the caller's: the internal re-chunking"""
        addr = (C.c_uint64 * 8)()
        assert pkg.lib().uspmv_dmat_plan_addresses(A.h, addr) == 0
        return int(addr[4]) != A.values.data_ptr()

    Ah, Ad = pkg.DeviceMatrix(s0, crs=crs, tlc=True), pkg.DeviceMatrix(s0, crs=crs)
    Ad.optimize_device()
    for k in (1, 0):
        s, a, _, want = M.struct(k, Cc, sigma, dtype)
        F = pkg.DeviceMatrix(s, crs=crs, tlc=True)
        assert rechunked(F)
        yF = spmv(pkg, t, F, xp)
        for how, A in (("host-planned", Ah), ("device-planned", Ad)):
            assert rechunked(A)
            if how == "host-planned":
                acts = A.update_values_from_coo(M.dI, M.dJ, M.dV[k], row_pos=o2n, col_perm=o2n)
            else:
                A.values.copy_(t.from_numpy(a["values"]).cuda())
                acts = A.values_changed()
            assert acts & pkg.REFRESH_RECHUNKED and not acts & (pkg.REFRESH_SWEEP_REBUILT | pkg.REFRESH_BLOCK_SWEEP_DROPPED), acts
            assert rechunked(A) and A.plan_info() == F.plan_info()
            y = spmv(pkg, t, A, xp)
            assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(y), bits(yF)), (how, k)
            assert same_arrays(pkg, A, F)


# ------------------------------------------------------------------------------------------ element plan on rows dealt to the tiles
def test_row_dealt_element_plan(pkg, t, mats):
    M = mats("dealt")
    s0, a0, xp, want0 = M.struct(0, 32, 512, pkg.F64)
    o2n = t.from_numpy(np.array(a0["old_to_new_idx"])).cuda()
    A = pkg.DeviceMatrix(s0, tlc=True)
    assert A.plan_rows_dealt() and A.plan_granularity() == 1
    y0 = spmv(pkg, t, A, xp)                                  # (A as planned: the fresh handle of V0)
    assert np.array_equal(bits(y0), bits(want0))
    plan0 = A.plan_download()
    s1, _, _, want1 = M.struct(1, 32, 512, pkg.F64)
    F = pkg.DeviceMatrix(s1, tlc=True)
    assert F.plan_rows_dealt()
    yF = spmv(pkg, t, F, xp)
    for k, want, fresh_y in ((1, want1, yF), (0, want0, y0)):
        acts = A.update_values_from_coo(M.dI, M.dJ, M.dV[k], row_pos=o2n, col_perm=o2n)
        assert acts & pkg.REFRESH_COPIES and not acts & ~pkg.REFRESH_COPIES, acts
        assert A.plan_rows_dealt() and A.plan_granularity() == 1
        y = spmv(pkg, t, A, xp)
        assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(y), bits(fresh_y)), k
    assert same_plan(A, F) and all(np.array_equal(plan0[q], A.plan_download()[q]) for q in ("tile_lines", "col16"))


# ------------------------------------------------------------------------------------------ block plans
class Block:
    def __init__(self, pkg, orc, t, M, Cc, sigma, dt):
        self.pkg, self.t, self.M, self.Cc, self.sigma = pkg, t, M, Cc, sigma
        self.dtype = pkg.F64 if dt == "dp" else pkg.F32
        self.b = 8 if dt == "dp" else 16
        s, a, xp, _ = M.struct(0, Cc, sigma, self.dtype)
        self.n, self.ld = s.n_rows_padded, max(s.n_rows_padded, s.n_cols)
        self.X, self.dX, self.want = {}, {}, {}
        for rowwise in (False, True):
            X = np.zeros(self.b * self.ld, xp.dtype)
            for v in range(self.b):
                col = xp * xp.dtype.type(1.0 + v / 8.0)
                if rowwise:
                    X[v::self.b] = col
                else:
                    X[v * self.ld:v * self.ld + xp.size] = col
            self.X[rowwise], self.dX[rowwise] = X, t.from_numpy(X).cuda()
            for k in (0, 1):
                sk, ak = M.struct(k, Cc, sigma, self.dtype)[:2]
                self.want[(k, rowwise)] = orc.spmmv_scs(Cc, sk.n_chunks, ak["chunk_ptrs"], ak["chunk_lengths"], ak["col_idxs"], ak["values"], X, self.b, self.ld,
                                                        rowwise)
        self.o2n = t.from_numpy(np.array(a["old_to_new_idx"])).cuda()

    def product(self, A, rowwise):
        t, pkg = self.t, self.pkg
        Y = t.full((self.b * self.ld,), -7.0, dtype=A.torch_dtype, device="cuda")
        pkg.spmmv(A, self.dX[rowwise], Y, self.b, self.ld, pkg.ROWWISE if rowwise else pkg.COLWISE)
        t.cuda.synchronize()
        return Y.cpu().numpy(), A.spmmv_last_path()[0]

    def same(self, got, k, rowwise):
        want, n, b, ld = self.want[(k, rowwise)], self.n, self.b, self.ld
        if rowwise:
            return np.array_equal(bits(got[:n * b]), bits(want[:n * b]))
        return all(np.array_equal(bits(got[v * ld:v * ld + n]), bits(want[v * ld:v * ld + n])) for v in range(b))

    def cycle(self, plan, kernel, info):
        """plan(A, s): the planner calls; kernel: what must answer before and after; info: what block_plan_info must say"""
        M, pkg = self.M, self.pkg
        A = pkg.DeviceMatrix(M.struct(0, self.Cc, self.sigma, self.dtype)[0])
        plan(A, M.struct(0, self.Cc, self.sigma, self.dtype)[0])
        for k in (1, 0):
            s = M.struct(k, self.Cc, self.sigma, self.dtype)[0]
            F = pkg.DeviceMatrix(s)
            plan(F, s)
            for key, val in info.items():
                assert A.block_plan_info()[key] == val and F.block_plan_info()[key] == val, (key, A.block_plan_info())
            for rowwise in (False, True):
                assert self.product(A, rowwise)[1] == kernel
            acts = A.update_values_from_coo(M.dI, M.dJ, M.dV[k], row_pos=self.o2n, col_perm=self.o2n)
            assert acts == pkg.REFRESH_COPIES, acts
            for key, val in info.items():
                assert A.block_plan_info()[key] == val
            for rowwise in (False, True):
                Y, ran = self.product(A, rowwise)
                YF, ranF = self.product(F, rowwise)
                assert ran == kernel and ranF == kernel, (ran, ranF)
                assert self.same(Y, k, rowwise) and np.array_equal(bits(Y), bits(YF)), (k, rowwise)
            assert A.block_plan_digest() == F.block_plan_digest() and same_arrays(pkg, A, F), k
        return A


@pytest.fixture(scope="module")
def blocks(pkg, orc, t, mats):
    cache = {}

    def get(name, dt):
        if (name, dt) not in cache:
            cache[(name, dt)] = Block(pkg, orc, t, mats(name), SHAPES[name][3], SHAPES[name][4], dt)
        return cache[(name, dt)]
    return get


@pytest.mark.parametrize("builder", ["optimize_block", "optimize_block_device"])
@pytest.mark.parametrize("dt", ["dp", "sp"])
@pytest.mark.parametrize("name", ["mesh3", "mesh2", "band40", "band11"])
def test_block_plans(pkg, blocks, name, dt, builder):
    K = blocks(name, dt)
    plan = (lambda A, s: A.optimize_block(s, K.b)) if builder == "optimize_block" else (lambda A, s: A.optimize_block_device(K.b))
    with tuning(pkg, **BASE):
        K.cycle(plan, kernel=8, info=dict(phased_plan=1))


def test_block_plan_reordered_copy_and_stream_schedule(pkg, blocks):
    K = blocks("mesh3", "dp")
    with tuning(pkg, **dict(BASE, spmmv_variant=5, spmmv_list_plan=1)):            # scs_spmmv_rowmajor on bt.values under the plan's row map
        K.cycle(lambda A, s: A.optimize_block(s, K.b), kernel=5, info=dict(list_plan=1, phased_plan=1))
    with tuning(pkg, **dict(BASE, spmmv_stream=1)):                                # the phased plan streamed by persistent workgroups
        A = K.cycle(lambda A, s: A.optimize_block(s, K.b), kernel=10, info=dict(phased_plan=1))
        assert A.block_plan_info()["stream_grid"] > 0


def test_no_leak_over_fifty_refreshes(pkg, t, blocks):
    K = blocks("mesh3", "dp")
    M = K.M
    with tuning(pkg, **BASE):
        A = pkg.DeviceMatrix(M.struct(0, K.Cc, K.sigma, K.dtype)[0])
        A.optimize_block(M.struct(0, K.Cc, K.sigma, K.dtype)[0], K.b)
        assert A.block_plan_info()["phased_plan"] == 1
        A.update_values_from_coo(M.dI, M.dJ, M.dV[1], row_pos=K.o2n, col_perm=K.o2n)
        t.cuda.synchronize()
        alloc0, (free0, _) = t.cuda.memory_allocated(), t.cuda.mem_get_info()
        for r in range(50):
            acts = A.update_values_from_coo(M.dI, M.dJ, M.dV[r % 2], row_pos=K.o2n, col_perm=K.o2n) if r % 3 else A.values_changed()
            assert acts == pkg.REFRESH_COPIES
        t.cuda.synchronize()
        alloc1, (free1, _) = t.cuda.memory_allocated(), t.cuda.mem_get_info()
        assert alloc1 == alloc0 and free1 == free0, (alloc1 - alloc0, free0 - free1)
        Y, ran = K.product(A, True)
        assert ran == 8 and K.same(Y, 1, True)                                     # (r = 49: the values of V1)


# ------------------------------------------------------------------------------------------ column-window sweep: rebuilt
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("wr", [(11, 1024), (13, 2048)])
@pytest.mark.parametrize("dt", ["dp", "sp"])
def test_sweep_plan_rebuilt(pkg, t, mats, dt, wr, builder):
    M = mats("banded")
    dtype = pkg.F64 if dt == "dp" else pkg.F32
    wlog, rows = wr
    s0, a0, xp, _ = M.struct(0, 32, 512, dtype)
    o2n = t.from_numpy(np.array(a0["old_to_new_idx"])).cuda()
    A = pkg.DeviceMatrix(s0)
    nt, nsw = A.optimize_sweep(s0, wlog, rows) if builder == "host" else A.optimize_sweep_device(None, wlog, rows)
    assert nsw == nt and A.plan_info()[0] == 2
    lengths = {}
    for k in (1, 0):
        s, a, _, want = M.struct(k, 32, 512, dtype)
        F = pkg.DeviceMatrix(s)
        assert F.optimize_sweep(s, wlog, rows) == (nt, nt) and F.plan_info()[0] == 2
        dF, mF = F.sweep_plan_digest()
        assert A.plan_info()[0] == 2
        if k == 1:
            acts = A.update_values_from_coo(M.dI, M.dJ, M.dV[k], row_pos=o2n, col_perm=o2n)
        else:
            A.values.copy_(t.from_numpy(a["values"]).cuda())
            acts = A.values_changed()
        assert acts == pkg.REFRESH_SWEEP_REBUILT, acts
        assert A.plan_info() == F.plan_info() and A.plan_info()[0] == 2
        dA, mA = A.sweep_plan_digest()
        assert mA == mF and dA == dF, (k, mA, mF)
        assert mA[1] == rows and mA[2] == wlog
        lengths[k] = mA[6]
        y, yF = spmv(pkg, t, A, xp), spmv(pkg, t, F, xp)
        assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(y), bits(yF)), k
    assert lengths[1] < lengths[0], lengths                    # V1 zeroes the last entry of every fifth row: those tails are stripped


# ------------------------------------------------------------------------------------------ block-vector sweep: released
def test_block_sweep_plan_dropped(pkg, orc, t, mats):
    M = mats("mesh3big")
    with tuning(pkg, **BASE):
        K = Block(pkg, orc, t, M, 32, 512, "dp")
        s0 = M.struct(0, 32, 512, pkg.F64)[0]
        A = pkg.DeviceMatrix(s0)
        nt, nsw = A.optimize_block_sweep(s0, 8, 9, 1024)
        assert nt == nsw and nt > 0
        for k in (1, 0):
            s = M.struct(k, 32, 512, pkg.F64)[0]
            F = pkg.DeviceMatrix(s)
            assert F.optimize_block_sweep(s, 8, 9, 1024) == (nt, nt)
            if k == 1:
                assert K.product(A, True)[1] == 9                                  # installed before
            acts = A.update_values_from_coo(M.dI, M.dJ, M.dV[k], row_pos=K.o2n, col_perm=K.o2n)
            assert acts == (pkg.REFRESH_BLOCK_SWEEP_DROPPED if k == 1 else 0), acts
            for rowwise in (False, True):
                Y, ran = K.product(A, rowwise)
                YF, ranF = K.product(F, rowwise)
                assert ran not in (0, 9) and ranF == 9, (ran, ranF)
                assert K.same(Y, k, rowwise) and np.array_equal(bits(Y), bits(YF)), (k, rowwise)
            assert same_arrays(pkg, A, F)


# ------------------------------------------------------------------------------------------ refusals: nothing written
def test_refusals_leave_the_handle_alone(pkg, t, mats):
    M = mats("stencil27")
    L = pkg.lib()
    s0, a0, xp, want0 = M.struct(0, 32, 512, pkg.F64)
    o2n = t.from_numpy(np.array(a0["old_to_new_idx"])).cuda()
    _, A1, o2n1, _ = pkg.convert_to_scs_device_from_arrays(M.dI, M.dJ, M.dV[0], M.n_rows, M.n_cols, 32, 512, pkg.F64)
    A2 = pkg.DeviceMatrix(s0, tlc=True)
    I, J, V1 = M.I, M.J, M.V[1]
    r = int(np.argmax(np.bincount(I, minlength=M.n_rows)))
    k = int(np.searchsorted(I, r, side="right"))
    pair = int(np.flatnonzero((I[1:] == I[:-1]) & (J[1:] != J[:-1]))[0])
    Js = J.copy(); Js[[pair, pair + 1]] = Js[[pair + 1, pair]]
    dev = lambda a: t.from_numpy(np.ascontiguousarray(a)).cuda()
    cases = [("column", (M.dI, dev(Js), M.dV[1]), f"entry {pair}: its column differs"),
             ("long", (dev(np.insert(I, k, r)), dev(np.insert(J, k, J[k - 1])), dev(np.insert(V1, k, 1.0))), "more entries than the chunk")]
    for A in (A1, A2):
        for what, (dI, dJ, dV), text in cases:
            with pytest.raises(pkg.UspmvError) as e:
                A.update_values_from_coo(dI, dJ, dV, row_pos=o2n, col_perm=o2n, check=True)
            assert e.value.status == INVALID and text in str(e.value), (what, str(e.value))
        acts = C.c_int(0)
        dst = A.values.data_ptr() if A is A2 else None
        rc = L.uspmv_dmat_update_values_from_arrays(A.h, M.dI.data_ptr(), M.dJ.data_ptr(), M.dV[1].data_ptr(), M.n_rows + 32, M.I.size, o2n.data_ptr(), o2n.data_ptr(), 1,
                                                    dst, None, C.byref(acts))
        assert rc == INVALID and "chunks" in L.uspmv_last_error().decode()
        assert np.array_equal(bits(pkg.dmat_download(A)["values"]), bits(np.array(a0["values"])))
        assert np.array_equal(bits(spmv(pkg, t, A, xp)), bits(want0))
    # an fp16 handle, and a pair that shares one plan: new values move entries between the parts
    sh = pkg.convert_to_scs(M.coo(0), 32, 512, pkg.F16)
    Ah = pkg.DeviceMatrix(sh)
    with pytest.raises(pkg.UspmvError) as e:
        Ah.values_changed()
    assert e.value.status == UNSUPPORTED and "fp16 handle" in str(e.value)
    big = pkg.gen_stencil27(16, 16, 16, magnitude_decades=6.0)
    dp, sp = pkg.partition_precisions(big, 1e-2)
    assert dp.nnz > 0 and sp.nnz > 0
    ds = pkg.convert_to_scs(dp, 32, 512, pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, 32, 512, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
    Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
    nt, nst = pkg.optimize_ap(Ad, As, ds, ss)
    assert nst > 0 and Ad.plan_info()[0] == 1
    for H in (Ad, As):
        with pytest.raises(pkg.UspmvError) as e:
            H.values_changed()
        assert e.value.status == UNSUPPORTED and "shared plan of an adaptive-precision split" in str(e.value)


# ------------------------------------------------------------------------------------------ raw arrays behind "raw_plan_cache"
def test_raw_plan_cache_values_changed(pkg, t, mats):
    M = mats("banded")
    s0, a0, xp, want0 = M.struct(0, 32, 512, pkg.F64)
    a1, want1 = M.struct(1, 32, 512, pkg.F64)[1], M.struct(1, 32, 512, pkg.F64)[3]
    cp, cl, ci = (t.from_numpy(np.array(a0[k])).cuda() for k in ("chunk_ptrs", "chunk_lengths", "col_idxs"))
    va = t.from_numpy(np.array(a0["values"])).cuda()
    x = t.from_numpy(xp).cuda()
    old = pkg.get_tuning("raw_plan_cache")
    try:
        pkg.lib().uspmv_raw_plan_cache_clear()
        pkg.set_tuning(raw_plan_cache=1)

        def product():
            y = t.full((s0.n_rows_padded,), -7.0, dtype=t.float64, device="cuda")
            pkg.uspmv_scs_gpu(32, s0.n_chunks, cp, cl, ci, va, x, y)
            t.cuda.synchronize()
            return y.cpu().numpy()

        assert pkg.raw_plan_cache_values_changed(va) == 0       # nothing planned yet
        assert np.array_equal(bits(product()), bits(want0))     # the first call plans: the column-window sweep, a private stream of the values
        for k, a, want in ((1, a1, want1), (0, a0, want0)):
            va.copy_(t.from_numpy(np.array(a["values"])).cuda())
            t.cuda.synchronize()
            assert not np.array_equal(bits(product()), bits(want))      # the path: the cached plan answers from its own copy of the values
            assert pkg.raw_plan_cache_values_changed(va) == 1
            assert np.array_equal(bits(product()), bits(want)), k
        assert pkg.raw_plan_cache_values_changed(x) == 0        # no plan behind this pointer
    finally:
        pkg.set_tuning(raw_plan_cache=old)
        pkg.lib().uspmv_raw_plan_cache_clear()
