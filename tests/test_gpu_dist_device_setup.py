"""Distributed set-up from device-resident COO arrays: uspmv_halo_discover_device and uspmv_dmat_chunk_classes_device
(csrc/halo_kernels.hip) against the reference's own integers (tests/golden/halo.npz) and against the host route -- uspmv_halo_discover
[_ap | _ap_hp] + uspmv_permute_scs_cols, uspmv_scs_chunk_classes -- and the object of uspmv_dist_create_from_arrays_ex against the one
DistNative(...) builds from the same block on the host.  Everything is compared exactly: integers, bits of y."""
import functools
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, make_x, mtx_path

pytestmark = pytest.mark.gpu
NAMES = ("bcsstk13", "impcol_e", "stencil", "ragged3000")
KINDS = ("dp", "sp", "dp_sp", "dp_hp", "sp_hp", "dp_sp_hp")
STENCIL = (16, 16, 24)            # 6144 rows: with P = 3 and seg-rows three blocks of eight 256-row tiles, which loopback can run


def _pkg():
    import __graft_entry__ as ge
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def matrix(name):
    pkg = _pkg()
    if name == "stencil":
        return pkg.gen_stencil27(*STENCIL, magnitude_decades=4.0)
    if name == "ragged3000":
        # rows of very unequal length (1 .. 200 entries, a few empty), columns anywhere, magnitudes over six decades
        rng = np.random.default_rng(20261020)
        n = 3001
        ln = np.where(rng.random(n) < 0.1, rng.integers(60, 201, n), rng.integers(0, 9, n))
        I = np.repeat(np.arange(n), ln)
        V = rng.standard_normal(I.size) * 10.0 ** rng.uniform(-4, 2, I.size)
        return pkg.Coo.from_arrays(n, n, I, rng.integers(0, n, I.size), V)
    return pkg.read_mtx(mtx_path(name))


def part_dtypes(pkg, kind):
    return {"dp": [pkg.F64], "sp": [pkg.F32], "dp_sp": [pkg.F64, pkg.F32], "dp_hp": [pkg.F64, pkg.F16], "sp_hp": [pkg.F32, pkg.F16],
            "dp_sp_hp": [pkg.F64, pkg.F32, pkg.F16]}[kind]


def thresholds(m):
    """the 0.7 / 0.35 quantiles of |v|"""
    a = np.abs(np.asarray(m.arrays()[2]))
    return float(np.quantile(a, 0.7)), float(np.quantile(a, 0.35))


def dev_coo(t, m):
    I, J, V = m.arrays()
    return t.from_numpy(np.array(I)).cuda(), t.from_numpy(np.array(J)).cuda(), t.from_numpy(np.array(V)).cuda()


def host_route(pkg, loc, wsa, rank, P, C, sigma, kind, t1, t2):
    """the structs of the host route after halo discovery and column permutation, and their halo plan"""
    dts = part_dtypes(pkg, kind)
    if kind in ("dp", "sp"):
        coos = [loc]
    elif kind == "dp_sp":
        coos = list(pkg.partition_precisions(loc, t1))
    else:
        coos = [c for c in pkg.partition_precisions_hp(loc, kind, t1, t2) if c is not None]
    ss = [pkg.convert_to_scs(coos[0], C, sigma, dts[0])]
    o2n = ss[0].arrays()["old_to_new_idx"].copy()
    ss += [pkg.convert_to_scs(c, C, sigma, dt, fixed_permutation=o2n) for c, dt in zip(coos[1:], dts[1:])]
    if len(ss) == 1:
        halo = pkg.HaloPlan(ss[0], wsa, rank, P)
    elif kind == "dp_sp":
        halo = pkg.halo_discover_ap(ss[0], ss[1], wsa, rank, P)
    else:
        halo = pkg.halo_discover_ap_hp(ss[0], ss[1] if len(ss) == 3 else None, ss[-1], wsa, rank, P)
    for s in ss:
        pkg.permute_scs_cols(s, o2n)
    return ss, halo


def device_handles(pkg, t, loc, dev, C, sigma, kind, t1, t2):
    """the handles of the device route before halo discovery: GLOBAL column ids, the other parts in the first part's row order"""
    dts = part_dtypes(pkg, kind)
    n, nc = loc.n_rows, loc.n_cols
    if kind in ("dp", "sp"):
        coos = [dev]
    else:
        coos = [p for p in pkg.partition_precisions_device(*dev, n, nc, kind, t1, t2) if p is not None]
    _, A0, o2n, _ = pkg.convert_to_scs_device_from_arrays(*coos[0], n, nc, C, sigma, dts[0], permute_cols=False, want_layout=False)
    As = [A0] + [pkg.convert_to_scs_device_from_arrays(*c, n, nc, C, sigma, dt, fixed_permutation=o2n, permute_cols=False, want_layout=False)[1]
                 for c, dt in zip(coos[1:], dts[1:])]
    return As, o2n


def same_halo(a, b):
    return (a.n_halo == b.n_halo and np.array_equal(a.recv_counts, b.recv_counts) and np.array_equal(a.recv_idxs, b.recv_idxs)
            and np.array_equal(a.recv_counts_cumsum, b.recv_counts_cumsum))


@functools.lru_cache(maxsize=None)
def grid(name, kind):
    """Both routes on every rank of P in {1, 2, 3, 4}, C in {1, 4, 10, 32}, sigma in {1, 512} of one matrix and kind: (cases run, what
    differed in the halo / col_idxs, what differed in the chunk classes).  A block the host route refuses must be refused alike."""
    import torch as t
    pkg = _pkg()
    t.cuda.set_device(0)
    m = matrix(name)
    t1, t2 = thresholds(m)
    n_cases, bad_halo, bad_cls = 0, [], []
    for P in (1, 2, 3, 4):
        wsa = pkg.seg_work_sharing_arr(m, "seg-nnz", P)
        for rank in range(P):
            loc = pkg.seg_local_coo(m, wsa, rank)
            assert loc.nnz > 256                            # more than one workgroup (256 entries) claims and rewrites, also on impcol_e / 4
            dev = dev_coo(t, loc)
            nl = int(wsa[rank + 1] - wsa[rank])
            for C in (1, 4, 10, 32):
                for sigma in (1, 512):
                    tag = (P, rank, C, sigma)
                    try:
                        ss, want = host_route(pkg, loc, wsa, rank, P, C, sigma, kind, t1, t2)
                    except pkg.UspmvError as e:
                        assert "padded slot" in str(e), (tag, str(e))
                        with pytest.raises(pkg.UspmvError, match="padded slot"):
                            device_handles(pkg, t, loc, dev, C, sigma, kind, t1, t2)
                        continue
                    As, o2n = device_handles(pkg, t, loc, dev, C, sigma, kind, t1, t2)
                    got = pkg.halo_discover_device(As, loc.n_cols, wsa, rank, P, o2n)
                    n_cases += 1
                    if not same_halo(got, want) or (P == 1 and got.n_halo != 0):
                        bad_halo.append((tag, "plan"))
                    for q, (s, A) in enumerate(zip(ss, As)):
                        a = s.arrays()
                        if not np.array_equal(pkg.dmat_download(A)["col_idxs"], a["col_idxs"]):
                            bad_halo.append((tag, "col_idxs", q))
                        hc, hp = s.chunk_classes(nl)
                        dc, dp_ = A.chunk_classes_device(nl)
                        if not np.array_equal(hc, dc) or hp != dp_:
                            bad_cls.append((tag, q, hp, dp_))
    return n_cases, bad_halo, bad_cls


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_halo_discover_device_equals_the_host_route(pkg, name, kind):
    n_cases, bad_halo, _ = grid(name, kind)
    assert n_cases >= 40 and not bad_halo, (n_cases, bad_halo[:8])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_chunk_classes_device_equal_the_host_classes(pkg, name, kind):
    """... on the same handles and ranks, F16 parts included, pad_col included"""
    n_cases, _, bad_cls = grid(name, kind)
    assert n_cases >= 40 and not bad_cls, (n_cases, bad_cls[:8])


def test_halo_discover_device_against_the_reference(pkg):
    """bcsstk13, P = 4, seg-nnz, C = 32, sigma = 512: the reference's own col_idxs and receive lists.  Rank 3's only element from rank 0 is
    the padding column."""
    import torch as t
    t.cuda.set_device(0)
    h = np.load(os.path.join(GOLDEN, "halo.npz"))
    key = "bcsstk13_C32_s512_seg-nnz_P4"
    m = matrix("bcsstk13")
    wsa = pkg.seg_work_sharing_arr(m, "seg-nnz", 4)
    assert np.array_equal(wsa, h[key + "_wsa"])
    for rank in range(4):
        loc = pkg.seg_local_coo(m, wsa, rank)
        (A,), o2n = device_handles(pkg, t, loc, dev_coo(t, loc), 32, 512, "dp", 0.0, 0.0)
        plan = pkg.halo_discover_device(A, loc.n_cols, wsa, rank, 4, o2n)
        assert np.array_equal(o2n.cpu().numpy(), h[f"{key}_r{rank}_old_to_new"])
        assert np.array_equal(pkg.dmat_download(A)["col_idxs"], h[f"{key}_r{rank}_col_idxs"]), rank
        assert np.array_equal(plan.recv_counts_cumsum, h[f"{key}_r{rank}_recv_cumsum"]), rank
        assert np.array_equal(plan.recv_idxs, h[f"{key}_r{rank}_recv_idxs"]), rank
    assert plan.recv_counts[0] == 1 and plan.recv_idxs_of(0)[0] == 0


@pytest.mark.parametrize("kind,t1,t2", [("dp_sp", 0.0, 0.0), ("dp_hp", 0.0, 0.0), ("dp_sp_hp", 1e300, 0.0)])
def test_halo_discover_device_with_an_empty_part(pkg, kind, t1, t2):
    """a threshold that leaves a part without entries: its struct is all padding (dp_sp_hp: the hi part, so the scan starts on column 0)"""
    import torch as t
    t.cuda.set_device(0)
    m = matrix("impcol_e")
    wsa = pkg.seg_work_sharing_arr(m, "seg-nnz", 3)
    for rank in range(3):
        loc = pkg.seg_local_coo(m, wsa, rank)
        ss, want = host_route(pkg, loc, wsa, rank, 3, 4, 1, kind, t1, t2)
        assert min(s.nnz for s in ss) == 0
        As, o2n = device_handles(pkg, t, loc, dev_coo(t, loc), 4, 1, kind, t1, t2)
        got = pkg.halo_discover_device(As, loc.n_cols, wsa, rank, 3, o2n)
        assert same_halo(got, want)
        nl = int(wsa[rank + 1] - wsa[rank])
        for s, A in zip(ss, As):
            assert np.array_equal(pkg.dmat_download(A)["col_idxs"], s.arrays()["col_idxs"])
            hc, hp = s.chunk_classes(nl)
            dc, dp_ = A.chunk_classes_device(nl)
            assert np.array_equal(hc, dc) and hp == dp_


# ---------------------------------------------------------------------------------------------------------------- the object
def _stencil_block(pkg, rank, P=3):
    m = matrix("stencil")
    wsa = pkg.seg_work_sharing_arr(m, "seg-rows", P)
    assert np.array_equal(np.diff(wsa), np.full(P, m.n_rows // P))
    return m, wsa, pkg.seg_local_coo(m, wsa, rank)


def _kind_kw(kind, t1, t2, pkg):
    if kind in ("dp", "sp"):
        return dict(dtype=pkg.F64 if kind == "dp" else pkg.F32)
    if kind == "dp_sp":
        return dict(ap_threshold=t1)
    return dict(ap_kind=kind, ap_threshold=t1, ap_threshold_2=t2)


def _plan_of(pkg, d):
    class H:
        pass
    A = H()
    A.h, A.n_chunks = d._A, d.scs.n_chunks
    return pkg.DeviceMatrix.plan_download(A)


def _same_dict(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _meta(d):
    return (d.n_local, d.n_halo, d.padded_vec_size, d.n_send, d.n_interior, d.n_boundary, d.use_tiles, d.n_rows_padded, d.loopback)


def _block_step(pkg, d, kind, X, Y, b, layout):
    if kind in ("dp", "sp"):
        return d.spmmv(X, Y, b, layout)
    return d.spmmv_ap(X, Y, b, layout) if kind == "dp_sp" else d.spmmv_ap_hp(X, Y, b, layout)


@pytest.mark.parametrize("tlc", (False, True))
@pytest.mark.parametrize("kind", ("dp", "dp_sp", "dp_hp", "sp_hp", "dp_sp_hp"))
def test_object_from_arrays_equals_the_host_route_object(pkg, kind, tlc):
    """loopback, P = 3, every block, USPMV_SORT_HOST: meta data, pad lists, exchange plan and line plan equal; check() clean with the same
    checksum bits; one step and one block step (b = 4, both layouts) on the same random x give the same bits"""
    import torch as t
    t.cuda.set_device(0)
    P, C, sigma, b = 3, 32, 512, 4
    t1, t2 = thresholds(matrix("stencil"))
    kw = dict(comm_rank=0, comm_size=1, tlc=tlc, exchange="peer", **_kind_kw(kind, t1, t2, pkg))
    rng = np.random.default_rng(7)
    for rank in range(P):
        m, wsa, loc = _stencil_block(pkg, rank)
        host = pkg.DistNative(loc, wsa, C, sigma, rank, P, None, **kw)
        dev = pkg.DistNative.from_device_arrays(*dev_coo(t, loc), m.n_cols, wsa, C, sigma, rank, P, None, sort_mode=pkg.SORT_HOST, **kw)
        tag = (kind, tlc, rank)
        assert dev.loopback and dev.n_halo > 0 and dev.use_tiles == tlc
        assert _meta(dev) == _meta(host), tag
        assert dev.pad_info() == host.pad_info(), tag
        assert all(np.array_equal(x, y) for x, y in zip(dev.comm_plan(), host.comm_plan())), tag
        assert _same_dict(_plan_of(pkg, dev), _plan_of(pkg, host)), tag
        assert (_plan_of(pkg, dev) is not None) == tlc
        assert np.array_equal(dev.old_to_new, host.old_to_new) and np.array_equal(dev.new_to_old, host.new_to_old)
        res = []
        for d in (host, dev):
            x, y = d.new_x(np.zeros(d.n_local)), d.new_y()
            bad, cs = d.check(loc, x, y)
            assert bad == 0, (tag, bad)
            res.append(np.float64(cs).view(np.uint64))
        assert res[0] == res[1], tag
        xl = rng.standard_normal(dev.n_local)
        ys = []
        for d in (host, dev):
            x, y = d.new_x(xl), d.new_y()
            d.spmv(x, y); d.synchronize()
            ys.append(y.clone())
        assert t.equal(ys[0], ys[1]), tag
        Xl = rng.standard_normal((b, dev.n_local))
        for layout in (pkg.COLWISE, pkg.ROWWISE):
            Ys = []
            for d in (host, dev):
                if kind == "dp":
                    d.set_option("block_plan", b)
                X = d.new_X(Xl, b, layout)
                Y = t.zeros(b * d.padded_vec_size, dtype=d.tdtype, device="cuda")
                _block_step(pkg, d, kind, X, Y, b, layout); d.synchronize()
                Ys.append(Y.clone())
            assert t.equal(Ys[0], Ys[1]), (tag, layout)
        host.close(); dev.close()


def test_object_from_arrays_over_rccl_and_with_the_stable_device_sort(pkg):
    """the RCCL self send / recv of loopback on an object made from arrays; USPMV_SORT_DEVICE_STABLE: check() clean, y in original order equal"""
    import torch as t
    t.cuda.set_device(0)
    P, C, sigma, rank = 3, 32, 512, 1
    m, wsa, loc = _stencil_block(pkg, rank)
    t1, _ = thresholds(m)
    xl = np.random.default_rng(3).standard_normal(loc.n_rows)
    for kw in (dict(), dict(ap_threshold=t1)):
        ys = []
        for sort in (pkg.SORT_HOST, pkg.SORT_DEVICE_STABLE):
            d = pkg.DistNative.from_device_arrays(*dev_coo(t, loc), m.n_cols, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1,
                                                  sort_mode=sort, **kw)
            assert d.exchange == "rccl" and d.loopback
            x, y = d.new_x(np.zeros(d.n_local)), d.new_y()
            assert d.check(loc, x, y)[0] == 0, (kw, sort)
            x, y = d.new_x(xl), d.new_y()
            d.spmv(x, y); d.synchronize()
            ys.append(d.y_to_original_order(y)[:d.n_local])
            d.close()
        assert np.array_equal(ys[0], ys[1]), kw


def test_object_from_arrays_narrow_chunks_end_on_chunk_lists(pkg):
    """C < 32: the host route re-chunks and ends on chunk lists; the device route must end there too"""
    import torch as t
    t.cuda.set_device(0)
    P, rank = 3, 2
    m, wsa, loc = _stencil_block(pkg, rank)
    for C, sigma in ((4, 64), (16, 512)):
        kw = dict(comm_rank=0, comm_size=1, exchange="peer")
        host = pkg.DistNative(loc, wsa, C, sigma, rank, P, None, **kw)
        dev = pkg.DistNative.from_device_arrays(*dev_coo(t, loc), m.n_cols, wsa, C, sigma, rank, P, None, **kw)
        assert not host.use_tiles and _meta(dev) == _meta(host), (C, _meta(dev), _meta(host))
        assert all(np.array_equal(x, y) for x, y in zip(dev.comm_plan(), host.comm_plan()))
        x, y = dev.new_x(np.zeros(dev.n_local)), dev.new_y()
        assert dev.check(loc, x, y)[0] == 0
        host.close(); dev.close()


# ---------------------------------------------------------------------------------------------------------------- real ranks
def _rank_worker(rank, world, q, job):
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.setdefault("OMP_NUM_THREADS", "4"); os.environ.setdefault("OMP_WAIT_POLICY", "passive")
        import torch
        import __graft_entry__ as ge
        pkg = ge.load_package()
        torch.cuda.set_device(0)
        hc = pkg.HostComm(job, rank, world, timeout_s=120)
        tot = pkg.read_mtx(mtx_path("bcsstk13"))
        wsa = pkg.seg_work_sharing_arr(tot, "seg-nnz", world)
        loc = pkg.seg_local_coo(tot, wsa, rank)
        # (the median of |v|: at the 0.7 quantile block 2 has rows without a dp entry that the dp ordering parks behind n_rows -- the
        #  host route's "padded slot" refusal, on one rank alone)
        t1 = float(np.quantile(np.abs(np.asarray(tot.arrays()[2])), 0.5))
        ys = {}
        for tag, kw in (("dp", dict()), ("dp_sp", dict(ap_threshold=t1))):
            for route in ("host", "device"):
                if route == "host":
                    d = pkg.DistNative(loc, wsa, 32, 512, rank, world, hostcomm=hc, host_exchange=True, **kw)
                else:
                    d = pkg.DistNative.from_device_arrays(*dev_coo(torch, loc), tot.n_cols, wsa, 32, 512, rank, world, hostcomm=hc, host_exchange=True, **kw)
                assert not d.loopback and d.n_local == int(wsa[rank + 1] - wsa[rank])
                x, y = d.new_x(np.zeros(d.n_local)), d.new_y()
                bad, _ = d.check(loc, x, y)
                assert bad == 0, (tag, route, bad)
                ys[tag, route] = (y.clone(), d.comm_plan())
                d.barrier()
                d.close()
            assert torch.equal(ys[tag, "host"][0], ys[tag, "device"][0]), tag
            assert all(np.array_equal(a, b) for a, b in zip(ys[tag, "host"][1], ys[tag, "device"][1])), tag
        hc.close()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def test_real_ranks_on_unequal_blocks_built_from_arrays(pkg):
    """three rank processes share the GPU over the host-staged exchange, seg-nnz blocks of bcsstk13 (unequal heights, asymmetric lists):
    every rank builds dp and ap[dp_sp] from arrays; check() clean on every rank, y and the exchange plan as on the host route"""
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    job = f"dds{os.getpid()}_{time.monotonic_ns()}"
    procs = [ctx.Process(target=_rank_worker, args=(r, world, q, job)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=300))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, msg in sorted(res):
        assert msg == "ok", f"rank {rank}: {msg}"


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_columns_alone(pkg):
    import torch as t
    t.cuda.set_device(0)
    m = matrix("impcol_e")
    P, rank, C, sigma = 3, 1, 4, 8
    wsa = pkg.seg_work_sharing_arr(m, "seg-nnz", P)
    loc = pkg.seg_local_coo(m, wsa, rank)
    dev = dev_coo(t, loc)
    t1, _ = thresholds(m)
    (A, B), o2n = device_handles(pkg, t, loc, dev, C, sigma, "dp_sp", t1, 0.0)
    before = [pkg.dmat_download(X)["col_idxs"].copy() for X in (A, B)]
    INVALID = 1

    def refused(parts, match, n_cols=loc.n_cols, w=wsa, r=rank, p=P):
        with pytest.raises(pkg.UspmvError, match=match) as e:
            pkg.halo_discover_device(parts, n_cols, w, r, p, o2n)
        assert e.value.status == INVALID, e.value
        for X, c in zip((A, B), before):
            assert np.array_equal(pkg.dmat_download(X)["col_idxs"], c)

    # a wrapped handle
    s = pkg.convert_to_scs(loc, C, sigma)
    W = pkg.DeviceMatrix(s, "cuda:0")
    refused([W], "does not own its arrays")
    # a handle that already carries a plan
    _, Pl, _, _ = pkg.convert_to_scs_device_from_arrays(*dev, loc.n_rows, loc.n_cols, 32, 512, permute_cols=False, want_layout=False)
    Pl.optimize_device()
    assert Pl.plan_download() is not None
    refused([Pl], "already carries a plan")
    # parts with different n_chunks
    _, Other, _, _ = pkg.convert_to_scs_device_from_arrays(*dev, loc.n_rows, loc.n_cols, 2 * C, sigma, permute_cols=False, want_layout=False)
    refused([A, Other], "must share C, n_chunks and the row layout")
    refused([A, A], "parts are one struct")
    # rank >= P
    refused([A, B], "bad argument", r=P)
    # n_cols and wsa[P] both below the largest column present
    top = int(loc.arrays()[1].max())
    assert top > wsa[2]
    small = np.array([wsa[0], wsa[1], wsa[2]], np.int32)          # a partition that ends below the block's columns
    with pytest.raises(pkg.UspmvError, match=r"column \d+ outside the global matrix") as e:
        pkg.halo_discover_device([A, B], int(wsa[2]), small, 1, 2, o2n)
    assert e.value.status == INVALID
    # ... names the first such column in scan order (the dp part's storage, then the sp part's), as the host scan would
    scan = np.concatenate(before)
    assert f"column {scan[scan >= wsa[2]][0]} outside" in str(e.value), e.value
    for X, c in zip((A, B), before):
        assert np.array_equal(pkg.dmat_download(X)["col_idxs"], c)
    # ... after all of which the handles still take the call
    want = host_route(pkg, loc, wsa, rank, P, C, sigma, "dp_sp", t1, 0.0)[1]
    assert same_halo(pkg.halo_discover_device([A, B], loc.n_cols, wsa, rank, P, o2n), want)


def test_object_refusals(pkg):
    import torch as t
    t.cuda.set_device(0)
    m, wsa, loc = _stencil_block(pkg, 0)
    dev = dev_coo(t, loc)
    kw = dict(comm_rank=0, comm_size=1, exchange="peer")
    # a block without rows in wsa: the host route's text, before anything else happens
    empty = np.array([0, 2048, 2048, 6144], np.int32)
    texts = []
    for make in (lambda: pkg.DistNative(loc, empty, 32, 512, 0, 3, None, **kw),
                 lambda: pkg.DistNative.from_device_arrays(*dev, m.n_cols, empty, 32, 512, 0, 3, None, **kw)):
        with pytest.raises(pkg.UspmvError, match="block 1 of 3 owns no rows") as e:
            make()
        texts.append(str(e.value).split(": block", 1)[1])
    assert texts[0] == texts[1]
    with pytest.raises(pkg.UspmvError, match="bad rank / P"):
        pkg.DistNative.from_device_arrays(*dev, m.n_cols, wsa, 32, 512, 3, 3, None, **kw)
    # the fp16 kinds' refusal of a parked non-empty row (the matrix of tests/test_gpu_ap_device_setup.py, found with the host path): 17
    # rows at C = 8, sigma = 32, the last three only in the hp part -- hi's ordering sends them behind n_rows
    n, C, sigma = 17, 8, 32
    I = np.arange(n)
    tiny = pkg.Coo.from_arrays(n, n, I, np.zeros(n, np.int64), np.where(I < n - 3, 2.0, 0.25))
    w1 = np.array([0, n], np.int32)
    texts = []
    for make in (lambda: pkg.DistNative(tiny, w1, C, sigma, 0, 1, None, ap_kind="dp_hp", ap_threshold=1.0, **kw),
                 lambda: pkg.DistNative.from_device_arrays(*dev_coo(t, tiny), n, w1, C, sigma, 0, 1, None, ap_kind="dp_hp", ap_threshold=1.0, **kw)):
        with pytest.raises(pkg.UspmvError, match="fixed_permutation maps a non-empty row onto a padded slot") as e:
            make()
        texts.append(e.value.status)
    assert texts[0] == texts[1]
