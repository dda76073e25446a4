"""The adaptive-precision kinds with an fp16 part (ap[dp_hp], ap[sp_hp], ap[dp_sp_hp]) across ranks: the tile- and chunk-list forms of
their single-vector kernels (uspmv_spmv_ap_hp_tiles / _chunks) and the distributed step on such an object
(uspmv_dist_create_ap_hp_from_coo) -- loopback on one GPU (RCCL self send / recv, peer stores) and real ranks sharing the GPU over the
host-staged exchange.  Every comparison is bitwise (a NaN equals any NaN, _same of test_gpu_ap_hp.py), against the oracle composed part by
part on the WHOLE matrix (set up the host way) with x tiled by the block height."""
import ctypes
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, make_x, mtx_path
from test_dist_ap_hp_host import DEC, T1, T2, whole_matrix_ap_hp_reference
from test_gpu_ap_hp import KINDS, _build, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _check_lists(t, launch, n_ids, full, x, n_rows_padded):
    """odd / even ids with -1 entries interleaved, each into a NaN-filled y: disjoint rows, together the full launch; only -1: untouched"""
    ys = []
    for par in (0, 1):
        real = np.arange(par, n_ids, 2, dtype=np.int32)
        ids = np.full(2 * len(real), -1, np.int32)
        ids[1::2] = real                                   # -1, id, -1, id, ...
        ids = ids[len(ids) - min(len(ids), n_ids):]        # (a list is at most n_ids long: an odd count drops the leading -1)
        assert (ids < 0).any() and np.array_equal(ids[ids >= 0], real)
        y = t.full((n_rows_padded,), float("nan"), dtype=full.dtype, device="cuda")
        launch(t.from_numpy(ids).cuda(), x, y)
        ys.append(y)
    t.cuda.synchronize()
    w0, w1 = ~t.isnan(ys[0]), ~t.isnan(ys[1])
    assert not (w0 & w1).any() and bool((w0 | w1).all())
    assert t.equal(t.where(w0, ys[0], ys[1]), full)
    y = t.full((n_rows_padded,), float("nan"), dtype=full.dtype, device="cuda")
    launch(t.full((min(5, n_ids),), -1, dtype=t.int32, device="cuda"), x, y)
    t.cuda.synchronize()
    assert bool(t.isnan(y).all())


@pytest.mark.parametrize("C,sigma,narrow", [(32, 512, False), (16, 64, False), (32, 512, True)])
@pytest.mark.parametrize("kind", KINDS)
def test_spmv_ap_hp_tiles_and_chunks_give_the_rows_of_the_full_launch(pkg, torch_cuda, kind, C, sigma, narrow):
    """C 32: the CT = 32 instantiation, C 16: CT = 0; narrow: a line budget that leaves some tiles without a line list (nl == 0, the
    wide-footprint branch) next to staged ones."""
    t = torch_cuda
    coo = pkg.gen_stencil27(40, 40, 5, magnitude_decades=DEC)
    structs, _ = _build(pkg, coo, kind, C, sigma, T1, T2)
    assert all(s.nnz > 0 for s in structs if s is not None) and (structs[1] is None) == (kind != "dp_sp_hp")
    A = [pkg.DeviceMatrix(s) if s is not None else None for s in structs]
    sh = structs[0]
    npad, dt = sh.n_rows_padded, t.float32 if kind == "sp_hp" else t.float64
    x = t.zeros(npad, dtype=dt, device="cuda")
    x[:sh.n_rows] = t.from_numpy(make_x(sh.n_rows)).cuda().to(dt)
    full = t.full((npad,), float("nan"), dtype=dt, device="cuda")
    pkg.spmv_ap_hp(*A, x, full)                           # planless: lane per row
    t.cuda.synchronize()
    assert not bool(t.isnan(full).any())
    ids = t.arange(4, dtype=t.int32, device="cuda")
    with pytest.raises(pkg.UspmvError, match="no shared tile-local-column plan"):
        pkg.spmv_ap_hp_tiles(*A, ids, x, t.zeros_like(full))
    _check_lists(t, lambda i, xx, yy: pkg.spmv_ap_hp_chunks(*A, i, xx, yy), sh.n_chunks, full, x, npad)
    pkg.set_tuning(sweep=0)                               # (keep the line plan whatever it stages: this test is about its kernel)
    try:
        n_tiles, n_staged = pkg.optimize_ap_hp(*A, *structs)
        nl = np.diff(A[0].plan_download()["tile_line_ptr"])
        assert n_tiles >= 4 and n_staged == n_tiles and (nl > 0).all()
        if narrow:
            budget = int(np.sort(nl)[len(nl) // 2])       # the median tile still stages, the fuller ones do not
            assert budget < nl.max()
            n_tiles, n_staged = pkg.optimize_ap_hp(*A, *structs, budget)
            nl = np.diff(A[0].plan_download()["tile_line_ptr"])
            assert (nl == 0).any() and (nl > 0).any() and 0 < n_staged < n_tiles
    finally:
        pkg.set_tuning(sweep=1)
    assert A[0].plan_info()[0] == 1
    y = t.full((npad,), float("nan"), dtype=dt, device="cuda")
    pkg.spmv_ap_hp(*A, x, y)                              # the full launch of the plan's kernel: same bits as lane per row
    t.cuda.synchronize()
    assert t.equal(y, full)
    _check_lists(t, lambda i, xx, yy: pkg.spmv_ap_hp_tiles(*A, i, xx, yy), n_tiles, full, x, npad)
    _check_lists(t, lambda i, xx, yy: pkg.spmv_ap_hp_chunks(*A, i, xx, yy), sh.n_chunks, full, x, npad)
    with pytest.raises(pkg.UspmvError, match="16-byte aligned"):
        pkg.spmv_ap_hp_tiles(*A, ids, x[1:], y)
    with pytest.raises(pkg.UspmvError, match="bad argument"):
        pkg.spmv_ap_hp_tiles(*A, t.zeros(n_tiles + 1, dtype=t.int32, device="cuda"), x, y)
    for f in (pkg.spmv_ap_hp_tiles, pkg.spmv_ap_hp_chunks):
        with pytest.raises(pkg.UspmvError, match="the parts must be"):
            f(A[2], None, A[0], ids, x, y)
    assert pkg.spmv_ap_hp_tiles(*A, ids[:0], x, y) is y and pkg.spmv_ap_hp_chunks(*A, ids[:0], x, y) is y      # n_ids == 0: nothing to launch


_REFS = {}


def _reference(pkg, orc, kind, shape, P, C, sigma, xblock=None):
    """the oracle's whole-matrix product of the kind for x_global = P copies of xblock (default: the ramp over one block), original order"""
    key = (kind, shape, P, C, sigma, None if xblock is None else xblock.tobytes())
    if key not in _REFS:
        coo = pkg.gen_stencil27(*shape, magnitude_decades=DEC)
        nl = coo.n_rows // P
        assert nl * P == coo.n_rows
        xb = make_x(nl) if xblock is None else xblock
        y, nnz = whole_matrix_ap_hp_reference(pkg, orc, coo, kind, C, sigma, T1, T2, np.tile(xb, P))
        _REFS[key] = (y, nl)
    return _REFS[key]


def _block(pkg, shape, P, rank):
    wsa = pkg.seg_from_row_counts(pkg.gen_stencil27_row_counts(*shape), "seg-rows", P)
    return wsa, pkg.gen_stencil27(*shape, magnitude_decades=DEC, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))


@pytest.mark.parametrize("P,shape,C,sigma,tlc", [(2, (24, 24, 24), 32, 512, True), (4, (16, 16, 40), 32, 512, True), (3, (20, 9, 27), 16, 64, True),
                                                 (2, (24, 24, 24), 32, 512, False)])
@pytest.mark.parametrize("kind", KINDS)
def test_native_step_loopback_bitexact(pkg, orc, torch_cuda, kind, P, shape, C, sigma, tlc):
    torch = torch_cuda
    y_ref, nl = _reference(pkg, orc, kind, shape, P, C, sigma)
    first = (P, shape, tlc) == (2, (24, 24, 24), True)
    tdt = torch.float32 if kind == "sp_hp" else torch.float64
    for rank in range(P):
        wsa, loc = _block(pkg, shape, P, rank)
        want = y_ref[wsa[rank]:wsa[rank + 1]]
        for exchange in ("rccl", "peer") if first else ("rccl",):
            d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id() if exchange == "rccl" else None, comm_rank=0, comm_size=1,
                               tlc=tlc, ap_kind=kind, ap_threshold=T1, ap_threshold_2=T2, exchange=exchange)
            assert d.loopback and d.n_local == nl and d.n_halo > 0 and d.n_send == d.n_halo
            assert d.scs.nnz > 0 and d.scs_hp.nnz > 0 and d.scs_sp is None and (d.scs_mid is None) == (kind != "dp_sp_hp")
            assert d.scs_mid is None or d.scs_mid.nnz > 0
            assert d.use_tiles == tlc, d.plan_info()
            assert d.new_y().dtype == tdt and want.dtype == (np.float32 if kind == "sp_hp" else np.float64)
            info = d.pad_info()
            got = {}

            def step(tag, fn):
                x = d.new_x(make_x(nl))
                y = torch.full_like(d.new_y(), float("nan"))
                fn(x, y); d.synchronize()
                assert _same(d.y_to_original_order(y)[:nl], want), (kind, P, rank, exchange, tag)
                got[tag] = (y[:d.n_rows_padded].clone(), x[d.n_local:d.n_local + d.n_halo].clone())
                assert torch.equal(got[tag][0], got["eager"][0]) and torch.equal(got[tag][1], got["eager"][1]), tag

            step("eager", lambda x, y: d.spmv(x, y))                          # overlap, "pad_split" 1: the object's default
            d.set_option("pad_split", 0); step("pad_split 0", lambda x, y: d.spmv(x, y)); d.set_option("pad_split", 1)
            d.set_option("overlap", 0); step("plain", lambda x, y: d.spmv(x, y)); d.set_option("overlap", 1)
            step("run eager", lambda x, y: d.run(x, y, 3, use_graph=False))
            d._refresh()
            assert not d.graph_captured
            if exchange == "rccl":
                step("run graph", lambda x, y: d.run(x, y, 4, use_graph=True))
                d._refresh()
                assert d.graph_captured and d.graph_launches == 4, (d.graph_captured, d.graph_launches)
                d.set_option("ba_synch", 1)
                step("ba_synch", lambda x, y: d.run(x, y, 2, use_graph=True))
                d.set_option("ba_synch", 0)
            else:
                d.set_option("ba_synch", 1); step("ba_synch", lambda x, y: d.spmv(x, y)); d.set_option("ba_synch", 0)
            x = d.new_x(make_x(nl)); y = d.new_y()
            d.spmv(x, y, comm_halos=False); d.synchronize()
            assert not torch.equal(y[:d.n_rows_padded], got["eager"][0])
            assert d.check(loc, d.new_x(np.zeros(nl)), d.new_y())[0] == 0
            if exchange == "rccl":
                assert d.check(loc, d.new_x(np.zeros(nl)), d.new_y(), use_graph=True)[0] == 0
            d.set_option("diag_skip_exchange", 1)
            assert d.check(loc, d.new_x(np.zeros(nl)), d.new_y())[0] > 0
            d.set_option("diag_skip_exchange", 0)
            if first and rank > 0:
                # most tiles touch the halo ONLY through the padding of some part: with "pad_split" they run before the exchange completes
                n_tiles = d.n_interior + d.n_boundary
                assert d.use_tiles and info["pad_tiles"] > 0 and info["pad_col"] >= d.n_local
                assert 2 * (d.n_interior + info["pad_tiles"]) > n_tiles, (d.n_interior, info, n_tiles)
                assert d.n_interior == n_tiles - info["pad_tiles"] - info["real_boundary_tiles"]
                print(f"tile census {kind} P={P} rank={rank}: interior {d.n_interior} padding-only {info['pad_tiles']} real boundary {info['real_boundary_tiles']}")
            if not tlc:
                assert not d.use_tiles and d.n_interior + d.n_boundary == d.scs.n_chunks and info["pad_tiles"] == 0
            form, ms = d.autotune(d.new_x(make_x(nl)), d.new_y()) if first and rank == 1 and exchange == "rccl" else ("overlap", {})
            assert form in ("overlap", "plain") and set(ms) <= {"overlap", "plain"}
            if ms:
                step("after autotune", lambda x, y: d.spmv(x, y))
            d.close()


@pytest.mark.parametrize("kind", ["dp_sp_hp", "sp_hp"])
def test_padding_tiles_run_with_the_interior_and_rerun_when_they_must(pkg, orc, torch_cuda, kind):
    """The padding of ALL parts is (+0, global column 0), a halo column on ranks > 0; dp_sp_hp runs the double guard, sp_hp the float one.
    Positive x[0]: no re-run; negative: one re-run, none on the next step; +Inf: NaN in the padded rows, as in the oracle's whole-matrix
    product, and a re-run every step.  Eager steps and graph replay; with "pad_split" 0 nothing is ever re-run."""
    P, shape, C, sigma, rank = 4, (16, 16, 40), 32, 512, 2
    wsa, loc = _block(pkg, shape, P, rank)
    nl = int(wsa[1] - wsa[0])
    cases, want = {}, {}
    for tag, x0 in (("pos", 3.25), ("neg", -2.5), ("inf", np.inf)):
        xb = make_x(nl).copy(); xb[0] = x0
        cases[tag] = xb
        want[tag] = _reference(pkg, orc, kind, shape, P, C, sigma, xb)[0][wsa[rank]:wsa[rank + 1]]
    # (with three parts nearly every row is padded in one of them, so +Inf in the padding column may leave no row of the block finite)
    assert np.isnan(want["inf"]).any() and not np.isnan(want["neg"]).any() and not np.isnan(want["pos"]).any()
    d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_kind=kind, ap_threshold=T1, ap_threshold_2=T2)
    info = d.pad_info()
    assert info["pad_tiles"] > 0 and info["pad_col"] >= d.n_local and info["real_boundary_tiles"] > 0, info
    assert info["pad_tiles"] + info["real_boundary_tiles"] == d.n_boundary

    def run(tag, graph=False, steps=1):
        x = d.new_x(cases[tag]); y = d.new_y()
        if graph: d.run(x, y, steps, use_graph=True)
        else:
            for _ in range(steps): d.spmv(x, y)
        d.synchronize()
        assert _same(d.y_to_original_order(y)[:nl], want[tag]), (kind, tag, graph, steps)
        return d.pad_info()["reruns"]

    r0 = d.pad_info()["reruns"]
    assert run("pos") == r0                               # a fresh x: the slot held +0, same sign
    r1 = run("neg")                                       # fresh x again: +0 -> -2.5
    assert r1 == r0 + 1
    assert run("neg", steps=2) == r1 + 1                  # the second step on the SAME x finds -2.5 in the slot already
    r2 = d.pad_info()["reruns"]
    assert run("inf", steps=2) == r2 + 2                  # not finite: every step
    r3 = run("neg", graph=True, steps=3)                  # one eager step before the capture (the re-run), then three replays without
    d._refresh()
    assert r3 == r2 + 2 + 1 and d.graph_captured
    r4 = run("inf", graph=True, steps=2)                  # the captured step carries guard and conditional list
    assert r4 - r3 in (2, 3)                              # every replay; + the eager step of a new capture when x / y got new addresses
    d.set_option("pad_split", 0)
    assert run("neg") == r4 and run("inf") == r4 and run("pos") == r4
    d.close()


@pytest.mark.parametrize("kind", KINDS)
def test_what_an_ap_hp_object_does_not_have_is_refused_with_a_reason(pkg, torch_cuda, kind):
    torch = torch_cuda
    from ultimate_spmv_amd import binding as B
    P, shape, C, sigma, rank = 2, (24, 24, 24), 32, 512, 1
    wsa, loc = _block(pkg, shape, P, rank)
    nl = int(wsa[1] - wsa[0])
    mk = dict(comm_rank=0, comm_size=1)
    d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), ap_kind=kind, ap_threshold=T1, ap_threshold_2=T2, **mk)
    pair = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), ap_threshold=1e-3, **mk)
    one = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), **mk)
    name = rf"ap\[{kind}\]"
    for key, value in (("fused_step", 1), ("block_plan", 8), ("autotune_all", 1)):
        with pytest.raises(pkg.UspmvError, match=name) as e:
            d.set_option(key, value)
        assert e.value.status == 3                                         # USPMV_ERR_UNSUPPORTED
        one.set_option(key, value)
        one.set_option(key, 0)
    d.set_option("fused_step", 0); d.set_option("block_plan", 0)           # switching off what is off is fine
    b, ld = 2, d.padded_vec_size
    X = torch.zeros(b * ld, dtype=d.tdtype, device="cuda")
    for call in (d.spmmv, d.spmmv_ap):
        with pytest.raises(pkg.UspmvError, match=name) as e:
            call(X, torch.zeros_like(X), b)
        assert e.value.status == 3
    with pytest.raises(pkg.UspmvError) as e:                               # its parts are lent by uspmv_dist_parts_ap_hp only
        B._ck(B.lib().uspmv_dist_parts_ap(d.h, None, None, None, None, None))
    assert e.value.status == 1                                             # USPMV_ERR_INVALID
    with pytest.raises(pkg.UspmvError):
        B._ck(B.lib().uspmv_dist_parts_ap_hp(pair.h, None, None, None, None, None, None, None, None))
    with pytest.raises(ValueError):
        pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), dtype=pkg.F64 if kind == "sp_hp" else pkg.F32, ap_kind=kind,
                       ap_threshold=T1, ap_threshold_2=T2, **mk)
    h = ctypes.c_void_p()
    idbuf = (ctypes.c_ubyte * 128).from_buffer_copy(pkg.comm_unique_id())
    with pytest.raises(pkg.UspmvError, match="uspmv_dist_create_ap_from_coo"):
        B._ck(B.lib().uspmv_dist_create_ap_hp_from_coo(idbuf, 0, 1, rank, P, loc.h, B._np_ptr(np.ascontiguousarray(wsa, np.int32)), C, sigma,
                                                       pkg.AP_DP_SP, T1, T2, 1, ctypes.byref(h)))
    assert not h.value
    # the objects next to it: their own bits, their own options
    Xo = one.new_X([make_x(nl), make_x(nl) * 1.125], b)
    one.spmmv(Xo, torch.zeros(b * one.padded_vec_size, dtype=torch.float64, device="cuda"), b); one.synchronize()
    assert one.check(loc, one.new_x(np.zeros(nl)), one.new_y())[0] == 0 and one.scs_sp is None and one.scs_hp is None
    assert pair.check(loc, pair.new_x(np.zeros(nl)), pair.new_y())[0] == 0 and pair.scs_sp is not None and pair.scs_hp is None
    assert d.check(loc, d.new_x(np.zeros(nl)), d.new_y())[0] == 0
    d.close(); pair.close(); one.close()


def test_a_block_the_host_route_refuses_fails_the_create_call_with_its_text(pkg, torch_cuda):
    """T1 = 50 leaves a quarter of the rows without an entry in the hi part; the hi permutation then parks some of them on the padded slots of
    the last chunk (1620 rows per block, C 16), which the conversion of the hp part refuses.  The same block at T1 = 2.4 works afterwards."""
    P, shape, C, sigma, rank = 3, (20, 9, 27), 16, 64, 2
    wsa, loc = _block(pkg, shape, P, rank)
    nl = int(wsa[rank + 1] - wsa[rank])
    assert nl % C != 0 and len(set(np.diff(wsa))) == 1
    for kind in KINDS:
        with pytest.raises(pkg.UspmvError, match="fixed_permutation maps a non-empty row onto a padded slot"):
            pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_kind=kind, ap_threshold=50.0, ap_threshold_2=T2)
        d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_kind=kind, ap_threshold=T1, ap_threshold_2=T2)
        assert d.check(loc, d.new_x(np.zeros(nl)), d.new_y())[0] == 0
        d.close()


def _ap_hp_worker(rank, world, q, job, case):
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.setdefault("OMP_NUM_THREADS", "4"); os.environ.setdefault("OMP_WAIT_POLICY", "passive")   # (several rank processes share the box's cores)
        import torch
        import __graft_entry__ as ge
        pkg = ge.load_package()
        from ultimate_spmv_amd import binding as B
        from oracle import oracle as orc
        torch.cuda.set_device(0)
        name, Cc, sg, method, t1, t2, kinds = case
        tot = pkg.read_mtx(mtx_path(name))
        wsa = pkg.seg_work_sharing_arr(tot, method, world)
        xg = make_x(tot.n_rows)
        loc = B.seg_local_coo(tot, wsa, rank)
        nl = int(wsa[rank + 1] - wsa[rank])
        for kind in kinds:
            hc = pkg.HostComm(job + kind, rank, world, timeout_s=120)
            y_ref, _ = whole_matrix_ap_hp_reference(pkg, orc, tot, kind, Cc, sg, t1, t2, xg)
            d = pkg.DistNative(loc, wsa, Cc, sg, rank, world, hostcomm=hc, host_exchange=True, ap_kind=kind, ap_threshold=t1, ap_threshold_2=t2)
            assert d.n_local == nl and not d.loopback and d.scs.nnz > 0 and d.scs_hp.nnz > 0 and (kind != "dp_sp_hp" or d.scs_mid.nnz > 0)
            want = y_ref[wsa[rank]:wsa[rank + 1]]
            for overlap in (1, 0):
                d.set_option("overlap", overlap)
                for pad in (1, 0):
                    d.set_option("pad_split", pad)
                    x = d.new_x(xg[wsa[rank]:wsa[rank + 1]]); y = d.new_y()
                    d.run(x, y, 2, use_graph=True); d.synchronize()      # (host-staged exchange: runs eagerly)
                    assert _same(d.y_to_original_order(y)[:nl], want), (kind, overlap, pad)
            d.set_option("overlap", 1); d.set_option("pad_split", 1)
            bad, _ = d.check(loc, d.new_x(np.zeros(nl)), d.new_y())
            assert bad == 0, (kind, bad)
            d.barrier()
            d.close(); hc.close()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def test_ap_hp_step_real_ranks_unequal_seg_nnz_blocks(pkg):
    """bcsstk13 cut by entries into three unequal blocks with asymmetric lists: three real processes share the GPU over the host-staged
    exchange; y of every rank is the oracle's whole-matrix product of its rows, for ap[dp_sp_hp] (double vectors) and ap[sp_hp] (float)."""
    world, case = 3, ("bcsstk13", 32, 512, "seg-nnz", 1.0, 0.01, ("dp_sp_hp", "sp_hp"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    job = f"aphp{os.getpid()}_{time.monotonic_ns()}"
    procs = [ctx.Process(target=_ap_hp_worker, args=(r, world, q, job, case)) for r in range(world)]
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
