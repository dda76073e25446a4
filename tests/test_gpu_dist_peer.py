"""The peer-store halo exchange (USPMV_EXCHANGE_PEER, csrc/uspmv_dist_api.hip): every rank owns a receive window exported through
hipIpcGetMemHandle, one push kernel stores its halo contributions straight into its neighbours' windows, the ranks meet in the
transport's barrier, an unpack kernel copies the window into the tail of x.  On one GPU: loopback (the process pushes into its own
window, no IPC, no transport) against the oracle, and real rank processes sharing the card (IPC windows on the same device) against
the reference's goldens, the host-staged exchange and the CLI's self-check.  Worker processes set HSA_ENABLE_IPC_MODE_LEGACY=0 before
the HIP runtime starts: IPC handles between processes need it on ROCm."""
import json
import multiprocessing as mp
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, make_x, mtx_path

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "ultimate-spmv_amd", "uspmv")
IPC_ENV = {"HSA_ENABLE_IPC_MODE_LEGACY": "0"}


# ---------------------------------------------------------------------------------------------------------------- loopback
def _global_reference(pkg, orc, shape, P, C, sigma):
    """y of the whole matrix for x_global = P copies of the ramp over one block (seg-rows, equal blocks), original order."""
    coo = pkg.gen_stencil27(*shape)
    n = coo.n_rows
    nl = n // P
    s = pkg.convert_to_scs(coo, C, sigma)
    a = s.arrays()
    pkg.permute_scs_cols(s, a["old_to_new_idx"])
    a = s.arrays()
    xp = np.zeros(s.n_rows_padded)
    xp[:n] = pkg.apply_permutation(np.tile(make_x(nl), P), a["new_to_old_idx"])
    y = orc.spmv_scs(C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
    return pkg.apply_permutation(y, a["old_to_new_idx"]), nl


@pytest.mark.parametrize("P,shape,C,sigma", [(2, (24, 24, 24), 32, 512), (4, (16, 16, 40), 32, 512), (3, (20, 9, 27), 16, 64)])
def test_peer_loopback_bitexact(pkg, orc, P, shape, C, sigma):
    """Loopback peer stores (no transport, no RCCL communicator): y against the oracle and the halo tail of x against the RCCL
    loopback's, for every arrangement of the step; a graph request runs eagerly."""
    import torch
    torch.cuda.set_device(0)
    y_ref, nl = _global_reference(pkg, orc, shape, P, C, sigma)
    counts = pkg.gen_stencil27_row_counts(*shape)
    wsa = pkg.seg_from_row_counts(counts, "seg-rows", P)
    assert np.array_equal(np.diff(wsa), np.full(P, nl))
    for rank in range(P):
        loc = pkg.gen_stencil27(*shape, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))
        want = y_ref[wsa[rank]:wsa[rank + 1]]
        r = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1)
        xr, yr = r.new_x(make_x(nl)), r.new_y()
        r.spmv(xr, yr); r.synchronize()
        tail = xr[nl:nl + r.n_halo].clone()
        r.close()
        d = pkg.DistNative(loc, wsa, C, sigma, rank, P, comm_rank=0, comm_size=1, exchange="peer")
        assert d.exchange == "peer" and d.loopback and d.comm_count() == 0
        assert d.n_local == nl and d.n_halo > 0 and d.n_send == d.n_halo
        for overlap, pad, fused in ((1, 0, 0), (0, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)):
            d.set_option("overlap", overlap); d.set_option("pad_split", pad); d.set_option("fused_step", fused)
            for ba in (0, 1):
                d.set_option("ba_synch", ba)
                x, y = d.new_x(make_x(nl)), d.new_y()
                d.spmv(x, y); d.spmv(x, y); d.synchronize()
                assert torch.equal(x[nl:nl + d.n_halo], tail), (P, rank, overlap, pad, fused, ba)
                assert np.array_equal(d.y_to_original_order(y)[:nl], want), (P, rank, overlap, pad, fused, ba)
        d.set_option("pad_split", 0); d.set_option("fused_step", 0); d.set_option("overlap", 1); d.set_option("ba_synch", 0)
        x, y = d.new_x(make_x(nl)), d.new_y()
        d._refresh()
        e0 = d.eager_steps
        d.run(x, y, 5, use_graph=True); d.synchronize()
        d._refresh()
        assert not d.graph_captured and d.graph_launches == 0 and d.eager_steps == e0 + 5
        assert np.array_equal(d.y_to_original_order(y)[:nl], want)
        # the exchange is what makes y right; the self-check sees it
        x[nl:].zero_()
        y4 = d.new_y(); d.spmv(x, y4, comm_halos=False); d.synchronize()
        assert not np.array_equal(d.y_to_original_order(y4)[:nl], want)
        bad, _ = d.check(loc, d.new_x(np.zeros(nl)), d.new_y())
        assert bad == 0
        d.set_option("diag_skip_exchange", 1)
        bad, _ = d.check(loc, d.new_x(np.zeros(nl)), d.new_y())
        assert bad > 0
        d.set_option("diag_skip_exchange", 0)
        d.barrier()
        assert d.allreduce_max(3.5) == 3.5
        d.close()


def test_peer_loopback_block_vectors_match_rccl(pkg):
    """Block vectors in loopback: one push of all b columns into a window grown for b, every message pattern and layout, Y bitwise
    equal to the RCCL loopback's; the single-vector step keeps working in the grown window."""
    import torch
    torch.cuda.set_device(0)
    shape, P, rank = (16, 16, 40), 4, 1
    counts = pkg.gen_stencil27_row_counts(*shape)
    wsa = pkg.seg_from_row_counts(counts, "seg-rows", P)
    loc = pkg.gen_stencil27(*shape, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))
    nl = int(wsa[rank + 1] - wsa[rank])
    r = pkg.DistNative(loc, wsa, 32, 512, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1)
    d = pkg.DistNative(loc, wsa, 32, 512, rank, P, comm_rank=0, comm_size=1, exchange="peer")
    for b in (4, 8):
        Xo = [make_x(nl) * (1.0 + v / 8.0) for v in range(b)]
        for overlap in (1, 0):
            for layout, mode in ((pkg.COLWISE, 0), (pkg.COLWISE, 1), (pkg.COLWISE, 2), (pkg.ROWWISE, 0)):
                Ys = []
                for o in (r, d):
                    o.set_option("overlap", overlap)
                    X = o.new_X(Xo, b, layout)
                    Y = torch.full((b * o.padded_vec_size,), 7.0, dtype=torch.float64, device="cuda")
                    o.spmmv(X, Y, b, layout, mode); o.synchronize()
                    Ys.append((X.cpu().numpy(), Y.cpu().numpy()))
                assert np.array_equal(Ys[0][0], Ys[1][0]) and np.array_equal(Ys[0][1], Ys[1][1]), (b, overlap, layout, mode)
    x, y = d.new_x(make_x(nl)), d.new_y()
    xr, yr = r.new_x(make_x(nl)), r.new_y()
    d.spmv(x, y); r.spmv(xr, yr); d.synchronize(); r.synchronize()
    assert torch.equal(y, yr) and torch.equal(x, xr)
    d.close(); r.close()


# ---------------------------------------------------------------------------------------------------------------- real ranks
def _boot():
    """worker start: IPC between processes needs the non-legacy IPC mode, set before the HIP runtime starts (torch import)"""
    os.environ.update(IPC_ENV)
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.setdefault("OMP_NUM_THREADS", "4"); os.environ.setdefault("OMP_WAIT_POLICY", "passive")
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    torch.cuda.set_device(0)
    return torch, pkg


def _worker(fn, rank, world, q, job, args):
    try:
        q.put((rank, "ok", globals()[fn](rank, world, job, *args)))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc(), None))


def _run_ranks(fn, world, args=(), timeout=300):
    """`world` spawned rank processes on the one GPU; every wait has a deadline.  Returns the workers' results by rank."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    job = f"pe{os.getpid()}_{time.monotonic_ns()}"
    procs = [ctx.Process(target=_worker, args=(fn, r, world, q, job, args)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=timeout))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, msg, _ in sorted(res, key=lambda t: t[0]):
        assert msg == "ok", f"rank {rank}: {msg}"
    return [v for _, _, v in sorted(res, key=lambda t: t[0])]


def _golden_ranks(rank, world, job, case):
    torch, pkg = _boot()
    from ultimate_spmv_amd import binding as B
    name, Cc, sg, method = case
    key = f"{name}_C{Cc}_s{sg}_{method}_P{world}"
    h = np.load(os.path.join(GOLDEN, "halo.npz"))
    hc = pkg.HostComm(job, rank, world, timeout_s=120)
    tot = pkg.read_mtx(mtx_path(name))
    wsa = pkg.seg_work_sharing_arr(tot, method, world)
    assert np.array_equal(wsa, h[key + "_wsa"])
    loc = B.seg_local_coo(tot, wsa, rank)
    d = pkg.DistNative(loc, wsa, Cc, sg, rank, world, hostcomm=hc, exchange="peer")
    nl = int(wsa[rank + 1] - wsa[rank])
    assert d.exchange == "peer" and not d.loopback and d.comm_count() == 0 and d.n_local == nl
    xg = 1.0 + 1e-3 * (np.arange(tot.n_rows) % 1000)
    want = h[key + "_y_global"][wsa[rank]:wsa[rank + 1]]
    gx = h[f"{key}_r{rank}_x_local"]
    for overlap in (1, 0):
        d.set_option("overlap", overlap)
        for ba in (0, 1):
            d.set_option("ba_synch", ba)
            x, y = d.new_x(xg[wsa[rank]:wsa[rank + 1]]), d.new_y()
            d.spmv(x, y); d.spmv(x, y); d.spmv(x, y); d.synchronize()
            assert np.array_equal(x.cpu().numpy()[:len(gx)], gx), ("x_local", overlap, ba)
            assert np.array_equal(d.y_to_original_order(y)[:nl], want), (overlap, ba)
    d.set_option("overlap", 1)
    for pad, fused in ((1, 0), (1, 1), (0, 1)):
        d.set_option("pad_split", pad); d.set_option("fused_step", fused)
        for ba in (0, 1):
            d.set_option("ba_synch", ba)
            x, y = d.new_x(xg[wsa[rank]:wsa[rank + 1]]), d.new_y()
            d.spmv(x, y); d.spmv(x, y); d.synchronize()
            assert np.array_equal(x.cpu().numpy()[:len(gx)], gx), (pad, fused, ba)
            assert np.array_equal(d.y_to_original_order(y)[:nl], want), (pad, fused, ba)
    d.set_option("pad_split", 0); d.set_option("fused_step", 0); d.set_option("ba_synch", 0)
    # a graph request runs eagerly (the host waits inside every step) and stays right
    x, y = d.new_x(xg[wsa[rank]:wsa[rank + 1]]), d.new_y()
    d._refresh()
    e0 = d.eager_steps
    d.run(x, y, 4, use_graph=True); d.synchronize()
    d._refresh()
    assert not d.graph_captured and d.eager_steps == e0 + 4
    assert np.array_equal(d.y_to_original_order(y)[:nl], want)
    bad, _ = d.check(loc, d.new_x(np.zeros(nl)), d.new_y())
    assert bad == 0, bad
    bad, _ = d.check(loc, d.new_x(np.zeros(nl)), d.new_y(), use_graph=True)
    assert bad == 0, bad
    d.barrier()
    assert d.allreduce_max(float(rank)) == float(world - 1)
    d.close(); hc.close()


@pytest.mark.parametrize("case,world", [(("impcol_e", 8, 16, "seg-nnz"), 2), (("FDM-2d-16", 16, 512, "seg-nnz"), 3), (("bcsstk13", 32, 512, "seg-nnz"), 4)])
def test_peer_real_ranks_unequal_seg_nnz_blocks(pkg, case, world):
    """Real rank processes sharing the GPU, windows opened through IPC on the same device, unequal seg-nnz blocks with asymmetric lists:
    x_local with its halo tail and y bitwise against the reference's (tests/golden/halo.npz) for every arrangement of the step."""
    assert f"{case[0]}_C{case[1]}_s{case[2]}_{case[3]}_P{world}_wsa" in np.load(os.path.join(GOLDEN, "halo.npz"))
    _run_ranks("_golden_ranks", world, (case,))


def _block_ranks(rank, world, job):
    torch, pkg = _boot()
    from ultimate_spmv_amd import binding as B
    hc = pkg.HostComm(job, rank, world, timeout_s=120)
    tot = pkg.read_mtx(mtx_path("bcsstk13"))
    wsa = pkg.seg_work_sharing_arr(tot, "seg-nnz", world)
    loc = B.seg_local_coo(tot, wsa, rank)
    dh = pkg.DistNative(loc, wsa, 32, 512, rank, world, hostcomm=hc, host_exchange=True)
    dp = pkg.DistNative(loc, wsa, 32, 512, rank, world, hostcomm=hc, exchange="peer")
    xg = 1.0 + 1e-3 * (np.arange(tot.n_rows) % 1000)
    xl = xg[wsa[rank]:wsa[rank + 1]]
    for b in (4, 8):
        Xo = [xl * (1.0 + v / 8.0) for v in range(b)]
        for plan in ((0, b) if b == 8 else (0,)):
            if plan:
                dh.set_option("block_plan", plan); dp.set_option("block_plan", plan)
            for overlap in (1, 0):
                for layout, mode in ((pkg.COLWISE, 0), (pkg.COLWISE, 1), (pkg.COLWISE, 2), (pkg.ROWWISE, 0)):
                    got = []
                    for d in (dh, dp):
                        d.set_option("overlap", overlap)
                        X = d.new_X(Xo, b, layout)
                        Y = torch.full((b * d.padded_vec_size,), 7.0, dtype=torch.float64, device="cuda")
                        d.spmmv(X, Y, b, layout, mode); d.spmmv(X, Y, b, layout, mode); d.synchronize()
                        got.append((X.cpu().numpy(), Y.cpu().numpy()))
                    assert np.array_equal(got[0][0], got[1][0]), ("X", b, plan, overlap, layout, mode)
                    assert np.array_equal(got[0][1], got[1][1]), ("Y", b, plan, overlap, layout, mode)
    # the single-vector step in the grown window
    xs = [(d.new_x(xl), d.new_y()) for d in (dh, dp)]
    for d, (x, y) in zip((dh, dp), xs):
        d.set_option("overlap", 1)
        d.spmv(x, y); d.synchronize()
    assert torch.equal(xs[0][0], xs[1][0]) and torch.equal(xs[0][1], xs[1][1])
    dp.close(); dh.close(); hc.close()


def test_peer_real_ranks_block_vectors_match_host_staged(pkg):
    """b = 4 and 8 (the window grows collectively twice), column-wise in all three patterns and row-wise bulk, both step forms, gather kernels
    and the phased block plan: X and Y bitwise those of the same ranks' host-staged exchange, on unequal seg-nnz blocks."""
    _run_ranks("_block_ranks", 3)


def test_cli_peer_exchange_three_real_ranks_seg_nnz(pkg, tmp_path):
    """`uspmv gen:96x96x96 scs -c 32 -s 512 -dp -seg_nnz -comm_halos 1 -check_y 1` as THREE real rank processes sharing the GPU with
    USPMV_EXCHANGE=peer: the self-check passes on every rank, no RCCL communicator exists, -step_form auto timed its candidates."""
    g, P = 96, 3
    counts = pkg.gen_stencil27_row_counts(g, g, g)
    wsa = pkg.seg_from_row_counts(counts, "seg-nnz", P)
    js = str(tmp_path / "peer.json")
    procs = []
    for rank in range(P):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(P), LOCAL_RANK=str(rank), USPMV_EXCHANGE="peer", USPMV_ID_DIR=str(tmp_path),
                   USPMV_JOB_ID=f"pe5_{os.getpid()}", USPMV_HC_TIMEOUT="240", USPMV_STAGES="1", OMP_NUM_THREADS="4", **IPC_ENV)
        env.pop("USPMV_LOOPBACK", None)
        procs.append(subprocess.Popen([EXE, f"gen:{g}x{g}x{g}", "scs", "-c", "32", "-s", "512", "-dp", "-seg_nnz", "-comm_halos", "1", "-ba_synch", "0",
                                       "-bench_steps", "20", "-bench_warmup", "5", "-check_y", "1", "-json", js], cwd=tmp_path, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=600)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
    rep = json.load(open(js))
    assert rep["y_checked"] is True and rep["y_mismatches"] == 0 and rep["steps"] == 20 and rep["ranks"] == P
    assert rep["exchange"] == "peer" and rep["rccl_nranks"] == 0 and rep["loopback"] is False
    assert rep["step_form"] in ("overlap", "plain") and set(rep["step_form_candidates_ms"]) == {"overlap", "plain"}
    assert all(v > 0 for v in rep["step_form_candidates_ms"].values())
    assert [r["n_local"] for r in rep["per_rank"]] == np.diff(wsa).tolist()
    assert "(peer-store exchange)" in outs[0] and "y checked bitwise on every rank: ok" in outs[0]


# ---------------------------------------------------------------------------------------------------------------- refusals, leaks
def test_peer_real_ranks_without_a_transport_are_refused(pkg):
    """comm_size == P > 1 without a transport: refused on every rank before any collective (nothing to wait for)."""
    import torch
    torch.cuda.set_device(0)
    shape, P = (12, 12, 30), 3
    wsa = pkg.seg_from_row_counts(pkg.gen_stencil27_row_counts(*shape), "seg-nnz", P)
    msgs = set()
    for rank in range(P):
        loc = pkg.gen_stencil27(*shape, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))
        with pytest.raises(pkg.UspmvError) as e:
            pkg.DistNative(loc, wsa, 32, 512, rank, P, exchange="peer")
        assert e.value.status == 1 and "needs a transport" in str(e.value)
        msgs.add(str(e.value))
    assert len(msgs) == 1


def _refusal_ranks(rank, world, job):
    torch, pkg = _boot()
    from ultimate_spmv_amd import binding as B
    hc = pkg.HostComm(job, rank, world, timeout_s=60)
    tot = pkg.read_mtx(mtx_path("FDM-2d-16"))
    out = {}
    # a transport of 2 ranks for a 3-way partition
    wsa3 = pkg.seg_work_sharing_arr(tot, "seg-nnz", 3)
    try:
        pkg.DistNative(B.seg_local_coo(tot, wsa3, rank), wsa3, 16, 512, rank, 3, hostcomm=hc, exchange="peer")
        out["size"] = None
    except pkg.UspmvError as e:
        out["size"] = (e.status, str(e).replace(f"rank {rank} of", "rank R of").replace(f"is {rank} of", "is R of"))
    hc.barrier()
    # rank 1 announces one element more from rank 0 than rank 0 sends it (test-only option "diag_peer_skew") at the window growth of the
    # block step: every rank refuses alike before any kernel runs, and the object, left without windows, refuses steps instead of faulting
    wsa = pkg.seg_work_sharing_arr(tot, "seg-nnz", world)
    loc = B.seg_local_coo(tot, wsa, rank)
    d = pkg.DistNative(loc, wsa, 16, 512, rank, world, hostcomm=hc, exchange="peer")
    bad0, _ = d.check(loc, d.new_x(np.zeros(d.n_local)), d.new_y())
    out["check0"] = bad0
    if rank == 1:
        d.set_option("diag_peer_skew", 1)
    xl = 1.0 + 1e-3 * (np.arange(d.n_local) % 1000)
    X = d.new_X([xl, 2.0 * xl], 2)
    Y = torch.zeros_like(X)
    try:
        d.spmmv(X, Y, 2)
        out["skew"] = None
    except pkg.UspmvError as e:
        out["skew"] = (e.status, str(e))
    x, y = d.new_x(xl), d.new_y()
    for what, call in (("lost_spmv", lambda: d.spmv(x, y)), ("lost_run", lambda: d.run(x, y, 2, use_graph=True))):
        try:
            call()
            out[what] = None
        except pkg.UspmvError as e:
            out[what] = (e.status, str(e))
    d.synchronize()
    # every rank calls the block step again without the skew: the windows are set up anew and the step is right again
    if rank == 1:
        d.set_option("diag_peer_skew", 0)
    d.spmmv(X, Y, 2); d.synchronize()
    bad, _ = d.check(loc, d.new_x(np.zeros(d.n_local)), d.new_y())
    out["check"] = bad
    d.close(); hc.close()
    return out


def test_peer_setup_refusals_are_the_same_on_every_rank(pkg):
    """A transport whose size is not P, and a receive count that disagrees with the sender's (at the window growth of the block step):
    both refused with USPMV_ERR_INVALID and the same message on every rank, before any kernel runs; no rank hangs.  The object the failed
    growth left without windows refuses its steps (eager and graph requests) instead of launching on them, and a later block step on
    every rank sets the windows up again."""
    res = _run_ranks("_refusal_ranks", 2, timeout=240)
    for r in res:
        assert r["size"] is not None and r["size"][0] == 1 and "the transport is rank R of 2, the block is R of 3" in r["size"][1], r
        assert r["skew"] is not None and r["skew"][0] == 1 and "rank 0 sends" in r["skew"][1] and "to rank 1, which expects" in r["skew"][1], r
        for what in ("lost_spmv", "lost_run"):
            assert r[what] is not None and r[what][0] == 1 and "receive windows were lost" in r[what][1], (what, r)
        assert r["check0"] == 0 and r["check"] == 0
    assert res[0]["size"] == res[1]["size"] and res[0]["skew"] == res[1]["skew"]


def _leak_ranks(rank, world, job):
    torch, pkg = _boot()
    hc = pkg.HostComm(job, rank, world, timeout_s=120)
    shape, b = (64, 64, 64), 128
    wsa = pkg.seg_from_row_counts(pkg.gen_stencil27_row_counts(*shape), "seg-nnz", world)
    loc = pkg.gen_stencil27(*shape, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))
    nl = int(wsa[rank + 1] - wsa[rank])

    def cycle(kw):
        d = pkg.DistNative(loc, wsa, 32, 512, rank, world, hostcomm=hc, **kw)
        x, y = d.new_x(make_x(nl)), d.new_y()
        d.spmv(x, y); d.spmv(x, y)
        X = d.new_X([make_x(nl)] * b, b)
        Y = torch.zeros_like(X)
        d.spmmv(X, Y, b)                        # (peer: grows the windows to n_halo x 128 -- a collective close / barrier / free)
        d.synchronize()
        win = 2 * d.n_halo * b * 8
        d.close()
        del x, y, X, Y
        torch.cuda.synchronize()
        hc.barrier()                            # both ranks have freed everything before anyone measures
        return win

    lost = {}
    for name, kw in (("host", {"host_exchange": True}), ("peer", {"exchange": "peer"})):
        cycle(kw); cycle(kw)
        free0, _ = torch.cuda.mem_get_info()
        hc.barrier()
        for _ in range(5):
            win = cycle(kw)
        free1, _ = torch.cuda.mem_get_info()
        hc.barrier()
        lost[name] = free0 - free1
    hc.close()
    return lost, win


def test_peer_objects_do_not_leak_device_memory(pkg):
    """Five create / step / spmmv / free cycles of a 2-rank peer object (windows exported, opened, grown, closed, freed each time): the
    GPU's free memory, seen by each rank after both have freed, is what it was after two warm-up cycles, within the allowance
    test_gpu_leaks.py grants every distributed object (4 MiB per cycle: the host-staged object, measured in the same processes, loses
    that much without any window) -- and no more than 4 MiB beyond what the host-staged object loses.  The grown window (n_halo x 128
    columns, two halves) is sized so that ONE rank keeping it every cycle exceeds both bounds, even when the host-staged object loses
    its whole allowance."""
    res = _run_ranks("_leak_ranks", 2)
    for rank, (lost, win) in enumerate(res):
        assert 5 * win > 5 * (4 << 20) + (4 << 20), win
        assert lost["peer"] <= 5 * (4 << 20), f"rank {rank}: {lost['peer'] / 2**20:.1f} MiB of device memory lost over five cycles"
        assert lost["peer"] <= lost["host"] + (4 << 20), (rank, lost)
