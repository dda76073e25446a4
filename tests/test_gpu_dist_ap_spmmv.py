"""Adaptive precision ap[dp_sp] on block vectors across ranks: the list forms of the pair's block kernels (uspmv_spmmv_ap_tiles /
_chunks, uspmv_spmmv_ap_tiles_path) and the block step of an ap object (uspmv_dist_spmmv_ap) -- loopback on one GPU, the block padding
guard, real ranks sharing the GPU over the host-staged exchange.  Every comparison is bitwise: against uspmv_spmmv_ap / uspmv_spmv_ap for
the kernels, against the oracle's scs_ap_impl_cpu on the WHOLE matrix and against b single-vector steps for the step.

The path query answers for 16-byte-aligned vectors (its ABI carries no pointers), so the unaligned launch is checked by its bits and its
untouched surroundings alone, as the whole-matrix tests do."""
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, make_x, mtx_path
from test_dist_ap_host import whole_matrix_ap_reference
from test_gpu_dist_ap import THR, _block, _pair_on_device, _reference

pytestmark = pytest.mark.gpu
COL, ROW = 0, 1
BULK, MULTI, SINGLE = 0, 1, 2
NAN = float("nan")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _scale(v):
    return 1.0 + (v % 8) / 8.0


def _view(T, b, ld, layout):
    """T as [vector][row]"""
    return T.view(ld, b).t() if layout == ROW else T.view(b, ld)


def _vectors(b, lines):
    """vectors per pass of the staged kernel: the largest of 8, 4, 2 that is at most b, divides b and whose `lines` lines x 16 X rows x 8
    bytes per vector fit the 160 KiB of LDS a workgroup can have"""
    return next(bs for bs in (8, 4, 2) if bs <= b and b % bs == 0 and lines * 128 * bs <= 160 * 1024)


def _ids_with_holes(n_ids, par):
    real = np.arange(par, n_ids, 2, dtype=np.int32)
    ids = np.full(2 * len(real), -1, np.int32)
    ids[1::2] = real                                   # -1, id, -1, id, ...
    ids = ids[len(ids) - min(len(ids), n_ids):]        # (a list is at most n_ids long: an odd count drops the leading -1)
    assert (ids < 0).any() and np.array_equal(ids[ids >= 0], real)
    return ids


def _check_block_lists(t, launch, n_ids, full, X, b, ld, layout, npad):
    """odd / even ids interleaved with -1, each into a NaN-filled Y: the rows written are disjoint and together the full launch (every
    column); only -1: untouched; the elements [n_rows_padded, ld) of a column are never written"""
    rows = ld if layout == COL else npad
    ws = []
    for par in (0, 1):
        Y = t.full((b * rows,), NAN, dtype=t.float64, device="cuda")
        launch(t.from_numpy(_ids_with_holes(n_ids, par)).cuda(), X, Y)
        Yv = _view(Y, b, rows, layout)
        w = ~t.isnan(Yv)
        assert bool((w == w[0]).all())                 # a row is written in every column or in none
        assert not bool(w[:, npad:].any())
        ws.append((w, Yv))
    t.cuda.synchronize()
    (w0, Y0), (w1, Y1) = ws
    assert not bool((w0 & w1).any()) and bool((w0 | w1)[:, :npad].all())
    assert t.equal(t.where(w0, Y0, Y1)[:, :npad], full)
    Y = t.full((b * rows,), NAN, dtype=t.float64, device="cuda")
    launch(t.full((min(5, n_ids),), -1, dtype=t.int32, device="cuda"), X, Y)
    t.cuda.synchronize()
    assert bool(t.isnan(Y).all())


@pytest.mark.parametrize("C,sigma,narrow", [(32, 512, False), (16, 64, False), (32, 512, True)])
def test_list_forms_give_the_rows_of_the_full_launch(pkg, torch_cuda, C, sigma, narrow):
    """C 32: the CT = 32 instantiations, C 16: CT = 0; narrow: a line budget at the median tile, so tiles without a line list (nl == 0,
    the wide-footprint branch) sit next to staged ones.  b 16 (and b 8 where only four vectors of the fullest tile fit LDS) are the
    several-pass cases of the staged kernel; b 3 / an odd column-major ld / "tlc" 0 / unaligned X run lane per row over the tiles' rows."""
    t = torch_cuda
    s_dp, s_sp, A_dp, A_sp = _pair_on_device(pkg, (40, 40, 5), C, sigma)
    npad, n = s_dp.n_rows_padded, s_dp.n_rows
    assert npad % 2 == 0
    xb = make_x(n)
    ycols = []                                            # column v of every Y below: uspmv_spmv_ap of column v, planless (lane per row)
    for v in range(8):
        x = t.zeros(npad, dtype=t.float64, device="cuda")
        x[:n] = t.from_numpy(xb * _scale(v)).cuda()
        y = t.full((npad,), NAN, dtype=t.float64, device="cuda")
        pkg.spmv_ap(A_dp, A_sp, x, y)
        ycols.append(y)
    t.cuda.synchronize()
    assert not any(bool(t.isnan(y).any()) for y in ycols)
    ids4 = t.arange(4, dtype=t.int32, device="cuda")
    X4, Y4 = t.zeros(4 * npad, dtype=t.float64, device="cuda"), t.zeros(4 * npad, dtype=t.float64, device="cuda")
    with pytest.raises(pkg.UspmvError, match="uspmv_spmmv_ap_tiles: the pair has no shared tile-local-column plan"):
        pkg.spmmv_ap_tiles(A_dp, A_sp, ids4, X4, Y4, 4, npad)
    with pytest.raises(pkg.UspmvError, match="uspmv_spmmv_ap_tiles_path: the pair has no shared tile-local-column plan"):
        pkg.spmmv_ap_tiles_path(A_dp, A_sp, 4, npad)
    pkg.set_tuning(sweep=0)                               # (keep the line plan whatever it stages: this test is about its kernel)
    try:
        n_tiles, n_staged = pkg.optimize_ap(A_dp, A_sp, s_dp, s_sp)
        nl = np.diff(A_dp.plan_download()["tile_line_ptr"])
        assert n_tiles >= 4 and n_staged == n_tiles and (nl > 0).all()
        if narrow:
            budget = int(np.sort(nl)[len(nl) // 2])       # the median tile still stages, the fuller ones do not
            assert budget < nl.max()
            n_tiles, n_staged = pkg.optimize_ap(A_dp, A_sp, s_dp, s_sp, budget)
            nl = np.diff(A_dp.plan_download()["tile_line_ptr"])
            assert (nl == 0).any() and (nl > 0).any() and 0 < n_staged < n_tiles
    finally:
        pkg.set_tuning(sweep=1)
    n_chunks = s_dp.n_chunks
    # Vectors per pass.  The staged kernel keeps the fullest tile's lines in LDS: L lines x 16 X rows x 8 bytes per vector, 160 KiB per
    # workgroup, so 8 vectors per pass need L <= 160.  The plan of C 16 / sigma 64 has 121 lines: min(b, 8) vectors, b 16 in two
    # passes.  The tiles of C 32 / sigma 512 list 194 (narrow budget: 173) lines -- 194 x 128 x 8 = 198 656 bytes do not fit,
    # so b 8 and b 16 run 4 vectors per pass there (two and four passes): what the LDS leaves, asserted from the plan's own line count.
    L = int(nl.max())
    print(f"C={C} sigma={sigma} narrow={narrow}: {n_tiles} tiles, fullest tile {L} lines")
    if (C, sigma) == (16, 64):
        assert L <= 160 and all(_vectors(b, L) == min(b, 8) for b in (2, 4, 8, 16))

    def make_X(b, ld, layout, offset=0):
        rows = ld if layout == COL else npad
        buf = t.zeros(b * rows + offset, dtype=t.float64, device="cuda")
        X = buf[offset:]
        Xv = _view(X, b, rows, layout)
        for v in range(b):
            Xv[v, :n] = t.from_numpy(xb * _scale(v)).cuda()
        return X

    def run_case(b, ld, layout, want_path, offset=0, chunks=True):
        rows = ld if layout == COL else npad
        X = make_X(b, ld, layout, offset)
        assert (X.data_ptr() % 16 == 0) == (offset == 0)
        if offset == 0:
            assert pkg.spmmv_ap_tiles_path(A_dp, A_sp, b, ld, layout) == want_path, (b, ld, layout)
        Yf = t.full((b * rows,), NAN, dtype=t.float64, device="cuda")
        pkg.spmmv_ap(A_dp, A_sp, X, Yf, b, ld, layout)
        t.cuda.synchronize()
        full = _view(Yf, b, rows, layout)[:, :npad]
        assert bool(t.isnan(_view(Yf, b, rows, layout)[:, npad:]).all())
        for v in range(b):
            assert t.equal(full[v], ycols[v % 8]), (b, ld, layout, v)
        _check_block_lists(t, lambda i, xx, yy: pkg.spmmv_ap_tiles(A_dp, A_sp, i, xx, yy, b, ld, layout), n_tiles, full, X, b, ld, layout, npad)
        if chunks:
            _check_block_lists(t, lambda i, xx, yy: pkg.spmmv_ap_chunks(A_dp, A_sp, i, xx, yy, b, ld, layout), n_chunks, full, X, b, ld, layout, npad)

    for b in (2, 4, 8, 16, 3):
        staged = (2, _vectors(b, L)) if b != 3 else (0, 0)
        run_case(b, npad, ROW, staged)
        run_case(b, npad, COL, staged)
        run_case(b, npad + 1, COL, (0, 0), chunks=b in (4, 3))         # odd ld: no 16-byte pieces of the columns
    run_case(4, npad, COL, None, offset=1, chunks=False)               # X 8 bytes off: lane per row, same bits
    run_case(4, npad, ROW, None, offset=1, chunks=False)
    pkg.set_tuning(tlc=0)
    try:
        for b in (2, 4, 8, 16):
            assert pkg.spmmv_ap_tiles_path(A_dp, A_sp, b, npad, COL) == (0, 0) and pkg.spmmv_ap_tiles_path(A_dp, A_sp, b, npad, ROW) == (0, 0)
        run_case(4, npad, COL, (0, 0), chunks=False)
    finally:
        pkg.set_tuning(tlc=1)
    variant = pkg.get_tuning("spmmv_variant")
    pkg.set_tuning(spmmv_variant=1)
    try:
        assert variant != 1 and pkg.spmmv_ap_tiles_path(A_dp, A_sp, 4, npad, ROW) == (0, 0)
    finally:
        pkg.set_tuning(spmmv_variant=variant)
    assert pkg.spmmv_ap_tiles_path(A_dp, A_sp, 4, npad, ROW) == (2, _vectors(4, L))
    # the refusals of the single-vector list forms, under the new names
    X, Y = make_X(4, npad, COL), t.full((4 * npad,), NAN, dtype=t.float64, device="cuda")
    for fn, n_max in ((pkg.spmmv_ap_tiles, n_tiles), (pkg.spmmv_ap_chunks, n_chunks)):
        name = "uspmv_" + fn.__name__
        with pytest.raises(pkg.UspmvError, match=name + ": bad argument"):
            fn(A_dp, A_sp, t.zeros(n_max + 1, dtype=t.int32, device="cuda"), X, Y, 4, npad)
        with pytest.raises(pkg.UspmvError, match=name + ": expects a double and a float"):
            fn(A_sp, A_dp, ids4, X, Y, 4, npad)
        with pytest.raises(pkg.UspmvError, match=name + ": ld="):
            fn(A_dp, A_sp, ids4, X, Y, 4, npad - 1, COL)
        with pytest.raises(pkg.UspmvError, match=name + ": b=0"):
            fn(A_dp, A_sp, ids4, X, Y, 0, npad)
        fn(A_dp, A_sp, ids4[:0], X, Y, 4, npad)                          # an empty list: USPMV_OK, nothing launched
    t.cuda.synchronize()
    assert bool(t.isnan(Y).all())
    with pytest.raises(pkg.UspmvError, match="uspmv_spmmv_ap_tiles_path: expects a double and a float"):
        pkg.spmmv_ap_tiles_path(A_sp, A_dp, 4, npad)


def _columns(nl, b, xb=None):
    base = make_x(nl) if xb is None else xb
    return [base * _scale(v) for v in range(b)]


def _halo_tail(d, X, b, layout):
    return _view(X, b, d.padded_vec_size, layout)[:, d.n_local:d.n_local + d.n_halo].clone()


@pytest.mark.parametrize("P,shape,C,sigma,tlc", [(2, (24, 24, 24), 32, 512, True), (4, (16, 16, 40), 32, 512, True), (3, (20, 9, 27), 16, 64, True),
                                                 (2, (24, 24, 24), 32, 512, False)])
def test_block_step_loopback_bitexact(pkg, orc, torch_cuda, P, shape, C, sigma, tlc):
    """Every rank of the four loopback cases of the single-vector test.  Y of the default form in original order is, per column, the
    oracle's whole-matrix product; Y and the halo tail of X are those of b single-vector steps; "pad_split" 0, "overlap" 0 and "ba_synch" 1
    give the same bits, comm_halos=False does not; uspmv_dist_spmmv_info counts the forms taken."""
    torch = torch_cuda
    first = (P, shape, tlc) == (2, (24, 24, 24), True)
    nl = _reference(pkg, orc, shape, P, C, sigma)[1]
    want = [_reference(pkg, orc, shape, P, C, sigma, xblock=c)[0] for c in _columns(nl, 8)]
    for rank in range(P):
        wsa, loc = _block(pkg, shape, P, rank)
        rows = slice(int(wsa[rank]), int(wsa[rank + 1]))
        for exchange in ("rccl", "peer") if first else ("rccl",):
            d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id() if exchange == "rccl" else None, comm_rank=0, comm_size=1,
                               tlc=tlc, ap_threshold=THR, exchange=exchange)
            assert d.loopback and d.n_local == nl and d.n_halo > 0 and d.use_tiles == tlc
            ld, npad = d.padded_vec_size, d.n_rows_padded
            single = []                                                 # (y, halo tail of x) of the single-vector step, per column
            for v, c in enumerate(_columns(nl, 8)):
                x = d.new_x(c); y = torch.full_like(d.new_y(), NAN)
                d.spmv(x, y); d.synchronize()
                assert np.array_equal(d.y_to_original_order(y)[:nl], want[v][rows]), (rank, exchange, v)
                single.append((y[:npad].clone(), x[d.n_local:d.n_local + d.n_halo].clone()))
            counts = d.spmmv_info()
            two, one = counts["two_part"], counts["one_part"]
            for b in (2, 4, 8, 3, 16) if first else (2, 4, 8, 3):
                for layout, mode in ((COL, BULK), (COL, MULTI), (COL, SINGLE), (ROW, BULK)):
                    tag = (P, rank, exchange, b, layout, mode)

                    def step(**kw):
                        X = d.new_X(_columns(nl, b), b, layout)
                        Y = torch.full((b * ld,), NAN, dtype=torch.float64, device="cuda")
                        d.spmmv_ap(X, Y, b, layout, mode, **kw); d.synchronize()
                        return _view(Y, b, ld, layout), _halo_tail(d, X, b, layout)

                    Yv, halo = step()                                   # overlap, "pad_split" 1: the object's default
                    two += 1
                    assert not bool(torch.isnan(Yv[:, :npad]).any()) and bool(torch.isnan(Yv[:, npad:]).all()), tag
                    for v in range(b):
                        assert np.array_equal(d.y_to_original_order(Yv[v].contiguous())[:nl], want[v % 8][rows]), (tag, v)
                        assert torch.equal(Yv[v, :npad], single[v % 8][0]) and torch.equal(halo[v], single[v % 8][1]), (tag, v)
                    d.set_option("pad_split", 0); Y2, h2 = step(); d.set_option("pad_split", 1)
                    two += 1
                    assert torch.equal(Y2[:, :npad], Yv[:, :npad]) and torch.equal(h2, halo), (tag, "pad_split 0")
                    d.set_option("overlap", 0); Y2, h2 = step(); d.set_option("overlap", 1)
                    one += 1
                    assert torch.equal(Y2[:, :npad], Yv[:, :npad]) and torch.equal(h2, halo), (tag, "overlap 0")
                    if mode == BULK:
                        d.set_option("ba_synch", 1); Y2, h2 = step(); d.set_option("ba_synch", 0)
                        two += 1
                        assert torch.equal(Y2[:, :npad], Yv[:, :npad]) and torch.equal(h2, halo), (tag, "ba_synch")
                        Y2, h2 = step(comm_halos=False)
                        assert not torch.equal(Y2[:, :npad], Yv[:, :npad]) and not bool(h2.any()), (tag, "comm_halos=False")
                    counts = d.spmmv_info()
                    assert (counts["two_part"], counts["one_part"]) == (two, one), (tag, counts)
            # b = 1 is the eager single-vector step
            x = d.new_x(make_x(nl)); y = torch.full_like(d.new_y(), NAN)
            d.spmmv_ap(x, y, 1); d.synchronize()
            assert torch.equal(y[:npad], single[0][0]) and d.spmmv_info()["two_part"] == two
            d.close()


def test_block_padding_guard(pkg, orc, torch_cuda):
    """The slot of the padding column holds one value per vector.  Positive in every column: no re-run.  Negative in the last column
    only: one re-run, none on a second step over the same X.  +Inf in one column only: NaN where the oracle has it, in that column only,
    and a re-run every step.  "pad_split" 0: never a re-run."""
    torch = torch_cuda
    P, shape, C, sigma, rank, b = 4, (16, 16, 40), 32, 512, 2, 4
    wsa, loc = _block(pkg, shape, P, rank)
    nl = int(wsa[1] - wsa[0])
    rows = slice(int(wsa[rank]), int(wsa[rank + 1]))
    pos = _columns(nl, b)
    neg = [c.copy() for c in pos]; neg[b - 1][0] = -2.5
    inf = [c.copy() for c in pos]; inf[1][0] = np.inf
    cases = {"pos": pos, "neg": neg, "inf": inf}
    want = {tag: [_reference(pkg, orc, shape, P, C, sigma, xblock=c)[0][rows] for c in cols] for tag, cols in cases.items()}
    assert np.isnan(want["inf"][1]).any() and not np.isnan(want["inf"][1]).all()
    assert not any(np.isnan(w).any() for tag in ("pos", "neg") for w in want[tag]) and not any(np.isnan(want["inf"][v]).any() for v in (0, 2, 3))
    d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_threshold=THR)
    info = d.pad_info()
    assert info["pad_tiles"] > 0 and info["pad_col"] >= d.n_local and info["real_boundary_tiles"] > 0, info
    ld = d.padded_vec_size

    def run(tag, layout, steps=1):
        X = d.new_X(cases[tag], b, layout)
        Y = torch.full((b * ld,), NAN, dtype=torch.float64, device="cuda")
        for _ in range(steps):
            d.spmmv_ap(X, Y, b, layout)
        d.synchronize()
        Yv = _view(Y, b, ld, layout)
        for v in range(b):
            assert np.array_equal(d.y_to_original_order(Yv[v].contiguous())[:nl], want[tag][v], equal_nan=True), (tag, layout, steps, v)
        return d.pad_info()["reruns"]

    for layout in (COL, ROW):
        r0 = d.pad_info()["reruns"]
        assert run("pos", layout) == r0                       # a fresh X: the slots held +0, same sign in every column
        r1 = run("neg", layout)                               # fresh X again: +0 -> -2.5 in the last column only
        assert r1 == r0 + 1
        assert run("neg", layout, steps=2) == r1 + 1          # the second step over the SAME X finds -2.5 in the slot already
        r2 = d.pad_info()["reruns"]
        assert run("inf", layout, steps=2) == r2 + 2          # not finite: every step
        d.set_option("pad_split", 0)
        r3 = d.pad_info()["reruns"]
        assert run("neg", layout) == r3 and run("inf", layout) == r3 and run("pos", layout) == r3
        d.set_option("pad_split", 1)
    d.close()


def test_block_step_refusals(pkg, torch_cuda):
    torch = torch_cuda
    P, shape, C, sigma, rank, b = 2, (24, 24, 24), 32, 512, 1, 2
    wsa, loc = _block(pkg, shape, P, rank)
    d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_threshold=THR)
    one = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1)
    X = torch.zeros(b * d.padded_vec_size, dtype=torch.float64, device="cuda")
    Y = torch.zeros_like(X)
    with pytest.raises(pkg.UspmvError, match="uspmv_dist_spmmv_ap: a one-precision object") as e:
        one.spmmv_ap(X, Y, b)
    assert e.value.status == 3                                # USPMV_ERR_UNSUPPORTED
    for mode in (MULTI, SINGLE):
        with pytest.raises(pkg.UspmvError, match="uspmv_dist_spmmv_ap: row-wise block vectors travel in one message per neighbour") as e:
            d.spmmv_ap(X, Y, b, ROW, mode)
        assert e.value.status == 3
    with pytest.raises(pkg.UspmvError, match="uspmv_dist_spmmv_ap: unknown mode 3"):
        d.spmmv_ap(X, Y, b, COL, 3)
    with pytest.raises(pkg.UspmvError, match="adaptive-precision"):      # what stays refused on an ap object
        d.spmmv(X, Y, b)
    assert d.spmmv_info()["two_part"] == 0 and d.spmmv_info()["one_part"] == 0
    d.close(); one.close()


def _ap_block_worker(rank, world, q, job, case):
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.setdefault("OMP_NUM_THREADS", "4"); os.environ.setdefault("OMP_WAIT_POLICY", "passive")   # (several rank processes share the box's cores)
        import torch
        import __graft_entry__ as ge
        pkg = ge.load_package()
        from ultimate_spmv_amd import binding as B
        from oracle import oracle as orc
        torch.cuda.set_device(0)
        name, Cc, sg, method, thr, b = case
        hc = pkg.HostComm(job, rank, world, timeout_s=120)
        tot = pkg.read_mtx(mtx_path(name))
        wsa = pkg.seg_work_sharing_arr(tot, method, world)
        xg = make_x(tot.n_rows)
        rows = slice(int(wsa[rank]), int(wsa[rank + 1]))
        want = []
        for v in range(b):
            y_ref, n_dp, n_sp = whole_matrix_ap_reference(pkg, orc, tot, Cc, sg, thr, xg * _scale(v))
            assert n_dp > 0 and n_sp > 0
            want.append(y_ref[rows])
        loc = B.seg_local_coo(tot, wsa, rank)
        d = pkg.DistNative(loc, wsa, Cc, sg, rank, world, hostcomm=hc, host_exchange=True, ap_threshold=thr)
        nl = int(wsa[rank + 1] - wsa[rank])
        assert d.n_local == nl and not d.loopback
        ld = d.padded_vec_size
        for layout, mode in ((COL, MULTI), (ROW, BULK)):
            for overlap in (1, 0):
                d.set_option("overlap", overlap)
                X = d.new_X([xg[rows] * _scale(v) for v in range(b)], b, layout)
                Y = torch.full((b * ld,), NAN, dtype=torch.float64, device="cuda")
                d.spmmv_ap(X, Y, b, layout, mode); d.synchronize()
                Yv = _view(Y, b, ld, layout)
                for v in range(b):
                    assert np.array_equal(d.y_to_original_order(Yv[v].contiguous())[:nl], want[v]), (layout, mode, overlap, v)
        info = d.spmmv_info()
        assert (info["two_part"], info["one_part"]) == (2, 2), info
        d.barrier()
        d.close(); hc.close()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def test_block_step_real_ranks_unequal_seg_nnz_blocks(pkg):
    """bcsstk13 cut by entries into three unequal blocks with asymmetric lists: three real processes share the GPU over the host-staged
    exchange; b = 4, column-wise multivec and row-wise bulkvec, every row of every rank against the oracle's whole-matrix ap product.
    Every child is bounded by a time limit; the first failure ends the run and nothing is tried again."""
    world, case = 3, ("bcsstk13", 32, 512, "seg-nnz", 1.0, 4)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    job = f"apb{os.getpid()}_{time.monotonic_ns()}"
    procs = [ctx.Process(target=_ap_block_worker, args=(r, world, q, job, case)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=240))
            if res[-1][1] != "ok":
                break
    finally:
        failed = any(msg != "ok" for _, msg in res) or len(res) < world
        for p in procs:
            if failed and p.is_alive():
                p.kill()
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, msg in sorted(res):
        assert msg == "ok", f"rank {rank}: {msg}"
    assert len(res) == world
