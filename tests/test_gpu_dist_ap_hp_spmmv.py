"""The adaptive-precision kinds with an fp16 part (ap[dp_hp], ap[sp_hp], ap[dp_sp_hp]) on block vectors across ranks: the list forms of
their block kernels (uspmv_spmmv_ap_hp_tiles / _chunks, uspmv_spmmv_ap_hp_tiles_path) -- with column-major X at leading dimensions whose
columns do not start on 16-byte boundaries, staged in 8- and 4-byte pieces -- and the block step of such an object
(uspmv_dist_spmmv_ap_hp): loopback on one GPU, the block padding guard on doubles and on floats, real ranks sharing the GPU over the
host-staged exchange.  Every comparison is bitwise (a NaN equals any NaN, _same of test_gpu_ap_hp.py): against uspmv_spmv_ap_hp /
uspmv_spmmv_ap_hp for the kernels, against the oracle composed part by part on the WHOLE matrix and against b single-vector steps for the
step.

The path query answers for 16-byte-aligned vectors (its ABI carries no pointers), so the unaligned launch is checked by its bits and its
untouched surroundings alone."""
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, make_x, mtx_path
from test_dist_ap_hp_host import DEC, T1, T2, whole_matrix_ap_hp_reference
from test_gpu_ap_hp import KINDS, _build, _same
from test_gpu_dist_ap_hp import _block, _reference
from test_gpu_dist_ap_spmmv import _columns, _halo_tail, _ids_with_holes, _scale, _view

pytestmark = pytest.mark.gpu
COL, ROW = 0, 1
BULK, MULTI, SINGLE = 0, 1, 2
NAN = float("nan")
CASES = [(2, (24, 24, 24), 32, 512, True), (4, (16, 16, 40), 32, 512, True), (3, (20, 9, 27), 16, 64, True), (2, (24, 24, 24), 32, 512, False)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _vectors(b, lines, itemsize):
    """vectors per pass of the staged kernel: the largest of 8, 4, 2 that is at most b, divides b and whose `lines` lines x 16 X rows x
    itemsize bytes per vector fit the 160 KiB of LDS a workgroup can have"""
    return next(bs for bs in (8, 4, 2) if bs <= b and b % bs == 0 and lines * 16 * itemsize * bs <= 160 * 1024)


def _check_block_lists(t, launch, n_ids, full, X, b, ld, layout, npad):
    """odd / even ids interleaved with -1, each into a NaN-filled Y: the rows written are disjoint and together the full launch (every
    column); only -1: untouched; the elements [n_rows_padded, ld) of a column are never written"""
    rows = ld if layout == COL else npad
    ws = []
    for par in (0, 1):
        Y = t.full((b * rows,), NAN, dtype=full.dtype, device="cuda")
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
    Y = t.full((b * rows,), NAN, dtype=full.dtype, device="cuda")
    launch(t.full((min(5, n_ids),), -1, dtype=t.int32, device="cuda"), X, Y)
    t.cuda.synchronize()
    assert bool(t.isnan(Y).all())


@pytest.mark.parametrize("C,sigma,narrow", [(32, 512, False), (16, 64, False), (32, 512, True)])
@pytest.mark.parametrize("kind", KINDS)
def test_list_forms_give_the_rows_of_the_full_launch(pkg, torch_cuda, kind, C, sigma, narrow):
    """C 32: the CT = 32 instantiations, C 16: CT = 0; narrow: a line budget at the median tile, so tiles without a line list (nl == 0,
    the wide-footprint branch) sit next to staged ones.  Column-major X at ld = npad + 1 .. npad + 3: columns that start 8 bytes off the
    16-byte grid for double X (8-byte pieces), 4, 8 and 12 bytes off for float X (4-, 8- and 4-byte pieces) -- all staged; the rows of X
    beyond the plan's x_len hold NaN there, which no product may meet.  b 3 / "tlc" 0 / "spmmv_variant" 1 / unaligned X run lane per
    row over the tiles' rows."""
    t = torch_cuda
    coo = pkg.gen_stencil27(40, 40, 5, magnitude_decades=DEC)
    structs, _ = _build(pkg, coo, kind, C, sigma, T1, T2)
    assert all(s.nnz > 0 for s in structs if s is not None) and (structs[1] is None) == (kind != "dp_sp_hp")
    A = [pkg.DeviceMatrix(s) if s is not None else None for s in structs]
    sh = structs[0]
    npad, n, dt = sh.n_rows_padded, sh.n_rows, t.float32 if kind == "sp_hp" else t.float64
    size = 4 if kind == "sp_hp" else 8
    x_len = max(int(s.arrays()["col_idxs"].max()) for s in structs if s is not None) + 1
    assert npad % 4 == 0 and n <= x_len <= npad
    xb = make_x(n)
    cols = [t.from_numpy(xb * _scale(v)).cuda().to(dt) for v in range(8)]
    ycols = []                                            # column v of every Y below: uspmv_spmv_ap_hp of column v, planless (lane per row)
    for v in range(8):
        x = t.zeros(npad, dtype=dt, device="cuda")
        x[:n] = cols[v]
        y = t.full((npad,), NAN, dtype=dt, device="cuda")
        pkg.spmv_ap_hp(*A, x, y)
        ycols.append(y)
    t.cuda.synchronize()
    assert not any(bool(t.isnan(y).any()) for y in ycols)
    ids4 = t.arange(4, dtype=t.int32, device="cuda")
    X4, Y4 = t.zeros(4 * npad, dtype=dt, device="cuda"), t.zeros(4 * npad, dtype=dt, device="cuda")
    with pytest.raises(pkg.UspmvError, match="uspmv_spmmv_ap_hp_tiles: the parts have no shared tile-local-column plan"):
        pkg.spmmv_ap_hp_tiles(*A, ids4, X4, Y4, 4, npad)
    with pytest.raises(pkg.UspmvError, match="uspmv_spmmv_ap_hp_tiles_path: the parts have no shared tile-local-column plan"):
        pkg.spmmv_ap_hp_tiles_path(*A, 4, npad)
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
    n_chunks = sh.n_chunks
    L = int(nl.max())
    print(f"{kind} C={C} sigma={sigma} narrow={narrow}: {n_tiles} tiles, fullest tile {L} lines, x_len {x_len}, npad {npad}")

    def make_X(b, ld, layout, offset=0):
        rows = ld if layout == COL else npad
        buf = t.zeros(b * rows + offset, dtype=dt, device="cuda")
        X = buf[offset:]
        Xv = _view(X, b, rows, layout)
        for v in range(b):
            Xv[v, :n] = cols[v % 8]
            if ld > npad:
                Xv[v, x_len:] = NAN                       # nothing references these rows; the staging writes zeros for them
        return X

    def run_case(b, ld, layout, want_path, offset=0, chunks=True):
        rows = ld if layout == COL else npad
        X = make_X(b, ld, layout, offset)
        assert (X.data_ptr() % 16 == 0) == (offset == 0)
        if offset == 0:
            assert pkg.spmmv_ap_hp_tiles_path(*A, b, ld, layout) == want_path, (b, ld, layout)
        Yf = t.full((b * rows,), NAN, dtype=dt, device="cuda")
        pkg.spmmv_ap_hp(*A, X, Yf, b, ld, layout)
        t.cuda.synchronize()
        full = _view(Yf, b, rows, layout)[:, :npad]
        assert bool(t.isnan(_view(Yf, b, rows, layout)[:, npad:]).all())
        for v in range(b):
            assert t.equal(full[v], ycols[v % 8]), (b, ld, layout, v)
        _check_block_lists(t, lambda i, xx, yy: pkg.spmmv_ap_hp_tiles(*A, i, xx, yy, b, ld, layout), n_tiles, full, X, b, ld, layout, npad)
        if chunks:
            _check_block_lists(t, lambda i, xx, yy: pkg.spmmv_ap_hp_chunks(*A, i, xx, yy, b, ld, layout), n_chunks, full, X, b, ld, layout, npad)

    for b in (2, 4, 8, 16, 3):
        staged = (2, _vectors(b, L, size)) if b != 3 else (0, 0)
        run_case(b, npad, ROW, staged)
        run_case(b, npad, COL, staged)
        lds = (npad + 1, npad + 2, npad + 3)              # column-major takes every ld
        assert [(ld * size) % 16 for ld in lds] == ([8, 0, 8] if size == 8 else [4, 8, 12])
        for ld in lds:
            run_case(b, ld, COL, staged)
    run_case(4, npad, COL, None, offset=1, chunks=False)               # X one element off: lane per row, same bits
    run_case(4, npad, ROW, None, offset=1, chunks=False)
    pkg.set_tuning(tlc=0)
    try:
        for b in (2, 4, 8, 16):
            assert pkg.spmmv_ap_hp_tiles_path(*A, b, npad + 1, COL) == (0, 0) and pkg.spmmv_ap_hp_tiles_path(*A, b, npad, ROW) == (0, 0)
        run_case(4, npad, COL, (0, 0), chunks=False)
        run_case(4, npad + 1, COL, (0, 0), chunks=False)
    finally:
        pkg.set_tuning(tlc=1)
    variant = pkg.get_tuning("spmmv_variant")
    pkg.set_tuning(spmmv_variant=1)
    try:
        assert variant != 1
        run_case(4, npad, ROW, (0, 0), chunks=False)
        run_case(4, npad + 1, COL, (0, 0), chunks=False)
    finally:
        pkg.set_tuning(spmmv_variant=variant)
    assert pkg.spmmv_ap_hp_tiles_path(*A, 4, npad, ROW) == (2, _vectors(4, L, size))
    # the refusals of the pair's list forms, under the new names
    X, Y = make_X(4, npad, COL), t.full((4 * npad,), NAN, dtype=dt, device="cuda")
    for fn, n_max in ((pkg.spmmv_ap_hp_tiles, n_tiles), (pkg.spmmv_ap_hp_chunks, n_chunks)):
        name = "uspmv_" + fn.__name__
        with pytest.raises(pkg.UspmvError, match=name + ": bad argument"):
            fn(*A, t.zeros(n_max + 1, dtype=t.int32, device="cuda"), X, Y, 4, npad)
        with pytest.raises(pkg.UspmvError, match=name + ": the parts must be"):
            fn(A[2], None, A[0], ids4, X, Y, 4, npad)
        with pytest.raises(pkg.UspmvError, match=name + ": ld="):
            fn(*A, ids4, X, Y, 4, npad - 1, COL)
        with pytest.raises(pkg.UspmvError, match=name + ": b=0"):
            fn(*A, ids4, X, Y, 0, npad)
        with pytest.raises(pkg.UspmvError, match=name + ": unknown layout 2"):
            fn(*A, ids4, X, Y, 4, npad, 2)
        fn(*A, ids4[:0], X, Y, 4, npad)                                  # an empty list: USPMV_OK, nothing launched
    t.cuda.synchronize()
    assert bool(t.isnan(Y).all())
    with pytest.raises(pkg.UspmvError, match="uspmv_spmmv_ap_hp_tiles_path: the parts must be"):
        pkg.spmmv_ap_hp_tiles_path(A[2], None, A[0], 4, npad)
    with pytest.raises(pkg.UspmvError, match="uspmv_spmmv_ap_hp_tiles_path: b=0"):
        pkg.spmmv_ap_hp_tiles_path(*A, 0, npad)
    # a sweep-planned split has no line plan to list tiles of: refused as on the single-vector list form
    S = [pkg.DeviceMatrix(s) if s is not None else None for s in structs]
    pkg.optimize_sweep_ap_hp(*S, *structs)
    assert S[0].plan_info()[0] == 2
    with pytest.raises(pkg.UspmvError, match="uspmv_spmv_ap_hp_tiles: the parts have no shared tile-local-column plan"):
        pkg.spmv_ap_hp_tiles(*S, ids4, X, Y)
    with pytest.raises(pkg.UspmvError, match="uspmv_spmmv_ap_hp_tiles: the parts have no shared tile-local-column plan"):
        pkg.spmmv_ap_hp_tiles(*S, ids4, X, Y, 4, npad)


@pytest.mark.parametrize("P,shape,C,sigma,tlc", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_block_step_loopback_bitexact(pkg, orc, torch_cuda, kind, P, shape, C, sigma, tlc):
    """Every rank of the four loopback cases of the single-vector test.  Y of the default form in original order is, per column, the
    oracle's whole-matrix composition; Y and the halo tail of X are those of b single-vector steps on the same object; "pad_split" 0,
    "overlap" 0 and "ba_synch" 1 give the same bits, comm_halos=False does not; uspmv_dist_spmmv_info counts the forms taken.
    padded_vec_size is n_local + max(n_rows_padded - n_local, n_halo): every rank but the first counts the padding column among its halo
    columns, so 576 + 1, 512 + 1, 256 + 1, 360 + 1 and 180 + 1 halo elements behind 6912, 2560 and 1620 local ones make an odd leading
    dimension there -- 8-byte pieces for double vectors, 4-byte pieces for float ones (found with the host halo planner,
    uspmv_halo_discover_ap_hp, on the blocks of the four cases; float columns 8 bytes off the grid are in the kernel test above).
    Asserted from the objects: in every case some rank's columns start off the 16-byte grid, and its tile lists report the staged kernel."""
    torch = torch_cuda
    first = (P, shape, tlc) == (2, (24, 24, 24), True)
    nl = _reference(pkg, orc, kind, shape, P, C, sigma)[1]
    want = [_reference(pkg, orc, kind, shape, P, C, sigma, xblock=c)[0] for c in _columns(nl, 8)]
    tdt = torch.float32 if kind == "sp_hp" else torch.float64
    off_grid = []                                                       # (rank, ld) of the objects with ld * itemsize % 16 != 0
    for rank in range(P):
        wsa, loc = _block(pkg, shape, P, rank)
        rows = slice(int(wsa[rank]), int(wsa[rank + 1]))
        for exchange in ("rccl", "peer") if first else ("rccl",):
            d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id() if exchange == "rccl" else None, comm_rank=0, comm_size=1,
                               tlc=tlc, ap_kind=kind, ap_threshold=T1, ap_threshold_2=T2, exchange=exchange)
            assert d.loopback and d.n_local == nl and d.n_halo > 0 and d.use_tiles == tlc and d.tdtype == tdt
            ld, npad = d.padded_vec_size, d.n_rows_padded
            size = 4 if kind == "sp_hp" else 8
            if tlc:
                for b in (2, 4, 8):                                     # the tile lists stage at whatever ld the halo made
                    path = d.spmmv_ap_hp_tiles_path(b, COL)
                    assert path[0] == 2 and path[1] >= 2 and path == d.spmmv_ap_hp_tiles_path(b, ROW), (kind, P, rank, b, path)
            if (ld * size) % 16 != 0:
                off_grid.append((rank, ld))
            single = []                                                 # (y, halo tail of x) of the single-vector step, per column
            for v, c in enumerate(_columns(nl, 8)):
                x = d.new_x(c); y = torch.full_like(d.new_y(), NAN)
                d.spmv(x, y); d.synchronize()
                assert _same(d.y_to_original_order(y)[:nl], want[v][rows]), (rank, exchange, v)
                single.append((y[:npad].clone(), x[d.n_local:d.n_local + d.n_halo].clone()))
            counts = d.spmmv_info()
            two, one = counts["two_part"], counts["one_part"]
            for b in (2, 4, 8):
                for layout, mode in ((COL, BULK), (COL, MULTI), (COL, SINGLE), (ROW, BULK)):
                    tag = (kind, P, rank, exchange, b, layout, mode)

                    def step(**kw):
                        X = d.new_X(_columns(nl, b), b, layout)
                        assert X.dtype == tdt
                        Y = torch.full((b * ld,), NAN, dtype=tdt, device="cuda")
                        d.spmmv_ap_hp(X, Y, b, layout, mode, **kw); d.synchronize()
                        return _view(Y, b, ld, layout), _halo_tail(d, X, b, layout)

                    Yv, halo = step()                                   # overlap, "pad_split" 1: the object's default
                    two += 1
                    assert not bool(torch.isnan(Yv[:, :npad]).any()) and bool(torch.isnan(Yv[:, npad:]).all()), tag
                    for v in range(b):
                        assert _same(d.y_to_original_order(Yv[v].contiguous())[:nl], want[v][rows]), (tag, v)
                        assert torch.equal(Yv[v, :npad], single[v][0]) and torch.equal(halo[v], single[v][1]), (tag, v)
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
            d.spmmv_ap_hp(x, y, 1); d.synchronize()
            assert torch.equal(y[:npad], single[0][0]) and d.spmmv_info()["two_part"] == two
            d.close()
    assert off_grid and {r for r, _ in off_grid} == set(range(1, P)), (kind, P, shape, off_grid)


@pytest.mark.parametrize("kind", ["dp_sp_hp", "sp_hp"])
def test_block_padding_guard(pkg, orc, torch_cuda, kind):
    """The slot of the padding column holds one value per vector, a double for ap[dp_sp_hp], a float for ap[sp_hp].  Positive in every
    column: no re-run.  Negative in the last column only: one re-run, none on a second step over the same X.  +Inf in one column only:
    NaN where the oracle has it, in that column only, the other columns those of the positive case, and a re-run every step.
    "pad_split" 0: never a re-run."""
    torch = torch_cuda
    P, shape, C, sigma, rank, b = 4, (16, 16, 40), 32, 512, 2, 4
    wsa, loc = _block(pkg, shape, P, rank)
    nl = int(wsa[1] - wsa[0])
    rows = slice(int(wsa[rank]), int(wsa[rank + 1]))
    tdt = torch.float32 if kind == "sp_hp" else torch.float64
    pos = _columns(nl, b)
    neg = [c.copy() for c in pos]; neg[b - 1][0] = -2.5
    inf = [c.copy() for c in pos]; inf[1][0] = np.inf
    cases = {"pos": pos, "neg": neg, "inf": inf}
    want = {tag: [_reference(pkg, orc, kind, shape, P, C, sigma, xblock=c)[0][rows] for c in cols] for tag, cols in cases.items()}
    assert np.isnan(want["inf"][1]).any()
    assert not any(np.isnan(w).any() for tag in ("pos", "neg") for w in want[tag]) and not any(np.isnan(want["inf"][v]).any() for v in (0, 2, 3))
    assert all(np.array_equal(want["inf"][v], want["pos"][v]) for v in (0, 2, 3))
    d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, ap_kind=kind, ap_threshold=T1, ap_threshold_2=T2)
    info = d.pad_info()
    assert info["pad_tiles"] > 0 and info["pad_col"] >= d.n_local and info["real_boundary_tiles"] > 0, info
    ld = d.padded_vec_size

    def run(tag, layout, steps=1):
        X = d.new_X(cases[tag], b, layout)
        Y = torch.full((b * ld,), NAN, dtype=tdt, device="cuda")
        for _ in range(steps):
            d.spmmv_ap_hp(X, Y, b, layout)
        d.synchronize()
        Yv = _view(Y, b, ld, layout)
        for v in range(b):
            assert _same(d.y_to_original_order(Yv[v].contiguous())[:nl], want[tag][v]), (kind, tag, layout, steps, v)
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
    mk = dict(comm_rank=0, comm_size=1)
    d = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), ap_kind="dp_sp_hp", ap_threshold=T1, ap_threshold_2=T2, **mk)
    pair = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), ap_threshold=1e-3, **mk)
    one = pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), **mk)
    X = torch.zeros(b * d.padded_vec_size, dtype=torch.float64, device="cuda")
    Y = torch.zeros_like(X)
    with pytest.raises(pkg.UspmvError, match="uspmv_dist_spmmv_ap_hp: a one-precision object.*uspmv_dist_spmmv") as e:
        one.spmmv_ap_hp(X, Y, b)
    assert e.value.status == 3                                # USPMV_ERR_UNSUPPORTED
    with pytest.raises(pkg.UspmvError, match=r"uspmv_dist_spmmv_ap_hp: an adaptive-precision ap\[dp_sp\] object.*uspmv_dist_spmmv_ap") as e:
        pair.spmmv_ap_hp(X, Y, b)
    assert e.value.status == 3
    for mode in (MULTI, SINGLE):
        with pytest.raises(pkg.UspmvError, match="uspmv_dist_spmmv_ap_hp: row-wise block vectors travel in one message per neighbour") as e:
            d.spmmv_ap_hp(X, Y, b, ROW, mode)
        assert e.value.status == 3
    with pytest.raises(pkg.UspmvError, match="uspmv_dist_spmmv_ap_hp: unknown mode 3"):
        d.spmmv_ap_hp(X, Y, b, COL, 3)
    with pytest.raises(pkg.UspmvError, match="uspmv_dist_spmmv_ap_hp: unknown layout 2"):
        d.spmmv_ap_hp(X, Y, b, 2)
    with pytest.raises(pkg.UspmvError, match="uspmv_dist_spmmv_ap_hp: b=0"):
        d.spmmv_ap_hp(X, Y, 0)
    for call in (d.spmmv, d.spmmv_ap):                        # what stays refused on such an object, now with a pointer to its own step
        with pytest.raises(pkg.UspmvError, match=r"ap\[dp_sp_hp\].*uspmv_dist_spmmv_ap_hp") as e:
            call(X, Y, b)
        assert e.value.status == 3
    for key, value in (("fused_step", 1), ("block_plan", 8), ("autotune_all", 1)):
        with pytest.raises(pkg.UspmvError, match=r"ap\[dp_sp_hp\]") as e:
            d.set_option(key, value)
        assert e.value.status == 3
    assert d.spmmv_info()["two_part"] == 0 and d.spmmv_info()["one_part"] == 0
    d.close(); pair.close(); one.close()


def _ap_hp_block_worker(rank, world, q, job, case):
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.setdefault("OMP_NUM_THREADS", "4"); os.environ.setdefault("OMP_WAIT_POLICY", "passive")   # (several rank processes share the box's cores)
        import torch
        import __graft_entry__ as ge
        pkg = ge.load_package()
        from ultimate_spmv_amd import binding as B
        from oracle import oracle as orc
        torch.cuda.set_device(0)
        name, Cc, sg, method, t1, t2, b, kinds = case
        tot = pkg.read_mtx(mtx_path(name))
        wsa = pkg.seg_work_sharing_arr(tot, method, world)
        xg = make_x(tot.n_rows)
        rows = slice(int(wsa[rank]), int(wsa[rank + 1]))
        loc = B.seg_local_coo(tot, wsa, rank)
        nl = int(wsa[rank + 1] - wsa[rank])
        for kind in kinds:
            hc = pkg.HostComm(job + kind, rank, world, timeout_s=120)
            want = [whole_matrix_ap_hp_reference(pkg, orc, tot, kind, Cc, sg, t1, t2, xg * _scale(v))[0][rows] for v in range(b)]
            d = pkg.DistNative(loc, wsa, Cc, sg, rank, world, hostcomm=hc, host_exchange=True, ap_kind=kind, ap_threshold=t1, ap_threshold_2=t2)
            assert d.n_local == nl and not d.loopback and d.scs.nnz > 0 and d.scs_hp.nnz > 0 and (kind != "dp_sp_hp" or d.scs_mid.nnz > 0)
            ld = d.padded_vec_size
            for layout, mode in ((COL, MULTI), (ROW, BULK)):
                for overlap in (1, 0):
                    d.set_option("overlap", overlap)
                    X = d.new_X([xg[rows] * _scale(v) for v in range(b)], b, layout)
                    Y = torch.full((b * ld,), NAN, dtype=d.tdtype, device="cuda")
                    d.spmmv_ap_hp(X, Y, b, layout, mode); d.synchronize()
                    Yv = _view(Y, b, ld, layout)
                    for v in range(b):
                        assert _same(d.y_to_original_order(Yv[v].contiguous())[:nl], want[v]), (kind, layout, mode, overlap, v)
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
    exchange; b = 4, column-wise multivec and row-wise bulkvec, for ap[dp_sp_hp] (double vectors) and ap[sp_hp] (float), every row of
    every rank against the oracle's whole-matrix composition.  Every child is bounded by a time limit; the first failure ends the run and
    nothing is tried again."""
    world, case = 3, ("bcsstk13", 32, 512, "seg-nnz", 1.0, 0.01, 4, ("dp_sp_hp", "sp_hp"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    job = f"aphpb{os.getpid()}_{time.monotonic_ns()}"
    procs = [ctx.Process(target=_ap_hp_block_worker, args=(r, world, q, job, case)) for r in range(world)]
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
