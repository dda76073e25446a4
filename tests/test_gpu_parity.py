"""Parity of the HIP path (through the C ABI of libuspmv.so) with the oracle and with the golden
vectors of the genuine reference.  Integer work: bit-exact.  Floating point: the lane-per-row
kernels are bit-exact (same FMA chain as the reference's CPU kernels); kernels that split a row
over lanes (two-lane SELL variant, CRS) are held to
    |y - y_ref| <= tol * sum_j |a_ij x_j|,   tol = 1e-13 (dp) / 1e-5 (sp)
the reference's own max_rel_error constants (code/utilities.hpp:35-47)."""
import hashlib
import json
import os
import time

import numpy as np
import pytest

from conftest import ADV_CS, GOLDEN, block_x, golden, make_x, mtx_path

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-13, "f32": 1e-5}
FULL = ["FDM-2d-16", "impcol_e", "matrix1", "myBigMat", "mySymmMat", "matrix_band_klein", "bcsstk13"]


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert pkg.device_count() >= 1
    torch.cuda.set_device(0)
    yield torch
    pkg.set_tuning(unroll=8, nontemporal=1, xcd_remap=256, block=256, spmv_variant=0, csr_lanes=0, tail_batch=0, tlc=1)


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a)).cuda()


def _prep(pkg, coo, Cc, sg, dtype, x_orig):
    """Reference flow on the host (convert, permute cols, permute x) -> (scs, arrays, x_perm padded)."""
    s = pkg.convert_to_scs(coo, Cc, sg, dtype)
    a = s.arrays()
    pkg.permute_scs_cols(s, a["old_to_new_idx"])
    a = s.arrays()
    xp = np.zeros(s.n_rows_padded, s.np_dtype)
    xp[:s.n_rows] = pkg.apply_permutation(x_orig.astype(s.np_dtype), a["new_to_old_idx"])
    return s, a, xp


@pytest.mark.parametrize("name", FULL)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_spmv_golden_bitexact_all_variants(pkg, torch_cuda, name, dt):
    t = torch_cuda
    g = golden(f"scs_{name}.npz")
    m = pkg.read_mtx(mtx_path(name))
    s = pkg.convert_to_scs(m, int(g["C"]), int(g["sigma"]), pkg.F64 if dt == "f64" else pkg.F32)
    pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"])
    A = pkg.DeviceMatrix(s)
    x = _dev(t, g[f"{dt}_x_perm"])
    for variant in (0, 2):          # lane-per-row kernels: plain and software-pipelined, both bit-exact
        for unroll in (1, 2, 4, 8):
            for nt in (0, 1):
                for xcd in (0, 1, 3):
                    for block in (64, 256, 1024):
                        for tail in (0, 1):
                            pkg.set_tuning(unroll=unroll, nontemporal=nt, xcd_remap=xcd, block=block, spmv_variant=variant,
                                           tail_batch=tail)
                            y = t.full((s.n_rows_padded,), -7.0, dtype=x.dtype, device="cuda")
                            pkg.spmv(A, x, y)
                            assert np.array_equal(y.cpu().numpy(), g[f"{dt}_y_perm"]), (variant, unroll, nt, xcd, block, tail)
    pkg.set_tuning(spmv_variant=0, tail_batch=0)
    pkg.set_tuning(unroll=8, nontemporal=1, xcd_remap=256, block=256)
    # raw-array entry point with the interface.hpp argument list
    y = t.zeros(s.n_rows_padded, dtype=x.dtype, device="cuda")
    pkg.uspmv_scs_gpu(s.C, s.n_chunks, A.chunk_ptrs, A.chunk_lengths, A.col_idxs, A.values, x, y)
    assert np.array_equal(y.cpu().numpy(), g[f"{dt}_y_perm"])
    yo = pkg.apply_permutation(y.cpu().numpy(), g[f"{dt}_old_to_new"])
    assert np.array_equal(yo, g[f"{dt}_y_orig"])


def test_spmv_grid_vs_oracle_and_reference_hashes(pkg, orc, torch_cuda):
    """C x sigma grid of scripts/validate_master.sh:16-23 (+ C = 1, 128): bit-exact vs the oracle on
    the same arrays and vs the sha1 of the reference's y."""
    t = torch_cuda
    grid = json.load(open(os.path.join(GOLDEN, "scs_grid_sha1.json")))
    mats = {}
    n = 0
    for key, ent in grid.items():
        name, Cc, sg = key.split("|")
        Cc, sg = int(Cc), int(sg)
        if name == "bcsstk13" and sg not in (1, 64, 512):
            continue
        m = mats.setdefault(name, pkg.read_mtx(mtx_path(name)))
        x0 = make_x(m.n_rows)
        for dt, code in (("f64", pkg.F64), ("f32", pkg.F32)):
            s, a, xp = _prep(pkg, m, Cc, sg, code, x0)
            A = pkg.DeviceMatrix(s)
            y_or = orc.spmv_scs(Cc, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
            for variant in (0, 2):
                pkg.set_tuning(spmv_variant=variant)
                y = t.full((s.n_rows_padded,), 3.0, dtype=A.torch_dtype, device="cuda")
                pkg.spmv(A, _dev(t, xp), y)
                yh = y.cpu().numpy()
                assert np.array_equal(yh, y_or), (key, dt, variant)
                assert sha(yh) == ent[dt]["y_perm"], (key, dt, variant)
            pkg.set_tuning(spmv_variant=0)
            n += 1
    assert n > 300


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_spmv_two_lane_variant_tolerance(pkg, orc, torch_cuda, dt):
    t = torch_cuda
    for name in ("bcsstk13", "impcol_e"):
        g = golden(f"scs_{name}.npz")
        m = pkg.read_mtx(mtx_path(name))
        s, a, xp = _prep(pkg, m, 32, 512, pkg.F64 if dt == "f64" else pkg.F32, g["x"])
        A = pkg.DeviceMatrix(s)
        y = t.zeros(s.n_rows_padded, dtype=A.torch_dtype, device="cuda")
        pkg.set_tuning(spmv_variant=1)
        pkg.spmv(A, _dev(t, xp), y)
        pkg.set_tuning(spmv_variant=0)
        bound = orc.spmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], np.abs(a["values"]),
                             np.abs(xp)).astype(np.float64)
        err = np.abs(y.cpu().numpy().astype(np.float64) - g[f"{dt}_y_perm"].astype(np.float64))
        assert np.all(err <= TOL[dt] * bound + 1e-300)


@pytest.mark.parametrize("name", ["FDM-2d-16", "impcol_e", "matrix1", "bcsstk13"])
def test_crs(pkg, orc, torch_cuda, name):
    t = torch_cuda
    c = golden("csr.npz")
    m = pkg.read_mtx(mtx_path(name))
    x0 = make_x(m.n_rows)
    for dt, code in (("f64", pkg.F64), ("f32", pkg.F32)):
        s, a, xp = _prep(pkg, m, 1, 1, code, x0)
        assert np.array_equal(a["chunk_ptrs"], c[f"{name}_{dt}_row_ptrs"])
        bound = orc.spmv_csr(s.n_rows, a["chunk_ptrs"], a["col_idxs"], np.abs(a["values"]), np.abs(xp)).astype(np.float64)
        ref = c[f"{name}_{dt}_y"].astype(np.float64)
        x = _dev(t, xp)
        A = pkg.DeviceMatrix(s, crs=True)
        for lanes in (0, 1, 2, 8, 64):
            pkg.set_tuning(csr_lanes=lanes)
            y = t.zeros(s.n_rows, dtype=A.torch_dtype, device="cuda")
            pkg.spmv(A, x, y)
            assert np.all(np.abs(y.cpu().numpy().astype(np.float64) - ref) <= TOL[dt] * bound + 1e-300), (dt, lanes)
        pkg.set_tuning(csr_lanes=0)
        y = t.zeros(s.n_rows, dtype=A.torch_dtype, device="cuda")
        pkg.uspmv_csr_gpu(s.n_rows, A.chunk_ptrs, A.col_idxs, A.values, x, y)
        assert np.all(np.abs(y.cpu().numpy().astype(np.float64) - ref) <= TOL[dt] * bound + 1e-300)
        # the generic SELL kernel at C = 1 is the sequential chain: bit-exact with the oracle
        y_seq = orc.spmv_csr(s.n_rows, a["chunk_ptrs"], a["col_idxs"], a["values"], xp)
        A1 = pkg.DeviceMatrix(s)
        pkg.spmv(A1, x, y)
        assert np.array_equal(y.cpu().numpy(), y_seq)
        # optimised crs handle: internally SELL-32-1 (+ tile-local columns), still the sequential chain
        A2 = pkg.DeviceMatrix(s, crs=True, tlc=True)
        y2 = t.full((s.n_rows,), 4.0, dtype=A.torch_dtype, device="cuda")      # exactly n_rows elements: no overrun allowed
        pkg.spmv(A2, x, y2)
        # (bit-exact when the re-chunked struct is used; ragged matrices whose padding would grow > 25 % keep the
        #  multi-lane CRS kernel, which is held to the CRS tolerance)
        assert np.all(np.abs(y2.cpu().numpy().astype(np.float64) - y_seq.astype(np.float64)) <= TOL[dt] * bound + 1e-300)
        if name in ("FDM-2d-16",):
            assert np.array_equal(y2.cpu().numpy(), y_seq)


@pytest.mark.parametrize("name", ["FDM-2d-16", "impcol_e", "bcsstk13"])
def test_spmmv_golden_bitexact(pkg, orc, torch_cuda, name):
    t = torch_cuda
    g = golden(f"scs_{name}.npz")
    sp = golden("spmmv.npz")
    m = pkg.read_mtx(mtx_path(name))
    for dt, code in (("f64", pkg.F64), ("f32", pkg.F32)):
        s, a, xp = _prep(pkg, m, int(g["C"]), int(g["sigma"]), code, g["x"])
        A = pkg.DeviceMatrix(s)
        ld = s.n_rows_padded
        for variant, pf in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 1)): # 0: auto, 1: generic kernel, 2: row-major + transposing X phase, 3: row-major lane per row (pf: with prefetch)
            pkg.set_tuning(spmmv_variant=variant, spmmv_prefetch=pf)
            for b in (2, 8):
                for rowwise in (0, 1):
                    X = block_x(xp, ld, b, ld, rowwise)
                    Y = t.full((b * ld,), -3.0, dtype=A.torch_dtype, device="cuda")
                    pkg.spmmv(A, _dev(t, X), Y, b, ld, pkg.ROWWISE if rowwise else pkg.COLWISE)
                    assert np.array_equal(Y.cpu().numpy(), sp[f"{name}_{dt}_b{b}_{'row' if rowwise else 'col'}_Y"]), (dt, b, rowwise, variant)
        pkg.set_tuning(spmmv_variant=0, spmmv_prefetch=0)
        for b in (1, 3, 4, 5, 13, 16):     # widths without a golden: vs the oracle, colwise ld > n_rows_padded too
            for rowwise in (0, 1):
                ld2 = ld + 7
                X = block_x(xp, ld, b, ld2, rowwise)
                Y = t.zeros(b * ld2, dtype=A.torch_dtype, device="cuda")
                pkg.spmmv(A, _dev(t, X), Y, b, ld2, pkg.ROWWISE if rowwise else pkg.COLWISE)
                Yo = orc.spmmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, b, ld2, rowwise)
                got = Y.cpu().numpy()
                if rowwise:
                    assert np.array_equal(got[:ld * b], Yo[:ld * b])
                else:
                    assert np.array_equal(got, Yo)


def test_convert_to_scs_device_bitexact(pkg, torch_cuda):
    """uspmv_convert_to_scs_device = uspmv_convert_to_scs (+ permute_scs_cols) + upload, bit for bit: C x sigma grid,
    dp / sp, fixed permutation, empty rows; and the SpMV on the device-built struct matches the host-built one."""
    t = torch_cuda
    rng = np.random.default_rng(3)
    n = 300                                               # rows 0, 7, 14, ... and the last 40 rows are empty
    I = np.sort(rng.integers(0, n - 40, 3000)); I = I[I % 7 != 0]
    ragged = pkg.Coo.from_arrays(n, n, I, rng.integers(0, n, I.size), rng.standard_normal(I.size))
    for name in ("FDM-2d-16", "impcol_e", "bcsstk13", "matrix1", "matrix_band_klein", ragged):
        m = pkg.read_mtx(mtx_path(name)) if isinstance(name, str) else name
        for C, sigma in ((1, 1), (4, 4), (16, 512), (32, 512), (32, 1), (64, 128), (128, 256), (5, 7)):
            for code in (pkg.F64, pkg.F32):
                for permute in (True, False):
                    s = pkg.convert_to_scs(m, C, sigma, code)
                    if permute:
                        pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"])
                    a = s.arrays()
                    lay, A = pkg.convert_to_scs_device(m, C, sigma, code, permute_cols=permute)
                    assert (lay.n_chunks, lay.n_elements, lay.n_rows_padded, lay.nnz) == (s.n_chunks, s.n_elements, s.n_rows_padded, s.nnz)
                    la = lay.arrays()
                    assert la["col_idxs"] is None and la["values"] is None
                    for k in ("chunk_ptrs", "chunk_lengths", "old_to_new_idx", "new_to_old_idx"):
                        assert np.array_equal(la[k], a[k]), (name, C, sigma, k)
                    d = pkg.dmat_download(A)
                    for k in ("chunk_ptrs", "chunk_lengths", "col_idxs", "values"):
                        assert np.array_equal(d[k], a[k]), (name, C, sigma, code, permute, k)
        # fixed permutation (a valid one: the struct's own sort order), quirk included
        s0 = pkg.convert_to_scs(m, 8, 32, pkg.F64)
        fp = s0.arrays()["old_to_new_idx"].copy()
        s1 = pkg.convert_to_scs(m, 8, 32, pkg.F64, fixed_permutation=fp)
        lay, A = pkg.convert_to_scs_device(m, 8, 32, pkg.F64, fixed_permutation=fp, permute_cols=False)
        d = pkg.dmat_download(A)
        for k in ("chunk_ptrs", "chunk_lengths", "col_idxs", "values"):
            assert np.array_equal(d[k], s1.arrays()[k]), (name, "fixed", k)
        assert np.array_equal(lay.arrays()["old_to_new_idx"], s1.arrays()["old_to_new_idx"])
    # SpMV on the device-built struct; layout-only structs are refused where host entries are needed
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    lay, A = pkg.convert_to_scs_device(m, 32, 512, pkg.F64)
    s, a, xp = _prep(pkg, m, 32, 512, pkg.F64, make_x(m.n_rows))
    A0 = pkg.DeviceMatrix(s)
    x = _dev(t, xp)
    y = t.zeros(s.n_rows_padded, dtype=t.float64, device="cuda"); y0 = t.zeros_like(y)
    pkg.spmv(A, x, y); pkg.spmv(A0, x, y0)
    assert t.equal(y, y0)
    with pytest.raises(pkg.UspmvError):
        A.optimize(lay)
    with pytest.raises(pkg.UspmvError):
        pkg.permute_scs_cols(lay, la["old_to_new_idx"])
    unsorted = pkg.Coo.from_arrays(3, 3, [2, 0, 1], [0, 1, 2], [1.0, 2.0, 3.0])
    with pytest.raises(pkg.UspmvError):
        pkg.convert_to_scs_device(unsorted, 2, 2)


def C_tile_rows(pkg, A):
    import ctypes
    from ultimate_spmv_amd import binding
    tr = ctypes.c_int()
    assert binding.lib().uspmv_dmat_tile_rows(A.h, ctypes.byref(tr)) == 0
    return tr.value


def test_tile_rows_follow_the_lines_a_tile_needs(pkg, orc, torch_cuda):
    """uspmv_dmat_optimize[_device] with tlc_tile_rows 0: 256-row tiles, unless the largest of them needs more than 250 x lines and
    1024-row (or 512-row) tiles still stage >= 99 % of the tiles (csrc/tlc_planner.hip tile_rows_grow).  Host and device planners take the
    same decision and build the same arrays; y has the reference's bits whatever the tile size; tlc_auto_tile 0 keeps 256."""
    t = torch_cuda
    for gen, want in ((lambda: pkg.gen_banded_random(40000, 30, 2000), 1024),      # ~270 lines per 256-row tile, ~320 per 1024-row tile
                      (lambda: pkg.gen_stencil27(40, 40, 24), 256)):               # a stencil: few lines, stays at 256
        m = gen()
        s, a, xp = _prep(pkg, m, 32, 512, pkg.F64, make_x(m.n_rows))
        yo = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
        Ah = pkg.DeviceMatrix(s); Ah.optimize(s)
        Ad = pkg.DeviceMatrix(s); Ad.optimize_device()
        assert C_tile_rows(pkg, Ah) == C_tile_rows(pkg, Ad) == want, (C_tile_rows(pkg, Ah), C_tile_rows(pkg, Ad), want)
        assert Ah.plan_info() == Ad.plan_info() and Ah.plan_info()[0] == 1
        ph, pd = Ah.plan_download(), Ad.plan_download()
        for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16"):
            assert np.array_equal(ph[k], pd[k]), (want, k)
        for A in (Ah, Ad):
            y = t.full((s.n_rows_padded,), 3.0, dtype=t.float64, device="cuda")
            pkg.spmv(A, _dev(t, xp), y)
            assert np.array_equal(y.cpu().numpy(), yo), want
        pkg.set_tuning(tlc_auto_tile=0)
        try:
            A0 = pkg.DeviceMatrix(s); A0.optimize(s)
            A1 = pkg.DeviceMatrix(s); A1.optimize_device()
        finally:
            pkg.set_tuning(tlc_auto_tile=1)
        assert C_tile_rows(pkg, A0) == C_tile_rows(pkg, A1) == 256
        if want != 256:
            assert ph["max_lines_used"] <= 512 and A0.plan_download()["max_lines_used"] > 250
        y = t.full((s.n_rows_padded,), 3.0, dtype=t.float64, device="cuda")
        pkg.spmv(A0, _dev(t, xp), y)
        assert np.array_equal(y.cpu().numpy(), yo)


def test_device_plan_builder_far_apart_column_clusters(pkg, orc, torch_cuda):
    """Tiles whose columns form clusters millions of columns apart -- a KKT matrix large enough that states and multipliers lie more than
    2^20 columns from each other (uspmv_gen_kkt N = 104), with the padding column as a third cluster: the device builder's bitmap works on
    up to 16 windows of 4 096 lines wherever they lie (csrc/plan_kernels.hip), stages what the host planner stages, and builds the same
    arrays.  (Before round 3 only clusters at either end of a tile's range were representable: the middle one left such tiles unstaged.)"""
    t = torch_cuda
    m = pkg.gen_kkt(104)
    assert m.n_rows > (1 << 21)
    pkg.set_tuning(tlc_measure_tile=0)                         # (compare the planners at the rule's tile size, not at a measured one)
    try:
        s, a, xp = _prep(pkg, m, 32, 512, pkg.F64, make_x(m.n_rows))
        span = a["col_idxs"].reshape(-1)
        assert int(span.max()) - int(span.min()) > (1 << 20)
        Ah = pkg.DeviceMatrix(s); Ah.optimize(s)
        Ad = pkg.DeviceMatrix(s); Ad.optimize_device()
    finally:
        pkg.set_tuning(tlc_measure_tile=1)
    assert Ah.plan_info()[0] == 1 and Ah.tlc_staged * 100 >= Ah.tlc_tiles * 99
    assert (Ad.tlc_tiles, Ad.tlc_staged) == (Ah.tlc_tiles, Ah.tlc_staged) and C_tile_rows(pkg, Ah) == C_tile_rows(pkg, Ad)
    ph, pd = Ah.plan_download(), Ad.plan_download()
    for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16"):
        assert np.array_equal(ph[k], pd[k]), k
    yo = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
    y = t.full((s.n_rows_padded,), 3.0, dtype=t.float64, device="cuda")
    pkg.spmv(Ad, _dev(t, xp), y)
    assert np.array_equal(y.cpu().numpy(), yo)


def test_measured_tile_rows_on_a_large_struct(pkg, orc, torch_cuda):
    """Structs of >= 2^20 padded rows: the rows per tile are measured (plans for 256 / 512 / 1024 rows built on the device, the kernel timed,
    a larger tile kept when > 3 % ahead; tlc_planner.hip measured_tile_rows).  Whatever wins, the host and the device planner of the same
    matrix agree (the choice is remembered per shape), the plans are identical, y has the reference's bits; "tlc_measure_tile" 0 gives the
    rule-based 256 rows."""
    t = torch_cuda
    m = pkg.gen_stencil27(104, 104, 104)                      # 1 124 864 rows
    s, a, xp = _prep(pkg, m, 32, 512, pkg.F64, make_x(m.n_rows))
    assert s.n_rows_padded >= 1 << 20
    yo = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
    Ah = pkg.DeviceMatrix(s); Ah.optimize(s)
    Ad = pkg.DeviceMatrix(s); Ad.optimize_device()
    assert C_tile_rows(pkg, Ah) == C_tile_rows(pkg, Ad) and C_tile_rows(pkg, Ah) in (256, 512, 1024)
    ph, pd = Ah.plan_download(), Ad.plan_download()
    for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16"):
        assert np.array_equal(ph[k], pd[k]), k
    for A in (Ah, Ad):
        y = t.full((s.n_rows_padded,), 3.0, dtype=t.float64, device="cuda")
        pkg.spmv(A, _dev(t, xp), y)
        assert np.array_equal(y.cpu().numpy(), yo)
    pkg.set_tuning(tlc_measure_tile=0)
    try:
        A0 = pkg.DeviceMatrix(s); A0.optimize_device()
    finally:
        pkg.set_tuning(tlc_measure_tile=1)
    assert C_tile_rows(pkg, A0) == 256
    y = t.full((s.n_rows_padded,), 3.0, dtype=t.float64, device="cuda")
    pkg.spmv(A0, _dev(t, xp), y)
    assert np.array_equal(y.cpu().numpy(), yo)


def test_device_plan_builder_matches_host_planner(pkg, orc, torch_cuda):
    """uspmv_dmat_optimize_device: the plan built on the GPU from the handle's arrays equals the host planner's
    (line lists, 16-bit indices) and the SpMV on it is bit-exact; also on handles made by convert_to_scs_device and
    with a line budget that leaves some tiles unstaged."""
    t = torch_cuda
    for name, C, sigma, max_lines in (("bcsstk13", 32, 512, 0), ("bcsstk13", 32, 512, 40), ("FDM-2d-16", 16, 512, 0),
                                      ("impcol_e", 64, 64, 0), ("bcsstk13", 128, 128, 0), ("matrix1", 256, 256, 0),
                                      ("bcsstk13", 8, 1, 0)):
        m = pkg.read_mtx(mtx_path(name))
        for code in (pkg.F64, pkg.F32):
            s, a, xp = _prep(pkg, m, C, sigma, code, make_x(m.n_rows))
            pkg.set_tuning(rechunk=0)                         # compare like with like: no internal C = 32 re-chunking
            Ah = pkg.DeviceMatrix(s); Ah.optimize(s, max_lines)
            Ad = pkg.DeviceMatrix(s); Ad.optimize_device(max_lines)
            pkg.set_tuning(rechunk=1)
            if C < 32:                                        # narrow chunks: the device builder re-chunks to C = 32 like the host one
                Ar = pkg.DeviceMatrix(s); Ar.optimize_device(max_lines)
                Ahr = pkg.DeviceMatrix(s); Ahr.optimize(s, max_lines)
                assert Ar.plan_info() == Ahr.plan_info() and Ar.plan_info()[0] == 1
                yr = t.full((s.n_rows_padded,), 3.0, dtype=Ar.torch_dtype, device="cuda")
                pkg.spmv(Ar, _dev(t, xp), yr)
                assert np.array_equal(yr.cpu().numpy(), orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)), (name, C, code, "device re-chunk")
            assert (Ad.tlc_tiles, Ad.tlc_staged) == (Ah.tlc_tiles, Ah.tlc_staged), (name, C, code)
            ph, pd = Ah.plan_download(), Ad.plan_download()
            assert (ph is None) == (pd is None)
            if ph is not None:
                for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16"):
                    assert np.array_equal(ph[k], pd[k]), (name, C, code, k)
                assert ph["max_lines_used"] == pd["max_lines_used"]
            yo = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
            y = t.full((s.n_rows_padded,), 3.0, dtype=Ad.torch_dtype, device="cuda")
            pkg.spmv(Ad, _dev(t, xp), y)
            assert np.array_equal(y.cpu().numpy(), yo), (name, C, code)
    # tiles of 512 / 1024 rows (a lane of the builder owns 2 / 4 rows), and the shared plan of an ap[dp_sp] pair (512 rows by default)
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    for C, sigma in ((32, 512), (64, 64), (16, 16)):
        s, a, xp = _prep(pkg, m, C, sigma, pkg.F64, make_x(m.n_rows))
        yo = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
        for tile_rows in (512, 1024):
            pkg.set_tuning(tlc_tile_rows=tile_rows, rechunk=0)
            Ah = pkg.DeviceMatrix(s); Ah.optimize(s)
            Ad = pkg.DeviceMatrix(s); Ad.optimize_device()
            pkg.set_tuning(tlc_tile_rows=0, rechunk=1)
            assert Ah.tile_rows == tile_rows and Ad.tile_rows == tile_rows
            assert (Ad.tlc_tiles, Ad.tlc_staged) == (Ah.tlc_tiles, Ah.tlc_staged), (C, tile_rows)
            ph, pd = Ah.plan_download(), Ad.plan_download()
            for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16"):
                assert np.array_equal(ph[k], pd[k]), (C, tile_rows, k)
            y = t.full((s.n_rows_padded,), 3.0, dtype=t.float64, device="cuda")
            pkg.spmv(Ad, _dev(t, xp), y)
            assert np.array_equal(y.cpu().numpy(), yo), (C, tile_rows)
    dp, sp = pkg.partition_precisions(m, 1e-1)
    assert dp.nnz > 0 and sp.nnz > 0
    ds = pkg.convert_to_scs(dp, 32, 512, pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, 32, 512, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
    Ahd, Ahs = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
    Add, Ads = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
    pkg.optimize_ap(Ahd, Ahs, ds, ss)
    pkg.optimize_device_ap(Add, Ads)
    for Ah, Ad in ((Ahd, Add), (Ahs, Ads)):
        th, td = C_tile_rows(pkg, Ah), C_tile_rows(pkg, Ad)
        assert th == td == 512
    ph, pd = Ahd.plan_download(), Add.plan_download()
    for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16"):
        assert np.array_equal(ph[k], pd[k]), ("ap pair", k)
    m = pkg.read_mtx(mtx_path("bcsstk13"))                    # device-converted handle, no host entries at all
    lay, A = pkg.convert_to_scs_device(m, 32, 512, pkg.F64)
    nt, ns = A.optimize_device()
    assert nt > 0 and ns == nt
    s, a, xp = _prep(pkg, m, 32, 512, pkg.F64, make_x(m.n_rows))
    y = t.zeros(s.n_rows_padded, dtype=t.float64, device="cuda")
    pkg.spmv(A, _dev(t, xp), y)
    assert np.array_equal(y.cpu().numpy(), orc.spmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp))


def test_raw_entry_point_plan_cache(pkg, orc, torch_cuda):
    """uspmv_scs_gpu_f64/f32 with the opt-in plan cache ("raw_plan_cache"): same bits as without, for repeated calls,
    several matrices behind different pointers, and after uspmv_raw_plan_cache_clear()."""
    t = torch_cuda
    mats = []
    for name, C, sigma, code in (("bcsstk13", 32, 512, pkg.F64), ("impcol_e", 64, 64, pkg.F32), ("FDM-2d-16", 5, 7, pkg.F64)):
        m = pkg.read_mtx(mtx_path(name))
        s, a, xp = _prep(pkg, m, C, sigma, code, make_x(m.n_rows))
        A = pkg.DeviceMatrix(s)          # torch-owned device arrays = what a host application would pass
        yo = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
        mats.append((s, A, _dev(t, xp), yo))
    try:
        for cache in (1, 0, 1):
            pkg.set_tuning(raw_plan_cache=cache)
            for rep in range(3):
                for s, A, x, yo in mats:
                    y = t.full((s.n_rows_padded,), -5.0, dtype=A.torch_dtype, device="cuda")
                    pkg.uspmv_scs_gpu(s.C, s.n_chunks, A.chunk_ptrs, A.chunk_lengths, A.col_idxs, A.values, x, y)
                    assert np.array_equal(y.cpu().numpy(), yo), (cache, rep, s.C)
            pkg.lib().uspmv_raw_plan_cache_clear()
    finally:
        pkg.set_tuning(raw_plan_cache=0)
        pkg.lib().uspmv_raw_plan_cache_clear()


def test_special_values_propagate_like_the_reference(pkg, orc, torch_cuda):
    """Inf / NaN / signed zeros in x (also at the column the padding entries point to): the kernels multiply the very
    same (value, x) pairs in the same order as the reference, so the non-finite results agree too: NaN in the same
    places (its sign / payload is the hardware's: x86 makes 0*inf the negative "indefinite" NaN, gfx950 the positive
    canonical one), everything else -- infinities, signed zeros -- bit for bit.  Gather kernel, tile-local-column
    kernel, SpMMV with and without the block plan."""
    t = torch_cuda

    def same_bits(got, ref, it):
        return np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~np.isnan(ref)].view(it), ref[~np.isnan(ref)].view(it))

    m = pkg.read_mtx(mtx_path("bcsstk13"))
    for code, it in ((pkg.F64, np.int64), (pkg.F32, np.int32)):
        s, a, xp = _prep(pkg, m, 32, 512, code, make_x(m.n_rows))
        xp = xp.copy()
        pad_col = int(a["col_idxs"][a["values"] == 0][0]) if np.any(a["values"] == 0) else 0
        xp[pad_col] = np.inf                      # 0 * inf = NaN wherever a padding entry sits
        xp[5] = -np.inf; xp[17] = np.nan; xp[40:60] = -0.0; xp[100] = np.finfo(xp.dtype).max; xp[101] = np.finfo(xp.dtype).tiny
        yo = orc.spmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
        assert np.isnan(yo).any() and np.isfinite(yo).any()
        x = _dev(t, xp)
        for tlc in (False, True):
            A = pkg.DeviceMatrix(s, tlc=tlc)
            y = t.zeros(s.n_rows_padded, dtype=A.torch_dtype, device="cuda")
            pkg.spmv(A, x, y)
            assert same_bits(y.cpu().numpy(), yo, it), (code, tlc)
        b, ld = 4, s.n_rows_padded
        with np.errstate(over="ignore"):
            X = np.concatenate([xp * xp.dtype.type(1 + v) for v in range(b)])
        Yo = orc.spmmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, b, ld, 0)
        for plan in (0, b):
            A = pkg.DeviceMatrix(s, block_tlc=plan)
            pkg.set_tuning(spmmv_variant=4 if plan else 0)
            Y = t.zeros(b * ld, dtype=A.torch_dtype, device="cuda")
            pkg.spmmv(A, _dev(t, X), Y, b, ld, pkg.COLWISE)
            pkg.set_tuning(spmmv_variant=0)
            assert same_bits(Y.cpu().numpy(), Yo, it), (code, "spmmv", plan)


def test_spmmv_block_plan_bitexact(pkg, orc, torch_cuda):
    """uspmv_dmat_optimize_block: LDS-staged X rows + 16-bit local indices give the same bits as the gather
    kernels and the oracle (block_spmv_omp_scs_general, code/kernels.hpp:306-398); staged and unstaged tiles,
    ragged chunk lengths inside a wave."""
    t = torch_cuda
    seen_partial = seen_full = False
    for name, C, sigma, lds_kb, tile64 in (("FDM-2d-16", 16, 512, 0, 0), ("bcsstk13", 32, 512, 0, 0), ("bcsstk13", 4, 1, 0, 0),
                                           ("impcol_e", 64, 64, 0, 0), ("matrix1", 1, 1, 0, 0), ("bcsstk13", 128, 128, 0, 0),
                                           ("bcsstk13", 32, 1, 8, 0), ("bcsstk13", 64, 512, 12, 0), ("bcsstk13", 32, 512, 0, 64),
                                           ("impcol_e", 32, 1, 0, 0)):
        pkg.set_tuning(spmmv_lds_kb=lds_kb, spmmv_tile_rows=tile64, spmmv_list_plan=1)     # (apply to the plans built below; list plan: the older kernels too)
        m = pkg.read_mtx(mtx_path(name))
        for code in (pkg.F64, pkg.F32):
            s, a, xp = _prep(pkg, m, C, sigma, code, make_x(m.n_rows))
            ld = s.n_rows_padded + 5
            A0 = pkg.DeviceMatrix(s)
            for b in (2, 4, 8, 16, 3):
                A = pkg.DeviceMatrix(s, block_tlc=b)
                row_bytes = b * (8 if code == pkg.F64 else 4)
                if C not in (32, 64) or row_bytes not in (16, 32, 64, 128):
                    assert A.block_staged == 0
                else:
                    tr = 32 if (C == 32 and row_bytes >= 128 and not tile64) else 64
                    assert A.block_tiles == (s.n_rows_padded + tr - 1) // tr and 0 <= A.block_staged <= A.block_tiles
                    seen_partial |= 0 < A.block_staged < A.block_tiles
                    seen_full |= A.block_staged == A.block_tiles
                for rowwise in (0, 1):
                    X = block_x(xp, s.n_rows_padded, b, ld, rowwise)
                    lay = pkg.ROWWISE if rowwise else pkg.COLWISE
                    Y0 = t.full((b * ld,), -3.0, dtype=A.torch_dtype, device="cuda")
                    pkg.set_tuning(spmmv_variant=3)
                    pkg.spmmv(A0, _dev(t, X), Y0, b, ld, lay)
                    pkg.set_tuning(spmmv_variant=0)
                    for swz in (0, 1):                     # plan kernel for every width it supports, both LDS layouts
                        for var, pd in ((4, 0), (6, 0), (8, 0), (5, 0)):   # single-wave tiles; four lanes per row (64-byte rows): one tile per workgroup / phased plan; gather over the re-ordered copy
                            if (var, swz) == (5, 1):
                                continue
                            pkg.set_tuning(spmmv_variant=var, spmmv_swizzle=swz, spmmv_unroll=pd)
                            Y = t.full((b * ld,), -3.0, dtype=A.torch_dtype, device="cuda")
                            pkg.spmmv(A, _dev(t, X), Y, b, ld, lay)
                            assert t.equal(Y, Y0), (name, C, code, b, rowwise, swz, var, pd)
                    pkg.set_tuning(spmmv_unroll=0)
                    pkg.set_tuning(spmmv_variant=8, spmmv_swizzle=0, spmmv_xcol=1)   # phased kernel assembling its X rows from the column-major vector itself
                    Y.fill_(-3.0)
                    pkg.spmmv(A, _dev(t, X), Y, b, ld, lay)
                    assert t.equal(Y, Y0), (name, C, code, b, rowwise, "xcol=1")
                    pkg.set_tuning(spmmv_variant=0, spmmv_swizzle=0, spmmv_xcol=0)
                    if row_bytes == 64 and C in (32, 64):  # the phased plan with two-byte phase-local indices (one byte is the default when <= 256 rows per phase)
                        pkg.set_tuning(spmmv_idx8=0)
                        A16 = pkg.DeviceMatrix(s, block_tlc=b)
                        pkg.set_tuning(spmmv_idx8=1)
                        pkg.set_tuning(spmmv_variant=8)
                        Y.fill_(-3.0)
                        pkg.spmmv(A16, _dev(t, X), Y, b, ld, lay)
                        assert t.equal(Y, Y0), (name, C, code, b, rowwise, "idx16")
                        pkg.set_tuning(spmmv_reorder=2)                  # ... and over clustered rows (balls over all slots instead of the default's flat patches)
                        Acl = pkg.DeviceMatrix(s, block_tlc=b)
                        pkg.set_tuning(spmmv_reorder=4)
                        for var in (8, 6, 4):
                            pkg.set_tuning(spmmv_variant=var)
                            Y.fill_(-3.0)
                            pkg.spmmv(Acl, _dev(t, X), Y, b, ld, lay)
                            assert t.equal(Y, Y0), (name, C, code, b, rowwise, "clustered rows", var)
                        pkg.set_tuning(spmmv_variant=0)
                        del A16, Acl
                    Y.fill_(-3.0)                          # and whatever auto picks
                    pkg.spmmv(A, _dev(t, X), Y, b, ld, lay)
                    assert t.equal(Y, Y0), (name, C, code, b, rowwise, "auto")
                    pkg.set_tuning(spmmv_list_plan=0)      # ... on the default plan (no one-list-per-tile plan where the phased kernel takes the matrix)
                    Adef = pkg.DeviceMatrix(s, block_tlc=b)
                    pkg.set_tuning(spmmv_list_plan=1)
                    Y.fill_(-3.0)
                    pkg.spmmv(Adef, _dev(t, X), Y, b, ld, lay)
                    assert t.equal(Y, Y0), (name, C, code, b, rowwise, "auto, default plan")
                    del Adef
                    if b == 8:
                        Yo = orc.spmmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, b, ld, rowwise)
                        got = Y.cpu().numpy()
                        n = s.n_rows_padded
                        if rowwise:
                            assert np.array_equal(got[:n * b], Yo[:n * b])
                        else:
                            assert np.array_equal(got.reshape(b, ld)[:, :n], Yo.reshape(b, ld)[:, :n])
    pkg.set_tuning(spmmv_lds_kb=0, spmmv_tile_rows=0, spmmv_list_plan=0)
    assert seen_partial and seen_full
    # the plan from device arrays alone (uspmv_dmat_optimize_block_device: ties ordered by first column, no permutation known)
    for m, C, sigma in ((pkg.read_mtx(mtx_path("bcsstk13")), 32, 512), (pkg.gen_stencil27(20, 20, 20, dof=3), 32, 512), (pkg.gen_stencil27(9, 30, 11, dof=2), 64, 128)):
        s, a, xp = _prep(pkg, m, C, sigma, pkg.F64, make_x(m.n_rows))
        A = pkg.DeviceMatrix(s)
        nt, nst = A.optimize_block_device(8)
        assert nt == (s.n_rows_padded + 63) // 64 and nst > 0
        ld = s.n_rows_padded
        for rowwise in (0, 1):
            X = block_x(xp, ld, 8, ld, rowwise)
            Y = t.full((8 * ld,), -3.0, dtype=t.float64, device="cuda")
            pkg.spmmv(A, _dev(t, X), Y, 8, ld, pkg.ROWWISE if rowwise else pkg.COLWISE)
            Yo = orc.spmmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, 8, ld, rowwise)
            assert np.array_equal(Y.cpu().numpy(), Yo), (C, sigma, rowwise)


def test_crs_spmmv_golden(pkg, torch_cuda):
    """block_spmv_omp_csr (code/kernels.hpp:68-154): C = 1 structs through uspmv_spmmv, b = 4, both layouts."""
    t = torch_cuda
    c = golden("csr.npz")
    for name in ("FDM-2d-16", "impcol_e", "matrix1", "bcsstk13"):
        m = pkg.read_mtx(mtx_path(name))
        for dt, code in (("f64", pkg.F64), ("f32", pkg.F32)):
            s, a, xp = _prep(pkg, m, 1, 1, code, make_x(m.n_rows))
            for tlc in (False, True):      # True: optimised handle = internal SELL-32-1 re-chunking where the padding allows
                A = pkg.DeviceMatrix(s, tlc=tlc)
                for rowwise in (0, 1):
                    X = block_x(xp, s.n_rows, 4, s.n_rows, rowwise)
                    Y = t.full((4 * s.n_rows + 64,), 9.0, dtype=A.torch_dtype, device="cuda")     # + guard zone behind Y
                    pkg.spmmv(A, _dev(t, X), Y, 4, s.n_rows, pkg.ROWWISE if rowwise else pkg.COLWISE)
                    got = Y.cpu().numpy()
                    assert np.array_equal(got[:4 * s.n_rows], c[f"{name}_{dt}_Yb4_{'row' if rowwise else 'col'}"]), (name, dt, rowwise, tlc)
                    assert np.all(got[4 * s.n_rows:] == 9.0), "stores past the caller's rows"
    # narrow SELL chunks on an optimised handle (C = 4, 8, 16 re-chunked to 32): against the plain handle
    m = pkg.read_mtx(mtx_path("FDM-2d-16"))
    for C, sigma in ((4, 8), (8, 64), (16, 512)):
        for code in (pkg.F64, pkg.F32):
            s, a, xp = _prep(pkg, m, C, sigma, code, make_x(m.n_rows))
            A0, A1 = pkg.DeviceMatrix(s), pkg.DeviceMatrix(s, tlc=True)
            for b in (8, 3):
                for lay in (pkg.COLWISE, pkg.ROWWISE):
                    ld = s.n_rows_padded
                    X = block_x(xp, ld, b, ld, lay == pkg.ROWWISE)
                    Y0 = t.full((b * ld + 64,), 9.0, dtype=A0.torch_dtype, device="cuda"); Y1 = Y0.clone()
                    pkg.spmmv(A0, _dev(t, X), Y0, b, ld, lay); pkg.spmmv(A1, _dev(t, X), Y1, b, ld, lay)
                    assert t.equal(Y0, Y1), (C, code, b, lay)


@pytest.mark.parametrize("name", ["bcsstk13", "impcol_e", "FDM-2d-16", "matrix1"])
def test_ap_golden_bitexact(pkg, torch_cuda, name):
    t = torch_cuda
    a = golden("ap.npz")
    p = name + "_"
    m = pkg.read_mtx(mtx_path(name))
    dp, sp = pkg.partition_precisions(m, float(a[p + "th"]))
    Cc, sg = int(a[p + "C"]), int(a[p + "sigma"])
    ds = pkg.convert_to_scs(dp, Cc, sg, pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, Cc, sg, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
    Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
    y = t.zeros(ds.n_rows_padded, dtype=t.float64, device="cuda")
    pkg.spmv_ap(Ad, As, _dev(t, a[p + "x_perm"]), y)
    key = "y_perm_adv" if Cc in ADV_CS else "y_perm_gen"   # matrix1 (C=10): generic kernel reads the float x
    if Cc in ADV_CS:
        assert np.array_equal(y.cpu().numpy(), a[p + key])
        assert np.array_equal(pkg.apply_permutation(y.cpu().numpy(), perm), a[p + "y_orig_adv"])
    # generic-C variant (float x for the sp part): bit-exact with the reference's spmv_omp_scs_ap
    xs = _dev(t, a[p + "x_perm"].astype(np.float32))
    pkg.spmv_ap(Ad, As, _dev(t, a[p + "x_perm"]), y, x_sp=xs)
    assert np.array_equal(y.cpu().numpy(), a[p + "y_perm_gen"])
    # shared tile-local-column plan for the pair: same bits
    for max_lines, tile_rows in ((0, 256), (2, 256), (0, 1024)):
        pkg.set_tuning(tlc_tile_rows=tile_rows)
        nt_, ns_ = pkg.optimize_ap(Ad, As, ds, ss, max_lines)
        pkg.set_tuning(tlc_tile_rows=0)
        y.fill_(7.0)
        pkg.spmv_ap(Ad, As, _dev(t, a[p + "x_perm"]), y)
        if Cc in ADV_CS:
            assert np.array_equal(y.cpu().numpy(), a[p + "y_perm_adv"]), (max_lines, tile_rows, nt_, ns_)
    with pytest.raises(pkg.UspmvError):
        pkg.spmv_ap(As, Ad, _dev(t, a[p + "x_perm"]), y)      # wrong precision order


def test_chunk_subsets_pack_and_permutation(pkg, orc, torch_cuda):
    t = torch_cuda
    from ultimate_spmv_amd import binding as B
    h = golden("halo.npz")
    key = "bcsstk13_C32_s512_seg-nnz_P4"
    tot = pkg.read_mtx(mtx_path("bcsstk13"))
    wsa = pkg.seg_work_sharing_arr(tot, "seg-nnz", 4)
    xg = make_x(tot.n_rows)
    ys = []
    for r in range(4):
        loc = B.seg_local_coo(tot, wsa, r)
        s = pkg.convert_to_scs(loc, 32, 512)
        plan = pkg.HaloPlan(s, wsa, r, 4)
        a = s.arrays()
        pkg.permute_scs_cols(s, a["old_to_new_idx"])
        A = pkg.DeviceMatrix(s)
        inner, bnd = s.split_chunks(plan.n_local)
        x = _dev(t, h[f"{key}_r{r}_x_local"])
        pkg.set_tuning(spmv_variant=2 if r % 2 else 0)
        y = t.full((s.n_rows_padded,), np.nan, dtype=t.float64, device="cuda")
        pkg.spmv_chunks(A, _dev(t, inner), x, y)
        assert int(t.isnan(y).sum()) == len(bnd) * 32
        pkg.spmv_chunks(A, _dev(t, bnd), x, y)
        y2 = t.zeros_like(y)
        pkg.spmv(A, x, y2)
        assert t.equal(y, y2)
        # same split at tile granularity on a handle with a tile-local-column plan
        At = pkg.DeviceMatrix(s, tlc=True)
        cpt = At.tile_rows // s.C
        tb = np.unique(bnd // cpt).astype(np.int32)
        ti = np.setdiff1d(np.arange(At.tlc_tiles, dtype=np.int32), tb).astype(np.int32)
        y3 = t.full((s.n_rows_padded,), np.nan, dtype=t.float64, device="cuda")
        pkg.spmv_tiles(At, _dev(t, ti), x, y3)
        pkg.spmv_tiles(At, _dev(t, tb), x, y3)
        assert t.equal(y3, y2)
        ys.append(pkg.apply_permutation(y.cpu().numpy(), a["old_to_new_idx"]))
        # what this rank would send to everybody who asks for all of its rows, twice over
        idx = np.concatenate([np.arange(plan.n_local), np.arange(plan.n_local)[::-1]]).astype(np.int32)
        out = t.zeros(len(idx), dtype=t.float64, device="cuda")
        pkg.pack_send_buf(x, _dev(t, a["old_to_new_idx"]), _dev(t, idx), out)
        assert np.array_equal(out.cpu().numpy(), orc.pack_send_buf(h[f"{key}_r{r}_x_local"], a["old_to_new_idx"], idx))
        assert np.array_equal(out.cpu().numpy()[:plan.n_local], xg[wsa[r]:wsa[r + 1]])
        o = t.zeros(s.n_rows, dtype=t.float64, device="cuda")
        B.apply_permutation_dev(o, y, _dev(t, a["old_to_new_idx"]))
        assert np.array_equal(o.cpu().numpy(), ys[-1])
    pkg.set_tuning(spmv_variant=0)
    assert np.array_equal(np.concatenate(ys), h[key + "_y_global"])


@pytest.mark.parametrize("name", FULL)
def test_tile_local_column_kernel_bitexact(pkg, orc, torch_cuda, name):
    """uspmv_dmat_optimize: LDS-staged x tiles + 16-bit local column indices must not change a bit of y,
    whether all, some (tiny max_lines) or no tiles can be staged; every C that divides 256."""
    t = torch_cuda
    g = golden(f"scs_{name}.npz")
    m = pkg.read_mtx(mtx_path(name))
    x0 = g["x"]
    for code in (pkg.F64, pkg.F32):
        for Cc, sg in ((int(g["C"]), int(g["sigma"])), (1, 1), (2, 4), (8, 64), (32, 512), (64, 64), (128, 256), (256, 256)):
            s, a, xp = _prep(pkg, m, Cc, sg, code, x0)
            y_or = orc.spmv_scs(Cc, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
            x = _dev(t, xp)
            for max_lines, tile_rows, i12 in ((0, 256, 2), (0, 256, 0), (3, 256, 2), (1, 512, 1), (0, 512, 2), (0, 1024, 2), (5, 1024, 0)):
                pkg.set_tuning(tlc_tile_rows=tile_rows, tlc_idx12=i12)      # local indices in 12 bits wherever they can be (2), by the library's rule (1), never (0)
                A = pkg.DeviceMatrix(s, tlc=True, tlc_max_lines=max_lines)
                pkg.set_tuning(tlc_tile_rows=0, tlc_idx12=1)
                bits = A.index_bits()
                assert bits == (0 if not A.tlc_staged else 16 if i12 == 0 else bits) and bits in (0, 12, 16), (name, code, Cc, sg, max_lines, tile_rows, i12, bits)
                pd = A.plan_download() if Cc >= 32 else None      # (narrow chunks: the plan sits on the internal C = 32 copy)
                if pd is not None and i12 == 2: assert bits == (12 if pd["max_lines_used"] <= 256 else 16), (name, code, Cc, sg, max_lines, tile_rows, bits, pd["max_lines_used"])
                if Cc < 32:      # narrow chunks are re-chunked to C = 32 internally (same row order)
                    nc32 = (s.n_chunks * Cc + 31) // 32
                    assert A.tlc_tiles in (0, (nc32 + tile_rows // 32 - 1) // (tile_rows // 32))
                else:
                    assert A.tlc_tiles == (s.n_chunks + tile_rows // Cc - 1) // (tile_rows // Cc)
                for nt in (0, 1):
                    pkg.set_tuning(nontemporal=nt)
                    y = t.full((s.n_rows_padded,), 9.0, dtype=A.torch_dtype, device="cuda")
                    pkg.spmv(A, x, y)
                    assert np.array_equal(y.cpu().numpy(), y_or), (name, code, Cc, sg, max_lines, nt, A.tlc_staged)
                pkg.set_tuning(nontemporal=1)
            # a misaligned x (not 16-byte aligned) silently takes the plain kernel
            xo = t.zeros(s.n_rows_padded + 1, dtype=x.dtype, device="cuda")
            xo[1:] = x
            y = t.zeros(s.n_rows_padded, dtype=x.dtype, device="cuda")
            pkg.spmv(A, xo[1:], y)
            assert np.array_equal(y.cpu().numpy(), y_or)
    if name == "bcsstk13":
        s, a, xp = _prep(pkg, m, 32, 512, pkg.F64, x0)
        A = pkg.DeviceMatrix(s, tlc=True)
        assert A.tlc_staged == A.tlc_tiles > 0
        s2 = pkg.convert_to_scs(m, 10, 3)          # C does not divide 256: no plan, still correct
        A2 = pkg.DeviceMatrix(s2, tlc=True)
        assert A2.tlc_tiles == 0


def test_local_indices_in_12_bits_every_row_length(pkg, orc, torch_cuda):
    """scs_spmv_tlc over the 12-bit index stream (pairs of slot groups in three dwords, an odd last group in a dword + a ushort, partial
    last pairs): banded matrices whose chunk lengths run through every residue mod 8 from 1 to 41, C in {2 ... 256}, both precisions,
    all tiles / a subset of tiles, bit-identical to the oracle and to the 16-bit stream."""
    t = torch_cuda
    rng = np.random.default_rng(12)
    try:
        for C in (2, 4, 16, 32, 64, 128, 256):
            n = 3000
            I, J = [], []
            for r in range(n):
                k = 1 + (r // 64) % 41                               # rows of a 64-row block share their length: every chunk length occurs
                cols = np.unique(np.clip(r + rng.integers(-300, 301, 3 * k), 0, n - 1))[:k]
                I += [r] * len(cols); J += cols.tolist()
            V = rng.standard_normal(len(I))
            m = pkg.Coo.from_arrays(n, n, np.array(I, np.int32), np.array(J, np.int32), V)
            for code in (pkg.F64, pkg.F32):
                s, a, xp = _prep(pkg, m, C, 1, code, rng.standard_normal(n))
                y_or = orc.spmv_scs(C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
                x = _dev(t, xp)
                got = {}
                for i12 in (0, 2):
                    pkg.set_tuning(tlc_idx12=i12)
                    A = pkg.DeviceMatrix(s, tlc=True)
                    assert A.tlc_staged == A.tlc_tiles > 0 and A.index_bits() == (12 if i12 else 16), (C, code, i12, A.index_bits(), A.tlc_staged, A.tlc_tiles)
                    y = t.full((s.n_rows_padded,), 9.0, dtype=A.torch_dtype, device="cuda")
                    pkg.spmv(A, x, y)
                    assert np.array_equal(y.cpu().numpy(), y_or), (C, code, i12)
                    if C < 32: continue                              # (narrow chunks: the plan sits on the internal C = 32 copy, no tile subsets)
                    ids = t.arange(A.tlc_tiles - 1, -1, -2, dtype=t.int32, device="cuda")     # every other tile, backwards
                    y2 = t.full((s.n_rows_padded,), 9.0, dtype=A.torch_dtype, device="cuda")
                    pkg.spmv_tiles(A, ids, x, y2)
                    got[i12] = y2.cpu().numpy()
                if C >= 32: assert np.array_equal(got[0], got[2]), (C, code)
    finally:
        pkg.set_tuning(tlc_idx12=1)


def _random_coo(n, per_row, rng, empty_every=0, band=None):
    I, J = [], []
    for r in range(n):
        if empty_every and r % empty_every == 0:
            continue
        k = int(rng.integers(1, per_row + 1))
        cols = rng.integers(0, n, k) if band is None else np.clip(r + rng.integers(-band, band + 1, k), 0, n - 1)
        I += [r] * k
        J += cols.tolist()
    V = rng.standard_normal(len(I)) * 10.0 ** rng.integers(-3, 4, len(I))
    return np.array(I, np.int32), np.array(J, np.int32), V


@pytest.mark.parametrize("case", ["wide-random", "ragged-banded", "mostly-empty", "tiny"])
def test_edge_shapes_all_kernels(pkg, orc, torch_cuda, case):
    """Empty rows, all-empty chunks (chunk_lengths = 0), fewer rows than C, ragged row lengths, and
    footprints too wide to stage (gather-fallback tiles at default settings): SpMV (plan and no plan),
    SpMMV and AP against the oracle, bit for bit."""
    t = torch_cuda
    rng = np.random.default_rng(11)
    if case == "wide-random":
        n = 30000; I, J, V = _random_coo(n, 40, rng)
    elif case == "ragged-banded":
        n = 5000; I, J, V = _random_coo(n, 90, rng, empty_every=7, band=300)
    elif case == "mostly-empty":
        n = 4000; I, J, V = _random_coo(n, 3, rng, empty_every=1)          # no entries at all ...
        I = np.array([5, 5, 3999], np.int32); J = np.array([0, 3999, 17], np.int32); V = np.array([2.0, -1.5, 4.0])  # ... but three
    else:
        n = 5; I, J, V = _random_coo(n, 4, rng)
    m = pkg.Coo.from_arrays(n, n, I, J, V)
    x0 = make_x(n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
    for Cc, sg in ((32, 512), (8, 1), (64, 128), (1, 1)):
        for code in (pkg.F64, pkg.F32):
            s, a, xp = _prep(pkg, m, Cc, sg, code, x0)
            y_or = orc.spmv_scs(Cc, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
            x = _dev(t, xp)
            for tlc in (False, True):
                A = pkg.DeviceMatrix(s, tlc=tlc)
                y = t.full((s.n_rows_padded,), 5.0, dtype=A.torch_dtype, device="cuda")
                pkg.spmv(A, x, y)
                assert np.array_equal(y.cpu().numpy(), y_or), (case, Cc, sg, code, tlc, A.tlc_staged, A.tlc_tiles)
            if case == "wide-random" and Cc == 32 and code == pkg.F64:
                assert 0 <= A.tlc_staged < A.tlc_tiles          # some tiles really took the gather path
            ld = s.n_rows_padded
            for b, rowwise in ((4, 0), (8, 1), (3, 0)):
                X = block_x(xp, ld, b, ld, rowwise)
                Y = t.zeros(b * ld, dtype=A.torch_dtype, device="cuda")
                pkg.spmmv(A, _dev(t, X), Y, b, ld, pkg.ROWWISE if rowwise else pkg.COLWISE)
                assert np.array_equal(Y.cpu().numpy(), orc.spmmv_scs(Cc, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"],
                                                                      a["col_idxs"], a["values"], X, b, ld, rowwise)), (case, Cc, b, rowwise)
        # adaptive precision on the same matrix, threshold in the middle of the value range
        dp, sp = pkg.partition_precisions(m, 1.0)
        if dp.nnz:
            ds = pkg.convert_to_scs(dp, Cc, sg, pkg.F64)
            perm = ds.arrays()["old_to_new_idx"].copy()
            try:
                ss = pkg.convert_to_scs(sp, Cc, sg, pkg.F32, fixed_permutation=perm)
            except pkg.UspmvError:
                continue      # dp permutation parks a non-empty sp row on a padded slot (reference overruns here)
            pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
            da, sa = ds.arrays(), ss.arrays()
            xp = np.zeros(ds.n_rows_padded); xp[:n] = pkg.apply_permutation(x0, da["new_to_old_idx"])
            y_or = orc.spmv_scs_ap_adv(Cc, ds.n_chunks, (da["chunk_ptrs"], da["chunk_lengths"], da["col_idxs"], da["values"]),
                                       (sa["chunk_ptrs"], sa["chunk_lengths"], sa["col_idxs"], sa["values"]), xp)
            Ad, As = pkg.DeviceMatrix(ds), pkg.DeviceMatrix(ss)
            y = t.zeros(ds.n_rows_padded, dtype=t.float64, device="cuda")
            pkg.spmv_ap(Ad, As, _dev(t, xp), y)
            assert np.array_equal(y.cpu().numpy(), y_or), (case, Cc, "ap gather")
            pkg.optimize_ap(Ad, As, ds, ss)
            y.fill_(1.0)
            pkg.spmv_ap(Ad, As, _dev(t, xp), y)
            assert np.array_equal(y.cpu().numpy(), y_or), (case, Cc, "ap tlc")


def test_argument_errors(pkg, torch_cuda):
    t = torch_cuda
    s = pkg.convert_to_scs(pkg.gen_stencil27(4, 4, 4), 32, 512)
    A = pkg.DeviceMatrix(s)
    x = t.zeros(s.n_rows_padded, dtype=t.float64, device="cuda")
    with pytest.raises(pkg.UspmvError):
        pkg.spmmv(A, x, x, 2, s.n_rows_padded - 1)              # ld too small
    with pytest.raises(pkg.UspmvError):
        pkg.spmmv(A, x, x, 0, s.n_rows_padded)
    with pytest.raises(pkg.UspmvError):
        pkg.set_tuning(unroll=3)
    rc = pkg.lib().uspmv_spmv(A.h, None, None, None)
    assert rc == 1
    with pytest.raises(pkg.UspmvError):
        pkg.DeviceMatrix(s, crs=True)                           # crs needs C = 1


@pytest.mark.parametrize("shape,C,sigma", [((40, 40, 40), 32, 512), ((33, 17, 9), 64, 128), ((64, 64, 64), 128, 1),
                                           ((50, 20, 20), 16, 64), ((21, 21, 21), 3, 7)])
def test_synthetic_vs_oracle(pkg, orc, torch_cuda, shape, C, sigma):
    t = torch_cuda
    m = pkg.gen_stencil27(*shape)
    x0 = make_x(m.n_rows)
    for code in (pkg.F64, pkg.F32):
        s, a, xp = _prep(pkg, m, C, sigma, code, x0)
        A = pkg.DeviceMatrix(s, tlc=True)
        y_or = orc.spmv_scs(C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
        for variant in (0, 2):
            pkg.set_tuning(spmv_variant=variant)
            y = t.full((s.n_rows_padded,), 1.0, dtype=A.torch_dtype, device="cuda")
            pkg.spmv(A, _dev(t, xp), y)
            assert np.array_equal(y.cpu().numpy(), y_or), variant
        pkg.set_tuning(spmv_variant=0)


def test_full_size_nlpkkt200_class(pkg, orc, torch_cuda):
    """BASELINE config 2 size (27-pt stencil on 253^3, n = 16.2M, nnz = 4.3e8, SELL-32-512 dp):
    bit-exact against the oracle on the same arrays, plus size-independent properties:
    linearity A(2x) == 2 A x exactly, row sums A*1 against a numpy segment sum (tolerance), and
    un-permuting y reproduces the COO-order CSR product on a sample of rows."""
    t = torch_cuda
    n1 = int(os.environ.get("USPMV_FULL_N", "253"))
    t0 = time.time()
    m = pkg.gen_stencil27(n1, n1, n1)
    s = pkg.convert_to_scs(m, 32, 512)
    a = s.arrays()
    pkg.permute_scs_cols(s, a["old_to_new_idx"])
    a = s.arrays()
    print(f"\n[full] n={m.n_rows} nnz={m.nnz} n_el={s.n_elements} gen+convert {time.time() - t0:.1f}s", flush=True)
    x0 = make_x(m.n_rows)
    xp = np.zeros(s.n_rows_padded)
    xp[:s.n_rows] = pkg.apply_permutation(x0, a["new_to_old_idx"])
    A = pkg.DeviceMatrix(s, tlc=True)
    print(f"[full] tile-local-column plan: {A.tlc_staged} of {A.tlc_tiles} tiles staged", flush=True)
    x = _dev(t, xp)
    y = t.zeros(s.n_rows_padded, dtype=t.float64, device="cuda")
    pkg.set_tuning(tlc=0)
    pkg.spmv(A, x, y)
    y_plain = y.clone()
    pkg.set_tuning(tlc=1)
    y.zero_()
    pkg.spmv(A, x, y)
    assert t.equal(y, y_plain)
    yh = y.cpu().numpy()
    t0 = time.time()
    y_or = orc.spmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
    print(f"[full] oracle SpMV {time.time() - t0:.1f}s", flush=True)
    assert np.array_equal(yh, y_or)
    y2 = t.zeros_like(y)
    pkg.spmv(A, 2.0 * x, y2)
    assert t.equal(y2, 2.0 * y)
    # GPU-side set-up path at this size: device conversion + device plan builder == host conversion + host planner
    # (here every tile carries padding entries whose column lies far from the tile's own range: split bitmap)
    t0 = time.time()
    lay, Ad = pkg.convert_to_scs_device(m, 32, 512)
    Ad.optimize_device()
    print(f"[full] device convert + plan {time.time() - t0:.1f}s, {Ad.tlc_staged} of {Ad.tlc_tiles} tiles staged", flush=True)
    assert (Ad.tlc_tiles, Ad.tlc_staged) == (A.tlc_tiles, A.tlc_staged)
    ph, pd = A.plan_download(), Ad.plan_download()
    for k in ("tile_line_ptr", "tile_lines", "c16_ptrs", "col16"):
        assert np.array_equal(ph[k], pd[k]), k
    del ph, pd
    y2.zero_()
    pkg.spmv(Ad, x, y2)
    assert t.equal(y2, y)
    del Ad, lay
    # sample of rows against the row-sorted COO (original numbering)
    I, J, V = m.arrays()
    yo = pkg.apply_permutation(yh, a["old_to_new_idx"])
    rows = np.random.default_rng(0).integers(0, m.n_rows, 2000)
    starts = np.searchsorted(I, rows, side="left"); ends = np.searchsorted(I, rows, side="right")
    for r, b, e in zip(rows, starts, ends):
        acc = 0.0
        for k in range(b, e):
            acc = float(np.float64(V[k]) * np.float64(x0[J[k]]) + acc)   # not fused: tolerance
        assert abs(acc - yo[r]) <= 1e-13 * float(np.abs(V[b:e] * x0[J[b:e]]).sum())


def test_spmmv_line_plan_column_major_without_relayout(pkg, orc, torch_cuda):
    """Column-major block vectors with 64-byte rows staged by 128-byte LINES straight from the caller's X (scs_spmmv_quadph, XM = 2:
    no re-layout pass, no workspace) -- the path uspmv_spmmv takes when the handle's line plan qualifies (X rows that come in runs:
    sigma = 1 here; under sigma = 512 the column numbering is scrambled inside the windows and the planner turns the line plan
    down).  Same bits as the gather kernel, the re-layout path and the oracle (block_spmv_omp_scs_general, code/kernels.hpp:306-398)."""
    t = torch_cuda
    used = 0
    for shape, dof, C, sigma, code, b in (((30, 30, 30), 3, 32, 1, pkg.F64, 8), ((40, 36, 20), 1, 64, 1, pkg.F64, 8), ((36, 30, 24), 2, 32, 1, pkg.F32, 16),
                                          ((14, 12, 11), 3, 32, 512, pkg.F64, 8)):
        coo = pkg.gen_stencil27(*shape, dof=dof)
        s, a, xp = _prep(pkg, coo, C, sigma, code, make_x(coo.n_rows))
        ld = s.n_rows_padded + 8                     # (a multiple of the 16-byte piece: what the line path needs)
        pkg.set_tuning(spmmv_xline=1)                # (opt-in: measured slower than the re-layout pass on config 3 even where it qualifies)
        A = pkg.DeviceMatrix(s, block_tlc=b)
        info = A.block_plan_info()
        assert info["phased_plan"] == 1
        if sigma == 1 and code == pkg.F64 and dof == 3:      # (one oversize group anywhere turns the whole line plan down: only this shape is promised)
            assert info["line_plan"] == 1 and info["line_rows_staged"] > 0, info
        X = block_x(xp, s.n_rows_padded, b, ld, 0)
        Yo = orc.spmmv_scs(C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, b, ld, False)
        res = {}
        for xline in (1, 0):
            pkg.set_tuning(spmmv_xline=xline)
            Y = t.full((b * ld,), -3.0, dtype=A.torch_dtype, device="cuda")
            pkg.spmmv(A, _dev(t, X), Y, b, ld, pkg.COLWISE)
            res[xline] = Y.cpu().numpy()
        pkg.set_tuning(spmmv_xline=0)
        n = s.n_rows_padded
        for v in range(b):                           # (the guard zone between the columns keeps its fill value)
            assert np.array_equal(res[1][v * ld:v * ld + n], Yo[v * ld:v * ld + n]), (shape, C, sigma, v)
            assert np.all(res[1][v * ld + n:(v + 1) * ld] == -3.0)
        assert np.array_equal(res[1], res[0])
        used += info["line_plan"]
    assert used >= 1


def test_device_block_plan_builder_equals_host_planner(pkg, orc, torch_cuda):
    """uspmv_dmat_optimize_block_device with the plan built entirely on the device (csrc/block_plan_kernels.hip: row order, phases, X-row
    lists, one-byte indices, group-major values) against the same entry point planning the index part on the host ("block_plan_device" 0):
    every plan array bit for bit (digests of the device arrays), and Y against the oracle, both layouts.  The device builder undoes the
    ties and fills every phase to the brim, so the host planner is asked for the same ("spmmv_reorder" 1, "spmmv_phase_dp" 0; its own
    defaults -- flat row patches, cuts by dynamic programming -- are checked in test_block_plan_row_patches_and_dp_cuts)."""
    t = torch_cuda
    pkg.set_tuning(spmmv_reorder=1, spmmv_phase_dp=0)
    cases = [(pkg.gen_stencil27(20, 18, 16, dof=3), 32, 512, pkg.F64, 8), (pkg.gen_stencil27(20, 18, 16, dof=3), 32, 1, pkg.F64, 8),
             (pkg.gen_stencil27(16, 15, 14, dof=2), 64, 64, pkg.F64, 8), (pkg.gen_stencil27(14, 13, 12, dof=3), 32, 512, pkg.F32, 16),
             (pkg.read_mtx(mtx_path("bcsstk13")), 32, 512, pkg.F64, 8), (pkg.read_mtx(mtx_path("impcol_e")), 64, 64, pkg.F32, 16),
             (pkg.gen_banded_random(20000, 40, 3000), 32, 512, pkg.F64, 8)]
    try:
        for coo, C, sigma, code, b in cases:
            s, a, xp = _prep(pkg, coo, C, sigma, code, make_x(coo.n_rows))
            ld = s.n_rows_padded
            digests = {}
            for dev in (0, 1):
                pkg.set_tuning(block_plan_device=dev)
                A = pkg.DeviceMatrix(s)
                A.optimize_block_device(b)
                info = A.block_plan_info()
                assert info["phased_plan"] == 1 and info["idx8"] == 1 and info["device_built"] == dev, (C, sigma, dev, info)
                info.pop("device_built")
                digests[dev] = (A.block_plan_digest(), info)
                for rowwise in (0, 1):
                    X = block_x(xp, s.n_rows_padded, b, ld, rowwise)
                    Yo = orc.spmmv_scs(C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], X, b, ld, bool(rowwise))
                    Y = t.full((b * ld,), -3.0, dtype=A.torch_dtype, device="cuda")
                    pkg.spmmv(A, _dev(t, X), Y, b, ld, pkg.ROWWISE if rowwise else pkg.COLWISE)
                    assert np.array_equal(Y.cpu().numpy(), Yo), (C, sigma, code, dev, rowwise)
            assert digests[0][1] == digests[1][1], (C, sigma, digests[0][1], digests[1][1])
            assert digests[0][0] == digests[1][0], (C, sigma, code, [k for k in range(8) if digests[0][0][k] != digests[1][0][k]])
    finally:
        pkg.set_tuning(block_plan_device=1, spmmv_reorder=4, spmmv_phase_dp=24)


def test_block_plan_row_patches_and_dp_cuts(pkg, orc, torch_cuda):
    """The host planner's row orders (0 as is | 1 ties undone | 2 balls | 4 flat patches, the default) x phase cuts (0 greedy | 24 | 200: dynamic
    programming) on mesh, file and banded-random matrices, with and without sigma sorting / column permutation, handles with and without
    the host struct's permutation: both layouts bit-identical to the oracle, every plan a phased one-byte plan, and on the 3-dof mesh the
    default stages at most 0.85 of the X rows the ties-undone / greedy plan does."""
    t = torch_cuda
    cases = [("mesh3", pkg.gen_stencil27(24, 22, 20, dof=3), 32, 512, pkg.F64, 8), ("mesh3 s1", pkg.gen_stencil27(20, 18, 16, dof=3), 32, 1, pkg.F64, 8),
             ("mesh2 C64", pkg.gen_stencil27(16, 15, 14, dof=2), 64, 128, pkg.F64, 8), ("mesh3 sp", pkg.gen_stencil27(14, 13, 12, dof=3), 32, 512, pkg.F32, 16),
             ("bcsstk13", pkg.read_mtx(mtx_path("bcsstk13")), 32, 512, pkg.F64, 8), ("impcol_e", pkg.read_mtx(mtx_path("impcol_e")), 32, 64, pkg.F64, 8),
             ("banded", pkg.gen_banded_random(20000, 40, 3000), 32, 512, pkg.F64, 8)]
    staged = {}
    try:
        for name, coo, C, sigma, code, b in cases:
            s, a, xp = _prep(pkg, coo, C, sigma, code, make_x(coo.n_rows))
            ld = s.n_rows_padded
            Yo = {rw: orc.spmmv_scs(C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], block_x(xp, ld, b, ld, rw), b, ld, bool(rw)) for rw in (0, 1)}
            for reorder in (0, 1, 2, 4):
                for dp in (0, 24, 200):
                    for structless in (0, 1):
                        if structless and (reorder in (0, 2) or dp == 200): continue
                        pkg.set_tuning(spmmv_reorder=reorder, spmmv_phase_dp=dp, block_plan_device=0)
                        A = pkg.DeviceMatrix(s)
                        if structless: A.optimize_block_device(b)      # (arrays copied back, no permutation known: ties ordered by first column)
                        else: A.optimize_block(s, b)
                        info = A.block_plan_info()
                        assert info["phased_plan"] == 1 and info["idx8"] == 1 and info["device_built"] == 0, (name, reorder, dp, info)
                        if not structless: staged[(name, reorder, dp)] = info["rows_staged"]
                        for rw in (0, 1):
                            Y = t.full((b * ld,), -3.0, dtype=A.torch_dtype, device="cuda")
                            pkg.spmmv(A, _dev(t, block_x(xp, ld, b, ld, rw)), Y, b, ld, pkg.ROWWISE if rw else pkg.COLWISE)
                            assert np.array_equal(Y.cpu().numpy(), Yo[rw]), (name, reorder, dp, structless, rw)
                        del A
        assert staged[("mesh3", 4, 24)] <= 0.85 * staged[("mesh3", 1, 0)], staged
        for name, *_ in cases:                                  # the dynamic programme never stages more than the greedy cuts + its per-phase allowance
            for reorder in (0, 1, 2, 4):
                assert staged[(name, reorder, 24)] <= staged[(name, reorder, 0)] * 1.02 + 64, (name, reorder, staged)
    finally:
        pkg.set_tuning(block_plan_device=1, spmmv_reorder=4, spmmv_phase_dp=24)


def test_spmmv_column_major_x_prepared_once(pkg, orc, torch_cuda):
    """uspmv_spmmv_x_prepared: a caller whose column-major X does not change between calls (the reference's bench loop, code/main.cpp:458-519)
    pays the re-layout once.  Same bits as the per-call form; another X falls back to the per-call pass (and gives ITS result); after that
    the first X is right again; release ends it."""
    t = torch_cuda
    m = pkg.gen_stencil27(12, 11, 10, dof=3)
    s, a, xp = _prep(pkg, m, 32, 512, pkg.F64, make_x(m.n_rows))
    for b in (8, 4, 3):
        A = pkg.DeviceMatrix(s, block_tlc=b if b == 8 else 0)
        ld = s.n_rows_padded
        X1 = np.concatenate([xp * (1.0 + v / 8.0) for v in range(b)]); X2 = np.concatenate([xp * (2.0 - v / 16.0) for v in range(b)])
        d1, d2 = _dev(t, X1), _dev(t, X2)
        Y = t.zeros(b * ld, dtype=t.float64, device="cuda")
        ref = {}
        # x_pass of uspmv_spmmv_last_path: 0 X as passed (b = 3 has no re-layout pass), 1 re-laid out in the call, 2 the prepared workspace reused
        fresh, reused = (0, 0) if b == 3 else (1, 2)
        for nm, d in (("1", d1), ("2", d2)):
            pkg.spmmv(A, d, Y, b, ld, pkg.COLWISE); t.cuda.synchronize()
            assert A.spmmv_last_path()[1] == fresh, b
            ref[nm] = Y.clone()
            Yo = orc.spmmv_scs(32, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], d.cpu().numpy(), b, ld, False)
            assert np.array_equal(ref[nm].cpu().numpy(), Yo)
        pkg.spmmv_x_prepared(A, d1, b, ld)
        for _ in range(3):
            Y.zero_(); pkg.spmmv(A, d1, Y, b, ld, pkg.COLWISE); t.cuda.synchronize()
            assert t.equal(Y, ref["1"]), b
            assert A.spmmv_last_path()[1] == reused, b
        Y.zero_(); pkg.spmmv(A, d2, Y, b, ld, pkg.COLWISE); t.cuda.synchronize()
        assert t.equal(Y, ref["2"]), b
        assert A.spmmv_last_path()[1] == fresh, b             # (the other X: the per-call pass)
        Y.zero_(); pkg.spmmv(A, d1, Y, b, ld, pkg.COLWISE); t.cuda.synchronize()
        assert t.equal(Y, ref["1"]), b
        assert A.spmmv_last_path()[1] == fresh, b             # (the workspace held the other X)
        pkg.spmmv_x_prepared(A, d2, b, ld)
        d2.mul_(1.0)                                          # (contents unchanged)
        Y.zero_(); pkg.spmmv(A, d2, Y, b, ld, pkg.COLWISE); t.cuda.synchronize()
        assert t.equal(Y, ref["2"]), b
        assert A.spmmv_last_path()[1] == reused, b
        pkg.spmmv_x_release(A)
        Y.zero_(); pkg.spmmv(A, d2, Y, b, ld, pkg.ROWWISE if False else pkg.COLWISE); t.cuda.synchronize()
        assert t.equal(Y, ref["2"]), b
        assert A.spmmv_last_path()[1] == fresh, b
