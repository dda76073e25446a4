"""scs_spmv_tlc staging through the 2-byte block-local column map and the tagged line lists (csrc/spmv_kernels.hip, ADD): on every struct
of test_additive_map16_host.py -- the one whose permutation is not block-local included -- y of a handle planned with "tlc_additive" 2 is
bit-identical to the same struct planned with "tlc_additive" 0 and to the oracle, in double and float."""
import numpy as np
import pytest

from test_additive_map16_host import STENCILS, band_with_hole_coo, probe, strided_coo, struct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _run(pkg, t, s, key, x):
    pkg.set_tuning(tlc_additive=key)
    try:
        A = pkg.DeviceMatrix(s, tlc=True)
    finally:
        pkg.set_tuning(tlc_additive=1)
    y = t.full((s.n_rows_padded,), 9.0, dtype=A.torch_dtype, device="cuda")
    pkg.spmv(A, x, y)
    t.cuda.synchronize()
    return A, y.cpu().numpy()


def _ramp(s):
    """a non-constant ramp in the caller's (permuted) numbering"""
    xp = np.zeros(s.n_rows_padded, s.np_dtype)
    xp[:s.n_rows] = (1.0 + 1e-3 * (np.arange(s.n_rows) % 1009)).astype(s.np_dtype)
    return xp


def _check(pkg, orc, t, s, xp, want_records=True, tag="", oracle=True):
    a = s.arrays()
    x = t.from_numpy(np.ascontiguousarray(xp)).cuda()
    A0, y0 = _run(pkg, t, s, 0, x)
    assert A0.additive_chunks() == (0, 0), tag
    A1, y1 = _run(pkg, t, s, 2, x)
    n_add, n_ch = A1.additive_chunks()
    if want_records:
        per = max(1, 32 // s.C)                                                # (chunks narrower than 32 rows are re-chunked to 32 inside the handle)
        assert n_ch == (s.n_chunks + per - 1) // per, (tag, n_add, n_ch)         # every tile carries records
    else:
        assert (n_add, n_ch) == (0, 0), tag
    assert np.array_equal(_bits(y1), _bits(y0)), (tag, int((_bits(y1) != _bits(y0)).sum()))
    if oracle:
        y_or = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
        assert np.array_equal(_bits(y1), _bits(y_or)), tag
    return y1


@pytest.mark.parametrize("shape", STENCILS)
def test_stencils_every_window_both_precisions(pkg, orc, t, shape):
    m = pkg.gen_stencil27(*shape)
    for dtype in (pkg.F64, pkg.F32):
        for sigma in (1, 64, 512):
            for permute in (True, False):
                s = struct(pkg, m, 32, sigma, permute, dtype)
                _check(pkg, orc, t, s, _ramp(s), tag=(shape, dtype, sigma, permute))


def test_lines_fed_by_more_than_one_interval(pkg, orc, t):
    for dtype in (pkg.F64, pkg.F32):
        s = struct(pkg, strided_coo(pkg), 32, 512, True, dtype)
        assert probe(pkg, s)[2]["lines_listed_again"] > 0
        _check(pkg, orc, t, s, _ramp(s), tag=("strided", dtype))
        s = struct(pkg, band_with_hole_coo(pkg), 32, 512, True, dtype)
        _check(pkg, orc, t, s, _ramp(s), tag=("band with a hole", dtype))


def test_other_chunk_widths(pkg, orc, t):
    for C, dtype in ((8, pkg.F64), (64, pkg.F64), (64, pkg.F32), (8, pkg.F32)):
        s = struct(pkg, pkg.gen_stencil27(40, 40, 5), C, 512, True, dtype)
        _check(pkg, orc, t, s, _ramp(s), tag=(C, dtype))


def test_permutation_not_block_local_runs_on_the_local_indices(pkg, orc, t):
    m = pkg.gen_stencil27(48, 48, 32)
    for dtype in (pkg.F64, pkg.F32):
        s = struct(pkg, m, 32, 131072, True, dtype)
        _check(pkg, orc, t, s, _ramp(s), want_records=False, tag=("declined", dtype))


def test_nan_at_a_column_no_entry_refers_to(pkg, orc, t):
    drop = 1501
    for dtype in (pkg.F64, pkg.F32):
        s = struct(pkg, band_with_hole_coo(pkg, drop=drop), 32, 512, True, dtype)
        a = s.arrays()
        col = int(a["old_to_new_idx"][drop])                                  # where the caller's x holds that element
        assert not (a["col_idxs"] == col).any() and ((a["col_idxs"] >> 4) == (col >> 4)).any()   # unreferenced, on a staged line
        xp = _ramp(s)
        xp[col] = np.nan
        y = _check(pkg, orc, t, s, xp, tag=("nan", dtype))
        assert np.isfinite(y).all()
