"""scs_spmv_tlc over the additive chunk records ("tlc_additive"; host/tlc_plan.cpp, csrc/tlc_planner.hip, csrc/spmv_kernels.hip): y is
bit-identical to the same handle planned with "tlc_additive" 0 and to the oracle -- same operands, same slot order, only the LDS address of
the x operand is computed differently."""
import gc

import numpy as np
import pytest

from test_additive_plan_host import ragged_coo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _struct(pkg, coo, C, sigma, dtype, permute=True):
    s = pkg.convert_to_scs(coo, C, sigma, dtype)
    if permute:
        pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"])
    return s


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


def _check(pkg, orc, t, s, xp, key=2, want_records=True, tag=""):
    a = s.arrays()
    x = t.from_numpy(np.ascontiguousarray(xp)).cuda()
    y_or = orc.spmv_scs(s.C, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp)
    A0, y0 = _run(pkg, t, s, 0, x)
    assert A0.additive_chunks() == (0, 0), tag
    A1, y1 = _run(pkg, t, s, key, x)
    n_add, n_ch = A1.additive_chunks()
    assert (n_ch > 0) == want_records, (tag, n_add, n_ch)
    assert A1.index_bits() == A0.index_bits() and A1.tlc_staged == A0.tlc_staged, tag      # the local indices stay as built
    assert np.array_equal(_bits(y1), _bits(y0)), (tag, int((_bits(y1) != _bits(y0)).sum()))
    assert np.array_equal(y1, y_or, equal_nan=True), tag
    return n_add, n_ch


def _x(s, rng):
    xp = np.zeros(s.n_rows_padded, s.np_dtype)
    xp[:s.n_rows] = rng.standard_normal(s.n_rows).astype(s.np_dtype)
    return xp


@pytest.mark.parametrize("shape", [(37, 11, 6), (40, 40, 5)])
def test_stencils_every_window_both_precisions_count_as_the_host_encoder(pkg, orc, t, shape):
    rng = np.random.default_rng(7)
    m = pkg.gen_stencil27(*shape)                                       # (37, 11, 6): 77 chunks, the last tile is partial
    for dtype in (pkg.F64, pkg.F32):
        for sigma, permute in ((512, True), (1, True), (64, True), (512, False), (64, False)):
            s = _struct(pkg, m, 32, sigma, dtype, permute)
            n_add, n_ch = _check(pkg, orc, t, s, _x(s, rng), tag=(shape, dtype, sigma, permute))
            pkg.set_tuning(tlc_additive=2)
            try:
                st, _ = pkg.additive_plan_probe(s, decode=False)
            finally:
                pkg.set_tuning(tlc_additive=1)
            assert (n_add, n_ch) == (st["n_additive"], st["n_chunks"]) and n_ch == s.n_chunks, (shape, dtype, sigma, permute, n_add, n_ch, st)
            if sigma == 512 and permute:
                assert 2 * n_add >= n_ch
            st1, _ = pkg.additive_plan_probe(s, decode=False)            # the default: by the byte rule
            if st1["kept"]: assert 2 * st1["new_bytes"] <= st1["replaced_bytes"]
            if shape == (40, 40, 5) and sigma == 512: assert st1["kept"] == 1
            _check(pkg, orc, t, s, _x(s, rng), key=1, want_records=bool(st1["kept"]), tag=("by the rule", shape, dtype, sigma, permute))


def test_narrow_chunks_through_the_internal_rechunking(pkg, orc, t):
    rng = np.random.default_rng(8)
    s = _struct(pkg, pkg.gen_stencil27(40, 40, 5), 8, 512, pkg.F64)
    n_add, n_ch = _check(pkg, orc, t, s, _x(s, rng), tag="C = 8")
    assert n_add > 0


def test_nan_and_inf_at_the_padding_column_and_inside_an_additive_window(pkg, orc, t):
    rng = np.random.default_rng(9)
    s = _struct(pkg, pkg.gen_stencil27(40, 40, 5), 32, 512, pkg.F64)
    inside = int(s.arrays()["old_to_new_idx"][40 * 40 * 2 + 40 * 20 + 20])     # an interior node: its rows' chunks are additive
    for bad in (np.nan, np.inf, -np.inf):
        for where in (0, inside):                                             # column 0: what every padding entry multiplies
            xp = _x(s, rng)
            xp[where] = bad
            _check(pkg, orc, t, s, xp, tag=(bad, where))


def test_nothing_additive_all_per_entry_when_forced_dropped_by_the_rule(pkg, orc, t):
    rng = np.random.default_rng(10)
    m = ragged_coo(pkg)                                                 # chunk lengths 1 ... 41, random columns
    for dtype in (pkg.F64, pkg.F32):
        s = _struct(pkg, m, 32, 512, dtype)
        n_add, n_ch = _check(pkg, orc, t, s, _x(s, rng), tag="ragged, forced")
        assert n_add == 0 and n_ch == s.n_chunks
        _check(pkg, orc, t, s, _x(s, rng), key=1, want_records=False, tag="ragged, by the rule")


def test_every_chunk_length_banded(pkg, orc, t):
    """the matrices of test_local_indices_in_12_bits_every_row_length: chunk lengths through every residue mod 8 from 1 to 41"""
    rng = np.random.default_rng(12)
    n = 3000
    I, J = [], []
    for r in range(n):
        k = 1 + (r // 64) % 41
        cols = np.unique(np.clip(r + rng.integers(-300, 301, 3 * k), 0, n - 1))[:k]
        I += [r] * len(cols); J += cols.tolist()
    m = pkg.Coo.from_arrays(n, n, np.array(I, np.int32), np.array(J, np.int32), rng.standard_normal(len(I)))
    for C in (32, 64):
        for dtype in (pkg.F64, pkg.F32):
            s = _struct(pkg, m, C, 1, dtype)
            _check(pkg, orc, t, s, _x(s, rng), tag=("banded", C, dtype))
    # ... and with whole chunks additive at those lengths: a band of k consecutive columns per row
    I, J = [], []
    for r in range(n):
        k = 1 + (r // 64) % 41
        cols = np.arange(max(0, r - k // 2), min(n, r - k // 2 + k))
        I += [r] * len(cols); J += cols.tolist()
    m = pkg.Coo.from_arrays(n, n, np.array(I, np.int32), np.array(J, np.int32), rng.standard_normal(len(I)))
    for dtype in (pkg.F64, pkg.F32):
        s = _struct(pkg, m, 32, 128, dtype)
        n_add, n_ch = _check(pkg, orc, t, s, _x(s, rng), tag=("band of k", dtype))
        assert 2 * n_add >= n_ch, (n_add, n_ch)


def test_no_device_memory_is_lost_over_twenty_handles(pkg, t):
    s = _struct(pkg, pkg.gen_stencil27(40, 40, 5), 32, 512, pkg.F64)
    x = t.ones(s.n_rows_padded, dtype=t.float64, device="cuda"); y = t.zeros_like(x)

    def cycle(k):
        for _ in range(k):
            A = pkg.DeviceMatrix(s, tlc=True)
            assert A.additive_chunks()[1] == s.n_chunks
            pkg.spmv(A, x, y)
            A.optimize(s)                                               # planned again in place: the records are replaced, not leaked
            pkg.spmv(A, x, y)
            del A
        gc.collect(); t.cuda.synchronize(); t.cuda.empty_cache()

    cycle(1)
    free0, _ = t.cuda.mem_get_info()
    cycle(20)
    free1, _ = t.cuda.mem_get_info()
    assert free0 - free1 <= 2 << 20, f"{(free0 - free1) / 2**20:.1f} MiB of device memory lost over twenty handles"
