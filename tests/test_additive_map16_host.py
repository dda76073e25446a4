"""The staging data of the additive chunk records (host/tlc_plan.cpp: uspmv_build_additive_plan), on the host: the 2-byte column map that
stays inside aligned blocks of W columns, and the line lists whose entries name the interval their elements go to.  uspmv_additive_plan_probe
decodes every record through the tile's LDS image as the kernel stages it (tagged line list -> map -> interval row), so "decode equals
col_idxs" checks map, W, lists and interval table entry by entry; uspmv_additive_plan_probe2 reports W and the lists.  No GPU."""
import numpy as np
import pytest

STENCILS = [(37, 11, 6), (40, 40, 5)]          # 2 442 rows (not a multiple of 16; planes of 407) and 8 000 rows (planes of 1 600)


def struct(pkg, coo, C, sigma, permute, dtype=None):
    s = pkg.convert_to_scs(coo, C, sigma, pkg.F64 if dtype is None else dtype)
    if permute:
        pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"])
    return s


def band_with_hole_coo(pkg, n=3000, drop=None):
    """rows of {i-40 ... i-34, i, i+34 ... i+40}; drop: a column that is taken out of every row, so that no entry refers to it while
    its line-mates stay referenced"""
    I, J = [], []
    for i in range(n):
        for d in list(range(-40, -33)) + [0] + list(range(34, 41)):
            if 0 <= i + d < n and i + d != drop:
                I.append(i); J.append(i + d)
    rng = np.random.default_rng(3)
    return pkg.Coo.from_arrays(n, n, np.array(I, np.int32), np.array(J, np.int32), rng.standard_normal(len(I)))


def strided_coo(pkg, n=3000):
    """rows of {i ... i + i % 7, i + 600, i + 1162}: seven row lengths, so the sigma sort deals the rows of a window out by length and an x
    line holds every seventh pre-sort column; a 512-row tile has three intervals 88 and 50 columns apart, two of them inside one window"""
    I, J = [], []
    for i in range(n):
        for d in list(range(0, 1 + i % 7)) + [600, 1162]:
            if i + d < n:
                I.append(i); J.append(i + d)
    rng = np.random.default_rng(11)
    return pkg.Coo.from_arrays(n, n, np.array(I, np.int32), np.array(J, np.int32), rng.standard_normal(len(I)))


def probe(pkg, s, key=2):
    pkg.set_tuning(tlc_additive=key)
    try:
        st, cols = pkg.additive_plan_probe(s)
        return st, cols, pkg.additive_plan_probe2(s)
    finally:
        pkg.set_tuning(tlc_additive=1)


def _check_decoded(s, st, cols, st2):
    assert st["kept"] == 1 and st["tiles_with_records"] == st["tiles"] > 0 and st["n_chunks"] == s.n_chunks, st
    assert np.array_equal(cols, s.arrays()["col_idxs"]), (st, st2, int((cols != s.arrays()["col_idxs"]).sum()))
    assert st2["map_bytes"] == 2 * ((s.n_rows + 15) // 16 * 16), st2           # 2 bytes per column, padded to whole lines
    assert st2["list_entries"] >= st2["lines_listed_again"] >= 0 and st2["list_entries"] > 0, st2


@pytest.mark.parametrize("shape", STENCILS)
@pytest.mark.parametrize("sigma", [1, 64, 512])
@pytest.mark.parametrize("permute", [True, False])
def test_stencils_decode_and_block_size(pkg, shape, sigma, permute):
    s = struct(pkg, pkg.gen_stencil27(*shape), 32, sigma, permute)
    st, cols, st2 = probe(pkg, s)
    _check_decoded(s, st, cols, st2)                                            # (37, 11, 6): complete at the last, partial line too
    if permute:
        assert 16 <= st2["W"] <= max(16, sigma) and st2["W"] & (st2["W"] - 1) == 0, st2
    else:
        assert st2["W"] == 16, st2


def test_lines_fed_by_more_than_one_interval(pkg):
    again = []
    for shape in STENCILS:                                                      # planes of 407 and 1 600 elements against windows of 512
        s = struct(pkg, pkg.gen_stencil27(*shape), 32, 512, True)
        st, cols, st2 = probe(pkg, s)
        _check_decoded(s, st, cols, st2)
        again.append(st2["lines_listed_again"])
    assert max(again) > 0, again
    # ... and a matrix where every sixth x line is listed again
    s = struct(pkg, strided_coo(pkg), 32, 512, True)
    st, cols, st2 = probe(pkg, s)
    _check_decoded(s, st, cols, st2)
    assert st2["W"] == 512 and 8 * st2["lines_listed_again"] >= st2["list_entries"], st2
    assert st["n_additive"] > 0, st


def test_band_with_a_hole(pkg):
    for drop in (None, 1501):
        s = struct(pkg, band_with_hole_coo(pkg, drop=drop), 32, 512, True)
        st, cols, st2 = probe(pkg, s)
        _check_decoded(s, st, cols, st2)
        assert 2 * st["n_additive"] >= st["n_chunks"], st


def test_other_chunk_widths_and_float(pkg):
    for C, dtype in ((8, pkg.F64), (64, pkg.F64), (32, pkg.F32)):
        s = struct(pkg, pkg.gen_stencil27(40, 40, 5), C, 512, True, dtype)
        st, cols, st2 = probe(pkg, s)
        _check_decoded(s, st, cols, st2)
        assert st2["W"] <= 512, st2


def test_permutation_not_block_local_is_declined(pkg):
    s = struct(pkg, pkg.gen_stencil27(48, 48, 32), 32, 131072, True)           # 73 728 rows in one window: the sort moves rows across blocks
    assert s.n_rows == 73728
    assert int(s.arrays()["old_to_new_idx"][0]) // 32768 != 0                   # row 0 (a corner: a short row) lands in another 32 768-block
    st, cols, st2 = probe(pkg, s)
    assert st["kept"] == 0 and st["n_chunks"] == 0 and (cols == -1).all(), st
    assert st2 == {"W": 0, "list_entries": 0, "lines_listed_again": 0, "map_bytes": 0}, st2
