"""The additive chunk records of the SpMV planner (host/tlc_plan.cpp: uspmv_build_additive_plan), on the host: the planner's encoder runs
on a host struct through uspmv_additive_plan_probe, every record is read back -- interval list -> LDS position -> pre-sort column -> column
of x, the kernel's own steps -- and the column of every entry, padding included, must be the struct's col_idxs.  No GPU."""
import numpy as np
import pytest


def _struct(pkg, coo, C, sigma, permute, dtype=None):
    s = pkg.convert_to_scs(coo, C, sigma, pkg.F64 if dtype is None else dtype)
    if permute:
        pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"])
    return s


def ragged_coo(pkg, n=3000, seed=5):
    """n rows of 1 ... 41 random columns each (rows of a 64-row block share their length): nothing is additive"""
    rng = np.random.default_rng(seed)
    I, J = [], []
    for r in range(n):
        k = 1 + (r // 64) % 41
        cols = np.unique(rng.integers(0, n, 3 * k))[:k]
        I += [r] * len(cols); J += cols.tolist()
    return pkg.Coo.from_arrays(n, n, np.array(I, np.int32), np.array(J, np.int32), rng.standard_normal(len(I)))


def _probe(pkg, s, key):
    pkg.set_tuning(tlc_additive=key)
    try:
        return pkg.additive_plan_probe(s)
    finally:
        pkg.set_tuning(tlc_additive=1)


def _check_decoded(s, st, cols):
    assert st["kept"] == 1 and st["tiles_with_records"] == st["tiles"] > 0 and st["n_chunks"] == s.n_chunks, st
    assert np.array_equal(cols, s.arrays()["col_idxs"]), (st, int((cols != s.arrays()["col_idxs"]).sum()))


@pytest.mark.parametrize("shape,additive,chunks", [((37, 11, 6), 54, 77), ((40, 40, 5), 219, 250)])
def test_stencil_sell_32_512_permuted_columns(pkg, shape, additive, chunks):
    s = _struct(pkg, pkg.gen_stencil27(*shape), 32, 512, True)
    st, cols = _probe(pkg, s, 2)
    _check_decoded(s, st, cols)
    assert s.n_chunks == chunks and 2 * st["n_additive"] >= st["n_chunks"], st          # (cannot pass on the per-entry form alone)
    assert st["n_additive"] == additive, st
    assert st["max_elems"] <= 8192                                                      # the line plan's LDS budget in doubles


@pytest.mark.parametrize("shape", [(37, 11, 6), (40, 40, 5)])
@pytest.mark.parametrize("sigma", [1, 64])
@pytest.mark.parametrize("permute", [True, False])
def test_stencil_other_windows_and_unpermuted_columns(pkg, shape, sigma, permute):
    s = _struct(pkg, pkg.gen_stencil27(*shape), 32, sigma, permute)
    st, cols = _probe(pkg, s, 2)
    _check_decoded(s, st, cols)


@pytest.mark.parametrize("shape", [(37, 11, 6), (40, 40, 5)])
def test_stencil_sigma_512_unpermuted_columns(pkg, shape):
    s = _struct(pkg, pkg.gen_stencil27(*shape), 32, 512, False)
    st, cols = _probe(pkg, s, 2)
    _check_decoded(s, st, cols)


def test_nothing_additive_dropped_by_the_rule_all_per_entry_when_forced(pkg):
    s = _struct(pkg, ragged_coo(pkg), 32, 512, True)
    st, cols = _probe(pkg, s, 1)
    assert st["kept"] == 0 and st["n_additive"] == 0 and 2 * st["new_bytes"] > st["replaced_bytes"] > 0, st
    assert (cols == -1).all()
    st, cols = _probe(pkg, s, 2)
    _check_decoded(s, st, cols)
    assert st["n_additive"] == 0, st
    st, cols = _probe(pkg, s, 0)
    assert st["kept"] == 0 and st["n_chunks"] == 0, st


def test_float_struct_and_wider_chunks(pkg):
    for C, dtype in ((32, pkg.F32), (64, pkg.F64), (8, pkg.F64)):
        s = _struct(pkg, pkg.gen_stencil27(40, 40, 5), C, 512, True, dtype)
        st, cols = _probe(pkg, s, 2)
        _check_decoded(s, st, cols)
