"""Adaptive precision with an fp16 part, host side (no GPU): the split of uspmv_partition_precisions_hp (partition_precisions of the
library API, code/interface.hpp:691-987, non-equilibrated branch), its binary16 rounding against numpy, and SELL-C-sigma structs of dtype
F16 (uspmv_convert_to_scs)."""
import numpy as np
import pytest

from conftest import mtx_path


def _coo(pkg, vals, n=None):
    vals = np.asarray(vals, np.float64)
    k = len(vals)
    n = n or k
    I = np.arange(k) % n
    order = np.argsort(I, kind="stable")
    return pkg.Coo.from_arrays(n, n, I[order], (np.arange(k) * 7 % n)[order], vals[order]), vals[order]


def _parts(pkg, coo, kind, t1, t2=0.0):
    hi, mid, hp = pkg.partition_precisions_hp(coo, kind, t1, t2)
    return [None if p is None else np.array(p.arrays()[2]) for p in (hi, mid, hp)]


def _expect(vals, kind, t1, t2):
    a = np.abs(vals)
    if kind == "dp_sp_hp":
        hi = a >= t1
        mid = ~hi & (a <= t1) & (a >= t2)
        return hi, mid, ~hi & ~mid
    hi = a >= t1
    return hi, None, a < t1


@pytest.mark.parametrize("kind", ["dp_hp", "sp_hp", "dp_sp_hp"])
def test_partition_boundaries(pkg, kind):
    t1, t2 = 0.5, 0.125
    vals = [0.5, -0.5, 0.125, -0.125, 0.4999999, 0.1249999, 1e-9, -3.0, 0.0, -0.0, 0.25, 7e4, 1e-30]
    coo, v = _coo(pkg, vals, 5)
    hi, mid, hp = _parts(pkg, coo, kind, t1, t2)
    ehi, emid, ehp = _expect(v, kind, t1, t2)
    want_hi = v[ehi] if kind != "sp_hp" else v[ehi].astype(np.float32).astype(np.float64)
    assert np.array_equal(hi, want_hi)
    if kind == "dp_sp_hp":
        assert np.array_equal(mid, v[emid].astype(np.float32).astype(np.float64))
    else:
        assert mid is None
    want_hp = v[ehp].astype(np.float16).astype(np.float64)
    assert np.array_equal(hp.view(np.uint64), want_hp.view(np.uint64))      # -0.0 stays -0.0
    assert (v == t1).sum() and np.all(np.isin(v[np.abs(v) == t1], hi))      # |v| == t1 goes to hi
    if kind == "dp_sp_hp":
        assert np.all(np.isin(v[np.abs(v) == t2], mid))                      # |v| == t2 goes to sp


def test_partition_t2_above_t1(pkg):
    # t2 > t1: nothing satisfies t2 <= |v| <= t1 < ... so every entry below t1 lands in hp
    coo, v = _coo(pkg, [0.1, 0.3, 0.6, 2.0], 4)
    hi, mid, hp = _parts(pkg, coo, "dp_sp_hp", 0.5, 0.9)
    assert np.array_equal(hi, [0.6, 2.0]) and len(mid) == 0
    assert np.array_equal(hp, np.array([0.1, 0.3]).astype(np.float16).astype(np.float64))


def test_partition_nan(pkg):
    coo, _ = _coo(pkg, [1.0, np.nan, 0.01], 3)
    for kind in ("dp_hp", "sp_hp"):
        with pytest.raises(pkg.UspmvError) as e:
            pkg.partition_precisions_hp(coo, kind, 0.5)
        assert e.value.status == 1                                            # USPMV_ERR_INVALID
    hi, mid, hp = _parts(pkg, coo, "dp_sp_hp", 0.5, 0.1)                      # the `else` of interface.hpp: NaN lands in hp
    assert np.array_equal(hi, [1.0]) and len(mid) == 0
    assert len(hp) == 2 and np.isnan(hp).sum() == 1 and hp[~np.isnan(hp)][0] == np.float64(np.float16(0.01))


@pytest.mark.parametrize("kind", ["dp_hp", "sp_hp", "dp_sp_hp"])
def test_partition_all_in_one_part(pkg, kind):
    coo, v = _coo(pkg, np.linspace(-2, 2, 41), 8)
    hi, mid, hp = _parts(pkg, coo, kind, 0.0, 0.0)                            # every |v| >= 0: all in hi
    assert len(hi) == len(v) and len(hp) == 0
    hi, mid, hp = _parts(pkg, coo, kind, np.inf, np.inf)                      # nothing reaches t1 (or t2): all in hp
    assert len(hi) == 0 and len(hp) == len(v)
    if mid is not None:
        assert len(mid) == 0
        hi, mid, hp = _parts(pkg, coo, kind, np.inf, 0.0)                     # all in sp
        assert len(hi) == 0 and len(mid) == len(v) and len(hp) == 0


def _f16_bits_via_scs(pkg, vals):
    n = len(vals)
    coo = pkg.Coo.from_arrays(n, 1, np.arange(n), np.zeros(n), vals)
    s = pkg.convert_to_scs(coo, 1, 1, pkg.F16)
    a = s.arrays()
    assert a["values"].dtype == np.float16
    # C = 1, sigma = 1: element of row r at chunk_ptrs[r]
    return a["values"].view(np.uint16)[a["chunk_ptrs"][:-1]]


def test_fp16_rounding_matches_numpy(pkg):
    rng = np.random.default_rng(7)
    r = np.concatenate([rng.standard_normal(40000) * 10.0 ** rng.integers(-9, 6, 40000),
                        rng.uniform(-70000, 70000, 20000),
                        rng.uniform(-1, 1, 20000) * 2.0 ** -14,                # around and below the smallest normal
                        rng.standard_normal(20000)])
    # hand-picked: ties at 1 (1 + 2^-11, 1 + 3*2^-11), subnormal ties, the largest finite, the rounding limit to inf, infinities, zeros
    picks = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -40, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -60,
             2.0 ** -24, 2.0 ** -26, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 65504.0, 65519.99, 65520.0, 1e6, np.inf, -np.inf, 0.0, -0.0,
             5e-324, -5e-324, 1e-300, 6.103515625e-05, -65520.0, np.nan]
    vals = np.concatenate([r, picks, -np.asarray(picks)])
    got = _f16_bits_via_scs(pkg, vals)
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.uint16)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(vals[i], hex(got[i]), hex(want[i])) for i in bad[:5]]


@pytest.mark.parametrize("kind", ["dp_hp", "dp_sp_hp"])
def test_f16_struct_shares_hi_layout(pkg, kind):
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    hi, mid, hp = pkg.partition_precisions_hp(m, kind, 1e3, 1e1)
    assert hp.nnz > 0 and hi.nnz > 0
    C, sigma = 32, 64
    sh = pkg.convert_to_scs(hi, C, sigma, pkg.F64)
    perm = sh.arrays()["old_to_new_idx"].copy()
    sq = pkg.convert_to_scs(hp, C, sigma, pkg.F16, fixed_permutation=perm)
    sd = pkg.convert_to_scs(hp, C, sigma, pkg.F64, fixed_permutation=perm)  # the same part as doubles (values: the rounded fp16)
    a, q, d = sh.arrays(), sq.arrays(), sd.arrays()
    assert sq.dtype == pkg.F16 and sq.n_chunks == sh.n_chunks and sq.C == sh.C
    assert np.array_equal(q["chunk_ptrs"], d["chunk_ptrs"]) and np.array_equal(q["chunk_lengths"], d["chunk_lengths"])
    assert np.array_equal(q["col_idxs"], d["col_idxs"])
    assert np.array_equal(q["values"].view(np.uint16), d["values"].astype(np.float16).view(np.uint16))
    # rows sit where the hi part's permutation put them
    I, J, _ = hp.arrays()
    rows = perm[np.asarray(I)]
    assert np.all(q["chunk_lengths"][rows // C] > 0)
    assert np.array_equal(a["old_to_new_idx"], perm)


def test_bad_kind_and_dtype(pkg):
    coo, _ = _coo(pkg, [1.0, 2.0, 3.0], 3)
    assert pkg.convert_to_scs(coo, 2, 1, pkg.F16).dtype == pkg.F16
    with pytest.raises(pkg.UspmvError):
        pkg.convert_to_scs(coo, 2, 1, 3)                                    # no dtype beyond F16
    with pytest.raises(pkg.UspmvError):
        pkg.partition_precisions_hp(coo, 7, 1.0)                           # unknown kind
