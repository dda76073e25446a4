"""Equilibrated adaptive precision on the host (no GPU): uspmv_coo_equilibrate_scales against uspmv_coo_equilibrate, the pinned oracle
and numpy; uspmv_partition_precisions_eq against a numpy restatement of the reference's equilibrated branches
(code/utilities.hpp:2883-2896 ap[dp_sp], :2934-2950 ap[dp_hp], :2989-3007 ap[sp_hp], :3046-3078 ap[dp_sp_hp]) and -- ap[dp_sp] -- against
what partition_precisions<double,int> of the genuine reference gave (tests/golden/ap_equilibrated.npz).  numpy's double
arithmetic is IEEE, so every comparison is on bits.

The cases (CASES) and the helpers are shared with tests/test_gpu_ap_equilibrated.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, mtx_path

FIXTURE = os.path.join(GOLDEN, "ap_equilibrated.npz")
KINDS = ("dp_sp", "dp_hp", "sp_hp", "dp_sp_hp")
FILES = ("bcsstk13", "impcol_e", "matrix_band_klein")
CASES = FILES + ("rect_37x53", "rect_53x37")


def rect_case(n_rows, n_cols, seed):
    """random rectangular matrix, sorted by row, with some empty rows and some empty columns, no explicit zero"""
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, 2, 3, 5, 9], n_rows)
    lens[[1, n_rows - 1]] = 0
    cols = np.setdiff1d(np.arange(n_cols), [0, 7, n_cols - 1])          # columns that may be used
    I = np.repeat(np.arange(n_rows), lens)
    J = np.concatenate([np.sort(rng.choice(cols, k, replace=False)) for k in lens])
    V = rng.standard_normal(I.size) * 10.0 ** rng.integers(-6, 3, I.size)
    assert np.all(V != 0.0)
    return n_rows, n_cols, I.astype(np.int32), J.astype(np.int32), V


def pow2_case():
    """values +-2^a, a uniform in -8 .. 8: every scale and every threshold t / (c r) is a power of two, exact, and |v| == T really occurs"""
    rng = np.random.default_rng(4242)
    n_rows, n_cols = 61, 67
    lens = rng.integers(1, 9, n_rows)
    I = np.repeat(np.arange(n_rows), lens)
    J = np.concatenate([np.sort(rng.choice(n_cols, k, replace=False)) for k in lens])
    V = rng.choice([-1.0, 1.0], I.size) * 2.0 ** rng.integers(-8, 9, I.size)
    return n_rows, n_cols, I.astype(np.int32), J.astype(np.int32), V


def case_arrays(pkg, name):
    """(n_rows, n_cols, I, J, V) of a case, unscaled, as numpy copies"""
    if name == "rect_37x53":
        return rect_case(37, 53, 3753)
    if name == "rect_53x37":
        return rect_case(53, 37, 5337)
    if name == "pow2":
        return pow2_case()
    m = pkg.read_mtx(mtx_path(name))
    I, J, V = m.arrays()
    return m.n_rows, m.n_cols, I.copy(), J.copy(), V.copy()


def np_scales(n_rows, n_cols, I, J, V):
    """extract_largest_row_elems, scale_matrix_rows, extract_largest_col_elems, scale_matrix_cols (code/utilities.hpp:2605-2665)"""
    r = np.zeros(n_rows); c = np.zeros(n_cols)
    np.maximum.at(r, I, np.abs(V))
    with np.errstate(all="ignore"):
        s = V / r[I]
        np.maximum.at(c, J, np.abs(s))
        return s / c[J], r, c


def np_partition_eq(kind, I, J, V, r, c, t1, t2):
    """part of every entry (0 hi, 1 mid, 2 lo) and the values the parts store, the reference's branch order restated"""
    with np.errstate(all="ignore"):
        d = c[J] * r[I]                                          # (:2884: largest_col_elems[J] * largest_row_elems[I])
        T1, T2 = t1 / d, t2 / d
        av = np.abs(V)
        part = np.full(V.size, 2)                                # the plain else (:2890, :2940, :2996, :3066), a NaN included
        if kind == "dp_sp_hp":
            part[(av <= T1) & (av >= T2)] = 1                    # (:3056-3059)
        part[av >= T1] = 0                                       # the first branch wins (:2883, :2934, :2989, :3046)
        f32 = V.astype(np.float32).astype(np.float64)
        f16 = V.astype(np.float16).astype(np.float64)
    stored = [f32 if kind == "sp_hp" else V, f32, f32 if kind == "dp_sp" else f16]
    return part, stored, (av, T1, T2)


def quantile_thresholds(kind, I, J, V, r, c):
    """thresholds at quantiles of |v| c[J] r[I]: target 0.6 for the two-part kinds, 2/3 and 1/3 for the three-part kind.  Where the
    quantity takes few distinct values (matrix_band_klein: three) a quantile can sit on the smallest one, or both on the same, and leave a
    part empty: such a threshold moves up to the next distinct value."""
    q = np.abs(V) * c[J] * r[I]
    u = np.unique(q[np.isfinite(q)])

    def at(target, above):
        t = float(np.quantile(q[np.isfinite(q)], target))
        return t if t > above else float(u[u > above][0])
    if kind == "dp_sp_hp":
        t2 = at(1 / 3, u[0])
        return at(2 / 3, t2), t2
    return at(0.6, u[0]), 0.0


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_parts(parts, kind, I, J, V, part, stored, where=""):
    """parts: [hi, mid, lo] as (I, J, V) numpy triples or None"""
    assert (parts[1] is None) == (kind != "dp_sp_hp"), where
    for p in range(3):
        if parts[p] is None:
            assert not np.any(part == p), where
            continue
        sel = part == p
        pI, pJ, pV = parts[p]
        assert np.array_equal(pI, I[sel]) and np.array_equal(pJ, J[sel]), f"{where} part {p}: indices"
        assert same_bits(pV, stored[p][sel]), f"{where} part {p}: values"


def host_parts(coos):
    return [None if q is None else tuple(a.copy() for a in q.arrays()) for q in coos]


def scaled_case(pkg, name):
    """(Coo scaled in place, r, c, numpy copies of I, J, scaled V)"""
    n_rows, n_cols, I, J, V = case_arrays(pkg, name)
    m = pkg.Coo.from_arrays(n_rows, n_cols, I, J, V)
    r, c = m.equilibrate_scales()
    return m, r, c, I, J, m.arrays()[2].copy()


# ------------------------------------------------------------------------------------------------ scaled values
@pytest.mark.parametrize("name", CASES)
def test_equilibrate_scales_bitwise(pkg, orc, name):
    n_rows, n_cols, I, J, V = case_arrays(pkg, name)
    a = pkg.Coo.from_arrays(n_rows, n_cols, I, J, V)
    b = pkg.Coo.from_arrays(n_rows, n_cols, I, J, V)
    r, c = a.equilibrate_scales()
    b.equilibrate()
    got = a.arrays()[2]
    assert same_bits(got, b.arrays()[2])
    # (the reference sizes BOTH vectors by n_cols, code/utilities.hpp:2670: the 53 x 37 case is where vectors of n_rows and n_cols show;
    # the pinned oracle's restatement sizes its scratch for either shape)
    assert same_bits(got, orc.equilibrate_matrix(n_rows, n_cols, I, J, V))
    want, wr, wc = np_scales(n_rows, n_cols, I, J, V)
    assert same_bits(got, want) and same_bits(r, wr) and same_bits(c, wc)
    if name.startswith("rect"):
        assert np.any(r == 0.0) and np.any(c == 0.0), "the rectangular cases have empty rows and columns"
        assert r.shape == (n_rows,) and c.shape == (n_cols,)


# ------------------------------------------------------------------------------------------------ partition
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", CASES)
def test_partition_eq_matches_restatement(pkg, name, kind):
    m, r, c, I, J, V = scaled_case(pkg, name)
    t1, t2 = quantile_thresholds(kind, I, J, V, r, c)
    part, stored, _ = np_partition_eq(kind, I, J, V, r, c, t1, t2)
    for p in ((0, 2) if kind != "dp_sp_hp" else (0, 1, 2)):
        assert np.any(part == p), f"part {p} is empty: the thresholds do not split {name}"
    assert_parts(host_parts(pkg.partition_precisions_eq(m, kind, t1, t2, r, c)), kind, I, J, V, part, stored, f"{name} {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_partition_eq_power_of_two_equalities(pkg, kind):
    """|v| == T1 and |v| == T2 occur: pins >= against > and the <= && >= of the middle part"""
    m, r, c, I, J, V = scaled_case(pkg, "pow2")
    t1, t2 = 1.0, 2.0 ** -4
    part, stored, (av, T1, T2) = np_partition_eq(kind, I, J, V, r, c, t1, t2)
    assert np.count_nonzero(av == T1) > 0 and np.count_nonzero(av == T2) > 0
    assert np.all(part[av == T1] == 0)
    if kind == "dp_sp_hp":
        assert np.all(part[av == T2] == 1)
    assert_parts(host_parts(pkg.partition_precisions_eq(m, kind, t1, t2, r, c)), kind, I, J, V, part, stored, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_partition_eq_nan_goes_to_lo(pkg, kind):
    """the equilibrated branch of a two-part kind ends in a plain else (code/utilities.hpp:2890): a NaN lands in lo, not refused"""
    _, r, c, I, J, V = scaled_case(pkg, "rect_37x53")
    V = V.copy()
    k = V.size // 2
    V[k] = np.nan
    m = pkg.Coo.from_arrays(37, 53, I, J, V)
    t1, t2 = quantile_thresholds(kind, I, J, V, r, c)
    part, stored, _ = np_partition_eq(kind, I, J, V, r, c, t1, t2)
    assert part[k] == 2
    parts = host_parts(pkg.partition_precisions_eq(m, kind, t1, t2, r, c))
    assert np.count_nonzero(np.isnan(parts[2][2])) == 1 and not np.any(np.isnan(parts[0][2]))
    sel = part == 2
    assert np.array_equal(parts[2][0], I[sel]) and np.array_equal(parts[2][1], J[sel])
    ok = ~np.isnan(stored[2][sel])
    assert np.array_equal(bits(parts[2][2])[ok], bits(stored[2][sel])[ok])
    assert_parts([parts[0], parts[1], None], kind, I, J, V, np.where(part == 2, 3, part), stored, kind)


# ------------------------------------------------------------------------------------------------ refusals
def refused_cases():
    n_rows, n_cols, I, J, V = rect_case(37, 53, 3753)
    out = {}
    z = V.copy(); z[I == I[0]] = 0.0
    out["zero_row"] = (n_rows, n_cols, I, J, z)
    z = V.copy(); z[J == J[V.size // 2]] = 0.0
    out["zero_col"] = (n_rows, n_cols, I, J, z)
    z = V.copy(); z[V.size // 3] = np.inf
    out["inf"] = (n_rows, n_cols, I, J, z)
    return out


@pytest.mark.parametrize("what", ("zero_row", "zero_col", "inf"))
def test_equilibrate_scales_refusals(pkg, what):
    n_rows, n_cols, I, J, V = refused_cases()[what]
    m = pkg.Coo.from_arrays(n_rows, n_cols, I, J, V)
    with pytest.raises(pkg.UspmvError) as e:
        m.equilibrate_scales()
    assert e.value.status == 1
    assert same_bits(m.arrays()[2], V), "a refused matrix is left unchanged"


def test_symbols_exported_and_bound(pkg):
    from ultimate_spmv_amd import binding
    for name in ("uspmv_coo_equilibrate_scales", "uspmv_partition_precisions_eq", "uspmv_equilibrate_device",
                 "uspmv_partition_precisions_device_eq", "uspmv_convert_to_scs_device_ap_from_arrays_eq"):
        assert getattr(pkg.lib(), name).argtypes is not None
        assert name in binding._SIGS
    with pytest.raises(pkg.UspmvError):
        pkg.partition_precisions_eq(pkg.Coo.from_arrays(2, 2, [0], [0], [1.0]), 17, 1.0, 0.0, np.ones(2), np.ones(2))


# ------------------------------------------------------------------------------------------------ the genuine reference, ap[dp_sp]
@pytest.fixture(scope="module")
def ref():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", CASES + ("pow2",))
def test_partition_eq_dp_sp_matches_the_reference(pkg, ref, name):
    """what partition_precisions<double,int> (code/utilities.hpp:2878-2927) gave with config.equilibrate = 1 after the call order of
    code/main.cpp:1147-1166, the two vectors sized n_rows and n_cols: a mask (1: dp) per entry and the sp values"""
    n_rows, n_cols, I, J, V0 = case_arrays(pkg, name)
    if name in FILES:
        assert int(ref[name + "/nnz"]) == V0.size
    else:                                   # the inputs of the generated cases, as the fixture was made from them
        assert np.array_equal(ref[name + "/I"], I) and np.array_equal(ref[name + "/J"], J) and same_bits(ref[name + "/V"], V0)
    m, r, c, I, J, V = scaled_case(pkg, name)
    t1 = float(ref[name + "/t1"])
    hi, mid, lo = pkg.partition_precisions_eq(m, "dp_sp", t1, 0.0, r, c)
    assert mid is None
    mask = ref[name + "/dp_mask"].astype(bool)
    assert mask.any() and not mask.all()
    assert same_bits(ref[name + "/scaled"], V) if name + "/scaled" in ref else True
    hI, hJ, hV = hi.arrays()
    lI, lJ, lV = lo.arrays()
    assert np.array_equal(hI, I[mask]) and np.array_equal(hJ, J[mask]) and same_bits(hV, V[mask])
    assert np.array_equal(lI, I[~mask]) and np.array_equal(lJ, J[~mask])
    sp = ref[name + "/sp_values"]
    assert sp.dtype == np.float32 and np.array_equal(lV.astype(np.float32).view(np.uint32), sp.view(np.uint32))
    assert same_bits(lV, sp.astype(np.float64))


# ------------------------------------------------------------------------------------------------ the C++ header's overload
CPP_SRC = r'''
#include <cstdio>
#include "uspmv_interface.hpp"
int main(int argc, char **argv) {
    MtxData<double, int> m;
    read_mtx(argv[1], &m);
    uspmv_coo_t *coo = nullptr;
    if (uspmv_coo_create(m.n_rows, m.n_cols, m.nnz, m.I.data(), m.J.data(), m.values.data(), &coo)) return 1;
    std::vector<double> r(m.n_rows), c(m.n_cols);
    if (uspmv_coo_equilibrate_scales(coo, r.data(), c.data())) return 1;
    const int32_t *I, *J; const double *V;
    uspmv_coo_arrays(coo, &I, &J, &V);
    m.values.assign(V, V + m.nnz);
    MtxData<double, int> dp, dp0; MtxData<float, int> sp, sp0;
    partition_precisions(atof(argv[2]), &m, &dp, &sp, &r, &c, true);
    partition_precisions(atof(argv[2]), &m, &dp0, &sp0, &r, &c, false);
    double a = 0, b = 0;
    for (double v : dp.values) a += v;
    for (float v : sp.values) b += v;
    printf("%ld %ld %.17g %.17g %ld %ld\n", dp.nnz, sp.nnz, a, b, dp0.nnz, sp0.nnz);
    std::vector<double> few(1);
    try { partition_precisions(1.0, &m, &dp, &sp, &few, &c, true); }
    catch (const std::runtime_error &e) { printf("caught: %s\n", e.what()); }
    return 0;
}
'''


def test_cpp_overload_with_the_scaling_arguments(tmp_path, pkg, ref):
    import subprocess
    from conftest import ROOT
    src = tmp_path / "t.cpp"
    src.write_text(CPP_SRC)
    exe = tmp_path / "t"
    libdir = os.path.join(ROOT, "ultimate-spmv_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-luspmv", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    t1 = float(ref["impcol_e/t1"])
    out = subprocess.check_output([str(exe), mtx_path("impcol_e"), repr(t1)], text=True).splitlines()
    m, r, c, I, J, V = scaled_case(pkg, "impcol_e")
    mask = ref["impcol_e/dp_mask"].astype(bool)
    f = out[0].split()
    assert (int(f[0]), int(f[1])) == (int(mask.sum()), int((~mask).sum()))
    acc = 0.0
    for v in V[mask].tolist():
        acc += v
    assert float(f[2]) == acc
    acc = 0.0
    for v in ref["impcol_e/sp_values"].tolist():
        acc += v
    assert float(f[3]) == acc
    dp0, sp0 = pkg.partition_precisions(m, t1)                 # is_equilibrated = false: the unscaled branch on the same values
    assert (int(f[4]), int(f[5])) == (dp0.nnz, sp0.nnz) and int(f[4]) != int(f[0])
    assert out[1].startswith("caught: partition_precisions")
