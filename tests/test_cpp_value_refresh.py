"""DeviceScs::values_changed / update_values_from_device_coo of include/uspmv_interface.hpp (numeric refresh: new values on an unchanged
pattern): compile and link with g++ against libuspmv.so; on a GPU a matrix built by DeviceScs::from_device_coo on impcol_e takes new
values from COO arrays in HBM and reproduces the oracle's y on the host struct of those values, bit for bit, there and back."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_x, mtx_path
from test_value_refresh_host import new_values

LIBDIR = os.path.join(ROOT, "ultimate-spmv_amd")

SRC = r'''
#include <cstdio>
#include "uspmv_interface.hpp"
int main() {
    DeviceScs A;                            // no handle: both calls are refused with the library's text before any device is looked for
    int caught = 0;
    try { A.values_changed(); } catch (const std::runtime_error &e) { printf("caught: %s\n", e.what()); ++caught; }
    try { A.update_values_from_device_coo(nullptr, nullptr, nullptr, 4, 0, nullptr); } catch (const std::runtime_error &e) { printf("caught: %s\n", e.what()); ++caught; }
    static_assert(USPMV_REFRESH_COPIES == 1 && USPMV_REFRESH_RECHUNKED == 2 && USPMV_REFRESH_SWEEP_REBUILT == 4 && USPMV_REFRESH_BLOCK_SWEEP_DROPPED == 8, "actions");
    return caught == 2 ? 0 : 1;
}
'''


def test_refresh_calls_of_the_header_compile_and_link(tmp_path, pkg):
    src = tmp_path / "a.cpp"
    src.write_text(SRC)
    exe = tmp_path / "a"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", LIBDIR, "-luspmv", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert out[0].startswith("caught: uspmv_dmat_values_changed: uspmv_dmat_values_changed: NULL argument")
    assert out[1].startswith("caught: uspmv_dmat_update_values_from_arrays: uspmv_dmat_update_values_from_arrays: NULL argument")


GPU_SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <hip/hip_runtime_api.h>
#include "uspmv_interface.hpp"
template <typename T> static T *up(const std::vector<T> &v) {
    T *d = nullptr;
    if (hipMalloc((void **)&d, sizeof(T) * (v.size() + 4)) != hipSuccess) exit(2);
    hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    return d;
}
// argv: matrix, C, sigma, new values (nnz doubles, COO order), x file (n_rows_padded doubles, permuted), y file (three vectors: V0, V1, V0 again)
int main(int argc, char **argv) {
    if (argc < 7) return 3;
    MtxData<double, int> m;
    read_mtx(argv[1], &m);
    const ST C = atol(argv[2]), sigma = atol(argv[3]);
    std::vector<double> v1((size_t)m.nnz);
    FILE *f = fopen(argv[4], "rb"); if (!f || fread(v1.data(), 8, v1.size(), f) != v1.size()) return 4; fclose(f);
    int *dI = up(m.I), *dJ = up(m.J);
    double *dV[2] = {up(m.values), up(v1)};
    std::vector<int> perm((size_t)m.n_rows);
    int *d_perm = up(perm);
    DeviceScs A = DeviceScs::from_device_coo(dI, dJ, dV[0], m.n_rows, m.n_cols, m.nnz, C, sigma, false, d_perm, nullptr);
    const size_t n = (size_t)A.n_rows_padded();
    std::vector<double> x(n), y(n);
    f = fopen(argv[5], "rb"); if (!f || fread(x.data(), 8, n, f) != n) return 4; fclose(f);
    double *dx = up(x), *dy = up(y);
    f = fopen(argv[6], "wb");
    for (int step = 0; step < 3; ++step) {
        if (step) printf("%d\n", A.update_values_from_device_coo(dI, dJ, dV[step & 1], m.n_rows, m.nnz, d_perm));
        A.spmv(dx, dy);
        if (hipDeviceSynchronize() != hipSuccess) return 5;
        hipMemcpy(y.data(), dy, 8 * n, hipMemcpyDeviceToHost);
        fwrite(y.data(), 8, n, f);
    }
    fclose(f);
    try {                                   // another pattern behind the same call: refused, by name
        A.update_values_from_device_coo(dI, dI, dV[1], m.n_rows, m.nnz, d_perm);
        return 6;
    } catch (const std::runtime_error &e) { printf("%s\n", e.what()); }
    printf("%d\n", A.values_changed());
    return 0;
}
'''


@pytest.mark.gpu
def test_device_scs_refresh_on_impcol_e(tmp_path, pkg, orc):
    name, Cc, sg = "impcol_e", 32, 64
    m0 = pkg.read_mtx(mtx_path(name))
    I, J, V0 = [np.array(a) for a in m0.arrays()]
    V = [V0, new_values(I, V0)]
    want = []
    for k in (0, 1):
        s = pkg.convert_to_scs(pkg.Coo.from_arrays(m0.n_rows, m0.n_cols, I, J, V[k]), Cc, sg, pkg.F64)
        pkg.permute_scs_cols(s, s.arrays()["old_to_new_idx"].copy())
        a = s.arrays()
        xp = np.zeros(s.n_rows_padded)
        xp[:s.n_rows] = pkg.apply_permutation(make_x(s.n_rows), a["new_to_old_idx"])
        want.append(orc.spmv_scs(Cc, s.n_chunks, a["chunk_ptrs"], a["chunk_lengths"], a["col_idxs"], a["values"], xp))
    src = tmp_path / "g.cpp"
    src.write_text(GPU_SRC)
    exe = tmp_path / "g"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", LIBDIR, "-luspmv", f"-Wl,-rpath,{LIBDIR}"])
    vf, xf, yf = tmp_path / "v1.bin", tmp_path / "x.bin", tmp_path / "y.bin"
    V[1].tofile(vf); xp.tofile(xf)
    out = subprocess.check_output([str(exe), mtx_path(name), str(Cc), str(sg), str(vf), str(xf), str(yf)], text=True).splitlines()
    assert out[0] == out[1] and out[3] == out[0], out          # the same actions every time (whatever plan the device planner chose)
    assert "uspmv_dmat_update_values_from_arrays" in out[2] and "its column differs from the stored one" in out[2], out
    n = xp.size
    y = np.fromfile(yf, np.float64)
    assert y.size == 3 * n
    for step, k in enumerate((0, 1, 0)):
        assert np.array_equal(y[step * n:(step + 1) * n].view(np.uint64), want[k].view(np.uint64)), step
