"""DeviceApScs of include/uspmv_interface.hpp (the adaptive-precision set-up from COO arrays in HBM, uspmv_convert_to_scs_device_ap_from_arrays):
compiles and links with g++ against libuspmv.so; on a GPU the ap[dp_sp] handles it builds for impcol_e reproduce y of tests/golden/ap.npz
bit for bit, with and without the shared plan."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden, mtx_path

LIBDIR = os.path.join(ROOT, "ultimate-spmv_amd")

SRC = r'''
#include <cstdio>
#include "uspmv_interface.hpp"
int main(int argc, char **) {
    try {                                   // an unknown kind is refused with the library's text before any device is looked for
        DeviceApScs::from_device_coo(nullptr, nullptr, nullptr, 4, 4, 0, 2, 2, 40 + argc, 1.0, 0.0, nullptr, nullptr);
    } catch (const std::runtime_error &e) { printf("caught: %s\n", e.what()); return 0; }
    return 1;
}
'''


def test_device_ap_scs_of_the_header_compiles_and_links(tmp_path, pkg):
    src = tmp_path / "a.cpp"
    src.write_text(SRC)
    exe = tmp_path / "a"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", LIBDIR, "-luspmv", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([str(exe)], text=True)
    assert out.startswith("caught: uspmv_convert_to_scs_device_ap_from_arrays: uspmv_convert_to_scs_device_ap_from_arrays: unknown kind 41")


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
// argv: matrix, threshold, C, sigma, x file (n_rows_padded doubles, permuted), y file
int main(int argc, char **argv) {
    if (argc < 7) return 3;
    MtxData<double, int> m;
    read_mtx(argv[1], &m);
    const ST C = atol(argv[3]), sigma = atol(argv[4]);
    int *dI = up(m.I), *dJ = up(m.J);
    double *dV = up(m.values);
    std::vector<int> perm((size_t)m.n_rows);
    int *d_perm = up(perm);
    for (int planned = 0; planned < 2; ++planned) {
        DeviceApScs A = DeviceApScs::from_device_coo(dI, dJ, dV, m.n_rows, m.n_cols, m.nnz, C, sigma, USPMV_AP_DP_SP, atof(argv[2]), 0.0, d_perm, nullptr,
                                                     false, planned != 0);
        const size_t n = (size_t)A.n_rows_padded();
        std::vector<double> x(n), y(n, 9.0);
        FILE *f = fopen(argv[5], "rb"); if (!f || fread(x.data(), 8, n, f) != n) return 4; fclose(f);
        double *dx = up(x), *dy = up(y);
        A.spmv(dx, dy);
        if (hipDeviceSynchronize() != hipSuccess) return 5;
        hipMemcpy(y.data(), dy, 8 * n, hipMemcpyDeviceToHost);
        f = fopen(argv[6], planned ? "ab" : "wb"); fwrite(y.data(), 8, n, f); fclose(f);
        printf("%ld %ld %ld\n", (long)n, (long)A.part_nnz(0), (long)A.part_nnz(2));
        hipFree(dx); hipFree(dy);
    }
    hipMemcpy(perm.data(), d_perm, 4 * perm.size(), hipMemcpyDeviceToHost);
    printf("%d %d\n", perm[0], perm[perm.size() - 1]);
    return 0;
}
'''


@pytest.mark.gpu
def test_device_ap_scs_on_impcol_e(tmp_path, pkg):
    name, p = "impcol_e", "impcol_e_"
    a = golden("ap.npz")
    th, Cc, sg = float(a[p + "th"]), int(a[p + "C"]), int(a[p + "sigma"])
    xp, want = a[p + "x_perm"], a[p + "y_perm_adv"]
    src = tmp_path / "g.cpp"
    src.write_text(GPU_SRC)
    exe = tmp_path / "g"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", LIBDIR, "-luspmv", f"-Wl,-rpath,{LIBDIR}"])
    xf, yf = tmp_path / "x.bin", tmp_path / "y.bin"
    xp.tofile(xf)
    out = subprocess.check_output([str(exe), mtx_path(name), repr(th), str(Cc), str(sg), str(xf), str(yf)], text=True).split()
    n = xp.size
    assert [int(v) for v in out] == 2 * [n, a[p + "dp_I"].size, a[p + "sp_I"].size] + [int(a[p + "old_to_new"][0]), int(a[p + "old_to_new"][-1])]
    y = np.fromfile(yf, np.float64)
    assert y.size == 2 * n
    assert np.array_equal(y[:n].view(np.uint64), want.view(np.uint64)), "planless"
    assert np.array_equal(y[n:].view(np.uint64), want.view(np.uint64)), "shared plan built on the device"
