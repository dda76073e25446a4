"""DeviceApScs::spmv_axpby / spmv_axpby_path / axpby_reserve of include/uspmv_interface.hpp: they compile and link with g++ against
libuspmv.so, and on a GPU one ap[dp_sp] pair and one kind with an fp16 part (ap[sp_hp], float vectors) give the C ABI's y and dots bit
for bit -- and that y is the numpy restatement of the update on what DeviceApScs::spmv stores.  In the manner of
tests/test_cpp_ap_spmmv.py."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, mtx_path

LIBDIR = os.path.join(ROOT, "ultimate-spmv_amd")

SRC = r'''
#include <cstdio>
#include "uspmv_interface.hpp"
int main(int argc, char **) {
    DeviceApScs a;                          // empty handles: every call is refused with the library's text, no device needed
    int caught = 0;
    try { a.spmv_axpby(nullptr, nullptr, 1.0, 0.0); } catch (const std::runtime_error &e) { printf("caught: %s\n", e.what()); ++caught; }
    try { (void)a.spmv_axpby_path(&argc); } catch (const std::runtime_error &e) { printf("caught: %s\n", e.what()); ++caught; }
    try { a.axpby_reserve(); } catch (const std::runtime_error &e) { printf("caught: %s\n", e.what()); ++caught; }
    return caught == 3 ? 0 : 1;
}
'''


def test_the_members_compile_and_link(tmp_path, pkg):
    src = tmp_path / "a.cpp"
    src.write_text(SRC)
    exe = tmp_path / "a"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", LIBDIR, "-luspmv", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert len(out) == 3
    for line, name in zip(out, ("uspmv_spmv_ap_axpby", "uspmv_spmv_ap_axpby_path", "uspmv_spmv_ap_axpby_reserve")):
        assert line.startswith(f"caught: {name}: {name}: NULL matrix"), line


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
template <typename T> static void down(std::vector<T> &v, const T *d) { hipMemcpy(v.data(), d, sizeof(T) * v.size(), hipMemcpyDeviceToHost); }
template <typename T> static void put(FILE *f, const std::vector<T> &v) { fwrite(v.data(), sizeof(T), v.size(), f); }

// HT: the type of x, y, z, w
template <typename HT> static int run(const MtxData<double, int> &m, int kind, double t1, double t2, double alpha, double beta, const char *out) {
    int *dI = up(m.I), *dJ = up(m.J);
    double *dV = up(m.values);
    DeviceApScs A = DeviceApScs::from_device_coo(dI, dJ, dV, m.n_rows, m.n_cols, m.nnz, 32, 512, kind, t1, t2, nullptr, nullptr);
    const size_t np = (size_t)A.n_rows_padded(), n = (size_t)m.n_rows;
    std::vector<HT> x(np), z(np), w(np), t(np, (HT)9), y(np, (HT)9), ya(np, (HT)9);
    for (size_t i = 0; i < np; ++i) {
        x[i] = i < n ? (HT)(1.0 + 1e-3 * (double)(i % 1000)) : (HT)0;
        z[i] = (HT)((double)((i * 7) % 13) - 6.25);
        w[i] = (HT)(0.5 - (double)((i * 3) % 5));
    }
    HT *dx = up(x), *dz = up(z), *dw = up(w), *dt = up(t), *dy = up(y), *dya = up(ya);
    std::vector<double> dots(2, 7.0), dots_abi(2, 7.0);
    double *dd = up(dots), *dda = up(dots_abi);
    const int path = A.spmv_axpby_path(dx);
    A.axpby_reserve();
    A.spmv(dx, dt);
    A.spmv_axpby(dx, dy, alpha, beta, dz, dw, dd, (ST)n);
    const uspmv_axpby_t op{alpha, beta, dz, dw, dda, (int64_t)n};
    int rc;
    if (kind == USPMV_AP_DP_SP) rc = uspmv_spmv_ap_axpby(A.handle(0), A.handle(2), (const double *)dx, (double *)dya, &op, nullptr);
    else rc = uspmv_spmv_ap_hp_axpby(A.handle(0), A.handle(1), A.handle(2), dx, dya, &op, nullptr);
    if (rc != USPMV_OK || hipDeviceSynchronize() != hipSuccess) return 5;
    down(t, dt); down(y, dy); down(ya, dya); down(dots, dd); down(dots_abi, dda);
    FILE *f = fopen(out, "wb");
    if (!f) return 6;
    put(f, x); put(f, z); put(f, w); put(f, t); put(f, y); put(f, ya); put(f, dots); put(f, dots_abi);
    fclose(f);
    printf("%d %zu %zu %ld %ld %ld\n", path, n, np, (long)A.part_nnz(0), (long)A.part_nnz(1), (long)A.part_nnz(2));
    return 0;
}
// argv: matrix, kind (0 dp_sp | 2 sp_hp as the header numbers them), threshold 1, threshold 2, alpha, beta, out file
int main(int argc, char **argv) {
    if (argc < 8) return 3;
    MtxData<double, int> m;
    read_mtx(argv[1], &m);
    const int kind = atoi(argv[2]);
    try {
        if (kind == USPMV_AP_SP_HP) return run<float>(m, kind, atof(argv[3]), atof(argv[4]), atof(argv[5]), atof(argv[6]), argv[7]);
        return run<double>(m, kind, atof(argv[3]), atof(argv[4]), atof(argv[5]), atof(argv[6]), argv[7]);
    } catch (const std::runtime_error &e) { printf("error: %s\n", e.what()); return 4; }
}
'''


@pytest.mark.gpu
def test_spmv_axpby_of_the_header_against_the_c_abi(tmp_path, pkg):
    from test_gpu_ap_elem_plan import _quantiles
    from test_gpu_spmv_axpby import bits, check, restate
    m = pkg.read_mtx(mtx_path("bcsstk13"))
    src = tmp_path / "g.cpp"
    src.write_text(GPU_SRC)
    exe = tmp_path / "g"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", LIBDIR, "-luspmv", f"-Wl,-rpath,{LIBDIR}"])
    alpha, beta = 0.37, -2.5
    for name, kind, np_t in (("dp_sp", pkg.AP_DP_SP, np.float64), ("sp_hp", pkg.AP_SP_HP, np.float32)):
        t1, t2 = _quantiles(m, name)
        out = tmp_path / f"{name}.bin"
        res = subprocess.run([str(exe), mtx_path("bcsstk13"), str(kind), repr(t1), repr(t2), repr(alpha), repr(beta), str(out)],
                             text=True, capture_output=True)
        assert res.returncode == 0, (name, res.returncode, res.stdout, res.stderr)
        path, n, npad, nnz0, nnz1, nnz2 = (int(v) for v in res.stdout.split())
        assert path == 1 and n == m.n_rows and npad == 2016 and nnz0 > 0 and nnz2 > 0, res.stdout
        raw = np.fromfile(out, np.uint8)
        es = np.dtype(np_t).itemsize
        vecs = raw[:6 * npad * es].view(np_t).reshape(6, npad)
        x, z, w, t, y, y_abi = vecs
        dots, dots_abi = raw[6 * npad * es:].view(np.float64).reshape(2, 2)
        assert np.isfinite(t).all() and np.abs(t[:n]).max() > 0
        check(y, restate(t, alpha, beta, z), (name, "DeviceApScs::spmv_axpby against the restatement on DeviceApScs::spmv"))
        check(y, y_abi, (name, "against the C ABI"))
        assert np.array_equal(bits(dots), bits(dots_abi)), (name, dots, dots_abi)
        yd = y[:n].astype(np.float64)
        for k, prod in enumerate((yd * yd, w[:n].astype(np.float64) * yd)):
            ref, bound = math.fsum(prod), 2.0 * n * 2.0 ** -53 * math.fsum(np.abs(prod))     # any summation order plus one rounding per product
            assert abs(dots[k] - ref) <= bound, (name, k, dots[k], ref, bound)
