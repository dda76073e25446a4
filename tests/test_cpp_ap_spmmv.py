"""spmmv_ap of include/uspmv_interface.hpp (adaptive precision dp+sp on block vectors, over two DeviceScs): compiles and links with g++
against libuspmv.so; on a GPU it reproduces the oracle's per-column result on impcol_e bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, block_x, golden, mtx_path

LIBDIR = os.path.join(ROOT, "ultimate-spmv_amd")

SRC = r'''
#include <cstdio>
#include "uspmv_interface.hpp"
int main(int argc, char **) {
    DeviceScs dp, sp;                       // empty handles: the call is refused with the library's text, no device needed
    try { spmmv_ap(dp, sp, nullptr, nullptr, 4, (ST)argc, false); }
    catch (const std::runtime_error &e) { printf("caught: %s\n", e.what()); return 0; }
    return 1;
}
'''


def test_spmmv_ap_of_the_header_compiles_and_links(tmp_path, pkg):
    src = tmp_path / "a.cpp"
    src.write_text(SRC)
    exe = tmp_path / "a"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", LIBDIR, "-luspmv", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([str(exe)], text=True)
    assert out.startswith("caught: uspmv_spmmv_ap: uspmv_spmmv_ap")


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
template <typename VT> static DeviceScs wrap(const ScsData<VT, int> &s) {
    return DeviceScs::wrap<VT, int>(s.C, s.n_chunks, s.n_elements, up(s.chunk_ptrs), up(s.chunk_lengths), up(s.col_idxs), up(s.values), false);
}
// argv: matrix, threshold, C, sigma, b, ld, rowwise, X file (b * ld doubles), Y file
int main(int argc, char **argv) {
    if (argc < 10) return 3;
    MtxData<double, int> m, dpm; MtxData<float, int> spm;
    read_mtx(argv[1], &m);
    partition_precisions(atof(argv[2]), &m, &dpm, &spm);
    const ST C = atol(argv[3]), sigma = atol(argv[4]);
    ScsData<double, int> sd; ScsData<float, int> ss;
    convert_to_scs<double, double, int>(&dpm, C, sigma, &sd);
    convert_to_scs<float, float, int>(&spm, C, sigma, &ss, sd.old_to_new_idx.data());
    permute_scs_cols<double, int>(&sd, sd.old_to_new_idx.data());
    permute_scs_cols<float, int>(&ss, sd.old_to_new_idx.data());
    DeviceScs dp = wrap(sd), sp = wrap(ss);
    const int b = atoi(argv[5]); const ST ld = atol(argv[6]); const bool rowwise = atoi(argv[7]) != 0;
    std::vector<double> X((size_t)b * ld), Y((size_t)b * ld, 9.0);
    FILE *f = fopen(argv[8], "rb"); if (!f || fread(X.data(), 8, X.size(), f) != X.size()) return 4; fclose(f);
    double *dX = up(X), *dY = up(Y);
    spmmv_ap(dp, sp, dX, dY, b, ld, rowwise);
    if (hipDeviceSynchronize() != hipSuccess) return 5;
    hipMemcpy(Y.data(), dY, 8 * Y.size(), hipMemcpyDeviceToHost);
    f = fopen(argv[9], "wb"); fwrite(Y.data(), 8, Y.size(), f); fclose(f);
    printf("%ld %ld %ld\n", sd.n_chunks, sd.n_elements, ss.n_elements);
    return 0;
}
'''


@pytest.mark.gpu
def test_spmmv_ap_of_the_header_on_impcol_e(tmp_path, pkg, orc):
    name, p = "impcol_e", "impcol_e_"
    a = golden("ap.npz")
    th, Cc, sg = float(a[p + "th"]), int(a[p + "C"]), int(a[p + "sigma"])
    m = pkg.read_mtx(mtx_path(name))
    dp, sp = pkg.partition_precisions(m, th)
    ds = pkg.convert_to_scs(dp, Cc, sg, pkg.F64)
    perm = ds.arrays()["old_to_new_idx"].copy()
    ss = pkg.convert_to_scs(sp, Cc, sg, pkg.F32, fixed_permutation=perm)
    pkg.permute_scs_cols(ds, perm); pkg.permute_scs_cols(ss, perm)
    da, sa = ds.arrays(), ss.arrays()
    n = ds.n_rows_padded
    xp = np.zeros(n); xg = a[p + "x_perm"]; xp[:min(n, len(xg))] = xg[:n]
    src = tmp_path / "g.cpp"
    src.write_text(GPU_SRC)
    exe = tmp_path / "g"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", LIBDIR, "-luspmv", f"-Wl,-rpath,{LIBDIR}"])
    for b, ld, rowwise in ((4, n + 32, 0), (3, n, 1)):
        X = block_x(xp, n, b, ld, rowwise)
        xf, yf = tmp_path / "x.bin", tmp_path / "y.bin"
        X.tofile(xf)
        out = subprocess.check_output([str(exe), mtx_path(name), repr(th), str(Cc), str(sg), str(b), str(ld), str(rowwise), str(xf), str(yf)],
                                      text=True).split()
        assert [int(v) for v in out] == [ds.n_chunks, ds.n_elements, ss.n_elements]
        want = np.full(b * ld, 9.0)
        for v in range(b):
            xcol = np.ascontiguousarray(X[v:n * b:b] if rowwise else X[v * ld:v * ld + n])
            ycol = orc.spmv_scs_ap_adv(Cc, ds.n_chunks, (da["chunk_ptrs"], da["chunk_lengths"], da["col_idxs"], da["values"]),
                                       (sa["chunk_ptrs"], sa["chunk_lengths"], sa["col_idxs"], sa["values"]), xcol)
            if rowwise: want[v:n * b:b] = ycol
            else: want[v * ld:v * ld + n] = ycol
        assert np.array_equal(np.fromfile(yf, np.float64), want), (b, ld, rowwise)
