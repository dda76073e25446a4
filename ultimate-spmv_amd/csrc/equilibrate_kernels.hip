// equilibrate_matrix ON THE DEVICE (uspmv_equilibrate_device): device-resident COO arrays, sorted by row, are scaled as
// uspmv_coo_equilibrate_scales scales a host matrix (extract_largest_row_elems, scale_matrix_rows, extract_largest_col_elems,
// scale_matrix_cols; code/utilities.hpp:2605-2665 in the order of code/main.cpp:1147-1153), and the two divisor vectors are kept for the
// equilibrated branch of partition_precisions.  A maximum does not depend on the order it is taken in and an IEEE division is exact, so
// any schedule gives the host's bits.
//   pass (a)  eq_row_max_kernel   row_max[i] = max |v| of row i.  The rows are runs of the sorted I: a segmented maximum over the 128
//                                 entries of a wave (six shuffle steps, no LDS); the lane on a run's last entry stores it.  Only a run
//                                 that reaches into a neighbouring wave -- at most two per wave -- goes through an atomic maximum.
//                                 Checks the row indices, the row order and that every value is finite.
//   pass (b)  eq_col_max_kernel   col_max[j] = max |v / row_max[i]| of column j: a 64-bit unsigned atomic maximum on the bit pattern (the
//                                 candidates are non-negative doubles, whose order is that of their bits), issued only when a plain load
//                                 of col_max[j] shows a smaller value.  What the load sees is never above the true maximum, so a skipped
//                                 candidate could not have raised it; all but the record-setting updates of a column fall away.
//                                 Checks the column indices and the row divisors; notes whether any row-scaled value is 0.
//   (rare)    eq_zero_cols_kernel only after pass (b) met a row-scaled 0: is the divisor of some entry's column 0?
//   pass (c)  eq_scale_kernel     V_out = (v / row_max[i]) / col_max[j], after the host has read the flag word: nothing is written to
//                                 V_out once a check has failed.
// A lane holds two neighbouring entries (one 16-byte load of V, 8-byte loads of I and J where the arrays are aligned).  Bytes per entry:
// (a) reads I and V (12), (b) reads I, J and V (16), (c) reads them again and writes V (24): 52 in all, plus the gathers of row_max /
// col_max, which mostly hit in L2.
#include "uspmv_device.hpp"

#include <memory>

using namespace uspmv_dev;

namespace {

constexpr int WG = 256, PER_WG = 512;                      // entries: 256 lanes x 2
constexpr double F64_MAX = 1.7976931348623157e308;

__device__ __forceinline__ double max_gt(const double a, const double b) { return b > a ? b : a; }   // (the host's `if (a > local) local = a`)

template <bool VEC>
__global__ void __launch_bounds__(WG) eq_row_max_kernel(const int *__restrict__ I, const double *__restrict__ V, const long nnz, const int n_rows,
                                                        double *row_max, int *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const long k = 2 * ((long)blockIdx.x * WG + threadIdx.x);
    const int n = k + 1 < nnz ? 2 : (k < nnz ? 1 : 0);
    // an entry that does not exist sits in "row" n_rows (behind every row, never stored) with magnitude 0
    int i0 = n_rows, i1 = n_rows;
    double a0 = 0.0, a1 = 0.0;
    if (VEC && n == 2) {
        const int2 a = *(const int2 *)(I + k);
        const double2 c = *(const double2 *)(V + k);
        i0 = a.x; i1 = a.y; a0 = __builtin_fabs(c.x); a1 = __builtin_fabs(c.y);
    } else {
        if (n > 0) { i0 = I[k]; a0 = __builtin_fabs(V[k]); }
        if (n > 1) { i1 = I[k + 1]; a1 = __builtin_fabs(V[k + 1]); }
    }
    // the rows around this lane's pair: from the neighbouring lanes, from memory at the ends of the wave (-1: there is none)
    const int up = __shfl_up(i1, 1, 64), down = __shfl_down(i0, 1, 64);
    const int before = lane > 0 ? up : (n > 0 && k > 0 ? I[k - 1] : -1);
    const int after = lane < 63 ? down : (k + 2 < nnz ? I[k + 2] : -1);
    int err = 0;
    if (n > 0) {
        if (i0 < 0 || i0 >= n_rows) err |= 2;
        else if (i0 < before) err |= 1;
        if (!(a0 <= F64_MAX)) err |= 8;
    }
    if (n > 1) {
        if (i1 < 0 || i1 >= n_rows) err |= 2;
        else if (i1 < i0) err |= 1;
        if (!(a1 <= F64_MAX)) err |= 8;
    }
    if (err) atomicOr(flag, err);

    // segmented inclusive maximum over the lanes, keyed by the row of a lane's LAST entry; of a lane that holds the end of one row and the
    // start of the next only the second entry takes part.  The rows are sorted: where the key `o` lanes up equals mine, everything in
    // between, my first entry included, lies in that row too.
    const int key = i1;
    double val = i0 == i1 ? max_gt(a0, a1) : a1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double uv = __shfl_up(val, o, 64);
        const int uk = __shfl_up(key, o, 64);
        if (lane >= o && uk == key) val = max_gt(val, uv);
    }
    const double pv = __shfl_up(val, 1, 64);
    const int pk = __shfl_up(key, 1, 64);
    // the wave's first run is open to the left when the entry before the wave lies in the same row
    const int first_row = __shfl(i0, 0, 64);
    const int first_open = __shfl((int)(before == i0), 0, 64);

    auto put = [&](const int row, const double m, const bool partial) {
        if ((unsigned)row >= (unsigned)n_rows) return;     // (an entry that does not exist, or an index the flag has reported)
        if (partial) atomicMax((unsigned long long *)(row_max + row), (unsigned long long)__double_as_longlong(m));
        else row_max[row] = m;
    };
    // the run that ends on my first entry (my second one lies in another row, or does not exist)
    if (n > 0 && i0 != i1) put(i0, lane > 0 && pk == i0 ? max_gt(a0, pv) : a0, i0 == first_row && first_open);
    // the run my second entry lies in ends here, or leaves the wave here
    if (n > 1 && (after != key || lane == 63)) put(key, val, (key == first_row && first_open) || after == key);
}

template <bool VEC, bool COUNT>
__global__ void __launch_bounds__(WG) eq_col_max_kernel(const int *__restrict__ I, const int *__restrict__ J, const double *__restrict__ V, const long nnz,
                                                        const int n_rows, const int n_cols, const double *__restrict__ row_max, double *col_max,
                                                        int *__restrict__ flag, unsigned long long *__restrict__ n_atomics) {
    const long k = 2 * ((long)blockIdx.x * WG + threadIdx.x);
    int i[2], j[2];
    double v[2];
    const int n = load_pair<VEC>(I, J, V, k, nnz, i, j, v);
    int err = 0, issued = 0;
    for (int e = 0; e < n; ++e) {
        if (i[e] < 0 || i[e] >= n_rows) { err |= 2; continue; }
        if (j[e] < 0 || j[e] >= n_cols) { err |= 4; continue; }
        const double r = row_max[i[e]];
        if (r == 0.0) { err |= 16; continue; }             // a row of explicit zeros: 0 / 0
        const double s = __builtin_fabs(v[e] / r);
        if (s == 0.0) err |= 32;
        if (s > col_max[j[e]]) {                           // (a stale value is a smaller one: the skip is safe)
            atomicMax((unsigned long long *)(col_max + j[e]), (unsigned long long)__double_as_longlong(s));
            ++issued;
        }
    }
    if (err) atomicOr(flag, err);
    if (COUNT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) issued += __shfl_xor(issued, o, 64);
        if ((threadIdx.x & 63) == 0 && issued) atomicAdd(n_atomics, (unsigned long long)issued);
    }
}

// some row-scaled value is 0 (an explicit zero, or an underflow): 0 / 0 where its whole column is
__global__ void eq_zero_cols_kernel(const int *__restrict__ J, const long nnz, const double *__restrict__ col_max, int *__restrict__ flag) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nnz && col_max[J[k]] == 0.0) atomicOr(flag, 16);
}

template <bool VEC>
__global__ void __launch_bounds__(WG) eq_scale_kernel(const int *__restrict__ I, const int *__restrict__ J, const double *V, double *V_out, const long nnz,
                                                      const double *__restrict__ row_max, const double *__restrict__ col_max) {
    const long k = 2 * ((long)blockIdx.x * WG + threadIdx.x);
    int i[2], j[2];
    double v[2];
    const int n = load_pair<VEC>(I, J, V, k, nnz, i, j, v);
    for (int e = 0; e < n; ++e) v[e] = (v[e] / row_max[i[e]]) / col_max[j[e]];
    if (VEC && n == 2) *(double2 *)(V_out + k) = make_double2(v[0], v[1]);
    else
        for (int e = 0; e < n; ++e) V_out[k + e] = v[e];
}

unsigned eq_grid(long nnz) { return (unsigned)((nnz + PER_WG - 1) / PER_WG); }
bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

namespace uspmv_dev {

int launch_eq_row_max(const int *I, const double *V, long nnz, int n_rows, double *row_max, int *d_flag, hipStream_t st) {
    if (aligned(I, 8) && aligned(V, 16)) hipLaunchKernelGGL(eq_row_max_kernel<true>, dim3(eq_grid(nnz)), dim3(WG), 0, st, I, V, nnz, n_rows, row_max, d_flag);
    else hipLaunchKernelGGL(eq_row_max_kernel<false>, dim3(eq_grid(nnz)), dim3(WG), 0, st, I, V, nnz, n_rows, row_max, d_flag);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_eq_col_max(const int *I, const int *J, const double *V, long nnz, int n_rows, int n_cols, const double *row_max, double *col_max,
                      int *d_flag, unsigned long long *d_n_atomics, hipStream_t st) {
    const bool vec = aligned(I, 8) && aligned(J, 8) && aligned(V, 16), count = d_n_atomics != nullptr;
    auto *kern = vec ? (count ? eq_col_max_kernel<true, true> : eq_col_max_kernel<true, false>)
                     : (count ? eq_col_max_kernel<false, true> : eq_col_max_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3(eq_grid(nnz)), dim3(WG), 0, st, I, J, V, nnz, n_rows, n_cols, row_max, col_max, d_flag, d_n_atomics);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_eq_zero_cols(const int *J, long nnz, const double *col_max, int *d_flag, hipStream_t st) {
    hipLaunchKernelGGL(eq_zero_cols_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, J, nnz, col_max, d_flag);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_eq_scale(const int *I, const int *J, const double *V, double *V_out, long nnz, const double *row_max, const double *col_max, hipStream_t st) {
    if (aligned(I, 8) && aligned(J, 8) && aligned(V, 16) && aligned(V_out, 16))
        hipLaunchKernelGGL(eq_scale_kernel<true>, dim3(eq_grid(nnz)), dim3(WG), 0, st, I, J, V, V_out, nnz, row_max, col_max);
    else
        hipLaunchKernelGGL(eq_scale_kernel<false>, dim3(eq_grid(nnz)), dim3(WG), 0, st, I, J, V, V_out, nnz, row_max, col_max);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // namespace uspmv_dev

namespace {

int eq_args(const char *who, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols, int64_t nnz,
            const double *d_row_max, const double *d_col_max) {
    if (nnz < 0 || (nnz > 0 && (!d_I || !d_J || !d_V)) || !d_row_max || (n_cols > 0 && !d_col_max)) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (n_rows < 1 || n_cols < 0) return uspmv::fail(USPMV_ERR_INVALID, "%s: matrix has no rows", who);
    if (int rc = require_device()) return rc;
    if (n_rows > INT32_MAX || n_cols > INT32_MAX || nnz > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: rows / columns / entries exceed int32", who);
    return USPMV_OK;
}

int read_flag(const int *d_flag, hipStream_t st, int *h_flag) {
    HIP_TRY(hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return USPMV_OK;
}

}  // namespace

extern "C" int uspmv_equilibrate_device(const int32_t *d_I, const int32_t *d_J, const double *d_V, double *d_V_out, int64_t n_rows, int64_t n_cols,
                                        int64_t nnz, double *d_row_max, double *d_col_max, void *stream) {
    const char *who = "uspmv_equilibrate_device";
    if (nnz > 0 && !d_V_out) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (int rc = eq_args(who, d_I, d_J, d_V, n_rows, n_cols, nnz, d_row_max, d_col_max)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_row_max, 0, 8 * (size_t)n_rows, st));
    if (n_cols > 0) HIP_TRY(hipMemsetAsync(d_col_max, 0, 8 * (size_t)n_cols, st));
    if (nnz == 0) { HIP_TRY(hipStreamSynchronize(st)); return USPMV_OK; }
    DeviceBuf<int> flag;
    HIP_TRY(flag.alloc(4));
    HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
    if (int rc = launch_eq_row_max(d_I, d_V, (long)nnz, (int)n_rows, d_row_max, flag, st)) return rc;
    if (int rc = launch_eq_col_max(d_I, d_J, d_V, (long)nnz, (int)n_rows, (int)n_cols, d_row_max, d_col_max, flag, nullptr, st)) return rc;
    int h_flag = 0;
    if (int rc = read_flag(flag, st, &h_flag)) return rc;
    if (!(h_flag & (2 | 4 | 1 | 8 | 16)) && (h_flag & 32)) {
        if (int rc = launch_eq_zero_cols(d_J, (long)nnz, d_col_max, flag, st)) return rc;
        if (int rc = read_flag(flag, st, &h_flag)) return rc;
        if (h_flag & 16) return uspmv::fail(USPMV_ERR_INVALID, "%s: an element lies in a column whose largest row-scaled magnitude is 0 (0 / 0 has no portable bits)", who);
    }
    if (h_flag & 2) return uspmv::fail(USPMV_ERR_INVALID, "%s: a row index lies outside [0, n_rows)", who);
    if (h_flag & 4) return uspmv::fail(USPMV_ERR_INVALID, "%s: a column index lies outside [0, n_cols)", who);
    if (h_flag & 1) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: COO entries must be sorted by row (uspmv_read_mtx and the generators produce that order)", who);
    if (h_flag & 8) return uspmv::fail(USPMV_ERR_INVALID, "%s: an element is not finite", who);
    if (h_flag & 16) return uspmv::fail(USPMV_ERR_INVALID, "%s: an element lies in a row whose largest magnitude is 0 (0 / 0 has no portable bits)", who);
    if (int rc = launch_eq_scale(d_I, d_J, d_V, d_V_out, (long)nnz, d_row_max, d_col_max, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return USPMV_OK;
}

extern "C" int uspmv_equilibrate_device_count_atomics(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                                      int64_t nnz, const double *d_row_max, double *d_col_max, void *stream, int64_t *n_atomics) {
    const char *who = "uspmv_equilibrate_device_count_atomics";
    if (!n_atomics) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (int rc = eq_args(who, d_I, d_J, d_V, n_rows, n_cols, nnz, d_row_max, d_col_max)) return rc;
    hipStream_t st = (hipStream_t)stream;
    *n_atomics = 0;
    if (nnz == 0 || n_cols == 0) return USPMV_OK;
    DeviceBuf<int> flag;
    DeviceBuf<unsigned long long> cnt;
    HIP_TRY(flag.alloc(4));
    HIP_TRY(cnt.alloc(8));
    HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
    HIP_TRY(hipMemsetAsync(cnt, 0, 8, st));
    HIP_TRY(hipMemsetAsync(d_col_max, 0, 8 * (size_t)n_cols, st));
    if (int rc = launch_eq_col_max(d_I, d_J, d_V, (long)nnz, (int)n_rows, (int)n_cols, d_row_max, d_col_max, flag, cnt, st)) return rc;
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_atomics = (int64_t)h;
    return USPMV_OK;
}
