// partition_precisions ON THE DEVICE (uspmv_partition_precisions_device): device-resident COO arrays, sorted by row, are split into the
// two or three parts of an adaptive-precision kind, every part compacted in the input's order (= the FMA chain order of its rows).
// The classification is the branch order of uspmv_partition_precisions[_hp] (host/scs_convert.cpp); hp values are rounded once from the
// double with the integer routine of host/uspmv_f16_round.hpp.
//   pass (a)  ap_count_kernel    classify, validate the indices, one count per part and per workgroup
//   pass (b)  the exclusive scan of convert_kernels.hip over the 3 * n_workgroups counts (part-major, so the scan also places the parts)
//   pass (c)  ap_scatter_kernel  classify again, entry -> base[part][workgroup] + rank; the rank is the 64-bit ballot's lower-lane
//                                popcount plus the offsets of the earlier waves and rounds, summed from LDS
// No workgroup waits on another; atomics only raise the error flags.  A workgroup of 256 threads takes 1024 consecutive entries: two
// rounds of 512, a lane holding two neighbouring entries (one 16-byte load of V, 8-byte loads of I and J where the arrays are aligned).
// Bytes per entry: (a) reads I, J and V (16: the index checks belong to the pass that runs before anything is written), (c) reads them
// again and writes the part's I, J and V (32): 48 in all.
// EQ = true is the equilibrated branch (uspmv_partition_precisions_device_eq): entry (I, J, v) is held against
// t / (col_max[J] * row_max[I]), and a two-part kind ends in a plain else.  Both passes then gather row_max[I] and col_max[J] as well: 16
// more bytes per entry and pass where the gathers miss, 80 in all at the most; the vectors of a banded matrix stay in L2.  EQ = false
// compiles to the unscaled kernels as they were.
#include "uspmv_device.hpp"

#include "../host/uspmv_f16_round.hpp"

using namespace uspmv_dev;

namespace {

constexpr int WG = 256, PER_WG = 1024, ROUND = 512;      // entries: 2 rounds x 256 lanes x 2

// part of entry v (0 hi, 1 mid, 2 lo; -1: NaN in a two-part kind) and the value the part stores, as a double
template <bool EQ>
__device__ __forceinline__ int ap_classify(const int kind, const double v, const double t1, const double t2, double *stored) {
    const double av = __builtin_fabs(v);
    const bool hp_lo = kind != USPMV_AP_DP_SP;
    if (av >= t1) { *stored = kind == USPMV_AP_SP_HP ? (double)(float)v : v; return 0; }
    if (kind == USPMV_AP_DP_SP_HP && av <= t1 && av >= t2) { *stored = (double)(float)v; return 1; }
    if (EQ || kind == USPMV_AP_DP_SP_HP || av < t1) {      // (EQ: the plain else of the equilibrated branch, NaN included)
        if (hp_lo) *stored = __longlong_as_double((long long)uspmv_f16_to_f64_bits(uspmv_f64_bits_to_f16((uint64_t)__double_as_longlong(v))));
        else *stored = (double)(float)v;
        return 2;
    }
    return -1;
}

// the thresholds of entry (i, j) in the equilibrated branch: one multiplication, one division each
__device__ __forceinline__ void eq_thresholds(const double *__restrict__ row_max, const double *__restrict__ col_max, const int i, const int j,
                                              const double t1, const double t2, double *T1, double *T2) {
    const double d = col_max[j] * row_max[i];
    *T1 = t1 / d;
    *T2 = t2 / d;
}

template <bool VEC, bool EQ>
__global__ void __launch_bounds__(WG) ap_count_kernel(const int *__restrict__ I, const int *__restrict__ J, const double *__restrict__ V, const long nnz,
                                                      const int n_rows, const int n_cols, const int kind, const double t1, const double t2,
                                                      const long n_wg, long *__restrict__ counts, int *__restrict__ flag,
                                                      unsigned long long *__restrict__ first_nan, const double *__restrict__ row_max,
                                                      const double *__restrict__ col_max) {
    __shared__ int wcnt[3][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int mine[3] = {0, 0, 0};
    int err = 0;
    for (int r = 0; r < 2; ++r) {
        const long k = (long)blockIdx.x * PER_WG + r * ROUND + 2 * threadIdx.x;
        int i[2], j[2];
        double v[2];
        const int n = load_pair<VEC>(I, J, V, k, nnz, i, j, v);
        int prev = n > 0 && k > 0 ? I[k - 1] : 0;
        for (int e = 0; e < n; ++e) {
            if (i[e] < 0 || i[e] >= n_rows) err |= 2;
            else if (i[e] < prev) err |= 1;
            if (j[e] < 0 || j[e] >= n_cols) err |= 4;
            prev = i[e];
            double s, T1 = t1, T2 = t2;
            if (EQ && i[e] >= 0 && i[e] < n_rows && j[e] >= 0 && j[e] < n_cols) eq_thresholds(row_max, col_max, i[e], j[e], t1, t2, &T1, &T2);
            const int c = ap_classify<EQ>(kind, v[e], T1, T2, &s);
            if (c < 0) atomicMin(first_nan, (unsigned long long)(k + e));
            else ++mine[c];
        }
    }
    if (err) atomicOr(flag, err);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        int c = mine[p];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) wcnt[p][wave] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) counts[(long)threadIdx.x * n_wg + blockIdx.x] = (long)wcnt[threadIdx.x][0] + wcnt[threadIdx.x][1] + wcnt[threadIdx.x][2] + wcnt[threadIdx.x][3];
}

template <bool VEC, bool EQ>
__global__ void __launch_bounds__(WG) ap_scatter_kernel(const int *__restrict__ I, const int *__restrict__ J, const double *__restrict__ V, const long nnz,
                                                        const int kind, const double t1, const double t2, const long n_wg,
                                                        const int *__restrict__ base, const ApPartOut out, const double *__restrict__ row_max,
                                                        const double *__restrict__ col_max) {
    __shared__ int ucnt[3][8];                            // entries of part p in unit (round, wave), units in entry order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lower = (1ull << lane) - 1;
    int i[2][2], j[2][2], cls[2][2], rank[2][2] = {{0, 0}, {0, 0}};
    double s[2][2];
    for (int r = 0; r < 2; ++r) {
        const long k = (long)blockIdx.x * PER_WG + r * ROUND + 2 * threadIdx.x;
        double v[2];
        const int n = load_pair<VEC>(I, J, V, k, nnz, i[r], j[r], v);
        for (int e = 0; e < 2; ++e) {
            double T1 = t1, T2 = t2;
            if (EQ && e < n) eq_thresholds(row_max, col_max, i[r][e], j[r][e], t1, t2, &T1, &T2);   // (pass (a) has checked the indices)
            cls[r][e] = e < n ? ap_classify<EQ>(kind, v[e], T1, T2, &s[r][e]) : -1;
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const unsigned long long b0 = __ballot(cls[r][0] == p), b1 = __ballot(cls[r][1] == p);
            const int before = __popcll(b0 & lower) + __popcll(b1 & lower);
            if (cls[r][0] == p) rank[r][0] = before;
            if (cls[r][1] == p) rank[r][1] = before + (cls[r][0] == p ? 1 : 0);
            if (lane == 0) ucnt[p][r * 4 + wave] = __popcll(b0) + __popcll(b1);
        }
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r)
        for (int e = 0; e < 2; ++e) {
            const int p = cls[r][e];
            if (p < 0) continue;
            int off = 0;
            for (int u = 0; u < r * 4 + wave; ++u) off += ucnt[p][u];
            const long dst = (long)base[(long)p * n_wg + blockIdx.x] - base[(long)p * n_wg] + off + rank[r][e];
            // (selects, not out.I[p]: a kernel argument indexed at run time is copied to scratch)
            const long n = p == 0 ? out.n[0] : p == 1 ? out.n[1] : out.n[2];
            if (dst >= n) continue;                      // (cannot happen while the input stays as pass (a) read it)
            int *oI = p == 0 ? out.I[0] : p == 1 ? out.I[1] : out.I[2], *oJ = p == 0 ? out.J[0] : p == 1 ? out.J[1] : out.J[2];
            double *oV = p == 0 ? out.V[0] : p == 1 ? out.V[1] : out.V[2];
            oI[dst] = i[r][e]; oJ[dst] = j[r][e]; oV[dst] = s[r][e];
        }
}

}  // namespace

namespace uspmv_dev {

static bool pair_aligned(const void *I, const void *J, const void *V) {
    return ((uintptr_t)I & 7) == 0 && ((uintptr_t)J & 7) == 0 && ((uintptr_t)V & 15) == 0;
}

long ap_partition_workgroups(long nnz) { return (nnz + PER_WG - 1) / PER_WG; }

int launch_ap_partition_count(const int *I, const int *J, const double *V, long nnz, int n_rows, int n_cols, int kind, double t1, double t2,
                              long *d_counts, int *d_flag, unsigned long long *d_first_nan, hipStream_t st, const double *row_max, const double *col_max) {
    const long n_wg = ap_partition_workgroups(nnz);
    if (n_wg == 0) return USPMV_OK;
    const bool vec = pair_aligned(I, J, V), eq = row_max != nullptr;
    auto *kern = vec ? (eq ? ap_count_kernel<true, true> : ap_count_kernel<true, false>) : (eq ? ap_count_kernel<false, true> : ap_count_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(WG), 0, st, I, J, V, nnz, n_rows, n_cols, kind, t1, t2, n_wg, d_counts, d_flag, d_first_nan, row_max, col_max);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_ap_partition_scatter(const int *I, const int *J, const double *V, long nnz, int kind, double t1, double t2, const int *d_base,
                                const ApPartOut &out, hipStream_t st, const double *row_max, const double *col_max) {
    const long n_wg = ap_partition_workgroups(nnz);
    if (n_wg == 0) return USPMV_OK;
    const bool vec = pair_aligned(I, J, V), eq = row_max != nullptr;
    auto *kern = vec ? (eq ? ap_scatter_kernel<true, true> : ap_scatter_kernel<true, false>) : (eq ? ap_scatter_kernel<false, true> : ap_scatter_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(WG), 0, st, I, J, V, nnz, kind, t1, t2, n_wg, d_base, out, row_max, col_max);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // namespace uspmv_dev
