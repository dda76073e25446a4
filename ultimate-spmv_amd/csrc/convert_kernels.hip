// convert_to_scs ON THE DEVICE from device-resident COO arrays: a matrix that lives in HBM becomes a SELL-C-sigma
// handle without a trip through host memory.  Reference: convert_to_scs, code/utilities.hpp:1842-2104 --
//   row populations          :1901-1903   -> run_bounds_kernel (one pass over the row indices: the start of every row's run) + a difference
//   sigma-window ordering    :1930-1941   -> (a) USPMV_SORT_HOST: the reference's std::sort on the identical pair type and comparator, on the
//                                            HOST, over the O(n_rows) count array only (4 bytes per row down, 4 up): bit-exact incl. the tie
//                                            order of the unstable sort; (b) USPMV_SORT_DEVICE_STABLE: a stable rank per window on the device
//                                            (rows of equal length keep their original order) -- chunk_lengths / chunk_ptrs and y in original
//                                            row order come out bit-identical, the order of equal-length rows inside a window differs
//   chunk lengths            :1949-1966   -> chunk_max_kernel (max over the C rows of a chunk in the new order)
//   chunk pointers           :1949-1966   -> scan_* kernels (exclusive scan of C * length in 64-bit, overflow reported as in :1959-1962)
//   permutations             :1976-1982, :2060-2069 -> perm_kernel
//   scatter                  :2013-2036   -> scs_fill_kernel (uspmv_api.hip), permute_scs_cols (:1802-1831) folded in
// The fixed-permutation form (:1911-1928: the sp struct of an ap[dp_sp] pair takes the dp struct's permutation) skips the ordering.
#include "uspmv_device.hpp"

#include <memory>
#include <utility>
#include <vector>

using namespace uspmv_dev;

namespace uspmv_dev {
int launch_scs_fill(int dtype, long nnz, int C, int n_rows, const int *I, const int *J, const double *V, const int *row_start, const int *row_map,
                    const int *perm, const int *chunk_ptrs, int *col_idxs, void *values, hipStream_t st);   // uspmv_api.hip
}

namespace {

// start[r] = first entry of row r (= lower bound of r in the row-sorted index array) for every r in [0, n_rows], written by the thread
// that sits on the boundary between two runs; unsorted input raises the flag
__global__ void run_bounds_kernel(const int *__restrict__ I, const long nnz, const int n_rows, int *__restrict__ start, int *__restrict__ flag) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nnz) return;
    const int prev = k == 0 ? -1 : I[k - 1];
    const int cur = k == nnz ? n_rows : I[k];
    if (k < nnz && (cur < 0 || cur >= n_rows)) { atomicOr(flag, 2); return; }
    if (cur < prev) { atomicOr(flag, 1); return; }
    for (int r = prev + 1; r <= cur; ++r) start[r] = (int)k;
}

// Stable rank of a window's rows by descending length: new position of row i = #(rows of the window with a longer row) + #(rows before
// i with the same length).  One workgroup per window, lengths staged in LDS, O(sigma^2 / 256) compares per thread.  Rows >= n_rows (the
// padding of the last chunk) take part with length 0, as in the reference's rl array (code/utilities.hpp:1895-1899).
__global__ void __launch_bounds__(256) window_rank_kernel(const int *__restrict__ start, const int n_rows, const long n_pad, const int sigma,
                                                          int *__restrict__ new_pos, int *__restrict__ len_new) {
    extern __shared__ int wl[];
    const long b = (long)blockIdx.x * sigma;
    const int w = (int)min((long)sigma, n_pad - b);
    for (int i = threadIdx.x; i < w; i += 256) { const long r = b + i; wl[i] = r < n_rows ? start[r + 1] - start[r] : 0; }
    __syncthreads();
    for (int i = threadIdx.x; i < w; i += 256) {
        const int me = wl[i];
        int rank = 0;
        for (int j = 0; j < w; ++j) { const int o = wl[j]; rank += (o > me) || (o == me && j < i); }
        new_pos[b + i] = (int)(b + rank);
        len_new[b + rank] = me;
    }
}

// the caller's order of rows: len_new[pos[i]] = length of row i (rows without a position -- i >= n_rows -- keep length 0 where they sit)
__global__ void place_lengths_kernel(const int *__restrict__ start, const int *__restrict__ pos, const int n_rows, const long n_pad, int *__restrict__ len_new, int *__restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int p = pos[i];
    if (p < 0 || p >= n_pad) { atomicOr(flag, 4); return; }
    len_new[p] = start[i + 1] - start[i];
}

// fixed permutation: the slots of the padding rows are re-zeroed AFTER the move (loop order of code/utilities.hpp:1913-1923) ...
__global__ void zero_tail_kernel(int *__restrict__ len_new, const int n_rows, const long n_pad) {
    const long i = n_rows + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pad) len_new[i] = 0;
}
// ... and a non-empty row that now sits in a shorter chunk would overrun it in the scatter (the reference does, :1919-1922): refused
__global__ void check_fixed_kernel(const int *__restrict__ start, const int *__restrict__ pos, const int *__restrict__ chunk_lengths, const int n_rows, const int C, int *__restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    if (start[i + 1] - start[i] > chunk_lengths[pos[i] / C]) atomicOr(flag, 8);
}

__global__ void chunk_max_kernel(const int *__restrict__ len_new, const long n_chunks, const int C, int *__restrict__ chunk_lengths, long *__restrict__ elems) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    int mx = 0;
    for (int i = 0; i < C; ++i) mx = max(mx, len_new[c * C + i]);
    chunk_lengths[c] = mx;
    elems[c] = (long)mx * C;
}

// exclusive scan of `in` (n longs) in three passes: per block of 1024 (scan_block_kernel), over the block sums (one workgroup walking them
// 1024 at a time), and the add (scan_add_kernel), which also narrows to the 32-bit chunk_ptrs of the reference (IT = int)
__global__ void __launch_bounds__(256) scan_block_kernel(const long *__restrict__ in, const long n, long *__restrict__ out, long *__restrict__ sums) {
    __shared__ long s[256];
    const long base = (long)blockIdx.x * 1024 + threadIdx.x * 4;
    long v[4], t = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) { v[u] = base + u < n ? in[base + u] : 0; t += v[u]; }
    s[threadIdx.x] = t;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const long a = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += a;
        __syncthreads();
    }
    long run = s[threadIdx.x] - t;
#pragma unroll
    for (int u = 0; u < 4; ++u) { if (base + u < n) out[base + u] = run; run += v[u]; }
    if (threadIdx.x == 255) sums[blockIdx.x] = s[255];
}
__global__ void __launch_bounds__(1024) scan_sums_kernel(long *__restrict__ sums, const long nb, long *__restrict__ total) {
    __shared__ long s[1024];
    __shared__ long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long b = 0; b < nb; b += 1024) {
        const long i = b + threadIdx.x;
        const long v = i < nb ? sums[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long a = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < nb) sums[i] = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ void scan_add_kernel(const long *__restrict__ part, const long *__restrict__ sums, const long *__restrict__ total, const long n, int *__restrict__ ptrs) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ptrs[i] = (int)(part[i] + sums[i >> 10]);
    if (i == n) ptrs[n] = (int)*total;
}

// old_to_new / new_to_old of the struct (code/utilities.hpp:1976-1982, :2060-2069); identity for a fixed-permutation struct (:1915-1920)
__global__ void perm_kernel(const int *__restrict__ new_pos, const int n_rows, const bool identity, int *__restrict__ o2n, int *__restrict__ n2o) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int p = identity ? (int)i : new_pos[i];
    o2n[i] = p;
    if (p < n_rows) n2o[p] = (int)i;                       // (the reference writes out of bounds otherwise; such slots stay 0)
}

}  // namespace

namespace uspmv_dev {
int launch_exclusive_scan(const long *d_in, long n, long *d_part, long *d_sums, long *d_total, int *d_ptrs, hipStream_t st) {
    const long nb = (n + 1023) / 1024;
    hipLaunchKernelGGL(scan_block_kernel, dim3((unsigned)nb), dim3(256), 0, st, d_in, n, d_part, d_sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, d_sums, nb, d_total);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, d_part, d_sums, d_total, n, d_ptrs);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}
}  // namespace uspmv_dev

// uspmv_convert_to_scs_device_from_arrays, with the column permutation given explicitly: d_col_perm != NULL is what permute_scs_cols is
// folded in with (the parts of an adaptive-precision split all take the FIRST part's old_to_new, while a fixed-permutation struct's own
// is the identity); NULL: the struct's own old_to_new when permute_cols, none otherwise.
static int convert_from_arrays(const char *who, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                               int64_t nnz, int64_t C, int64_t sigma, int dtype, const int32_t *d_fixed_permutation, int permute_cols,
                               const int32_t *d_col_perm, int sort_mode, void *stream, uspmv_scs_t **layout, int32_t *d_old_to_new,
                               int32_t *d_new_to_old, uspmv_dmat_t **out) {
    if (!out || n_rows < 1 || nnz < 0 || (nnz > 0 && (!d_I || !d_J || !d_V))) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (C < 1 || sigma < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: C and sigma must be >= 1", who);
    if (dtype != USPMV_F64 && dtype != USPMV_F32 && dtype != USPMV_F16) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown dtype %d", who, dtype);
    if (sort_mode != USPMV_SORT_HOST && sort_mode != USPMV_SORT_DEVICE_STABLE) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown sort mode %d", who, sort_mode);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return uspmv::fail(USPMV_ERR_NO_DEVICE, "%s: no HIP device", who); }
    const int64_t n_chunks = (n_rows + C - 1) / C, n_pad = n_chunks * C;
    if (n_pad > INT32_MAX || nnz > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: padded rows / entries exceed int32", who);
    if (sort_mode == USPMV_SORT_DEVICE_STABLE && !d_fixed_permutation && std::min<int64_t>(sigma, n_pad) > 8192)
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: the device-side stable ordering takes sorting scopes of up to 8192 rows (sigma = %lld): use USPMV_SORT_HOST", who, (long long)sigma);
    hipStream_t st = (hipStream_t)stream;
    DeviceBuf<int> start, flag, new_pos, len_new, o2n_own, n2o_own;
    DeviceBuf<long> elems, part, sums, total;
    const long nb = (long)((n_chunks + 1023) / 1024);
    HIP_TRY(start.alloc(4 * ((size_t)n_rows + 1)));
    HIP_TRY(flag.alloc(4));
    HIP_TRY(new_pos.alloc(4 * (size_t)n_pad));
    HIP_TRY(len_new.alloc(4 * (size_t)n_pad));
    HIP_TRY(elems.alloc(8 * (size_t)n_chunks));
    HIP_TRY(part.alloc(8 * (size_t)n_chunks));
    HIP_TRY(sums.alloc(8 * (size_t)nb));
    HIP_TRY(total.alloc(8));
    HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
    HIP_TRY(hipMemsetAsync(len_new, 0, 4 * (size_t)n_pad, st));

    // ---- row populations (code/utilities.hpp:1901-1903)
    hipLaunchKernelGGL(run_bounds_kernel, dim3((unsigned)((nnz + 1 + 255) / 256)), dim3(256), 0, st, d_I, (long)nnz, (int)n_rows, start, flag);
    HIP_TRY(hipGetLastError());

    // ---- where every row goes
    const int32_t *row_map = d_fixed_permutation;           // (what the scatter uses: the caller's permutation, else the ordering's)
    std::vector<int32_t> h_o2n;
    if (d_fixed_permutation) {
        hipLaunchKernelGGL(place_lengths_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, start, d_fixed_permutation, (int)n_rows, (long)n_pad, len_new, flag);
        if (n_pad > n_rows) hipLaunchKernelGGL(zero_tail_kernel, dim3((unsigned)((n_pad - n_rows + 255) / 256)), dim3(256), 0, st, len_new, (int)n_rows, (long)n_pad);
        HIP_TRY(hipGetLastError());
    } else if (sort_mode == USPMV_SORT_DEVICE_STABLE) {
        const int sg = (int)std::min<int64_t>(sigma, n_pad);
        const unsigned nwin = (unsigned)((n_pad + sg - 1) / sg);
        hipLaunchKernelGGL(window_rank_kernel, dim3(nwin), dim3(256), (size_t)sg * 4, st, start, (int)n_rows, (long)n_pad, sg, new_pos, len_new);
        HIP_TRY(hipGetLastError());
        row_map = new_pos;
    } else {
        // the reference's own ordering: std::sort on std::pair<long,long>{row, length} with the comparator a.second > b.second, window by
        // window (code/utilities.hpp:1930-1941), on the host over the COUNTS only -- 4 bytes per row cross the bus each way
        std::vector<int32_t> hs((size_t)n_rows + 1);
        HIP_TRY(hipMemcpyAsync(hs.data(), start, 4 * ((size_t)n_rows + 1), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        using row_len = std::pair<long, long>;
        std::vector<row_len> rl((size_t)(n_pad + sigma));
        for (int64_t i = 0; i < n_pad; ++i) { rl[(size_t)i].first = i; rl[(size_t)i].second = i < n_rows ? hs[(size_t)i + 1] - hs[(size_t)i] : 0; }
        const int64_t n_win = (n_pad + sigma - 1) / sigma;
#pragma omp parallel for schedule(dynamic, 64)
        for (int64_t w = 0; w < n_win; ++w) {
            const int64_t b = w * sigma, e = std::min(b + sigma, n_pad);
            std::sort(rl.begin() + b, rl.begin() + e, [](const row_len &a, const row_len &b2) { return a.second > b2.second; });
        }
        std::vector<int32_t> pos((size_t)n_pad), ln((size_t)n_pad);
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < n_pad; ++i) { pos[(size_t)rl[(size_t)i].first] = (int32_t)i; ln[(size_t)i] = (int32_t)rl[(size_t)i].second; }
        HIP_TRY(hipMemcpyAsync(new_pos, pos.data(), 4 * (size_t)n_pad, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(len_new, ln.data(), 4 * (size_t)n_pad, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));                   // (pos / ln go out of scope)
        row_map = new_pos;
    }

    // ---- chunk lengths and pointers (code/utilities.hpp:1949-1966)
    std::unique_ptr<uspmv_dmat> A(new uspmv_dmat);
    A->C = C; A->n_chunks = n_chunks; A->dtype = dtype; A->n_store = (long)n_pad;
    hipError_t e = A->own.chunk_lengths.alloc(4 * (size_t)n_chunks);
    if (e == hipSuccess) e = A->own.chunk_ptrs.alloc(4 * ((size_t)n_chunks + 1));
    int *cl = A->own.chunk_lengths, *cp = A->own.chunk_ptrs;
    A->chunk_lengths = cl; A->chunk_ptrs = cp;
    if (e != hipSuccess) { return uspmv::fail(USPMV_ERR_ALLOC, "%s: %s", who, hipGetErrorString(e)); }
    hipLaunchKernelGGL(chunk_max_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, st, len_new, (long)n_chunks, (int)C, cl, elems);
    if (int rc = launch_exclusive_scan(elems, (long)n_chunks, part, sums, total, cp, st)) return rc;
    if (d_fixed_permutation)
        hipLaunchKernelGGL(check_fixed_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, start, d_fixed_permutation, cl, (int)n_rows, (int)C, flag);
    long h_total = 0;
    int h_flag = 0;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { return uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }
    if (h_flag & 2) { return uspmv::fail(USPMV_ERR_INVALID, "%s: a row index lies outside [0, n_rows)", who); }
    if (h_flag & 1) { return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: COO entries must be sorted by row (uspmv_read_mtx and the generators produce that order)", who); }
    if (h_flag & 4) return uspmv::fail(USPMV_ERR_INVALID, "%s: fixed_permutation has an entry outside [0, n_rows_padded)", who);
    if (h_flag & 8) return uspmv::fail(USPMV_ERR_INVALID, "%s: fixed_permutation maps a non-empty row onto a padded slot (the reference overruns its chunk here, code/utilities.hpp:1919-1922)", who);
    if (h_total > INT32_MAX) { return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: chunk_ptrs exceed the 32-bit index type", who); }   // (:1959-1962)
    A->n_elements = h_total;

    // ---- permutations, then the scatter (padding: value 0, column 0 -- mapped by permute_scs_cols like any local column, :1820-1826)
    int *o2n = d_old_to_new, *n2o = d_new_to_old;
    if (!o2n) { HIP_TRY(o2n_own.alloc(4 * (size_t)n_rows)); o2n = o2n_own; }
    if (!n2o) { HIP_TRY(n2o_own.alloc(4 * (size_t)n_rows)); n2o = n2o_own; }
    HIP_TRY(hipMemsetAsync(n2o, 0, 4 * (size_t)n_rows, st));
    hipLaunchKernelGGL(perm_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, new_pos, (int)n_rows, d_fixed_permutation != nullptr, o2n, n2o);
    const size_t vsz = uspmv_dtype_bytes(dtype), ne = (size_t)std::max<int64_t>(h_total, 1);
    e = A->own.col_idxs.alloc(4 * ne);
    if (e == hipSuccess) e = A->own.values.alloc(vsz * ne);
    void *ci = A->own.col_idxs, *va = A->own.values;
    A->col_idxs = (const int32_t *)ci; A->values = va;
    const int *col_perm = d_col_perm ? d_col_perm : permute_cols ? o2n : nullptr;
    int pad_col = 0;
    if (e == hipSuccess && col_perm) e = hipMemcpyAsync(&pad_col, col_perm, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && col_perm) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)ci, pad_col, ne, st);
    if (e == hipSuccess) e = hipMemsetAsync(va, 0, vsz * ne, st);
    if (e != hipSuccess) { return uspmv::fail(USPMV_ERR_ALLOC, "%s: %s", who, hipGetErrorString(e)); }
    if (nnz > 0)
        if (int rc = launch_scs_fill(dtype, (long)nnz, (int)C, (int)n_rows, d_I, d_J, d_V, start, row_map, col_perm, cp, (int *)ci, va, st)) { return rc; }

    // ---- optional host struct without entries (meta data, chunk arrays, permutations), as uspmv_convert_to_scs_device returns it
    if (layout) {
        auto *s = new uspmv_scs;
        s->C = C; s->sigma = sigma; s->n_rows = n_rows; s->n_cols = n_cols; s->nnz = nnz; s->n_chunks = n_chunks; s->n_rows_padded = n_pad; s->dtype = dtype;
        s->n_elements = h_total;
        s->chunk_lengths.resize((size_t)n_chunks); s->chunk_ptrs.resize((size_t)n_chunks + 1);
        s->old_to_new_idx.resize((size_t)n_rows); s->new_to_old_idx.resize((size_t)n_rows);
        e = hipMemcpyAsync(s->chunk_lengths.data(), cl, 4 * (size_t)n_chunks, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(s->chunk_ptrs.data(), cp, 4 * ((size_t)n_chunks + 1), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(s->old_to_new_idx.data(), o2n, 4 * (size_t)n_rows, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(s->new_to_old_idx.data(), n2o, 4 * (size_t)n_rows, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { delete s; return uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }
        *layout = s;
    }
    e = hipStreamSynchronize(st);                            // (the scratch of this call is released on return)
    if (e != hipSuccess) { if (layout) { delete *layout; *layout = nullptr; } return uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }
    *out = A.release();
    return USPMV_OK;
}

extern "C" int uspmv_convert_to_scs_device_from_arrays(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                                       int64_t nnz, int64_t C, int64_t sigma, int dtype, const int32_t *d_fixed_permutation,
                                                       int permute_cols, int sort_mode, void *stream, uspmv_scs_t **layout, int32_t *d_old_to_new,
                                                       int32_t *d_new_to_old, uspmv_dmat_t **out) {
    return convert_from_arrays("uspmv_convert_to_scs_device_from_arrays", d_I, d_J, d_V, n_rows, n_cols, nnz, C, sigma, dtype, d_fixed_permutation,
                               permute_cols, nullptr, sort_mode, stream, layout, d_old_to_new, d_new_to_old, out);
}

// ============================================================================ adaptive-precision set-up from device-resident COO arrays
// (struct uspmv_dcoo, one part of uspmv_partition_precisions_device: uspmv_device.hpp)
namespace {

bool ap_kind_known(int kind) { return kind == USPMV_AP_DP_HP || kind == USPMV_AP_SP_HP || kind == USPMV_AP_DP_SP_HP || kind == USPMV_AP_DP_SP; }

// the three passes (csrc/ap_partition_kernels.hip); the caller has checked the arguments and the device.  Nothing is written to a part
// before the index checks and the NaN check of pass (a) have come back clean.  d_row_max / d_col_max: the equilibrated branch (both NULL:
// the unscaled one).
int partition_device(const char *who, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols, int64_t nnz,
                     int kind, double t1, double t2, const double *d_row_max, const double *d_col_max, hipStream_t st,
                     std::unique_ptr<uspmv_dcoo> parts[3]) {
    const bool three = kind == USPMV_AP_DP_SP_HP;
    const long n_wg = ap_partition_workgroups((long)nnz), n_cnt = 3 * n_wg;
    int32_t h_base[4] = {0, 0, 0, 0};                     // where the parts start in the scan, and the total
    if (n_wg > 0) {
        DeviceBuf<long> counts, part, sums, total;
        DeviceBuf<int> base, flag;
        DeviceBuf<unsigned long long> first_nan;
        HIP_TRY(counts.alloc(8 * (size_t)n_cnt));
        HIP_TRY(part.alloc(8 * (size_t)n_cnt));
        HIP_TRY(sums.alloc(8 * (size_t)((n_cnt + 1023) / 1024)));
        HIP_TRY(total.alloc(8));
        HIP_TRY(base.alloc(4 * ((size_t)n_cnt + 1)));
        HIP_TRY(flag.alloc(4));
        HIP_TRY(first_nan.alloc(8));
        HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
        HIP_TRY(hipMemsetAsync(first_nan, 0xFF, 8, st));
        if (int rc = launch_ap_partition_count(d_I, d_J, d_V, (long)nnz, (int)n_rows, (int)n_cols, kind, t1, t2, counts, flag, first_nan, st, d_row_max, d_col_max)) return rc;
        if (int rc = launch_exclusive_scan(counts, n_cnt, part, sums, total, base, st)) return rc;
        int h_flag = 0;
        unsigned long long h_nan = 0;
        HIP_TRY(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&h_nan, first_nan, 8, hipMemcpyDeviceToHost, st));
        for (int p = 0; p < 4; ++p) HIP_TRY(hipMemcpyAsync(&h_base[p], (int *)base + (size_t)p * n_wg, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_flag & 2) return uspmv::fail(USPMV_ERR_INVALID, "%s: a row index lies outside [0, n_rows)", who);
        if (h_flag & 4) return uspmv::fail(USPMV_ERR_INVALID, "%s: a column index lies outside [0, n_cols)", who);
        if (h_flag & 1) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: COO entries must be sorted by row (uspmv_read_mtx and the generators produce that order)", who);
        if (h_nan != ~0ull) return uspmv::fail(USPMV_ERR_INVALID, "%s: element %lld fits neither struct", who, (long long)h_nan);
        ApPartOut o{};
        for (int p = 0; p < 3; ++p) {
            if (p == 1 && !three) continue;
            parts[p].reset(new uspmv_dcoo);
            const size_t n = (size_t)(h_base[p + 1] - h_base[p]);
            parts[p]->nnz = (int64_t)n;
            HIP_TRY(parts[p]->I.alloc(4 * n));
            HIP_TRY(parts[p]->J.alloc(4 * n));
            HIP_TRY(parts[p]->V.alloc(8 * n));
            o.I[p] = parts[p]->I; o.J[p] = parts[p]->J; o.V[p] = parts[p]->V; o.n[p] = (long)n;
        }
        if (int rc = launch_ap_partition_scatter(d_I, d_J, d_V, (long)nnz, kind, t1, t2, base, o, st, d_row_max, d_col_max)) return rc;
        HIP_TRY(hipStreamSynchronize(st));               // (the scratch of this call is released on return)
    } else {
        for (int p = 0; p < 3; ++p)
            if (p != 1 || three) parts[p].reset(new uspmv_dcoo);
    }
    return USPMV_OK;
}

int ap_common_args(const char *who, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols, int64_t nnz, int kind) {
    if (nnz < 0 || (nnz > 0 && (!d_I || !d_J || !d_V))) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (!ap_kind_known(kind)) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown kind %d", who, kind);
    if (n_rows < 1 || n_cols < 0) return uspmv::fail(USPMV_ERR_INVALID, "%s: matrix has no rows", who);
    return USPMV_OK;
}

}  // namespace

static int partition_precisions_device(const char *who, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                       int64_t nnz, int kind, double threshold_1, double threshold_2, const double *d_row_max,
                                       const double *d_col_max, void *stream, uspmv_dcoo_t *parts[3]) {
    if (!parts) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = ap_common_args(who, d_I, d_J, d_V, n_rows, n_cols, nnz, kind)) return rc;
    if (int rc = require_device()) return rc;
    if (n_rows > INT32_MAX || n_cols > INT32_MAX || nnz > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: rows / columns / entries exceed int32", who);
    std::unique_ptr<uspmv_dcoo> p[3];
    if (int rc = partition_device(who, d_I, d_J, d_V, n_rows, n_cols, nnz, kind, threshold_1, threshold_2, d_row_max, d_col_max, (hipStream_t)stream, p)) return rc;
    for (int k = 0; k < 3; ++k) parts[k] = p[k].release();
    return USPMV_OK;
}

extern "C" int uspmv_partition_precisions_device(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                                 int kind, double threshold_1, double threshold_2, void *stream, uspmv_dcoo_t *parts[3]) {
    return partition_precisions_device("uspmv_partition_precisions_device", d_I, d_J, d_V, n_rows, n_cols, nnz, kind, threshold_1, threshold_2, nullptr,
                                       nullptr, stream, parts);
}

extern "C" int uspmv_partition_precisions_device_eq(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                                    int kind, double threshold_1, double threshold_2, const double *d_row_max, const double *d_col_max,
                                                    void *stream, uspmv_dcoo_t *parts[3]) {
    const char *who = "uspmv_partition_precisions_device_eq";
    if (!d_row_max || !d_col_max) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    return partition_precisions_device(who, d_I, d_J, d_V, n_rows, n_cols, nnz, kind, threshold_1, threshold_2, d_row_max, d_col_max, stream, parts);
}

extern "C" int uspmv_dcoo_arrays(const uspmv_dcoo_t *p, const int32_t **d_I, const int32_t **d_J, const double **d_V, int64_t *nnz) {
    if (!p) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dcoo_arrays: NULL part");
    if (d_I) *d_I = p->I;
    if (d_J) *d_J = p->J;
    if (d_V) *d_V = p->V;
    if (nnz) *nnz = p->nnz;
    return USPMV_OK;
}

extern "C" int uspmv_dcoo_copy(const uspmv_dcoo_t *p, int32_t *d_I, int32_t *d_J, double *d_V, void *stream) {
    if (!p) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dcoo_copy: NULL part");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)p->nnz;
    if (n && d_I) HIP_TRY(hipMemcpyAsync(d_I, p->I, 4 * n, hipMemcpyDeviceToDevice, st));
    if (n && d_J) HIP_TRY(hipMemcpyAsync(d_J, p->J, 4 * n, hipMemcpyDeviceToDevice, st));
    if (n && d_V) HIP_TRY(hipMemcpyAsync(d_V, p->V, 8 * n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return USPMV_OK;
}

extern "C" void uspmv_dcoo_free(uspmv_dcoo_t *p) { delete p; }

// uspmv_convert_to_scs_device_ap_from_arrays[_eq]: one body, the unscaled function with both vectors NULL
static int convert_ap_from_arrays(const char *who, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                  int64_t nnz, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2,
                                  const double *d_row_max, const double *d_col_max, int sort_mode, void *stream, uspmv_scs_t **layout,
                                  int32_t *d_old_to_new, int32_t *d_new_to_old, int64_t part_nnz[3], uspmv_dmat_t **hi, uspmv_dmat_t **mid,
                                  uspmv_dmat_t **lo) {
    if (int rc = ap_common_args(who, d_I, d_J, d_V, n_rows, n_cols, nnz, kind)) return rc;
    const bool three = kind == USPMV_AP_DP_SP_HP;
    if (!hi || !lo || (three && !mid)) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL output for a part the kind has", who);
    if (C < 1 || sigma < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: C and sigma must be >= 1", who);
    if (sort_mode != USPMV_SORT_HOST && sort_mode != USPMV_SORT_DEVICE_STABLE) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown sort mode %d", who, sort_mode);
    if (int rc = require_device()) return rc;
    const int64_t n_pad = (n_rows + C - 1) / C * C;
    if (n_pad > INT32_MAX || n_cols > INT32_MAX || nnz > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: padded rows / columns / entries exceed int32", who);
    if (sort_mode == USPMV_SORT_DEVICE_STABLE && std::min<int64_t>(sigma, n_pad) > 8192)
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: the device-side stable ordering takes sorting scopes of up to 8192 rows (sigma = %lld): use USPMV_SORT_HOST", who, (long long)sigma);
    hipStream_t st = (hipStream_t)stream;
    std::unique_ptr<uspmv_dcoo> p[3];
    if (int rc = partition_device(who, d_I, d_J, d_V, n_rows, n_cols, nnz, kind, threshold_1, threshold_2, d_row_max, d_col_max, st, p)) return rc;

    // the first part orders the rows; the others take its permutation for their rows AND for their columns (what uspmv_main.cpp and the
    // host tests do with uspmv_convert_to_scs(fixed_permutation) + uspmv_permute_scs_cols(first part's old_to_new))
    struct Free { void operator()(uspmv_dmat_t *m) const { uspmv_dmat_free(m); } };
    std::unique_ptr<uspmv_dmat_t, Free> A[3];
    std::unique_ptr<uspmv_scs> lay;
    DeviceBuf<int32_t> o2n_own;
    int32_t *o2n = d_old_to_new;
    if (!o2n) { HIP_TRY(o2n_own.alloc(4 * (size_t)n_rows)); o2n = o2n_own; }
    const int dtypes[3] = {kind == USPMV_AP_SP_HP ? USPMV_F32 : USPMV_F64, USPMV_F32, kind == USPMV_AP_DP_SP ? USPMV_F32 : USPMV_F16};
    int64_t cnt[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        if (!p[k]) continue;
        cnt[k] = p[k]->nnz;
        uspmv_dmat_t *h = nullptr;
        uspmv_scs_t *l = nullptr;
        const int rc = convert_from_arrays(who, p[k]->I, p[k]->J, p[k]->V, n_rows, n_cols, p[k]->nnz, C, sigma, dtypes[k], k == 0 ? nullptr : o2n, 1,
                                           k == 0 ? nullptr : o2n, sort_mode, stream, k == 0 && layout ? &l : nullptr, k == 0 ? o2n : nullptr,
                                           k == 0 ? d_new_to_old : nullptr, &h);
        if (rc) return rc;                                // (what was built so far is released by its owner)
        A[k].reset(h);
        if (k == 0) lay.reset(l);
        p[k].reset();                                     // the part's COO copy is not needed any longer
    }
    if (layout) *layout = lay.release();
    if (part_nnz) { part_nnz[0] = cnt[0]; part_nnz[1] = cnt[1]; part_nnz[2] = cnt[2]; }
    *hi = A[0].release();
    if (mid) *mid = A[1].release();
    *lo = A[2].release();
    return USPMV_OK;
}

extern "C" int uspmv_convert_to_scs_device_ap_from_arrays(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                                          int64_t nnz, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2,
                                                          int sort_mode, void *stream, uspmv_scs_t **layout, int32_t *d_old_to_new,
                                                          int32_t *d_new_to_old, int64_t part_nnz[3], uspmv_dmat_t **hi, uspmv_dmat_t **mid,
                                                          uspmv_dmat_t **lo) {
    return convert_ap_from_arrays("uspmv_convert_to_scs_device_ap_from_arrays", d_I, d_J, d_V, n_rows, n_cols, nnz, C, sigma, kind, threshold_1,
                                  threshold_2, nullptr, nullptr, sort_mode, stream, layout, d_old_to_new, d_new_to_old, part_nnz, hi, mid, lo);
}

extern "C" int uspmv_convert_to_scs_device_ap_from_arrays_eq(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                                             int64_t nnz, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2,
                                                             const double *d_row_max, const double *d_col_max, int sort_mode, void *stream,
                                                             uspmv_scs_t **layout, int32_t *d_old_to_new, int32_t *d_new_to_old, int64_t part_nnz[3],
                                                             uspmv_dmat_t **hi, uspmv_dmat_t **mid, uspmv_dmat_t **lo) {
    const char *who = "uspmv_convert_to_scs_device_ap_from_arrays_eq";
    if ((d_row_max == nullptr) != (d_col_max == nullptr)) return uspmv::fail(USPMV_ERR_INVALID, "%s: one of the two divisor vectors is NULL", who);
    return convert_ap_from_arrays(who, d_I, d_J, d_V, n_rows, n_cols, nnz, C, sigma, kind, threshold_1, threshold_2, d_row_max, d_col_max, sort_mode,
                                  stream, layout, d_old_to_new, d_new_to_old, part_nnz, hi, mid, lo);
}
