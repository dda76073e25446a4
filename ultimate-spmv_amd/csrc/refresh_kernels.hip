// Numeric refresh: new values on an unchanged pattern, plans kept.  uspmv_dmat_update_values_from_arrays places the
// values of row-sorted COO arrays in HBM into a handle's SELL-C-sigma value array -- checks first, through flag words, nothing written
// before they come back clean -- and uspmv_dmat_values_changed brings every plan on the handle back in line with that array.  Which
// plan family keeps which private copy of the values is written ONCE, in refresh_plans below; the planners stay as they are.
//
// Kernels (no atomics beyond the flag words, none waits on another workgroup):
//   refresh_bounds_kernel   start[r] = first entry of row r, as run_bounds_kernel of convert_kernels.hip, but a row index outside
//                           [0, n_rows) on EITHER side of a run boundary ends the thread before it writes (no start[-4] for I[k] = -3)
//   refresh_rows_kernel     per row: its position inside the padded rows, its population against the chunk length there; writes the
//                           inverse of the row positions (row_at[position] = row, -1 for a position no row takes)
//   refresh_check_kernel    per padded position: the stored column of every entry against the (permuted) J; per row: two rows on one position
//   refresh_place_kernel    per padded position, slot after slot: the row's j-th value, +0 beyond its entries.  Every slot of the array is
//                           written exactly once (no memset), the stores of a chunk's rows are consecutive; columns are not touched.
//                           (Measured against one thread per COO entry behind a memset, the form of scs_fill_kernel: 3.8 against 5.0 ms
//                           per call on the 253^3 stencil, 4.9 against 6.5 on 111^3 x 3 dof; profiles/value_refresh.  This form was kept.)
//   refresh_rechunk_kernel  the values of rechunk32_kernel (plan_kernels.hip) without its columns: the internal C = 32 copy of a narrow struct
#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace {

enum : int { F_UNSORTED = 1, F_ROW = 2, F_POS = 4, F_LONG = 8, F_TWICE = 16, F_COL = 32 };

__global__ void __launch_bounds__(256) refresh_bounds_kernel(const int *__restrict__ I, const long nnz, const int n_rows, int *__restrict__ start,
                                                             int *__restrict__ flag) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nnz) return;
    const int prev = k == 0 ? -1 : I[k - 1];
    const int cur = k == nnz ? n_rows : I[k];
    if ((k < nnz && (cur < 0 || cur >= n_rows)) || (k > 0 && (prev < 0 || prev >= n_rows))) { atomicOr(flag, F_ROW); return; }
    if (cur < prev) { atomicOr(flag, F_UNSORTED); return; }
    for (int r = prev + 1; r <= cur; ++r) start[r] = (int)k;      // r in [0, n_rows]: both ends were checked above
}

// (every later kernel leaves at once when a flag is up: start[] has holes then)
__global__ void __launch_bounds__(256) refresh_rows_kernel(const int *__restrict__ start, const int *__restrict__ row_pos, const int n_rows, const long n_pad,
                                                           const int C, const int *__restrict__ chunk_lengths, int *__restrict__ row_at,
                                                           int *__restrict__ flag) {
    if (*(volatile int *)flag) return;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const long p = row_pos ? (long)row_pos[i] : i;
    if (p < 0 || p >= n_pad) { atomicOr(flag, F_POS); return; }
    if (start[i + 1] - start[i] > chunk_lengths[p / C]) atomicOr(flag, F_LONG);
    row_at[p] = (int)i;
}

template <bool COLS>
__global__ void __launch_bounds__(256) refresh_check_kernel(const int *__restrict__ J, const int *__restrict__ start, const int *__restrict__ row_pos,
                                                            const int *__restrict__ row_at, const int n_rows, const long n_pad, const int C,
                                                            const int *__restrict__ chunk_ptrs, const int *__restrict__ col_idxs,
                                                            const int *__restrict__ col_perm, int *__restrict__ flag,
                                                            unsigned long long *__restrict__ first_bad) {
    if (*(volatile int *)flag & (F_UNSORTED | F_ROW | F_POS | F_LONG)) return;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pad) return;
    if (q < n_rows && row_at[row_pos ? (long)row_pos[q] : q] != (int)q) atomicOr(flag, F_TWICE);
    if (!COLS) return;
    const int r = row_at[q];
    if (r < 0) return;
    const long c = q / C;
    const long dst = (long)chunk_ptrs[c] + (q - c * C);
    const int s0 = start[r], n = start[r + 1] - s0;
    for (int j = 0; j < n; ++j) {
        int col = J[s0 + j];
        if (col_perm && col >= 0 && col < n_rows) col = col_perm[col];
        if (col_idxs[dst + (long)j * C] != col) {
            atomicOr(flag, F_COL);
            atomicMin(first_bad, (unsigned long long)(s0 + j));
            return;
        }
    }
}

template <typename VT>
__global__ void __launch_bounds__(256) refresh_place_kernel(const double *__restrict__ V, const int *__restrict__ start, const int *__restrict__ row_at,
                                                            const long n_pad, const int C, const int *__restrict__ chunk_ptrs,
                                                            const int *__restrict__ chunk_lengths, VT *__restrict__ values) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pad) return;
    const long c = q / C;
    VT *__restrict__ out = values + (long)chunk_ptrs[c] + (q - c * C);
    const int L = chunk_lengths[c];
    const int r = row_at[q];
    const int s0 = r >= 0 ? start[r] : 0;
    const int n = r >= 0 ? min(start[r + 1] - s0, L) : 0;
    const double *__restrict__ v = V + s0;
    int j = 0;
#pragma unroll 4
    for (; j < n; ++j) out[(long)j * C] = (VT)v[j];               // (float)v for F32, as scs_fill_value rounds
    for (; j < L; ++j) out[(long)j * C] = (VT)0;                  // +0; the slot keeps its stored column, like padding
}

template <typename VT>
__global__ void __launch_bounds__(256) refresh_rechunk_kernel(const long n_rows_old, const int C, const int *__restrict__ cp_old,
                                                              const int *__restrict__ cl_old, const VT *__restrict__ va_old,
                                                              const int *__restrict__ cp_new, VT *__restrict__ va_new) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows_old) return;
    const long co = row / C;
    const VT *__restrict__ in = va_old + (long)cp_old[co] + (row - co * C);
    VT *__restrict__ out = va_new + (long)cp_new[row >> 5] + (row & 31);
    const int L = cl_old[co];
#pragma unroll 4
    for (int j = 0; j < L; ++j) out[(long)j * 32] = in[(long)j * C];
}

bool owns_values(const uspmv_dmat *A) { return A->own.values.get() != nullptr && A->values == (const void *)A->own.values.get(); }

// What every entry point refuses before a device is looked for.
int refresh_refusals(const uspmv_dmat *A, const char *who) {
    if (int rc = check_dmat(A, who)) return rc;
    if (A->dtype == USPMV_F16)
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: fp16 handle (the hp part of an adaptive-precision split: new values move entries between the parts; "
                                                  "set the split up again with uspmv_convert_to_scs_device_ap_from_arrays)", who);
    for (const uspmv_dmat *M = A; M; M = M->alt)
        if ((M->tlc.on && M->tlc.plan_id != 0) || (M->sw.on && (M->sw.n_parts > 1 || !M->sw.tile_ids)))
            return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: the handle carries the shared plan of an adaptive-precision split (new values move entries between "
                                                      "the parts; set the split up again with uspmv_convert_to_scs_device_ap_from_arrays)", who);
    return USPMV_OK;
}

// THE rule "which plan has which copy of the values" (uspmv_dmat, uspmv_device.hpp).  Line, element, 12-bit and additive-record plans on
// the caller's row order hold indices only: their kernels read A->values in place.
int refresh_plans(uspmv_dmat *A, hipStream_t st, int *actions, const char *who) {
    if (A->n_chunks == 0) return USPMV_OK;
    // the internal C = 32 re-chunking of a narrow struct (crs included): its value array, then whatever plans IT carries
    if (uspmv_dmat *alt = A->alt) {
        const long n_rows = (long)(A->n_chunks * A->C);
        if (A->dtype == USPMV_F64)
            hipLaunchKernelGGL(refresh_rechunk_kernel<double>, dim3(grid_for(n_rows, 256)), dim3(256), 0, st, n_rows, (int)A->C, A->chunk_ptrs, A->chunk_lengths,
                               (const double *)A->values, alt->chunk_ptrs, (double *)alt->own.values.get());
        else
            hipLaunchKernelGGL(refresh_rechunk_kernel<float>, dim3(grid_for(n_rows, 256)), dim3(256), 0, st, n_rows, (int)A->C, A->chunk_ptrs, A->chunk_lengths,
                               (const float *)A->values, alt->chunk_ptrs, (float *)alt->own.values.get());
        HIP_TRY(hipGetLastError());
        *actions |= USPMV_REFRESH_RECHUNKED;
        if (int rc = refresh_plans(alt, st, actions, who)) return rc;
    }
    // private copies under a row map: the element plan on rows dealt to the tiles, the list plan's re-ordered copy, the phased plan's
    // group-major copy (shared by the line plan, the unscrambled plan and the stream schedule) -- gathered exactly as the planners do
    if (A->tlc.on && A->tlc.values) {
        if (int rc = launch_block_values_gather(A, A->tlc.row_map, nullptr, A->tlc.values, false, st)) return rc;
        *actions |= USPMV_REFRESH_COPIES;
    }
    if (A->bt.values) {
        if (int rc = launch_block_values_gather(A, A->bt.row_map, nullptr, A->bt.values, false, st)) return rc;
        *actions |= USPMV_REFRESH_COPIES;
    }
    if (A->pb.on && A->pb.values) {
        if (int rc = launch_block_values_gather(A, A->bt.row_map, A->pb.c16_ptrs, A->pb.values, true, st)) return rc;
        *actions |= USPMV_REFRESH_COPIES;
    }
    // the block-vector sweep plan strips trailing (+0, last column) runs like the sweep plan below and has no device builder: released;
    // uspmv_spmmv answers from whatever block plan remains, or from the gather kernel
    if (A->bw.on) {
        HIP_TRY(hipStreamSynchronize(st));                       // (a product still reading the plan)
        A->bw = {};
        *actions |= USPMV_REFRESH_BLOCK_SWEEP_DROPPED;
    }
    // the column-window sweep plan: the SHAPE of its compacted stream depends on the values (effective_len, host/sweep_plan.cpp) --
    // rebuilt by the device builder (the host builder's equal, bit for bit) at the installed window and rows per tile
    if (A->sw.on) {
        const int wlog = A->sw.wlog, tile_rows = A->sw.tile_rows;
        HIP_TRY(hipStreamSynchronize(st));                       // (the builder works on the null stream and replaces the arrays)
        uspmv_dmat *parts[1] = {A};
        if (int rc = sweep_plan_install_device(parts, 1, wlog, tile_rows, nullptr, nullptr, who)) return rc;
        *actions |= USPMV_REFRESH_SWEEP_REBUILT;
    }
    return USPMV_OK;
}

int values_changed(uspmv_dmat *A, hipStream_t st, int *actions, const char *who) {
    int acts = 0;
    const int rc = refresh_plans(A, st, &acts, who);
    if (actions) *actions = acts;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return USPMV_OK;
}

}  // namespace

extern "C" {

int uspmv_dmat_values_changed(uspmv_dmat_t *A, void *stream, int *actions) {
    const char *who = "uspmv_dmat_values_changed";
    if (actions) *actions = 0;
    if (!A) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = refresh_refusals(A, who)) return rc;
    if (int rc = require_device()) return rc;
    return values_changed(A, (hipStream_t)stream, actions, who);
}

int uspmv_dmat_update_values(uspmv_dmat_t *A, const void *values, void *stream, int *actions) {
    const char *who = "uspmv_dmat_update_values";
    if (actions) *actions = 0;
    if (!A || !values) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = refresh_refusals(A, who)) return rc;
    if (!owns_values(A))
        return uspmv::fail(USPMV_ERR_INVALID, "%s: the handle wraps the caller's arrays (uspmv_dmat_wrap): write the value array and call uspmv_dmat_values_changed", who);
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (A->n_elements > 0) {
        HIP_TRY(hipMemcpyAsync(A->own.values.get(), values, uspmv_dtype_bytes(A->dtype) * (size_t)A->n_elements, hipMemcpyDefault, st));
        HIP_TRY(hipStreamSynchronize(st));                       // (a pageable host source may be gone when the caller returns)
    }
    return values_changed(A, st, actions, who);
}

int uspmv_dmat_update_values_from_arrays(uspmv_dmat_t *A, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t nnz,
                                         const int32_t *d_row_pos, const int32_t *d_col_perm, int check_pattern, void *d_values_dst, void *stream,
                                         int *actions) {
    const char *who = "uspmv_dmat_update_values_from_arrays";
    if (actions) *actions = 0;
    if (!A || nnz < 0 || (nnz > 0 && (!d_I || !d_V)) || (nnz > 0 && check_pattern && !d_J)) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = refresh_refusals(A, who)) return rc;
    if (!d_values_dst && !owns_values(A))
        return uspmv::fail(USPMV_ERR_INVALID, "%s: the handle wraps the caller's arrays (uspmv_dmat_wrap): pass the writable pointer to the wrapped value array as "
                                              "d_values_dst, or write the array and call uspmv_dmat_values_changed", who);
    if (d_values_dst && d_values_dst != A->values)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: d_values_dst is not the value array of the handle", who);
    if (n_rows < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: matrix has no rows", who);
    if ((n_rows + A->C - 1) / A->C != A->n_chunks)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: %lld rows make %lld chunks of %lld, the handle has %lld (the pattern changed)", who, (long long)n_rows,
                           (long long)((n_rows + A->C - 1) / A->C), (long long)A->C, (long long)A->n_chunks);
    if (nnz > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: entries exceed int32", who);
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long n_pad = (long)(A->n_chunks * A->C);
    const int C = (int)A->C;
    void *dst = d_values_dst ? d_values_dst : (void *)A->own.values.get();

    // ---- checks: nothing is written to the values before the flags come back clean
    DeviceBuf<int> start, row_at, flag;
    HIP_TRY(start.alloc(4 * ((size_t)n_rows + 1)));
    HIP_TRY(row_at.alloc(4 * (size_t)n_pad));
    HIP_TRY(flag.alloc(16));
    unsigned long long *first_bad = (unsigned long long *)(flag.get() + 2);
    HIP_TRY(hipMemsetAsync(flag, 0, 8, st));
    HIP_TRY(hipMemsetAsync(first_bad, 0xFF, 8, st));
    HIP_TRY(hipMemsetAsync(row_at, 0xFF, 4 * (size_t)n_pad, st));
    hipLaunchKernelGGL(refresh_bounds_kernel, dim3(grid_for(nnz + 1, 256)), dim3(256), 0, st, d_I, (long)nnz, (int)n_rows, start.get(), flag.get());
    hipLaunchKernelGGL(refresh_rows_kernel, dim3(grid_for(n_rows, 256)), dim3(256), 0, st, start.get(), d_row_pos, (int)n_rows, n_pad, C, A->chunk_lengths,
                       row_at.get(), flag.get());
    if (check_pattern)
        hipLaunchKernelGGL(refresh_check_kernel<true>, dim3(grid_for(n_pad, 256)), dim3(256), 0, st, d_J, start.get(), d_row_pos, row_at.get(), (int)n_rows, n_pad, C,
                           A->chunk_ptrs, A->col_idxs, d_col_perm, flag.get(), first_bad);
    else
        hipLaunchKernelGGL(refresh_check_kernel<false>, dim3(grid_for(n_pad, 256)), dim3(256), 0, st, d_J, start.get(), d_row_pos, row_at.get(), (int)n_rows, n_pad, C,
                           A->chunk_ptrs, A->col_idxs, d_col_perm, flag.get(), first_bad);
    HIP_TRY(hipGetLastError());
    int h_flag[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_flag, flag, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int f = h_flag[0];
    if (f & F_ROW) return uspmv::fail(USPMV_ERR_INVALID, "%s: a row index lies outside [0, n_rows)", who);
    if (f & F_UNSORTED) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: COO entries must be sorted by row (uspmv_read_mtx and the generators produce that order)", who);
    if (f & F_POS) return uspmv::fail(USPMV_ERR_INVALID, "%s: row_pos has an entry outside [0, n_rows_padded)", who);
    if (f & F_LONG) return uspmv::fail(USPMV_ERR_INVALID, "%s: a row has more entries than the chunk it sits in is long (the pattern changed)", who);
    if (f & F_TWICE) return uspmv::fail(USPMV_ERR_INVALID, "%s: row_pos sends two rows to one position", who);
    if (f & F_COL) {
        unsigned long long k = 0;
        memcpy(&k, h_flag + 2, 8);
        return uspmv::fail(USPMV_ERR_INVALID, "%s: entry %lld: its column differs from the stored one (the pattern changed)", who, (long long)k);
    }

    // ---- placement
    if (A->dtype == USPMV_F64)
        hipLaunchKernelGGL(refresh_place_kernel<double>, dim3(grid_for(n_pad, 256)), dim3(256), 0, st, d_V, start.get(), row_at.get(), n_pad, C, A->chunk_ptrs,
                           A->chunk_lengths, (double *)dst);
    else
        hipLaunchKernelGGL(refresh_place_kernel<float>, dim3(grid_for(n_pad, 256)), dim3(256), 0, st, d_V, start.get(), row_at.get(), n_pad, C, A->chunk_ptrs,
                           A->chunk_lengths, (float *)dst);
    HIP_TRY(hipGetLastError());

    // ---- refresh (returns behind a synchronise: the scratch of this call is released on return)
    return values_changed(A, st, actions, who);
}

}  // extern "C"
