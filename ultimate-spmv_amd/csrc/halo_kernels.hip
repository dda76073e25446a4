// Halo discovery and chunk classification ON THE DEVICE, for handles whose entries never visit the host: what
// discover_halo + uspmv_permute_scs_cols and uspmv_scs_classify_chunks (host/halo_plan.cpp) do to a host struct, done to the device arrays of
// handles converted with permute_cols = 0 (GLOBAL column ids).  Reference: collect_local_needed_heri, code/mpi_funcs.hpp:242-415.
//
// The serial scan numbers a remote column when it first SEES it, walking col_idxs in storage order, part after part.  In parallel:
//   first-seen position of a column  = min over the entries that name it of key = (part << 32 | storage index)
//   slot of a column inside its owner = its rank under that key among the owner's columns
// so one 64-bit atomicMin per (new) column into a dense table of keys, a compaction of the claimed entries, a sort of the n_halo records
// by (owner, key) on the host -- O(n_halo) records cross, the licence USPMV_SORT_HOST takes for row counts -- and one rewrite pass.
//   halo_claim_kernel     keys into the table; a column outside the table is reported by the least key that names one (the serial scan's
//                         first), nothing has been written by then
//   halo_count / _compact the claimed table entries as (key, column) records, in any order
//   halo_scatter_kernel   table[column] = final local index (n_local + base[owner] + slot)
//   halo_rewrite_kernel   col_idxs in place: local columns through the permutation, remote ones through the table
// No kernel waits on another workgroup; nothing spins.
// Contention: every padding entry of a rank > 0 names global column 0 -- on the sparse part of a split a large share of all entries on ONE
// table address.  Keys only fall, so an entry first READS the table and leaves when the key there is already at or below its own (a stale
// read only costs a redundant atomic), and the lanes of a wave that still want the same column send one atomic, the lowest lane's (within
// a wave the storage index rises with the lane, so that is the least key).
#include "uspmv_device.hpp"

#include <memory>
#include <vector>

using namespace uspmv_dev;

namespace {

typedef unsigned long long u64;
constexpr u64 NO_KEY = ~0ull;

struct HaloRec { u64 key; int col; int fin; };   // a claimed column: its first-seen key; fin = its local index once the host has ordered them

__global__ void __launch_bounds__(256) halo_claim_kernel(const int *__restrict__ ci, const long n_el, const u64 part_bits, const int lo, const int hi,
                                                         const long table_len, u64 *__restrict__ table, u64 *__restrict__ bad) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const u64 key = part_bits | (u64)k;
    int col = -1;
    bool want = false;
    if (k < n_el) {
        col = ci[k];
        if (col < 0 || col >= table_len) atomicMin(bad, key);
        else if (col < lo || col >= hi) want = table[col] > key;
    }
    // one atomic per distinct column of the wave (every lane of the wave walks this loop: no early return above)
    u64 todo = __ballot(want);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lcol = __shfl(col, leader);
        const bool same = want && col == lcol;
        const u64 group = __ballot(same);
        if (lane == leader) atomicMin(&table[col], key);
        want = want && !same;
        todo &= ~group;
    }
}

// the claimed entries of the table: counted (one atomic per wave), then written as records at positions drawn the same way
__global__ void __launch_bounds__(256) halo_count_kernel(const u64 *__restrict__ table, const long table_len, u64 *__restrict__ n_claimed) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const u64 m = __ballot(c < table_len && table[c] != NO_KEY);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_claimed, (u64)__popcll(m));
}
__global__ void __launch_bounds__(256) halo_compact_kernel(const u64 *__restrict__ table, const long table_len, const long cap, u64 *__restrict__ cursor,
                                                           HaloRec *__restrict__ rec) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const u64 key = c < table_len ? table[c] : NO_KEY;
    const u64 m = __ballot(key != NO_KEY);
    u64 base = 0;
    if (lane == 0 && m) base = atomicAdd(cursor, (u64)__popcll(m));
    base = __shfl(base, 0);
    if (key == NO_KEY) return;
    const long at = (long)(base + (u64)__popcll(m & ((1ull << lane) - 1)));
    if (at < cap) rec[at] = HaloRec{key, (int)c, 0};      // (cap = the count of halo_count_kernel: nothing claims in between)
}

__global__ void halo_scatter_kernel(const HaloRec *__restrict__ rec, const long n, u64 *__restrict__ table) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) table[rec[i].col] = (u64)(unsigned)rec[i].fin;
}

__global__ void halo_rewrite_kernel(int *__restrict__ ci, const long n_el, const int lo, const int hi, const int *__restrict__ perm,
                                    const u64 *__restrict__ table) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_el) return;
    const int col = ci[k];
    ci[k] = col >= lo && col < hi ? (perm ? perm[col - lo] : col - lo) : (int)table[col];   // (every column was range-checked by the claim pass)
}

// ---- chunk classes (uspmv_scs_classify_chunks): one wave per chunk, four chunks per workgroup
template <typename BT>
__device__ inline bool pos_zero(const void *values, long k) { return ((const BT *)values)[k] == 0; }   // +0.0 by its bits

// the padding column: the lowest halo column that carries a +0.0 entry
template <typename BT>
__global__ void __launch_bounds__(256) pad_col_kernel(const int *__restrict__ chunk_ptrs, const int *__restrict__ chunk_lengths, const int *__restrict__ ci,
                                                      const void *__restrict__ values, const long n_chunks, const int C, const int n_local, int *__restrict__ h0) {
    const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    int best = INT32_MAX;
    if (c < n_chunks) {
        const long b = chunk_ptrs[c], e = b + (long)chunk_lengths[c] * C;
        for (long k = b + lane; k < e; k += 64) {
            const int col = ci[k];
            if (col >= n_local && col < best && pos_zero<BT>(values, k)) best = col;
        }
    }
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if (lane == 0 && best != INT32_MAX) atomicMin(h0, best);
}

template <typename BT>
__global__ void __launch_bounds__(256) chunk_class_kernel(const int *__restrict__ chunk_ptrs, const int *__restrict__ chunk_lengths, const int *__restrict__ ci,
                                                          const void *__restrict__ values, const long n_chunks, const int C, const int n_local,
                                                          const int *__restrict__ h0p, unsigned char *__restrict__ cls) {
    const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int h0 = *h0p;
    int f = 0;
    if (c < n_chunks) {
        const long b = chunk_ptrs[c], e = b + (long)chunk_lengths[c] * C;
        for (long k = b + lane; k < e; k += 64) {
            const int col = ci[k];
            if (col >= n_local) f = max(f, col == h0 && pos_zero<BT>(values, k) ? 1 : 2);
        }
    }
    for (int o = 32; o > 0; o >>= 1) f = max(f, __shfl_xor(f, o));
    if (lane == 0 && c < n_chunks) cls[c] = (unsigned char)f;
}

bool carries_plan(const uspmv_dmat *A) { return A->tlc.on || A->bt.on || A->pb.on || A->pl.on || A->pu.on || A->bw.on || A->sw.on || A->ps.grid > 0; }

}  // namespace

extern "C" int uspmv_halo_discover_device(uspmv_dmat_t *const parts[], int n_parts, int64_t n_cols, const int32_t *wsa, int rank, int P,
                                          const int32_t *d_old_to_new, void *stream, uspmv_halo_t **out) {
    const char *who = "uspmv_halo_discover_device";
    if (!parts || !wsa || !out || n_parts < 1 || n_parts > 3 || P < 1 || rank < 0 || rank >= P || n_cols < 0)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    for (int q = 0; q < n_parts; ++q)
        if (!parts[q]) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    for (int q = 0; q < n_parts; ++q) {
        if (int rc = check_dmat(parts[q], who)) return rc;
        if (!parts[q]->own.col_idxs || parts[q]->col_idxs != parts[q]->own.col_idxs)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: the handle does not own its arrays (uspmv_dmat_wrap): their columns cannot be rewritten", who);
        if (parts[q]->alt || carries_plan(parts[q]))
            return uspmv::fail(USPMV_ERR_INVALID, "%s: the handle already carries a plan, built on the columns this call rewrites", who);
    }
    for (int q = 1; q < n_parts; ++q)
        for (int r = 0; r < q; ++r)
            if (parts[q] == parts[r]) return uspmv::fail(USPMV_ERR_INVALID, "%s: %s parts are one struct", who, n_parts == 2 ? "the two" : "two of the");
    for (int q = 1; q < n_parts; ++q)
        if (parts[0]->C != parts[q]->C || parts[0]->n_chunks != parts[q]->n_chunks)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: the parts must share C, n_chunks and the row layout (convert the other parts with the first part's permutation)", who);
    for (int p = 0; p < P; ++p)
        if (wsa[p + 1] < wsa[p]) return uspmv::fail(USPMV_ERR_INVALID, "%s: flaw in work_sharing_arr", who);
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int32_t lo = wsa[rank], hi = wsa[rank + 1];
    const int64_t n_local = hi - lo, table_len = std::max<int64_t>(wsa[P], n_cols);

    // ---- claim
    DeviceBuf<u64> table, scal;                              // scal[0] = least key of an entry outside the table, scal[1] = claimed columns, scal[2] = write cursor
    HIP_TRY(table.alloc(8 * (size_t)table_len));
    HIP_TRY(scal.alloc(8 * 3));
    HIP_TRY(hipMemsetAsync(table, 0xFF, 8 * (size_t)table_len, st));
    HIP_TRY(hipMemsetAsync(scal, 0xFF, 8, st));
    HIP_TRY(hipMemsetAsync(scal + 1, 0, 16, st));
    for (int q = 0; q < n_parts; ++q) {
        const long n_el = (long)parts[q]->n_elements;
        if (n_el > 0)
            hipLaunchKernelGGL(halo_claim_kernel, dim3(grid_for(n_el, 256)), dim3(256), 0, st, parts[q]->col_idxs, n_el, (u64)q << 32, lo, hi, (long)table_len,
                               table.get(), scal.get());
    }
    if (table_len > 0) hipLaunchKernelGGL(halo_count_kernel, dim3(grid_for((long)table_len, 256)), dim3(256), 0, st, table.get(), (long)table_len, scal + 1);
    HIP_TRY(hipGetLastError());
    u64 h_scal[2] = {NO_KEY, 0};
    HIP_TRY(hipMemcpyAsync(h_scal, scal, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    // ---- the claimed columns, ordered on the host
    const int64_t n_halo = (int64_t)h_scal[1];
    std::vector<HaloRec> rec((size_t)n_halo);
    DeviceBuf<HaloRec> d_rec;
    if (n_halo > 0) {
        HIP_TRY(d_rec.alloc(sizeof(HaloRec) * (size_t)n_halo));
        hipLaunchKernelGGL(halo_compact_kernel, dim3(grid_for((long)table_len, 256)), dim3(256), 0, st, table.get(), (long)table_len, (long)n_halo, scal + 2,
                           d_rec.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rec.data(), d_rec, sizeof(HaloRec) * (size_t)n_halo, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    auto owner_of = [&](int32_t col) { return (int)(std::upper_bound(wsa, wsa + P + 1, col) - wsa) - 1; };
    // the serial scan stops at the first entry it cannot place: a column outside the table, or one inside that no block owns
    u64 first_bad = h_scal[0];
    bool bad_is_orphan = false;
    int32_t orphan = 0;
    for (const HaloRec &r : rec) {
        const int p = owner_of(r.col);
        if ((p < 0 || p >= P) && r.key < first_bad) { first_bad = r.key; bad_is_orphan = true; orphan = r.col; }
    }
    if (first_bad != NO_KEY) {
        if (bad_is_orphan) return uspmv::fail(USPMV_ERR_INVALID, "%s: column %d has no owner", who, orphan);
        int32_t col = 0;
        HIP_TRY(hipMemcpy(&col, parts[first_bad >> 32]->col_idxs + (first_bad & 0xFFFFFFFFull), 4, hipMemcpyDeviceToHost));
        return uspmv::fail(USPMV_ERR_INVALID, "%s: column %d outside the global matrix", who, col);
    }
    if (n_local + n_halo > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: local + halo columns exceed int32", who);
    std::sort(rec.begin(), rec.end(), [&](const HaloRec &a, const HaloRec &b) {
        const int pa = owner_of(a.col), pb = owner_of(b.col);
        return pa != pb ? pa < pb : a.key < b.key;
    });
    std::vector<std::vector<int32_t>> lists((size_t)P);
    for (int64_t i = 0; i < n_halo; ++i) {
        HaloRec &r = rec[(size_t)i];
        const int p = owner_of(r.col);
        r.fin = (int)(n_local + i);                         // = n_local + base[owner] + slot: the records are grouped by owner ascending
        lists[(size_t)p].push_back(r.col - wsa[p]);
    }

    // ---- rewrite
    if (n_halo > 0) {
        HIP_TRY(hipMemcpyAsync(d_rec, rec.data(), sizeof(HaloRec) * (size_t)n_halo, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(halo_scatter_kernel, dim3(grid_for((long)n_halo, 256)), dim3(256), 0, st, d_rec.get(), (long)n_halo, table.get());
    }
    for (int q = 0; q < n_parts; ++q) {
        const long n_el = (long)parts[q]->n_elements;
        if (n_el > 0)
            hipLaunchKernelGGL(halo_rewrite_kernel, dim3(grid_for(n_el, 256)), dim3(256), 0, st, (int *)parts[q]->own.col_idxs, n_el, lo, hi, d_old_to_new,
                               table.get());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));                      // (rec and the scratch of this call are released on return)
    *out = uspmv::halo_from_lists(P, rank, n_local, lists);
    return USPMV_OK;
}

extern "C" int uspmv_dmat_chunk_classes_device(const uspmv_dmat_t *A, int64_t n_local, uint8_t *classes, int32_t *pad_col, void *stream) {
    const char *who = "uspmv_dmat_chunk_classes_device";
    if (!classes || !pad_col) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_dmat(A, who)) return rc;
    if (n_local < 0 || n_local > INT32_MAX) return uspmv::fail(USPMV_ERR_INVALID, "%s: n_local outside int32", who);
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long nc = (long)A->n_chunks;
    *pad_col = -1;
    if (nc < 1) return USPMV_OK;
    DeviceBuf<int> h0;
    DeviceBuf<unsigned char> cls;
    HIP_TRY(h0.alloc(4));
    HIP_TRY(cls.alloc((size_t)nc));
    const int32_t none = INT32_MAX;
    HIP_TRY(hipMemcpyAsync(h0, &none, 4, hipMemcpyHostToDevice, st));
    const dim3 grid(grid_for(nc, 4)), block(256);
#define CLASSIFY(BT)                                                                                                                          \
    do {                                                                                                                                      \
        hipLaunchKernelGGL(pad_col_kernel<BT>, grid, block, 0, st, A->chunk_ptrs, A->chunk_lengths, A->col_idxs, A->values, nc, (int)A->C,    \
                           (int)n_local, h0.get());                                                                                           \
        hipLaunchKernelGGL(chunk_class_kernel<BT>, grid, block, 0, st, A->chunk_ptrs, A->chunk_lengths, A->col_idxs, A->values, nc, (int)A->C, \
                           (int)n_local, h0.get(), cls.get());                                                                                \
    } while (0)
    if (A->dtype == USPMV_F64) CLASSIFY(uint64_t);
    else if (A->dtype == USPMV_F32) CLASSIFY(uint32_t);
    else CLASSIFY(uint16_t);
#undef CLASSIFY
    HIP_TRY(hipGetLastError());
    int32_t h_h0 = INT32_MAX;
    HIP_TRY(hipMemcpyAsync(classes, cls, (size_t)nc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_h0, h0, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool any_pad = false;
    for (long c = 0; c < nc && !any_pad; ++c) any_pad = classes[c] == 1;
    *pad_col = any_pad ? h_h0 : -1;
    return USPMV_OK;
}
