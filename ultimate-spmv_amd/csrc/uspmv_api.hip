// Device half of the C ABI (include/uspmv.h): handles (upload / wrap / GPU-side conversion / download / free), the tuning table, the
// SpMV / SpMMV / adaptive-precision entry points that dispatch into spmv_kernels.hip, spmmv_kernels.hip and ap_kernels.hip, the raw-array
// entry points with their plan cache, and the pack / permute helpers.  The planners are files of their own: csrc/tlc_planner.hip (SpMV:
// uspmv_dmat_optimize and its variants), csrc/block_planner.hip (block vectors) and csrc/sweep_planner.hip (column-window sweep); the
// STREAM calibrators are csrc/stream_kernels.hip.
#include "uspmv_device.hpp"

#include "../host/uspmv_f16_round.hpp"

#include <mutex>

using namespace uspmv_dev;

namespace uspmv_dev {

Tuning g_tune;

int require_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n < 1) {
        (void)hipGetLastError();
        return uspmv::fail(USPMV_ERR_NO_DEVICE, "no HIP device is visible (hipGetDeviceCount: %s); "
                           "libuspmv has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    }
    return USPMV_OK;
}

int check_dmat(const uspmv_dmat *A, const char *who) {
    if (!A) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL matrix", who);
    if (A->C < 1 || A->n_chunks < 0) return uspmv::fail(USPMV_ERR_INVALID, "%s: corrupt matrix handle", who);
    if (A->n_chunks * A->C > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: padded rows exceed int32", who);
    return USPMV_OK;
}

// one-precision entry points (SpMV, SpMMV and their plans): an fp16 handle only runs as the hp part of uspmv_spmv_ap_hp
int check_dmat_one_prec(const uspmv_dmat *A, const char *who) {
    if (int rc = check_dmat(A, who)) return rc;
    if (A->dtype == USPMV_F16)
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: fp16 handle; fp16 values run only as the hp part of uspmv_spmv_ap_hp", who);
    return USPMV_OK;
}


}  // namespace uspmv_dev

namespace {


// COO -> SELL-C-sigma scatter of uspmv_convert_to_scs_device: one thread per COO entry k (entries sorted by
// row, order inside a row preserved): slot = k - row_start[row], destination as convert_to_scs
// (code/utilities.hpp:2013-2036).  perm != nullptr folds permute_scs_cols (:1802-1831) into the same pass.
// VT = unsigned short: binary16 bits, rounded once from the double (uspmv_f16_round.hpp), as uspmv_convert_to_scs stores USPMV_F16.
template <typename VT>
__device__ __forceinline__ VT scs_fill_value(double v) {
    if constexpr (sizeof(VT) == 2) return uspmv_f64_bits_to_f16((uint64_t)__double_as_longlong(v));
    else return (VT)v;
}
template <typename VT>
__global__ void scs_fill_kernel(const long nnz, const int C, const int n_rows, const int *__restrict__ I,
                                const int *__restrict__ J, const double *__restrict__ V,
                                const int *__restrict__ row_start, const int *__restrict__ row_map,
                                const int *__restrict__ perm, const int *__restrict__ chunk_ptrs,
                                int *__restrict__ col_idxs, VT *__restrict__ values) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    const int r = I[k];
    const int slot = (int)(k - row_start[r]);
    const int row = row_map[r];
    const int c = row / C;
    const long dst = (long)chunk_ptrs[c] + (long)slot * C + (row - c * C);
    int col = J[k];
    if (perm && col < n_rows) col = perm[col];
    col_idxs[dst] = col;
    values[dst] = scs_fill_value<VT>(V[k]);
}

// out[i] = in[perm[idx ? idx[i] : i] + offset]   (pack_send_buf with idx, apply_permutation without)
template <typename VT>
__global__ void gather_kernel(VT *__restrict__ out, const VT *__restrict__ in, const int *__restrict__ perm,
                              const int *__restrict__ idx, const long n, const long offset) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[(long)perm[idx ? idx[i] : (int)i] + offset];
}

// The tuning keys of uspmv_set_tuning / uspmv_get_tuning: the field of Tuning (uspmv_device.hpp: meaning and default) and the rule a
// value passes on its way in.  A rule adjusts the value in place and returns false to refuse it (`refusal` is then the error text).
bool any(int &) { return true; }
bool flag(int &v) { v = v != 0; return true; }
template <int LO, int HI = INT32_MAX>
bool clamped(int &v) { v = v < LO ? LO : v > HI ? HI : v; return true; }
template <int LO, int HI>
bool within(int &v) { return v >= LO && v <= HI; }
template <int... SET>
bool one_of(int &v) { return ((v == SET) || ...); }
template <int ELSE, int... SET>
bool one_of_or(int &v) { if (!((v == SET) || ...)) v = ELSE; return true; }

struct TuneKey {
    const char *key;
    int Tuning::*field;
    bool (*rule)(int &);
    const char *refusal = nullptr;
    int (*unpack)(int word) = nullptr;           // keys that share a field with another one (xcd_remap: bits 0-19 the group size, 20+ the stagger)
    int (*pack)(int word, int v) = nullptr;
};
const TuneKey TUNE_KEYS[] = {
    {"unroll", &Tuning::unroll, one_of<1, 2, 4, 8>, "unroll must be 1|2|4|8"},
    {"nontemporal", &Tuning::nontemporal, flag},
    {"xcd_remap", &Tuning::xcd_remap, within<0, 65536>, "xcd_remap must be 0, 1 or a group size <= 65536",
     [](int w) { return w & 0xFFFFF; }, [](int w, int v) { return (w & ~0xFFFFF) | v; }},
    // XCD k starts its group value*k tiles in (remap_block); 0 = all XCDs in step
    {"xcd_stagger", &Tuning::xcd_remap, within<0, 2047>, "xcd_stagger must be in [0, 2047]",
     [](int w) { return w >> 20; }, [](int w, int v) { return (w & 0xFFFFF) | (v << 20); }},
    {"block", &Tuning::block, one_of<64, 128, 256, 512, 1024>, "block must be 64|128|256|512|1024"},
    {"spmv_variant", &Tuning::spmv_variant, within<0, 2>, "spmv_variant must be 0|1|2"},
    {"csr_lanes", &Tuning::csr_lanes, [](int &v) { return v >= 0 && v <= 64 && !(v & (v - 1)); }, "csr_lanes must be 0 or a power of two <= 64"},
    {"ablate", &Tuning::ablate, any},
    {"tlc", &Tuning::tlc, flag},
    {"rechunk", &Tuning::rechunk, flag},
    {"tlc_tile_rows", &Tuning::tlc_tile_rows, one_of<0, 256, 512, 1024>, "tlc_tile_rows must be 0|256|512|1024"},
    {"tlc_auto_tile", &Tuning::tlc_auto_tile, flag},
    {"tlc_measure_tile", &Tuning::tlc_measure_tile, flag},
    {"tlc_idx12", &Tuning::tlc_idx12, clamped<0, 2>},
    {"tlc_additive", &Tuning::tlc_additive, clamped<0, 2>},
    {"tlc_elem", &Tuning::tlc_elem, clamped<0, 2>},
    {"tlc_elem_rows", &Tuning::tlc_elem_rows, clamped<0>},
    {"tlc_elem_seg_rows", &Tuning::tlc_elem_seg_rows, clamped<65536>},
    {"tlc_elem_cap", &Tuning::tlc_elem_cap, clamped<64, 16384>},
    {"tail_batch", &Tuning::tail_batch, flag},
    {"raw_plan_cache", &Tuning::raw_plan_cache, flag},
    {"sweep", &Tuning::sweep, flag},
    {"sweep_nbuf", &Tuning::sweep_nbuf, one_of_or<2, 1>},
    {"sweep_unroll", &Tuning::sweep_unroll, [](int &v) { v = v >= 8 ? 8 : v >= 4 ? 4 : 2; return true; }},
    {"sweep_pair", &Tuning::sweep_pair, clamped<0, 2>},
    {"sweep_remap", &Tuning::sweep_remap, clamped<0>},
    {"sweep_wlog", &Tuning::sweep_wlog, [](int &v) { return v == 0 || (v >= 8 && v <= 16); }, "sweep_wlog must be 0 or 8..16"},
    {"sweep_tile_rows", &Tuning::sweep_tile_rows, one_of<0, 256, 512, 1024, 2048, 4096>, "sweep_tile_rows must be 0|256|512|1024|2048|4096"},
    {"sweep_threads", &Tuning::sweep_threads, one_of_or<0, 256, 512, 1024>},
    {"sweep_max_stage", &Tuning::sweep_max_stage, clamped<0>},
    {"spmmv_variant", &Tuning::spmmv_variant, [](int &v) { return v >= 0 && v <= 9 && v != 7; }, "spmmv_variant must be 0..6, 8 or 9 (9: the block-vector window sweep only)"},
    {"spmmv_unroll", &Tuning::spmmv_unroll, any},
    {"spmmv_prefetch", &Tuning::spmmv_prefetch, flag},
    {"spmmv_swizzle", &Tuning::spmmv_swizzle, flag},
    {"spmmv_reorder", &Tuning::spmmv_reorder, clamped<0, 4>},
    {"spmmv_brick_stride", &Tuning::spmmv_brick_stride, clamped<0>},
    {"spmmv_brick_lines", &Tuning::spmmv_brick_lines, clamped<1>},
    {"spmmv_phase_dp", &Tuning::spmmv_phase_dp, clamped<0>},
    {"spmmv_stream", &Tuning::spmmv_stream, [](int &v) { v = v < 0 ? 0 : v >= 99 ? 99 : v > 5 ? 5 : v; return true; }},
    {"spmmv_stream_waves", &Tuning::spmmv_stream_waves, clamped<4, 5>},
    {"spmmv_stream_xcd", &Tuning::spmmv_stream_xcd, flag},
    {"spmmv_stream_depth", &Tuning::spmmv_stream_depth, clamped<1, 2>},
    {"spmmv_phased", &Tuning::spmmv_phased, flag},
    {"spmmv_phase_rows", &Tuning::spmmv_phase_rows, one_of_or<256, 512>},
    {"spmmv_xcol", &Tuning::spmmv_xcol, flag},
    {"spmmv_ycol_nt", &Tuning::spmmv_ycol_nt, flag},
    {"spmmv_xline", &Tuning::spmmv_xline, flag},
    {"spmmv_unscramble", &Tuning::spmmv_unscramble, flag},
    {"spmmv_idx8", &Tuning::spmmv_idx8, flag},
    {"spmmv_list_plan", &Tuning::spmmv_list_plan, flag},
    {"spmmv_tile_rows", &Tuning::spmmv_tile_rows, one_of_or<0, 64, 32>},
    {"spmmv_lds_kb", &Tuning::spmmv_lds_kb, clamped<0>},
    {"block_plan_device", &Tuning::block_plan_device, flag},
};
const TuneKey *find_tune_key(const char *key) {
    for (const TuneKey &k : TUNE_KEYS)
        if (!strcmp(key, k.key)) return &k;
    return nullptr;
}

}  // namespace

namespace uspmv_dev {
// the O(nnz) scatter of convert_to_scs for callers in other files (csrc/convert_kernels.hip)
int launch_scs_fill(int dtype, long nnz, int C, int n_rows, const int *I, const int *J, const double *V, const int *row_start, const int *row_map,
                    const int *perm, const int *chunk_ptrs, int *col_idxs, void *values, hipStream_t st) {
    const unsigned grid = (unsigned)((nnz + 255) / 256);
    if (dtype == USPMV_F64)
        hipLaunchKernelGGL(scs_fill_kernel<double>, dim3(grid), dim3(256), 0, st, nnz, C, n_rows, I, J, V, row_start, row_map, perm, chunk_ptrs, col_idxs, (double *)values);
    else if (dtype == USPMV_F32)
        hipLaunchKernelGGL(scs_fill_kernel<float>, dim3(grid), dim3(256), 0, st, nnz, C, n_rows, I, J, V, row_start, row_map, perm, chunk_ptrs, col_idxs, (float *)values);
    else
        hipLaunchKernelGGL(scs_fill_kernel<unsigned short>, dim3(grid), dim3(256), 0, st, nnz, C, n_rows, I, J, V, row_start, row_map, perm, chunk_ptrs, col_idxs, (unsigned short *)values);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}
}  // namespace uspmv_dev

// ============================================================================================ C ABI
extern "C" {

int uspmv_device_count(int *count) {
    if (!count) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_device_count: NULL argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count = n;
    return USPMV_OK;
}

int uspmv_set_device(int device) {
    if (int rc = require_device()) return rc;
    HIP_TRY(hipSetDevice(device));
    return USPMV_OK;
}

int uspmv_stream_synchronize(void *stream) {
    if (int rc = require_device()) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return USPMV_OK;
}

int uspmv_set_tuning(const char *key, int value) {
    if (!key) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_set_tuning: NULL key");
    const TuneKey *k = find_tune_key(key);
    if (!k) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_set_tuning: unknown key '%s'", key);
    if (!k->rule(value)) return uspmv::fail(USPMV_ERR_INVALID, "%s", k->refusal);
    g_tune.*k->field = k->pack ? k->pack(g_tune.*k->field, value) : value;
    return USPMV_OK;
}

int uspmv_get_tuning(const char *key, int *value) {
    if (!key || !value) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_get_tuning: NULL argument");
    const TuneKey *k = find_tune_key(key);
    if (!k) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_get_tuning: unknown key '%s'", key);
    *value = k->unpack ? k->unpack(g_tune.*k->field) : g_tune.*k->field;
    return USPMV_OK;
}

int uspmv_dmat_upload(const uspmv_scs_t *s, uspmv_dmat_t **out) {
    if (!s || !out) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_upload: NULL argument");
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_upload: layout-only struct (its entries already live on the device)");
    if (int rc = require_device()) return rc;
    auto *A = new uspmv_dmat;
    A->C = s->C; A->n_chunks = s->n_chunks; A->n_elements = s->n_elements; A->dtype = s->dtype;
    A->n_store = (long)(s->n_chunks * s->C);
    const size_t vsz = uspmv_dtype_bytes(s->dtype);
    hipError_t e = A->own_arrays();
    if (e != hipSuccess) {
        delete A;
        return uspmv::fail(USPMV_ERR_ALLOC, "uspmv_dmat_upload: hipMalloc failed: %s", hipGetErrorString(e));
    }
    e = hipMemcpy(A->own.chunk_ptrs, s->chunk_ptrs.data(), sizeof(int32_t) * (size_t)(s->n_chunks + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(A->own.chunk_lengths, s->chunk_lengths.data(), sizeof(int32_t) * (size_t)s->n_chunks, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(A->own.col_idxs, s->col_idxs.data(), sizeof(int32_t) * (size_t)s->n_elements, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(A->own.values, s->values_ptr(), vsz * (size_t)s->n_elements, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete A;
        return uspmv::fail(USPMV_ERR_HIP, "uspmv_dmat_upload: hipMemcpy failed: %s", hipGetErrorString(e));
    }
    *out = A;
    return USPMV_OK;
}

int uspmv_dmat_wrap(int64_t C, int64_t n_chunks, int64_t n_elements, int dtype, const int32_t *d_chunk_ptrs,
                    const int32_t *d_chunk_lengths, const int32_t *d_col_idxs, const void *d_values,
                    uspmv_dmat_t **out) {
    if (!out || C < 1 || n_chunks < 0 || n_elements < 0 || (dtype != USPMV_F64 && dtype != USPMV_F32 && dtype != USPMV_F16) ||
        !d_chunk_ptrs || (n_chunks > 0 && !d_chunk_lengths) || (n_elements > 0 && (!d_col_idxs || !d_values)))
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_wrap: bad argument");
    auto *A = new uspmv_dmat;
    A->C = C; A->n_chunks = n_chunks; A->n_elements = n_elements; A->dtype = dtype; A->n_store = (long)(n_chunks * C);
    A->chunk_ptrs = d_chunk_ptrs; A->chunk_lengths = d_chunk_lengths; A->col_idxs = d_col_idxs; A->values = d_values;
    *out = A;
    return USPMV_OK;
}

int uspmv_convert_to_scs_device(const uspmv_coo_t *m, int64_t C, int64_t sigma, int dtype, const int32_t *fixed_permutation,
                                int permute_cols, uspmv_scs_t **layout, uspmv_dmat_t **out) {
    if (!m || !layout || !out) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_convert_to_scs_device: NULL argument");
    if (dtype == USPMV_F16) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "uspmv_convert_to_scs_device: no device-side conversion of fp16 parts (uspmv_convert_to_scs + uspmv_dmat_upload)");
    if (int rc = require_device()) return rc;
    auto *s = new uspmv_scs;
    std::vector<int64_t> row_start;
    if (int rc = uspmv_scs_layout(m, C, sigma, dtype, fixed_permutation, s, &row_start, "uspmv_convert_to_scs_device")) { delete s; return rc; }
    if (row_start.empty() && m->nnz > 0) {
        delete s;
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "uspmv_convert_to_scs_device: COO entries must be sorted by row "
                                                  "(uspmv_read_mtx and the generators produce that order)");
    }
    if (m->nnz > INT32_MAX) { delete s; return uspmv::fail(USPMV_ERR_OVERFLOW, "uspmv_convert_to_scs_device: nnz exceeds int32"); }
    std::vector<int32_t> rs32(row_start.begin(), row_start.end());
    const int32_t *row_map = fixed_permutation ? fixed_permutation : s->old_to_new_idx.data();
    auto *A = new uspmv_dmat;
    A->C = s->C; A->n_chunks = s->n_chunks; A->n_elements = s->n_elements; A->dtype = dtype;
    A->n_store = (long)(s->n_chunks * s->C);
    const size_t vsz = dtype == USPMV_F64 ? 8 : 4;
    const size_t ne = (size_t)std::max<int64_t>(s->n_elements, 1), nz = (size_t)std::max<int64_t>(m->nnz, 1);
    hipError_t e = A->own_arrays();
    void *cp = A->own.chunk_ptrs, *ci = A->own.col_idxs, *va = A->own.values;
    DeviceBuf<int32_t> dI, dJ, drs, dmap, dperm;
    DeviceBuf<double> dV;
    if (e == hipSuccess) e = hipMemcpy(cp, s->chunk_ptrs.data(), 4 * s->chunk_ptrs.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(A->own.chunk_lengths, s->chunk_lengths.data(), 4 * s->chunk_lengths.size(), hipMemcpyHostToDevice);
    // padding: value 0, column 0 -- which permute_scs_cols maps like any other local column (code/utilities.hpp:1820-1826)
    const int pad_col = (permute_cols && m->n_rows > 0) ? s->old_to_new_idx[0] : 0;
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)ci, pad_col, ne, nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(va, 0, vsz * ne, nullptr);
    if (e == hipSuccess) e = dI.upload(m->I.data(), 4 * (size_t)m->nnz);
    if (e == hipSuccess) e = dJ.upload(m->J.data(), 4 * (size_t)m->nnz);
    if (e == hipSuccess) e = dV.upload(m->values.data(), 8 * (size_t)m->nnz);
    if (e == hipSuccess) e = drs.upload(rs32.data(), 4 * rs32.size());
    if (e == hipSuccess) e = dmap.upload(row_map, 4 * (size_t)m->n_rows);
    if (e == hipSuccess && permute_cols) e = dperm.upload(s->old_to_new_idx.data(), 4 * (size_t)m->n_rows);
    if (e == hipSuccess && m->nnz > 0) {
        const unsigned grid = (unsigned)((nz + 255) / 256);
        if (dtype == USPMV_F64)
            hipLaunchKernelGGL(scs_fill_kernel<double>, dim3(grid), dim3(256), 0, nullptr, (long)m->nnz, (int)C, (int)m->n_rows, dI.get(), dJ.get(), dV.get(),
                               drs.get(), dmap.get(), dperm.get(), (const int *)cp, (int *)ci, (double *)va);
        else
            hipLaunchKernelGGL(scs_fill_kernel<float>, dim3(grid), dim3(256), 0, nullptr, (long)m->nnz, (int)C, (int)m->n_rows, dI.get(), dJ.get(), dV.get(),
                               drs.get(), dmap.get(), dperm.get(), (const int *)cp, (int *)ci, (float *)va);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        delete A; delete s;
        return uspmv::fail(USPMV_ERR_HIP, "uspmv_convert_to_scs_device: %s", hipGetErrorString(e));
    }
    *layout = s;
    *out = A;
    return USPMV_OK;
}

int uspmv_dmat_plan_addresses(const uspmv_dmat_t *A, uint64_t addr[8]) {
    if (!A || !addr) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_plan_addresses: NULL argument");
    const uspmv_dmat *M = A->alt ? A->alt : A;
    addr[0] = (uint64_t)(uintptr_t)M->tlc.col16.get(); addr[1] = (uint64_t)(uintptr_t)M->tlc.lines.get(); addr[2] = (uint64_t)(uintptr_t)M->tlc.line_ptr.get();
    addr[3] = (uint64_t)(uintptr_t)M->tlc.c16_ptrs.get(); addr[4] = (uint64_t)(uintptr_t)M->values; addr[5] = (uint64_t)(uintptr_t)M->col_idxs;
    addr[6] = (uint64_t)(uintptr_t)M->chunk_ptrs; addr[7] = (uint64_t)(uintptr_t)M->chunk_lengths;
    return USPMV_OK;
}

int uspmv_dmat_meta(const uspmv_dmat_t *A, int64_t meta[4]) {
    if (!A || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_meta: NULL argument");
    meta[0] = A->C; meta[1] = A->n_chunks; meta[2] = A->n_elements; meta[3] = A->dtype;
    return USPMV_OK;
}

int uspmv_dmat_download(const uspmv_dmat_t *A, int32_t *chunk_ptrs, int32_t *chunk_lengths, int32_t *col_idxs, void *values) {
    if (int rc = check_dmat(A, "uspmv_dmat_download")) return rc;
    if (int rc = require_device()) return rc;
    const size_t vsz = uspmv_dtype_bytes(A->dtype);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && chunk_ptrs) e = hipMemcpy(chunk_ptrs, A->chunk_ptrs, 4 * (size_t)(A->n_chunks + 1), hipMemcpyDeviceToHost);
    if (e == hipSuccess && chunk_lengths) e = hipMemcpy(chunk_lengths, A->chunk_lengths, 4 * (size_t)A->n_chunks, hipMemcpyDeviceToHost);
    if (e == hipSuccess && col_idxs) e = hipMemcpy(col_idxs, A->col_idxs, 4 * (size_t)A->n_elements, hipMemcpyDeviceToHost);
    if (e == hipSuccess && values) e = hipMemcpy(values, A->values, vsz * (size_t)A->n_elements, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return uspmv::fail(USPMV_ERR_HIP, "uspmv_dmat_download: %s", hipGetErrorString(e));
    return USPMV_OK;
}

int uspmv_spmv_ap_hp(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, void *d_y, void *stream) {
    if (int rc = check_ap_hp(hi, mid, hp, "uspmv_spmv_ap_hp")) return rc;
    if (!d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_ap_hp: NULL vector");
    if (int rc = require_device()) return rc;
    if (hi->n_chunks == 0) return USPMV_OK;
    return launch_spmv_ap_hp(hi, mid, hp, d_x, d_y, (hipStream_t)stream);
}

int uspmv_spmv_ap_hp_tiles(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const int32_t *d_tile_ids, int64_t n_ids,
                           const void *d_x, void *d_y, void *stream) {
    const char *who = "uspmv_spmv_ap_hp_tiles";
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    const uint64_t id = hi->tlc.plan_id;
    if (!hi->tlc.on || id == 0 || !hp->tlc.on || hp->tlc.plan_id != id || (mid && (!mid->tlc.on || mid->tlc.plan_id != id)))
        return uspmv::fail(USPMV_ERR_INVALID, "%s: the parts have no shared tile-local-column plan (uspmv_dmat_optimize_ap_hp)", who);
    if (n_ids < 0 || n_ids > hi->tlc.n_tiles || (n_ids > 0 && !d_tile_ids) || !d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if ((uintptr_t)d_x % 16) return uspmv::fail(USPMV_ERR_INVALID, "%s: x must be 16-byte aligned", who);
    if (int rc = require_device()) return rc;
    return launch_spmv_ap_hp_tiles(hi, mid, hp, d_tile_ids, (long)n_ids, d_x, d_y, (hipStream_t)stream);
}

int uspmv_spmv_ap_hp_chunks(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const int32_t *d_chunk_ids, int64_t n_ids,
                            const void *d_x, void *d_y, void *stream) {
    const char *who = "uspmv_spmv_ap_hp_chunks";
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    if (n_ids < 0 || n_ids > hi->n_chunks || (n_ids > 0 && !d_chunk_ids) || !d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (int rc = require_device()) return rc;
    return launch_spmv_ap_hp_chunks(hi, mid, hp, d_chunk_ids, (long)n_ids, d_x, d_y, (hipStream_t)stream);
}

// the argument checks uspmv_spmmv_ap_hp, uspmv_spmmv_ap_hp_path and the list forms share
static int check_spmmv_ap_hp(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, int b, int64_t ld, int layout, const char *who) {
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    if (b < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: b=%d", who, b);
    if (layout != USPMV_COLWISE && layout != USPMV_ROWWISE) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown layout %d", who, layout);
    if (layout == USPMV_COLWISE && ld < hi->n_chunks * hi->C)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: ld=%lld smaller than n_rows_padded=%lld", who, (long long)ld,
                           (long long)(hi->n_chunks * hi->C));
    return USPMV_OK;
}

int uspmv_spmmv_ap_hp(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_X, void *d_Y, int b, int64_t ld,
                      int layout, void *stream) {
    const char *who = "uspmv_spmmv_ap_hp";
    if (int rc = check_spmmv_ap_hp(hi, mid, hp, b, ld, layout, who)) return rc;
    if (!d_X || !d_Y) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL vector", who);
    if (int rc = require_device()) return rc;
    if (hi->n_chunks == 0) return USPMV_OK;
    return launch_spmmv_ap_hp(hi, mid, hp, d_X, d_Y, b, (long)ld, layout, (hipStream_t)stream);
}

int uspmv_spmmv_ap_hp_path(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, int b, int64_t ld, int layout, int *path,
                           int *vectors_per_pass) {
    const char *who = "uspmv_spmmv_ap_hp_path";
    if (int rc = check_spmmv_ap_hp(hi, mid, hp, b, ld, layout, who)) return rc;
    if (!path || !vectors_per_pass) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL result pointer", who);
    spmmv_ap_hp_path(hi, mid, hp, b, (long)ld, layout, path, vectors_per_pass);
    return USPMV_OK;
}

// the checks of the list forms of uspmv_spmmv_ap_hp: those of uspmv_spmmv_ap_hp and of uspmv_spmv_ap_hp_tiles.  Nothing here touches a
// device.
static int check_ap_hp_block_list(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, int b, int64_t ld, int layout, bool tiles,
                                  const char *who) {
    if (int rc = check_spmmv_ap_hp(hi, mid, hp, b, ld, layout, who)) return rc;
    const uint64_t id = hi->tlc.plan_id;
    if (tiles && (!hi->tlc.on || id == 0 || !hp->tlc.on || hp->tlc.plan_id != id || (mid && (!mid->tlc.on || mid->tlc.plan_id != id))))
        return uspmv::fail(USPMV_ERR_INVALID, "%s: the parts have no shared tile-local-column plan (uspmv_dmat_optimize_ap_hp)", who);
    return USPMV_OK;
}

int uspmv_spmmv_ap_hp_tiles(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const int32_t *d_tile_ids, int64_t n_ids,
                            const void *d_X, void *d_Y, int b, int64_t ld, int layout, void *stream) {
    const char *who = "uspmv_spmmv_ap_hp_tiles";
    if (int rc = check_ap_hp_block_list(hi, mid, hp, b, ld, layout, true, who)) return rc;
    if (n_ids < 0 || n_ids > hi->tlc.n_tiles || (n_ids > 0 && !d_tile_ids) || !d_X || !d_Y) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (n_ids == 0) return USPMV_OK;
    if (int rc = require_device()) return rc;
    return launch_spmmv_ap_hp_tiles(hi, mid, hp, d_tile_ids, (long)n_ids, d_X, d_Y, b, (long)ld, layout, (hipStream_t)stream);
}

int uspmv_spmmv_ap_hp_chunks(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const int32_t *d_chunk_ids, int64_t n_ids,
                             const void *d_X, void *d_Y, int b, int64_t ld, int layout, void *stream) {
    const char *who = "uspmv_spmmv_ap_hp_chunks";
    if (int rc = check_ap_hp_block_list(hi, mid, hp, b, ld, layout, false, who)) return rc;
    if (n_ids < 0 || n_ids > hi->n_chunks || (n_ids > 0 && !d_chunk_ids) || !d_X || !d_Y) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (n_ids == 0) return USPMV_OK;
    if (int rc = require_device()) return rc;
    return launch_spmmv_ap_hp_chunks(hi, mid, hp, d_chunk_ids, (long)n_ids, d_X, d_Y, b, (long)ld, layout, (hipStream_t)stream);
}

int uspmv_spmmv_ap_hp_tiles_path(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, int b, int64_t ld, int layout, int *path,
                                 int *vectors_per_pass) {
    const char *who = "uspmv_spmmv_ap_hp_tiles_path";
    if (int rc = check_ap_hp_block_list(hi, mid, hp, b, ld, layout, true, who)) return rc;
    if (!path || !vectors_per_pass) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL result pointer", who);
    spmmv_ap_hp_tiles_path(hi, b, path, vectors_per_pass);
    return USPMV_OK;
}

int uspmv_spmmv_ap_hp_plan_lines(int b, int x_dtype, int *max_lines) {
    if (b < 1 || (x_dtype != USPMV_F64 && x_dtype != USPMV_F32) || !max_lines)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv_ap_hp_plan_lines: bad argument");
    *max_lines = spmmv_ap_hp_plan_lines(b, x_dtype);
    return USPMV_OK;
}

int uspmv_spmmv_ap_hp_sweep_vectors(int b, int wlog, int x_dtype, int *vectors) {
    if (b < 1 || wlog < 8 || wlog > 16 || (x_dtype != USPMV_F64 && x_dtype != USPMV_F32) || !vectors)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv_ap_hp_sweep_vectors: bad argument");
    *vectors = spmmv_ap_hp_sweep_vectors(b, wlog, x_dtype);
    return USPMV_OK;
}

void uspmv_dmat_free(uspmv_dmat_t *A) {
    if (!A) return;
    uspmv_dmat_free(A->alt);
    delete A;
}

int uspmv_dmat_set_crs(uspmv_dmat_t *A, int on) {
    if (!A) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_set_crs: NULL matrix");
    if (on && A->C != 1) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_set_crs: crs needs C = 1 (got %lld)", (long long)A->C);
    A->crs = on != 0;
    return USPMV_OK;
}

int uspmv_spmv(const uspmv_dmat_t *A, const void *d_x, void *d_y, void *stream) {
    if (int rc = check_dmat_one_prec(A, "uspmv_spmv")) return rc;
    if (!d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv: NULL vector");
    if (int rc = require_device()) return rc;
    if (A->alt && g_tune.tlc && g_tune.rechunk && g_tune.spmv_variant == 0 && !g_tune.ablate) {
        if (A->dtype == USPMV_F64) return launch_spmv_scs<double>(A->alt, nullptr, 0, (const double *)d_x, (double *)d_y, (hipStream_t)stream);
        return launch_spmv_scs<float>(A->alt, nullptr, 0, (const float *)d_x, (float *)d_y, (hipStream_t)stream);
    }
    if (A->crs) {
        if (A->dtype == USPMV_F64)
            return launch_csr<double>((long)A->n_chunks, (long)A->n_elements, A->chunk_ptrs, A->col_idxs,
                                      (const double *)A->values, (const double *)d_x, (double *)d_y, (hipStream_t)stream);
        return launch_csr<float>((long)A->n_chunks, (long)A->n_elements, A->chunk_ptrs, A->col_idxs,
                                 (const float *)A->values, (const float *)d_x, (float *)d_y, (hipStream_t)stream);
    }
    if (A->dtype == USPMV_F64) return launch_spmv_scs<double>(A, nullptr, 0, (const double *)d_x, (double *)d_y, (hipStream_t)stream);
    return launch_spmv_scs<float>(A, nullptr, 0, (const float *)d_x, (float *)d_y, (hipStream_t)stream);
}

// ---- y = alpha A x + beta z with <y,y> and <w,y> ----
extern "C++" {
namespace {

// the struct uspmv_spmv launches for this handle (its re-chunking where it carries one and the tuning takes it) and whether by the csr kernel
const uspmv_dmat *axpby_struct(const uspmv_dmat *A, bool *crs) {
    *crs = false;
    if (A->alt && g_tune.tlc && g_tune.rechunk && g_tune.spmv_variant == 0 && !g_tune.ablate) return A->alt;
    *crs = A->crs;
    return A;
}

// what the three entry points refuse before a device is looked for: handles uspmv_spmv refuses, and the parts of an adaptive-precision split
int axpby_refusals(const uspmv_dmat *A, const char *who) {
    if (int rc = check_dmat(A, who)) return rc;
    if (A->dtype == USPMV_F16)
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: fp16 handle; fp16 values run only as the hp part of uspmv_spmv_ap_hp", who);
    for (const uspmv_dmat *M = A; M; M = M->alt)
        if ((M->tlc.on && M->tlc.plan_id != 0) || (M->sw.on && (M->sw.n_parts > 1 || !M->sw.tile_ids)))
            return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: the handle carries the shared plan of an adaptive-precision split (a part's product is not y; "
                                                      "run uspmv_spmv_ap[_hp] and apply the update to its result)", who);
    return USPMV_OK;
}

// room for `slots` partial pairs (and `tmp_bytes` of the in-place temporary of path 2) on the handle; `st` capturing: no allocation
// (reserve: the call that allocates ahead of a capture, named in the refusal)
int axpby_room(const uspmv_dmat *A, size_t slots, size_t tmp_bytes, hipStream_t st, bool check_capture, const char *who,
               const char *reserve = "uspmv_spmv_axpby_reserve") {
    const bool grow_part = slots > A->axpby_slots, grow_tmp = tmp_bytes > A->axpby_tmp_bytes;
    if (!grow_part && !grow_tmp) return USPMV_OK;
    if (check_capture) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
        if (cs != hipStreamCaptureStatusNone)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: the stream is capturing and the handle's workspace would have to be allocated; call "
                                                  "%s before the capture (under the tuning the call runs with)", who, reserve);
    }
    if (grow_part) {
        A->axpby_slots = 0;
        HIP_TRY(A->axpby_part.alloc(slots * 2 * sizeof(double)));
        A->axpby_slots = slots;
    }
    if (grow_tmp) {
        A->axpby_tmp_bytes = 0;
        HIP_TRY(A->axpby_tmp.alloc(tmp_bytes));
        A->axpby_tmp_bytes = tmp_bytes;
    }
    return USPMV_OK;
}

template <typename VT>
int spmv_axpby_typed(const uspmv_dmat *A, const VT *x, VT *y, const uspmv_axpby_t *op, hipStream_t st) {
    const char *who = "uspmv_spmv_axpby";
    bool crs = false;
    const uspmv_dmat *M = axpby_struct(A, &crs);
    long slots = 0;
    const int path = spmv_axpby_route(M, crs, (uintptr_t)x % 16 == 0, &slots);
    const bool dots = op->d_dots != nullptr;
    const bool in_place = op->beta != 0.0 && op->d_z == (const void *)y;
    const size_t tmp_bytes = (path == 2 && in_place) ? (size_t)A->n_store * sizeof(VT) : 0;
    if (int rc = axpby_room(A, dots ? (size_t)slots : 0, tmp_bytes, st, true, who)) return rc;
    AxpbyArgs<VT> ep;
    ep.alpha = (VT)op->alpha; ep.beta = (VT)op->beta;
    ep.z = (const VT *)op->d_z; ep.w = (const VT *)op->d_w;
    ep.part = dots ? A->axpby_part.get() : nullptr;
    ep.n_dot = (long)op->n_dot_rows;
    if (path == 1) {
        int rc;
        if (crs) rc = launch_csr<VT>((long)M->n_chunks, (long)M->n_elements, M->chunk_ptrs, M->col_idxs, (const VT *)M->values, x, y, st, &ep);
        else rc = launch_spmv_scs<VT>(M, nullptr, 0, x, y, st, &ep);
        if (rc) return rc;
    } else {
        // uspmv_spmv's own launch, then one pass over its result (an in-place call: the product goes to the temporary, y still holds z)
        VT *t = tmp_bytes ? (VT *)A->axpby_tmp.get() : y;
        if (int rc = uspmv_spmv(A, x, t, st)) return rc;
        if (int rc = launch_axpby_pass<VT>(t, y, (long)A->n_store, ep, st, &slots)) return rc;
    }
    if (dots) return launch_axpby_finalize(ep.part, A->n_chunks == 0 ? 0 : slots, op->d_dots, st);
    return USPMV_OK;
}

}  // namespace
}  // extern "C++"

int uspmv_spmv_axpby(const uspmv_dmat_t *A, const void *d_x, void *d_y, const uspmv_axpby_t *op, void *stream) {
    const char *who = "uspmv_spmv_axpby";
    if (int rc = axpby_refusals(A, who)) return rc;
    if (!op) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL op", who);
    if (!d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL vector", who);
    if (op->beta != 0.0 && !op->d_z) return uspmv::fail(USPMV_ERR_INVALID, "%s: beta != 0 needs d_z", who);
    const size_t es = uspmv_dtype_bytes(A->dtype);
    const long n = A->n_store;
    if (op->beta != 0.0 && op->d_z != (const void *)d_y) {
        const uintptr_t z0 = (uintptr_t)op->d_z, y0 = (uintptr_t)d_y, len = (uintptr_t)n * es;
        if (z0 < y0 + len && y0 < z0 + len)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: d_z overlaps d_y partially (in place means d_z == d_y)", who);
    }
    if (op->n_dot_rows < 0 || op->n_dot_rows > n)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: n_dot_rows=%lld outside [0, %lld], the rows y may be written", who, (long long)op->n_dot_rows, (long long)n);
    if (int rc = require_device()) return rc;
    if (A->dtype == USPMV_F64) return spmv_axpby_typed<double>(A, (const double *)d_x, (double *)d_y, op, (hipStream_t)stream);
    return spmv_axpby_typed<float>(A, (const float *)d_x, (float *)d_y, op, (hipStream_t)stream);
}

int uspmv_spmv_axpby_path(const uspmv_dmat_t *A, const void *d_x, int *path) {
    const char *who = "uspmv_spmv_axpby_path";
    if (int rc = axpby_refusals(A, who)) return rc;
    if (!d_x || !path) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    bool crs = false;
    const uspmv_dmat *M = axpby_struct(A, &crs);
    *path = spmv_axpby_route(M, crs, (uintptr_t)d_x % 16 == 0, nullptr);
    return USPMV_OK;
}

int uspmv_spmv_axpby_reserve(uspmv_dmat_t *A) {
    const char *who = "uspmv_spmv_axpby_reserve";
    if (int rc = axpby_refusals(A, who)) return rc;
    if (int rc = require_device()) return rc;
    bool crs = false;
    const uspmv_dmat *M = axpby_struct(A, &crs);
    long s1 = 0;
    const int path = spmv_axpby_route(M, crs, true, &s1);
    // the larger of the routed path's grid and the vector pass's (an x off the 16-byte grid falls to path 2); the in-place temporary
    // only where a 16-byte-aligned x already takes path 2
    const long slots = std::max(s1, axpby_pass_slots((long)A->n_store));
    return axpby_room(A, (size_t)slots, path == 2 ? (size_t)A->n_store * uspmv_dtype_bytes(A->dtype) : 0, nullptr, false, who);
}

int uspmv_spmv_chunks(const uspmv_dmat_t *A, const int32_t *d_chunk_ids, int64_t n_ids, const void *d_x, void *d_y,
                      void *stream) {
    if (int rc = check_dmat_one_prec(A, "uspmv_spmv_chunks")) return rc;
    if (n_ids < 0 || n_ids > A->n_chunks || (n_ids > 0 && !d_chunk_ids) || !d_x || !d_y)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_chunks: bad argument");
    if (int rc = require_device()) return rc;
    if (n_ids == 0) return USPMV_OK;
    if (A->dtype == USPMV_F64) return launch_spmv_scs<double>(A, d_chunk_ids, n_ids, (const double *)d_x, (double *)d_y, (hipStream_t)stream);
    return launch_spmv_scs<float>(A, d_chunk_ids, n_ids, (const float *)d_x, (float *)d_y, (hipStream_t)stream);
}

int uspmv_spmv_tiles(const uspmv_dmat_t *A, const int32_t *d_tile_ids, int64_t n_ids, const void *d_x, void *d_y,
                     void *stream) {
    if (int rc = check_dmat_one_prec(A, "uspmv_spmv_tiles")) return rc;
    if (!A->tlc.on || A->tlc.plan_id != 0) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_tiles: handle has no tile-local-column plan (uspmv_dmat_optimize)");
    if (n_ids < 0 || n_ids > A->tlc.n_tiles || (n_ids > 0 && !d_tile_ids) || !d_x || !d_y)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_tiles: bad argument");
    if ((uintptr_t)d_x % 16) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_tiles: x must be 16-byte aligned");
    if (int rc = require_device()) return rc;
    if (A->dtype == USPMV_F64) return launch_spmv_tlc<double>(A, d_tile_ids, (long)n_ids, (const double *)d_x, (double *)d_y, (hipStream_t)stream);
    return launch_spmv_tlc<float>(A, d_tile_ids, (long)n_ids, (const float *)d_x, (float *)d_y, (hipStream_t)stream);
}

int uspmv_dmat_plan_info(const uspmv_dmat_t *A, int *kind, int64_t *n_tiles, int64_t *n_planned) {
    if (!A) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_plan_info: NULL matrix");
    const uspmv_dmat_t *M = A->alt ? A->alt : A;
    int k = 0; int64_t nt = 0, np = 0;
    if (M->sw.on) { k = 2; nt = M->sw.all_tiles; np = M->sw.n_tiles; }
    else if (M->tlc.on) { k = 1; nt = M->tlc.n_tiles; np = M->tlc.staged; }
    if (kind) *kind = k;
    if (n_tiles) *n_tiles = nt;
    if (n_planned) *n_planned = np;
    return USPMV_OK;
}

int uspmv_dmat_plan_granularity(const uspmv_dmat_t *A, int *elements_per_list_entry) {
    if (!A || !elements_per_list_entry) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_plan_granularity: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    *elements_per_list_entry = !M->tlc.on ? 0 : M->tlc.elem ? 1 : 16;
    return USPMV_OK;
}

int uspmv_dmat_plan_rows_dealt(const uspmv_dmat_t *A, int *dealt) {
    if (!A || !dealt) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_plan_rows_dealt: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    *dealt = M->tlc.on && M->tlc.row_map != nullptr;
    return USPMV_OK;
}

int uspmv_dmat_tile_rows(const uspmv_dmat_t *A, int *tile_rows) {
    if (!A || !tile_rows) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_tile_rows: NULL argument");
    *tile_rows = A->tlc.on ? A->tlc.tile_rows : 0;
    return USPMV_OK;
}

int uspmv_dmat_index_bits(const uspmv_dmat_t *A, int *bits) {
    if (!A || !bits) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_index_bits: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    *bits = !M->tlc.on ? 0 : M->tlc.col12 ? 12 : 16;
    return USPMV_OK;
}

int uspmv_dmat_additive_chunks(const uspmv_dmat_t *A, int64_t *n_additive, int64_t *n_chunks) {
    if (!A || !n_additive || !n_chunks) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_additive_chunks: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    const bool on = M->tlc.on && M->tlc.add_ptrs;
    *n_additive = on ? M->tlc.add_additive : 0;
    *n_chunks = on ? M->tlc.add_chunks : 0;
    return USPMV_OK;
}

int uspmv_spmmv(const uspmv_dmat_t *A, const void *d_X, void *d_Y, int b, int64_t ld, int layout, void *stream) {
    if (int rc = check_dmat_one_prec(A, "uspmv_spmmv")) return rc;
    if (!d_X || !d_Y || b < 1) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv: bad argument");
    if (layout != USPMV_COLWISE && layout != USPMV_ROWWISE) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv: unknown layout %d", layout);
    if (layout == USPMV_COLWISE && ld < A->n_chunks * A->C)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv: ld=%lld smaller than n_rows_padded=%lld", (long long)ld,
                           (long long)(A->n_chunks * A->C));
    if (int rc = require_device()) return rc;
    // narrow-chunk handles optimised by uspmv_dmat_optimize carry an internal C = 32 re-chunking with the same row
    // order (crs: SELL-32-1): coalesced matrix stream for the block kernels too; its stores stop at the caller's rows
    if (A->alt && g_tune.rechunk) A = A->alt;
    if (A->dtype == USPMV_F64) return launch_spmmv<double>(A, (const double *)d_X, (double *)d_Y, b, (long)ld, layout, (hipStream_t)stream);
    return launch_spmmv<float>(A, (const float *)d_X, (float *)d_Y, b, (long)ld, layout, (hipStream_t)stream);
}

int uspmv_spmmv_last_path(const uspmv_dmat_t *A, int *kernel, int *x_pass) {
    if (int rc = check_dmat(A, "uspmv_spmmv_last_path")) return rc;
    if (!kernel || !x_pass) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv_last_path: NULL result pointer");
    if (A->alt && g_tune.rechunk) A = A->alt;                 // (the handle uspmv_spmmv launches on)
    *kernel = A->last_kernel; *x_pass = A->last_xpass;
    return USPMV_OK;
}

int uspmv_spmmv_x_prepared(const uspmv_dmat_t *A, const void *d_X, int b, int64_t ld, void *stream) {
    if (int rc = check_dmat_one_prec(A, "uspmv_spmmv_x_prepared")) return rc;
    if (!d_X || b < 1 || ld < A->n_chunks * A->C) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv_x_prepared: bad argument");
    if (int rc = require_device()) return rc;
    if (A->alt && g_tune.rechunk) A = A->alt;
    A->xprep_ptr = nullptr;
    const int rc = A->dtype == USPMV_F64 ? prepare_x<double>(A, (const double *)d_X, b, (long)ld, (hipStream_t)stream)
                                         : prepare_x<float>(A, (const float *)d_X, b, (long)ld, (hipStream_t)stream);
    if (rc > 0) return USPMV_OK;                              // (this width / alignment has no re-layout pass: nothing to prepare, nothing skipped)
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int uspmv_spmmv_x_release(const uspmv_dmat_t *A) {
    if (int rc = check_dmat(A, "uspmv_spmmv_x_release")) return rc;
    A->xprep_ptr = nullptr;
    if (A->alt) A->alt->xprep_ptr = nullptr;
    return USPMV_OK;
}

static int spmv_ap_impl(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, const float *d_x_sp,
                        double *d_y, void *stream, const char *who) {
    if (int rc = check_dmat(dp, who)) return rc;
    if (int rc = check_dmat(sp, who)) return rc;
    if (dp->dtype != USPMV_F64 || sp->dtype != USPMV_F32)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: expects a double and a float struct", who);
    if (dp->C != sp->C || dp->n_chunks != sp->n_chunks)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: dp and sp structs must share C and n_chunks", who);
    if (!d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL vector", who);
    if (int rc = require_device()) return rc;
    if (dp->n_chunks == 0) return USPMV_OK;
    return launch_spmv_ap(dp, sp, d_x, d_x_sp, d_y, (hipStream_t)stream);
}

int uspmv_spmv_ap(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, double *d_y, void *stream) {
    return spmv_ap_impl(dp, sp, d_x, nullptr, d_y, stream, "uspmv_spmv_ap");
}

// the pair checks of spmv_ap_impl for the list forms
static int check_ap_pair(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const char *who) {
    if (int rc = check_dmat(dp, who)) return rc;
    if (int rc = check_dmat(sp, who)) return rc;
    if (dp->dtype != USPMV_F64 || sp->dtype != USPMV_F32) return uspmv::fail(USPMV_ERR_INVALID, "%s: expects a double and a float struct", who);
    if (dp->C != sp->C || dp->n_chunks != sp->n_chunks) return uspmv::fail(USPMV_ERR_INVALID, "%s: dp and sp structs must share C and n_chunks", who);
    return USPMV_OK;
}

int uspmv_spmv_ap_tiles(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const int32_t *d_tile_ids, int64_t n_ids, const double *d_x,
                        double *d_y, void *stream) {
    if (int rc = check_ap_pair(dp, sp, "uspmv_spmv_ap_tiles")) return rc;
    if (!dp->tlc.on || !sp->tlc.on || dp->tlc.plan_id == 0 || dp->tlc.plan_id != sp->tlc.plan_id)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_ap_tiles: the pair has no shared tile-local-column plan (uspmv_dmat_optimize_ap)");
    if (n_ids < 0 || n_ids > dp->tlc.n_tiles || (n_ids > 0 && !d_tile_ids) || !d_x || !d_y)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_ap_tiles: bad argument");
    if ((uintptr_t)d_x % 16) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_ap_tiles: x must be 16-byte aligned");
    if (int rc = require_device()) return rc;
    return launch_spmv_ap_tiles(dp, sp, d_tile_ids, (long)n_ids, d_x, d_y, (hipStream_t)stream);
}

int uspmv_spmv_ap_chunks(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const int32_t *d_chunk_ids, int64_t n_ids, const double *d_x,
                         double *d_y, void *stream) {
    if (int rc = check_ap_pair(dp, sp, "uspmv_spmv_ap_chunks")) return rc;
    if (n_ids < 0 || n_ids > dp->n_chunks || (n_ids > 0 && !d_chunk_ids) || !d_x || !d_y)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_ap_chunks: bad argument");
    if (int rc = require_device()) return rc;
    return launch_spmv_ap_chunks(dp, sp, d_chunk_ids, (long)n_ids, d_x, d_y, (hipStream_t)stream);
}

int uspmv_spmv_ap_generic(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, const float *d_x_sp,
                          double *d_y, void *stream) {
    if (!d_x_sp) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmv_ap_generic: NULL float x");
    return spmv_ap_impl(dp, sp, d_x, d_x_sp, d_y, stream, "uspmv_spmv_ap_generic");
}

// ---- y = alpha A x + beta z with <y,y> and <w,y> on the parts of an adaptive-precision split ----
extern "C++" {
namespace {

// uspmv_spmv_axpby's own refusals (5.12) on n rows of es bytes
int ap_axpby_op_refusals(const uspmv_axpby_t *op, const void *d_x, const void *d_y, long n, size_t es, const char *who) {
    if (!op) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL op", who);
    if (!d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL vector", who);
    if (op->beta != 0.0 && !op->d_z) return uspmv::fail(USPMV_ERR_INVALID, "%s: beta != 0 needs d_z", who);
    if (op->beta != 0.0 && op->d_z != d_y) {
        const uintptr_t z0 = (uintptr_t)op->d_z, y0 = (uintptr_t)d_y, len = (uintptr_t)n * es;
        if (z0 < y0 + len && y0 < z0 + len)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: d_z overlaps d_y partially (in place means d_z == d_y)", who);
    }
    if (op->n_dot_rows < 0 || op->n_dot_rows > n)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: n_dot_rows=%lld outside [0, %lld], the rows y may be written", who, (long long)op->n_dot_rows, (long long)n);
    return USPMV_OK;
}

// One call on either family: `first` carries the workspace (dp / hi); sp != nullptr: the pair, else (first, mid, hp).
template <typename HT>
int spmv_ap_axpby_typed(const uspmv_dmat *first, const uspmv_dmat *sp, const uspmv_dmat *mid, const uspmv_dmat *hp, const HT *x, HT *y,
                        const uspmv_axpby_t *op, hipStream_t st, const char *who, const char *reserve) {
    const long n = (long)first->n_chunks * first->C;
    const bool x16 = (uintptr_t)x % 16 == 0;
    long slots = 0;
    const int path = sp ? spmv_ap_axpby_route(first, sp, x16, &slots) : spmv_ap_hp_axpby_route(first, mid, hp, x16, &slots);
    const bool dots = op->d_dots != nullptr;
    const bool in_place = op->beta != 0.0 && op->d_z == (const void *)y;
    const size_t tmp_bytes = (path == 2 && in_place) ? (size_t)n * sizeof(HT) : 0;
    if (int rc = axpby_room(first, dots ? (size_t)slots : 0, tmp_bytes, st, true, who, reserve)) return rc;
    AxpbyArgs<HT> ep;
    ep.alpha = (HT)op->alpha; ep.beta = (HT)op->beta;
    ep.z = (const HT *)op->d_z; ep.w = (const HT *)op->d_w;
    ep.part = dots ? first->axpby_part.get() : nullptr;
    ep.n_dot = (long)op->n_dot_rows;
    if (n == 0) {
        slots = 0;
    } else if (path == 1) {
        int rc;
        if constexpr (sizeof(HT) == 8) rc = sp ? launch_spmv_ap(first, sp, x, nullptr, y, st, &ep) : launch_spmv_ap_hp(first, mid, hp, x, y, st, &ep);
        else rc = launch_spmv_ap_hp(first, mid, hp, x, y, st, &ep);
        if (rc) return rc;
    } else {
        // the plain call's own launch, then one pass over its result (an in-place call: the product goes to the temporary, y still holds z)
        HT *t = tmp_bytes ? (HT *)first->axpby_tmp.get() : y;
        int rc;
        if constexpr (sizeof(HT) == 8) rc = sp ? launch_spmv_ap(first, sp, x, nullptr, t, st) : launch_spmv_ap_hp(first, mid, hp, x, t, st);
        else rc = launch_spmv_ap_hp(first, mid, hp, x, t, st);
        if (rc) return rc;
        if (int rc2 = launch_axpby_pass<HT>(t, y, n, ep, st, &slots)) return rc2;
    }
    if (dots) return launch_axpby_finalize(ep.part, slots, op->d_dots, st);
    return USPMV_OK;
}

// the workspace of either family under the current tuning: the larger of the routed path's grid and the vector pass's (an x off the
// 16-byte grid leaves the plan), the in-place temporary only where a 16-byte-aligned x already takes path 2
int ap_axpby_reserve(uspmv_dmat *first, const uspmv_dmat *sp, const uspmv_dmat *mid, const uspmv_dmat *hp, const char *who) {
    if (int rc = require_device()) return rc;
    const long n = (long)first->n_chunks * first->C;
    long s1 = 0, s0 = 0;
    const int path = sp ? spmv_ap_axpby_route(first, sp, true, &s1) : spmv_ap_hp_axpby_route(first, mid, hp, true, &s1);
    if (sp) (void)spmv_ap_axpby_route(first, sp, false, &s0); else (void)spmv_ap_hp_axpby_route(first, mid, hp, false, &s0);
    const long slots = std::max(std::max(s1, s0), axpby_pass_slots(n));
    return axpby_room(first, (size_t)slots, path == 2 ? (size_t)n * uspmv_dtype_bytes(first->dtype) : 0, nullptr, false, who);
}

}  // namespace
}  // extern "C++"

int uspmv_spmv_ap_axpby(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, double *d_y, const uspmv_axpby_t *op, void *stream) {
    const char *who = "uspmv_spmv_ap_axpby";
    if (int rc = check_ap_pair(dp, sp, who)) return rc;
    if (int rc = ap_axpby_op_refusals(op, d_x, d_y, (long)dp->n_chunks * dp->C, sizeof(double), who)) return rc;
    if (int rc = require_device()) return rc;
    return spmv_ap_axpby_typed<double>(dp, sp, nullptr, nullptr, d_x, d_y, op, (hipStream_t)stream, who, "uspmv_spmv_ap_axpby_reserve");
}

int uspmv_spmv_ap_axpby_path(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const void *d_x, int *path) {
    const char *who = "uspmv_spmv_ap_axpby_path";
    if (int rc = check_ap_pair(dp, sp, who)) return rc;
    if (!d_x || !path) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    *path = spmv_ap_axpby_route(dp, sp, (uintptr_t)d_x % 16 == 0, nullptr);
    return USPMV_OK;
}

int uspmv_spmv_ap_axpby_reserve(uspmv_dmat_t *dp, const uspmv_dmat_t *sp) {
    const char *who = "uspmv_spmv_ap_axpby_reserve";
    if (int rc = check_ap_pair(dp, sp, who)) return rc;
    return ap_axpby_reserve(dp, sp, nullptr, nullptr, who);
}

int uspmv_spmv_ap_hp_axpby(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, void *d_y,
                           const uspmv_axpby_t *op, void *stream) {
    const char *who = "uspmv_spmv_ap_hp_axpby";
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    if (int rc = ap_axpby_op_refusals(op, d_x, d_y, (long)hi->n_chunks * hi->C, uspmv_dtype_bytes(hi->dtype), who)) return rc;
    if (int rc = require_device()) return rc;
    const char *reserve = "uspmv_spmv_ap_hp_axpby_reserve";
    if (hi->dtype == USPMV_F32)
        return spmv_ap_axpby_typed<float>(hi, nullptr, nullptr, hp, (const float *)d_x, (float *)d_y, op, (hipStream_t)stream, who, reserve);
    return spmv_ap_axpby_typed<double>(hi, nullptr, mid, hp, (const double *)d_x, (double *)d_y, op, (hipStream_t)stream, who, reserve);
}

int uspmv_spmv_ap_hp_axpby_path(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, int *path) {
    const char *who = "uspmv_spmv_ap_hp_axpby_path";
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    if (!d_x || !path) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    *path = spmv_ap_hp_axpby_route(hi, mid, hp, (uintptr_t)d_x % 16 == 0, nullptr);
    return USPMV_OK;
}

int uspmv_spmv_ap_hp_axpby_reserve(uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp) {
    const char *who = "uspmv_spmv_ap_hp_axpby_reserve";
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    return ap_axpby_reserve(hi, nullptr, mid, hp, who);
}

int uspmv_spmmv_ap(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const void *d_X, void *d_Y, int b, int64_t ld, int layout, void *stream) {
    const char *who = "uspmv_spmmv_ap";
    if (int rc = check_dmat(dp, who)) return rc;
    if (int rc = check_dmat(sp, who)) return rc;
    if (dp->dtype != USPMV_F64 || sp->dtype != USPMV_F32)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: expects a double and a float struct", who);
    if (dp->C != sp->C || dp->n_chunks != sp->n_chunks)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: dp and sp structs must share C and n_chunks", who);
    if (!d_X || !d_Y) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL vector", who);
    if (b < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: b=%d", who, b);
    if (layout != USPMV_COLWISE && layout != USPMV_ROWWISE) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown layout %d", who, layout);
    if (layout == USPMV_COLWISE && ld < dp->n_chunks * dp->C)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: ld=%lld smaller than n_rows_padded=%lld", who, (long long)ld,
                           (long long)(dp->n_chunks * dp->C));
    if (int rc = require_device()) return rc;
    if (dp->n_chunks == 0) return USPMV_OK;
    return launch_spmmv_ap(dp, sp, (const double *)d_X, (double *)d_Y, b, (long)ld, layout, (hipStream_t)stream);
}

int uspmv_spmmv_ap_path(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, int b, int64_t ld, int layout, int *path, int *vectors_per_pass) {
    const char *who = "uspmv_spmmv_ap_path";
    if (int rc = check_dmat(dp, who)) return rc;
    if (int rc = check_dmat(sp, who)) return rc;
    if (dp->dtype != USPMV_F64 || sp->dtype != USPMV_F32)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: expects a double and a float struct", who);
    if (dp->C != sp->C || dp->n_chunks != sp->n_chunks)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: dp and sp structs must share C and n_chunks", who);
    if (!path || !vectors_per_pass) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL result pointer", who);
    if (b < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: b=%d", who, b);
    if (layout != USPMV_COLWISE && layout != USPMV_ROWWISE) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown layout %d", who, layout);
    if (layout == USPMV_COLWISE && ld < dp->n_chunks * dp->C)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: ld=%lld smaller than n_rows_padded=%lld", who, (long long)ld,
                           (long long)(dp->n_chunks * dp->C));
    *path = 0; *vectors_per_pass = 0;
    if (b == 1) {  // uspmv_spmv_ap: its sweep kernel, its staged kernel or lane per row, one vector each
        if (dp->sw.on && sp->sw.on && dp->sw.tile_ids && dp->sw.n_parts >= 2 && dp->sw.plan_id == sp->sw.plan_id && g_tune.sweep) *path = 3;
        else if (dp->tlc.on && sp->tlc.on && dp->tlc.plan_id != 0 && dp->tlc.plan_id == sp->tlc.plan_id && g_tune.tlc) *path = 2;
        *vectors_per_pass = *path ? 1 : 0;
        return USPMV_OK;
    }
    spmmv_ap_path(dp, sp, b, (long)ld, layout, path, vectors_per_pass);
    return USPMV_OK;
}

// the checks the list forms of uspmv_spmmv_ap share: those of uspmv_spmv_ap_tiles / _chunks and of uspmv_spmmv_ap.  Nothing here
// touches a device.
static int check_ap_block_list(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, int b, int64_t ld, int layout, bool tiles, const char *who) {
    if (b < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: b=%d", who, b);
    if (layout != USPMV_COLWISE && layout != USPMV_ROWWISE) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown layout %d", who, layout);
    if (int rc = check_ap_pair(dp, sp, who)) return rc;
    if (layout == USPMV_COLWISE && ld < dp->n_chunks * dp->C)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: ld=%lld smaller than n_rows_padded=%lld", who, (long long)ld, (long long)(dp->n_chunks * dp->C));
    if (tiles && (!dp->tlc.on || !sp->tlc.on || dp->tlc.plan_id == 0 || dp->tlc.plan_id != sp->tlc.plan_id))
        return uspmv::fail(USPMV_ERR_INVALID, "%s: the pair has no shared tile-local-column plan (uspmv_dmat_optimize_ap)", who);
    return USPMV_OK;
}

int uspmv_spmmv_ap_tiles(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const int32_t *d_tile_ids, int64_t n_ids, const void *d_X, void *d_Y,
                         int b, int64_t ld, int layout, void *stream) {
    const char *who = "uspmv_spmmv_ap_tiles";
    if (int rc = check_ap_block_list(dp, sp, b, ld, layout, true, who)) return rc;
    if (n_ids < 0 || n_ids > dp->tlc.n_tiles || (n_ids > 0 && !d_tile_ids) || !d_X || !d_Y) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (n_ids == 0) return USPMV_OK;
    if (int rc = require_device()) return rc;
    return launch_spmmv_ap_tiles(dp, sp, d_tile_ids, (long)n_ids, (const double *)d_X, (double *)d_Y, b, (long)ld, layout, (hipStream_t)stream);
}

int uspmv_spmmv_ap_chunks(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const int32_t *d_chunk_ids, int64_t n_ids, const void *d_X, void *d_Y,
                          int b, int64_t ld, int layout, void *stream) {
    const char *who = "uspmv_spmmv_ap_chunks";
    if (int rc = check_ap_block_list(dp, sp, b, ld, layout, false, who)) return rc;
    if (n_ids < 0 || n_ids > dp->n_chunks || (n_ids > 0 && !d_chunk_ids) || !d_X || !d_Y) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    if (n_ids == 0) return USPMV_OK;
    if (int rc = require_device()) return rc;
    return launch_spmmv_ap_chunks(dp, sp, d_chunk_ids, (long)n_ids, (const double *)d_X, (double *)d_Y, b, (long)ld, layout, (hipStream_t)stream);
}

int uspmv_spmmv_ap_tiles_path(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, int b, int64_t ld, int layout, int *path, int *vectors_per_pass) {
    const char *who = "uspmv_spmmv_ap_tiles_path";
    if (int rc = check_ap_block_list(dp, sp, b, ld, layout, true, who)) return rc;
    if (!path || !vectors_per_pass) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL result pointer", who);
    spmmv_ap_tiles_path(dp, sp, b, (long)ld, layout, path, vectors_per_pass);
    return USPMV_OK;
}

int uspmv_spmmv_ap_sweep_vectors(int b, int wlog, int *vectors) {
    if (b < 1 || wlog < 8 || wlog > 16 || !vectors) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv_ap_sweep_vectors: bad argument");
    *vectors = spmmv_ap_sweep_vectors(b, wlog);
    return USPMV_OK;
}

int uspmv_spmmv_ap_plan_lines(int b, int *max_lines) {
    if (b < 1 || !max_lines) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_spmmv_ap_plan_lines: bad argument");
    *max_lines = spmmv_ap_plan_lines(b);
    return USPMV_OK;
}

// Opt-in plan cache of the raw-array entry points (tuning key "raw_plan_cache"): the reference's function-pointer
// seam passes the same device arrays on every call (code/classes_structs.hpp:997-1034), so the first call wraps them,
// builds the tile-local-column plan on the device and later calls run the plan kernel.  Keyed on the array
// addresses and shape -- the caller promises not to put a different matrix behind the same pointers
// (uspmv_raw_plan_cache_clear() after freeing them; uspmv_raw_plan_cache_values_changed() after rewriting the values of the same
// pattern: the refresh of csrc/refresh_kernels.hip on every plan behind that pointer).  Mutex-guarded; a handful of entries.
namespace {
struct RawKey { const void *cp, *cl, *ci, *va; int64_t C, n_chunks; int dtype; };
struct RawEntry { RawKey k; uspmv_dmat_t *A; };
std::vector<RawEntry> g_raw_cache;
std::mutex g_raw_mutex;

const uspmv_dmat *raw_cached(const RawKey &k) {
    std::lock_guard<std::mutex> lock(g_raw_mutex);
    for (const RawEntry &e : g_raw_cache)
        if (e.k.cp == k.cp && e.k.cl == k.cl && e.k.ci == k.ci && e.k.va == k.va && e.k.C == k.C && e.k.n_chunks == k.n_chunks && e.k.dtype == k.dtype)
            return e.A;
    int32_t last = 0;
    if (hipMemcpy(&last, (const int32_t *)k.cp + k.n_chunks, 4, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    uspmv_dmat_t *A = nullptr;
    if (uspmv_dmat_wrap(k.C, k.n_chunks, last, k.dtype, (const int32_t *)k.cp, (const int32_t *)k.cl, (const int32_t *)k.ci, k.va, &A)) return nullptr;
    if (uspmv_dmat_optimize_device(A, 0, nullptr, nullptr)) { uspmv_dmat_free(A); return nullptr; }
    if (g_raw_cache.size() >= 16) { uspmv_dmat_free(g_raw_cache.front().A); g_raw_cache.erase(g_raw_cache.begin()); }
    g_raw_cache.push_back(RawEntry{k, A});
    return A;
}
}  // namespace

void uspmv_raw_plan_cache_clear(void) {
    std::lock_guard<std::mutex> lock(g_raw_mutex);
    for (RawEntry &e : g_raw_cache) uspmv_dmat_free(e.A);
    g_raw_cache.clear();
}

int uspmv_raw_plan_cache_values_changed(const void *d_values, void *stream, int *n_entries) {
    if (n_entries) *n_entries = 0;
    if (!d_values) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_raw_plan_cache_values_changed: NULL argument");
    std::lock_guard<std::mutex> lock(g_raw_mutex);
    for (RawEntry &e : g_raw_cache) {
        if (e.k.va != d_values) continue;
        if (int rc = uspmv_dmat_values_changed(e.A, stream, nullptr)) return rc;
        if (n_entries) ++*n_entries;
    }
    return USPMV_OK;
}

#define RAW_SCS(SUF, VT, DT)                                                                                        \
    int uspmv_scs_gpu_##SUF(int64_t C, int64_t n_chunks, const int32_t *cp, const int32_t *cl, const int32_t *ci,   \
                            const VT *va, const VT *x, VT *y, void *stream) {                                       \
        if (C < 1 || n_chunks < 0 || !cp || (n_chunks > 0 && (!cl || !ci || !va || !x || !y)))                      \
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_scs_gpu_" #SUF ": bad argument");                          \
        if (int rc = require_device()) return rc;                                                                   \
        uspmv_dmat A;                                                                                               \
        A.C = C; A.n_chunks = n_chunks; A.dtype = DT; A.chunk_ptrs = cp; A.chunk_lengths = cl; A.col_idxs = ci;     \
        A.n_store = (long)(C * n_chunks);                                                                           \
        A.values = va;                                                                                              \
        if (int rc = check_dmat(&A, "uspmv_scs_gpu_" #SUF)) return rc;                                              \
        if (g_tune.raw_plan_cache && n_chunks > 0)                                                                  \
            if (const uspmv_dmat *P = raw_cached(RawKey{cp, cl, ci, va, C, n_chunks, DT}))                          \
                return launch_spmv_scs<VT>(P, nullptr, 0, x, y, (hipStream_t)stream);                               \
        return launch_spmv_scs<VT>(&A, nullptr, 0, x, y, (hipStream_t)stream);                                      \
    }                                                                                                               \
    int uspmv_csr_gpu_##SUF(int64_t n_rows, const int32_t *rp, const int32_t *ci, const VT *va, const VT *x, VT *y, \
                            void *stream) {                                                                         \
        if (n_rows < 0 || !rp || (n_rows > 0 && (!x || !y)))                                                        \
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_csr_gpu_" #SUF ": bad argument");                          \
        if (int rc = require_device()) return rc;                                                                   \
        return launch_csr<VT>((long)n_rows, 0, rp, ci, va, x, y, (hipStream_t)stream);                              \
    }
RAW_SCS(f64, double, USPMV_F64)
RAW_SCS(f32, float, USPMV_F32)
#undef RAW_SCS

static int peek_bytes(const void *p, void *out, size_t n, const char *who) {
    if (!p || !out) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) { (void)hipGetLastError(); memcpy(out, p, n); return USPMV_OK; }   // not known to the runtime: plain host memory
    if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) {
        HIP_TRY(hipMemcpy(out, p, n, hipMemcpyDeviceToHost));
        return USPMV_OK;
    }
    memcpy(out, p, n);
    return USPMV_OK;
}
int uspmv_peek_i64(const void *p, int64_t *out) { return peek_bytes(p, out, 8, "uspmv_peek_i64"); }
int uspmv_peek_i32(const void *p, int32_t *out) { return peek_bytes(p, out, 4, "uspmv_peek_i32"); }

int uspmv_apply_permutation_dev(void *d_out, const void *d_in, const int32_t *d_perm, int64_t n, int dtype,
                                void *stream) {
    if (!d_out || !d_in || !d_perm || n < 0) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_apply_permutation_dev: bad argument");
    if (int rc = require_device()) return rc;
    if (n == 0) return USPMV_OK;
    const unsigned grid = grid_for(n, 256);
    if (dtype == USPMV_F64)
        hipLaunchKernelGGL((gather_kernel<double>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (double *)d_out,
                           (const double *)d_in, d_perm, (const int *)nullptr, (long)n, 0L);
    else if (dtype == USPMV_F32)
        hipLaunchKernelGGL((gather_kernel<float>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (float *)d_out,
                           (const float *)d_in, d_perm, (const int *)nullptr, (long)n, 0L);
    else return uspmv::fail(USPMV_ERR_INVALID, "uspmv_apply_permutation_dev: unknown dtype %d", dtype);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int uspmv_pack_send_buf(const void *d_x, const int32_t *d_perm, const int32_t *d_send_idxs, int64_t n,
                        int64_t block_offset, void *d_send, int dtype, void *stream) {
    if (n < 0 || (n > 0 && (!d_x || !d_perm || !d_send_idxs || !d_send)))
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_pack_send_buf: bad argument");
    if (int rc = require_device()) return rc;
    if (n == 0) return USPMV_OK;
    const unsigned grid = grid_for(n, 256);
    if (dtype == USPMV_F64)
        hipLaunchKernelGGL((gather_kernel<double>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (double *)d_send,
                           (const double *)d_x, d_perm, d_send_idxs, (long)n, (long)block_offset);
    else if (dtype == USPMV_F32)
        hipLaunchKernelGGL((gather_kernel<float>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (float *)d_send,
                           (const float *)d_x, d_perm, d_send_idxs, (long)n, (long)block_offset);
    else return uspmv::fail(USPMV_ERR_INVALID, "uspmv_pack_send_buf: unknown dtype %d", dtype);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // extern "C"
