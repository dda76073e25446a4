// Device half of the C ABI (include/uspmv.h): handles, tuning, the sweep and block plans, GPU-side conversion, the small gather /
// stream kernels and the entry points that dispatch into spmv_kernels.hip, spmmv_kernels.hip and ap_kernels.hip.  The SpMV planner
// (uspmv_dmat_optimize and its variants) is csrc/tlc_planner.hip.
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

// STREAM-style calibrators.  copy / triad: every thread moves eight 16-byte pieces, all loads issued before the first store
// (32 KiB in flight per 256-thread workgroup), non-temporal loads and stores -- the shape the guide's 6.3 TB/s copy has; the
// grid-stride form of round 1 (one 16-byte piece in flight per thread, plain stores) stopped at 4.9 TB/s.
__global__ void __launch_bounds__(256) stream_copy_kernel(double2 *__restrict__ a, const double2 *__restrict__ b, const long n2) {
    const long base = (long)blockIdx.x * (256 * 8) + threadIdx.x;
    double v[16];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long i = base + u * 256;
        if (i < n2) { const double *p = (const double *)(b + i); v[2 * u] = __builtin_nontemporal_load(p); v[2 * u + 1] = __builtin_nontemporal_load(p + 1); }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long i = base + u * 256;
        if (i < n2) { double *p = (double *)(a + i); __builtin_nontemporal_store(v[2 * u], p); __builtin_nontemporal_store(v[2 * u + 1], p + 1); }
    }
}
__global__ void __launch_bounds__(256) stream_triad_kernel(double2 *__restrict__ a, const double2 *__restrict__ b,
                                                          const double2 *__restrict__ c, const double s, const long n2) {
    const long base = (long)blockIdx.x * (256 * 4) + threadIdx.x;
    double vb[8], vc[8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i = base + u * 256;
        if (i < n2) {
            const double *pb = (const double *)(b + i), *pc = (const double *)(c + i);
            vb[2 * u] = __builtin_nontemporal_load(pb); vb[2 * u + 1] = __builtin_nontemporal_load(pb + 1);
            vc[2 * u] = __builtin_nontemporal_load(pc); vc[2 * u + 1] = __builtin_nontemporal_load(pc + 1);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i = base + u * 256;
        if (i < n2) {
            double *p = (double *)(a + i);
            __builtin_nontemporal_store(vb[2 * u] + s * vc[2 * u], p); __builtin_nontemporal_store(vb[2 * u + 1] + s * vc[2 * u + 1], p + 1);
        }
    }
}
__global__ void stream_read_kernel(const double2 *__restrict__ b, const long n2, double *__restrict__ partial) {
    double acc = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
        const double *pb = (const double *)(b + i);
        acc += __builtin_nontemporal_load(pb) + __builtin_nontemporal_load(pb + 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) partial[((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6] = acc;
}

// Second yardstick (what the tile-local-column kernel asks of the cache hierarchy beyond a stream): as many workgroups as the SpMV has
// tiles, mapped to the XCDs like its tiles, each reading the x lines a `rows`-row tile of a 27-point stencil touches -- nine runs of
// rows + 2 elements (rounded out to whole 128-byte lines) at the offsets {-plane, 0, +plane} + {-line, 0, +line} around its own rows --
// with the plain 16-byte loads of the kernel's staging phase.  Every element of x is asked for by ~9 workgroups, ~3 of them far apart
// in launch order (the neighbouring planes): what comes from the XCD's L2, what from the fabric, is exactly the SpMV's x traffic,
// without its matrix stream.  Reported as gathered bytes per second.
__global__ void __launch_bounds__(256) stream_gather_lines_kernel(const double2 *__restrict__ x, const long n, const long plane, const long line,
                                                                  const int rows, const int xcd_remap, double *__restrict__ partial) {
    const unsigned tile = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const long base = (long)tile * rows;
    double acc = 0.0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
            long lo = base + dz * plane + dy * line - 1, hi = base + rows + dz * plane + dy * line + 1;
            lo = lo < 0 ? 0 : (lo & ~15L);
            hi = hi > n ? n : hi;
            hi = (hi + 15) & ~15L;
            if (hi > (n & ~15L)) hi = n & ~15L;
            for (long i = lo / 2 + threadIdx.x; i < hi / 2; i += 256) { const double2 v = x[i]; acc += v.x + v.y; }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) partial[(long)blockIdx.x * 4 + (threadIdx.x >> 6)] = acc;
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

// the argument checks uspmv_spmmv_ap_hp and uspmv_spmmv_ap_hp_path share
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

extern "C++" {
namespace uspmv_dev {

static int part_build(uspmv_dmat *A, int order, int rows_per_flag, const unsigned char *d_flags) {
    auto &len = A->part_len[order];
    len[0].reset(); len[1].reset();
    const size_t bytes = 4 * (size_t)std::max<int64_t>(A->n_chunks, 1);
    hipError_t e = len[0].alloc(bytes);
    if (e == hipSuccess) e = len[1].alloc(bytes);
    int rc = e == hipSuccess ? launch_part_len_fill(A, rows_per_flag, d_flags, A->part_len[order][0], A->part_len[order][1], nullptr)
                             : uspmv::fail(USPMV_ERR_ALLOC, "two-part SpMMV: %s", hipGetErrorString(e));
    if (!rc && (e = hipStreamSynchronize(nullptr)) != hipSuccess) rc = uspmv::fail(USPMV_ERR_HIP, "two-part SpMMV: %s", hipGetErrorString(e));
    if (rc) { len[0].reset(); len[1].reset(); }
    return rc;
}

int dmat_part_set_chunks(uspmv_dmat *A, const unsigned char *h_chunk_flags) {
    DeviceBuf<unsigned char> f;
    HIP_TRY(f.upload(h_chunk_flags, (size_t)A->n_chunks));
    return part_build(A, 0, (int)A->C, f);
}

int dmat_part_set_plan(uspmv_dmat *A, long n_local, int64_t *n_boundary_tiles) {
    A->part_len[1][0].reset(); A->part_len[1][1].reset();
    if (n_boundary_tiles) *n_boundary_tiles = 0;
    if (!A->pb.on || A->pb.n_tiles == 0) return USPMV_OK;
    DeviceBuf<unsigned char> f;
    HIP_TRY(f.alloc((size_t)A->pb.n_tiles));
    if (int rc = launch_block_tile_class(A, n_local, f, nullptr)) return rc;
    if (n_boundary_tiles) {
        std::vector<unsigned char> h((size_t)A->pb.n_tiles);
        HIP_TRY(hipMemcpy(h.data(), f, h.size(), hipMemcpyDeviceToHost));
        for (unsigned char v : h) *n_boundary_tiles += v;
    }
    return part_build(A, 1, 64, f);
}

}  // namespace uspmv_dev
}  // extern "C++"

int uspmv_dmat_optimize_block(uspmv_dmat_t *A, const uspmv_scs_t *s, int block_vec_size, int64_t *n_tiles, int64_t *n_staged) {
    if (!A || !s) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block: NULL argument");
    if (int rc = check_dmat_one_prec(A, "uspmv_dmat_optimize_block")) return rc;
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block: layout-only struct; the plan builder needs the host column indices");
    if (A->C != s->C || A->n_chunks != s->n_chunks || A->dtype != s->dtype)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block: handle and host struct do not describe the same matrix");
    if (block_vec_size < 1) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block: block_vec_size must be >= 1");
    if (int rc = require_device()) return rc;
    block_plan_reset(A);
    if (n_tiles) *n_tiles = 0;
    if (n_staged) *n_staged = 0;
    // a struct rebuilt from the handle's device arrays (uspmv_dmat_optimize_block_device) carries the indices only: the plan's private
    // copies of the VALUES are then gathered on the device from the handle's own array (launch_block_values_gather)
    const bool host_values = (int64_t)(s->dtype == USPMV_F64 ? s->values_f64.size() : s->values_f32.size()) == s->n_elements;
    const size_t row_bytes = (size_t)block_vec_size * (s->dtype == USPMV_F64 ? 8 : 4);
    // only the 16-byte-piece kernels (b*sizeof(VT) in {16,32,64,128}) read the plan, compiled for C = 32 and 64
    if (row_bytes % 16 != 0 || (row_bytes & (row_bytes - 1)) != 0 || row_bytes > 128 || (s->C != 32 && s->C != 64)) return USPMV_OK;
    const size_t cap = g_tune.spmmv_lds_kb > 0 ? std::min<size_t>((size_t)g_tune.spmmv_lds_kb * 1024, BT_LDS_CAP) : BT_LDS_CAP;
    const int max_rows = (int)(cap / row_bytes);
    // rows of >= 64 bytes on C = 32: 32-row tiles, two lanes per row (half the LDS per tile, twice the tiles per CU)
    const int tile_rows = (s->C == 32 && g_tune.spmmv_tile_rows != 64 && (row_bytes >= 128 || (row_bytes >= 32 && g_tune.spmmv_tile_rows == 32))) ? 32 : 64;
    uspmv_tlc_plan p;
    uspmv_scs r;                       // private copy with the sigma sort's ties undone (only kept when rows moved)
    std::vector<int32_t> row_map;
    const bool moved = g_tune.spmmv_reorder && (g_tune.spmmv_reorder == 3 ? uspmv_scs_reorder_bricks(s, g_tune.spmmv_brick_stride, g_tune.spmmv_brick_lines, &r, &row_map)
                                                                          : uspmv_scs_reorder_rows(s, g_tune.spmmv_reorder == 2 ? 2 : (g_tune.spmmv_reorder == 4 && !g_tune.spmmv_xline) ? 4 : 1, &r, &row_map)) == 1;
    // (with the line plan requested -- "spmmv_xline": X staged by 128-byte lines of the column-major vector -- the rows stay in original order,
    //  ties undone: a patch of several mesh lines touches more LINES of X than a run of consecutive rows)
    // 64-byte rows: the phased plan over the same (re-ordered) entries -- what uspmv_spmmv runs by default.  When the phased kernel
    // can take it (at most 512 rows per phase), the one-list-per-tile plan of the older kernels and its column-major copy of the entries
    // (8 + 6 bytes per non-zero of HBM, a second or two of planning) are only built on request ("spmmv_list_plan" 1).
    uspmv_phased_plan pp;
    if (row_bytes == 64 && tile_rows == 64 && g_tune.spmmv_phased)
        if (int rc = uspmv_build_phased_plan(moved ? &r : s, g_tune.spmmv_phase_rows, 8, &pp, 0, g_tune.spmmv_phase_dp)) return rc;
    const bool phased_ok = pp.valid && pp.ngp <= 8 && (pp.max_rows_used * 4 + 255) / 256 <= 8;
    // ... and once more with LINE lists for column-major block vectors (no re-layout pass over X): kept when no phase needs more
    // than 256 rows' worth of lines and the lines staged stay below twice the rows the row plan stages
    uspmv_phased_plan pl;
    if (phased_ok && g_tune.spmmv_xline && g_tune.spmmv_phase_rows == 256) {
        const int shift = s->dtype == USPMV_F64 ? 4 : 5;
        if (int rc = uspmv_build_phased_plan(moved ? &r : s, 256, 8, &pl, shift)) return rc;
        if (getenv("USPMV_VERBOSE")) {
            int64_t over = 0;
            for (int64_t ph = 0; ph < pl.n_phases; ++ph) over += (pl.ph_list_ptr[(size_t)ph + 1] - pl.ph_list_ptr[(size_t)ph]) > (256 >> shift);
            fprintf(stderr, "[uspmv] line plan candidate: valid=%d phases=%lld lines_total=%zu (= %zu rows; row plan stages %zu) max_rows=%d phases over the cap: %lld\n",
                    (int)pl.valid, (long long)pl.n_phases, pl.xrows.size(), pl.xrows.size() << shift, pp.xrows.size(), pl.max_rows_used, (long long)over);
        }
        if (pl.valid && (pl.max_rows_used > 256 || pl.ngp > 8 || ((int64_t)pl.xrows.size() << shift) > 2 * (int64_t)pp.xrows.size())) pl.valid = false;
    }
    // ... and once more over ORIGINAL X-row numbering (column index c -> new_to_old[c]) for column-major callers: their re-layout pass
    // undoes the sigma permutation on the way, so the rows a tile needs are runs of the workspace again
    uspmv_phased_plan pu;
    const bool have_perm = host_values && s->sigma > 1 && (int64_t)s->new_to_old_idx.size() >= s->n_rows && (int64_t)s->old_to_new_idx.size() >= s->n_rows;
    if (phased_ok && g_tune.spmmv_unscramble && have_perm && pp.max_rows_used <= 256 && g_tune.spmmv_idx8) {
        uspmv_scs u;                                    // indices only: a struct with the renumbered columns
        const uspmv_scs *src = moved ? &r : s;
        u.C = src->C; u.sigma = src->sigma; u.n_rows = src->n_rows; u.n_cols = src->n_cols; u.n_rows_padded = src->n_rows_padded; u.n_chunks = src->n_chunks;
        u.n_elements = src->n_elements; u.nnz = src->nnz; u.dtype = src->dtype;
        u.chunk_ptrs = src->chunk_ptrs; u.chunk_lengths = src->chunk_lengths;
        u.col_idxs.resize(src->col_idxs.size());
        const int32_t *n2o = s->new_to_old_idx.data();
        const int64_t nr = s->n_rows;
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < (int64_t)src->col_idxs.size(); ++k) { const int32_t c = src->col_idxs[(size_t)k]; u.col_idxs[(size_t)k] = c < nr ? n2o[c] : c; }
        if (int rc = uspmv_build_phased_plan(&u, 256, 8, &pu, 0, g_tune.spmmv_phase_dp)) return rc;
        if (pu.valid && (pu.max_rows_used > 256 || pu.ngp > 8)) pu.valid = false;
    }
    const bool list_plan = !phased_ok || g_tune.spmmv_list_plan;
    if (list_plan) {
        if (int rc = uspmv_build_tlc_plan(moved ? &r : s, nullptr, max_rows, tile_rows, &p, /*line_shift=*/0)) return rc;
        if (n_tiles) *n_tiles = p.n_tiles;
        if (n_staged) *n_staged = p.valid ? p.n_staged_tiles : 0;
        if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] block plan: b=%d tile_rows=%d tiles=%lld staged=%lld max_rows=%d (cap %d) rows_total=%zu\n",
                                             block_vec_size, p.tile_rows, (long long)p.n_tiles, (long long)p.n_staged_tiles, p.max_lines_used, max_rows, p.tile_lines.size());
        if (!p.valid && !pp.valid) return USPMV_OK;
    } else {
        if (n_tiles) *n_tiles = pp.n_tiles;
        if (n_staged) *n_staged = pp.n_tiles;
    }
    hipError_t e = hipSuccess;
    if (moved) e = A->bt.row_map.upload(row_map.data(), row_map.size() * 4);
    if (list_plan && p.valid) {
        if (e == hipSuccess) e = A->bt.line_ptr.upload(p.tile_line_ptr.data(), p.tile_line_ptr.size() * 4);
        if (e == hipSuccess) e = A->bt.xrows.upload(p.tile_lines.data(), p.tile_lines.size() * 4);
        if (e == hipSuccess) e = A->bt.c16_ptrs.upload(p.c16_ptrs.data(), p.c16_ptrs.size() * 4);
        if (e == hipSuccess) e = A->bt.col16.upload(p.col16.data(), p.col16.size() * 2);
        if (e == hipSuccess && moved) {
            if (host_values) e = A->bt.values.upload(r.values_ptr(), (size_t)r.n_elements * (r.dtype == USPMV_F64 ? 8 : 4));
            else {
                e = A->bt.values.alloc(std::max<size_t>((size_t)r.n_elements, 1) * (r.dtype == USPMV_F64 ? 8 : 4));
                if (e == hipSuccess && launch_block_values_gather(A, A->bt.row_map, nullptr, A->bt.values, false, nullptr) != USPMV_OK) e = hipErrorUnknown;
            }
            if (e == hipSuccess && (p.n_staged_tiles < p.n_tiles || g_tune.spmmv_variant == 5)) e = A->bt.cols.upload(r.col_idxs.data(), (size_t)r.n_elements * 4);
        }
    }
    if (e == hipSuccess && pp.valid) {
        {
            e = A->pb.ph_ptr.upload(pp.ph_ptr.data(), pp.ph_ptr.size() * 4);
            if (e == hipSuccess) e = A->pb.g0.upload(pp.ph_g0.data(), pp.ph_g0.size() * 4);
            if (e == hipSuccess) e = A->pb.list_ptr.upload(pp.ph_list_ptr.data(), pp.ph_list_ptr.size() * 4);
            if (e == hipSuccess) e = A->pb.xrows.upload(pp.xrows.data(), pp.xrows.size() * 4);
            if (e == hipSuccess) e = A->pb.c16_ptrs.upload(pp.c16_ptrs.data(), pp.c16_ptrs.size() * 4);
            A->pb.idx8 = g_tune.spmmv_idx8 && pp.max_rows_used <= 256;
            if (e == hipSuccess && A->pb.idx8) {             // same layout, one byte per entry
                std::vector<uint8_t> c8(pp.col16.size());
                for (size_t k = 0; k < c8.size(); ++k) c8[k] = (uint8_t)pp.col16[k];
                e = A->pb.col16.upload(c8.data(), c8.size());
            } else if (e == hipSuccess) e = A->pb.col16.upload(pp.col16.data(), pp.col16.size() * 2);
            if (e == hipSuccess && !host_values) {
                const size_t vs = s->dtype == USPMV_F64 ? 8 : 4;
                e = A->pb.values.zeros(std::max<size_t>(pp.col16.size(), 1) * vs);     // padded slots of the last group of a chunk
                if (e == hipSuccess && launch_block_values_gather(A, moved ? A->bt.row_map : nullptr, A->pb.c16_ptrs, A->pb.values, true, nullptr) != USPMV_OK) e = hipErrorUnknown;
                if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
            } else if (e == hipSuccess) {
                // the entries once more, group-major like the indices (what scs_spmmv_quadph streams)
                const uspmv_scs *src = moved ? &r : s;
                const size_t vs = src->dtype == USPMV_F64 ? 8 : 4;
                std::vector<unsigned char> gv(pp.col16.size() * vs, 0);
                const int64_t C_ = src->C;
#pragma omp parallel for schedule(static)
                for (int64_t c = 0; c < src->n_chunks; ++c) {
                    const int64_t cs = src->chunk_ptrs[(size_t)c], L = src->chunk_lengths[(size_t)c];
                    const size_t base = pp.c16_ptrs[(size_t)c];
                    for (int64_t j = 0; j < L; ++j)
                        for (int64_t i = 0; i < C_; ++i) {
                            const size_t dst = base + (size_t)((j / 4) * 4 * C_ + i * 4 + (j % 4)), from = (size_t)(cs + j * C_ + i);
                            if (vs == 8) ((double *)gv.data())[dst] = src->values_f64[from]; else ((float *)gv.data())[dst] = src->values_f32[from];
                        }
                }
                e = A->pb.values.upload(gv.data(), gv.size());
            }
            if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] phased block plan: tiles=%lld phases=%lld rows_total=%zu max_rows=%d (cap %d)\n",
                                                 (long long)pp.n_tiles, (long long)pp.n_phases, pp.xrows.size(), pp.max_rows_used, pp.cap_rows);
            if (e == hipSuccess && pu.valid) {
                e = A->pu.ph_ptr.upload(pu.ph_ptr.data(), pu.ph_ptr.size() * 4);
                if (e == hipSuccess) e = A->pu.g0.upload(pu.ph_g0.data(), pu.ph_g0.size() * 4);
                if (e == hipSuccess) e = A->pu.list_ptr.upload(pu.ph_list_ptr.data(), pu.ph_list_ptr.size() * 4);
                if (e == hipSuccess) e = A->pu.xrows.upload(pu.xrows.data(), pu.xrows.size() * 4);
                if (e == hipSuccess) e = A->pu.perm.upload(s->old_to_new_idx.data(), (size_t)s->n_rows * 4);
                if (e == hipSuccess) {
                    std::vector<uint8_t> c8(pu.col16.size());
                    for (size_t k = 0; k < c8.size(); ++k) c8[k] = (uint8_t)pu.col16[k];
                    e = A->pu.col8.upload(c8.data(), c8.size());
                }
                if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] unscrambled plan (column-major X behind the permuting re-layout): phases=%lld rows_total=%zu (scrambled: %zu) max_rows=%d\n",
                                                     (long long)pu.n_phases, pu.xrows.size(), pp.xrows.size(), pu.max_rows_used);
            }
            if (e == hipSuccess && pl.valid) {
                e = A->pl.ph_ptr.upload(pl.ph_ptr.data(), pl.ph_ptr.size() * 4);
                if (e == hipSuccess) e = A->pl.g0.upload(pl.ph_g0.data(), pl.ph_g0.size() * 4);
                if (e == hipSuccess) e = A->pl.list_ptr.upload(pl.ph_list_ptr.data(), pl.ph_list_ptr.size() * 4);
                if (e == hipSuccess) e = A->pl.lines.upload(pl.xrows.data(), pl.xrows.size() * 4);
                if (e == hipSuccess) {
                    std::vector<uint8_t> c8(pl.col16.size());
                    for (size_t k = 0; k < c8.size(); ++k) c8[k] = (uint8_t)pl.col16[k];
                    e = A->pl.col8.upload(c8.data(), c8.size());
                }
                if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] line plan (column-major X): phases=%lld lines_total=%zu (= %zu rows) max_rows=%d\n",
                                                     (long long)pl.n_phases, pl.xrows.size(), pl.xrows.size() << pl.line_shift, pl.max_rows_used);
            }
        }
    }
    if (e != hipSuccess) {
        block_plan_reset(A);
        return uspmv::fail(USPMV_ERR_ALLOC, "uspmv_dmat_optimize_block: device copy failed: %s", hipGetErrorString(e));
    }
    if (pp.valid && pu.valid) { A->pu.on = true; A->pu.max_rows = pu.max_rows_used; A->pu.n_phases = pu.n_phases; A->pu.n_perm = s->n_rows; }
    if (pp.valid && pl.valid) { A->pl.on = true; A->pl.shift = pl.line_shift; A->pl.max_rows = pl.max_rows_used; A->pl.n_phases = pl.n_phases; A->pl.rows_staged = (int64_t)pl.xrows.size() << pl.line_shift; }
    if (pp.valid) { A->pb.on = true; A->pb.cap_rows = pp.cap_rows; A->pb.ngp = pp.ngp; A->pb.max_rows = pp.max_rows_used; A->pb.n_tiles = pp.n_tiles; A->pb.n_phases = pp.n_phases; A->pb.rows_staged = (int64_t)pp.xrows.size(); }
    if (list_plan && p.valid) { A->bt.on = true; A->bt.tile_rows = p.tile_rows; A->bt.max_rows = p.max_lines_used; A->bt.n_tiles = p.n_tiles; A->bt.staged = p.n_staged_tiles; }
    if (A->pb.on && g_tune.spmmv_stream > 0) return dmat_stream_schedule(A, g_tune.spmmv_stream);
    return USPMV_OK;
}

// The phased block plan built entirely on the device (csrc/block_plan_kernels.hip): row order, phases, X-row lists, one-byte indices and
// the group-major value copy; the host sees the chunk lengths (offsets of the index array) and two integers per tile (exclusive scans).
// Returns 1 when the shape / tuning is not the default one this builder covers (the caller then plans the index part on the host).
static int block_plan_install_device(uspmv_dmat_t *A, int block_vec_size, int64_t *n_tiles, int64_t *n_staged) {
    const size_t vsz = A->dtype == USPMV_F64 ? 8 : 4;
    const size_t row_bytes = (size_t)block_vec_size * vsz;
    if (row_bytes != 64 || (A->C != 32 && A->C != 64) || !g_tune.spmmv_phased || g_tune.spmmv_phase_rows != 256 || g_tune.spmmv_list_plan ||
        (g_tune.spmmv_reorder != 1 && g_tune.spmmv_reorder != 4) || !g_tune.spmmv_idx8 || g_tune.spmmv_tile_rows == 32 || g_tune.spmmv_xline || !g_tune.block_plan_device) return 1;
    const int64_t C = A->C, nc = A->n_chunks, n_pad = nc * C, nt = (n_pad + 63) / 64;
    block_plan_reset(A);
    std::vector<int32_t> cl((size_t)nc);
    std::vector<uint32_t> c16p;
    int64_t tot16 = 0;
    HIP_TRY(hipMemcpy(cl.data(), A->chunk_lengths, 4 * (size_t)nc, hipMemcpyDeviceToHost));
    if (!c16_offsets(cl, C, &c16p, &tot16)) return USPMV_OK;
    DeviceBuf<int> d_changed, d_tph, d_tl;
    hipError_t e = d_changed.zeros(8);
    int *const d_max = d_changed ? d_changed.get() + 1 : nullptr;
    if (e == hipSuccess) e = A->bt.row_map.alloc(4 * (size_t)std::max<int64_t>(n_pad, 1));
    if (e == hipSuccess) e = A->pb.c16_ptrs.upload(c16p.data(), 4 * ((size_t)nc + 1));
    if (e == hipSuccess) e = d_tph.alloc(4 * (size_t)nt);
    if (e == hipSuccess) e = d_tl.alloc(4 * (size_t)nt);
    auto fail_out = [&](const char *what) {
        block_plan_reset(A);
        return uspmv::fail(USPMV_ERR_HIP, "uspmv_dmat_optimize_block_device: %s: %s", what, hipGetErrorString(e));
    };
    if (e != hipSuccess) return fail_out("allocation");
    // ---- row order (ties of the sigma sort undone by first column), then the phases: count, scan, write
    int rc = launch_block_reorder(A, A->bt.row_map, d_changed, nullptr);
    int changed = 0;
    if (!rc) { e = hipMemcpy(&changed, d_changed, 4, hipMemcpyDeviceToHost); if (e != hipSuccess) return fail_out("row order"); }
    const int *rmap = changed ? A->bt.row_map : nullptr;
    if (!changed) A->bt.row_map.reset();
    if (!rc) rc = launch_block_phase_plan(A, false, 256, 8, rmap, A->pb.c16_ptrs, d_tph, d_tl, nullptr, nullptr, nullptr, nullptr, d_max, nullptr);
    std::vector<int32_t> tph((size_t)nt + 1, 0), tl((size_t)nt + 1, 0);
    if (!rc) {
        e = hipMemcpy(tph.data(), d_tph, 4 * (size_t)nt, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(tl.data(), d_tl, 4 * (size_t)nt, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail_out("phase counts");
    }
    if (rc) { block_plan_reset(A); return rc; }
    int64_t n_ph = 0, n_list = 0;
    for (int64_t t = 0; t < nt; ++t) {   // exclusive scans (ph_ptr of the plan; list bases)
        const int32_t a = tph[(size_t)t], b = tl[(size_t)t];
        tph[(size_t)t] = (int32_t)n_ph; tl[(size_t)t] = (int32_t)n_list;
        n_ph += a; n_list += b;
        if (n_ph > INT32_MAX || n_list > INT32_MAX) { block_plan_reset(A); return USPMV_OK; }
    }
    tph[(size_t)nt] = (int32_t)n_ph; tl[(size_t)nt] = (int32_t)n_list;
    if (n_tiles) *n_tiles = nt;
    if (n_staged) *n_staged = n_ph > 0 ? nt : 0;
    if (n_ph == 0) { block_plan_reset(A); return USPMV_OK; }
    e = A->pb.ph_ptr.upload(tph.data(), 4 * ((size_t)nt + 1));
    if (e == hipSuccess) e = hipMemcpy(d_tl, tl.data(), 4 * (size_t)nt, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = A->pb.g0.alloc(4 * (size_t)n_ph);
    if (e == hipSuccess) e = A->pb.list_ptr.alloc(4 * ((size_t)n_ph + 1));
    if (e == hipSuccess) e = A->pb.xrows.alloc(4 * (size_t)std::max<int64_t>(n_list, 1));
    if (e == hipSuccess) e = A->pb.col16.zeros((size_t)std::max<int64_t>(tot16, 1));
    if (e == hipSuccess) { const int32_t last = (int32_t)n_list; e = hipMemcpy(A->pb.list_ptr + n_ph, &last, 4, hipMemcpyHostToDevice); }
    if (e == hipSuccess) e = A->pb.values.zeros((size_t)std::max<int64_t>(tot16, 1) * vsz);
    if (e != hipSuccess) return fail_out("plan arrays");
    rc = launch_block_phase_plan(A, true, 256, 8, rmap, A->pb.c16_ptrs, A->pb.ph_ptr, d_tl, A->pb.g0, A->pb.list_ptr, A->pb.xrows, (unsigned char *)A->pb.col16, d_max, nullptr);
    if (!rc) rc = launch_block_values_gather(A, rmap, A->pb.c16_ptrs, A->pb.values, true, nullptr);
    int max_rows = 0;
    if (!rc) { e = hipMemcpy(&max_rows, d_max, 4, hipMemcpyDeviceToHost); if (e != hipSuccess) return fail_out("plan kernels"); }
    d_changed.reset(); d_tph.reset(); d_tl.reset();
    if (rc) { block_plan_reset(A); return rc; }
    A->pb.on = true; A->pb.idx8 = true; A->pb.device_built = true; A->pb.cap_rows = 256; A->pb.ngp = 8; A->pb.max_rows = max_rows; A->pb.n_tiles = nt; A->pb.n_phases = n_ph; A->pb.rows_staged = n_list;
    if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] phased block plan (device builder): tiles=%lld phases=%lld rows_total=%lld max_rows=%d rows %s\n",
                                         (long long)nt, (long long)n_ph, (long long)n_list, max_rows, changed ? "re-ordered" : "in the caller's order");
    if (g_tune.spmmv_stream > 0) return dmat_stream_schedule(A, g_tune.spmmv_stream);
    return USPMV_OK;
}

// The block plan for a handle whose arrays exist only in HBM (uspmv_dmat_wrap around a harness' own device arrays -- what the
// function-pointer launchers hold): the INDEX arrays (4 of the 12 bytes per non-zero) are copied to the host once, the index part of
// the plan (row order, phases, X-row lists, local indices) is built there like in uspmv_dmat_optimize_block and uploaded; the
// plan's copies of the VALUES (8 bytes per non-zero, group-major under the plan's row map) are gathered on the device from the
// handle's own array and never cross the bus.  Without the caller's permutation the tie re-ordering orders the rows of equal-length
// chunks by their first column (uspmv_scs_reorder_ties), which for locally numbered matrices restores the original row order.
int uspmv_dmat_optimize_block_device(uspmv_dmat_t *A, int block_vec_size, int64_t *n_tiles, int64_t *n_staged) {
    if (int rc = check_dmat_one_prec(A, "uspmv_dmat_optimize_block_device")) return rc;
    if (block_vec_size < 1) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block_device: block_vec_size must be >= 1");
    if (int rc = require_device()) return rc;
    uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;      // narrow chunks: the internal C = 32 re-chunking is what uspmv_spmmv runs on
    if (n_tiles) *n_tiles = 0;
    if (n_staged) *n_staged = 0;
    if ((M->C != 32 && M->C != 64) || M->n_chunks < 1) return USPMV_OK;
    {   // the default shape: everything on the device
        const int rc = block_plan_install_device(M, block_vec_size, n_tiles, n_staged);
        if (rc != 1) return rc;
    }
    uspmv_scs s;
    s.C = M->C; s.sigma = 0; s.n_chunks = M->n_chunks; s.n_rows = s.n_rows_padded = M->n_chunks * M->C; s.dtype = M->dtype;
    s.chunk_ptrs.resize((size_t)M->n_chunks + 1); s.chunk_lengths.resize((size_t)M->n_chunks);
    HIP_TRY(hipMemcpy(s.chunk_ptrs.data(), M->chunk_ptrs, 4 * ((size_t)M->n_chunks + 1), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s.chunk_lengths.data(), M->chunk_lengths, 4 * (size_t)M->n_chunks, hipMemcpyDeviceToHost));
    s.n_elements = s.chunk_ptrs[(size_t)M->n_chunks]; s.nnz = s.n_elements;
    s.col_idxs.resize((size_t)s.n_elements);
    HIP_TRY(hipMemcpy(s.col_idxs.data(), M->col_idxs, 4 * (size_t)s.n_elements, hipMemcpyDeviceToHost));
    int32_t mc = 0;
    for (int32_t c : s.col_idxs) mc = std::max(mc, c);
    s.n_cols = (int64_t)mc + 1;
    // (the values stay where they are: uspmv_dmat_optimize_block gathers the plan's private copies on the device)
    return uspmv_dmat_optimize_block(M, &s, block_vec_size, n_tiles, n_staged);
}

extern "C++" {
namespace uspmv_dev {

// What the two builders of a sweep plan do before they look at the matrix: a plan on the handles is dropped, the results are zeroed,
// wlog and tile_rows get their defaults (vsz: bytes of an x element, n_pad: padded rows), and a window that does not fit LDS is refused.
static int sweep_plan_defaults(uspmv_dmat_t *const parts[], int n_parts, size_t vsz, int64_t n_pad, int *wlog, int *tile_rows,
                               int64_t *n_tiles, int64_t *n_sweep, const char *who) {
    for (int k = 0; k < n_parts; ++k) parts[k]->sw = {};
    if (n_tiles) *n_tiles = 0;
    if (n_sweep) *n_sweep = 0;
    if (*wlog <= 0) *wlog = g_tune.sweep_wlog;
    const int nbuf = g_tune.sweep_nbuf == 2 ? 2 : 1;
    // window: as much of the LDS as one buffer per workgroup allows (128 KiB; 64 KiB each when double-buffered) -- on config 4b every
    // doubling from 8 KiB up paid (1.51 / 0.97 / 0.74 / 0.61 ms for the ap kernel at 2^10 .. 2^13 elements, 0.55 at 2^14 with 4 096-row
    // tiles; profiles/r02/config4b_sweep_variants.txt): fewer, longer rounds per wave and fewer barriers
    if (*wlog <= 0) *wlog = (vsz == 8 ? 13 : 14) + (nbuf == 1 ? 1 : 0);
    if (((size_t)1 << *wlog) * vsz * (size_t)nbuf > WG_LDS_BYTES)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: %d window buffer(s) of 2^%d elements do not fit the 160 KB of LDS", who, nbuf, *wlog);
    if (*tile_rows <= 0) *tile_rows = g_tune.sweep_tile_rows;
    // rows per tile: the windows are staged once per tile, so more rows = fewer staged bytes per non-zero (a lane owns up to four rows);
    // but at least ~1.5 tiles per CU
    if (*tile_rows <= 0) {
        *tile_rows = 4096;
        while (*tile_rows > 1024 && n_pad / *tile_rows < 384) *tile_rows /= 2;
    }
    return USPMV_OK;
}

// ... and after the arrays are on the first handle: the plan's metadata there; the other handles carry the plan id and the tile counts
static void sweep_plan_stamp(uspmv_dmat_t *const parts[], int n_parts, uint64_t id, int tile_rows, int wlog, int64_t n_sweep,
                             int64_t n_tiles, int64_t x_len, int64_t n_rest, int64_t cnt_bytes) {
    auto &w = parts[0]->sw;
    w.on = true; w.tile_rows = tile_rows; w.wlog = wlog; w.n_tiles = n_sweep; w.all_tiles = n_tiles;
    w.x_len = x_len; w.n_rest = n_rest; w.plan_id = id; w.cnt_bytes = cnt_bytes; w.n_parts = n_parts;
    for (int k = 1; k < n_parts; ++k) {
        auto &o = parts[k]->sw;
        o.on = true; o.plan_id = id; o.n_tiles = n_sweep; o.all_tiles = n_tiles;
    }
}

// builds and uploads a sweep plan for the one struct, or the n_parts parts of an ap split, behind parts / ss; returns the number of
// sweep tiles.  A plan on the handles is replaced.
int sweep_plan_install(uspmv_dmat_t *const parts[], const uspmv_scs_t *const ss[], int n_parts, int wlog, int tile_rows,
                       int64_t *n_tiles, int64_t *n_sweep, const char *who) {
    const uspmv_scs_t *s = ss[0];
    if (int rc = sweep_plan_defaults(parts, n_parts, s->dtype == USPMV_F64 ? 8 : 4, s->n_chunks * s->C, &wlog, &tile_rows, n_tiles, n_sweep, who))
        return rc;
    uspmv_sweep_plan p;
    const double max_stage = g_tune.sweep_max_stage > 0 ? (double)g_tune.sweep_max_stage : 24.0;
    if (int rc = uspmv_build_sweep_plan(ss, n_parts, wlog, tile_rows, max_stage, &p)) return rc;
    if (n_tiles) *n_tiles = p.n_tiles;
    if (n_sweep) *n_sweep = p.valid ? p.n_sweep_tiles : 0;
    if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] sweep plan: tile_rows=%d wlog=%d tiles=%lld sweep=%lld rest_chunks=%zu elements=%zu cnt_bytes=%zu\n",
                                         p.tile_rows, p.wlog, (long long)p.n_tiles, (long long)p.n_sweep_tiles, p.rest_chunks.size(), p.part[0].idx.size(), p.part[0].cnt.size());
    if (!p.valid) return USPMV_OK;
    auto &w = parts[0]->sw;
    hipError_t e = w.tile_ids.upload(p.tile_ids.data(), p.tile_ids.size() * 4);
    if (e == hipSuccess) e = w.smin.upload(p.t_smin.data(), p.t_smin.size() * 4);
    if (e == hipSuccess) e = w.S.upload(p.t_S.data(), p.t_S.size() * 4);
    if (e == hipSuccess) e = w.cnt_off.upload(p.t_cnt_off.data(), p.t_cnt_off.size() * 8);
    if (e == hipSuccess) e = w.rest.upload(p.rest_chunks.data(), p.rest_chunks.size() * 4);
    for (int k = 0; k < n_parts; ++k) {
        const auto &h = p.part[k];
        auto &d = w.part[k];
        d.dtype = h.dtype; d.n_vals = (int64_t)h.idx.size() - 64;
        if (e == hipSuccess) e = d.wave_off.upload(h.wave_off.data(), h.wave_off.size() * 4);
        if (e == hipSuccess) e = d.cnt.upload(h.cnt.data(), h.cnt.size());
        if (e == hipSuccess) e = d.vals.upload(h.vals(), h.idx.size() * uspmv_dtype_bytes(h.dtype));
        if (e == hipSuccess) e = d.idx.upload(h.idx.data(), h.idx.size() * 2);
        if (e == hipSuccess) e = d.pad.upload(h.pad_col.data(), h.pad_col.size() * 4);
    }
    if (e != hipSuccess) {
        w = {};
        return uspmv::fail(USPMV_ERR_ALLOC, "%s: device copy failed: %s", who, hipGetErrorString(e));
    }
    static uint64_t next_sweep_id = 1;
    sweep_plan_stamp(parts, n_parts, next_sweep_id++, p.tile_rows, p.wlog, p.n_sweep_tiles, p.n_tiles, p.x_len_min, (int64_t)p.rest_chunks.size(),
                     (int64_t)p.part[0].cnt.size());
    return USPMV_OK;
}

// The same plan from the handles' DEVICE arrays (csrc/sweep_plan_kernels.hip): a scan kernel per struct, the tile decisions and the
// offsets on the host (O(n_tiles); 16 bytes per 64-row group come back), a fill kernel per struct.  Same defaults, same criteria and
// -- by construction of the fill kernel -- the same arrays as sweep_plan_install builds from host structs.
int sweep_plan_install_device(uspmv_dmat_t *const parts[], int ns, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep,
                              const char *who) {
    uspmv_dmat_t *const A = parts[0];
    const int64_t C = A->C, nc = A->n_chunks, n_pad = nc * C;
    const size_t vsz = A->dtype == USPMV_F64 ? 8 : 4;
    if (int rc = sweep_plan_defaults(parts, ns, vsz, n_pad, &wlog, &tile_rows, n_tiles, n_sweep, who)) return rc;
    if (tile_rows != 256 && tile_rows != 512 && tile_rows != 1024 && tile_rows != 2048 && tile_rows != 4096) tile_rows = 1024;
    if (C < 1 || C > 64 || 64 % C != 0 || nc < 1 || wlog < 8 || wlog > 16) return USPMV_OK;
    for (int w = 0; w < ns; ++w) if (parts[w]->n_elements > (int64_t)UINT32_MAX) return USPMV_OK;
    const int64_t R = tile_rows, nt = (n_pad + R - 1) / R, wpt = R / 64, n_groups = (n_pad + 63) / 64;
    const double max_stage = g_tune.sweep_max_stage > 0 ? (double)g_tune.sweep_max_stage : 24.0;
    // ---- scan
    DeviceBuf<int> d_le[3], d_pad[3], d_grp[3], d_max;
    hipError_t e = d_max.zeros(4);
    for (int w = 0; w < ns && e == hipSuccess; ++w) {
        e = d_le[w].alloc(4 * (size_t)n_groups * 64);
        if (e == hipSuccess) e = d_pad[w].alloc(4 * (size_t)n_groups * 64);
        if (e == hipSuccess) e = d_grp[w].alloc(16 * (size_t)n_groups);
    }
    if (e != hipSuccess) return uspmv::fail(USPMV_ERR_ALLOC, "%s: %s", who, hipGetErrorString(e));
    std::vector<int32_t> grp[3];
    int max_col = 0;
    int rc = USPMV_OK;
    for (int w = 0; w < ns && !rc; ++w) rc = launch_sweep_scan(parts[w], wlog, d_le[w], d_pad[w], d_grp[w], d_max, nullptr);
    for (int w = 0; w < ns && !rc; ++w) {
        grp[w].resize((size_t)n_groups * 4);
        e = hipMemcpy(grp[w].data(), d_grp[w], 16 * (size_t)n_groups, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (!rc && hipMemcpy(&max_col, d_max, 4, hipMemcpyDeviceToHost) != hipSuccess) rc = uspmv::fail(USPMV_ERR_HIP, "%s: scan results", who);
    if (rc) return rc;
    // ---- which tiles sweep (sweep_plan.cpp pass 1), offsets
    std::vector<int32_t> tile_ids, t_smin, t_S, rest;
    std::vector<uint64_t> t_cnt_off;
    int64_t cnt_bytes = 0, tot[3] = {0, 0, 0};
    for (int64_t t = 0; t < nt; ++t) {
        int32_t lo = INT32_MAX, hi = -1;
        bool good = true;
        int64_t nnz_t = 0;
        for (int w = 0; w < ns; ++w)
            for (int64_t g = t * wpt; g < std::min((t + 1) * wpt, n_groups); ++g) {
                const int32_t *q = grp[w].data() + (size_t)g * 4;
                nnz_t += q[0]; lo = std::min(lo, q[1]); hi = std::max(hi, q[2]); good = good && !q[3];
            }
        const int64_t nS = (int64_t)hi - lo + 1;
        const bool ok = good && hi >= 0 && (double)nS * (double)((int64_t)1 << wlog) * (double)vsz <= max_stage * (double)std::max<int64_t>(nnz_t, 1) && nS <= 4096;
        if (!ok) { for (int64_t c = t * R / C; c < std::min((t + 1) * R / C, nc); ++c) rest.push_back((int32_t)c); continue; }
        tile_ids.push_back((int32_t)t); t_smin.push_back(lo); t_S.push_back((int32_t)nS); t_cnt_off.push_back((uint64_t)cnt_bytes);
        cnt_bytes += nS * R;
    }
    const int64_t nsw = (int64_t)tile_ids.size();
    if (n_tiles) *n_tiles = nt;
    if (n_sweep) *n_sweep = nsw;
    if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] sweep plan (device builder): tile_rows=%d wlog=%d tiles=%lld sweep=%lld rest_chunks=%zu cnt_bytes=%lld\n",
                                         tile_rows, wlog, (long long)nt, (long long)nsw, rest.size(), (long long)cnt_bytes);
    if (nsw == 0) return USPMV_OK;
    std::vector<uint32_t> wave_off[3];
    for (int w = 0; w < ns; ++w) {
        wave_off[w].assign((size_t)(nsw * wpt), 0);
        for (int64_t k = 0; k < nsw; ++k)
            for (int64_t v = 0; v < wpt; ++v) {
                wave_off[w][(size_t)(k * wpt + v)] = (uint32_t)tot[w];
                const int64_t g = (int64_t)tile_ids[(size_t)k] * wpt + v;
                if (g < n_groups) tot[w] += grp[w][(size_t)g * 4];
            }
        if (tot[w] > (int64_t)UINT32_MAX) return USPMV_OK;
    }
    // ---- device arrays of the plan
    constexpr size_t SPARE = 64;
    auto &sw = A->sw;
    if (e == hipSuccess) e = sw.tile_ids.upload(tile_ids.data(), tile_ids.size() * 4);
    if (e == hipSuccess) e = sw.smin.upload(t_smin.data(), t_smin.size() * 4);
    if (e == hipSuccess) e = sw.S.upload(t_S.data(), t_S.size() * 4);
    if (e == hipSuccess) e = sw.cnt_off.upload(t_cnt_off.data(), t_cnt_off.size() * 8);
    if (e == hipSuccess) e = sw.rest.upload(rest.data(), rest.size() * 4);
    for (int w = 0; w < ns; ++w) {
        auto &d = sw.part[w];
        d.dtype = parts[w]->dtype; d.n_vals = tot[w];
        if (e == hipSuccess) e = d.wave_off.upload(wave_off[w].data(), wave_off[w].size() * 4);
        if (e == hipSuccess) e = d.cnt.zeros((size_t)cnt_bytes);
        if (e == hipSuccess) e = d.vals.zeros(((size_t)tot[w] + SPARE) * uspmv_dtype_bytes(d.dtype));
        if (e == hipSuccess) e = d.idx.zeros(((size_t)tot[w] + SPARE) * 2);
        if (e == hipSuccess) e = d.pad.zeros((size_t)(nsw * R) * 4);
    }
    for (int w = 0; w < ns; ++w) {
        auto &d = sw.part[w];
        if (e == hipSuccess && launch_sweep_fill(parts[w], wlog, (int)R, (long)nsw, sw.tile_ids, sw.smin, sw.S, (const unsigned long long *)sw.cnt_off,
                                                 d.wave_off, d_le[w], d_pad[w], d.cnt, d.vals, d.idx, d.pad, nullptr) != USPMV_OK) e = hipErrorUnknown;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    for (int w = 0; w < 3; ++w) { d_le[w].reset(); d_pad[w].reset(); d_grp[w].reset(); }
    d_max.reset();
    if (e != hipSuccess) {
        sw = {};
        return uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    static uint64_t next_dev_sweep_id = (uint64_t)1 << 41;
    sweep_plan_stamp(parts, ns, next_dev_sweep_id++, tile_rows, wlog, nsw, nt, (int64_t)max_col + 1, (int64_t)rest.size(), cnt_bytes);
    return USPMV_OK;
}

}  // namespace uspmv_dev
}  // extern "C++"

int uspmv_dmat_optimize_sweep(uspmv_dmat_t *A, const uspmv_scs_t *s, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep) {
    if (!A || !s) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep: NULL argument");
    if (int rc = check_dmat_one_prec(A, "uspmv_dmat_optimize_sweep")) return rc;
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep: layout-only struct; the plan builder needs the host entries");
    if (A->C != s->C || A->n_chunks != s->n_chunks || A->dtype != s->dtype)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep: handle and host struct do not describe the same matrix");
    if (int rc = require_device()) return rc;
    return sweep_plan_install(&A, &s, 1, wlog, tile_rows, n_tiles, n_sweep, "uspmv_dmat_optimize_sweep");
}

int uspmv_dmat_optimize_sweep_ap(uspmv_dmat_t *dp, uspmv_dmat_t *sp, const uspmv_scs_t *s_dp, const uspmv_scs_t *s_sp, int wlog, int tile_rows,
                                 int64_t *n_tiles, int64_t *n_sweep) {
    if (!dp || !sp || !s_dp || !s_sp) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep_ap: NULL argument");
    if (!uspmv::scs_has_entries(s_dp) || !uspmv::scs_has_entries(s_sp))
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep_ap: layout-only struct; the plan builder needs the host entries");
    if (dp->C != s_dp->C || dp->n_chunks != s_dp->n_chunks || dp->dtype != USPMV_F64 || s_dp->dtype != USPMV_F64 ||
        sp->C != s_sp->C || sp->n_chunks != s_sp->n_chunks || sp->dtype != USPMV_F32 || s_sp->dtype != USPMV_F32 ||
        dp->C != sp->C || dp->n_chunks != sp->n_chunks)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep_ap: handles / host structs do not form a dp+sp pair");
    if (int rc = require_device()) return rc;
    uspmv_dmat_t *const ms[2] = {dp, sp};
    const uspmv_scs_t *const ss[2] = {s_dp, s_sp};
    return sweep_plan_install(ms, ss, 2, wlog, tile_rows, n_tiles, n_sweep, "uspmv_dmat_optimize_sweep_ap");
}

int uspmv_dmat_optimize_sweep_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, const uspmv_scs_t *s_hi, const uspmv_scs_t *s_mid,
                                    const uspmv_scs_t *s_hp, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep) {
    const char *who = "uspmv_dmat_optimize_sweep_ap_hp";
    if (!s_hi || !s_hp || (mid && !s_mid)) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    const uspmv_scs_t *ss[3] = {s_hi, mid ? s_mid : s_hp, mid ? s_hp : nullptr};
    uspmv_dmat_t *const ms[3] = {hi, mid ? mid : hp, mid ? hp : nullptr};
    for (int k = 0; k < 3; ++k) {
        if (!ms[k]) continue;
        if (!uspmv::scs_has_entries(ss[k])) return uspmv::fail(USPMV_ERR_INVALID, "%s: layout-only struct; the plan builder needs the host entries", who);
        if (ms[k]->C != ss[k]->C || ms[k]->n_chunks != ss[k]->n_chunks || ms[k]->dtype != ss[k]->dtype)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: handles and host structs do not describe the same parts", who);
    }
    if (int rc = require_device()) return rc;
    return sweep_plan_install(ms, ss, mid ? 3 : 2, wlog, tile_rows, n_tiles, n_sweep, who);
}

int uspmv_dmat_optimize_sweep_device_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, int wlog, int tile_rows, int64_t *n_tiles,
                                           int64_t *n_sweep) {
    const char *who = "uspmv_dmat_optimize_sweep_device_ap_hp";
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    if (int rc = require_device()) return rc;
    uspmv_dmat_t *const ms[3] = {hi, mid ? mid : hp, mid ? hp : nullptr};
    return sweep_plan_install_device(ms, mid ? 3 : 2, wlog, tile_rows, n_tiles, n_sweep, who);
}

// The block-vector column-window sweep plan (host/sweep_plan.cpp: uspmv_build_block_sweep_plan; kernel csrc/spmmv_sweep.hip) for 64-byte X
// rows.  Installed only when EVERY tile sweeps (rows column-sorted at window granularity, staging within "spmmv_sweep_max_stage" bytes
// per non-zero); otherwise the handle keeps whatever block plan it has.  wlog / tile_rows 0 = defaults (2^11 rows = 128 KiB windows, one
// buffer; 4 096-row tiles, fewer when the matrix is small).
int uspmv_dmat_optimize_block_sweep(uspmv_dmat_t *A, const uspmv_scs_t *s, int block_vec_size, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep) {
    if (!A || !s) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block_sweep: NULL argument");
    if (int rc = check_dmat_one_prec(A, "uspmv_dmat_optimize_block_sweep")) return rc;
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block_sweep: layout-only struct; the plan builder needs the host entries");
    if (A->C != s->C || A->n_chunks != s->n_chunks || A->dtype != s->dtype)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block_sweep: handle and host struct do not describe the same matrix");
    if (int rc = require_device()) return rc;
    A->bw = {};
    if (n_tiles) *n_tiles = 0;
    if (n_sweep) *n_sweep = 0;
    const size_t vsz = s->dtype == USPMV_F64 ? 8 : 4;
    if ((size_t)block_vec_size * vsz != 64) return USPMV_OK;                 // the kernel is written for 64-byte X rows
    // defaults: the largest window (2^11 rows = 128 KiB, one buffer) and 4 096-row tiles measured best on the Queen_4147-class matrix
    // (0.998 / 1.016 ms row- / column-wise; 2^9-row windows with two buffers 1.26 / 1.29: profiles/r04/spmmv_sweep_probe.txt)
    if (wlog <= 0) wlog = 11;
    if (((size_t)1 << wlog) * 64 > WG_LDS_BYTES) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block_sweep: a window of 2^%d rows does not fit the LDS", wlog);
    if (tile_rows <= 0) {
        tile_rows = 4096;
        while (tile_rows > 1024 && s->n_chunks * s->C / tile_rows < 384) tile_rows /= 2;   // (at least ~1.5 tiles per CU)
    }
    uspmv_block_sweep_plan p;
    const double max_stage = g_tune.sweep_max_stage > 0 ? (double)g_tune.sweep_max_stage : 24.0;
    if (int rc = uspmv_build_block_sweep_plan(s, wlog, tile_rows, 64, max_stage, &p)) return rc;
    if (n_tiles) *n_tiles = p.n_tiles;
    if (n_sweep) *n_sweep = p.valid ? p.n_sweep_tiles : 0;
    if (getenv("USPMV_VERBOSE"))
        fprintf(stderr, "[uspmv] block sweep plan: tile_rows=%d wlog=%d tiles=%lld sweep=%lld rest_chunks=%zu elements=%zu windows staged=%lld (%.2f X rows per matrix row) cnt_bytes=%zu\n",
                p.tile_rows, p.wlog, (long long)p.n_tiles, (long long)p.n_sweep_tiles, p.rest_chunks.size(), p.idx.size(), (long long)p.windows_staged,
                (double)p.windows_staged * (double)((int64_t)1 << p.wlog) / (double)std::max<int64_t>(s->n_chunks * s->C, 1), p.cnt.size());
    if (!p.valid || p.n_sweep_tiles != p.n_tiles || !p.rest_chunks.empty()) return USPMV_OK;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = A->bw.tile_ids.upload(p.tile_ids.data(), p.tile_ids.size() * 4);
    if (e == hipSuccess) e = A->bw.win_ptr.upload(p.t_win_ptr.data(), p.t_win_ptr.size() * 4);
    if (e == hipSuccess) e = A->bw.wins.upload(p.wins.data(), p.wins.size() * 4);
    if (e == hipSuccess) e = A->bw.cnt_off.upload(p.t_cnt_off.data(), p.t_cnt_off.size() * 8);
    if (e == hipSuccess) e = A->bw.wave_off.upload(p.wave_off.data(), p.wave_off.size() * 4);
    if (e == hipSuccess) e = A->bw.cnt.upload(p.cnt.data(), p.cnt.size());
    if (e == hipSuccess) e = A->bw.vals.upload(vsz == 8 ? (const void *)p.vals_f64.data() : (const void *)p.vals_f32.data(), p.idx.size() * vsz);
    if (e == hipSuccess) e = A->bw.idx.upload(p.idx.data(), p.idx.size() * 2);
    if (e == hipSuccess) e = A->bw.pad.upload(p.pad_col.data(), p.pad_col.size() * 4);
    if (e != hipSuccess) { A->bw = {}; (void)hipGetLastError(); return uspmv::fail(USPMV_ERR_ALLOC, "uspmv_dmat_optimize_block_sweep: %s", hipGetErrorString(e)); }
    A->bw.on = true; A->bw.tile_rows = p.tile_rows; A->bw.wlog = p.wlog; A->bw.b = block_vec_size;
    A->bw.n_tiles = p.n_sweep_tiles; A->bw.all_tiles = p.n_tiles; A->bw.x_rows = p.x_rows_min; A->bw.windows = p.windows_staged;
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

int uspmv_dmat_optimize_sweep_device(uspmv_dmat_t *A, uspmv_dmat_t *sp, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep) {
    if (int rc = check_dmat_one_prec(A, "uspmv_dmat_optimize_sweep_device")) return rc;
    if (sp) {
        if (int rc = check_dmat(sp, "uspmv_dmat_optimize_sweep_device")) return rc;
        if (A->dtype != USPMV_F64 || sp->dtype != USPMV_F32 || A->C != sp->C || A->n_chunks != sp->n_chunks)
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep_device: handles do not form a dp+sp pair");
    }
    if (int rc = require_device()) return rc;
    uspmv_dmat_t *const ms[2] = {A, sp};
    return sweep_plan_install_device(ms, sp ? 2 : 1, wlog, tile_rows, n_tiles, n_sweep, "uspmv_dmat_optimize_sweep_device");
}

// FNV-1a digest of a device array (tests: a plan built on the device must equal the host planner's)
static int device_fnv(const void *d, size_t bytes, uint64_t *out) {
    uint64_t h = 1469598103934665603ull;
    if (d && bytes) {
        std::vector<unsigned char> buf(bytes);
        HIP_TRY(hipMemcpy(buf.data(), d, bytes, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < bytes; ++k) { h ^= buf[k]; h *= 1099511628211ull; }
    }
    *out = h;
    return USPMV_OK;
}

// ... of one part's arrays of the sweep plan: wave offsets, counts, values, indices, padding columns
static int sweep_part_digest(const uspmv_dmat::SweepPlan &w, int part, uint64_t digest[5]) {
    const auto &pt = w.part[part];
    const size_t nsw = (size_t)w.n_tiles, wpt = (size_t)w.tile_rows / 64, nv = (size_t)pt.n_vals;
    int rc = device_fnv(pt.wave_off, nsw * wpt * 4, &digest[0]);
    if (!rc) rc = device_fnv(pt.cnt, (size_t)w.cnt_bytes, &digest[1]);
    if (!rc) rc = device_fnv(pt.vals, nv * uspmv_dtype_bytes(pt.dtype), &digest[2]);
    if (!rc) rc = device_fnv(pt.idx, nv * 2, &digest[3]);
    if (!rc) rc = device_fnv(pt.pad, nsw * (size_t)w.tile_rows * 4, &digest[4]);
    return rc;
}

// ... of the whole plan: digest[0..3] the tile arrays, [4..8] part 0, [9] the rest chunks, [10..14] part 1
int uspmv_dmat_sweep_plan_digest(const uspmv_dmat_t *A, uint64_t digest[16], int64_t meta[8]) {
    if (int rc = check_dmat(A, "uspmv_dmat_sweep_plan_digest")) return rc;
    if (!digest || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_sweep_plan_digest: NULL argument");
    for (int k = 0; k < 16; ++k) digest[k] = 0;
    const auto &w = A->sw;
    meta[0] = w.on; meta[1] = w.tile_rows; meta[2] = w.wlog; meta[3] = w.n_tiles; meta[4] = w.all_tiles; meta[5] = w.n_rest;
    meta[6] = w.part[0].n_vals; meta[7] = w.part[1].n_vals;
    if (!w.on || !w.tile_ids) return USPMV_OK;
    const size_t nsw = (size_t)w.n_tiles;
    int rc = device_fnv(w.tile_ids, nsw * 4, &digest[0]);
    if (!rc) rc = device_fnv(w.smin, nsw * 4, &digest[1]);
    if (!rc) rc = device_fnv(w.S, nsw * 4, &digest[2]);
    if (!rc) rc = device_fnv(w.cnt_off, nsw * 8, &digest[3]);
    if (!rc) rc = sweep_part_digest(w, 0, &digest[4]);
    if (!rc) rc = device_fnv(w.rest, (size_t)w.n_rest * 4, &digest[9]);
    if (!rc && w.n_parts >= 2) rc = sweep_part_digest(w, 1, &digest[10]);
    return rc;
}

int uspmv_dmat_sweep_plan_digest_part(const uspmv_dmat_t *A, int part, uint64_t digest[5], int64_t *n_vals) {
    if (int rc = check_dmat(A, "uspmv_dmat_sweep_plan_digest_part")) return rc;
    if (!digest || part < 0 || part > 2) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_sweep_plan_digest_part: bad argument");
    for (int k = 0; k < 5; ++k) digest[k] = 0;
    if (n_vals) *n_vals = 0;
    const auto &w = A->sw;
    if (!w.on || !w.tile_ids || part >= w.n_parts) return USPMV_OK;
    if (n_vals) *n_vals = w.part[part].n_vals;
    return sweep_part_digest(w, part, digest);
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

// FNV-1a digests of the phased block plan's device arrays (tests: device-built == host-planned)
int uspmv_dmat_block_plan_digest(const uspmv_dmat_t *A0, uint64_t digest[8]) {
    if (int rc = check_dmat(A0, "uspmv_dmat_block_plan_digest")) return rc;
    if (!digest) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_block_plan_digest: NULL argument");
    const uspmv_dmat_t *A = (A0->alt && g_tune.rechunk) ? A0->alt : A0;
    for (int k = 0; k < 8; ++k) digest[k] = 0;
    if (!A->pb.on) return USPMV_OK;
    const size_t nt = (size_t)A->pb.n_tiles, nph = (size_t)A->pb.n_phases, nc = (size_t)A->n_chunks, vsz = A->dtype == USPMV_F64 ? 8 : 4;
    int32_t n_list = 0;
    uint32_t tot16 = 0;
    HIP_TRY(hipMemcpy(&n_list, A->pb.list_ptr + nph, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&tot16, A->pb.c16_ptrs + nc, 4, hipMemcpyDeviceToHost));
    int rc = device_fnv(A->pb.ph_ptr, (nt + 1) * 4, &digest[0]);
    if (!rc) rc = device_fnv(A->pb.g0, nph * 4, &digest[1]);
    if (!rc) rc = device_fnv(A->pb.list_ptr, (nph + 1) * 4, &digest[2]);
    if (!rc) rc = device_fnv(A->pb.xrows, (size_t)n_list * 4, &digest[3]);
    if (!rc) rc = device_fnv(A->pb.c16_ptrs, (nc + 1) * 4, &digest[4]);
    if (!rc) rc = device_fnv(A->pb.col16, (size_t)tot16 * (A->pb.idx8 ? 1 : 2), &digest[5]);
    if (!rc) rc = device_fnv(A->pb.values, (size_t)tot16 * vsz, &digest[6]);
    if (!rc) rc = device_fnv(A->bt.row_map, A->bt.row_map ? nc * (size_t)A->C * 4 : 0, &digest[7]);
    return rc;
}

int uspmv_dmat_block_plan_staged(const uspmv_dmat_t *A, int64_t *rows_staged) {
    if (!A || !rows_staged) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_block_plan_staged: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    *rows_staged = M->pb.on ? M->pb.rows_staged : 0;
    return USPMV_OK;
}

int uspmv_dmat_block_plan_info(const uspmv_dmat_t *A, int64_t meta[10]) {
    if (!A || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_block_plan_info: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    meta[0] = M->bt.on; meta[1] = M->pb.on; meta[2] = M->pl.on; meta[3] = M->pb.n_tiles; meta[4] = M->pb.n_phases; meta[5] = M->pl.n_phases;
    meta[6] = M->pl.rows_staged; meta[7] = M->pb.idx8; meta[8] = M->pb.device_built; meta[9] = M->pb.max_rows;
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

int uspmv_dmat_stream_info(const uspmv_dmat_t *A, int64_t meta[2]) {
    if (!A || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_stream_info: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    meta[0] = M->ps.desc ? M->ps.grid : 0; meta[1] = M->ps.desc ? M->ps.n_desc : 0;
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
// (uspmv_raw_plan_cache_clear() after freeing or rewriting them).  Mutex-guarded; a handful of entries.
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

int uspmv_stream_copy(double *a, const double *b, int64_t n, void *stream) {
    if (!a || !b || n < 0 || (n & 1)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_stream_copy: bad argument (n must be even)");
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(stream_copy_kernel, dim3((unsigned)((n / 2 + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream, (double2 *)a, (const double2 *)b, (long)(n / 2));
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int uspmv_stream_triad(double *a, const double *b, const double *c, double s, int64_t n, void *stream) {
    if (!a || !b || !c || n < 0 || (n & 1)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_stream_triad: bad argument (n must be even)");
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(stream_triad_kernel, dim3((unsigned)((n / 2 + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, (double2 *)a, (const double2 *)b, (const double2 *)c, s, (long)(n / 2));
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int uspmv_stream_read(const double *b, int64_t n, double *partial, void *stream) {
    if (!b || !partial || n < 0 || (n & 1)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_stream_read: bad argument (n must be even; partial needs 8192 doubles)");
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(stream_read_kernel, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, (const double2 *)b, (long)(n / 2), partial);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int uspmv_stream_gather_lines(const double *x, int64_t n, int64_t plane, int64_t line, int rows, double *partial, void *stream, int64_t *bytes) {
    if (!x || !partial || n < 4096 || rows < 16 || rows > 4096 || plane < 0 || line < 0)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_stream_gather_lines: bad argument (partial needs 4 * ceil(n / rows) doubles)");
    if (int rc = require_device()) return rc;
    const long tiles = (long)((n + rows - 1) / rows);
    hipLaunchKernelGGL(stream_gather_lines_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const double2 *)x, (long)n, (long)plane, (long)line, rows,
                       g_tune.xcd_remap, partial);
    HIP_TRY(hipGetLastError());
    if (bytes) *bytes = tiles * 9 * (int64_t)(((rows + 2 + 15) / 16 + 1) * 128);   // (nine runs of whole lines per tile; the ends of the vector ask for a little less)
    return USPMV_OK;
}

int uspmv_time_launches(int what, int reps, const uspmv_dmat_t *A, const uspmv_dmat_t *B, const void *d_x, void *d_y,
                        int64_t n, int b, int64_t ld, int layout, void *stream, double *avg_ms) {
    if (reps < 1 || !avg_ms) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_time_launches: bad argument");
    if (int rc = require_device()) return rc;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    hipStream_t st = (hipStream_t)stream;
    int rc = USPMV_OK;
    for (int r = -2; r < reps && rc == USPMV_OK; ++r) {      // two untimed launches first (page tables, caches, clocks)
        if (r == 0) HIP_TRY(hipEventRecord(e0, st));
        switch (what) {
            case 0: rc = uspmv_spmv(A, d_x, d_y, stream); break;
            case 1: rc = uspmv_stream_copy((double *)d_y, (const double *)d_x, n, stream); break;
            case 2: rc = uspmv_stream_triad((double *)d_y, (const double *)d_x, (const double *)d_x + n, 3.0, n, stream); break;
            case 3: rc = uspmv_stream_read((const double *)d_x, n, (double *)d_y, stream); break;
            case 4: rc = uspmv_spmv_ap(A, B, (const double *)d_x, (double *)d_y, stream); break;
            case 5: rc = uspmv_spmmv(A, d_x, d_y, b, ld, layout, stream); break;
            case 6: rc = uspmv_stream_gather_lines((const double *)d_x, n, ld, (int64_t)b, layout, (double *)d_y, stream, nullptr); break;
            case 7: rc = uspmv_spmmv_ap(A, B, d_x, d_y, b, ld, layout, stream); break;
            default: rc = uspmv::fail(USPMV_ERR_INVALID, "uspmv_time_launches: unknown kind %d", what);
        }
    }
    hipError_t e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc != USPMV_OK) return rc;
    if (e != hipSuccess) return uspmv::fail(USPMV_ERR_HIP, "uspmv_time_launches: %s", hipGetErrorString(e));
    *avg_ms = (double)ms / reps;
    return USPMV_OK;
}

}  // extern "C"
