/*
 * uspmv.h -- C ABI of the MI355X-native SELL-C-sigma SpMV / SpMMV engine (libuspmv.so).
 *
 * Drop-in boundary for the scs/crs kernel path of RRZE-HPC/Ultimate-SpMV.  The reference has no
 * FFI; its seam is the C++ function-pointer type SpmvKernel::OnePrecFuncPtr / MultiPrecFuncPtr
 * (code/classes_structs.hpp:283-333) and the free functions of code/interface.hpp.  Every entry
 * point below names the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers and sizes only; indices are 32-bit (`IT = int`, code/main.cpp:1711-1718),
 *     sizes 64-bit (`ST = long`, code/classes_structs.hpp:31);
 *   - every function returns a uspmv_status (0 = success) and NEVER calls exit(); the text of
 *     the last failure of the calling thread is available from uspmv_last_error();
 *   - pointers prefixed d_ are device (HBM) pointers of the current HIP device; all others are
 *     host pointers;  `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - device entry points are asynchronous with respect to the host (the reference's launchers
 *     call cudaDeviceSynchronize, code/classes_structs.hpp:1032-1034; callers that need that
 *     behaviour call uspmv_stream_synchronize);
 *   - there is NO CPU fallback: device entry points fail with USPMV_ERR_NO_DEVICE / USPMV_ERR_HIP
 *     when no gfx950 device is usable.
 */
#ifndef USPMV_H
#define USPMV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    USPMV_OK = 0,
    USPMV_ERR_INVALID = 1,     /* bad argument (NULL, negative size, unknown enum ...)        */
    USPMV_ERR_IO = 2,          /* file cannot be opened / parsed                               */
    USPMV_ERR_UNSUPPORTED = 3, /* valid request the engine does not implement                  */
    USPMV_ERR_OVERFLOW = 4,    /* a 32-bit index would overflow (code/utilities.hpp:1959-1962) */
    USPMV_ERR_NO_DEVICE = 5,   /* no HIP device visible                                        */
    USPMV_ERR_HIP = 6,         /* a HIP runtime call failed                                    */
    USPMV_ERR_ALLOC = 7,
    USPMV_ERR_COMM = 8         /* a peer rank failed, never arrived or disagrees (host communicator / transport) */
} uspmv_status;

typedef enum { USPMV_F64 = 0, USPMV_F32 = 1, USPMV_F16 = 2 } uspmv_dtype;   /* -dp / -sp / hp part      */
/* USPMV_F16: IEEE binary16 values (uint16_t bits), the hp part of an adaptive-precision split (uspmv_partition_precisions_hp).
 * Accepted by uspmv_convert_to_scs, uspmv_convert_to_scs_device_from_arrays, uspmv_dmat_upload and uspmv_dmat_wrap; a one-precision SpMV / SpMMV or plan of an F16 handle
 * returns USPMV_ERR_UNSUPPORTED (the reference's -hp accumulates in _Float16); such a handle only runs inside uspmv_spmv_ap_hp. */
typedef enum { USPMV_COLWISE = 0, USPMV_ROWWISE = 1 } uspmv_layout;   /* Makefile:26-31         */
typedef enum { USPMV_SEG_ROWS = 0, USPMV_SEG_NNZ = 1 } uspmv_seg;     /* -seg_rows / -seg_nnz   */

typedef struct uspmv_coo uspmv_coo_t;     /* host COO,           MtxData  code/classes_structs.hpp:1169-1238 */
typedef struct uspmv_scs uspmv_scs_t;     /* host SELL-C-sigma,  ScsData  code/classes_structs.hpp:1313-1339 */
typedef struct uspmv_dmat uspmv_dmat_t;   /* device-resident SCS (what assign_spmv_kernel_gpu_data
                                             uploads, code/utilities.hpp:3721-3811)                         */
typedef struct uspmv_halo uspmv_halo_t;   /* per-rank halo description (ContextData,
                                             code/classes_structs.hpp:156-184)                             */

const char *uspmv_status_string(int status);
const char *uspmv_last_error(void);
const char *uspmv_version(void);
/* debugging aid: SIGSEGV / SIGBUS / SIGABRT print the native call stack (module+offset) to stderr before the default action */
int uspmv_debug_backtrace_on_crash(int on);

/* ------------------------------------------------------------------ L1: COO / MatrixMarket */
/* read_mtx (code/utilities.hpp:2148-2309) + mm_read_unsymmetric_sparse (code/mmio.h:132-263):
 * real / integer / pattern (= 0.01) coordinate files, general or symmetric (expanded), entries
 * stable-sorted by row. */
int uspmv_read_mtx(const char *path, uspmv_coo_t **out);
/* Binary cache of a COO handle (no reference counterpart): what uspmv_read_mtx returned --
 * expanded, row-sorted -- written / read back verbatim, so that later runs skip the text parse. */
int uspmv_coo_save(const uspmv_coo_t *m, const char *path);
int uspmv_coo_load(const char *path, uspmv_coo_t **out);
/* MatrixMarket writer (the reference only reads; used to produce inputs): coordinate real general, or -- symmetric != 0 -- the entries
 * with column <= row under a "symmetric" banner, which uspmv_read_mtx / read_mtx expand again.  17 significant digits. */
int uspmv_coo_write_mtx(const uspmv_coo_t *m, const char *path, int symmetric);
/* -equilibrate 1 of a one-precision run: equilibrate_matrix (code/utilities.hpp:2667-2685), in place.  (With
 * ap[dp_sp] the reference indexes two empty vectors here, code/main.cpp:1143-1153 -- undefined behaviour, not offered.) */
int uspmv_coo_equilibrate(uspmv_coo_t *m);
/* The same, in place and bit for bit, handing out the two divisor vectors that the equilibrated branch of partition_precisions takes
 * (largest_row_elems, largest_col_elems; code/main.cpp:1147-1153 calls extract_largest_row_elems, scale_matrix_rows,
 * extract_largest_col_elems, scale_matrix_cols of code/utilities.hpp:2605-2665 in this order): row_max[n_rows] = largest magnitude of
 * every row, col_max[n_cols] = largest magnitude of every column of the ROW-SCALED matrix; 0 for an empty row or column.  (The
 * reference's CLI indexes two empty vectors there; its library function is sound for vectors sized like these.)
 * USPMV_ERR_INVALID, before any value is written: a non-finite value, or an entry whose row or column divisor is 0 (a row or column of
 * explicit zeros only, or scaled values that underflowed to 0) -- 0 / 0 is a NaN whose sign differs between x86 and the GPU. */
int uspmv_coo_equilibrate_scales(uspmv_coo_t *m, double *row_max, double *col_max);
/* MtxData filled by a host application (API_doc.md:7-9).  Arrays are copied. */
int uspmv_coo_create(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *I, const int32_t *J,
                     const double *values, uspmv_coo_t **out);
int uspmv_coo_dims(const uspmv_coo_t *m, int64_t *n_rows, int64_t *n_cols, int64_t *nnz);
/* borrowed pointers, valid until uspmv_coo_free */
int uspmv_coo_arrays(const uspmv_coo_t *m, const int32_t **I, const int32_t **J, const double **values);
void uspmv_coo_free(uspmv_coo_t *m);

/* Deterministic synthetic matrices for the BASELINE configurations whose SuiteSparse files are
 * not available offline: 27-point stencil with `dof` unknowns per grid node on
 * an nx*ny*nz grid, rows [row_begin,row_end) only (so that every rank of a distributed run
 * generates just its block; column indices stay global).  Symmetric pattern and values
 * v(i,j) = hash(min,max,seed) in [-1,1), diagonal 27*dof + u.  magnitude_decades > 0 spreads the
 * off-diagonal magnitudes log-uniformly over that many decades (HV15R-class, for -ap splits). */
int uspmv_gen_stencil27(int64_t nx, int64_t ny, int64_t nz, int dof, uint64_t seed, double magnitude_decades,
                        int64_t row_begin, int64_t row_end, uspmv_coo_t **out);
/* entries per row of that matrix for rows [row_begin,row_end) -- with uspmv_seg_from_row_counts the ranks of a distributed
 * run agree on the partition without anybody generating the whole matrix */
int uspmv_gen_stencil27_row_counts(int64_t nx, int64_t ny, int64_t nz, int dof, int64_t row_begin, int64_t row_end, int32_t *out);
/* Banded-random matrix of SURVEY.md 8(d) (HV15R-class: n = 2 017 169, 140 entries per row, band +-50 000, magnitudes
 * over 10 decades): the diagonal plus nnz_per_row - 1 hashed distinct columns in [i - band, i + band], general
 * pattern, columns ascending inside a row; the irregular counterpart of the stencil generator. */
int uspmv_gen_banded_random(int64_t n, int nnz_per_row, int64_t band, uint64_t seed, double magnitude_decades,
                            int64_t row_begin, int64_t row_end, uspmv_coo_t **out);
/* KKT-structured matrix of the nlpkkt class ([H A^T; A 0], PDE-constrained optimisation on an N^3 grid with boundary control;
 * n = 2 N^3 + 6 N^2 as in SuiteSparse nlpkkt200 / nlpkkt240): unknowns = states, multipliers, boundary controls; interior state
 * rows 28 entries, multiplier rows 25, control rows 5-7; a row's columns live in two index ranges N^3 apart.  Symmetric pattern
 * and values, columns ascending inside a row; rows [row_begin, row_end) with local row ids and global column ids. */
int uspmv_gen_kkt(int64_t N, uint64_t seed, int64_t row_begin, int64_t row_end, uspmv_coo_t **out);
int uspmv_gen_kkt_row_counts(int64_t N, int64_t row_begin, int64_t row_end, int32_t *out);

/* ------------------------------------------------------------------ L2: format conversion */
/* convert_to_scs (code/utilities.hpp:1842-2104; library twin code/interface.hpp:401-656).
 * fixed_permutation may be NULL (sigma-window sort by descending row length, std::sort tie order
 * reproduced) or an old->new row map of n_rows entries (:1911-1928).  dtype selects VT. */
int uspmv_convert_to_scs(const uspmv_coo_t *m, int64_t C, int64_t sigma, int dtype,
                         const int32_t *fixed_permutation, uspmv_scs_t **out);
/* meta[8] = C, sigma, n_rows, n_cols, n_rows_padded, n_chunks, n_elements, nnz */
int uspmv_scs_meta(const uspmv_scs_t *s, int64_t meta[8]);
int uspmv_scs_dtype(const uspmv_scs_t *s, int *dtype);
/* borrowed pointers (chunk_ptrs[n_chunks+1], chunk_lengths[n_chunks], col_idxs/values[n_elements],
 * old_to_new_idx/new_to_old_idx[n_rows]); any argument may be NULL */
int uspmv_scs_arrays(const uspmv_scs_t *s, const int32_t **chunk_ptrs, const int32_t **chunk_lengths,
                     const int32_t **col_idxs, const void **values, const int32_t **old_to_new_idx,
                     const int32_t **new_to_old_idx);
/* mutable view of col_idxs (halo set-up rewrites it in place like the reference does) */
int uspmv_scs_col_idxs_mut(uspmv_scs_t *s, int32_t **col_idxs);
/* permute_scs_cols (code/utilities.hpp:1802-1831): col = perm[col] where col < n_rows */
int uspmv_permute_scs_cols(uspmv_scs_t *s, const int32_t *perm);
void uspmv_scs_free(uspmv_scs_t *s);
/* apply_permutation (code/utilities.hpp:1768-1782): out[i] = in[perm[i]], host vectors */
int uspmv_apply_permutation(void *out, const void *in, const int32_t *perm, int64_t n, int dtype);
/* partition_precisions, ap[dp_sp] non-equilibrated branch (code/utilities.hpp:2899-2911):
 * |v| >= threshold_1 -> dp, else sp (values rounded to float), COO order kept. */
int uspmv_partition_precisions(const uspmv_coo_t *m, double threshold_1, uspmv_coo_t **dp, uspmv_coo_t **sp);
/* partition_precisions with an fp16 part, ap[dp_hp] / ap[sp_hp] / ap[dp_sp_hp] (code/interface.hpp:691-987, non-equilibrated branch), COO
 * order kept, every part's values stored as doubles holding the rounded value:
 *   USPMV_AP_DP_HP     |v| >= t1 -> hi (double), |v| < t1 -> hp;                      NaN: USPMV_ERR_INVALID
 *   USPMV_AP_SP_HP     |v| >= t1 -> hi ((float)v), |v| < t1 -> hp;                    NaN: USPMV_ERR_INVALID
 *   USPMV_AP_DP_SP_HP  |v| >= t1 -> hi (double), else t2 <= |v| <= t1 -> mid ((float)v), else -> hp (NaN included)
 * hp values are rounded once to binary16, to nearest even (subnormals kept, overflow to +-inf, bit-equal to numpy's float64 -> float16).
 * *mid is set to NULL for the two-part kinds (mid may then be NULL). */
enum { USPMV_AP_DP_HP = 0, USPMV_AP_SP_HP = 1, USPMV_AP_DP_SP_HP = 2, USPMV_AP_DP_SP = 3 };   /* (DP_SP: the device-side set-up below only) */
int uspmv_partition_precisions_hp(const uspmv_coo_t *m, int kind, double threshold_1, double threshold_2, uspmv_coo_t **hi,
                                  uspmv_coo_t **mid, uspmv_coo_t **hp);
/* partition_precisions, the EQUILIBRATED branch of all four kinds (config->equilibrate: code/utilities.hpp:2883-2896 ap[dp_sp],
 * :2934-2950 ap[dp_hp], :2989-3007 ap[sp_hp], :3046-3078 ap[dp_sp_hp]; library twin code/interface.hpp:691-987).  m is the matrix
 * uspmv_coo_equilibrate_scales scaled, row_max / col_max its vectors.  Entry k = (I, J, v) has its own thresholds
 * T1 = threshold_1 / (col_max[J] * row_max[I]) and T2 likewise (one multiplication, one division):
 *   two-part kinds     |v| >= T1 -> hi, else -> lo (a plain else: a NaN goes to lo, where the non-equilibrated branch refuses it)
 *   USPMV_AP_DP_SP_HP  |v| >= T1 -> hi, else T2 <= |v| <= T1 -> mid, else -> lo
 * Stored values as in uspmv_partition_precisions[_hp]: (double)(float)v for an sp part, one rounding to binary16 for an hp part.
 * parts[0] = hi, parts[1] = mid (NULL for the two-part kinds), parts[2] = lo, as uspmv_partition_precisions_device; COO order kept. */
int uspmv_partition_precisions_eq(const uspmv_coo_t *m, int kind, double threshold_1, double threshold_2, const double *row_max,
                                  const double *col_max, uspmv_coo_t *parts[3]);

/* ------------------------------------------------------------------ L3: device kernels    */
int uspmv_device_count(int *count);
int uspmv_set_device(int device);
int uspmv_stream_synchronize(void *stream);

/* H2D staging of one SCS struct (assign_spmv_kernel_gpu_data, code/utilities.hpp:3721-3811). */
int uspmv_dmat_upload(const uspmv_scs_t *s, uspmv_dmat_t **out);
/* GPU-side conversion: the result of uspmv_convert_to_scs [+ uspmv_permute_scs_cols with the
 * struct's own old_to_new_idx when permute_cols != 0] + uspmv_dmat_upload, bit for bit, but only the
 * O(n_rows) layout (row lengths, sigma-window std::sort, chunk lengths / pointers, permutations) is
 * computed on the host; the O(nnz) scatter of code/utilities.hpp:2013-2036 runs on the device straight
 * from the uploaded COO arrays.  *layout is a host struct WITHOUT entries: meta data, chunk arrays and
 * the permutations are there, uspmv_scs_arrays returns NULL for col_idxs / values, and the functions that
 * need host entries (uspmv_dmat_upload / _optimize*, uspmv_halo_discover, ...) refuse it.  The COO entries
 * must be sorted by row (uspmv_read_mtx and the generators produce that order). */
int uspmv_convert_to_scs_device(const uspmv_coo_t *m, int64_t C, int64_t sigma, int dtype, const int32_t *fixed_permutation,
                                int permute_cols, uspmv_scs_t **layout, uspmv_dmat_t **out);
/* The same from DEVICE-resident COO arrays (d_I, d_J: int32, d_V: double; entries sorted by row, order inside a row = summation order):
 * nothing but O(n_rows) integers ever leaves the device.  Row populations by a run-boundary kernel (code/utilities.hpp:1901-1903), chunk
 * lengths by a per-chunk maximum and chunk_ptrs by a device scan (:1949-1966), the scatter as above (:2013-2036).  The sigma-window
 * ordering (:1930-1941) in one of two ways:
 *   USPMV_SORT_HOST          the reference's std::sort (same pair type, same comparator) on the host over the row COUNTS only -- 4 bytes
 *                            per row down, 4 up; every array bit-identical to uspmv_convert_to_scs incl. the tie order of the unstable sort;
 *   USPMV_SORT_DEVICE_STABLE a stable rank per window on the device (sigma <= 8192): rows of equal length keep their original order.
 *                            chunk_lengths, chunk_ptrs and y in ORIGINAL row order are bit-identical to the reference's; the order of
 *                            equal-length rows inside a window, hence old_to_new_idx and the row order of y_permuted, differs.
 * d_fixed_permutation (device, n_rows entries, may be NULL) as fixed_permutation above.  d_old_to_new / d_new_to_old (device, n_rows
 * int32 each, may be NULL) receive the struct's permutations for uspmv_apply_permutation_dev; *layout (may be NULL) a host struct
 * without entries as above.  Works on `stream`; returns when the handle is complete.  dtype USPMV_F16: the values are rounded once from
 * the double to binary16, as uspmv_convert_to_scs stores them. */
/* diagnosis: device addresses of {tile-local-column indices, x-line lists, line pointers, index offsets, values, col_idxs, chunk_ptrs,
 * chunk_lengths} of the struct the SpMV kernels read (tools/placement_probe.py) */
int uspmv_dmat_plan_addresses(const uspmv_dmat_t *m, uint64_t addr[8]);
/* meta[4] = C, n_chunks, n_elements, dtype of a device handle (one without a host struct has nothing else to ask) */
int uspmv_dmat_meta(const uspmv_dmat_t *m, int64_t meta[4]);
enum { USPMV_SORT_HOST = 0, USPMV_SORT_DEVICE_STABLE = 1 };
int uspmv_convert_to_scs_device_from_arrays(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                            int64_t C, int64_t sigma, int dtype, const int32_t *d_fixed_permutation, int permute_cols,
                                            int sort_mode, void *stream, uspmv_scs_t **layout, int32_t *d_old_to_new, int32_t *d_new_to_old,
                                            uspmv_dmat_t **out);
/* Adaptive-precision set-up from DEVICE-resident COO arrays: uspmv_partition_precisions[_hp] on the device.  d_I, d_J
 * (int32) and d_V (double) as above: sorted by row, order inside a row = summation order, which every part keeps.  kind: USPMV_AP_DP_SP
 * (|v| >= t1 -> dp, |v| < t1 -> sp stored as (double)(float)v, NaN refused) or one of the kinds of uspmv_partition_precisions_hp, classified
 * in the host functions' branch order; hp values are rounded once from the double (host/uspmv_f16_round.hpp).  Every part equals the host
 * function's bit for bit.  parts[0] = hi, parts[1] = mid (NULL for the two-part kinds), parts[2] = lo; a part may be empty.
 * Three passes, none waiting on another workgroup: classify and count per workgroup of 1024 entries, scan the counts, classify again and
 * scatter.  The first pass also checks 0 <= I < n_rows, 0 <= J < n_cols and the row order: USPMV_ERR_INVALID / _UNSUPPORTED, and a NaN in
 * a two-part kind "element %lld fits neither struct" (the first such element), all before anything is written.
 * Device memory beyond the returned parts (16 bytes per entry in all): 3 * (nnz / 1024) * 20 bytes of counts and bases. */
typedef struct uspmv_dcoo uspmv_dcoo_t;   /* one compacted part in HBM */
int uspmv_partition_precisions_device(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                      int kind, double threshold_1, double threshold_2, void *stream, uspmv_dcoo_t *parts[3]);
/* borrowed device pointers, valid until uspmv_dcoo_free (any argument may be NULL) */
int uspmv_dcoo_arrays(const uspmv_dcoo_t *p, const int32_t **d_I, const int32_t **d_J, const double **d_V, int64_t *nnz);
/* the part copied into the caller's device arrays of nnz elements each (a framework's own allocations; any of them may be NULL) */
int uspmv_dcoo_copy(const uspmv_dcoo_t *p, int32_t *d_I, int32_t *d_J, double *d_V, void *stream);
void uspmv_dcoo_free(uspmv_dcoo_t *p);
/* uspmv_gen_stencil27 on the device (csrc/gen_kernels.hip): rows [row_begin,row_end) as COO arrays in HBM -- row ids local,
 * column ids global, sorted by row, columns ascending inside a row: what uspmv_dist_create_from_arrays takes (uspmv_dcoo_arrays / _copy /
 * _free handle the result).  I, J and V equal uspmv_gen_stencil27's in every bit.  magnitude_decades > 0 is refused with
 * USPMV_ERR_UNSUPPORTED (the host's pow is not the device's; a generated matrix must not depend on where it was generated).  The host
 * function's other refusals, before any HIP call: bad argument, bad row range (USPMV_ERR_INVALID), more than INT32_MAX rows
 * (USPMV_ERR_OVERFLOW); more than INT32_MAX local entries: USPMV_ERR_OVERFLOW once they are counted, nothing returned.  Works on `stream`,
 * returns when the arrays are written. */
int uspmv_gen_stencil27_device(int64_t nx, int64_t ny, int64_t nz, int dof, uint64_t seed, double magnitude_decades, int64_t row_begin,
                               int64_t row_end, void *stream, uspmv_dcoo_t **out);
/* The whole set-up in one call: the partition above, the first part (hi: F64, F32 for ap[sp_hp]) converted with its own sigma ordering
 * (sort_mode as in uspmv_convert_to_scs_device_from_arrays), the other parts (mid: F32; lo: F32 for ap[dp_sp], else F16) with the first
 * part's permutation as their fixed permutation, and the columns of ALL parts permuted by the first part's old_to_new -- the handles the
 * host route (partition, uspmv_convert_to_scs with fixed_permutation, uspmv_permute_scs_cols, upload) gives, array for array.  They go
 * straight into uspmv_dmat_optimize_device_ap / _device_ap_hp / _sweep_device* and uspmv_spmv_ap[_hp] / uspmv_spmmv_ap[_hp].
 * layout, d_old_to_new, d_new_to_old (any may be NULL) describe the first part; part_nnz[3] (may be NULL) = entries of hi, mid, lo;
 * mid may be NULL for the two-part kinds (*mid is set to NULL otherwise).  A row without an entry in the first part that its ordering
 * sends behind n_rows while another part has entries in it is refused as uspmv_convert_to_scs refuses it.  On failure nothing is returned.
 * Device memory beyond the returned handles: the compacted copy of the parts (16 bytes per entry, each part released as soon as it is
 * converted) + 60 bytes per 1024 entries + about 24 bytes per padded row of conversion scratch. */
int uspmv_convert_to_scs_device_ap_from_arrays(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                               int64_t nnz, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2,
                                               int sort_mode, void *stream, uspmv_scs_t **layout, int32_t *d_old_to_new, int32_t *d_new_to_old,
                                               int64_t part_nnz[3], uspmv_dmat_t **hi, uspmv_dmat_t **mid, uspmv_dmat_t **lo);
/* uspmv_coo_equilibrate_scales on the device (csrc/equilibrate_kernels.hip): device COO sorted by row as above; the
 * scaled values go to d_V_out (nnz doubles; may be d_V), the divisors to d_row_max[n_rows] and d_col_max[n_cols].  Values and vectors
 * equal the host function's bit for bit (max is order-independent, IEEE division exact).  Three passes: row maxima by a segmented
 * maximum per wave (an atomic only for a row's run that crosses a wave), column maxima of the row-scaled values by a 64-bit integer
 * atomic maximum on the bit pattern, issued only where a plain load shows a smaller value, then the scaling.  The host function's
 * refusals (USPMV_ERR_INVALID: non-finite value, zero divisor) and the index / row-order checks of uspmv_partition_precisions_device
 * are raised through a flag BEFORE d_V_out is written; the two vectors are overwritten either way.  Works on `stream`, returns when
 * d_V_out is written.  No device memory beyond a flag word. */
int uspmv_equilibrate_device(const int32_t *d_I, const int32_t *d_J, const double *d_V, double *d_V_out, int64_t n_rows, int64_t n_cols,
                             int64_t nnz, double *d_row_max, double *d_col_max, void *stream);
/* diagnosis (tools/ap_equilibrate_probe.py): the column pass alone, with the vectors as uspmv_equilibrate_device left d_row_max and a
 * zeroed d_col_max, counting the atomics it issues after the skip */
int uspmv_equilibrate_device_count_atomics(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                           int64_t nnz, const double *d_row_max, double *d_col_max, void *stream, int64_t *n_atomics);
/* uspmv_partition_precisions_eq on the device: uspmv_partition_precisions_device with the per-entry thresholds
 * t / (d_col_max[J] * d_row_max[I]) (device vectors of n_rows / n_cols doubles, as uspmv_equilibrate_device wrote them; d_V the scaled
 * values).  Every part equals the host function's bit for bit; no element is refused as fitting no part. */
int uspmv_partition_precisions_device_eq(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                         int kind, double threshold_1, double threshold_2, const double *d_row_max, const double *d_col_max,
                                         void *stream, uspmv_dcoo_t *parts[3]);
/* uspmv_convert_to_scs_device_ap_from_arrays of an equilibrated matrix: the same set-up with the partition above (both vectors NULL:
 * the unscaled function).  The handles, the layout and the permutations are those of the host route uspmv_coo_equilibrate_scales ->
 * uspmv_partition_precisions_eq -> uspmv_convert_to_scs with the first part's permutation -> uspmv_permute_scs_cols -> upload. */
int uspmv_convert_to_scs_device_ap_from_arrays_eq(const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t n_cols,
                                                  int64_t nnz, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2,
                                                  const double *d_row_max, const double *d_col_max, int sort_mode, void *stream,
                                                  uspmv_scs_t **layout, int32_t *d_old_to_new, int32_t *d_new_to_old, int64_t part_nnz[3],
                                                  uspmv_dmat_t **hi, uspmv_dmat_t **mid, uspmv_dmat_t **lo);
/* copies of the device arrays of a handle (any pointer may be NULL): n_chunks+1, n_chunks, n_elements, n_elements */
int uspmv_dmat_download(const uspmv_dmat_t *m, int32_t *chunk_ptrs, int32_t *chunk_lengths, int32_t *col_idxs, void *values);
/* Wrap arrays that already live in HBM (owned by the caller, e.g. a framework allocator). */
int uspmv_dmat_wrap(int64_t C, int64_t n_chunks, int64_t n_elements, int dtype, const int32_t *d_chunk_ptrs,
                    const int32_t *d_chunk_lengths, const int32_t *d_col_idxs, const void *d_values,
                    uspmv_dmat_t **out);
void uspmv_dmat_free(uspmv_dmat_t *m);
/* Numeric refresh (no reference counterpart): the matrix changed numerically, not structurally -- Newton steps, time
 * stepping, re-assembled blocks -- and the handle keeps its plans.  *actions (may be NULL) receives what the call had to do beyond the
 * value array itself:
 *   USPMV_REFRESH_COPIES               private copies of the values re-gathered under their plan's row map (the element plan on rows dealt
 *                                      to the tiles; the block plans' re-ordered and group-major copies)
 *   USPMV_REFRESH_RECHUNKED            the internal C = 32 re-chunking of a narrow struct (C in {1, 2, 4, 8, 16}, crs included) re-copied
 *   USPMV_REFRESH_SWEEP_REBUILT        the column-window sweep plan of a one-struct handle rebuilt by the device builder at the installed
 *                                      window and rows per tile (its stream strips trailing +0 runs: its SHAPE depends on the values)
 *   USPMV_REFRESH_BLOCK_SWEEP_DROPPED  the block-vector sweep plan released (host-built only, same stripping rule); uspmv_spmmv then
 *                                      answers from whatever block plan remains, or from the gather kernel
 * 0: line, element, 12-bit and additive-record plans on the caller's row order, and a handle without a plan -- their kernels read the
 * value array in place.  All three calls refuse, before a device is looked for, with USPMV_ERR_UNSUPPORTED: an F16 handle, and a handle
 * that carries the shared plan of an adaptive-precision split (new values move entries between the parts: set the split up again with
 * uspmv_convert_to_scs_device_ap_from_arrays); with USPMV_ERR_INVALID: NULL arguments.  They work on `stream` and return when the handle
 * is consistent; uspmv_spmmv_x_prepared state is untouched; not thread-safe per handle, like every other call on a handle. */
enum { USPMV_REFRESH_COPIES = 1, USPMV_REFRESH_RECHUNKED = 2, USPMV_REFRESH_SWEEP_REBUILT = 4, USPMV_REFRESH_BLOCK_SWEEP_DROPPED = 8 };
/* The handle's values array has new contents (same pattern): bring every plan on the handle back in line with it. */
int uspmv_dmat_values_changed(uspmv_dmat_t *m, void *stream, int *actions);
/* New values in the handle's own layout and dtype (n_elements; host or device pointer), for handles that OWN their arrays
 * (uspmv_dmat_upload, the device conversions): copy, then uspmv_dmat_values_changed.  A wrapped handle is refused with
 * USPMV_ERR_INVALID: its caller writes the array and calls uspmv_dmat_values_changed. */
int uspmv_dmat_update_values(uspmv_dmat_t *m, const void *values, void *stream, int *actions);
/* New values as COO arrays in HBM, in the order the handle was converted from: d_I, d_J (int32), d_V (double) sorted by row, the order
 * inside a row = summation order, as at conversion (d_J is read only when check_pattern is set).  d_row_pos[n_rows]: the position of row i
 * in the struct -- the struct's old_to_new, or the fixed permutation it was converted with; NULL = the identity.  d_col_perm: what the
 * columns were permuted with (permute_scs_cols' rule: only columns below n_rows), NULL = as converted; read only when check_pattern is
 * set.  d_values_dst: NULL = the handle's own array (handles that own their arrays only); for a wrapped handle the WRITABLE pointer to
 * the array that was wrapped, which must equal the handle's values -- how the caller grants the write uspmv_dmat_wrap's const withheld.
 * Checks first, through flag words, nothing written before they come back clean: rows in [0, n_rows) (USPMV_ERR_INVALID) and sorted
 * (USPMV_ERR_UNSUPPORTED), with the texts of uspmv_convert_to_scs_device_from_arrays; ceil(n_rows / C) = n_chunks; every d_row_pos entry
 * inside the padded rows and no two alike; no row longer than the chunk where it sits; with check_pattern the stored column of every entry
 * equal to the (permuted) d_J -- USPMV_ERR_INVALID, the text names the first offending entry.  Placement: element (row, slot j) receives
 * the row's j-th value rounded as at conversion ((float)v for F32); slots beyond a row's entries receive +0 and keep their stored column,
 * like padding.  Then uspmv_dmat_values_changed.  Device memory beyond the handle: 4 bytes per row + 4 per padded row. */
int uspmv_dmat_update_values_from_arrays(uspmv_dmat_t *m, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t n_rows, int64_t nnz,
                                         const int32_t *d_row_pos, const int32_t *d_col_perm, int check_pattern, void *d_values_dst, void *stream,
                                         int *actions);
/* host twin on a host struct (it carries n_rows and its own old_to_new_idx): same placement, same checks, no device */
int uspmv_scs_update_values(uspmv_scs_t *s, const uspmv_coo_t *m, const int32_t *col_perm, int check_pattern);
/* Optional, MI355X-specific: derive a tile-local-column plan from the host struct the handle was made
 * from: per 256-row tile the list of 16-element x lines it touches plus 16-bit LDS-local
 * column indices.  uspmv_spmv then stages the x lines of a tile in LDS and streams 2-byte instead of
 * 4-byte indices (results unchanged, bit for bit).  Tiles touching more than max_lines lines (0 = default
 * 512) keep the gather path.  n_tiles / n_staged report the outcome (may be NULL).
 * With max_lines = 0 the planner has three fallbacks when the line plan leaves a tenth of the tiles or more unstaged: the same
 * plan over single x ELEMENTS (uspmv_dmat_plan_granularity = 1); that plan on rows dealt to the tiles by the matrix graph (a private copy of the values
 * in HBM, y stored through a row map -- for matrices whose rows and columns are numbered alike but not coherently); the column-window sweep for wide
 * irregular rows.  Every one of them walks each row's slots in the reference's order (scs_impl_cpu, code/kernels.hpp:218-258): same bits. */
int uspmv_dmat_optimize(uspmv_dmat_t *m, const uspmv_scs_t *s, int max_lines, int64_t *n_tiles, int64_t *n_staged);
/* Same for an ap[dp_sp] pair (structs with identical row layout): one shared line list per tile, 16-bit
 * indices for both structs; uspmv_spmv_ap then streams 10 + 6 instead of 12 + 8 bytes per non-zero.
 * Fallback order: lines -> elements -> sweep.  The shared plan over single x ELEMENTS (one list per 256-row tile over the columns of both
 * structs, the policy of uspmv_dmat_optimize: max_lines 0, a line plan that is invalid or stages under nine tenths of its tiles, at most a
 * tenth of the sampled tiles over "tlc_elem_cap", four entries per listed element) is installed on BOTH handles
 * (uspmv_dmat_plan_granularity = 1 on each, *n_tiles / *n_staged then describe it).  A pair falls to it by itself from 2^20 padded rows
 * on; a smaller pair goes from the line plan straight to the column-window sweep unless tuning "tlc_elem" is 2 (DESIGN.md 9.9 says why).
 * Same bits on every plan. */
int uspmv_dmat_optimize_ap(uspmv_dmat_t *dp, uspmv_dmat_t *sp, const uspmv_scs_t *s_dp, const uspmv_scs_t *s_sp,
                           int max_lines, int64_t *n_tiles, int64_t *n_staged);
/* Same for the two or three parts of an ap split with an fp16 part (hi: F64 or F32, mid: F32 or NULL, hp: F16; identical row layout):
 * one line list per tile over every part's columns, 16-bit local indices per part.  When the line plan stages fewer than half of the
 * tiles the column-window sweep shared by the parts is tried (uspmv_dmat_optimize_sweep_ap_hp with its defaults) and kept when it covers
 * at least half of its tiles; else the handles stay planless and uspmv_spmv_ap_hp runs its lane-per-row kernel.  n_tiles / n_staged
 * report the line plan's outcome either way; uspmv_dmat_plan_info tells which plan the handles carry.
 * Fallback order: lines -> elements -> sweep.  Between the two, under uspmv_dmat_optimize's policy (max_lines 0, a line plan that is
 * invalid or stages under nine tenths of its tiles, at most a tenth of the sampled tiles over "tlc_elem_cap" distinct columns -- counted
 * over all parts --, four entries per listed element; "tlc_elem" 0 never, 2 always tries), the shared plan over single x ELEMENTS is
 * installed on every part: uspmv_dmat_plan_granularity answers 1 on each handle, *n_tiles / *n_staged describe that plan, the cap is
 * counted in elements of x (double, float for ap[sp_hp]).  Same bits on every plan. */
int uspmv_dmat_optimize_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, const uspmv_scs_t *s_hi, const uspmv_scs_t *s_mid,
                              const uspmv_scs_t *s_hp, int max_lines, int64_t *n_tiles, int64_t *n_staged);
/* SpMMV counterpart of uspmv_dmat_optimize (no reference counterpart): plan for block vectors of
 * block_vec_size columns -- per 64-row tile the X rows it touches are staged in LDS once and the
 * kernel reads them with 2-byte local indices.  Used by uspmv_spmmv for b*sizeof(VT) in {16,32,64,128}
 * whose tiles fit, C = 32 or 64; other widths and chunk heights keep the gather kernels
 * (*n_staged = 0).  Results are bit-identical with and without the plan. */
int uspmv_dmat_optimize_block(uspmv_dmat_t *m, const uspmv_scs_t *s, int block_vec_size, int64_t *n_tiles, int64_t *n_staged);

/* Column-window sweep plan (no reference counterpart): for matrices with wide, irregular rows, where a
 * 256-row tile touches more x lines than LDS holds.  x is cut into windows of 2^wlog elements; a tile of tile_rows
 * (256 | 512 | 1024) rows whose rows all visit the windows in non-decreasing slot order (column-sorted rows do) is
 * processed by one workgroup that stages window after window in LDS and runs every row's entries of the staged
 * window -- same slot-ordered FMA chain, bit-identical y.  The plan holds a private, padding-free copy of the entries
 * (sizeof(VT) + 2 bytes per non-zero).  Tiles that do not qualify keep the gather kernel inside the same uspmv_spmv call.
 * wlog / tile_rows 0 = defaults (64 KiB windows; 2048 rows, 1024 for an ap pair).  uspmv_dmat_optimize[_ap] tries this by itself when the
 * tile-local-column plan stages less than half of the tiles.  n_tiles / n_sweep report the outcome (may be NULL). */
int uspmv_dmat_optimize_sweep(uspmv_dmat_t *m, const uspmv_scs_t *s, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep);
int uspmv_dmat_optimize_sweep_ap(uspmv_dmat_t *dp, uspmv_dmat_t *sp, const uspmv_scs_t *s_dp, const uspmv_scs_t *s_sp, int wlog,
                                 int tile_rows, int64_t *n_tiles, int64_t *n_sweep);
/* ... for the two or three parts of a split with an fp16 part (hi: F64 or F32, mid: F32 or NULL, hp: F16): one set of tile decisions
 * over all parts, per part its own padding-free stream -- 10 / 6 / 4 bytes per dp / sp / hp entry plus a count byte per (row, window).
 * The windows hold x in the type of the hi part (the default window of ap[sp_hp] holds twice the elements).  uspmv_spmv_ap_hp runs the
 * tiles that do not qualify on its lane-per-row kernel in the same call.  _device: built from the handles' own arrays, equal bit for bit. */
int uspmv_dmat_optimize_sweep_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, const uspmv_scs_t *s_hi, const uspmv_scs_t *s_mid,
                                    const uspmv_scs_t *s_hp, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep);
int uspmv_dmat_optimize_sweep_device_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, int wlog, int tile_rows, int64_t *n_tiles,
                                           int64_t *n_sweep);
/* Which single-vector plan uspmv_spmv / uspmv_spmv_ap will use: kind 0 none (gather kernel), 1 tile-local-column, 2 column-window
 * sweep; tiles of that plan and how many of them it covers (any pointer may be NULL). */
/* The column-window sweep plan built on the DEVICE from the handle's own arrays (csrc/sweep_plan_kernels.hip): what
 * uspmv_dmat_optimize_device[_ap] falls through to when the tile-local-column plan stages fewer than half of the tiles, so that
 * handles without a host struct (uspmv_dmat_wrap, the launchers of include/uspmv_launchers.hpp) reach scs_spmv_sweep.  sp: the sp
 * part of an ap[dp_sp] pair or NULL.  The arrays equal those of uspmv_dmat_optimize_sweep[_ap] bit for bit. */
int uspmv_dmat_optimize_sweep_device(uspmv_dmat_t *m, uspmv_dmat_t *sp, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep);
/* FNV-1a digests of the sweep plan's device arrays -- digest[0..3] the tile arrays, [4..8] part 0 as uspmv_dmat_sweep_plan_digest_part
 * gives it, [9] the chunks left to the gather kernel, [10..14] part 1 -- and meta[8] = present, rows per tile, log2 window, sweep
 * tiles, tiles, chunks left to the gather kernel, elements of the stream of part 0 / of part 1 (tests) */
int uspmv_dmat_sweep_plan_digest(const uspmv_dmat_t *m, uint64_t digest[16], int64_t meta[8]);
/* ... and of the arrays of ONE part of a shared sweep plan (m: the first part's handle; part 0, 1 or 2 in the order of the split):
 * digest[5] = wave offsets, counts, values, indices, padding columns; *n_vals = elements of the part's stream (may be NULL).  Zeros
 * when the handle has no such part (tests) */
int uspmv_dmat_sweep_plan_digest_part(const uspmv_dmat_t *m, int part, uint64_t digest[5], int64_t *n_vals);
int uspmv_dmat_plan_info(const uspmv_dmat_t *m, int *kind, int64_t *n_tiles, int64_t *n_planned);
/* block-vector plans of the handle: meta[10] = one-list-per-tile plan present, phased plan present, line plan present (column-major
 * block vectors staged by 128-byte lines, no re-layout pass), tiles, phases of the phased plan, phases of the line plan, X rows the
 * line plan stages, one-byte indices, index part built on the device, most X rows of a phase */
int uspmv_dmat_block_plan_info(const uspmv_dmat_t *m, int64_t meta[10]);
/* X rows the phased block plan stages per product (sum of its phases' lists; 0 without such a plan) */
int uspmv_dmat_block_plan_staged(const uspmv_dmat_t *m, int64_t *rows_staged);
/* x elements per entry of the tile-local-column plan's lists: 16 (128-byte lines, the default), 1 (single elements: the plan uspmv_dmat_optimize falls
 * to when a tile's columns are scattered over too many lines -- row numberings that are only locally coherent), 0 without such a plan.  Same kernel
 * arithmetic as scs_impl_cpu (code/kernels.hpp:218-258) either way.  Every handle of an ap split answers for the plan the split shares,
 * the parts that hold only their local indices included. */
int uspmv_dmat_plan_granularity(const uspmv_dmat_t *m, int *elements_per_list_entry);
/* 1 when that plan runs on rows dealt to its tiles by the matrix graph (private value copy in HBM, y stored through a row map), else 0 */
int uspmv_dmat_plan_rows_dealt(const uspmv_dmat_t *m, int *dealt);
/* the phased block plan laid out as a flat schedule for persistent workgroups (tuning "spmmv_stream" > 0 at plan time; the streaming form of
 * block_spmv_omp_scs_general, code/kernels.hpp:306-398): meta[2] = workgroups of the launch (0: no schedule on the handle), phase descriptors */
int uspmv_dmat_stream_info(const uspmv_dmat_t *m, int64_t meta[2]);
/* FNV-1a digests of the phased block plan's device arrays: phase pointers, first groups, list pointers, X-row lists, index offsets,
 * local indices, the group-major values, the row map (tests: a plan built on the device equals the host planner's) */
int uspmv_dmat_block_plan_digest(const uspmv_dmat_t *m, uint64_t digest[8]);

/* Block vectors with 64-byte X rows (dp b = 8, sp b = 16): the column-window sweep plan for block vectors.  A tile of 1 024 - 4 096 rows
 * walks the windows of 2^wlog X rows its rows touch, each staged in LDS once per tile (the phased plan above stages every X row once per
 * slot range: 11.9 against ~5 rows per matrix row on a 3-dof 27-point stencil), a lane owning whole rows; column-major X and Y are taken
 * as they are, without a re-layout pass.  Installed only when every tile qualifies (rows column-sorted at window granularity); uspmv_spmmv
 * then prefers it.  wlog / tile_rows 0 = defaults.  *n_sweep < *n_tiles: not installed.  Same bits as every other path. */
int uspmv_dmat_optimize_block_sweep(uspmv_dmat_t *m, const uspmv_scs_t *s, int block_vec_size, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep);

/* The block plan for a handle without a host struct (uspmv_dmat_wrap): the device arrays are copied to the host once and the plan is
 * built there.  No permutation is known then: ties of the sigma sort are ordered by first column instead of by original row. */
int uspmv_dmat_optimize_block_device(uspmv_dmat_t *m, int block_vec_size, int64_t *n_tiles, int64_t *n_staged);

/* The same plan built ON THE DEVICE from the handle's own arrays: for handles without a host struct
 * (uspmv_dmat_wrap around the reference's cudaMalloc'ed arrays, uspmv_convert_to_scs_device).  Chunk heights that
 * divide 256; tiles whose line range exceeds 65 536 lines stay on the gather path (the host planner may still
 * stage those); otherwise the plan is identical to uspmv_dmat_optimize's.  Narrow chunks (C in {1,2,4,8,16}, incl. crs) get the
 * same internal C = 32 re-chunking as in uspmv_dmat_optimize, copied on the device.
 * The order of the plans is uspmv_dmat_optimize's: the line plan, then -- max_lines 0 and a line plan that is invalid or stages under
 * nine tenths of its tiles -- the plan over single x elements on 256-row tiles, built on the device as well (a set of the tile's columns
 * in LDS, sorted; equal to the host planner's element plan array for array, *n_tiles / *n_staged then describe it and
 * uspmv_dmat_plan_granularity answers 1), then the column-window sweep.  Same tuning keys ("tlc_elem", "tlc_elem_cap").  Not here:
 * the element plan on rows dealt to the tiles by the matrix graph ("tlc_elem_rows"), which needs the host struct. */
int uspmv_dmat_optimize_device(uspmv_dmat_t *m, int max_lines, int64_t *n_tiles, int64_t *n_staged);
/* The shared plan of an ap[dp_sp] pair (uspmv_dmat_optimize_ap) built on the device from the two handles' own arrays, in the same
 * fallback order under the same policy: lines -> elements -> sweep (the element plan built on the device as well, equal to the host
 * planner's array for array; by itself from 2^20 padded rows on, else under "tlc_elem" 2). */
int uspmv_dmat_optimize_device_ap(uspmv_dmat_t *dp, uspmv_dmat_t *sp, int max_lines, int64_t *n_tiles, int64_t *n_staged);
/* The plan of uspmv_dmat_optimize_ap_hp built on the device from the handles' own arrays (equal to the host planner's array for array),
 * in the same fallback order under the same policy: lines -> elements -> sweep. */
int uspmv_dmat_optimize_device_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, int max_lines, int64_t *n_tiles, int64_t *n_staged);
/* host copies of a handle's plan (tests): meta = {n_tiles, n_lines_total, n_col16, max_lines_used}; call with NULL
 * arrays first to size them */
int uspmv_dmat_plan_download(const uspmv_dmat_t *m, int64_t meta[4], int32_t *tile_line_ptr, int32_t *tile_lines,
                             uint32_t *c16_ptrs, uint16_t *col16);

/* Rows per tile of the plan (256 | 512 | 1024; 0 = no plan).  A tile covers tile_rows/C consecutive chunks. */
int uspmv_dmat_tile_rows(const uspmv_dmat_t *m, int *tile_rows);
/* Bits per tile-local column index the plan's kernel streams: 16, or 12 where the plan packed them (tiles of at most 256 lines; kept when
 * the mean row length is >= 8; tuning key "tlc_idx12" 0 switches it off, 2 keeps it wherever it can be built); 0 = no plan */
int uspmv_dmat_index_bits(const uspmv_dmat_t *m, int *bits);
/* Additive chunk records (uspmv_dmat_optimize on one struct that carries its permutation, n_rows == n_cols, line plan kept; tuning key
 * "tlc_additive": 0 never, 1 kept when records + column map are at most half of the local-index stream they replace, 2 wherever they can
 * be built): the tiles' x windows are laid out in LDS in the column order the sigma sort started from, where the entries of most chunks of a
 * banded matrix sit at (one position per lane) + (one per slot); the kernel streams 64 + 2 * length bytes for such a chunk instead of 1.5 or
 * 2 bytes per entry.  n_chunks: chunks of the tiles that carry records (0: the handle has none), n_additive: the additive ones among them.
 * uspmv_dmat_index_bits keeps describing the local-index arrays, which stay as built. */
int uspmv_dmat_additive_chunks(const uspmv_dmat_t *m, int64_t *n_additive, int64_t *n_chunks);
/* The planner's encoder of those records on a host struct, no device needed (tests): the line plan uspmv_dmat_optimize would build at its
 * default rows per tile (256, or tuning key "tlc_tile_rows"), the records over it under the current "tlc_additive", then every record read back to the column of its entry.
 * stats = {kept, n_additive, n_chunks, tiles with records, tiles (of the records' own size where they have one), record bytes + map bytes, bytes of the stream replaced, LDS elements of the
 * fullest tile}; cols[n_elements] (may be NULL): the decoded column of every entry, padding included (-1: the entry's tile has no records). */
int uspmv_additive_plan_probe(const uspmv_scs_t *s, int64_t stats[8], int32_t *cols);
/* The staging data of the same plan: stats = {W (the 2-byte column map stays inside aligned blocks of W columns), entries of the tagged
 * line lists, x lines listed more than once (their elements go to more than one interval), bytes of the map}; all 0 without a plan. */
int uspmv_additive_plan_probe2(const uspmv_scs_t *s, int64_t stats[4]);
/* uspmv_spmv over a subset of tiles (d_tile_ids[n_ids]) of a handle with a plan: the interior /
 * boundary split of the halo-overlap scheme at tile granularity.  Entries < 0 are skipped (a list another kernel switches on or off). */
int uspmv_spmv_tiles(const uspmv_dmat_t *A, const int32_t *d_tile_ids, int64_t n_ids, const void *d_x, void *d_y,
                     void *stream);
/* Mark a C = 1 struct as "crs" (uspmv <mtx> crs): uspmv_spmv then uses the CRS kernel (several lanes
 * per row, twin of spmv_omp_csr) instead of the generic SELL kernel (twin of spmv_omp_scs). */
int uspmv_dmat_set_crs(uspmv_dmat_t *m, int on);

/* y = A x.  Replaces SpmvKernel::execute_one_prec -> spmv_gpu_scs_adv_launcher /
 * spmv_gpu_scs_launcher / spmv_gpu_csr_launcher (code/classes_structs.hpp:997-1035,
 * code/kernels.hpp:579-775), i.e. the GPU twins of spmv_omp_scs_adv / spmv_omp_scs /
 * spmv_omp_csr.  d_x: padded_vec_size elements; d_y: n_rows_padded elements written. */
int uspmv_spmv(const uspmv_dmat_t *A, const void *d_x, void *d_y, void *stream);
/* The fused update y = alpha A x + beta z with two dot products (no reference counterpart): what a residual, a CG step
 * or a Chebyshev / KPM recurrence does around an SpMV, applied where the kernel stores y instead of in extra passes over the vectors.
 * Numerics, with t_i exactly what uspmv_spmv stores for row i (the slot-ordered FMA chain) and alpha, beta converted ONCE to the handle's
 * value type:  beta == 0: y_i = rn(alpha t_i), z is never read (may be NULL, may hold NaN);  else y_i = rn(rn(alpha t_i) + rn(beta z_i)),
 * three separately rounded operations, never an FMA -- numpy arithmetic in the handle's type restates it bit for bit.  alpha = 1, beta = 0
 * gives uspmv_spmv's y.  Rows the call does not own stay untouched, as with uspmv_spmv.  Non-finite alpha / beta simply propagate.
 * dots (both accumulated in double from operands widened to double, one rounding per product): dots[0] = <y,y>, dots[1] = <w,y> over rows
 * [0, n_dot_rows); bitwise reproducible from call to call on the same handle, plan and tuning: every workgroup stores its two partial
 * sums at the slot of its logical id in a workspace of the handle, one small kernel on the same stream adds the slots in a fixed order --
 * no floating-point atomics, no host synchronisation.  The workspace is allocated on first use or by uspmv_spmv_axpby_reserve; a call that
 * would have to allocate while its stream is capturing returns USPMV_ERR_INVALID.  Not thread-safe per handle.
 * Refused before anything is launched or written: USPMV_ERR_UNSUPPORTED an F16 handle or a part of an adaptive-precision split;
 * USPMV_ERR_INVALID NULL op / d_x / d_y, beta != 0 with NULL d_z, d_z overlapping d_y partially (d_z == d_y, in place, is allowed),
 * n_dot_rows outside [0, rows y may be written].  d_y must NOT overlap d_x (not checked: a planless handle cannot know x's length). */
typedef struct {
    double alpha, beta;   /* converted ONCE to the handle's value type; all arithmetic is in that type */
    const void *d_z;      /* rows-y-may-be-written elements in y's row order; NULL allowed iff beta == 0; may be d_y itself (in place) */
    const void *d_w;      /* optional, y's row order: the second factor of dots[1]; NULL: dots[1] = 0, w never read */
    double *d_dots;       /* optional, 2 doubles on the device: dots[0] = <y,y>, dots[1] = <w,y>; NULL: no reduction at all */
    int64_t n_dot_rows;   /* rows [0, n_dot_rows) of y enter the dots (the caller's n_rows: padding rows stay out) */
} uspmv_axpby_t;
int uspmv_spmv_axpby(const uspmv_dmat_t *A, const void *d_x, void *d_y, const uspmv_axpby_t *op, void *stream);
/* Which way a call with this x goes, by the conditions the launcher uses: 1 fused in the epilogue of the SpMV kernel (every kernel
 * uspmv_spmv launches under the default tuning), 2 uspmv_spmv followed by one vector pass with the same epilogue (non-default "unroll",
 * "tail_batch", "nontemporal", "sweep_unroll", "sweep_pair", "spmv_variant", ablations).  An x off the 16-byte grid takes a planned
 * handle to the lane-per-row kernel, as in uspmv_spmv, which is fused under the default tuning as well.
 * Same numerics either way; the dots' summation order belongs to the path. */
int uspmv_spmv_axpby_path(const uspmv_dmat_t *A, const void *d_x, int *path);
/* Allocate the handle's workspace now (before a stream capture): the partial sums of either path under the current tuning, and the
 * in-place temporary of path 2 (one vector) where the handle takes path 2 under that tuning. */
int uspmv_spmv_axpby_reserve(uspmv_dmat_t *A);
/* Same over a subset of chunks (d_chunk_ids[n_ids], ascending): interior / boundary split used to
 * overlap the halo exchange with the kernel (absent in the reference, code/main.cpp:464-468). */
int uspmv_spmv_chunks(const uspmv_dmat_t *A, const int32_t *d_chunk_ids, int64_t n_ids, const void *d_x,
                      void *d_y, void *stream);
/* Y = A X, b right-hand sides.  Replaces block_spmv_gpu_scs_{adv,general}_launcher /
 * block_spmv_gpu_csr_launcher, which the reference only stubs on GPU (code/kernels.hpp:777-844);
 * semantics = block_spmv_omp_scs_general (code/kernels.hpp:306-398).  ld = vec_length of the
 * colwise layout (ignored for rowwise). */
int uspmv_spmmv(const uspmv_dmat_t *A, const void *d_X, void *d_Y, int b, int64_t ld, int layout, void *stream);
/* Which kernel the last uspmv_spmmv on this handle launched, as recorded on the host at the launch itself (tests: "the kernel under test
 * is the one that answered"; every rung of uspmv_spmmv's launch ladder that declines a call falls through to the next one, with the
 * same bits).  *kernel, the "spmmv_variant" number where there is one: 0 nothing launched yet, 1 the generic lane-per-row kernel
 * (scs_spmmv_rows), 2 scs_spmmv_xpose, 3 the gather kernel scs_spmmv_rowmajor on the original arrays, 4 scs_spmmv_tlc, 5
 * scs_spmmv_rowmajor on the block plan's re-ordered copy, 6 scs_spmmv_quad, 8 the phased kernel, 9 the block-vector window sweep
 * (scs_spmmv_sweep), 10 the phased plan streamed by persistent workgroups ("spmmv_stream").  *x_pass, what happened to X in that call:
 * 0 used as passed, 1 re-laid out into the workspace in this call, 2 the workspace prepared by uspmv_spmmv_x_prepared reused, 3 a
 * re-layout that also undid the sigma permutation ("spmmv_unscramble").  A handle that carries an internal re-chunking answers for it,
 * as uspmv_spmmv runs on it.  Nothing is launched. */
int uspmv_spmmv_last_path(const uspmv_dmat_t *m, int *kernel, int *x_pass);
/* Column-major block vectors whose X does NOT change between calls -- the reference's bench loop multiplies the same X in every
 * iteration (code/main.cpp:458-519): re-lay X out into the handle's row-major workspace once, now.  Until uspmv_spmmv_x_release, every
 * uspmv_spmmv(m, d_X, ..., b, ld, USPMV_COLWISE) with THIS pointer, b and ld skips its re-layout pass (another X, b or ld takes the
 * per-call re-layout as before and overwrites the workspace: call again afterwards).  The caller promises that the CONTENTS of X are
 * unchanged since this call; a caller that writes X (solve mode: x <- y) must call again or release.  Widths without a re-layout pass
 * (b not in {2, 4, 8, 16}) return USPMV_OK and skip nothing. */
int uspmv_spmmv_x_prepared(const uspmv_dmat_t *m, const void *d_X, int block_vec_size, int64_t ld, void *stream);
int uspmv_spmmv_x_release(const uspmv_dmat_t *m);
/* Adaptive precision dp+sp.  Replaces execute_two_prec -> spmv_gpu_ap_scs_adv_launcher
 * (code/classes_structs.hpp:1037-1075, code/ap_kernels.hpp:821-953); numerics follow the CPU
 * kernel scs_ap_impl_cpu (code/ap_kernels.hpp:24-82): both parts accumulated in double from the
 * double x, y = dp_sum + sp_sum.  dp and sp must share C and n_chunks. */
int uspmv_spmv_ap(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, double *d_y, void *stream);
/* uspmv_spmv_ap restricted to a subset of the rows, for the distributed ap step (no twin in the reference, which refuses ap under MPI:
 * "not supported at this time", code/utilities.hpp:1445-1451).  Extends uspmv_spmv_tiles / uspmv_spmv_chunks to the ap[dp_sp] pair; every
 * row written carries the bits uspmv_spmv_ap gives it, rows outside the list are not touched.
 * _tiles: the tiles of the pair's shared tile-local-column plan (uspmv_dmat_optimize_ap; tile t = rows [t * tile_rows, (t + 1) * tile_rows)),
 *   x must be 16-byte aligned.  _chunks: chunk ids, lane per row, any pair.  Entries < 0 are skipped (a conditional list). */
int uspmv_spmv_ap_tiles(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const int32_t *d_tile_ids, int64_t n_ids, const double *d_x,
                        double *d_y, void *stream);
int uspmv_spmv_ap_chunks(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const int32_t *d_chunk_ids, int64_t n_ids, const double *d_x,
                         double *d_y, void *stream);
/* Adaptive precision dp+sp on block vectors: Y = (A_dp + A_sp) X, b right-hand sides, X and Y double.  The reference has no such path
 * (its CLI stops at "SpMMV is not yet implemented for AP kernels", code/utilities.hpp:1389).  For every C, column v of Y is bitwise what
 * uspmv_spmv_ap gives for column v of X: per (row, v) the dp FMA chain and the sp FMA chain of scs_ap_impl_cpu, each in slot order,
 * Y(r, v) = dp + sp.  Layouts and ld as uspmv_spmmv; all n_rows_padded rows of every vector are written and nothing else of Y.
 * b = 1 is uspmv_spmv_ap.  uspmv_spmmv_x_prepared(dp, ...) / uspmv_spmmv_x_release(dp) are honoured for column-major X as by uspmv_spmmv:
 * the re-layout workspace of the pair lives on the dp handle.  b in {2, 4, 8, 16} with 16-byte-aligned X and Y (and an even ld for
 * column-major vectors): a pair that carries the column-window sweep plan (uspmv_dmat_optimize_ap / _device_ap on wide irregular rows,
 * uspmv_dmat_optimize_sweep_ap / _device) whose windows leave room for two vectors in LDS (uspmv_spmmv_ap_sweep_vectors(b, wlog) >= 2:
 * wlog <= 13) runs the block form of the sweep kernel, except for row-major X in more than two passes: the plan's compacted dp and sp
 * streams are walked once per uspmv_spmmv_ap_sweep_vectors(b, wlog) vectors, the windows of X staged in LDS straight from either layout (no workspace is used or
 * grown, and uspmv_spmmv_x_prepared has nothing to skip there); tiles that do not sweep run lane per row.  A pair that carries one shared
 * tile-local-column plan (uspmv_dmat_optimize_ap / _device_ap) of at most uspmv_spmmv_ap_plan_lines(b) lines per tile runs the kernel
 * that stages the tile's X rows in LDS and streams 10 + 6 bytes per non-zero and pass over the vectors; without a plan (none, or tuning
 * "sweep" / "tlc" 0) the gather kernel runs on the original arrays.  Any other b or alignment: the generic kernel.
 * uspmv_spmmv_ap_path reports which of these a call would take. */
int uspmv_spmmv_ap(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const void *d_X, void *d_Y, int b, int64_t ld, int layout,
                   void *stream);
/* The largest max_lines a caller can pass to uspmv_dmat_optimize_ap / _device_ap for which the staged kernel of uspmv_spmmv_ap applies
 * to width b whatever the matrix: 640 for b in {2, 4, 8, 16} (two vectors of 640 lines x 16 X rows fill the 160 KiB of LDS a workgroup
 * can have; fewer lines leave room for 4 or 8 vectors per pass), 0 where no staged kernel exists for that b. */
int uspmv_spmmv_ap_plan_lines(int b, int *max_lines);
/* What uspmv_spmmv_ap(dp, sp, X, Y, b, ld, layout) would run for 16-byte-aligned X and Y, under the current tuning.  *path: 0 the generic
 * lane-per-row kernel, 1 the gather kernel on the original arrays, 2 the staged kernel over the shared tile-local-column plan, 3 the
 * column-window sweep kernel.  *vectors_per_pass: the vectors the sweep kernel (path 3) or the staged kernel (path 2) serves per pass over
 * the matrix entries, else 0.  b = 1 reports uspmv_spmv_ap's choice: 3 its sweep kernel, 2 its staged kernel (one vector per pass), 0
 * lane per row.  Same argument checks and error texts as uspmv_spmmv_ap (under this function's name); nothing is launched. */
int uspmv_spmmv_ap_path(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, int b, int64_t ld, int layout, int *path, int *vectors_per_pass);
/* uspmv_spmmv_ap restricted to a subset of the rows, for the distributed ap block step (uspmv_dist_spmmv_ap): the block twins of
 * uspmv_spmv_ap_tiles / _chunks.  X and Y double, layouts and ld as uspmv_spmmv_ap.  Every row written carries, in every column, the bits
 * uspmv_spmmv_ap gives it (one lane per row, every chain in slot order); rows outside the list are not touched.  Entries < 0 are skipped
 * (a conditional list); n_ids == 0 is USPMV_OK and launches nothing.
 * _tiles: the tiles of the pair's shared tile-local-column plan (tile t = rows [t * tile_rows, (t + 1) * tile_rows)); a pair without one
 *   is refused.  b in {2, 4, 8, 16}, X and Y 16-byte aligned, an even ld for column-major vectors, "tlc" 1, "spmmv_variant" not 1 and room
 *   for two vectors of the fullest tile in LDS: workgroup g runs tile d_tile_ids[g] with the staged kernel of uspmv_spmmv_ap, which here
 *   stages X straight from EITHER layout (no re-layout workspace: a part of a step has no whole X to re-lay out).  Otherwise lane per
 *   row over the tiles' rows.
 * _chunks: chunk ids, lane per row, any pair, any b, layout and alignment.
 * _tiles_path: what _tiles would run for 16-byte-aligned X and Y under the current tuning -- *path 2 the staged kernel
 *   (*vectors_per_pass of the b vectors per pass over the entries), 0 lane per row (*vectors_per_pass 0).  The checks and error texts of
 *   _tiles under this function's name; nothing is launched. */
int uspmv_spmmv_ap_tiles(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const int32_t *d_tile_ids, int64_t n_ids, const void *d_X, void *d_Y,
                         int b, int64_t ld, int layout, void *stream);
int uspmv_spmmv_ap_chunks(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const int32_t *d_chunk_ids, int64_t n_ids, const void *d_X,
                          void *d_Y, int b, int64_t ld, int layout, void *stream);
int uspmv_spmmv_ap_tiles_path(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, int b, int64_t ld, int layout, int *path,
                              int *vectors_per_pass);
/* The vectors per pass the sweep kernel of uspmv_spmmv_ap takes at width b on a plan whose windows hold 2^wlog doubles: the largest of
 * {8, 4, 2} that is at most b, divides b and fits 160 KiB of LDS with one window (2^wlog * 8 bytes per vector); 0 where the kernel does not
 * apply (b not in {2, 4, 8, 16}, or wlog >= 14: two vectors of a window do not fit).  A pure function: callers use it to choose wlog for
 * uspmv_dmat_optimize_sweep_ap / _device when they want all b vectors in one pass (wlog 13 serves 2, 12 serves 4, 11 serves 8).
 * Narrower windows win from b = 4 on (banded-random 500 k x 140 pair: b = 4 0.347 ms at wlog 12 against 0.450 at 13; b = 8 0.704-0.777 at
 * wlog 11 against 0.878-1.170 at 13), the opposite of uspmv_spmv_ap, whose best window is the planner's default: 2^14 doubles under
 * "sweep_nbuf" 1 (no block kernel there), 2^13 under "sweep_nbuf" 2.  Row-major X in more than two passes (b / vectors > 2) keeps the
 * gather kernel whatever this function says: uspmv_spmmv_ap_path reports it.
 * b < 1, wlog outside 8..16 or a NULL pointer is refused. */
int uspmv_spmmv_ap_sweep_vectors(int b, int wlog, int *vectors);
/* Generic-C variant of the reference, spmv_omp_scs_ap / spmv_gpu_ap_scs (code/ap_kernels.hpp:562-634,
 * :721-816; selected for C outside {2,4,...,128}, code/classes_structs.hpp:630-636): the sp part
 * multiplies with the FLOAT copy of x (d_x_sp), the float product being rounded before it is added
 * to the double accumulator. */
int uspmv_spmv_ap_generic(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, const float *d_x_sp,
                          double *d_y, void *stream);
/* Adaptive precision with an fp16 part (the reference's uspmv_scs_apdphp_cpu / _apsphp_cpu / _apdpsphp_cpu, code/interface.hpp:1512-1740;
 * its GPU path stops at "not yet implemented", code/classes_structs.hpp:553-600).  hi F64 or F32, mid F32 or NULL (hi F64 then), hp F16,
 * all sharing C and n_chunks.  One set of numerics for every C:
 *   ap[dp_hp]     (hi F64, no mid): x, y double; a dp and an hp chain in double (hp widened exactly), each an FMA chain in slot order;
 *                 y = dp + hp
 *   ap[dp_sp_hp]  (hi F64, mid F32): three such chains; y = (dp + sp) + hp
 *   ap[sp_hp]     (hi F32, no mid): x, y float; every product sp_v * x and (float)hp_v * x rounded to float, then added to a double
 *                 accumulator per part; y = (float)(sp + hp) */
int uspmv_spmv_ap_hp(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, void *d_y, void *stream);
/* The fused update y = alpha A x + beta z with two dot products on the parts of an adaptive-precision split (no reference counterpart;
 * DESIGN.md 5.13): uspmv_spmv_axpby's operand struct and contract with ONE change -- t_i is what uspmv_spmv_ap / uspmv_spmv_ap_hp stores
 * for row i on these handles, the parts' slot-ordered chains combined as there: dp + sp, hi + hp, (hi + mid) + hp, or (float)(sp + hp).
 * alpha and beta are converted ONCE to the type of x and y (double; float for ap[sp_hp], whose z and w are float as well).
 * beta == 0: y_i = rn(alpha t_i), z is never read (may be NULL, may hold NaN);  else y_i = rn(rn(alpha t_i) + rn(beta z_i)), three
 * separately rounded operations, never an FMA.  alpha = 1, beta = 0 without dots gives uspmv_spmv_ap[_hp]'s y bit for bit.  d_z may be
 * d_y (in place).  dots as in uspmv_spmv_axpby: accumulated in double over rows [0, n_dot_rows), one rounding per product, no
 * floating-point atomics, no host synchronisation; every workgroup stores its two partial sums at the slot of its logical id -- a call
 * served by two launches (sweep tiles, then the chunks the plan leaves over) gives the second launch the slots behind the first's -- and
 * one finalize kernel on the same stream adds the slots in a fixed order: bitwise reproducible on the same handles, plan and tuning.
 * The workspace (the partial sums and, on path 2, the in-place temporary) lives on the FIRST handle (dp / hi); it is allocated on
 * first use or by the _reserve call, and a call that would have to allocate while its stream is capturing returns USPMV_ERR_INVALID and
 * names the _reserve call.  Not thread-safe per first handle.
 * Refused before anything is launched or written: the argument checks of uspmv_spmv_ap / uspmv_spmv_ap_hp (handles that do not form a
 * split, wrong dtypes, mismatched C or n_chunks), then USPMV_ERR_INVALID for NULL op / d_x / d_y, beta != 0 with NULL d_z, d_z overlapping
 * d_y partially, n_dot_rows outside [0, n_chunks * C].  d_y must NOT overlap d_x (not checked).  The generic-C variant with a float copy
 * of x (uspmv_spmv_ap_generic) has no fused form.
 * _path: 1 fused in the store epilogue of the kernel(s) uspmv_spmv_ap[_hp] launches (every kernel of the default tuning), 2 that call
 * followed by one vector pass with the same epilogue ("nontemporal" 0; "unroll" < 8 on the pair's lane-per-row kernel; "sweep_unroll" < 8
 * or "sweep_pair" != 2 on a sweep plan).  An x off the 16-byte grid leaves the plan for the lane-per-row kernel, as in the plain call. */
int uspmv_spmv_ap_axpby(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const double *d_x, double *d_y, const uspmv_axpby_t *op, void *stream);
int uspmv_spmv_ap_axpby_path(const uspmv_dmat_t *dp, const uspmv_dmat_t *sp, const void *d_x, int *path);
int uspmv_spmv_ap_axpby_reserve(uspmv_dmat_t *dp, const uspmv_dmat_t *sp);
int uspmv_spmv_ap_hp_axpby(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, void *d_y,
                           const uspmv_axpby_t *op, void *stream);
int uspmv_spmv_ap_hp_axpby_path(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_x, int *path);
int uspmv_spmv_ap_hp_axpby_reserve(uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp);
/* uspmv_spmv_ap_hp restricted to a subset of the rows, for the distributed step of the kinds with an fp16 part (uspmv_dist_create_ap_hp_from_coo):
 * the twins of uspmv_spmv_ap_tiles / _chunks.  Handles as for uspmv_spmv_ap_hp (mid NULL for the two-part kinds), x and y in the type of the hi
 * part.  Every row written carries the bits uspmv_spmv_ap_hp gives it, rows outside the list are not touched.  Entries < 0 are skipped (a
 * conditional list); n_ids == 0 is USPMV_OK and launches nothing.
 * _tiles: the tiles of the parts' shared tile-local-column plan (tile t = rows [t * tile_rows, (t + 1) * tile_rows)); parts without one are
 *   refused ("no shared tile-local-column plan").  x must be 16-byte aligned, n_ids at most the number of tiles.
 * _chunks: chunk ids, lane per row, any such handles. */
int uspmv_spmv_ap_hp_tiles(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const int32_t *d_tile_ids, int64_t n_ids,
                           const void *d_x, void *d_y, void *stream);
int uspmv_spmv_ap_hp_chunks(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const int32_t *d_chunk_ids, int64_t n_ids,
                            const void *d_x, void *d_y, void *stream);
/* Adaptive precision with an fp16 part on block vectors: b right-hand sides, X and Y in the type of the hi part (double for ap[dp_hp] and
 * ap[dp_sp_hp], float for ap[sp_hp]), handles as for uspmv_spmv_ap_hp, layouts and ld as uspmv_spmmv / uspmv_spmmv_ap (column-major
 * X[col + v*ld] with ld >= n_rows_padded, row-major X[col*b + v]).  The reference has no such path.  For every C, both layouts and every
 * b >= 1, column v of Y is bit for bit what uspmv_spmv_ap_hp writes for column v of X: per (row, v) one chain per part in slot order with
 * the numerics above, then y = hi + hp, (hi + mid) + hp or (float)(sp + hp).  All n_rows_padded rows of every vector are written and
 * nothing else of Y; b = 1 is uspmv_spmv_ap_hp.  No workspace is used on any handle (uspmv_spmmv_x_prepared has nothing to skip here).
 * b in {2, 4, 8, 16} with 16-byte-aligned X and Y (and, column-major, ld * sizeof(element) a multiple of 16) takes one of two block
 * kernels.  Parts that carry one shared column-window sweep plan (uspmv_dmat_optimize_ap_hp / _device_ap_hp on wide irregular rows,
 * uspmv_dmat_optimize_sweep_ap_hp / _device_ap_hp) whose window leaves room for two vectors in the 160 KiB of LDS
 * (uspmv_spmmv_ap_hp_sweep_vectors(b, wlog, x_dtype) >= 2: wlog <= 13 for double X, <= 14 for float X) run the block form of the sweep
 * kernel under tuning "sweep" 1: every part's compacted stream is walked once per BS = uspmv_spmmv_ap_hp_sweep_vectors vectors, the
 * windows of X staged in LDS straight from either layout, b / BS passes inside one launch, in one pass or several (every multi-pass
 * combination of layout and number of passes measured ahead of the generic kernel);
 * tiles that do not sweep run lane per row.  The planner's default window (2^14 doubles / 2^15 floats under "sweep_nbuf" 1) holds one
 * vector: such handles keep the generic kernel until they are planned with a narrower window.  Parts that carry one shared
 * tile-local-column plan (uspmv_dmat_optimize_ap_hp / _device_ap_hp) whose fullest tile fits the LDS with two vectors run the staged
 * kernel: per pass over the matrix entries the tile's X rows of BS vectors are staged in LDS straight from either layout and every part
 * streams sizeof(value) + 2 bytes per entry; BS is the largest of {8, 4, 2} that is at most b and fits the fullest tile, b / BS passes
 * inside one launch.  Everything else -- planless handles, tuning "tlc" 0 / "sweep" 0 or "spmmv_variant" 1, other widths, unaligned
 * vectors -- runs the generic lane-per-row kernel.  uspmv_spmmv_ap_hp_path reports which. */
int uspmv_spmmv_ap_hp(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const void *d_X, void *d_Y, int b, int64_t ld,
                      int layout, void *stream);
/* What uspmv_spmmv_ap_hp(hi, mid, hp, X, Y, b, ld, layout) would run for 16-byte-aligned X and Y, under the current tuning; the codes keep
 * the meaning they have in uspmv_spmmv_ap_path.  *path: 0 the generic lane-per-row kernel, 2 the staged kernel over the shared
 * tile-local-column plan, 3 the column-window sweep kernel over the shared sweep plan (1 is not returned by this function).
 * *vectors_per_pass: the vectors per pass of the staged or the sweep kernel, else 0.  b = 1 reports uspmv_spmv_ap_hp's own choice with
 * one vector per pass: 3 its sweep kernel, 2 its staged kernel, 0 lane per row.
 * Same argument checks and error texts as uspmv_spmmv_ap_hp (under this function's name); nothing is launched. */
int uspmv_spmmv_ap_hp_path(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, int b, int64_t ld, int layout, int *path,
                           int *vectors_per_pass);
/* uspmv_spmmv_ap_hp restricted to a subset of the rows, for the distributed block step of the kinds with an fp16 part
 * (uspmv_dist_spmmv_ap_hp): the block twins of uspmv_spmv_ap_hp_tiles / _chunks and the twins of uspmv_spmmv_ap_tiles / _chunks / _tiles_path
 * for these kinds.  Handles as for uspmv_spmmv_ap_hp (mid NULL for the two-part kinds), X and Y in the type of the hi part, layouts and ld
 * as there.  Every row written carries, in every column, the bits uspmv_spmmv_ap_hp gives it (one lane per row, every chain in slot order,
 * (hi + mid) folded before the hp chain); rows outside the list are not touched.  Entries < 0 are skipped (a conditional list);
 * n_ids == 0 is USPMV_OK and launches nothing.
 * _tiles: the tiles of the parts' shared tile-local-column plan (tile t = rows [t * tile_rows, (t + 1) * tile_rows)); parts without one --
 *   planless ones, and those that carry a column-window sweep plan instead -- are refused ("no shared tile-local-column plan").
 *   b in {2, 4, 8, 16}, X and Y 16-byte aligned, "tlc" 1, "spmmv_variant" not 1 and room for two vectors of the fullest tile in LDS:
 *   workgroup g runs tile d_tile_ids[g] with the staged kernel of uspmv_spmmv_ap_hp, X staged straight from either layout.  Column-major
 *   X is taken at EVERY ld: where ld * sizeof(element) is no multiple of 16 -- a rank's padded_vec_size is whatever its halo makes it -- the
 *   columns are staged in the widest pieces all of them start aligned to (8 bytes for double X and for float X with ld % 4 == 2, 4 bytes
 *   for float X with an odd ld), a wave's loads of one column's line running over consecutive addresses.  Otherwise lane per row over
 *   the tiles' rows.
 * _chunks: chunk ids, lane per row, any such handles, any b, layout and alignment.
 * _tiles_path: what _tiles would run for 16-byte-aligned X and Y under the current tuning -- *path 2 the staged kernel
 *   (*vectors_per_pass of the b vectors per pass over the entries), 0 lane per row (*vectors_per_pass 0).  The checks and error texts of
 *   _tiles under this function's name; nothing is launched. */
int uspmv_spmmv_ap_hp_tiles(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const int32_t *d_tile_ids, int64_t n_ids,
                            const void *d_X, void *d_Y, int b, int64_t ld, int layout, void *stream);
int uspmv_spmmv_ap_hp_chunks(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, const int32_t *d_chunk_ids, int64_t n_ids,
                             const void *d_X, void *d_Y, int b, int64_t ld, int layout, void *stream);
int uspmv_spmmv_ap_hp_tiles_path(const uspmv_dmat_t *hi, const uspmv_dmat_t *mid, const uspmv_dmat_t *hp, int b, int64_t ld, int layout,
                                 int *path, int *vectors_per_pass);
/* The largest max_lines a caller can pass to uspmv_dmat_optimize_ap_hp / _device_ap_hp for which the staged kernel of uspmv_spmmv_ap_hp
 * applies at width b whatever the matrix: two vectors of the fullest tile (16 X rows per line) in the 160 KiB of LDS -- 640 for
 * x_dtype USPMV_F64 and 1280 for USPMV_F32 at b in {2, 4, 8, 16}, 0 for every other b.  b < 1, another dtype or a NULL pointer is refused. */
int uspmv_spmmv_ap_hp_plan_lines(int b, int x_dtype, int *max_lines);
/* The vectors per pass the sweep kernel of uspmv_spmmv_ap_hp takes at width b on a plan whose windows hold 2^wlog elements of X
 * (x_dtype USPMV_F64 for ap[dp_hp] and ap[dp_sp_hp], USPMV_F32 for ap[sp_hp]): the largest of {8, 4, 2} that is at most b, divides b
 * and fits the 160 KiB of LDS with one window (2^wlog * sizeof(element) bytes per vector); 0 where the kernel does not apply (b not in
 * {2, 4, 8, 16}, or not even two vectors fit):
 *     wlog       <= 11   12   13   14   15
 *     double X      8     4    2    0    0
 *     float X       8     8    4    2    0
 * A function of (b, wlog, x_dtype) alone, never of the matrix: callers use it to choose wlog for uspmv_dmat_optimize_sweep_ap_hp /
 * _device_ap_hp (all b vectors in one pass: wlog 13 / 14 serves 2, 12 / 13 serves 4, 11 / 12 serves 8).  Several passes stay on the sweep kernel in
 * both layouts, but a narrower window that takes more vectors per pass is faster from b = 4 on.
 * b < 1, wlog outside 8..16, another x_dtype or a NULL pointer is refused (USPMV_ERR_INVALID). */
int uspmv_spmmv_ap_hp_sweep_vectors(int b, int wlog, int x_dtype, int *vectors);

/* Raw-array forms with the argument lists of the library kernels of code/interface.hpp
 * (uspmv_scs_gpu :1766-1793, uspmv_scs_c_gpu :1835-1867, uspmv_csr_gpu :1741-1760). */
int uspmv_scs_gpu_f64(int64_t C, int64_t n_chunks, const int32_t *d_chunk_ptrs, const int32_t *d_chunk_lengths,
                      const int32_t *d_col_idxs, const double *d_values, const double *d_x, double *d_y,
                      void *stream);
int uspmv_scs_gpu_f32(int64_t C, int64_t n_chunks, const int32_t *d_chunk_ptrs, const int32_t *d_chunk_lengths,
                      const int32_t *d_col_idxs, const float *d_values, const float *d_x, float *d_y,
                      void *stream);
int uspmv_csr_gpu_f64(int64_t n_rows, const int32_t *d_row_ptrs, const int32_t *d_col_idxs,
                      const double *d_values, const double *d_x, double *d_y, void *stream);
int uspmv_csr_gpu_f32(int64_t n_rows, const int32_t *d_row_ptrs, const int32_t *d_col_idxs,
                      const float *d_values, const float *d_x, float *d_y, void *stream);

/* Read one scalar through a pointer that may point to host OR device memory (the reference's GPU build keeps C and n_chunks
 * in device memory, code/utilities.hpp:3803-3811; include/uspmv_launchers.hpp reads them once per set of arrays). */
int uspmv_peek_i64(const void *p, int64_t *out);
int uspmv_peek_i32(const void *p, int32_t *out);

/* Device apply_permutation: d_out[i] = d_in[d_perm[i]] (code/utilities.hpp:1768-1782). */
int uspmv_apply_permutation_dev(void *d_out, const void *d_in, const int32_t *d_perm, int64_t n, int dtype,
                                void *stream);

/* Kernel-variant selection for A/B measurements (DESIGN.md "variants").  key/value pairs:
 *   "unroll" 1|2|4|8, "nontemporal" 0|1, "block" 64|128|256|512|1024,
 *   "xcd_remap" 0 (hardware order) | 1 (one contiguous eighth of the grid per XCD) | G >= 2 (groups
 *   of G consecutive workgroups per XCD), "spmv_variant" 0 (lane per row, bit-exact) | 1 (two lanes
 *   per row, C=32 only), "csr_lanes" 0 (auto) | 1..64 lanes per row of the CRS kernel,
 *   "tlc" 1|0 use the tile-local-column kernel when the handle has a plan, "tail_batch" 0|1,
 *   "tlc_tile_rows" 0|256|512|1024 rows (= threads) per tile of the NEXT uspmv_dmat_optimize[_ap|_device|_device_ap]
 *   (0 = 256 for one struct, 512 for an ap[dp_sp] pair), "tlc_auto_tile" 1|0: with "tlc_tile_rows" 0 and one struct, take
 *   1024- or 512-row tiles instead when the largest 256-row tile needs more than 250 x lines and the larger tiles stage >= 99 %
 *   of the tiles (same y bits; measured in profiles/r03/tile_rows_sweep.txt), "tlc_measure_tile" 1|0: structs of >= 2^20 padded rows get
 *   the tile size that MEASURES fastest (plans for 256 / 512 / 1024 rows built on the device, three timed launches each, once per matrix
 *   shape and process),
 *   "spmmv_variant" 0 (auto) | 1 (generic) | 2 (row-major, transposing X phase) | 3 (row-major, lane per row)
 *                   | 4 (single-wave block-plan tiles) | 5 (3 over the plan's tie-re-ordered copy) | 6 (four lanes per row, 64-byte rows)
 *                   | 8 (four lanes per row over the phased plan; what auto picks for 64-byte rows),
 *   "spmmv_phased" 1|0 and "spmmv_phase_rows" 256|512: NEXT uspmv_dmat_optimize_block with 64-byte rows also builds the phased plan,
 *   "spmmv_xcol" 0|1: phased kernel on column-major X behind a re-layout pass (0) or assembling its X rows from the caller's vector itself (1),
 *   "spmmv_swizzle" 0|1 bank-swizzled LDS rows in the block-plan kernel,
 *   "spmmv_reorder" 1|2|0 NEXT uspmv_dmat_optimize_block, row order of the plan's private copy of the entries: 1 = the sigma sort's tie
 *   scrambling undone, 2 = rows re-dealt to the 64-row tiles as breadth-first balls of the matrix graph (fewer X rows per tile, but
 *   scattered y rows: measured slower on config 3, kept as an option), 0 = the caller's order;
 *   "spmmv_idx8" 1|0 NEXT uspmv_dmat_optimize_block: one-byte phase-local indices when no phase lists more than 256 X rows,
 *   "spmmv_list_plan" 0|1 NEXT uspmv_dmat_optimize_block: also build the one-list-per-tile plan of variants 4-6 (and its column-major copy
 *   of the entries) when the phased kernel can take the matrix,
 *   "sweep" 1|0 use a handle's column-window sweep plan (uspmv_spmv, uspmv_spmv_ap, uspmv_spmv_ap_hp, uspmv_spmmv, and uspmv_spmmv_ap at b in {2, 4, 8, 16}: 0 there = the gather kernel),
 *   "sweep_nbuf" 1|2 LDS buffers, "sweep_unroll" 2|4|8, "sweep_remap" tiles per XCD group,
 *   "sweep_threads" 0|256|512|1024 threads per sweep workgroup (0 = min(tile rows, 1024); fewer threads = more rows per lane, at most 4),
 *   "sweep_wlog" / "sweep_tile_rows" / "sweep_max_stage" defaults of the NEXT sweep plan (window = 2^wlog elements; rows per tile;
 *   largest staging cost in bytes per non-zero for a tile to qualify, 0 = 24),
 *   "raw_plan_cache" 0|1 uspmv_scs_gpu_f64/f32 keep a device-built plan per set of array addresses (the caller
 *   promises not to put another matrix behind the same pointers; uspmv_raw_plan_cache_clear() otherwise),
 *   "spmmv_tile_rows" 0 (auto) | 32 | 64 rows per tile and "spmmv_lds_kb" 0 (= 80) | LDS KiB per tile of the NEXT
 *   uspmv_dmat_optimize_block,
 *   "spmmv_prefetch" 1|0 (lane-per-row kernel: next batch of matrix entries requested behind the X rows),
 *   "spmmv_unroll" 0 (auto) | 1|2|4|8 slots per batch,
 *   "ablate" 0 | 1 | 2 (measurement only: gathers collapsed / removed, results are wrong). */
void uspmv_raw_plan_cache_clear(void);
/* raw-array entry points behind "raw_plan_cache": the caller rewrote the value array at d_values in place (same pattern) -- refresh the
 * cached plans whose values pointer is d_values (uspmv_dmat_values_changed on each) instead of clearing the cache and planning again;
 * *n_entries (may be NULL) = how many */
int uspmv_raw_plan_cache_values_changed(const void *d_values, void *stream, int *n_entries);
int uspmv_set_tuning(const char *key, int value);
int uspmv_get_tuning(const char *key, int *value);

/* ------------------------------------------------------------------ L4: halo exchange     */
/* seg_work_sharing_arr (code/mpi_funcs.hpp:424-622), seg-rows and seg-nnz: wsa[P+1]. */
int uspmv_seg_work_sharing_arr(const uspmv_coo_t *total, int seg_method, int P, int32_t *wsa);
/* -seg_metis (code/mpi_funcs.hpp:494-598) without METIS: a part id per row from the built-in partitioner (breadth-first level sets
 * from a pseudo-peripheral vertex, P equal pieces of that ordering, boundary refinement; vertex counts balanced like
 * METIS_PartGraphKway without weights) or from a file with one part id per line (the output format of gpmetis) ... */
int uspmv_graph_partition(const uspmv_coo_t *total, int P, int32_t *part /* n_rows */);
int uspmv_read_partition(const char *path, int64_t n_rows, int P, int32_t *part);
/* ... and the reference's post-processing of it (:529-598): rows stable-sorted by part (new row r = old row perm[r]), the matrix
 * permuted symmetrically (entry order inside a row kept), wsa[P+1] from the part sizes.  perm may be NULL. */
int uspmv_coo_apply_partition(const uspmv_coo_t *total, int P, const int32_t *part, uspmv_coo_t **permuted, int32_t *wsa, int32_t *perm);
/* the same rule from per-row entry counts alone (bit-identical wsa to the call above on the row-sorted COO) */
int uspmv_seg_from_row_counts(const int32_t *row_nnz, int64_t n_rows, int seg_method, int P, int32_t *wsa);
/* seg_mtx_struct + localize_row_idx (code/mpi_funcs.hpp:636-674, :862-877): rows
 * [wsa[rank], wsa[rank+1]) with process-local row ids and GLOBAL column ids. */
int uspmv_seg_local_coo(const uspmv_coo_t *total, const int32_t *wsa, int rank, uspmv_coo_t **out);
/* collect_local_needed_heri (code/mpi_funcs.hpp:242-415): discovers remote columns of the local
 * SCS struct (scanned in storage order, padding entries included), rewrites col_idxs to
 * local + halo numbering, and records per owner which of ITS local rows this rank needs. */
int uspmv_halo_discover(uspmv_scs_t *local_scs, const int32_t *wsa, int rank, int P, uspmv_halo_t **out);
/* uspmv_halo_discover for the two structs of an ap[dp_sp] pair: ONE halo, as if collect_local_needed_heri ran over the dp struct's
 * col_idxs followed by the sp struct's (first-seen scan in that order), both structs' columns rewritten against that one numbering.
 * The structs must share C, n_chunks and the row layout (sp converted with dp's permutation). */
int uspmv_halo_discover_ap(uspmv_scs_t *dp, uspmv_scs_t *sp, const int32_t *wsa, int rank, int P, uspmv_halo_t **out);
/* ... and for the two or three structs of a split with an fp16 part (mid NULL for ap[dp_hp] and ap[sp_hp]): ONE halo, the first-seen scan over
 * hi's col_idxs, then mid's, then hp's; all structs' columns rewritten against that one numbering.  Refusals as above: the structs must share
 * C, n_chunks and the row layout, no struct may appear twice, and nothing is rewritten when the call is refused. */
int uspmv_halo_discover_ap_hp(uspmv_scs_t *hi, uspmv_scs_t *mid, uspmv_scs_t *hp, const int32_t *wsa, int rank, int P, uspmv_halo_t **out);
/* n_halo = recv_counts_cumsum.back(); recv_counts_cumsum[P+1]; recv_idxs grouped by owner rank
 * ascending with recv_counts[P] entries each (borrowed pointers). */
int uspmv_halo_meta(const uspmv_halo_t *h, int64_t *n_halo, const int32_t **recv_counts_cumsum,
                    const int32_t **recv_idxs, const int32_t **recv_counts);
void uspmv_halo_free(uspmv_halo_t *h);
/* Chunk ids whose columns are all local (< n_local) and the rest (touch the halo region). Arrays
 * are malloc'ed; release with uspmv_free. */
int uspmv_scs_split_chunks(const uspmv_scs_t *s, int64_t n_local, int32_t **interior, int64_t *n_interior,
                           int32_t **boundary, int64_t *n_boundary);
/* The same split in three classes, classes[n_chunks]: 0 = no halo column; 1 = halo columns only through the reference's padding -- entries
 * that are +0.0 on the ONE column *pad_col (value 0, column 0: code/utilities.hpp:1991-2002; a halo column on every rank but the first,
 * code/mpi_funcs.hpp:279-306); 2 = other halo references.  *pad_col = -1 when no chunk is of class 1.  (What "pad_split" of
 * uspmv_dist_set_option is built on.) */
int uspmv_scs_chunk_classes(const uspmv_scs_t *s, int64_t n_local, uint8_t *classes, int32_t *pad_col);
/* collect_local_needed_heri (code/mpi_funcs.hpp:242-415) + permute_scs_cols (code/utilities.hpp:1802-1831) ON THE DEVICE, for handles whose
 * entries never visit the host (csrc/halo_kernels.hip): parts[0 .. n_parts) (1 .. 3: one struct, or the parts of an
 * adaptive-precision split in the order hi, mid, lo) hold GLOBAL column ids (converted with permute_cols = 0), own their arrays (a
 * uspmv_dmat_wrap handle is refused), carry no plan, and share C and n_chunks.  ONE first-seen numbering over the parts' col_idxs taken as
 * one array in storage order, part after part, padding entries (column 0) included -- a column's first-seen position is the least
 * (part << 32 | storage index) among the entries that name it, found by a 64-bit atomic minimum per column; its slot within its owner is
 * its rank under that key (the n_halo claimed columns are ordered on the host, O(n_halo) records cross).  Then every part's col_idxs is
 * rewritten in place: a local column to d_old_to_new[col - wsa[rank]] (device array of n_local entries; NULL: col - wsa[rank]), a remote
 * one to n_local + base[owner] + slot.  *out equals the plan of uspmv_halo_discover[_ap | _ap_hp] on the same structs integer for
 * integer.  n_cols: columns of the global matrix (the table has max(wsa[P], n_cols) entries of 8 bytes -- the device memory this call takes
 * beyond the handles, plus 16 bytes per halo column).  Refused before anything is written: a column outside [0, max(wsa[P], n_cols))
 * ("column %d outside the global matrix", the first in scan order, as on the host), a column no block owns, n_local + n_halo beyond
 * int32 (USPMV_ERR_OVERFLOW).  Works on `stream`; returns when the handles are rewritten. */
int uspmv_halo_discover_device(uspmv_dmat_t *const parts[], int n_parts, int64_t n_cols, const int32_t *wsa, int rank, int P,
                               const int32_t *d_old_to_new, void *stream, uspmv_halo_t **out);
/* uspmv_scs_chunk_classes of a device handle (F64, F32 or F16; the +0.0 test is on the value's bits), bit for bit: one wave per chunk,
 * O(n_chunks) bytes come back.  classes: host array of n_chunks. */
int uspmv_dmat_chunk_classes_device(const uspmv_dmat_t *m, int64_t n_local, uint8_t *classes, int32_t *pad_col, void *stream);
void uspmv_free(void *p);
/* Send-buffer gather for ALL neighbours in one launch over the concatenated index list:
 * d_send[i] = d_x[d_perm[d_send_idxs[i]] + block_offset].  Replaces pack_send_buf /
 * pack_d_send_buf (code/classes_structs.hpp:786-855, code/kernels.hpp:554-577: one launch +
 * device sync per neighbour). */
int uspmv_pack_send_buf(const void *d_x, const int32_t *d_perm, const int32_t *d_send_idxs, int64_t n,
                        int64_t block_offset, void *d_send, int dtype, void *stream);

/* ------------------------------------------------------------------ L4a: set-up transport, host communicator, exchange plan */
/* collect_comm_info (code/mpi_funcs.hpp:1061-1124) needs two exchanges between the ranks: every rank tells every owner HOW MANY
 * of the owner's rows it needs (the reference all-gathers the cumsums, :190-196) and WHICH (the MPI_INT index all-to-all,
 * :143-171).  Both run over this small transport, so the SAME C++ set-up is driven by RCCL (device staging, the default of
 * uspmv_dist_create), by the host communicator below (real processes, no GPU: tests/test_dist_setup_mp.py) and in loopback.
 * All buffers are HOST memory; offsets are in bytes with size+1 entries:
 *   alltoallv: recv[recv_off[q] .. recv_off[q+1]) <- rank q's send[send_off_q[me] .. send_off_q[me+1])
 *   allgather: recv[q*bytes .. (q+1)*bytes) <- rank q's send[0 .. bytes) */
typedef struct uspmv_transport {
    void *ctx;
    int rank, size;
    int (*alltoallv)(void *ctx, const void *send, const int64_t *send_off, void *recv, const int64_t *recv_off);
    int (*allgather)(void *ctx, const void *send, void *recv, int64_t bytes_per_rank);
    int (*barrier)(void *ctx);
} uspmv_transport_t;

/* Host communicator of ONE node: the ranks of a job meet in a memory-mapped segment (<USPMV_HC_DIR or /dev/shm>/uspmv_hc_<job>,
 * published by rank 0 with an atomic rename and unlinked as soon as every rank has attached; leftovers of a crashed job are
 * recognised by their dead creator and ignored).  Stands where the reference has MPI_Bcast / MPI_Allgather / the index exchange
 * during set-up (code/mpi_funcs.hpp:143-171, :190-196, :732-736); every wait has a deadline (timeout_s, <= 0: 300 s) and fails
 * on all ranks with USPMV_ERR_COMM when a peer dies. */
typedef struct uspmv_hostcomm uspmv_hostcomm_t;
int uspmv_hostcomm_create(const char *job, int rank, int size, double timeout_s, uspmv_hostcomm_t **out);
int uspmv_hostcomm_info(const uspmv_hostcomm_t *h, int *rank, int *size, uint64_t *nonce /* random per segment, same on all ranks */);
int uspmv_hostcomm_barrier(uspmv_hostcomm_t *h);
int uspmv_hostcomm_abort(uspmv_hostcomm_t *h);   /* tell the peers this rank cannot go on: their next wait fails at once */
int uspmv_hostcomm_bcast(uspmv_hostcomm_t *h, void *buf, int64_t bytes, int root);
int uspmv_hostcomm_allgather(uspmv_hostcomm_t *h, const void *send, void *recv, int64_t bytes_per_rank);
int uspmv_hostcomm_alltoallv(uspmv_hostcomm_t *h, const void *send, const int64_t *send_off, void *recv, const int64_t *recv_off);
int uspmv_hostcomm_allreduce_max_f64(uspmv_hostcomm_t *h, double *value);
int uspmv_hostcomm_transport(uspmv_hostcomm_t *h, uspmv_transport_t *t);   /* the transport view (h must outlive its users) */
void uspmv_hostcomm_free(uspmv_hostcomm_t *h);

/* organize_cumsums + collect_comm_idxs (code/mpi_funcs.hpp:117-232): from what this rank NEEDS from whom (its halo description)
 * to what it must SEND to whom -- collective over the transport, no GPU involved.  send_off[P+1] / recv_off[P+1] count elements;
 * send_idxs[send_off[p] .. send_off[p+1]) are THIS rank's local rows (original order) rank p asked for, i.e. the reference's
 * comm_send_idxs[p].  Every id is checked against [0, n_local): a peer asking for a row this rank does not own is an error on
 * this rank (USPMV_ERR_INVALID), never an out-of-bounds gather. */
typedef struct uspmv_comm_plan uspmv_comm_plan_t;
int uspmv_comm_plan_create(const uspmv_transport_t *t, const uspmv_halo_t *halo, uspmv_comm_plan_t **out);
int uspmv_comm_plan_meta(const uspmv_comm_plan_t *p, int64_t *n_send, const int64_t **send_off, const int32_t **send_idxs,
                         const int64_t **recv_off);
void uspmv_comm_plan_free(uspmv_comm_plan_t *p);

/* ------------------------------------------------------------------ L4b: the distributed step on RCCL */
/* One process per GPU.  Replaces the per-iteration MPI flow of the reference -- init_local_structs (code/main.cpp:1075-1334),
 * collect_comm_info (code/mpi_funcs.hpp:1061-1124), init/finalize_halo_exchange (code/classes_structs.hpp:857-995) and the
 * exchange-then-kernel iteration of bench_spmv (code/main.cpp:458-474) -- by a C++ object that owns an RCCL communicator:
 * per SpMV one pack kernel, one grouped ncclSend/ncclRecv landing in the tail of x on a side stream, the interior tiles /
 * chunks meanwhile, the boundary ones after it; uspmv_dist_run replays the whole step from ONE captured hipGraph. */
typedef struct uspmv_dist uspmv_dist_t;
#define USPMV_COMM_ID_BYTES 128
/* ncclGetUniqueId on the root rank; the bytes reach the other ranks by any side channel (a file, torch.distributed, MPI_Bcast) */
int uspmv_comm_unique_id(void *id128);
/* Partition block `rank` of P on communicator rank comm_rank of comm_size.  comm_size == P (one rank per block), or comm_size == 1
 * with P > 1: LOOPBACK -- this process plays block `rank` and every neighbour is itself (RCCL self send/recv of the ids it asked
 * for); with an x that repeats with the block height that reproduces the multi-rank result of the block's rows on one GPU.
 * A / halo / the id lists are the caller's (A must outlive the object): halo from uspmv_halo_discover, old_to_new_idx the row
 * permutation of the local struct, interior / boundary ids from uspmv_scs_split_chunks (chunk ids) or tile ids of A's plan. */
int uspmv_dist_create(const void *comm_id, int comm_rank, int comm_size, int rank, int P, uspmv_dmat_t *A, const uspmv_halo_t *halo,
                      const int32_t *old_to_new_idx, const int32_t *interior_ids, int64_t n_interior, const int32_t *boundary_ids,
                      int64_t n_boundary, int ids_are_tiles, uspmv_dist_t **out);
/* The whole of init_local_structs for one block: convert_to_scs -> halo discovery -> column permutation -> upload -> plan ->
 * interior / boundary split -> uspmv_dist_create.  `local` = rows [wsa[rank], wsa[rank+1]) with local row ids and GLOBAL
 * column ids (uspmv_seg_local_coo or a generator's row range).  The object owns everything it built. */
int uspmv_dist_create_from_coo(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                               const int32_t *wsa, int64_t C, int64_t sigma, int dtype, int tlc, uspmv_dist_t **out);
/* The same two with options.  transport: who carries the set-up exchanges (NULL = the RCCL communicator, device-staged; loopback
 * uses an identity transport).  exchange: USPMV_EXCHANGE_RCCL (default) or USPMV_EXCHANGE_HOST -- the per-step halo exchange
 * staged through host memory over `transport` (pack kernel -> D2H -> all-to-all-v -> H2D into the tail of x), which lets P real
 * processes share ONE GPU: it is how a single-GPU box runs the C++ step with unequal seg-nnz blocks and asymmetric send / recv
 * lists (tests/test_dist_native_gpu.py).  With USPMV_EXCHANGE_HOST no RCCL communicator is created (comm_id may be NULL);
 * transport->size must equal P and transport->rank the block.  The transport must outlive the object.
 * USPMV_EXCHANGE_PEER: peer stores.  Every rank owns a receive window (hipMalloc, double-buffered by step parity, exported through
 * hipIpcGetMemHandle); one push kernel per step stores the rank's halo contributions straight into its neighbours' windows (opened
 * through hipIpcOpenMemHandle: across xGMI on a node, device to device when ranks share one GPU), the host waits for it, the ranks
 * meet in the transport's barrier, and an unpack kernel copies the window into the tail of x.  No communication kernel, no host copy
 * of the data, no RCCL communicator (comm_id may be NULL; uspmv_dist_comm_count gives 0).  Real ranks (comm_size == P > 1) need a
 * transport (all-gather and barrier: set-up, per-step barrier, uspmv_dist_barrier / _allreduce_max / _allgather_i64); loopback
 * (comm_size == 1, P > 1) takes none and pushes into its own window.  Set-up is collective and fails on every rank alike (export /
 * open failures, inconsistent send / receive counts); a failed set-up (also the window growth of uspmv_dist_spmmv) leaves the object
 * without windows: its steps then fail with USPMV_ERR_INVALID until uspmv_dist_spmmv on every rank sets them up again.
 * uspmv_dist_free is collective too (close, barrier, free).  Steps run eagerly:
 * uspmv_dist_run(use_graph = 1) falls back to eager steps.  Every option and step form applies, with the same bits as the other
 * exchanges.  On ROCm, IPC between processes needs HSA_ENABLE_IPC_MODE_LEGACY=0 in every rank's environment. */
typedef enum { USPMV_EXCHANGE_RCCL = 0, USPMV_EXCHANGE_HOST = 1, USPMV_EXCHANGE_PEER = 2 } uspmv_exchange;
typedef struct uspmv_dist_options {
    const uspmv_transport_t *transport;
    int exchange;
} uspmv_dist_options_t;
int uspmv_dist_create_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, uspmv_dmat_t *A, const uspmv_halo_t *halo,
                         const int32_t *old_to_new_idx, const int32_t *interior_ids, int64_t n_interior, const int32_t *boundary_ids,
                         int64_t n_boundary, int ids_are_tiles, const uspmv_dist_options_t *opt, uspmv_dist_t **out);
int uspmv_dist_create_from_coo_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                  const int32_t *wsa, int64_t C, int64_t sigma, int dtype, int tlc, const uspmv_dist_options_t *opt,
                                  uspmv_dist_t **out);
/* uspmv_dist_create_from_coo[_ex] for adaptive precision ap[dp_sp] (the reference refuses ap under MPI, code/utilities.hpp:1445-1451):
 * uspmv_partition_precisions of the block at threshold_1 -> convert the dp part -> the sp part with the dp part's permutation ->
 * uspmv_halo_discover_ap -> column permutation of both -> upload -> with tlc the pair's shared line plan at 256-row tiles -> tile classes
 * from both parts -> the object.  Vectors are double.  Its step is uspmv_spmv_ap split into interior and boundary tiles (chunks);
 * "pad_split" defaults to 1 here (an ap pair pads nearly every chunk of both parts, and the padding column is a halo column on every
 * rank but the first).  "fused_step", "block_plan", "autotune_all" and uspmv_dist_spmmv answer USPMV_ERR_UNSUPPORTED on such an object; its
 * block-vector step is uspmv_dist_spmmv_ap. */
int uspmv_dist_create_ap_from_coo(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                  const int32_t *wsa, int64_t C, int64_t sigma, double threshold_1, int tlc, uspmv_dist_t **out);
int uspmv_dist_create_ap_from_coo_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                     const int32_t *wsa, int64_t C, int64_t sigma, double threshold_1, int tlc,
                                     const uspmv_dist_options_t *opt, uspmv_dist_t **out);
/* ... for the kinds with an fp16 part: kind USPMV_AP_DP_HP, USPMV_AP_SP_HP or USPMV_AP_DP_SP_HP (USPMV_AP_DP_SP is refused: that object is
 * made by uspmv_dist_create_ap_from_coo).  uspmv_partition_precisions_hp of the block -> convert the hi part (F32 for ap[sp_hp], else F64) ->
 * the mid and hp parts with hi's permutation -> uspmv_halo_discover_ap_hp -> column permutation of all parts -> upload -> with tlc the
 * parts' shared line plan at 256-row tiles, as built (no timing, no sweep plan; dropped for chunk lists when it stages nothing) -> tile
 * classes from all parts -> the object.  A block whose conversion the host route refuses ("fixed_permutation maps a non-empty row onto a
 * padded slot") fails the call with that text.  Vectors are in the type of the hi part: float for ap[sp_hp] (pack, exchange, padding
 * guard and self-check then work on floats), double otherwise.  The step is uspmv_spmv_ap_hp split into interior and boundary tiles
 * (uspmv_spmv_ap_hp_tiles / _chunks) in the overlap, plain and "pad_split" forms ("pad_split" defaults to 1), eager or captured, over every
 * exchange.  "fused_step" 1, "autotune_all" 1, "block_plan" b > 0, uspmv_dist_spmmv and uspmv_dist_spmmv_ap answer USPMV_ERR_UNSUPPORTED
 * with the kind's name: block vectors for these kinds run through uspmv_dist_spmmv_ap_hp. */
int uspmv_dist_create_ap_hp_from_coo(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                     const int32_t *wsa, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2, int tlc,
                                     uspmv_dist_t **out);
int uspmv_dist_create_ap_hp_from_coo_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                        const int32_t *wsa, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2, int tlc,
                                        const uspmv_dist_options_t *opt, uspmv_dist_t **out);
/* uspmv_dist_create_from_coo / _ap_from_coo / _ap_hp_from_coo for a block that lives in HBM: d_I local row ids, d_J GLOBAL
 * column ids, d_V (device arrays of nnz entries, sorted by row -- what uspmv_seg_local_coo gives), n_cols the columns of the global matrix.
 * kind: USPMV_ONE_PRECISION (dtype F64 | F32), USPMV_AP_DP_SP, or a kind with an fp16 part (dtype is then ignored; threshold_2 only for
 * USPMV_AP_DP_SP_HP).  The host route's steps in the host route's order (init_local_structs, code/main.cpp:1075-1334), each on the device:
 * uspmv_partition_precisions_device -> uspmv_convert_to_scs_device_from_arrays (first part with its own sigma ordering under sort_mode,
 * the others with its permutation; permute_cols 0) -> uspmv_halo_discover_device -> with tlc the (shared) line plan at 256-row tiles
 * from the handles' own arrays -> uspmv_dmat_chunk_classes_device -> the object; nothing of O(nnz) crosses to the host.  Refusals as on
 * the host route, an empty block of wsa first and on all ranks alike.  USPMV_SORT_HOST: every array of the object equals the host
 * route's; USPMV_SORT_DEVICE_STABLE: y in original row order does, the permutations may differ in the order of equal-length rows.
 * The object owns handles and halo; uspmv_dist_parts[_ap | _ap_hp] hand out the first part's struct WITHOUT entries (meta data, chunk
 * arrays, permutations -- what uspmv_dist_check needs) and NULL for the other parts' structs.  "block_plan" plans from the handle. */
enum { USPMV_ONE_PRECISION = -1 };
int uspmv_dist_create_from_arrays(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const int32_t *d_I, const int32_t *d_J,
                                  const double *d_V, int64_t nnz, int64_t n_cols, const int32_t *wsa, int64_t C, int64_t sigma, int kind, int dtype,
                                  double threshold_1, double threshold_2, int tlc, int sort_mode, void *stream, uspmv_dist_t **out);
int uspmv_dist_create_from_arrays_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const int32_t *d_I, const int32_t *d_J,
                                     const double *d_V, int64_t nnz, int64_t n_cols, const int32_t *wsa, int64_t C, int64_t sigma, int kind, int dtype,
                                     double threshold_1, double threshold_2, int tlc, int sort_mode, const uspmv_dist_options_t *opt, void *stream,
                                     uspmv_dist_t **out);
/* the exchange plan of the object (borrowed): n_send, send_off[P+1], send_idxs[n_send], recv_off[P+1] as in uspmv_comm_plan_meta */
int uspmv_dist_comm_plan(const uspmv_dist_t *d, int64_t *n_send, const int64_t **send_off, const int32_t **send_idxs,
                         const int64_t **recv_off);
/* Options by name: "overlap" 1|0, "no_pack" 0|1, "ba_synch" 0|1 (a stream-ordered one-element all-reduce after every step: the
 * MPI_Barrier the reference issues per iteration by default, code/main.cpp:467, :417; part of the captured graph),
 * "capture_mode" 0 global | 1 thread-local | 2 relaxed (hipStreamCaptureMode of uspmv_dist_run's capture),
 * "diag_skip_exchange" 0|1 (diagnosis only: the step skips the halo exchange, results are wrong),
 * "diag_peer_skew" 0|1 (test only, USPMV_EXCHANGE_PEER: this rank announces one halo element too many from its first neighbour at the
 *   next window set-up -- the growth in uspmv_dist_spmmv -- which every rank must then refuse alike),
 * "fused_step" 0|1 (default 0; tile lists: the step's tiles in ONE launch -- interior and padding tiles first, the boundary tiles at the end of
 *   the grid, each of which looks once whether the exchange has completed and otherwise defers itself to a small second launch behind
 *   the exchange; nothing spins.  0: interior launch, exchange, boundary launch),
 * "pad_split" 0|1 (default 0, on an ap[dp_sp] object 1; 1: padding tiles run with the interior ones, see uspmv_dist_pad_info; 0: with the
 *   boundary tiles),
 * "autotune_all" 0|1 (default 0: uspmv_dist_autotune times overlap | plain; 1: the pad / fused arrangements as well),
 * "diag_spmmv_part" 0|1|2 (diagnosis only: the two-part block-vector step runs both parts, its interior part, its boundary part),
 * "block_plan" b (block vectors: build the phased block plan for b columns on the rank's matrix, 0 drops it; see uspmv_dist_spmmv).
 * On an ap[dp_sp] object (uspmv_dist_create_ap_from_coo) "fused_step" 1, "autotune_all" 1 and "block_plan" b > 0 answer
 * USPMV_ERR_UNSUPPORTED; uspmv_dist_autotune times overlap | plain there and leaves "pad_split" as it is.  The same holds for an object
 * of a kind with an fp16 part (uspmv_dist_create_ap_hp_from_coo), whose "pad_split" defaults to 1 as well. */
int uspmv_dist_set_option(uspmv_dist_t *d, const char *key, int value);
/* How the single-vector step is arranged around the exchange: interior tiles during the exchange and boundary tiles after it | the
 * exchange, then the whole matrix (the reference's order) | overlap with the padding-only tiles in front of the exchange ("pad_split") |
 * that in one launch ("fused_step", eager steps only).  uspmv_dist_autotune times the first two (all four with "autotune_all" 1: the last
 * two have never run next to an exchange between different GPUs) for 2 x (10 + 40) steps on the machine at hand --
 * COLLECTIVE: every rank calls it; the ranks agree on the slowest rank's clock -- sets the options of the fastest and returns it with
 * the candidates' ms per step (0: not tried; negative: fastest but refused by the self-check).  With `local` and `wsa` (as for
 * uspmv_dist_check, which it then runs) a pad / fused winner must pass the bitwise self-check on every rank or the faster of the first
 * two takes over.  d_x keeps its local part (its halo tail and d_y are overwritten).  All arrangements give the same bits. */
typedef enum { USPMV_STEP_OVERLAP = 0, USPMV_STEP_PLAIN = 1, USPMV_STEP_PAD = 2, USPMV_STEP_FUSED = 3 } uspmv_step_form;
int uspmv_dist_autotune(uspmv_dist_t *d, void *d_x, void *d_y, int use_graph, const uspmv_coo_t *local, const int32_t *wsa, void *stream,
                        int *form, double ms[4]);
/* Self-check of the whole distributed path (partition, halo discovery, exchange plan, exchange, kernels) on the object's own
 * matrix: one step with x_global[j] = 1 + 1e-3 * (j mod 1000) -- every halo element differs from its neighbours, unlike the
 * benchmark's constant 5.0 -- and y of the local rows compared BITWISE with the rows' entry-ordered FMA chains evaluated on the
 * host straight from `local` (global column ids; the role of the reference's MKL validation, code/write_results.hpp:442-556).
 * mismatches = rows that differ on this rank, checksum = sum of the local y in original order (both optional). */
int uspmv_dist_check(uspmv_dist_t *d, const uspmv_coo_t *local, const int32_t *wsa, void *d_x, void *d_y, int use_graph,
                     void *stream, int64_t *mismatches, double *checksum);
/* uspmv_dist_check against a block that lives in HBM (d_I local row ids, d_J GLOBAL column ids, d_V; nnz entries sorted by row -- the
 * arrays the object was made from by uspmv_dist_create_from_arrays, or uspmv_gen_stencil27_device's): the same x, the same single step,
 * the same meaning of mismatches and checksum.  The rows' entry-ordered FMA chains are evaluated by a kernel from the device arrays (row
 * bounds from the sorted row ids; F64 object: double chain; F32 object: (float) value and float x, float chain; ap[dp_sp]: the dp chain
 * over |v| >= threshold_1 and the sp chain over the rest with (double)(float)v, y = dp + sp); x_global is evaluated on the host and
 * uploaded (O(columns)), the comparison and the checksum run on the host on the downloaded y of the local rows (O(local rows), the
 * summation order of uspmv_dist_check).  Nothing of O(nnz) exists on the host.  An object of a kind with an fp16 part:
 * USPMV_ERR_UNSUPPORTED; a column id outside the global matrix (wsa[P] columns): USPMV_ERR_INVALID. */
int uspmv_dist_check_arrays(uspmv_dist_t *d, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t nnz, const int32_t *wsa,
                            void *d_x, void *d_y, int use_graph, void *stream, int64_t *mismatches, double *checksum);
/* The host half of that check alone (no GPU): y_ref[i] (n_rows of `local`, dtype) = the entry-ordered FMA chain of local row i over
 * x_global[j] = 1 + 1e-3 * (j mod 1000), for steps that do not run on a uspmv_dist object (bench.py's torch.distributed twin). */
int uspmv_dist_check_reference(const uspmv_coo_t *local, const int32_t *wsa, int rank, int P, int dtype, void *y_ref);
/* uspmv_dist_check_reference for an ap[dp_sp] object (uspmv_dist_check applies it there): per local row the dp chain over the entries
 * with |v| >= threshold_1 and the sp chain over the others with the value (double)(float)v, each an FMA chain in entry order from +0.0
 * (scs_ap_impl_cpu, code/ap_kernels.hpp:24-82), y_ref[i] = dp + sp (double). */
int uspmv_dist_check_reference_ap(const uspmv_coo_t *local, const int32_t *wsa, int rank, int P, double threshold_1, double *y_ref);
/* ... for an object of a kind with an fp16 part (uspmv_dist_check applies it there).  The entries are classified exactly as
 * uspmv_partition_precisions_hp classifies them (hp values rounded once to binary16), and the numerics are those of uspmv_spmv_ap_hp.
 * USPMV_AP_DP_HP / USPMV_AP_DP_SP_HP: one FMA chain per part in entry order from +0.0, y_ref[i] = hi + hp resp. (hi + mid) + hp (double).
 * USPMV_AP_SP_HP: x converted to float, every product rounded to float and then added to the part's double accumulator,
 * y_ref[i] = (float)(sp + hp) (float). */
int uspmv_dist_check_reference_ap_hp(const uspmv_coo_t *local, const int32_t *wsa, int rank, int P, int kind, double threshold_1,
                                     double threshold_2, void *y_ref);
/* HIP / RCCL versions this library was COMPILED against and the ones it RUNS on in this process:
 * v[0] HIP_VERSION (build), v[1] hipRuntimeGetVersion, v[2] NCCL_VERSION_CODE (build), v[3] ncclGetVersion. */
int uspmv_runtime_versions(int v[4]);
/* Ranks of the RCCL communicator the step's exchange runs on (ncclCommCount; the reference prints MPI_Comm_size, code/main.cpp:1838);
 * 0 when the exchange is staged through the host or stored by peers (no communicator exists). */
int uspmv_dist_comm_count(const uspmv_dist_t *d, int *n_ranks);
/* the object's exchange (uspmv_exchange) */
int uspmv_dist_exchange(const uspmv_dist_t *d, int *exchange);
/* meta[12] = n_local, n_halo, padded_vec_size, n_send, n_interior, n_boundary, ids_are_tiles, n_rows_padded, loopback,
 *            graph captured, graph launches so far, eager steps so far */
int uspmv_dist_info(const uspmv_dist_t *d, int64_t meta[12]);
/* borrowed handles of an object made by uspmv_dist_create_from_coo (NULL scs / halo otherwise).  An object made by
 * uspmv_dist_create_from_arrays answers with a struct that has no entries (uspmv_scs_arrays: NULL col_idxs / values), here and below. */
int uspmv_dist_parts(const uspmv_dist_t *d, const uspmv_scs_t **scs, const uspmv_dmat_t **A, const uspmv_halo_t **halo);
/* uspmv_dist_parts of an ap[dp_sp] object: both structs, both handles, the one halo (uspmv_dist_parts answers with the dp ones);
 * the sp ones are NULL on a one-precision object */
int uspmv_dist_parts_ap(const uspmv_dist_t *d, const uspmv_scs_t **scs_dp, const uspmv_scs_t **scs_sp, const uspmv_dmat_t **A_dp,
                        const uspmv_dmat_t **A_sp, const uspmv_halo_t **halo);
/* uspmv_dist_parts of an object of a kind with an fp16 part: its kind, the structs, the handles (mid NULL for the two-part kinds) and
 * the one halo.  uspmv_dist_parts answers such an object with the hi ones, uspmv_dist_parts_ap with USPMV_ERR_INVALID; any other object
 * is refused here. */
int uspmv_dist_parts_ap_hp(const uspmv_dist_t *d, int *kind, const uspmv_scs_t **scs_hi, const uspmv_scs_t **scs_mid, const uspmv_scs_t **scs_hp,
                           const uspmv_dmat_t **A_hi, const uspmv_dmat_t **A_mid, const uspmv_dmat_t **A_hp, const uspmv_halo_t **halo);
int uspmv_dist_set_overlap(uspmv_dist_t *d, int overlap);
/* -no_pack 1 of the reference (code/classes_structs.hpp:941): no element is packed (pushed), every exchange of the object ships a
 * stale buffer (timing only) */
int uspmv_dist_set_no_pack(uspmv_dist_t *d, int no_pack);
/* one step, issued eagerly: d_x (padded_vec_size elements; its halo tail is written), d_y (n_rows_padded written) */
int uspmv_dist_spmv(uspmv_dist_t *d, void *d_x, void *d_y, int comm_halos, void *stream);
/* n_steps steps back to back.  use_graph != 0: the step is captured once per (d_x, d_y, stream) into a hipGraph and
 * replayed (needs an explicit stream); falls back to eager steps when the runtime refuses the capture. */
int uspmv_dist_run(uspmv_dist_t *d, void *d_x, void *d_y, int n_steps, int use_graph, void *stream);
/* Block vectors: Y = A X with the halo exchange of the b vectors in one of the reference's message patterns (compile-time modes
 * there: SINGLEVEC / MULTIVEC / BULKVEC_MPI_MODE, code/classes_structs.hpp:875-924, code/mpi_funcs.hpp:35-60), then uspmv_spmmv on
 * the block (ld = padded_vec_size).  Column-wise X: all three; row-wise X: USPMV_BULKVEC (its per-neighbour block IS the halo
 * region of X, no staging).
 * The reference exchanges first and computes then (code/mpi_funcs.hpp:25-60).  Here the step has the same two parts as the
 * single-vector one ("overlap" 1, the default): the chunks that touch no halo row run on a side stream while the exchange is under
 * way, the others after it -- the same kernel twice over chunk-length arrays in which the other part's chunks are marked, so every
 * row's FMA chain is the one-part step's (bit-identical Y).  Column-wise X: the interior part re-lays out the local rows into the
 * handle's row-major workspace, the boundary part the halo rows once they are there.  uspmv_dist_set_option(d, "block_plan", b)
 * builds the phased block plan of uspmv_dmat_optimize_block on the rank's matrix (64-byte X rows) together with the
 * interior / boundary classes of its tiles; uspmv_dist_set_option(d, "overlap", 0) restores exchange-then-compute.
 * With USPMV_EXCHANGE_HOST the same wire formats travel through pinned host memory and the transport's all-to-all-v (tests: real ranks
 * sharing one GPU on unequal blocks).  With USPMV_EXCHANGE_PEER one push stores all b columns into windows sized for n_halo x b, grown
 * collectively when a wider block first appears; the three patterns share that one wire format. */
typedef enum { USPMV_BULKVEC = 0, USPMV_MULTIVEC = 1, USPMV_SINGLEVEC = 2 } uspmv_vecmode;
int uspmv_dist_spmmv(uspmv_dist_t *d, void *d_X, void *d_Y, int b, int layout, int mode, int comm_halos, void *stream);
/* uspmv_dist_spmmv for an ap[dp_sp] object (uspmv_dist_create_ap_from_coo; one entry point per kind, as uspmv_spmmv / uspmv_spmmv_ap):
 * same arguments, X and Y double, ld = padded_vec_size, row-wise X bulkvec only; a one-precision object is refused.  b = 1 is the eager
 * single-vector step (uspmv_dist_spmv).  P == 1 or comm_halos 0: uspmv_spmmv_ap on the block.  "overlap" 0: the exchange, then
 * uspmv_spmmv_ap.  "overlap" 1 (default): the single-vector step's interior list through uspmv_spmmv_ap_tiles (_chunks on an object
 * without tile lists) on a side stream while the exchange runs, the boundary list after both.  "pad_split" 1 (the object's default) is
 * honoured: the b values of the padding column's slot are kept before the exchange, and the padding tiles run again after the boundary
 * tiles iff for ANY column the kept or the delivered value is not finite or their signs differ (one re-run per step in
 * uspmv_dist_pad_info).  Every arrangement gives the same bits: column v of Y is what uspmv_dist_spmv gives for column v of X.
 * uspmv_dist_spmmv_info counts these steps.  uspmv_dist_spmmv itself, "block_plan", "fused_step" and "autotune_all" stay refused on
 * an ap object. */
int uspmv_dist_spmmv_ap(uspmv_dist_t *d, void *d_X, void *d_Y, int b, int layout, int mode, int comm_halos, void *stream);
/* ... and for an object of a kind with an fp16 part (uspmv_dist_create_ap_hp_from_coo): the same step with the same arguments and forms,
 * X and Y in the object's vector type (float for ap[sp_hp], else double), over uspmv_spmmv_ap_hp and its list forms
 * (uspmv_spmmv_ap_hp_tiles / _chunks).  Column-wise X is staged at every padded_vec_size (see uspmv_spmmv_ap_hp_tiles).  The padding
 * guard keeps and compares values of the vector type, under the same rule.  Column v of Y is what uspmv_dist_spmv gives for column v
 * of X, in every arrangement.  A one-precision object and an ap[dp_sp] object are refused with USPMV_ERR_UNSUPPORTED and the name of
 * their own entry point; "block_plan", "fused_step" and "autotune_all" stay refused on these objects. */
int uspmv_dist_spmmv_ap_hp(uspmv_dist_t *d, void *d_X, void *d_Y, int b, int layout, int mode, int comm_halos, void *stream);
/* Padding tiles of the single-vector step (tile lists, "pad_split" 1; an option, off by default -- see DESIGN 6.4 for the A/B).  The reference pads chunks with (value +0, column 0);
 * on every rank but the first, column 0 is a halo column (code/mpi_funcs.hpp:279-306), so most tiles of a rank touch the halo only
 * through fma(+0, x[pad_col], acc).  They run with the interior tiles, before the exchange has delivered x[pad_col]: for finite
 * operands of one sign the product is the same signed zero and y comes out bit for bit as with the delivered value; a guard kernel
 * compares the slot's value before and after the exchange and re-runs those tiles after the boundary tiles otherwise.
 * meta[4] = padding tiles, boundary tiles with real halo references, the padding column's local index (-1: none), re-runs so far */
int uspmv_dist_pad_info(const uspmv_dist_t *d, int64_t meta[4]);
/* meta[6] = block-vector steps taken in two parts, in one part, block width of the plan built through "block_plan" (0 = none),
 * tiles of that plan, its boundary tiles, 1 when the handle can run two-part steps at all */
int uspmv_dist_spmmv_info(const uspmv_dist_t *d, int64_t meta[6]);
/* MPI_Barrier / MPI_Allreduce(MAX) / MPI_Allgather twins on the object's communicator (bench loop, code/main.cpp:461-474) */
int uspmv_dist_barrier(uspmv_dist_t *d, void *stream);
int uspmv_dist_allreduce_max(uspmv_dist_t *d, double *value, void *stream);
int uspmv_dist_allgather_i64(uspmv_dist_t *d, int64_t value, int64_t *all /* comm_size (loopback: P) */, void *stream);
void uspmv_dist_free(uspmv_dist_t *d);

/* ------------------------------------------------------------------ measurement helpers   */
/* Device STREAM kernels (copy: a=b, triad: a=b+s*c, read: sum-reduce b) used as the roofline
 * denominator measured in the same run.  n = number of doubles. */
int uspmv_stream_copy(double *d_a, const double *d_b, int64_t n, void *stream);
int uspmv_stream_triad(double *d_a, const double *d_b, const double *d_c, double s, int64_t n, void *stream);
int uspmv_stream_read(const double *d_b, int64_t n, double *d_partial, void *stream);
/* Second yardstick next to the streams: the x traffic of the tile-local-column SpMV without its matrix stream.  ceil(n / rows) workgroups,
 * mapped to the XCDs like the kernel's tiles ("xcd_remap"), each read the nine runs of x lines a `rows`-row tile of a 27-point stencil
 * with the given plane / line strides touches (16-byte loads).  d_partial: 4 * ceil(n / rows) doubles.  *bytes = bytes gathered. */
int uspmv_stream_gather_lines(const double *d_x, int64_t n, int64_t plane, int64_t line, int rows, double *d_partial, void *stream, int64_t *bytes);
/* Time `reps` back-to-back launches of one entry point with HIP events on `stream`;
 * what: 0 spmv(A,x,y) 1 stream_copy 2 stream_triad 3 stream_read 4 spmv_ap(A,B,x,y)
 *       5 spmmv(A,X,Y,b,ld,layout) 6 stream_gather_lines(x, n, plane = ld, line = b, rows = layout) 7 spmmv_ap(A,B,X,Y,b,ld,layout).  Two untimed launches precede the timed ones; returns the average milliseconds per launch.
 * For the STREAM kinds d_x is the source (n doubles; 2n for the triad: b = d_x, c = d_x + n) and d_y
 * the destination (n doubles; 8192 for the read kernel's partial sums). */
int uspmv_time_launches(int what, int reps, const uspmv_dmat_t *A, const uspmv_dmat_t *B, const void *d_x,
                        void *d_y, int64_t n, int b, int64_t ld, int layout, void *stream, double *avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* USPMV_H */
