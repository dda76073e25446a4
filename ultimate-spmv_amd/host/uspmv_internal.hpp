// Internal definitions shared by the host data layer and the HIP C-ABI layer of libuspmv.so.
#pragma once
#include <sys/mman.h>
#include <algorithm>
#include <cstdint>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <memory>
#include <utility>
#include <vector>

#include "uspmv.h"

// COO matrix, 0-based, entries stable-sorted by row when produced by uspmv_read_mtx
// (role of MtxData<double,int>, reference code/classes_structs.hpp:1169-1238).
// allocator whose resize() leaves new elements uninitialised: the three arrays of a large COO are first touched by the threads that fill
// them (a value-initialising resize is a serial 3 GB memset for 2e8 entries, host/mtx_io.cpp)
template <class T> struct uspmv_noinit_alloc : std::allocator<T> {
    template <class U> struct rebind { using other = uspmv_noinit_alloc<U>; };
    uspmv_noinit_alloc() = default;
    template <class U> uspmv_noinit_alloc(const uspmv_noinit_alloc<U> &) {}
    template <class U, class... A> void construct(U *p, A &&...a) {
        if constexpr (sizeof...(A) == 0) ::new ((void *)p) U;
        else ::new ((void *)p) U(std::forward<A>(a)...);
    }
};
using uspmv_ivec = std::vector<int32_t, uspmv_noinit_alloc<int32_t>>;
using uspmv_dvec = std::vector<double, uspmv_noinit_alloc<double>>;

struct uspmv_coo {
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    uspmv_ivec I, J;
    uspmv_dvec values;
};

// SELL-C-sigma matrix on the host (role of ScsData<VT,int>, code/classes_structs.hpp:1313-1339).
// Element (row-in-chunk i, slot j) of chunk c lives at chunk_ptrs[c] + j*C + i (column-major
// inside a chunk); padding entries have value 0 and column 0.
struct uspmv_scs {
    int64_t C = 0, sigma = 0, n_rows = 0, n_cols = 0, n_rows_padded = 0, n_chunks = 0, n_elements = 0, nnz = 0;
    int dtype = USPMV_F64;
    std::vector<int32_t> chunk_ptrs, chunk_lengths, col_idxs, old_to_new_idx, new_to_old_idx;
    std::vector<double> values_f64;
    std::vector<float> values_f32;
    std::vector<uint16_t> values_f16;     // USPMV_F16: binary16 bits
    const void *values_ptr() const {
        return dtype == USPMV_F64 ? (const void *)values_f64.data()
             : dtype == USPMV_F32 ? (const void *)values_f32.data() : (const void *)values_f16.data();
    }
};
// bytes per value of a dtype
inline size_t uspmv_dtype_bytes(int dtype) { return dtype == USPMV_F64 ? 8 : dtype == USPMV_F32 ? 4 : 2; }
// binary16 <-> double (host/scs_convert.cpp): one round-to-nearest-even step from the double, bit-equal to numpy's float64 -> float16
uint16_t uspmv_f64_to_f16(double v);
double uspmv_f16_to_f64(uint16_t h);

// Per-rank halo description (role of ContextData, code/classes_structs.hpp:156-184).
struct uspmv_halo {
    int P = 0, rank = 0;
    int64_t n_local = 0, n_halo = 0;
    std::vector<int32_t> recv_counts_cumsum;  // P+1, assembled as code/mpi_funcs.hpp:403-414
    std::vector<int32_t> recv_counts;         // P
    std::vector<int32_t> recv_idxs;           // grouped by owner ascending, owner-local row ids
};

// Exchange plan of one rank (host/comm_plan.cpp): what to send to whom, derived from the peers' halo descriptions
// (role of comm_send_idxs / send_counts_cumsum, code/mpi_funcs.hpp:117-232)
struct uspmv_comm_plan {
    int P = 0, rank = 0;
    int64_t n_local = 0, n_send = 0;
    std::vector<int64_t> send_off, recv_off;   // P+1, elements
    std::vector<int32_t> send_idxs;            // this rank's local rows (original order), grouped by receiver
};

// resize() of a large vector of trivially constructible elements without the serial 4-KiB page faults of its zero fill: the storage is
// reserved first and the kernel asked for huge pages on it (a 4 GB copy of config 3's entries: 16 s -> under a second in the build container)
template <typename V>
inline void uspmv_resize_huge(V &v, size_t n) {
    v.reserve(n);
    const uintptr_t a = ((uintptr_t)v.data() + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1), e = ((uintptr_t)(v.data() + v.capacity())) & ~(uintptr_t)((2u << 20) - 1);
    if (n * sizeof(typename V::value_type) >= (64u << 20) && e > a) {
        (void)madvise((void *)a, e - a, MADV_HUGEPAGE);
        volatile char *b = (volatile char *)a;               // first touch by all threads (the storage is raw until resize() fills it)
        const int64_t pages = (int64_t)((e - a) >> 12);
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < pages; ++k) b[(size_t)k << 12] = 0;
    }
    v.resize(n);
}

// Tile-local-column plan (host copy), see host/tlc_plan.cpp
struct uspmv_tlc_plan {
    bool valid = false;
    int chunks_per_tile = 0, max_lines_used = 0, tile_rows = 256, line_shift = 4;
    int64_t n_tiles = 0, n_staged_tiles = 0, x_len_min = 0;
    std::vector<int32_t> tile_line_ptr;   // n_tiles+1
    std::vector<int32_t> tile_lines;      // line ids (col >> 4), sorted per tile; empty tile list = gather path
    std::vector<uint32_t> c16_ptrs;       // n_chunks+1, offsets into col16
    std::vector<uint16_t> col16;          // [chunk][slot/4][row][slot%4]
    std::vector<uint32_t> c16_ptrs_b;     // same for the optional second struct (sp part of an ap pair)
    std::vector<uint16_t> col16_b;
    std::vector<uint32_t> c16_ptrs_c;     // ... and the optional third (the hp part of ap[dp_sp_hp])
    std::vector<uint16_t> col16_c;
};
int uspmv_build_tlc_plan(const uspmv_scs *s, const uspmv_scs *s2, int max_lines, int tile_rows, uspmv_tlc_plan *plan, int line_shift = 4,
                         const uspmv_scs *s3 = nullptr);

// Additive chunk records (host copy), see host/tlc_plan.cpp: a third, derived index stream of a line plan.  The x window of a tile is laid
// out in LDS in PRE-SORT column order (a few intervals of columns of the numbering the sigma sort started from), where
// the entries of most chunks sit at (position of the lane's row) + (one offset per slot).
struct uspmv_additive_plan {
    bool valid = false;
    bool cols_permuted = false;            // the column map that was taken: the struct's own permutation, or (false) the identity
    int tile_rows = 256, max_elems = 0;    // max_elems: LDS elements of the fullest tile
    int64_t n_tiles = 0, n_add_tiles = 0;  // tiles of the line plan / tiles that carry intervals
    int64_t n_chunks = 0, n_additive = 0;  // chunks of the tiles with intervals / of these, the additive ones
    int64_t rec_bytes = 0;                 // of `rec` (what the kernel streams instead of the local indices of those tiles)
    bool own_tiles = false;                // tile_rows other than the line plan's: every (non-empty) tile carries intervals
    int w_log = 4;                         // W = 1 << w_log, 16 ... 32768: the column map stays inside aligned blocks of W columns
    // per tile with intervals its x line list, every entry naming the interval its elements go to: line | interval << 27, by line, then by
    // interval; a line whose referenced elements fall into k intervals is listed k times
    std::vector<int32_t> line_ptr, lines;
    int64_t n_lines_again = 0, n_entries_again = 0;   // lines listed more than once / entries that list a line again
    std::vector<int32_t> iv_ptr;           // n_tiles + 1: the tile's intervals (none: the tile keeps its line list)
    std::vector<int32_t> iv;               // per interval four ints: first pre-sort column, length, first LDS element, 0
    std::vector<uint32_t> rec_ptrs;        // per chunk: (offset into rec in units of 16 bytes) << 1 | additive
    // additive chunk: R[C] (pre-sort position of the lane's row above the chunk's lowest), then S[slots rounded up to 8] (LDS position of the slot's
    // entry in the lowest row): the entry of (lane i, slot j) reads LDS element R[i] + S[j].  Any other chunk: the LDS position of every entry,
    // [batch of eight slots][row][slot % 8] -- a lane reads 16 bytes per batch in both kinds, so the two chunks of a wave share one loop.
    std::vector<uint16_t> rec;
    std::vector<int32_t> o2n;              // n_cols: pre-sort column -> column of x (the identity when !cols_permuted)
    std::vector<uint16_t> map16;           // what the kernel stages through: the pre-sort column of x[q] is (q & ~(W - 1)) + map16[q]; padded to whole lines
};
// lp: the line plan of s (16-element lines); budget: most LDS elements a tile may take; new_to_old: the permutation of s's rows when s does not
// carry it itself (the internal re-chunking of a narrow struct keeps the caller's row order); tile_rows: rows per tile the records are wanted
// for (0: the line plan's), kept when every tile then gets intervals
int uspmv_build_additive_plan(const uspmv_scs *s, const uspmv_tlc_plan *lp, int budget, uspmv_additive_plan *plan,
                              const std::vector<int32_t> *new_to_old = nullptr, int tile_rows = 0);   // host/tlc_plan.cpp
// the column of every entry (padding included) of the chunks whose tiles carry intervals, read back from the records alone; -1 elsewhere
void uspmv_additive_plan_decode(const uspmv_scs *s, const uspmv_additive_plan *plan, int32_t *cols);                 // host/tlc_plan.cpp

// Column-window sweep plan (host copy), see host/sweep_plan.cpp
struct uspmv_sweep_plan {
    bool valid = false;
    int tile_rows = 1024, wlog = 13;
    int64_t n_tiles = 0, n_sweep_tiles = 0, x_len_min = 0;
    std::vector<int32_t> tile_ids, t_smin, t_S;   // per sweep tile: tile number, first window, number of windows
    std::vector<uint64_t> t_cnt_off;              // per sweep tile: offset of its S*tile_rows count bytes
    // one record per struct of the plan, in the order the builder was given them: [one struct], [dp, sp] of ap[dp_sp], or the parts of a
    // split with an fp16 part, [hi, hp] or [hi, mid, hp].  Records from n_parts on stay empty.
    struct part_t {
        int dtype = USPMV_F64;
        std::vector<uint32_t> wave_off;           // per (sweep tile, wave): first element of the wave's compacted stream
        std::vector<uint8_t> cnt;                 // [tile][window][row]: entries of the row in the window
        std::vector<uint16_t> idx;                // column - window start
        std::vector<int32_t> pad_col;             // per (sweep tile, row): column of the stripped trailing padding, -1 = none
        // the stream's values as uspmv_scs stores them: only the vector of `dtype` is filled
        std::vector<double> vals_f64;
        std::vector<float> vals_f32;
        std::vector<uint16_t> vals_f16;           // binary16 bits
        const void *vals() const {
            return dtype == USPMV_F64 ? (const void *)vals_f64.data()
                 : dtype == USPMV_F32 ? (const void *)vals_f32.data() : (const void *)vals_f16.data();
        }
    };
    int n_parts = 1;
    part_t part[3];
    std::vector<int32_t> rest_chunks;             // chunks of the tiles that do not sweep (gather kernel)
};
// Two rules that the host builders below and the device builder (csrc/sweep_planner.hip: sweep_plan_install_device) share; the tests
// hold host- and device-built plans to the same bits.
// Rows per tile: a value outside the builder's set becomes its default -- 256 | 512 | 1024 | 2048 | 4096, else 1024, for the plan over
// vectors; 1024 | 2048 | 4096, else 2048, for the plan over block vectors (blocks).
inline int uspmv_sweep_tile_rows(int tile_rows, bool blocks) {
    const bool in_set = tile_rows == 1024 || tile_rows == 2048 || tile_rows == 4096 || (!blocks && (tile_rows == 256 || tile_rows == 512));
    return in_set ? tile_rows : blocks ? 2048 : 1024;
}
// Does this tile sweep: each of its n_windows windows of 2^wlog units (x elements, or X rows) of unit_bytes is copied once per tile, which
// may cost at most max_stage_bytes_per_nnz for each of the tile's nnz entries; and a tile has at most 4 096 windows.
inline bool uspmv_sweep_tile_ok(int64_t n_windows, int wlog, size_t unit_bytes, int64_t nnz, double max_stage_bytes_per_nnz) {
    return (double)n_windows * (double)((int64_t)1 << wlog) * (double)unit_bytes <= max_stage_bytes_per_nnz * (double)std::max<int64_t>(nnz, 1) &&
           n_windows <= 4096;
}
// parts: one to three structs with one row layout (one struct; ap[dp_sp]: F64, F32; with an fp16 part: F64 | F32, [F32,] F16)
int uspmv_build_sweep_plan(const uspmv_scs *const parts[], int n_parts, int wlog, int tile_rows, double max_stage_bytes_per_nnz,
                           uspmv_sweep_plan *plan);   // host/sweep_plan.cpp

// Block-vector column-window sweep plan (host copy; host/sweep_plan.cpp, csrc/spmmv_sweep.hip): like uspmv_sweep_plan, but the windows
// are windows of X ROWS (2^wlog rows of block_vec_size values each) and a tile lists only the windows its rows TOUCH -- the rows of a
// 3-D grid matrix reach into three plane-sized index ranges far apart, and staging the gaps between them would cost more than it saves
struct uspmv_block_sweep_plan {
    bool valid = false;
    int tile_rows = 2048, wlog = 9;
    int64_t n_tiles = 0, n_sweep_tiles = 0, x_rows_min = 0, windows_staged = 0;
    std::vector<int32_t> tile_ids;       // per sweep tile: tile number
    std::vector<int32_t> t_win_ptr;      // n_sweep_tiles + 1: the tile's windows in `wins`
    std::vector<int32_t> wins;           // window ids, ascending per tile
    std::vector<uint64_t> t_cnt_off;     // per sweep tile: offset of its (windows x tile_rows) count bytes
    std::vector<uint32_t> wave_off;      // per (sweep tile, wave): first element of the wave's compacted stream
    std::vector<uint8_t> cnt;            // [tile][window of the tile][row]: entries of the row in the window
    std::vector<uint16_t> idx;           // X row - first row of the window
    std::vector<double> vals_f64;
    std::vector<float> vals_f32;
    std::vector<int32_t> pad_col;        // per (sweep tile, row): column of the stripped trailing padding, -1 = none
    std::vector<int32_t> rest_chunks;    // chunks of the tiles that do not sweep
};
int uspmv_build_block_sweep_plan(const uspmv_scs *s, int wlog, int tile_rows, int row_bytes, double max_stage_bytes_per_nnz,
                                 uspmv_block_sweep_plan *plan);   // host/sweep_plan.cpp

// Phased block plan (host copy), see host/tlc_plan.cpp
struct uspmv_phased_plan {
    bool valid = false;
    int cap_rows = 256, ngp = 8, max_rows_used = 0, line_shift = 0;   // line_shift > 0: the lists hold lines of 2^line_shift X rows
    int64_t n_tiles = 0, n_phases = 0;
    std::vector<int32_t> ph_ptr;        // n_tiles+1: phases of a tile
    std::vector<int32_t> ph_g0;         // n_phases: first group (of four slots) of the phase; it ends where the tile's next phase starts
    std::vector<int32_t> ph_list_ptr;   // n_phases+1: the phase's X-row list in xrows
    std::vector<int32_t> xrows;         // sorted per phase
    std::vector<uint32_t> c16_ptrs;     // n_chunks+1
    std::vector<uint16_t> col16;        // [chunk][slot/4][row][slot%4], index into the list of the slot's phase
};
int uspmv_build_phased_plan(const uspmv_scs *s, int cap_rows, int ngp, uspmv_phased_plan *plan, int line_shift = 0, int phase_cost = 0);   // host/tlc_plan.cpp

int uspmv_scs_rechunk32(const uspmv_scs *s, uspmv_scs *out);   // host/tlc_plan.cpp
// per chunk 0 = no halo column, 1 = halo only through +0.0 padding entries on the one column *pad_col, 2 = other halo references (host/halo_plan.cpp)
int uspmv_scs_classify_chunks(const uspmv_scs *s, int64_t n_local, std::vector<uint8_t> *cls, int32_t *pad_col);
// private copy of the entries with the rows of equal-length chunks of a sigma window back in original order;
// returns 1 when anything moved, 0 when the copy is identical (row_map = identity)
int uspmv_scs_reorder_ties(const uspmv_scs *s, uspmv_scs *r, std::vector<int32_t> *row_map);   // host/tlc_plan.cpp
// mode 1 = the above; mode 2 = rows re-dealt to the 64-row tiles as breadth-first balls of the matrix graph (per chunk-length
// class, so the chunk structure is still untouched); mode -1 = copy under the caller's row_map
int uspmv_scs_reorder_rows(const uspmv_scs *s, int mode, uspmv_scs *r, std::vector<int32_t> *row_map, int tile_rows = 64, int64_t seg_rows = 65536);   // host/tlc_plan.cpp
int uspmv_scs_reorder_bricks(const uspmv_scs *s, int64_t stride, int64_t lines, uspmv_scs *r, std::vector<int32_t> *row_map);   // host/tlc_plan.cpp (measurement aid)

int uspmv_scs_layout(const uspmv_coo *m, int64_t C, int64_t sigma, int dtype, const int32_t *fixed_permutation,
                     uspmv_scs *s, std::vector<int64_t> *row_start, const char *who);   // host/scs_convert.cpp

namespace uspmv {
int fail(int status, const char *fmt, ...);  // records the thread-local error text, returns status
// false for the layout-only structs uspmv_convert_to_scs_device hands back (entries live on the device only)
inline bool scs_has_entries(const uspmv_scs *s) { return (int64_t)s->col_idxs.size() == s->n_elements; }
// the halo description of a rank from its per-owner lists of owner-local row ids in first-seen order (host/halo_plan.cpp)
uspmv_halo *halo_from_lists(int P, int rank, int64_t n_local, const std::vector<std::vector<int32_t>> &lists);
// host side of uspmv_dist_check (host/dist_check.cpp)
double check_x(int64_t global_col);
int64_t check_col(int64_t j, const int32_t *wsa, int P, int rank, bool loopback);
int dist_reference_rows(const uspmv_coo *local, const int32_t *wsa, int P, int rank, bool loopback, int dtype, void *y_ref);
int dist_reference_rows_ap(const uspmv_coo *local, const int32_t *wsa, int P, int rank, bool loopback, double threshold_1, double *y_ref);
int dist_reference_rows_ap_hp(const uspmv_coo *local, const int32_t *wsa, int P, int rank, bool loopback, int kind, double threshold_1,
                              double threshold_2, void *y_ref);
}
