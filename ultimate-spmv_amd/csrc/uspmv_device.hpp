// Shared declarations of the device half of libuspmv: the matrix handle, the tuning knobs, the
// device helpers every kernel file uses and the launch entry points the C ABI calls (uspmv_api.hip: handles, tuning, SpMV / SpMMV / ap
// entry points; tlc_planner.hip, block_planner.hip, sweep_planner.hip: the plans; stream_kernels.hip: the STREAM calibrators).
// Kernels live in spmv_kernels.hip, spmmv_kernels.hip, ap_kernels.hip, ap_spmmv_kernels.hip (ap[dp_sp] on block vectors: dispatch and
// the row-major gather kernel) and ap_hp_spmmv_kernels.hip (the lane-per-row and staged block kernels of every ap kind).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../host/uspmv_internal.hpp"

// An owned device allocation (host code only): move-only, freed by its destructor or reset().  Every helper frees what the buffer
// held, allocates at least MIN_BYTES and returns the HIP status; on failure the buffer is empty or holds the new, unfilled allocation.
template <typename T>
class DeviceBuf {
  public:
    static constexpr size_t MIN_BYTES = 16;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    DeviceBuf(DeviceBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~DeviceBuf() { reset(); }
    void reset() {
        if (p_) (void)hipFree((void *)p_);
        p_ = nullptr;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    template <typename U>
    explicit operator U *() const { return (U *)p_; }   // the launchers' casts: (const VT *)A->pb.values, (const int *)A->ps.wg_ptr, ...
    hipError_t alloc(size_t bytes) {
        reset();
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max(bytes, MIN_BYTES));
        p_ = (T *)q;
        return e;
    }
    hipError_t zeros(size_t bytes) {
        hipError_t e = alloc(bytes);
        if (e == hipSuccess && bytes) e = hipMemset((void *)p_, 0, bytes);
        return e;
    }
    hipError_t upload(const void *host, size_t bytes) {
        hipError_t e = alloc(bytes);
        if (e == hipSuccess && bytes) e = hipMemcpy((void *)p_, host, bytes, hipMemcpyHostToDevice);
        return e;
    }

  private:
    T *p_ = nullptr;
};

// An owned pinned host allocation (hipHostMalloc), shaped like DeviceBuf: move-only, freed by its destructor or reset().
class PinnedBuf {
  public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
    }
    void *get() const { return p_; }
    hipError_t alloc(size_t bytes) {
        reset();
        void *q = nullptr;
        const hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
        p_ = q;
        return e;
    }

  private:
    void *p_ = nullptr;
};

// COO arrays in HBM, owned by the object (uspmv_dcoo_t of the C ABI): one compacted part of uspmv_partition_precisions_device
// (convert_kernels.hip), or a block of uspmv_gen_stencil27_device (gen_kernels.hip).
struct uspmv_dcoo {
    DeviceBuf<int32_t> I, J;
    DeviceBuf<double> V;
    int64_t nnz = 0;
};

namespace uspmv_dev {
// The shapes of a phased block plan the SpMMV kernels are compiled for: what block_planner.hip plans within, what the device builder
// (block_plan_kernels.hip) is asked for and what spmmv_phased.hip / spmmv_stream.hip dispatch on.
constexpr int PHASE_ROWS_IDX8 = 256;       // most list entries of a phase that one-byte phase-local indices address
constexpr int PHASE_GROUPS = 8;            // most groups of four slots per phase
constexpr int PHASE_PIECES_SMALL = 4, PHASE_PIECES_MAX = 8;   // LDS pieces of 64 X rows the phased kernel exists for
inline int phase_pieces(int max_rows) { return (max_rows * 4 + 255) / 256; }

// The phase lists of a phased block plan -- what uspmv_dmat's phased, line and unscrambled plans each carry one of.  Tile t runs the
// phases ph_ptr[t] .. ph_ptr[t + 1]; phase p starts at group g0[p] of its chunks and lists list[list_ptr[p] .. list_ptr[p + 1]): X rows,
// or lines of X rows.  idx: per entry of the matrix the position in its phase's list, laid out like the plan's values.
struct PhaseLists {
    DeviceBuf<int32_t> ph_ptr, g0, list_ptr, list;
    DeviceBuf<void> idx;
    int idx_bytes = 2;                     // of an element of idx: 1 (no phase lists more than PHASE_ROWS_IDX8 entries) or 2
    int max_rows = 0;                      // X rows of the fullest phase
    int64_t n_phases = 0, rows_staged = 0;
    bool idx8() const { return idx_bytes == 1; }
};
}  // namespace uspmv_dev

// The device matrix.  Every plan family is one member struct holding its device arrays and metadata; `on` says the plan is installed,
// and assigning {} to the member releases the plan and resets every field of it.
struct uspmv_dmat {
    using PhaseLists = uspmv_dev::PhaseLists;
    uspmv_dmat() = default;
    uspmv_dmat(const uspmv_dmat &) = delete;
    uspmv_dmat &operator=(const uspmv_dmat &) = delete;

    int64_t C = 0, n_chunks = 0, n_elements = 0;
    int dtype = USPMV_F64;
    // the SELL-C-sigma arrays: views of `own` (uspmv_dmat_upload and the device conversions) or of the caller's arrays (uspmv_dmat_wrap)
    const int32_t *chunk_ptrs = nullptr, *chunk_lengths = nullptr, *col_idxs = nullptr;
    const void *values = nullptr;
    struct {
        DeviceBuf<int32_t> chunk_ptrs, chunk_lengths, col_idxs;
        DeviceBuf<void> values;
    } own;
    // allocates `own` for the handle's n_chunks / n_elements / dtype and points the views at it
    hipError_t own_arrays() {
        const size_t ne = (size_t)std::max<int64_t>(n_elements, 1);
        hipError_t e = own.chunk_ptrs.alloc(4 * ((size_t)n_chunks + 1));
        if (e == hipSuccess) e = own.chunk_lengths.alloc(4 * (size_t)std::max<int64_t>(n_chunks, 1));
        if (e == hipSuccess) e = own.col_idxs.alloc(4 * ne);
        if (e == hipSuccess) e = own.values.alloc(uspmv_dtype_bytes(dtype) * ne);
        chunk_ptrs = own.chunk_ptrs; chunk_lengths = own.chunk_lengths; col_idxs = own.col_idxs; values = own.values;
        return e;
    }
    bool crs = false;
    long n_store = 0;              // rows of y the kernels may write (= n_chunks*C unless re-chunked)
    uspmv_dmat *alt = nullptr;     // internal C = 32 re-chunking of a C in {1,2,4,8,16} struct (same row order)
    // scratch for the internal row-major copies of column-major block vectors (uspmv_spmmv); grown
    // on demand, released with the handle.  Not thread-safe per handle, like the reference's kernel object.
    mutable DeviceBuf<void> ws;
    mutable size_t ws_bytes = 0;
    // uspmv_spmmv_x_prepared: the workspace holds the re-laid-out copy of THIS column-major X (b, ld; form 1 plain / 2 sigma permutation undone)
    mutable const void *xprep_ptr = nullptr;
    mutable int xprep_b = 0, xprep_form = 0;
    mutable long xprep_ld = 0;
    // uspmv_spmmv_last_path: what the last uspmv_spmmv on this handle launched, written on the host at the launch sites themselves.
    // last_kernel: 0 nothing yet, 1 scs_spmmv_rows, 2 _xpose, 3 _rowmajor, 4 _tlc, 5 _rowmajor on the block plan's re-ordered copy, 6 _quad,
    // 8 the phased kernel, 9 scs_spmmv_sweep, 10 the streamed phased kernel (the "spmmv_variant" numbers where there is one).
    // last_xpass: 0 X as passed, 1 re-laid out in this call, 2 the prepared workspace reused, 3 a re-layout that undid the sigma permutation.
    mutable int last_kernel = 0, last_xpass = 0;
    // uspmv_spmv_axpby: two doubles per workgroup of the launches that serve one call, summed by its finalize kernel;
    // axpby_tmp: A x of an in-place call on path 2 (y is z there, so the SpMV cannot write it).  Like ws: grown on demand or by
    // uspmv_spmv_axpby_reserve, released with the handle, not thread-safe per handle.
    mutable DeviceBuf<double> axpby_part;
    mutable size_t axpby_slots = 0;
    mutable DeviceBuf<void> axpby_tmp;
    mutable size_t axpby_tmp_bytes = 0;
    // SpMMV in two parts (the halo overlap of uspmv_dist_spmmv, csrc/uspmv_dist_api.hip): chunk-length arrays in which the chunks of the
    // OTHER part carry USPMV_SKIP_LEN -- a kernel that meets it leaves those rows of Y alone.  [order][part - 1]: order 0 = the caller's
    // row order (gather kernels), order 1 = the phased plan's tie-re-ordered rows (scs_spmmv_quadph), classified per 64-row plan tile.
    // `part` selects around ONE launch: 0 the whole matrix, 1 interior, 2 boundary; column-major callers: part 1 re-lays out X rows
    // [0, part_split) into the workspace, part 2 the rest (the halo rows, after the exchange).
    DeviceBuf<int32_t> part_len[2][2];
    int part = 0;
    long part_split = 0;
    // tile-local-column plan (host/tlc_plan.cpp)
    struct TlcPlan {
        bool on = false;
        bool elem = false;   // the plan lists single x ELEMENTS instead of 16-element lines (max_lines counts elements): rows whose columns are scattered
                             // (a numbering that is only locally coherent) -- uspmv_dmat_optimize falls to it when the line plan stages too few tiles
        int max_lines = 0, tile_rows = 256;
        int64_t x_len = 0, n_tiles = 0, staged = 0;
        uint64_t plan_id = 0;   // structs planned together (ap pair) carry the same non-zero id
        DeviceBuf<int32_t> line_ptr, lines;
        DeviceBuf<uint32_t> c16_ptrs;
        DeviceBuf<uint16_t> col16;
        // ... and the same local indices packed to 12 bits (plans of at most 256 lines per tile: 9.5 instead of 10 bytes per non-zero of the stream):
        // per chunk, at c12_ptrs[c] dwords: for every PAIR of slot groups [row][3 dwords] (96 bits per row = 8 indices, one 12-byte load per
        // lane; three planes of C dwords measured 3 % slower), then for an odd last group one plane of C dwords + one of C ushorts (48 bits per
        // row).  What scs_spmv_tlc reads when present.
        DeviceBuf<uint32_t> c12_ptrs, col12;
        // element plan over rows DEALT TO THE TILES BY THE MATRIX GRAPH (uspmv_scs_reorder_rows mode 4, as for the block plan): a private copy of the values in that
        // order and row_map[plan row] = row of y.  Null when the caller's row order is kept.
        DeviceBuf<void> values;
        DeviceBuf<int32_t> row_map, cols;     // (cols: the column indices in that order, for the few tiles that do not stage)
        // additive chunk records (uspmv_additive_plan, host/tlc_plan.cpp; installed by tlc_planner.hip under "tlc_additive"): what the
        // single-struct SpMV kernel streams instead of col12 / col16 in the tiles that carry intervals.  add_ptrs null: none.
        DeviceBuf<int32_t> add_iv_ptr, add_iv;
        DeviceBuf<uint32_t> add_ptrs;
        DeviceBuf<uint16_t> add_rec, add_map16;       // add_map16: 2-byte block-local column map (blocks of 1 << add_w_log columns)
        DeviceBuf<int32_t> add_line_ptr, add_lines;   // the tagged line lists (line | interval << 27) of the records' tiles (add_tile_rows, add_n_tiles)
        int add_max_elems = 0, add_tile_rows = 0;     // LDS elements of the fullest tile; rows per tile of the records
        int add_w_log = 4;
        bool add_own_tiles = false;                   // the records' tiles are not the line plan's: every tile carries intervals
        int64_t add_n_tiles = 0;
        int64_t add_chunks = 0, add_additive = 0;   // chunks of the tiles with intervals / the additive ones among them
    } tlc;
    // block (SpMMV) plan: 64-row tiles, per tile the list of X rows it touches (uspmv_dmat_optimize_block)
    struct BlockPlan {
        bool on = false;
        int max_rows = 0, tile_rows = 64;
        int64_t n_tiles = 0, staged = 0;
        DeviceBuf<int32_t> line_ptr, xrows;
        DeviceBuf<uint32_t> c16_ptrs;
        DeviceBuf<uint16_t> col16;
        // the plan's private copy of the entries with ties of the sigma sort back in original-row order
        // (uspmv_scs_reorder_ties): values (+ 32-bit columns when some tile keeps the gather path) and
        // row_map[plan row] = row of y.  All null when the caller's order is kept.
        DeviceBuf<void> values;
        DeviceBuf<int32_t> cols, row_map;
    } bt;
    // phased block plan (uspmv_build_phased_plan; 64-byte X rows): per tile a run of phases, each with its own X-row list
    struct PhasedPlan {
        bool on = false;
        int cap_rows = 0, ngp = 0;
        int64_t n_tiles = 0;
        PhaseLists lists;                   // X rows
        DeviceBuf<void> values;             // the entries again, GROUP-major like the indices ([chunk][group of four slots][row][slot % 4])
        DeviceBuf<uint32_t> c16_ptrs;
        bool device_built = false;          // the plan's index part was built by csrc/block_plan_kernels.hip
    } pb;
    // the phased plan once more as a flat schedule of 32-byte phase descriptors for persistent workgroups (spmmv_stream.hip; "spmmv_stream")
    struct StreamSchedule {
        int grid = 0;
        bool per_tile = false;              // the schedule has one tile per workgroup ("spmmv_stream" 99)
        int64_t n_desc = 0;
        DeviceBuf<int32_t> wg_ptr;
        DeviceBuf<void> desc;
    } ps;
    // the same plan once more with LINE lists (128 bytes of one column: 16 doubles / 32 floats) for column-major block vectors:
    // shares pb.values / pb.c16_ptrs / the row map; one-byte local indices (line << shift | row in line)
    struct LinePlan {
        bool on = false;
        int shift = 0;
        PhaseLists lists;                   // X lines
    } pl;
    // ... and once more for column-major block vectors behind the re-layout pass, with the X rows numbered in the ORIGINAL row order:
    // the pass that turns the caller's column-major X into the row-major workspace also undoes the sigma permutation
    // (Xr[r] = X[old_to_new[r]]), so a tile's X rows form long runs again instead of ~30 fragments per phase and a 128-byte line of the
    // workspace holds two rows the tile needs instead of 1.1 (shares pb.values / pb.c16_ptrs / the row map)
    struct UnscrambledPlan {
        bool on = false;
        int64_t n_perm = 0;
        PhaseLists lists;                   // X rows in original numbering; one-byte local indices
        DeviceBuf<int32_t> perm;
    } pu;
    // block-vector column-window sweep plan (uspmv_build_block_sweep_plan, csrc/spmmv_sweep.hip): 64-byte X rows, windows of 2^wlog X rows,
    // per tile the list of windows its rows touch
    struct BlockSweepPlan {
        bool on = false;
        int tile_rows = 2048, wlog = 9, b = 0;
        int64_t n_tiles = 0, all_tiles = 0, x_rows = 0, windows = 0;
        DeviceBuf<int32_t> tile_ids, win_ptr, wins, pad;
        DeviceBuf<uint64_t> cnt_off;
        DeviceBuf<uint32_t> wave_off;
        DeviceBuf<uint8_t> cnt;
        DeviceBuf<void> vals;
        DeviceBuf<uint16_t> idx;
    } bw;
    // column-window sweep plan (host/sweep_plan.cpp, uspmv_dmat_optimize_sweep[_ap | _ap_hp]): part[k] holds the arrays of the plan's
    // k-th struct, in the order of the split -- [one struct], [dp, sp] of an ap[dp_sp] pair, [hi, hp] or [hi, mid, hp] of a split with an
    // fp16 part.  All live on the first part's handle; the other handles only carry the plan id and the tile counts.
    struct SweepPlan {
        bool on = false;
        int tile_rows = 1024, wlog = 13;
        int64_t n_tiles = 0, all_tiles = 0, x_len = 0, n_rest = 0, cnt_bytes = 0;   // (cnt_bytes: bytes of a part's count array)
        int n_parts = 1;
        uint64_t plan_id = 0;
        DeviceBuf<int32_t> tile_ids, smin, S, rest;
        DeviceBuf<uint64_t> cnt_off;
        struct Part {
            int dtype = USPMV_F64;      // what vals holds: double, float or binary16 bits (part[0]: the handle's dtype)
            int64_t n_vals = 0;         // elements of the compacted stream (without the spare tail)
            DeviceBuf<uint32_t> wave_off;
            DeviceBuf<uint8_t> cnt;
            DeviceBuf<void> vals;
            DeviceBuf<uint16_t> idx;
            DeviceBuf<int32_t> pad;
        } part[3];
    } sw;
};

namespace uspmv_dev {

// What the SpMV planner (csrc/tlc_planner.hip) may do beyond the line plan at the default rows per tile.  Each is on when the option
// AND its tuning key say so: measure -- time 256 / 512 / 1024 rows per tile on large structs ("tlc_measure_tile"); elements -- fall to
// the plan over single x elements ("tlc_elem"); deal_rows -- ... on rows dealt to the tiles by the matrix graph ("tlc_elem_rows"),
// after which tile t no longer covers rows [t * tile_rows, (t + 1) * tile_rows) of the caller's order.
// additive -- the additive chunk records beside the local indices ("tlc_additive"; not for the rank blocks of the distributed object);
// new_to_old: the permutation of the struct's rows where the struct does not carry it (the internal re-chunking of a narrow struct).
struct TlcPlanOpts { bool measure = true, elements = true, deal_rows = true, additive = true; const std::vector<int32_t> *new_to_old = nullptr; };
// The entries below are argument checks around ONE driver, plan_parts: line plan at the kind's rows per tile -> plan over single x
// elements -> column-window sweep -> keep or drop the line plan; *n_tiles / *n_staged describe the line plan unless the element plan
// was taken.  What the kinds differ in is the table POLICY there (rows per tile, keep rule, when elements are allowed), and for the parts
// of a split (ap[dp_sp], the kinds with an fp16 part) `measure` off means: ONE candidate at the rows per tile of one struct (256) in the
// caller's row order, installed whenever it is valid, neither elements nor sweep -- what the distributed object needs of them.  A single
// struct tries the sweep whatever the options say.
// uspmv_dmat_optimize, uspmv_dmat_optimize_ap and uspmv_dmat_optimize_ap_hp (mid / s_mid NULL for the two-part kinds) with the options
// spelled out, from the host structs:
int dmat_optimize(uspmv_dmat *A, const uspmv_scs *s, int max_lines, const TlcPlanOpts &opts, int64_t *n_tiles, int64_t *n_staged);
int dmat_optimize_ap(uspmv_dmat *dp, uspmv_dmat *sp, const uspmv_scs *s_dp, const uspmv_scs *s_sp, int max_lines, const TlcPlanOpts &opts,
                     int64_t *n_tiles, int64_t *n_staged);
int dmat_optimize_ap_hp(uspmv_dmat *hi, uspmv_dmat *mid, uspmv_dmat *hp, const uspmv_scs *s_hi, const uspmv_scs *s_mid, const uspmv_scs *s_hp,
                        int max_lines, const TlcPlanOpts &opts, int64_t *n_tiles, int64_t *n_staged);
// ... and from the handles' own device arrays (no host struct; deal_rows and additive: host only): uspmv_dmat_optimize_device with the
// options spelled out, and the driver with `measure` off and the default line budget on the two or three parts of a split (parts[2]
// NULL: two)
int dmat_optimize_device(uspmv_dmat *A, int max_lines, const TlcPlanOpts &opts, int64_t *n_tiles, int64_t *n_staged);
int dmat_optimize_device_shared(uspmv_dmat *const parts[3], int64_t *n_tiles, int64_t *n_staged, const char *who);

// One-launch distributed step (csrc/uspmv_dist_api.hip): the tile list of a step is [early | late | conditional | early].  Early entries
// (interior + padding tiles) run at once.  A late entry (a tile with real halo references) looks ONCE at the exchange counter: if the
// exchange of this step has completed it proceeds (acquire), otherwise it appends its position to the step's deferred list and
// leaves -- nothing ever spins, so no schedule can deadlock.  A second, small launch after the exchange runs the deferred entries.
// Conditional entries are the padding tiles again; they only run when x[pad_col] changed sign or is not finite (uspmv_dist::pad_col).
struct StepSync {          // device memory, 32 bytes
    int flag;              // exchanges completed so far (incremented by a one-thread kernel behind the RCCL group)
    int expect;            // value `flag` must have reached for the current step's late entries
    int count[2];          // deferred entries of the current / next step (indexed by expect & 1)
    int reruns;            // steps whose conditional entries ran
    int spare[3];
};
struct StepArgs {
    long n_early = 0, n_real = 0, n_cond = 0, defer_cap = 0;
    long late0 = 0;                // the late + conditional entries sit at [late0, late0 + n_real + n_cond) of the list, early entries around them
    StepSync *ss = nullptr;
    int *defer = nullptr;          // [2][defer_cap] positions in the step list
    const void *stale = nullptr;   // value of x[pad_col] before the exchange
    int pad_col = -1;
};

// the additive chunk records as scs_spmv_tlc<..., ADD = true> takes them (uspmv_dmat::TlcPlan::add_*)
struct AddArgs {
    const int *iv_ptr = nullptr, *iv = nullptr;
    const unsigned short *map16 = nullptr;         // pre-sort column of x[q] = (q & ~w_mask) + map16[q]
    const int *line_ptr = nullptr, *lines = nullptr;   // per tile with intervals: line | interval << 27
    int w_mask = 15;
    int ivt_off = 0;                               // byte offset in LDS of the per-wave copies of the tile's interval table
    const unsigned *ptrs = nullptr;
    const unsigned short *rec = nullptr;
};

// y = alpha A x + beta z with two dot products (uspmv_spmv_axpby) as the kernels' store epilogue takes it: alpha and
// beta already in the handle's value type; z, w in y's row order (z is read only when beta != 0, w only when it is there); part: two
// doubles per workgroup, the workgroup with logical id b writes slot slot0 + b (nullptr: no reduction code runs); rows below n_dot
// enter the dots.
template <typename VT>
struct AxpbyArgs {
    VT alpha = VT(1), beta = VT(0);
    const VT *z = nullptr, *w = nullptr;
    double *part = nullptr;
    long n_dot = 0;
    unsigned slot0 = 0;
};
constexpr int AXPBY_RED_BYTES = 16 * 2 * 8;   // LDS of the workgroup reduction: 16 waves x 2 doubles, the front of the kernel's dynamic window

constexpr int USPMV_SKIP_LEN = -4;    // (a multiple of four: no kernel sees a partial group or a tail in it)

// the chunk lengths a launcher hands to its kernel: the handle's own, or the selected part's (order 0 caller's rows, 1 phased plan rows)
inline const int32_t *part_lengths(const uspmv_dmat *A, int order) {
    return A->part && A->part_len[order][A->part - 1] ? A->part_len[order][A->part - 1] : A->chunk_lengths;
}
// false: a part is selected and this order has no arrays for it -- the launcher must not run
inline bool part_ok(const uspmv_dmat *A, int order) { return !A->part || A->part_len[order][A->part - 1]; }

struct Tuning {
    // defaults = fastest of the interleaved sweep on the nlpkkt200-class matrix (profiles/r01_sweep253.txt)
    int unroll = 8;
    int nontemporal = 1;
    int xcd_remap = 256;  // groups of 256 consecutive workgroups per XCD (profiles/r01/sweepH.txt); bits 20+: the stagger (remap_block)
    int block = 256;
    int spmv_variant = 0;
    int csr_lanes = 0;  // 0 = choose from average row length
    int ablate = 0;     // measurement only
    int tlc = 1;            // use the tile-local-column kernel when the handle carries a plan
    int rechunk = 1;        // uspmv_dmat_optimize may re-chunk C < 32 structs to C = 32 internally
    int tlc_tile_rows = 0;    // rows (= threads) per tile used by the NEXT uspmv_dmat_optimize[_ap / _device]: 256 | 512 | 1024, 0 = 256 for one
                              // struct and 512 for an ap[dp_sp] pair (two streams: the x window of 256 rows left 20 waves per CU, profiles/r02/ap_tile_rows.txt)
    int tlc_auto_tile = 1;    // with tlc_tile_rows 0 and one struct: 1024- or 512-row tiles when the largest 256-row tile needs > 250 x lines
                              // (<= 16 waves per CU) and the larger tiles still stage >= 99 % of the tiles (profiles/r03/tile_rows_sweep.txt)
    int tlc_measure_tile = 1; // large single structs (>= 2^20 padded rows): build the plan for 256 / 512 / 1024 rows on the device, time the kernel, keep
                              // a larger tile when it is > 3 % ahead (tlc_planner.hip measured_tile_rows; the 304^3 stencil: 512 rows, 7 % ahead)
    int tail_batch = 0;     // ragged tail of a chunk as one predicated batch
    int spmmv_unroll = 0;   // 0 = auto (256 bytes of X rows per lane and batch)
    int spmmv_lds_kb = 0;    // block plan: LDS budget per tile in KiB for the NEXT uspmv_dmat_optimize_block (0 = 80)
    int spmmv_tile_rows = 0; // block plan: 0 = auto (32-row tiles for >= 64-byte rows on C = 32), 64 = always 64
    int raw_plan_cache = 0; // uspmv_scs_gpu_*: remember a device-built plan per set of array addresses (opt-in)
    int spmmv_swizzle = 0;  // block-plan kernel: 1 = piece-swizzled X rows in LDS (all 64 banks); 0 = plain layout, which
                            // needs ~10 fewer address instructions per non-zero and measures 5-7 % faster (spmmv_probe16.txt)
    int spmmv_prefetch = 1; // row-major lane-per-row kernel: request batch k+1's matrix entries behind batch k's X rows
    int sweep = 1;          // use the column-window sweep kernel when the handle carries a sweep plan
    int sweep_threads = 0;     // threads per sweep workgroup (0 = min(tile rows, 1024); 256 | 512: a lane owns tile rows / threads rows, at most 4)
    int sweep_nbuf = 1;     // LDS buffers per workgroup: 1 = two 1024-thread workgroups per CU cover each other's staging (0.63 vs 0.72 ms on
                            // config 4b); 2 = one workgroup, window s+1 lands while window s is consumed
    int sweep_pair = 2;     // 1: two chains per lane side by side (two rows of the lane, or the dp and the sp part of a row): twice the entries in flight per
                            // wave (config 4b: ap 0.536 -> 0.514 ms, dp 0.585 -> 0.576); 2: ... and the FMAs under the rounds' lane masks (EXEC) instead of
                            // copy + FMA + two selects (ap 0.527 -> 0.511, dp 0.578 -> 0.570; profiles/r03/config4b_sweep.txt); 0: one chain at a time
    int sweep_unroll = 8;   // rounds per batch
    int sweep_remap = 8;    // consecutive sweep tiles per XCD (neighbouring tiles share their x windows)
    int sweep_wlog = 0;     // NEXT uspmv_dmat_optimize_sweep: log2 of the window width in elements (0 = 64 KiB of VT)
    int sweep_tile_rows = 0;  // NEXT uspmv_dmat_optimize_sweep: 256 | 512 | 1024 | 2048 | 4096 rows per tile (0 = default; above 1024: several rows per lane)
    int sweep_max_stage = 0;  // NEXT plan: largest staging cost in bytes per non-zero for a tile to sweep (0 = 24)
    int spmmv_unscramble = 0;  // 1: NEXT uspmv_dmat_optimize_block (64-byte rows, sigma > 1, host struct with its permutation) also builds the plan over
                               // ORIGINAL X-row numbering; uspmv_spmmv on column-major vectors then lets the re-layout pass undo the sigma permutation (a tile's X
                               // rows become runs of the workspace, two needed rows per 128-byte line instead of 1.1).  Measured 1 % SLOWER on config 3
                               // (0.925 vs 0.912-0.919 ms, profiles/r03/config3_colwise.txt): the staging is not bound by L2 -> L1 lines.  Off by default.
    int block_plan_device = 1;  // uspmv_dmat_optimize_block_device: 1 = row order, phases, lists and indices built on the device (block_plan_kernels.hip),
                               // 0 = index arrays copied to the host and planned there (values gathered on the device either way)
    int spmmv_xline = 0;       // 1: NEXT uspmv_dmat_optimize_block with 64-byte rows also builds the LINE plan and uspmv_spmmv stages column-major X by 128-byte
                               // lines, without the re-layout pass.  Off by default: under sigma > 1 the column numbering is scrambled inside the windows (lines
                               // are 1/3 used, the planner turns the plan down), and at sigma = 1, where it qualifies, it measures 0.930 ms against 0.905 ms
                               // behind the re-layout pass on config 3 (1.35 x the phases; profiles/r03/config3_colwise.txt)
    int spmmv_ycol_nt = 0;     // phased SpMMV kernel, column-major Y: 1 = non-temporal element stores, 0 = plain (write-back) stores that the L2 can merge into whole lines
    int spmmv_xcol = 0;        // phased SpMMV kernel on column-major X: 0 = separate re-layout pass first (1.078 ms on config 3), 1 = rows assembled in LDS by
                               // the kernel itself from the column-major vector (no workspace, no extra launch, but 1.123 ms: 74 registers, six workgroups per CU)
    int spmmv_phased = 1;      // NEXT uspmv_dmat_optimize_block with 64-byte rows: also build the phased plan (eight workgroups per CU)
    int spmmv_phase_rows = 256;  // ... X rows per phase (256 | 512)
    int spmmv_list_plan = 0;   // NEXT optimize_block: also build the one-list-per-tile plan (variants 4 / 5 / 6) when the phased kernel can take the matrix
    int spmmv_idx8 = 1;        // NEXT optimize_block: one-byte phase-local indices when every phase lists <= 256 rows
    int tlc_elem = 1;        // NEXT uspmv_dmat_optimize[_device] (one struct): when the 16-element-line plan stages under nine tenths of the tiles, try the
                             // plan over single x elements (each distinct column of a tile gathered once into LDS) before the column-window sweep; 2 = always try.
                             // The parts of an ap split likewise, one shared plan (uspmv_dmat_optimize_ap[_hp] and their _device forms; an ap[dp_sp] pair under
                             // 2^20 padded rows only under 2: tlc_planner.hip ap_elements_by_default)
    int tlc_elem_rows = 1;   // ... (host planner only) when the element plan over the caller's row order fails too: 1 = deal the rows to the tiles by the matrix graph first (private value copy + row map)
    int tlc_elem_seg_rows = 65536;  // ... rows of the segments the row dealing clusters independently (larger: numberings that scatter related rows further apart)
    int tlc_elem_cap = 4096; // ... most elements a tile may list (4096: 32 KiB of doubles, local indices still fit 12 bits)
    int tlc_idx12 = 1;       // NEXT optimize: tile-local-column plans of <= 256 lines per tile also get their local indices packed to 12 bits: 0 = never,
                             // 1 = kept when the mean row length is >= 8, 2 = kept wherever it can be built
    int tlc_additive = 1;    // NEXT uspmv_dmat_optimize (one struct with its permutation, square, line plan kept): additive chunk records beside the local
                             // indices: 0 = never, 1 = kept when records + map are at most half of the index stream they replace, 2 = wherever they can be built
    int spmmv_reorder = 4;  // block plan's private copy of the entries (host planner): 1 = rows of equal-length chunks of a sigma window back in original order;
                            // 4 = on top of that, rows re-dealt to the tiles as FLAT patches of the matrix graph (grown along the slots of one phase
                            // around the diagonal: 7.9 instead of 11.9 staged X rows per row on config 3; kept only where a sample of tiles
                            // confirms it); 2 = the same with balls over all slots (fewer distinct X rows per tile, but more per phase); 0 = as is.
                            // The device-side builder (handles without a host struct) always does 1.
    int spmmv_brick_stride = 0;   // spmmv_reorder 3 (measurement aid): rows of a mesh line in ORIGINAL numbering; tiles = flat bricks of spmmv_brick_lines lines
    int spmmv_brick_lines = 4;
    int spmmv_phase_dp = 24;  // NEXT optimize_block (host planner): > 0 = phase cuts by dynamic programming (least staged rows + this many rows' worth per
                              // phase), 0 = every phase filled to the brim (what the device-side builder does)
    int spmmv_stream = 0;   // NEXT optimize_block (64-byte rows, C = 32, one-byte indices): > 0 = also lay the phased plan out as a flat schedule for this many
                            // persistent workgroups per CU (at most 5: 32 KiB of LDS each) and let uspmv_spmmv run the streaming kernel (spmmv_stream.hip)
    int spmmv_stream_waves = 4;  // ... depth 1: register budget of the kernel in waves per SIMD (4 | 5)
    int spmmv_stream_depth = 1;  // ... 1 = X rows and entries one phase ahead (two LDS buffers, full wait per phase); 2 = two phases ahead (three buffers, partial wait)
    int spmmv_stream_xcd = 1;  // ... 1 = the workgroups of an XCD take consecutive tiles, 0 = tile t goes to workgroup t % grid
    int spmmv_variant = 0;  // 0 = auto (= 3 where a B-specialised kernel exists); 1 = generic kernel; 2 = row-major with transposing X phase; 3 = row-major, lane per row
};
extern Tuning g_tune;   // uspmv_api.hip

int require_device();                                    // uspmv_api.hip
int check_dmat(const uspmv_dmat *A, const char *who);    // uspmv_api.hip
int check_dmat_one_prec(const uspmv_dmat *A, const char *who);   // uspmv_api.hip: ... and not an fp16 handle
// the parts of an ap split with an fp16 part: hi F64 | F32, mid F32 (hi F64) or NULL, hp F16, one row layout
int check_ap_hp(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const char *who);   // tlc_planner.hip
// 16-bit index offsets per chunk from the chunk lengths (O(n_chunks) on the host); false: too large for 32-bit offsets
bool c16_offsets(const std::vector<int32_t> &cl, int64_t C, std::vector<uint32_t> *c16p, int64_t *tot16);   // tlc_planner.hip
// the column-window sweep plan from host structs / from the handles' device arrays (sweep_planner.hip); wlog, tile_rows 0: defaults
// (parts: the one struct, or the parts of an ap split sharing the plan, see uspmv_dmat::SweepPlan)
int sweep_plan_install(uspmv_dmat *const parts[], const uspmv_scs *const ss[], int n_parts, int wlog, int tile_rows, int64_t *n_tiles,
                       int64_t *n_sweep, const char *who);
int sweep_plan_install_device(uspmv_dmat *const parts[], int n_parts, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep,
                              const char *who);
// what a sweep plan -- of vectors or of block vectors -- is built with when the caller and the tuning table leave it open (sweep_planner.hip):
// rows per tile for n_pad padded rows, and the most staged bytes per non-zero at which a tile still sweeps
int sweep_default_tile_rows(int64_t n_pad);
double sweep_max_stage();
// FNV-1a digest of a device array (sweep_planner.hip; the plan digests the tests compare host and device builders by)
int device_fnv(const void *d, size_t bytes, uint64_t *out);
constexpr size_t WG_LDS_BYTES = 160 * 1024;   // all the LDS a gfx950 workgroup can have: what a sweep kernel's window buffer(s) and the staged block kernel's tile must fit
// threads per workgroup of every sweep kernel: 1 024 (or the tile, if smaller) unless "sweep_threads" asks for fewer -- a lane then owns
// tile_rows / threads rows, at most 4
inline int sweep_threads(const uspmv_dmat::SweepPlan &w) {
    int threads = std::min<int>(w.tile_rows, g_tune.sweep_threads > 0 ? g_tune.sweep_threads : 1024);
    if (w.tile_rows / threads > 4) threads = w.tile_rows / 4;
    return threads;
}
// the block sweep kernels (ap_spmmv_sweep.hip, ap_hp_spmmv_sweep.hip): vectors per pass at width b on windows of 2^wlog elements of
// x_bytes each (0: does not apply) / on this plan with its threads per workgroup
inline int sweep_vectors(int b, int wlog, size_t x_bytes) {
    if (b != 2 && b != 4 && b != 8 && b != 16) return 0;
    for (int bs = 8; bs >= 2; bs >>= 1)
        if (bs <= b && b % bs == 0 && (x_bytes << wlog) * bs <= WG_LDS_BYTES) return bs;
    return 0;
}
inline int sweep_block_bs(const uspmv_dmat::SweepPlan &w, int b, size_t x_bytes) {
    const int threads = sweep_threads(w);
    if (threads < 64 || threads % 64 || w.tile_rows % threads) return 0;
    const int rpl = w.tile_rows / threads;
    if (rpl != 1 && rpl != 2 && rpl != 4) return 0;
    return sweep_vectors(b, w.wlog, x_bytes);
}
// the staged block kernel of the ap kinds (ap_hp_spmmv_kernels.hip): as many of the b vectors per pass as the plan's fullest tile leaves
// room for in LDS (at most 8: 2 * 8 accumulators per lane); 0: not two
inline int tlc_block_bs(const uspmv_dmat::TlcPlan &t, int b, size_t x_bytes) {
    const size_t line_bytes = (size_t)t.max_lines * 16 * x_bytes;
    for (int bs = 8; bs >= 2; bs >>= 1)
        if (bs <= b && b % bs == 0 && line_bytes * bs <= WG_LDS_BYTES) return bs;
    return 0;
}
inline unsigned grid_for(long work_items, int block) { return (unsigned)((work_items + block - 1) / block); }

constexpr size_t BT_LDS_CAP = 80 * 1024;  // LDS per single-wave SpMMV tile (block plan): two tiles per CU at worst

// launch entry points (explicitly instantiated for double and float in their kernel files)
// ep != nullptr (uspmv_spmv_axpby on path 1 only, spmv_axpby_route): the fused instantiations, which store alpha t + beta z and leave
// their workgroups' dot partials in ep->part
template <typename VT>
int launch_spmv_scs(const uspmv_dmat *A, const int *chunk_ids, long n_ids, const VT *x, VT *y, hipStream_t st, const AxpbyArgs<VT> *ep = nullptr);   // spmv_kernels.hip
template <typename VT>
int launch_spmv_tlc(const uspmv_dmat *A, const int *tile_ids, long n_tiles, const VT *x, VT *y, hipStream_t st, const AxpbyArgs<VT> *ep = nullptr);  // spmv_kernels.hip
// uspmv_spmv_axpby on the struct uspmv_spmv would launch (M: the handle or its re-chunking; crs: the csr kernel): 1 when the launch that
// serves it has a fused instantiation -- the conditions launch_spmv_scs / launch_csr branch on --, else 2; *slots: workgroups of the
// launch(es) that serve the call on that path
int spmv_axpby_route(const uspmv_dmat *M, bool crs, bool x16, long *slots);                                        // spmv_kernels.hip
// path 2's vector pass over rows [0, n): y = alpha t + beta z from the stored t (t may be y), the same epilogue routine, same partials
template <typename VT>
int launch_axpby_pass(const VT *t, VT *y, long n, const AxpbyArgs<VT> &ep, hipStream_t st, long *slots);            // spmv_kernels.hip (*slots: workgroups launched)
long axpby_pass_slots(long n);   // the most it launches for n rows
// dots[0 .. 2) = the sums of part[2 k], part[2 k + 1] over k < slots, in one fixed order
int launch_axpby_finalize(const double *part, long slots, double *dots, hipStream_t st);                           // spmv_kernels.hip
// the one-launch distributed step over `step_ids` = [early | late | conditional] (sync 1) and its deferred entries (sync 2)
template <typename VT>
int launch_spmv_tlc_step(const uspmv_dmat *A, const int *step_ids, const StepArgs &sa, int sync, const VT *x, VT *y, hipStream_t st);
template <typename VT>
int launch_csr(long n_rows, long nnz_hint, const int *rp, const int *ci, const VT *va, const VT *x, VT *y, hipStream_t st, const AxpbyArgs<VT> *ep = nullptr);  // spmv_kernels.hip
template <typename VT>
int launch_spmmv(const uspmv_dmat *A, const VT *X, VT *Y, int b, long ld, int layout, hipStream_t st);            // spmmv_kernels.hip
template <typename VT>
int launch_spmmv_sweep(const uspmv_dmat *A, const VT *X, VT *Y, int b, long ld, bool xcol, bool ycol, hipStream_t st);   // spmmv_sweep.hip; false-y: USPMV_OK when launched, > 0 when the plan does not apply
template <typename VT>
int prepare_x(const uspmv_dmat *A, const VT *X, int b, long ld, hipStream_t st);                                    // spmmv_kernels.hip
int relayout_x_plain(const uspmv_dmat *A, const double *X, int b, long ld, hipStream_t st);                       // spmmv_kernels.hip
// phased block plan, 64-byte X rows (spmmv_phased.hip); false: no plan / schedule on the handle or it does not fit the compiled shapes
// xmode: 0 = row-major X, 1 = column-major X assembled through registers, 2 = column-major X staged by 128-byte lines (line plan)
bool spmmv_phased(const uspmv_dmat *A, const double *X, double *Y, long ld, bool ycol, int xmode, hipStream_t st);
bool spmmv_phased(const uspmv_dmat *A, const float *X, float *Y, long ld, bool ycol, int xmode, hipStream_t st);
// the same plan walked by persistent workgroups (spmmv_stream.hip); false: no schedule on the handle / shape not covered
bool spmmv_stream(const uspmv_dmat *A, const double *X, double *Y, long ld, bool ycol, hipStream_t st);
bool spmmv_stream(const uspmv_dmat *A, const float *X, float *Y, long ld, bool ycol, hipStream_t st);
int dmat_stream_schedule(uspmv_dmat *A, int wgs_per_cu);
int launch_spmv_ap(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *d_x, const float *d_x_sp, double *d_y,
                   hipStream_t stream, const AxpbyArgs<double> *ep = nullptr);                                    // ap_kernels.hip
// uspmv_spmv_ap_axpby on this pair: 1 when the launch(es) launch_spmv_ap would make have fused instantiations -- its own conditions --,
// else 2; *slots: workgroups of the launch(es) that serve the call on that path (path 2: of the vector pass)
int spmv_ap_axpby_route(const uspmv_dmat *dp, const uspmv_dmat *sp, bool x16, long *slots);                        // ap_kernels.hip
// ap[dp_sp] on block vectors: b = 1 forwards to launch_spmv_ap; B in {2, 4, 8, 16} the pair's column-window sweep plan where it carries one,
// else the row-major kernels (column-major X through the dp handle's workspace); any other b lane per row with VB vectors per pass
int launch_spmmv_ap(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, int b, long ld, int layout,
                    hipStream_t st);                                                                              // ap_spmmv_kernels.hip
int spmmv_ap_plan_lines(int b);   // most lines per tile of a shared plan the staged block kernel takes at width b (0: no such kernel)
// what launch_spmmv_ap runs for 16-byte-aligned X / Y (b >= 2): 0 generic lane per row, 1 gather, 2 staged over the shared line plan,
// 3 column-window sweep; vectors: per pass of the sweep / staged kernel, else 0
void spmmv_ap_path(const uspmv_dmat *dp, const uspmv_dmat *sp, int b, long ld, int layout, int *path, int *vectors);   // ap_spmmv_kernels.hip
// the tiles in tile_ids of the pair's shared tile-local-column plan (entries < 0 skipped), X and Y in `layout`: the staged kernel where
// spmmv_ap_tiles_path says 2, else lane per row over the tiles' rows
int launch_spmmv_ap_tiles(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *tile_ids, long n_ids, const double *X, double *Y, int b,
                          long ld, int layout, hipStream_t st);                                                     // ap_spmmv_kernels.hip
// what launch_spmmv_ap_tiles runs for 16-byte-aligned X / Y: 2 the staged kernel (vectors per pass), 0 lane per row (vectors 0)
void spmmv_ap_tiles_path(const uspmv_dmat *dp, const uspmv_dmat *sp, int b, long ld, int layout, int *path, int *vectors);   // ap_spmmv_kernels.hip
// lane per row over a list of chunks (the rest chunks of the pair's sweep plan, the chunk lists of a distributed step; entries < 0
// skipped), any b
int launch_spmmv_ap_chunks(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *chunk_ids, long n_ids, const double *X, double *Y, int b,
                           long ld, int layout, hipStream_t st);                                                    // ap_spmmv_kernels.hip
// the block sweep kernel (ap_spmmv_sweep.hip): vectors per pass at width b on windows of 2^wlog doubles (0: does not apply) / on this
// handle's plan and threads per workgroup (capped by the accumulators a lane can hold); the launch: sweep tiles, then the rest chunks
int spmmv_ap_sweep_vectors(int b, int wlog);
int spmmv_ap_sweep_bs(const uspmv_dmat *dp, int b);
int launch_spmmv_ap_sweep(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, int b, long ld, bool colwise, int bs,
                          hipStream_t st);
// ap with an fp16 part (hi F64 | F32, mid F32 or nullptr, hp F16): the shared tile-local-column plan when all parts carry it, else lane per row
int launch_spmv_ap_hp(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const void *d_x, void *d_y, hipStream_t stream,
                      const void *ep = nullptr);                                                                    // ap_kernels.hip
// uspmv_spmv_ap_hp_axpby on these parts, as spmv_ap_axpby_route
int spmv_ap_hp_axpby_route(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, bool x16, long *slots);   // ap_kernels.hip
// what launch_spmv_ap_hp runs: 3 the shared column-window sweep, 2 the shared tile-local-column plan, 0 lane per row
int spmv_ap_hp_path(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, bool x_aligned16);                                   // ap_kernels.hip
// ... on block vectors (X, Y in the type of the hi part): b = 1 forwards to launch_spmv_ap_hp; b in {2, 4, 8, 16} on 16-byte-aligned
// vectors the sweep kernel over the parts' shared column-window sweep plan where two vectors of a window fit LDS, the staged kernel over
// their shared tile-local-column plan where two vectors of its fullest tile fit LDS; else lane per row with VB vectors per pass
// (handles without a plan, any other b, layout or alignment)
int launch_spmmv_ap_hp(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const void *X, void *Y, int b, long ld, int layout,
                       hipStream_t st);                                                                           // ap_hp_spmmv_kernels.hip
int spmmv_ap_hp_plan_lines(int b, int x_dtype);   // most lines per tile of a shared plan the staged block kernel takes at width b (0: no such kernel)
// what launch_spmmv_ap_hp runs for 16-byte-aligned X / Y: 0 lane per row, 2 staged over the shared line plan (b = 1: spmv_ap_hp_path);
// 3 the column-window sweep kernel over the shared sweep plan; vectors: per pass of the staged / sweep kernel, else 0
void spmmv_ap_hp_path(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, int b, long ld, int layout, int *path, int *vectors);
// the block kernels every ap kind shares (ap_hp_spmmv_kernels.hip); the kind follows from the handles: hi F64 | F32, mid F32 or nullptr,
// last F16 -- or F32 for the ap[dp_sp] pair (dp, nullptr, sp).  X, Y in the type of hi.
// lane per row, any b, layout and alignment: over the chunks chunk_ids[0 .. n_ids) (entries < 0 skipped), or over all where chunk_ids is
// nullptr.  tile_rows > 0: the ids are tiles, tile t = the rows [t * tile_rows, (t + 1) * tile_rows)
int launch_spmmv_ap_rows(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *last, const int *chunk_ids, long n_ids, const void *X,
                         void *Y, int b, long ld, int layout, hipStream_t st, int tile_rows = 0);
// staged over the parts' shared tile-local-column plan, b in {2, 4, 8, 16}, bs vectors per pass (tlc_block_bs), 16-byte-aligned X / Y.
// ycol: column-major Y.  The kinds with an fp16 part read X in the layout of Y; the pair always reads row-major X -- except over
// tile_ids (workgroup g runs tile tile_ids[g] of the n_ids listed, entries < 0 skipped), where X is in the layout of Y.  Over tile_ids the
// kinds with an fp16 part take column-major X at every ld (columns off the 16-byte grid are staged in 8- or 4-byte pieces)
int launch_spmmv_ap_staged(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *last, const void *X, void *Y, int b, long ld, bool ycol,
                           int bs, hipStream_t st, const int *tile_ids = nullptr, long n_ids = 0);
// lane per row over a list of chunks (the rest chunks of a sweep plan's block form, the chunk lists of a distributed step; entries < 0
// skipped), any b
int launch_spmmv_ap_hp_chunks(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *chunk_ids, long n_ids,
                              const void *X, void *Y, int b, long ld, int layout, hipStream_t st);                 // ap_hp_spmmv_kernels.hip
// the tiles in tile_ids of the parts' shared tile-local-column plan (entries < 0 skipped; the caller has checked that they share one),
// X and Y in `layout`: the staged kernel where spmmv_ap_hp_tiles_path says 2, else lane per row over the tiles' rows
int launch_spmmv_ap_hp_tiles(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *tile_ids, long n_ids, const void *X,
                             void *Y, int b, long ld, int layout, hipStream_t st);                                  // ap_hp_spmmv_kernels.hip
// what launch_spmmv_ap_hp_tiles runs for 16-byte-aligned X / Y: 2 the staged kernel (vectors per pass), 0 lane per row (vectors 0)
void spmmv_ap_hp_tiles_path(const uspmv_dmat *hi, int b, int *path, int *vectors);                                 // ap_hp_spmmv_kernels.hip
// the block sweep kernel of the splits with an fp16 part (ap_hp_spmmv_sweep.hip): vectors per pass at width b on windows of 2^wlog
// elements of x_dtype (USPMV_F64 | USPMV_F32; 0: does not apply) / on this handle's plan and threads per workgroup; the launch: sweep
// tiles, then the rest chunks
int spmmv_ap_hp_sweep_vectors(int b, int wlog, int x_dtype);
int spmmv_ap_hp_sweep_bs(const uspmv_dmat *hi, int b);
int launch_spmmv_ap_hp_sweep(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const void *X, void *Y, int b, long ld,
                             bool colwise, int bs, hipStream_t st);
template <typename VT>
int launch_spmv_sweep(const uspmv_dmat *A, const VT *x, VT *y, hipStream_t st, const AxpbyArgs<VT> *ep = nullptr);   // sweep_kernels.hip (sweep tiles only)
bool sweep_axpby_fused(const uspmv_dmat *A);   // sweep_kernels.hip: the sweep launch of this handle under the current tuning has a fused instantiation
// ep != nullptr here and in the launchers of the ap splits below (uspmv_spmv_ap[_hp]_axpby on path 1 only, spmv_ap[_hp]_axpby_route):
// the fused instantiations; the launchers of the kinds with an fp16 part take it as const AxpbyArgs<HT> * behind a void pointer, HT the
// type of x and y
int launch_spmv_sweep_ap(const uspmv_dmat *dp, const double *x, double *y, hipStream_t st, const AxpbyArgs<double> *ep = nullptr);   // sweep_kernels.hip
int launch_spmv_ap_chunks(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *chunk_ids, long n_ids, const double *d_x,
                          double *d_y, hipStream_t stream, const AxpbyArgs<double> *ep = nullptr);                 // ap_kernels.hip
// the tiles in tile_ids of the pair's shared tile-local-column plan (entries < 0 skipped): scs_spmv_ap_tlc over a tile list
int launch_spmv_ap_tiles(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *tile_ids, long n_ids, const double *d_x, double *d_y,
                         hipStream_t stream);                                                                      // ap_kernels.hip
// the sweep tiles of a plan shared by the parts of a split with an fp16 part (sweep_ap_hp_kernels.hip) and the chunks it leaves over
int launch_spmv_sweep_ap_hp(const uspmv_dmat *hi, bool mid, const void *x, void *y, hipStream_t st, const void *ep = nullptr);
int launch_spmv_ap_hp_chunks(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *chunk_ids, long n_ids,
                             const void *d_x, void *d_y, hipStream_t stream);                                      // ap_kernels.hip
// the tiles in tile_ids of the parts' shared tile-local-column plan (entries < 0 skipped): scs_spmv_ap_hp_tlc over a tile list
int launch_spmv_ap_hp_tiles(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *tile_ids, long n_ids,
                            const void *d_x, void *d_y, hipStream_t stream);                                       // ap_kernels.hip

// The line plan of one struct or of the two or three parts of an ap split (parts[k] NULL from the first missing one on; the sp part of an
// ap[dp_sp] pair, the hp part(s) of a split with an fp16 part): lines per tile of tile_rows rows, then the lists and part k's local indices
// (to d_col16[k] at d_c16_ptrs[k])
int launch_plan_count(const uspmv_dmat *const parts[3], long n_tiles, int max_lines, int *d_n_lines, int *d_max_col, int tile_rows, hipStream_t st);   // plan_kernels.hip
int launch_plan_pack12(const uspmv_dmat *A, const unsigned *d_c16_ptrs, const unsigned short *d_col16, const unsigned *d_c12_ptrs, unsigned *d_col12, hipStream_t st);   // plan_kernels.hip
int launch_plan_write(const uspmv_dmat *const parts[3], long n_tiles, const int *d_tile_line_ptr, int *d_tile_lines, const unsigned *const d_c16_ptrs[3],
                      unsigned short *const d_col16[3], int tile_rows, hipStream_t st);                                    // plan_kernels.hip
// the plan over single x elements on 256-row tiles: distinct columns per tile clipped at cap + 1 (cap <= 16384), then the sorted lists
// and the slots' ranks; most_listed: the longest list of d_tile_line_ptr
// the plan over single x elements of one struct or of the two or three parts of an ap split (parts[k] NULL from the first missing one on)
int launch_plan_count_elems(const uspmv_dmat *const parts[3], long n_tiles, int cap, int *d_n_elems, int *d_max_col, hipStream_t st);   // plan_kernels.hip
int launch_plan_write_elems(const uspmv_dmat *const parts[3], long n_tiles, int most_listed, const int *d_tile_line_ptr, int *d_tile_lines,
                            const unsigned *const d_c16_ptrs[3], unsigned short *const d_col16[3], hipStream_t st);          // plan_kernels.hip
int launch_rechunk32(const uspmv_dmat *A, const int *d_cp_new, int *d_ci_new, void *d_va_new, hipStream_t st);             // plan_kernels.hip
int launch_block_values_gather(const uspmv_dmat *A, const int *d_row_map, const unsigned *d_c16_ptrs, void *d_out, bool group_major, hipStream_t st);   // plan_kernels.hip
// device-side builder of the phased block plan (block_plan_kernels.hip)
int launch_block_reorder(const uspmv_dmat *A, int *d_row_map, int *d_changed, hipStream_t st);
int launch_block_tile_class(const uspmv_dmat *A, long n_local, unsigned char *d_flags, hipStream_t st);
int launch_part_len_fill(const uspmv_dmat *A, int rows_per_flag, const unsigned char *d_flags, int *d_len_int, int *d_len_bnd, hipStream_t st);
// drops every block plan: the list plan, the phased plan with its stream schedule, the line and unscrambled plans, and the part
// arrays classified per tile of the phased plan (part_len[1])
inline void block_plan_reset(uspmv_dmat *A) {
    A->bt = {}; A->pb = {}; A->ps = {}; A->pl = {}; A->pu = {};
    A->part_len[1][0].reset(); A->part_len[1][1].reset();
}
// two-part SpMMV (uspmv_dmat::part_len; block_planner.hip): order 0 from per-chunk flags (1 = the chunk touches a halo column), order 1 from
// the lists of the handle's phased plan (no-op without one); the arrays belong to the handle (order 1 goes with the plan)
int dmat_part_set_chunks(uspmv_dmat *A, const unsigned char *h_chunk_flags);
int dmat_part_set_plan(uspmv_dmat *A, long n_local, int64_t *n_boundary_tiles);
int launch_block_phase_plan(const uspmv_dmat *A, bool write, int cap, int ngp, const int *d_row_map, const unsigned *d_c16_ptrs, int *d_t_phases,
                            int *d_t_list, int *d_ph_g0, int *d_ph_list_ptr, int *d_xrows, unsigned char *d_col8, int *d_max_rows, hipStream_t st);
// device-side builder of the column-window sweep plan (sweep_plan_kernels.hip)
int launch_sweep_scan(const uspmv_dmat *A, int wlog, int *d_row_le, int *d_row_pad, int *d_grp, int *d_max_col, hipStream_t st);
int launch_sweep_fill(const uspmv_dmat *A, int wlog, int R, long n_sweep_tiles, const int *d_tile_ids, const int *d_smin, const int *d_S,
                      const unsigned long long *d_cnt_off, const unsigned *d_wave_off, const int *d_row_le, const int *d_row_pad,
                      unsigned char *d_cnt, void *d_vals, unsigned short *d_idx, int *d_pad_col, hipStream_t st);

// exclusive scan of n longs on the device, narrowed to 32 bits: d_ptrs[0 .. n] (d_ptrs[n] = *d_total = the sum); d_part: n longs,
// d_sums: (n + 1023) / 1024 longs of scratch (convert_kernels.hip: the chunk pointers, the bases of the partition)
int launch_exclusive_scan(const long *d_in, long n, long *d_part, long *d_sums, long *d_total, int *d_ptrs, hipStream_t st);
// partition_precisions on the device (ap_partition_kernels.hip): the compacted parts' arrays (n: their sizes) ...
struct ApPartOut {
    int *I[3], *J[3];
    double *V[3];
    long n[3];
};
// ... workgroups of the two passes = counts per part, d_counts[part * n_wg + wg]; d_flag: 1 rows unsorted, 2 row index / 4 column index
// outside the matrix; *d_first_nan: the first element that fits no part (min over the workgroups); d_base: the scan of d_counts
long ap_partition_workgroups(long nnz);
int launch_ap_partition_count(const int *I, const int *J, const double *V, long nnz, int n_rows, int n_cols, int kind, double t1, double t2,
                              long *d_counts, int *d_flag, unsigned long long *d_first_nan, hipStream_t st, const double *row_max = nullptr,
                              const double *col_max = nullptr);
int launch_ap_partition_scatter(const int *I, const int *J, const double *V, long nnz, int kind, double t1, double t2, const int *d_base,
                                const ApPartOut &out, hipStream_t st, const double *row_max = nullptr, const double *col_max = nullptr);
// (row_max / col_max: device vectors of the equilibrated branch, both NULL for the unscaled one)
// equilibrate_matrix on the device (equilibrate_kernels.hip).  d_flag bits: 1 rows unsorted, 2 row index / 4 column index outside the matrix,
// 8 a non-finite value, 16 an entry whose row divisor is 0, 32 a row-scaled value that is 0 (its column's divisor may be: launch_eq_zero_cols)
int launch_eq_row_max(const int *I, const double *V, long nnz, int n_rows, double *row_max, int *d_flag, hipStream_t st);
int launch_eq_col_max(const int *I, const int *J, const double *V, long nnz, int n_rows, int n_cols, const double *row_max, double *col_max,
                      int *d_flag, unsigned long long *d_n_atomics, hipStream_t st);
int launch_eq_zero_cols(const int *J, long nnz, const double *col_max, int *d_flag, hipStream_t st);
int launch_eq_scale(const int *I, const int *J, const double *V, double *V_out, long nnz, const double *row_max, const double *col_max, hipStream_t st);

}  // namespace uspmv_dev

#define HIP_TRY(call)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return uspmv::fail(USPMV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                               __FILE__, __LINE__);                                                \
    } while (0)


// device COO arrays read two neighbouring entries per lane, k and k + 1 (n: how many of them exist); VEC: the arrays are aligned for one
// 8-byte load of I and J and one 16-byte load of V (ap_partition_kernels.hip, equilibrate_kernels.hip)
template <bool VEC>
__device__ __forceinline__ int load_pair(const int *__restrict__ I, const int *__restrict__ J, const double *__restrict__ V, const long k, const long nnz,
                                         int i[2], int j[2], double v[2]) {
    const int n = k + 1 < nnz ? 2 : (k < nnz ? 1 : 0);
    if (VEC && n == 2) {
        const int2 a = *(const int2 *)(I + k), b = *(const int2 *)(J + k);
        const double2 c = *(const double2 *)(V + k);
        i[0] = a.x; i[1] = a.y; j[0] = b.x; j[1] = b.y; v[0] = c.x; v[1] = c.y;
    } else {
        for (int e = 0; e < n; ++e) { i[e] = I[k + e]; j[e] = J[k + e]; v[e] = V[k + e]; }
    }
    return n;
}

// ------------------------------------------------------------------------------------------
template <bool NT, typename T>
__device__ __forceinline__ T ld_stream(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
// the same through an explicitly GLOBAL pointer: where the address reaches the load through a reference or a local pointer array
// the compiler no longer knows the address space and emits flat_load (which also ties up the LDS counter) instead of global_load
template <bool NT, typename T>
__device__ __forceinline__ T ld_stream_g(const T *p) {
    typedef const T __attribute__((address_space(1))) *gp_t;
    if constexpr (NT) return __builtin_nontemporal_load((gp_t)p);
    else return *(gp_t)p;
}
// y store.  A y vector is ~2 % of the bytes of an SpMV, but its HBM write stream costs 15-18 % of the
// kernel when it goes through the write-back L2 (profiles/r01_microbench.txt: 0.74 ms without the
// store, 0.88 ms with plain stores).  Non-temporal stores (`global_store ... nt`) are the cheapest form
// measured: A/B of two builds on one box (tools/ab.sh, profiles/r01/ystore_ab.txt) 0.765 ms against 0.822 ms
// for write-through agent-scope stores (`sc1`) and 0.840 ms for plain stores on the nlpkkt200-class matrix.
template <bool WT, typename T>
__device__ __forceinline__ void st_y(T *p, T v) {
    if constexpr (WT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// ---- the store epilogue of uspmv_spmv_axpby (AxpbyArgs above) ----
// One rounding per operation, whatever -ffp-contract says: the products and sums below carry no `contract` flag, so neither the
// front end nor the back end fuses them into an FMA.
template <typename T>
__device__ __forceinline__ T mul_rn_t(T a, T b) {
#pragma clang fp contract(off)
    return a * b;
}
template <typename T>
__device__ __forceinline__ T add_rn_t(T a, T b) {
#pragma clang fp contract(off)
    return a + b;
}
// The value row `row` stores when its chain ended in t: rn(alpha t), or rn(rn(alpha t) + rn(beta z[row])) when beta != 0 (z is not
// read otherwise).  With a partial buffer, rows below n_dot add their terms <y,y> and <w,y> to the lane's d0 / d1: the operands widened
// to double (exact for floats), one rounding per product.  Called by the lane that stores the row, for rows it may store only.
template <typename VT>
__device__ __forceinline__ VT axpby_row(const uspmv_dev::AxpbyArgs<VT> &ep, const long row, const VT t, double &d0, double &d1) {
    VT v = mul_rn_t(ep.alpha, t);
    if (ep.beta != VT(0)) v = add_rn_t(v, mul_rn_t(ep.beta, ep.z[row]));
    if (ep.part && row < ep.n_dot) {
        const double vd = (double)v;
        d0 = add_rn_t(d0, mul_rn_t(vd, vd));
        if (ep.w) d1 = add_rn_t(d1, mul_rn_t((double)ep.w[row], vd));
    }
    return v;
}
// The workgroup's two partial sums, stored at slot slot0 + lb (lb: the LOGICAL block id, so that the slot does not depend on the
// dispatch order): the lanes of a wave through cross-lane adds, the waves through LDS in wave order.  EVERY thread of the workgroup
// calls this (lanes without a row with zero terms); red: AXPBY_RED_BYTES of LDS that are dead once all threads are here -- the front
// of the kernel's window.  Without a partial buffer (kernel-uniform) nothing runs.  blockDim.x is a multiple of 64.
template <typename VT>
__device__ __forceinline__ void axpby_reduce(const uspmv_dev::AxpbyArgs<VT> &ep, const unsigned lb, double d0, double d1, double *red) {
    if (!ep.part) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        d0 = add_rn_t(d0, __shfl_xor(d0, o, 64));
        d1 = add_rn_t(d1, __shfl_xor(d1, o, 64));
    }
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();                                      // everybody is through with the window
    if ((threadIdx.x & 63) == 0) { red[2 * wave] = d0; red[2 * wave + 1] = d1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int k = 0; k < nw; ++k) { s0 = add_rn_t(s0, red[2 * k]); s1 = add_rn_t(s1, red[2 * k + 1]); }
        double *p = ep.part + 2 * ((long)ep.slot0 + lb);
        p[0] = s0; p[1] = s1;
    }
}

// Adaptive precision (ap_kernels.hip, ap_hp_spmmv_kernels.hip, sweep_ap_hp_kernels.hip): one step of a part's chain.  With a double x every
// product is an FMA in double on the exactly widened value (scs_ap_impl_cpu's convention, hp in the place of sp), with a float x the
// product is rounded to float and then added to the part's double accumulator (the sp part of spmv_omp_scs_ap).  hp values arrive
// as the binary16 bits; v_cvt_f32_f16 widens them exactly.
__device__ __forceinline__ float hp_val(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ double ap_step(double v, double x, double acc) { return __builtin_fma(v, x, acc); }
__device__ __forceinline__ double ap_step(float v, double x, double acc) { return __builtin_fma((double)v, x, acc); }
__device__ __forceinline__ double ap_step(unsigned short v, double x, double acc) { return __builtin_fma((double)hp_val(v), x, acc); }
__device__ __forceinline__ double ap_step(float v, float x, double acc) { return acc + (double)__fmul_rn(v, x); }
__device__ __forceinline__ double ap_step(unsigned short v, float x, double acc) { return acc + (double)__fmul_rn(hp_val(v), x); }
// y = hi + hp, (hi + mid) + hp, or (float)(sp + hp)
template <typename HT, bool MID>
__device__ __forceinline__ HT ap_hp_y(double h, double m, double q) {
    if constexpr (sizeof(HT) == 4) return (float)(h + q);
    else if constexpr (MID) return (h + m) + q;
    else return h + q;
}

// the parts' arrays as the kernels take them (mid: nullptr unless ap[dp_sp_hp]); c16p / c16: the shared plan's per-part local indices
struct ApHpParts {
    const int *cp[3], *cl[3], *ci[3];
    const void *va[3];
    const unsigned *c16p[3];
    const unsigned short *c16[3];
};
inline ApHpParts ap_hp_parts(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp) {
    ApHpParts P{};
    const uspmv_dmat *ms[3] = {hi, mid, hp};
    for (int k = 0; k < 3; ++k) {
        if (!ms[k]) continue;
        P.cp[k] = ms[k]->chunk_ptrs; P.cl[k] = ms[k]->chunk_lengths; P.ci[k] = ms[k]->col_idxs; P.va[k] = ms[k]->values;
        P.c16p[k] = ms[k]->tlc.c16_ptrs; P.c16[k] = ms[k]->tlc.col16;
    }
    return P;
}

// DPP quad broadcast: every lane of a quad gets lane U's value (the four-lanes-per-row SpMMV kernels)
template <int U>
__device__ __forceinline__ int quad_bcast(int v) { return __builtin_amdgcn_update_dpp(0, v, U * 0x55, 0xf, 0xf, true); }   // (bound_ctrl + full masks: every lane is written, `old` is dead)
template <int U>
__device__ __forceinline__ double quad_bcast(double v) {
    return __hiloint2double(quad_bcast<U>(__double2hiint(v)), quad_bcast<U>(__double2loint(v)));
}
template <int U>
__device__ __forceinline__ float quad_bcast(float v) { return __int_as_float(quad_bcast<U>(__float_as_int(v))); }

// logical block id.  Hardware deals blocks round-robin over the 8 XCDs (b, b+8, b+16, ... share
// one).  mode 0: identity.  mode 1: every XCD walks one contiguous eighth of the grid.
// mode G >= 2: groups of G consecutive logical blocks per XCD, the 8 groups of a super-block
// of 8*G blocks being processed concurrently (keeps all XCDs inside one moving DRAM window while
// neighbouring blocks -- which share x lines -- share an L2).
// Bits 20+ of `mode` (tuning "xcd_stagger" S): XCD k starts its group S*k blocks in, wrapping around -- the eight XCDs, which move
// through their groups in step, then no longer touch addresses that differ by exact multiples of the group's byte size (256 tiles x 2 KB
// of y = 512 KiB: eight write streams 2^19 bytes apart land on whatever memory channels the physical address bits above 2^19 select --
// the same few, or all different, by the luck of the process's physical pages: profiles/r04/placement_*.txt).
__device__ __forceinline__ unsigned remap_block(unsigned b, unsigned nb, int mode) {
    const unsigned S = (unsigned)mode >> 20;
    mode &= 0xFFFFF;
    if (mode == 0 || nb < 16) return b;
    if (mode == 1) {
        const unsigned xcd = b & 7u, q = nb >> 3, r = nb & 7u;
        const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        return base + (b >> 3);
    }
    const unsigned G = (unsigned)mode, SG = 8u * G;
    const unsigned full = (nb / SG) * SG;
    if (b >= full) return b;
    const unsigned sup = b / SG, rem = b - sup * SG;
    const unsigned xcd = rem & 7u;
    unsigned pos = (rem >> 3) + S * xcd;
    if (S) pos %= G;
    return sup * SG + xcd * G + pos;
}

