// The block-vector (SpMMV) planner: uspmv_dmat_optimize_block (from a host struct through host/tlc_plan.cpp), its device builder
// (uspmv_dmat_optimize_block_device through block_plan_kernels.hip), the block-vector column-window sweep plan and the two-part
// chunk-length arrays of the distributed SpMMV.  Every decision -- which row widths get a plan, the rows per tile, what the phased
// kernel can take, when the line and the unscrambled plan are kept, what the device builder covers -- is written once here, and the
// shape limits the kernels are compiled for are named in uspmv_device.hpp.  tests/test_gpu_parity.py
// (test_device_block_plan_builder_equals_host_planner) compares the host and the device builder's plans array for array.
#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace {

bool verbose() { return getenv("USPMV_VERBOSE") != nullptr; }

size_t value_bytes(int dtype) { return dtype == USPMV_F64 ? 8 : 4; }

// only the 16-byte-piece kernels (b * sizeof(VT) in {16, 32, 64, 128}) read a block plan, compiled for C = 32 and 64
bool width_gets_plan(size_t row_bytes, int64_t C) {
    return row_bytes % 16 == 0 && (row_bytes & (row_bytes - 1)) == 0 && row_bytes <= 128 && (C == 32 || C == 64);
}
// rows of >= 64 bytes on C = 32: 32-row tiles, two lanes per row (half the LDS per tile, twice the tiles per CU); "spmmv_tile_rows" 64
// keeps 64 rows, 32 asks for 32 from 32-byte rows on
int plan_tile_rows(size_t row_bytes, int64_t C) {
    return (C == 32 && g_tune.spmmv_tile_rows != 64 && (row_bytes >= 128 || (row_bytes >= 32 && g_tune.spmmv_tile_rows == 32))) ? 32 : 64;
}
// 64-byte rows on 64-row tiles get the phased plan -- what uspmv_spmmv runs by default
bool wants_phased(size_t row_bytes, int tile_rows) { return row_bytes == 64 && tile_rows == 64 && g_tune.spmmv_phased; }
// the phased kernel can take this plan: the groups per phase and the LDS pieces of its fullest phase it is compiled for
bool phased_kernel_takes(const uspmv_phased_plan &pp) {
    return pp.valid && pp.ngp <= PHASE_GROUPS && phase_pieces(pp.max_rows_used) <= PHASE_PIECES_MAX;
}
bool one_byte_indices(const uspmv_phased_plan &pp) { return g_tune.spmmv_idx8 && pp.max_rows_used <= PHASE_ROWS_IDX8; }
// the line plan (column-major X staged by 128-byte lines, "spmmv_xline") is kept when no phase needs more than 256 rows' worth of lines
// and the lines staged stay below twice the rows the row plan stages
bool wants_line_plan() { return g_tune.spmmv_xline && g_tune.spmmv_phase_rows == PHASE_ROWS_IDX8; }
bool keep_line_plan(const uspmv_phased_plan &pl, const uspmv_phased_plan &pp, int shift) {
    return pl.valid && pl.max_rows_used <= PHASE_ROWS_IDX8 && pl.ngp <= PHASE_GROUPS && ((int64_t)pl.xrows.size() << shift) <= 2 * (int64_t)pp.xrows.size();
}
// the unscrambled plan (X rows in original numbering, "spmmv_unscramble") needs one-byte indices in both plans
bool wants_unscrambled_plan(const uspmv_phased_plan &pp) { return g_tune.spmmv_unscramble && pp.max_rows_used <= PHASE_ROWS_IDX8 && g_tune.spmmv_idx8; }
bool keep_unscrambled_plan(const uspmv_phased_plan &pu) { return pu.valid && pu.max_rows_used <= PHASE_ROWS_IDX8 && pu.ngp <= PHASE_GROUPS; }
// the device builder covers the default shape and tuning only: 64-byte rows, phases filled to the brim with one-byte indices, rows in
// tie-re-ordered order, no list / line plan beside the phased one
bool device_builder_covers(size_t row_bytes, int64_t C) {
    return row_bytes == 64 && (C == 32 || C == 64) && g_tune.spmmv_phased && g_tune.spmmv_phase_rows == PHASE_ROWS_IDX8 && !g_tune.spmmv_list_plan &&
           (g_tune.spmmv_reorder == 1 || g_tune.spmmv_reorder == 4) && g_tune.spmmv_idx8 && g_tune.spmmv_tile_rows != 32 && !g_tune.spmmv_xline &&
           g_tune.block_plan_device;
}

// a host-planned phase list onto the handle; one_byte: the phase-local indices narrowed to bytes (same layout)
hipError_t upload_phase_lists(const uspmv_phased_plan &h, bool one_byte, PhaseLists *L) {
    hipError_t e = L->ph_ptr.upload(h.ph_ptr.data(), h.ph_ptr.size() * 4);
    if (e == hipSuccess) e = L->g0.upload(h.ph_g0.data(), h.ph_g0.size() * 4);
    if (e == hipSuccess) e = L->list_ptr.upload(h.ph_list_ptr.data(), h.ph_list_ptr.size() * 4);
    if (e == hipSuccess) e = L->list.upload(h.xrows.data(), h.xrows.size() * 4);
    if (e == hipSuccess && one_byte) {
        std::vector<uint8_t> c8(h.col16.begin(), h.col16.end());
        e = L->idx.upload(c8.data(), c8.size());
    } else if (e == hipSuccess) e = L->idx.upload(h.col16.data(), h.col16.size() * 2);
    L->idx_bytes = one_byte ? 1 : 2;
    L->max_rows = h.max_rows_used; L->n_phases = h.n_phases; L->rows_staged = (int64_t)h.xrows.size() << h.line_shift;
    return e;
}

// the entries once more, group-major like the phased plan's indices (what scs_spmmv_quadph streams)
std::vector<unsigned char> group_major_values(const uspmv_scs *src, const uspmv_phased_plan &pp) {
    const size_t vs = value_bytes(src->dtype);
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
    return gv;
}

int part_build(uspmv_dmat *A, int order, int rows_per_flag, const unsigned char *d_flags) {
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

}  // namespace

namespace uspmv_dev {

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

extern "C" {

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
    const size_t vs = value_bytes(s->dtype), row_bytes = (size_t)block_vec_size * vs;
    if (!width_gets_plan(row_bytes, s->C)) return USPMV_OK;
    const size_t cap = g_tune.spmmv_lds_kb > 0 ? std::min<size_t>((size_t)g_tune.spmmv_lds_kb * 1024, BT_LDS_CAP) : BT_LDS_CAP;
    const int max_rows = (int)(cap / row_bytes);
    const int tile_rows = plan_tile_rows(row_bytes, s->C);
    uspmv_tlc_plan p;
    uspmv_scs r;                       // private copy with the sigma sort's ties undone (only kept when rows moved)
    std::vector<int32_t> row_map;
    const bool moved = g_tune.spmmv_reorder && (g_tune.spmmv_reorder == 3 ? uspmv_scs_reorder_bricks(s, g_tune.spmmv_brick_stride, g_tune.spmmv_brick_lines, &r, &row_map)
                                                                          : uspmv_scs_reorder_rows(s, g_tune.spmmv_reorder == 2 ? 2 : (g_tune.spmmv_reorder == 4 && !g_tune.spmmv_xline) ? 4 : 1, &r, &row_map)) == 1;
    // (with the line plan requested -- "spmmv_xline": X staged by 128-byte lines of the column-major vector -- the rows stay in original order,
    //  ties undone: a patch of several mesh lines touches more LINES of X than a run of consecutive rows)
    const uspmv_scs *src = moved ? &r : s;
    // The phased plan over the same (re-ordered) entries.  When the phased kernel can take it, the one-list-per-tile plan of the older
    // kernels and its column-major copy of the entries (8 + 6 bytes per non-zero of HBM, a second or two of planning) are only built on
    // request ("spmmv_list_plan" 1).
    uspmv_phased_plan pp;
    if (wants_phased(row_bytes, tile_rows))
        if (int rc = uspmv_build_phased_plan(src, g_tune.spmmv_phase_rows, PHASE_GROUPS, &pp, 0, g_tune.spmmv_phase_dp)) return rc;
    const bool phased_ok = phased_kernel_takes(pp);
    // ... and once more with LINE lists for column-major block vectors (no re-layout pass over X)
    uspmv_phased_plan pl;
    if (phased_ok && wants_line_plan()) {
        const int shift = s->dtype == USPMV_F64 ? 4 : 5;
        if (int rc = uspmv_build_phased_plan(src, PHASE_ROWS_IDX8, PHASE_GROUPS, &pl, shift)) return rc;
        if (verbose()) {
            int64_t over = 0;
            for (int64_t ph = 0; ph < pl.n_phases; ++ph) over += (pl.ph_list_ptr[(size_t)ph + 1] - pl.ph_list_ptr[(size_t)ph]) > (PHASE_ROWS_IDX8 >> shift);
            fprintf(stderr, "[uspmv] line plan candidate: valid=%d phases=%lld lines_total=%zu (= %zu rows; row plan stages %zu) max_rows=%d phases over the cap: %lld\n",
                    (int)pl.valid, (long long)pl.n_phases, pl.xrows.size(), pl.xrows.size() << shift, pp.xrows.size(), pl.max_rows_used, (long long)over);
        }
        pl.valid = keep_line_plan(pl, pp, shift);
    }
    // ... and once more over ORIGINAL X-row numbering (column index c -> new_to_old[c]) for column-major callers: their re-layout pass
    // undoes the sigma permutation on the way, so the rows a tile needs are runs of the workspace again
    uspmv_phased_plan pu;
    const bool have_perm = host_values && s->sigma > 1 && (int64_t)s->new_to_old_idx.size() >= s->n_rows && (int64_t)s->old_to_new_idx.size() >= s->n_rows;
    if (phased_ok && have_perm && wants_unscrambled_plan(pp)) {
        uspmv_scs u;                                    // indices only: a struct with the renumbered columns
        u.C = src->C; u.sigma = src->sigma; u.n_rows = src->n_rows; u.n_cols = src->n_cols; u.n_rows_padded = src->n_rows_padded; u.n_chunks = src->n_chunks;
        u.n_elements = src->n_elements; u.nnz = src->nnz; u.dtype = src->dtype;
        u.chunk_ptrs = src->chunk_ptrs; u.chunk_lengths = src->chunk_lengths;
        u.col_idxs.resize(src->col_idxs.size());
        const int32_t *n2o = s->new_to_old_idx.data();
        const int64_t nr = s->n_rows;
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < (int64_t)src->col_idxs.size(); ++k) { const int32_t c = src->col_idxs[(size_t)k]; u.col_idxs[(size_t)k] = c < nr ? n2o[c] : c; }
        if (int rc = uspmv_build_phased_plan(&u, PHASE_ROWS_IDX8, PHASE_GROUPS, &pu, 0, g_tune.spmmv_phase_dp)) return rc;
        pu.valid = keep_unscrambled_plan(pu);
    }
    const bool list_plan = !phased_ok || g_tune.spmmv_list_plan;
    if (list_plan) {
        if (int rc = uspmv_build_tlc_plan(src, nullptr, max_rows, tile_rows, &p, /*line_shift=*/0)) return rc;
        if (n_tiles) *n_tiles = p.n_tiles;
        if (n_staged) *n_staged = p.valid ? p.n_staged_tiles : 0;
        if (verbose()) fprintf(stderr, "[uspmv] block plan: b=%d tile_rows=%d tiles=%lld staged=%lld max_rows=%d (cap %d) rows_total=%zu\n",
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
            if (host_values) e = A->bt.values.upload(r.values_ptr(), (size_t)r.n_elements * vs);
            else {
                e = A->bt.values.alloc(std::max<size_t>((size_t)r.n_elements, 1) * vs);
                if (e == hipSuccess && launch_block_values_gather(A, A->bt.row_map, nullptr, A->bt.values, false, nullptr) != USPMV_OK) e = hipErrorUnknown;
            }
            if (e == hipSuccess && (p.n_staged_tiles < p.n_tiles || g_tune.spmmv_variant == 5)) e = A->bt.cols.upload(r.col_idxs.data(), (size_t)r.n_elements * 4);
        }
    }
    if (e == hipSuccess && pp.valid) {
        e = upload_phase_lists(pp, one_byte_indices(pp), &A->pb.lists);
        if (e == hipSuccess) e = A->pb.c16_ptrs.upload(pp.c16_ptrs.data(), pp.c16_ptrs.size() * 4);
        if (e == hipSuccess && !host_values) {
            e = A->pb.values.zeros(std::max<size_t>(pp.col16.size(), 1) * vs);     // padded slots of the last group of a chunk
            if (e == hipSuccess && launch_block_values_gather(A, moved ? A->bt.row_map : nullptr, A->pb.c16_ptrs, A->pb.values, true, nullptr) != USPMV_OK) e = hipErrorUnknown;
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        } else if (e == hipSuccess) {
            const std::vector<unsigned char> gv = group_major_values(src, pp);
            e = A->pb.values.upload(gv.data(), gv.size());
        }
        if (verbose()) fprintf(stderr, "[uspmv] phased block plan: tiles=%lld phases=%lld rows_total=%zu max_rows=%d (cap %d)\n",
                               (long long)pp.n_tiles, (long long)pp.n_phases, pp.xrows.size(), pp.max_rows_used, pp.cap_rows);
        if (e == hipSuccess && pu.valid) {
            e = upload_phase_lists(pu, true, &A->pu.lists);
            if (e == hipSuccess) e = A->pu.perm.upload(s->old_to_new_idx.data(), (size_t)s->n_rows * 4);
            if (verbose()) fprintf(stderr, "[uspmv] unscrambled plan (column-major X behind the permuting re-layout): phases=%lld rows_total=%zu (scrambled: %zu) max_rows=%d\n",
                                   (long long)pu.n_phases, pu.xrows.size(), pp.xrows.size(), pu.max_rows_used);
        }
        if (e == hipSuccess && pl.valid) {
            e = upload_phase_lists(pl, true, &A->pl.lists);
            if (verbose()) fprintf(stderr, "[uspmv] line plan (column-major X): phases=%lld lines_total=%zu (= %zu rows) max_rows=%d\n",
                                   (long long)pl.n_phases, pl.xrows.size(), pl.xrows.size() << pl.line_shift, pl.max_rows_used);
        }
    }
    if (e != hipSuccess) {
        block_plan_reset(A);
        return uspmv::fail(USPMV_ERR_ALLOC, "uspmv_dmat_optimize_block: device copy failed: %s", hipGetErrorString(e));
    }
    if (pp.valid && pu.valid) { A->pu.on = true; A->pu.n_perm = s->n_rows; }
    if (pp.valid && pl.valid) { A->pl.on = true; A->pl.shift = pl.line_shift; }
    if (pp.valid) { A->pb.on = true; A->pb.cap_rows = pp.cap_rows; A->pb.ngp = pp.ngp; A->pb.n_tiles = pp.n_tiles; }
    if (list_plan && p.valid) { A->bt.on = true; A->bt.tile_rows = p.tile_rows; A->bt.max_rows = p.max_lines_used; A->bt.n_tiles = p.n_tiles; A->bt.staged = p.n_staged_tiles; }
    if (A->pb.on && g_tune.spmmv_stream > 0) return dmat_stream_schedule(A, g_tune.spmmv_stream);
    return USPMV_OK;
}

// The phased block plan built entirely on the device (csrc/block_plan_kernels.hip): row order, phases, X-row lists, one-byte indices and
// the group-major value copy; the host sees the chunk lengths (offsets of the index array) and two integers per tile (exclusive scans).
// Returns 1 when the shape / tuning is not the default one this builder covers (the caller then plans the index part on the host).
static int block_plan_install_device(uspmv_dmat_t *A, int block_vec_size, int64_t *n_tiles, int64_t *n_staged) {
    const size_t vsz = value_bytes(A->dtype);
    if (!device_builder_covers((size_t)block_vec_size * vsz, A->C)) return 1;
    const int64_t C = A->C, nc = A->n_chunks, n_pad = nc * C, nt = (n_pad + 63) / 64;
    block_plan_reset(A);
    auto &L = A->pb.lists;
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
    if (!rc) rc = launch_block_phase_plan(A, false, PHASE_ROWS_IDX8, PHASE_GROUPS, rmap, A->pb.c16_ptrs, d_tph, d_tl, nullptr, nullptr, nullptr, nullptr, d_max, nullptr);
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
    e = L.ph_ptr.upload(tph.data(), 4 * ((size_t)nt + 1));
    if (e == hipSuccess) e = hipMemcpy(d_tl, tl.data(), 4 * (size_t)nt, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = L.g0.alloc(4 * (size_t)n_ph);
    if (e == hipSuccess) e = L.list_ptr.alloc(4 * ((size_t)n_ph + 1));
    if (e == hipSuccess) e = L.list.alloc(4 * (size_t)std::max<int64_t>(n_list, 1));
    if (e == hipSuccess) e = L.idx.zeros((size_t)std::max<int64_t>(tot16, 1));
    if (e == hipSuccess) { const int32_t last = (int32_t)n_list; e = hipMemcpy(L.list_ptr + n_ph, &last, 4, hipMemcpyHostToDevice); }
    if (e == hipSuccess) e = A->pb.values.zeros((size_t)std::max<int64_t>(tot16, 1) * vsz);
    if (e != hipSuccess) return fail_out("plan arrays");
    rc = launch_block_phase_plan(A, true, PHASE_ROWS_IDX8, PHASE_GROUPS, rmap, A->pb.c16_ptrs, L.ph_ptr, d_tl, L.g0, L.list_ptr, L.list, (unsigned char *)L.idx, d_max, nullptr);
    if (!rc) rc = launch_block_values_gather(A, rmap, A->pb.c16_ptrs, A->pb.values, true, nullptr);
    int max_rows = 0;
    if (!rc) { e = hipMemcpy(&max_rows, d_max, 4, hipMemcpyDeviceToHost); if (e != hipSuccess) return fail_out("plan kernels"); }
    d_changed.reset(); d_tph.reset(); d_tl.reset();
    if (rc) { block_plan_reset(A); return rc; }
    L.idx_bytes = 1; L.max_rows = max_rows; L.n_phases = n_ph; L.rows_staged = n_list;
    A->pb.on = true; A->pb.device_built = true; A->pb.cap_rows = PHASE_ROWS_IDX8; A->pb.ngp = PHASE_GROUPS; A->pb.n_tiles = nt;
    if (verbose()) fprintf(stderr, "[uspmv] phased block plan (device builder): tiles=%lld phases=%lld rows_total=%lld max_rows=%d rows %s\n",
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

// The block-vector column-window sweep plan (host/sweep_plan.cpp: uspmv_build_block_sweep_plan; kernel csrc/spmmv_sweep.hip) for 64-byte X
// rows.  Installed only when EVERY tile sweeps (rows column-sorted at window granularity, staging within "sweep_max_stage" bytes
// per non-zero); otherwise the handle keeps whatever block plan it has.  wlog / tile_rows 0 = defaults (2^11 rows = 128 KiB windows, one
// buffer; the rows per tile of the sweep plan over vectors, sweep_planner.hip).
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
    const size_t vsz = value_bytes(s->dtype);
    if ((size_t)block_vec_size * vsz != 64) return USPMV_OK;                 // the kernel is written for 64-byte X rows
    // defaults: the largest window (2^11 rows = 128 KiB, one buffer) and 4 096-row tiles measured best on the Queen_4147-class matrix
    // (0.998 / 1.016 ms row- / column-wise; 2^9-row windows with two buffers 1.26 / 1.29: profiles/r04/spmmv_sweep_probe.txt)
    if (wlog <= 0) wlog = 11;
    if (((size_t)1 << wlog) * 64 > WG_LDS_BYTES) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_block_sweep: a window of 2^%d rows does not fit the LDS", wlog);
    if (tile_rows <= 0) tile_rows = sweep_default_tile_rows(s->n_chunks * s->C);
    uspmv_block_sweep_plan p;
    if (int rc = uspmv_build_block_sweep_plan(s, wlog, tile_rows, 64, sweep_max_stage(), &p)) return rc;
    if (n_tiles) *n_tiles = p.n_tiles;
    if (n_sweep) *n_sweep = p.valid ? p.n_sweep_tiles : 0;
    if (verbose())
        fprintf(stderr, "[uspmv] block sweep plan: tile_rows=%d wlog=%d tiles=%lld sweep=%lld rest_chunks=%zu elements=%zu windows staged=%lld (%.2f X rows per matrix row) cnt_bytes=%zu\n",
                p.tile_rows, p.wlog, (long long)p.n_tiles, (long long)p.n_sweep_tiles, p.rest_chunks.size(), p.idx.size(), (long long)p.windows_staged,
                (double)p.windows_staged * (double)((int64_t)1 << p.wlog) / (double)std::max<int64_t>(s->n_chunks * s->C, 1), p.cnt.size());
    if (!p.valid || p.n_sweep_tiles != p.n_tiles || !p.rest_chunks.empty()) return USPMV_OK;
    hipError_t e = A->bw.tile_ids.upload(p.tile_ids.data(), p.tile_ids.size() * 4);
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

// FNV-1a digests of the phased block plan's device arrays (tests: device-built == host-planned)
int uspmv_dmat_block_plan_digest(const uspmv_dmat_t *A0, uint64_t digest[8]) {
    if (int rc = check_dmat(A0, "uspmv_dmat_block_plan_digest")) return rc;
    if (!digest) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_block_plan_digest: NULL argument");
    const uspmv_dmat_t *A = (A0->alt && g_tune.rechunk) ? A0->alt : A0;
    for (int k = 0; k < 8; ++k) digest[k] = 0;
    if (!A->pb.on) return USPMV_OK;
    const auto &L = A->pb.lists;
    const size_t nt = (size_t)A->pb.n_tiles, nph = (size_t)L.n_phases, nc = (size_t)A->n_chunks;
    int32_t n_list = 0;
    uint32_t tot16 = 0;
    HIP_TRY(hipMemcpy(&n_list, L.list_ptr + nph, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&tot16, A->pb.c16_ptrs + nc, 4, hipMemcpyDeviceToHost));
    int rc = device_fnv(L.ph_ptr, (nt + 1) * 4, &digest[0]);
    if (!rc) rc = device_fnv(L.g0, nph * 4, &digest[1]);
    if (!rc) rc = device_fnv(L.list_ptr, (nph + 1) * 4, &digest[2]);
    if (!rc) rc = device_fnv(L.list, (size_t)n_list * 4, &digest[3]);
    if (!rc) rc = device_fnv(A->pb.c16_ptrs, (nc + 1) * 4, &digest[4]);
    if (!rc) rc = device_fnv(L.idx, (size_t)tot16 * (size_t)L.idx_bytes, &digest[5]);
    if (!rc) rc = device_fnv(A->pb.values, (size_t)tot16 * value_bytes(A->dtype), &digest[6]);
    if (!rc) rc = device_fnv(A->bt.row_map, A->bt.row_map ? nc * (size_t)A->C * 4 : 0, &digest[7]);
    return rc;
}

int uspmv_dmat_block_plan_staged(const uspmv_dmat_t *A, int64_t *rows_staged) {
    if (!A || !rows_staged) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_block_plan_staged: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    *rows_staged = M->pb.on ? M->pb.lists.rows_staged : 0;
    return USPMV_OK;
}

int uspmv_dmat_block_plan_info(const uspmv_dmat_t *A, int64_t meta[10]) {
    if (!A || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_block_plan_info: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    meta[0] = M->bt.on; meta[1] = M->pb.on; meta[2] = M->pl.on; meta[3] = M->pb.n_tiles; meta[4] = M->pb.lists.n_phases; meta[5] = M->pl.lists.n_phases;
    meta[6] = M->pl.lists.rows_staged; meta[7] = M->pb.lists.idx8(); meta[8] = M->pb.device_built; meta[9] = M->pb.lists.max_rows;
    return USPMV_OK;
}

int uspmv_dmat_stream_info(const uspmv_dmat_t *A, int64_t meta[2]) {
    if (!A || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_stream_info: NULL argument");
    const uspmv_dmat_t *M = (A->alt && g_tune.rechunk) ? A->alt : A;
    meta[0] = M->ps.desc ? M->ps.grid : 0; meta[1] = M->ps.desc ? M->ps.n_desc : 0;
    return USPMV_OK;
}

}  // extern "C"
