// The SpMV planner: uspmv_dmat_optimize and its variants (one struct, the ap[dp_sp] pair, the splits with an fp16 part; from a host
// struct through host/tlc_plan.cpp or from the handle's device arrays through plan_kernels.hip).  Every decision between the plans
// -- the line budget, the rows per tile, when the element plan or the column-window sweep takes over -- is a predicate written once, and
// so is their sequence: plan_parts runs lines -> elements -> sweep -> keep or drop for every entry.  What differs between the host and
// the device planner is a source (HostSource, DeviceSource: how a candidate is built and reaches the handles), what differs between the
// kinds a row of POLICY (PartsPolicy); the public entries are argument checks and one call.  tests/test_gpu_planner_routes.py pins every
// entry's route and plan, tests/test_gpu_parity.py and tests/test_gpu_elem_plan_device.py compare the two planners array for array.
// Outside the driver stays what only a single struct has: the internal C = 32 re-chunking, the 12-bit indices, the additive chunk records,
// and (a hook of the host source, tried before the sweep) the element plan on rows dealt to the tiles by the matrix graph.
#include "uspmv_device.hpp"

#include <mutex>

using namespace uspmv_dev;

namespace {

bool verbose() {
    static const bool on = getenv("USPMV_VERBOSE") != nullptr;
    return on;
}

// Most x lines (of 16 values) a tile may list.  The caller's wish, 512 when it has none (64 KiB of doubles: 2 workgroups per CU at worst)
// -- the term that binds by default.  A larger wish stops at what 160 KiB of LDS hold in the value type of the first part (1280 lines of
// doubles, 2560 of floats), and a plan shared by the parts of an ap split at 1280 whatever that type is (binds for a float first part).
// 4096 lines x 16 values are all that a 16-bit local index can address: below the LDS term for both types, so it never binds.
int line_budget(int max_lines, int dtype_of_first_part, bool shared) {
    const int lds = (int)(160 * 1024 / (16 * (dtype_of_first_part == USPMV_F64 ? 8 : 4)));
    return std::min({max_lines <= 0 ? 512 : max_lines, lds, shared ? 1280 : 4096});
}

// rows per tile of the next tile-local-column plan (g_tune.tlc_tile_rows = 0: by kind)
int plan_tile_rows(bool ap) { return g_tune.tlc_tile_rows ? g_tune.tlc_tile_rows : (ap ? 512 : 256); }

// Rows per tile by what the 256-row plan turned out to be (tuning tlc_auto_tile, default on; only when tlc_tile_rows is 0).  The x lines
// of a tile live in LDS (128 B each): when the largest 256-row tile needs more than 250 of them, at most 4 workgroups = 16 waves fit a
// CU, too few to cover the staging latency, and every line is fetched by several neighbouring tiles.  1024-row tiles (or 512-row ones)
// fetch each line fewer times and keep 32 (16) waves per CU when their lines still fit; they are taken when they stage >= 99 % of the
// tiles.  Measured (tools/tile_rows_sweep.py, profiles/r03/tile_rows_sweep.txt): KKT N = 200 0.82 -> 0.73 ms, banded 30 per row over
// +-2000 columns 0.27 -> 0.22 ms; matrices whose 256-row tiles need <= 217 lines (all the stencils) are fastest at 256 and stay there.
bool tile_rows_grow(int rows, int lines_used) { return g_tune.tlc_auto_tile && g_tune.tlc_tile_rows == 0 && rows == 256 && lines_used > 250; }
bool tile_rows_accept(int64_t n_tiles, int64_t n_staged) { return n_staged * 100 >= n_tiles * 99; }

// How much of a plan stages, by the thresholds the decisions below use: a line plan under nine tenths leaves "a tenth of the tiles or more
// to the gather path" (the element plans are tried); 19 of 20 is enough for the plan on dealt rows (what would run instead is 2 x
// slower); under half, the column-window sweep is tried (sweep_takes_over), and a shared plan with an fp16 part is not worth keeping.
bool stages_nine_tenths(int64_t n_tiles, int64_t n_staged) { return n_staged * 10 >= n_tiles * 9; }
bool stages_19_of_20(int64_t n_tiles, int64_t n_staged) { return n_staged * 20 >= n_tiles * 19; }
bool stages_half(int64_t n_tiles, int64_t n_staged) { return n_staged * 2 >= n_tiles; }
// shared line plan of the two or three parts of a split with an fp16 part: kept where it stages at least half of the tiles
bool ap_hp_plan_worth(int64_t n_tiles, int64_t n_staged) { return n_staged > 0 && stages_half(n_tiles, n_staged); }

// the internal C = 32 re-chunking of a narrow struct is taken when its padding stays within a quarter (+ 4096) of the entries
bool rechunk_worth(int64_t new_elements, int64_t old_elements) {
    return (double)new_elements <= 1.25 * (double)std::max<int64_t>(old_elements, 1) + 4096;
}

// what a plan candidate (over lines at some rows per tile, or over single x elements) turned out to be
struct PlanStats {
    bool valid = false;
    int64_t n_tiles = 0, n_staged = 0;
    int lines = 0;                       // list entries of the fullest tile
    int64_t listed = 0;                  // ... of all lists together
};
PlanStats stats_of(const uspmv_tlc_plan &p) { return {p.valid, p.n_tiles, p.n_staged_tiles, p.max_lines_used, (int64_t)p.tile_lines.size()}; }

// The rows per tile, for the host and the device planner alike: the measured verdict when there is one, else R0 (the default by kind),
// else -- where the kind grows its tiles and tile_rows_grow asks for it -- the first of 1024 and 512 rows that tile_rows_accept takes.
// src.line(R, &stats) builds a candidate at R rows, src.keep() makes the last candidate the plan; *st describes the plan kept.
template <typename Source>
int plan_at_chosen_rows(int R_meas, int R0, bool grow, Source &src, PlanStats *st) {
    if (R_meas) R0 = R_meas;
    if (int rc = src.line(R0, st)) return rc;
    src.keep();
    if (R_meas || !grow || !st->valid || !tile_rows_grow(R0, st->lines)) return USPMV_OK;
    for (int R : {1024, 512}) {
        PlanStats q;
        if (int rc = src.line(R, &q)) return rc;
        if (q.valid && tile_rows_accept(q.n_tiles, q.n_staged)) { src.keep(); *st = q; break; }
    }
    return USPMV_OK;
}

// The metadata every part of a plan carries.  Parts planned together share one non-zero id (the ap launchers check it); a single struct has 0.
void stamp_plan(uspmv_dmat *const parts[3], int tile_rows, int max_lines, int64_t x_len, int64_t n_tiles, int64_t staged, bool elem) {
    static uint64_t next_plan_id = 1;
    const uint64_t id = parts[1] ? next_plan_id++ : 0;
    for (int k = 0; k < 3; ++k) {
        if (!parts[k]) continue;
        auto &t = parts[k]->tlc;
        t.on = true; t.elem = elem; t.tile_rows = tile_rows; t.max_lines = max_lines; t.x_len = x_len; t.n_tiles = n_tiles; t.staged = staged; t.plan_id = id;
    }
}

// a host-built plan onto the handles: line list and local indices with the first part, the further parts their local indices only
int install_host_plan(uspmv_dmat *const parts[3], const uspmv_tlc_plan &p, bool elem, const char *who) {
    auto &t = parts[0]->tlc;
    hipError_t e = t.line_ptr.upload(p.tile_line_ptr.data(), p.tile_line_ptr.size() * 4);
    if (e == hipSuccess) e = t.lines.upload(p.tile_lines.data(), p.tile_lines.size() * 4);
    const std::vector<uint32_t> *ptrs[3] = {&p.c16_ptrs, &p.c16_ptrs_b, &p.c16_ptrs_c};
    const std::vector<uint16_t> *cols[3] = {&p.col16, &p.col16_b, &p.col16_c};
    for (int k = 0; k < 3; ++k) {
        if (!parts[k]) continue;
        if (e == hipSuccess) e = parts[k]->tlc.c16_ptrs.upload(ptrs[k]->data(), ptrs[k]->size() * 4);
        if (e == hipSuccess) e = parts[k]->tlc.col16.upload(cols[k]->data(), cols[k]->size() * 2);
    }
    if (e != hipSuccess) {
        for (int k = 0; k < 3; ++k) if (parts[k]) parts[k]->tlc = {};
        return uspmv::fail(USPMV_ERR_ALLOC, "%s: device copy failed: %s", who, hipGetErrorString(e));
    }
    stamp_plan(parts, p.tile_rows, p.max_lines_used, p.x_len_min, p.n_tiles, p.n_staged_tiles, elem);
    return USPMV_OK;
}

// Wide, irregular rows: most tiles touch too many x lines to stage them.  When the plan stages fewer than half of its tiles, try the
// column-window sweep (from the host structs, or -- ss == nullptr -- built on the device as well); *took: it covers at least half of its
// tiles and stays on the handles.  One struct, the ap[dp_sp] pair and the splits with an fp16 part alike: ms / ss hold the n parts.
int sweep_takes_over(uspmv_dmat *const ms[], const uspmv_scs *const ss[], int n, const PlanStats &st, const char *who, bool *took) {
    *took = false;
    for (int k = 0; k < n; ++k) ms[k]->sw = {};
    if (!g_tune.sweep || (st.valid && stages_half(st.n_tiles, st.n_staged))) return USPMV_OK;
    int64_t swt = 0, sws = 0;
    if (int rc = ss ? sweep_plan_install(ms, ss, n, 0, 0, &swt, &sws, who) : sweep_plan_install_device(ms, n, 0, 0, &swt, &sws, who)) return rc;
    *took = ms[0]->sw.on && stages_half(swt, sws);
    if (!*took) for (int k = 0; k < n; ++k) ms[k]->sw = {};
    return USPMV_OK;
}

// The plan's local indices once more in 12 bits (single structs whose tiles list at most 256 lines, i.e. local indices below 4096; even C):
// what scs_spmv_tlc then streams instead of the 16-bit array -- 1.5 instead of 2 bytes per non-zero.  The 16-bit array stays (the
// adaptive-precision kernels, uspmv_dmat_plan_download and the plan digests read it).  cl: the chunk lengths when the caller has them on
// the host, else they are copied back (4 bytes per chunk).
// (the two rules of tlc_pack12, for the additive records' byte count as well: can the 12-bit array be built, is it kept)
bool pack12_applies(bool elem, int max_lines, int64_t C, int64_t n_chunks) {
    return g_tune.tlc_idx12 && !(elem ? max_lines > 4096 : max_lines > 256) && C >= 2 && C % 2 == 0 && n_chunks >= 1;
}
bool pack12_kept(int64_t n_elements, int64_t padded_rows) { return g_tune.tlc_idx12 == 2 || !((double)n_elements < 8.0 * (double)padded_rows); }
// dwords of a chunk's 12-bit indices / ushorts of its 16-bit ones
int64_t c12_dwords(int64_t L, int64_t C) { const int64_t ngt = (L + 3) / 4; return (ngt / 2) * 3 * C + (ngt & 1) * (C + C / 2); }

int tlc_pack12(uspmv_dmat *A, const std::vector<int32_t> *cl, const char *who) {
    if (!A->tlc.on || !pack12_applies(A->tlc.elem, A->tlc.max_lines, A->C, A->n_chunks)) return USPMV_OK;
    std::vector<int32_t> own;
    if (!cl || (int64_t)cl->size() != A->n_chunks) {
        own.resize((size_t)A->n_chunks);
        HIP_TRY(hipMemcpy(own.data(), A->chunk_lengths, 4 * (size_t)A->n_chunks, hipMemcpyDeviceToHost));
        cl = &own;
    }
    const int64_t C = A->C, nc = A->n_chunks;
    std::vector<uint32_t> p12((size_t)nc + 1);
    int64_t tot = 0;                                             // dwords
    for (int64_t c = 0; c < nc; ++c) {
        p12[(size_t)c] = (uint32_t)tot;
        tot += c12_dwords((*cl)[(size_t)c], C);
        if (tot > (int64_t)UINT32_MAX) return USPMV_OK;          // (too large for 32-bit offsets: the 16-bit array serves)
    }
    p12[(size_t)nc] = (uint32_t)tot;
    hipError_t e = A->tlc.c12_ptrs.upload(p12.data(), 4 * ((size_t)nc + 1));
    if (e == hipSuccess) e = A->tlc.col12.alloc(4 * (size_t)std::max<int64_t>(tot, 1));
    if (e == hipSuccess && launch_plan_pack12(A, A->tlc.c16_ptrs, A->tlc.col16, A->tlc.c12_ptrs, A->tlc.col12, nullptr) != USPMV_OK) e = hipErrorUnknown;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        A->tlc.c12_ptrs.reset(); A->tlc.col12.reset();
        return uspmv::fail(USPMV_ERR_HIP, "%s: packing the local indices to 12 bits failed: %s", who, hipGetErrorString(e));
    }
    // Keep it?  Rows of a dozen entries gain or lose a per cent either way (one more load instruction per row for an odd last group), long
    // rows gain 1-15 % depending on matrix and box (profiles/r04/idx12_probe_*.txt: the 253^3 stencil 0.763 -> 0.691 ms on a slow box, 0.710 ->
    // 0.700 on a fast one; 304^3 between -15 % and +2 %).  The rule is a fixed one -- mean row length >= 8 -- and not a timing on the spot
    // (which was built first): a bench run, its counter passes and its profiler run must execute the same kernel, and a 1-2 % verdict
    // flips under a profiler's overhead.  "tlc_idx12" 2 keeps it regardless, 0 never builds it.
    if (!pack12_kept(A->n_elements, nc * C)) { A->tlc.c12_ptrs.reset(); A->tlc.col12.reset(); }
    return USPMV_OK;
}

// Additive chunk records (host/tlc_plan.cpp: uspmv_build_additive_plan) beside the local indices of a kept line plan: eligibility, the
// keep rule and the install.  Eligible: one struct in dp or sp, the line plan on the caller's row order (not the element plan, not dealt
// rows, not the sweep), n_rows == n_cols, the permutation at hand (the struct's own, or the caller's for the internal re-chunking) and not
// a rank block of the distributed object (TlcPlanOpts::additive).
bool additive_eligible(const uspmv_scs *s, const uspmv_tlc_plan &p, bool elem, const std::vector<int32_t> *n2o) {
    if (!g_tune.tlc_additive || elem || !p.valid || p.line_shift != 4) return false;
    if (s->dtype != USPMV_F64 && s->dtype != USPMV_F32) return false;
    return s->n_rows == s->n_cols && s->n_rows > 0 && (int64_t)(n2o ? n2o->size() : s->new_to_old_idx.size()) >= s->n_rows;
}
// The keep rule, a fixed one in bytes like tlc_pack12's (a verdict timed on the spot flips under a profiler): the records of the
// tiles that carry them plus 2 bytes per column of the map, counted once, plus the tagged line lists where they are new (every entry on the
// line plan's tiles, whose own list is no longer read there; on tiles of the records' own the entries that list a line again), against the
// local indices of those tiles as the kernel would stream them otherwise (12 bits where that array is kept, else 16).  Kept at half or
// less; "tlc_additive" 2 keeps whatever could be built.
struct AdditiveBytes { int64_t fresh = 0, replaced = 0; };
AdditiveBytes additive_bytes(const uspmv_scs *s, const uspmv_additive_plan &a, bool idx12) {
    AdditiveBytes b;
    if (!a.valid) return b;
    const int64_t C = s->C, T = a.tile_rows / C;
    for (int64_t c = 0; c < s->n_chunks; ++c) {
        if (a.iv_ptr[(size_t)(c / T) + 1] == a.iv_ptr[(size_t)(c / T)]) continue;
        const int64_t L = s->chunk_lengths[(size_t)c];
        b.replaced += idx12 ? 4 * c12_dwords(L, C) : 2 * ((L + 3) / 4) * 4 * C;
    }
    b.fresh = a.rec_bytes + 2 * (int64_t)a.map16.size() + 4 * (a.own_tiles ? a.n_entries_again : (int64_t)a.lines.size());
    return b;
}
// Rows per tile of the records.  In pre-sort order all rows of a sigma window reach into the same intervals (the stencil: window + 2 lines per
// plane), so a tile that is a whole window stages them once where two half-window tiles stage them twice: 0.695 against 0.804 ms on the 253^3
// stencil, whose line plan is fastest at 256 rows.  Windows of 512 or 1024 rows that are larger than the line plan's tiles.
int additive_tile_rows(const uspmv_scs *s, int line_plan_rows) {
    return (s->sigma == 512 || s->sigma == 1024) && s->sigma > line_plan_rows && s->sigma % s->C == 0 ? (int)s->sigma : line_plan_rows;
}
// ... and at most five intervals per tile on average.  The stencils have 4.0 (three planes and the padding column) and gain 3-10 %; the KKT
// matrix has 7.1 and ran 16 % slower on its records although they are a fifth of its local indices, when every staged element was still
// looked up in all of its tile's intervals (tools/additive_probe.py; with the tagged line lists: DESIGN 9.11).
bool additive_kept(const uspmv_additive_plan &a, const AdditiveBytes &b) {
    if (!a.valid || g_tune.tlc_additive == 2) return a.valid;
    return 2 * b.fresh <= b.replaced && (int64_t)(a.iv.size() / 4) <= 5 * a.n_add_tiles;
}

int tlc_additive_install(uspmv_dmat *A, const uspmv_scs *s, const uspmv_tlc_plan &p, int max_lines, const std::vector<int32_t> *n2o, const char *who) {
    if (!A->tlc.on || !additive_eligible(s, p, A->tlc.elem, n2o)) return USPMV_OK;
    uspmv_additive_plan a;
    if (int rc = uspmv_build_additive_plan(s, &p, max_lines * 16, &a, n2o, additive_tile_rows(s, p.tile_rows))) return rc;
    const AdditiveBytes b = additive_bytes(s, a, A->tlc.col12 != nullptr);
    if (verbose()) fprintf(stderr, "[uspmv] additive chunk records: valid=%d tiles=%lld of %lld chunks=%lld additive=%lld max_elems=%d tile_rows=%d records+map=%lld B against %lld B of local indices (columns %s) -> %s\n",
                           (int)a.valid, (long long)a.n_add_tiles, (long long)a.n_tiles, (long long)a.n_chunks, (long long)a.n_additive, a.max_elems, a.tile_rows, (long long)b.fresh,
                           (long long)b.replaced, a.cols_permuted ? "permuted" : "as they are", additive_kept(a, b) ? "kept" : "dropped");
    if (!additive_kept(a, b)) return USPMV_OK;
    auto &t = A->tlc;
    hipError_t e = t.add_iv_ptr.upload(a.iv_ptr.data(), a.iv_ptr.size() * 4);
    if (e == hipSuccess) e = t.add_iv.upload(a.iv.data(), a.iv.size() * 4);
    if (e == hipSuccess) e = t.add_map16.upload(a.map16.data(), a.map16.size() * 2);
    if (e == hipSuccess) e = t.add_rec.upload(a.rec.data(), a.rec.size() * 2);
    if (e == hipSuccess) e = t.add_ptrs.upload(a.rec_ptrs.data(), a.rec_ptrs.size() * 4);
    if (e == hipSuccess) e = t.add_line_ptr.upload(a.line_ptr.data(), a.line_ptr.size() * 4);
    if (e == hipSuccess) e = t.add_lines.upload(a.lines.data(), a.lines.size() * 4);
    if (e != hipSuccess) {
        t.add_line_ptr.reset(); t.add_lines.reset();
        t.add_iv_ptr.reset(); t.add_iv.reset(); t.add_map16.reset(); t.add_rec.reset(); t.add_ptrs.reset();
        return uspmv::fail(USPMV_ERR_ALLOC, "%s: device copy of the additive chunk records failed: %s", who, hipGetErrorString(e));
    }
    t.add_max_elems = a.max_elems; t.add_chunks = a.n_chunks; t.add_additive = a.n_additive;
    t.add_tile_rows = a.tile_rows; t.add_n_tiles = a.n_tiles; t.add_own_tiles = a.own_tiles; t.add_w_log = a.w_log;
    return USPMV_OK;
}

// The shape shared by the device-built plans: 256 % C == 0 and at least one chunk; *nt: tiles of R rows
bool device_plan_shape(const uspmv_dmat *A, int R, int64_t *nt) {
    if (A->C > 256 || 256 % A->C != 0 || A->n_chunks < 1) return false;
    const int64_t T = R / A->C;
    *nt = (A->n_chunks + T - 1) / T;
    return true;
}

// The count pass of a device-built plan: per tile the list entries all parts together need (0: the tile gathers), and the largest column.
// count(d_n, d_max) launches it; O(n_tiles) comes back to the host.
struct TileCounts {
    int max_col = 0;
    std::vector<int32_t> n;
};
template <typename Count>
int device_tile_counts(int64_t nt, Count count, TileCounts *o, const char *who) {
    *o = {};
    DeviceBuf<int> d_n, d_max;
    hipError_t e = d_n.alloc(4 * (size_t)nt);
    if (e == hipSuccess) e = d_max.zeros(4);
    if (e != hipSuccess) return uspmv::fail(USPMV_ERR_ALLOC, "%s: %s", who, hipGetErrorString(e));
    if (int rc = count(d_n, d_max)) return rc;
    o->n.resize((size_t)nt);
    e = hipMemcpy(o->n.data(), d_n, 4 * (size_t)nt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&o->max_col, d_max, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { o->n.clear(); return uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }
    return USPMV_OK;
}

// The install both device-built plans end in, on handles without a plan: the prefix sum over the tiles' counts and its INT32 guard, the
// offsets of every part's local indices (c16_offsets: 32-bit as well), owned buffers -- the list with the first part, every part its own
// local indices, padded slots index 0 --, the write pass write(d_c16_ptrs, d_col16), stamp_plan.  O(n_chunks) + O(n_tiles) on the host.
// No plan (and USPMV_OK) beyond 32-bit offsets and when no tile stages; on a failure the handles have none either.  *cl: the chunk
// lengths of the last part (a single struct: what tlc_pack12 takes).
template <typename Write>
int device_install_tail(uspmv_dmat *const parts[3], const TileCounts &cnt, int cap, int tile_rows, bool elem, Write write, PlanStats *st,
                        std::vector<int32_t> *cl, const char *who) {
    uspmv_dmat *const A = parts[0];
    *st = {};
    const int64_t nc = A->n_chunks, nt = (int64_t)cnt.n.size();
    std::vector<int32_t> lp((size_t)nt + 1, 0);
    int64_t staged = 0, total = 0;
    int used = 0;
    for (int64_t t = 0; t < nt; ++t) {
        const int n = cnt.n[(size_t)t] <= cap ? cnt.n[(size_t)t] : 0;         // over the cap: the tile gathers
        staged += n > 0; used = std::max(used, n);
        total += n;
        if (total > INT32_MAX) return USPMV_OK;
        lp[(size_t)t + 1] = (int32_t)total;
    }
    std::vector<uint32_t> c16p[3];
    int64_t tot16[3] = {0, 0, 0};
    cl->resize((size_t)nc);
    for (int k = 0; k < 3; ++k) {
        if (!parts[k]) continue;
        HIP_TRY(hipMemcpy(cl->data(), parts[k]->chunk_lengths, 4 * (size_t)nc, hipMemcpyDeviceToHost));
        if (!c16_offsets(*cl, A->C, &c16p[k], &tot16[k])) return USPMV_OK;
    }
    st->n_tiles = nt; st->n_staged = staged;
    if (staged == 0) return USPMV_OK;
    hipError_t e = A->tlc.line_ptr.upload(lp.data(), 4 * ((size_t)nt + 1));
    if (e == hipSuccess) e = A->tlc.lines.alloc(4 * (size_t)std::max<int64_t>(total, 1));
    const unsigned *d_c16p[3] = {nullptr, nullptr, nullptr};
    unsigned short *d_c16[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k) {
        if (!parts[k]) continue;
        if (e == hipSuccess) e = parts[k]->tlc.c16_ptrs.upload(c16p[k].data(), 4 * ((size_t)nc + 1));
        if (e == hipSuccess) e = parts[k]->tlc.col16.zeros(2 * (size_t)std::max<int64_t>(tot16[k], 1));
        d_c16p[k] = parts[k]->tlc.c16_ptrs; d_c16[k] = parts[k]->tlc.col16;
    }
    if (e == hipSuccess && write(used, d_c16p, d_c16) != USPMV_OK) e = hipErrorUnknown;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        for (int k = 0; k < 3; ++k) if (parts[k]) parts[k]->tlc = {};
        return uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    stamp_plan(parts, tile_rows, used, (int64_t)cnt.max_col + 1, nt, staged, elem);
    *st = {true, nt, staged, used, total};
    return USPMV_OK;
}

// The tile-local-column plan of parts[0] at R rows per tile, built on the device; parts[1] (the sp part of an ap pair, or the hp part of a
// two-part split) and parts[2] (the hp part of ap[dp_sp_hp]; only with parts[1]) share its line list.  No plan (and USPMV_OK) for shapes
// without one and where device_install_tail has none.  A single struct gets its 12-bit indices at once (measured_tile_rows times them).
// budget: lines a tile may list (line_budget).
int device_plan_install_rows(uspmv_dmat *const parts[3], int budget, const int R, PlanStats *st, const char *who) {
    uspmv_dmat *const A = parts[0];
    for (int k = 0; k < 3; ++k) if (parts[k]) parts[k]->tlc = {};
    *st = {};
    int64_t nt = 0;
    if (!device_plan_shape(A, R, &nt)) return USPMV_OK;
    TileCounts cnt;                                                            // (a tile over the budget counts 0 lines)
    if (int rc = device_tile_counts(nt, [&](int *d_n, int *d_max) { return launch_plan_count(parts, (long)nt, budget, d_n, d_max, R, nullptr); }, &cnt, who))
        return rc;
    std::vector<int32_t> cl;
    if (int rc = device_install_tail(parts, cnt, INT32_MAX, R, /*elem=*/false, [&](int, const unsigned *const c16p[3], unsigned short *const c16[3]) {
            return launch_plan_write(parts, (long)nt, A->tlc.line_ptr, A->tlc.lines, c16p, c16, R, nullptr);
        }, st, &cl, who))
        return rc;
    return st->valid && !parts[1] ? tlc_pack12(A, &cl, who) : USPMV_OK;
}

// For LARGE single structs the rows per tile are MEASURED (tuning tlc_measure_tile, default on; only when tlc_tile_rows is 0): the plan
// is built on the device for 256, 512 and 1024 rows (two passes over the column indices each), the kernel timed three times on a zero
// vector, and a larger tile kept when it is more than 3 % ahead of 256.  Why: which size wins depends on how far apart the x lines of
// neighbouring tiles lie -- the 27-point stencil on 253^3 is fastest at 256 rows, the same stencil on 304^3 (planes of 739 instead of
// 512 KB: more of the x lines miss the XCD's L2) at 512 (1.249 against 1.341 ms, profiles/r03/tile_rows_sweep.txt).  The choice is
// remembered per (shape, size) for the life of the process, so the host and the device planner of one matrix agree.  0 = no opinion.
int measured_tile_rows(uspmv_dmat *const parts[3], int max_lines, const char *who) {
    uspmv_dmat *const A = parts[0], *const B = parts[1];
    // one measurement at a time, and the verdict table only read / written under the lock (the verdict is keyed on the struct's shape and
    // size, not its content: two matrices with equal counts share it -- the price of host and device planner of ONE matrix agreeing)
    static std::mutex mtx;
    std::lock_guard<std::mutex> lock(mtx);
    if (!g_tune.tlc_measure_tile || g_tune.tlc_tile_rows != 0 || A->alt || A->C > 256 || 256 % A->C != 0) return 0;
    if (A->n_chunks * A->C < (int64_t)1 << 20) return 0;
    if (B && (B->alt || B->C != A->C || B->n_chunks != A->n_chunks || A->dtype != USPMV_F64 || B->dtype != USPMV_F32)) return 0;
    struct Key { int64_t nc, ne, ne2, C; int dtype, ml; };
    static std::vector<std::pair<Key, int>> seen;
    const int64_t ne2 = B ? B->n_elements : -1;
    for (auto &kv : seen)
        if (kv.first.nc == A->n_chunks && kv.first.ne == A->n_elements && kv.first.ne2 == ne2 && kv.first.C == A->C && kv.first.dtype == A->dtype && kv.first.ml == max_lines)
            return kv.second;
    const size_t vsz = A->dtype == USPMV_F64 ? 8 : 4;
    DeviceBuf<void> x, y;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int best = 0;
    auto done = [&]() {
        x.reset(); y.reset();
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        A->tlc = {};
        if (B) B->tlc = {};
    };
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { done(); (void)hipGetLastError(); return 0; }
    // the size to beat: 256 rows for one struct, 512 for an ap[dp_sp] pair (two entry streams per row, profiles/r02/ap_tile_rows.txt);
    // it is timed first and once more at the end (the first candidate may have met a cold clock)
    const int base = B ? 512 : 256;
    const int order[4] = {base, base == 256 ? 512 : 256, 1024, base};
    float tmin[3] = {0, 0, 0};                                  // best time seen for 256 / 512 / 1024 rows (0: not usable)
    auto slot_of = [](int R) { return R == 256 ? 0 : R == 512 ? 1 : 2; };
    for (int k = 0; k < 4; ++k) {
        const int R = order[k], slot = slot_of(R), bs = slot_of(base);
        if (k == 3) {                                           // re-check the base only when something is about to beat it
            bool beaten = false;
            for (int o = 0; o < 3; ++o) beaten |= o != bs && tmin[o] > 0 && tmin[bs] > 0 && tmin[o] < 0.97f * tmin[bs];
            if (!beaten) break;
        }
        PlanStats c;
        if (device_plan_install_rows(parts, max_lines, R, &c, who) != USPMV_OK || !A->tlc.on) { (void)hipGetLastError(); continue; }
        if (!tile_rows_accept(c.n_tiles, c.n_staged)) continue;
        if (!x) {
            const size_t xb = vsz * (size_t)std::max<int64_t>(A->tlc.x_len + 16, 16), yb = vsz * (size_t)std::max<int64_t>(A->n_chunks * A->C, 1);
            if (x.zeros(xb) != hipSuccess || y.alloc(yb) != hipSuccess) { done(); (void)hipGetLastError(); return 0; }
        }
        float ms = 0;
        bool ok = true;
        for (int rep = 0; rep < 2 && ok; ++rep) {             // (first round warms up)
            ok = hipEventRecord(e0, nullptr) == hipSuccess;
            for (int l = 0; l < 3 && ok; ++l) {
                if (B) ok = launch_spmv_ap(A, B, (const double *)x, nullptr, (double *)y, nullptr) == USPMV_OK;
                else ok = (A->dtype == USPMV_F64 ? launch_spmv_tlc<double>(A, nullptr, (long)A->tlc.n_tiles, (const double *)x, (double *)y, nullptr)
                                                 : launch_spmv_tlc<float>(A, nullptr, (long)A->tlc.n_tiles, (const float *)x, (float *)y, nullptr)) == USPMV_OK;
            }
            ok = ok && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        }
        if (!ok) { (void)hipGetLastError(); continue; }
        if (verbose()) fprintf(stderr, "[uspmv] measured tile size%s: %d rows -> %.4f ms per SpMV (%lld of %lld tiles staged, %d lines at most)\n", B ? " (ap pair)" : "",
                               R, ms / 3, (long long)c.n_staged, (long long)c.n_tiles, A->tlc.max_lines);
        tmin[slot] = tmin[slot] > 0 ? std::min(tmin[slot], ms) : ms;
    }
    // the base size unless another one is more than 3 % ahead of it (the fastest of those that are)
    {
        const int bs = slot_of(base);
        float tbest = tmin[bs] > 0 ? 0.97f * tmin[bs] : 1e30f;
        best = tmin[bs] > 0 ? base : 0;
        const int sizes[3] = {256, 512, 1024};
        for (int o = 0; o < 3; ++o)
            if (o != bs && tmin[o] > 0 && tmin[o] < tbest) { best = sizes[o]; tbest = tmin[o]; }
    }
    done();
    seen.push_back({Key{A->n_chunks, A->n_elements, ne2, A->C, A->dtype, max_lines}, best});
    return best;
}

// A quick look before an element plan is built in full (a sort per tile over all entries): of ~64 tiles spread over the struct, how many list more distinct
// columns than `cap`?  More than a tenth of them: the element plan would be turned down anyway (wide irregular rows: the sweep's matrices).
// The sampled tiles are t = step/2, step/2 + step, ... with step = max(1, n_tiles / 64); over(t): tile t lists more than the cap.  The host
// planner sorts those tiles' columns, the device planner reads its count pass's array at the same indices.
template <typename Over>
double sampled_over_cap_frac(int64_t nt, Over over) {
    const int64_t step = std::max<int64_t>(1, nt / 64);
    int64_t seen = 0, n_over = 0;
    for (int64_t t = step / 2; t < nt; t += step) { ++seen; n_over += over(t) ? 1 : 0; }
    return seen > 0 ? (double)n_over / (double)seen : 1.0;
}
// (ss[0 .. n): one struct, or the parts of an ap split, which share a row layout -- a tile's columns are the union over the parts)
double elements_over_cap_frac(const uspmv_scs *const ss[], int n, int cap, int tile_rows) {
    const uspmv_scs *s = ss[0];
    const int64_t C = s->C, T = std::max<int64_t>(1, tile_rows / C), nt = (s->n_chunks + T - 1) / T;
    std::vector<int32_t> cols;
    return sampled_over_cap_frac(nt, [&](int64_t t) {
        const int64_t c0 = t * T, c1 = std::min<int64_t>(c0 + T, s->n_chunks);
        cols.clear();
        for (int k = 0; k < n; ++k)
            cols.insert(cols.end(), ss[k]->col_idxs.begin() + ss[k]->chunk_ptrs[(size_t)c0], ss[k]->col_idxs.begin() + ss[k]->chunk_ptrs[(size_t)c1]);
        std::sort(cols.begin(), cols.end());
        return (int64_t)(std::unique(cols.begin(), cols.end()) - cols.begin()) > cap;
    });
}
double elements_over_cap_frac(const uspmv_scs *s, int cap, int tile_rows) { return elements_over_cap_frac(&s, 1, cap, tile_rows); }

// The element plans: most elements a tile may list (64 KiB of the value type at most), "an element serves four entries or more on
// average", and when they are tried at all: the caller gave no line budget of its own and the line plan is invalid or leaves a tenth
// of the tiles or more to the gather path.
int element_cap(int dtype) { return std::min(g_tune.tlc_elem_cap, (int)(64 * 1024 / (dtype == USPMV_F64 ? 8 : 4))); }
bool elements_pay(int64_t listed, int64_t n_elements) { return (double)listed * 4.0 <= (double)n_elements; }
bool line_plan_short(bool own_budget, const PlanStats &line) { return !own_budget && (!line.valid || !stages_nine_tenths(line.n_tiles, line.n_staged)); }

// The fallback from the line plan to the plan over single x elements on the caller's row order, for the host and the device planner alike.
// Columns scattered over many lines (x in a numbering that is only loosely related to the rows'): the line plan leaves a tenth of the tiles
// or more to the gather path.  List the tile's distinct ELEMENTS instead -- taken when (nearly) every tile fits and an element serves
// four entries or more on average (else the line plan stays, or the column-window sweep takes over).  Measured (tools/numbering_probe.py,
// profiles/r04/numbering_probe_*.txt): 27-point x 3 dof stencil with x renumbered at random inside blocks of 1 000 / 5 000 / 20 000 nodes
// 0.97 / 0.90 / 0.89 of the roofline against 0.74 (line plan, 69 % of the tiles staged) / 0.70 / 0.61 (sweep); 1 dof, 4.2 entries per
// element: 0.65 against 0.59; on a regular numbering the line plan is 20 % ahead (0.683 against 0.819 ms on the 253^3 stencil), which is
// why this is a fallback only ("tlc_elem" 2, a measurement aid, always tries).
// src.sample(cap, &frac): the share of the sampled tiles over the cap; src.elements(cap, &stats): the candidate, in full (a sort per
// tile) -- the caller installs it when *took, and the call then reports the element plan's tiles.
template <typename Source>
int elements_take_over(bool own_budget, const PlanStats &line, bool allowed, int dtype, int64_t n_elements, Source &src, bool *took,
                       int64_t *n_tiles, int64_t *n_staged) {
    *took = false;
    if (!(line_plan_short(own_budget, line) || g_tune.tlc_elem == 2) || !g_tune.tlc_elem || !allowed) return USPMV_OK;
    const int ecap = element_cap(dtype);
    double over = 1.0;
    if (int rc = src.sample(ecap, &over)) return rc;
    if (over > 0.1) return USPMV_OK;                   // would be turned down anyway (wide irregular rows: the sweep's matrices)
    PlanStats e;
    if (int rc = src.elements(ecap, &e)) return rc;
    if (!e.valid || !tile_rows_accept(e.n_tiles, e.n_staged) || !(elements_pay(e.listed, n_elements) || g_tune.tlc_elem == 2)) return USPMV_OK;
    *took = true;
    if (n_tiles) *n_tiles = e.n_tiles;
    if (n_staged) *n_staged = e.n_staged;
    if (verbose()) fprintf(stderr, "[uspmv] tlc plan over single x elements: tiles=%lld staged=%lld max_elements=%d elements_total=%lld (%.1f entries per element)\n",
                           (long long)e.n_tiles, (long long)e.n_staged, e.lines, (long long)e.listed, (double)n_elements / (double)std::max<int64_t>(e.listed, 1));
    return USPMV_OK;
}

// The parts of an ap split fall to the element plan by themselves -- "tlc_elem" 1 -- kind by kind, where it was measured faster than what
// the split runs otherwise by more than the run-to-run spread (tools/ap_numbering_probe.py, profiles/ap_elem/, DESIGN 9.9: all four kinds,
// 1.16 - 1.80 x on 1.5 M rows); "tlc_elem" 2 tries it whatever the kind and size.  ap[dp_sp] pairs do so only from 2^20 padded rows on (the
// size from which measured_tile_rows counts a struct as large): tests/test_gpu_elem_plan_device.py pins the pair of the scattered
// 40^3 x 3 dof stencil (192 000 rows) to lines -> sweep, so below that size a pair keeps those plans.
bool ap_elements_by_default(int dtype_last, int64_t padded_rows) {
    return dtype_last != USPMV_F32 || padded_rows >= (int64_t)1 << 20;   // (F32 last: ap[dp_sp]; F16 last: the kinds with an fp16 part)
}
bool ap_elements_allowed(const TlcPlanOpts &opts, const uspmv_dmat *first, const uspmv_dmat *last) {
    return opts.elements && (g_tune.tlc_elem == 2 || ap_elements_by_default(last->dtype, first->n_chunks * first->C));
}
int64_t sum_elements(uspmv_dmat *const parts[3]) {
    int64_t n = 0;
    for (int k = 0; k < 3; ++k) if (parts[k]) n += parts[k]->n_elements;
    return n;
}

// The element plan's count pass on the device (plan_kernels.hip): per 256-row tile the distinct columns -- of all parts together --
// clipped at cap + 1, and the largest column.  Shapes without a plan: no tiles.
int device_elem_count(uspmv_dmat *const parts[3], int cap, TileCounts *o, const char *who) {
    *o = {};
    int64_t nt = 0;
    if (!device_plan_shape(parts[0], 256, &nt)) return USPMV_OK;
    return device_tile_counts(nt, [&](int *d_n, int *d_max) { return launch_plan_count_elems(parts, (long)nt, cap, d_n, d_max, nullptr); }, o, who);
}

// ... and its write pass, installed on the (plan-less) handles as device_plan_install_rows installs the line plan (device_install_tail)
int device_elem_install(uspmv_dmat *const parts[3], const TileCounts &cnt, int cap, PlanStats *st, std::vector<int32_t> *cl, const char *who) {
    for (int k = 0; k < 3; ++k) if (parts[k]) parts[k]->tlc = {};
    *st = {};
    if (cnt.n.empty()) return USPMV_OK;
    return device_install_tail(parts, cnt, cap, 256, /*elem=*/true, [&](int most, const unsigned *const c16p[3], unsigned short *const c16[3]) {
        return launch_plan_write_elems(parts, (long)cnt.n.size(), most, parts[0]->tlc.line_ptr, parts[0]->tlc.lines, c16p, c16, nullptr);
    }, st, cl, who);
}

// ---- The two sources of a plan: what differs between the host and the device planner, and nothing else.  plan_parts below drives either:
//   line(R, &stats)        a line-plan candidate at R rows per tile (budget: the lines a tile may list)
//   keep()                 the last candidate is the line plan to keep
//   sample(cap, &frac)     the share of the sampled 256-row tiles that list more than cap elements
//   elements(cap, &stats)  the candidate over single x elements, in full
//   install_elements()     ... onto the handles; on a failure they carry no plan
//   dealt_rows(...)        a further element plan only this source has, tried before the sweep
//   install_line()         the kept line plan onto the handles
//   structs()              what sweep_takes_over builds from (nullptr: the handles' device arrays)

// The host structs of the parts (ss[k] the struct of parts[k]), through host/tlc_plan.cpp: candidates are host copies, and only the plan
// that is kept reaches the handles.
struct HostSource {
    uspmv_dmat *const *parts;
    const uspmv_scs *const *ss;
    const char *who;
    bool deal_rows = false;              // dmat_optimize: one struct, TlcPlanOpts::deal_rows
    int budget = 0;
    uspmv_tlc_plan p, q;                 // the plan kept, the last candidate
    uspmv_scs rr;                        // the struct on rows dealt to the tiles by the matrix graph, and its row map
    std::vector<int32_t> rr_map;
    bool dealt = false;

    int n() const { return ss[2] ? 3 : ss[1] ? 2 : 1; }
    int line(int R, PlanStats *o) {
        q = {};
        const int rc = uspmv_build_tlc_plan(ss[0], ss[1], budget, R, &q, /*line_shift=*/4, ss[2]);
        *o = stats_of(q);
        return rc;
    }
    void keep() { p = std::move(q); }
    int sample(int cap, double *over) { *over = elements_over_cap_frac(ss, n(), cap, 256); return USPMV_OK; }
    int elements(int cap, PlanStats *o) {
        q = {};
        const int rc = uspmv_build_tlc_plan(ss[0], ss[1], cap, 256, &q, /*line_shift=*/0, ss[2]);
        *o = stats_of(q);
        return rc;
    }
    int install_elements() { p = std::move(q); return install_host_plan(parts, p, /*elem=*/true, who); }
    int install_line() { return install_host_plan(parts, p, /*elem=*/false, who); }
    const uspmv_scs *const *structs() const { return ss; }

    // When the ROWS of a tile are scattered as well (rows and columns renumbered alike: a tile of 256 consecutive rows is no compact piece of the
    // mesh any more): deal the rows to the tiles by the matrix graph first, as the block plan does (uspmv_scs_reorder_rows mode 4: rows change places
    // only with rows of equal-length chunks, every row keeps its slot sequence), then the element plan on that order -- a private copy of the values
    // (8 / 4 bytes per element of HBM), of the column indices (for the few tiles that do not stage) and a row map for y.
    int dealt_rows(bool own_budget, const PlanStats &line, bool *took, int64_t *n_tiles, int64_t *n_staged) {
        const uspmv_scs *s = ss[0];
        if (!deal_rows || !line_plan_short(own_budget, line) || !g_tune.tlc_elem || !g_tune.tlc_elem_rows || s->n_rows != s->n_cols) return USPMV_OK;
        // first with the clusters confined to segments of tlc_elem_seg_rows rows (64 Ki: many segments in parallel, and a trial on a sample of them that stops
        // irregular matrices early); when that leaves some, but not most, of the sampled tiles over the cap -- related rows further apart than a segment --
        // once more with segments of 2^20 rows (a second or more of clustering per million rows on few threads: only where it looks promising)
        const int ecap = element_cap(s->dtype);
        const int64_t seg_stage[2] = {(int64_t)g_tune.tlc_elem_seg_rows, (int64_t)1 << 20};
        for (int stage = 0; stage < 2 && !dealt; ++stage) {
            if (stage == 1 && seg_stage[1] <= seg_stage[0]) break;
            if (uspmv_scs_reorder_rows(s, g_tune.tlc_elem_rows == 4 ? 4 : 2, &rr, &rr_map, g_tune.tlc_elem_rows == 4 ? 64 : 256, seg_stage[stage]) != 1) break;
            const double over = elements_over_cap_frac(&rr, ecap, 256);
            q = {};
            if (over <= 0.1)
                if (int rc = uspmv_build_tlc_plan(&rr, nullptr, ecap, 256, &q, /*line_shift=*/0)) return rc;
            if (verbose()) fprintf(stderr, "[uspmv] element plan on the graph-dealt rows (segments of %lld rows): %.0f %% of the sampled tiles over the cap; valid=%d tiles=%lld staged=%lld max_elements=%d (cap %d) elements_total=%zu\n",
                                   (long long)seg_stage[stage], 100.0 * over, (int)q.valid, (long long)q.n_tiles, (long long)q.n_staged_tiles, q.max_lines_used, ecap, q.tile_lines.size());
            // (19 of 20 tiles staged is enough here: what would run instead -- sweep or gather kernel -- is 2 x slower on such matrices)
            if (q.valid && stages_19_of_20(q.n_tiles, q.n_staged_tiles) && elements_pay((int64_t)q.tile_lines.size(), s->n_elements)) dealt = true;
            else if (over > 0.6) break;                      // most tiles far over the cap: larger segments will not repair that
        }
        if (!dealt) return USPMV_OK;
        if (int rc = install_elements()) return rc;
        if (verbose()) fprintf(stderr, "[uspmv] tlc plan over single x elements, rows dealt to the tiles by the matrix graph: tiles=%lld max_elements=%d elements_total=%zu (%.1f entries per element)\n",
                               (long long)p.n_tiles, p.max_lines_used, p.tile_lines.size(), (double)s->n_elements / (double)std::max<size_t>(p.tile_lines.size(), 1));
        auto &t = parts[0]->tlc;
        hipError_t e = t.values.upload(rr.values_ptr(), (size_t)rr.n_elements * (rr.dtype == USPMV_F64 ? 8 : 4));
        if (e == hipSuccess) e = t.row_map.upload(rr_map.data(), rr_map.size() * 4);
        if (e == hipSuccess && p.n_staged_tiles < p.n_tiles) e = t.cols.upload(rr.col_idxs.data(), (size_t)rr.n_elements * 4);
        if (e != hipSuccess) {
            t = {};
            return uspmv::fail(USPMV_ERR_ALLOC, "%s: device copy failed: %s", who, hipGetErrorString(e));
        }
        *took = true;
        if (n_tiles) *n_tiles = p.n_tiles;
        if (n_staged) *n_staged = p.n_staged_tiles;
        return USPMV_OK;
    }
};

// The handles' own device arrays, through plan_kernels.hip: every candidate is built on the handles; the line plan to keep waits in kept[]
// while the element plan is tried, and a failed element attempt puts it back.
struct DeviceSource {
    uspmv_dmat *const *parts;
    const char *who;
    int budget = 0;
    uspmv_dmat::TlcPlan kept[3];
    TileCounts cnt;
    std::vector<int32_t> cl;             // chunk lengths of the element plan's last part

    int line(int R, PlanStats *o) { return device_plan_install_rows(parts, budget, R, o, who); }
    void keep() { for (int k = 0; k < 3; ++k) if (parts[k]) { kept[k] = std::move(parts[k]->tlc); parts[k]->tlc = {}; } }
    int install_line() { for (int k = 0; k < 3; ++k) if (parts[k]) parts[k]->tlc = std::move(kept[k]); return USPMV_OK; }
    int or_line_back(int rc) { if (rc) install_line(); return rc; }
    int sample(int cap, double *over) {
        const int rc = device_elem_count(parts, cap, &cnt, who);
        *over = sampled_over_cap_frac((int64_t)cnt.n.size(), [&](int64_t t) { return cnt.n[(size_t)t] > cap; });
        return or_line_back(rc);
    }
    int elements(int cap, PlanStats *o) { return or_line_back(device_elem_install(parts, cnt, cap, o, &cl, who)); }
    int install_elements() { return or_line_back(parts[1] ? USPMV_OK : tlc_pack12(parts[0], &cl, who)); }
    int dealt_rows(bool, const PlanStats &, bool *, int64_t *, int64_t *) { return USPMV_OK; }      // (needs the host struct)
    const uspmv_scs *const *structs() const { return nullptr; }
};

// ---- What differs between the kinds, side by side.  With TlcPlanOpts::measure off every kind builds at plan_tile_rows(false), one struct's rows.
struct PartsPolicy {
    const char *kind;
    bool rows_512;           // measure on: plan_tile_rows(true) -- 512 rows per tile, two or three entry streams per row -- not 256
    bool measured;           // measure on: the verdict of measured_tile_rows goes first (structs of 2^20 padded rows or more)
    bool grow;               // tiles of 256 rows grow to 1024 / 512 under tile_rows_grow / tile_rows_accept (never beside a measured verdict)
    bool measure_off_plain;  // measure off: that one candidate, installed whenever it is valid, and neither elements nor sweep
    bool shared_budget;      // line_budget of a plan the parts share
    bool keep_if_worth;      // after the fallbacks the line plan stays under ap_hp_plan_worth (else: whenever valid)
    bool elements_by_kind;   // elements under ap_elements_allowed (else: TlcPlanOpts::elements)
};
constexpr PartsPolicy POLICY[3] = {
    //                           rows_512  measured  grow   measure_off_plain  shared_budget  keep_if_worth  elements_by_kind
    {"one struct",               false,    true,     true,  false,             false,         false,         false},
    {"ap[dp_sp]",                true,     true,     false, true,              true,          false,         true},
    {"split with an fp16 part",  true,     false,    false, true,              true,          true,          true},
};
int n_parts(uspmv_dmat *const parts[3]) { return parts[2] ? 3 : parts[1] ? 2 : 1; }
const PartsPolicy &policy_of(uspmv_dmat *const parts[3]) { return POLICY[!parts[1] ? 0 : parts[n_parts(parts) - 1]->dtype == USPMV_F16 ? 2 : 1]; }

// THE planner: lines -> elements -> sweep, once, for every kind and either source.  The handles end with the plan over single x elements
// (*n_tiles / *n_staged then describe it), or the column-window sweep, or the line plan where the kind's keep rule holds, or none; but for the
// element plan *n_tiles / *n_staged describe the line plan, also when the sweep took over or the plan was dropped (uspmv_dmat_plan_info tells
// what the handles ended up with).
template <typename Source>
int plan_parts(uspmv_dmat *const parts[3], Source &src, int max_lines, const TlcPlanOpts &opts, int64_t *n_tiles, int64_t *n_staged) {
    const char *who = src.who;
    const PartsPolicy &pol = policy_of(parts);
    const int n = n_parts(parts);
    for (int k = 0; k < n; ++k) { parts[k]->tlc = {}; parts[k]->sw = {}; }
    const bool own_budget = max_lines > 0;                     // (a caller with a line budget of its own keeps the line plan: no element fallback)
    src.budget = line_budget(max_lines, parts[0]->dtype, pol.shared_budget);
    const int R_meas = opts.measure && pol.measured ? measured_tile_rows(parts, src.budget, who) : 0;
    PlanStats st;
    if (int rc = plan_at_chosen_rows(R_meas, plan_tile_rows(opts.measure && pol.rows_512), pol.grow, src, &st)) return rc;
    if (n_tiles) *n_tiles = st.n_tiles;
    if (n_staged) *n_staged = st.valid ? st.n_staged : 0;
    if (verbose()) fprintf(stderr, "[uspmv] tlc plan (%s): valid=%d tiles=%lld staged=%lld max_lines=%d lines_total=%lld\n", pol.kind, (int)st.valid,
                           (long long)st.n_tiles, (long long)st.n_staged, st.lines, (long long)st.listed);
    bool keep = st.valid;
    if (opts.measure || !pol.measure_off_plain) {
        bool took = false;
        const bool allowed = pol.elements_by_kind ? ap_elements_allowed(opts, parts[0], parts[n - 1]) : opts.elements;
        if (int rc = elements_take_over(own_budget, st, allowed, parts[0]->dtype, sum_elements(parts), src, &took, n_tiles, n_staged)) return rc;
        if (took) return src.install_elements();
        if (int rc = src.dealt_rows(own_budget, st, &took, n_tiles, n_staged)) return rc;
        if (took) return USPMV_OK;
        if (int rc = sweep_takes_over(parts, src.structs(), n, st, who, &took)) return rc;
        keep = keep && !took && (!pol.keep_if_worth || ap_hp_plan_worth(st.n_tiles, st.n_staged));
    }
    if (keep) return src.install_line();
    for (int k = 0; k < n; ++k) parts[k]->tlc = {};          // (a candidate a device source left behind)
    return USPMV_OK;
}

int plan_parts_device(uspmv_dmat *const parts[3], int max_lines, const TlcPlanOpts &opts, int64_t *n_tiles, int64_t *n_staged, const char *who) {
    DeviceSource src{parts, who};
    return plan_parts(parts, src, max_lines, opts, n_tiles, n_staged);
}

}  // namespace

namespace uspmv_dev {

int check_ap_hp(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const char *who) {
    if (int rc = check_dmat(hi, who)) return rc;
    if (int rc = check_dmat(hp, who)) return rc;
    if (mid) if (int rc = check_dmat(mid, who)) return rc;
    const bool ok = hp->dtype == USPMV_F16 && (mid ? hi->dtype == USPMV_F64 && mid->dtype == USPMV_F32 : hi->dtype == USPMV_F64 || hi->dtype == USPMV_F32);
    if (!ok) return uspmv::fail(USPMV_ERR_INVALID, "%s: the parts must be (F64, -, F16), (F32, -, F16) or (F64, F32, F16)", who);
    if (hi->C != hp->C || hi->n_chunks != hp->n_chunks || (mid && (mid->C != hi->C || mid->n_chunks != hi->n_chunks)))
        return uspmv::fail(USPMV_ERR_INVALID, "%s: the parts must share C and n_chunks", who);
    return USPMV_OK;
}

bool c16_offsets(const std::vector<int32_t> &cl, int64_t C, std::vector<uint32_t> *c16p, int64_t *tot16) {
    const int64_t nc = (int64_t)cl.size();
    c16p->assign((size_t)nc + 1, 0);
    int64_t tot = 0;
    for (int64_t c = 0; c < nc; ++c) {
        (*c16p)[(size_t)c] = (uint32_t)tot;
        tot += ((int64_t)(cl[(size_t)c] + 3) / 4) * 4 * C;
        if (tot > (int64_t)UINT32_MAX) return false;
    }
    (*c16p)[(size_t)nc] = (uint32_t)tot;
    *tot16 = tot;
    return true;
}

int dmat_optimize_ap(uspmv_dmat *dp, uspmv_dmat *sp, const uspmv_scs *s_dp, const uspmv_scs *s_sp, int max_lines, const TlcPlanOpts &opts,
                     int64_t *n_tiles, int64_t *n_staged) {
    const char *who = "uspmv_dmat_optimize_ap";
    if (!dp || !sp || !s_dp || !s_sp) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (!uspmv::scs_has_entries(s_dp) || !uspmv::scs_has_entries(s_sp))
        return uspmv::fail(USPMV_ERR_INVALID, "%s: layout-only struct; the plan builder needs the host column indices", who);
    if (dp->C != s_dp->C || dp->n_chunks != s_dp->n_chunks || dp->dtype != USPMV_F64 || s_dp->dtype != USPMV_F64 ||
        sp->C != s_sp->C || sp->n_chunks != s_sp->n_chunks || sp->dtype != USPMV_F32 || s_sp->dtype != USPMV_F32 ||
        dp->C != sp->C || dp->n_chunks != sp->n_chunks)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: handles / host structs do not form a dp+sp pair", who);
    if (int rc = require_device()) return rc;
    uspmv_dmat *const parts[3] = {dp, sp, nullptr};
    const uspmv_scs *const ss[3] = {s_dp, s_sp, nullptr};
    HostSource src{parts, ss, who};
    return plan_parts(parts, src, max_lines, opts, n_tiles, n_staged);
}

int dmat_optimize(uspmv_dmat *A, const uspmv_scs *s, int max_lines, const TlcPlanOpts &opts, int64_t *n_tiles, int64_t *n_staged) {
    const char *who = "uspmv_dmat_optimize";
    if (!A || !s) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_dmat_one_prec(A, who)) return rc;
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "%s: layout-only struct; the plan builder needs the host column indices", who);
    if (A->C != s->C || A->n_chunks != s->n_chunks || A->dtype != s->dtype)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: handle and host struct do not describe the same matrix", who);
    if (int rc = require_device()) return rc;
    A->tlc = {};
    if (A->alt) { uspmv_dmat_free(A->alt); A->alt = nullptr; }
    if (s->C < 32 && 32 % s->C == 0 && g_tune.rechunk) {
        // narrow chunks (incl. crs = C 1): run on an internal C = 32 re-chunking with the same row order
        uspmv_scs r;
        int rc = uspmv_scs_rechunk32(s, &r);
        if (rc == USPMV_OK && rechunk_worth(r.n_elements, s->n_elements)) {
            uspmv_dmat_t *alt = nullptr;
            if (int rc2 = uspmv_dmat_upload(&r, &alt)) return rc2;
            alt->n_store = (long)(s->n_chunks * s->C);      // y of the caller has only the original padded rows
            TlcPlanOpts inner = opts;
            inner.new_to_old = &s->new_to_old_idx;          // (same row order: the caller's permutation serves the re-chunked struct)
            rc = dmat_optimize(alt, &r, max_lines, inner, n_tiles, n_staged);   // (C = 32: does not re-enter this branch)
            if (rc) { uspmv_dmat_free(alt); return rc; }
            A->alt = alt;
            return USPMV_OK;
        }
    }
    uspmv_dmat *const parts[3] = {A, nullptr, nullptr};
    const uspmv_scs *const ss[3] = {s, nullptr, nullptr};
    HostSource src{parts, ss, who, opts.deal_rows};
    if (int rc = plan_parts(parts, src, max_lines, opts, n_tiles, n_staged)) return rc;
    // (each of the two does nothing on a handle that ended without a tile-local-column plan)
    if (int rc = tlc_pack12(A, &s->chunk_lengths, who)) return rc;
    if (src.dealt || !opts.additive) return USPMV_OK;
    return tlc_additive_install(A, s, src.p, src.budget, opts.new_to_old, who);
}

int dmat_optimize_ap_hp(uspmv_dmat *hi, uspmv_dmat *mid, uspmv_dmat *hp, const uspmv_scs *s_hi, const uspmv_scs *s_mid, const uspmv_scs *s_hp,
                        int max_lines, const TlcPlanOpts &opts, int64_t *n_tiles, int64_t *n_staged) {
    const char *who = "uspmv_dmat_optimize_ap_hp";
    if (!s_hi || !s_hp || (mid && !s_mid)) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    const uspmv_scs_t *const ss[3] = {s_hi, mid ? s_mid : s_hp, mid ? s_hp : nullptr};
    uspmv_dmat_t *const ms[3] = {hi, mid ? mid : hp, mid ? hp : nullptr};
    for (int k = 0; k < 3; ++k) {
        if (!ms[k]) continue;
        if (!uspmv::scs_has_entries(ss[k]))
            return uspmv::fail(USPMV_ERR_INVALID, "%s: layout-only struct; the plan builder needs the host column indices", who);
        if (ms[k]->C != ss[k]->C || ms[k]->n_chunks != ss[k]->n_chunks || ms[k]->dtype != ss[k]->dtype)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: handles and host structs do not describe the same parts", who);
    }
    if (int rc = require_device()) return rc;
    HostSource src{ms, ss, who};
    return plan_parts(ms, src, max_lines, opts, n_tiles, n_staged);
}

}  // namespace uspmv_dev

extern "C" {

int uspmv_additive_plan_probe(const uspmv_scs_t *s, int64_t stats[8], int32_t *cols) {
    const char *who = "uspmv_additive_plan_probe";
    if (!s || !stats) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "%s: layout-only struct", who);
    for (int k = 0; k < 8; ++k) stats[k] = 0;
    if (cols) for (int64_t k = 0; k < s->n_elements; ++k) cols[k] = -1;
    const int max_lines = line_budget(0, s->dtype, false);
    uspmv_tlc_plan p;
    if (int rc = uspmv_build_tlc_plan(s, nullptr, max_lines, plan_tile_rows(false), &p)) return rc;
    stats[4] = p.n_tiles;
    if (!additive_eligible(s, p, false, nullptr)) return USPMV_OK;
    uspmv_additive_plan a;
    if (int rc = uspmv_build_additive_plan(s, &p, max_lines * 16, &a, nullptr, additive_tile_rows(s, p.tile_rows))) return rc;
    const bool idx12 = pack12_applies(false, p.max_lines_used, s->C, s->n_chunks) && pack12_kept(s->n_elements, s->n_chunks * s->C);
    if (verbose()) fprintf(stderr, "[uspmv] additive probe: line plan tile_rows=%d max_lines=%d; records tile_rows=%d tiles=%lld with records=%lld intervals=%zu max_elems=%d\n", p.tile_rows, p.max_lines_used,
                           a.tile_rows, (long long)a.n_tiles, (long long)a.n_add_tiles, a.iv.size() / 4, a.max_elems);
    const AdditiveBytes b = additive_bytes(s, a, idx12);
    stats[0] = additive_kept(a, b); stats[1] = a.n_additive; stats[2] = a.n_chunks; stats[3] = a.n_add_tiles;
    stats[5] = b.fresh; stats[6] = b.replaced; stats[7] = a.max_elems;
    if (a.valid) stats[4] = a.n_tiles;               // (the records' own tiles: whole sigma windows where additive_tile_rows says so)
    if (cols && stats[0]) uspmv_additive_plan_decode(s, &a, cols);
    return USPMV_OK;
}

int uspmv_additive_plan_probe2(const uspmv_scs_t *s, int64_t stats[4]) {
    const char *who = "uspmv_additive_plan_probe2";
    if (!s || !stats) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "%s: layout-only struct", who);
    for (int k = 0; k < 4; ++k) stats[k] = 0;
    const int max_lines = line_budget(0, s->dtype, false);
    uspmv_tlc_plan p;
    if (int rc = uspmv_build_tlc_plan(s, nullptr, max_lines, plan_tile_rows(false), &p)) return rc;
    if (!additive_eligible(s, p, false, nullptr)) return USPMV_OK;
    uspmv_additive_plan a;
    if (int rc = uspmv_build_additive_plan(s, &p, max_lines * 16, &a, nullptr, additive_tile_rows(s, p.tile_rows))) return rc;
    if (!a.valid) return USPMV_OK;
    stats[0] = (int64_t)1 << a.w_log; stats[1] = (int64_t)a.lines.size(); stats[2] = a.n_lines_again; stats[3] = 2 * (int64_t)a.map16.size();
    return USPMV_OK;
}

int uspmv_dmat_optimize(uspmv_dmat_t *A, const uspmv_scs_t *s, int max_lines, int64_t *n_tiles, int64_t *n_staged) {
    return dmat_optimize(A, s, max_lines, TlcPlanOpts{}, n_tiles, n_staged);
}

int uspmv_dmat_optimize_device(uspmv_dmat_t *A, int max_lines, int64_t *n_tiles, int64_t *n_staged) {
    return dmat_optimize_device(A, max_lines, TlcPlanOpts{}, n_tiles, n_staged);
}

int uspmv_dmat_optimize_device_ap(uspmv_dmat_t *dp, uspmv_dmat_t *sp, int max_lines, int64_t *n_tiles, int64_t *n_staged) {
    const char *who = "uspmv_dmat_optimize_device_ap";
    if (int rc = check_dmat(dp, who)) return rc;
    if (int rc = check_dmat(sp, who)) return rc;
    if (dp->dtype != USPMV_F64 || sp->dtype != USPMV_F32 || dp->C != sp->C || dp->n_chunks != sp->n_chunks)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: handles do not form a dp+sp pair", who);
    if (int rc = require_device()) return rc;
    uspmv_dmat *const parts[3] = {dp, sp, nullptr};
    return plan_parts_device(parts, max_lines, TlcPlanOpts{}, n_tiles, n_staged, who);
}

}  // extern "C"

// uspmv_dmat_optimize_device with the options spelled out, as dmat_optimize above takes them (deal_rows and additive: host planner only)
int uspmv_dev::dmat_optimize_device(uspmv_dmat *A, int max_lines, const TlcPlanOpts &opts, int64_t *n_tiles, int64_t *n_staged) {
    const char *who = "uspmv_dmat_optimize_device";
    if (int rc = check_dmat_one_prec(A, who)) return rc;
    if (int rc = require_device()) return rc;
    if (A->alt) { uspmv_dmat_free(A->alt); A->alt = nullptr; }
    if (A->C < 32 && 32 % A->C == 0 && g_tune.rechunk && A->n_chunks > 0) {
        // narrow chunks (incl. crs = C 1): the internal C = 32 re-chunking of uspmv_dmat_optimize, built on the device --
        // O(n_chunks) layout on the host, the O(n_elements) copy by rechunk32_kernel
        const int64_t C = A->C, nc_old = A->n_chunks, per = 32 / C, nc = (nc_old + per - 1) / per;
        std::vector<int32_t> cl_old((size_t)nc_old), cl((size_t)nc, 0), cp((size_t)nc + 1, 0);
        int32_t last = 0;
        HIP_TRY(hipMemcpy(cl_old.data(), A->chunk_lengths, 4 * (size_t)nc_old, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&last, A->chunk_ptrs + nc_old, 4, hipMemcpyDeviceToHost));
        int64_t cur = 0;
        bool fits = true;
        for (int64_t k = 0; k < nc && fits; ++k) {
            int32_t L = 0;
            for (int64_t c = k * per; c < std::min((k + 1) * per, nc_old); ++c) L = std::max(L, cl_old[(size_t)c]);
            cl[(size_t)k] = L; cp[(size_t)k] = (int32_t)cur;
            cur += (int64_t)L * 32;
            fits = cur <= INT32_MAX;
        }
        if (fits && rechunk_worth(cur, last)) {
            cp[(size_t)nc] = (int32_t)cur;
            auto *alt = new uspmv_dmat;
            alt->C = 32; alt->n_chunks = nc; alt->n_elements = cur; alt->dtype = A->dtype;
            alt->n_store = (long)(nc_old * C);              // y of the caller has only the original padded rows
            const size_t vsz = A->dtype == USPMV_F64 ? 8 : 4, ne = (size_t)std::max<int64_t>(cur, 1);
            hipError_t e = alt->own_arrays();
            if (e == hipSuccess) e = hipMemcpy(alt->own.chunk_ptrs, cp.data(), 4 * ((size_t)nc + 1), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(alt->own.chunk_lengths, cl.data(), 4 * (size_t)nc, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemsetAsync(alt->own.col_idxs, 0, 4 * ne, nullptr);
            if (e == hipSuccess) e = hipMemsetAsync(alt->own.values, 0, vsz * ne, nullptr);
            int rc = e == hipSuccess ? launch_rechunk32(A, alt->chunk_ptrs, alt->own.col_idxs, alt->own.values, nullptr) : uspmv::fail(USPMV_ERR_ALLOC, "%s: %s", who, hipGetErrorString(e));
            uspmv_dmat *const alt_parts[3] = {alt, nullptr, nullptr};
            if (!rc) rc = plan_parts_device(alt_parts, max_lines, opts, n_tiles, n_staged, who);
            if (rc) { uspmv_dmat_free(alt); return rc; }
            A->tlc = {};
            A->alt = alt;
            return USPMV_OK;
        }
    }
    uspmv_dmat *const parts[3] = {A, nullptr, nullptr};
    return plan_parts_device(parts, max_lines, opts, n_tiles, n_staged, who);
}

// The line plan shared by the two or three parts of a split (parts[2] NULL: two), as dmat_optimize_ap / _ap_hp install it with `measure`
// off (PartsPolicy::measure_off_plain), under the default line budget
int uspmv_dev::dmat_optimize_device_shared(uspmv_dmat *const parts[3], int64_t *n_tiles, int64_t *n_staged, const char *who) {
    TlcPlanOpts plain;
    plain.measure = false;
    return plan_parts_device(parts, 0, plain, n_tiles, n_staged, who);
}

extern "C" {

int uspmv_dmat_optimize_ap(uspmv_dmat_t *dp, uspmv_dmat_t *sp, const uspmv_scs_t *s_dp, const uspmv_scs_t *s_sp,
                           int max_lines, int64_t *n_tiles, int64_t *n_staged) {
    return dmat_optimize_ap(dp, sp, s_dp, s_sp, max_lines, TlcPlanOpts{}, n_tiles, n_staged);
}

int uspmv_dmat_optimize_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, const uspmv_scs_t *s_hi, const uspmv_scs_t *s_mid,
                              const uspmv_scs_t *s_hp, int max_lines, int64_t *n_tiles, int64_t *n_staged) {
    return dmat_optimize_ap_hp(hi, mid, hp, s_hi, s_mid, s_hp, max_lines, TlcPlanOpts{}, n_tiles, n_staged);
}

int uspmv_dmat_optimize_device_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, int max_lines, int64_t *n_tiles, int64_t *n_staged) {
    const char *who = "uspmv_dmat_optimize_device_ap_hp";
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    if (int rc = require_device()) return rc;
    uspmv_dmat_t *const ms[3] = {hi, mid ? mid : hp, mid ? hp : nullptr};
    return plan_parts_device(ms, max_lines, TlcPlanOpts{}, n_tiles, n_staged, who);
}

int uspmv_dmat_plan_download(const uspmv_dmat_t *A, int64_t meta[4], int32_t *tile_line_ptr, int32_t *tile_lines, uint32_t *c16_ptrs,
                             uint16_t *col16) {
    if (int rc = check_dmat(A, "uspmv_dmat_plan_download")) return rc;
    if (!meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_plan_download: NULL meta");
    meta[0] = meta[1] = meta[2] = meta[3] = 0;
    if (!A->tlc.on) return USPMV_OK;
    if (int rc = require_device()) return rc;
    int32_t last = 0; uint32_t last16 = 0;
    // (the second and third part of a shared ap plan hold only their local indices: the line list lives with the first part)
    if (A->tlc.line_ptr) HIP_TRY(hipMemcpy(&last, A->tlc.line_ptr + A->tlc.n_tiles, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&last16, A->tlc.c16_ptrs + A->n_chunks, 4, hipMemcpyDeviceToHost));
    meta[0] = A->tlc.n_tiles; meta[1] = last; meta[2] = last16; meta[3] = A->tlc.max_lines;
    if (tile_line_ptr && A->tlc.line_ptr) HIP_TRY(hipMemcpy(tile_line_ptr, A->tlc.line_ptr, 4 * ((size_t)A->tlc.n_tiles + 1), hipMemcpyDeviceToHost));
    if (tile_lines && last) HIP_TRY(hipMemcpy(tile_lines, A->tlc.lines, 4 * (size_t)last, hipMemcpyDeviceToHost));
    if (c16_ptrs) HIP_TRY(hipMemcpy(c16_ptrs, A->tlc.c16_ptrs, 4 * ((size_t)A->n_chunks + 1), hipMemcpyDeviceToHost));
    if (col16 && last16) HIP_TRY(hipMemcpy(col16, A->tlc.col16, 2 * (size_t)last16, hipMemcpyDeviceToHost));
    return USPMV_OK;
}

}  // extern "C"
