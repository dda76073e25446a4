// Host-side check of the block-vector column-window sweep plan (ultimate-spmv_amd/host/sweep_plan.cpp: uspmv_build_block_sweep_plan):
// replays the plan exactly the way scs_spmmv_sweep / sweep_window_block (csrc/spmmv_sweep.hip) consume it -- per sweep tile and
// (h, wave) the stream at wave_off[k*wpt + h*nw + wave], the tile's windows ascending, rounds in batches of U = 4 (ballot masks,
// off = first[u] + lanes_below, advance by first[U]), idx relative to the window's first row, the trailing padding once per column as
// fma(0, X[pad_col], acc) -- and compares all B accumulators of every row bit for bit (NaN equals NaN) with the plain slot-ordered FMA
// chain over the SCS arrays (the reference's summation, code/kernels.hpp:306-398).  Shapes: those of tests/test_gpu_spmmv_sweep_edges.py
// (partial last wave, a tile without windows, a count byte of 255, 14-20 windows per tile) and of tests/test_gpu_spmmv_sweep.py.
// One deliberately corrupted plan must be reported as a mismatch.  Test infrastructure only; built by tests/test_block_sweep_plan.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uspmv_internal.hpp"

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0 || (std::isnan(a) && std::isnan(b)); }

template <typename VT> static const std::vector<VT> &vals_of(const uspmv_scs *s);
template <> const std::vector<double> &vals_of<double>(const uspmv_scs *s) { return s->values_f64; }
template <> const std::vector<float> &vals_of<float>(const uspmv_scs *s) { return s->values_f32; }
template <typename VT> static const std::vector<VT> &vals_of(const uspmv_block_sweep_plan &p);
template <> const std::vector<double> &vals_of<double>(const uspmv_block_sweep_plan &p) { return p.vals_f64; }
template <> const std::vector<float> &vals_of<float>(const uspmv_block_sweep_plan &p) { return p.vals_f32; }
template <typename VT> static std::vector<VT> &vals_of(uspmv_block_sweep_plan &p);
template <> std::vector<double> &vals_of<double>(uspmv_block_sweep_plan &p) { return p.vals_f64; }
template <> std::vector<float> &vals_of<float>(uspmv_block_sweep_plan &p) { return p.vals_f32; }

// the reference: per row and column the slot-ordered chain over every slot of the chunk, padding included; X row-major, B values per row
template <typename VT>
static std::vector<VT> chain(const uspmv_scs *s, const std::vector<VT> &X, int B) {
    const std::vector<VT> &va = vals_of<VT>(s);
    std::vector<VT> y((size_t)(s->n_chunks * s->C) * B);
    for (int64_t c = 0; c < s->n_chunks; ++c)
        for (int64_t i = 0; i < s->C; ++i)
            for (int w = 0; w < B; ++w) {
                VT acc = 0;
                for (int64_t j = 0; j < s->chunk_lengths[c]; ++j) {
                    const int64_t k = s->chunk_ptrs[c] + j * s->C + i;
                    acc = std::fma(va[(size_t)k], X[(size_t)s->col_idxs[k] * B + w], acc);
                }
                y[(size_t)(c * s->C + i) * B + w] = acc;
            }
    return y;
}

struct Walk {
    int64_t mismatches = 0, rows = 0, bad_structure = 0;
    int max_cnt = 0;
    int64_t min_windows = INT64_MAX, max_windows = 0;
};

// the kernel's walk over the plan; bad_structure counts violations that would make the kernel read outside the plan or X
template <typename VT>
static Walk replay(const uspmv_scs *s, const uspmv_block_sweep_plan &p, const std::vector<VT> &X, int64_t x_rows, int B, const std::vector<VT> &ref) {
    constexpr int U = 4;
    Walk r;
    const std::vector<VT> &va = vals_of<VT>(p);
    const int64_t R = p.tile_rows, n_pad = s->n_chunks * s->C, W = (int64_t)1 << p.wlog;
    const int64_t T = std::min<int64_t>(R, 1024), RPL = R / T, nw = T / 64, wpt = nw * RPL;
    std::vector<int> covered((size_t)n_pad, 0);
    std::vector<VT> acc((size_t)64 * B);
    for (int64_t k = 0; k < p.n_sweep_tiles; ++k) {
        const int64_t tile = p.tile_ids[(size_t)k], wp0 = p.t_win_ptr[(size_t)k], S = p.t_win_ptr[(size_t)k + 1] - wp0;
        r.min_windows = std::min(r.min_windows, S); r.max_windows = std::max(r.max_windows, S);
        for (int64_t sw = 1; sw < S; ++sw) if (p.wins[(size_t)(wp0 + sw)] <= p.wins[(size_t)(wp0 + sw - 1)]) ++r.bad_structure;
        for (int64_t h = 0; h < RPL; ++h)
            for (int64_t wave = 0; wave < nw; ++wave) {
                uint64_t o = p.wave_off[(size_t)(k * wpt + h * nw + wave)];
                std::fill(acc.begin(), acc.end(), VT(0));
                for (int64_t sw = 0; sw < S; ++sw) {
                    const int64_t g0 = (int64_t)p.wins[(size_t)(wp0 + sw)] << p.wlog;
                    const uint8_t *cnt = p.cnt.data() + p.t_cnt_off[(size_t)k] + sw * R + h * T + wave * 64;
                    for (int l = 0; l < 64; ++l) {
                        r.max_cnt = std::max<int>(r.max_cnt, cnt[l]);
                        if (tile * R + h * T + wave * 64 + l >= n_pad && cnt[l] != 0) ++r.bad_structure;
                    }
                    for (int k0 = 0;; k0 += U) {
                        uint64_t m[U];
                        unsigned first[U + 1];
                        first[0] = 0;
                        for (int u = 0; u < U; ++u) {
                            m[u] = 0;
                            for (int l = 0; l < 64; ++l) if (k0 + u < cnt[l]) m[u] |= 1ull << l;
                            first[u + 1] = first[u] + (unsigned)__builtin_popcountll(m[u]);
                        }
                        if (m[0] == 0) break;
                        for (int u = 0; u < U; ++u)
                            for (int l = 0; l < 64; ++l) {
                                if (!(k0 + u < cnt[l])) continue;
                                const uint64_t off = o + first[u] + (unsigned)__builtin_popcountll(m[u] & ((1ull << l) - 1));
                                if (off >= p.idx.size() || off >= va.size()) { ++r.bad_structure; continue; }
                                const int64_t ix = p.idx[(size_t)off];
                                if (ix >= W || g0 + ix >= x_rows) { ++r.bad_structure; continue; }
                                for (int w = 0; w < B; ++w)
                                    acc[(size_t)l * B + w] = std::fma(va[(size_t)off], X[(size_t)(g0 + ix) * B + w], acc[(size_t)l * B + w]);
                            }
                        o += first[U];
                    }
                }
                // the wave's stream ends where the next one starts
                const size_t nxt = (size_t)(k * wpt + h * nw + wave) + 1;
                if (nxt < p.wave_off.size() && o != p.wave_off[nxt]) ++r.bad_structure;
                for (int l = 0; l < 64; ++l) {
                    const int64_t lr = h * T + wave * 64 + l, row = tile * R + lr;
                    const int32_t pc = p.pad_col[(size_t)(k * R + lr)];
                    if (row >= n_pad) { if (pc != -1) ++r.bad_structure; continue; }
                    if (pc >= x_rows) { ++r.bad_structure; continue; }
                    for (int w = 0; w < B; ++w) {
                        VT a = acc[(size_t)l * B + w];
                        if (pc >= 0) a = std::fma(VT(0), X[(size_t)pc * B + w], a);
                        if (!same_bits(a, ref[(size_t)row * B + w])) ++r.mismatches;
                    }
                    ++covered[(size_t)row]; ++r.rows;
                }
            }
    }
    for (int64_t q = 0; q < n_pad; ++q) if (covered[(size_t)q] != 1) ++r.bad_structure;   // (every tile sweeps in the plans replayed here)
    return r;
}

// swaps two stream entries of different rounds (and different lanes) in one wave; false: the plan has no such pair
template <typename VT>
static bool corrupt(uspmv_block_sweep_plan &p) {
    std::vector<VT> &va = vals_of<VT>(p);
    const int64_t R = p.tile_rows, T = std::min<int64_t>(R, 1024), nw = T / 64, wpt = nw * (R / T);
    for (int64_t k = 0; k < p.n_sweep_tiles; ++k) {
        if (p.t_win_ptr[(size_t)k + 1] == p.t_win_ptr[(size_t)k]) continue;
        for (int64_t v = 0; v < wpt; ++v) {
            const uint8_t *cnt = p.cnt.data() + p.t_cnt_off[(size_t)k] + v * 64;      // first window of the tile: the stream starts with it
            int n0 = 0, la = -1, lb = -1;
            for (int l = 0; l < 64; ++l) if (cnt[l] > 0) { if (la < 0) la = l; ++n0; }
            for (int l = 0; l < 64; ++l) if (cnt[l] > 1) lb = l;
            if (la < 0 || lb < 0 || la == lb) continue;
            int below = 0;
            for (int l = 0; l < lb; ++l) if (cnt[l] > 1) ++below;
            const size_t a = p.wave_off[(size_t)(k * wpt + v)], b = a + (size_t)n0 + (size_t)below;   // round 0 of lane la, round 1 of lane lb
            if (va[a] == va[b] && p.idx[a] == p.idx[b]) continue;
            std::swap(va[a], va[b]); std::swap(p.idx[a], p.idx[b]);
            return true;
        }
    }
    return false;
}

template <typename VT>
static std::vector<VT> make_X(const uspmv_scs *s, int64_t x_rows, int B, bool special) {
    std::vector<VT> X((size_t)x_rows * B);
    for (int64_t i = 0; i < x_rows; ++i)
        for (int w = 0; w < B; ++w) X[(size_t)i * B + w] = (VT)((1.0 + 1e-3 * (double)(i % 1000)) * (1.0 + w / 8.0));
    if (special) {
        uint64_t h = 88172645463325252ull;
        for (int q = 0; q < 200; ++q) {
            h ^= h << 13; h ^= h >> 7; h ^= h << 17;
            const size_t at = (size_t)(h % X.size());
            X[at] = q % 4 == 0 ? (VT)INFINITY : q % 4 == 1 ? (VT)-INFINITY : q % 4 == 2 ? (VT)NAN : (VT)-0.0;
        }
        // the X row at the padding column of the first padded row
        for (int64_t c = 0; c < s->n_chunks; ++c) {
            const int64_t L = s->chunk_lengths[c];
            if (L == 0) continue;
            const int32_t pc = s->col_idxs[(size_t)(s->chunk_ptrs[c] + (L - 1) * s->C + s->C - 1)];
            const VT row[4] = {(VT)INFINITY, (VT)-INFINITY, (VT)NAN, (VT)-0.0};
            for (int w = 0; w < B; ++w) X[(size_t)pc * B + w] = row[w % 4];
            break;
        }
    }
    return X;
}

enum Expect { SWEEPS, DECLINED };

template <typename VT>
static void run_t(const char *name, const uspmv_coo_t *coo, int C, int sigma, int wlog, int tile_rows, double max_stage, Expect expect, int want_max_cnt,
                  bool want_empty_tile, bool corrupt_it, bool exact_x) {
    constexpr int B = 64 / (int)sizeof(VT);
    uspmv_scs_t *s = nullptr;
    REQUIRE(uspmv_convert_to_scs(coo, C, sigma, sizeof(VT) == 8 ? USPMV_F64 : USPMV_F32, nullptr, &s) == 0);
    REQUIRE(uspmv_permute_scs_cols(s, s->old_to_new_idx.data()) == 0);
    uspmv_block_sweep_plan p;
    REQUIRE(uspmv_build_block_sweep_plan(s, wlog, tile_rows, 64, max_stage, &p) == 0);
    const bool installable = p.valid && p.n_sweep_tiles == p.n_tiles && p.rest_chunks.empty();
    if (expect == DECLINED) {
        printf("%s %s C=%d sigma=%d wlog=%d tile=%d: valid=%d, %ld of %ld tiles sweep (declined, as expected)\n", name, sizeof(VT) == 8 ? "f64" : "f32", C,
               sigma, wlog, tile_rows, (int)p.valid, (long)p.n_sweep_tiles, (long)p.n_tiles);
        REQUIRE(!installable);
        uspmv_scs_free(s);
        return;
    }
    REQUIRE(installable);
    if (!installable) { uspmv_scs_free(s); return; }
    int32_t max_col = 0;
    for (int32_t c : s->col_idxs) max_col = std::max(max_col, c);
    REQUIRE(p.x_rows_min == (int64_t)max_col + 1);
    // exact_x: X of x_rows_min rows and no more (the kernel's contract), which a row block needs beyond its padded rows
    if (exact_x) REQUIRE(s->n_rows != s->n_cols && p.x_rows_min > s->n_rows_padded);
    const int64_t x_rows = exact_x ? p.x_rows_min : std::max<int64_t>(std::max<int64_t>(s->n_rows_padded, s->n_cols), p.x_rows_min);
    for (int special = 0; special < 2; ++special) {
        const std::vector<VT> X = make_X<VT>(s, x_rows, B, special != 0);
        const std::vector<VT> ref = chain<VT>(s, X, B);
        const Walk r = replay<VT>(s, p, X, x_rows, B, ref);
        printf("%s %s C=%d sigma=%d wlog=%d tile=%d special=%d: rows padded %ld, tiles %ld, windows per tile %ld..%ld, largest count %d, rows %ld, "
               "structure errors %ld, mismatches %ld\n", name, sizeof(VT) == 8 ? "f64" : "f32", C, sigma, wlog, tile_rows, special, (long)(s->n_chunks * s->C),
               (long)p.n_tiles, (long)r.min_windows, (long)r.max_windows, r.max_cnt, (long)r.rows, (long)r.bad_structure, (long)r.mismatches);
        REQUIRE(r.bad_structure == 0);
        REQUIRE(r.mismatches == 0);
        REQUIRE(r.rows == s->n_chunks * s->C);
        if (want_max_cnt) REQUIRE(r.max_cnt == want_max_cnt);
        if (want_empty_tile) REQUIRE(r.min_windows == 0);
    }
    if (corrupt_it) {
        uspmv_block_sweep_plan q = p;
        const bool done = corrupt<VT>(q);
        REQUIRE(done);
        const std::vector<VT> X = make_X<VT>(s, x_rows, B, false);
        const Walk r = replay<VT>(s, q, X, x_rows, B, chain<VT>(s, X, B));
        printf("%s %s corrupted plan (two stream entries of different rounds swapped in one wave): mismatches %ld -> %s\n", name,
               sizeof(VT) == 8 ? "f64" : "f32", (long)r.mismatches, r.mismatches > 0 ? "caught" : "NOT CAUGHT");
        REQUIRE(r.mismatches > 0);
    }
    uspmv_scs_free(s);
}

static void run(const char *name, const uspmv_coo_t *coo, int C, int sigma, int wlog_f64, int wlog_f32, int tile_rows, double max_stage = 24.0,
                Expect expect = SWEEPS, int want_max_cnt = 0, bool want_empty_tile = false, bool corrupt_it = false, bool exact_x = false) {
    run_t<double>(name, coo, C, sigma, wlog_f64, tile_rows, max_stage, expect, want_max_cnt, want_empty_tile, corrupt_it, exact_x);
    run_t<float>(name, coo, C, sigma, wlog_f32, tile_rows, max_stage, expect, want_max_cnt, want_empty_tile, corrupt_it, exact_x);
}

static uspmv_coo_t *from_rows(int64_t n, const std::vector<std::vector<int32_t>> &rows) {
    std::vector<int32_t> I, J;
    std::vector<double> V;
    for (int64_t i = 0; i < n; ++i)
        for (int32_t j : rows[(size_t)i]) { I.push_back((int32_t)i); J.push_back(j); V.push_back(0.5 + (double)((i * 7 + j * 3) % 29) / 16.0); }
    uspmv_coo_t *coo = nullptr;
    REQUIRE(uspmv_coo_create(n, n, (int64_t)I.size(), I.data(), J.data(), V.data(), &coo) == 0);
    return coo;
}

// shape H: rows {i-3 .. i+3}, rows 1024..2047 and every row with i % 7 == 3 emptied: a tile without windows
static uspmv_coo_t *shape_h() {
    const int64_t n = 3500;
    std::vector<std::vector<int32_t>> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if ((i >= 1024 && i < 2048) || i % 7 == 3) continue;
        for (int64_t j = std::max<int64_t>(i - 3, 0); j <= std::min<int64_t>(i + 3, n - 1); ++j) rows[(size_t)i].push_back((int32_t)j);
    }
    return from_rows(n, rows);
}

// shape D: row 5 with `wide` entries in columns 0 .. wide-1, every other row the diagonal and column i + 300 (where the matrix has it)
static uspmv_coo_t *shape_d(int wide) {
    const int64_t n = 2048;
    std::vector<std::vector<int32_t>> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (i == 5) { for (int j = 0; j < wide; ++j) rows[5].push_back(j); continue; }
        rows[(size_t)i].push_back((int32_t)i);
        if (i + 300 < n) rows[(size_t)i].push_back((int32_t)(i + 300));
    }
    return from_rows(n, rows);
}

int main() {
    uspmv_coo_t *a = nullptr, *band = nullptr, *st3 = nullptr;
    REQUIRE(uspmv_gen_stencil27(15, 11, 7, 1, 0x5EED, 0.0, 0, 15 * 11 * 7, &a) == 0);
    REQUIRE(uspmv_gen_banded_random(5000, 40, 700, 0x5EED, 4.0, 0, 5000, &band) == 0);
    REQUIRE(uspmv_gen_stencil27(14, 13, 12, 3, 0x5EED, 0.0, 0, 14 * 13 * 12 * 3, &st3) == 0);
    uspmv_coo_t *h = shape_h(), *d255 = shape_d(255), *d256 = shape_d(256);
    // A: n_rows_padded 1184 = 18.5 waves, the last tile 160 rows
    for (int wlog = 6; wlog <= 8; ++wlog) run("A", a, 32, 64, wlog, wlog, 1024);
    run("A", a, 8, 1, 7, 7, 1024);
    for (int C : {16, 32, 64}) run("H", h, C, 1, 7, 8, 1024, 24.0, SWEEPS, 0, true);
    run("D255", d255, 32, 1, 8, 8, 1024, 4096.0, SWEEPS, 255);
    run("D255", d255, 32, 1, 8, 8, 1024, 24.0, DECLINED);                  // staging cost above the default 24 bytes per non-zero
    run("D256", d256, 32, 1, 8, 8, 1024, 4096.0, DECLINED);                // 256 entries of one row in one window: no count byte holds it
    run("band", band, 32, 64, 7, 7, 1024, 24.0, SWEEPS, 0, false, true);
    run("stencil3", st3, 32, 1, 10, 10, 4096);                             // four rows per lane
    run("stencil3", st3, 32, 512, 9, 9, 1024);
    run("stencil3", st3, 32, 512, 8, 8, 2048, 24.0, DECLINED);
    run("stencil3", st3, 32, 512, 11, 11, 1024);                           // 128-KiB windows: one LDS buffer whatever "sweep_nbuf" asks
    // a row block, rows 4001..7001 of the 9999-row banded matrix (tests/test_gpu_nonsquare.py): 3001 x 9999, X of x_rows_min rows
    uspmv_coo_t *rb = nullptr;
    const int64_t row_begin = 4001, row_end = 7002;
    REQUIRE(uspmv_gen_banded_random(9999, 23, 700, 7, 10.0, row_begin, row_end, &rb) == 0);
    REQUIRE(rb->n_rows == row_end - row_begin && rb->n_cols == 9999);
    run("row block", rb, 32, 512, 9, 9, 1024, 24.0, SWEEPS, 0, false, false, true);
    run("row block", rb, 64, 1, 11, 11, 1024, 24.0, SWEEPS, 0, false, false, true);
    for (uspmv_coo_t *m : {a, band, st3, h, d255, d256, rb}) uspmv_coo_free(m);
    printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
