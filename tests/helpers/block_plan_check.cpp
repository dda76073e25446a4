// Test helper (CPU only): invariants of the block plan's row orders and phase cuts (host/tlc_plan.cpp) on generated and file matrices.
//   block_plan_check [file.mtx ...]   prints one "ok <name> ..." line per case, exit code 1 on the first violated invariant
#include "uspmv.h"
#include "uspmv_internal.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

// The other forms of the planner the device code reads: phases of up to cap_rows X rows (512: two-byte indices, MAXP = 8 kernel) and lists
// of LINES of 2^shift X rows (what the XM = 2 kernel stages from a column-major block vector).  Same invariants as the 256-row / row-list
// form checked in check(): phases tile the groups in order, <= 8 groups each, lists strictly ascending and within the cap unless the phase
// is a single group, and every local index decodes to its entry's column by (xrows[list + (li >> shift)] << shift) | (li & mask).
// *over = phases that list more than cap_rows >> shift items (what uspmv_dmat_optimize_block turns the line plan down on).
static int check_form(const char *name, const uspmv_scs *src, int cap_rows, int shift, int cost, uspmv_phased_plan *p, int64_t *over) {
    const int64_t C = src->C, nc = src->n_chunks, T = 64 / C;
    const int cap_items = cap_rows >> shift, mask = (1 << shift) - 1;
    REQUIRE(uspmv_build_phased_plan(src, cap_rows, 8, p, shift, cost) == 0 && p->valid, "%s cap %d shift %d cost %d", name, cap_rows, shift, cost);
    REQUIRE(p->cap_rows == cap_rows && p->line_shift == shift && p->n_tiles == (nc + T - 1) / T, "%s cap %d shift %d", name, cap_rows, shift);
    REQUIRE((int64_t)p->ph_ptr.size() == p->n_tiles + 1 && p->ph_ptr[(size_t)p->n_tiles] == p->n_phases && (int64_t)p->ph_list_ptr.size() == p->n_phases + 1 &&
            p->ph_list_ptr[(size_t)p->n_phases] == (int)p->xrows.size(), "%s cap %d shift %d: array sizes", name, cap_rows, shift);
    *over = 0;
    int longest = 0;
    for (int64_t t = 0; t < p->n_tiles; ++t) {
        int64_t ng = 0;
        for (int64_t c = t * T; c < std::min(nc, (t + 1) * T); ++c) ng = std::max<int64_t>(ng, (src->chunk_lengths[(size_t)c] + 3) / 4);
        const int p0 = p->ph_ptr[(size_t)t], p1 = p->ph_ptr[(size_t)t + 1];
        REQUIRE((ng == 0) == (p0 == p1), "%s tile %lld", name, (long long)t);
        for (int ph = p0; ph < p1; ++ph) {
            const int g0 = p->ph_g0[(size_t)ph], g1 = ph + 1 < p1 ? p->ph_g0[(size_t)ph + 1] : (int)ng;
            REQUIRE((ph == p0 ? g0 == 0 : true) && g1 > g0 && g1 - g0 <= 8, "%s tile %lld phase %d groups [%d,%d)", name, (long long)t, ph, g0, g1);
            const int lp = p->ph_list_ptr[(size_t)ph], len = p->ph_list_ptr[(size_t)ph + 1] - lp;
            REQUIRE(len >= 1 && (len <= cap_items || g1 - g0 == 1), "%s tile %lld phase %d lists %d items (cap %d)", name, (long long)t, ph, len, cap_items);
            *over += len > cap_items;
            longest = std::max(longest, len);
            for (int k = 1; k < len; ++k) REQUIRE(p->xrows[(size_t)(lp + k - 1)] < p->xrows[(size_t)(lp + k)], "%s list order", name);
            for (int64_t c = t * T; c < std::min(nc, (t + 1) * T); ++c) {
                const int64_t cs = src->chunk_ptrs[(size_t)c], L = src->chunk_lengths[(size_t)c];
                for (int64_t j = (int64_t)g0 * 4; j < std::min<int64_t>((int64_t)g1 * 4, L); ++j)
                    for (int64_t i = 0; i < C; ++i) {
                        const int li = p->col16[(size_t)(p->c16_ptrs[(size_t)c] + (j / 4) * 4 * C + i * 4 + j % 4)];
                        REQUIRE((li >> shift) < len && (((int64_t)p->xrows[(size_t)(lp + (li >> shift))] << shift) | (li & mask)) == src->col_idxs[(size_t)(cs + j * C + i)],
                                "%s cap %d shift %d tile %lld slot %lld row %lld", name, cap_rows, shift, (long long)t, (long long)j, (long long)i);
                    }
            }
        }
    }
    REQUIRE(p->max_rows_used == (longest << shift), "%s cap %d shift %d: max_rows_used %d, longest list %d", name, cap_rows, shift, p->max_rows_used, longest);
    return 0;
}

static int check(const char *name, uspmv_coo_t *coo, int C, int sigma, bool permute, std::map<std::string, int64_t> *staged_out) {
    uspmv_scs_t *s = nullptr;
    REQUIRE(uspmv_convert_to_scs(coo, C, sigma, USPMV_F64, nullptr, &s) == 0, "%s", name);
    if (permute) REQUIRE(uspmv_permute_scs_cols(s, s->old_to_new_idx.data()) == 0, "%s", name);
    const int64_t nc = s->n_chunks, n_pad = nc * C;
    {   // line lists of 32 floats on the F32 struct (rows in the order uspmv_dmat_optimize_block keeps under "spmmv_xline": ties undone)
        uspmv_scs_t *f = nullptr;
        REQUIRE(uspmv_convert_to_scs(coo, C, sigma, USPMV_F32, nullptr, &f) == 0, "%s f32", name);
        if (permute) REQUIRE(uspmv_permute_scs_cols(f, f->old_to_new_idx.data()) == 0, "%s f32", name);
        uspmv_scs r; std::vector<int32_t> map;
        const int moved = uspmv_scs_reorder_rows(f, 1, &r, &map);
        REQUIRE(moved == 0 || moved == 1, "%s f32", name);
        uspmv_phased_plan p; int64_t over = 0;
        if (check_form(name, moved ? &r : f, 256, 5, 0, &p, &over)) return 1;
        (*staged_out)[std::string(name) + "/f32/over5"] = over;
        printf("ok %s C=%d sigma=%d f32 shift=5 phases=%lld lines=%zu max_rows=%d over=%lld\n", name, C, sigma, (long long)p.n_phases, p.xrows.size(), p.max_rows_used, (long long)over);
        uspmv_scs_free(f);
    }
    for (int mode : {1, 2, 4}) {
        uspmv_scs r; std::vector<int32_t> map;
        const int moved = uspmv_scs_reorder_rows(s, mode, &r, &map);
        REQUIRE(moved == 0 || moved == 1, "%s mode %d", name, mode);
        REQUIRE((int64_t)map.size() == n_pad, "%s mode %d", name, mode);
        // the map is a permutation of the positions that exchanges rows only between chunks of equal length
        std::vector<char> seen((size_t)n_pad, 0);
        for (int64_t q = 0; q < n_pad; ++q) {
            const int32_t v = map[(size_t)q];
            REQUIRE(v >= 0 && v < n_pad && !seen[(size_t)v], "%s mode %d position %lld -> %d", name, mode, (long long)q, v);
            seen[(size_t)v] = 1;
            REQUIRE(s->chunk_lengths[(size_t)(q / C)] == s->chunk_lengths[(size_t)(v / C)], "%s mode %d: row %d moved between chunk lengths", name, mode, v);
        }
        const uspmv_scs *src = moved ? &r : s;
        if (moved) {                                             // the copy holds every row's slots in order
            REQUIRE(r.chunk_ptrs == s->chunk_ptrs && r.chunk_lengths == s->chunk_lengths, "%s mode %d", name, mode);
            for (int64_t q = 0; q < n_pad; q += 7) {
                const int64_t v = map[(size_t)q], L = s->chunk_lengths[(size_t)(q / C)];
                for (int64_t j = 0; j < L; ++j) {
                    const int64_t a = s->chunk_ptrs[(size_t)(q / C)] + j * C + q % C, b = s->chunk_ptrs[(size_t)(v / C)] + j * C + v % C;
                    REQUIRE(r.col_idxs[(size_t)a] == s->col_idxs[(size_t)b] && r.values_f64[(size_t)a] == s->values_f64[(size_t)b], "%s mode %d row %lld slot %lld", name, mode, (long long)q, (long long)j);
                }
            }
        }
        for (int cost : {0, 24, 200}) {
            uspmv_phased_plan p;
            REQUIRE(uspmv_build_phased_plan(src, 256, 8, &p, 0, cost) == 0 && p.valid, "%s mode %d cost %d", name, mode, cost);
            const int64_t T = 64 / C;
            REQUIRE(p.n_tiles == (nc + T - 1) / T, "%s", name);
            for (int64_t t = 0; t < p.n_tiles; ++t) {
                int64_t ng = 0;
                for (int64_t c = t * T; c < std::min(nc, (t + 1) * T); ++c) ng = std::max<int64_t>(ng, (src->chunk_lengths[(size_t)c] + 3) / 4);
                const int p0 = p.ph_ptr[(size_t)t], p1 = p.ph_ptr[(size_t)t + 1];
                REQUIRE((ng == 0) == (p0 == p1), "%s tile %lld", name, (long long)t);
                for (int ph = p0; ph < p1; ++ph) {               // phases tile the groups [0, ng) in order, <= 8 groups and <= 256 rows each
                    const int g0 = p.ph_g0[(size_t)ph], g1 = ph + 1 < p1 ? p.ph_g0[(size_t)ph + 1] : (int)ng;
                    REQUIRE((ph == p0 ? g0 == 0 : true) && g1 > g0 && g1 - g0 <= 8, "%s tile %lld phase %d groups [%d,%d)", name, (long long)t, ph, g0, g1);
                    const int len = p.ph_list_ptr[(size_t)ph + 1] - p.ph_list_ptr[(size_t)ph];
                    REQUIRE(len >= 1 && (len <= 256 || g1 - g0 == 1), "%s tile %lld phase %d lists %d rows", name, (long long)t, ph, len);
                    for (int k = 1; k < len; ++k) REQUIRE(p.xrows[(size_t)(p.ph_list_ptr[(size_t)ph] + k - 1)] < p.xrows[(size_t)(p.ph_list_ptr[(size_t)ph] + k)], "%s list order", name);
                    for (int64_t c = t * T; c < std::min(nc, (t + 1) * T); ++c) {   // every local index points at its entry's column
                        const int64_t cs = src->chunk_ptrs[(size_t)c], L = src->chunk_lengths[(size_t)c];
                        for (int64_t j = (int64_t)g0 * 4; j < std::min<int64_t>((int64_t)g1 * 4, L); ++j)
                            for (int64_t i = 0; i < C; ++i) {
                                const int li = p.col16[(size_t)(p.c16_ptrs[(size_t)c] + (j / 4) * 4 * C + i * 4 + j % 4)];
                                REQUIRE(li < len && p.xrows[(size_t)(p.ph_list_ptr[(size_t)ph] + li)] == src->col_idxs[(size_t)(cs + j * C + i)], "%s tile %lld slot %lld row %lld", name, (long long)t, (long long)j, (long long)i);
                            }
                    }
                }
            }
            (*staged_out)[std::string(name) + "/" + std::to_string(mode) + "/" + std::to_string(cost)] = (int64_t)p.xrows.size();
            printf("ok %s C=%d sigma=%d mode=%d cost=%d tiles=%lld phases=%lld staged=%zu\n", name, C, sigma, mode, cost, (long long)p.n_tiles, (long long)p.n_phases, p.xrows.size());
            // 512-row phases ("spmmv_phase_rows" 512); filled to the brim (cost 0) they are never more than the 256-row phases: a
            // phase that fits 256 rows fits 512, and the greedy cut gives the fewest phases under a limit that sub-ranges inherit
            uspmv_phased_plan p5; int64_t over5 = 0;
            if (check_form(name, src, 512, 0, cost, &p5, &over5)) return 1;
            REQUIRE(cost > 0 || p5.n_phases <= p.n_phases, "%s mode %d cost %d: %lld phases of 512 rows against %lld of 256", name, mode, cost, (long long)p5.n_phases, (long long)p.n_phases);
            (*staged_out)[std::string(name) + "/" + std::to_string(mode) + "/" + std::to_string(cost) + "/max512"] = p5.max_rows_used;
            printf("ok %s C=%d sigma=%d mode=%d cost=%d cap=512 phases=%lld staged=%zu max_rows=%d over=%lld\n", name, C, sigma, mode, cost, (long long)p5.n_phases, p5.xrows.size(), p5.max_rows_used, (long long)over5);
        }
        // line lists of 16 doubles (the XM = 2 kernel's form; built with greedy cuts like uspmv_dmat_optimize_block does)
        uspmv_phased_plan pl; int64_t over = 0;
        if (check_form(name, src, 256, 4, 0, &pl, &over)) return 1;
        (*staged_out)[std::string(name) + "/" + std::to_string(mode) + "/over4"] = over;
        printf("ok %s C=%d sigma=%d mode=%d shift=4 phases=%lld lines=%zu max_rows=%d over=%lld\n", name, C, sigma, mode, (long long)pl.n_phases, pl.xrows.size(), pl.max_rows_used, (long long)over);
    }
    uspmv_scs_free(s);
    return 0;
}

int main(int argc, char **argv) {
    std::map<std::string, int64_t> st;
    uspmv_coo_t *m = nullptr;
    REQUIRE(uspmv_gen_stencil27(24, 22, 20, 3, 0x5EED, 0.0, 0, 24L * 22 * 20 * 3, &m) == 0, "gen");
    if (check("mesh3", m, 32, 512, true, &st)) return 1;
    if (check("mesh3-s1", m, 32, 1, true, &st)) return 1;
    if (check("mesh3-C64", m, 64, 128, true, &st)) return 1;
    if (check("mesh3-noperm", m, 32, 512, false, &st)) return 1;     // columns left in original numbering: clustering must not hurt
    uspmv_coo_free(m);
    REQUIRE(uspmv_gen_stencil27(60, 50, 1, 2, 0x5EED, 0.0, 0, 60L * 50 * 2, &m) == 0, "gen");
    if (check("mesh2d", m, 32, 256, true, &st)) return 1;
    uspmv_coo_free(m);
    REQUIRE(uspmv_gen_banded_random(20000, 40, 3000, 0x5EED, 0.0, 0, 20000, &m) == 0, "gen");
    if (check("banded", m, 32, 512, true, &st)) return 1;
    uspmv_coo_free(m);
    // three small shapes tests/test_gpu_spmmv_phased_arms.py runs the 512-row and the line-list kernels on
    REQUIRE(uspmv_gen_banded_random(1000, 11, 900, 0x5EED, 0.0, 0, 1000, &m) == 0, "gen");
    if (check("band11", m, 32, 1, true, &st)) return 1;
    uspmv_coo_free(m);
    REQUIRE(uspmv_gen_stencil27(12, 11, 10, 3, 0x5EED, 0.0, 0, 12L * 11 * 10 * 3, &m) == 0, "gen");
    if (check("mesh3small-s1", m, 32, 1, true, &st)) return 1;
    uspmv_coo_free(m);
    REQUIRE(uspmv_gen_stencil27(9, 30, 11, 2, 0x5EED, 0.0, 0, 9L * 30 * 11 * 2, &m) == 0, "gen");
    if (check("mesh2small", m, 64, 128, true, &st)) return 1;
    uspmv_coo_free(m);
    // mesh2small: 512-row phases list more than 256 rows only when filled to the brim (the GPU test builds that plan with "spmmv_phase_dp" 0)
    REQUIRE(st["mesh2small/4/0/max512"] > 256 && st["mesh2small/4/0/max512"] <= 512, "mesh2small: %lld rows in the longest 512-row phase", (long long)st["mesh2small/4/0/max512"]);
    // band11 under the default row order and cuts: some phase of the 512-row form lists more than 256 rows (only then does the MAXP = 8
    // kernel run); mesh3small-s1 in the order "spmmv_xline" keeps (ties undone): no phase over 16 lines, the line plan is not turned down
    REQUIRE(st["band11/4/24/max512"] > 256 && st["band11/4/24/max512"] <= 512, "band11: %lld rows in the longest 512-row phase", (long long)st["band11/4/24/max512"]);
    REQUIRE(st.count("mesh3small-s1/1/over4") && st["mesh3small-s1/1/over4"] == 0, "mesh3small-s1: %lld phases over 16 lines", (long long)st["mesh3small-s1/1/over4"]);
    for (int a = 1; a < argc; ++a) {
        REQUIRE(uspmv_read_mtx(argv[a], &m) == 0, "%s", argv[a]);
        const char *bn = strrchr(argv[a], '/');
        if (check(bn ? bn + 1 : argv[a], m, 32, 64, true, &st)) return 1;
        uspmv_coo_free(m);
    }
    // flat patches + dynamic-programming cuts: at most 0.8 of the rows the ties-undone / greedy plan stages on the 3-dof mesh; never more
    // anywhere (the sample refuses a clustering that does not help); the dynamic programme alone never stages more than the greedy cuts
    REQUIRE(st["mesh3/4/24"] * 100 <= st["mesh3/1/0"] * 80, "mesh3: %lld against %lld", (long long)st["mesh3/4/24"], (long long)st["mesh3/1/0"]);
    for (auto &kv : st) {
        const std::string k = kv.first, base = k.substr(0, k.find('/'));
        if (k.size() > 5 && k.substr(k.size() - 5) == "/4/24") REQUIRE(kv.second <= st[base + "/1/24"] * 102 / 100 + 64, "%s: %lld against %lld", k.c_str(), (long long)kv.second, (long long)st[base + "/1/24"]);
        if (k.size() > 3 && k.substr(k.size() - 3) == "/24") { const std::string g = k.substr(0, k.size() - 2) + "0"; REQUIRE(kv.second <= st[g], "%s: %lld against greedy %lld", k.c_str(), (long long)kv.second, (long long)st[g]); }
    }
    printf("all ok\n");
    return 0;
}
