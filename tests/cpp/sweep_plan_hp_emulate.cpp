// Host-side check of the column-window sweep plan for the adaptive-precision splits with an fp16 part (host/sweep_plan.cpp with two or
// three structs): the plan is replayed the way scs_spmv_sweep_ap_hp consumes it -- windows ascending, per window every part's rounds,
// lanes ascending, each part's compacted stream, each part's trailing padding once -- and y is compared bit for bit with every part's
// slot-ordered chain over the SCS arrays, composed as ap_hp_y does (hi + hp, (hi + mid) + hp, (float)(sp + hp)).
// It also restates the layout of the one-struct and the dp+sp plan as it was before the third part existed (layout_before) and
// requires uspmv_build_sweep_plan to reproduce it byte for byte, and repeats on the three-part planner the coverage the GPU tests
// rely on.  Test infrastructure only; built by tests/test_sweep_plan_hp.py (with -ffp-contract=off: the float products must round).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "uspmv_internal.hpp"

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

enum { DP_HP = USPMV_AP_DP_HP, SP_HP = USPMV_AP_SP_HP, DP_SP_HP = USPMV_AP_DP_SP_HP };
static const char *kind_name(int k) { return k == DP_HP ? "dp_hp" : k == SP_HP ? "sp_hp" : "dp_sp_hp"; }

// value of element q of a struct, widened exactly
static double val64(const uspmv_scs *s, size_t q) {
    return s->dtype == USPMV_F64 ? s->values_f64[q] : s->dtype == USPMV_F32 ? (double)s->values_f32[q] : uspmv_f16_to_f64(s->values_f16[q]);
}
// one step of a part's chain (ap_step of the kernels): double x -> FMA in double; float x -> product rounded to float, added in double
static double step(double v, double x, double acc, bool float_x) {
    if (!float_x) return std::fma(v, x, acc);
    const float p = (float)v * (float)x;
    return acc + (double)p;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }
static double compose(int kind, const double a[3], int np) {
    if (kind == SP_HP) return (double)(float)(a[0] + a[1]);
    return np == 3 ? (a[0] + a[1]) + a[2] : a[0] + a[1];
}

struct Split {
    int kind = 0, np = 0;
    uspmv_scs_t *s[3] = {nullptr, nullptr, nullptr};      // in the order of the split: hi, [mid,] hp
    void free() { for (auto *p : s) if (p) uspmv_scs_free(p); }
};

// |v| quantile of the non-zero finite values
static double quantile(const uspmv_coo *m, double q) {
    std::vector<double> a;
    for (double v : m->values) if (std::isfinite(v) && v != 0.0) a.push_back(std::fabs(v));
    std::sort(a.begin(), a.end());
    return a.empty() ? 1.0 : a[(size_t)(q * (double)(a.size() - 1))];
}

static bool make_split(const uspmv_coo_t *coo, int kind, double t1, double t2, int C, int sigma, Split *out) {
    uspmv_coo_t *hi = nullptr, *mid = nullptr, *hp = nullptr;
    REQUIRE(uspmv_partition_precisions_hp(coo, kind, t1, t2, &hi, &mid, &hp) == 0);
    out->kind = kind;
    uspmv_scs_t *sh = nullptr, *sm = nullptr, *sq = nullptr;
    bool ok = uspmv_convert_to_scs(hi, C, sigma, kind == SP_HP ? USPMV_F32 : USPMV_F64, nullptr, &sh) == 0;
    REQUIRE(ok);
    const int32_t *perm = sh->old_to_new_idx.data();
    if (ok && mid) ok = uspmv_convert_to_scs(mid, C, sigma, USPMV_F32, perm, &sm) == 0;
    if (ok) ok = uspmv_convert_to_scs(hp, C, sigma, USPMV_F16, perm, &sq) == 0;
    if (ok) {
        for (uspmv_scs_t *s : {sh, sm, sq}) if (s) REQUIRE(uspmv_permute_scs_cols(s, perm) == 0);
        out->np = 0;
        out->s[out->np++] = sh;
        if (sm) out->s[out->np++] = sm;
        out->s[out->np++] = sq;
    } else {
        for (uspmv_scs_t *s : {sh, sm, sq}) if (s) uspmv_scs_free(s);
    }
    uspmv_coo_free(hi); if (mid) uspmv_coo_free(mid); uspmv_coo_free(hp);
    return ok;
}

static std::vector<double> make_x(int64_t n, bool float_x, bool special) {
    std::vector<double> x((size_t)n);
    for (size_t i = 0; i < x.size(); ++i) x[i] = 1.0 + 1e-3 * (double)(i % 1000);
    if (special) { x[0] = -INFINITY; x[5] = -0.0; x[17] = NAN; }
    if (float_x) for (double &v : x) v = (double)(float)v;
    return x;
}

struct PartView { const uint32_t *wave_off; const uint8_t *cnt; const uint16_t *idx; const int32_t *pad; const void *vals; int dtype; };
static PartView part_view(const uspmv_sweep_plan &p, const Split &sp, int w) {
    const auto &pt = p.part[w];
    REQUIRE(pt.dtype == sp.s[w]->dtype);
    return {pt.wave_off.data(), pt.cnt.data(), pt.idx.data(), pt.pad_col.data(), pt.vals(), sp.s[w]->dtype};
}
static double stream_val(const PartView &v, size_t k) {
    return v.dtype == USPMV_F64 ? ((const double *)v.vals)[k] : v.dtype == USPMV_F32 ? (double)((const float *)v.vals)[k] : uspmv_f16_to_f64(((const uint16_t *)v.vals)[k]);
}

// replay + compare; returns sweep tiles.  expect: 0 = any coverage > 0, 1 = every tile sweeps, 2 = some tiles sweep and some do not
static int64_t check_split(const char *what, const Split &sp, int wlog, int tile_rows, double max_stage, bool special, int expect, bool exact_x = false) {
    const bool fx = sp.kind == SP_HP;
    const uspmv_scs *s0 = sp.s[0];
    const int64_t C = s0->C, n_pad = s0->n_chunks * C;
    uspmv_sweep_plan p;
    REQUIRE(uspmv_build_sweep_plan(sp.s, sp.np, wlog, tile_rows, max_stage, &p) == 0);
    REQUIRE(p.n_parts == sp.np);
    REQUIRE(p.valid);
    if (!p.valid) return 0;
    int64_t max_col = -1;
    for (int w = 0; w < sp.np; ++w) for (int32_t c : sp.s[w]->col_idxs) max_col = std::max<int64_t>(max_col, c);
    REQUIRE(p.x_len_min == max_col + 1);
    // exact_x: x of x_len_min elements and no more (the kernels' contract), which a row block needs beyond its padded rows
    if (exact_x) REQUIRE(s0->n_rows != s0->n_cols && p.x_len_min > s0->n_rows_padded);
    std::vector<double> x = make_x(exact_x ? p.x_len_min : std::max<int64_t>(s0->n_rows_padded, s0->n_cols), fx, special);
    const int64_t R = p.tile_rows, wpt = R / 64;
    std::vector<double> y((size_t)n_pad, 12345.0);
    std::vector<char> covered((size_t)n_pad, 0);
    PartView pv[3];
    for (int w = 0; w < sp.np; ++w) pv[w] = part_view(p, sp, w);
    for (int64_t k = 0; k < p.n_sweep_tiles; ++k) {
        const int64_t t = p.tile_ids[(size_t)k];
        for (int64_t v = 0; v < wpt; ++v) {
            double acc[3][64];
            uint32_t base[3];
            for (int w = 0; w < 3; ++w) { for (int l = 0; l < 64; ++l) acc[w][l] = 0.0; base[w] = w < sp.np ? pv[w].wave_off[(size_t)(k * wpt + v)] : 0; }
            for (int64_t sw = 0; sw < p.t_S[(size_t)k]; ++sw) {
                const int64_t g0 = (int64_t)(p.t_smin[(size_t)k] + sw) << wlog;
                for (int w = 0; w < sp.np; ++w) {
                    const uint8_t *cnt = pv[w].cnt + p.t_cnt_off[(size_t)k] + sw * R + v * 64;
                    for (int kk = 0;; ++kk) {
                        bool any = false;
                        for (int l = 0; l < 64; ++l) {
                            if (cnt[l] <= kk) continue;
                            any = true;
                            acc[w][l] = step(stream_val(pv[w], base[w]), x[(size_t)(g0 + pv[w].idx[base[w]])], acc[w][l], fx);
                            ++base[w];
                        }
                        if (!any) break;
                    }
                }
            }
            for (int l = 0; l < 64; ++l) {
                const int64_t row = t * R + v * 64 + l;
                if (row >= n_pad) continue;
                double a[3] = {0, 0, 0};
                for (int w = 0; w < sp.np; ++w) {
                    const int32_t pc = pv[w].pad[(size_t)(k * R + v * 64 + l)];
                    if (pc >= 0) acc[w][l] = step(0.0, x[(size_t)pc], acc[w][l], fx);
                    a[w] = acc[w][l];
                }
                y[(size_t)row] = compose(sp.kind, a, sp.np); covered[(size_t)row] = 1;
            }
        }
    }
    for (int32_t c : p.rest_chunks) for (int64_t i = 0; i < C; ++i) covered[(size_t)(c * C + i)] = 2;
    // every part's slot-ordered chain over the SCS arrays
    int64_t bad = 0, nsw = 0, stream_total = 0;
    for (int64_t c = 0; c < s0->n_chunks; ++c)
        for (int64_t i = 0; i < C; ++i) {
            const int64_t r = c * C + i;
            REQUIRE(covered[(size_t)r] != 0);
            if (covered[(size_t)r] != 1) continue;
            double a[3] = {0, 0, 0};
            for (int w = 0; w < sp.np; ++w) {
                const uspmv_scs *s = sp.s[w];
                for (int64_t j = 0; j < s->chunk_lengths[(size_t)c]; ++j) {
                    const size_t q = (size_t)(s->chunk_ptrs[(size_t)c] + j * C + i);
                    a[w] = step(val64(s, q), x[(size_t)s->col_idxs[q]], a[w], fx);
                }
            }
            ++nsw;
            if (!same_bits(y[(size_t)r], compose(sp.kind, a, sp.np))) ++bad;
        }
    // the streams hold sizeof(value) + 2 bytes per stored entry and nothing else
    for (int w = 0; w < sp.np; ++w) {
        const std::vector<uint16_t> &ix = p.part[w].idx;
        stream_total += (int64_t)ix.size() - 64;
        if (p.n_sweep_tiles == p.n_tiles) REQUIRE((int64_t)ix.size() - 64 <= sp.s[w]->n_elements);
    }
    printf("%s %s C=%ld sigma=%ld wlog=%d tile=%d special=%d: sweep tiles %ld/%ld, rows checked %ld, stream entries %ld, mismatches %ld\n", what,
           kind_name(sp.kind), (long)C, (long)s0->sigma, wlog, tile_rows, (int)special, (long)p.n_sweep_tiles, (long)p.n_tiles, (long)nsw,
           (long)stream_total, (long)bad);
    REQUIRE(bad == 0);
    if (expect == 1) REQUIRE(p.n_sweep_tiles == p.n_tiles && p.rest_chunks.empty());
    else if (expect == 2) REQUIRE(p.n_sweep_tiles > 0 && p.n_sweep_tiles < p.n_tiles && !p.rest_chunks.empty());
    else REQUIRE(nsw > 0);
    return p.n_sweep_tiles;
}

static void run(int64_t n, int nnz_row, int64_t band, int C, int sigma, int wlog, int tile_rows, int kind, bool special, int expect,
                double q1 = 0.7, double q2 = 0.35, int64_t row_begin = 0, int64_t row_end = -1) {
    if (row_end < 0) row_end = n;
    const bool block = row_begin != 0 || row_end != n;      // a row block of n columns, rows renumbered from 0
    uspmv_coo_t *coo = nullptr;
    REQUIRE(uspmv_gen_banded_random(n, nnz_row, band, 7, 10.0, row_begin, row_end, &coo) == 0);
    double t1 = q1 < 0 ? 0.0 : q1 > 1 ? INFINITY : quantile(coo, q1), t2 = q2 < 0 ? 0.0 : q2 > 1 ? INFINITY : quantile(coo, q2);
    if (special) {
        t1 = std::max(t1, 1e6); t2 = std::max(t2, 1e5);       // 7e4 lands in the hp part of every kind and overflows binary16 there
        // +-0, +-inf, values that overflow binary16 in the hp part, (dp_sp_hp only: partition refuses NaN elsewhere) NaN, and an explicit +0 on
        // the last column of a row (indistinguishable from SELL padding: stripped and applied once)
        const int64_t nnz = coo->nnz;
        for (int64_t e = 0; e + 1 < nnz; ++e) {
            const bool last_of_row = coo->I[(size_t)e] != coo->I[(size_t)e + 1];
            const int r = coo->I[(size_t)e];
            if (last_of_row && r % 3 == 0) coo->values[(size_t)e] = 0.0;
            else if (e % 97 == 1) coo->values[(size_t)e] = -0.0;
            else if (e % 97 == 2) coo->values[(size_t)e] = 0.0;
            else if (e % 1009 == 3) coo->values[(size_t)e] = INFINITY;
            else if (e % 1009 == 4) coo->values[(size_t)e] = -INFINITY;
            else if (e % 211 == 5) coo->values[(size_t)e] = (e & 1) ? -7e4 : 7e4;
            else if (e % 13 == 7) coo->values[(size_t)e] = 3e5 + (double)(e % 1000);      // (keeps the mid part of dp_sp_hp populated)
            else if (e % 13 == 8) coo->values[(size_t)e] = 2e6 + (double)(e % 1000) / 3.0; // (... and the hi part)
            else if (e % 1013 == 6 && kind == DP_SP_HP) coo->values[(size_t)e] = NAN;
        }
    }
    Split sp;
    if (make_split(coo, kind, t1, t2, C, sigma, &sp)) {
        if (block) REQUIRE(sp.s[0]->n_rows == row_end - row_begin);
        check_split(block ? "row block" : "split", sp, wlog, tile_rows, 1e9, special, expect, block);
        sp.free();
    } else REQUIRE(!"conversion of a part refused");
    uspmv_coo_free(coo);
}

// a row whose columns are not sorted: its window index decreases, so its tile must go to the rest list
static void run_unsorted(int kind) {
    uspmv_coo_t *coo = nullptr;
    REQUIRE(uspmv_gen_banded_random(8192, 40, 3000, 11, 10.0, 0, 8192, &coo) == 0);
    const double t1 = quantile(coo, 0.7), t2 = quantile(coo, 0.35);
    // row 1000: first and last entry change places (column and value)
    int64_t a = -1, b = -1;
    for (int64_t e = 0; e < coo->nnz; ++e) if (coo->I[(size_t)e] == 1000) { if (a < 0) a = e; b = e; }
    REQUIRE(a >= 0 && b > a);
    std::swap(coo->J[(size_t)a], coo->J[(size_t)b]); std::swap(coo->values[(size_t)a], coo->values[(size_t)b]);
    // both of them into the hp part (below every other magnitude), so that this part's row is out of order whatever the thresholds
    double tiny = INFINITY;
    for (double v : coo->values) if (v != 0.0) tiny = std::min(tiny, std::fabs(v));
    coo->values[(size_t)a] = coo->values[(size_t)b] = 0.5 * tiny;
    Split sp;
    REQUIRE(make_split(coo, kind, t1, t2, 32, 1, &sp));
    check_split("unsorted row", sp, 9, 256, 1e9, false, 2);
    sp.free();
    uspmv_coo_free(coo);
}

// ---- the layout of the one-struct and the dp+sp plan before the third part existed, restated: per row the entries are binned by window
// first, then the streams are emitted tile by tile, wave by wave, window by window, round by round, lanes ascending
struct Before {
    std::vector<int32_t> tile_ids, t_smin, t_S, rest, pad[2];
    std::vector<uint64_t> t_cnt_off;
    std::vector<uint32_t> wave_off[2];
    std::vector<uint8_t> cnt[2];
    std::vector<uint16_t> idx[2];
    std::vector<double> v64[2];
    std::vector<float> v32[2];
    int64_t n_tiles = 0;
};
static void layout_before(const uspmv_scs *const ss[2], int ns, int wlog, int R, double max_stage, Before *o) {
    const int64_t C = ss[0]->C, nc = ss[0]->n_chunks, n_pad = nc * C, nt = (n_pad + R - 1) / R, wpt = R / 64;
    const double xbytes = ss[0]->dtype == USPMV_F64 ? 8.0 : 4.0;
    o->n_tiles = nt;
    struct Row { int64_t le = 0; int32_t pad = -1; bool bad = false; std::map<int32_t, std::vector<int64_t>> bins; };   // window -> element positions
    auto scan_row = [&](const uspmv_scs *s, int64_t q) {
        Row r;
        const int64_t c = q / C, i = q % C, cs = s->chunk_ptrs[(size_t)c], L = s->chunk_lengths[(size_t)c];
        if (L == 0) return r;
        auto pos = [&](int64_t j) { return cs + j * C + i; };
        auto pz = [&](int64_t e) {
            if (s->dtype == USPMV_F64) { uint64_t b; std::memcpy(&b, &s->values_f64[(size_t)e], 8); return b == 0; }
            uint32_t b; std::memcpy(&b, &s->values_f32[(size_t)e], 4); return b == 0;
        };
        const int32_t pc = s->col_idxs[(size_t)pos(L - 1)];
        int64_t le = L;
        while (le > 0 && s->col_idxs[(size_t)pos(le - 1)] == pc && pz(pos(le - 1))) --le;
        if (le < L) r.pad = pc;
        r.le = le;
        int32_t prev = -1;
        for (int64_t j = 0; j < le; ++j) {
            const int32_t w = s->col_idxs[(size_t)pos(j)] >> wlog;
            if (w < prev) r.bad = true;
            prev = w;
            r.bins[w].push_back(pos(j));
        }
        for (auto &kv : r.bins) if (kv.second.size() > 255) r.bad = true;
        return r;
    };
    int64_t cnt_bytes = 0, tot[2] = {0, 0};
    for (int64_t t = 0; t < nt; ++t) {
        const int64_t q0 = t * R, q1 = std::min(q0 + R, n_pad);
        std::vector<Row> rows[2];
        bool good = true;
        int32_t lo = INT32_MAX, hi = -1;
        int64_t nnz_t = 0;
        for (int w = 0; w < ns; ++w)
            for (int64_t q = q0; q < q1; ++q) {
                rows[w].push_back(scan_row(ss[w], q));
                const Row &r = rows[w].back();
                good = good && !r.bad;
                nnz_t += r.le;
                if (!r.bins.empty()) { lo = std::min(lo, r.bins.begin()->first); hi = std::max(hi, r.bins.rbegin()->first); }
            }
        const int64_t nS = (int64_t)hi - lo + 1;
        if (!good || hi < 0 || (double)nS * (double)((int64_t)1 << wlog) * xbytes > max_stage * (double)std::max<int64_t>(nnz_t, 1) || nS > 4096) {
            for (int64_t c = t * R / C; c < std::min((t + 1) * R / C, nc); ++c) o->rest.push_back((int32_t)c);
            continue;
        }
        o->tile_ids.push_back((int32_t)t); o->t_smin.push_back(lo); o->t_S.push_back((int32_t)nS); o->t_cnt_off.push_back((uint64_t)cnt_bytes);
        for (int w = 0; w < ns; ++w) {
            const uspmv_scs *s = ss[w];
            o->cnt[w].resize((size_t)(cnt_bytes + nS * R), 0);
            for (int64_t r = 0; r < R; ++r) o->pad[w].push_back(r < (int64_t)rows[w].size() ? rows[w][(size_t)r].pad : -1);
            for (int64_t r = 0; r < (int64_t)rows[w].size(); ++r)
                for (auto &kv : rows[w][(size_t)r].bins) o->cnt[w][(size_t)(cnt_bytes + (kv.first - lo) * R + r)] = (uint8_t)kv.second.size();
            for (int64_t v = 0; v < wpt; ++v) {
                o->wave_off[w].push_back((uint32_t)tot[w]);
                for (int64_t sw = 0; sw < nS; ++sw)
                    for (size_t kk = 0;; ++kk) {
                        bool any = false;
                        for (int64_t r = v * 64; r < std::min<int64_t>(v * 64 + 64, (int64_t)rows[w].size()); ++r) {
                            auto it = rows[w][(size_t)r].bins.find((int32_t)(lo + sw));
                            if (it == rows[w][(size_t)r].bins.end() || it->second.size() <= kk) continue;
                            any = true;
                            const int64_t e = it->second[kk];
                            o->idx[w].push_back((uint16_t)(s->col_idxs[(size_t)e] - ((int32_t)(lo + sw) << wlog)));
                            if (s->dtype == USPMV_F64) o->v64[w].push_back(s->values_f64[(size_t)e]); else o->v32[w].push_back(s->values_f32[(size_t)e]);
                            ++tot[w];
                        }
                        if (!any) break;
                    }
            }
        }
        cnt_bytes += nS * R;
    }
    if (o->tile_ids.empty()) return;
    for (int w = 0; w < ns; ++w) {           // the spare tail of the streams
        o->idx[w].resize(o->idx[w].size() + 64, 0);
        if (ss[w]->dtype == USPMV_F64) o->v64[w].resize(o->v64[w].size() + 64, 0.0); else o->v32[w].resize(o->v32[w].size() + 64, 0.0f);
    }
}
template <typename T>
static bool same_vec(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static void run_before(int64_t n, int nnz_row, int64_t band, int C, int sigma, int wlog, int tile_rows, bool ap, int dtype, double max_stage) {
    uspmv_coo_t *coo = nullptr;
    REQUIRE(uspmv_gen_banded_random(n, nnz_row, band, 7, ap ? 10.0 : 0.0, 0, n, &coo) == 0);
    uspmv_coo_t *dpc = coo, *spc = nullptr;
    if (ap) REQUIRE(uspmv_partition_precisions(coo, 1e-3, &dpc, &spc) == 0);
    uspmv_scs_t *s = nullptr, *s2 = nullptr;
    REQUIRE(uspmv_convert_to_scs(dpc, C, sigma, ap ? USPMV_F64 : dtype, nullptr, &s) == 0);
    REQUIRE(uspmv_permute_scs_cols(s, s->old_to_new_idx.data()) == 0);
    if (ap) {
        REQUIRE(uspmv_convert_to_scs(spc, C, sigma, USPMV_F32, s->old_to_new_idx.data(), &s2) == 0);
        REQUIRE(uspmv_permute_scs_cols(s2, s->old_to_new_idx.data()) == 0);
    }
    uspmv_sweep_plan p;
    const uspmv_scs *ss[2] = {s, s2};
    const int ns = ap ? 2 : 1;
    REQUIRE(uspmv_build_sweep_plan(ss, ns, wlog, tile_rows, max_stage, &p) == 0);
    Before b;
    layout_before(ss, ns, wlog, tile_rows, max_stage, &b);
    REQUIRE(p.n_tiles == b.n_tiles && p.n_sweep_tiles == (int64_t)b.tile_ids.size());
    REQUIRE(same_vec(p.tile_ids, b.tile_ids) && same_vec(p.t_smin, b.t_smin) && same_vec(p.t_S, b.t_S) && same_vec(p.t_cnt_off, b.t_cnt_off));
    REQUIRE(same_vec(p.rest_chunks, b.rest));
    if (!b.tile_ids.empty()) {
        REQUIRE(p.valid);
        REQUIRE(p.n_parts == ns);
        for (int w = 0; w < ns; ++w) {
            const auto &pt = p.part[w];
            REQUIRE(pt.dtype == ss[w]->dtype);
            REQUIRE(same_vec(pt.wave_off, b.wave_off[w]) && same_vec(pt.cnt, b.cnt[w]) && same_vec(pt.idx, b.idx[w]) && same_vec(pt.pad_col, b.pad[w]));
            // the stream in the part's own type and in no other: nothing in binary16
            REQUIRE(same_vec(pt.vals_f64, b.v64[w]) && same_vec(pt.vals_f32, b.v32[w]) && pt.vals_f16.empty());
        }
        // the parts the plan has not are empty
        for (int w = ns; w < 3; ++w) {
            const auto &pt = p.part[w];
            REQUIRE(pt.wave_off.empty() && pt.cnt.empty() && pt.idx.empty() && pt.pad_col.empty());
            REQUIRE(pt.vals_f64.empty() && pt.vals_f32.empty() && pt.vals_f16.empty());
        }
    }
    printf("layout as before: n=%ld C=%d sigma=%d wlog=%d tile=%d ap=%d dtype=%d: sweep tiles %ld/%ld, %zu + %zu stream entries\n", (long)n, C, sigma, wlog,
           tile_rows, (int)ap, s->dtype, (long)p.n_sweep_tiles, (long)p.n_tiles, p.part[0].idx.size(), p.part[1].idx.size());
    uspmv_scs_free(s); if (s2) uspmv_scs_free(s2);
    if (ap) { uspmv_coo_free(dpc); uspmv_coo_free(spc); }
    uspmv_coo_free(coo);
}

// What tests/test_gpu_sweep_ap_hp.py relies on, on the three-part planner itself: for its banded matrix every conversion is accepted, the
// shared line plan (512-row tiles, 512 lines) stages fewer than half of the tiles, and the sweep covers every tile at the staging bound
// of 24 bytes per non-zero for the window / tile shapes the tests use, the defaults among them.
static void run_coverage() {
    uspmv_coo_t *coo = nullptr;
    REQUIRE(uspmv_gen_banded_random(51200, 70, 6000, 0x5EED, 10.0, 0, 51200, &coo) == 0);
    const double t1 = quantile(coo, 0.7), t2 = quantile(coo, 0.35);
    const int layouts[][2] = {{8, 1}, {8, 128}, {32, 1}, {32, 128}, {64, 1}, {64, 128}, {32, 512}, {64, 64}, {32, 32}};
    const int shapes[][2] = {{11, 256}, {12, 1024}, {12, 2048}, {13, 1024}, {13, 4096}, {14, 1024}, {14, 2048}, {14, 4096}, {15, 1024}};
    for (int kind : {DP_HP, SP_HP, DP_SP_HP})
        for (auto &cs : layouts) {
                const int C = cs[0], sigma = cs[1];
                Split sp;
                REQUIRE(make_split(coo, kind, t1, t2, C, sigma, &sp));
                uspmv_tlc_plan lp;
                REQUIRE(uspmv_build_tlc_plan(sp.s[0], sp.s[1], 512, 512, &lp, 4, sp.np == 3 ? sp.s[2] : nullptr) == 0);
                REQUIRE(!lp.valid || lp.n_staged_tiles * 2 < lp.n_tiles);
                int64_t all = 0;
                for (auto &sh : shapes) {
                    if (kind != SP_HP && sh[0] > 14) continue;          // 2^15 doubles do not fit the LDS
                    uspmv_sweep_plan p;
                    REQUIRE(uspmv_build_sweep_plan(sp.s, sp.np, sh[0], sh[1], 24.0, &p) == 0);
                    REQUIRE(p.valid && p.n_sweep_tiles == p.n_tiles && p.rest_chunks.empty());
                    all += p.valid && p.n_sweep_tiles == p.n_tiles;
                }
                printf("coverage %s C=%d sigma=%d: line plan stages %ld of %ld tiles; sweep covers every tile for %ld shapes\n", kind_name(kind), C, sigma,
                       (long)(lp.valid ? lp.n_staged_tiles : 0), (long)lp.n_tiles, (long)all);
                sp.free();
            }
    uspmv_coo_free(coo);
}

int main() {
    // ---- the layout of the existing plans has not moved
    run_before(20000, 40, 3000, 32, 512, 9, 256, false, USPMV_F64, 1e9);
    run_before(9999, 23, 700, 16, 64, 8, 512, false, USPMV_F32, 1e9);
    run_before(5000, 300, 2400, 32, 1, 11, 256, false, USPMV_F64, 1e9);    // tiles with > 255 entries per window: rest list
    run_before(20000, 40, 3000, 32, 512, 10, 2048, true, USPMV_F64, 1e9);
    run_before(7777, 31, 900, 64, 128, 8, 256, true, USPMV_F64, 24.0);     // the staging bound turns tiles down
    run_before(9999, 23, 700, 8, 1, 9, 4096, true, USPMV_F64, 1e9);
    // ---- replay of the two- and three-part plans
    for (int kind : {DP_HP, SP_HP, DP_SP_HP}) {
        run(20000, 40, 3000, 32, 512, 9, 256, kind, false, 1);
        run(20000, 40, 3000, 32, 512, 10, 1024, kind, true, 1);
        run(9999, 23, 700, 8, 64, 8, 512, kind, false, 1);
        run(9999, 23, 700, 1, 1, 9, 4096, kind, true, 1);
        run(7777, 31, 900, 64, 128, 8, 2048, kind, true, 1);
        run(5000, 400, 2400, 32, 1, 11, 256, kind, false, 2, 0.02, 0.01);  // > 255 entries of the hi part in a window (rows at the matrix' edge): such tiles must not sweep
        run(6016, 30, 800, 32, 64, 9, 1024, kind, false, 1, -1.0, -1.0);   // thresholds 0: everything in hi, the other parts empty
        run(6016, 30, 800, 32, 64, 9, 1024, kind, false, 1, 2.0, 2.0);     // thresholds inf: hi empty (and mid: everything in hp)
        run(6016, 30, 800, 64, 1, 10, 256, kind, false, 1, 2.0, -1.0);     // dp_sp_hp: everything in mid
        run(6016, 30, 800, 32, 64, 9, 512, kind, false, 1, 0.98, 0.02);    // thin hi and hp parts: rows empty in some parts only
        run_unsorted(kind);
        // a row block, 3001 x 9999 (tests/test_gpu_nonsquare.py): x windows beyond the padded rows, x of x_len_min elements and no more
        run(9999, 23, 700, 32, 512, 10, 1024, kind, false, 1, 0.7, 0.35, 4001, 7002);
    }
    run_coverage();
    printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
