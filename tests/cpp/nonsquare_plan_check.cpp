// Host-side facts about a NON-SQUARE matrix that tests/test_gpu_nonsquare.py asserts again on the device: for a COO file (uspmv_coo_save)
// and one (C, sigma) it builds the structs the GPU tests build -- the matrix in dp and sp, the ap[dp_sp] pair and the three splits with
// an fp16 part, columns permuted with the first part's permutation -- runs the host planners on them and prints one line of key=value
// facts per struct or split: which plans are valid, how many tiles they stage or sweep, and x_len_min, which must be 1 + the highest
// column over ALL parts.  tests/test_nonsquare_host.py compares the lines with the table the GPU file asserts.  Test infrastructure only.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "uspmv_internal.hpp"

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const int SWEEPS[3][2] = {{8, 256}, {10, 1024}, {13, 4096}};
static const double MAX_STAGE = 1048576.0;      // "sweep_max_stage" 1 << 20, which the GPU tests plan under

static int64_t x_rows_of(const uspmv_scs *const ss[], int np) {
    int64_t mc = -1;
    for (int w = 0; w < np; ++w) for (int32_t c : ss[w]->col_idxs) mc = std::max<int64_t>(mc, c);
    return mc + 1;
}

// the sweep plan of the parts at the three shapes: "all" every tile sweeps, "none" the planner declines, "some" a mixture
static void sweeps(const uspmv_scs *const ss[], int np, int64_t xr) {
    for (auto &sh : SWEEPS) {
        if (256 % ss[0]->C != 0) { printf(" sweep%d=skip", sh[0]); continue; }
        uspmv_sweep_plan p;
        REQUIRE(uspmv_build_sweep_plan(ss, np, sh[0], sh[1], MAX_STAGE, &p) == 0);
        const int64_t ns = p.valid ? p.n_sweep_tiles : 0;
        if (p.valid) REQUIRE(p.x_len_min == xr);
        printf(" sweep%d=%s:%ld", sh[0], ns == 0 ? "none" : ns == p.n_tiles ? "all" : "some", (long)p.n_tiles);
    }
}

static void one_struct(const uspmv_coo_t *coo, int C, int sigma, int dtype) {
    uspmv_scs_t *s = nullptr;
    REQUIRE(uspmv_convert_to_scs(coo, C, sigma, dtype, nullptr, &s) == 0);
    REQUIRE(uspmv_permute_scs_cols(s, s->old_to_new_idx.data()) == 0);
    const uspmv_scs *const ss[1] = {s};
    const int64_t xr = x_rows_of(ss, 1);
    int64_t parked = 0;
    for (int32_t q : s->old_to_new_idx) parked += q >= s->n_rows;
    printf("struct %s n_pad=%ld x_rows=%ld parked=%ld", dtype == USPMV_F64 ? "f64" : "f32", (long)s->n_rows_padded, (long)xr, (long)parked);
    for (int rows : {256, 512, 1024}) {
        uspmv_tlc_plan p;
        REQUIRE(uspmv_build_tlc_plan(s, nullptr, 512, rows, &p) == 0);
        if (p.valid) REQUIRE(p.x_len_min == xr);
        printf(" line%d=%ld/%ld", rows, (long)(p.valid ? p.n_staged_tiles : 0), (long)p.n_tiles);
    }
    {
        uspmv_tlc_plan p;
        REQUIRE(uspmv_build_tlc_plan(s, nullptr, 4096, 256, &p, /*line_shift=*/0) == 0);
        if (p.valid) REQUIRE(p.x_len_min == xr);
        printf(" elem=%ld/%ld", (long)(p.valid ? p.n_staged_tiles : 0), (long)p.n_tiles);
    }
    sweeps(ss, 1, xr);
    for (int wlog : {9, 11}) {
        if (64 % C != 0) { printf(" bsweep%d=skip", wlog); continue; }
        uspmv_block_sweep_plan p;
        REQUIRE(uspmv_build_block_sweep_plan(s, wlog, 1024, 64, MAX_STAGE, &p) == 0);
        const bool all = p.valid && p.n_sweep_tiles == p.n_tiles && p.rest_chunks.empty();
        if (all) REQUIRE(p.x_rows_min == xr);
        printf(" bsweep%d=%s:%ld", wlog, all ? "all" : "none", (long)p.n_tiles);
    }
    if (C == 32 || C == 64) {
        uspmv_phased_plan p;
        REQUIRE(uspmv_build_phased_plan(s, 256, 8, &p) == 0);
        printf(" phased=%d", (int)p.valid);
        // the line plan of uspmv_dmat_optimize_block under "spmmv_xline" 1 and the default cuts: rows in original order with the ties
        // undone, the phased plan (256-row phases, cuts by dynamic programming at 24), the same with lists of 128-byte lines -- kept
        // when no phase needs more than 256 rows' worth of lines and the lines staged stay below twice the row plan's rows
        uspmv_scs r;
        std::vector<int32_t> row_map;
        const bool moved = uspmv_scs_reorder_rows(s, 1, &r, &row_map) == 1;
        const uspmv_scs *q = moved ? &r : s;
        const int shift = dtype == USPMV_F64 ? 4 : 5;
        uspmv_phased_plan pp, pl;
        REQUIRE(uspmv_build_phased_plan(q, 256, 8, &pp, 0, 24) == 0);
        REQUIRE(uspmv_build_phased_plan(q, 256, 8, &pl, shift) == 0);
        const bool phased_ok = pp.valid && pp.ngp <= 8 && (pp.max_rows_used * 4 + 255) / 256 <= 8;
        const bool line = phased_ok && pl.valid && pl.max_rows_used <= 256 && pl.ngp <= 8 && ((int64_t)pl.xrows.size() << shift) <= 2 * (int64_t)pp.xrows.size();
        printf(" line_plan=%d", (int)line);
    }
    int64_t st[8];
    REQUIRE(uspmv_additive_plan_probe(s, st, nullptr) == 0);
    printf(" additive=%ld/%ld\n", (long)st[0], (long)st[2]);
    uspmv_scs_free(s);
}

// parts: COO parts in the order of the split (hi, [mid,] lo) with their value types
static void one_split(const char *name, uspmv_coo_t *const parts[], const int dtypes[], int np, int C, int sigma) {
    uspmv_scs_t *s[3] = {nullptr, nullptr, nullptr};
    bool ok = uspmv_convert_to_scs(parts[0], C, sigma, dtypes[0], nullptr, &s[0]) == 0;
    REQUIRE(ok);
    for (int w = 1; w < np && ok; ++w) ok = uspmv_convert_to_scs(parts[w], C, sigma, dtypes[w], s[0]->old_to_new_idx.data(), &s[w]) == 0;
    printf("%s", name);
    if (!ok) { printf(" refused\n"); REQUIRE(!"conversion of a part refused"); return; }
    for (int w = 0; w < np; ++w) REQUIRE(uspmv_permute_scs_cols(s[w], s[0]->old_to_new_idx.data()) == 0);
    const uspmv_scs *ss[3] = {s[0], s[1], s[2]};
    const int64_t xr = x_rows_of(ss, np);
    printf(" n_pad=%ld x_rows=%ld x_rows_first=%ld nnz=", (long)s[0]->n_rows_padded, (long)xr, (long)x_rows_of(ss, 1));
    for (int w = 0; w < np; ++w) printf("%s%ld", w ? "," : "", (long)s[w]->nnz);
    {
        uspmv_tlc_plan p;
        REQUIRE(uspmv_build_tlc_plan(ss[0], ss[1], 512, 512, &p, 4, np == 3 ? ss[2] : nullptr) == 0);
        if (p.valid) REQUIRE(p.x_len_min == xr);
        printf(" line512=%ld/%ld", (long)(p.valid ? p.n_staged_tiles : 0), (long)p.n_tiles);
    }
    sweeps(ss, np, xr);
    printf("\n");
    for (int w = 0; w < np; ++w) uspmv_scs_free(s[w]);
}

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s matrix.coo C sigma threshold_dp_sp 'threshold_1,threshold_2'\n", argv[0]); return 2; }
    uspmv_coo_t *coo = nullptr;
    REQUIRE(uspmv_coo_load(argv[1], &coo) == 0);
    if (!coo) return 1;
    const int C = atoi(argv[2]), sigma = atoi(argv[3]);
    const double th = atof(argv[4]);
    double t1 = 0, t2 = 0;
    REQUIRE(sscanf(argv[5], "%lf,%lf", &t1, &t2) == 2);
    REQUIRE(coo->n_rows != coo->n_cols);
    one_struct(coo, C, sigma, USPMV_F64);
    one_struct(coo, C, sigma, USPMV_F32);
    if (th > 0) {
        uspmv_coo_t *p[2] = {nullptr, nullptr};
        REQUIRE(uspmv_partition_precisions(coo, th, &p[0], &p[1]) == 0);
        const int dt[2] = {USPMV_F64, USPMV_F32};
        one_split("dp_sp", p, dt, 2, C, sigma);
        uspmv_coo_free(p[0]); uspmv_coo_free(p[1]);
        const int kinds[3] = {USPMV_AP_DP_HP, USPMV_AP_SP_HP, USPMV_AP_DP_SP_HP};
        const char *names[3] = {"dp_hp", "sp_hp", "dp_sp_hp"};
        for (int k = 0; k < 3; ++k) {
            uspmv_coo_t *hi = nullptr, *mid = nullptr, *hp = nullptr;
            REQUIRE(uspmv_partition_precisions_hp(coo, kinds[k], t1, t2, &hi, &mid, &hp) == 0);
            uspmv_coo_t *q[3] = {hi, mid ? mid : hp, mid ? hp : nullptr};
            const int dq[3] = {kinds[k] == USPMV_AP_SP_HP ? USPMV_F32 : USPMV_F64, mid ? USPMV_F32 : USPMV_F16, USPMV_F16};
            one_split(names[k], q, dq, mid ? 3 : 2, C, sigma);
            uspmv_coo_free(hi); if (mid) uspmv_coo_free(mid); uspmv_coo_free(hp);
        }
    }
    uspmv_coo_free(coo);
    printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
