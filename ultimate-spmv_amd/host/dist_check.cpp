// Host side of uspmv_dist_check (csrc/uspmv_dist_api.hip): the y a distributed step MUST produce for the rows of one block,
// evaluated straight from the block's COO entries -- global column ids, the x vector a closed form of the global column --
// as one FMA chain per row in entry order.  That is the summation order of every kernel of the path (column order
// inside a row = file order = order of the FMA chain, code/kernels.hpp:242-246), so the comparison is bitwise and covers
// partition, halo discovery, exchange plan, exchange and kernels at any size.  It plays the part of the reference's MKL
// validation (code/write_results.hpp:442-556); it is a checker, never a result.
#include <algorithm>
#include <cmath>

#include "uspmv_internal.hpp"

namespace uspmv {

double check_x(int64_t g) { return 1.0 + 1e-3 * (double)(g % 1000); }

// loopback: a halo column j owned by block p is served by THIS block's row j - wsa[p] (equal block heights)
int64_t check_col(int64_t j, const int32_t *wsa, int P, int rank, bool loopback) {
    if (!loopback) return j;
    const int p = (int)(std::upper_bound(wsa, wsa + P + 1, (int32_t)j) - wsa) - 1;
    return p == rank || p < 0 || p >= P ? j : (int64_t)wsa[rank] + (j - wsa[p]);
}

template <typename VT>
static void rows(const uspmv_coo *m, const int32_t *wsa, int P, int rank, bool loopback, VT *y) {
    const int64_t n = m->n_rows, nnz = m->nnz;
    bool sorted = true;
    for (int64_t k = 1; k < nnz && sorted; ++k) sorted = m->I[(size_t)k] >= m->I[(size_t)k - 1];
    auto xval = [&](int32_t j) { return (VT)check_x(check_col(j, wsa, P, rank, loopback)); };
    if (!sorted) {
        for (int64_t i = 0; i < n; ++i) y[i] = VT(0);
        for (int64_t k = 0; k < nnz; ++k) {
            VT &a = y[m->I[(size_t)k]];
            a = std::fma((VT)m->values[(size_t)k], xval(m->J[(size_t)k]), a);
        }
        return;
    }
    std::vector<int64_t> rp((size_t)n + 1, 0);
    for (int64_t k = 0; k < nnz; ++k) ++rp[(size_t)m->I[(size_t)k] + 1];
    for (int64_t i = 0; i < n; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
        VT a = VT(0);
        for (int64_t k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k) a = std::fma((VT)m->values[(size_t)k], xval(m->J[(size_t)k]), a);
        y[i] = a;
    }
}

// what every reference below asks of its block: the arguments, and row ids inside the block (rows() indexes y by them)
static int check_block(const uspmv_coo *local, const int32_t *wsa, const void *y_ref) {
    if (!local || !wsa || !y_ref) return fail(USPMV_ERR_INVALID, "uspmv_dist_check: NULL argument");
    for (int64_t k = 0; k < local->nnz; ++k)
        if (local->I[(size_t)k] < 0 || local->I[(size_t)k] >= local->n_rows) return fail(USPMV_ERR_INVALID, "uspmv_dist_check: row id outside the block");
    return USPMV_OK;
}

int dist_reference_rows(const uspmv_coo *local, const int32_t *wsa, int P, int rank, bool loopback, int dtype, void *y_ref) {
    if (int rc = check_block(local, wsa, y_ref)) return rc;
    if (dtype == USPMV_F64) rows<double>(local, wsa, P, rank, loopback, (double *)y_ref);
    else rows<float>(local, wsa, P, rank, loopback, (float *)y_ref);
    return USPMV_OK;
}

// ap[dp_sp]: the block split as the object's set-up splits it (the sp part holds (double)(float)v), one chain per part, y = dp + sp
int dist_reference_rows_ap(const uspmv_coo *local, const int32_t *wsa, int P, int rank, bool loopback, double threshold_1, double *y_ref) {
    if (int rc = check_block(local, wsa, y_ref)) return rc;
    uspmv_coo *dp = nullptr, *sp = nullptr;
    if (int rc = uspmv_partition_precisions(local, threshold_1, &dp, &sp)) return rc;
    std::vector<double> ys((size_t)std::max<int64_t>(local->n_rows, 1));
    rows<double>(dp, wsa, P, rank, loopback, y_ref);
    rows<double>(sp, wsa, P, rank, loopback, ys.data());
    for (int64_t i = 0; i < local->n_rows; ++i) y_ref[i] += ys[(size_t)i];
    uspmv_coo_free(dp); uspmv_coo_free(sp);
    return USPMV_OK;
}

// one part of ap[sp_hp]: x float, every product rounded to float and then added to the row's double accumulator (ap_step(float, float, double)
// of the kernels; the part's values are floats, resp. binary16 values, held in doubles)
static void rows_float_products(const uspmv_coo *m, const int32_t *wsa, int P, int rank, bool loopback, double *acc) {
    for (int64_t i = 0; i < m->n_rows; ++i) acc[i] = 0.0;
    for (int64_t k = 0; k < m->nnz; ++k) {
        const float v = (float)m->values[(size_t)k], x = (float)check_x(check_col(m->J[(size_t)k], wsa, P, rank, loopback));
        const float prod = v * x;
        acc[m->I[(size_t)k]] += (double)prod;
    }
}

// the kinds with an fp16 part: the block split as the object's set-up splits it (uspmv_partition_precisions_hp: sp values (double)(float)v, hp
// values rounded once to binary16), the numerics of uspmv_spmv_ap_hp
int dist_reference_rows_ap_hp(const uspmv_coo *local, const int32_t *wsa, int P, int rank, bool loopback, int kind, double threshold_1,
                              double threshold_2, void *y_ref) {
    if (int rc = check_block(local, wsa, y_ref)) return rc;
    uspmv_coo *hi = nullptr, *mid = nullptr, *hp = nullptr;
    if (int rc = uspmv_partition_precisions_hp(local, kind, threshold_1, threshold_2, &hi, kind == USPMV_AP_DP_SP_HP ? &mid : nullptr, &hp)) return rc;
    const int64_t n = local->n_rows;
    std::vector<double> a((size_t)std::max<int64_t>(n, 1)), b(a.size()), c(a.size());
    if (kind == USPMV_AP_SP_HP) {
        rows_float_products(hi, wsa, P, rank, loopback, a.data());
        rows_float_products(hp, wsa, P, rank, loopback, c.data());
        for (int64_t i = 0; i < n; ++i) ((float *)y_ref)[i] = (float)(a[(size_t)i] + c[(size_t)i]);
    } else {
        rows<double>(hi, wsa, P, rank, loopback, a.data());
        if (mid) rows<double>(mid, wsa, P, rank, loopback, b.data());
        rows<double>(hp, wsa, P, rank, loopback, c.data());
        for (int64_t i = 0; i < n; ++i) ((double *)y_ref)[i] = mid ? (a[(size_t)i] + b[(size_t)i]) + c[(size_t)i] : a[(size_t)i] + c[(size_t)i];
    }
    uspmv_coo_free(hi); uspmv_coo_free(mid); uspmv_coo_free(hp);
    return USPMV_OK;
}

}  // namespace uspmv

// The rows of the check on the host alone (no GPU): y_ref[i] = the entry-ordered FMA chain of local row i over
// x_global[j] = 1 + 1e-3 (j mod 1000) -- what uspmv_dist_check compares the device's y with; for steps that do not run on a
// uspmv_dist object (the torch.distributed twin of bench.py).
extern "C" int uspmv_dist_check_reference(const uspmv_coo_t *local, const int32_t *wsa, int rank, int P, int dtype, void *y_ref) {
    if (P < 1 || rank < 0 || rank >= P) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_check_reference: bad rank / P");
    if (dtype != USPMV_F64 && dtype != USPMV_F32) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_check_reference: unknown dtype %d", dtype);
    return uspmv::dist_reference_rows(local, wsa, P, rank, /*loopback=*/false, dtype, y_ref);
}

// ... and for an ap[dp_sp] object: the dp chain over |v| >= threshold_1, the sp chain over the others with (double)(float)v, y = dp + sp
extern "C" int uspmv_dist_check_reference_ap(const uspmv_coo_t *local, const int32_t *wsa, int rank, int P, double threshold_1, double *y_ref) {
    if (P < 1 || rank < 0 || rank >= P) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_check_reference_ap: bad rank / P");
    return uspmv::dist_reference_rows_ap(local, wsa, P, rank, /*loopback=*/false, threshold_1, y_ref);
}

// ... and for an object of a kind with an fp16 part (uspmv_dist_create_ap_hp_from_coo): parts as uspmv_partition_precisions_hp makes them, one
// chain per part in entry order, y_ref in the type of the hi part (float for USPMV_AP_SP_HP, else double)
extern "C" int uspmv_dist_check_reference_ap_hp(const uspmv_coo_t *local, const int32_t *wsa, int rank, int P, int kind, double threshold_1,
                                                double threshold_2, void *y_ref) {
    if (P < 1 || rank < 0 || rank >= P) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_check_reference_ap_hp: bad rank / P");
    if (kind != USPMV_AP_DP_HP && kind != USPMV_AP_SP_HP && kind != USPMV_AP_DP_SP_HP)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_check_reference_ap_hp: unknown kind %d", kind);
    return uspmv::dist_reference_rows_ap_hp(local, wsa, P, rank, /*loopback=*/false, kind, threshold_1, threshold_2, y_ref);
}
