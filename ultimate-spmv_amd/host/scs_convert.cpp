// COO -> SELL-C-sigma conversion and the small host-side helpers around it.
//
// Contract = reference convert_to_scs (code/utilities.hpp:1842-2104; library twin
// code/interface.hpp:401-656), permute_scs_cols (code/utilities.hpp:1802-1831),
// apply_permutation (:1768-1782), partition_precisions ap[dp_sp] (:2899-2911).
// All integer outputs (chunk_ptrs, chunk_lengths, col_idxs, old_to_new_idx, new_to_old_idx)
// are bit-identical to the reference's for the same input, including
//   * the tie order of the sigma-window sort: the reference calls the UNSTABLE std::sort on
//     std::pair<long,long>{row, length} with the comparator a.second > b.second
//     (:1892-1941); we call the same libstdc++ algorithm on the same element type and
//     comparator, window by window (windows are independent, so they are sorted in parallel);
//   * the fixed_permutation quirks (:1911-1928): row lengths are moved to their new slots but
//     `.first` stays the identity, so old_to_new_idx/new_to_old_idx of such a struct come out
//     as the identity while the entries themselves are placed with fixed_permutation (:2017-2019);
//     padded slots i >= n_rows are re-zeroed AFTER the move (loop order of :1913-1923).
// Unlike the reference the conversion is O(nnz) parallel work (OpenMP over windows / rows) and
// reports 32-bit overflow instead of continuing.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "uspmv_internal.hpp"
#include "uspmv_f16_round.hpp"

// binary16 from a double in ONE rounding step (to nearest, ties to even) and back, with integer operations on the bits (the host
// compiler has no _Float16 here): uspmv_f16_round.hpp, the text the device-side partition compiles as well.
uint16_t uspmv_f64_to_f16(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return uspmv_f64_bits_to_f16(b);
}

double uspmv_f16_to_f64(uint16_t h) {
    const uint64_t b = uspmv_f16_to_f64_bits(h);
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

// Everything of convert_to_scs except the O(nnz) scatter: row lengths, sigma-window sort (or the
// fixed permutation), chunk lengths / pointers, both permutations.  `s` comes back with empty
// col_idxs / values ("layout-only").  row_start (n_rows + 1 offsets into the COO arrays) is filled
// when the COO entries are sorted by row, left empty otherwise.
int uspmv_scs_layout(const uspmv_coo_t *m, int64_t C, int64_t sigma, int dtype, const int32_t *fixed_permutation,
                     uspmv_scs *s, std::vector<int64_t> *row_start, const char *who) {
    if (C < 1 || sigma < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: C and sigma must be >= 1", who);
    if (dtype != USPMV_F64 && dtype != USPMV_F32 && dtype != USPMV_F16) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown dtype %d", who, dtype);
    if (m->n_rows < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: matrix has no rows", who);

    const int64_t n_rows = m->n_rows, nnz = m->nnz;
    const int64_t n_chunks = (n_rows + C - 1) / C;
    const int64_t n_pad = n_chunks * C;
    if (n_pad > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: padded rows exceed int32", who);

    using row_len = std::pair<long, long>;  // {original row, population count}
    std::vector<row_len> rl((size_t)(n_pad + sigma));
    for (int64_t i = 0; i < n_pad; ++i) rl[(size_t)i].first = i;
    // row populations and the sortedness test in one parallel sweep: every thread walks a contiguous piece of
    // the entry list and adds one count per run of equal row indices (one atomic per run, not per entry)
    bool sorted = true;
    const int32_t *I = m->I.data();
#pragma omp parallel
    {
        bool my_sorted = true;
#pragma omp for schedule(static) nowait
        for (int64_t blk = 0; blk < (nnz + 65535) / 65536; ++blk) {
            const int64_t k0 = blk * 65536, k1 = std::min(k0 + 65536, nnz);
            if (k0 > 0 && I[k0 - 1] > I[k0]) my_sorted = false;
            int64_t run_start = k0;
            for (int64_t k = k0 + 1; k <= k1; ++k) {
                if (k == k1 || I[k] != I[k - 1]) {
                    long &cnt = rl[(size_t)I[k - 1]].second;
                    const long add = (long)(k - run_start);
#pragma omp atomic
                    cnt += add;
                    run_start = k;
                }
                if (k < k1 && I[k - 1] > I[k]) my_sorted = false;
            }
        }
        if (!my_sorted) {
#pragma omp atomic write
            sorted = false;
        }
    }
    row_start->clear();
    if (sorted) {
        row_start->assign((size_t)n_rows + 1, 0);
        for (int64_t r = 0; r < n_rows; ++r) (*row_start)[(size_t)r + 1] = (*row_start)[(size_t)r] + rl[(size_t)r].second;
    }

    if (fixed_permutation) {
        for (int64_t i = 0; i < n_rows; ++i)
            if (fixed_permutation[i] < 0 || fixed_permutation[i] >= n_pad)
                return uspmv::fail(USPMV_ERR_INVALID, "%s: fixed_permutation[%lld]=%d out of range", who, (long long)i,
                                   fixed_permutation[i]);
        std::vector<row_len> tmp((size_t)n_pad);
        for (int64_t i = 0; i < n_pad; ++i) {
            tmp[(size_t)i].first = rl[(size_t)i].first;
            if (i < n_rows) tmp[(size_t)fixed_permutation[i]].second = rl[(size_t)i].second;
            else tmp[(size_t)i].second = rl[(size_t)i].second;
        }
        std::copy(tmp.begin(), tmp.end(), rl.begin());
    } else {
        const int64_t n_win = (n_pad + sigma - 1) / sigma;
#pragma omp parallel for schedule(dynamic, 64)
        for (int64_t w = 0; w < n_win; ++w) {
            int64_t b = w * sigma, e = std::min(b + sigma, n_pad);
            std::sort(rl.begin() + b, rl.begin() + e,
                      [](const row_len &a, const row_len &b2) { return a.second > b2.second; });
        }
    }

    s->C = C; s->sigma = sigma; s->n_rows = n_rows; s->n_cols = m->n_cols; s->nnz = nnz;
    s->n_chunks = n_chunks; s->n_rows_padded = n_pad; s->dtype = dtype;
    s->chunk_lengths.assign((size_t)n_chunks, 0);
    s->chunk_ptrs.assign((size_t)n_chunks + 1, 0);

    int64_t cur = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        long mx = 0;
        for (int64_t i = 0; i < C; ++i) mx = std::max(mx, rl[(size_t)(c * C + i)].second);
        s->chunk_lengths[(size_t)c] = (int32_t)mx;
        s->chunk_ptrs[(size_t)c] = (int32_t)cur;
        cur += mx * C;
        if (cur > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: chunk_ptrs exceed the 32-bit index type", who);
    }
    s->chunk_ptrs[(size_t)n_chunks] = (int32_t)cur;
    s->n_elements = cur;

    s->old_to_new_idx.assign((size_t)n_rows, 0);
    for (int64_t i = 0; i < n_pad; ++i) {
        long old_row = rl[(size_t)i].first;
        if (old_row < n_rows) s->old_to_new_idx[(size_t)old_row] = (int32_t)i;
    }
    s->new_to_old_idx.assign((size_t)n_rows, 0);
    for (int64_t i = 0; i < n_rows; ++i) {
        int32_t p = s->old_to_new_idx[(size_t)i];
        if (p < n_rows) s->new_to_old_idx[(size_t)p] = (int32_t)i;  // (reference writes out of bounds otherwise)
    }
    if (fixed_permutation && sorted) {
        // a non-empty row mapped onto a slot of a shorter chunk would overrun it (the reference does, code/utilities.hpp:1919-1922)
        for (int64_t r = 0; r < n_rows; ++r)
            if ((*row_start)[(size_t)r + 1] - (*row_start)[(size_t)r] > s->chunk_lengths[(size_t)(fixed_permutation[r] / C)])
                return uspmv::fail(USPMV_ERR_INVALID,
                                   "%s: fixed_permutation maps a non-empty row onto a padded slot "
                                   "(the reference overruns its chunk here, code/utilities.hpp:1919-1922)", who);
    }
    return USPMV_OK;
}

extern "C" {

int uspmv_convert_to_scs(const uspmv_coo_t *m, int64_t C, int64_t sigma, int dtype,
                         const int32_t *fixed_permutation, uspmv_scs_t **out) {
    if (!m || !out) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_convert_to_scs: NULL argument");
    auto *s = new uspmv_scs;
    std::vector<int64_t> row_start;
    if (int rc = uspmv_scs_layout(m, C, sigma, dtype, fixed_permutation, s, &row_start, "uspmv_convert_to_scs")) { delete s; return rc; }
    const int64_t n_rows = m->n_rows, nnz = m->nnz, n_pad = s->n_rows_padded, cur = s->n_elements;

    // ---- fill, preserving the COO order inside every row
    s->col_idxs.assign((size_t)cur, 0);  // padding: column 0 (code/utilities.hpp:1991-2002)
    if (dtype == USPMV_F64) s->values_f64.assign((size_t)cur, 0.0);
    else if (dtype == USPMV_F32) s->values_f32.assign((size_t)cur, 0.0f);
    else s->values_f16.assign((size_t)cur, 0);

    const int32_t *row_map = fixed_permutation ? fixed_permutation : s->old_to_new_idx.data();
    int bad = 0;
    auto place = [&](int64_t k, int64_t slot) {
        int64_t row = row_map[m->I[(size_t)k]];
        int64_t c = row / C;
        if (slot >= s->chunk_lengths[(size_t)c]) { bad = 1; return; }
        int64_t idx = (int64_t)s->chunk_ptrs[(size_t)c] + slot * C + row % C;
        s->col_idxs[(size_t)idx] = m->J[(size_t)k];
        if (dtype == USPMV_F64) s->values_f64[(size_t)idx] = m->values[(size_t)k];
        else if (dtype == USPMV_F32) s->values_f32[(size_t)idx] = (float)m->values[(size_t)k];
        else s->values_f16[(size_t)idx] = uspmv_f64_to_f16(m->values[(size_t)k]);
    };
    if (!row_start.empty()) {
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < n_rows; ++r)
            for (int64_t k = row_start[(size_t)r]; k < row_start[(size_t)r + 1]; ++k) place(k, k - row_start[(size_t)r]);
    } else {
        std::vector<int32_t> fill((size_t)n_pad, 0);
        for (int64_t k = 0; k < nnz; ++k) {
            int64_t row = row_map[m->I[(size_t)k]];
            place(k, fill[(size_t)row]++);
        }
    }
    if (bad) {
        delete s;
        return uspmv::fail(USPMV_ERR_INVALID,
                           "uspmv_convert_to_scs: fixed_permutation maps a non-empty row onto a padded slot "
                           "(the reference overruns its chunk here, code/utilities.hpp:1919-1922)");
    }
    *out = s;
    return USPMV_OK;
}

int uspmv_scs_meta(const uspmv_scs_t *s, int64_t meta[8]) {
    if (!s || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_scs_meta: NULL argument");
    meta[0] = s->C; meta[1] = s->sigma; meta[2] = s->n_rows; meta[3] = s->n_cols;
    meta[4] = s->n_rows_padded; meta[5] = s->n_chunks; meta[6] = s->n_elements; meta[7] = s->nnz;
    return USPMV_OK;
}

int uspmv_scs_dtype(const uspmv_scs_t *s, int *dtype) {
    if (!s || !dtype) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_scs_dtype: NULL argument");
    *dtype = s->dtype;
    return USPMV_OK;
}

int uspmv_scs_arrays(const uspmv_scs_t *s, const int32_t **chunk_ptrs, const int32_t **chunk_lengths,
                     const int32_t **col_idxs, const void **values, const int32_t **old_to_new_idx,
                     const int32_t **new_to_old_idx) {
    if (!s) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_scs_arrays: NULL matrix");
    if (chunk_ptrs) *chunk_ptrs = s->chunk_ptrs.data();
    if (chunk_lengths) *chunk_lengths = s->chunk_lengths.data();
    const bool full = uspmv::scs_has_entries(s);      // layout-only structs (uspmv_convert_to_scs_device): NULL
    if (col_idxs) *col_idxs = full ? s->col_idxs.data() : nullptr;
    if (values) *values = full ? s->values_ptr() : nullptr;
    if (old_to_new_idx) *old_to_new_idx = s->old_to_new_idx.data();
    if (new_to_old_idx) *new_to_old_idx = s->new_to_old_idx.data();
    return USPMV_OK;
}

int uspmv_scs_col_idxs_mut(uspmv_scs_t *s, int32_t **col_idxs) {
    if (!s || !col_idxs) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_scs_col_idxs_mut: NULL argument");
    *col_idxs = s->col_idxs.data();
    return USPMV_OK;
}

int uspmv_permute_scs_cols(uspmv_scs_t *s, const int32_t *perm) {
    if (!s || !perm) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_permute_scs_cols: NULL argument");
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_permute_scs_cols: layout-only struct (uspmv_convert_to_scs_device)");
    const int64_t n = s->n_elements, n_rows = s->n_rows;
    int32_t *ci = s->col_idxs.data();
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i)
        if (ci[i] < n_rows) ci[i] = perm[ci[i]];
    return USPMV_OK;
}

void uspmv_scs_free(uspmv_scs_t *s) { delete s; }

// Host twin of uspmv_dmat_update_values_from_arrays (csrc/refresh_kernels.hip): the values of m, a matrix with the pattern s was converted
// from, placed into s -- same checks in the same order, same placement, nothing written before every check has passed.  Row r sits at
// the struct's own old_to_new_idx[r].
int uspmv_scs_update_values(uspmv_scs_t *s, const uspmv_coo_t *m, const int32_t *col_perm, int check_pattern) {
    const char *who = "uspmv_scs_update_values";
    if (!s || !m) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "%s: layout-only struct (its entries live on the device: uspmv_dmat_update_values_from_arrays)", who);
    const int64_t n_rows = s->n_rows, nnz = m->nnz, C = s->C, n_pad = s->n_rows_padded;
    if (m->n_rows != n_rows)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: the matrix has %lld rows, the struct %lld (the pattern changed)", who, (long long)m->n_rows, (long long)n_rows);
    const int32_t *I = m->I.data(), *J = m->J.data();
    for (int64_t k = 0; k < nnz; ++k)
        if (I[k] < 0 || I[k] >= n_rows) return uspmv::fail(USPMV_ERR_INVALID, "%s: a row index lies outside [0, n_rows)", who);
    std::vector<int64_t> start((size_t)n_rows + 1, 0);
    for (int64_t k = 0; k < nnz; ++k) {
        if (k > 0 && I[k] < I[k - 1])
            return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: COO entries must be sorted by row (uspmv_read_mtx and the generators produce that order)", who);
        ++start[(size_t)I[k] + 1];
    }
    for (int64_t r = 0; r < n_rows; ++r) start[(size_t)r + 1] += start[(size_t)r];
    const int32_t *pos = s->old_to_new_idx.data();
    std::vector<int32_t> row_at((size_t)n_pad, -1);
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t p = pos[r];
        if (p < 0 || p >= n_pad) return uspmv::fail(USPMV_ERR_INVALID, "%s: row_pos has an entry outside [0, n_rows_padded)", who);
        if (start[(size_t)r + 1] - start[(size_t)r] > s->chunk_lengths[(size_t)(p / C)])
            return uspmv::fail(USPMV_ERR_INVALID, "%s: a row has more entries than the chunk it sits in is long (the pattern changed)", who);
    }
    for (int64_t r = 0; r < n_rows; ++r) {
        if (row_at[(size_t)pos[r]] >= 0) return uspmv::fail(USPMV_ERR_INVALID, "%s: row_pos sends two rows to one position", who);
        row_at[(size_t)pos[r]] = (int32_t)r;
    }
    auto slot0 = [&](int64_t q) { return (int64_t)s->chunk_ptrs[(size_t)(q / C)] + q % C; };
    if (check_pattern) {
        int64_t bad = -1;
#pragma omp parallel for schedule(static) reduction(max : bad)
        for (int64_t r = 0; r < n_rows; ++r) {
            const int64_t dst = slot0(pos[r]);
            for (int64_t k = start[(size_t)r]; k < start[(size_t)r + 1]; ++k) {        // (bad = nnz - the FIRST offending entry)
                int32_t col = J[k];
                if (col_perm && col >= 0 && col < n_rows) col = col_perm[col];
                if (s->col_idxs[(size_t)(dst + (k - start[(size_t)r]) * C)] != col) bad = std::max(bad, nnz - k);
            }
        }
        if (bad >= 0)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: entry %lld: its column differs from the stored one (the pattern changed)", who, (long long)(nnz - bad));
    }
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < n_pad; ++q) {
        const int64_t dst = slot0(q), L = s->chunk_lengths[(size_t)(q / C)];
        const int32_t r = row_at[(size_t)q];
        const int64_t s0 = r >= 0 ? start[(size_t)r] : 0, n = r >= 0 ? start[(size_t)r + 1] - s0 : 0;
        for (int64_t j = 0; j < L; ++j) {
            const double v = j < n ? m->values[(size_t)(s0 + j)] : 0.0;   // +0 beyond the row's entries; the slot keeps its stored column
            const size_t e = (size_t)(dst + j * C);
            if (s->dtype == USPMV_F64) s->values_f64[e] = v;
            else if (s->dtype == USPMV_F32) s->values_f32[e] = (float)v;
            else s->values_f16[e] = uspmv_f64_to_f16(v);
        }
    }
    return USPMV_OK;
}

int uspmv_coo_equilibrate(uspmv_coo_t *m) {
    // equilibrate_matrix (code/utilities.hpp:2667-2685, -equilibrate 1 of a one-precision run): every value divided
    // by the largest magnitude of its row, then by the largest magnitude of its column in the row-scaled matrix.
    // max and division are order-independent, so the parallel sweeps give the reference's bits.
    if (!m) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_coo_equilibrate: NULL matrix");
    const int64_t nnz = m->nnz;
    for (int pass = 0; pass < 2; ++pass) {
        const uspmv_ivec &idx = pass == 0 ? m->I : m->J;
        std::vector<double> mx((size_t)std::max<int64_t>(pass == 0 ? m->n_rows : m->n_cols, 1), 0.0);
#pragma omp parallel
        {
            std::vector<double> local(mx.size(), 0.0);
#pragma omp for schedule(static) nowait
            for (int64_t k = 0; k < nnz; ++k) {
                const double a = std::fabs(m->values[(size_t)k]);
                if (a > local[(size_t)idx[(size_t)k]]) local[(size_t)idx[(size_t)k]] = a;
            }
#pragma omp critical
            for (size_t r = 0; r < mx.size(); ++r) mx[r] = std::max(mx[r], local[r]);
        }
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < nnz; ++k) m->values[(size_t)k] = m->values[(size_t)k] / mx[(size_t)idx[(size_t)k]];
    }
    return USPMV_OK;
}

int uspmv_coo_equilibrate_scales(uspmv_coo_t *m, double *row_max, double *col_max) {
    // uspmv_coo_equilibrate keeping its two divisor vectors: extract_largest_row_elems, scale_matrix_rows, extract_largest_col_elems,
    // scale_matrix_cols (code/utilities.hpp:2605-2665) in the order of code/main.cpp:1147-1153, the vectors sized n_rows and n_cols.
    // Nothing is written to the values before every refusal has been decided.
    const char *who = "uspmv_coo_equilibrate_scales";
    if (!m || !row_max || !col_max) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    const int64_t nnz = m->nnz, n_rows = m->n_rows, n_cols = m->n_cols;
    const int32_t *I = m->I.data(), *J = m->J.data();
    double *V = m->values.data();
    std::vector<double> r((size_t)std::max<int64_t>(n_rows, 1), 0.0), c((size_t)std::max<int64_t>(n_cols, 1), 0.0);
    int64_t bad_value = -1, bad_div = -1;                   // the first element refused, by either rule
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<double> &mx = pass == 0 ? r : c;
        const int32_t *idx = pass == 0 ? I : J;
#pragma omp parallel
        {
            std::vector<double> local(mx.size(), 0.0);
            int64_t my_value = -1, my_div = -1;
#pragma omp for schedule(static) nowait
            for (int64_t k = 0; k < nnz; ++k) {
                double a = std::fabs(V[k]);
                if (pass == 0) {
                    if (!std::isfinite(a) && my_value < 0) my_value = k;
                } else {
                    if (r[(size_t)I[k]] == 0.0) { if (my_div < 0) my_div = k; continue; }
                    a = std::fabs(V[k] / r[(size_t)I[k]]);
                }
                if (a > local[(size_t)idx[k]]) local[(size_t)idx[k]] = a;
            }
#pragma omp critical
            {
                for (size_t q = 0; q < mx.size(); ++q) mx[q] = std::max(mx[q], local[q]);
                if (my_value >= 0 && (bad_value < 0 || my_value < bad_value)) bad_value = my_value;
                if (my_div >= 0 && (bad_div < 0 || my_div < bad_div)) bad_div = my_div;
            }
        }
        if (bad_value >= 0) return uspmv::fail(USPMV_ERR_INVALID, "%s: element %lld is not finite", who, (long long)bad_value);
        if (bad_div >= 0)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: element %lld lies in a row whose largest magnitude is 0 (0 / 0 has no portable bits)", who,
                               (long long)bad_div);
    }
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < nnz; ++k)
        if (c[(size_t)J[k]] == 0.0) {
#pragma omp critical
            if (bad_div < 0 || k < bad_div) bad_div = k;
        }
    if (bad_div >= 0)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: element %lld lies in a column whose largest row-scaled magnitude is 0 (0 / 0 has no portable bits)",
                           who, (long long)bad_div);
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < nnz; ++k) V[k] = (V[k] / r[(size_t)I[k]]) / c[(size_t)J[k]];
    std::copy(r.begin(), r.begin() + n_rows, row_max);
    std::copy(c.begin(), c.begin() + std::max<int64_t>(n_cols, 0), col_max);
    return USPMV_OK;
}

int uspmv_apply_permutation(void *out, const void *in, const int32_t *perm, int64_t n, int dtype) {
    if (!out || !in || !perm || n < 0) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_apply_permutation: bad argument");
    if (dtype == USPMV_F64) {
        auto *o = (double *)out; auto *i = (const double *)in;
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < n; ++k) o[k] = i[perm[k]];
    } else if (dtype == USPMV_F32) {
        auto *o = (float *)out; auto *i = (const float *)in;
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < n; ++k) o[k] = i[perm[k]];
    } else {
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_apply_permutation: unknown dtype %d", dtype);
    }
    return USPMV_OK;
}

int uspmv_partition_precisions(const uspmv_coo_t *m, double threshold_1, uspmv_coo_t **dp, uspmv_coo_t **sp) {
    if (!m || !dp || !sp) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_partition_precisions: NULL argument");
    auto *d = new uspmv_coo; auto *s = new uspmv_coo;
    d->n_rows = s->n_rows = m->n_rows;
    d->n_cols = s->n_cols = m->n_cols;
    for (int64_t k = 0; k < m->nnz; ++k) {
        double v = m->values[(size_t)k];
        if (std::fabs(v) >= threshold_1) {
            d->I.push_back(m->I[(size_t)k]); d->J.push_back(m->J[(size_t)k]); d->values.push_back(v);
        } else if (std::fabs(v) < threshold_1) {
            s->I.push_back(m->I[(size_t)k]); s->J.push_back(m->J[(size_t)k]);
            s->values.push_back((double)(float)v);  // static_cast<float> (code/utilities.hpp:2907)
        } else {  // NaN fits neither bucket (code/utilities.hpp:2912-2915)
            delete d; delete s;
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_partition_precisions: element %lld fits neither struct",
                               (long long)k);
        }
    }
    d->nnz = (int64_t)d->values.size(); s->nnz = (int64_t)s->values.size();
    *dp = d; *sp = s;
    return USPMV_OK;
}

int uspmv_partition_precisions_hp(const uspmv_coo_t *m, int kind, double threshold_1, double threshold_2, uspmv_coo_t **hi,
                                  uspmv_coo_t **mid, uspmv_coo_t **hp) {
    // partition_precisions of the library API (code/interface.hpp:691-987), non-equilibrated branch, with the parts' values stored as doubles
    // holding the rounded value (as uspmv_partition_precisions stores its sp part)
    const bool three = kind == USPMV_AP_DP_SP_HP;
    if (!m || !hi || !hp || (three && !mid)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_partition_precisions_hp: NULL argument");
    if (kind != USPMV_AP_DP_HP && kind != USPMV_AP_SP_HP && !three)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_partition_precisions_hp: unknown kind %d", kind);
    auto *a = new uspmv_coo, *b = three ? new uspmv_coo : nullptr, *h = new uspmv_coo;
    for (uspmv_coo *p : {a, b, h})
        if (p) { p->n_rows = m->n_rows; p->n_cols = m->n_cols; }
    auto put = [&](uspmv_coo *p, int64_t k, double v) {
        p->I.push_back(m->I[(size_t)k]); p->J.push_back(m->J[(size_t)k]); p->values.push_back(v);
    };
    for (int64_t k = 0; k < m->nnz; ++k) {
        const double v = m->values[(size_t)k], av = std::fabs(v);
        if (av >= threshold_1) put(a, k, kind == USPMV_AP_SP_HP ? (double)(float)v : v);
        else if (three && av <= threshold_1 && av >= threshold_2) put(b, k, (double)(float)v);
        else if (three || av < threshold_1) put(h, k, uspmv_f16_to_f64(uspmv_f64_to_f16(v)));   // (ap[dp_sp_hp]: the else, NaN included)
        else {  // NaN fits neither part of a two-part split
            delete a; delete h;
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_partition_precisions_hp: element %lld fits neither struct", (long long)k);
        }
    }
    for (uspmv_coo *p : {a, b, h})
        if (p) p->nnz = (int64_t)p->values.size();
    *hi = a; *hp = h;
    if (mid) *mid = b;
    return USPMV_OK;
}

int uspmv_partition_precisions_eq(const uspmv_coo_t *m, int kind, double threshold_1, double threshold_2, const double *row_max,
                                  const double *col_max, uspmv_coo_t *parts[3]) {
    // partition_precisions, the config->equilibrate branches (code/utilities.hpp:2883-2896 ap[dp_sp], :2934-2950 ap[dp_hp], :2989-3007
    // ap[sp_hp], :3046-3078 ap[dp_sp_hp]; library twin code/interface.hpp:691-987): every entry is held against its own thresholds
    // t / (largest_col_elems[J] * largest_row_elems[I]); a two-part kind ends in a plain else, so a NaN goes to the low part.
    const char *who = "uspmv_partition_precisions_eq";
    if (!m || !row_max || !col_max || !parts) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (kind != USPMV_AP_DP_HP && kind != USPMV_AP_SP_HP && kind != USPMV_AP_DP_SP_HP && kind != USPMV_AP_DP_SP)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown kind %d", who, kind);
    const bool three = kind == USPMV_AP_DP_SP_HP;
    uspmv_coo *p[3] = {new uspmv_coo, three ? new uspmv_coo : nullptr, new uspmv_coo};
    for (uspmv_coo *q : p)
        if (q) { q->n_rows = m->n_rows; q->n_cols = m->n_cols; }
    auto put = [&](uspmv_coo *q, int64_t k, double v) {
        q->I.push_back(m->I[(size_t)k]); q->J.push_back(m->J[(size_t)k]); q->values.push_back(v);
    };
    for (int64_t k = 0; k < m->nnz; ++k) {
        const double v = m->values[(size_t)k], av = std::fabs(v);
        const double d = col_max[m->J[(size_t)k]] * row_max[m->I[(size_t)k]];
        const double T1 = threshold_1 / d, T2 = threshold_2 / d;
        if (av >= T1) put(p[0], k, kind == USPMV_AP_SP_HP ? (double)(float)v : v);
        else if (three && av <= T1 && av >= T2) put(p[1], k, (double)(float)v);
        else put(p[2], k, kind == USPMV_AP_DP_SP ? (double)(float)v : uspmv_f16_to_f64(uspmv_f64_to_f16(v)));
    }
    for (int q = 0; q < 3; ++q) {
        if (p[q]) p[q]->nnz = (int64_t)p[q]->values.size();
        parts[q] = p[q];
    }
    return USPMV_OK;
}

}  // extern "C"
