// Stand-alone host program for the sanitizer pass over host/dist_check.cpp and host/halo_plan.cpp (README.md, "Host memory safety"): for
// every block of a small stencil cut P = 2 and P = 3 ways and every kind of object, the host half of the distributed set-up -- split,
// convert, the one halo of all parts, column permutation, chunk classes -- and the three references of the self-check, plus their
// refusals.  Also checks on the host what the merged set-up relies on: a chunk is in uspmv_scs_split_chunks' boundary list exactly when
// its class is not 0.  No device, no Python.
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I ultimate-spmv_amd/host
//       profiles/dist_setup/host_sanitizer_check.cpp ultimate-spmv_amd/host/{dist_check,halo_plan,scs_convert,gen_matrix,comm_plan,debug}.cpp ...
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "uspmv.h"

#define OK(call) do { if (int rc_ = (call)) { fprintf(stderr, "%s:%d: %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, uspmv_last_error()); exit(1); } } while (0)
#define REFUSED(call) do { if ((call) == USPMV_OK) { fprintf(stderr, "%s:%d: %s was not refused\n", __FILE__, __LINE__, #call); exit(1); } } while (0)

enum { ONE = -1 };

int main() {
    const int64_t C = 4, sigma = 8;
    const double t1 = 2.4, t2 = 0.016;
    uspmv_coo_t *tot = nullptr;
    OK(uspmv_gen_stencil27(6, 5, 4, 1, 0, 6.0, 0, 120, &tot));
    int64_t n = 0, nc = 0, nnz = 0;
    OK(uspmv_coo_dims(tot, &n, &nc, &nnz));
    long blocks = 0;
    for (int P = 2; P <= 3; ++P) {
        std::vector<int32_t> wsa((size_t)P + 1);
        for (int p = 0; p <= P; ++p) wsa[(size_t)p] = (int32_t)(n * p / P);
        for (int rank = 0; rank < P; ++rank) {
            uspmv_coo_t *loc = nullptr;
            OK(uspmv_seg_local_coo(tot, wsa.data(), rank, &loc));
            const int64_t nl = wsa[(size_t)rank + 1] - wsa[(size_t)rank];
            for (int kind : {(int)ONE, (int)USPMV_AP_DP_SP, (int)USPMV_AP_DP_HP, (int)USPMV_AP_SP_HP, (int)USPMV_AP_DP_SP_HP}) {
                // parts by slot: hi, float, fp16
                uspmv_coo_t *coo[3] = {nullptr, nullptr, nullptr};
                int dtype[3] = {kind == USPMV_AP_SP_HP ? USPMV_F32 : USPMV_F64, -1, -1};
                if (kind == USPMV_AP_DP_SP) { OK(uspmv_partition_precisions(loc, t1, &coo[0], &coo[1])); dtype[1] = USPMV_F32; }
                else if (kind != ONE) {
                    const bool three = kind == USPMV_AP_DP_SP_HP;
                    OK(uspmv_partition_precisions_hp(loc, kind, t1, t2, &coo[0], three ? &coo[1] : nullptr, &coo[2]));
                    if (three) dtype[1] = USPMV_F32;
                    dtype[2] = USPMV_F16;
                }
                uspmv_scs_t *s[3] = {nullptr, nullptr, nullptr};
                const int32_t *o2n = nullptr;
                for (int q = 0; q < 3; ++q) {
                    if (dtype[q] < 0) continue;
                    OK(uspmv_convert_to_scs(kind == ONE ? loc : coo[q], C, sigma, dtype[q], o2n, &s[q]));
                    if (q == 0) OK(uspmv_scs_arrays(s[0], nullptr, nullptr, nullptr, nullptr, &o2n, nullptr));
                }
                for (auto *c : coo) uspmv_coo_free(c);
                uspmv_halo_t *halo = nullptr;
                if (kind == ONE) OK(uspmv_halo_discover(s[0], wsa.data(), rank, P, &halo));
                else if (kind == USPMV_AP_DP_SP) OK(uspmv_halo_discover_ap(s[0], s[1], wsa.data(), rank, P, &halo));
                else OK(uspmv_halo_discover_ap_hp(s[0], s[1], s[2], wsa.data(), rank, P, &halo));
                int64_t n_halo = -1;
                OK(uspmv_halo_meta(halo, &n_halo, nullptr, nullptr, nullptr));
                if (n_halo <= 0) { fprintf(stderr, "no halo on rank %d of %d\n", rank, P); return 1; }
                // a second scan of structs already rewritten, and structs that do not belong together: refused, nothing written
                if (kind != ONE && kind != USPMV_AP_DP_SP) {
                    uspmv_halo_t *h2 = nullptr;
                    REFUSED(uspmv_halo_discover_ap_hp(s[0], s[0], s[2], wsa.data(), rank, P, &h2));
                    REFUSED(uspmv_halo_discover_ap_hp(s[0], s[1], nullptr, wsa.data(), rank, P, &h2));
                }
                for (int q = 0; q < 3; ++q) {
                    if (!s[q]) continue;
                    OK(uspmv_permute_scs_cols(s[q], o2n));
                    int64_t meta[8];
                    OK(uspmv_scs_meta(s[q], meta));
                    std::vector<uint8_t> cls((size_t)meta[5] + 1);
                    int32_t pad_col = -2;
                    OK(uspmv_scs_chunk_classes(s[q], nl, cls.data(), &pad_col));
                    int32_t *in = nullptr, *bd = nullptr;
                    int64_t n_in = 0, n_bd = 0;
                    OK(uspmv_scs_split_chunks(s[q], nl, &in, &n_in, &bd, &n_bd));
                    int64_t a = 0, b = 0;
                    for (int64_t c = 0; c < meta[5]; ++c) {
                        const bool ok = cls[(size_t)c] ? (b < n_bd && bd[b++] == c) : (a < n_in && in[a++] == c);
                        if (!ok) { fprintf(stderr, "chunk %ld: class %d against the split lists\n", (long)c, cls[(size_t)c]); return 1; }
                    }
                    if (a != n_in || b != n_bd || pad_col < -1 || (pad_col >= 0 && pad_col < nl)) { fprintf(stderr, "split lists / pad_col\n"); return 1; }
                    uspmv_free(in); uspmv_free(bd);
                }
                for (auto *q : s) uspmv_scs_free(q);
                uspmv_halo_free(halo);
                // the references of the self-check
                std::vector<double> y((size_t)nl);
                if (kind == ONE) {
                    OK(uspmv_dist_check_reference(loc, wsa.data(), rank, P, USPMV_F64, y.data()));
                    OK(uspmv_dist_check_reference(loc, wsa.data(), rank, P, USPMV_F32, y.data()));
                    REFUSED(uspmv_dist_check_reference(loc, wsa.data(), rank, P, USPMV_F64, nullptr));
                    REFUSED(uspmv_dist_check_reference(nullptr, wsa.data(), rank, P, USPMV_F64, y.data()));
                } else if (kind == USPMV_AP_DP_SP) {
                    OK(uspmv_dist_check_reference_ap(loc, wsa.data(), rank, P, t1, y.data()));
                    REFUSED(uspmv_dist_check_reference_ap(loc, nullptr, rank, P, t1, y.data()));
                } else {
                    OK(uspmv_dist_check_reference_ap_hp(loc, wsa.data(), rank, P, kind, t1, t2, y.data()));
                    REFUSED(uspmv_dist_check_reference_ap_hp(loc, wsa.data(), rank, P, kind, t1, t2, nullptr));
                    REFUSED(uspmv_dist_check_reference_ap_hp(loc, wsa.data(), rank, P, USPMV_AP_DP_SP, t1, t2, y.data()));
                }
                ++blocks;
            }
            uspmv_coo_free(loc);
        }
    }
    // a row id outside the block: every reference refuses it before it indexes y
    const int32_t I[2] = {0, 7}, J[2] = {0, 1};
    const double V[2] = {1.0, 0.001};
    const int32_t w1[2] = {0, 2};
    uspmv_coo_t *bad = nullptr;
    double y2[2];
    if (uspmv_coo_create(2, 2, 2, I, J, V, &bad) == USPMV_OK) {
        REFUSED(uspmv_dist_check_reference(bad, w1, 0, 1, USPMV_F64, y2));
        REFUSED(uspmv_dist_check_reference_ap(bad, w1, 0, 1, 0.5, y2));
        REFUSED(uspmv_dist_check_reference_ap_hp(bad, w1, 0, 1, USPMV_AP_DP_HP, 0.5, 0.1, y2));
        uspmv_coo_free(bad);
    }
    uspmv_coo_free(tot);
    printf("host sanitizer check: %ld (block, kind) set-ups and references, no finding\n", blocks);
    return 0;
}
