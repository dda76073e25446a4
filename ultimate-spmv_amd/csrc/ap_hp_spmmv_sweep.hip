// Adaptive precision with an fp16 part on block vectors over the parts' shared column-window sweep plan: the block form of
// scs_spmv_sweep_ap_hp (sweep_ap_hp_kernels.hip); scs_spmmv_ap_sweep (ap_spmmv_sweep.hip) is the same for the ap[dp_sp] pair.  It reads the
// same plan arrays (uspmv_dmat::SweepPlan on the hi handle, parts [hi, hp] or [hi, mid, hp]) and walks every part's compacted stream of
// a tile once for BS of the b vectors: one workgroup per sweep tile, per window the 2^wlog X rows of the pass's BS vectors staged in LDS
// in the type of X, and every wave runs its compacted rounds as the single-vector kernel does -- one ballot per round and chain gives a
// lane's position and the advance, the stream positions stay wave-uniform -- with BS x operands from LDS and BS updates per owned entry
// under the round's lane mask.  b / BS passes inside the one launch.
// Numerics: those of every ap_hp kernel (ap_step / ap_hp_y, uspmv_device.hpp).  Per (row, v) one chain per part in slot order: a double
// X with one FMA in double per entry on the exactly widened value, a float X (ap[sp_hp]) with the product rounded to float and added to
// the part's double accumulator.  A part's chain runs across all windows, so the parts' accumulators stay apart until the end: the
// stripped padding column of every part once per vector after the last window, in the part's own type, then y = hi + hp,
// (hi + mid) + hp or (float)(sp + hp).  A lane that sits a round out changes nothing.  Column v of Y is bitwise uspmv_spmv_ap_hp of
// column v of X.
//
// LDS image of a window: it follows X, as in ap_spmmv_sweep.hip.  Row-major X: row r of the window at r * BS elements (W rows of BS
// elements taken at stride b, by LDS-DMA in 16-byte pieces; float rows of two vectors are 8 bytes, which the DMA has no form for: at
// b = 2 the rows are contiguous and one piece is two rows, else they pass through registers).  Column-major X: BS planes of W elements,
// plane w = column v0 + w of the window straight from the caller's array (no re-layout pass, no workspace).
//
// Registers: 1 024-thread workgroups leave a lane 128.  ap[dp_sp_hp] has three accumulators per (row, vector), so a lane holds the
// accumulators of G rows at a time with G * BS <= 8 (24 doubles at most) and the parts run one after the other inside a window; a plan
// with more rows per lane is walked in groups of G rows that stage the tile's windows again (profiles/ap_hp_spmmv_sweep/resource_usage.txt).
#include "uspmv_device.hpp"
#include "sweep_common.hpp"

using namespace uspmv_dev;

namespace {

constexpr int APHSW_U = 4;                 // rounds per batch

// One window, one part of one of the lane's rows: batches of U rounds over the wave's compacted stream, which starts at element o of
// vals / idx; returns where the next window's starts.  c: the row's entries of this part in this window.  Entry registers of lanes that
// sit a round out keep a valid window index and a value whose products are never added.
template <typename AT, typename HT, int BS, bool XCOL, int U, bool NT>
__device__ __forceinline__ unsigned hpb_window(const HT *win, const int wlog, const int c, const AT *__restrict__ vals,
                                               const unsigned short *__restrict__ idx, unsigned o, double (&acc)[BS]) {
    AT v[U];
    unsigned ix[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { v[u] = AT(0); ix[u] = 0u; }
    for (int k0 = 0;; k0 += U) {
        unsigned long long m[U];
        unsigned first[U + 1];
        first[0] = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            m[u] = __ballot(k0 + u < c);
            first[u + 1] = first[u] + (unsigned)__popcll(m[u]);
        }
        if (m[0] == 0ull) break;                             // wave-uniform: every row of the wave is through this window
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + u < c) {
                const unsigned off = o + first[u] + lanes_below(m[u]);
                v[u] = ld_stream_g<NT>(vals + off); ix[u] = ld_stream_g<NT>(idx + off);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            HT x[BS];
            window_x<HT, BS, XCOL>(win, wlog, ix[u], x);
            if constexpr (sizeof(HT) == 8) {
                masked_fma_round<BS>(acc, hp_widen(v[u], HT(0)), x, m[u]);
            } else {
                double t[BS];
                const float a = hp_widen(v[u], HT(0));
#pragma unroll
                for (int w = 0; w < BS; ++w) t[w] = (double)__fmul_rn(a, x[w]);
                masked_add_round<BS>(acc, t, m[u]);
            }
        }
        o += first[U];
    }
    return o;
}

// HT: type of X, Y and the first part (double, or float for ap[sp_hp]); MID: ap[dp_sp_hp].  XCOL: X[col + v*ld], else X[col*b + v];
// YCOL: Y[row + v*ld], else Y[row*b + v].  x_rows: X rows the staging may read (of every vector).  nbuf: LDS buffers (2: window s+1
// lands while window s is consumed).  A lane owns RPL * n_groups rows of the tile and holds the accumulators of RPL of them at a time.
template <typename HT, bool MID, int BS, bool XCOL, bool YCOL, bool NT, int RPL>
__global__ void __launch_bounds__(1024) scs_spmmv_ap_hp_sweep(const int wlog, const int nbuf, const int *__restrict__ tile_ids,
        const int *__restrict__ t_smin, const int *__restrict__ t_S, const unsigned long long *__restrict__ t_cnt_off,
        const SweepParts P, const HT *__restrict__ X, HT *__restrict__ Y, const int b, const long ld, const long x_rows,
        const long n_store, const int n_groups, const int xcd_remap) {
    static_assert(RPL * BS <= 8, "3 * RPL * BS accumulators per lane");
    extern __shared__ __attribute__((aligned(16))) unsigned char aphsw_smem[];
    constexpr int U = APHSW_U;
    constexpr int EPL = 16 / (int)sizeof(HT);           // elements per 16-byte DMA piece
    const unsigned bt = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const int T = blockDim.x, nw = T >> 6;              // threads, waves of the workgroup
    const int rpl_all = RPL * n_groups;                 // rows of a lane
    const long R = (long)T * rpl_all;                   // rows of the tile
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tile = tile_ids[bt], smin = t_smin[bt], S = t_S[bt];
    const long W = 1L << wlog;
    const long welems = W * BS;                         // elements of one buffer
    HT *const xs_all = (HT *)aphsw_smem;                 // buffer k starts at element k * welems
    const HT *const va0 = (const HT *)P.vals[0];
    const float *const va1 = (const float *)P.vals[1];
    const unsigned short *const va2 = (const unsigned short *)P.vals[2];
    bool first = true;

#pragma unroll 1
    for (int v0 = 0; v0 < b; v0 += BS)                   // one pass over the tile's streams per BS vectors ...
#pragma unroll 1
    for (int h0 = 0; h0 < rpl_all; h0 += RPL) {          // ... and group of RPL rows per lane
        const long coff = (long)t_cnt_off[bt] + (long)h0 * T + threadIdx.x;     // + h*T + s*R: the lane's count byte, in every part's array
        auto stage = [&](const int s, const int buf) {
            const long g0 = (long)(smin + s) << wlog;    // first X row of the window
            HT *dst = xs_all + (long)buf * welems;
            if constexpr (XCOL) {
                // plane w: W elements of column v0 + w from X + (v0 + w)*ld + g0; one wave instruction = 64 pieces of one column
                const int ppc = (int)(W / (64 * EPL));
                for (int p = wave; p < BS * ppc; p += nw) {
                    const int w = p / ppc, q = p - w * ppc;
                    const long r = (long)q * (64 * EPL) + lane * EPL;
                    const long gi = (long)(v0 + w) * ld + g0 + r;
                    const long lo = ((long)w << wlog) + (long)q * (64 * EPL);     // first element of the wave's 1-KiB run
                    if (g0 + r + EPL <= x_rows) {
                        __builtin_amdgcn_global_load_lds((glb_cvoid_t *)(X + gi), (lds_void_t *)(dst + lo), 16, 0, 0);
                    } else {
#pragma unroll
                        for (int e = 0; e < EPL; ++e)
                            if (g0 + r + e < x_rows) dst[lo + lane * EPL + e] = X[gi + e];
                    }
                }
            } else if constexpr (BS >= EPL) {
                // piece q of the window = EPL elements of X row q / PPR; a row's BS elements never cross the end of X
                constexpr int PPR = BS / EPL;
                const int n_inst = (int)((W * PPR) >> 6);
                for (int p = wave; p < n_inst; p += nw) {
                    const long q = (long)p * 64 + lane;
                    const long r = q / PPR;
                    const int k = (int)(q - r * PPR);
                    if (g0 + r < x_rows)
                        __builtin_amdgcn_global_load_lds((glb_cvoid_t *)(X + (g0 + r) * b + v0 + EPL * k),
                                                         (lds_void_t *)(dst + (long)p * (64 * EPL)), 16, 0, 0);
                }
            } else {
                // float X, two vectors: 8-byte rows
                static_assert(sizeof(HT) == 4 && BS == 2, "the one row shorter than a DMA piece");
                typedef HT row_t __attribute__((ext_vector_type(2)));
                if (b == 2) {                            // contiguous rows: one piece = rows 2q and 2q + 1
                    const int n_inst = (int)(W >> 7);
                    for (int p = wave; p < n_inst; p += nw) {
                        const long r = ((long)p * 64 + lane) * 2;
                        if (g0 + r + 2 <= x_rows)
                            __builtin_amdgcn_global_load_lds((glb_cvoid_t *)(X + (g0 + r) * 2), (lds_void_t *)(dst + (long)p * 256), 16, 0, 0);
                        else if (g0 + r < x_rows)
                            *(row_t *)(dst + r * 2) = *(const row_t *)(X + (g0 + r) * 2);
                    }
                } else {                                 // through registers
                    for (long r = threadIdx.x; r < W; r += T)
                        if (g0 + r < x_rows) *(row_t *)(dst + r * 2) = *(const row_t *)(X + (g0 + r) * b + v0);
                }
            }
        };

        unsigned o[RPL][3];
        double acc[3][RPL][BS];
        // the rows' entry counts in the current / next window, one byte per row of the lane and part (a count is a byte in the plan as well)
        unsigned c_cur[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c_cur[k] = 0u;
#pragma unroll
            for (int h = 0; h < RPL; ++h) {
                o[h][k] = 0u;
#pragma unroll
                for (int w = 0; w < BS; ++w) acc[k][h][w] = 0.0;
                if (k != 1 || MID) {
                    o[h][k] = (unsigned)__builtin_amdgcn_readfirstlane(P.wave_off[k][bt * (nw * rpl_all) + (h0 + h) * nw + wave]);
                    if (S > 0) c_cur[k] |= (unsigned)P.cnt[k][coff + h * T] << (8 * h);
                }
            }
        }
        if (!first) __syncthreads();                      // everybody is through with the last window of the previous pass
        first = false;
        if (nbuf == 2 && S > 0) stage(0, 0);
        for (int s = 0; s < S; ++s) {
            const int cb = nbuf == 2 ? (s & 1) : 0;
            const HT *cur = xs_all + (long)cb * welems;
            if (nbuf == 1) {
                __syncthreads();                          // everybody is through with window s-1
                stage(s, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's share of window s has landed
            __syncthreads();
            unsigned c_next[3] = {0u, 0u, 0u};
            if (s + 1 < S) {
                if (nbuf == 2) stage(s + 1, cb ^ 1);      // that buffer was read last in window s-1: all waves are past it
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k != 1 || MID)
#pragma unroll
                        for (int h = 0; h < RPL; ++h) c_next[k] |= (unsigned)P.cnt[k][coff + (long)(s + 1) * R + h * T] << (8 * h);
            }
#pragma unroll
            for (int h = 0; h < RPL; ++h) {               // one part after the other
                o[h][0] = hpb_window<HT, HT, BS, XCOL, U, NT>(cur, wlog, (int)((c_cur[0] >> (8 * h)) & 0xFFu), va0, P.idx[0], o[h][0], acc[0][h]);
                if constexpr (MID)
                    o[h][1] = hpb_window<float, HT, BS, XCOL, U, NT>(cur, wlog, (int)((c_cur[1] >> (8 * h)) & 0xFFu), va1, P.idx[1], o[h][1], acc[1][h]);
                o[h][2] = hpb_window<unsigned short, HT, BS, XCOL, U, NT>(cur, wlog, (int)((c_cur[2] >> (8 * h)) & 0xFFu), va2, P.idx[2], o[h][2],
                                                                          acc[2][h]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) c_cur[k] = c_next[k];
        }
        // trailing padding of every part of the row, applied once per vector in the part's own type (see sweep_plan.cpp)
#pragma unroll
        for (int h = 0; h < RPL; ++h) {
            const long row = (long)tile * R + (long)(h0 + h) * T + threadIdx.x;
            const long pr = (long)bt * R + (long)(h0 + h) * T + threadIdx.x;
            const int pc0 = P.pad[0][pr];
            const int pc1 = MID ? P.pad[1][pr] : -1;
            const int pc2 = P.pad[2][pr];
            auto xel = [&](const int col, const int w) { return XCOL ? X[(long)col + (long)(v0 + w) * ld] : X[(long)col * b + v0 + w]; };
            HT yv[BS];
#pragma unroll
            for (int w = 0; w < BS; ++w) {
                if (pc0 >= 0) acc[0][h][w] = ap_step(HT(0), xel(pc0, w), acc[0][h][w]);
                if constexpr (MID) {
                    if (pc1 >= 0) acc[1][h][w] = ap_step(0.0f, xel(pc1, w), acc[1][h][w]);
                }
                if (pc2 >= 0) acc[2][h][w] = ap_step((unsigned short)0, xel(pc2, w), acc[2][h][w]);
                yv[w] = ap_hp_y<HT, MID>(acc[0][h][w], acc[1][h][w], acc[2][h][w]);
            }
            if (row < n_store) {
                if constexpr (YCOL) {
#pragma unroll
                    for (int w = 0; w < BS; ++w) st_y<NT>(Y + (row + (long)(v0 + w) * ld), yv[w]);
                } else {
                    constexpr int PE = EPL < BS ? EPL : BS;
                    typedef HT piece_t __attribute__((ext_vector_type(PE)));
                    piece_t *yp = (piece_t *)(Y + row * b + v0);
#pragma unroll
                    for (int k = 0; k < BS / PE; ++k) {
                        piece_t t;
#pragma unroll
                        for (int e = 0; e < PE; ++e) t[e] = yv[k * PE + e];
                        st_y<NT>(yp + k, t);
                    }
                }
            }
        }
    }
}

template <typename HT, bool MID, int BS, bool COL, bool NT, int RPL>
void aphsw_launch(const uspmv_dmat *hi, const SweepParts &P, const HT *X, HT *Y, int b, long ld, int threads, int n_groups,
                  hipStream_t st) {
    const auto &w = hi->sw;
    auto kfn = scs_spmmv_ap_hp_sweep<HT, MID, BS, COL, COL, NT, RPL>;
    const size_t win = (sizeof(HT) << w.wlog) * BS;
    // (the second buffer only where two windows of BS vectors fit)
    const int nbuf = (g_tune.sweep_nbuf == 2 && 2 * win <= WG_LDS_BYTES) ? 2 : 1;
    const size_t lds = nbuf * win;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // X rows the staging may read: the columns the matrix references, and within one column of a column-major X at most ld
    const long x_rows = COL ? std::min<long>((long)w.x_len, ld) : (long)w.x_len;
    hipLaunchKernelGGL(kfn, dim3((unsigned)w.n_tiles), dim3(threads), lds, st, w.wlog, nbuf, w.tile_ids.get(), w.smin.get(), w.S.get(),
                       (const unsigned long long *)w.cnt_off, P, X, Y, b, ld, x_rows, (long)hi->n_store, n_groups, g_tune.sweep_remap);
}

// rpl: rows of a lane (1, 2 or 4), held 8 / BS at a time at most
template <typename HT, bool MID, int BS, bool COL, bool NT>
void aphsw_launch_r(const uspmv_dmat *hi, const SweepParts &P, const HT *X, HT *Y, int b, long ld, int threads, int rpl, hipStream_t st) {
    constexpr int G = 8 / BS;
    if constexpr (G >= 4) { if (rpl == 4) { aphsw_launch<HT, MID, BS, COL, NT, 4>(hi, P, X, Y, b, ld, threads, 1, st); return; } }
    if constexpr (G >= 2) { if (rpl >= 2) { aphsw_launch<HT, MID, BS, COL, NT, 2>(hi, P, X, Y, b, ld, threads, rpl / 2, st); return; } }
    aphsw_launch<HT, MID, BS, COL, NT, 1>(hi, P, X, Y, b, ld, threads, rpl, st);
}

template <typename HT, bool MID, int BS>
void aphsw_launch_bs(const uspmv_dmat *hi, const SweepParts &P, const HT *X, HT *Y, int b, long ld, bool col, int threads, int rpl,
                     hipStream_t st) {
    const bool nt = g_tune.nontemporal != 0;
    if (col) { if (nt) aphsw_launch_r<HT, MID, BS, true, true>(hi, P, X, Y, b, ld, threads, rpl, st);
               else aphsw_launch_r<HT, MID, BS, true, false>(hi, P, X, Y, b, ld, threads, rpl, st); }
    else { if (nt) aphsw_launch_r<HT, MID, BS, false, true>(hi, P, X, Y, b, ld, threads, rpl, st);
           else aphsw_launch_r<HT, MID, BS, false, false>(hi, P, X, Y, b, ld, threads, rpl, st); }
}

template <typename HT, bool MID>
int aphsw_launch_kind(const uspmv_dmat *hi, const HT *X, HT *Y, int b, long ld, bool col, int bs, hipStream_t st) {
    const auto &w = hi->sw;
    const SweepParts P = sweep_parts(w);
    const int threads = sweep_threads(w);
    const int rpl = w.tile_rows / threads;
    if (bs == 8) aphsw_launch_bs<HT, MID, 8>(hi, P, X, Y, b, ld, col, threads, rpl, st);
    else if (bs == 4) aphsw_launch_bs<HT, MID, 4>(hi, P, X, Y, b, ld, col, threads, rpl, st);
    else aphsw_launch_bs<HT, MID, 2>(hi, P, X, Y, b, ld, col, threads, rpl, st);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // namespace

namespace uspmv_dev {

int spmmv_ap_hp_sweep_vectors(int b, int wlog, int x_dtype) { return sweep_vectors(b, wlog, x_dtype == USPMV_F32 ? 4 : 8); }
int spmmv_ap_hp_sweep_bs(const uspmv_dmat *hi, int b) { return sweep_block_bs(hi->sw, b, hi->dtype == USPMV_F32 ? 4 : 8); }

int launch_spmmv_ap_hp_sweep(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const void *X, void *Y, int b, long ld,
                             bool colwise, int bs, hipStream_t st) {
    if (hi->sw.n_tiles > 0) {
        int rc;
        if (hi->dtype == USPMV_F32) rc = aphsw_launch_kind<float, false>(hi, (const float *)X, (float *)Y, b, ld, colwise, bs, st);
        else if (mid) rc = aphsw_launch_kind<double, true>(hi, (const double *)X, (double *)Y, b, ld, colwise, bs, st);
        else rc = aphsw_launch_kind<double, false>(hi, (const double *)X, (double *)Y, b, ld, colwise, bs, st);
        if (rc != USPMV_OK) return rc;
    }
    // the tiles that do not sweep: lane per row over the plan's rest chunks, the same chains
    return launch_spmmv_ap_hp_chunks(hi, mid, hp, hi->sw.rest, (long)hi->sw.n_rest, X, Y, b, ld, colwise ? USPMV_COLWISE : USPMV_ROWWISE, st);
}

}  // namespace uspmv_dev
