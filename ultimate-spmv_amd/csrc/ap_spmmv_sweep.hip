// ap[dp_sp] SpMMV on the pair's column-window sweep plan: the block form of scs_spmv_sweep<double, AP> (sweep_kernels.hip).  It reads the
// same plan arrays (uspmv_dmat::SweepPlan on the dp handle) and walks the compacted dp and sp entry streams of a tile once for BS of
// the b vectors: one workgroup per sweep tile, RPL rows of a lane at a time, per row BS dp and BS sp accumulators in double.  Per window the
// 2^wlog X rows are staged in LDS by LDS-DMA for the BS vectors of the pass, and every wave runs its compacted rounds as the
// single-vector kernel does -- one ballot per round and chain gives a lane's position and the advance, the stream pointers stay
// wave-uniform -- with BS x operands from LDS and BS FMAs per owned entry.  b / BS passes inside the one launch.
// Numerics: per (row, v) the dp chain fma(val, X, acc) and the sp chain fma((double)valf, X, acc_b), each in slot order; a lane that
// sits a round out adds nothing, not even a signed zero (the FMAs run under the round's lane mask); stripped padding columns once per
// vector after the last window; Y(r, v) = acc + acc_b.  Column v of Y is bitwise uspmv_spmv_ap of column v of X.
//
// LDS image of a window: it follows X.  Row-major X: row r of the window at r * BS * 8 bytes (W rows of BS doubles taken at stride
// b * 8, one 16-byte DMA piece per lane; an entry's operands are BS / 2 16-byte reads).  Column-major X: BS planes of W doubles, plane w
// = column v0 + w of the window staged straight from the caller's array (no re-layout pass, no workspace; an entry's operands are BS
// 8-byte reads 2^wlog elements apart).  The DMA writes 64 consecutive 16-byte pieces per wave instruction, so each layout of X has
// exactly one image it can be staged into without passing through registers.
#include "uspmv_device.hpp"
#include "sweep_common.hpp"

using namespace uspmv_dev;

namespace {

// Rows of a lane whose accumulators are held at a time (2 * rows * BS doubles) beside the batch registers: 1 024-thread workgroups leave
// a lane 128 registers.  Four rows of four vectors spilled 8-14 registers even at two rounds per batch; two rows of eight fit at two
// rounds per batch (profiles/ap_spmmv_sweep/resource_usage.txt).
constexpr int apsw_group_rows(int bs) { return bs == 2 ? 4 : 2; }

// where a wave stands in the compacted dp / sp streams (a part's values and indices advance together): wave-uniform
struct ApSweepPos { unsigned o0, o1; };

// One window of one of the lane's rows: the dp and the sp chain side by side in batches of U rounds, as sweep_window2 runs them for one
// vector (both batches of loads issued before the first wait; each chain in slot order).  c0 / c1: the row's dp / sp entries in this
// window.  Entry registers of lanes that sit a round out keep a valid window index and a value whose products are never added.
template <int BS, bool XCOL, int U, bool NT>
__device__ __forceinline__ ApSweepPos sweep_window_ap_block(const double *win, const int wlog, const int c0, const int c1, ApSweepPos pos,
                                                            const double *__restrict__ vals, const unsigned short *__restrict__ idx,
                                                            const float *__restrict__ vals1, const unsigned short *__restrict__ idx1,
                                                            double (&a0)[BS], double (&a1)[BS]) {
    struct { const double *v0; const unsigned short *i0; const float *v1; const unsigned short *i1; } p{vals + pos.o0, idx + pos.o0,
                                                                                                        vals1 + pos.o1, idx1 + pos.o1};
    double v0[U];
    float v1[U];
    unsigned ix0[U], ix1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { v0[u] = 0.0; v1[u] = 0.0f; ix0[u] = 0u; ix1[u] = 0u; }
    for (int k0 = 0;; k0 += U) {
        unsigned long long m0[U], m1[U];
        unsigned f0[U + 1], f1[U + 1];
        f0[0] = 0u; f1[0] = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            m0[u] = __ballot(k0 + u < c0);
            m1[u] = __ballot(k0 + u < c1);
            f0[u + 1] = f0[u] + (unsigned)__popcll(m0[u]);
            f1[u + 1] = f1[u] + (unsigned)__popcll(m1[u]);
        }
        if ((m0[0] | m1[0]) == 0ull) break;                  // wave-uniform: both chains of every lane are through this window
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + u < c0) {
                const unsigned off = f0[u] + lanes_below(m0[u]);
                v0[u] = ld_stream_g<NT>(p.v0 + off); ix0[u] = ld_stream_g<NT>(p.i0 + off);
            }
            if (k0 + u < c1) {
                const unsigned off = f1[u] + lanes_below(m1[u]);
                v1[u] = ld_stream_g<NT>(p.v1 + off); ix1[u] = ld_stream_g<NT>(p.i1 + off);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double x[BS];
            window_x<double, BS, XCOL>(win, wlog, ix0[u], x);
            masked_fma_round<BS>(a0, v0[u], x, m0[u]);
            window_x<double, BS, XCOL>(win, wlog, ix1[u], x);
            masked_fma_round<BS>(a1, (double)v1[u], x, m1[u]);
        }
        p.v0 += f0[U]; p.i0 += f0[U];
        p.v1 += f1[U]; p.i1 += f1[U];
        pos.o0 += f0[U]; pos.o1 += f1[U];
    }
    return pos;
}

// colwise: X[col + v*ld], Y[row + v*ld];  rowwise: X[col*b + v], Y[row*b + v].  x_rows: X rows the staging may read (of every vector).
// A lane owns RPL * n_groups rows of the tile and holds the accumulators of RPL of them at a time: where the plan gives a lane more rows
// than 2 * RPL * BS accumulators leave registers for, the tile's windows are walked once per group of RPL rows (the vectors per pass
// stay what LDS allows; a group stages the windows again, as a tile of a quarter or half the rows would).
template <int BS, bool XCOL, bool YCOL, bool NT, int NBUF, int U, int RPL>
__global__ void __launch_bounds__(1024) scs_spmmv_ap_sweep(const int wlog, const int *__restrict__ tile_ids, const int *__restrict__ t_smin,
        const int *__restrict__ t_S, const unsigned long long *__restrict__ t_cnt_off,
        const unsigned *__restrict__ wave_off, const unsigned char *__restrict__ cnt, const double *__restrict__ vals,
        const unsigned short *__restrict__ idx, const int *__restrict__ pad_col,
        const unsigned *__restrict__ wave_off_b, const unsigned char *__restrict__ cnt_b, const float *__restrict__ vals_b,
        const unsigned short *__restrict__ idx_b, const int *__restrict__ pad_col_b,
        const double *__restrict__ X, double *__restrict__ Y, const int b, const long ld, const long x_rows, const long n_store,
        const int n_groups, const int xcd_remap) {
    static_assert(RPL <= apsw_group_rows(BS), "2 * RPL * BS accumulators per lane");
    extern __shared__ __attribute__((aligned(16))) unsigned char apsw_smem[];
    typedef double vec_t __attribute__((ext_vector_type(2)));
    const unsigned bt = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const int T = blockDim.x, nw = T >> 6;              // threads, waves of the workgroup
    const int rpl_all = RPL * n_groups;                 // rows of a lane
    const long R = (long)T * rpl_all;                   // rows of the tile
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tile = tile_ids[bt], smin = t_smin[bt], S = t_S[bt];
    const long W = 1L << wlog;
    const long wdoubles = W * BS;                       // doubles of one buffer
    double *const xs_all = (double *)apsw_smem;          // buffer k starts at double k * wdoubles
    bool first = true;

#pragma unroll 1
    for (int v0 = 0; v0 < b; v0 += BS)                   // one pass over the tile's streams per BS vectors ...
#pragma unroll 1
    for (int h0 = 0; h0 < rpl_all; h0 += RPL) {          // ... and group of RPL rows per lane
        const unsigned char *cp = cnt + t_cnt_off[bt] + (long)h0 * T + threadIdx.x;                 // + h*T + s*R
        const unsigned char *cpb = cnt_b + t_cnt_off[bt] + (long)h0 * T + threadIdx.x;
        auto stage = [&](const int s, const int buf) {
            const long g0 = (long)(smin + s) << wlog;    // first X row of the window
            double *dst = xs_all + (long)buf * wdoubles;
            if constexpr (XCOL) {
                // plane w: W elements of column v0 + w from X + (v0 + w)*ld + g0; one wave instruction = 64 pieces = 128 rows of one column
                const int ppc = (int)(W >> 7);
                for (int p = wave; p < BS * ppc; p += nw) {
                    const int w = p / ppc, q = p - w * ppc;
                    const long r = (long)q * 128 + lane * 2;
                    const long gi = (long)(v0 + w) * ld + g0 + r;
                    const long lo = ((long)w << wlog) + (long)q * 128;     // first double of the wave's 1-KiB run
                    if (g0 + r + 2 <= x_rows) {
                        __builtin_amdgcn_global_load_lds((glb_cvoid_t *)(X + gi), (lds_void_t *)(dst + lo), 16, 0, 0);
                    } else {
#pragma unroll
                        for (int e = 0; e < 2; ++e)
                            if (g0 + r + e < x_rows) dst[lo + lane * 2 + e] = X[gi + e];
                    }
                }
            } else {
                // piece q of the window = two doubles of X row q / (BS / 2); a row's BS doubles never cross the end of X
                constexpr int PPR = BS / 2;
                const int n_inst = (int)((W * PPR) >> 6);
                for (int p = wave; p < n_inst; p += nw) {
                    const long q = (long)p * 64 + lane;
                    const long r = q / PPR;
                    const int k = (int)(q - r * PPR);
                    if (g0 + r < x_rows)
                        __builtin_amdgcn_global_load_lds((glb_cvoid_t *)(X + (g0 + r) * b + v0 + 2 * k), (lds_void_t *)(dst + (long)p * 128), 16, 0, 0);
                }
            }
        };

        ApSweepPos pr[RPL];
#pragma unroll
        for (int h = 0; h < RPL; ++h) {
            const unsigned o = (unsigned)__builtin_amdgcn_readfirstlane(wave_off[bt * (nw * rpl_all) + (h0 + h) * nw + wave]);
            const unsigned ob = (unsigned)__builtin_amdgcn_readfirstlane(wave_off_b[bt * (nw * rpl_all) + (h0 + h) * nw + wave]);
            pr[h] = ApSweepPos{o, ob};
        }
        double acc[RPL][BS], acc_b[RPL][BS];
        // the rows' entry counts in the current / next window, one byte per row of the lane (a count is a byte in the plan as well)
        unsigned c_cur = 0u, cb_cur = 0u;
#pragma unroll
        for (int h = 0; h < RPL; ++h) {
#pragma unroll
            for (int w = 0; w < BS; ++w) { acc[h][w] = 0.0; acc_b[h][w] = 0.0; }
            if (S > 0) { c_cur |= (unsigned)cp[h * T] << (8 * h); cb_cur |= (unsigned)cpb[h * T] << (8 * h); }
        }
        if (!first) __syncthreads();                      // everybody is through with the last window of the previous pass
        first = false;
        if (NBUF == 2 && S > 0) stage(0, 0);
        for (int s = 0; s < S; ++s) {
            const int cb = NBUF == 2 ? (s & 1) : 0;
            const double *cur = xs_all + (long)cb * wdoubles;
            if (NBUF == 1) {
                __syncthreads();                          // everybody is through with window s-1
                stage(s, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's share of window s has landed
            __syncthreads();
            unsigned c_next = 0u, cb_next = 0u;
            if (s + 1 < S) {
                if (NBUF == 2) stage(s + 1, cb ^ 1);      // that buffer was read last in window s-1: all waves are past it
#pragma unroll
                for (int h = 0; h < RPL; ++h) {
                    c_next |= (unsigned)cp[(long)(s + 1) * R + h * T] << (8 * h);
                    cb_next |= (unsigned)cpb[(long)(s + 1) * R + h * T] << (8 * h);
                }
            }
#pragma unroll
            for (int h = 0; h < RPL; ++h)
                pr[h] = sweep_window_ap_block<BS, XCOL, U, NT>(cur, wlog, (int)((c_cur >> (8 * h)) & 0xFFu), (int)((cb_cur >> (8 * h)) & 0xFFu),
                                                              pr[h], vals, idx, vals_b, idx_b, acc[h], acc_b[h]);
            c_cur = c_next; cb_cur = cb_next;
        }
        // trailing padding of the row, applied once per vector (see sweep_plan.cpp)
#pragma unroll
        for (int h = 0; h < RPL; ++h) {
            const long row = (long)tile * R + (long)(h0 + h) * T + threadIdx.x;
            const int pc = pad_col[(long)bt * R + (long)(h0 + h) * T + threadIdx.x];
            const int pcb = pad_col_b[(long)bt * R + (long)(h0 + h) * T + threadIdx.x];
#pragma unroll
            for (int w = 0; w < BS; ++w) {
                if (pc >= 0) acc[h][w] = __builtin_fma(0.0, XCOL ? X[(long)pc + (long)(v0 + w) * ld] : X[(long)pc * b + v0 + w], acc[h][w]);
                if (pcb >= 0)
                    acc_b[h][w] = __builtin_fma((double)0.0f, XCOL ? X[(long)pcb + (long)(v0 + w) * ld] : X[(long)pcb * b + v0 + w], acc_b[h][w]);
            }
            if (row < n_store) {
                if constexpr (YCOL) {
#pragma unroll
                    for (int w = 0; w < BS; ++w) st_y<NT>(Y + (row + (long)(v0 + w) * ld), acc[h][w] + acc_b[h][w]);
                } else {
                    vec_t *yp = (vec_t *)(Y + row * b + v0);
#pragma unroll
                    for (int k = 0; k < BS / 2; ++k) {
                        vec_t t;
                        t[0] = acc[h][2 * k] + acc_b[h][2 * k]; t[1] = acc[h][2 * k + 1] + acc_b[h][2 * k + 1];
                        st_y<NT>(yp + k, t);
                    }
                }
            }
        }
    }
}

template <int BS, bool COL, bool NT, int NBUF, int RPL>
void apsw_launch(const uspmv_dmat *dp, const double *X, double *Y, int b, long ld, int threads, int n_groups, hipStream_t st) {
    // (rounds per batch: the batch registers of both chains stand beside 2 * RPL * BS accumulators -- four, and two where those are 32)
    constexpr int U = RPL * BS >= 16 ? 2 : 4;
    auto kfn = scs_spmmv_ap_sweep<BS, COL, COL, NT, NBUF, U, RPL>;
    const auto &w = dp->sw;
    const auto &p0 = w.part[0], &p1 = w.part[1];          // the dp and the sp part
    const size_t lds = (size_t)NBUF * ((size_t)8 << w.wlog) * BS;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // X rows the staging may read: the columns the matrix references, and within one column of a column-major X at most ld
    const long x_rows = COL ? std::min<long>((long)w.x_len, ld) : (long)w.x_len;
    hipLaunchKernelGGL(kfn, dim3((unsigned)w.n_tiles), dim3(threads), lds, st, w.wlog, w.tile_ids.get(), w.smin.get(), w.S.get(),
                       (const unsigned long long *)w.cnt_off, p0.wave_off.get(), p0.cnt.get(), (const double *)p0.vals, p0.idx.get(),
                       p0.pad.get(), p1.wave_off.get(), p1.cnt.get(), (const float *)p1.vals, p1.idx.get(), p1.pad.get(), X, Y, b, ld,
                       x_rows, (long)dp->n_store, n_groups, g_tune.sweep_remap);
}

// rpl: rows of a lane (1, 2 or 4), held apsw_group_rows(BS) at a time
template <int BS, bool COL, bool NT, int NBUF>
void apsw_launch_r(const uspmv_dmat *dp, const double *X, double *Y, int b, long ld, int threads, int rpl, hipStream_t st) {
    constexpr int G = apsw_group_rows(BS);
    if constexpr (G >= 4) { if (rpl == 4) { apsw_launch<BS, COL, NT, NBUF, 4>(dp, X, Y, b, ld, threads, 1, st); return; } }
    if (rpl >= 2) apsw_launch<BS, COL, NT, NBUF, 2>(dp, X, Y, b, ld, threads, rpl / 2, st);
    else apsw_launch<BS, COL, NT, NBUF, 1>(dp, X, Y, b, ld, threads, 1, st);
}

template <int BS>
void apsw_launch_bs(const uspmv_dmat *dp, const double *X, double *Y, int b, long ld, bool col, int threads, int rpl, hipStream_t st) {
    // (the second buffer only where two windows of BS vectors fit)
    const bool two = g_tune.sweep_nbuf == 2 && 2 * ((size_t)8 << dp->sw.wlog) * BS <= WG_LDS_BYTES;
    const bool nt = g_tune.nontemporal != 0;
#define APSW_NB(COLV, NTV) do { if (two) apsw_launch_r<BS, COLV, NTV, 2>(dp, X, Y, b, ld, threads, rpl, st); \
                                else apsw_launch_r<BS, COLV, NTV, 1>(dp, X, Y, b, ld, threads, rpl, st); } while (0)
    if (col) { if (nt) APSW_NB(true, true); else APSW_NB(true, false); }
    else { if (nt) APSW_NB(false, true); else APSW_NB(false, false); }
#undef APSW_NB
}

}  // namespace

namespace uspmv_dev {

int spmmv_ap_sweep_vectors(int b, int wlog) { return sweep_vectors(b, wlog, sizeof(double)); }
int spmmv_ap_sweep_bs(const uspmv_dmat *dp, int b) { return sweep_block_bs(dp->sw, b, sizeof(double)); }

int launch_spmmv_ap_sweep(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, int b, long ld, bool colwise, int bs,
                          hipStream_t st) {
    if (dp->sw.n_tiles > 0) {
        const int threads = sweep_threads(dp->sw);
        const int rpl = dp->sw.tile_rows / threads;
        if (bs == 8) apsw_launch_bs<8>(dp, X, Y, b, ld, colwise, threads, rpl, st);
        else if (bs == 4) apsw_launch_bs<4>(dp, X, Y, b, ld, colwise, threads, rpl, st);
        else apsw_launch_bs<2>(dp, X, Y, b, ld, colwise, threads, rpl, st);
        HIP_TRY(hipGetLastError());
    }
    // the tiles that do not sweep: lane per row over the plan's rest chunks, the same chains
    return launch_spmmv_ap_chunks(dp, sp, dp->sw.rest, (long)dp->sw.n_rest, X, Y, b, ld, colwise ? USPMV_COLWISE : USPMV_ROWWISE, st);
}

}  // namespace uspmv_dev
