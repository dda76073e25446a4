// Adaptive-precision dp+sp SpMMV (block vectors): uspmv_spmmv_ap.  The reference has no twin (its CLI stops at "SpMMV is not yet
// implemented for AP kernels", code/utilities.hpp:1389); the numerics are scs_ap_impl_cpu<C> (code/ap_kernels.hpp:24-82) applied to every
// column of X: per (row, v) a dp FMA chain and an sp FMA chain (float value widened, times the DOUBLE x), each in slot order,
// Y(r, v) = dp + sp.  One lane per row everywhere, so column v of Y is bitwise uspmv_spmv_ap of column v of X.  See DESIGN.md 5.7.
#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace {

// Any b, either layout, 8-byte-aligned pointers: the ap twin of scs_spmmv_rows, VB vectors per pass held in registers (2 * VB
// accumulators), the dp chain and then the sp chain of the pass.
// colwise: X[col + v*ld], Y[row + v*ld];  rowwise: X[col*b + v], Y[row*b + v].
// IDS: the chunks chunk_ids[0 .. n_chunks) instead of all (the rest chunks of a column-window sweep plan).
template <int VB, bool ROWWISE, bool NT, bool IDS = false>
__global__ void scs_spmmv_ap_rows(const long n_chunks, const int C, const int *__restrict__ dp_cp, const int *__restrict__ dp_cl,
                                  const int *__restrict__ dp_ci, const double *__restrict__ dp_va, const int *__restrict__ sp_cp,
                                  const int *__restrict__ sp_cl, const int *__restrict__ sp_ci, const float *__restrict__ sp_va,
                                  const double *__restrict__ X, double *__restrict__ Y, const int b, const long ld, const int xcd_remap,
                                  const int *__restrict__ chunk_ids) {
    const unsigned lb = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    long row = (long)lb * blockDim.x + threadIdx.x;
    long c = row / C;
    const int i = (int)(row - c * C);
    if (c >= n_chunks) return;
    if constexpr (IDS) { c = chunk_ids[c]; row = c * C + i; }
    const long dcs = dp_cp[c], scs_ = sp_cp[c];
    const int Ld = dp_cl[c], Ls = sp_cl[c];
    const double *dvp = dp_va + dcs + i;
    const int *dcp = dp_ci + dcs + i;
    const float *svp = sp_va + scs_ + i;
    const int *scp = sp_ci + scs_ + i;
    for (int v0 = 0; v0 < b; v0 += VB) {
        double dt[VB], st[VB];
#pragma unroll
        for (int v = 0; v < VB; ++v) { dt[v] = 0.0; st[v] = 0.0; }
        for (int j = 0; j < Ld; ++j) {
            const double a = ld_stream<NT>(dvp + (long)j * C);
            const long col = ld_stream<NT>(dcp + (long)j * C);
#pragma unroll
            for (int v = 0; v < VB; ++v)
                if (v0 + v < b) dt[v] = __builtin_fma(a, ROWWISE ? X[col * b + v0 + v] : X[col + (long)(v0 + v) * ld], dt[v]);
        }
        for (int j = 0; j < Ls; ++j) {
            const double a = (double)ld_stream<NT>(svp + (long)j * C);
            const long col = ld_stream<NT>(scp + (long)j * C);
#pragma unroll
            for (int v = 0; v < VB; ++v)
                if (v0 + v < b) st[v] = __builtin_fma(a, ROWWISE ? X[col * b + v0 + v] : X[col + (long)(v0 + v) * ld], st[v]);
        }
#pragma unroll
        for (int v = 0; v < VB; ++v) {
            if (v0 + v < b) {
                if (ROWWISE) st_y<NT>(Y + (row * b + v0 + v), dt[v] + st[v]);
                else st_y<NT>(Y + (row + (long)(v0 + v) * ld), dt[v] + st[v]);
            }
        }
    }
}

// ROW-MAJOR X of compile-time width B (X[col*B + v]): per slot a lane reads its whole X row with 16-byte loads, as scs_spmmv_rowmajor
// does; B dp and B sp accumulators per lane.  While both parts still have U slots left, a dp batch and an sp batch are issued together
// (the fused trip of scs_spmv_ap_rows: two independent chains, twice the bytes in flight per wave); each chain still runs in slot order.
// YCOL: Y column-major (Y[row + v*ld]) straight from the accumulators, for column-major callers behind the X re-layout pass.
// CT = 32: slot strides become immediate offsets.  xs: doubles between two rows of X (and of a row-major Y) -- B, or 2 * B where the
// launch covers one half of the vectors of a block of 16.
template <int B, int U, bool NT, bool YCOL, int CT>
__global__ void __launch_bounds__(256) scs_spmmv_ap_rowmajor(const long n_chunks, const int C_rt, const int *__restrict__ dp_cp,
        const int *__restrict__ dp_cl, const int *__restrict__ dp_ci, const double *__restrict__ dp_va, const int *__restrict__ sp_cp,
        const int *__restrict__ sp_cl, const int *__restrict__ sp_ci, const float *__restrict__ sp_va, const double *__restrict__ X,
        double *__restrict__ Y, const long ld, const int xs, const int xcd_remap) {
    constexpr int NV = B / 2;                 // 16-byte pieces per X row
    typedef double vec_t __attribute__((ext_vector_type(2)));
    const int C = CT > 0 ? CT : C_rt;
    const unsigned lb = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const long row = (long)lb * blockDim.x + threadIdx.x;
    const long c = row / C;
    const int i = (int)(row - c * C);
    if (c >= n_chunks) return;
    const long dcs = dp_cp[c], scs_ = sp_cp[c];
    const int Ld = dp_cl[c], Ls = sp_cl[c];
    const double *dvp = dp_va + dcs + i;
    const int *dcp = dp_ci + dcs + i;
    const float *svp = sp_va + scs_ + i;
    const int *scp = sp_ci + scs_ + i;
    double dt[B], st[B];
#pragma unroll
    for (int v = 0; v < B; ++v) { dt[v] = 0.0; st[v] = 0.0; }
    auto x_row = [&](const int col, vec_t (&xr)[NV]) {
        const vec_t *xp = (const vec_t *)(X + (long)col * xs);
#pragma unroll
        for (int k = 0; k < NV; ++k) xr[k] = xp[k];
    };
    auto fma_row = [&](const double a, const vec_t (&xr)[NV], double (&acc)[B]) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            acc[2 * k] = __builtin_fma(a, xr[k][0], acc[2 * k]);
            acc[2 * k + 1] = __builtin_fma(a, xr[k][1], acc[2 * k + 1]);
        }
    };
    int jd = 0, js = 0;
    for (; jd + U <= Ld && js + U <= Ls; jd += U, js += U) {
        double dv[U]; int dci[U]; float sv[U]; int sci[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            dv[u] = ld_stream<NT>(dvp + (long)(jd + u) * C); dci[u] = ld_stream<NT>(dcp + (long)(jd + u) * C);
            sv[u] = ld_stream<NT>(svp + (long)(js + u) * C); sci[u] = ld_stream<NT>(scp + (long)(js + u) * C);
        }
        vec_t dx[U][NV], sx[U][NV];
#pragma unroll
        for (int u = 0; u < U; ++u) x_row(dci[u], dx[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) x_row(sci[u], sx[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) { fma_row(dv[u], dx[u], dt); fma_row((double)sv[u], sx[u], st); }
    }
    for (; jd + U <= Ld; jd += U) {
        double v[U]; int ci[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { v[u] = ld_stream<NT>(dvp + (long)(jd + u) * C); ci[u] = ld_stream<NT>(dcp + (long)(jd + u) * C); }
        vec_t xr[U][NV];
#pragma unroll
        for (int u = 0; u < U; ++u) x_row(ci[u], xr[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) fma_row(v[u], xr[u], dt);
    }
    for (; jd < Ld; ++jd) {
        const double v = ld_stream<NT>(dvp + (long)jd * C);
        vec_t xr[NV];
        x_row(ld_stream<NT>(dcp + (long)jd * C), xr);
        fma_row(v, xr, dt);
    }
    for (; js + U <= Ls; js += U) {
        float v[U]; int ci[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { v[u] = ld_stream<NT>(svp + (long)(js + u) * C); ci[u] = ld_stream<NT>(scp + (long)(js + u) * C); }
        vec_t xr[U][NV];
#pragma unroll
        for (int u = 0; u < U; ++u) x_row(ci[u], xr[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) fma_row((double)v[u], xr[u], st);
    }
    for (; js < Ls; ++js) {
        const float v = ld_stream<NT>(svp + (long)js * C);
        vec_t xr[NV];
        x_row(ld_stream<NT>(scp + (long)js * C), xr);
        fma_row((double)v, xr, st);
    }
    if (YCOL) {
#pragma unroll
        for (int v = 0; v < B; ++v) st_y<NT>(Y + (row + (long)v * ld), dt[v] + st[v]);
    } else {
        vec_t *yp = (vec_t *)(Y + row * xs);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            vec_t t;
            t[0] = dt[2 * k] + st[2 * k]; t[1] = dt[2 * k + 1] + st[2 * k + 1];
            yp[k] = t;
        }
    }
}

// One part's chain of the staged kernel: values one per lane and slot, the 16-bit local indices four slots per 8-byte load (the streams of
// scs_spmv_ap_tlc: sizeof(VT) + 2 bytes per entry), the X row of a slot B doubles from LDS with 16-byte reads.
// W: slots per batch, 8 or 4 (4 where the kernel makes several passes: the pass loop costs registers, and 128 is all a 1024-thread
// workgroup leaves a lane).
template <int B, bool NT, int W, typename VT>
__device__ __forceinline__ void tlc_block_chain(const VT *__restrict__ vp, const unsigned long long *__restrict__ cq, const int L, const int C,
                                                const double *xs, double (&acc)[B]) {
    typedef double vec_t __attribute__((ext_vector_type(2)));
    auto step = [&](const VT a, const unsigned li) {
        const vec_t *xp = (const vec_t *)(xs + li * B);
#pragma unroll
        for (int k = 0; k < B / 2; ++k) {
            const vec_t xv = xp[k];
            acc[2 * k] = ap_step(a, xv[0], acc[2 * k]);
            acc[2 * k + 1] = ap_step(a, xv[1], acc[2 * k + 1]);
        }
    };
    const int ng = L >> 2;
    int g = 0;
    if constexpr (W >= 8) {
        for (; g + 2 <= ng; g += 2) {
            VT v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ld_stream<NT>(vp + (long)(4 * g + u) * C);
            const unsigned long long qa = ld_stream<NT>(cq + (long)g * C), qb = ld_stream<NT>(cq + (long)(g + 1) * C);
#pragma unroll
            for (int u = 0; u < 4; ++u) step(v[u], (unsigned)(qa >> (16 * u)) & 0xFFFFu);
#pragma unroll
            for (int u = 0; u < 4; ++u) step(v[4 + u], (unsigned)(qb >> (16 * u)) & 0xFFFFu);
        }
    }
    for (; g < ng; ++g) {
        VT v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ld_stream<NT>(vp + (long)(4 * g + u) * C);
        const unsigned long long qa = ld_stream<NT>(cq + (long)g * C);
#pragma unroll
        for (int u = 0; u < 4; ++u) step(v[u], (unsigned)(qa >> (16 * u)) & 0xFFFFu);
    }
    const int rem = L & 3;
    if (rem) {
        const unsigned long long qa = ld_stream<NT>(cq + (long)ng * C);
        for (int u = 0; u < rem; ++u) step(ld_stream<NT>(vp + (long)(4 * ng + u) * C), (unsigned)(qa >> (16 * u)) & 0xFFFFu);
    }
}

// ... and with 32-bit columns and X rows gathered from global memory (tiles without a line list)
template <int B, bool NT, typename VT>
__device__ __forceinline__ void gather_block_chain(const VT *__restrict__ vp, const int *__restrict__ cp, const int L, const int C,
                                                   const double *__restrict__ X, const int xstride, double (&acc)[B]) {
    typedef double vec_t __attribute__((ext_vector_type(2)));
    for (int j = 0; j < L; ++j) {
        const VT a = ld_stream<NT>(vp + (long)j * C);
        const vec_t *xp = (const vec_t *)(X + (long)ld_stream<NT>(cp + (long)j * C) * xstride);
#pragma unroll
        for (int k = 0; k < B / 2; ++k) {
            const vec_t xv = xp[k];
            acc[2 * k] = ap_step(a, xv[0], acc[2 * k]);
            acc[2 * k + 1] = ap_step(a, xv[1], acc[2 * k + 1]);
        }
    }
}

// The pair's shared tile-local-column plan on ROW-MAJOR X of width B, the twin of scs_spmv_ap_tlc: a line of the plan (16 consecutive x
// elements there) is 16 consecutive X rows here.  Per pass BS of the B vectors: the tile's lines are staged once in LDS (lines x 16 rows x
// BS doubles, row-major, 16-byte loads; BS = B: 128 * B contiguous bytes per line), then the dp chain streams 8-byte values + 2-byte
// local indices and the sp chain 4-byte values + 2-byte local indices: 10 and 6 bytes per entry and pass.  B / BS passes: a tile whose
// lines do not fit LDS at the full width still keeps its gathers out of the L2 -> L1 path, at the price of streaming its entries again
// (from the caches: the same workgroup has just read them).  Tiles without a line list gather from global X.  Same chains per (row, v):
// bit-exact.
template <int B, int BS, int CT, bool NT, bool YCOL>
__global__ void __launch_bounds__(1024) scs_spmmv_ap_tlc(const long n_chunks, const int C_rt, const int *__restrict__ dp_cp,
        const int *__restrict__ dp_cl, const int *__restrict__ dp_ci, const double *__restrict__ dp_va, const int *__restrict__ sp_cp,
        const int *__restrict__ sp_cl, const int *__restrict__ sp_ci, const float *__restrict__ sp_va, const double *__restrict__ X,
        double *__restrict__ Y, const long ld, const int *__restrict__ tile_line_ptr, const int *__restrict__ tile_lines,
        const unsigned *__restrict__ dp_c16p, const unsigned short *__restrict__ dp_c16, const unsigned *__restrict__ sp_c16p,
        const unsigned short *__restrict__ sp_c16, const long x_rows, const int xcd_remap) {
    static_assert(BS >= 2 && BS <= B && B % BS == 0 && BS % 2 == 0, "whole 16-byte pieces, whole passes");
    extern __shared__ __attribute__((aligned(16))) unsigned char tlc_smem[];
    double *xs = (double *)tlc_smem;
    typedef double vec_t __attribute__((ext_vector_type(2)));
    constexpr int PPR = BS / 2;               // 16-byte pieces per staged X row
    constexpr int PPL = 16 * PPR;             // ... per line
    constexpr int W = (BS < B && BS >= 4) ? 4 : 8;   // slots per batch of the chains
    const int C = CT > 0 ? CT : C_rt;
    const unsigned tile = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const int lp0 = tile_line_ptr[tile];
    const int nl = tile_line_ptr[tile + 1] - lp0;
    const long row = (long)tile * blockDim.x + threadIdx.x;
    const long c = row / C;
    const int i = (int)(row - c * C);
    const bool valid = c < n_chunks;
    int dcs = 0, Ld = 0, scs_ = 0, Ls = 0;
    unsigned dq0 = 0, sq0 = 0;
    if (valid) { dcs = dp_cp[c]; Ld = dp_cl[c]; scs_ = sp_cp[c]; Ls = sp_cl[c]; dq0 = dp_c16p[c]; sq0 = sp_c16p[c]; }
#pragma unroll 1
    for (int v0 = 0; v0 < B; v0 += BS) {
        double dt[BS], st[BS];
#pragma unroll
        for (int v = 0; v < BS; ++v) { dt[v] = 0.0; st[v] = 0.0; }
        if (nl > 0) {
            if (v0) __syncthreads();              // (the previous pass has read its X rows)
            for (int p = threadIdx.x; p < nl * PPL; p += blockDim.x) {     // piece p of the tile: LDS position = p, two doubles of one X row
                const int k = p / PPL, w = p - k * PPL;
                const long xrow = (long)tile_lines[lp0 + k] * 16 + w / PPR;
                vec_t v;
                v[0] = 0.0; v[1] = 0.0;
                if (xrow < x_rows) v = *(const vec_t *)(X + xrow * B + v0 + 2 * (w % PPR));
                *(vec_t *)(xs + 2 * (long)p) = v;
            }
            __syncthreads();
            if (Ld > 0) tlc_block_chain<BS, NT, W>(dp_va + (long)dcs + i, (const unsigned long long *)(dp_c16 + dq0) + i, Ld, C, xs, dt);
            if (Ls > 0) tlc_block_chain<BS, NT, W>(sp_va + (long)scs_ + i, (const unsigned long long *)(sp_c16 + sq0) + i, Ls, C, xs, st);
        } else {  // wide-footprint tile: 32-bit columns, global gathers
            gather_block_chain<BS, NT>(dp_va + (long)dcs + i, dp_ci + (long)dcs + i, Ld, C, X + v0, B, dt);
            gather_block_chain<BS, NT>(sp_va + (long)scs_ + i, sp_ci + (long)scs_ + i, Ls, C, X + v0, B, st);
        }
        if (valid) {
            if (YCOL) {
#pragma unroll
                for (int v = 0; v < BS; ++v) st_y<NT>(Y + (row + (long)(v0 + v) * ld), dt[v] + st[v]);
            } else {
                vec_t *yp = (vec_t *)(Y + row * B + v0);
#pragma unroll
                for (int k = 0; k < PPR; ++k) {
                    vec_t t;
                    t[0] = dt[2 * k] + st[2 * k]; t[1] = dt[2 * k + 1] + st[2 * k + 1];
                    yp[k] = t;
                }
            }
        }
    }
}

#define AP_PAIR_ARGS(dp, sp)                                                                                                    \
    (long)(dp)->n_chunks, (int)(dp)->C, (dp)->chunk_ptrs, (dp)->chunk_lengths, (dp)->col_idxs, (const double *)(dp)->values,    \
        (sp)->chunk_ptrs, (sp)->chunk_lengths, (sp)->col_idxs, (const float *)(sp)->values

// ids: the chunks to run (n_ids of them), or nullptr for all
template <int VB>
void launch_ap_vb(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, int b, long ld, int layout, hipStream_t st,
                  const int *ids = nullptr, long n_ids = 0) {
    const int block = g_tune.block;
    const long n_chunks = ids ? n_ids : (long)dp->n_chunks;
    const unsigned grid = grid_for(n_chunks * dp->C, block);
    const bool nt = g_tune.nontemporal != 0;
#define APV_LAUNCH(RW, NTV)                                                                                                          \
    do {                                                                                                                             \
        if (ids)                                                                                                                     \
            hipLaunchKernelGGL((scs_spmmv_ap_rows<VB, RW, NTV, true>), dim3(grid), dim3(block), 0, st, n_chunks, (int)dp->C, dp->chunk_ptrs,  \
                               dp->chunk_lengths, dp->col_idxs, (const double *)dp->values, sp->chunk_ptrs, sp->chunk_lengths, sp->col_idxs,  \
                               (const float *)sp->values, X, Y, b, ld, g_tune.xcd_remap, ids);                                      \
        else                                                                                                                         \
            hipLaunchKernelGGL((scs_spmmv_ap_rows<VB, RW, NTV, false>), dim3(grid), dim3(block), 0, st, AP_PAIR_ARGS(dp, sp), X, Y, b, ld,    \
                               g_tune.xcd_remap, (const int *)nullptr);                                                             \
    } while (0)
    if (layout == USPMV_ROWWISE) { if (nt) APV_LAUNCH(true, true); else APV_LAUNCH(true, false); }
    else { if (nt) APV_LAUNCH(false, true); else APV_LAUNCH(false, false); }
#undef APV_LAUNCH
}

// any b through the lane-per-row kernel, VB vectors per pass
void launch_ap_generic(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, int b, long ld, int layout, hipStream_t st,
                       const int *ids = nullptr, long n_ids = 0) {
    if (b <= 2) launch_ap_vb<2>(dp, sp, X, Y, b, ld, layout, st, ids, n_ids);
    else if (b <= 4) launch_ap_vb<4>(dp, sp, X, Y, b, ld, layout, st, ids, n_ids);
    else launch_ap_vb<8>(dp, sp, X, Y, b, ld, layout, st, ids, n_ids);
}

template <int B, int U>
void launch_ap_rowmajor_u(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, long ld, int xs, bool ycol, hipStream_t st) {
    const int block = std::min(g_tune.block, 256);      // (__launch_bounds__(256))
    const unsigned grid = grid_for(dp->n_chunks * dp->C, block);
#define APR_LAUNCH(NTV, YC)                                                                                                         \
    do {                                                                                                                            \
        if (dp->C == 32)                                                                                                            \
            hipLaunchKernelGGL((scs_spmmv_ap_rowmajor<B, U, NTV, YC, 32>), dim3(grid), dim3(block), 0, st, AP_PAIR_ARGS(dp, sp), X, Y, ld, \
                               xs, g_tune.xcd_remap);                                                                                   \
        else                                                                                                                        \
            hipLaunchKernelGGL((scs_spmmv_ap_rowmajor<B, U, NTV, YC, 0>), dim3(grid), dim3(block), 0, st, AP_PAIR_ARGS(dp, sp), X, Y, ld, \
                               xs, g_tune.xcd_remap);                                                                                   \
    } while (0)
    if (g_tune.nontemporal) { if (ycol) APR_LAUNCH(true, true); else APR_LAUNCH(true, false); }
    else { if (ycol) APR_LAUNCH(false, true); else APR_LAUNCH(false, false); }
#undef APR_LAUNCH
}

// slots per batch: "spmmv_unroll", 0 = 256 bytes of X rows per lane and fused trip (both chains together); at most 512 bytes.
// B = 16 runs as two launches over eight vectors each (rows 128 bytes apart): 2 x 16 accumulators and whole 128-byte rows per slot leave a
// lane three waves per SIMD and one slot per batch, and measured 7.6 ms against 6.5 ms for the two launches on the 74^3 x 5 dof pair.
template <int B>
void launch_ap_rowmajor(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, long ld, bool ycol, hipStream_t st) {
    if constexpr (B == 16) {
        for (int v0 = 0; v0 < 16; v0 += 8) launch_ap_rowmajor_u<8, 2>(dp, sp, X + v0, ycol ? Y + (long)v0 * ld : Y + v0, ld, 16, ycol, st);
    } else {
        constexpr int UMAX = B >= 8 ? 4 : 8;
        constexpr int UDEF = B >= 8 ? 2 : B >= 4 ? 4 : 8;
        const int U = std::min(g_tune.spmmv_unroll ? g_tune.spmmv_unroll : UDEF, UMAX);
        if constexpr (UMAX >= 8) { if (U >= 8) { launch_ap_rowmajor_u<B, 8>(dp, sp, X, Y, ld, B, ycol, st); return; } }
        if (U >= 4) launch_ap_rowmajor_u<B, 4>(dp, sp, X, Y, ld, B, ycol, st);
        else if (U >= 2) launch_ap_rowmajor_u<B, 2>(dp, sp, X, Y, ld, B, ycol, st);
        else launch_ap_rowmajor_u<B, 1>(dp, sp, X, Y, ld, B, ycol, st);
    }
}

constexpr size_t AP_TLC_LDS = 160 * 1024;   // LDS budget of the staged kernel: all a gfx950 workgroup can have

// the staged kernel applies: both handles carry one shared line plan whose fullest tile fits the LDS budget with at least two vectors
bool ap_tlc_applies(const uspmv_dmat *dp, const uspmv_dmat *sp) {
    return g_tune.tlc && dp->tlc.on && sp->tlc.on && !dp->tlc.elem && dp->tlc.plan_id != 0 && dp->tlc.plan_id == sp->tlc.plan_id &&
           dp->tlc.max_lines >= 1 && (size_t)dp->tlc.max_lines * 128 * 2 <= AP_TLC_LDS;
}

template <int B, int BS>
void launch_ap_tlc_bs(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, long ld, bool ycol, hipStream_t st) {
    const size_t lds = (size_t)dp->tlc.max_lines * 128 * BS;     // (what the fullest tile lists, not the budget)
    const int C = (int)dp->C;
#define APT_LAUNCH(CTV, NTV, YC)                                                                                                    \
    do {                                                                                                                            \
        auto kfn = scs_spmmv_ap_tlc<B, BS, CTV, NTV, YC>;                                                                           \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);    \
        hipLaunchKernelGGL(kfn, dim3((unsigned)dp->tlc.n_tiles), dim3(dp->tlc.tile_rows), lds, st, AP_PAIR_ARGS(dp, sp), X, Y, ld,  \
                           dp->tlc.line_ptr.get(), dp->tlc.lines.get(), dp->tlc.c16_ptrs.get(), dp->tlc.col16.get(),                \
                           sp->tlc.c16_ptrs.get(), sp->tlc.col16.get(), (long)dp->tlc.x_len, g_tune.xcd_remap);                     \
    } while (0)
#define APT_NT(CTV, NTV) do { if (ycol) APT_LAUNCH(CTV, NTV, true); else APT_LAUNCH(CTV, NTV, false); } while (0)
    if (g_tune.nontemporal) { if (C == 32) APT_NT(32, true); else APT_NT(0, true); }
    else { if (C == 32) APT_NT(32, false); else APT_NT(0, false); }
#undef APT_NT
#undef APT_LAUNCH
}

// as many of the B vectors per pass as the plan's fullest tile leaves room for in LDS (at most 8: 2 * 8 accumulators per lane)
int ap_tlc_bs(const uspmv_dmat *dp, int b) {
    const size_t line_bytes = (size_t)dp->tlc.max_lines * 128;
    if (b >= 8 && line_bytes * 8 <= AP_TLC_LDS) return 8;
    if (b >= 4 && line_bytes * 4 <= AP_TLC_LDS) return 4;
    return 2;
}

template <int B>
void launch_ap_tlc(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, long ld, bool ycol, hipStream_t st) {
    const int bs = ap_tlc_bs(dp, B);
    if constexpr (B >= 8) { if (bs == 8) { launch_ap_tlc_bs<B, 8>(dp, sp, X, Y, ld, ycol, st); return; } }
    if constexpr (B >= 4) { if (bs == 4) { launch_ap_tlc_bs<B, 4>(dp, sp, X, Y, ld, ycol, st); return; } }
    launch_ap_tlc_bs<B, 2>(dp, sp, X, Y, ld, ycol, st);
}

// What uspmv_spmmv_ap runs for b >= 2: the ONE predicate behind the launch and behind uspmv_spmmv_ap_path.
// bs: vectors per pass of the sweep kernel (path 3) or of the staged kernel (path 2), else 0.
enum { AP_PATH_GENERIC = 0, AP_PATH_GATHER = 1, AP_PATH_STAGED = 2, AP_PATH_SWEEP = 3 };
struct ApBlockPath { int path, bs; };

ApBlockPath ap_block_path(const uspmv_dmat *dp, const uspmv_dmat *sp, int b, long ld, int layout, bool aligned16) {
    const uspmv_dmat *W = (dp->alt && g_tune.rechunk) ? dp->alt : dp;      // (the workspace of the pair: where uspmv_spmmv_x_prepared(dp, ...) put it)
    const bool col = layout != USPMV_ROWWISE;
    if (g_tune.spmmv_variant == 1 || !aligned16 || (b != 2 && b != 4 && b != 8 && b != 16)) return {AP_PATH_GENERIC, 0};
    // the pair's column-window sweep plan, under the conditions of launch_spmv_ap plus the block ones: the float second part, column-major
    // pieces of 16 bytes, no part of a distributed two-part step, and at least two vectors of a window in LDS
    if (g_tune.sweep && dp->sw.on && sp->sw.on && dp->sw.tile_ids && dp->sw.n_parts == 2 && dp->sw.plan_id == sp->sw.plan_id &&
        dp->sw.part[1].dtype == USPMV_F32 && !(col && (ld & 1)) && !dp->part && !sp->part && !W->part) {
        const int bs = spmmv_ap_sweep_bs(dp, b);
        // row-major X in more than two passes keeps the gather kernel: a pass stages bs * 8 bytes out of every b * 8-byte X row, so the rows'
        // sectors are read b / bs times (banded-random 500 k x 140 pair: 1.17 / 2.23 / 3.89 ms against 0.89 / 2.05 / 2.05 ms)
        if (bs >= 2 && (col || b / bs <= 2)) return {AP_PATH_SWEEP, bs};
    }
    if (col && W->part) return {AP_PATH_GENERIC, 0};         // (a handle inside a two-part distributed step: no whole re-layout)
    if (ap_tlc_applies(dp, sp)) return {AP_PATH_STAGED, ap_tlc_bs(dp, b)};
    return {AP_PATH_GATHER, 0};
}

// the staged kernel over the shared plan or the gather kernel on the original arrays, as ap_block_path chose
template <int B>
void launch_ap_block(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, long ld, bool ycol, bool staged, hipStream_t st) {
    if (staged) launch_ap_tlc<B>(dp, sp, X, Y, ld, ycol, st);
    else launch_ap_rowmajor<B>(dp, sp, X, Y, ld, ycol, st);
}

// B-specialised path.  Column-major callers: X re-laid out into the dp handle's workspace (per call, or once by
// uspmv_spmmv_x_prepared(dp, ...)), Y written column-major by the kernel.  W: the handle that owns the workspace.
template <int B>
int spmmv_ap_fast(const uspmv_dmat *dp, const uspmv_dmat *sp, const uspmv_dmat *W, const double *X, double *Y, long ld, int layout,
                  bool staged, hipStream_t st) {
    if (layout == USPMV_ROWWISE) {
        launch_ap_block<B>(dp, sp, X, Y, ld, false, staged, st);
        return USPMV_OK;
    }
    const bool prepared = W->xprep_ptr == (const void *)X && W->xprep_b == B && W->xprep_ld == ld && W->xprep_form == 1 && W->ws;
    if (!prepared) {
        W->xprep_ptr = nullptr;                               // (the workspace is about to hold another X)
        if (int rc = relayout_x_plain(W, X, B, ld, st)) return rc;
    }
    launch_ap_block<B>(dp, sp, (const double *)W->ws, Y, ld, true, staged, st);
    return USPMV_OK;
}

}  // namespace

namespace uspmv_dev {

// the staged kernel takes a shared plan at every B-specialised width as long as two vectors of the fullest tile's X rows fit LDS
int spmmv_ap_plan_lines(int b) { return (b == 2 || b == 4 || b == 8 || b == 16) ? (int)(AP_TLC_LDS / (128 * 2)) : 0; }

void spmmv_ap_path(const uspmv_dmat *dp, const uspmv_dmat *sp, int b, long ld, int layout, int *path, int *vectors) {
    const ApBlockPath p = ap_block_path(dp, sp, b, ld, layout, true);
    *path = p.path; *vectors = p.bs;
}

int launch_spmmv_ap_chunks(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *chunk_ids, long n_ids, const double *X, double *Y, int b,
                           long ld, int layout, hipStream_t st) {
    if (n_ids == 0) return USPMV_OK;
    launch_ap_generic(dp, sp, X, Y, b, ld, layout, st, chunk_ids, n_ids);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_spmmv_ap(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, int b, long ld, int layout, hipStream_t st) {
    if (dp->n_chunks == 0) return USPMV_OK;
    if (b == 1) return launch_spmv_ap(dp, sp, X, nullptr, Y, st);
    const uspmv_dmat *W = (dp->alt && g_tune.rechunk) ? dp->alt : dp;
    const ApBlockPath p = ap_block_path(dp, sp, b, ld, layout, ((uintptr_t)X % 16 == 0) && ((uintptr_t)Y % 16 == 0));
    if (p.path == AP_PATH_SWEEP) return launch_spmmv_ap_sweep(dp, sp, X, Y, b, ld, layout != USPMV_ROWWISE, p.bs, st);
    if (p.path == AP_PATH_GENERIC) {  // generic width / layout / alignment
        launch_ap_generic(dp, sp, X, Y, b, ld, layout, st);
    } else {
        const bool staged = p.path == AP_PATH_STAGED;
        int rc = USPMV_OK;
        switch (b) {
            case 2: rc = spmmv_ap_fast<2>(dp, sp, W, X, Y, ld, layout, staged, st); break;
            case 4: rc = spmmv_ap_fast<4>(dp, sp, W, X, Y, ld, layout, staged, st); break;
            case 8: rc = spmmv_ap_fast<8>(dp, sp, W, X, Y, ld, layout, staged, st); break;
            default: rc = spmmv_ap_fast<16>(dp, sp, W, X, Y, ld, layout, staged, st); break;
        }
        if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // namespace uspmv_dev
