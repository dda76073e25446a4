// Adaptive-precision dp+sp SpMMV (block vectors): uspmv_spmmv_ap.  The reference has no twin (its CLI stops at "SpMMV is not yet
// implemented for AP kernels", code/utilities.hpp:1389); the numerics are scs_ap_impl_cpu<C> (code/ap_kernels.hpp:24-82) applied to every
// column of X: per (row, v) a dp FMA chain and an sp FMA chain (float value widened, times the DOUBLE x), each in slot order,
// Y(r, v) = dp + sp.  One lane per row everywhere, so column v of Y is bitwise uspmv_spmv_ap of column v of X.  See DESIGN.md 5.7.
// The pair is the kind <double, no mid, float last part> of the lane-per-row and staged block kernels in ap_hp_spmmv_kernels.hip
// (launch_spmmv_ap_rows, launch_spmmv_ap_staged); what lives here is its own: the path predicate, the row-major gather kernel, and the
// column-major re-layout through the dp handle's workspace, and the dispatch of the list forms (uspmv_spmmv_ap_tiles / _chunks: the parts
// of the distributed block step).
#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace {

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

#define AP_PAIR_ARGS(dp, sp)                                                                                                    \
    (long)(dp)->n_chunks, (int)(dp)->C, (dp)->chunk_ptrs, (dp)->chunk_lengths, (dp)->col_idxs, (const double *)(dp)->values,    \
        (sp)->chunk_ptrs, (sp)->chunk_lengths, (sp)->col_idxs, (const float *)(sp)->values

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

// the staged kernel applies: both handles carry one shared line plan whose fullest tile fits the LDS budget with at least two vectors
bool ap_tlc_applies(const uspmv_dmat *dp, const uspmv_dmat *sp) {
    return g_tune.tlc && dp->tlc.on && sp->tlc.on && !dp->tlc.elem && dp->tlc.plan_id != 0 && dp->tlc.plan_id == sp->tlc.plan_id &&
           dp->tlc.max_lines >= 1 && (size_t)dp->tlc.max_lines * 128 * 2 <= WG_LDS_BYTES;
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
    if (ap_tlc_applies(dp, sp)) return {AP_PATH_STAGED, tlc_block_bs(dp->tlc, b, sizeof(double))};
    return {AP_PATH_GATHER, 0};
}

// What uspmv_spmmv_ap_tiles runs: the ONE predicate behind the launch and behind uspmv_spmmv_ap_tiles_path.  The staged kernel over the
// listed tiles -- X staged straight from the caller's layout, so column-major X wants whole 16-byte pieces of its columns (ld even) --
// or lane per row over the tiles' rows: any other width, alignment or leading dimension, "tlc" 0, "spmmv_variant" 1, or a plan whose
// fullest tile leaves no room for two vectors in LDS.
ApBlockPath ap_tiles_path(const uspmv_dmat *dp, const uspmv_dmat *sp, int b, long ld, int layout, bool aligned16) {
    if (g_tune.spmmv_variant == 1 || !aligned16 || (b != 2 && b != 4 && b != 8 && b != 16)) return {AP_PATH_GENERIC, 0};
    if (layout != USPMV_ROWWISE && (ld & 1)) return {AP_PATH_GENERIC, 0};
    if (!ap_tlc_applies(dp, sp)) return {AP_PATH_GENERIC, 0};
    const int bs = tlc_block_bs(dp->tlc, b, sizeof(double));
    if (bs < 2) return {AP_PATH_GENERIC, 0};
    return {AP_PATH_STAGED, bs};
}

// the staged kernel over the shared plan (bs vectors per pass) or the gather kernel on the original arrays (bs 0), as ap_block_path
// chose; X row-major
template <int B>
int launch_ap_block(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, long ld, bool ycol, int bs, hipStream_t st) {
    if (bs) return launch_spmmv_ap_staged(dp, nullptr, sp, X, Y, B, ld, ycol, bs, st);
    launch_ap_rowmajor<B>(dp, sp, X, Y, ld, ycol, st);
    return USPMV_OK;
}

// B-specialised path.  Column-major callers: X re-laid out into the dp handle's workspace (per call, or once by
// uspmv_spmmv_x_prepared(dp, ...)), Y written column-major by the kernel.  W: the handle that owns the workspace.
template <int B>
int spmmv_ap_fast(const uspmv_dmat *dp, const uspmv_dmat *sp, const uspmv_dmat *W, const double *X, double *Y, long ld, int layout,
                  int bs, hipStream_t st) {
    if (layout == USPMV_ROWWISE) return launch_ap_block<B>(dp, sp, X, Y, ld, false, bs, st);
    const bool prepared = W->xprep_ptr == (const void *)X && W->xprep_b == B && W->xprep_ld == ld && W->xprep_form == 1 && W->ws;
    if (!prepared) {
        W->xprep_ptr = nullptr;                               // (the workspace is about to hold another X)
        if (int rc = relayout_x_plain(W, X, B, ld, st)) return rc;
    }
    return launch_ap_block<B>(dp, sp, (const double *)W->ws, Y, ld, true, bs, st);
}

}  // namespace

namespace uspmv_dev {

// the staged kernel takes a shared plan at every B-specialised width as long as two vectors of the fullest tile's X rows fit LDS
int spmmv_ap_plan_lines(int b) { return (b == 2 || b == 4 || b == 8 || b == 16) ? (int)(WG_LDS_BYTES / (128 * 2)) : 0; }

void spmmv_ap_path(const uspmv_dmat *dp, const uspmv_dmat *sp, int b, long ld, int layout, int *path, int *vectors) {
    const ApBlockPath p = ap_block_path(dp, sp, b, ld, layout, true);
    *path = p.path; *vectors = p.bs;
}

int launch_spmmv_ap_chunks(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *chunk_ids, long n_ids, const double *X, double *Y, int b,
                           long ld, int layout, hipStream_t st) {
    if (n_ids == 0) return USPMV_OK;
    return launch_spmmv_ap_rows(dp, nullptr, sp, chunk_ids, n_ids, X, Y, b, ld, layout, st);
}

void spmmv_ap_tiles_path(const uspmv_dmat *dp, const uspmv_dmat *sp, int b, long ld, int layout, int *path, int *vectors) {
    const ApBlockPath p = ap_tiles_path(dp, sp, b, ld, layout, true);
    *path = p.path; *vectors = p.bs;
}

int launch_spmmv_ap_tiles(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *tile_ids, long n_ids, const double *X, double *Y, int b,
                          long ld, int layout, hipStream_t st) {
    if (n_ids == 0) return USPMV_OK;
    const ApBlockPath p = ap_tiles_path(dp, sp, b, ld, layout, ((uintptr_t)X % 16 == 0) && ((uintptr_t)Y % 16 == 0));
    if (p.path == AP_PATH_STAGED) return launch_spmmv_ap_staged(dp, nullptr, sp, X, Y, b, ld, layout != USPMV_ROWWISE, p.bs, st, tile_ids, n_ids);
    return launch_spmmv_ap_rows(dp, nullptr, sp, tile_ids, n_ids, X, Y, b, ld, layout, st, dp->tlc.tile_rows);
}

int launch_spmmv_ap(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *X, double *Y, int b, long ld, int layout, hipStream_t st) {
    if (dp->n_chunks == 0) return USPMV_OK;
    if (b == 1) return launch_spmv_ap(dp, sp, X, nullptr, Y, st);
    const uspmv_dmat *W = (dp->alt && g_tune.rechunk) ? dp->alt : dp;
    const ApBlockPath p = ap_block_path(dp, sp, b, ld, layout, ((uintptr_t)X % 16 == 0) && ((uintptr_t)Y % 16 == 0));
    if (p.path == AP_PATH_SWEEP) return launch_spmmv_ap_sweep(dp, sp, X, Y, b, ld, layout != USPMV_ROWWISE, p.bs, st);
    if (p.path == AP_PATH_GENERIC) return launch_spmmv_ap_rows(dp, nullptr, sp, nullptr, 0, X, Y, b, ld, layout, st);   // generic width / layout / alignment
    int rc = USPMV_OK;
    switch (b) {
        case 2: rc = spmmv_ap_fast<2>(dp, sp, W, X, Y, ld, layout, p.bs, st); break;
        case 4: rc = spmmv_ap_fast<4>(dp, sp, W, X, Y, ld, layout, p.bs, st); break;
        case 8: rc = spmmv_ap_fast<8>(dp, sp, W, X, Y, ld, layout, p.bs, st); break;
        default: rc = spmmv_ap_fast<16>(dp, sp, W, X, Y, ld, layout, p.bs, st); break;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // namespace uspmv_dev
