// Adaptive-precision dp+sp SpMV kernels: reference twins scs_ap_impl_cpu<C> (code/ap_kernels.hpp:24-82) and
// spmv_omp_scs_ap (:562-634).  See uspmv_device.hpp / DESIGN.md 5.
#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace {

// Adaptive precision dp+sp over a tile-local-column plan shared by the two structs (one line list
// per tile covering the columns of both): x lines staged once, then the dp chain (8-byte values +
// 2-byte local indices) and the sp chain (4-byte values + 2-byte local indices), y = dp + sp.
// 10 and 6 bytes per non-zero instead of 12 and 8; numerics of scs_ap_impl_cpu, bit-exact.
// IDS: workgroup b runs tile tile_ids[b] (the interior / boundary lists of the distributed step); an entry < 0 is a conditional entry
// that was switched off (uspmv_dist's padding re-run) and returns before the barrier, uniformly for the workgroup.
// ELEM: the shared plan lists single x ELEMENTS (TlcPlan::elem): thread k gathers element k of the tile's list into xs[k], as scs_spmv_tlc's
// ELEM arm does -- one 8-byte gather per distinct column of the tile; the chains over xs are the same code, same slot order, same bits.
// EP (here and in the kernels below, always the LAST template parameter, off by default): EP = 1 is uspmv_spmv_ap[_hp]_axpby's path 1 --
// the one store site, where the parts' accumulators are combined, stores axpby_row's value and the kernel ends in axpby_reduce, which
// every thread must reach: lanes without a row add zero terms.  With EP = 0 `ep` is never read and every branch on EP folds away.
template <int CT, bool NT, bool IDS = false, bool ELEM = false, int EP = 0>
__global__ void __launch_bounds__(1024) scs_spmv_ap_tlc(const long n_chunks, const int C_rt,
        const int *__restrict__ dp_cp, const int *__restrict__ dp_cl, const int *__restrict__ dp_ci, const double *__restrict__ dp_va,
        const int *__restrict__ sp_cp, const int *__restrict__ sp_cl, const int *__restrict__ sp_ci, const float *__restrict__ sp_va,
        const double *__restrict__ x, double *__restrict__ y, const int *__restrict__ tile_line_ptr,
        const int *__restrict__ tile_lines, const unsigned *__restrict__ dp_c16p, const unsigned short *__restrict__ dp_c16,
        const unsigned *__restrict__ sp_c16p, const unsigned short *__restrict__ sp_c16, const long x_len, const int xcd_remap,
        const int *__restrict__ tile_ids, const AxpbyArgs<double> ep) {
    static_assert(EP == 0 || !IDS, "fused epilogue: the launch over all tiles only (no early return ahead of the reduction)");
    extern __shared__ __attribute__((aligned(16))) unsigned char tlc_smem[];
    double *xs = (double *)tlc_smem;
    typedef double vec_t __attribute__((ext_vector_type(2)));
    const int C = CT > 0 ? CT : C_rt;
    const unsigned lbt = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const unsigned tile = IDS ? (unsigned)tile_ids[lbt] : lbt;
    if (IDS && (int)tile < 0) return;
    const int lp0 = tile_line_ptr[tile];
    const int nl = tile_line_ptr[tile + 1] - lp0;
    const long row = (long)tile * blockDim.x + threadIdx.x;
    const long c = row / C;
    const int i = (int)(row - c * C);
    const bool valid = c < n_chunks;
    int dcs = 0, Ld = 0, scs_ = 0, Ls = 0;
    unsigned dq0 = 0, sq0 = 0;
    if (valid) { dcs = dp_cp[c]; Ld = dp_cl[c]; scs_ = sp_cp[c]; Ls = sp_cl[c]; dq0 = dp_c16p[c]; sq0 = sp_c16p[c]; }
    double dt = 0.0, st = 0.0;
    if (nl > 0) {
        if constexpr (ELEM) {
            for (int k = threadIdx.x; k < nl; k += blockDim.x) {
                const long idx = tile_lines[lp0 + k];
                xs[k] = idx < x_len ? x[idx] : 0.0;
            }
        } else {
            const int sub = threadIdx.x & 7, lk = threadIdx.x >> 3;
            for (int k = lk; k < nl; k += blockDim.x >> 3) {
                const long idx = (long)tile_lines[lp0 + k] * 16 + sub * 2;
                vec_t v;
                if (idx + 2 <= x_len) v = *(const vec_t *)(x + idx);
                else { v[0] = idx < x_len ? x[idx] : 0.0; v[1] = 0.0; }
                *(vec_t *)(xs + k * 16 + sub * 2) = v;
            }
        }
        __syncthreads();
        if (Ld > 0) {
            const double *vp = dp_va + (long)dcs + i;
            const unsigned long long *cq = (const unsigned long long *)(dp_c16 + dq0) + i;
            const int ng = Ld >> 2;
            int g = 0;
            for (; g + 2 <= ng; g += 2) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = ld_stream<NT>(vp + (long)(4 * g + u) * C);
                const unsigned long long qa = ld_stream<NT>(cq + (long)g * C), qb = ld_stream<NT>(cq + (long)(g + 1) * C);
#pragma unroll
                for (int u = 0; u < 4; ++u) dt = __builtin_fma(v[u], xs[(qa >> (16 * u)) & 0xFFFFu], dt);
#pragma unroll
                for (int u = 0; u < 4; ++u) dt = __builtin_fma(v[4 + u], xs[(qb >> (16 * u)) & 0xFFFFu], dt);
            }
            for (; g < ng; ++g) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = ld_stream<NT>(vp + (long)(4 * g + u) * C);
                const unsigned long long qa = ld_stream<NT>(cq + (long)g * C);
#pragma unroll
                for (int u = 0; u < 4; ++u) dt = __builtin_fma(v[u], xs[(qa >> (16 * u)) & 0xFFFFu], dt);
            }
            const int rem = Ld & 3;
            if (rem) {
                const unsigned long long qa = ld_stream<NT>(cq + (long)ng * C);
                for (int u = 0; u < rem; ++u) dt = __builtin_fma(ld_stream<NT>(vp + (long)(4 * ng + u) * C), xs[(qa >> (16 * u)) & 0xFFFFu], dt);
            }
        }
        if (Ls > 0) {
            const float *vp = sp_va + (long)scs_ + i;
            const unsigned long long *cq = (const unsigned long long *)(sp_c16 + sq0) + i;
            const int ng = Ls >> 2;
            int g = 0;
            for (; g + 2 <= ng; g += 2) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = ld_stream<NT>(vp + (long)(4 * g + u) * C);
                const unsigned long long qa = ld_stream<NT>(cq + (long)g * C), qb = ld_stream<NT>(cq + (long)(g + 1) * C);
#pragma unroll
                for (int u = 0; u < 4; ++u) st = __builtin_fma((double)v[u], xs[(qa >> (16 * u)) & 0xFFFFu], st);
#pragma unroll
                for (int u = 0; u < 4; ++u) st = __builtin_fma((double)v[4 + u], xs[(qb >> (16 * u)) & 0xFFFFu], st);
            }
            for (; g < ng; ++g) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = ld_stream<NT>(vp + (long)(4 * g + u) * C);
                const unsigned long long qa = ld_stream<NT>(cq + (long)g * C);
#pragma unroll
                for (int u = 0; u < 4; ++u) st = __builtin_fma((double)v[u], xs[(qa >> (16 * u)) & 0xFFFFu], st);
            }
            const int rem = Ls & 3;
            if (rem) {
                const unsigned long long qa = ld_stream<NT>(cq + (long)ng * C);
                for (int u = 0; u < rem; ++u) st = __builtin_fma((double)ld_stream<NT>(vp + (long)(4 * ng + u) * C), xs[(qa >> (16 * u)) & 0xFFFFu], st);
            }
        }
    } else {  // wide-footprint tile: 32-bit columns, global gathers
        const double *dvp = dp_va + (long)dcs + i;
        const int *dcp = dp_ci + (long)dcs + i;
        for (int j = 0; j < Ld; ++j) dt = __builtin_fma(ld_stream<NT>(dvp + (long)j * C), x[ld_stream<NT>(dcp + (long)j * C)], dt);
        const float *svp = sp_va + (long)scs_ + i;
        const int *scp = sp_ci + (long)scs_ + i;
        for (int j = 0; j < Ls; ++j) st = __builtin_fma((double)ld_stream<NT>(svp + (long)j * C), x[ld_stream<NT>(scp + (long)j * C)], st);
    }
    if constexpr (EP == 0) {
        if (valid) st_y<NT>(y + row, dt + st);
    } else {
        double d0 = 0.0, d1 = 0.0;
        if (valid) st_y<NT>(y + row, axpby_row(ep, row, dt + st, d0, d1));
        axpby_reduce(ep, lbt, d0, d1, (double *)tlc_smem);   // (the x window is dead: the front of it)
    }
}

// Adaptive precision dp+sp, one lane per row: the dp chain, then the sp chain (float value widened,
// times the DOUBLE x, accumulated in double), y = dp + sp  (code/ap_kernels.hpp:59-75).
// SPX: the generic-C reference kernel spmv_omp_scs_ap multiplies the sp values with the FLOAT copy
// of x (float product, rounded, then widened and added; code/ap_kernels.hpp:619-623).
// EP = 1: the early exits become "own no row, add zero terms" (a barrier cannot sit behind a return); AXPBY_RED_BYTES of dynamic LDS.
template <int U, bool NT, bool SPX, int CT, bool IDS = false, int EP = 0>
__global__ void scs_spmv_ap_rows(const long n_chunks, const int C_rt, const int *__restrict__ dp_cp,
                                 const int *__restrict__ dp_cl, const int *__restrict__ dp_ci,
                                 const double *__restrict__ dp_va, const int *__restrict__ sp_cp,
                                 const int *__restrict__ sp_cl, const int *__restrict__ sp_ci,
                                 const float *__restrict__ sp_va, const double *__restrict__ x,
                                 const float *__restrict__ x_sp, double *__restrict__ y, const int xcd_remap,
                                 const int *__restrict__ chunk_ids, const AxpbyArgs<double> ep) {
    static_assert(EP == 0 || !SPX, "fused epilogue: not for the generic-C reference variant");
    const int C = CT > 0 ? CT : C_rt;        // CT = 32: slot strides become immediate offsets
    const unsigned lb = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const long vrow = (long)lb * blockDim.x + threadIdx.x;
    const long vc = vrow / C;                // IDS: virtual chunk vc -> chunk_ids[vc] (the chunks a sweep plan leaves over)
    const int i = (int)(vrow - vc * C);
    if constexpr (EP == 0) { if (vc >= n_chunks) return; }
    const long c = (EP != 0 && vc >= n_chunks) ? -1 : IDS ? (long)chunk_ids[vc] : vc;
    if constexpr (EP == 0) { if (IDS && c < 0) return; }   // (an entry that was switched off, as in the tile lists)
    const bool live = EP == 0 || c >= 0;
    const long row = c * C + i;
    double dt = 0.0, st = 0.0;
    const long dcs = live ? dp_cp[c] : 0, scs_ = live ? sp_cp[c] : 0;
    const int Ld = live ? dp_cl[c] : 0, Ls = live ? sp_cl[c] : 0;
    const double *dvp = dp_va + dcs + i;
    const int *dcp = dp_ci + dcs + i;
    const float *svp = sp_va + scs_ + i;
    const int *scp = sp_ci + scs_ + i;
    int jd = 0, js = 0;
    // fused part: one dp batch and one sp batch per trip -- the two accumulators are independent
    // chains, so their streams and gathers are issued together (twice the bytes in flight per
    // wave); each chain still runs in slot order, i.e. bit-identical to dp-then-sp.
    for (; jd + U <= Ld && js + U <= Ls; jd += U, js += U) {
        double dv[U]; int dci[U]; float sv[U]; int sci[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            dv[u] = ld_stream<NT>(dvp + (long)(jd + u) * C); dci[u] = ld_stream<NT>(dcp + (long)(jd + u) * C);
            sv[u] = ld_stream<NT>(svp + (long)(js + u) * C); sci[u] = ld_stream<NT>(scp + (long)(js + u) * C);
        }
        double dx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dx[u] = x[dci[u]];
        if constexpr (SPX) {
            float sx[U];
#pragma unroll
            for (int u = 0; u < U; ++u) sx[u] = x_sp[sci[u]];
#pragma unroll
            for (int u = 0; u < U; ++u) { dt = __builtin_fma(dv[u], dx[u], dt); st = st + (double)__fmul_rn(sv[u], sx[u]); }
        } else {
            double sx[U];
#pragma unroll
            for (int u = 0; u < U; ++u) sx[u] = x[sci[u]];
#pragma unroll
            for (int u = 0; u < U; ++u) { dt = __builtin_fma(dv[u], dx[u], dt); st = __builtin_fma((double)sv[u], sx[u], st); }
        }
    }
    for (; jd + U <= Ld; jd += U) {
        double v[U]; int ci[U]; double xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { v[u] = ld_stream<NT>(dvp + (long)(jd + u) * C); ci[u] = ld_stream<NT>(dcp + (long)(jd + u) * C); }
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = x[ci[u]];
#pragma unroll
        for (int u = 0; u < U; ++u) dt = __builtin_fma(v[u], xv[u], dt);
    }
    for (; jd < Ld; ++jd) dt = __builtin_fma(ld_stream<NT>(dvp + (long)jd * C), x[ld_stream<NT>(dcp + (long)jd * C)], dt);
    for (; js + U <= Ls; js += U) {
        float v[U]; int ci[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { v[u] = ld_stream<NT>(svp + (long)(js + u) * C); ci[u] = ld_stream<NT>(scp + (long)(js + u) * C); }
        if constexpr (SPX) {
            float xs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) xs[u] = x_sp[ci[u]];
#pragma unroll
            for (int u = 0; u < U; ++u) st = st + (double)__fmul_rn(v[u], xs[u]);
        } else {
            double xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) xv[u] = x[ci[u]];
#pragma unroll
            for (int u = 0; u < U; ++u) st = __builtin_fma((double)v[u], xv[u], st);
        }
    }
    for (; js < Ls; ++js) {
        const float v = ld_stream<NT>(svp + (long)js * C);
        const int ci = ld_stream<NT>(scp + (long)js * C);
        if constexpr (SPX) st = st + (double)__fmul_rn(v, x_sp[ci]);
        else st = __builtin_fma((double)v, x[ci], st);
    }
    if constexpr (EP == 0) {
        st_y<NT>(y + row, dt + st);
    } else {
        extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];   // (AXPBY_RED_BYTES, fused launches only)
        double d0 = 0.0, d1 = 0.0;
        if (live) st_y<NT>(y + row, axpby_row(ep, row, dt + st, d0, d1));
        axpby_reduce(ep, lb, d0, d1, (double *)rows_smem);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Adaptive precision with an fp16 part: ap[dp_hp] (HT double, no mid), ap[dp_sp_hp] (HT double, mid float), ap[sp_hp] (HT float, x and
// y float).  One chain per part, each in slot order; with a double x every product is an FMA in double on the exactly widened value
// (scs_ap_impl_cpu's convention, hp in the place of sp), with a float x the product is rounded to float and then added to the part's
// double accumulator (the sp part of spmv_omp_scs_ap).  y = hi + hp, (hi + mid) + hp, or (float)(sp + hp).  The steps (ap_step,
// ap_hp_y) are shared with the column-window sweep form (sweep_ap_hp_kernels.hip) and live in uspmv_device.hpp.

// one part's chain over the staged x lines: values one per lane per slot, the 16-bit local indices four slots per 8-byte load
template <bool NT, typename VT, typename XT>
__device__ __forceinline__ double tlc_chain(const VT *__restrict__ vp, const unsigned long long *__restrict__ cq, const int L, const int C,
                                            const XT *xs, double acc) {
    const int ng = L >> 2;
    int g = 0;
    for (; g + 2 <= ng; g += 2) {
        VT v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ld_stream<NT>(vp + (long)(4 * g + u) * C);
        const unsigned long long qa = ld_stream<NT>(cq + (long)g * C), qb = ld_stream<NT>(cq + (long)(g + 1) * C);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = ap_step(v[u], xs[(qa >> (16 * u)) & 0xFFFFu], acc);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = ap_step(v[4 + u], xs[(qb >> (16 * u)) & 0xFFFFu], acc);
    }
    for (; g < ng; ++g) {
        VT v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ld_stream<NT>(vp + (long)(4 * g + u) * C);
        const unsigned long long qa = ld_stream<NT>(cq + (long)g * C);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = ap_step(v[u], xs[(qa >> (16 * u)) & 0xFFFFu], acc);
    }
    const int rem = L & 3;
    if (rem) {
        const unsigned long long qa = ld_stream<NT>(cq + (long)ng * C);
        for (int u = 0; u < rem; ++u) acc = ap_step(ld_stream<NT>(vp + (long)(4 * ng + u) * C), xs[(qa >> (16 * u)) & 0xFFFFu], acc);
    }
    return acc;
}

// one part's chain with 32-bit columns and global gathers of x, U slots per batch
template <bool NT, int U, typename VT, typename XT>
__device__ __forceinline__ double gather_chain(const VT *__restrict__ vp, const int *__restrict__ cp, const int L, const int C,
                                               const XT *__restrict__ x, double acc) {
    int j = 0;
    for (; j + U <= L; j += U) {
        VT v[U]; int ci[U]; XT xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { v[u] = ld_stream<NT>(vp + (long)(j + u) * C); ci[u] = ld_stream<NT>(cp + (long)(j + u) * C); }
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = x[ci[u]];
#pragma unroll
        for (int u = 0; u < U; ++u) acc = ap_step(v[u], xv[u], acc);
    }
    for (; j < L; ++j) acc = ap_step(ld_stream<NT>(vp + (long)j * C), x[ld_stream<NT>(cp + (long)j * C)], acc);
    return acc;
}

// Tile-local-column form: the tile's x lines (the union over all parts) staged once in LDS, then the parts' chains one after the other,
// each streaming sizeof(VT) + 2 bytes per non-zero.  Tiles without a line list (footprint over the plan's line budget) gather from x.
// IDS: workgroup b runs tile tile_ids[b] (the interior / boundary lists of the distributed step), an entry < 0 returns before the barrier,
// uniformly for the workgroup -- as in scs_spmv_ap_tlc.  ELEM: the list holds single x elements, staged one per thread (as there).
template <int CT, bool NT, typename HT, bool MID, bool IDS = false, bool ELEM = false, int EP = 0>
__global__ void __launch_bounds__(1024) scs_spmv_ap_hp_tlc(const long n_chunks, const int C_rt, const ApHpParts P, const HT *__restrict__ x,
                                                           HT *__restrict__ y, const int *__restrict__ tile_line_ptr,
                                                           const int *__restrict__ tile_lines, const long x_len, const int xcd_remap,
                                                           const int *__restrict__ tile_ids, const AxpbyArgs<HT> ep) {
    static_assert(EP == 0 || !IDS, "fused epilogue: the launch over all tiles only (no early return ahead of the reduction)");
    extern __shared__ __attribute__((aligned(16))) unsigned char tlc_smem[];
    HT *xs = (HT *)tlc_smem;
    typedef HT vec_t __attribute__((ext_vector_type(2)));
    const int C = CT > 0 ? CT : C_rt;
    const unsigned lbt = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const unsigned tile = IDS ? (unsigned)tile_ids[lbt] : lbt;
    if (IDS && (int)tile < 0) return;
    const int lp0 = tile_line_ptr[tile];
    const int nl = tile_line_ptr[tile + 1] - lp0;
    const long row = (long)tile * blockDim.x + threadIdx.x;
    const long c = row / C;
    const int i = (int)(row - c * C);
    const bool valid = c < n_chunks;
    int cs[3] = {0, 0, 0}, L[3] = {0, 0, 0};
    unsigned q0[3] = {0, 0, 0};
    if (valid)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k != 1 || MID) { cs[k] = P.cp[k][c]; L[k] = P.cl[k][c]; q0[k] = P.c16p[k][c]; }
    double acc[3] = {0.0, 0.0, 0.0};
    if (nl > 0) {
        if constexpr (ELEM) {
            for (int k = threadIdx.x; k < nl; k += blockDim.x) {
                const long idx = tile_lines[lp0 + k];
                xs[k] = idx < x_len ? x[idx] : (HT)0;
            }
        } else {
            const int sub = threadIdx.x & 7, lk = threadIdx.x >> 3;
            for (int k = lk; k < nl; k += blockDim.x >> 3) {
                const long idx = (long)tile_lines[lp0 + k] * 16 + sub * 2;
                vec_t v;
                if (idx + 2 <= x_len) v = *(const vec_t *)(x + idx);
                else { v[0] = idx < x_len ? x[idx] : (HT)0; v[1] = (HT)0; }
                *(vec_t *)(xs + k * 16 + sub * 2) = v;
            }
        }
        __syncthreads();
        if (L[0] > 0)
            acc[0] = tlc_chain<NT>((const HT *)P.va[0] + (long)cs[0] + i, (const unsigned long long *)(P.c16[0] + q0[0]) + i, L[0], C, xs, 0.0);
        if constexpr (MID)
            if (L[1] > 0)
                acc[1] = tlc_chain<NT>((const float *)P.va[1] + (long)cs[1] + i, (const unsigned long long *)(P.c16[1] + q0[1]) + i, L[1], C, xs, 0.0);
        if (L[2] > 0)
            acc[2] = tlc_chain<NT>((const unsigned short *)P.va[2] + (long)cs[2] + i, (const unsigned long long *)(P.c16[2] + q0[2]) + i, L[2], C,
                                   xs, 0.0);
    } else {  // wide-footprint tile: 32-bit columns, global gathers
        acc[0] = gather_chain<NT, 1>((const HT *)P.va[0] + (long)cs[0] + i, P.ci[0] + (long)cs[0] + i, L[0], C, x, 0.0);
        if constexpr (MID) acc[1] = gather_chain<NT, 1>((const float *)P.va[1] + (long)cs[1] + i, P.ci[1] + (long)cs[1] + i, L[1], C, x, 0.0);
        acc[2] = gather_chain<NT, 1>((const unsigned short *)P.va[2] + (long)cs[2] + i, P.ci[2] + (long)cs[2] + i, L[2], C, x, 0.0);
    }
    if constexpr (EP == 0) {
        if (valid) st_y<NT>(y + row, ap_hp_y<HT, MID>(acc[0], acc[1], acc[2]));
    } else {
        double d0 = 0.0, d1 = 0.0;
        if (valid) st_y<NT>(y + row, axpby_row(ep, row, ap_hp_y<HT, MID>(acc[0], acc[1], acc[2]), d0, d1));
        axpby_reduce(ep, lbt, d0, d1, (double *)tlc_smem);   // (the x window is dead: the front of it)
    }
}

// Lane per row, any C and handles without a plan: the parts' chains one after the other with global gathers.  IDS: virtual chunk vc ->
// chunk_ids[vc] (the chunks a sweep plan leaves over; the chunk lists of the distributed step, where an entry < 0 is switched off)
template <int U, bool NT, int CT, typename HT, bool MID, bool IDS = false, int EP = 0>
__global__ void scs_spmv_ap_hp_rows(const long n_chunks, const int C_rt, const ApHpParts P, const HT *__restrict__ x, HT *__restrict__ y,
                                    const int xcd_remap, const int *__restrict__ chunk_ids, const AxpbyArgs<HT> ep) {
    const int C = CT > 0 ? CT : C_rt;
    const unsigned lb = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const long vrow = (long)lb * blockDim.x + threadIdx.x;
    const long vc = vrow / C;
    const int i = (int)(vrow - vc * C);
    if constexpr (EP == 0) { if (vc >= n_chunks) return; }
    const long c = (EP != 0 && vc >= n_chunks) ? -1 : IDS ? (long)chunk_ids[vc] : vc;
    if constexpr (EP == 0) { if (IDS && c < 0) return; }
    const bool live = EP == 0 || c >= 0;     // (EP: a lane without a row runs chains of length 0)
    const long row = c * C + i;
    double acc[3] = {0.0, 0.0, 0.0};
    long cs = live ? P.cp[0][c] : 0;
    acc[0] = gather_chain<NT, U>((const HT *)P.va[0] + cs + i, P.ci[0] + cs + i, live ? P.cl[0][c] : 0, C, x, 0.0);
    if constexpr (MID) {
        cs = live ? P.cp[1][c] : 0;
        acc[1] = gather_chain<NT, U>((const float *)P.va[1] + cs + i, P.ci[1] + cs + i, live ? P.cl[1][c] : 0, C, x, 0.0);
    }
    cs = live ? P.cp[2][c] : 0;
    acc[2] = gather_chain<NT, U>((const unsigned short *)P.va[2] + cs + i, P.ci[2] + cs + i, live ? P.cl[2][c] : 0, C, x, 0.0);
    if constexpr (EP == 0) {
        st_y<NT>(y + row, ap_hp_y<HT, MID>(acc[0], acc[1], acc[2]));
    } else {
        extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];   // (AXPBY_RED_BYTES, fused launches only)
        double d0 = 0.0, d1 = 0.0;
        if (live) st_y<NT>(y + row, axpby_row(ep, row, ap_hp_y<HT, MID>(acc[0], acc[1], acc[2]), d0, d1));
        axpby_reduce(ep, lb, d0, d1, (double *)rows_smem);
    }
}

// the chunks in chunk_ids through the lane-per-row kernel
template <typename HT, bool MID>
int launch_ap_hp_chunks(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *chunk_ids, long n_ids, const HT *d_x,
                        HT *d_y, hipStream_t stream, const AxpbyArgs<HT> *ep = nullptr) {
    const ApHpParts P = ap_hp_parts(hi, mid, hp);
    const unsigned grid = grid_for(n_ids * hi->C, 256);
    if (ep)   // (non-temporal stream only: spmv_ap_hp_axpby_route)
        hipLaunchKernelGGL((scs_spmv_ap_hp_rows<4, true, 0, HT, MID, true, 1>), dim3(grid), dim3(256), AXPBY_RED_BYTES, stream, n_ids, (int)hi->C, P,
                           d_x, d_y, g_tune.xcd_remap, chunk_ids, *ep);
    else if (g_tune.nontemporal)
        hipLaunchKernelGGL((scs_spmv_ap_hp_rows<4, true, 0, HT, MID, true>), dim3(grid), dim3(256), 0, stream, n_ids, (int)hi->C, P, d_x, d_y,
                           g_tune.xcd_remap, chunk_ids, AxpbyArgs<HT>{});
    else
        hipLaunchKernelGGL((scs_spmv_ap_hp_rows<4, false, 0, HT, MID, true>), dim3(grid), dim3(256), 0, stream, n_ids, (int)hi->C, P, d_x, d_y,
                           g_tune.xcd_remap, chunk_ids, AxpbyArgs<HT>{});
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

// the tiles in tile_ids through the tile-local-column kernel of the shared line plan
template <typename HT, bool MID>
int launch_ap_hp_tiles(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *tile_ids, long n_ids, const HT *d_x,
                       HT *d_y, hipStream_t stream) {
    const ApHpParts P = ap_hp_parts(hi, mid, hp);
    const bool elem = hi->tlc.elem;                               // (max_lines then counts elements)
    const size_t lds = (size_t)hi->tlc.max_lines * (elem ? 1 : 16) * sizeof(HT);
    const int C = (int)hi->C;
#define APHP_IDS(CTV, NTV)                                                                                                        \
    do {                                                                                                                         \
        auto kfn = elem ? scs_spmv_ap_hp_tlc<CTV, NTV, HT, MID, true, true> : scs_spmv_ap_hp_tlc<CTV, NTV, HT, MID, true>;       \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);  \
        hipLaunchKernelGGL(kfn, dim3((unsigned)n_ids), dim3(hi->tlc.tile_rows), lds, stream, (long)hi->n_chunks, C, P, d_x, d_y,  \
                           hi->tlc.line_ptr.get(), hi->tlc.lines.get(), (long)hi->tlc.x_len, g_tune.xcd_remap, tile_ids, AxpbyArgs<HT>{}); \
    } while (0)
    if (g_tune.nontemporal) { if (C == 32) APHP_IDS(32, true); else APHP_IDS(0, true); }
    else { if (C == 32) APHP_IDS(32, false); else APHP_IDS(0, false); }
#undef APHP_IDS
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

template <typename HT, bool MID>
int launch_ap_hp(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const HT *d_x, HT *d_y, hipStream_t stream,
                 const AxpbyArgs<HT> *ep = nullptr) {
    const int path = spmv_ap_hp_path(hi, mid, hp, (uintptr_t)d_x % 16 == 0);
    if (ep && !g_tune.nontemporal) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "launch_ap_hp: no fused instantiation under this tuning");
    if (path == 3) {
        if (int rc = launch_spmv_sweep_ap_hp(hi, MID, d_x, d_y, stream, ep)) return rc;
        if (hi->sw.n_rest == 0) return USPMV_OK;
        if (!ep) return launch_ap_hp_chunks<HT, MID>(hi, mid, hp, hi->sw.rest, (long)hi->sw.n_rest, d_x, d_y, stream);
        AxpbyArgs<HT> rest = *ep;                 // the second launch of the call owns the slots behind the sweep tiles'
        rest.slot0 += (unsigned)hi->sw.n_tiles;
        return launch_ap_hp_chunks<HT, MID>(hi, mid, hp, hi->sw.rest, (long)hi->sw.n_rest, d_x, d_y, stream, &rest);
    }
    const ApHpParts P = ap_hp_parts(hi, mid, hp);
    const bool nt = g_tune.nontemporal != 0;
    const int C = (int)hi->C;
    if (path == 2) {
        const bool elem = hi->tlc.elem;
        const size_t lds = (size_t)hi->tlc.max_lines * (elem ? 1 : 16) * sizeof(HT);
#define APHP_TLC(CTV, NTV)                                                                                                       \
    do {                                                                                                                         \
        auto kfn = elem ? scs_spmv_ap_hp_tlc<CTV, NTV, HT, MID, false, true> : scs_spmv_ap_hp_tlc<CTV, NTV, HT, MID>;            \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);  \
        hipLaunchKernelGGL(kfn, dim3((unsigned)hi->tlc.n_tiles), dim3(hi->tlc.tile_rows), lds, stream, (long)hi->n_chunks, C, P,  \
                           d_x, d_y, hi->tlc.line_ptr.get(), hi->tlc.lines.get(), (long)hi->tlc.x_len, g_tune.xcd_remap,         \
                           (const int *)nullptr, AxpbyArgs<HT>{});                                                               \
    } while (0)
        // the same choice among the fused instantiations (non-temporal stream); the reduction needs the front of the window
#define APHP_TLC_EP(CTV)                                                                                                         \
    do {                                                                                                                         \
        auto kfn = elem ? scs_spmv_ap_hp_tlc<CTV, true, HT, MID, false, true, 1> : scs_spmv_ap_hp_tlc<CTV, true, HT, MID, false, false, 1>; \
        const size_t lds_ep = std::max(lds, (size_t)AXPBY_RED_BYTES);                                                            \
        if (lds_ep > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ep); \
        hipLaunchKernelGGL(kfn, dim3((unsigned)hi->tlc.n_tiles), dim3(hi->tlc.tile_rows), lds_ep, stream, (long)hi->n_chunks, C, P, \
                           d_x, d_y, hi->tlc.line_ptr.get(), hi->tlc.lines.get(), (long)hi->tlc.x_len, g_tune.xcd_remap,         \
                           (const int *)nullptr, *ep);                                                                           \
    } while (0)
        if (ep) { if (C == 32) APHP_TLC_EP(32); else APHP_TLC_EP(0); }
        else if (nt) { if (C == 32) APHP_TLC(32, true); else APHP_TLC(0, true); }
        else { if (C == 32) APHP_TLC(32, false); else APHP_TLC(0, false); }
#undef APHP_TLC_EP
#undef APHP_TLC
    } else {
        const int block = g_tune.block;
        const unsigned grid = grid_for(hi->n_chunks * hi->C, block);
#define APHP_ROWS(CTV, NTV) hipLaunchKernelGGL((scs_spmv_ap_hp_rows<4, NTV, CTV, HT, MID>), dim3(grid), dim3(block), 0, stream, \
                                               (long)hi->n_chunks, C, P, d_x, d_y, g_tune.xcd_remap, (const int *)nullptr, AxpbyArgs<HT>{})
#define APHP_ROWS_EP(CTV) hipLaunchKernelGGL((scs_spmv_ap_hp_rows<4, true, CTV, HT, MID, false, 1>), dim3(grid), dim3(block), AXPBY_RED_BYTES, stream, \
                                             (long)hi->n_chunks, C, P, d_x, d_y, g_tune.xcd_remap, (const int *)nullptr, *ep)
        if (ep) { if (C == 32) APHP_ROWS_EP(32); else APHP_ROWS_EP(0); }
        else if (nt) { if (C == 32) APHP_ROWS(32, true); else APHP_ROWS(0, true); }
        else { if (C == 32) APHP_ROWS(32, false); else APHP_ROWS(0, false); }
#undef APHP_ROWS_EP
#undef APHP_ROWS
    }
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // namespace

namespace uspmv_dev {

int spmv_ap_hp_path(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, bool x_aligned16) {
    // a column-window sweep plan shared by all parts first (its arrays live on hi), then the shared line plan, then lane per row
    const uint64_t sid = hi->sw.plan_id;
    if (hi->sw.on && hi->sw.tile_ids && hi->sw.n_parts == (mid ? 3 : 2) && hp->sw.on && hp->sw.plan_id == sid &&
        (!mid || (mid->sw.on && mid->sw.plan_id == sid)) && g_tune.sweep && x_aligned16)
        return 3;
    const uint64_t id = hi->tlc.plan_id;
    const bool planned = hi->tlc.on && id != 0 && hp->tlc.on && hp->tlc.plan_id == id && (!mid || (mid->tlc.on && mid->tlc.plan_id == id));
    return planned && g_tune.tlc && x_aligned16 ? 2 : 0;
}

// the sweep launch of an ap split under the current tuning has a fused instantiation (the tuning sweep_axpby_fused names, the pairing
// at its default for every number of rows per lane)
static bool sweep_ap_axpby_fused() { return g_tune.nontemporal && g_tune.sweep_unroll >= 8 && g_tune.sweep_pair == 2; }

int spmv_ap_hp_axpby_route(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, bool x16, long *slots) {
    long n = 0;
    int path = 2;
    const int kernel = spmv_ap_hp_path(hi, mid, hp, x16);
    if (hi->n_chunks == 0) {
        path = 1;                                                       // (nothing is launched)
    } else if (kernel == 3) {
        if (sweep_ap_axpby_fused()) { path = 1; n = (long)hi->sw.n_tiles + (hi->sw.n_rest ? (long)grid_for((long)hi->sw.n_rest * hi->C, 256) : 0); }
    } else if (kernel == 2) {
        if (g_tune.nontemporal) { path = 1; n = (long)hi->tlc.n_tiles; }
    } else if (g_tune.nontemporal) {                                    // (lane per row: U is fixed at 4, "unroll" is not consulted)
        path = 1; n = grid_for((long)hi->n_chunks * hi->C, g_tune.block);
    }
    if (path == 2) n = axpby_pass_slots((long)hi->n_chunks * hi->C);
    if (slots) *slots = n;
    return path;
}

int spmv_ap_axpby_route(const uspmv_dmat *dp, const uspmv_dmat *sp, bool x16, long *slots) {
    long n = 0;
    int path = 2;
    if (dp->n_chunks == 0) {
        path = 1;                                                       // (nothing is launched)
    } else if (dp->sw.on && sp->sw.on && dp->sw.tile_ids && dp->sw.n_parts >= 2 && dp->sw.plan_id == sp->sw.plan_id && g_tune.sweep && x16) {
        if (sweep_ap_axpby_fused()) { path = 1; n = (long)dp->sw.n_tiles + (dp->sw.n_rest ? (long)grid_for((long)dp->sw.n_rest * dp->C, 256) : 0); }
    } else if (dp->tlc.on && sp->tlc.on && dp->tlc.plan_id != 0 && dp->tlc.plan_id == sp->tlc.plan_id && g_tune.tlc && x16) {
        if (g_tune.nontemporal) { path = 1; n = (long)dp->tlc.n_tiles; }
    } else if (g_tune.nontemporal && g_tune.unroll >= 8) {
        path = 1; n = grid_for((long)dp->n_chunks * dp->C, g_tune.block);
    }
    if (path == 2) n = axpby_pass_slots((long)dp->n_chunks * dp->C);
    if (slots) *slots = n;
    return path;
}

int launch_spmv_ap_hp(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const void *d_x, void *d_y, hipStream_t stream,
                      const void *ep) {
    if (hi->dtype == USPMV_F32) return launch_ap_hp<float, false>(hi, nullptr, hp, (const float *)d_x, (float *)d_y, stream, (const AxpbyArgs<float> *)ep);
    if (mid) return launch_ap_hp<double, true>(hi, mid, hp, (const double *)d_x, (double *)d_y, stream, (const AxpbyArgs<double> *)ep);
    return launch_ap_hp<double, false>(hi, nullptr, hp, (const double *)d_x, (double *)d_y, stream, (const AxpbyArgs<double> *)ep);
}

int launch_spmv_ap_hp_chunks(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *chunk_ids, long n_ids,
                             const void *d_x, void *d_y, hipStream_t stream) {
    if (n_ids == 0) return USPMV_OK;
    if (hi->dtype == USPMV_F32) return launch_ap_hp_chunks<float, false>(hi, nullptr, hp, chunk_ids, n_ids, (const float *)d_x, (float *)d_y, stream);
    if (mid) return launch_ap_hp_chunks<double, true>(hi, mid, hp, chunk_ids, n_ids, (const double *)d_x, (double *)d_y, stream);
    return launch_ap_hp_chunks<double, false>(hi, nullptr, hp, chunk_ids, n_ids, (const double *)d_x, (double *)d_y, stream);
}

int launch_spmv_ap_hp_tiles(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *tile_ids, long n_ids,
                            const void *d_x, void *d_y, hipStream_t stream) {
    if (n_ids == 0) return USPMV_OK;
    if (hi->dtype == USPMV_F32) return launch_ap_hp_tiles<float, false>(hi, nullptr, hp, tile_ids, n_ids, (const float *)d_x, (float *)d_y, stream);
    if (mid) return launch_ap_hp_tiles<double, true>(hi, mid, hp, tile_ids, n_ids, (const double *)d_x, (double *)d_y, stream);
    return launch_ap_hp_tiles<double, false>(hi, nullptr, hp, tile_ids, n_ids, (const double *)d_x, (double *)d_y, stream);
}

int launch_spmv_ap_chunks(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *chunk_ids, long n_ids, const double *d_x,
                          double *d_y, hipStream_t stream, const AxpbyArgs<double> *ep) {
    if (n_ids == 0) return USPMV_OK;
    const unsigned grid = grid_for(n_ids * dp->C, 256);
    if (ep)   // (non-temporal stream only: spmv_ap_axpby_route)
        hipLaunchKernelGGL((scs_spmv_ap_rows<4, true, false, 0, true, 1>), dim3(grid), dim3(256), AXPBY_RED_BYTES, stream, n_ids, (int)dp->C,
                           dp->chunk_ptrs, dp->chunk_lengths, dp->col_idxs, (const double *)dp->values, sp->chunk_ptrs, sp->chunk_lengths,
                           sp->col_idxs, (const float *)sp->values, d_x, (const float *)nullptr, d_y, g_tune.xcd_remap, chunk_ids, *ep);
    else if (g_tune.nontemporal)
        hipLaunchKernelGGL((scs_spmv_ap_rows<4, true, false, 0, true>), dim3(grid), dim3(256), 0, stream, n_ids, (int)dp->C, dp->chunk_ptrs,
                           dp->chunk_lengths, dp->col_idxs, (const double *)dp->values, sp->chunk_ptrs, sp->chunk_lengths, sp->col_idxs,
                           (const float *)sp->values, d_x, (const float *)nullptr, d_y, g_tune.xcd_remap, chunk_ids, AxpbyArgs<double>{});
    else
        hipLaunchKernelGGL((scs_spmv_ap_rows<4, false, false, 0, true>), dim3(grid), dim3(256), 0, stream, n_ids, (int)dp->C, dp->chunk_ptrs,
                           dp->chunk_lengths, dp->col_idxs, (const double *)dp->values, sp->chunk_ptrs, sp->chunk_lengths, sp->col_idxs,
                           (const float *)sp->values, d_x, (const float *)nullptr, d_y, g_tune.xcd_remap, chunk_ids, AxpbyArgs<double>{});
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_spmv_ap_tiles(const uspmv_dmat *dp, const uspmv_dmat *sp, const int *tile_ids, long n_ids, const double *d_x, double *d_y,
                         hipStream_t stream) {
    if (n_ids == 0) return USPMV_OK;
    const bool elem = dp->tlc.elem;                               // (max_lines then counts elements)
    const size_t lds = (size_t)dp->tlc.max_lines * (elem ? 1 : 16) * sizeof(double);
    const int C = (int)dp->C;
#define APT_IDS_LAUNCH(CTV, NTV)                                                                                      \
    do {                                                                                                              \
        auto kfn = elem ? scs_spmv_ap_tlc<CTV, NTV, true, true> : scs_spmv_ap_tlc<CTV, NTV, true>;                   \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL(kfn, dim3((unsigned)n_ids), dim3(dp->tlc.tile_rows), lds, stream, (long)dp->n_chunks, C,   \
                           dp->chunk_ptrs, dp->chunk_lengths, dp->col_idxs, (const double *)dp->values, sp->chunk_ptrs, \
                           sp->chunk_lengths, sp->col_idxs, (const float *)sp->values, d_x, d_y, dp->tlc.line_ptr,     \
                           dp->tlc.lines, dp->tlc.c16_ptrs, dp->tlc.col16, sp->tlc.c16_ptrs, sp->tlc.col16,            \
                           (long)dp->tlc.x_len, g_tune.xcd_remap, tile_ids, AxpbyArgs<double>{});                     \
    } while (0)
    if (g_tune.nontemporal) { if (C == 32) APT_IDS_LAUNCH(32, true); else APT_IDS_LAUNCH(0, true); }
    else { if (C == 32) APT_IDS_LAUNCH(32, false); else APT_IDS_LAUNCH(0, false); }
#undef APT_IDS_LAUNCH
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_spmv_ap(const uspmv_dmat *dp, const uspmv_dmat *sp, const double *d_x, const float *d_x_sp, double *d_y,
                   hipStream_t stream, const AxpbyArgs<double> *ep) {
    if (ep && (d_x_sp || !g_tune.nontemporal)) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "launch_spmv_ap: no fused instantiation for this launch");
    if (!d_x_sp && dp->sw.on && sp->sw.on && dp->sw.tile_ids && dp->sw.n_parts >= 2 && dp->sw.plan_id == sp->sw.plan_id && g_tune.sweep &&
        ((uintptr_t)d_x % 16 == 0)) {
        if (int rc = launch_spmv_sweep_ap(dp, d_x, d_y, stream, ep)) return rc;
        if (!ep) return launch_spmv_ap_chunks(dp, sp, dp->sw.rest, (long)dp->sw.n_rest, d_x, d_y, stream);
        AxpbyArgs<double> rest = *ep;             // the second launch of the call owns the slots behind the sweep tiles'
        rest.slot0 += (unsigned)dp->sw.n_tiles;
        return launch_spmv_ap_chunks(dp, sp, dp->sw.rest, (long)dp->sw.n_rest, d_x, d_y, stream, &rest);
    }
    if (!d_x_sp && dp->tlc.on && sp->tlc.on && dp->tlc.plan_id != 0 && dp->tlc.plan_id == sp->tlc.plan_id && g_tune.tlc &&
        ((uintptr_t)d_x % 16 == 0)) {
        const bool elem = dp->tlc.elem;
        const size_t lds = (size_t)dp->tlc.max_lines * (elem ? 1 : 16) * sizeof(double);
        const int C = (int)dp->C;
#define APT_LAUNCH(CTV, NTV)                                                                                          \
    do {                                                                                                              \
        auto kfn = elem ? scs_spmv_ap_tlc<CTV, NTV, false, true> : scs_spmv_ap_tlc<CTV, NTV>;                        \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL(kfn, dim3((unsigned)dp->tlc.n_tiles), dim3(dp->tlc.tile_rows), lds, (hipStream_t)stream,     \
                           (long)dp->n_chunks, C, dp->chunk_ptrs, dp->chunk_lengths, dp->col_idxs, (const double *)dp->values, \
                           sp->chunk_ptrs, sp->chunk_lengths, sp->col_idxs, (const float *)sp->values, d_x, d_y,         \
                           dp->tlc.line_ptr, dp->tlc.lines, dp->tlc.c16_ptrs, dp->tlc.col16, sp->tlc.c16_ptrs,           \
                           sp->tlc.col16, (long)dp->tlc.x_len, g_tune.xcd_remap, (const int *)nullptr, AxpbyArgs<double>{}); \
    } while (0)
        // the same choice among the fused instantiations (non-temporal stream); the reduction needs the front of the window
#define APT_LAUNCH_EP(CTV)                                                                                            \
    do {                                                                                                              \
        auto kfn = elem ? scs_spmv_ap_tlc<CTV, true, false, true, 1> : scs_spmv_ap_tlc<CTV, true, false, false, 1>;   \
        const size_t lds_ep = std::max(lds, (size_t)AXPBY_RED_BYTES);                                                 \
        if (lds_ep > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ep); \
        hipLaunchKernelGGL(kfn, dim3((unsigned)dp->tlc.n_tiles), dim3(dp->tlc.tile_rows), lds_ep, (hipStream_t)stream, \
                           (long)dp->n_chunks, C, dp->chunk_ptrs, dp->chunk_lengths, dp->col_idxs, (const double *)dp->values, \
                           sp->chunk_ptrs, sp->chunk_lengths, sp->col_idxs, (const float *)sp->values, d_x, d_y,         \
                           dp->tlc.line_ptr, dp->tlc.lines, dp->tlc.c16_ptrs, dp->tlc.col16, sp->tlc.c16_ptrs,           \
                           sp->tlc.col16, (long)dp->tlc.x_len, g_tune.xcd_remap, (const int *)nullptr, *ep);             \
    } while (0)
        if (ep) { if (C == 32) APT_LAUNCH_EP(32); else APT_LAUNCH_EP(0); }
        else if (g_tune.nontemporal) { if (C == 32) APT_LAUNCH(32, true); else APT_LAUNCH(0, true); }
        else { if (C == 32) APT_LAUNCH(32, false); else APT_LAUNCH(0, false); }
#undef APT_LAUNCH_EP
#undef APT_LAUNCH
        HIP_TRY(hipGetLastError());
        return USPMV_OK;
    }
    const int block = g_tune.block;
    const unsigned grid = grid_for(dp->n_chunks * dp->C, block);
#define AP_LAUNCH_UC(UU, NTV, SPXV, CTV)                                                                             \
    hipLaunchKernelGGL((scs_spmv_ap_rows<UU, NTV, SPXV, CTV>), dim3(grid), dim3(block), 0, (hipStream_t)stream,      \
                       (long)dp->n_chunks, (int)dp->C, dp->chunk_ptrs, dp->chunk_lengths, dp->col_idxs,              \
                       (const double *)dp->values, sp->chunk_ptrs, sp->chunk_lengths, sp->col_idxs,                  \
                       (const float *)sp->values, d_x, d_x_sp, d_y, g_tune.xcd_remap, (const int *)nullptr, AxpbyArgs<double>{})
    if (ep) {   // (the default tuning only: unroll 8, non-temporal stream -- spmv_ap_axpby_route)
        if (g_tune.unroll < 8) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "launch_spmv_ap: no fused instantiation under this tuning");
#define AP_LAUNCH_EP(CTV)                                                                                            \
    hipLaunchKernelGGL((scs_spmv_ap_rows<8, true, false, CTV, false, 1>), dim3(grid), dim3(block), AXPBY_RED_BYTES, (hipStream_t)stream, \
                       (long)dp->n_chunks, (int)dp->C, dp->chunk_ptrs, dp->chunk_lengths, dp->col_idxs,              \
                       (const double *)dp->values, sp->chunk_ptrs, sp->chunk_lengths, sp->col_idxs,                  \
                       (const float *)sp->values, d_x, (const float *)nullptr, d_y, g_tune.xcd_remap, (const int *)nullptr, *ep)
        if (dp->C == 32) AP_LAUNCH_EP(32); else AP_LAUNCH_EP(0);
#undef AP_LAUNCH_EP
        HIP_TRY(hipGetLastError());
        return USPMV_OK;
    }
#define AP_LAUNCH_U(UU, NTV, SPXV) do { if (dp->C == 32) AP_LAUNCH_UC(UU, NTV, SPXV, 32); else AP_LAUNCH_UC(UU, NTV, SPXV, 0); } while (0)
#define AP_LAUNCH(NTV, SPXV)                                                                                         \
    do { if (g_tune.unroll >= 8) AP_LAUNCH_U(8, NTV, SPXV); else if (g_tune.unroll == 4) AP_LAUNCH_U(4, NTV, SPXV);  \
         else AP_LAUNCH_U(2, NTV, SPXV); } while (0)
    if (d_x_sp) { if (g_tune.nontemporal) AP_LAUNCH(true, true); else AP_LAUNCH(false, true); }
    else { if (g_tune.nontemporal) AP_LAUNCH(true, false); else AP_LAUNCH(false, false); }
#undef AP_LAUNCH_U
#undef AP_LAUNCH_UC
#undef AP_LAUNCH
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // namespace uspmv_dev
