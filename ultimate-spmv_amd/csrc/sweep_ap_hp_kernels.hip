// Column-window sweep SpMV for adaptive precision with an fp16 part: ap[dp_hp], ap[sp_hp], ap[dp_sp_hp] (plan: host/sweep_plan.cpp with
// two or three structs; the dp / sp / ap[dp_sp] forms and the description of the sweep itself are in sweep_kernels.hip).
//
// One workgroup = one tile; the windows of x are staged by LDS-DMA ONCE per tile, and per window every part runs its own compacted
// stream: sizeof(value) + 2 bytes per non-zero -- 10 / 6 / 4 for a dp / sp / hp entry -- plus one count byte per (row, window, part).
// Numerics are those of the other ap_hp kernels (ap_step / ap_hp_y, uspmv_device.hpp): one chain per part in slot order, a double x
// with one FMA in double per entry on the exactly widened value, a float x (ap[sp_hp]) with the product rounded to float and added
// to the part's double accumulator; y = hi + hp, (hi + mid) + hp or (float)(sp + hp).  A lane that sits a round out leaves its
// accumulator alone: the step's result is selected, or the update runs under the round's lane mask (masked_fma_batch for a double x,
// masked_add_batch on the finished terms for a float x).
//
// Registers: a 1024-thread workgroup leaves 128 VGPRs per lane, and the ap[dp_sp] pair form sits at 115 with two chains side by side.
// Three do not fit, so "sweep_pair" 1 | 2 runs TWO parts side by side and the third one alone: the mid and the hp part of
// ap[dp_sp_hp] (a split by magnitude puts most entries there), the two parts of the other kinds.  "sweep_pair" 0: one part after the
// other.  The streams are addressed as base pointer (wave-uniform kernel argument) + 32-bit element offset per (row of the lane, part):
// one scalar register each, where the pair kernel's pointers take four.
#include <cstddef>
#include "uspmv_device.hpp"
#include "sweep_common.hpp"

using namespace uspmv_dev;

namespace {

// One window, one part of one row per lane: batches of U rounds over the wave's compacted stream, which starts at element o of vals /
// idx; returns where the next window's starts.  In round u the active lanes are those with more than k0+u entries in this window -- one
// ballot --, a lane's element sits `active lanes below it` behind the round's first one.  Loads run under the lane mask, the step's
// result is selected.
template <typename AT, typename XT, int U, bool NT>
__device__ __forceinline__ unsigned hp_window(const XT *__restrict__ xs, const int c, const AT *__restrict__ vals,
                                              const unsigned short *__restrict__ idx, unsigned o, double &acc) {
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
            const double t = ap_step(v[u], xs[ix[u]], acc);
            acc = (k0 + u < c) ? t : acc;
        }
        o += first[U];
    }
    return o;
}

// Two parts of a row side by side through the same window: both parts' ballots, then BOTH batches of loads before the first wait (see
// sweep_window2 in sweep_kernels.hip for why).  Each chain still sees its entries in slot order.  MF: the updates under the rounds'
// lane masks (EXEC) instead of step + select.
struct HpOffs { unsigned o0, o1; };

template <typename AT, typename XT, int U>
__device__ __forceinline__ void hp_masked_batch(const XT *__restrict__ xs, const AT (&v)[U], const unsigned (&ix)[U],
                                                const unsigned long long (&m)[U], double &acc) {
    if constexpr (sizeof(XT) == 8) {
        double w[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { w[u] = hp_widen(v[u], XT(0)); xv[u] = xs[ix[u]]; }
        masked_fma_batch<U>(acc, w, xv, m);
    } else {
        double t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = (double)__fmul_rn(hp_widen(v[u], XT(0)), xs[ix[u]]);
        masked_add_batch<U>(acc, t, m);
    }
}

template <typename A0, typename A1, typename XT, int U, bool NT, bool MF>
__device__ __forceinline__ HpOffs hp_window2(const XT *__restrict__ xs, const int c0, const int c1, const A0 *__restrict__ vals0,
                                             const unsigned short *__restrict__ idx0, const A1 *__restrict__ vals1,
                                             const unsigned short *__restrict__ idx1, HpOffs o, double &acc0, double &acc1) {
    A0 v0[U];
    A1 v1[U];
    unsigned ix0[U], ix1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { v0[u] = A0(0); v1[u] = A1(0); ix0[u] = 0u; ix1[u] = 0u; }
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
                const unsigned off = o.o0 + f0[u] + lanes_below(m0[u]);
                v0[u] = ld_stream_g<NT>(vals0 + off); ix0[u] = ld_stream_g<NT>(idx0 + off);
            }
            if (k0 + u < c1) {
                const unsigned off = o.o1 + f1[u] + lanes_below(m1[u]);
                v1[u] = ld_stream_g<NT>(vals1 + off); ix1[u] = ld_stream_g<NT>(idx1 + off);
            }
        }
        if constexpr (MF) {
            hp_masked_batch<A0, XT, U>(xs, v0, ix0, m0, acc0);
            hp_masked_batch<A1, XT, U>(xs, v1, ix1, m1, acc1);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double t0 = ap_step(v0[u], xs[ix0[u]], acc0);
                acc0 = (k0 + u < c0) ? t0 : acc0;
                const double t1 = ap_step(v1[u], xs[ix1[u]], acc1);
                acc1 = (k0 + u < c1) ? t1 : acc1;
            }
        }
        o.o0 += f0[U];
        o.o1 += f1[U];
    }
    return o;
}

// scs_spmv_sweep_ap_hp's arguments as they lie in the kernel-argument segment (each at its natural alignment, in the order of the
// signature -- the layout of this struct): where the fused form finds `ep`
template <typename HT>
struct SweepHpKernargs {
    int wlog, nbuf;
    const int *tile_ids, *t_smin, *t_S;
    const unsigned long long *t_cnt_off;
    SweepParts P;
    const HT *x;
    HT *y;
    long x_len, n_store;
    int xcd_remap;
    AxpbyArgs<HT> ep;
};

// HT: type of x, y and the first part (double, or float for ap[sp_hp]); MID: ap[dp_sp_hp].  RPL rows per lane: a tile is
// RPL * blockDim.x rows, lane <-> rows tid, tid + blockDim.x, ...  nbuf: LDS buffers (2: window s+1 lands while window s is consumed).
// EP = 1: the store epilogue of uspmv_spmv_ap_hp_axpby (uspmv_device.hpp) on the value the plain form stores.  No thread of a sweep tile
// leaves early, and the window buffers are dead behind the last window: the reduction takes the front of them.
template <typename HT, bool MID, bool NT, int U, int RPL, int PAIRM, int EP = 0>
__global__ void __launch_bounds__(1024) scs_spmv_sweep_ap_hp(const int wlog, const int nbuf, const int *__restrict__ tile_ids,
        const int *__restrict__ t_smin, const int *__restrict__ t_S, const unsigned long long *__restrict__ t_cnt_off, const SweepParts P,
        const HT *__restrict__ x, HT *__restrict__ y, const long x_len, const long n_store, const int xcd_remap, const AxpbyArgs<HT> ep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sweep_smem[];
    constexpr int EPL = 16 / (int)sizeof(HT);           // elements per 16-byte DMA lane
    constexpr int EPP = 1024 / (int)sizeof(HT);         // elements per 1-KiB piece (one wave-instruction)
    const unsigned bt = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const int T = blockDim.x, nw = T >> 6;              // threads, waves of the workgroup
    const long R = (long)T * RPL;                       // rows of the tile
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tile = tile_ids[bt], smin = t_smin[bt], S = t_S[bt];
    const long W = 1L << wlog;
    const int n_pieces = (int)(W / EPP);
    const long coff = (long)t_cnt_off[bt] + threadIdx.x;                         // + h*T + s*R: the lane's count byte, in every part's array
    const HT *const va0 = (const HT *)P.vals[0];
    const float *const va1 = (const float *)P.vals[1];
    const unsigned short *const va2 = (const unsigned short *)P.vals[2];
    unsigned o[RPL][3];
#pragma unroll
    for (int h = 0; h < RPL; ++h)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[h][k] = 0u;
            if (k != 1 || MID) o[h][k] = (unsigned)__builtin_amdgcn_readfirstlane(P.wave_off[k][bt * (nw * RPL) + h * nw + wave]);
        }
    HT *const xs_all = (HT *)sweep_smem;                 // buffer b starts at element b * W

    auto stage = [&](const int s, const int b) {
        const long g0 = (long)(smin + s) << wlog;
        for (int p = wave; p < n_pieces; p += nw) {
            const long gi = g0 + (long)p * EPP + lane * EPL;
            const long lo = (long)b * W + (long)p * EPP;   // first element of the piece in LDS
            if (gi + EPL <= x_len) {
                __builtin_amdgcn_global_load_lds((glb_cvoid_t *)(x + gi), (lds_void_t *)(sweep_smem + lo * (long)sizeof(HT)), 16, 0, 0);
            } else {
#pragma unroll
                for (int e = 0; e < EPL; ++e)
                    if (gi + e < x_len) xs_all[lo + lane * EPL + e] = x[gi + e];
            }
        }
    };

    double acc[RPL][3];
    int c_cur[RPL][3];
#pragma unroll
    for (int h = 0; h < RPL; ++h)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[h][k] = 0.0; c_cur[h][k] = 0;
            if (S > 0 && (k != 1 || MID)) c_cur[h][k] = P.cnt[k][coff + h * T];
        }
    if (nbuf == 2 && S > 0) stage(0, 0);
    for (int s = 0; s < S; ++s) {
        const int cb = nbuf == 2 ? (s & 1) : 0;
        const HT *cur = xs_all + (long)cb * W;
        if (nbuf == 1) {
            __syncthreads();                              // everybody is through with window s-1
            stage(s, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's share of window s has landed
        __syncthreads();
        int c_next[RPL][3];
#pragma unroll
        for (int h = 0; h < RPL; ++h)
#pragma unroll
            for (int k = 0; k < 3; ++k) c_next[h][k] = 0;
        if (s + 1 < S) {
            if (nbuf == 2) stage(s + 1, cb ^ 1);              // that buffer was read last in window s-1: all waves are past it
#pragma unroll
            for (int h = 0; h < RPL; ++h)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k != 1 || MID) c_next[h][k] = P.cnt[k][coff + (long)(s + 1) * R + h * T];
        }
        constexpr bool MF = PAIRM == 2;
#pragma unroll
        for (int h = 0; h < RPL; ++h) {
            if constexpr (PAIRM != 0 && MID) {         // hi alone, then mid and hp side by side
                o[h][0] = hp_window<HT, HT, U, NT>(cur, c_cur[h][0], va0, P.idx[0], o[h][0], acc[h][0]);
                const HpOffs r = hp_window2<float, unsigned short, HT, U, NT, MF>(cur, c_cur[h][1], c_cur[h][2], va1, P.idx[1], va2, P.idx[2],
                                                                                  HpOffs{o[h][1], o[h][2]}, acc[h][1], acc[h][2]);
                o[h][1] = r.o0; o[h][2] = r.o1;
            } else if constexpr (PAIRM != 0) {         // hi and hp side by side
                const HpOffs r = hp_window2<HT, unsigned short, HT, U, NT, MF>(cur, c_cur[h][0], c_cur[h][2], va0, P.idx[0], va2, P.idx[2],
                                                                               HpOffs{o[h][0], o[h][2]}, acc[h][0], acc[h][2]);
                o[h][0] = r.o0; o[h][2] = r.o1;
            } else {                                   // one part after the other
                o[h][0] = hp_window<HT, HT, U, NT>(cur, c_cur[h][0], va0, P.idx[0], o[h][0], acc[h][0]);
                if constexpr (MID) o[h][1] = hp_window<float, HT, U, NT>(cur, c_cur[h][1], va1, P.idx[1], o[h][1], acc[h][1]);
                o[h][2] = hp_window<unsigned short, HT, U, NT>(cur, c_cur[h][2], va2, P.idx[2], o[h][2], acc[h][2]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) c_cur[h][k] = c_next[h][k];
        }
    }
    // trailing padding of every part of the row, applied once in the part's own type (see sweep_plan.cpp)
    [[maybe_unused]] double d0 = 0.0, d1 = 0.0;           // (EP: the lane's dot terms over its RPL rows)
    // EP: the epilogue's arguments are read from the kernel-argument segment HERE, behind the last window, and not through `ep`: loaded
    // at the kernel's entry, their 13 scalar registers stay live across the window loop, and the four-rows-per-lane dp + hp form -- 128
    // vector registers without them -- then spills scalars into a 129th, i.e. into scratch.  (`ep` itself stays in the signature: it is
    // what the launch fills.)
    AxpbyArgs<HT> e;
    if constexpr (EP != 0) {
        typedef const char __attribute__((address_space(4))) *karg_t;
        karg_t kp = (karg_t)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));                      // (opaque: the loads below cannot move above this point)
        kp += offsetof(SweepHpKernargs<HT>, ep);
#define KARG(T, M) (*(T const __attribute__((address_space(4))) *)(kp + offsetof(AxpbyArgs<HT>, M)))
        e.alpha = KARG(HT, alpha); e.beta = KARG(HT, beta);
        e.z = KARG(const HT *, z); e.w = KARG(const HT *, w);
        e.part = KARG(double *, part); e.n_dot = KARG(long, n_dot); e.slot0 = KARG(unsigned, slot0);
#undef KARG
    }
#pragma unroll
    for (int h = 0; h < RPL; ++h) {
        const long row = (long)tile * R + h * T + threadIdx.x;
        const long pr = (long)bt * R + h * T + threadIdx.x;
        const int pc0 = P.pad[0][pr];
        if (pc0 >= 0) acc[h][0] = ap_step(HT(0), x[pc0], acc[h][0]);
        if constexpr (MID) {
            const int pc1 = P.pad[1][pr];
            if (pc1 >= 0) acc[h][1] = ap_step(0.0f, x[pc1], acc[h][1]);
        }
        const int pc2 = P.pad[2][pr];
        if (pc2 >= 0) acc[h][2] = ap_step((unsigned short)0, x[pc2], acc[h][2]);
        if constexpr (EP == 0) {
            if (row < n_store) st_y<NT>(y + row, ap_hp_y<HT, MID>(acc[h][0], acc[h][1], acc[h][2]));
        } else {
            if (row < n_store) st_y<NT>(y + row, axpby_row(e, row, ap_hp_y<HT, MID>(acc[h][0], acc[h][1], acc[h][2]), d0, d1));
        }
    }
    if constexpr (EP != 0) axpby_reduce(e, bt, d0, d1, (double *)sweep_smem);
}

template <typename HT, bool MID>
int launch_sweep_hp(const uspmv_dmat *A, const HT *x, HT *y, hipStream_t st, const AxpbyArgs<HT> *ep) {
    const auto &w = A->sw;
    const SweepParts P = sweep_parts(w);
    const long W = 1L << w.wlog;
    // (two buffers only where the plan's window leaves room for them)
    const int nbuf = (g_tune.sweep_nbuf == 2 && 2 * (size_t)W * sizeof(HT) <= WG_LDS_BYTES) ? 2 : 1;
    const size_t lds = (size_t)nbuf * (size_t)W * sizeof(HT);
    const int threads = sweep_threads(w);
    const int rpl = w.tile_rows / threads;
#define SWH_LAUNCH(NTV, UU, RP, PM)                                                                                              \
    do {                                                                                                                         \
        auto kfn = scs_spmv_sweep_ap_hp<HT, MID, NTV, UU, RP, PM>;                                                               \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);  \
        hipLaunchKernelGGL(kfn, dim3((unsigned)w.n_tiles), dim3(threads), lds, st, w.wlog, nbuf, w.tile_ids.get(), w.smin.get(),  \
                           w.S.get(), (const unsigned long long *)w.cnt_off, P, x, y, (long)w.x_len, (long)A->n_store,           \
                           g_tune.sweep_remap, AxpbyArgs<HT>{});                                                                 \
    } while (0)
    // the fused instantiations: non-temporal, eight rounds, the default pairing (spmv_ap_hp_axpby_route)
#define SWH_AXPBY(RP)                                                                                                            \
    do {                                                                                                                         \
        auto kfn = scs_spmv_sweep_ap_hp<HT, MID, true, 8, RP, 2, 1>;                                                             \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);  \
        hipLaunchKernelGGL(kfn, dim3((unsigned)w.n_tiles), dim3(threads), lds, st, w.wlog, nbuf, w.tile_ids.get(), w.smin.get(),  \
                           w.S.get(), (const unsigned long long *)w.cnt_off, P, x, y, (long)w.x_len, (long)A->n_store,           \
                           g_tune.sweep_remap, *ep);                                                                             \
    } while (0)
    if (ep) {
        if (!(g_tune.nontemporal && g_tune.sweep_unroll >= 8 && g_tune.sweep_pair == 2))
            return uspmv::fail(USPMV_ERR_UNSUPPORTED, "launch_sweep_hp: no fused instantiation under this tuning");
        if (rpl == 4) SWH_AXPBY(4); else if (rpl == 2) SWH_AXPBY(2); else SWH_AXPBY(1);
        HIP_TRY(hipGetLastError());
        return USPMV_OK;
    }
#undef SWH_AXPBY
#define SWH_LAUNCH_P(NTV, UU, RP) do { if (g_tune.sweep_pair == 2) SWH_LAUNCH(NTV, UU, RP, 2); else if (g_tune.sweep_pair == 1) SWH_LAUNCH(NTV, UU, RP, 1); else SWH_LAUNCH(NTV, UU, RP, 0); } while (0)
#define SWH_LAUNCH_R(NTV, UU) do { if (rpl == 4) SWH_LAUNCH_P(NTV, UU, 4); else if (rpl == 2) SWH_LAUNCH_P(NTV, UU, 2); else SWH_LAUNCH_P(NTV, UU, 1); } while (0)
#define SWH_LAUNCH_U(NTV) do { if (g_tune.sweep_unroll >= 8) SWH_LAUNCH_R(NTV, 8); else SWH_LAUNCH_R(NTV, 4); } while (0)
    if (g_tune.nontemporal) SWH_LAUNCH_U(true); else SWH_LAUNCH_U(false);
#undef SWH_LAUNCH_U
#undef SWH_LAUNCH_R
#undef SWH_LAUNCH_P
#undef SWH_LAUNCH
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

}  // namespace

namespace uspmv_dev {

int launch_spmv_sweep_ap_hp(const uspmv_dmat *hi, bool mid, const void *x, void *y, hipStream_t st, const void *ep) {
    if (hi->sw.n_tiles == 0) return USPMV_OK;
    if (hi->dtype == USPMV_F32) return launch_sweep_hp<float, false>(hi, (const float *)x, (float *)y, st, (const AxpbyArgs<float> *)ep);
    if (mid) return launch_sweep_hp<double, true>(hi, (const double *)x, (double *)y, st, (const AxpbyArgs<double> *)ep);
    return launch_sweep_hp<double, false>(hi, (const double *)x, (double *)y, st, (const AxpbyArgs<double> *)ep);
}

}  // namespace uspmv_dev
