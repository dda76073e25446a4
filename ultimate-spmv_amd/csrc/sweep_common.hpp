// What the column-window sweep kernels share (sweep_kernels.hip: one struct and the ap[dp_sp] pair; sweep_ap_hp_kernels.hip: the
// splits with an fp16 part; ap_spmmv_sweep.hip, ap_hp_spmmv_sweep.hip: their block forms): the address-space types of the LDS-DMA, the
// lane's place in a ballot, the plan's per-part arrays as a kernel argument, the operands of a window element, and the batches of
// accumulator updates under the rounds' lane masks.
#pragma once
#include "uspmv_device.hpp"

namespace {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_cvoid_t;

// active lanes strictly below this one
__device__ __forceinline__ unsigned lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the plan's per-part arrays as the kernels of the splits with an fp16 part take them: slot 0 hi, 1 mid, 2 hp; [1] is unused unless
// ap[dp_sp_hp]
struct SweepParts {
    const unsigned *wave_off[3];
    const unsigned char *cnt[3];
    const void *vals[3];
    const unsigned short *idx[3];
    const int *pad[3];
};
// the plan stores its parts in the order of the split: [hi, hp] goes to slots 0 and 2, [hi, mid, hp] to 0, 1, 2
inline SweepParts sweep_parts(const uspmv_dmat::SweepPlan &w) {
    SweepParts P{};
    for (int k = 0; k < w.n_parts; ++k) {
        const int slot = (w.n_parts == 2 && k == 1) ? 2 : k;
        const auto &pt = w.part[k];
        P.wave_off[slot] = pt.wave_off; P.cnt[slot] = pt.cnt; P.vals[slot] = pt.vals; P.idx[slot] = pt.idx; P.pad[slot] = pt.pad;
    }
    return P;
}

// the stored value widened to the type the product is formed in (double for a double x, float for a float x); exact
__device__ __forceinline__ double hp_widen(double v, double) { return v; }
__device__ __forceinline__ double hp_widen(float v, double) { return (double)v; }
__device__ __forceinline__ double hp_widen(unsigned short v, double) { return (double)hp_val(v); }
__device__ __forceinline__ float hp_widen(float v, float) { return v; }
__device__ __forceinline__ float hp_widen(unsigned short v, float) { return hp_val(v); }

// the BS operands of window element i of a block kernel's LDS image: one X row of the row-major image (16-byte reads; 8 bytes for two
// floats), or one element of each plane
template <typename HT, int BS, bool XCOL>
__device__ __forceinline__ void window_x(const HT *win, const int wlog, const unsigned i, HT (&x)[BS]) {
    if constexpr (XCOL) {
#pragma unroll
        for (int w = 0; w < BS; ++w) x[w] = win[i + ((unsigned)w << wlog)];
    } else {
        constexpr int PE = (int)(16 / sizeof(HT)) < BS ? (int)(16 / sizeof(HT)) : BS;
        typedef HT piece_t __attribute__((ext_vector_type(PE)));
        const piece_t *xp = (const piece_t *)(win + i * BS);
#pragma unroll
        for (int k = 0; k < BS / PE; ++k) {
            const piece_t t = xp[k];
#pragma unroll
            for (int e = 0; e < PE; ++e) x[k * PE + e] = t[e];
        }
    }
}

// A batch of U fused multiply-adds, each under ITS round's lane mask: EXEC is set to the round's ballot, so that a lane that sits the
// round out keeps its accumulator -- not even a signed zero is added -- without the copy + two selects per round that the
// select form costs (v_mov_b64, v_fmac_f64, 2 x v_cndmask_b32: the rounds are issue-bound, profiles/r03/config4b.txt).  All lanes
// of the wave are active around the call (the kernel's control flow is wave-uniform); EXEC is saved and restored regardless.
template <int U>
__device__ __forceinline__ void masked_fma_batch(double &acc, const double (&v)[U], const double (&x)[U], const unsigned long long (&m)[U]) {
    static_assert(U == 4 || U == 8, "batch of 4 or 8 rounds");
    unsigned long long save;
    if constexpr (U == 8)
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "s_mov_b64 exec, %[m0]\n\tv_fmac_f64 %[a], %[v0], %[x0]\n\t"
                     "s_mov_b64 exec, %[m1]\n\tv_fmac_f64 %[a], %[v1], %[x1]\n\t"
                     "s_mov_b64 exec, %[m2]\n\tv_fmac_f64 %[a], %[v2], %[x2]\n\t"
                     "s_mov_b64 exec, %[m3]\n\tv_fmac_f64 %[a], %[v3], %[x3]\n\t"
                     "s_mov_b64 exec, %[m4]\n\tv_fmac_f64 %[a], %[v4], %[x4]\n\t"
                     "s_mov_b64 exec, %[m5]\n\tv_fmac_f64 %[a], %[v5], %[x5]\n\t"
                     "s_mov_b64 exec, %[m6]\n\tv_fmac_f64 %[a], %[v6], %[x6]\n\t"
                     "s_mov_b64 exec, %[m7]\n\tv_fmac_f64 %[a], %[v7], %[x7]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(save)
                     : [m0] "s"(m[0]), [m1] "s"(m[1]), [m2] "s"(m[2]), [m3] "s"(m[3]), [m4] "s"(m[4]), [m5] "s"(m[5]), [m6] "s"(m[6]), [m7] "s"(m[7]),
                       [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3]), [v4] "v"(v[4]), [v5] "v"(v[5]), [v6] "v"(v[6]), [v7] "v"(v[7]),
                       [x0] "v"(x[0]), [x1] "v"(x[1]), [x2] "v"(x[2]), [x3] "v"(x[3]), [x4] "v"(x[4]), [x5] "v"(x[5]), [x6] "v"(x[6]), [x7] "v"(x[7]));
    else
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "s_mov_b64 exec, %[m0]\n\tv_fmac_f64 %[a], %[v0], %[x0]\n\t"
                     "s_mov_b64 exec, %[m1]\n\tv_fmac_f64 %[a], %[v1], %[x1]\n\t"
                     "s_mov_b64 exec, %[m2]\n\tv_fmac_f64 %[a], %[v2], %[x2]\n\t"
                     "s_mov_b64 exec, %[m3]\n\tv_fmac_f64 %[a], %[v3], %[x3]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(save)
                     : [m0] "s"(m[0]), [m1] "s"(m[1]), [m2] "s"(m[2]), [m3] "s"(m[3]),
                       [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3]), [x0] "v"(x[0]), [x1] "v"(x[1]), [x2] "v"(x[2]), [x3] "v"(x[3]));
}
template <int U>
__device__ __forceinline__ void masked_fma_batch(float &acc, const float (&v)[U], const float (&x)[U], const unsigned long long (&m)[U]) {
    static_assert(U == 4 || U == 8, "batch of 4 or 8 rounds");
    unsigned long long save;
    if constexpr (U == 8)
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "s_mov_b64 exec, %[m0]\n\tv_fmac_f32 %[a], %[v0], %[x0]\n\t"
                     "s_mov_b64 exec, %[m1]\n\tv_fmac_f32 %[a], %[v1], %[x1]\n\t"
                     "s_mov_b64 exec, %[m2]\n\tv_fmac_f32 %[a], %[v2], %[x2]\n\t"
                     "s_mov_b64 exec, %[m3]\n\tv_fmac_f32 %[a], %[v3], %[x3]\n\t"
                     "s_mov_b64 exec, %[m4]\n\tv_fmac_f32 %[a], %[v4], %[x4]\n\t"
                     "s_mov_b64 exec, %[m5]\n\tv_fmac_f32 %[a], %[v5], %[x5]\n\t"
                     "s_mov_b64 exec, %[m6]\n\tv_fmac_f32 %[a], %[v6], %[x6]\n\t"
                     "s_mov_b64 exec, %[m7]\n\tv_fmac_f32 %[a], %[v7], %[x7]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(save)
                     : [m0] "s"(m[0]), [m1] "s"(m[1]), [m2] "s"(m[2]), [m3] "s"(m[3]), [m4] "s"(m[4]), [m5] "s"(m[5]), [m6] "s"(m[6]), [m7] "s"(m[7]),
                       [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3]), [v4] "v"(v[4]), [v5] "v"(v[5]), [v6] "v"(v[6]), [v7] "v"(v[7]),
                       [x0] "v"(x[0]), [x1] "v"(x[1]), [x2] "v"(x[2]), [x3] "v"(x[3]), [x4] "v"(x[4]), [x5] "v"(x[5]), [x6] "v"(x[6]), [x7] "v"(x[7]));
    else
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "s_mov_b64 exec, %[m0]\n\tv_fmac_f32 %[a], %[v0], %[x0]\n\t"
                     "s_mov_b64 exec, %[m1]\n\tv_fmac_f32 %[a], %[v1], %[x1]\n\t"
                     "s_mov_b64 exec, %[m2]\n\tv_fmac_f32 %[a], %[v2], %[x2]\n\t"
                     "s_mov_b64 exec, %[m3]\n\tv_fmac_f32 %[a], %[v3], %[x3]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(save)
                     : [m0] "s"(m[0]), [m1] "s"(m[1]), [m2] "s"(m[2]), [m3] "s"(m[3]),
                       [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3]), [x0] "v"(x[0]), [x1] "v"(x[1]), [x2] "v"(x[2]), [x3] "v"(x[3]));
}

// The same for the chains whose step is not an FMA (ap[sp_hp]: the product is rounded to float first): a batch of U additions of the
// finished terms t[u], each under its round's lane mask.
template <int U>
__device__ __forceinline__ void masked_add_batch(double &acc, const double (&t)[U], const unsigned long long (&m)[U]) {
    static_assert(U == 4 || U == 8, "batch of 4 or 8 rounds");
    unsigned long long save;
    if constexpr (U == 8)
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "s_mov_b64 exec, %[m0]\n\tv_add_f64 %[a], %[a], %[t0]\n\t"
                     "s_mov_b64 exec, %[m1]\n\tv_add_f64 %[a], %[a], %[t1]\n\t"
                     "s_mov_b64 exec, %[m2]\n\tv_add_f64 %[a], %[a], %[t2]\n\t"
                     "s_mov_b64 exec, %[m3]\n\tv_add_f64 %[a], %[a], %[t3]\n\t"
                     "s_mov_b64 exec, %[m4]\n\tv_add_f64 %[a], %[a], %[t4]\n\t"
                     "s_mov_b64 exec, %[m5]\n\tv_add_f64 %[a], %[a], %[t5]\n\t"
                     "s_mov_b64 exec, %[m6]\n\tv_add_f64 %[a], %[a], %[t6]\n\t"
                     "s_mov_b64 exec, %[m7]\n\tv_add_f64 %[a], %[a], %[t7]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(save)
                     : [m0] "s"(m[0]), [m1] "s"(m[1]), [m2] "s"(m[2]), [m3] "s"(m[3]), [m4] "s"(m[4]), [m5] "s"(m[5]), [m6] "s"(m[6]), [m7] "s"(m[7]),
                       [t0] "v"(t[0]), [t1] "v"(t[1]), [t2] "v"(t[2]), [t3] "v"(t[3]), [t4] "v"(t[4]), [t5] "v"(t[5]), [t6] "v"(t[6]), [t7] "v"(t[7]));
    else
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "s_mov_b64 exec, %[m0]\n\tv_add_f64 %[a], %[a], %[t0]\n\t"
                     "s_mov_b64 exec, %[m1]\n\tv_add_f64 %[a], %[a], %[t1]\n\t"
                     "s_mov_b64 exec, %[m2]\n\tv_add_f64 %[a], %[a], %[t2]\n\t"
                     "s_mov_b64 exec, %[m3]\n\tv_add_f64 %[a], %[a], %[t3]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(save)
                     : [m0] "s"(m[0]), [m1] "s"(m[1]), [m2] "s"(m[2]), [m3] "s"(m[3]), [t0] "v"(t[0]), [t1] "v"(t[1]), [t2] "v"(t[2]), [t3] "v"(t[3]));
}

// The block kernels (ap_spmmv_sweep.hip, ap_hp_spmmv_sweep.hip): one round of one chain for BS vectors: BS FMAs under the round's lane mask (EXEC), see masked_fma_batch.  All lanes of the wave are
// active around the call.
template <int BS>
__device__ __forceinline__ void masked_fma_round(double (&a)[BS], const double v, const double (&x)[BS], const unsigned long long m) {
    static_assert(BS == 2 || BS == 4 || BS == 8, "2, 4 or 8 vectors per pass");
    unsigned long long save;
    if constexpr (BS == 2)
        asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[m]\n\t"
                     "v_fmac_f64 %[a0], %[v], %[x0]\n\tv_fmac_f64 %[a1], %[v], %[x1]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [sv] "=&s"(save)
                     : [m] "s"(m), [v] "v"(v), [x0] "v"(x[0]), [x1] "v"(x[1]));
    else if constexpr (BS == 4)
        asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[m]\n\t"
                     "v_fmac_f64 %[a0], %[v], %[x0]\n\tv_fmac_f64 %[a1], %[v], %[x1]\n\t"
                     "v_fmac_f64 %[a2], %[v], %[x2]\n\tv_fmac_f64 %[a3], %[v], %[x3]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3]), [sv] "=&s"(save)
                     : [m] "s"(m), [v] "v"(v), [x0] "v"(x[0]), [x1] "v"(x[1]), [x2] "v"(x[2]), [x3] "v"(x[3]));
    else
        asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[m]\n\t"
                     "v_fmac_f64 %[a0], %[v], %[x0]\n\tv_fmac_f64 %[a1], %[v], %[x1]\n\t"
                     "v_fmac_f64 %[a2], %[v], %[x2]\n\tv_fmac_f64 %[a3], %[v], %[x3]\n\t"
                     "v_fmac_f64 %[a4], %[v], %[x4]\n\tv_fmac_f64 %[a5], %[v], %[x5]\n\t"
                     "v_fmac_f64 %[a6], %[v], %[x6]\n\tv_fmac_f64 %[a7], %[v], %[x7]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3]), [a4] "+v"(a[4]), [a5] "+v"(a[5]),
                       [a6] "+v"(a[6]), [a7] "+v"(a[7]), [sv] "=&s"(save)
                     : [m] "s"(m), [v] "v"(v), [x0] "v"(x[0]), [x1] "v"(x[1]), [x2] "v"(x[2]), [x3] "v"(x[3]), [x4] "v"(x[4]),
                       [x5] "v"(x[5]), [x6] "v"(x[6]), [x7] "v"(x[7]));
}

// ... and of one chain whose step is not an FMA (a float x: the products are rounded to float first): BS additions of the finished
// terms under the round's lane mask, see masked_add_batch.
template <int BS>
__device__ __forceinline__ void masked_add_round(double (&a)[BS], const double (&t)[BS], const unsigned long long m) {
    static_assert(BS == 2 || BS == 4 || BS == 8, "2, 4 or 8 vectors per pass");
    unsigned long long save;
    if constexpr (BS == 2)
        asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[m]\n\t"
                     "v_add_f64 %[a0], %[a0], %[t0]\n\tv_add_f64 %[a1], %[a1], %[t1]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [sv] "=&s"(save)
                     : [m] "s"(m), [t0] "v"(t[0]), [t1] "v"(t[1]));
    else if constexpr (BS == 4)
        asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[m]\n\t"
                     "v_add_f64 %[a0], %[a0], %[t0]\n\tv_add_f64 %[a1], %[a1], %[t1]\n\t"
                     "v_add_f64 %[a2], %[a2], %[t2]\n\tv_add_f64 %[a3], %[a3], %[t3]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3]), [sv] "=&s"(save)
                     : [m] "s"(m), [t0] "v"(t[0]), [t1] "v"(t[1]), [t2] "v"(t[2]), [t3] "v"(t[3]));
    else
        asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[m]\n\t"
                     "v_add_f64 %[a0], %[a0], %[t0]\n\tv_add_f64 %[a1], %[a1], %[t1]\n\t"
                     "v_add_f64 %[a2], %[a2], %[t2]\n\tv_add_f64 %[a3], %[a3], %[t3]\n\t"
                     "v_add_f64 %[a4], %[a4], %[t4]\n\tv_add_f64 %[a5], %[a5], %[t5]\n\t"
                     "v_add_f64 %[a6], %[a6], %[t6]\n\tv_add_f64 %[a7], %[a7], %[t7]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3]), [a4] "+v"(a[4]), [a5] "+v"(a[5]),
                       [a6] "+v"(a[6]), [a7] "+v"(a[7]), [sv] "=&s"(save)
                     : [m] "s"(m), [t0] "v"(t[0]), [t1] "v"(t[1]), [t2] "v"(t[2]), [t3] "v"(t[3]), [t4] "v"(t[4]), [t5] "v"(t[5]),
                       [t6] "v"(t[6]), [t7] "v"(t[7]));
}

}  // namespace
