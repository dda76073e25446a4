// Adaptive precision on block vectors: the lane-per-row kernel and the staged (tile-local-column) kernel of all four kinds -- ap[dp_hp],
// ap[sp_hp], ap[dp_sp_hp] (uspmv_spmmv_ap_hp, dispatched here) and ap[dp_sp] (uspmv_spmmv_ap, dispatched in ap_spmmv_kernels.hip).  A kind
// is <HT, MID, LT>: HT the type of X, Y and the first part, MID whether a float part sits in the middle, LT the value type of the last
// part -- unsigned short (binary16 bits) for the three kinds with an fp16 part, float for ap[dp_sp], which is <double, false, float>.
// The reference has no twin (its CLI stops at "SpMMV is not yet implemented for AP kernels", code/utilities.hpp:1389, and its GPU path
// has no hp kernels at all, code/classes_structs.hpp:553-600); the numerics are those of uspmv_spmv_ap_hp / uspmv_spmv_ap applied to
// every column of X: per (row, v) one chain per part in slot order (ap_step), then ap_hp_y.  One lane per row everywhere and no chain is
// ever re-associated, so column v of Y is bitwise the single-vector product of column v of X.  See DESIGN.md 5.7, 5.8.
#include <type_traits>

#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace {

// y from the folded sum of the leading parts and the last part's chain: hi + last, (hi + mid) + hp, or (float)(sp + hp) -- ap_hp_y with
// the (hi + mid) already taken
template <typename HT>
__device__ __forceinline__ HT ap_hp_fold_y(double s, double q) { return ap_hp_y<HT, false>(s, 0.0, q); }

// Any b, either layout, any C, no alignment demands: the block form of scs_spmmv_rows for a split.  VB vectors per pass held in
// registers; per vector the parts' chains run one after the other with global gathers of X, (hi + mid) folded before the last chain starts.
// colwise: X[col + v*ld], Y[row + v*ld];  rowwise: X[col*b + v], Y[row*b + v].
// IDS 1: the chunks ids[0 .. n_chunks) instead of all (the rest chunks of a column-window sweep plan, the chunk lists of the distributed
// step); IDS 2: the tiles ids[0 .. n_chunks), tile t = the rows [t * unit_rows, (t + 1) * unit_rows) as far as the matrix has them
// (n_total chunks) -- tile lists at widths, alignments and leading dimensions the staged kernel does not take.  An entry < 0 is a
// conditional entry that was switched off: its lanes return, no row of it is touched.
template <int VB, bool ROWWISE, bool NT, typename HT, bool MID, typename LT, int IDS = 0>
__global__ void scs_spmmv_ap_rows(const long n_chunks, const int C, const ApHpParts P, const HT *__restrict__ X, HT *__restrict__ Y,
                                  const int b, const long ld, const int xcd_remap, const int *__restrict__ ids, const int unit_rows,
                                  const long n_total) {
    const unsigned lb = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    long row = (long)lb * blockDim.x + threadIdx.x;
    long c;
    int i;
    if constexpr (IDS == 2) {
        const long u = row / unit_rows;
        if (u >= n_chunks) return;
        const long t = ids[u];
        if (t < 0) return;
        row = t * unit_rows + (row - u * unit_rows);
        c = row / C;
        i = (int)(row - c * C);
        if (c >= n_total) return;
    } else {
        c = row / C;
        i = (int)(row - c * C);
        if (c >= n_chunks) return;
        if constexpr (IDS == 1) {
            c = ids[c];
            if (c < 0) return;
            row = c * C + i;
        }
    }
    auto chain = [&](auto vtag, const int k, const int v0, double (&acc)[VB]) {
        typedef decltype(vtag) VT;
        const long cs = P.cp[k][c];
        const int L = P.cl[k][c];
        const VT *vp = (const VT *)P.va[k] + cs + i;
        const int *cp = P.ci[k] + cs + i;
        for (int j = 0; j < L; ++j) {
            const VT a = ld_stream<NT>(vp + (long)j * C);
            const long col = ld_stream<NT>(cp + (long)j * C);
#pragma unroll
            for (int v = 0; v < VB; ++v)
                if (v0 + v < b) acc[v] = ap_step(a, ROWWISE ? X[col * b + v0 + v] : X[col + (long)(v0 + v) * ld], acc[v]);
        }
    };
    for (int v0 = 0; v0 < b; v0 += VB) {
        double s[VB], q[VB];
#pragma unroll
        for (int v = 0; v < VB; ++v) { s[v] = 0.0; q[v] = 0.0; }
        chain(HT(), 0, v0, s);
        if constexpr (MID) {
            chain(float(), 1, v0, q);
#pragma unroll
            for (int v = 0; v < VB; ++v) { s[v] = s[v] + q[v]; q[v] = 0.0; }
        }
        chain(LT(), 2, v0, q);
#pragma unroll
        for (int v = 0; v < VB; ++v) {
            if (v0 + v < b) {
                if (ROWWISE) st_y<NT>(Y + (row * b + v0 + v), ap_hp_fold_y<HT>(s[v], q[v]));
                else st_y<NT>(Y + (row + (long)(v0 + v) * ld), ap_hp_fold_y<HT>(s[v], q[v]));
            }
        }
    }
}

// A staged X row: BS elements of HT, moved in pieces of 16 bytes (8 bytes for two floats)
template <typename HT, int BS>
struct XRow {
    static constexpr int PE = (int)(16 / sizeof(HT)) < BS ? (int)(16 / sizeof(HT)) : BS;   // elements per piece
    static constexpr int NP = BS / PE;                                                      // pieces per row
    typedef HT piece_t __attribute__((ext_vector_type(PE)));
};

// One part's chain of the staged kernel: values one per lane and slot, the 16-bit local indices four slots per 8-byte load (the streams of
// scs_spmv_ap_tlc / scs_spmv_ap_hp_tlc: sizeof(VT) + 2 bytes per entry), the X row of a slot BS elements from LDS.  W: slots per batch,
// 8 or 4.
template <int BS, bool NT, int W, typename VT, typename HT>
__device__ __forceinline__ void tlc_block_chain(const VT *__restrict__ vp, const unsigned long long *__restrict__ cq, const int L,
                                                const int C, const HT *xs, double (&acc)[BS]) {
    typedef XRow<HT, BS> R;
    auto step = [&](const VT a, const unsigned li) {
        const typename R::piece_t *xp = (const typename R::piece_t *)(xs + li * BS);
#pragma unroll
        for (int k = 0; k < R::NP; ++k) {
            const typename R::piece_t xv = xp[k];
#pragma unroll
            for (int e = 0; e < R::PE; ++e) acc[k * R::PE + e] = ap_step(a, xv[e], acc[k * R::PE + e]);
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

// ... and with 32-bit columns and X gathered from global memory in the caller's layout (tiles without a line list).
// X points at vector v0 of the pass: row-major X[col * xstride + v], column-major X[col + v * xstride].
template <int BS, bool NT, bool XCOL, typename VT, typename HT>
__device__ __forceinline__ void gather_block_chain(const VT *__restrict__ vp, const int *__restrict__ cp, const int L, const int C,
                                                   const HT *__restrict__ X, const long xstride, double (&acc)[BS]) {
    typedef XRow<HT, BS> R;
    for (int j = 0; j < L; ++j) {
        const VT a = ld_stream<NT>(vp + (long)j * C);
        const long col = ld_stream<NT>(cp + (long)j * C);
        if constexpr (XCOL) {
#pragma unroll
            for (int v = 0; v < BS; ++v) acc[v] = ap_step(a, X[col + v * xstride], acc[v]);
        } else {
            const typename R::piece_t *xp = (const typename R::piece_t *)(X + col * xstride);
#pragma unroll
            for (int k = 0; k < R::NP; ++k) {
                const typename R::piece_t xv = xp[k];
#pragma unroll
                for (int e = 0; e < R::PE; ++e) acc[k * R::PE + e] = ap_step(a, xv[e], acc[k * R::PE + e]);
            }
        }
    }
}

// Slots per batch of the staged kernel's chains: four where the kernel makes several passes (the pass loop costs registers, and 128 is
// all a 1024-thread workgroup leaves a lane); the kinds with an fp16 part also at eight vectors per pass (<8, 8> spilled 2-3 VGPRs
// there), where ap[dp_sp] keeps the eight it was measured with.
constexpr int tlc_chain_slots(int B, int BS, bool pair) { return ((BS >= 8 && !pair) || (BS < B && BS >= 4)) ? 4 : 8; }

// Column-major X whose columns start on multiples of NE elements only (NE * sizeof(HT) = 8 or 4 bytes): the nl lines of a tile into
// LDS as [X row][BS], in pieces of NE elements.  Piece p: the piece of the line's 16 rows fastest, then the vector, then the line, so
// the 16 / NE lanes of one (line, vector) read consecutive addresses.  X points at the first vector of the pass; rows at or beyond
// x_rows are staged as +0 and never read.
template <int BS, int NE, typename HT>
__device__ __forceinline__ void stage_x_narrow(HT *xs, const HT *__restrict__ X, const long ld, const int *__restrict__ lines, const int nl,
                                               const long x_rows) {
    constexpr int NPL = 16 / NE;              // pieces per (line, vector)
    constexpr int PPL = BS * NPL;
    typedef HT npiece_t __attribute__((ext_vector_type(NE)));
    for (int p = threadIdx.x; p < nl * PPL; p += blockDim.x) {
        const int k = p / PPL, w = p - k * PPL;
        const int v = w / NPL, r0 = (w % NPL) * NE;
        const long xrow = (long)lines[k] * 16 + r0;
        const HT *xp = X + xrow + (long)v * ld;
        npiece_t t;
        if (xrow + NE <= x_rows) t = *(const npiece_t *)xp;
        else {
#pragma unroll
            for (int e = 0; e < NE; ++e) t[e] = xrow + e < x_rows ? xp[e] : (HT)0;
        }
        HT *dst = xs + ((long)k * 16 + r0) * BS + v;
#pragma unroll
        for (int e = 0; e < NE; ++e) dst[e * BS] = t[e];
    }
}

// The parts' shared tile-local-column plan on block vectors of width B: the block form of scs_spmv_ap_tlc / scs_spmv_ap_hp_tlc.  A line
// of the plan (16 consecutive x elements there) is 16 consecutive X rows here.  Per pass BS of the B vectors:
// the tile's lines are staged once in LDS as [X row][BS] in the type of X, then every part runs its chain from its own streams
// (sizeof(value) + 2 bytes per entry and pass) with BS accumulators and the X operands from LDS.  (hi + mid) is folded per vector before
// the hp chain starts -- exactly the (dp + sp) + hp of ap_hp_y -- so at most two sets of BS double accumulators are live.  B / BS
// passes: a tile whose lines do not fit LDS at the full width still keeps its gathers out of the L2 -> L1 path, at the price of
// streaming its entries again (from the caches: the same workgroup has just read them).
// XCOL: X column-major (X[col + v*ld]), staged straight from the caller's columns: per line and vector 16 consecutive elements (128 or
// 64 contiguous bytes), read in 16-byte pieces and stored element by element into the rows of LDS; else row-major (X[col*B + v]), read
// and stored in 16-byte pieces (8 bytes for float X at BS = 2).  Rows at or beyond x_rows are staged as zeros.  Tiles without a line
// list gather from global X.  YCOL: Y[row + v*ld], else Y[row*B + v].
// IDS: workgroup g runs tile tile_ids[g] (the interior / boundary lists of the distributed block step, uspmv_spmmv_ap_tiles); an entry < 0
// is a conditional entry that was switched off and returns before the first barrier, uniformly for the workgroup.
// xpiece (the list form of the kinds with an fp16 part on column-major X only; 16 everywhere else): the bytes of the widest power-of-two
// piece every column of X starts aligned to -- 16, or 8 / 4 where ld * sizeof(HT) is no multiple of 16 (a rank's padded_vec_size is
// whatever its halo makes it).  Below 16 the columns are staged in pieces of that size, the pieces of one (line, vector) on consecutive
// lanes: a wave's loads of a line run over its 128 (64) contiguous bytes, column after column.
template <int B, int BS, int CT, bool NT, typename HT, bool MID, typename LT, bool XCOL, bool YCOL, bool IDS = false>
__global__ void __launch_bounds__(1024) scs_spmmv_ap_tlc(const long n_chunks, const int C_rt, const ApHpParts P, const HT *__restrict__ X,
                                                         HT *__restrict__ Y, const long ld, const int *__restrict__ tile_line_ptr,
                                                         const int *__restrict__ tile_lines, const long x_rows, const int xcd_remap,
                                                         const int *__restrict__ tile_ids = nullptr, const int xpiece = 16) {
    static_assert(BS >= 2 && BS <= B && B % BS == 0, "whole passes");
    extern __shared__ __attribute__((aligned(16))) unsigned char tlc_smem[];
    HT *xs = (HT *)tlc_smem;
    typedef XRow<HT, BS> R;
    typedef typename R::piece_t piece_t;
    constexpr bool PAIR = std::is_same<LT, float>::value;    // ap[dp_sp]
    constexpr bool NARROW = IDS && XCOL && !PAIR;            // the forms that read xpiece
    constexpr int W = tlc_chain_slots(B, BS, PAIR);
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
#pragma unroll 1
    for (int v0 = 0; v0 < B; v0 += BS) {
        double s[BS], q[BS];
#pragma unroll
        for (int v = 0; v < BS; ++v) { s[v] = 0.0; q[v] = 0.0; }
        if (nl > 0) {
            if (v0) __syncthreads();              // (the previous pass has read its X rows)
            if (NARROW && xpiece < 16) {          // (uniform for the workgroup)
                if (sizeof(HT) == 4 && xpiece == 8) stage_x_narrow<BS, 2>(xs, X + (long)v0 * ld, ld, tile_lines + lp0, nl, x_rows);
                else stage_x_narrow<BS, 1>(xs, X + (long)v0 * ld, ld, tile_lines + lp0, nl, x_rows);
            } else if constexpr (XCOL) {
                // piece p of the tile: vector v fastest, then the piece of the line's 16 rows, then the line
                constexpr int XE = (int)(16 / sizeof(HT));    // consecutive X rows of one vector per 16-byte piece
                constexpr int PPL = BS * (16 / XE);
                typedef HT xpiece_t __attribute__((ext_vector_type(XE)));
                for (int p = threadIdx.x; p < nl * PPL; p += blockDim.x) {
                    const int k = p / PPL, w = p - k * PPL;
                    const int v = w % BS, r0 = (w / BS) * XE;
                    const long xrow = (long)tile_lines[lp0 + k] * 16 + r0;
                    const HT *xp = X + xrow + (long)(v0 + v) * ld;
                    xpiece_t t;
                    if (xrow + XE <= x_rows) t = *(const xpiece_t *)xp;
                    else {
#pragma unroll
                        for (int e = 0; e < XE; ++e) t[e] = xrow + e < x_rows ? xp[e] : (HT)0;
                    }
                    HT *dst = xs + ((long)k * 16 + r0) * BS + v;
#pragma unroll
                    for (int e = 0; e < XE; ++e) dst[e * BS] = t[e];
                }
            } else {
                constexpr int PPL = 16 * R::NP;
                for (int p = threadIdx.x; p < nl * PPL; p += blockDim.x) {     // piece p of the tile: LDS position = p
                    const int k = p / PPL, w = p - k * PPL;
                    const long xrow = (long)tile_lines[lp0 + k] * 16 + w / R::NP;
                    piece_t t = (piece_t)(HT)0;
                    if (xrow < x_rows) t = *(const piece_t *)(X + xrow * B + v0 + R::PE * (w % R::NP));
                    *(piece_t *)(xs + (long)p * R::PE) = t;
                }
            }
            __syncthreads();
            if (L[0] > 0)
                tlc_block_chain<BS, NT, W>((const HT *)P.va[0] + (long)cs[0] + i, (const unsigned long long *)(P.c16[0] + q0[0]) + i, L[0], C, xs, s);
            if constexpr (MID) {
                if (L[1] > 0)
                    tlc_block_chain<BS, NT, W>((const float *)P.va[1] + (long)cs[1] + i, (const unsigned long long *)(P.c16[1] + q0[1]) + i, L[1], C,
                                                  xs, q);
#pragma unroll
                for (int v = 0; v < BS; ++v) { s[v] = s[v] + q[v]; q[v] = 0.0; }
            }
            if (L[2] > 0)
                tlc_block_chain<BS, NT, W>((const LT *)P.va[2] + (long)cs[2] + i, (const unsigned long long *)(P.c16[2] + q0[2]) + i, L[2], C, xs, q);
        } else {  // wide-footprint tile: 32-bit columns, global gathers
            const HT *Xv = XCOL ? X + (long)v0 * ld : X + v0;
            const long xstride = XCOL ? ld : (long)B;
            gather_block_chain<BS, NT, XCOL>((const HT *)P.va[0] + (long)cs[0] + i, P.ci[0] + (long)cs[0] + i, L[0], C, Xv, xstride, s);
            if constexpr (MID) {
                gather_block_chain<BS, NT, XCOL>((const float *)P.va[1] + (long)cs[1] + i, P.ci[1] + (long)cs[1] + i, L[1], C, Xv, xstride, q);
#pragma unroll
                for (int v = 0; v < BS; ++v) { s[v] = s[v] + q[v]; q[v] = 0.0; }
            }
            gather_block_chain<BS, NT, XCOL>((const LT *)P.va[2] + (long)cs[2] + i, P.ci[2] + (long)cs[2] + i, L[2], C, Xv, xstride, q);
        }
        if (valid) {
            if constexpr (YCOL) {
#pragma unroll
                for (int v = 0; v < BS; ++v) st_y<NT>(Y + (row + (long)(v0 + v) * ld), ap_hp_fold_y<HT>(s[v], q[v]));
            } else {
                piece_t *yp = (piece_t *)(Y + row * B + v0);
#pragma unroll
                for (int k = 0; k < R::NP; ++k) {
                    piece_t t;
#pragma unroll
                    for (int e = 0; e < R::PE; ++e) t[e] = ap_hp_fold_y<HT>(s[k * R::PE + e], q[k * R::PE + e]);
                    st_y<NT && !PAIR>(yp + k, t);     // (ap[dp_sp] keeps the plain row-major store it was measured with)
                }
            }
        }
    }
}

// ids: the chunks to run (n_ids of them), or nullptr for all; tile_rows > 0: ids are tiles of that many rows
template <int VB, typename HT, bool MID, typename LT>
void launch_ap_vb(const uspmv_dmat *hi, const ApHpParts &P, const HT *X, HT *Y, int b, long ld, int layout, hipStream_t st, const int *ids,
                  long n_ids, int tile_rows) {
    const int block = g_tune.block;
    const long n_chunks = ids ? n_ids : (long)hi->n_chunks;
    const unsigned grid = grid_for(n_chunks * (ids && tile_rows > 0 ? (long)tile_rows : (long)hi->C), block);
    const bool nt = g_tune.nontemporal != 0;
#define APV_LAUNCH_I(RW, NTV, IDSV)                                                                                                       \
    hipLaunchKernelGGL((scs_spmmv_ap_rows<VB, RW, NTV, HT, MID, LT, IDSV>), dim3(grid), dim3(block), 0, st, n_chunks, (int)hi->C, P, X, Y, b, \
                       ld, g_tune.xcd_remap, ids, tile_rows, (long)hi->n_chunks)
#define APV_LAUNCH(RW, NTV)                                                                                                               \
    do {                                                                                                                                  \
        if (!ids) APV_LAUNCH_I(RW, NTV, 0);                                                                                               \
        else if (tile_rows <= 0) APV_LAUNCH_I(RW, NTV, 1);                                                                                \
        else APV_LAUNCH_I(RW, NTV, 2);                                                                                                    \
    } while (0)
    if (layout == USPMV_ROWWISE) { if (nt) APV_LAUNCH(true, true); else APV_LAUNCH(true, false); }
    else { if (nt) APV_LAUNCH(false, true); else APV_LAUNCH(false, false); }
#undef APV_LAUNCH
#undef APV_LAUNCH_I
}

// <XCOL, YCOL>: the kinds with an fp16 part stage X and store Y in the caller's layout; ap[dp_sp] always reads row-major X (column-major
// callers arrive through the re-layout workspace) and stores Y either way -- except over a tile list (ids), where it too stages X straight
// from the caller's columns: a part of a distributed step has no whole X to re-lay out.  Over a list the fp16 kinds take every ld: columns
// that do not start on 16-byte boundaries are staged in 8- or 4-byte pieces (xpiece)
template <int B, int BS, typename HT, bool MID, typename LT>
void launch_ap_tlc_bs(const uspmv_dmat *hi, const ApHpParts &P, const HT *X, HT *Y, long ld, bool ycol, hipStream_t st, const int *ids, long n_ids) {
    constexpr bool PAIR = std::is_same<LT, float>::value;
    const size_t lds = (size_t)hi->tlc.max_lines * 16 * sizeof(HT) * BS;     // (what the fullest tile lists, not the budget)
    const int C = (int)hi->C;
    const unsigned grid = ids ? (unsigned)n_ids : (unsigned)hi->tlc.n_tiles;
    const long x_rows = ids && ycol ? std::min<long>((long)hi->tlc.x_len, ld) : (long)hi->tlc.x_len;
    const size_t col_bytes = (size_t)ld * sizeof(HT);
    const int xpiece = !(ids && ycol) || PAIR || col_bytes % 16 == 0 ? 16 : col_bytes % 8 == 0 ? 8 : 4;
#define APT_LAUNCH(CTV, NTV, XC, YC, IDSV)                                                                                           \
    do {                                                                                                                             \
        auto kfn = scs_spmmv_ap_tlc<B, BS, CTV, NTV, HT, MID, LT, XC, YC, IDSV>;                                                     \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);     \
        hipLaunchKernelGGL(kfn, dim3(grid), dim3(hi->tlc.tile_rows), lds, st, (long)hi->n_chunks, C, P, X, Y, ld,                    \
                           hi->tlc.line_ptr.get(), hi->tlc.lines.get(), x_rows, g_tune.xcd_remap, ids, xpiece);                      \
    } while (0)
#define APT_NT(CTV, NTV)                                                                                                             \
    do {                                                                                                                             \
        if (ids) { if (ycol) APT_LAUNCH(CTV, NTV, true, true, true); else APT_LAUNCH(CTV, NTV, false, false, true); }                \
        else if (!ycol) APT_LAUNCH(CTV, NTV, false, false, false);                                                                   \
        else if constexpr (PAIR) APT_LAUNCH(CTV, NTV, false, true, false);                                                           \
        else APT_LAUNCH(CTV, NTV, true, true, false);                                                                                \
    } while (0)
    if (g_tune.nontemporal) { if (C == 32) APT_NT(32, true); else APT_NT(0, true); }
    else { if (C == 32) APT_NT(32, false); else APT_NT(0, false); }
#undef APT_NT
#undef APT_LAUNCH
}

template <int B, typename HT, bool MID, typename LT>
void launch_ap_tlc(const uspmv_dmat *hi, const ApHpParts &P, const HT *X, HT *Y, long ld, bool ycol, int bs, hipStream_t st, const int *ids,
                   long n_ids) {
    if constexpr (B >= 8) { if (bs == 8) { launch_ap_tlc_bs<B, 8, HT, MID, LT>(hi, P, X, Y, ld, ycol, st, ids, n_ids); return; } }
    if constexpr (B >= 4) { if (bs == 4) { launch_ap_tlc_bs<B, 4, HT, MID, LT>(hi, P, X, Y, ld, ycol, st, ids, n_ids); return; } }
    launch_ap_tlc_bs<B, 2, HT, MID, LT>(hi, P, X, Y, ld, ycol, st, ids, n_ids);
}

// The kind of a split from its handles, handed to f as tags: HT(), whether there is a mid part, LT().
template <typename F>
void ap_kind(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *last, F &&f) {
    if (last->dtype == USPMV_F32) f(double(), std::false_type(), float());                     // ap[dp_sp]
    else if (hi->dtype == USPMV_F32) f(float(), std::false_type(), (unsigned short)0);         // ap[sp_hp]
    else if (mid) f(double(), std::true_type(), (unsigned short)0);                            // ap[dp_sp_hp]
    else f(double(), std::false_type(), (unsigned short)0);                                    // ap[dp_hp]
}

// What uspmv_spmmv_ap_hp runs for b >= 2: the ONE predicate behind the launch and behind uspmv_spmmv_ap_hp_path.  The codes are
// uspmv_spmmv_ap_path's: 0 the generic lane-per-row kernel, 2 the staged kernel, 3 the column-window sweep kernel (bs: the vectors per
// pass of the staged / sweep kernel, else 0); 1 has no hp kernel.
// The sweep kernel (ap_hp_spmmv_sweep.hip) takes parts that carry one shared sweep plan -- spmv_ap_hp_path's test -- under "sweep" 1
// wherever the plan's window leaves room for two vectors in LDS (spmmv_ap_hp_sweep_vectors) and the threads / rows-per-lane shape is
// one it serves, in one pass or several.
enum { AP_HP_PATH_GENERIC = 0, AP_HP_PATH_STAGED = 2, AP_HP_PATH_SWEEP = 3 };
struct ApHpBlockPath { int path, bs; };

ApHpBlockPath ap_hp_block_path(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, int b, long ld, int layout, bool aligned16) {
    const size_t x_bytes = hi->dtype == USPMV_F32 ? 4 : 8;
    if (g_tune.spmmv_variant == 1 || !aligned16 || (b != 2 && b != 4 && b != 8 && b != 16)) return {AP_HP_PATH_GENERIC, 0};
    if (layout != USPMV_ROWWISE && ((size_t)ld * x_bytes) % 16 != 0) return {AP_HP_PATH_GENERIC, 0};   // (16-byte pieces of the columns)
    if (hi->sw.on) {
        const uint64_t sid = hi->sw.plan_id;
        const bool shared = hi->sw.tile_ids && hi->sw.n_parts == (mid ? 3 : 2) && hp->sw.on && hp->sw.plan_id == sid &&
                            (!mid || (mid->sw.on && mid->sw.plan_id == sid));
        if (!shared || !g_tune.sweep) return {AP_HP_PATH_GENERIC, 0};
        const int bs = spmmv_ap_hp_sweep_bs(hi, b);
        if (bs < 2) return {AP_HP_PATH_GENERIC, 0};          // not even two vectors of a window fit LDS (the planner's default window)
        return {AP_HP_PATH_SWEEP, bs};
    }
    const uint64_t id = hi->tlc.plan_id;
    const bool planned = hi->tlc.on && id != 0 && hp->tlc.on && hp->tlc.plan_id == id && (!mid || (mid->tlc.on && mid->tlc.plan_id == id));
    if (!planned || !g_tune.tlc || hi->tlc.elem || hi->tlc.max_lines < 1) return {AP_HP_PATH_GENERIC, 0};   // (a plan over single x elements: not for block vectors)
    const int bs = tlc_block_bs(hi->tlc, b, x_bytes);
    if (bs < 2) return {AP_HP_PATH_GENERIC, 0};              // not even two vectors of the fullest tile fit LDS
    return {AP_HP_PATH_STAGED, bs};
}

// What uspmv_spmmv_ap_hp_tiles runs: the ONE predicate behind the launch and behind uspmv_spmmv_ap_hp_tiles_path.  The staged kernel over
// the listed tiles -- X staged straight from the caller's layout; column-major X at every ld, in pieces of 16, 8 or 4 bytes -- or lane
// per row over the tiles' rows: any other width or alignment of X / Y, "tlc" 0, "spmmv_variant" 1, a plan over single x elements, or a
// plan whose fullest tile leaves no room for two vectors in LDS.  (The caller has checked that the parts share a line plan.)
ApHpBlockPath ap_hp_tiles_path(const uspmv_dmat *hi, int b, bool aligned16) {
    if (g_tune.spmmv_variant == 1 || !aligned16 || (b != 2 && b != 4 && b != 8 && b != 16)) return {AP_HP_PATH_GENERIC, 0};
    if (!g_tune.tlc || hi->tlc.elem || hi->tlc.max_lines < 1) return {AP_HP_PATH_GENERIC, 0};
    const int bs = tlc_block_bs(hi->tlc, b, hi->dtype == USPMV_F32 ? 4 : 8);
    if (bs < 2) return {AP_HP_PATH_GENERIC, 0};
    return {AP_HP_PATH_STAGED, bs};
}

}  // namespace

namespace uspmv_dev {

// two vectors of the fullest tile's X rows (16 per line) in LDS: the staged kernel then takes a shared plan at every specialised width
int spmmv_ap_hp_plan_lines(int b, int x_dtype) {
    const size_t xb = x_dtype == USPMV_F32 ? 4 : 8;
    return (b == 2 || b == 4 || b == 8 || b == 16) ? (int)(WG_LDS_BYTES / (16 * 2 * xb)) : 0;
}

void spmmv_ap_hp_path(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, int b, long ld, int layout, int *path, int *vectors) {
    if (b == 1) {       // uspmv_spmv_ap_hp's own choice, one vector per pass
        *path = spmv_ap_hp_path(hi, mid, hp, true);
        *vectors = *path ? 1 : 0;
        return;
    }
    const ApHpBlockPath p = ap_hp_block_path(hi, mid, hp, b, ld, layout, true);
    *path = p.path; *vectors = p.bs;
}

int launch_spmmv_ap_rows(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *last, const int *chunk_ids, long n_ids, const void *X,
                         void *Y, int b, long ld, int layout, hipStream_t st, int tile_rows) {
    const ApHpParts P = ap_hp_parts(hi, mid, last);
    ap_kind(hi, mid, last, [&](auto ht, auto m, auto lt) {      // VB vectors per pass
        typedef decltype(ht) HT; typedef decltype(lt) LT;
        constexpr bool MID = decltype(m)::value;
        if (b <= 2) launch_ap_vb<2, HT, MID, LT>(hi, P, (const HT *)X, (HT *)Y, b, ld, layout, st, chunk_ids, n_ids, tile_rows);
        else if (b <= 4) launch_ap_vb<4, HT, MID, LT>(hi, P, (const HT *)X, (HT *)Y, b, ld, layout, st, chunk_ids, n_ids, tile_rows);
        else launch_ap_vb<8, HT, MID, LT>(hi, P, (const HT *)X, (HT *)Y, b, ld, layout, st, chunk_ids, n_ids, tile_rows);
    });
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_spmmv_ap_staged(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *last, const void *X, void *Y, int b, long ld, bool ycol,
                           int bs, hipStream_t st, const int *tile_ids, long n_ids) {
    const ApHpParts P = ap_hp_parts(hi, mid, last);
    ap_kind(hi, mid, last, [&](auto ht, auto m, auto lt) {
        typedef decltype(ht) HT; typedef decltype(lt) LT;
        constexpr bool MID = decltype(m)::value;
        switch (b) {
            case 2: launch_ap_tlc<2, HT, MID, LT>(hi, P, (const HT *)X, (HT *)Y, ld, ycol, bs, st, tile_ids, n_ids); break;
            case 4: launch_ap_tlc<4, HT, MID, LT>(hi, P, (const HT *)X, (HT *)Y, ld, ycol, bs, st, tile_ids, n_ids); break;
            case 8: launch_ap_tlc<8, HT, MID, LT>(hi, P, (const HT *)X, (HT *)Y, ld, ycol, bs, st, tile_ids, n_ids); break;
            default: launch_ap_tlc<16, HT, MID, LT>(hi, P, (const HT *)X, (HT *)Y, ld, ycol, bs, st, tile_ids, n_ids); break;
        }
    });
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int launch_spmmv_ap_hp_chunks(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *chunk_ids, long n_ids,
                              const void *X, void *Y, int b, long ld, int layout, hipStream_t st) {
    if (n_ids == 0) return USPMV_OK;
    return launch_spmmv_ap_rows(hi, mid, hp, chunk_ids, n_ids, X, Y, b, ld, layout, st);
}

void spmmv_ap_hp_tiles_path(const uspmv_dmat *hi, int b, int *path, int *vectors) {
    const ApHpBlockPath p = ap_hp_tiles_path(hi, b, true);
    *path = p.path; *vectors = p.bs;
}

int launch_spmmv_ap_hp_tiles(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const int *tile_ids, long n_ids, const void *X,
                             void *Y, int b, long ld, int layout, hipStream_t st) {
    if (n_ids == 0) return USPMV_OK;
    const ApHpBlockPath p = ap_hp_tiles_path(hi, b, ((uintptr_t)X % 16 == 0) && ((uintptr_t)Y % 16 == 0));
    if (p.path == AP_HP_PATH_STAGED) return launch_spmmv_ap_staged(hi, mid, hp, X, Y, b, ld, layout != USPMV_ROWWISE, p.bs, st, tile_ids, n_ids);
    return launch_spmmv_ap_rows(hi, mid, hp, tile_ids, n_ids, X, Y, b, ld, layout, st, hi->tlc.tile_rows);
}

int launch_spmmv_ap_hp(const uspmv_dmat *hi, const uspmv_dmat *mid, const uspmv_dmat *hp, const void *X, void *Y, int b, long ld, int layout,
                       hipStream_t st) {
    if (hi->n_chunks == 0) return USPMV_OK;
    if (b == 1) return launch_spmv_ap_hp(hi, mid, hp, X, Y, st);
    const bool col = layout != USPMV_ROWWISE;
    const ApHpBlockPath p = ap_hp_block_path(hi, mid, hp, b, ld, layout, ((uintptr_t)X % 16 == 0) && ((uintptr_t)Y % 16 == 0));
    if (p.path == AP_HP_PATH_SWEEP) return launch_spmmv_ap_hp_sweep(hi, mid, hp, X, Y, b, ld, col, p.bs, st);
    if (p.path == AP_HP_PATH_STAGED) return launch_spmmv_ap_staged(hi, mid, hp, X, Y, b, ld, col, p.bs, st);
    return launch_spmmv_ap_rows(hi, mid, hp, nullptr, 0, X, Y, b, ld, layout, st);
}

}  // namespace uspmv_dev
