// Distributed SpMV step on RCCL (xGMI), in C++ behind the C ABI (include/uspmv.h, sections L4a / L4b).
//
// Replaces the per-iteration part of the reference's MPI flow for the single-vector one-precision path:
//   init_local_structs            code/main.cpp:1075-1334      (partition block -> SELL-C-sigma, halo discovery)
//   collect_comm_info             code/mpi_funcs.hpp:1061-1124 (who sends what to whom)
//   init/finalize_halo_exchange   code/classes_structs.hpp:857-995
//   the iteration of bench_spmv   code/main.cpp:458-474        (exchange, then kernel, then the -ba_synch barrier)
// One process per GPU.  Per SpMV: ONE pack kernel over the concatenated send list, ONE grouped ncclSend/ncclRecv with every
// receive landing directly in x[n_local + recv_cumsum[p]] (the reference's halo numbering) on a side stream, the tiles /
// chunks that touch no halo column meanwhile on the caller's stream, the boundary ones after the exchange.  The whole step
// (two streams, two events, three kernels, the RCCL group, the optional barrier) can be captured once into a hipGraph and
// replayed: per step the host then pays one hipGraphLaunch instead of ~12 runtime calls (the strong-scaling regime of
// BASELINE config 5, where a rank's kernel takes < 0.2 ms).
//
// Set-up ("who sends what to whom") runs over a uspmv_transport (host/comm_plan.cpp): RCCL with device staging by default,
// the host communicator when the caller passes one (real processes on a CPU box test exactly this code), identity in loopback.
//
// Loopback (comm_size == 1 and P > 1): this process plays logical rank `rank` of a P-way partition and every neighbour is
// itself -- sends and receives become RCCL self send/recv pairs of the ids it asked for.  With an x that repeats with the
// block height this reproduces the true multi-rank result for the rank's rows; it is how a single-GPU box exercises the
// RCCL calls end to end (tests/test_dist_native_gpu.py).  It needs equal block heights (seg-rows on a divisible size): the
// ids a rank asks block p for index p's rows, and the set-up refuses ids outside this block.
// USPMV_EXCHANGE_HOST: the per-step exchange staged through host memory over the transport -- P real processes may then share
// ONE GPU, which is how the step runs with unequal seg-nnz blocks and asymmetric lists on a single-GPU box.
// USPMV_EXCHANGE_PEER: every rank owns a receive window (hipMalloc, exported by hipIpcGetMemHandle) and one push kernel stores its
// halo contributions straight into the neighbours' windows; completion is host-ordered (event, transport barrier), then an unpack
// kernel copies the window into the tail of x.  No communication kernel, no host copy of the data (see push, peer_complete).
//
// Round 3 additions in this file: optional arrangements of the step around the exchange ("pad_split": tiles that touch the halo only
// through the reference's padding run before the exchange under a sign / finiteness guard; "fused_step": one launch whose boundary
// tiles look once at an exchange counter and defer themselves otherwise), uspmv_dist_autotune (times the arrangements collectively and
// keeps the fastest, self-checked), the block-vector step in two parts over marked chunk-length arrays (uspmv_dist_spmmv, also with
// the phased block plan built on the rank's matrix), the block exchange staged through the host for real ranks on one GPU.
//
// Adaptive precision ap[dp_sp] (uspmv_dist_create_ap_from_coo; the reference refuses ap with MPI, code/utilities.hpp:1445-1451): the object
// carries the sp part as a second handle.  One halo for the pair, tile classes from both parts, "pad_split" on by default; the single-vector
// step and, for block vectors, uspmv_dist_spmmv_ap: the same lists run by the list forms of the pair's block kernels
// (uspmv_spmmv_ap_tiles / _chunks), the padding guard over the b values of the slot.
//
// The kinds with an fp16 part, ap[dp_hp], ap[sp_hp], ap[dp_sp_hp] (uspmv_dist_create_ap_hp_from_coo): A / scs are the hi part, the
// object carries the hp part and, for ap[dp_sp_hp], the mid part beside it.  One halo for all parts, tile classes from all of them, the
// single-vector step in the vector type of the hi part (float for ap[sp_hp]); block vectors through uspmv_dist_spmmv_ap_hp: the step of
// uspmv_dist_spmmv_ap over the list forms of these kinds' block kernels (uspmv_spmmv_ap_hp_tiles / _chunks), guard in that type.
#include <rccl/rccl.h>

#include <chrono>
#include <string>

#include "uspmv_device.hpp"

struct uspmv_dist {
    int rank = 0, P = 1, comm_rank = 0, comm_size = 1;
    int exchange = USPMV_EXCHANGE_RCCL;   // the per-step exchange (uspmv_exchange; USPMV_EXCHANGE_PEER: see "peer-store exchange" below)
    bool loopback = false, overlap = true, tiles = false, owns_setup = false, no_pack = false, ba_synch = false;
    bool diag_skip_exchange = false;
    bool autotune_all = false;        // uspmv_dist_autotune also times the speculative arrangements (pad, fused); off: overlap | plain only
    int diag_spmmv_part = 0;          // diagnosis: the two-part block-vector step runs only its interior (1) or boundary (2) part
    int capture_mode = hipStreamCaptureModeRelaxed;
    ncclComm_t comm = nullptr;
    uspmv_transport_t tr{};           // set-up transport (and the per-step one of USPMV_EXCHANGE_HOST)
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_main = nullptr, ev_comm = nullptr;
    // The rank's matrix: one precision, or an adaptive-precision split of kind USPMV_AP_DP_SP | _DP_HP | _SP_HP | _DP_SP_HP (uspmv.h).  Its parts
    // by slot: pt[0] the hi part (the vectors have its type -- F32 for ap[sp_hp], else F64 -- so pack, exchange, guard, barrier and capture are
    // the one-precision object's; only part() and the whole-matrix launch differ), pt[1] the float part below it (sp of ap[dp_sp], mid of
    // ap[dp_sp_hp]), pt[2] the fp16 part.  A slot the kind does not have is NULL; n_pt counts the others.  The handles and structs (and the
    // halo) are owned when a _from_coo creator built them (owns_setup); uspmv_dist_create lends A and leaves scs NULL.
    enum { ONE_PRECISION = -1 };
    struct Part { uspmv_dmat_t *A = nullptr; uspmv_scs_t *scs = nullptr; };
    int kind = ONE_PRECISION;
    Part pt[3];
    int n_pt = 1;
    uspmv_dmat_t *&A = pt[0].A;       // (the names most of the step knows the hi part by)
    uspmv_scs_t *&scs = pt[0].scs;
    double ap_threshold = 0.0, ap_threshold_2 = 0.0;   // the split's thresholds (uspmv_partition_precisions / _hp), for the self-check's reference
    uspmv_halo_t *halo = nullptr;
    uspmv_comm_plan_t *plan = nullptr;
    int dtype = USPMV_F64;
    int64_t n_local = 0, n_halo = 0, n_send = 0, n_int = 0, n_bnd = 0, vec_len = 0, n_rows_padded = 0;
    std::vector<int64_t> send_off, recv_off;
    std::vector<int32_t> recv_counts;
    DeviceBuf<int32_t> d_send_idxs, d_perm, d_int, d_bnd;
    DeviceBuf<int32_t> d_src;         // send[i] = x[d_src[i]], d_src = perm[send_idxs] composed once: the pack of every b = 1 plan, the push
    // Padding tiles (tile lists only).  The reference pads chunks with (value +0, column 0); on ranks > 0 column 0 is a halo column
    // (code/mpi_funcs.hpp:279-306), so more than half of a rank's tiles "touch the halo" only through fma(+0, x[pad_col], acc).  Those
    // run with the interior tiles, before the exchange has delivered x[pad_col]: for a finite operand of the same sign the product is
    // the same signed zero and every row's chain comes out bit for bit as with the delivered value.  The step keeps the value the
    // slot held before the exchange, compares it with the delivered one (pad_guard_kernel), and only when either is not finite or the
    // signs differ runs the padding tiles AGAIN after the boundary tiles (a conditional tile list: ids or -1).
    // d_early = interior and padding tiles in ascending order (ONE launch before the exchange completes); d_late = the boundary tiles
    // with real halo references followed by n_pad conditional entries (ONE launch after it): the guard writes ids or -1 there
    DeviceBuf<int32_t> d_early, d_late, d_pad;
    // ONE-launch step ("fused_step" 1, the default with tile lists): d_step = [early | real boundary | padding again (conditional)] in one
    // launch on the side stream; late entries that find the exchange unfinished defer themselves to a second, small launch behind it
    // (uspmv_dev::StepSync -- nothing spins).  Saves the second launch's ramp-up and the join in the common case.
    DeviceBuf<int32_t> d_step, d_defer;
    DeviceBuf<uspmv_dev::StepSync> d_ss;
    uspmv_dev::StepArgs sa;
    bool fused = false, sync_dirty = false, capturing = false;   // (off by default: 0.222 against 0.209 ms, same file)
    int64_t n_bnd_real = 0, n_pad = 0;
    int32_t pad_col = -1;
    bool pad_split = false;           // (off by default: on one GPU it measures 0.221 against 0.209 ms per step, profiles/r03/dist_step_ab.txt)
    DeviceBuf<void> d_stale;
    DeviceBuf<double> d_stale_b;      // the block step of an ap object (uspmv_dist_spmmv_ap / _ap_hp): the slot's b values in the vector type,
                                      // 8 bytes each whatever that type is, grown to b at first use
    int stale_b = 0;
    // peer-store exchange: this rank's receive window = two halves (step parity) of win_half elements, sized for block vectors of up to
    // win_b columns; the windows of the ranks it sends to, opened through IPC (nullptr: not opened; loopback opens nothing); the push
    // table (per neighbour q: q's window, its half size, where this rank's block starts in it) and the send offsets it is indexed by
    DeviceBuf<void> d_win;
    int64_t win_half = 0;
    int win_b = 0, parity = 0;
    std::vector<void *> peer_win;
    DeviceBuf<void> d_push;
    DeviceBuf<int64_t> d_seg;
    hipEvent_t ev_push = nullptr, ev_unpack = nullptr;
    bool unpack_queued = false;       // ev_unpack marks the last unpack (see peer_complete)
    bool diag_peer_skew = false;      // test only: the next window set-up announces one element too many (see peer_setup)
    DeviceBuf<int> d_scratch;
    // captured step
    hipGraphExec_t gexec = nullptr;
    void *g_x = nullptr, *g_y = nullptr;
    hipStream_t g_stream = nullptr;
    bool graph_failed = false;
    int64_t graph_launches = 0, eager_steps = 0;
    // exchange plans of RCCL and USPMV_EXCHANGE_HOST, one per (b, layout, mode) used so far; the single-vector step's
    // (1, USPMV_ROWWISE, USPMV_BULKVEC) is built with the object
    struct BlockPlan {
        int b = 0, layout = 0, mode = 0;
        DeviceBuf<int32_t> d_src;                    // wire order of the send buffer: send[i] = X[d_src[i]] (b = 1: uspmv_dist::d_src)
        std::vector<DeviceBuf<int32_t>> d_unpack;    // staged receive (bulk, column-wise): per vector, halo slot -> position in d_recv
        DeviceBuf<void> d_send, d_recv;
        PinnedBuf h_send, h_recv;                    // pinned staging of USPMV_EXCHANGE_HOST
    };
    std::vector<BlockPlan> block_plans;
    std::vector<int32_t> h_send_idxs, h_perm;        // host copies for building those plans
    // two-part SpMMV (interior chunks while the block-vector exchange runs): see uspmv_dmat::part_len
    bool parts = false;                              // the handle carries the caller's-order arrays
    int64_t plan_b = 0, plan_bnd_tiles = 0;          // block width of the phased plan built through "block_plan", its boundary tiles
    int64_t spmmv_two_part = 0, spmmv_one_part = 0;  // steps taken in either form
};

namespace {

#define NCCL_TRY(call)                                                                                           \
    do {                                                                                                         \
        ncclResult_t r_ = (call);                                                                                \
        if (r_ != ncclSuccess) return uspmv::fail(USPMV_ERR_HIP, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

inline int peer(const uspmv_dist *D, int p) { return D->loopback ? 0 : p; }
inline ncclDataType_t nccl_vt(const uspmv_dist *D) { return D->dtype == USPMV_F64 ? ncclDouble : ncclFloat; }
inline size_t vsize(const uspmv_dist *D) { return D->dtype == USPMV_F64 ? 8 : 4; }

// ---- set-up transports that live in this file: RCCL with device staging, identity for loopback
int rccl_alltoallv(void *ctx, const void *send, const int64_t *so, void *recv, const int64_t *ro) {
    auto *D = (uspmv_dist *)ctx;
    const int P = D->comm_size;
    const int64_t sb = so[P] - so[0], rb = ro[P] - ro[0];
    DeviceBuf<char> ds, dr;
    HIP_TRY(ds.alloc((size_t)sb));
    HIP_TRY(dr.alloc((size_t)rb));
    if (sb) HIP_TRY(hipMemcpy(ds, (const char *)send + so[0], (size_t)sb, hipMemcpyHostToDevice));
    hipStream_t st = D->side_stream;
    NCCL_TRY(ncclGroupStart());
    for (int q = 0; q < P; ++q) {
        const int64_t ns = so[q + 1] - so[q], nr = ro[q + 1] - ro[q];
        if (nr) NCCL_TRY(ncclRecv((char *)dr + (ro[q] - ro[0]), (size_t)nr, ncclInt8, q, D->comm, st));
        if (ns) NCCL_TRY(ncclSend((const char *)ds + (so[q] - so[0]), (size_t)ns, ncclInt8, q, D->comm, st));
    }
    NCCL_TRY(ncclGroupEnd());
    HIP_TRY(hipStreamSynchronize(st));
    if (rb) HIP_TRY(hipMemcpy((char *)recv + ro[0], dr, (size_t)rb, hipMemcpyDeviceToHost));
    return USPMV_OK;
}
int rccl_allgather(void *ctx, const void *send, void *recv, int64_t bytes) {
    auto *D = (uspmv_dist *)ctx;
    if (bytes == 0) return USPMV_OK;
    DeviceBuf<char> ds, dr;
    HIP_TRY(ds.alloc((size_t)bytes));
    HIP_TRY(dr.alloc((size_t)bytes * (size_t)D->comm_size));
    HIP_TRY(hipMemcpy(ds, send, (size_t)bytes, hipMemcpyHostToDevice));
    NCCL_TRY(ncclAllGather(ds, dr, (size_t)bytes, ncclInt8, D->comm, D->side_stream));
    HIP_TRY(hipStreamSynchronize(D->side_stream));
    HIP_TRY(hipMemcpy(recv, dr, (size_t)bytes * (size_t)D->comm_size, hipMemcpyDeviceToHost));
    return USPMV_OK;
}
int rccl_barrier(void *ctx) {
    auto *D = (uspmv_dist *)ctx;
    NCCL_TRY(ncclAllReduce(D->d_scratch, D->d_scratch, 1, ncclInt32, ncclSum, D->comm, D->side_stream));
    HIP_TRY(hipStreamSynchronize(D->side_stream));
    return USPMV_OK;
}
// loopback: "rank p needs from me" := what I asked p for -- every exchange is the identity on this process
int self_alltoallv(void *ctx, const void *send, const int64_t *so, void *recv, const int64_t *ro) {
    const int P = ((uspmv_dist *)ctx)->P;
    for (int q = 0; q < P; ++q) {
        if (so[q + 1] - so[q] != ro[q + 1] - ro[q]) return uspmv::fail(USPMV_ERR_INVALID, "loopback all-to-all-v: segment lengths differ");
        if (so[q + 1] > so[q]) memmove((char *)recv + ro[q], (const char *)send + so[q], (size_t)(so[q + 1] - so[q]));
    }
    return USPMV_OK;
}
int self_allgather(void *ctx, const void *send, void *recv, int64_t bytes) {
    const int P = ((uspmv_dist *)ctx)->P;
    for (int q = 0; q < P; ++q) memcpy((char *)recv + (size_t)q * (size_t)bytes, send, (size_t)bytes);
    return USPMV_OK;
}
int self_barrier(void *) { return USPMV_OK; }

// ---- the per-step exchange
// pack_send_buf (code/mpi_funcs.hpp:25-33) with the two index levels composed at set-up; thread 0 also keeps the value the padding
// column's slot holds BEFORE the exchange overwrites it (see uspmv_dist::pad_col)
template <typename VT>
__global__ void pack_kernel(VT *__restrict__ out, const VT *__restrict__ x, const int *__restrict__ src, const long n, const int pad_col, VT *__restrict__ stale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x[src[i]];
    if (i == 0 && pad_col >= 0) *stale = x[pad_col];
}

// after the exchange: must the padding tiles run again?  (not when the slot held, and now holds, finite values of one sign:
// fma(+0, s, acc) == fma(+0, c, acc) bit for bit then)
template <typename VT>
__global__ void pad_guard_kernel(const VT *__restrict__ x, const int pad_col, const VT *__restrict__ stale, const int *__restrict__ pad_ids,
                                 int *__restrict__ rerun, const long n_pad, int *__restrict__ counter) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const VT s = *stale, c = x[pad_col];
    const bool need = !(isfinite(s) && isfinite(c) && (signbit(s) == signbit(c)));
    if (k < n_pad) rerun[k] = need ? pad_ids[k] : -1;
    if (k == 0 && need) atomicAdd(counter, 1);
}

// The block form of that pair for uspmv_dist_spmmv_ap / _ap_hp: the padding column's slot holds one value per vector -- X[pad_col + v*ld]
// column-wise, X[pad_col*b + v] row-wise.  Kept before the exchange; after it the padding tiles run again iff for ANY vector the kept
// or the delivered value is not finite or their signs differ (a tile computes all b columns, so one such column re-runs it).
template <typename VT>
__global__ void pad_keep_block_kernel(const VT *__restrict__ X, const int pad_col, const int b, const long ld, const int rowwise,
                                      VT *__restrict__ stale) {
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v < b) stale[v] = rowwise ? X[(long)pad_col * b + v] : X[pad_col + (long)v * ld];
}
template <typename VT>
__global__ void pad_guard_block_kernel(const VT *__restrict__ X, const int pad_col, const int b, const long ld, const int rowwise,
                                       const VT *__restrict__ stale, const int *__restrict__ pad_ids, int *__restrict__ rerun,
                                       const long n_pad, int *__restrict__ counter) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool need = false;
    for (int v = 0; v < b; ++v) {
        const VT s = stale[v], c = rowwise ? X[(long)pad_col * b + v] : X[pad_col + (long)v * ld];
        need = need || !(isfinite(s) && isfinite(c) && (signbit(s) == signbit(c)));
    }
    if (k < n_pad) rerun[k] = need ? pad_ids[k] : -1;
    if (k == 0 && need) atomicAdd(counter, 1);
}

__global__ void exchange_done_kernel(uspmv_dev::StepSync *ss) { __hip_atomic_store(&ss->flag, ss->flag + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }

int sync_reset(uspmv_dist *D) {
    if (!D->d_ss) return USPMV_OK;
    HIP_TRY(hipDeviceSynchronize());
    uspmv_dev::StepSync z{};
    z.expect = 1;
    HIP_TRY(hipMemcpy(D->d_ss, &z, sizeof z, hipMemcpyHostToDevice));
    D->sync_dirty = false;
    return USPMV_OK;
}

// an adaptive-precision object; one of a kind with an fp16 part
inline bool is_ap(const uspmv_dist *D) { return D->kind != uspmv_dist::ONE_PRECISION; }
inline bool has_hp(const uspmv_dist *D) { return is_ap(D) && D->kind != USPMV_AP_DP_SP; }
inline const char *ap_name(const uspmv_dist *D) {
    return D->kind == USPMV_AP_DP_SP ? "ap[dp_sp]" : D->kind == USPMV_AP_DP_HP ? "ap[dp_hp]" : D->kind == USPMV_AP_SP_HP ? "ap[sp_hp]" : "ap[dp_sp_hp]";
}

inline bool fused_on(const uspmv_dist *D) { return !is_ap(D) && D->fused && D->overlap && D->tiles && D->d_step && D->sa.n_real + D->sa.n_cond > 0; }

inline bool pads_on(const uspmv_dist *D) { return D->pad_split && D->overlap && D->tiles && D->n_pad > 0 && D->pad_col >= 0; }

// send[i] = X[src[i]] for i < n, and the padding column's value when pad_col >= 0
int pack(uspmv_dist *D, void *send, const void *d_X, const int32_t *src, long n, int pad_col, hipStream_t st) {
    if (n == 0 && pad_col < 0) return USPMV_OK;
    const unsigned grid = (unsigned)std::max<long>((n + 255) / 256, 1);
    if (D->dtype == USPMV_F64)
        hipLaunchKernelGGL(pack_kernel<double>, dim3(grid), dim3(256), 0, st, (double *)send, (const double *)d_X, src, n, pad_col, (double *)D->d_stale);
    else
        hipLaunchKernelGGL(pack_kernel<float>, dim3(grid), dim3(256), 0, st, (float *)send, (const float *)d_X, src, n, pad_col, (float *)D->d_stale);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int pad_guard(uspmv_dist *D, const void *d_x, hipStream_t st) {
    const unsigned grid = (unsigned)((D->n_pad + 255) / 256);
    if (D->dtype == USPMV_F64)
        hipLaunchKernelGGL(pad_guard_kernel<double>, dim3(grid), dim3(256), 0, st, (const double *)d_x, D->pad_col, (const double *)D->d_stale, D->d_pad, D->d_late + D->n_bnd_real,
                           (long)D->n_pad, D->d_scratch + 2);
    else
        hipLaunchKernelGGL(pad_guard_kernel<float>, dim3(grid), dim3(256), 0, st, (const float *)d_x, D->pad_col, (const float *)D->d_stale, D->d_pad, D->d_late + D->n_bnd_real,
                           (long)D->n_pad, D->d_scratch + 2);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

// the block forms of the guard's two halves, in the object's vector type (D->d_stale_b holds b values of it)
int pad_keep_block(uspmv_dist *D, const void *d_X, int b, long ld, int rowwise, hipStream_t st) {
    const dim3 grid((unsigned)((b + 63) / 64));
    if (D->dtype == USPMV_F64)
        hipLaunchKernelGGL(pad_keep_block_kernel<double>, grid, dim3(64), 0, st, (const double *)d_X, D->pad_col, b, ld, rowwise, D->d_stale_b.get());
    else
        hipLaunchKernelGGL(pad_keep_block_kernel<float>, grid, dim3(64), 0, st, (const float *)d_X, D->pad_col, b, ld, rowwise, (float *)D->d_stale_b.get());
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}
int pad_guard_block(uspmv_dist *D, const void *d_X, int b, long ld, int rowwise, hipStream_t st) {
    const dim3 grid((unsigned)((D->n_pad + 255) / 256));
    if (D->dtype == USPMV_F64)
        hipLaunchKernelGGL(pad_guard_block_kernel<double>, grid, dim3(256), 0, st, (const double *)d_X, D->pad_col, b, ld, rowwise,
                           (const double *)D->d_stale_b.get(), D->d_pad.get(), D->d_late + D->n_bnd_real, (long)D->n_pad, D->d_scratch + 2);
    else
        hipLaunchKernelGGL(pad_guard_block_kernel<float>, grid, dim3(256), 0, st, (const float *)d_X, D->pad_col, b, ld, rowwise,
                           (const float *)D->d_stale_b.get(), D->d_pad.get(), D->d_late + D->n_bnd_real, (long)D->n_pad, D->d_scratch + 2);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

// ---- USPMV_EXCHANGE_PEER: peer-store exchange
// Set-up (peer_setup, collective): every rank hipMallocs a window of 2 x win_half elements (win_half = n_halo x widest block seen so far)
// and exports it; one all-gather carries every rank's export status, handle, half size, send and receive offsets, so every rank
// validates EVERY pair (r's send count to q == q's receive count from r, the destination range inside q's window) on the same data and
// reaches the same verdict before any kernel runs; then each rank opens the windows of the ranks it sends to and a second all-gather
// agrees on the open status.  Sender r writes its send_off[q] .. send_off[q+1] elements to q's window at recv_off_q[r] + j.
// Loopback: the destination of every neighbour is this process's own window at its own recv_off[q] (what it asked q for), no IPC.
struct PeerDst {
    void *base;      // q's window (opened through IPC; this rank's own in loopback)
    int64_t half;    // elements per parity half of q's window
    int64_t off;     // first halo slot of this rank's block in q's numbering
};

// Stores another process reads once this kernel has completed: system scope (global_store ... sc0 sc1 on gfx950).  They are written
// through to memory and the line is dropped from this XCD's L2, so neither an L2 of this GPU that the owner's kernels do not flush nor
// a remote GPU's fabric path can hold the bytes back; the host waits for the kernel's completion before the barrier tells the owner.
// (Plain stores plus one system-scope release per workgroup would do too, but cost a full L2 write-back per workgroup.)
__device__ __forceinline__ void st_sys(double *p, double v) {
    __hip_atomic_store((unsigned long long *)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st_sys(float *p, float v) { __hip_atomic_store((unsigned *)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
// Loads of bytes another process wrote: system scope (global_load ... sc0 sc1), served from memory -- the half read here was read
// two steps ago as well, and this GPU's L1 / L2 may still hold those lines, which the writer's stores did not invalidate.
__device__ __forceinline__ double ld_sys(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
__device__ __forceinline__ float ld_sys(const float *p) { return __uint_as_float(__hip_atomic_load((const unsigned *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)); }

// One launch over the concatenated send list (all neighbours, all b vectors): thread t = element i = t / b of the list, vector v = t % b.
// The neighbour q is found by a binary search over the P + 1 send offsets (the largest q with seg[q] <= i: empty ranges are skipped).
// X column-wise (ld) or row-wise; single vector: b = 1, row-wise.  Window layout: halo slot k of vector v at k * b + v.  Thread 0 also
// keeps the padding column's value before the exchange overwrites it, as pack_kernel does (uspmv_dist::pad_col).
template <typename VT>
__global__ void push_kernel(const VT *__restrict__ x, const int *__restrict__ src, const int64_t *__restrict__ seg, const PeerDst *__restrict__ dst,
                            const int P, const long n, const int b, const long ld, const int rowwise, const int s, const int pad_col,
                            VT *__restrict__ stale) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0 && pad_col >= 0) *stale = x[pad_col];
    if (t >= n * b) return;
    const long i = t / b;
    const int v = (int)(t - i * b);
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const PeerDst d = dst[lo];
    const VT val = x[rowwise ? (long)src[i] * b + v : (long)src[i] + (long)v * ld];
    st_sys((VT *)d.base + (long)s * d.half + (d.off + (i - seg[lo])) * b + v, val);
}

// window half -> halo region of X: slot k of vector v to X[(n_local + k) * b + v] (row-wise; b = 1: the tail of x) or X[v * ld + n_local + k]
template <typename VT>
__global__ void unpack_kernel(VT *__restrict__ x, const VT *__restrict__ win, const long n_local, const long n, const int b, const long ld,
                              const int rowwise) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * b) return;
    const long k = t / b;
    const int v = (int)(t - k * b);
    x[rowwise ? n_local * b + t : (long)v * ld + n_local + k] = ld_sys(win + t);
}

int push(uspmv_dist *D, const void *d_x, int b, long ld, int rowwise, long n, int pad_col, hipStream_t st) {
    // (a window set-up that failed -- the growth in uspmv_dist_spmmv -- leaves the object without windows: refuse, never launch on them)
    if (!D->d_win || !D->d_push)
        return uspmv::fail(USPMV_ERR_INVALID, "USPMV_EXCHANGE_PEER: the receive windows were lost in a failed set-up; uspmv_dist_spmmv on every rank "
                           "sets them up again, or free the object");
    if (D->unpack_queued) HIP_TRY(hipStreamWaitEvent(st, D->ev_unpack, 0));   // this step's push (and the host's wait for it) after the last unpack
    if (n == 0 && pad_col < 0) return USPMV_OK;
    const unsigned grid = (unsigned)std::max<long>((n * b + 255) / 256, 1);
    const PeerDst *dst = (const PeerDst *)D->d_push.get();
    if (D->dtype == USPMV_F64)
        hipLaunchKernelGGL(push_kernel<double>, dim3(grid), dim3(256), 0, st, (const double *)d_x, D->d_src, D->d_seg, dst, D->P, n, b, ld, rowwise, D->parity,
                           pad_col, (double *)D->d_stale);
    else
        hipLaunchKernelGGL(push_kernel<float>, dim3(grid), dim3(256), 0, st, (const float *)d_x, D->d_src, D->d_seg, dst, D->P, n, b, ld, rowwise, D->parity,
                           pad_col, (float *)D->d_stale);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

// After the push of this step (parity s) has been queued on `st`: real ranks wait for it on the host and meet in the transport barrier
// (deadline: a dead peer fails every rank with USPMV_ERR_COMM), then every push into this rank's window[s] has completed; the unpack
// follows on the same stream.  Loopback: stream order alone puts the unpack behind the push.
// Why no rank overwrites a window half before its owner has unpacked it: rank r pushes into q's half s at step k and, next, at step
// k + 2, after barrier k + 1.  q reaches barrier k + 1 only after its host has waited for its push of step k + 1, which q queued behind
// its unpack of step k (same stream, or -- when the caller switches streams between steps -- behind ev_unpack, see push) -- so that
// unpack has completed before anyone leaves barrier k + 1.  The push of step k + 1 itself goes to the other half, which is what the
// second half is for: q's unpack of step k may still be queued then.
int peer_complete(uspmv_dist *D, void *d_X, int b, long ld, int rowwise, hipStream_t st) {
    const int s = D->parity;
    D->parity ^= 1;
    if (!D->loopback) {
        HIP_TRY(hipEventRecord(D->ev_push, st));
        HIP_TRY(hipEventSynchronize(D->ev_push));
        if (int rc = D->tr.barrier(D->tr.ctx)) return rc;
    }
    const long n = (long)D->n_halo;
    if (n == 0) return USPMV_OK;
    if (!D->d_win) return uspmv::fail(USPMV_ERR_INVALID, "USPMV_EXCHANGE_PEER: no receive window");
    const unsigned grid = (unsigned)((n * b + 255) / 256);
    const size_t woff = (size_t)s * (size_t)D->win_half;
    if (D->dtype == USPMV_F64)
        hipLaunchKernelGGL(unpack_kernel<double>, dim3(grid), dim3(256), 0, st, (double *)d_X, (const double *)D->d_win.get() + woff, (long)D->n_local, n, b, ld, rowwise);
    else
        hipLaunchKernelGGL(unpack_kernel<float>, dim3(grid), dim3(256), 0, st, (float *)d_X, (const float *)D->d_win.get() + woff, (long)D->n_local, n, b, ld, rowwise);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(D->ev_unpack, st));
    D->unpack_queued = true;
    return USPMV_OK;
}

// close what this rank opened, barrier (no rank frees a window another still has open: the HIP header calls freeing an exported region
// before the importer's hipIpcCloseMemHandle undefined), free the window.  A peer that is gone fails the barrier on its deadline: the
// window is freed anyway and the barrier's status returned.
int peer_release(uspmv_dist *D, bool barrier) {
    if (!D->d_win) return USPMV_OK;
    (void)hipDeviceSynchronize();                                    // no push or unpack of this process still touches a window
    for (void *&w : D->peer_win)
        if (w) { (void)hipIpcCloseMemHandle(w); w = nullptr; }
    int rc = USPMV_OK;
    if (barrier && !D->loopback && D->tr.barrier) rc = D->tr.barrier(D->tr.ctx);
    D->d_win.reset();
    D->d_push.reset();
    D->win_half = 0; D->win_b = 0;
    return rc;
}

enum { PEER_OK = 0, PEER_MALLOC = 1, PEER_EXPORT = 2, PEER_OPEN = 3, PEER_UPLOAD = 4 };
const char *peer_call_name(int c) {
    return c == PEER_MALLOC ? "hipMalloc of the receive window" : c == PEER_EXPORT ? "hipIpcGetMemHandle" : c == PEER_OPEN ? "hipIpcOpenMemHandle" : "upload of the push table";
}

// Collective: (re)build the windows for block vectors of up to b columns (see above).  Every failure is agreed on: all ranks return the
// same status and message, and none waits in a barrier for a rank that has given up.  A failure leaves the object without windows (push
// then refuses every step); a later call sets them up anew.
int peer_setup(uspmv_dist *D, int b) {
    const int P = D->P, me = D->rank;
    const size_t vsz = vsize(D);
    if (int rc = peer_release(D, true)) return rc;
    const int64_t half = std::max<int64_t>(D->n_halo * (int64_t)b, 1);
    // ---- own window, zeroed (-no_pack unpacks it unwritten) and complete before any peer can write into it
    int status = PEER_OK;
    hipError_t err = D->d_win.alloc(2 * (size_t)half * vsz);
    if (err != hipSuccess) status = PEER_MALLOC;
    if (!status && (err = hipMemset(D->d_win.get(), 0, 2 * (size_t)half * vsz)) == hipSuccess) err = hipDeviceSynchronize();
    if (!status && err != hipSuccess) status = PEER_MALLOC;
    hipIpcMemHandle_t handle;
    memset(&handle, 0, sizeof handle);
    if (!status && !D->loopback && (err = hipIpcGetMemHandle(&handle, D->d_win.get())) != hipSuccess) status = PEER_EXPORT;
    (void)hipGetLastError();
    // ---- one record per rank: status, HIP error, half, n_halo, recv_off[P+1], send_off[P+1], handle
    const size_t hw = (sizeof handle + 7) / 8, nrec = 4 + 2 * ((size_t)P + 1) + hw;
    std::vector<int64_t> rec(nrec, 0), all(nrec * (size_t)P, 0);
    rec[0] = status; rec[1] = (int64_t)err; rec[2] = half; rec[3] = D->n_halo;
    for (int p = 0; p <= P; ++p) { rec[4 + (size_t)p] = D->recv_off[(size_t)p]; rec[5 + (size_t)P + (size_t)p] = D->send_off[(size_t)p]; }
    // (test only, option "diag_peer_skew": this rank announces one element more from its first neighbour than that neighbour sends it)
    if (D->diag_peer_skew)
        for (int p = 0; p < P; ++p)
            if (D->recv_off[(size_t)p + 1] > D->recv_off[(size_t)p]) { for (int j = p + 1; j <= P; ++j) ++rec[4 + (size_t)j]; break; }
    memcpy(&rec[6 + 2 * (size_t)P], &handle, sizeof handle);
    auto fail_all = [&](int code, const std::string &msg) { D->d_win.reset(); D->win_half = 0; return uspmv::fail(code, "%s", msg.c_str()); };
    if (int rc = D->tr.allgather(D->tr.ctx, rec.data(), all.data(), (int64_t)(nrec * 8))) { D->d_win.reset(); return rc; }
    auto R = [&](int q) { return all.data() + (size_t)q * nrec; };
    const char *hint = " -- on ROCm, IPC between processes needs HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of every rank";
    char buf[512];
    for (int q = 0; q < P; ++q)
        if (R(q)[0]) {
            snprintf(buf, sizeof buf, "USPMV_EXCHANGE_PEER set-up: rank %d: %s failed: %s%s", q, peer_call_name((int)R(q)[0]),
                     hipGetErrorString((hipError_t)R(q)[1]), R(q)[0] == PEER_EXPORT ? hint : "");
            return fail_all(R(q)[0] == PEER_MALLOC ? USPMV_ERR_ALLOC : USPMV_ERR_HIP, buf);
        }
    // ---- validate every pair on the same data (loopback: the records are all this process's, the destination of "q" is its own block)
    std::vector<PeerDst> tab((size_t)P, PeerDst{nullptr, 0, 0});
    for (int r = 0; r < P; ++r)
        for (int q = 0; q < P && (r == me || !D->loopback); ++q) {
            // loopback: "q expects from me" := what this process asked q for, in its own window
            const int64_t *so = R(r) + 5 + P, *ro = D->loopback ? R(me) + 4 + q : R(q) + 4 + r, *qq = D->loopback ? R(me) : R(q);
            const int64_t ns = so[q + 1] - so[q], nr = ro[1] - ro[0];
            if (ns != nr) {
                snprintf(buf, sizeof buf, "USPMV_EXCHANGE_PEER set-up: rank %d sends %ld elements to rank %d, which expects %ld from it", r, (long)ns, q, (long)nr);
                return fail_all(USPMV_ERR_INVALID, buf);
            }
            if (ns && (ro[0] < 0 || ro[1] > qq[4 + P] || qq[4 + P] != qq[3] || qq[3] * b > qq[2])) {
                snprintf(buf, sizeof buf, "USPMV_EXCHANGE_PEER set-up: rank %d's block [%ld, %ld) lies outside rank %d's window (%ld halo slots, %ld x %d elements)",
                         r, (long)ro[0], (long)ro[1], q, (long)qq[3], (long)qq[2], b);
                return fail_all(USPMV_ERR_INVALID, buf);
            }
            if (r == me && ns) tab[(size_t)q] = PeerDst{nullptr, qq[2], ro[0]};
        }
    // ---- open the windows of the ranks this one sends to; agree on the outcome
    D->peer_win.assign((size_t)P, nullptr);
    int64_t ost[3] = {PEER_OK, 0, 0};   // status, HIP error, whose window
    for (int q = 0; q < P; ++q) {
        if (!tab[(size_t)q].half) continue;
        if (D->loopback || q == me) { tab[(size_t)q].base = D->d_win.get(); continue; }
        hipIpcMemHandle_t hq;
        memcpy(&hq, R(q) + 6 + 2 * (size_t)P, sizeof hq);
        const hipError_t e = hipIpcOpenMemHandle(&D->peer_win[(size_t)q], hq, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) { (void)hipGetLastError(); D->peer_win[(size_t)q] = nullptr; ost[0] = PEER_OPEN; ost[1] = (int64_t)e; ost[2] = q; break; }
        tab[(size_t)q].base = D->peer_win[(size_t)q];
    }
    if (!ost[0]) {
        hipError_t e = D->d_push.upload(tab.data(), sizeof(PeerDst) * tab.size());
        if (e == hipSuccess) e = D->d_seg.upload(D->send_off.data(), 8 * D->send_off.size());
        if (e != hipSuccess) { (void)hipGetLastError(); D->d_push.reset(); ost[0] = PEER_UPLOAD; ost[1] = (int64_t)e; ost[2] = me; }
    }
    std::vector<int64_t> oall(3 * (size_t)P, 0);
    if (D->loopback) std::copy(ost, ost + 3, oall.begin());
    else if (int rc = D->tr.allgather(D->tr.ctx, ost, oall.data(), sizeof ost)) { (void)peer_release(D, false); return rc; }
    for (int q = 0; q < (D->loopback ? 1 : P); ++q)
        if (const int64_t *o = &oall[3 * (size_t)q]; o[0]) {
            if (o[0] == PEER_OPEN)
                snprintf(buf, sizeof buf, "USPMV_EXCHANGE_PEER set-up: rank %d: hipIpcOpenMemHandle of rank %ld's window failed: %s%s", q,
                         (long)o[2], hipGetErrorString((hipError_t)o[1]), hint);
            else
                snprintf(buf, sizeof buf, "USPMV_EXCHANGE_PEER set-up: rank %d: %s failed: %s", q, peer_call_name((int)o[0]), hipGetErrorString((hipError_t)o[1]));
            const std::string msg = buf;
            (void)peer_release(D, true);                                 // (every rank is here: close, barrier, free)
            return uspmv::fail(USPMV_ERR_HIP, "%s", msg.c_str());
        }
    D->win_half = half; D->win_b = b; D->parity = 0; D->unpack_queued = false;
    return USPMV_OK;
}

// ---- the exchange of b vectors in the reference's three message patterns (the single-vector step: b = 1, row-wise, bulk)
//   USPMV_BULKVEC   one message per neighbour carrying all b vectors           (code/classes_structs.hpp:909-924, :971-981)
//   USPMV_MULTIVEC  one message per neighbour and vector, all posted together  (:893-907, :953-960)
//   USPMV_SINGLEVEC one exchange per vector, one after the other               (:875-891, :943-951; the loop of code/mpi_funcs.hpp:35-60)
// Row-wise X ([element][v]): a neighbour's bulk block is exactly the row-wise halo region, so it lands in the tail of X directly.
// Column-wise X: per-vector messages land in the halo region of their column directly; the bulk block ([v][element] per neighbour)
// lands in a staging buffer and b small gathers move it.  Row-wise X with per-vector messages would need strided receives: refused.
// The peer-store exchange needs no plan: its stores carry no messages, so one push serves every pattern.

// Appends the plan of (b, layout, mode) to D->block_plans; on failure nothing of it stays behind
hipError_t add_block_plan(uspmv_dist *D, int b, int layout, int mode) {
    uspmv_dist::BlockPlan bp;
    bp.b = b; bp.layout = layout; bp.mode = mode;
    const int64_t ld = D->vec_len, ns = D->n_send, nh = D->n_halo;
    const size_t vsz = vsize(D);
    hipError_t e = hipSuccess;
    if (b > 1) {                                           // (b = 1: the wire order of every pattern is uspmv_dist::d_src)
        std::vector<int32_t> src((size_t)(ns * b));
        if (layout == USPMV_ROWWISE) {                     // wire = [element][v] (bulk only)
            for (int64_t i = 0; i < ns; ++i)
                for (int v = 0; v < b; ++v) src[(size_t)(i * b + v)] = (int32_t)((int64_t)D->h_perm[(size_t)D->h_send_idxs[(size_t)i]] * b + v);
        } else if (mode == USPMV_BULKVEC) {                // wire = per neighbour [v][element]
            size_t o = 0;
            for (int p = 0; p < D->P; ++p)
                for (int v = 0; v < b; ++v)
                    for (int64_t i = D->send_off[(size_t)p]; i < D->send_off[(size_t)p + 1]; ++i)
                        src[o++] = (int32_t)(D->h_perm[(size_t)D->h_send_idxs[(size_t)i]] + (int64_t)v * ld);
        } else {                                           // wire = [v][element over all neighbours]
            for (int v = 0; v < b; ++v)
                for (int64_t i = 0; i < ns; ++i) src[(size_t)(v * ns + i)] = (int32_t)(D->h_perm[(size_t)D->h_send_idxs[(size_t)i]] + (int64_t)v * ld);
        }
        e = bp.d_src.upload(src.data(), 4 * src.size());
    }
    if (e == hipSuccess) e = bp.d_send.alloc(vsz * std::max<size_t>((size_t)(ns * b), 1));
    if (e == hipSuccess && D->exchange == USPMV_EXCHANGE_HOST) e = bp.h_send.alloc(vsz * std::max<size_t>((size_t)(ns * b), 1));
    if (e == hipSuccess && D->exchange == USPMV_EXCHANGE_HOST) e = bp.h_recv.alloc(vsz * std::max<size_t>((size_t)(nh * b), 1));
    if (e == hipSuccess && layout == USPMV_COLWISE && mode == USPMV_BULKVEC) {
        e = bp.d_recv.alloc(vsz * std::max<size_t>((size_t)(nh * b), 1));
        std::vector<int32_t> un((size_t)nh);
        for (int v = 0; v < b && e == hipSuccess; ++v) {
            for (int p = 0; p < D->P; ++p) {
                const int64_t nr = D->recv_counts[(size_t)p], ro = D->recv_off[(size_t)p];
                for (int64_t k = 0; k < nr; ++k) un[(size_t)(ro + k)] = (int32_t)((int64_t)b * ro + (int64_t)v * nr + k);
            }
            bp.d_unpack.emplace_back();
            e = bp.d_unpack.back().upload(un.data(), 4 * un.size());
        }
    }
    if (e == hipSuccess) D->block_plans.push_back(std::move(bp));
    return e;
}

// The plan of (b, layout, mode), built at its first use; the pointer is valid until the next plan is added
uspmv_dist::BlockPlan *block_plan(uspmv_dist *D, int b, int layout, int mode) {
    for (auto &bp : D->block_plans)
        if (bp.b == b && bp.layout == layout && bp.mode == mode) return &bp;
    if (const hipError_t e = add_block_plan(D, b, layout, mode)) {
        (void)hipGetLastError();
        uspmv::fail(USPMV_ERR_ALLOC, "uspmv_dist_spmmv: %s", hipGetErrorString(e));
        return nullptr;
    }
    return &D->block_plans.back();
}

// The per-step halo exchange of b vectors of X in (layout, mode), queued on `st`.  The single-vector step passes (1, USPMV_ROWWISE,
// USPMV_BULKVEC) and the padding column whose value the pack keeps (pads_on), block vectors -1.  For every transport, -no_pack 1 packs
// (pushes) no element and a stale buffer travels (timing only, code/classes_structs.hpp:941); diag_skip_exchange packs (pushes) no
// element and nothing travels: the halo region keeps what it held.
int exchange(uspmv_dist *D, void *d_X, int b, int layout, int mode, int pad_col, hipStream_t st) {
    const long n = D->no_pack || D->diag_skip_exchange ? 0 : (long)D->n_send;   // elements packed (pushed) per vector
    const size_t vsz = vsize(D);
    const int64_t ld = D->vec_len, ns = D->n_send, nh = D->n_halo;
    if (D->exchange == USPMV_EXCHANGE_PEER) {
        // one push of all b columns into the neighbours' windows, one unpack of this rank's window into the halo region of X
        const int rowwise = layout == USPMV_ROWWISE;
        if (int rc = push(D, d_X, b, (long)ld, rowwise, n, pad_col, st)) return rc;
        return D->diag_skip_exchange ? USPMV_OK : peer_complete(D, d_X, b, (long)ld, rowwise, st);
    }
    uspmv_dist::BlockPlan *bp = block_plan(D, b, layout, mode);
    if (!bp) return USPMV_ERR_ALLOC;
    if (int rc = pack(D, bp->d_send, d_X, b == 1 ? D->d_src.get() : bp->d_src.get(), n * b, pad_col, st)) return rc;
    if (D->diag_skip_exchange) return USPMV_OK;
    char *X = (char *)d_X;
    const char *S = (const char *)bp->d_send.get();
    const bool bulk = mode == USPMV_BULKVEC;
    char *R = layout == USPMV_ROWWISE ? X + (size_t)D->n_local * b * vsz : (char *)bp->d_recv.get();   // where a bulk block lands
    if (D->exchange == USPMV_EXCHANGE_HOST) {
        // pack -> pinned host buffer -> all-to-all-v over the transport -> X.  The host waits for the pack (and returns with the upload
        // queued on `st`), so the caller may queue independent device work on another stream first.  One all-to-all-v of b vectors
        // (bulk) or one per vector (multivec and singlevec differ in posting order only)
        char *hs = (char *)bp->h_send.get(), *hr = (char *)bp->h_recv.get();
        if (ns * b > 0) HIP_TRY(hipMemcpyAsync(hs, S, (size_t)(ns * b) * vsz, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int w = bulk ? b : 1;                          // vectors per message
        std::vector<int64_t> so((size_t)D->P + 1), ro((size_t)D->P + 1);
        for (int p = 0; p <= D->P; ++p) { so[(size_t)p] = D->send_off[(size_t)p] * w * (int64_t)vsz; ro[(size_t)p] = D->recv_off[(size_t)p] * w * (int64_t)vsz; }
        for (int v = 0; v < b / w; ++v) {
            if (int rc = D->tr.alltoallv(D->tr.ctx, hs + (size_t)(v * ns) * vsz, so.data(), hr + (size_t)(v * nh) * vsz, ro.data())) return rc;
            char *dst = bulk ? R : X + (size_t)(v * ld + D->n_local) * vsz;
            if (nh * w > 0) HIP_TRY(hipMemcpyAsync(dst, hr + (size_t)(v * nh) * vsz, (size_t)(nh * w) * vsz, hipMemcpyHostToDevice, st));
        }
    } else if (bulk) {
        NCCL_TRY(ncclGroupStart());
        for (int p = 0; p < D->P; ++p) {
            const int64_t nsp = D->send_off[(size_t)p + 1] - D->send_off[(size_t)p], nr = D->recv_counts[(size_t)p];
            if (nr) NCCL_TRY(ncclRecv(R + (size_t)(D->recv_off[(size_t)p] * b) * vsz, (size_t)(nr * b), nccl_vt(D), peer(D, p), D->comm, st));
            if (nsp) NCCL_TRY(ncclSend(S + (size_t)(D->send_off[(size_t)p] * b) * vsz, (size_t)(nsp * b), nccl_vt(D), peer(D, p), D->comm, st));
        }
        NCCL_TRY(ncclGroupEnd());
    } else {
        // per-vector messages: one group of all b vectors (multivec) or one group per vector (singlevec)
        const int per_group = mode == USPMV_MULTIVEC ? b : 1;
        for (int v0 = 0; v0 < b; v0 += per_group) {
            NCCL_TRY(ncclGroupStart());
            for (int v = v0; v < v0 + per_group; ++v)
                for (int p = 0; p < D->P; ++p) {
                    const int64_t nsp = D->send_off[(size_t)p + 1] - D->send_off[(size_t)p], nr = D->recv_counts[(size_t)p];
                    if (nr) NCCL_TRY(ncclRecv(X + (size_t)(v * ld + D->n_local + D->recv_off[(size_t)p]) * vsz, (size_t)nr, nccl_vt(D), peer(D, p), D->comm, st));
                    if (nsp) NCCL_TRY(ncclSend(S + (size_t)(v * ns + D->send_off[(size_t)p]) * vsz, (size_t)nsp, nccl_vt(D), peer(D, p), D->comm, st));
                }
            NCCL_TRY(ncclGroupEnd());
        }
    }
    if (bulk && layout == USPMV_COLWISE && nh)               // the staged bulk block -> the halo region of every column
        for (int v = 0; v < b; ++v)
            if (int rc = uspmv_apply_permutation_dev(X + (size_t)(v * ld + D->n_local) * vsz, bp->d_recv, bp->d_unpack[(size_t)v], nh, D->dtype, st)) return rc;
    return USPMV_OK;
}

// The exchange of a block of b > 1 vectors: their gather lists index b * padded_vec_size elements in int32; the peer-store windows grow
// (collectively, as the call is) the first time a wider block appears -- never in the single-vector step, which refuses once a failed
// growth lost them
int block_exchange(uspmv_dist *D, void *d_X, int b, int layout, int mode, hipStream_t st, const char *who) {
    if ((int64_t)b * std::max(D->vec_len, (int64_t)1) > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: b * padded_vec_size exceeds int32", who);
    if (D->exchange == USPMV_EXCHANGE_PEER && b > D->win_b)
        if (int rc = peer_setup(D, b)) return rc;
    return exchange(D, d_X, b, layout, mode, -1, st);
}

// the single-vector step's exchange
inline int exchange_x(uspmv_dist *D, void *d_x, hipStream_t st) {
    return exchange(D, d_x, 1, USPMV_ROWWISE, USPMV_BULKVEC, pads_on(D) ? D->pad_col : -1, st);
}
// steps that block the host inside the exchange (host-staged, peer-store between real ranks) run eagerly: there is nothing to capture
inline bool eager_only(const uspmv_dist *D) { return D->exchange != USPMV_EXCHANGE_RCCL; }

int part(uspmv_dist *D, const int32_t *ids, int64_t n, const void *x, void *y, hipStream_t st) {
    if (n == 0) return USPMV_OK;
    const uspmv_dist::Part *p = D->pt;
    if (has_hp(D))
        return D->tiles ? uspmv_spmv_ap_hp_tiles(p[0].A, p[1].A, p[2].A, ids, n, x, y, st) : uspmv_spmv_ap_hp_chunks(p[0].A, p[1].A, p[2].A, ids, n, x, y, st);
    if (is_ap(D))
        return D->tiles ? uspmv_spmv_ap_tiles(p[0].A, p[1].A, ids, n, (const double *)x, (double *)y, st)
                        : uspmv_spmv_ap_chunks(p[0].A, p[1].A, ids, n, (const double *)x, (double *)y, st);
    return D->tiles ? uspmv_spmv_tiles(D->A, ids, n, x, y, st) : uspmv_spmv_chunks(D->A, ids, n, x, y, st);
}

// the whole matrix in one launch
int whole(uspmv_dist *D, const void *x, void *y, hipStream_t st) {
    const uspmv_dist::Part *p = D->pt;
    if (has_hp(D)) return uspmv_spmv_ap_hp(p[0].A, p[1].A, p[2].A, x, y, st);
    return is_ap(D) ? uspmv_spmv_ap(p[0].A, p[1].A, (const double *)x, (double *)y, st) : uspmv_spmv(D->A, x, y, st);
}

// -ba_synch 1: the barrier the reference issues after every iteration (code/main.cpp:467, :417; default on,
// code/classes_structs.hpp:90) as a stream-ordered one-element all-reduce -- no rank's next step starts before every rank has
// finished this one, and the host is not involved (so it is part of the captured graph)
int step_barrier(uspmv_dist *D, hipStream_t main) {
    if (!D->ba_synch || D->P == 1) return USPMV_OK;
    if (!D->comm) {                                                  // (host-staged / peer-store: over the transport; loopback: stream order)
        if (D->loopback) return USPMV_OK;
        HIP_TRY(hipStreamSynchronize(main));
        return D->tr.barrier ? D->tr.barrier(D->tr.ctx) : USPMV_OK;
    }
    if (D->diag_skip_exchange) return USPMV_OK;
    NCCL_TRY(ncclAllReduce(D->d_scratch, D->d_scratch + 1, 1, ncclInt32, ncclSum, D->comm, main));
    return USPMV_OK;
}

// The one-launch form of the step below (uspmv_dist::d_step)
int step_fused(uspmv_dist *D, void *d_x, void *d_y, hipStream_t main) {
    if (D->sync_dirty) if (int rc = sync_reset(D)) return rc;
    D->sync_dirty = true;                                            // (cleared when every launch of the step has been issued)
    HIP_TRY(hipEventRecord(D->ev_main, main));
    HIP_TRY(hipStreamWaitEvent(D->side_stream, D->ev_main, 0));
    int rc = D->dtype == USPMV_F64 ? uspmv_dev::launch_spmv_tlc_step<double>(D->A, D->d_step, D->sa, 1, (const double *)d_x, (double *)d_y, D->side_stream)
                                   : uspmv_dev::launch_spmv_tlc_step<float>(D->A, D->d_step, D->sa, 1, (const float *)d_x, (float *)d_y, D->side_stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(D->ev_comm, D->side_stream));
    if ((rc = exchange_x(D, d_x, main))) return rc;                  // (a failure here leaves the counters out of step: sync_dirty stays set)
    hipLaunchKernelGGL(exchange_done_kernel, dim3(1), dim3(1), 0, main, D->d_ss);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamWaitEvent(main, D->ev_comm, 0));                // join: the deferred list is complete
    rc = D->dtype == USPMV_F64 ? uspmv_dev::launch_spmv_tlc_step<double>(D->A, D->d_step, D->sa, 2, (const double *)d_x, (double *)d_y, main)
                               : uspmv_dev::launch_spmv_tlc_step<float>(D->A, D->d_step, D->sa, 2, (const float *)d_x, (float *)d_y, main);
    if (rc) return rc;
    D->sync_dirty = false;
    return step_barrier(D, main);
}

// One SpMV: the interior tiles on the side stream, the exchange meanwhile on the caller's stream, the boundary tiles after both.
// The RCCL group stays on the CALLER's stream on purpose: when the step is captured, that is the capture's origin stream.  Under
// the HIP 7.0 / RCCL 2.26 pair that torch bundles, hipStreamEndCapture crashes if an RCCL p2p group was captured on a stream that
// JOINED the capture through an event, while the same group on the origin stream, and kernels on joined streams, capture fine
// (profiles/r03/graph_capture_diag_before_fix.txt / _after_fix.txt; the system's HIP 7.2 / RCCL 2.27 takes either form).  Same DAG, same overlap.
int step(uspmv_dist *D, void *d_x, void *d_y, hipStream_t main, bool comm_halos) {
    if (D->P == 1 || !comm_halos) return whole(D, d_x, d_y, main);
    if (!D->overlap) {
        if (int rc = exchange_x(D, d_x, main)) return rc;
        if (int rc = whole(D, d_x, d_y, main)) return rc;
        return step_barrier(D, main);
    }
    // (not under capture: replayed from a hipGraph the one-launch form measured 0.54 ms against 0.21 ms, profiles/r03/dist_step_ab.txt)
    if (fused_on(D) && !D->capturing && (pads_on(D) || D->n_pad == 0)) return step_fused(D, d_x, d_y, main);
    const bool pads = pads_on(D);                                    // padding tiles run with the interior ones (see uspmv_dist::pad_col)
    HIP_TRY(hipEventRecord(D->ev_main, main));                       // fork: everything queued on `main` so far precedes the interior tiles
    HIP_TRY(hipStreamWaitEvent(D->side_stream, D->ev_main, 0));
    if (int rc = pads ? part(D, D->d_early, D->n_int + D->n_pad, d_x, d_y, D->side_stream) : part(D, D->d_int, D->n_int, d_x, d_y, D->side_stream)) return rc;
    HIP_TRY(hipEventRecord(D->ev_comm, D->side_stream));
    if (int rc = exchange_x(D, d_x, main)) return rc;                // pack kernel + grouped send / recv into the tail of x (host mode: blocks the host)
    if (pads) if (int rc = pad_guard(D, d_x, main)) return rc;
    HIP_TRY(hipStreamWaitEvent(main, D->ev_comm, 0));                // join
    // (pads: the conditional entries are switched off by the guard unless x[pad_col] changed sign or is not finite)
    if (int rc = pads ? part(D, D->d_late, D->n_bnd_real + D->n_pad, d_x, d_y, main) : part(D, D->d_bnd, D->n_bnd, d_x, d_y, main)) return rc;
    return step_barrier(D, main);
}

void drop_graph(uspmv_dist *D) {
    if (D->gexec) (void)hipGraphExecDestroy(D->gexec);
    D->gexec = nullptr; D->g_x = D->g_y = nullptr; D->g_stream = nullptr;
}

#define DBG(msg) do { if (getenv("USPMV_VERBOSE")) { fprintf(stderr, "[uspmv] dist capture: %s\n", msg); fflush(stderr); } } while (0)

int capture(uspmv_dist *D, void *d_x, void *d_y, hipStream_t main) {
    drop_graph(D);
    hipGraph_t g = nullptr;
    DBG("begin");
    hipError_t e = hipStreamBeginCapture(main, (hipStreamCaptureMode)D->capture_mode);
    if (e != hipSuccess) { (void)hipGetLastError(); return uspmv::fail(USPMV_ERR_HIP, "uspmv_dist_run: hipStreamBeginCapture: %s", hipGetErrorString(e)); }
    D->capturing = true;
    const int rc = step(D, d_x, d_y, main, true);
    D->capturing = false;
    DBG("step issued");
    e = hipStreamEndCapture(main, &g);
    DBG("end capture");
    if (rc != USPMV_OK || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return rc != USPMV_OK ? rc : uspmv::fail(USPMV_ERR_HIP, "uspmv_dist_run: hipStreamEndCapture: %s", hipGetErrorString(e));
    }
    e = hipGraphInstantiate(&D->gexec, g, nullptr, nullptr, 0);
    DBG("instantiated");
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { D->gexec = nullptr; (void)hipGetLastError(); return uspmv::fail(USPMV_ERR_HIP, "uspmv_dist_run: hipGraphInstantiate: %s", hipGetErrorString(e)); }
    D->g_x = d_x; D->g_y = d_y; D->g_stream = main;
    return USPMV_OK;
}

}  // namespace

extern "C" {

int uspmv_comm_unique_id(void *id128) {
    if (!id128) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_comm_unique_id: NULL argument");
    static_assert(sizeof(ncclUniqueId) == USPMV_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    memcpy(id128, &id, sizeof id);
    return USPMV_OK;
}

int uspmv_runtime_versions(int v[4]) {
    if (!v) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_runtime_versions: NULL argument");
    v[0] = HIP_VERSION; v[1] = 0; v[2] = NCCL_VERSION_CODE; v[3] = 0;
    (void)hipRuntimeGetVersion(&v[1]);
    (void)ncclGetVersion(&v[3]);
    return USPMV_OK;
}

void uspmv_dist_free(uspmv_dist_t *D) {
    if (!D) return;
    drop_graph(D);
    (void)peer_release(D, true);                                    // collective: close, barrier, free (see peer_release)
    if (D->ev_main) (void)hipEventDestroy(D->ev_main);
    if (D->ev_comm) (void)hipEventDestroy(D->ev_comm);
    if (D->ev_push) (void)hipEventDestroy(D->ev_push);
    if (D->ev_unpack) (void)hipEventDestroy(D->ev_unpack);
    if (D->side_stream) (void)hipStreamDestroy(D->side_stream);
    if (D->comm) (void)ncclCommDestroy(D->comm);
    uspmv_comm_plan_free(D->plan);
    if (D->owns_setup) {
        for (auto &p : D->pt) { uspmv_dmat_free(p.A); uspmv_scs_free(p.scs); }
        uspmv_halo_free(D->halo);
    }
    delete D;
}

// uspmv_dist_create_ex; windows = false leaves the collective window set-up of USPMV_EXCHANGE_PEER to the caller
static int create_dist(const void *comm_id, int comm_rank, int comm_size, int rank, int P, uspmv_dmat_t *A, const uspmv_halo_t *halo,
                       const int32_t *old_to_new_idx, const int32_t *interior_ids, int64_t n_interior, const int32_t *boundary_ids,
                       int64_t n_boundary, int ids_are_tiles, const uspmv_dist_options_t *opt, uspmv_dist_t **out, bool windows,
                       bool ap = false) {
    const int ex = opt ? opt->exchange : USPMV_EXCHANGE_RCCL;
    if (ex != USPMV_EXCHANGE_RCCL && ex != USPMV_EXCHANGE_HOST && ex != USPMV_EXCHANGE_PEER)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: unknown exchange %d", ex);
    if (!A || !halo || !out || P < 1 || rank < 0 || rank >= P || n_interior < 0 || n_boundary < 0 || (n_interior > 0 && !interior_ids) ||
        (n_boundary > 0 && !boundary_ids))
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: bad argument");
    switch (ex) {
    case USPMV_EXCHANGE_HOST:
        if (!opt->transport || !opt->transport->alltoallv) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: USPMV_EXCHANGE_HOST needs a transport");
        comm_rank = rank; comm_size = P;
        break;
    case USPMV_EXCHANGE_PEER:
        // comm_size == P: real ranks, which need a transport (set-up exchanges, per-step barrier); comm_size == 1: loopback, no transport
        if (comm_size < 1 || comm_rank < 0 || comm_rank >= comm_size) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: bad communicator argument");
        if (!(comm_size == P && comm_rank == rank) && !(comm_size == 1 && comm_rank == 0))
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: USPMV_EXCHANGE_PEER takes one rank per partition block (comm_size == P) or a single rank (loopback)");
        if (comm_size == P && P > 1 && (!opt->transport || !opt->transport->allgather || !opt->transport->barrier))
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: USPMV_EXCHANGE_PEER between real ranks needs a transport with all-gather and barrier "
                               "(it carries the set-up exchanges and the per-step barrier)");
        if (comm_size == 1 && P > 1 && opt->transport)
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: USPMV_EXCHANGE_PEER in loopback takes no transport");
        break;
    default:
        if (!comm_id || comm_size < 1 || comm_rank < 0 || comm_rank >= comm_size) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: bad communicator argument");
        if (!(comm_size == P && comm_rank == rank) && !(comm_size == 1 && comm_rank == 0))
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: the communicator must have one rank per partition block (comm_size == P) or a single rank (loopback)");
    }
    if (opt && opt->transport && (opt->transport->size != P || opt->transport->rank != rank))
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: the transport is rank %d of %d, the block is %d of %d", opt->transport->rank, opt->transport->size, rank, P);
    if (halo->P != P || halo->rank != rank) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: halo description belongs to another partition");
    if (halo->n_local > 0 && !old_to_new_idx) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: NULL permutation");
    if (int rc = uspmv_dev::check_dmat(A, "uspmv_dist_create")) return rc;
    if (A->dtype == USPMV_F16) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "uspmv_dist_create: fp16 handle (no one-precision fp16 SpMV)");
    if (int rc = uspmv_dev::require_device()) return rc;
    auto *D = new uspmv_dist;
    D->rank = rank; D->P = P; D->comm_rank = comm_rank; D->comm_size = comm_size; D->loopback = comm_size == 1 && P > 1;   // (host: comm_size == P)
    D->exchange = ex;
    D->A = A; D->dtype = A->dtype; D->tiles = ids_are_tiles != 0;
    D->pad_split = ap;                // (adaptive precision: on by default; kind and the other parts are attached by setup_from_coo at its hand-over)
    D->n_local = halo->n_local; D->n_halo = halo->n_halo; D->n_int = n_interior; D->n_bnd = n_boundary;
    D->recv_counts = halo->recv_counts;
    auto bail = [&](int code) { uspmv_dist_free(D); return code; };
#define D_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return bail(uspmv::fail(USPMV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__)); } while (0)
#define D_NCCL(call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) return bail(uspmv::fail(USPMV_ERR_HIP, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(r_), __FILE__, __LINE__)); } while (0)
    if (ex == USPMV_EXCHANGE_RCCL) {
        ncclUniqueId id;
        memcpy(&id, comm_id, sizeof id);
        D_NCCL(ncclCommInitRank(&D->comm, comm_size, id, comm_rank));
    }
    D_HIP(hipStreamCreateWithFlags(&D->side_stream, hipStreamNonBlocking));
    D_HIP(hipEventCreateWithFlags(&D->ev_main, hipEventDisableTiming));
    D_HIP(hipEventCreateWithFlags(&D->ev_comm, hipEventDisableTiming));
    if (ex == USPMV_EXCHANGE_PEER) D_HIP(hipEventCreateWithFlags(&D->ev_push, hipEventDisableTiming));
    if (ex == USPMV_EXCHANGE_PEER) D_HIP(hipEventCreateWithFlags(&D->ev_unpack, hipEventDisableTiming));
    D_HIP(D->d_scratch.zeros(256));
    // ---- who sends what to whom (collect_comm_info, code/mpi_funcs.hpp:1061-1124) over the set-up transport
    if (opt && opt->transport) D->tr = *opt->transport;
    else if (D->loopback) { D->tr.ctx = D; D->tr.rank = rank; D->tr.size = P; D->tr.alltoallv = self_alltoallv; D->tr.allgather = self_allgather; D->tr.barrier = self_barrier; }
    else { D->tr.ctx = D; D->tr.rank = comm_rank; D->tr.size = comm_size; D->tr.alltoallv = rccl_alltoallv; D->tr.allgather = rccl_allgather; D->tr.barrier = rccl_barrier; }
    if (int rc = uspmv_comm_plan_create(&D->tr, halo, &D->plan)) {
        if (D->loopback && rc == USPMV_ERR_INVALID) {
            const std::string why = uspmv_last_error();
            rc = uspmv::fail(USPMV_ERR_INVALID, "%s -- loopback needs equal block heights (seg-rows on a size divisible by P); unequal blocks run with real "
                             "ranks (USPMV_EXCHANGE_HOST on one GPU, RCCL on several)", why.c_str());
        }
        return bail(rc);
    }
    D->send_off = D->plan->send_off; D->recv_off = D->plan->recv_off; D->n_send = D->plan->n_send;
    D->h_send_idxs = D->plan->send_idxs;
    D->h_perm.assign(old_to_new_idx, old_to_new_idx + D->n_local);
    // ---- device state of the step
    D_HIP(D->d_send_idxs.upload(D->h_send_idxs.data(), 4 * (size_t)D->n_send));
    D_HIP(D->d_perm.upload(old_to_new_idx, 4 * (size_t)D->n_local));
    {
        std::vector<int32_t> src((size_t)D->n_send);
        for (int64_t i = 0; i < D->n_send; ++i) src[(size_t)i] = old_to_new_idx[D->h_send_idxs[(size_t)i]];     // (ids validated in [0, n_local) by the plan)
        D_HIP(D->d_src.upload(src.data(), 4 * (size_t)D->n_send));
        D_HIP(D->d_stale.zeros(16));
    }
    D_HIP(D->d_int.upload(interior_ids, 4 * (size_t)n_interior));
    D_HIP(D->d_bnd.upload(boundary_ids, 4 * (size_t)n_boundary));
    D->n_rows_padded = A->n_chunks * A->C;
    D->vec_len = D->n_local + std::max(D->n_rows_padded - D->n_local, D->n_halo);       // padded_vec_size (code/main.cpp:1406-1412)
    // the single-vector step's exchange plan, here so that no step allocates (a captured one must not); peer stores need none
    if (ex != USPMV_EXCHANGE_PEER) D_HIP(add_block_plan(D, 1, USPMV_ROWWISE, USPMV_BULKVEC));
    if (P > 1 && !A->alt && A->n_chunks > 0 && !ap) {
        // the same split for block vectors: per chunk, does it (or its tile) touch a halo column
        std::vector<unsigned char> flag((size_t)A->n_chunks, 0);
        const int64_t cpt = ids_are_tiles ? std::max<int64_t>(A->tlc.tile_rows / A->C, 1) : 1;
        bool ok = true;
        for (int64_t k = 0; k < n_boundary && ok; ++k) {
            const int64_t c0 = (int64_t)boundary_ids[k] * cpt;
            if (boundary_ids[k] < 0 || c0 >= A->n_chunks) { ok = false; break; }
            for (int64_t c = c0; c < std::min(c0 + cpt, A->n_chunks); ++c) flag[(size_t)c] = 1;
        }
        if (!ok) return bail(uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_create: boundary id outside the matrix"));
        if (int rc = uspmv_dev::dmat_part_set_chunks(A, flag.data())) return bail(rc);
        D->parts = true;
    }
    // the collective window set-up last, after every check that could fail on one rank alone (that rank's free would then enter a barrier
    // the others never join); uspmv_dist_create_from_coo_ex runs it after its own rank-local steps instead
    if (ex == USPMV_EXCHANGE_PEER && P > 1 && windows)
        if (int rc = peer_setup(D, 1)) return bail(rc);
#undef D_HIP
#undef D_NCCL
    *out = D;
    return USPMV_OK;
}

int uspmv_dist_create_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, uspmv_dmat_t *A, const uspmv_halo_t *halo,
                         const int32_t *old_to_new_idx, const int32_t *interior_ids, int64_t n_interior, const int32_t *boundary_ids,
                         int64_t n_boundary, int ids_are_tiles, const uspmv_dist_options_t *opt, uspmv_dist_t **out) {
    return create_dist(comm_id, comm_rank, comm_size, rank, P, A, halo, old_to_new_idx, interior_ids, n_interior, boundary_ids, n_boundary,
                       ids_are_tiles, opt, out, true);
}

int uspmv_dist_create(const void *comm_id, int comm_rank, int comm_size, int rank, int P, uspmv_dmat_t *A, const uspmv_halo_t *halo,
                      const int32_t *old_to_new_idx, const int32_t *interior_ids, int64_t n_interior, const int32_t *boundary_ids,
                      int64_t n_boundary, int ids_are_tiles, uspmv_dist_t **out) {
    return uspmv_dist_create_ex(comm_id, comm_rank, comm_size, rank, P, A, halo, old_to_new_idx, interior_ids, n_interior, boundary_ids, n_boundary,
                                ids_are_tiles, nullptr, out);
}

}  // extern "C"

namespace {

// ---- set-up from a rank's COO block (setup_from_coo), for every kind of object

// What the set-up is told about the kind of object it makes; filled in by the public creators below.  What else differs between one
// precision and the adaptive-precision kinds is marked "one precision:" / "ap kinds:" inside setup_from_coo.
struct CooSetup {
    const char *who;                   // the creator's public name: the prefix of every message
    int kind;                          // uspmv_dist::kind
    int dtype[3];                      // value type of the part in slot q of uspmv_dist::pt; -1: the kind has no such part
    double threshold_1, threshold_2;   // of the split (uspmv_partition_precisions / _hp); kept for the self-check's reference
    const char *refusal;               // what the creator's own check (dtype, kind) objects to, "" if nothing: reported after the NULL and rank checks
    const char *empty_tail;            // how the "owns no rows" refusal ends
};

// The units of the step (tiles; chunks without tile lists), ascending, by class: no halo column at all / halo only through the +0.0 padding
// on one column / real halo references; boundary = the latter two together
struct StepLists { std::vector<int32_t> interior, boundary, pad, real; };

// A unit is cpt consecutive chunks (1: chunk lists), its class the largest of its chunks' classes (uspmv_scs_classify_chunks)
StepLists fold_classes(const std::vector<uint8_t> &cls, int64_t cpt, int64_t n_units) {
    std::vector<uint8_t> uc((size_t)n_units, 0);
    for (int64_t c = 0; c < (int64_t)cls.size(); ++c) uc[(size_t)(c / cpt)] = std::max(uc[(size_t)(c / cpt)], cls[(size_t)c]);
    StepLists L;
    for (int64_t u = 0; u < n_units; ++u) {
        if (uc[(size_t)u] == 0) L.interior.push_back((int32_t)u);
        else { L.boundary.push_back((int32_t)u); (uc[(size_t)u] == 1 ? L.pad : L.real).push_back((int32_t)u); }
    }
    return L;
}

// The lists of the padding-tile step (uspmv_dist::d_early): d_pad, d_early = *early, d_late = the real boundary tiles and one conditional
// entry per padding tile
hipError_t upload_pad_lists(uspmv_dist *D, const StepLists &L, int32_t pad_col, std::vector<int32_t> *early) {
    early->resize(L.interior.size() + L.pad.size());
    std::merge(L.interior.begin(), L.interior.end(), L.pad.begin(), L.pad.end(), early->begin());
    std::vector<int32_t> late(L.real.size() + L.pad.size(), -1);
    std::copy(L.real.begin(), L.real.end(), late.begin());
    hipError_t e = D->d_pad.upload(L.pad.data(), 4 * L.pad.size());
    if (e == hipSuccess) e = D->d_early.upload(early->data(), 4 * early->size());
    if (e == hipSuccess) e = D->d_late.upload(late.data(), 4 * late.size());
    if (e != hipSuccess) return e;
    D->n_pad = (int64_t)L.pad.size(); D->n_bnd_real = (int64_t)L.real.size(); D->pad_col = pad_col;
    return hipSuccess;
}

// The list and the state of the one-launch step (uspmv_dist::d_step): `early` with the late entries -- `real`, then the conditional `cond`
// -- spliced in
hipError_t upload_one_launch_lists(uspmv_dist *D, const std::vector<int32_t> &early, const std::vector<int32_t> &real, const std::vector<int32_t> &cond,
                                   int32_t pad_col) {
    // the late entries three quarters into the grid: late enough for the exchange to have completed in the common case, early enough
    // for their slower (system-scope) loads not to be the tail of the launch
    const size_t late0 = early.size() - early.size() / 4, n_late = real.size() + cond.size();
    std::vector<int32_t> stepl(early.begin(), early.begin() + (long)late0);
    stepl.insert(stepl.end(), real.begin(), real.end());
    stepl.insert(stepl.end(), cond.begin(), cond.end());
    stepl.insert(stepl.end(), early.begin() + (long)late0, early.end());
    hipError_t e = D->d_step.upload(stepl.data(), 4 * stepl.size());
    if (e == hipSuccess) e = D->d_defer.alloc(4 * 2 * std::max<size_t>(n_late, 1));
    if (e == hipSuccess) e = D->d_ss.alloc(sizeof(uspmv_dev::StepSync));
    if (e != hipSuccess) return e;
    D->sa.n_early = (long)early.size(); D->sa.n_real = (long)real.size(); D->sa.n_cond = (long)cond.size(); D->sa.defer_cap = (long)std::max<size_t>(n_late, 1);
    D->sa.late0 = (long)late0;
    D->sa.ss = D->d_ss; D->sa.defer = D->d_defer; D->sa.stale = D->d_stale; D->sa.pad_col = pad_col;
    return hipSuccess;
}

// Chunk classes over all parts of a split: per chunk the largest of the parts' classes.  One padding column for all of them (all pad with
// global column 0, one halo numbering); if they ever disagree, no chunk is padding-only
struct PartClasses {
    std::vector<uint8_t> cls;
    int32_t pad_col = -1;
    bool pad_clash = false;
    void merge(const std::vector<uint8_t> &cq, int32_t pq) {
        if (cls.empty()) cls.assign(cq.size(), 0);
        for (size_t c = 0; c < cls.size(); ++c) cls[c] = std::max(cls[c], cq[c]);
        if (pq >= 0) { pad_clash = pad_clash || (pad_col >= 0 && pad_col != pq); pad_col = pq; }
    }
    void settle() {
        if (!pad_clash) return;
        for (auto &c : cls) if (c == 1) c = 2;
        pad_col = -1;
    }
};

// Where the set-up routes meet (setup_from_coo: host structs; setup_from_arrays: device arrays only): the handles pt[] exist, columns in
// the rank's numbering of `halo`, the (shared) line plan installed where the route builds one, the chunks classified.  From here: the
// step's lists, the object, the pad and one-launch lists, the collective window set-up, the hand-over of pt[] and halo to the object.
// *D is set as soon as the object exists, so that the caller's exit can free it when a later step fails.
int finish_setup(const CooSetup &k, const void *comm_id, int comm_rank, int comm_size, int rank, int P, int64_t C, uspmv_dist::Part (&pt)[3],
                 uspmv_halo_t *halo, const int32_t *o2n, PartClasses &pc, int64_t n_tiles, int64_t n_staged, const uspmv_dist_options_t *opt,
                 uspmv_dist_t **Dp, uspmv_dist_t **out) {
    const char *who = k.who;
    const bool ap = k.kind != uspmv_dist::ONE_PRECISION;
    pc.settle();
    const std::vector<uint8_t> &cls = pc.cls;
    const int32_t pad_col = pc.pad_col;
    // tile lists when the plan stages something.  one precision: whatever line plan the handle carries, unless it runs on a re-chunked copy;
    // ap kinds: only the shared line plan (plan_id != 0)
    const auto &plan = pt[0].A->tlc;
    const int tile_rows = plan.on && (!ap || plan.plan_id != 0) ? plan.tile_rows : 0;
    const bool use_tiles = tile_rows > 0 && n_staged > 0 && (ap || !pt[0].A->alt);
    // ap kinds: a plan that stages nothing is dropped, so that the whole-matrix launch takes the lane-per-row kernel too
    if (ap && !use_tiles)
        for (auto &p : pt) if (p.A && p.A->tlc.on) p.A->tlc = {};
    const StepLists L = use_tiles ? fold_classes(cls, std::max<int64_t>(tile_rows / C, 1), n_tiles) : fold_classes(cls, 1, (int64_t)cls.size());
    // (ap kinds: create_dist switches "pad_split" on, and leaves the block-vector split of the hi handle's chunks alone)
    int rc = create_dist(comm_id, comm_rank, comm_size, rank, P, pt[0].A, halo, o2n, L.interior.data(), (int64_t)L.interior.size(), L.boundary.data(),
                         (int64_t)L.boundary.size(), use_tiles ? 1 : 0, opt, Dp, false, ap);
    if (rc) return rc;
    uspmv_dist_t *D = *Dp;
    const bool pads = use_tiles && P > 1 && pad_col >= 0 && !L.pad.empty();
    std::vector<int32_t> early = L.interior;
    hipError_t e = pads ? upload_pad_lists(D, L, pad_col, &early) : hipSuccess;
    // one precision: the one-launch step.  Without padding tiles every boundary tile is a late entry and none is conditional
    if (!ap && use_tiles && P > 1 && e == hipSuccess)
        e = upload_one_launch_lists(D, early, pads ? L.real : L.boundary, pads ? L.pad : std::vector<int32_t>(), pads ? pad_col : -1);
    if (e != hipSuccess) return uspmv::fail(USPMV_ERR_ALLOC, "%s: %s", who, hipGetErrorString(e));
    if (!ap && (rc = sync_reset(D))) return rc;                     // (the one-launch step's counters)
    // the collective window set-up after every step above that could fail on this rank alone
    if (D->exchange == USPMV_EXCHANGE_PEER && P > 1)
        if ((rc = peer_setup(D, 1))) return rc;
    D->owns_setup = true; D->halo = halo;
    D->kind = k.kind; D->ap_threshold = k.threshold_1; D->ap_threshold_2 = k.threshold_2;
    D->n_pt = 0;
    for (int q = 0; q < 3; ++q) { D->pt[q] = pt[q]; D->n_pt += pt[q].A != nullptr; }
    *out = D;
    return USPMV_OK;
}

// uspmv_dist_create_ex on a block given as COO: converts it (one struct, or the two or three of a split), discovers the one halo of all
// parts, plans, and sorts the tiles (chunks) into the step's lists.  A tile of a split is a tile of ALL parts (same rows), its class the
// largest of the parts' classes; the lists, the padding column and the guard are then the one-precision object's, in the vector type of the
// hi part.
// Why the padding guard stays sufficient for a split: every part pads with (value +0 of its type, global column 0), one slot of one halo
// numbering.  On the double kinds a padding slot contributes fma(+0.0, x, acc) to its part's chain (the float and fp16 zeros widen to +0.0
// exactly); on ap[sp_hp] it contributes acc + (double)(0.0f * x) with a float x.  In both, a finite x of unchanged sign gives the same signed
// zero product, so every chain -- and y, a fixed expression of the chains -- comes out bit for bit as with the delivered value; the guard
// (pad_guard_kernel<double | float>, by D->dtype) re-runs the padding tiles whenever the kept or the delivered value is not finite or
// their signs differ.
int setup_from_coo(const CooSetup &k, const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local, const int32_t *wsa,
                   int64_t C, int64_t sigma, int tlc, const uspmv_dist_options_t *opt, uspmv_dist_t **out) {
    const char *who = k.who;
    const bool ap = k.kind != uspmv_dist::ONE_PRECISION;
    if (!local || !wsa || !out) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (P < 1 || rank < 0 || rank >= P) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad rank / P", who);
    if (k.refusal[0]) return uspmv::fail(USPMV_ERR_INVALID, "%s: %s", who, k.refusal);
    // every rank sees the whole work_sharing_arr: a block without rows is refused HERE, by all ranks alike, before the first collective
    // (the conversion of that block would fail on its rank alone and leave the others waiting in the set-up exchange)
    for (int p = 0; p < P; ++p)
        if (wsa[p + 1] <= wsa[p])
            return uspmv::fail(USPMV_ERR_INVALID, "%s: block %d of %d owns no rows (work_sharing_arr %d .. %d) -- fewer ranks or another partition%s", who, p, P,
                               (int)wsa[p], (int)wsa[p + 1], k.empty_tail);
    if (int rc = uspmv_dev::require_device()) return rc;
    uspmv_coo_t *coo[3] = {nullptr, nullptr, nullptr};   // the parts of a split, by slot (one precision converts `local` itself)
    uspmv_dist::Part pt[3];
    uspmv_halo_t *halo = nullptr;
    uspmv_dist_t *D = nullptr;
    auto free_coo = [&]() { for (auto *&c : coo) { uspmv_coo_free(c); c = nullptr; } };
    // every exit: a failure frees whatever exists by then (D lends A, scs and halo until the hand-over at the very end)
    auto done = [&](int rc) {
        free_coo();
        if (rc == USPMV_OK) return rc;
        uspmv_dist_free(D);
        for (auto &p : pt) { uspmv_dmat_free(p.A); uspmv_scs_free(p.scs); }
        uspmv_halo_free(halo);
        return rc;
    };
    // order of the reference: convert -> halo discovery (rewrites columns) -> column permutation (code/main.cpp:1128, :1271-1308); a split in
    // the single-GPU order of the host route (host/uspmv_main.cpp): partition, hi, the other parts with hi's permutation
    int rc = USPMV_OK;
    if (k.kind == USPMV_AP_DP_SP) rc = uspmv_partition_precisions(local, k.threshold_1, &coo[0], &coo[1]);
    else if (ap) rc = uspmv_partition_precisions_hp(local, k.kind, k.threshold_1, k.threshold_2, &coo[0], k.dtype[1] >= 0 ? &coo[1] : nullptr, &coo[2]);
    const int32_t *o2n = nullptr;
    for (int q = 0; q < 3 && !rc; ++q) {
        if (k.dtype[q] < 0) continue;
        rc = uspmv_convert_to_scs(ap ? coo[q] : local, C, sigma, k.dtype[q], o2n, &pt[q].scs);
        if (!rc && q == 0) rc = uspmv_scs_arrays(pt[0].scs, nullptr, nullptr, nullptr, nullptr, &o2n, nullptr);
    }
    free_coo();
    if (!rc) rc = !ap                        ? uspmv_halo_discover(pt[0].scs, wsa, rank, P, &halo)
                  : k.kind == USPMV_AP_DP_SP ? uspmv_halo_discover_ap(pt[0].scs, pt[1].scs, wsa, rank, P, &halo)
                                             : uspmv_halo_discover_ap_hp(pt[0].scs, pt[1].scs, pt[2].scs, wsa, rank, P, &halo);
    for (int q = 0; q < 3 && !rc; ++q)
        if (pt[q].scs) rc = uspmv_permute_scs_cols(pt[q].scs, o2n);
    for (int q = 0; q < 3 && !rc; ++q)
        if (pt[q].scs) rc = uspmv_dmat_upload(pt[q].scs, &pt[q].A);
    int64_t n_tiles = 0, n_staged = 0;
    if (!rc && tlc) {
        // The (shared) line plan as built, at 256-row tiles in the caller's row order.  A rank's block keeps the 256-row tiles unless its lines
        // ask for more: larger tiles measured level on a block of the 304^3 stencil -- 0.1785 / 0.1791 / 0.1822 ms -- and a 512-row tile (the
        // pair's single-GPU size) = a whole sigma window always holds a padded chunk, i.e. no interior tile is left.  The caller's row order:
        // the tile classes below take tile t for rows [t * tile_rows, (t + 1) * tile_rows) -- a sweep plan's tiles are no row ranges -- and the
        // step kernel has no element plan.
        const uspmv_dev::TlcPlanOpts as_is{/*measure=*/false, /*elements=*/false, /*deal_rows=*/false, /*additive=*/false};
        rc = !ap                        ? uspmv_dev::dmat_optimize(pt[0].A, pt[0].scs, 0, as_is, &n_tiles, &n_staged)
             : k.kind == USPMV_AP_DP_SP ? uspmv_dev::dmat_optimize_ap(pt[0].A, pt[1].A, pt[0].scs, pt[1].scs, 0, as_is, &n_tiles, &n_staged)
                                        : uspmv_dev::dmat_optimize_ap_hp(pt[0].A, pt[1].A, pt[2].A, pt[0].scs, pt[1].scs, pt[2].scs, 0, as_is, &n_tiles, &n_staged);
    }
    // chunk classes over all parts
    const int64_t n_local = wsa[rank + 1] - wsa[rank];
    PartClasses pc;
    for (int q = 0; q < 3 && !rc; ++q) {
        if (!pt[q].scs) continue;
        std::vector<uint8_t> cq;
        int32_t pq = -1;
        if ((rc = uspmv_scs_classify_chunks(pt[q].scs, n_local, &cq, &pq))) break;
        pc.merge(cq, pq);
    }
    if (rc) return done(rc);
    return done(finish_setup(k, comm_id, comm_rank, comm_size, rank, P, C, pt, halo, o2n, pc, n_tiles, n_staged, opt, &D, out));
}

// setup_from_coo for a block that lives in HBM (d_I local row ids, d_J GLOBAL column ids, d_V; sorted by row): the same steps in the same
// order, each on the device -- uspmv_partition_precisions_device, uspmv_convert_to_scs_device_from_arrays with permute_cols = 0 (the first
// part with its own sigma ordering, the others with its old_to_new as fixed permutation; a part's COO copy is released once it is
// converted), uspmv_halo_discover_device with that permutation, the (shared) line plan from the handles' own arrays, and
// uspmv_dmat_chunk_classes_device per part.  Nothing of O(nnz) crosses to the host.  The object keeps the first part's layout-only struct
// (the permutations) as pt[0].scs; the other slots have none.
int setup_from_arrays(const CooSetup &k, const void *comm_id, int comm_rank, int comm_size, int rank, int P, const int32_t *d_I, const int32_t *d_J,
                      const double *d_V, int64_t nnz, int64_t n_cols, const int32_t *wsa, int64_t C, int64_t sigma, int tlc, int sort_mode,
                      const uspmv_dist_options_t *opt, void *stream, uspmv_dist_t **out) {
    const char *who = k.who;
    const bool ap = k.kind != uspmv_dist::ONE_PRECISION;
    if (!wsa || !out || nnz < 0 || (nnz > 0 && (!d_I || !d_J || !d_V))) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (P < 1 || rank < 0 || rank >= P) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad rank / P", who);
    if (k.refusal[0]) return uspmv::fail(USPMV_ERR_INVALID, "%s: %s", who, k.refusal);
    // (as in setup_from_coo: by all ranks alike, before the first collective)
    for (int p = 0; p < P; ++p)
        if (wsa[p + 1] <= wsa[p])
            return uspmv::fail(USPMV_ERR_INVALID, "%s: block %d of %d owns no rows (work_sharing_arr %d .. %d) -- fewer ranks or another partition%s", who, p, P,
                               (int)wsa[p], (int)wsa[p + 1], k.empty_tail);
    if (int rc = uspmv_dev::require_device()) return rc;
    const int64_t n_local = wsa[rank + 1] - wsa[rank];
    uspmv_dcoo_t *coo[3] = {nullptr, nullptr, nullptr};
    uspmv_dist::Part pt[3];
    uspmv_halo_t *halo = nullptr;
    uspmv_dist_t *D = nullptr;
    DeviceBuf<int32_t> d_o2n;
    auto free_coo = [&]() { for (auto *&c : coo) { uspmv_dcoo_free(c); c = nullptr; } };
    auto done = [&](int rc) {
        free_coo();
        if (rc == USPMV_OK) return rc;
        uspmv_dist_free(D);
        for (auto &p : pt) { uspmv_dmat_free(p.A); uspmv_scs_free(p.scs); }
        uspmv_halo_free(halo);
        return rc;
    };
    if (hipError_t e = d_o2n.alloc(4 * (size_t)n_local); e != hipSuccess) return uspmv::fail(USPMV_ERR_ALLOC, "%s: %s", who, hipGetErrorString(e));
    int rc = ap ? uspmv_partition_precisions_device(d_I, d_J, d_V, n_local, n_cols, nnz, k.kind, k.threshold_1, k.threshold_2, stream, coo) : USPMV_OK;
    for (int q = 0; q < 3 && !rc; ++q) {
        if (k.dtype[q] < 0) continue;
        const int32_t *I = d_I, *J = d_J;
        const double *V = d_V;
        int64_t n = nnz;
        uspmv_dcoo_t *&part = coo[k.kind == USPMV_AP_DP_SP && q == 1 ? 2 : q];   // (the partition hands the sp part of ap[dp_sp] out as its last)
        if (ap) rc = uspmv_dcoo_arrays(part, &I, &J, &V, &n);
        if (!rc) rc = uspmv_convert_to_scs_device_from_arrays(I, J, V, n_local, n_cols, n, C, sigma, k.dtype[q], q == 0 ? nullptr : d_o2n.get(), /*permute_cols=*/0,
                                                              sort_mode, stream, q == 0 ? &pt[0].scs : nullptr, q == 0 ? d_o2n.get() : nullptr, nullptr, &pt[q].A);
        uspmv_dcoo_free(part); part = nullptr;
    }
    uspmv_dmat_t *hs[3];
    int n_hs = 0;
    for (auto &p : pt) if (p.A) hs[n_hs++] = p.A;
    if (!rc) rc = uspmv_halo_discover_device(hs, n_hs, n_cols, wsa, rank, P, d_o2n, stream, &halo);
    int64_t n_tiles = 0, n_staged = 0;
    if (!rc && tlc) {
        // (the options of setup_from_coo, which says why)
        const uspmv_dev::TlcPlanOpts as_is{/*measure=*/false, /*elements=*/false, /*deal_rows=*/false, /*additive=*/false};
        uspmv_dmat_t *const shared[3] = {hs[0], n_hs > 1 ? hs[1] : nullptr, n_hs > 2 ? hs[2] : nullptr};
        rc = !ap ? uspmv_dev::dmat_optimize_device(pt[0].A, 0, as_is, &n_tiles, &n_staged) : uspmv_dev::dmat_optimize_device_shared(shared, &n_tiles, &n_staged, who);
    }
    PartClasses pc;
    for (int q = 0; q < 3 && !rc; ++q) {
        if (!pt[q].A) continue;
        std::vector<uint8_t> cq((size_t)pt[q].A->n_chunks);
        int32_t pq = -1;
        if ((rc = uspmv_dmat_chunk_classes_device(pt[q].A, n_local, cq.data(), &pq, stream))) break;
        pc.merge(cq, pq);
    }
    if (rc) return done(rc);
    return done(finish_setup(k, comm_id, comm_rank, comm_size, rank, P, C, pt, halo, pt[0].scs->old_to_new_idx.data(), pc, n_tiles, n_staged, opt, &D, out));
}

// ---- the self-check (uspmv_dist_check, uspmv_dist_check_arrays)

// The step of the check: x_perm[k] = x_global[wsa[rank] + new_to_old[k]] in the kernel's (permuted) order, halo tail and padding zero; y
// preset to a NaN pattern (a row nobody writes cannot pass); one step; hy = the padded y
int check_step(uspmv_dist *D, const int32_t *wsa, void *d_x, void *d_y, int use_graph, void *stream, std::vector<char> *hy) {
    const size_t vsz = vsize(D);
    hipStream_t st = (hipStream_t)stream;
    std::vector<char> hx((size_t)D->vec_len * vsz, 0);
    hy->resize((size_t)D->vec_len * vsz);
    const int32_t *n2o = D->scs->new_to_old_idx.data();
    for (int64_t k = 0; k < D->n_local; ++k) {
        const double v = uspmv::check_x((int64_t)wsa[D->rank] + n2o[k]);
        if (D->dtype == USPMV_F64) ((double *)hx.data())[k] = v; else ((float *)hx.data())[k] = (float)v;
    }
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(d_x, hx.data(), hx.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_y, 0xff, (size_t)D->n_rows_padded * vsz));
    if (int rc = uspmv_dist_run(D, d_x, d_y, 1, use_graph, stream)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(hy->data(), d_y, (size_t)D->n_rows_padded * vsz, hipMemcpyDeviceToHost));
    return USPMV_OK;
}

// ... and its verdict: y of the local rows in original order against ref (n_local values of the object's vector type), bitwise
void check_compare(const uspmv_dist *D, const std::vector<char> &hy, const char *ref, int64_t *mismatches, double *checksum) {
    const size_t vsz = vsize(D);
    const int32_t *o2n = D->scs->old_to_new_idx.data();
    int64_t bad = 0;
    double sum = 0.0;
    for (int64_t i = 0; i < D->n_local; ++i) {   // copy_back_result: y_orig[i] = y[old_to_new[i]] (code/utilities.hpp:3862)
        const char *got = hy.data() + (size_t)o2n[i] * vsz, *want = ref + (size_t)i * vsz;
        if (memcmp(got, want, vsz) != 0) ++bad;
        sum += D->dtype == USPMV_F64 ? *(const double *)got : (double)*(const float *)got;
    }
    if (mismatches) *mismatches = bad;
    if (checksum) *checksum = sum;
}

// The reference rows of uspmv_dist_check_arrays: one lane per local row; its entries are the run of row id `row` in the sorted I (two
// bisections), taken in entry order as ONE FMA chain from +0 (std::fma of host/dist_check.cpp = the fma instruction here: the calls
// below are the builtins, nothing is left to contraction).  VT double | float: value and x in VT.  AP (VT double): two chains, the dp one
// over |v| >= t1, the sp one over |v| < t1 with (double)(float)v, y = dp + sp (uspmv_partition_precisions's branch order; a NaN fits
// neither and raises flag 4).  xg: x_global by GLOBAL column, in VT.  flag 2: a column outside [0, n_glob).
template <typename VT, bool AP>
__global__ void __launch_bounds__(256) check_rows_kernel(const int *__restrict__ I, const int *__restrict__ J, const double *__restrict__ V, const long nnz,
                                                         const int n_local, const int n_glob, const VT *__restrict__ xg, const double t1,
                                                         VT *__restrict__ y_ref, int *__restrict__ flag) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_local) return;
    auto lower = [&](const int key) {                     // first k with I[k] >= key
        long lo = 0, hi = nnz;
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (I[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const long k0 = lower(row), k1 = lower(row + 1);
    VT a = VT(0), b = VT(0);
    int err = 0;
    for (long k = k0; k < k1; ++k) {
        const int j = J[k];
        if (j < 0 || j >= n_glob) { err |= 2; continue; }
        const double v = V[k];
        if constexpr (AP) {
            const double av = __builtin_fabs(v);
            if (av >= t1) a = __builtin_fma(v, xg[j], a);
            else if (av < t1) b = __builtin_fma((double)(float)v, xg[j], b);
            else err |= 4;
        } else if constexpr (sizeof(VT) == 8) {
            a = __builtin_fma(v, xg[j], a);
        } else {
            a = __builtin_fmaf((float)v, xg[j], a);
        }
    }
    y_ref[row] = AP ? a + b : a;
    if (err) atomicOr(flag, err);
}

}  // namespace

extern "C" {

int uspmv_dist_create_from_coo_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                  const int32_t *wsa, int64_t C, int64_t sigma, int dtype, int tlc, const uspmv_dist_options_t *opt,
                                  uspmv_dist_t **out) {
    char bad[32] = "";
    if (dtype != USPMV_F64 && dtype != USPMV_F32) snprintf(bad, sizeof bad, "unknown dtype %d", dtype);
    const CooSetup k{"uspmv_dist_create_from_coo", uspmv_dist::ONE_PRECISION, {dtype, -1, -1}, 0.0, 0.0, bad,
                     " (the reference's seg methods only repair an empty LAST block, code/mpi_funcs.hpp:602-606)"};
    return setup_from_coo(k, comm_id, comm_rank, comm_size, rank, P, local, wsa, C, sigma, tlc, opt, out);
}

// ... for an ap[dp_sp] pair: the dp part, the sp part
int uspmv_dist_create_ap_from_coo_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                     const int32_t *wsa, int64_t C, int64_t sigma, double threshold_1, int tlc,
                                     const uspmv_dist_options_t *opt, uspmv_dist_t **out) {
    const CooSetup k{"uspmv_dist_create_ap_from_coo", USPMV_AP_DP_SP, {USPMV_F64, USPMV_F32, -1}, threshold_1, 0.0, "", ""};
    return setup_from_coo(k, comm_id, comm_rank, comm_size, rank, P, local, wsa, C, sigma, tlc, opt, out);
}

// ... for the kinds with an fp16 part: the hi part (float for ap[sp_hp]), the float part of ap[dp_sp_hp], the fp16 part
int uspmv_dist_create_ap_hp_from_coo_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                        const int32_t *wsa, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2, int tlc,
                                        const uspmv_dist_options_t *opt, uspmv_dist_t **out) {
    char bad[96] = "";
    if (kind == USPMV_AP_DP_SP) snprintf(bad, sizeof bad, "ap[dp_sp] has no fp16 part; its object is made by uspmv_dist_create_ap_from_coo");
    else if (kind != USPMV_AP_DP_HP && kind != USPMV_AP_SP_HP && kind != USPMV_AP_DP_SP_HP) snprintf(bad, sizeof bad, "unknown kind %d", kind);
    const CooSetup k{"uspmv_dist_create_ap_hp_from_coo", kind, {kind == USPMV_AP_SP_HP ? USPMV_F32 : USPMV_F64, kind == USPMV_AP_DP_SP_HP ? USPMV_F32 : -1, USPMV_F16},
                     threshold_1, threshold_2, bad, ""};
    return setup_from_coo(k, comm_id, comm_rank, comm_size, rank, P, local, wsa, C, sigma, tlc, opt, out);
}

int uspmv_dist_create_from_coo(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                               const int32_t *wsa, int64_t C, int64_t sigma, int dtype, int tlc, uspmv_dist_t **out) {
    return uspmv_dist_create_from_coo_ex(comm_id, comm_rank, comm_size, rank, P, local, wsa, C, sigma, dtype, tlc, nullptr, out);
}

int uspmv_dist_create_ap_from_coo(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                  const int32_t *wsa, int64_t C, int64_t sigma, double threshold_1, int tlc, uspmv_dist_t **out) {
    return uspmv_dist_create_ap_from_coo_ex(comm_id, comm_rank, comm_size, rank, P, local, wsa, C, sigma, threshold_1, tlc, nullptr, out);
}

int uspmv_dist_create_ap_hp_from_coo(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const uspmv_coo_t *local,
                                     const int32_t *wsa, int64_t C, int64_t sigma, int kind, double threshold_1, double threshold_2, int tlc,
                                     uspmv_dist_t **out) {
    return uspmv_dist_create_ap_hp_from_coo_ex(comm_id, comm_rank, comm_size, rank, P, local, wsa, C, sigma, kind, threshold_1, threshold_2, tlc, nullptr, out);
}

// ... from a block in HBM, for every kind of object
int uspmv_dist_create_from_arrays_ex(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const int32_t *d_I, const int32_t *d_J,
                                     const double *d_V, int64_t nnz, int64_t n_cols, const int32_t *wsa, int64_t C, int64_t sigma, int kind, int dtype,
                                     double threshold_1, double threshold_2, int tlc, int sort_mode, const uspmv_dist_options_t *opt, void *stream,
                                     uspmv_dist_t **out) {
    const char *who = "uspmv_dist_create_from_arrays";
    char bad[48] = "";
    if (kind == USPMV_ONE_PRECISION) {
        if (dtype != USPMV_F64 && dtype != USPMV_F32) snprintf(bad, sizeof bad, "unknown dtype %d", dtype);
        const CooSetup k{who, uspmv_dist::ONE_PRECISION, {dtype, -1, -1}, 0.0, 0.0, bad,
                         " (the reference's seg methods only repair an empty LAST block, code/mpi_funcs.hpp:602-606)"};
        return setup_from_arrays(k, comm_id, comm_rank, comm_size, rank, P, d_I, d_J, d_V, nnz, n_cols, wsa, C, sigma, tlc, sort_mode, opt, stream, out);
    }
    if (kind != USPMV_AP_DP_SP && kind != USPMV_AP_DP_HP && kind != USPMV_AP_SP_HP && kind != USPMV_AP_DP_SP_HP) snprintf(bad, sizeof bad, "unknown kind %d", kind);
    const bool hp = kind != USPMV_AP_DP_SP;
    const CooSetup k{who, kind, {kind == USPMV_AP_SP_HP ? USPMV_F32 : USPMV_F64, kind == USPMV_AP_DP_SP_HP || !hp ? USPMV_F32 : -1, hp ? USPMV_F16 : -1},
                     threshold_1, hp ? threshold_2 : 0.0, bad, ""};
    return setup_from_arrays(k, comm_id, comm_rank, comm_size, rank, P, d_I, d_J, d_V, nnz, n_cols, wsa, C, sigma, tlc, sort_mode, opt, stream, out);
}

int uspmv_dist_create_from_arrays(const void *comm_id, int comm_rank, int comm_size, int rank, int P, const int32_t *d_I, const int32_t *d_J,
                                  const double *d_V, int64_t nnz, int64_t n_cols, const int32_t *wsa, int64_t C, int64_t sigma, int kind, int dtype,
                                  double threshold_1, double threshold_2, int tlc, int sort_mode, void *stream, uspmv_dist_t **out) {
    return uspmv_dist_create_from_arrays_ex(comm_id, comm_rank, comm_size, rank, P, d_I, d_J, d_V, nnz, n_cols, wsa, C, sigma, kind, dtype, threshold_1,
                                            threshold_2, tlc, sort_mode, nullptr, stream, out);
}

int uspmv_dist_comm_plan(const uspmv_dist_t *D, int64_t *n_send, const int64_t **send_off, const int32_t **send_idxs, const int64_t **recv_off) {
    if (!D || !D->plan) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_comm_plan: NULL argument");
    return uspmv_comm_plan_meta(D->plan, n_send, send_off, send_idxs, recv_off);
}

int uspmv_dist_set_option(uspmv_dist_t *D, const char *key, int value) {
    if (!D || !key) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_set_option: NULL argument");
    const std::string k(key);
    if (is_ap(D) && (((k == "fused_step" || k == "autotune_all") && value != 0) || (k == "block_plan" && value > 0)))
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "uspmv_dist_set_option: '%s' is not available on an adaptive-precision (%s) object: its step has "
                           "the overlap, plain and pad_split forms%s", key, ap_name(D),
                           has_hp(D) ? "; block vectors run through uspmv_dist_spmmv_ap_hp" : "; block vectors run through uspmv_dist_spmmv_ap");
    if (k == "overlap") { if ((value != 0) != D->overlap) drop_graph(D); D->overlap = value != 0; }
    else if (k == "no_pack") { if ((value != 0) != D->no_pack) drop_graph(D); D->no_pack = value != 0; }
    else if (k == "ba_synch") { if ((value != 0) != D->ba_synch) drop_graph(D); D->ba_synch = value != 0; }
    else if (k == "fused_step") { if ((value != 0) != D->fused) drop_graph(D); D->fused = value != 0; }
    else if (k == "pad_split") { if ((value != 0) != D->pad_split) drop_graph(D); D->pad_split = value != 0; }
    else if (k == "autotune_all") D->autotune_all = value != 0;
    else if (k == "diag_spmmv_part") {
        if (value < 0 || value > 2) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_set_option: diag_spmmv_part is 0 (both), 1 (interior only) or 2 (boundary only)");
        D->diag_spmmv_part = value;
    }
    else if (k == "block_plan") {
        // the phased block plan for block vectors of `value` columns on the rank's matrix (64-byte X rows: dp 8, sp 16; other widths
        // and shapes the planner turns down keep the gather kernels) + its interior / boundary tiles.  0: drop the plan.
        if (value < 0) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_set_option: block_plan takes a block width >= 0");
        D->plan_b = 0; D->plan_bnd_tiles = 0;
        int64_t nt = 0, ns = 0;
        if (value == 0) { uspmv_dev::block_plan_reset(D->A); return USPMV_OK; }
        // (a layout-only struct -- an object made from device arrays -- has no entries for the host planner)
        int rc = D->scs && uspmv::scs_has_entries(D->scs) ? uspmv_dmat_optimize_block(D->A, D->scs, value, &nt, &ns)
                                                          : uspmv_dmat_optimize_block_device(D->A, value, &nt, &ns);
        if (rc) return rc;
        if (D->A->pb.on) {
            D->plan_b = value;
            if (D->parts) rc = uspmv_dev::dmat_part_set_plan(D->A, (long)D->n_local, &D->plan_bnd_tiles);
        }
        return rc;
    }
    else if (k == "capture_mode") {
        if (value < 0 || value > 2) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_set_option: capture_mode is 0 (global), 1 (thread-local) or 2 (relaxed)");
        D->capture_mode = value == 0 ? hipStreamCaptureModeGlobal : value == 1 ? hipStreamCaptureModeThreadLocal : hipStreamCaptureModeRelaxed;
        drop_graph(D); D->graph_failed = false;
    }
    else if (k == "diag_skip_exchange") { drop_graph(D); D->diag_skip_exchange = value != 0; }
    else if (k == "diag_peer_skew") D->diag_peer_skew = value != 0;
    else return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_set_option: unknown key '%s'", key);
    return USPMV_OK;
}

int uspmv_dist_comm_count(const uspmv_dist_t *D, int *n_ranks) {
    if (!D || !n_ranks) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_comm_count: NULL argument");
    *n_ranks = 0;                                                   // (host-staged / peer-store exchange: no RCCL communicator exists)
    if (D->comm) NCCL_TRY(ncclCommCount(D->comm, n_ranks));
    return USPMV_OK;
}

int uspmv_dist_exchange(const uspmv_dist_t *D, int *exchange) {
    if (!D || !exchange) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_exchange: NULL argument");
    *exchange = D->exchange;
    return USPMV_OK;
}

int uspmv_dist_pad_info(const uspmv_dist_t *D, int64_t meta[4]) {
    if (!D || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_pad_info: NULL argument");
    int reruns = 0, r2 = 0;
    if (D->d_scratch) HIP_TRY(hipMemcpy(&reruns, D->d_scratch + 2, 4, hipMemcpyDeviceToHost));
    if (D->d_ss) { HIP_TRY(hipMemcpy(&r2, &D->d_ss.get()->reruns, 4, hipMemcpyDeviceToHost)); reruns += r2; }
    meta[0] = D->n_pad; meta[1] = D->n_pad ? D->n_bnd_real : D->n_bnd; meta[2] = D->pad_col; meta[3] = reruns;
    return USPMV_OK;
}

int uspmv_dist_spmmv_info(const uspmv_dist_t *D, int64_t meta[6]) {
    if (!D || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_spmmv_info: NULL argument");
    meta[0] = D->spmmv_two_part; meta[1] = D->spmmv_one_part; meta[2] = D->A->pb.on ? D->plan_b : 0; meta[3] = D->A->pb.on ? D->A->pb.n_tiles : 0;
    meta[4] = D->A->pb.on ? D->plan_bnd_tiles : 0; meta[5] = D->parts && !D->A->alt;
    return USPMV_OK;
}

int uspmv_dist_info(const uspmv_dist_t *D, int64_t meta[12]) {
    if (!D || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_info: NULL argument");
    meta[0] = D->n_local; meta[1] = D->n_halo; meta[2] = D->vec_len; meta[3] = D->n_send; meta[4] = D->n_int; meta[5] = D->n_bnd;
    meta[6] = D->tiles; meta[7] = D->n_rows_padded; meta[8] = D->loopback; meta[9] = D->gexec != nullptr; meta[10] = D->graph_launches;
    meta[11] = D->eager_steps;
    return USPMV_OK;
}

int uspmv_dist_parts(const uspmv_dist_t *D, const uspmv_scs_t **scs, const uspmv_dmat_t **A, const uspmv_halo_t **halo) {
    if (!D) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_parts: NULL argument");
    if (scs) *scs = D->scs;
    if (A) *A = D->A;
    if (halo) *halo = D->halo;
    return USPMV_OK;
}

int uspmv_dist_parts_ap(const uspmv_dist_t *D, const uspmv_scs_t **scs_dp, const uspmv_scs_t **scs_sp, const uspmv_dmat_t **A_dp,
                        const uspmv_dmat_t **A_sp, const uspmv_halo_t **halo) {
    if (!D) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_parts_ap: NULL argument");
    if (has_hp(D)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_parts_ap: an %s object (its parts: uspmv_dist_parts_ap_hp)", ap_name(D));
    if (scs_dp) *scs_dp = D->pt[0].scs;
    if (scs_sp) *scs_sp = D->pt[1].scs;
    if (A_dp) *A_dp = D->pt[0].A;
    if (A_sp) *A_sp = D->pt[1].A;
    if (halo) *halo = D->halo;
    return USPMV_OK;
}

int uspmv_dist_parts_ap_hp(const uspmv_dist_t *D, int *kind, const uspmv_scs_t **scs_hi, const uspmv_scs_t **scs_mid, const uspmv_scs_t **scs_hp,
                           const uspmv_dmat_t **A_hi, const uspmv_dmat_t **A_mid, const uspmv_dmat_t **A_hp, const uspmv_halo_t **halo) {
    if (!D) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_parts_ap_hp: NULL argument");
    if (!has_hp(D)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_parts_ap_hp: not an object made by uspmv_dist_create_ap_hp_from_coo");
    if (kind) *kind = D->kind;
    if (scs_hi) *scs_hi = D->pt[0].scs;
    if (scs_mid) *scs_mid = D->pt[1].scs;
    if (scs_hp) *scs_hp = D->pt[2].scs;
    if (A_hi) *A_hi = D->pt[0].A;
    if (A_mid) *A_mid = D->pt[1].A;
    if (A_hp) *A_hp = D->pt[2].A;
    if (halo) *halo = D->halo;
    return USPMV_OK;
}

int uspmv_dist_set_overlap(uspmv_dist_t *D, int overlap) {
    if (!D) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_set_overlap: NULL argument");
    if ((overlap != 0) != D->overlap) drop_graph(D);
    D->overlap = overlap != 0;
    return USPMV_OK;
}

int uspmv_dist_set_no_pack(uspmv_dist_t *D, int no_pack) {
    if (!D) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_set_no_pack: NULL argument");
    if ((no_pack != 0) != D->no_pack) drop_graph(D);
    D->no_pack = no_pack != 0;
    return USPMV_OK;
}

int uspmv_dist_spmv(uspmv_dist_t *D, void *d_x, void *d_y, int comm_halos, void *stream) {
    if (!D || !d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_spmv: NULL argument");
    ++D->eager_steps;
    return step(D, d_x, d_y, (hipStream_t)stream, comm_halos != 0);
}

int uspmv_dist_run(uspmv_dist_t *D, void *d_x, void *d_y, int n_steps, int use_graph, void *stream) {
    if (!D || !d_x || !d_y || n_steps < 0) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_run: bad argument");
    hipStream_t main = (hipStream_t)stream;
    if (use_graph && D->P > 1 && !D->graph_failed && !eager_only(D)) {   // (the host-staged / peer-store exchange blocks the host: nothing to capture)
        if (!main) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_run: graph replay needs an explicit (non-default) stream");
        if (!D->gexec || D->g_x != d_x || D->g_y != d_y || D->g_stream != main) {
            // RCCL sets up its p2p channels at the first use of a pair: one eager step before the capture
            if (int rc = step(D, d_x, d_y, main, true)) return rc;
            HIP_TRY(hipStreamSynchronize(main));
            if (capture(D, d_x, d_y, main) != USPMV_OK) {
                D->graph_failed = true;
                if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] dist: graph capture unavailable (%s); eager steps\n", uspmv_last_error());
            }
        }
        if (D->gexec) {
            DBG("launching");
            for (int k = 0; k < n_steps; ++k) HIP_TRY(hipGraphLaunch(D->gexec, main));
            DBG("launched");
            D->graph_launches += n_steps;
            return USPMV_OK;
        }
    }
    for (int k = 0; k < n_steps; ++k)
        if (int rc = step(D, d_x, d_y, main, true)) return rc;
    D->eager_steps += n_steps;
    return USPMV_OK;
}

// How the step should be arranged around the exchange depends on what the exchange costs next to the kernel on the machine at hand
// (one GPU cannot tell for real links): time the arrangements and keep the fastest.  Collective: every rank must call it; the ranks
// agree on the slowest rank's clock through one all-reduce per measurement, so all take the same decision.
int uspmv_dist_autotune(uspmv_dist_t *D, void *d_x, void *d_y, int use_graph, const uspmv_coo_t *local, const int32_t *wsa, void *stream, int *form,
                        double ms[4]) {
    if (!D || !d_x || !d_y || !form || !ms) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_autotune: NULL argument");
    for (int k = 0; k < 4; ++k) ms[k] = 0;
    *form = USPMV_STEP_OVERLAP;
    if (D->P < 2) return USPMV_OK;
    hipStream_t st = (hipStream_t)stream;
    auto apply = [&](int f) -> int {
        if (int rc = uspmv_dist_set_option(D, "overlap", f == USPMV_STEP_PLAIN ? 0 : 1)) return rc;
        // (an ap object times overlap | plain only, and its overlap form keeps the "pad_split" it has -- 1 unless the caller changed it)
        if (is_ap(D)) return USPMV_OK;
        if (int rc = uspmv_dist_set_option(D, "pad_split", f == USPMV_STEP_PAD || f == USPMV_STEP_FUSED ? 1 : 0)) return rc;
        return uspmv_dist_set_option(D, "fused_step", f == USPMV_STEP_FUSED ? 1 : 0);
    };
    // Candidates: the two arrangements every run has executed (overlap | plain).  The padding-tile and one-launch forms have only ever
    // run next to an exchange on the SAME GPU (loopback / host-staged), where they measured slower; they are timed only on request
    // ("autotune_all" 1, -step_form auto_all) until a run with real peers has shown what they are worth.
    std::vector<int> cand = {USPMV_STEP_OVERLAP, USPMV_STEP_PLAIN};
    if (D->autotune_all) {
        cand.push_back(USPMV_STEP_PAD);
        if (!use_graph || eager_only(D)) cand.push_back(USPMV_STEP_FUSED);      // (a captured step never takes the one-launch form)
    }
    // every collective the measurement uses once before anything is timed (RCCL sets its channels up lazily, 40 ms the first time), and two
    // rounds over the candidates of which the faster counts: the first candidate must not pay for a cold start
    { double warm = 0; if (int rc = uspmv_dist_barrier(D, st)) return rc; if (int rc = uspmv_dist_allreduce_max(D, &warm, st)) return rc; }
    for (int round = 0; round < 2; ++round)
        for (int f : cand) {
            if (int rc = apply(f)) return rc;
            if (int rc = uspmv_dist_run(D, d_x, d_y, 10, use_graph, st)) return rc;
            HIP_TRY(hipStreamSynchronize(st));
            if (int rc = uspmv_dist_barrier(D, st)) return rc;
            const auto t0 = std::chrono::steady_clock::now();
            if (int rc = uspmv_dist_run(D, d_x, d_y, 40, use_graph, st)) return rc;
            HIP_TRY(hipStreamSynchronize(st));
            if (int rc = uspmv_dist_barrier(D, st)) return rc;
            double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / 40 * 1e3;
            if (int rc = uspmv_dist_allreduce_max(D, &t, st)) return rc;
            ms[f] = round == 0 ? t : std::min(ms[f], t);
        }
    int best = cand[0];
    for (int f : cand) if (ms[f] < ms[best]) best = f;
    if (int rc = apply(best)) return rc;
    // an arrangement beyond the two plain ones is only kept if one step of it passes the bitwise self-check on every rank (collective: all
    // ranks reach the same verdict); otherwise the faster of overlap / plain takes over and ms[] of the rejected form is negated
    if ((best == USPMV_STEP_PAD || best == USPMV_STEP_FUSED) && local && wsa) {
        int64_t mm = 0;
        DeviceBuf<void> keep;                                           // (the check runs on its own x: put the caller's local part back afterwards)
        const size_t xb = vsize(D) * (size_t)std::max<int64_t>(D->n_local, 1);
        HIP_TRY(keep.alloc(xb));
        HIP_TRY(hipMemcpyAsync(keep, d_x, xb, hipMemcpyDeviceToDevice, st));
        const int rc_check = uspmv_dist_check(D, local, wsa, d_x, d_y, use_graph, stream, &mm, nullptr);
        HIP_TRY(hipMemcpyAsync(d_x, keep, xb, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (rc_check) return rc_check;
        std::vector<int64_t> all((size_t)std::max(D->P, D->comm_size), 0);
        if (int rc = uspmv_dist_allgather_i64(D, mm, all.data(), stream)) return rc;
        int64_t tot = 0;
        for (int p = 0; p < (D->loopback ? 1 : D->comm_size); ++p) tot += all[(size_t)p];
        if (tot) {
            ms[best] = -ms[best];
            best = ms[USPMV_STEP_PLAIN] < ms[USPMV_STEP_OVERLAP] ? USPMV_STEP_PLAIN : USPMV_STEP_OVERLAP;
            if (int rc = apply(best)) return rc;
        }
    }
    *form = best;
    return USPMV_OK;
}

int uspmv_dist_barrier(uspmv_dist_t *D, void *stream) {
    if (!D) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_barrier: NULL argument");
    if (!D->comm) {                                                  // no RCCL communicator: over the transport
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return D->tr.barrier ? D->tr.barrier(D->tr.ctx) : USPMV_OK;
    }
    NCCL_TRY(ncclAllReduce(D->d_scratch, D->d_scratch + 1, 1, ncclInt32, ncclSum, D->comm, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return USPMV_OK;
}

int uspmv_dist_allreduce_max(uspmv_dist_t *D, double *value, void *stream) {
    if (!D || !value) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_allreduce_max: NULL argument");
    if (!D->comm) {
        if (!D->tr.allgather) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "uspmv_dist_allreduce_max: the transport has no all-gather");
        std::vector<double> all((size_t)D->P, *value);
        if (int rc = D->tr.allgather(D->tr.ctx, value, all.data(), 8)) return rc;
        for (double v : all) *value = std::max(*value, v);
        return USPMV_OK;
    }
    double *d_t = (double *)(D->d_scratch + 16);
    HIP_TRY(hipMemcpy(d_t, value, 8, hipMemcpyHostToDevice));
    NCCL_TRY(ncclAllReduce(d_t, d_t, 1, ncclDouble, ncclMax, D->comm, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(value, d_t, 8, hipMemcpyDeviceToHost));
    return USPMV_OK;
}

int uspmv_dist_allgather_i64(uspmv_dist_t *D, int64_t value, int64_t *all, void *stream) {
    if (!D || !all) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_allgather_i64: NULL argument");
    if (D->loopback) { for (int p = 0; p < D->P; ++p) all[p] = value; return USPMV_OK; }
    if (!D->comm) {
        if (!D->tr.allgather) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "uspmv_dist_allgather_i64: the transport has no all-gather");
        return D->tr.allgather(D->tr.ctx, &value, all, 8);
    }
    DeviceBuf<int64_t> d_v, d_all;
    HIP_TRY(d_v.alloc(8));
    HIP_TRY(d_all.alloc(8 * (size_t)D->comm_size));
    HIP_TRY(hipMemcpy(d_v, &value, 8, hipMemcpyHostToDevice));
    NCCL_TRY(ncclAllGather(d_v, d_all, 1, ncclInt64, D->comm, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(all, d_all, 8 * (size_t)D->comm_size, hipMemcpyDeviceToHost));
    return USPMV_OK;
}

// Self-check of the distributed path on the object's own matrix (include/uspmv.h): x_global[j] = 1 + 1e-3 * (j mod 1000), one
// step, y of the local rows compared bitwise with the entry-ordered FMA chains of the block's COO (host/dist_check.cpp).
int uspmv_dist_check(uspmv_dist_t *D, const uspmv_coo_t *local, const int32_t *wsa, void *d_x, void *d_y, int use_graph, void *stream,
                     int64_t *mismatches, double *checksum) {
    if (!D || !local || !wsa || !d_x || !d_y) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_check: NULL argument");
    if (!D->scs) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_check: needs an object made by uspmv_dist_create_from_coo (it owns the row permutation)");
    if (local->n_rows != D->n_local || wsa[D->rank + 1] - wsa[D->rank] != D->n_local)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_check: the COO block has %ld rows, the object %ld", (long)local->n_rows, (long)D->n_local);
    std::vector<char> hy;
    if (int rc = check_step(D, wsa, d_x, d_y, use_graph, stream, &hy)) return rc;
    std::vector<char> ref((size_t)std::max<int64_t>(D->n_local, 1) * vsize(D));
    if (int rc = has_hp(D) ? uspmv::dist_reference_rows_ap_hp(local, wsa, D->P, D->rank, D->loopback, D->kind, D->ap_threshold, D->ap_threshold_2, ref.data())
                 : is_ap(D) ? uspmv::dist_reference_rows_ap(local, wsa, D->P, D->rank, D->loopback, D->ap_threshold, (double *)ref.data())
                            : uspmv::dist_reference_rows(local, wsa, D->P, D->rank, D->loopback, D->dtype, ref.data()))
        return rc;
    check_compare(D, hy, ref.data(), mismatches, checksum);
    return USPMV_OK;
}

// ... against a block that lives in HBM: the reference rows by check_rows_kernel from the device arrays, over an x_global evaluated on the
// host exactly as dist_reference_rows evaluates it (check_x of check_col: in loopback a halo column reads this block's own row) and
// uploaded in the vector type -- O(columns), and the device never re-derives that expression
int uspmv_dist_check_arrays(uspmv_dist_t *D, const int32_t *d_I, const int32_t *d_J, const double *d_V, int64_t nnz, const int32_t *wsa, void *d_x,
                            void *d_y, int use_graph, void *stream, int64_t *mismatches, double *checksum) {
    const char *who = "uspmv_dist_check_arrays";
    if (!D || !wsa || !d_x || !d_y || nnz < 0 || (nnz > 0 && (!d_I || !d_J || !d_V))) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (has_hp(D)) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: not available on an %s object (its check is uspmv_dist_check, on the host block)", who, ap_name(D));
    if (!D->scs) return uspmv::fail(USPMV_ERR_INVALID, "%s: needs an object made by uspmv_dist_create_from_coo / _from_arrays (it owns the row permutation)", who);
    if (wsa[D->rank + 1] - wsa[D->rank] != D->n_local)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: work_sharing_arr gives this rank %ld rows, the object has %ld", who, (long)(wsa[D->rank + 1] - wsa[D->rank]), (long)D->n_local);
    const size_t vsz = vsize(D);
    const int64_t nl = D->n_local, n_glob = wsa[D->P];
    hipStream_t st = (hipStream_t)stream;
    std::vector<char> hy;
    if (int rc = check_step(D, wsa, d_x, d_y, use_graph, stream, &hy)) return rc;
    std::vector<char> xg((size_t)std::max<int64_t>(n_glob, 1) * vsz);
    for (int64_t j = 0; j < n_glob; ++j) {
        const double v = uspmv::check_x(uspmv::check_col(j, wsa, D->P, D->rank, D->loopback));
        if (D->dtype == USPMV_F64) ((double *)xg.data())[j] = v; else ((float *)xg.data())[j] = (float)v;
    }
    DeviceBuf<void> d_xg, d_ref;
    DeviceBuf<int> d_flag;
    HIP_TRY(d_xg.upload(xg.data(), xg.size()));
    HIP_TRY(d_ref.alloc((size_t)nl * vsz));
    HIP_TRY(d_flag.zeros(4));
    const dim3 grid((unsigned)((nl + 255) / 256)), block(256);
    if (is_ap(D))
        hipLaunchKernelGGL((check_rows_kernel<double, true>), grid, block, 0, st, d_I, d_J, d_V, (long)nnz, (int)nl, (int)n_glob, (const double *)d_xg.get(), D->ap_threshold, (double *)d_ref.get(), d_flag.get());
    else if (D->dtype == USPMV_F64)
        hipLaunchKernelGGL((check_rows_kernel<double, false>), grid, block, 0, st, d_I, d_J, d_V, (long)nnz, (int)nl, (int)n_glob, (const double *)d_xg.get(), 0.0, (double *)d_ref.get(), d_flag.get());
    else
        hipLaunchKernelGGL((check_rows_kernel<float, false>), grid, block, 0, st, d_I, d_J, d_V, (long)nnz, (int)nl, (int)n_glob, (const float *)d_xg.get(), 0.0, (float *)d_ref.get(), d_flag.get());
    HIP_TRY(hipGetLastError());
    std::vector<char> ref((size_t)std::max<int64_t>(nl, 1) * vsz);
    int h_flag = 0;
    HIP_TRY(hipMemcpyAsync(ref.data(), d_ref, (size_t)nl * vsz, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_flag & 2) return uspmv::fail(USPMV_ERR_INVALID, "%s: a column index lies outside the global matrix (work_sharing_arr ends at %ld)", who, (long)n_glob);
    if (h_flag & 4) return uspmv::fail(USPMV_ERR_INVALID, "%s: an element fits neither part", who);
    check_compare(D, hy, ref.data(), mismatches, checksum);
    return USPMV_OK;
}

int uspmv_dist_spmmv(uspmv_dist_t *D, void *d_X, void *d_Y, int b, int layout, int mode, int comm_halos, void *stream) {
    if (!D || !d_X || !d_Y || b < 1) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_spmmv: bad argument");
    if (is_ap(D))
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "uspmv_dist_spmmv: not available on an adaptive-precision (%s) object (%s)", ap_name(D),
                           has_hp(D) ? "its block step is uspmv_dist_spmmv_ap_hp" : "its block step is uspmv_dist_spmmv_ap");
    if (layout != USPMV_COLWISE && layout != USPMV_ROWWISE) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_spmmv: unknown layout %d", layout);
    if (mode != USPMV_BULKVEC && mode != USPMV_MULTIVEC && mode != USPMV_SINGLEVEC) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dist_spmmv: unknown mode %d", mode);
    if (layout == USPMV_ROWWISE && mode != USPMV_BULKVEC)
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "uspmv_dist_spmmv: row-wise block vectors travel in one message per neighbour (bulkvec) only");
    hipStream_t main = (hipStream_t)stream;
    if (!(D->P > 1 && comm_halos)) return uspmv_spmmv(D->A, d_X, d_Y, b, D->vec_len, layout, stream);
    auto grow_and_exchange = [&]() -> int { return block_exchange(D, d_X, b, layout, mode, main, "uspmv_dist_spmmv"); };
    // (a handle whose only block plan is the one-list-per-tile one runs that plan's kernels on the whole matrix: they are ahead of the
    //  gather kernels by more than the exchange costs)
    if (!(D->overlap && D->parts && !D->A->alt) || (D->A->bt.on && !(D->A->pb.on && D->A->part_len[1][0]))) {
        // exchange first, then the whole matrix (the reference's order, code/mpi_funcs.hpp:25-60)
        if (int rc = grow_and_exchange()) return rc;
        if (int rc = uspmv_spmmv(D->A, d_X, d_Y, b, D->vec_len, layout, stream)) return rc;
        ++D->spmmv_one_part;
        return step_barrier(D, main);
    }
    // Two parts, as the single-vector step: the chunks (plan tiles) that touch no halo row run on the side stream while the
    // exchange is under way on the caller's stream, the others after it.  A part is the same kernel over chunk lengths in which the
    // other part's chunks are marked (uspmv_dmat::part_len), so every row's FMA chain is what the one-part step computes.
    // Column-wise X: the interior part re-lays out the local rows into the handle's row-major workspace, the boundary part the
    // halo rows once they have arrived.
    uspmv_dmat_t *A = D->A;
    struct PartGuard { uspmv_dmat_t *A; ~PartGuard() { A->part = 0; } } guard{A};
    A->part_split = (long)D->n_local;
    HIP_TRY(hipEventRecord(D->ev_main, main));
    HIP_TRY(hipStreamWaitEvent(D->side_stream, D->ev_main, 0));
    A->part = 1;
    if (D->diag_spmmv_part != 2)
        if (int rc = uspmv_spmmv(A, d_X, d_Y, b, D->vec_len, layout, D->side_stream)) return rc;
    HIP_TRY(hipEventRecord(D->ev_comm, D->side_stream));
    if (int rc = grow_and_exchange()) return rc;
    HIP_TRY(hipStreamWaitEvent(main, D->ev_comm, 0));
    A->part = 2;
    if (D->diag_spmmv_part != 1)
        if (int rc = uspmv_spmmv(A, d_X, d_Y, b, D->vec_len, layout, main)) return rc;
    ++D->spmmv_two_part;
    return step_barrier(D, main);
}

// The block step of an adaptive-precision object, behind uspmv_dist_spmmv_ap (ap[dp_sp]) and uspmv_dist_spmmv_ap_hp (the kinds with an fp16
// part).  Unlike the dp object's two-part step (marked chunk-length arrays, uspmv_dmat::part_len) the parts here are the single-vector
// step's own tile (chunk) lists run by the list forms of the kind's block kernels, so "pad_split" carries over: see pad_keep_block_kernel.
// X and Y are in the object's vector type (float for ap[sp_hp]).
static int ap_block_step(uspmv_dist_t *D, void *d_X, void *d_Y, int b, int layout, int mode, int comm_halos, void *stream, const char *who) {
    if (layout == USPMV_ROWWISE && mode != USPMV_BULKVEC)
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: row-wise block vectors travel in one message per neighbour (bulkvec) only", who);
    hipStream_t main = (hipStream_t)stream;
    if (b == 1) { ++D->eager_steps; return step(D, d_X, d_Y, main, comm_halos != 0); }
    const int64_t ld = D->vec_len;
    const uspmv_dist::Part *p = D->pt;
    const bool hp = has_hp(D);
    auto whole_b = [&]() -> int {
        return hp ? uspmv_spmmv_ap_hp(p[0].A, p[1].A, p[2].A, d_X, d_Y, b, ld, layout, stream) : uspmv_spmmv_ap(p[0].A, p[1].A, d_X, d_Y, b, ld, layout, stream);
    };
    if (!(D->P > 1 && comm_halos)) return whole_b();
    if ((int64_t)b * std::max(ld, (int64_t)1) > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: b * padded_vec_size exceeds int32", who);
    if (!D->overlap) {
        if (int rc = block_exchange(D, d_X, b, layout, mode, main, who)) return rc;
        if (int rc = whole_b()) return rc;
        ++D->spmmv_one_part;
        return step_barrier(D, main);
    }
    const bool pads = pads_on(D);
    const int rowwise = layout == USPMV_ROWWISE;
    if (pads && b > D->stale_b) {
        HIP_TRY(D->d_stale_b.zeros(sizeof(double) * (size_t)b));
        D->stale_b = b;
    }
    auto part_b = [&](const int32_t *ids, int64_t n, hipStream_t st) -> int {
        if (n == 0) return USPMV_OK;
        if (hp)
            return D->tiles ? uspmv_spmmv_ap_hp_tiles(p[0].A, p[1].A, p[2].A, ids, n, d_X, d_Y, b, ld, layout, st)
                            : uspmv_spmmv_ap_hp_chunks(p[0].A, p[1].A, p[2].A, ids, n, d_X, d_Y, b, ld, layout, st);
        return D->tiles ? uspmv_spmmv_ap_tiles(p[0].A, p[1].A, ids, n, d_X, d_Y, b, ld, layout, st)
                        : uspmv_spmmv_ap_chunks(p[0].A, p[1].A, ids, n, d_X, d_Y, b, ld, layout, st);
    };
    HIP_TRY(hipEventRecord(D->ev_main, main));                       // fork, join and the lists: those of step()
    HIP_TRY(hipStreamWaitEvent(D->side_stream, D->ev_main, 0));
    if (int rc = pads ? part_b(D->d_early, D->n_int + D->n_pad, D->side_stream) : part_b(D->d_int, D->n_int, D->side_stream)) return rc;
    HIP_TRY(hipEventRecord(D->ev_comm, D->side_stream));
    if (pads)
        if (int rc = pad_keep_block(D, d_X, b, (long)ld, rowwise, main)) return rc;
    if (int rc = block_exchange(D, d_X, b, layout, mode, main, who)) return rc;
    if (pads)
        if (int rc = pad_guard_block(D, d_X, b, (long)ld, rowwise, main)) return rc;
    HIP_TRY(hipStreamWaitEvent(main, D->ev_comm, 0));                // join
    if (int rc = pads ? part_b(D->d_late, D->n_bnd_real + D->n_pad, main) : part_b(D->d_bnd, D->n_bnd, main)) return rc;
    ++D->spmmv_two_part;
    return step_barrier(D, main);
}

// the argument checks the two block steps of an ap object share, before the kind is looked at
static int check_ap_block_step(const uspmv_dist_t *D, const void *d_X, const void *d_Y, int b, int layout, int mode, const char *who) {
    if (b < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: b=%d", who, b);
    if (layout != USPMV_COLWISE && layout != USPMV_ROWWISE) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown layout %d", who, layout);
    if (mode != USPMV_BULKVEC && mode != USPMV_MULTIVEC && mode != USPMV_SINGLEVEC) return uspmv::fail(USPMV_ERR_INVALID, "%s: unknown mode %d", who, mode);
    if (!D || !d_X || !d_Y) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    return USPMV_OK;
}

int uspmv_dist_spmmv_ap(uspmv_dist_t *D, void *d_X, void *d_Y, int b, int layout, int mode, int comm_halos, void *stream) {
    const char *who = "uspmv_dist_spmmv_ap";
    if (int rc = check_ap_block_step(D, d_X, d_Y, b, layout, mode, who)) return rc;
    if (has_hp(D)) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: an adaptive-precision %s object; its block step is uspmv_dist_spmmv_ap_hp", who, ap_name(D));
    if (!is_ap(D))
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: a one-precision object (uspmv_dist_create_from_coo); its block step is uspmv_dist_spmmv", who);
    return ap_block_step(D, d_X, d_Y, b, layout, mode, comm_halos, stream, who);
}

int uspmv_dist_spmmv_ap_hp(uspmv_dist_t *D, void *d_X, void *d_Y, int b, int layout, int mode, int comm_halos, void *stream) {
    const char *who = "uspmv_dist_spmmv_ap_hp";
    if (int rc = check_ap_block_step(D, d_X, d_Y, b, layout, mode, who)) return rc;
    if (!is_ap(D))
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: a one-precision object (uspmv_dist_create_from_coo); its block step is uspmv_dist_spmmv", who);
    if (!has_hp(D)) return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: an adaptive-precision %s object; its block step is uspmv_dist_spmmv_ap", who, ap_name(D));
    return ap_block_step(D, d_X, d_Y, b, layout, mode, comm_halos, stream, who);
}

}  // extern "C"
