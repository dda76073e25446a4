// The column-window sweep planner: uspmv_dmat_optimize_sweep and its variants (one struct, the ap[dp_sp] pair, the splits with an fp16
// part; from host structs through host/sweep_plan.cpp or from the handles' device arrays through sweep_plan_kernels.hip), and the plan
// digests.  The defaults -- window width, rows per tile, staging cap -- are written once here (the block-vector sweep plan of
// block_planner.hip takes the last two from here as well); which tiles sweep and which rows per tile a builder accepts are the inline rules
// of host/uspmv_internal.hpp, shared with the host builders.  tests/test_gpu_sweep.py, test_gpu_sweep_ap_hp.py and
// test_gpu_sweep_ragged.py compare the host and the device builder's plans array for array.
#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace uspmv_dev {

// rows per tile: the windows are staged once per tile, so more rows = fewer staged bytes per non-zero (a lane owns up to four rows);
// but at least ~1.5 tiles per CU
int sweep_default_tile_rows(int64_t n_pad) {
    int tile_rows = 4096;
    while (tile_rows > 1024 && n_pad / tile_rows < 384) tile_rows /= 2;
    return tile_rows;
}
// largest staging cost in bytes per non-zero at which a tile sweeps ("sweep_max_stage", 0 = 24)
double sweep_max_stage() { return g_tune.sweep_max_stage > 0 ? (double)g_tune.sweep_max_stage : 24.0; }

// What the two builders of a sweep plan do before they look at the matrix: a plan on the handles is dropped, the results are zeroed,
// wlog and tile_rows get their defaults (vsz: bytes of an x element, n_pad: padded rows), and a window that does not fit LDS is refused.
static int sweep_plan_defaults(uspmv_dmat_t *const parts[], int n_parts, size_t vsz, int64_t n_pad, int *wlog, int *tile_rows,
                               int64_t *n_tiles, int64_t *n_sweep, const char *who) {
    for (int k = 0; k < n_parts; ++k) parts[k]->sw = {};
    if (n_tiles) *n_tiles = 0;
    if (n_sweep) *n_sweep = 0;
    if (*wlog <= 0) *wlog = g_tune.sweep_wlog;
    const int nbuf = g_tune.sweep_nbuf == 2 ? 2 : 1;
    // window: as much of the LDS as one buffer per workgroup allows (128 KiB; 64 KiB each when double-buffered) -- on config 4b every
    // doubling from 8 KiB up paid (1.51 / 0.97 / 0.74 / 0.61 ms for the ap kernel at 2^10 .. 2^13 elements, 0.55 at 2^14 with 4 096-row
    // tiles; profiles/r02/config4b_sweep_variants.txt): fewer, longer rounds per wave and fewer barriers
    if (*wlog <= 0) *wlog = (vsz == 8 ? 13 : 14) + (nbuf == 1 ? 1 : 0);
    if (((size_t)1 << *wlog) * vsz * (size_t)nbuf > WG_LDS_BYTES)
        return uspmv::fail(USPMV_ERR_INVALID, "%s: %d window buffer(s) of 2^%d elements do not fit the 160 KB of LDS", who, nbuf, *wlog);
    if (*tile_rows <= 0) *tile_rows = g_tune.sweep_tile_rows;
    if (*tile_rows <= 0) *tile_rows = sweep_default_tile_rows(n_pad);
    return USPMV_OK;
}

// ... and after the arrays are on the first handle: the plan's metadata there; the other handles carry the plan id and the tile counts
static void sweep_plan_stamp(uspmv_dmat_t *const parts[], int n_parts, uint64_t id, int tile_rows, int wlog, int64_t n_sweep,
                             int64_t n_tiles, int64_t x_len, int64_t n_rest, int64_t cnt_bytes) {
    auto &w = parts[0]->sw;
    w.on = true; w.tile_rows = tile_rows; w.wlog = wlog; w.n_tiles = n_sweep; w.all_tiles = n_tiles;
    w.x_len = x_len; w.n_rest = n_rest; w.plan_id = id; w.cnt_bytes = cnt_bytes; w.n_parts = n_parts;
    for (int k = 1; k < n_parts; ++k) {
        auto &o = parts[k]->sw;
        o.on = true; o.plan_id = id; o.n_tiles = n_sweep; o.all_tiles = n_tiles;
    }
}

// builds and uploads a sweep plan for the one struct, or the n_parts parts of an ap split, behind parts / ss; returns the number of
// sweep tiles.  A plan on the handles is replaced.
int sweep_plan_install(uspmv_dmat_t *const parts[], const uspmv_scs_t *const ss[], int n_parts, int wlog, int tile_rows,
                       int64_t *n_tiles, int64_t *n_sweep, const char *who) {
    const uspmv_scs_t *s = ss[0];
    if (int rc = sweep_plan_defaults(parts, n_parts, s->dtype == USPMV_F64 ? 8 : 4, s->n_chunks * s->C, &wlog, &tile_rows, n_tiles, n_sweep, who))
        return rc;
    uspmv_sweep_plan p;
    if (int rc = uspmv_build_sweep_plan(ss, n_parts, wlog, tile_rows, sweep_max_stage(), &p)) return rc;
    if (n_tiles) *n_tiles = p.n_tiles;
    if (n_sweep) *n_sweep = p.valid ? p.n_sweep_tiles : 0;
    if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] sweep plan: tile_rows=%d wlog=%d tiles=%lld sweep=%lld rest_chunks=%zu elements=%zu cnt_bytes=%zu\n",
                                         p.tile_rows, p.wlog, (long long)p.n_tiles, (long long)p.n_sweep_tiles, p.rest_chunks.size(), p.part[0].idx.size(), p.part[0].cnt.size());
    if (!p.valid) return USPMV_OK;
    auto &w = parts[0]->sw;
    hipError_t e = w.tile_ids.upload(p.tile_ids.data(), p.tile_ids.size() * 4);
    if (e == hipSuccess) e = w.smin.upload(p.t_smin.data(), p.t_smin.size() * 4);
    if (e == hipSuccess) e = w.S.upload(p.t_S.data(), p.t_S.size() * 4);
    if (e == hipSuccess) e = w.cnt_off.upload(p.t_cnt_off.data(), p.t_cnt_off.size() * 8);
    if (e == hipSuccess) e = w.rest.upload(p.rest_chunks.data(), p.rest_chunks.size() * 4);
    for (int k = 0; k < n_parts; ++k) {
        const auto &h = p.part[k];
        auto &d = w.part[k];
        d.dtype = h.dtype; d.n_vals = (int64_t)h.idx.size() - 64;
        if (e == hipSuccess) e = d.wave_off.upload(h.wave_off.data(), h.wave_off.size() * 4);
        if (e == hipSuccess) e = d.cnt.upload(h.cnt.data(), h.cnt.size());
        if (e == hipSuccess) e = d.vals.upload(h.vals(), h.idx.size() * uspmv_dtype_bytes(h.dtype));
        if (e == hipSuccess) e = d.idx.upload(h.idx.data(), h.idx.size() * 2);
        if (e == hipSuccess) e = d.pad.upload(h.pad_col.data(), h.pad_col.size() * 4);
    }
    if (e != hipSuccess) {
        w = {};
        return uspmv::fail(USPMV_ERR_ALLOC, "%s: device copy failed: %s", who, hipGetErrorString(e));
    }
    static uint64_t next_sweep_id = 1;
    sweep_plan_stamp(parts, n_parts, next_sweep_id++, p.tile_rows, p.wlog, p.n_sweep_tiles, p.n_tiles, p.x_len_min, (int64_t)p.rest_chunks.size(),
                     (int64_t)p.part[0].cnt.size());
    return USPMV_OK;
}

// The same plan from the handles' DEVICE arrays (csrc/sweep_plan_kernels.hip): a scan kernel per struct, the tile decisions and the
// offsets on the host (O(n_tiles); 16 bytes per 64-row group come back), a fill kernel per struct.  Same defaults, same criteria and
// -- by construction of the fill kernel -- the same arrays as sweep_plan_install builds from host structs.
int sweep_plan_install_device(uspmv_dmat_t *const parts[], int ns, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep,
                              const char *who) {
    uspmv_dmat_t *const A = parts[0];
    const int64_t C = A->C, nc = A->n_chunks, n_pad = nc * C;
    const size_t vsz = A->dtype == USPMV_F64 ? 8 : 4;
    if (int rc = sweep_plan_defaults(parts, ns, vsz, n_pad, &wlog, &tile_rows, n_tiles, n_sweep, who)) return rc;
    tile_rows = uspmv_sweep_tile_rows(tile_rows, /*blocks=*/false);
    if (C < 1 || C > 64 || 64 % C != 0 || nc < 1 || wlog < 8 || wlog > 16) return USPMV_OK;
    for (int w = 0; w < ns; ++w) if (parts[w]->n_elements > (int64_t)UINT32_MAX) return USPMV_OK;
    const int64_t R = tile_rows, nt = (n_pad + R - 1) / R, wpt = R / 64, n_groups = (n_pad + 63) / 64;
    // ---- scan
    DeviceBuf<int> d_le[3], d_pad[3], d_grp[3], d_max;
    hipError_t e = d_max.zeros(4);
    for (int w = 0; w < ns && e == hipSuccess; ++w) {
        e = d_le[w].alloc(4 * (size_t)n_groups * 64);
        if (e == hipSuccess) e = d_pad[w].alloc(4 * (size_t)n_groups * 64);
        if (e == hipSuccess) e = d_grp[w].alloc(16 * (size_t)n_groups);
    }
    if (e != hipSuccess) return uspmv::fail(USPMV_ERR_ALLOC, "%s: %s", who, hipGetErrorString(e));
    std::vector<int32_t> grp[3];
    int max_col = 0;
    int rc = USPMV_OK;
    for (int w = 0; w < ns && !rc; ++w) rc = launch_sweep_scan(parts[w], wlog, d_le[w], d_pad[w], d_grp[w], d_max, nullptr);
    for (int w = 0; w < ns && !rc; ++w) {
        grp[w].resize((size_t)n_groups * 4);
        e = hipMemcpy(grp[w].data(), d_grp[w], 16 * (size_t)n_groups, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (!rc && hipMemcpy(&max_col, d_max, 4, hipMemcpyDeviceToHost) != hipSuccess) rc = uspmv::fail(USPMV_ERR_HIP, "%s: scan results", who);
    if (rc) return rc;
    // ---- which tiles sweep (sweep_plan.cpp pass 1), offsets
    std::vector<int32_t> tile_ids, t_smin, t_S, rest;
    std::vector<uint64_t> t_cnt_off;
    int64_t cnt_bytes = 0, tot[3] = {0, 0, 0};
    for (int64_t t = 0; t < nt; ++t) {
        int32_t lo = INT32_MAX, hi = -1;
        bool good = true;
        int64_t nnz_t = 0;
        for (int w = 0; w < ns; ++w)
            for (int64_t g = t * wpt; g < std::min((t + 1) * wpt, n_groups); ++g) {
                const int32_t *q = grp[w].data() + (size_t)g * 4;
                nnz_t += q[0]; lo = std::min(lo, q[1]); hi = std::max(hi, q[2]); good = good && !q[3];
            }
        const int64_t nS = (int64_t)hi - lo + 1;
        const bool ok = good && hi >= 0 && uspmv_sweep_tile_ok(nS, wlog, vsz, nnz_t, sweep_max_stage());
        if (!ok) { for (int64_t c = t * R / C; c < std::min((t + 1) * R / C, nc); ++c) rest.push_back((int32_t)c); continue; }
        tile_ids.push_back((int32_t)t); t_smin.push_back(lo); t_S.push_back((int32_t)nS); t_cnt_off.push_back((uint64_t)cnt_bytes);
        cnt_bytes += nS * R;
    }
    const int64_t nsw = (int64_t)tile_ids.size();
    if (n_tiles) *n_tiles = nt;
    if (n_sweep) *n_sweep = nsw;
    if (getenv("USPMV_VERBOSE")) fprintf(stderr, "[uspmv] sweep plan (device builder): tile_rows=%d wlog=%d tiles=%lld sweep=%lld rest_chunks=%zu cnt_bytes=%lld\n",
                                         tile_rows, wlog, (long long)nt, (long long)nsw, rest.size(), (long long)cnt_bytes);
    if (nsw == 0) return USPMV_OK;
    std::vector<uint32_t> wave_off[3];
    for (int w = 0; w < ns; ++w) {
        wave_off[w].assign((size_t)(nsw * wpt), 0);
        for (int64_t k = 0; k < nsw; ++k)
            for (int64_t v = 0; v < wpt; ++v) {
                wave_off[w][(size_t)(k * wpt + v)] = (uint32_t)tot[w];
                const int64_t g = (int64_t)tile_ids[(size_t)k] * wpt + v;
                if (g < n_groups) tot[w] += grp[w][(size_t)g * 4];
            }
        if (tot[w] > (int64_t)UINT32_MAX) return USPMV_OK;
    }
    // ---- device arrays of the plan
    constexpr size_t SPARE = 64;
    auto &sw = A->sw;
    if (e == hipSuccess) e = sw.tile_ids.upload(tile_ids.data(), tile_ids.size() * 4);
    if (e == hipSuccess) e = sw.smin.upload(t_smin.data(), t_smin.size() * 4);
    if (e == hipSuccess) e = sw.S.upload(t_S.data(), t_S.size() * 4);
    if (e == hipSuccess) e = sw.cnt_off.upload(t_cnt_off.data(), t_cnt_off.size() * 8);
    if (e == hipSuccess) e = sw.rest.upload(rest.data(), rest.size() * 4);
    for (int w = 0; w < ns; ++w) {
        auto &d = sw.part[w];
        d.dtype = parts[w]->dtype; d.n_vals = tot[w];
        if (e == hipSuccess) e = d.wave_off.upload(wave_off[w].data(), wave_off[w].size() * 4);
        if (e == hipSuccess) e = d.cnt.zeros((size_t)cnt_bytes);
        if (e == hipSuccess) e = d.vals.zeros(((size_t)tot[w] + SPARE) * uspmv_dtype_bytes(d.dtype));
        if (e == hipSuccess) e = d.idx.zeros(((size_t)tot[w] + SPARE) * 2);
        if (e == hipSuccess) e = d.pad.zeros((size_t)(nsw * R) * 4);
    }
    for (int w = 0; w < ns; ++w) {
        auto &d = sw.part[w];
        if (e == hipSuccess && launch_sweep_fill(parts[w], wlog, (int)R, (long)nsw, sw.tile_ids, sw.smin, sw.S, (const unsigned long long *)sw.cnt_off,
                                                 d.wave_off, d_le[w], d_pad[w], d.cnt, d.vals, d.idx, d.pad, nullptr) != USPMV_OK) e = hipErrorUnknown;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    for (int w = 0; w < 3; ++w) { d_le[w].reset(); d_pad[w].reset(); d_grp[w].reset(); }
    d_max.reset();
    if (e != hipSuccess) {
        sw = {};
        return uspmv::fail(USPMV_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    static uint64_t next_dev_sweep_id = (uint64_t)1 << 41;
    sweep_plan_stamp(parts, ns, next_dev_sweep_id++, tile_rows, wlog, nsw, nt, (int64_t)max_col + 1, (int64_t)rest.size(), cnt_bytes);
    return USPMV_OK;
}

// FNV-1a digest of a device array (tests: a plan built on the device must equal the host planner's)
int device_fnv(const void *d, size_t bytes, uint64_t *out) {
    uint64_t h = 1469598103934665603ull;
    if (d && bytes) {
        std::vector<unsigned char> buf(bytes);
        HIP_TRY(hipMemcpy(buf.data(), d, bytes, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < bytes; ++k) { h ^= buf[k]; h *= 1099511628211ull; }
    }
    *out = h;
    return USPMV_OK;
}

}  // namespace uspmv_dev

extern "C" {

int uspmv_dmat_optimize_sweep(uspmv_dmat_t *A, const uspmv_scs_t *s, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep) {
    if (!A || !s) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep: NULL argument");
    if (int rc = check_dmat_one_prec(A, "uspmv_dmat_optimize_sweep")) return rc;
    if (!uspmv::scs_has_entries(s)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep: layout-only struct; the plan builder needs the host entries");
    if (A->C != s->C || A->n_chunks != s->n_chunks || A->dtype != s->dtype)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep: handle and host struct do not describe the same matrix");
    if (int rc = require_device()) return rc;
    return sweep_plan_install(&A, &s, 1, wlog, tile_rows, n_tiles, n_sweep, "uspmv_dmat_optimize_sweep");
}

int uspmv_dmat_optimize_sweep_ap(uspmv_dmat_t *dp, uspmv_dmat_t *sp, const uspmv_scs_t *s_dp, const uspmv_scs_t *s_sp, int wlog, int tile_rows,
                                 int64_t *n_tiles, int64_t *n_sweep) {
    if (!dp || !sp || !s_dp || !s_sp) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep_ap: NULL argument");
    if (!uspmv::scs_has_entries(s_dp) || !uspmv::scs_has_entries(s_sp))
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep_ap: layout-only struct; the plan builder needs the host entries");
    if (dp->C != s_dp->C || dp->n_chunks != s_dp->n_chunks || dp->dtype != USPMV_F64 || s_dp->dtype != USPMV_F64 ||
        sp->C != s_sp->C || sp->n_chunks != s_sp->n_chunks || sp->dtype != USPMV_F32 || s_sp->dtype != USPMV_F32 ||
        dp->C != sp->C || dp->n_chunks != sp->n_chunks)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep_ap: handles / host structs do not form a dp+sp pair");
    if (int rc = require_device()) return rc;
    uspmv_dmat_t *const ms[2] = {dp, sp};
    const uspmv_scs_t *const ss[2] = {s_dp, s_sp};
    return sweep_plan_install(ms, ss, 2, wlog, tile_rows, n_tiles, n_sweep, "uspmv_dmat_optimize_sweep_ap");
}

int uspmv_dmat_optimize_sweep_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, const uspmv_scs_t *s_hi, const uspmv_scs_t *s_mid,
                                    const uspmv_scs_t *s_hp, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep) {
    const char *who = "uspmv_dmat_optimize_sweep_ap_hp";
    if (!s_hi || !s_hp || (mid && !s_mid)) return uspmv::fail(USPMV_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    const uspmv_scs_t *ss[3] = {s_hi, mid ? s_mid : s_hp, mid ? s_hp : nullptr};
    uspmv_dmat_t *const ms[3] = {hi, mid ? mid : hp, mid ? hp : nullptr};
    for (int k = 0; k < 3; ++k) {
        if (!ms[k]) continue;
        if (!uspmv::scs_has_entries(ss[k])) return uspmv::fail(USPMV_ERR_INVALID, "%s: layout-only struct; the plan builder needs the host entries", who);
        if (ms[k]->C != ss[k]->C || ms[k]->n_chunks != ss[k]->n_chunks || ms[k]->dtype != ss[k]->dtype)
            return uspmv::fail(USPMV_ERR_INVALID, "%s: handles and host structs do not describe the same parts", who);
    }
    if (int rc = require_device()) return rc;
    return sweep_plan_install(ms, ss, mid ? 3 : 2, wlog, tile_rows, n_tiles, n_sweep, who);
}

int uspmv_dmat_optimize_sweep_device_ap_hp(uspmv_dmat_t *hi, uspmv_dmat_t *mid, uspmv_dmat_t *hp, int wlog, int tile_rows, int64_t *n_tiles,
                                           int64_t *n_sweep) {
    const char *who = "uspmv_dmat_optimize_sweep_device_ap_hp";
    if (int rc = check_ap_hp(hi, mid, hp, who)) return rc;
    if (int rc = require_device()) return rc;
    uspmv_dmat_t *const ms[3] = {hi, mid ? mid : hp, mid ? hp : nullptr};
    return sweep_plan_install_device(ms, mid ? 3 : 2, wlog, tile_rows, n_tiles, n_sweep, who);
}

int uspmv_dmat_optimize_sweep_device(uspmv_dmat_t *A, uspmv_dmat_t *sp, int wlog, int tile_rows, int64_t *n_tiles, int64_t *n_sweep) {
    if (int rc = check_dmat_one_prec(A, "uspmv_dmat_optimize_sweep_device")) return rc;
    if (sp) {
        if (int rc = check_dmat(sp, "uspmv_dmat_optimize_sweep_device")) return rc;
        if (A->dtype != USPMV_F64 || sp->dtype != USPMV_F32 || A->C != sp->C || A->n_chunks != sp->n_chunks)
            return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_optimize_sweep_device: handles do not form a dp+sp pair");
    }
    if (int rc = require_device()) return rc;
    uspmv_dmat_t *const ms[2] = {A, sp};
    return sweep_plan_install_device(ms, sp ? 2 : 1, wlog, tile_rows, n_tiles, n_sweep, "uspmv_dmat_optimize_sweep_device");
}

// ... of one part's arrays of the sweep plan: wave offsets, counts, values, indices, padding columns
static int sweep_part_digest(const uspmv_dmat::SweepPlan &w, int part, uint64_t digest[5]) {
    const auto &pt = w.part[part];
    const size_t nsw = (size_t)w.n_tiles, wpt = (size_t)w.tile_rows / 64, nv = (size_t)pt.n_vals;
    int rc = device_fnv(pt.wave_off, nsw * wpt * 4, &digest[0]);
    if (!rc) rc = device_fnv(pt.cnt, (size_t)w.cnt_bytes, &digest[1]);
    if (!rc) rc = device_fnv(pt.vals, nv * uspmv_dtype_bytes(pt.dtype), &digest[2]);
    if (!rc) rc = device_fnv(pt.idx, nv * 2, &digest[3]);
    if (!rc) rc = device_fnv(pt.pad, nsw * (size_t)w.tile_rows * 4, &digest[4]);
    return rc;
}

// ... of the whole plan: digest[0..3] the tile arrays, [4..8] part 0, [9] the rest chunks, [10..14] part 1
int uspmv_dmat_sweep_plan_digest(const uspmv_dmat_t *A, uint64_t digest[16], int64_t meta[8]) {
    if (int rc = check_dmat(A, "uspmv_dmat_sweep_plan_digest")) return rc;
    if (!digest || !meta) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_sweep_plan_digest: NULL argument");
    for (int k = 0; k < 16; ++k) digest[k] = 0;
    const auto &w = A->sw;
    meta[0] = w.on; meta[1] = w.tile_rows; meta[2] = w.wlog; meta[3] = w.n_tiles; meta[4] = w.all_tiles; meta[5] = w.n_rest;
    meta[6] = w.part[0].n_vals; meta[7] = w.part[1].n_vals;
    if (!w.on || !w.tile_ids) return USPMV_OK;
    const size_t nsw = (size_t)w.n_tiles;
    int rc = device_fnv(w.tile_ids, nsw * 4, &digest[0]);
    if (!rc) rc = device_fnv(w.smin, nsw * 4, &digest[1]);
    if (!rc) rc = device_fnv(w.S, nsw * 4, &digest[2]);
    if (!rc) rc = device_fnv(w.cnt_off, nsw * 8, &digest[3]);
    if (!rc) rc = sweep_part_digest(w, 0, &digest[4]);
    if (!rc) rc = device_fnv(w.rest, (size_t)w.n_rest * 4, &digest[9]);
    if (!rc && w.n_parts >= 2) rc = sweep_part_digest(w, 1, &digest[10]);
    return rc;
}

int uspmv_dmat_sweep_plan_digest_part(const uspmv_dmat_t *A, int part, uint64_t digest[5], int64_t *n_vals) {
    if (int rc = check_dmat(A, "uspmv_dmat_sweep_plan_digest_part")) return rc;
    if (!digest || part < 0 || part > 2) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_dmat_sweep_plan_digest_part: bad argument");
    for (int k = 0; k < 5; ++k) digest[k] = 0;
    if (n_vals) *n_vals = 0;
    const auto &w = A->sw;
    if (!w.on || !w.tile_ids || part >= w.n_parts) return USPMV_OK;
    if (n_vals) *n_vals = w.part[part].n_vals;
    return sweep_part_digest(w, part, digest);
}

}  // extern "C"
