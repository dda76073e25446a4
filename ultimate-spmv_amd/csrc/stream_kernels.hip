// The STREAM-style calibrators (copy, triad, read and the gather of the x lines a stencil tile touches) with their entry points, and
// uspmv_time_launches: what the benchmark measures the kernels against.
#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace {

// STREAM-style calibrators.  copy / triad: every thread moves eight 16-byte pieces, all loads issued before the first store
// (32 KiB in flight per 256-thread workgroup), non-temporal loads and stores -- the shape the guide's 6.3 TB/s copy has; the
// grid-stride form of round 1 (one 16-byte piece in flight per thread, plain stores) stopped at 4.9 TB/s.
__global__ void __launch_bounds__(256) stream_copy_kernel(double2 *__restrict__ a, const double2 *__restrict__ b, const long n2) {
    const long base = (long)blockIdx.x * (256 * 8) + threadIdx.x;
    double v[16];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long i = base + u * 256;
        if (i < n2) { const double *p = (const double *)(b + i); v[2 * u] = __builtin_nontemporal_load(p); v[2 * u + 1] = __builtin_nontemporal_load(p + 1); }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long i = base + u * 256;
        if (i < n2) { double *p = (double *)(a + i); __builtin_nontemporal_store(v[2 * u], p); __builtin_nontemporal_store(v[2 * u + 1], p + 1); }
    }
}
__global__ void __launch_bounds__(256) stream_triad_kernel(double2 *__restrict__ a, const double2 *__restrict__ b,
                                                          const double2 *__restrict__ c, const double s, const long n2) {
    const long base = (long)blockIdx.x * (256 * 4) + threadIdx.x;
    double vb[8], vc[8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i = base + u * 256;
        if (i < n2) {
            const double *pb = (const double *)(b + i), *pc = (const double *)(c + i);
            vb[2 * u] = __builtin_nontemporal_load(pb); vb[2 * u + 1] = __builtin_nontemporal_load(pb + 1);
            vc[2 * u] = __builtin_nontemporal_load(pc); vc[2 * u + 1] = __builtin_nontemporal_load(pc + 1);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i = base + u * 256;
        if (i < n2) {
            double *p = (double *)(a + i);
            __builtin_nontemporal_store(vb[2 * u] + s * vc[2 * u], p); __builtin_nontemporal_store(vb[2 * u + 1] + s * vc[2 * u + 1], p + 1);
        }
    }
}
__global__ void stream_read_kernel(const double2 *__restrict__ b, const long n2, double *__restrict__ partial) {
    double acc = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
        const double *pb = (const double *)(b + i);
        acc += __builtin_nontemporal_load(pb) + __builtin_nontemporal_load(pb + 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) partial[((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6] = acc;
}

// Second yardstick (what the tile-local-column kernel asks of the cache hierarchy beyond a stream): as many workgroups as the SpMV has
// tiles, mapped to the XCDs like its tiles, each reading the x lines a `rows`-row tile of a 27-point stencil touches -- nine runs of
// rows + 2 elements (rounded out to whole 128-byte lines) at the offsets {-plane, 0, +plane} + {-line, 0, +line} around its own rows --
// with the plain 16-byte loads of the kernel's staging phase.  Every element of x is asked for by ~9 workgroups, ~3 of them far apart
// in launch order (the neighbouring planes): what comes from the XCD's L2, what from the fabric, is exactly the SpMV's x traffic,
// without its matrix stream.  Reported as gathered bytes per second.
__global__ void __launch_bounds__(256) stream_gather_lines_kernel(const double2 *__restrict__ x, const long n, const long plane, const long line,
                                                                  const int rows, const int xcd_remap, double *__restrict__ partial) {
    const unsigned tile = remap_block(blockIdx.x, gridDim.x, xcd_remap);
    const long base = (long)tile * rows;
    double acc = 0.0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
            long lo = base + dz * plane + dy * line - 1, hi = base + rows + dz * plane + dy * line + 1;
            lo = lo < 0 ? 0 : (lo & ~15L);
            hi = hi > n ? n : hi;
            hi = (hi + 15) & ~15L;
            if (hi > (n & ~15L)) hi = n & ~15L;
            for (long i = lo / 2 + threadIdx.x; i < hi / 2; i += 256) { const double2 v = x[i]; acc += v.x + v.y; }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) partial[(long)blockIdx.x * 4 + (threadIdx.x >> 6)] = acc;
}

}  // namespace

extern "C" {

int uspmv_stream_copy(double *a, const double *b, int64_t n, void *stream) {
    if (!a || !b || n < 0 || (n & 1)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_stream_copy: bad argument (n must be even)");
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(stream_copy_kernel, dim3((unsigned)((n / 2 + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream, (double2 *)a, (const double2 *)b, (long)(n / 2));
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int uspmv_stream_triad(double *a, const double *b, const double *c, double s, int64_t n, void *stream) {
    if (!a || !b || !c || n < 0 || (n & 1)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_stream_triad: bad argument (n must be even)");
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(stream_triad_kernel, dim3((unsigned)((n / 2 + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, (double2 *)a, (const double2 *)b, (const double2 *)c, s, (long)(n / 2));
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int uspmv_stream_read(const double *b, int64_t n, double *partial, void *stream) {
    if (!b || !partial || n < 0 || (n & 1)) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_stream_read: bad argument (n must be even; partial needs 8192 doubles)");
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(stream_read_kernel, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, (const double2 *)b, (long)(n / 2), partial);
    HIP_TRY(hipGetLastError());
    return USPMV_OK;
}

int uspmv_stream_gather_lines(const double *x, int64_t n, int64_t plane, int64_t line, int rows, double *partial, void *stream, int64_t *bytes) {
    if (!x || !partial || n < 4096 || rows < 16 || rows > 4096 || plane < 0 || line < 0)
        return uspmv::fail(USPMV_ERR_INVALID, "uspmv_stream_gather_lines: bad argument (partial needs 4 * ceil(n / rows) doubles)");
    if (int rc = require_device()) return rc;
    const long tiles = (long)((n + rows - 1) / rows);
    hipLaunchKernelGGL(stream_gather_lines_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const double2 *)x, (long)n, (long)plane, (long)line, rows,
                       g_tune.xcd_remap, partial);
    HIP_TRY(hipGetLastError());
    if (bytes) *bytes = tiles * 9 * (int64_t)(((rows + 2 + 15) / 16 + 1) * 128);   // (nine runs of whole lines per tile; the ends of the vector ask for a little less)
    return USPMV_OK;
}

int uspmv_time_launches(int what, int reps, const uspmv_dmat_t *A, const uspmv_dmat_t *B, const void *d_x, void *d_y,
                        int64_t n, int b, int64_t ld, int layout, void *stream, double *avg_ms) {
    if (reps < 1 || !avg_ms) return uspmv::fail(USPMV_ERR_INVALID, "uspmv_time_launches: bad argument");
    if (int rc = require_device()) return rc;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    hipStream_t st = (hipStream_t)stream;
    int rc = USPMV_OK;
    for (int r = -2; r < reps && rc == USPMV_OK; ++r) {      // two untimed launches first (page tables, caches, clocks)
        if (r == 0) HIP_TRY(hipEventRecord(e0, st));
        switch (what) {
            case 0: rc = uspmv_spmv(A, d_x, d_y, stream); break;
            case 1: rc = uspmv_stream_copy((double *)d_y, (const double *)d_x, n, stream); break;
            case 2: rc = uspmv_stream_triad((double *)d_y, (const double *)d_x, (const double *)d_x + n, 3.0, n, stream); break;
            case 3: rc = uspmv_stream_read((const double *)d_x, n, (double *)d_y, stream); break;
            case 4: rc = uspmv_spmv_ap(A, B, (const double *)d_x, (double *)d_y, stream); break;
            case 5: rc = uspmv_spmmv(A, d_x, d_y, b, ld, layout, stream); break;
            case 6: rc = uspmv_stream_gather_lines((const double *)d_x, n, ld, (int64_t)b, layout, (double *)d_y, stream, nullptr); break;
            case 7: rc = uspmv_spmmv_ap(A, B, d_x, d_y, b, ld, layout, stream); break;
            default: rc = uspmv::fail(USPMV_ERR_INVALID, "uspmv_time_launches: unknown kind %d", what);
        }
    }
    hipError_t e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc != USPMV_OK) return rc;
    if (e != hipSuccess) return uspmv::fail(USPMV_ERR_HIP, "uspmv_time_launches: %s", hipGetErrorString(e));
    *avg_ms = (double)ms / reps;
    return USPMV_OK;
}

}  // extern "C"
