// uspmv_gen_stencil27 ON THE DEVICE (uspmv_gen_stencil27_device): rows [row_begin, row_end) of the 27-point stencil matrix of
// host/gen_matrix.cpp as COO arrays in HBM -- row ids local, column ids global, sorted by row, columns ascending inside a row: the input
// of uspmv_dist_create_from_arrays.  I, J and V equal the host generator's in every bit (tests/test_gpu_gen_device.py).
//   pass (a)  gen_counts_kernel  one lane per row: span(x) * span(y) * span(z) * dof entries (gen_matrix.cpp:39-44)
//   pass (b)  the exclusive scan of convert_kernels.hip: where every row starts, and the block's nnz
//   pass (c)  gen_fill_kernel    one lane per ENTRY.  A workgroup takes 1024 consecutive entries, four rounds of 256: lane l of a round
//                                writes entry k0 + 256 * round + l, so a wave stores 256 contiguous bytes of I, 256 of J and 512 of V.
//                                Which row an entry belongs to: thread 0 finds the workgroup's first row by bisection of the row starts,
//                                the (at most 1025, every row has an entry) starts from there go to LDS and every lane bisects those.
//                                The position inside the row gives (dz, dy, dx, e) by division: the host's loop order.
// Values: the hash (mix64, pair_hash) is 64-bit integer arithmetic, the same on any machine.  With magnitude_decades == 0 every product in
// the value formulas is exact ((h >> 11) * 2^-53, 2.0 * u, 27.0 * dof), so each formula rounds exactly once whether or not the compiler
// contracts a product and a sum into an FMA; gen_value is compiled with contraction off all the same, so that this stays a fact about the
// source and not about what one compiler version happens to emit.  magnitude_decades > 0 is refused: the host calls glibc's pow, the
// device has another pow, and a generated matrix must not depend on where it was generated.
// Bytes: (a) + (b) 28 per row, (c) writes 16 per entry and reads the row starts (4 per row and workgroup, from L2).
#include <memory>

#include "uspmv_device.hpp"

using namespace uspmv_dev;

namespace {

constexpr int WG = 256, PER_WG = 1024;

struct GenGrid {
    unsigned nx, ny, nz, dof, nxy;     // (all below 2^31: nx * ny * nz * dof <= INT32_MAX is checked on the host)
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t pair_hash(uint64_t a, uint64_t b, uint64_t seed) { return mix64(mix64(a ^ seed) + b); }

// v(i, j) of gen_matrix.cpp for magnitude_decades == 0: 2 u01(h) - 1, on the diagonal 27 dof + that
__device__ __forceinline__ double gen_value(const uint64_t h, const bool diagonal, const unsigned dof) {
#pragma clang fp contract(off)
    const double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);
    const double w = 2.0 * u - 1.0;
    return diagonal ? 27.0 * (double)dof + w : w;
}

__device__ __forceinline__ unsigned span(const unsigned c, const unsigned nc) { return 1u + (c > 0) + (c + 1 < nc); }

__global__ void __launch_bounds__(WG) gen_counts_kernel(const GenGrid g, const long row_begin, const long nloc, long *__restrict__ counts) {
    const long r = (long)blockIdx.x * WG + threadIdx.x;
    if (r >= nloc) return;
    const unsigned node = (unsigned)(row_begin + r) / g.dof;
    const unsigned x = node % g.nx, y = (node / g.nx) % g.ny, z = node / g.nxy;
    counts[r] = (long)(span(x, g.nx) * span(y, g.ny) * span(z, g.nz)) * g.dof;
}

// start: nloc + 1 row starts (start[0] = 0, start[nloc] = nnz), every row with at least one entry
__global__ void __launch_bounds__(WG) gen_fill_kernel(const GenGrid g, const unsigned long long seed, const long row_begin, const long nloc, const long nnz,
                                                      const int *__restrict__ start, int *__restrict__ I, int *__restrict__ J, double *__restrict__ V) {
    __shared__ int s[PER_WG + 1];
    __shared__ long s_r0;
    const long k0 = (long)blockIdx.x * PER_WG;            // (< nnz by the grid size)
    if (threadIdx.x == 0) {
        long lo = 0, hi = nloc;                           // start[lo] <= k0 < start[hi]
        while (hi - lo > 1) {
            const long mid = (lo + hi) >> 1;
            if (start[mid] <= k0) lo = mid; else hi = mid;
        }
        s_r0 = lo;
    }
    __syncthreads();
    const long r0 = s_r0;
    // the rows of this workgroup's entries lie in [r0, r0 + PER_WG): s[t] = start[r0 + t], and s[m - 1] > every k of the workgroup
    const int m = (int)(nloc + 1 - r0 < PER_WG + 1 ? nloc + 1 - r0 : PER_WG + 1);
    for (int t = threadIdx.x; t < m; t += WG) s[t] = start[r0 + t];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER_WG / WG; ++u) {
        const long k = k0 + u * WG + threadIdx.x;
        if (k >= nnz) break;
        int lo = 0, hi = m - 1;                           // s[lo] <= k < s[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s[mid] <= k) lo = mid; else hi = mid;
        }
        const long r = r0 + lo;
        unsigned q = (unsigned)(k - s[lo]);               // position in the row: ((iz * sy + iy) * sx + ix) * dof + e
        const unsigned row = (unsigned)(row_begin + r), node = row / g.dof;
        const unsigned x = node % g.nx, y = (node / g.nx) % g.ny, z = node / g.nxy;
        const unsigned sx = span(x, g.nx), sy = span(y, g.ny);
        const unsigned e = q % g.dof; q /= g.dof;
        const unsigned ix = q % sx; q /= sx;
        const unsigned iy = q % sy, iz = q / sy;
        // the first neighbour in a direction is c - 1 unless c sits on the low face
        const unsigned cx = x + ix - (x > 0), cy = y + iy - (y > 0), cz = z + iz - (z > 0);
        const unsigned col = ((cz * g.ny + cy) * g.nx + cx) * g.dof + e;
        const uint64_t h = pair_hash(row < col ? row : col, row < col ? col : row, seed);
        I[k] = (int)r; J[k] = (int)col; V[k] = gen_value(h, col == row, g.dof);
    }
}

}  // namespace

extern "C" int uspmv_gen_stencil27_device(int64_t nx, int64_t ny, int64_t nz, int dof, uint64_t seed, double magnitude_decades, int64_t row_begin,
                                          int64_t row_end, void *stream, uspmv_dcoo_t **out) {
    const char *who = "uspmv_gen_stencil27_device";
    // the host function's refusals, before any HIP call
    if (!out || nx < 1 || ny < 1 || nz < 1 || dof < 1) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad argument", who);
    const int64_t n = nx * ny * nz * dof;
    if (row_begin < 0 || row_end > n || row_begin >= row_end) return uspmv::fail(USPMV_ERR_INVALID, "%s: bad row range", who);
    if (n > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: %lld rows exceed int32", who, (long long)n);
    if (magnitude_decades > 0.0)
        return uspmv::fail(USPMV_ERR_UNSUPPORTED, "%s: magnitude_decades > 0 takes pow, which differs between host and device (a generated matrix must not "
                           "depend on where it was generated): use uspmv_gen_stencil27 and upload the block", who);
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long nloc = (long)(row_end - row_begin);
    const GenGrid g{(unsigned)nx, (unsigned)ny, (unsigned)nz, (unsigned)dof, (unsigned)(nx * ny)};
    DeviceBuf<long> counts, part, sums, total;
    DeviceBuf<int> start;
    HIP_TRY(counts.alloc(8 * (size_t)nloc));
    HIP_TRY(part.alloc(8 * (size_t)nloc));
    HIP_TRY(sums.alloc(8 * (size_t)((nloc + 1023) / 1024)));
    HIP_TRY(total.alloc(8));
    HIP_TRY(start.alloc(4 * ((size_t)nloc + 1)));
    hipLaunchKernelGGL(gen_counts_kernel, dim3((unsigned)((nloc + WG - 1) / WG)), dim3(WG), 0, st, g, (long)row_begin, nloc, counts.get());
    HIP_TRY(hipGetLastError());
    if (int rc = launch_exclusive_scan(counts, nloc, part, sums, total, start, st)) return rc;
    long nnz = 0;
    HIP_TRY(hipMemcpyAsync(&nnz, total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (the row starts are 32-bit: past this point they are only read when they are right)
    if (nnz > INT32_MAX) return uspmv::fail(USPMV_ERR_OVERFLOW, "%s: %lld local nnz exceed int32", who, (long long)nnz);
    std::unique_ptr<uspmv_dcoo> m(new uspmv_dcoo);
    m->nnz = nnz;
    HIP_TRY(m->I.alloc(4 * (size_t)nnz));
    HIP_TRY(m->J.alloc(4 * (size_t)nnz));
    HIP_TRY(m->V.alloc(8 * (size_t)nnz));
    hipLaunchKernelGGL(gen_fill_kernel, dim3((unsigned)((nnz + PER_WG - 1) / PER_WG)), dim3(WG), 0, st, g, (unsigned long long)seed, (long)row_begin, nloc, nnz,
                       (const int *)start.get(), m->I.get(), m->J.get(), m->V.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));                   // (the scratch of this call is released on return)
    *out = m.release();
    return USPMV_OK;
}
