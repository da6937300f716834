// sdfgpu_resample.hip -- the two Resample kernels (sdfgpu_resample.hpp) and their launcher.  Compiled beside sdfgpu.hip and linked
// into the same libsdfgpu.so (sdf_tools_amd/build.py).
// The family's host orchestration and C ABI entry points (sdfgpu_resample_cells*, sdfgpu_debug_resample_times) are at the end of this file, over the handle of
// sdfgpu_context.hpp.
//
// Arithmetic: the destination of a source cell must round exactly as VoxelGrid::GridIndexToLocation followed by
// VoxelGrid::LocationToGridIndex4d does on the host (separate products and sums in eigen_lite order), because a source centre
// that sits on a result cell boundary is placed by rounding noise alone; so nothing in this file may be contracted into an FMA
// (hipcc contracts by default).
// The host code at the end of this file falls under the pragma too.  It is compiled for baseline x86-64, which has no FMA to
// contract into, so the pragma changes nothing there -- look again before giving the host pass a -march.
#pragma clang fp contract(off)
#include "sdfgpu_context.hpp"
#include "sdfgpu_resample.hpp"
#include "sdfgpu.h"

namespace sdfgpu {

namespace {

// One dimension of a HIP launch takes fewer than 2^32 threads (a larger one is not refused: its size wraps), so more than
// kRsGridX workgroups go over two grid dimensions and a workgroup's number is y * gridDim.x + x (as in sdfgpu_batch.hip).
dim3 rs_grid(int64_t workgroups) {
    if (workgroups <= kRsGridX) return dim3((unsigned)workgroups);
    return dim3((unsigned)kRsGridX, (unsigned)((workgroups + kRsGridX - 1) / kRsGridX));
}

__device__ __forceinline__ int64_t rs_workgroup() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// Isometry3d * Vector4d of eigen_lite.hpp, row r of a row-major 4 x 4: ((m0 v0 + m1 v1) + m2 v2) + m3 v3
__device__ __forceinline__ double rs_row(const double* m, int r, double v0, double v1, double v2, double v3) {
    return m[4 * r] * v0 + m[4 * r + 1] * v1 + m[4 * r + 2] * v2 + m[4 * r + 3] * v3;
}

// The result cell of source cell (x, y, z) as a linear index, or -1 when it falls outside the result (or is not finite).
__device__ __forceinline__ int64_t rs_destination(const ResampleArgs& a, int64_t x, int64_t y, int64_t z) {
    // GridIndexToLocationGridFrame, then the origin transform (all four rows: the fourth carries into the second product)
    const double g0 = a.cell[0] * ((double)x + 0.5), g1 = a.cell[1] * ((double)y + 0.5), g2 = a.cell[2] * ((double)z + 0.5), g3 = 1.0;
    const double l0 = rs_row(a.origin, 0, g0, g1, g2, g3), l1 = rs_row(a.origin, 1, g0, g1, g2, g3);
    const double l2 = rs_row(a.origin, 2, g0, g1, g2, g3), l3 = rs_row(a.origin, 3, g0, g1, g2, g3);
    // LocationToGridIndex4d of the result: its inverse origin transform, then a product with 1 / cell (not a division)
    const double v0 = rs_row(a.inverse, 0, l0, l1, l2, l3) * a.inv_cell[0];
    const double v1 = rs_row(a.inverse, 1, l0, l1, l2, l3) * a.inv_cell[1];
    const double v2 = rs_row(a.inverse, 2, l0, l1, l2, l3) * a.inv_cell[2];
    // floor(v) in [0, n) <=> v in [0, n) for finite v; NaN and the infinities fail a comparison (no cast of such a double)
    if (!(v0 >= 0.0 && v0 < (double)a.mx && v1 >= 0.0 && v1 < (double)a.my && v2 >= 0.0 && v2 < (double)a.mz)) return -1;
    return ((int64_t)floor(v0) * a.my + (int64_t)floor(v1)) * a.mz + (int64_t)floor(v2);
}

// W = uint32_t: n_src < 2^32 - 1, so the source index and its decomposition fit 32-bit arithmetic
template <typename W, bool PLAIN>
__global__ __launch_bounds__(kRsThreads) void k_rs_winner(const ResampleArgs a) {
    const int64_t i = rs_workgroup() * kRsThreads + threadIdx.x;
    if (rs_workgroup() * kRsThreads >= a.n_src) return;                     // (the last row of a two-dimensional launch)
    int64_t d = -1;
    if (i < a.n_src) {
        int64_t x, y, z;
        if (sizeof(W) == 4) {
            const uint32_t u = (uint32_t)i, unz = (uint32_t)a.nz, uny = (uint32_t)a.ny;
            const uint32_t t = u / unz;
            z = u - t * unz; x = t / uny; y = t - (uint32_t)x * uny;
        } else {
            const int64_t t = i / a.nz;
            z = i - t * a.nz; x = t / a.ny; y = t - x * a.ny;
        }
        d = rs_destination(a, x, y, z);
    }
    bool issue = d >= 0;
    if (!PLAIN) {
        // lanes ascend in the source index: a lane whose successor in the wave has the same destination loses to it anyway
        const int64_t next = __shfl_down((long long)d, 1);
        issue = issue && ((threadIdx.x & 63) == 63 || next != d);
    }
    if (issue) atomicMax(static_cast<W*>(a.winner) + d, (W)(i + 1));
}

// REC dwords per record, moved ACC dwords at a time (ACC > 1 only when both pointers are aligned for it)
template <int REC, int ACC>
__device__ __forceinline__ void rs_load(const uint32_t* __restrict__ p, uint32_t (&r)[REC]) {
    if constexpr (ACC == 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else if constexpr (ACC == 2) {
        for (int k = 0; k < REC; k += 2) { const uint2 v = *reinterpret_cast<const uint2*>(p + k); r[k] = v.x; r[k + 1] = v.y; }
    } else {
        for (int k = 0; k < REC; ++k) r[k] = p[k];
    }
}
template <int REC, int ACC>
__device__ __forceinline__ void rs_store(uint32_t* __restrict__ p, const uint32_t (&r)[REC]) {
    if constexpr (ACC == 4) {
        *reinterpret_cast<uint4*>(p) = make_uint4(r[0], r[1], r[2], r[3]);
    } else if constexpr (ACC == 2) {
        for (int k = 0; k < REC; k += 2) *reinterpret_cast<uint2*>(p + k) = make_uint2(r[k], r[k + 1]);
    } else {
        for (int k = 0; k < REC; ++k) p[k] = r[k];
    }
}

template <typename W, int REC, int ACC>
__global__ __launch_bounds__(kRsThreads) void k_rs_gather(const ResampleArgs a) {
    static_assert(ACC <= REC, "an access is at most one record");
    __shared__ uint32_t wave_hits[kRsThreads / 64];
    const int64_t d = rs_workgroup() * kRsThreads + threadIdx.x;
    if (rs_workgroup() * kRsThreads >= a.n_dst) return;
    bool hit = false;
    if (d < a.n_dst) {
        const W w = static_cast<const W*>(a.winner)[d];
        hit = w != 0;
        uint32_t r[REC];
        if (hit) rs_load<REC, ACC>(static_cast<const uint32_t*>(a.src) + (int64_t)(w - 1) * REC, r);
        else for (int k = 0; k < REC; ++k) r[k] = a.fill[k];
        rs_store<REC, ACC>(static_cast<uint32_t*>(a.dst) + d * REC, r);
    }
    if (a.written) {                                                        // (uniform)
        const unsigned long long b = __ballot(hit);
        if ((threadIdx.x & 63) == 0) wave_hits[threadIdx.x >> 6] = (uint32_t)__popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int k = 0; k < kRsThreads / 64; ++k) t += wave_hits[k];
            if (t) atomicAdd(a.written, (unsigned long long)t);
        }
    }
}

template <typename W, int REC>
void rs_launch_gather(const ResampleArgs& a, int acc, dim3 grid, hipStream_t s) {
    if (acc >= 4 && REC >= 4) hipLaunchKernelGGL((k_rs_gather<W, REC, (REC >= 4 ? 4 : REC)>), grid, dim3(kRsThreads), 0, s, a);
    else if (acc >= 2 && REC >= 2) hipLaunchKernelGGL((k_rs_gather<W, REC, (REC >= 2 ? 2 : REC)>), grid, dim3(kRsThreads), 0, s, a);
    else hipLaunchKernelGGL((k_rs_gather<W, REC, 1>), grid, dim3(kRsThreads), 0, s, a);
}

template <typename W>
hipError_t rs_launch(const ResampleArgs& a, hipStream_t s, hipEvent_t after_winner) {
    const dim3 grid_src = rs_grid((a.n_src + kRsThreads - 1) / kRsThreads), grid_dst = rs_grid((a.n_dst + kRsThreads - 1) / kRsThreads);
    if (a.plain_atomics) hipLaunchKernelGGL((k_rs_winner<W, true>), grid_src, dim3(kRsThreads), 0, s, a);
    else hipLaunchKernelGGL((k_rs_winner<W, false>), grid_src, dim3(kRsThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && after_winner) e = hipEventRecord(after_winner, s);
    if (e != hipSuccess) return e;
    // the widest access both pointers are aligned for, chosen once per launch (records keep that alignment: their size is a multiple)
    const uintptr_t both = reinterpret_cast<uintptr_t>(a.src) | reinterpret_cast<uintptr_t>(a.dst);
    const int acc = (both & 15) == 0 ? 4 : (both & 7) == 0 ? 2 : 1;
    if (a.cell_bytes == 16) rs_launch_gather<W, 4>(a, acc, grid_dst, s);
    else if (a.cell_bytes == 8) rs_launch_gather<W, 2>(a, acc, grid_dst, s);
    else rs_launch_gather<W, 1>(a, acc, grid_dst, s);
    return hipGetLastError();
}

}  // namespace

hipError_t resample_launch(const ResampleArgs& a, hipStream_t s, hipEvent_t after_winner) {
    hipError_t e = hipMemsetAsync(a.winner, 0, resample_scratch_bytes(a.n_dst, a.winner_bytes), s);
    if (e != hipSuccess) return e;
    return a.winner_bytes == 4 ? rs_launch<uint32_t>(a, s, after_winner) : rs_launch<unsigned long long>(a, s, after_winner);
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

// ---- resample (sdfgpu_resample.hpp) ------------------------------------------------------------------------------------------------
// Only rs_scratch (and, in the host form, the cell and field staging and the pinned chunks) is used.
int check_resample_args(sdfgpu_handle h, const void* src, size_t cell_bytes, int64_t nx, int64_t ny, int64_t nz, const double* src_cell,
                        const double* origin, const double* dst_inverse_origin, const double* dst_inv_cell, const void* dst, int64_t mx,
                        int64_t my, int64_t mz, const void* fill_cell, ResampleArgs& a) {
    if (!src || !dst || !src_cell || !origin || !dst_inverse_origin || !dst_inv_cell || !fill_cell)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: null pointer");
    if (cell_bytes != 4 && cell_bytes != 8 && cell_bytes != 16)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: cell_bytes must be 4, 8 or 16 (got %zu)", cell_bytes);
    if (src == dst) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: the source and the result must be different buffers");
    const int64_t kMaxCells = INT64_MAX / 16;
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx > kMaxCells / ny || nx * ny > kMaxCells / nz)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: unsupported source grid %lld x %lld x %lld", (long long)nx, (long long)ny, (long long)nz);
    if (mx <= 0 || my <= 0 || mz <= 0 || mx > kMaxCells / my || mx * my > kMaxCells / mz)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: unsupported result grid %lld x %lld x %lld", (long long)mx, (long long)my, (long long)mz);
    a = ResampleArgs{};
    a.nx = nx; a.ny = ny; a.nz = nz; a.mx = mx; a.my = my; a.mz = mz;
    a.n_src = nx * ny * nz; a.n_dst = mx * my * mz;
    for (int i = 0; i < 3; ++i) { a.cell[i] = src_cell[i]; a.inv_cell[i] = dst_inv_cell[i]; }
    for (int i = 0; i < 16; ++i) { a.origin[i] = origin[i]; a.inverse[i] = dst_inverse_origin[i]; }
    memcpy(a.fill, fill_cell, cell_bytes);
    a.cell_bytes = (int)cell_bytes;
    a.winner_bytes = resample_winner_bytes(a.n_src);
    a.plain_atomics = h->opt.rs_plain_atomics;
    return SDFGPU_OK;
}

// a.src -> a.dst (device) on `st`; synchronises `st` only when out_written is asked for
int resample_impl(sdfgpu_handle h, ResampleArgs& a, uint64_t* out_written, hipStream_t st) {
    // the winner words belong to the handle and the call may return with its kernels pending: a call on another stream waits for
    // them on the device first, as the local extrema do (ensure() below may free the scratch: hipFree waits for the device)
    HIP_TRY(h, h->rs_order.create());
    HIP_TRY(h, h->rs_order.wait(st));
    if (int rc = ensure(h, h->rs_scratch, resample_scratch_bytes(a.n_dst, a.winner_bytes), "resample winners")) return rc;
    a.winner = h->rs_scratch.ptr;
    unsigned long long* const counter =
        reinterpret_cast<unsigned long long*>(static_cast<char*>(h->rs_scratch.ptr) + resample_counter_offset(a.n_dst, a.winner_bytes));
    a.written = out_written ? counter : nullptr;
    if (h->opt.rs_timing) {
        for (hipEvent_t& e : h->rs_time_ev) if (!e) HIP_TRY(h, hipEventCreate(&e));
        HIP_TRY(h, hipEventRecord(h->rs_time_ev[0], st));
    }
    const hipError_t le = resample_launch(a, st, h->opt.rs_timing ? h->rs_time_ev[1] : nullptr);
    if (h->opt.rs_timing) h->rs_timed = le == hipSuccess && hipEventRecord(h->rs_time_ev[2], st) == hipSuccess;
    (void)h->rs_order.record(st);                       // (also behind a failed launch: what it did enqueue is ordered)
    HIP_TRY(h, le);
    if (out_written) {
        unsigned long long count = 0;
        HIP_TRY(h, hipMemcpyAsync(&count, counter, sizeof count, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        *out_written = (uint64_t)count;
    }
    return SDFGPU_OK;
}

}  // namespace

extern "C" {

int sdfgpu_resample_cells_device(sdfgpu_handle h, const void* d_src, size_t cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                                 const double src_cell[3], const double origin[16], const double dst_inverse_origin[16],
                                 const double dst_inv_cell[3], void* d_dst, int64_t mx, int64_t my, int64_t mz, const void* fill_cell,
                                 uint64_t* out_cells_written, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        ResampleArgs a;
        if (int rc = check_resample_args(h, d_src, cell_bytes, nx, ny, nz, src_cell, origin, dst_inverse_origin, dst_inv_cell, d_dst, mx, my,
                                         mz, fill_cell, a)) return rc;
        if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: d_src and d_dst must be 4-byte aligned");
        HIP_TRY(h, hipSetDevice(h->device));
        a.src = d_src; a.dst = d_dst;
        return resample_impl(h, a, out_cells_written, (hipStream_t)stream);
    });
}

int sdfgpu_debug_resample_times(sdfgpu_handle h, double* out_winner_ms, double* out_gather_ms) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!out_winner_ms || !out_gather_ms) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
    if (!h->rs_timed) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no resample timed on this handle (option \"resample_timing\")");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventSynchronize(h->rs_time_ev[2]));
    float a = 0.0f, b = 0.0f;
    HIP_TRY(h, hipEventElapsedTime(&a, h->rs_time_ev[0], h->rs_time_ev[1]));
    HIP_TRY(h, hipEventElapsedTime(&b, h->rs_time_ev[1], h->rs_time_ev[2]));
    *out_winner_ms = (double)a;
    *out_gather_ms = (double)b;
    return SDFGPU_OK;
}

int sdfgpu_resample_cells(sdfgpu_handle h, const void* src, size_t cell_bytes, int64_t nx, int64_t ny, int64_t nz, const double src_cell[3],
                          const double origin[16], const double dst_inverse_origin[16], const double dst_inv_cell[3], void* dst, int64_t mx,
                          int64_t my, int64_t mz, const void* fill_cell, uint64_t* out_cells_written) {
    return rz_wrap(h, nullptr, [&]() -> int {
        ResampleArgs a;
        if (int rc = check_resample_args(h, src, cell_bytes, nx, ny, nz, src_cell, origin, dst_inverse_origin, dst_inv_cell, dst, mx, my, mz,
                                         fill_cell, a)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        // the null stream throughout: source records through the cell staging, the result through the field staging
        const size_t src_bytes = (size_t)a.n_src * cell_bytes, dst_bytes = (size_t)a.n_dst * cell_bytes;
        if (int rc = stage_input(h, src_bytes)) return rc;
        if (int rc = ensure(h, h->stage_out, dst_bytes, "output staging")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, src, src_bytes)) return rc;
        a.src = h->stage_in.ptr; a.dst = h->stage_out.ptr;
        if (int rc = resample_impl(h, a, out_cells_written, nullptr)) return rc;
        return copy_to_host(h, dst, h->stage_out.ptr, dst_bytes);
    });
}

}  // extern "C"
