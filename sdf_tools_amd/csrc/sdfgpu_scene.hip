// sdfgpu_scene.hip -- the shape rasteriser (sdfgpu_scene.hpp, include/sdfgpu.h "Shape rasteriser"): three
// kernels, their launcher, the host orchestration and the C ABI entry points sdfgpu_rasterize_shapes*.  Compiled beside sdfgpu.hip
// and linked into the same libsdfgpu.so (sdf_tools_amd/build.py).
//
//   k_sc_prepare   one thread per shape: refuses it (status word) or writes its world bounds, inflated by the resolution
//   k_sc_coarse    one thread per (coarse region, 32 shapes): the candidate bits of the region
//   k_sc_raster    one workgroup per fine region (256 consecutive voxels, one lane per voxel): narrows the coarse region's
//                  candidates to its own, then every lane walks the survivors in list order until one hits; a wave's 64 verdicts
//                  are two whole words of the bit field, written by one lane (nobody else owns them: no atomics, no pre-clear)
//
// Arithmetic: the decision procedure may not be contracted into FMAs (sdfgpu_scene.hpp).  The host code at the end of this file
// falls under the pragma too; it is compiled for baseline x86-64, which has no FMA to contract into.
#pragma clang fp contract(off)
#include "sdfgpu_context.hpp"
#include "sdfgpu_scene.hpp"
#include "sdfgpu.h"

namespace sdfgpu {

namespace {

constexpr uint32_t kScNoBadShape = 0xFFFFFFFFu;

dim3 sc_grid(int64_t workgroups) {
    if (workgroups <= kScGridX) return dim3((unsigned)workgroups);
    return dim3((unsigned)kScGridX, (unsigned)((workgroups + kScGridX - 1) / kScGridX));
}

__device__ __forceinline__ int64_t sc_workgroup() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__global__ __launch_bounds__(kScThreads) void k_sc_prepare(const SceneArgs a) {
    const int64_t i = sc_workgroup() * kScThreads + threadIdx.x;
    if (i >= a.n_shapes) return;
    const sdfgpu_shape& s = a.shapes[i];
    double* b = a.bounds + 6 * i;
    if (!sc_shape_valid(s) || (a.ids && s.object_id == 0)) {
        atomicMin(a.status, (uint32_t)i);
        for (int k = 0; k < 3; ++k) { b[k] = 1.0; b[3 + k] = -1.0; }
        return;
    }
    if (s.type == SDFGPU_SHAPE_PLANE) {                                      // unbounded: a candidate everywhere
        for (int k = 0; k < 3; ++k) { b[k] = -1.0e308; b[3 + k] = 1.0e308; }
        return;
    }
    double e[3];
    sc_half_extents(s, e);
    for (int k = 0; k < 3; ++k) {
        const double t = s.pose[4 * k + 3], r = e[k] + a.res;
        b[k] = t - r;
        b[3 + k] = t + r;
    }
}

// World bounds of the centres of voxels v0 .. v1 (linear, inclusive): the index box that holds the run (one z run, whole z rows of
// one x, or whole x planes), through the origin, padded by a relative 2^-30 against the rounding of its own arithmetic.
__device__ void sc_region_bounds(const SceneArgs& a, int64_t v0, int64_t v1, double lo[3], double hi[3]) {
    int64_t i0[3], i1[3];
    if (a.n <= 0x7FFFFFFF) {                                                 // (uniform) 32-bit divisions where the indices fit
        const uint32_t plane = (uint32_t)(a.ny * a.nz), nz = (uint32_t)a.nz, u0 = (uint32_t)v0, u1 = (uint32_t)v1;
        const uint32_t x0 = u0 / plane, x1 = u1 / plane;
        i0[0] = x0; i1[0] = x1;
        if (x0 != x1) { i0[1] = 0; i1[1] = a.ny - 1; i0[2] = 0; i1[2] = a.nz - 1; }
        else {
            const uint32_t r0 = u0 - x0 * plane, r1 = u1 - x0 * plane, y0 = r0 / nz, y1 = r1 / nz;
            i0[1] = y0; i1[1] = y1;
            if (y0 != y1) { i0[2] = 0; i1[2] = a.nz - 1; }
            else { i0[2] = r0 - y0 * nz; i1[2] = r1 - y1 * nz; }
        }
    } else {
        const int64_t plane = a.ny * a.nz;
        i0[0] = v0 / plane; i1[0] = v1 / plane;
        if (i0[0] != i1[0]) { i0[1] = 0; i1[1] = a.ny - 1; i0[2] = 0; i1[2] = a.nz - 1; }
        else {
            const int64_t r0 = v0 - i0[0] * plane, r1 = v1 - i0[0] * plane;
            i0[1] = r0 / a.nz; i1[1] = r1 / a.nz;
            if (i0[1] != i1[1]) { i0[2] = 0; i1[2] = a.nz - 1; }
            else { i0[2] = r0 - i0[1] * a.nz; i1[2] = r1 - i1[1] * a.nz; }
        }
    }
    double mid[3], half[3];
    for (int k = 0; k < 3; ++k) {
        mid[k] = a.res * (0.5 * (double)(i0[k] + i1[k]) + 0.5);
        half[k] = a.res * (0.5 * (double)(i1[k] - i0[k]));
    }
    for (int r = 0; r < 3; ++r) {
        const double* o = a.origin + 4 * r;
        const double c = o[0] * mid[0] + o[1] * mid[1] + o[2] * mid[2] + o[3];
        double e = sc_abs(o[0]) * half[0] + sc_abs(o[1]) * half[1] + sc_abs(o[2]) * half[2];
        e = e + 9.313225746154785e-10 * (sc_abs(c) + e + a.res);
        lo[r] = c - e;
        hi[r] = c + e;
    }
}

// the shapes of word w (32 of them) whose bounds meet lo .. hi, among those of `among`
__device__ __forceinline__ uint32_t sc_meeting(const SceneArgs& a, int64_t w, uint32_t among, const double lo[3], const double hi[3]) {
    uint32_t out = 0;
    while (among) {
        const int bit = __ffs((int)among) - 1;
        among &= among - 1;
        const double* b = a.bounds + 6 * (w * 32 + bit);
        if (b[0] <= hi[0] && b[3] >= lo[0] && b[1] <= hi[1] && b[4] >= lo[1] && b[2] <= hi[2] && b[5] >= lo[2]) out |= 1u << bit;
    }
    return out;
}

__global__ __launch_bounds__(kScThreads) void k_sc_coarse(const SceneArgs a) {
    const int64_t i = sc_workgroup() * kScThreads + threadIdx.x;
    if (i >= a.n_coarse * a.n_words) return;
    const int64_t region = i / a.n_words, w = i - region * a.n_words;
    const int64_t v0 = region * a.coarse_voxels;
    const int64_t v1 = (v0 + a.coarse_voxels < a.n ? v0 + a.coarse_voxels : a.n) - 1;
    double lo[3], hi[3];
    sc_region_bounds(a, v0, v1, lo, hi);
    const int64_t left = a.n_shapes - w * 32;
    const uint32_t among = left >= 32 ? 0xFFFFFFFFu : (1u << (int)left) - 1u;
    a.cand[i] = sc_meeting(a, w, among, lo, hi);
}

template <bool IDS>
__global__ __launch_bounds__(kScThreads, 4) void k_sc_raster(const SceneArgs a) {
    __shared__ uint32_t fine[kScThreads];
    __shared__ unsigned long long nonzero[kScThreads / 64];
    const int64_t v0 = sc_workgroup() * kScThreads;
    if (v0 >= a.n) return;                                                   // (the last row of a two-dimensional launch)
    const int64_t v = v0 + threadIdx.x;
    const bool live = v < a.n;
    const bool refused = *a.status != kScNoBadShape;                         // (uniform) a refused shape: the outputs are cleared
    // the workgroup's own bounds, by every lane for itself: no LDS round trip and no barrier in front of the candidate loads
    double lo[3], hi[3];
    sc_region_bounds(a, v0, (v0 + kScThreads < a.n ? v0 + kScThreads : a.n) - 1, lo, hi);
    double c[3] = {0.0, 0.0, 0.0};
    bool have_centre = false;
    const uint32_t* cand = a.cand + (v0 / a.coarse_voxels) * a.n_words;
    bool hit = false;
    uint32_t id = 0;
    const int wave = threadIdx.x >> 6;
    for (int64_t base = 0; base < a.n_words && !refused; base += kScThreads) {
        const int64_t w = base + threadIdx.x;
        const uint32_t mine = w < a.n_words ? sc_meeting(a, w, cand[w], lo, hi) : 0u;
        fine[threadIdx.x] = mine;
        const unsigned long long any = __ballot(mine != 0);
        if ((threadIdx.x & 63) == 0) nonzero[wave] = any;
        __syncthreads();
        if (!have_centre && (nonzero[0] | nonzero[1] | nonzero[2] | nonzero[3])) {        // (uniform) the first survivors: now the centre is needed
            have_centre = true;
            if (live) {
                int64_t x, y, z;
                if (a.n <= 0x7FFFFFFF) {
                    const uint32_t u = (uint32_t)v, t = u / (uint32_t)a.nz;
                    z = u - t * (uint32_t)a.nz; x = t / (uint32_t)a.ny; y = t - (uint32_t)x * (uint32_t)a.ny;
                } else {
                    const int64_t t = v / a.nz;
                    z = v - t * a.nz; x = t / a.ny; y = t - x * a.ny;
                }
                sc_centre(a.origin, a.res, x, y, z, c);
            }
        }
        // every wave walks the same survivors, in list order; a lane that has its verdict sits the rest out
        for (int g = 0; g < kScThreads / 64; ++g) {
            unsigned long long words = nonzero[g];
            while (words) {
                if (__all(hit || !live)) { words = 0; break; }
                const int k = __ffsll((long long)words) - 1;
                words &= words - 1;
                uint32_t members = fine[g * 64 + k];
                const int64_t first = (base + g * 64 + k) * 32;
                while (members) {
                    const int bit = __ffs((int)members) - 1;
                    members &= members - 1;
                    const int s = __builtin_amdgcn_readfirstlane((int)(first + bit));
                    if (live && !hit) {
                        const sdfgpu_shape& shape = a.shapes[s];
                        if (sc_hit(shape, c, a.half)) { hit = true; id = shape.object_id; }
                    }
                }
            }
        }
        __syncthreads();                                                     // (fine and nonzero are rewritten by the next round)
    }
    const unsigned long long verdicts = __ballot(hit);
    if (a.bits && (threadIdx.x & 63) == 0) {
        const int64_t word = (v0 + wave * 64) >> 5, n_bit_words = (a.n + 31) >> 5;
        if (word < n_bit_words) a.bits[word] = (uint32_t)verdicts;
        if (word + 1 < n_bit_words) a.bits[word + 1] = (uint32_t)(verdicts >> 32);
    }
    if (live) {
        if (a.mask) a.mask[v] = hit ? 1 : 0;
        if (IDS) a.ids[v] = id;
    }
}

}  // namespace

// the three kernels on `s`, behind a memset of the status word
hipError_t scene_launch(const SceneArgs& a, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.status, 0xFF, kScStatusBytes, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sc_prepare, sc_grid((a.n_shapes + kScThreads - 1) / kScThreads), dim3(kScThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sc_coarse, sc_grid((a.n_coarse * a.n_words + kScThreads - 1) / kScThreads), dim3(kScThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 grid = sc_grid((a.n + kScThreads - 1) / kScThreads);
    if (a.ids) hipLaunchKernelGGL(k_sc_raster<true>, grid, dim3(kScThreads), 0, s, a);
    else hipLaunchKernelGGL(k_sc_raster<false>, grid, dim3(kScThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

int check_scene_args(sdfgpu_handle h, const sdfgpu_shape* shapes, int64_t n_shapes, const double* origin, double resolution, int64_t nx,
                     int64_t ny, int64_t nz, const void* bits, const void* mask, const void* ids, SceneArgs& a) {
    if (!origin) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: null origin");
    if (!bits && !mask && !ids) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: no output asked for");
    if (n_shapes < 0 || (n_shapes > 0 && !shapes)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: null shapes");
    if (n_shapes > kScMaxShapes)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: %lld shapes, the limit is %lld", (long long)n_shapes, (long long)kScMaxShapes);
    const int64_t kMaxCells = INT64_MAX / 16;
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx > kMaxCells / ny || nx * ny > kMaxCells / nz)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: unsupported grid %lld x %lld x %lld", (long long)nx, (long long)ny, (long long)nz);
    if (!(std::isfinite(resolution) && resolution > 0.0))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: the resolution must be positive and finite");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(origin[i])) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: origin entry %d is not finite", i);
    a = SceneArgs{};
    a.n_shapes = n_shapes; a.n_words = scene_shape_words(n_shapes);
    for (int i = 0; i < 12; ++i) a.origin[i] = origin[i];
    a.res = resolution; a.half = resolution * 0.5;
    a.nx = nx; a.ny = ny; a.nz = nz; a.n = nx * ny * nz;
    a.coarse_voxels = scene_coarse_voxels(a.n); a.n_coarse = scene_coarse_count(a.n);
    return SDFGPU_OK;
}

// a.shapes -> a.bits / a.mask / a.ids (device) on `st`; synchronises `st` only when out_bad_shape is asked for
int rasterize_impl(sdfgpu_handle h, SceneArgs& a, int64_t* out_bad_shape, hipStream_t st) {
    const size_t bit_bytes = (size_t)((a.n + 31) / 32) * 4;
    if (a.n_shapes == 0) {                                                   // nothing to test: the outputs are cleared
        if (a.bits) HIP_TRY(h, hipMemsetAsync(a.bits, 0, bit_bytes, st));
        if (a.mask) HIP_TRY(h, hipMemsetAsync(a.mask, 0, (size_t)a.n, st));
        if (a.ids) HIP_TRY(h, hipMemsetAsync(a.ids, 0, (size_t)a.n * 4, st));
        if (out_bad_shape) { HIP_TRY(h, hipStreamSynchronize(st)); *out_bad_shape = -1; }
        return SDFGPU_OK;
    }
    // the scratch belongs to the handle and the call may return with its kernels pending: a call on another stream waits for them
    // on the device first, as a resample does (ensure() below may free the scratch: hipFree waits for the device)
    HIP_TRY(h, h->sc_order.create());
    HIP_TRY(h, h->sc_order.wait(st));
    if (int rc = ensure(h, h->sc_scratch, scene_scratch_bytes(a.n, a.n_shapes), "shape rasteriser scratch")) return rc;
    char* const base = static_cast<char*>(h->sc_scratch.ptr);
    a.status = reinterpret_cast<uint32_t*>(base);
    a.bounds = reinterpret_cast<double*>(base + scene_bounds_offset());
    a.cand = reinterpret_cast<uint32_t*>(base + scene_cand_offset(a.n_shapes));
    const hipError_t le = scene_launch(a, st);
    (void)h->sc_order.record(st);                       // (also behind a failed launch: what it did enqueue is ordered)
    HIP_TRY(h, le);
    if (out_bad_shape) {
        uint32_t word = 0;
        HIP_TRY(h, hipMemcpyAsync(&word, a.status, sizeof word, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        *out_bad_shape = word == 0xFFFFFFFFu ? -1 : (int64_t)word;
        if (word != 0xFFFFFFFFu)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: shape %lld is refused (type, dims, pose or object id); the outputs are cleared",
                        (long long)word);
    }
    return SDFGPU_OK;
}

}  // namespace

extern "C" {

int sdfgpu_rasterize_shapes_device(sdfgpu_handle h, const sdfgpu_shape* d_shapes, int64_t n_shapes, const double origin[16], double voxel_size,
                                   int64_t nx, int64_t ny, int64_t nz, uint32_t* d_bits, uint8_t* d_mask, uint32_t* d_object_ids,
                                   int64_t* out_bad_shape, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        SceneArgs a;
        if (int rc = check_scene_args(h, d_shapes, n_shapes, origin, voxel_size, nx, ny, nz, d_bits, d_mask, d_object_ids, a)) return rc;
        if ((reinterpret_cast<uintptr_t>(d_shapes) & 7) || ((reinterpret_cast<uintptr_t>(d_bits) | reinterpret_cast<uintptr_t>(d_object_ids)) & 3))
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: d_shapes must be 8-byte aligned, d_bits and d_object_ids 4-byte aligned");
        HIP_TRY(h, hipSetDevice(h->device));
        a.shapes = d_shapes; a.bits = d_bits; a.mask = d_mask; a.ids = d_object_ids;
        return rasterize_impl(h, a, out_bad_shape, (hipStream_t)stream);
    });
}

int sdfgpu_rasterize_shapes(sdfgpu_handle h, const sdfgpu_shape* shapes, int64_t n_shapes, const double origin[16], double voxel_size,
                            int64_t nx, int64_t ny, int64_t nz, uint32_t* bits, uint8_t* mask, uint32_t* object_ids) {
    return rz_wrap(h, nullptr, [&]() -> int {
        SceneArgs a;
        if (int rc = check_scene_args(h, shapes, n_shapes, origin, voxel_size, nx, ny, nz, bits, mask, object_ids, a)) return rc;
        for (int64_t i = 0; i < n_shapes; ++i)
            if (!sc_shape_valid(shapes[i]) || (object_ids && shapes[i].object_id == 0))
                return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "rasterize_shapes: shape %lld is refused (type %u: a box, sphere or cylinder with finite "
                            "dims >= 0 or a plane with a finite non-zero normal, a finite pose and, for object ids, an id >= 1 is taken)", (long long)i, shapes[i].type);
        HIP_TRY(h, hipSetDevice(h->device));
        // the null stream throughout: the shapes through the cell staging, the outputs through the field staging
        const size_t shape_bytes = (size_t)n_shapes * sizeof(sdfgpu_shape);
        const size_t bit_bytes = (((size_t)((a.n + 31) / 32) * 4) + 255) & ~(size_t)255, mask_bytes = ((size_t)a.n + 255) & ~(size_t)255;
        const size_t off_mask = bits ? bit_bytes : 0, off_ids = off_mask + (mask ? mask_bytes : 0);
        if (int rc = stage_input(h, shape_bytes ? shape_bytes : 256)) return rc;
        if (int rc = ensure(h, h->stage_out, off_ids + (object_ids ? (size_t)a.n * 4 : 0), "output staging")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, shapes, shape_bytes)) return rc;
        char* const out = static_cast<char*>(h->stage_out.ptr);
        a.shapes = static_cast<const sdfgpu_shape*>(h->stage_in.ptr);
        a.bits = bits ? reinterpret_cast<uint32_t*>(out) : nullptr;
        a.mask = mask ? reinterpret_cast<uint8_t*>(out + off_mask) : nullptr;
        a.ids = object_ids ? reinterpret_cast<uint32_t*>(out + off_ids) : nullptr;
        if (int rc = rasterize_impl(h, a, nullptr, nullptr)) return rc;
        if (bits) if (int rc = copy_to_host(h, bits, a.bits, (size_t)((a.n + 31) / 32) * 4)) return rc;
        if (mask) if (int rc = copy_to_host(h, mask, a.mask, (size_t)a.n)) return rc;
        if (object_ids) if (int rc = copy_to_host(h, object_ids, a.ids, (size_t)a.n * 4)) return rc;
        return SDFGPU_OK;
    });
}

}  // extern "C"
