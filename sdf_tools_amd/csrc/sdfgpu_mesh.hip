// sdfgpu_mesh.hip -- the mesh rasteriser (sdfgpu_mesh.hpp, include/sdfgpu.h "Planes and triangle meshes"):
// five kernels, their launcher, the host orchestration and the C ABI entry points sdfgpu_rasterize_meshes*.  Compiled beside
// sdfgpu.hip and linked into the same libsdfgpu.so (sdf_tools_amd/build.py).
//
//   k_mr_meshes       one workgroup: refuses mesh records (status word), scans their triangle counts into first slots
//   k_mr_setup        one thread per slot (a triangle of a mesh): refuses it or writes its world vertices, its object id and the
//                     number of 16^3 tiles its index box splits into
//   k_mr_scan_blocks  exclusive scan of the tile counts within blocks of 1024 slots, one workgroup each; the blocks' sums
//   k_mr_scan_top     one workgroup: exclusive scan of the blocks' sums; the total number of work items (tiles)
//   k_mr_scatter      a fixed number of workgroups whose waves stride over chunks of 16 work items.  A wave finds the chunk's first
//                     slot by binary search in the scan; per tile its 64 lanes first judge the tile's 64 sub-tiles (4^3 voxels
//                     each) conservatively, then take the surviving sub-tiles one lane per voxel.  The verdicts of a sub-tile reach
//                     the bit field as one atomic OR per word, the mask as plain stores of 1, the ids as a bounded
//                     compare-and-swap "minimum over non-zero".
// No workgroup waits for another and every loop is bounded by a count computed before it.
//
// Arithmetic: the decision procedure may not be contracted into FMAs (sdfgpu_mesh.hpp).
#pragma clang fp contract(off)
#include "sdfgpu_context.hpp"
#include "sdfgpu_mesh_solid.hpp"
#include "sdfgpu.h"

namespace sdfgpu {

namespace {

// exclusive scan of one value per thread over the workgroup's kMrThreads threads; `total` is the sum, in every thread
__device__ int64_t mr_block_scan(int64_t v, int64_t& total) {
    __shared__ int64_t wave_sum[kMrThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t other = __shfl_up(inc, d, 64);
        if (lane >= d) inc += other;
    }
    __syncthreads();                                                         // (wave_sum may still be read from an earlier call)
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int w = 0; w < kMrThreads / 64; ++w) {
        if (w < wave) before += wave_sum[w];
        all += wave_sum[w];
    }
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kMrThreads) void k_mr_meshes(const MeshArgs a) {
    const int64_t per = (a.n_meshes + kMrThreads - 1) / kMrThreads;
    const int64_t m0 = (int64_t)threadIdx.x * per, m1 = m0 + per < a.n_meshes ? m0 + per : a.n_meshes;
    int64_t mine = 0;
    for (int64_t m = m0; m < m1; ++m) {
        if (mr_mesh_valid(a.meshes[m], a.n_vertices, a.n_triangles, a.ids != nullptr)) mine += a.meshes[m].n_triangles;
        else atomicMin(a.status, (uint32_t)m);
    }
    int64_t total;
    int64_t at = mr_block_scan(mine, total);
    for (int64_t m = m0; m < m1; ++m) {
        a.first[m] = at;
        if (mr_mesh_valid(a.meshes[m], a.n_vertices, a.n_triangles, a.ids != nullptr)) {
            at += a.meshes[m].n_triangles;
            if (at > a.n_triangles) atomicMin(a.status, (uint32_t)m);        // the triangle counts sum past the array
        }
    }
    if (threadIdx.x == 0) a.first[a.n_meshes] = total;
}

__global__ __launch_bounds__(kMrThreads) void k_mr_setup(const MeshArgs a) {
    const int64_t s = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (s >= a.n_triangles) return;
    int64_t count = 0;
    if (s < a.first[a.n_meshes]) {
        // the last mesh whose first slot is <= s (meshes without triangles share their first slot with the next one)
        int64_t lo = 0, hi = a.n_meshes;
        for (int step = 0; step < 20 && hi - lo > 1; ++step) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.first[mid] <= s) lo = mid; else hi = mid;
        }
        const sdfgpu_mesh& m = a.meshes[lo];
        double* W = a.world + 9 * s;
        if (mr_triangle_valid(m, a.vertices, a.triangles + 3 * (m.first_triangle + (s - a.first[lo])), W)) {
            MrTriangle t;
            mr_triangle(W, W + 3, W + 6, t);
            int64_t blo[3], bhi[3], per[3];
            mr_index_box(a, t, blo, bhi);
            count = mr_tiles(blo, bhi, per);
            a.slot_id[s] = m.object_id;
        } else {
            atomicMin(a.status, (uint32_t)lo);
        }
    }
    a.scan[s] = count;
}

__global__ __launch_bounds__(kMrThreads) void k_mr_scan_blocks(const MeshArgs a) {
    const int64_t base = (int64_t)blockIdx.x * kMrScanBlock + (int64_t)threadIdx.x * 4;
    int64_t v[4], mine = 0;
    for (int k = 0; k < 4; ++k) { v[k] = base + k < a.n_triangles ? a.scan[base + k] : 0; mine += v[k]; }
    int64_t total;
    int64_t at = mr_block_scan(mine, total);
    for (int k = 0; k < 4; ++k) {
        if (base + k < a.n_triangles) a.scan[base + k] = at;
        at += v[k];
    }
    if (threadIdx.x == 0) a.top[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMrThreads) void k_mr_scan_top(const MeshArgs a) {
    const int64_t blocks = mr_scan_blocks(a.n_triangles);
    const int64_t per = (blocks + kMrThreads - 1) / kMrThreads;
    const int64_t b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
    int64_t mine = 0;
    for (int64_t b = b0; b < b1; ++b) mine += a.top[b];
    int64_t total;
    int64_t at = mr_block_scan(mine, total);
    for (int64_t b = b0; b < b1; ++b) { const int64_t v = a.top[b]; a.top[b] = at; at += v; }
    if (threadIdx.x == 0) {
        a.top[blocks] = total;
        *reinterpret_cast<int64_t*>(a.status + 2) = total;
    }
}

// the first work item of slot s (s == n_triangles: the total)
__device__ __forceinline__ int64_t mr_first_item(const MeshArgs& a, int64_t s, int64_t total) {
    return s < a.n_triangles ? a.scan[s] + a.top[s / kMrScanBlock] : total;
}

// the slot that work item i belongs to: the last one whose first item is <= i (a slot without tiles shares it with the next)
__device__ int64_t mr_slot_of(const MeshArgs& a, int64_t i, int64_t total) {
    int64_t lo = 0, hi = a.n_triangles;
    for (int step = 0; step < 26 && hi - lo > 1; ++step) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (mr_first_item(a, mid, total) <= i) lo = mid; else hi = mid;
    }
    return lo;
}

template <bool IDS>
__global__ __launch_bounds__(kMrThreads) void k_mr_scatter(const MeshArgs a) {
    if (*a.status != kMrNoBadMesh) return;                                   // a refused mesh: nothing is written
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kMrThreads / 64) + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * (kMrThreads / 64);
    const int64_t total = *reinterpret_cast<const int64_t*>(a.status + 2);
    const int64_t chunks = (total + kMrChunk - 1) / kMrChunk;
    const int id_tries = (int)a.n_meshes + 2;
    const int sx = lane >> 4, sy = (lane >> 2) & 3, sz = lane & 3;           // a lane's sub-tile of a tile, and its voxel of a sub-tile
    // the world box that holds the probes of a sub-tile about the centre of its middle: 1.5 voxels each way in the grid frame
    double H[3];
    for (int r = 0; r < 3; ++r)
        H[r] = a.half + 1.5 * (a.res * (sc_abs(a.origin[4 * r]) + sc_abs(a.origin[4 * r + 1]) + sc_abs(a.origin[4 * r + 2])));
    for (int64_t chunk = wave; chunk < chunks; chunk += waves) {
        const int64_t i0 = chunk * kMrChunk, i1 = i0 + kMrChunk < total ? i0 + kMrChunk : total;
        int64_t s = mr_slot_of(a, i0, total);
        for (int64_t i = i0; i < i1; ++i) {
            if (i >= mr_first_item(a, s + 1, total)) {
                ++s;
                if (i >= mr_first_item(a, s + 1, total)) s = mr_slot_of(a, i, total);
            }
            s = __builtin_amdgcn_readfirstlane((int)s);                      // (uniform by construction; slots are below 2^24)
            const double* W = a.world + 9 * s;
            MrTriangle t;
            mr_triangle(W, W + 3, W + 6, t);
            int64_t blo[3], bhi[3], per[3];
            mr_index_box(a, t, blo, bhi);
            mr_tiles(blo, bhi, per);
            const int64_t k = i - mr_first_item(a, s, total);
            const int64_t kxy = k / per[2];
            const int64_t tz = k - kxy * per[2], tx = kxy / per[1], ty = kxy - tx * per[1];
            const int64_t t0[3] = {blo[0] + tx * kMrTile, blo[1] + ty * kMrTile, blo[2] + tz * kMrTile};
            // sub-tiles: one per lane
            bool may = false;
            {
                const int64_t q[3] = {t0[0] + sx * kMrSub, t0[1] + sy * kMrSub, t0[2] + sz * kMrSub};
                if (q[0] <= bhi[0] && q[1] <= bhi[1] && q[2] <= bhi[2]) {
                    double c[3];
                    sc_centre(a.origin, a.res, q[0], q[1], q[2], c);         // the centre of voxel q, then 1.5 voxels on along each grid axis
                    for (int r = 0; r < 3; ++r)
                        c[r] = c[r] + 1.5 * (a.res * ((a.origin[4 * r] + a.origin[4 * r + 1]) + a.origin[4 * r + 2]));
                    may = mr_may_hit(t, c, H);
                }
            }
            unsigned long long todo = __ballot(may);
            const uint32_t oid = IDS ? a.slot_id[s] : 0u;
            for (int left = __popcll(todo); left > 0; --left) {
                const int sub = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int64_t x = t0[0] + (sub >> 4) * kMrSub + sx, y = t0[1] + ((sub >> 2) & 3) * kMrSub + sy, z = t0[2] + (sub & 3) * kMrSub + sz;
                const bool live = x <= bhi[0] && y <= bhi[1] && z <= bhi[2];
                bool hit = false;
                if (live) {
                    double c[3];
                    sc_centre(a.origin, a.res, x, y, z, c);
                    hit = mr_hit(t, c, a.half);
                }
                if (__ballot(hit) == 0) continue;
                // linear indices ascend with the lane (coordinates outside the box clamped to it), so the lanes of one bit word
                // are consecutive: a suffix OR within runs of equal words, and the first lane of a run issues the atomic
                const int64_t xc = x < bhi[0] ? x : bhi[0], yc = y < bhi[1] ? y : bhi[1], zc = z < bhi[2] ? z : bhi[2];
                const int64_t v = (xc * a.ny + yc) * a.nz + zc;
                if (a.bits) {
                    const int64_t word = v >> 5;
                    uint32_t m = hit ? 1u << (int)(v & 31) : 0u;
                    const uint32_t wlo = (uint32_t)word, whi = (uint32_t)(word >> 32);
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t om = __shfl_down(m, d, 64), olo = __shfl_down(wlo, d, 64), ohi = __shfl_down(whi, d, 64);
                        if (lane + d < 64 && olo == wlo && ohi == whi) m |= om;
                    }
                    const uint32_t plo = __shfl_up(wlo, 1, 64), phi = __shfl_up(whi, 1, 64);
                    if (m && (lane == 0 || plo != wlo || phi != whi)) atomicOr(a.bits + word, m);
                }
                if (hit) {
                    if (a.mask) a.mask[v] = 1;
                    if (IDS) {
                        // the smallest non-zero id: a failed exchange means another one went through, and an id only ever descends
                        uint32_t seen = __hip_atomic_load(a.ids + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        for (int tries = 0; tries < id_tries; ++tries) {
                            if (seen != 0 && seen <= oid) break;
                            const uint32_t was = atomicCAS(a.ids + v, seen, oid);
                            if (was == seen) break;
                            seen = was;
                        }
                    }
                }
            }
        }
    }
}

}  // namespace

// the kernels on `s`, behind a memset of the status block, in three parts that the solid call (sdfgpu_mesh_solid.hip) interleaves
// with its own: the checks and world vertices | the scan of a.scan into a.top and the total | the scatter
hipError_t mesh_launch_setup(const MeshArgs& a, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.status, 0xFF, kScStatusBytes, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mr_meshes, dim3(1), dim3(kMrThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.n_triangles > 0) {
        hipLaunchKernelGGL(k_mr_setup, dim3((unsigned)((a.n_triangles + kMrThreads - 1) / kMrThreads)), dim3(kMrThreads), 0, s, a);
        e = hipGetLastError();
    }
    return e;
}

hipError_t mesh_launch_scan(const MeshArgs& a, hipStream_t s) {
    if (a.n_triangles > 0) {
        hipLaunchKernelGGL(k_mr_scan_blocks, dim3((unsigned)mr_scan_blocks(a.n_triangles)), dim3(kMrThreads), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_mr_scan_top, dim3(1), dim3(kMrThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t mesh_launch_scatter(const MeshArgs& a, hipStream_t s) {
    if (a.n_triangles <= 0) return hipSuccess;
    if (a.ids) hipLaunchKernelGGL(k_mr_scatter<true>, dim3(kMrScatterGroups), dim3(kMrThreads), 0, s, a);
    else hipLaunchKernelGGL(k_mr_scatter<false>, dim3(kMrScatterGroups), dim3(kMrThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t mesh_launch(const MeshArgs& a, hipStream_t s) {
    hipError_t e = mesh_launch_setup(a, s);
    if (e == hipSuccess) e = mesh_launch_scan(a, s);
    if (e == hipSuccess) e = mesh_launch_scatter(a, s);
    return e;
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

int check_mesh_args(sdfgpu_handle h, const sdfgpu_mesh* meshes, int64_t n_meshes, const double* vertices, int64_t n_vertices,
                    const uint32_t* triangles, int64_t n_triangles, const double* origin, double resolution, int64_t nx, int64_t ny, int64_t nz,
                    const void* bits, const void* mask, const void* ids, int accumulate, MeshArgs& a, bool solid = false) {
    const char* const who = solid ? "rasterize_solid_meshes" : "rasterize_meshes";
    if (!origin) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: null origin", who);
    if (!bits && !mask && !ids) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: no output asked for", who);
    if (accumulate != 0 && accumulate != 1) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: accumulate must be 0 or 1", who);
    if (n_meshes < 0 || n_meshes > kMrMaxMeshes)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: %lld meshes, the limit is %lld", who, (long long)n_meshes, (long long)kMrMaxMeshes);
    if (solid && n_meshes > kMsMaxMeshes)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: %lld meshes, the limit is %lld (one pair of launches each)", who, (long long)n_meshes, (long long)kMsMaxMeshes);
    if (n_triangles < 0 || n_triangles > kMrMaxTriangles)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: %lld triangles, the limit is %lld", who, (long long)n_triangles, (long long)kMrMaxTriangles);
    if (n_vertices < 0 || n_vertices > ((int64_t)1 << 32))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: %lld vertices, the limit is 2^32", who, (long long)n_vertices);
    if ((n_meshes > 0 && !meshes) || (n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: null meshes, vertices or triangles", who);
    if ((reinterpret_cast<uintptr_t>(meshes) | reinterpret_cast<uintptr_t>(vertices)) & 7)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: meshes and vertices must be 8-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(triangles) | reinterpret_cast<uintptr_t>(bits) | reinterpret_cast<uintptr_t>(ids)) & 3)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: triangles, bits and object ids must be 4-byte aligned", who);
    const int64_t kMaxCells = INT64_MAX / 16;
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx > kMaxCells / ny || nx * ny > kMaxCells / nz)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: unsupported grid %lld x %lld x %lld", who, (long long)nx, (long long)ny, (long long)nz);
    if (!(std::isfinite(resolution) && resolution > 0.0))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: the resolution must be positive and finite", who);
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(origin[i])) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: origin entry %d is not finite", who, i);
    a = MeshArgs{};
    a.n_meshes = n_meshes; a.n_vertices = n_vertices; a.n_triangles = n_triangles;
    for (int i = 0; i < 12; ++i) a.origin[i] = origin[i];
    // the inverse of the origin's 3 x 3 block by cofactors: for the index boxes, and the frame of the solid fill
    a.no_inverse = ms_inverse(origin, a.inverse) ? 0 : 1;
    a.res = resolution; a.half = resolution * 0.5;
    a.nx = nx; a.ny = ny; a.nz = nz; a.n = nx * ny * nz;
    a.accumulate = accumulate;
    if (solid && a.no_inverse)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: the origin's 3 x 3 block has no inverse (the fill works in grid coordinates)", who);
    return SDFGPU_OK;
}

// a.meshes, a.vertices, a.triangles -> a.bits / a.mask / a.ids (device) on `st`; synchronises `st` only when out_bad_mesh is asked for
// solid: the meshes are also filled inside (sdfgpu_mesh_solid.hpp); the toggle field is the handle's and all zero between calls
int rasterize_meshes_impl(sdfgpu_handle h, MeshArgs& a, int64_t* out_bad_mesh, hipStream_t st, bool solid = false) {
    const char* const who = solid ? "rasterize_solid_meshes" : "rasterize_meshes";
    if (!a.accumulate) {
        if (a.bits) HIP_TRY(h, hipMemsetAsync(a.bits, 0, (size_t)((a.n + 31) / 32) * 4, st));
        if (a.mask) HIP_TRY(h, hipMemsetAsync(a.mask, 0, (size_t)a.n, st));
        if (a.ids) HIP_TRY(h, hipMemsetAsync(a.ids, 0, (size_t)a.n * 4, st));
    }
    if (a.n_meshes == 0) {
        if (out_bad_mesh) { HIP_TRY(h, hipStreamSynchronize(st)); *out_bad_mesh = -1; }
        return SDFGPU_OK;
    }
    // the scratch belongs to the handle and the call may return with its kernels pending: a call on another stream waits for them
    // on the device first, as a shape rasterisation does (ensure() below may free the scratch: hipFree waits for the device)
    HIP_TRY(h, h->mr_order.create());
    HIP_TRY(h, h->mr_order.wait(st));
    if (int rc = ensure(h, h->mr_scratch, solid ? mesh_solid_scratch_bytes(a.n_meshes, a.n_triangles) : mesh_scratch_bytes(a.n_meshes, a.n_triangles),
                        "mesh rasteriser scratch")) return rc;
    char* const base = static_cast<char*>(h->mr_scratch.ptr);
    a.status = reinterpret_cast<uint32_t*>(base);
    a.first = reinterpret_cast<int64_t*>(base + mr_first_offset());
    a.top = reinterpret_cast<int64_t*>(base + mr_top_offset(a.n_meshes));
    a.scan = reinterpret_cast<int64_t*>(base + mr_scan_offset(a.n_meshes, a.n_triangles));
    a.world = reinterpret_cast<double*>(base + mr_world_offset(a.n_meshes, a.n_triangles));
    a.slot_id = reinterpret_cast<uint32_t*>(base + mr_id_offset(a.n_meshes, a.n_triangles));
    hipError_t le;
    if (solid) {
        SolidArgs sa{};
        sa.wz = ms_row_words(a.nz);
        const size_t toggle_bytes = (size_t)(a.nx * a.ny * sa.wz) * 4;
        const void* const had = h->ms_toggle.bytes >= toggle_bytes ? h->ms_toggle.ptr : nullptr;
        if (int rc = ensure(h, h->ms_toggle, toggle_bytes, "solid mesh toggle field")) return rc;
        if (h->ms_toggle.ptr != had || h->ms_dirty) HIP_TRY(h, hipMemsetAsync(h->ms_toggle.ptr, 0, h->ms_toggle.bytes, st));
        sa.m = a;
        sa.scan = reinterpret_cast<int64_t*>(base + ms_scan_offset(a.n_meshes, a.n_triangles));
        sa.top = reinterpret_cast<int64_t*>(base + ms_top_offset(a.n_meshes, a.n_triangles));
        sa.box_lo = reinterpret_cast<unsigned long long*>(base + ms_box_offset(a.n_meshes, a.n_triangles));
        sa.box_hi = reinterpret_cast<unsigned long long*>(base + ms_box_offset(a.n_meshes, a.n_triangles) + ms_box_bytes(a.n_meshes));
        sa.toggle = static_cast<uint32_t*>(h->ms_toggle.ptr);
        h->ms_dirty = true;                             // (until every merge that clears what a scatter set is enqueued)
        le = mesh_solid_launch(sa, st);
        if (le == hipSuccess) h->ms_dirty = false;
    } else {
        le = mesh_launch(a, st);
    }
    (void)h->mr_order.record(st);                       // (also behind a failed launch: what it did enqueue is ordered)
    HIP_TRY(h, le);
    if (out_bad_mesh) {
        uint32_t word = 0;
        HIP_TRY(h, hipMemcpyAsync(&word, a.status, sizeof word, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        *out_bad_mesh = word == kMrNoBadMesh ? -1 : (int64_t)word;
        if (word != kMrNoBadMesh)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: mesh %lld is refused (ranges, pose, vertices, vertex indices or object id%s); "
                        "the outputs are %s", who, (long long)word, solid ? ", or a vertex whose grid coordinates are not finite" : "",
                        a.accumulate ? "unchanged" : "cleared");
    }
    return SDFGPU_OK;
}

}  // namespace

extern "C" {

static int rasterize_meshes_device_form(bool solid, sdfgpu_handle h, const sdfgpu_mesh* d_meshes, int64_t n_meshes, const double* d_vertices, int64_t n_vertices,
                                   const uint32_t* d_triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx,
                                   int64_t ny, int64_t nz, uint32_t* d_bits, uint8_t* d_mask, uint32_t* d_object_ids, int accumulate,
                                   int64_t* out_bad_mesh, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        MeshArgs a;
        if (int rc = check_mesh_args(h, d_meshes, n_meshes, d_vertices, n_vertices, d_triangles, n_triangles, origin, voxel_size, nx, ny, nz,
                                     d_bits, d_mask, d_object_ids, accumulate, a, solid)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        a.meshes = d_meshes; a.vertices = d_vertices; a.triangles = d_triangles;
        a.bits = d_bits; a.mask = d_mask; a.ids = d_object_ids;
        return rasterize_meshes_impl(h, a, out_bad_mesh, (hipStream_t)stream, solid);
    });
}

static int rasterize_meshes_host_form(bool solid, sdfgpu_handle h, const sdfgpu_mesh* meshes, int64_t n_meshes, const double* vertices, int64_t n_vertices,
                            const uint32_t* triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx, int64_t ny,
                            int64_t nz, uint32_t* bits, uint8_t* mask, uint32_t* object_ids) {
    return rz_wrap(h, nullptr, [&]() -> int {
        MeshArgs a;
        if (int rc = check_mesh_args(h, meshes, n_meshes, vertices, n_vertices, triangles, n_triangles, origin, voxel_size, nx, ny, nz, bits,
                                     mask, object_ids, 0, a, solid)) return rc;
        const char* const who = solid ? "rasterize_solid_meshes" : "rasterize_meshes";
        int64_t slots = 0;
        for (int64_t m = 0; m < n_meshes; ++m) {
            const sdfgpu_mesh& mesh = meshes[m];
            bool ok = mr_mesh_valid(mesh, n_vertices, n_triangles, object_ids != nullptr);
            if (ok) { slots += mesh.n_triangles; ok = slots <= n_triangles; }
            double W[9];
            for (int64_t j = 0; ok && j < mesh.n_triangles; ++j) {
                ok = mr_triangle_valid(mesh, vertices, triangles + 3 * (mesh.first_triangle + j), W);
                double G[3][3];
                if (ok && solid) ok = ms_grid_triangle(a, W, G);
            }
            if (!ok)
                return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: mesh %lld is refused (its triangle and vertex runs must lie inside the "
                            "arrays and its triangles, with those of the meshes before it, number n_triangles at most; a finite pose, finite "
                            "vertices, vertex indices below its n_vertices and, for object ids, an id other than 0 and 0xFFFFFFFF are taken%s)", who, (long long)m,
                            solid ? "; for the fill, grid coordinates that are finite" : "");
        }
        if (solid) {                                    // every record and vertex is valid by now: what is left is an open mesh, or no memory
            int64_t bad_mesh = -1, bad_triangle = -1;
            if (sdfgpu_check_closed_meshes(meshes, n_meshes, vertices, n_vertices, triangles, n_triangles, &bad_mesh, &bad_triangle) != SDFGPU_OK) {
                if (bad_mesh < 0 || bad_triangle < 0)
                    return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: the closedness check could not be made (out of host memory?)", who);
                return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s: mesh %lld is not closed: an edge of its triangle %lld is used by an odd number of "
                            "triangles", who, (long long)bad_mesh, (long long)bad_triangle);
            }
        }
        HIP_TRY(h, hipSetDevice(h->device));
        // the null stream throughout: meshes | vertices | triangles through the cell staging, the outputs through the field staging
        const size_t mesh_bytes = (size_t)n_meshes * sizeof(sdfgpu_mesh), vertex_bytes = (size_t)n_vertices * 24, triangle_bytes = (size_t)n_triangles * 12;
        const size_t off_v = mr_round(mesh_bytes), off_t = off_v + mr_round(vertex_bytes);
        const size_t bit_bytes = mr_round((size_t)((a.n + 31) / 32) * 4), mask_bytes = mr_round((size_t)a.n);
        const size_t off_mask = bits ? bit_bytes : 0, off_ids = off_mask + (mask ? mask_bytes : 0);
        if (int rc = stage_input(h, off_t + mr_round(triangle_bytes) + 256)) return rc;
        if (int rc = ensure(h, h->stage_out, off_ids + (object_ids ? (size_t)a.n * 4 : 0), "output staging")) return rc;
        char* const in = static_cast<char*>(h->stage_in.ptr);
        if (mesh_bytes) if (int rc = copy_from_host(h, in, meshes, mesh_bytes)) return rc;
        if (vertex_bytes) if (int rc = copy_from_host(h, in + off_v, vertices, vertex_bytes)) return rc;
        if (triangle_bytes) if (int rc = copy_from_host(h, in + off_t, triangles, triangle_bytes)) return rc;
        char* const out = static_cast<char*>(h->stage_out.ptr);
        a.meshes = reinterpret_cast<const sdfgpu_mesh*>(in);
        a.vertices = reinterpret_cast<const double*>(in + off_v);
        a.triangles = reinterpret_cast<const uint32_t*>(in + off_t);
        a.bits = bits ? reinterpret_cast<uint32_t*>(out) : nullptr;
        a.mask = mask ? reinterpret_cast<uint8_t*>(out + off_mask) : nullptr;
        a.ids = object_ids ? reinterpret_cast<uint32_t*>(out + off_ids) : nullptr;
        if (int rc = rasterize_meshes_impl(h, a, nullptr, nullptr, solid)) return rc;
        if (bits) if (int rc = copy_to_host(h, bits, a.bits, (size_t)((a.n + 31) / 32) * 4)) return rc;
        if (mask) if (int rc = copy_to_host(h, mask, a.mask, (size_t)a.n)) return rc;
        if (object_ids) if (int rc = copy_to_host(h, object_ids, a.ids, (size_t)a.n * 4)) return rc;
        return SDFGPU_OK;
    });
}

int sdfgpu_rasterize_meshes_device(sdfgpu_handle h, const sdfgpu_mesh* d_meshes, int64_t n_meshes, const double* d_vertices, int64_t n_vertices,
                                   const uint32_t* d_triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx,
                                   int64_t ny, int64_t nz, uint32_t* d_bits, uint8_t* d_mask, uint32_t* d_object_ids, int accumulate,
                                   int64_t* out_bad_mesh, void* stream) {
    return rasterize_meshes_device_form(false, h, d_meshes, n_meshes, d_vertices, n_vertices, d_triangles, n_triangles, origin, voxel_size, nx, ny, nz,
                                        d_bits, d_mask, d_object_ids, accumulate, out_bad_mesh, stream);
}

int sdfgpu_rasterize_solid_meshes_device(sdfgpu_handle h, const sdfgpu_mesh* d_meshes, int64_t n_meshes, const double* d_vertices, int64_t n_vertices,
                                         const uint32_t* d_triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx,
                                         int64_t ny, int64_t nz, uint32_t* d_bits, uint8_t* d_mask, uint32_t* d_object_ids, int accumulate,
                                         int64_t* out_bad_mesh, void* stream) {
    return rasterize_meshes_device_form(true, h, d_meshes, n_meshes, d_vertices, n_vertices, d_triangles, n_triangles, origin, voxel_size, nx, ny, nz,
                                        d_bits, d_mask, d_object_ids, accumulate, out_bad_mesh, stream);
}

int sdfgpu_rasterize_meshes(sdfgpu_handle h, const sdfgpu_mesh* meshes, int64_t n_meshes, const double* vertices, int64_t n_vertices,
                            const uint32_t* triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx, int64_t ny,
                            int64_t nz, uint32_t* bits, uint8_t* mask, uint32_t* object_ids) {
    return rasterize_meshes_host_form(false, h, meshes, n_meshes, vertices, n_vertices, triangles, n_triangles, origin, voxel_size, nx, ny, nz, bits,
                                      mask, object_ids);
}

int sdfgpu_rasterize_solid_meshes(sdfgpu_handle h, const sdfgpu_mesh* meshes, int64_t n_meshes, const double* vertices, int64_t n_vertices,
                                  const uint32_t* triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx, int64_t ny,
                                  int64_t nz, uint32_t* bits, uint8_t* mask, uint32_t* object_ids) {
    return rasterize_meshes_host_form(true, h, meshes, n_meshes, vertices, n_vertices, triangles, n_triangles, origin, voxel_size, nx, ny, nz, bits,
                                      mask, object_ids);
}

}  // extern "C"
