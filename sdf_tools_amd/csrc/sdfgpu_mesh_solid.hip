// sdfgpu_mesh_solid.hip -- solid fill of closed meshes (sdfgpu_mesh_solid.hpp, include/sdfgpu.h "Solid meshes"):
// three kernels and their launcher beside the surface pass of sdfgpu_mesh.hip, and the host-only closedness check.  The entry
// points sdfgpu_rasterize_solid_meshes* are in sdfgpu_mesh.hip, next to the argument checks and the staging they share.
//
//   k_ms_setup    one thread per slot: the triangle's grid vertices (refused when not finite), the number of 16 x 16 column tiles
//                 of its xy index box, and that box into the mesh's column box (64-bit atomic minimum and maximum)
//   k_ms_scatter  one mesh: a fixed number of workgroups whose waves stride over chunks of 16 work items (column tiles) of that
//                 mesh's slots.  One lane per column, four rows of a tile a pass; a crossing is one no-return atomic XOR of one bit
//                 of the toggle field, at the first cell of the column whose centre is above it
//   k_ms_merge    one mesh: over the columns of its column box.  A column's toggle words are read and cleared, the prefix parity
//                 within a word is five shift-XOR steps, the carry across words a ballot of the words' top bits (chunks of 64 words
//                 with a carry between them); the parity words are funnel-shifted onto the unpadded bit field and ORed in, the
//                 mask gets stores of 1 and the ids the bounded compare-and-swap minimum of the surface pass.
// Between the two the tile counts go through k_mr_scan_blocks and k_mr_scan_top (mesh_launch_scan).  No workgroup waits for
// another, every loop is bounded by a count computed before it, and XOR, OR and minimum commute: the result depends neither on
// scheduling nor on the order of triangles or meshes.
#pragma clang fp contract(off)
#include <algorithm>
#include <cstring>
#include <vector>

#include "sdfgpu_context.hpp"
#include "sdfgpu_mesh_solid.hpp"
#include "sdfgpu.h"

namespace sdfgpu {

namespace {

__global__ __launch_bounds__(kMrThreads) void k_ms_setup(const SolidArgs a) {
    const MeshArgs& m = a.m;
    const int64_t s = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (s >= m.n_triangles) return;
    int64_t count = 0;
    // The status word is not consulted: it changes while this kernel runs, and the lowest refused index must not depend on who saw
    // it when.  A slot whose triangle k_mr_setup refused holds stale world vertices; judged here it can at worst refuse its own
    // mesh once more, and its box is clipped to the grid like any other.
    if (s < m.first[m.n_meshes]) {
        int64_t lo = 0, hi = m.n_meshes;
        for (int step = 0; step < 20 && hi - lo > 1; ++step) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (m.first[mid] <= s) lo = mid; else hi = mid;
        }
        double G[3][3];
        if (ms_grid_triangle(m, m.world + 9 * s, G)) {
            int64_t blo[2], bhi[2], per[2];
            ms_column_box(m, G, blo, bhi);
            count = ms_tiles(blo, bhi, per);
            if (count > 0) {
                atomicMin(a.box_lo + 2 * lo, (unsigned long long)blo[0]);
                atomicMin(a.box_lo + 2 * lo + 1, (unsigned long long)blo[1]);
                atomicMax(a.box_hi + 2 * lo, (unsigned long long)bhi[0] + 1);
                atomicMax(a.box_hi + 2 * lo + 1, (unsigned long long)bhi[1] + 1);
            }
        } else {
            atomicMin(m.status, (uint32_t)lo);
        }
    }
    a.scan[s] = count;
}

// the first work item of slot s (s == n_triangles: the total)
__device__ __forceinline__ int64_t ms_first_item(const SolidArgs& a, int64_t s, int64_t total) {
    return s < a.m.n_triangles ? a.scan[s] + a.top[s / kMrScanBlock] : total;
}

// the slot of [s0, s1) that work item i belongs to: the last one whose first item is <= i
__device__ int64_t ms_slot_of(const SolidArgs& a, int64_t i, int64_t s0, int64_t s1, int64_t total) {
    int64_t lo = s0, hi = s1;
    for (int step = 0; step < 26 && hi - lo > 1; ++step) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ms_first_item(a, mid, total) <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kMrThreads) void k_ms_scatter(const SolidArgs a) {
    const MeshArgs& m = a.m;
    if (*m.status != kMrNoBadMesh) return;                                   // a refused mesh: nothing is written
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kMrThreads / 64) + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * (kMrThreads / 64);
    const int64_t total = a.top[mr_scan_blocks(m.n_triangles)];
    const int64_t s0 = m.first[a.mesh], s1 = m.first[a.mesh + 1];
    if (s1 <= s0) return;
    const int64_t item0 = ms_first_item(a, s0, total), item1 = ms_first_item(a, s1, total);
    const int64_t chunks = (item1 - item0 + kMrChunk - 1) / kMrChunk;
    for (int64_t chunk = wave; chunk < chunks; chunk += waves) {
        const int64_t i0 = item0 + chunk * kMrChunk, i1 = i0 + kMrChunk < item1 ? i0 + kMrChunk : item1;
        int64_t s = ms_slot_of(a, i0, s0, s1, total);
        for (int64_t i = i0; i < i1; ++i) {
            if (i >= ms_first_item(a, s + 1, total)) {
                ++s;
                if (i >= ms_first_item(a, s + 1, total)) s = ms_slot_of(a, i, s0, s1, total);
            }
            s = __builtin_amdgcn_readfirstlane((int)s);                      // (uniform by construction; slots are below 2^24)
            double G[3][3];
            ms_grid_triangle(m, m.world + 9 * s, G);
            int64_t blo[2], bhi[2], per[2];
            ms_column_box(m, G, blo, bhi);
            ms_tiles(blo, bhi, per);
            const int64_t k = i - ms_first_item(a, s, total);
            const int64_t tx = k / per[1], ty = k - tx * per[1];
            const int64_t x0 = blo[0] + tx * kMsTile, y = blo[1] + ty * kMsTile + (lane & 15);
            for (int pass = 0; pass < kMsTile / 4; ++pass) {
                const int64_t x = x0 + pass * 4 + (lane >> 4);
                if (x0 + pass * 4 > bhi[0]) break;                           // (uniform)
                if (x > bhi[0] || y > bhi[1]) continue;
                const double C[2] = {m.res * ((double)x + 0.5), m.res * ((double)y + 0.5)};
                double zc;
                if (!ms_crossing(G, C, zc)) continue;
                const int64_t cell = ms_first_above(m.res, m.nz, zc);
                if (cell < m.nz) atomicXor(a.toggle + (x * m.ny + y) * a.wz + (cell >> 5), 1u << (int)(cell & 31));
            }
        }
    }
}

template <bool IDS>
__global__ __launch_bounds__(kMrThreads) void k_ms_merge(const SolidArgs a) {
    const MeshArgs& m = a.m;
    if (*m.status != kMrNoBadMesh) return;
    // a mesh none of whose triangles reaches the grid's columns still has its lows at all ones and its highs at 0: compared as
    // unsigned, and the highs against the grid, before anything is indexed with them
    const unsigned long long uxlo = a.box_lo[2 * a.mesh], uylo = a.box_lo[2 * a.mesh + 1];
    const unsigned long long uxhi = a.box_hi[2 * a.mesh], uyhi = a.box_hi[2 * a.mesh + 1];               // one past
    if (uxhi <= uxlo || uyhi <= uylo || uxhi > (unsigned long long)m.nx || uyhi > (unsigned long long)m.ny) return;
    const int64_t xlo = (int64_t)uxlo, ylo = (int64_t)uylo, xhi = (int64_t)uxhi, yhi = (int64_t)uyhi;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kMrThreads / 64) + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * (kMrThreads / 64);
    // a column takes a group of `group` lanes, the least power of two that holds its words (64 at the most: longer columns go in chunks)
    int group = 1;
    for (int step = 0; step < 6 && group < a.wz; ++step) group <<= 1;
    const int per_wave = 64 / group, j0 = lane & (group - 1);
    const unsigned long long group_mask = (group == 64 ? ~0ull : ((1ull << group) - 1)) << (lane - j0);
    const unsigned long long below = group_mask & ((1ull << lane) - 1);
    const int64_t chunks = (a.wz + group - 1) / group;
    const int64_t bh = yhi - ylo, columns = (xhi - xlo) * bh, steps = (columns + per_wave - 1) / per_wave;
    const uint32_t oid = IDS ? m.meshes[a.mesh].object_id : 0u;
    const int id_tries = (int)m.n_meshes + 2;
    const uint32_t tail = (m.nz & 31) ? (1u << (int)(m.nz & 31)) - 1 : 0xFFFFFFFFu;
    for (int64_t st = wave; st < steps; st += waves) {
        const int64_t col = st * per_wave + (lane / group);
        const bool live = col < columns;
        const int64_t x = xlo + (live ? col / bh : 0), y = ylo + (live ? col % bh : 0);
        uint32_t* const row = a.toggle + (x * m.ny + y) * a.wz;
        const int64_t b0 = (x * m.ny + y) * m.nz;
        const int sh = (int)(b0 & 31);
        uint32_t carry = 0, before = 0;                                      // the parity below this chunk; the word before its first
        for (int64_t ch = 0; ch < chunks; ++ch) {
            const int64_t j = ch * group + j0;
            const bool valid = live && j < a.wz;
            uint32_t w = valid ? row[j] : 0u;
            if (w) row[j] = 0u;
            w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16;
            const unsigned long long tops = __ballot(w >> 31);
            if ((__popcll(tops & below) & 1) ^ carry) w = ~w;
            carry ^= (uint32_t)(__popcll(tops & group_mask) & 1);
            if (!valid) w = 0u;
            else if (j == a.wz - 1) w &= tail;
            // onto the unpadded field: word (b0 >> 5) + j takes this word's low part and the high part of the word before
            uint32_t prev = __shfl_up(w, 1, 64);
            if (j0 == 0) prev = before;
            before = __shfl(w, lane | (group - 1), 64);
            if (valid) {
                const int64_t at = (b0 >> 5) + j;
                const uint32_t out = sh ? (w << sh) | (prev >> (32 - sh)) : w;
                if (m.bits && out) atomicOr(m.bits + at, out);
                if (m.bits && sh && j == a.wz - 1 && (w >> (32 - sh))) atomicOr(m.bits + at + 1, w >> (32 - sh));
                uint32_t rest = w;
                for (int left = __popc(w); left > 0 && (m.mask || IDS); --left) {
                    const int b = __ffs((int)rest) - 1;
                    rest &= rest - 1;
                    const int64_t v = b0 + 32 * j + b;
                    if (m.mask) m.mask[v] = 1;
                    if (IDS) {
                        uint32_t seen = __hip_atomic_load(m.ids + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        for (int tries = 0; tries < id_tries; ++tries) {
                            if (seen != 0 && seen <= oid) break;
                            const uint32_t was = atomicCAS(m.ids + v, seen, oid);
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

// behind mesh_launch_setup: the column tiles and their scan, the surface pass's scan and scatter, then one pair per mesh
hipError_t mesh_solid_launch(const SolidArgs& a, hipStream_t s) {
    hipError_t e = mesh_launch_setup(a.m, s);
    if (e != hipSuccess) return e;
    if (a.m.n_triangles == 0) return mesh_launch_scan(a.m, s);               // (nothing to fill; the status word is still served)
    const size_t box_bytes = ms_box_bytes(a.m.n_meshes);
    if ((e = hipMemsetAsync(a.box_lo, 0xFF, box_bytes, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.box_hi, 0, box_bytes, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ms_setup, dim3((unsigned)((a.m.n_triangles + kMrThreads - 1) / kMrThreads)), dim3(kMrThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    MeshArgs columns = a.m;
    columns.scan = a.scan;
    columns.top = a.top;
    if ((e = mesh_launch_scan(columns, s)) != hipSuccess) return e;
    if ((e = mesh_launch_scan(a.m, s)) != hipSuccess) return e;              // (second: the status block keeps the surface pass's total)
    if ((e = mesh_launch_scatter(a.m, s)) != hipSuccess) return e;
    SolidArgs one = a;
    for (int64_t mesh = 0; mesh < a.m.n_meshes; ++mesh) {
        one.mesh = mesh;
        hipLaunchKernelGGL(k_ms_scatter, dim3(kMsScatterGroups), dim3(kMrThreads), 0, s, one);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (a.m.ids) hipLaunchKernelGGL(k_ms_merge<true>, dim3(kMsMergeGroups), dim3(kMrThreads), 0, s, one);
        else hipLaunchKernelGGL(k_ms_merge<false>, dim3(kMsMergeGroups), dim3(kMrThreads), 0, s, one);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sdfgpu

// ---- the closedness check: host only ----------------------------------------------------------------------------------------------------
using namespace sdfgpu;

namespace {

struct MsEdge {
    uint64_t key[6];                   // the bit patterns of the two endpoints' world positions, the smaller endpoint first
    int64_t triangle;
    bool operator<(const MsEdge& o) const {
        const int c = std::memcmp(key, o.key, sizeof key);
        return c != 0 ? c < 0 : triangle < o.triangle;
    }
};

}  // namespace

extern "C" {

int sdfgpu_check_closed_meshes(const sdfgpu_mesh* meshes, int64_t n_meshes, const double* vertices, int64_t n_vertices, const uint32_t* triangles,
                               int64_t n_triangles, int64_t* out_bad_mesh, int64_t* out_bad_triangle) {
    if (out_bad_mesh) *out_bad_mesh = -1;
    if (out_bad_triangle) *out_bad_triangle = -1;
    if (n_meshes < 0 || n_vertices < 0 || n_triangles < 0 || (n_meshes > 0 && !meshes) || (n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles))
        return SDFGPU_ERR_INVALID_ARGUMENT;
    try {
        std::vector<MsEdge> edges;
        for (int64_t mi = 0; mi < n_meshes; ++mi) {
            const sdfgpu_mesh& mesh = meshes[mi];
            if (!mr_mesh_valid(mesh, n_vertices, n_triangles, false)) {
                if (out_bad_mesh) *out_bad_mesh = mi;
                return SDFGPU_ERR_INVALID_ARGUMENT;
            }
            edges.clear();
            edges.reserve((size_t)mesh.n_triangles * 3);
            for (int64_t j = 0; j < mesh.n_triangles; ++j) {
                double W[9];
                if (!mr_triangle_valid(mesh, vertices, triangles + 3 * (mesh.first_triangle + j), W)) {
                    if (out_bad_mesh) *out_bad_mesh = mi;
                    if (out_bad_triangle) *out_bad_triangle = j;
                    return SDFGPU_ERR_INVALID_ARGUMENT;
                }
                uint64_t key[3][3];
                for (int i = 0; i < 3; ++i)
                    for (int k = 0; k < 3; ++k) {
                        const double v = W[3 * i + k] == 0.0 ? 0.0 : W[3 * i + k];        // -0 and 0 are one position
                        std::memcpy(&key[i][k], &v, 8);
                    }
                for (int i = 0; i < 3; ++i) {
                    const uint64_t* p = key[i];
                    const uint64_t* q = key[(i + 1) % 3];
                    const int c = std::memcmp(p, q, 24);
                    if (c == 0) continue;                                    // an edge from a position to itself bounds nothing
                    MsEdge e;
                    std::memcpy(e.key, c < 0 ? p : q, 24);
                    std::memcpy(e.key + 3, c < 0 ? q : p, 24);
                    e.triangle = j;
                    edges.push_back(e);
                }
            }
            std::sort(edges.begin(), edges.end());
            int64_t bad = -1;
            for (size_t i = 0; i < edges.size();) {
                size_t k = i + 1;
                while (k < edges.size() && std::memcmp(edges[k].key, edges[i].key, sizeof edges[i].key) == 0) ++k;
                if (((k - i) & 1) && (bad < 0 || edges[i].triangle < bad)) bad = edges[i].triangle;      // (the run's lowest triangle)
                i = k;
            }
            if (bad >= 0) {
                if (out_bad_mesh) *out_bad_mesh = mi;
                if (out_bad_triangle) *out_bad_triangle = bad;
                return SDFGPU_ERR_INVALID_ARGUMENT;
            }
        }
    } catch (...) {
        return SDFGPU_ERR_INVALID_ARGUMENT;
    }
    return SDFGPU_OK;
}

}  // extern "C"
