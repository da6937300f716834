// sdfgpu_components.hip -- the connected-components kernels (sdfgpu_components.hpp) and their launcher.  Compiled beside
// sdfgpu.hip and linked into the same libsdfgpu.so (sdf_tools_amd/build.py).
// The family's host orchestration and C ABI entry points (sdfgpu_components*) are at the end of this file, over the handle of
// sdfgpu_context.hpp.
//
// The global union-find of k_cc_merge (its invariant, its memory scope) and the root ranking of k_cc_flatten / k_cc_scan /
// k_cc_relabel are stated once, in sdfgpu_unionfind.hpp.
#include "sdfgpu_context.hpp"
#include "sdfgpu_components.hpp"
#include "sdfgpu_unionfind.hpp"
#include "sdfgpu.h"

#include <algorithm>

namespace sdfgpu {

namespace {

constexpr int kLocalThreads = 1024;
constexpr int kMergeThreads = 256;
constexpr int kRelabelPerThread = 4;

__device__ __forceinline__ uint32_t bit_at(const uint32_t* __restrict__ bits, uint64_t g) {
    return (bits[g >> 5] >> (g & 31)) & 1u;
}

struct CcArgs {
    const uint32_t* bits;
    uint32_t* L;
    int64_t nx, ny, nz;
    int tx, ty, tz;
    int64_t nty, ntz;
    uint64_t nwords;                // ceil(n / 32)
};

__device__ __forceinline__ void tile_origin(const CcArgs& a, uint64_t b, int64_t& x0, int64_t& y0, int64_t& z0,
                                            bool& lo_x, bool& lo_y, bool& lo_z) {
    const int64_t tzi = (int64_t)(b % (uint64_t)a.ntz);
    const int64_t r = (int64_t)(b / (uint64_t)a.ntz);
    const int64_t tyi = r % a.nty, txi = r / a.nty;
    x0 = txi * a.tx; y0 = tyi * a.ty; z0 = tzi * a.tz;
    lo_x = txi > 0; lo_y = tyi > 0; lo_z = tzi > 0;
}

// ---- k_cc_local ---------------------------------------------------------------------------------------------------------------
// Local index i = (ix * ty + iy) * tz + iz is increasing in the same order as the global index of the voxel, so the tile-local
// minimum IS the global minimum of the tile's part of the component.
__global__ __launch_bounds__(kLocalThreads) void k_cc_local(const CcArgs a) {
    __shared__ uint32_t lab[kCcTileVoxels];
    __shared__ uint32_t cls[kCcTileVoxels / 32];
    int64_t x0, y0, z0;
    bool lx, ly, lz;
    tile_origin(a, blockIdx.x, x0, y0, z0, lx, ly, lz);
    const int tz = a.tz, ty = a.ty, wz = tz >> 5, rows = a.tx * ty, nv = rows * tz;

    // class words of the tile's rows: 32 voxels from an arbitrary bit offset (rows share words when nz % 32 != 0)
    for (int w = threadIdx.x; w < rows * wz; w += kLocalThreads) {
        const int row = w / wz, k = w - row * wz;
        const int64_t x = x0 + row / ty, y = y0 + row % ty, z = z0 + 32 * k;
        uint32_t word = 0;
        if (x < a.nx && y < a.ny && z < a.nz) {
            const uint64_t g = ((uint64_t)x * (uint64_t)a.ny + (uint64_t)y) * (uint64_t)a.nz + (uint64_t)z;
            const uint64_t q = g >> 5;
            const uint32_t s = (uint32_t)(g & 31);
            const uint32_t lo = a.bits[q];
            const uint32_t hi = (s && q + 1 < a.nwords) ? a.bits[q + 1] : 0u;
            word = s ? (lo >> s) | (hi << (32 - s)) : lo;
            const int64_t rem = a.nz - z;
            if (rem < 32) word &= (1u << rem) - 1u;
        }
        cls[w] = word;
    }
    __syncthreads();

    // z runs: every voxel starts under the first voxel of its run inside the tile row
    for (int i = threadIdx.x; i < nv; i += kLocalThreads) {
        const int row = i / tz, iz = i - row * tz;
        const int64_t x = x0 + row / ty, y = y0 + row % ty, z = z0 + iz;
        if (x >= a.nx || y >= a.ny || z >= a.nz) { lab[i] = (uint32_t)i; continue; }
        const uint32_t* cw = cls + row * wz;
        int k = iz >> 5;
        const uint32_t c = (cw[k] >> (iz & 31)) & 1u;
        uint32_t d = (c ? ~cw[k] : cw[k]) & ((1u << (iz & 31)) - 1u);   // voxels of the other class below iz in this word
        while (!d && k > 0) { --k; d = c ? ~cw[k] : cw[k]; }
        lab[i] = (uint32_t)(row * tz + (d ? 32 * k + (31 - __clz(d)) + 1 : 0));
    }
    __syncthreads();

    // y and x faces inside the tile.  A pair whose z predecessors are a same-class pair too is already joined through them.
    for (int i = threadIdx.x; i < nv; i += kLocalThreads) {
        const int row = i / tz, iz = i - row * tz, ix = row / ty, iy = row - ix * ty;
        if (x0 + ix >= a.nx || y0 + iy >= a.ny || z0 + iz >= a.nz) continue;
        const int k = iz >> 5, s = iz & 31;
        const uint32_t c = (cls[row * wz + k] >> s) & 1u;
        const bool zp = iz > 0 && ((cls[row * wz + ((iz - 1) >> 5)] >> ((iz - 1) & 31)) & 1u) == c;
        if (iy > 0) {
            const int r2 = row - 1;
            if (((cls[r2 * wz + k] >> s) & 1u) == c &&
                !(zp && ((cls[r2 * wz + ((iz - 1) >> 5)] >> ((iz - 1) & 31)) & 1u) == c))
                lds_union(lab, (uint32_t)i, (uint32_t)(i - tz));
        }
        if (ix > 0) {
            const int r2 = row - ty;
            if (((cls[r2 * wz + k] >> s) & 1u) == c &&
                !(zp && ((cls[r2 * wz + ((iz - 1) >> 5)] >> ((iz - 1) & 31)) & 1u) == c))
                lds_union(lab, (uint32_t)i, (uint32_t)(i - ty * tz));
        }
    }
    __syncthreads();

    for (int i = threadIdx.x; i < nv; i += kLocalThreads) {
        const int row = i / tz, iz = i - row * tz;
        const int64_t x = x0 + row / ty, y = y0 + row % ty, z = z0 + iz;
        if (x >= a.nx || y >= a.ny || z >= a.nz) continue;
        const uint32_t r = lds_find(lab, (uint32_t)i);
        const int rrow = (int)r / tz, riz = (int)r - rrow * tz;
        const uint64_t gr = ((uint64_t)(x0 + rrow / ty) * (uint64_t)a.ny + (uint64_t)(y0 + rrow % ty)) * (uint64_t)a.nz + (uint64_t)(z0 + riz);
        const uint64_t g = ((uint64_t)x * (uint64_t)a.ny + (uint64_t)y) * (uint64_t)a.nz + (uint64_t)z;
        a.L[g] = (uint32_t)gr;
    }
}

// ---- k_cc_merge ---------------------------------------------------------------------------------------------------------------
// One workgroup per tile joins each voxel of the tile's low x / y / z faces with its neighbour in the previous tile.
__global__ __launch_bounds__(kMergeThreads) void k_cc_merge(const CcArgs a) {
    int64_t x0, y0, z0;
    bool lx, ly, lz;
    tile_origin(a, blockIdx.x, x0, y0, z0, lx, ly, lz);
    const uint64_t ny = (uint64_t)a.ny, nz = (uint64_t)a.nz, plane = ny * nz;
    auto gidx = [&](int64_t x, int64_t y, int64_t z) { return ((uint64_t)x * ny + (uint64_t)y) * nz + (uint64_t)z; };
    if (lx) {                               // neighbour (x0 - 1, y, z); skip when (z - 1) pairs up the same way
        for (int idx = threadIdx.x; idx < a.ty * a.tz; idx += kMergeThreads) {
            const int iy = idx / a.tz, iz = idx - iy * a.tz;
            const int64_t y = y0 + iy, z = z0 + iz;
            if (x0 >= a.nx || y >= a.ny || z >= a.nz) continue;
            const uint64_t v = gidx(x0, y, z), u = v - plane;
            const uint32_t c = bit_at(a.bits, v);
            if (bit_at(a.bits, u) != c) continue;
            if (iz > 0 && bit_at(a.bits, v - 1) == c && bit_at(a.bits, u - 1) == c) continue;
            uf_union<RootIsSelf>(a.L, (uint32_t)v, (uint32_t)u);
        }
    }
    if (ly) {                               // neighbour (x, y0 - 1, z)
        for (int idx = threadIdx.x; idx < a.tx * a.tz; idx += kMergeThreads) {
            const int ix = idx / a.tz, iz = idx - ix * a.tz;
            const int64_t x = x0 + ix, z = z0 + iz;
            if (x >= a.nx || y0 >= a.ny || z >= a.nz) continue;
            const uint64_t v = gidx(x, y0, z), u = v - nz;
            const uint32_t c = bit_at(a.bits, v);
            if (bit_at(a.bits, u) != c) continue;
            if (iz > 0 && bit_at(a.bits, v - 1) == c && bit_at(a.bits, u - 1) == c) continue;
            uf_union<RootIsSelf>(a.L, (uint32_t)v, (uint32_t)u);
        }
    }
    if (lz) {                               // neighbour (x, y, z0 - 1); skip when (y - 1) pairs up the same way
        for (int idx = threadIdx.x; idx < a.tx * a.ty; idx += kMergeThreads) {
            const int ix = idx / a.ty, iy = idx - ix * a.ty;
            const int64_t x = x0 + ix, y = y0 + iy;
            if (x >= a.nx || y >= a.ny || z0 >= a.nz) continue;
            const uint64_t v = gidx(x, y, z0), u = v - 1;
            const uint32_t c = bit_at(a.bits, v);
            if (bit_at(a.bits, u) != c) continue;
            if (iy > 0 && bit_at(a.bits, v - nz) == c && bit_at(a.bits, u - nz) == c) continue;
            uf_union<RootIsSelf>(a.L, (uint32_t)v, (uint32_t)u);
        }
    }
}

// ---- k_cc_flatten / k_cc_scan / k_cc_relabel: the root ranking of sdfgpu_unionfind.hpp; every self-labelled voxel is a root --------
__global__ __launch_bounds__(256) void k_cc_flatten(uint32_t* __restrict__ L, uint64_t n, uint32_t* __restrict__ rb,
                                                    uint32_t* __restrict__ wr, uint32_t* __restrict__ cc) {
    rank_flatten(L, n, RankTables{rb, wr, cc, nullptr}, [](uint64_t) { return true; });
}

__global__ __launch_bounds__(kRankScanThreads) void k_cc_scan(const uint32_t* __restrict__ cc, uint32_t* __restrict__ co,
                                                              uint64_t chunks, uint32_t* __restrict__ count) {
    rank_scan(cc, co, chunks, count);
}

// Reads only the voxel's own label (its root r) and the rank tables, so rewriting labels in place races with nothing.
__global__ __launch_bounds__(256) void k_cc_relabel(uint32_t* __restrict__ L, uint64_t n, const uint32_t* __restrict__ rb,
                                                    const uint32_t* __restrict__ wr, const uint32_t* __restrict__ co) {
    const uint64_t base = (uint64_t)blockIdx.x * (256 * kRelabelPerThread) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kRelabelPerThread; ++j) {
        const uint64_t v = base + (uint64_t)j * 256;
        if (v >= n) return;
        L[v] = rank_of(L[v], rb, wr, co);
    }
}

// ---- component statistics (include/sdfgpu.h "Component statistics") ------------------------------------------
// The table is one sdfgpu_component_stats per label in 0 .. label_count: k_cs_init makes every entry the neutral element, k_cs_gather
// folds the voxels in with integer atomics (sums, minima and maxima: any order gives the same table), k_cs_count counts the labels
// that took a voxel and k_cs_compact lists them in label order.
constexpr int kStatsThreads = 256;
constexpr int kStatsCompactThreads = 1024;

__global__ __launch_bounds__(kStatsThreads) void k_cs_init(sdfgpu_component_stats* __restrict__ table, uint64_t entries) {
    const uint64_t i = (uint64_t)blockIdx.x * kStatsThreads + threadIdx.x;
    if (i >= entries) return;
    sdfgpu_component_stats s;
    s.label = (uint32_t)i; s.reserved = 0; s.count = 0;
    for (int a = 0; a < 3; ++a) { s.sum[a] = 0; s.lo[a] = INT32_MAX; s.hi[a] = INT32_MIN; }
    table[i] = s;
}

template <class T, class Op>
__device__ __forceinline__ T cs_wave_fold(T v, Op op) {
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}

// One thread per voxel.  The lanes of a wave that share a label fold their voxels first (neighbouring voxels mostly do: a wave is
// 64 voxels of a few z rows), and the first of them adds the sum to the label's entry: one round per distinct label in the wave.
__global__ __launch_bounds__(kStatsThreads) void k_cs_gather(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ labels, uint64_t n,
                                                             uint32_t ny, uint32_t nz, uint32_t label_count,
                                                             sdfgpu_component_stats* __restrict__ table) {
    const uint64_t v = (uint64_t)blockIdx.x * kStatsThreads + threadIdx.x;
    uint32_t label = 0;
    if (v < n && bit_at(bits, v)) label = labels[v];
    if (label > label_count) label = 0;                                        // (not a label of this call: no entry to add to)
    const uint64_t q = v / nz;
    const uint32_t z = (uint32_t)(v - q * nz), x = (uint32_t)(q / ny), y = (uint32_t)(q - (uint64_t)x * ny);
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(label != 0);
    while (todo) {                                                             // (uniform over the wave)
        const uint32_t current = (uint32_t)__shfl((int)label, __ffsll(todo) - 1);
        const bool same = label == current;
        const unsigned long long members = __ballot(same);
        const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
        const auto lower = [](int a, int b) { return a < b ? a : b; };
        const auto upper = [](int a, int b) { return a > b ? a : b; };
        const unsigned long long sx = cs_wave_fold<unsigned long long>(same ? x : 0, add), sy = cs_wave_fold<unsigned long long>(same ? y : 0, add),
                                 sz = cs_wave_fold<unsigned long long>(same ? z : 0, add);
        const int lx = cs_wave_fold<int>(same ? (int)x : INT32_MAX, lower), ly = cs_wave_fold<int>(same ? (int)y : INT32_MAX, lower),
                  lz = cs_wave_fold<int>(same ? (int)z : INT32_MAX, lower);
        const int hx = cs_wave_fold<int>(same ? (int)x : INT32_MIN, upper), hy = cs_wave_fold<int>(same ? (int)y : INT32_MIN, upper),
                  hz = cs_wave_fold<int>(same ? (int)z : INT32_MIN, upper);
        if (lane == __ffsll(members) - 1) {
            sdfgpu_component_stats* const s = table + current;
            atomicAdd(reinterpret_cast<unsigned long long*>(&s->count), (unsigned long long)__popcll(members));
            atomicAdd(reinterpret_cast<unsigned long long*>(&s->sum[0]), sx);
            atomicAdd(reinterpret_cast<unsigned long long*>(&s->sum[1]), sy);
            atomicAdd(reinterpret_cast<unsigned long long*>(&s->sum[2]), sz);
            atomicMin(&s->lo[0], lx); atomicMin(&s->lo[1], ly); atomicMin(&s->lo[2], lz);
            atomicMax(&s->hi[0], hx); atomicMax(&s->hi[1], hy); atomicMax(&s->hi[2], hz);
        }
        todo &= ~members;
    }
}

// *total = labels in 1 .. label_count with a voxel, one atomic per wave
__global__ __launch_bounds__(kStatsThreads) void k_cs_count(const sdfgpu_component_stats* __restrict__ table, uint32_t label_count,
                                                            unsigned long long* total) {
    const uint64_t label = (uint64_t)blockIdx.x * kStatsThreads + threadIdx.x + 1;
    const unsigned long long used = __ballot(label <= label_count && table[label].count > 0);
    if ((threadIdx.x & 63) == 0 && used) atomicAdd(total, (unsigned long long)__popcll(used));
}

// One workgroup walks the labels, kStatsCompactThreads at a time, and writes the entries that took a voxel in label order.
__global__ __launch_bounds__(kStatsCompactThreads) void k_cs_compact(const sdfgpu_component_stats* __restrict__ table, uint32_t label_count,
                                                                     sdfgpu_component_stats* __restrict__ out) {
    __shared__ uint32_t wave_sum[kStatsCompactThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t written = 0;
    for (uint64_t base = 1; base <= label_count; base += kStatsCompactThreads) {
        const uint64_t label = base + threadIdx.x;
        const bool used = label <= label_count && table[label].count > 0;
        const unsigned long long b = __ballot(used);
        __syncthreads();                                                       // (wave_sum may still be read from the round before)
        if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kStatsCompactThreads / 64; ++w) {
            if (w < wave) before += wave_sum[w];
            total += wave_sum[w];
        }
        if (used) out[written + before + (uint32_t)__popcll(b & ((1ull << lane) - 1))] = table[label];
        written += total;
    }
}

}  // namespace

CcPlan cc_plan(int64_t nx, int64_t ny, int64_t nz) {
    CcPlan p;
    // singleton axes to the front (index = x * ny * nz + y * nz + z is unchanged, and a singleton axis has no neighbours)
    if (nz == 1) { nz = ny; ny = nx; nx = 1; }
    if (nz == 1) { nz = ny; ny = nx; nx = 1; }
    if (ny == 1) { ny = nx; nx = 1; }
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.tz = nz <= 32 ? 32 : 64;
    p.ty = (int)std::min<int64_t>(ny, 16);
    p.tx = (int)std::min<int64_t>(nx, kCcTileVoxels / (p.tz * p.ty));
    if (p.tx == nx) {                       // thin grids: spend the rest of the tile on z
        const int cap = (kCcTileVoxels / (p.tx * p.ty)) & ~31;
        const int64_t nz32 = (nz + 31) & ~(int64_t)31;
        p.tz = (int)std::min<int64_t>(nz32, std::max(p.tz, cap));
    }
    p.ntx = (nx + p.tx - 1) / p.tx;
    p.nty = (ny + p.ty - 1) / p.ty;
    p.ntz = (nz + p.tz - 1) / p.tz;
    p.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    p.chunks = rank_chunks(p.n);
    p.scratch_bytes = rank_tables_bytes(p.chunks) + 4 * 4;     // K and three spare words
    return p;
}

uint32_t* cc_count_word(const CcPlan& p, void* d_scratch) {
    return reinterpret_cast<uint32_t*>(static_cast<char*>(d_scratch) + rank_tables_bytes(p.chunks));
}

hipError_t cc_launch(const CcPlan& p, const uint32_t* d_bits, uint32_t* d_labels, void* d_scratch, hipStream_t s) {
    CcArgs a;
    a.bits = d_bits;
    a.L = d_labels;
    a.nx = p.nx; a.ny = p.ny; a.nz = p.nz;
    a.tx = p.tx; a.ty = p.ty; a.tz = p.tz;
    a.nty = p.nty; a.ntz = p.ntz;
    a.nwords = (p.n + 31) / 32;
    const uint64_t tiles = (uint64_t)p.ntx * (uint64_t)p.nty * (uint64_t)p.ntz;
    const RankTables t = rank_tables_at(d_scratch, p.chunks);
    hipLaunchKernelGGL(k_cc_local, dim3((unsigned)tiles), dim3(kLocalThreads), 0, s, a);
    if (tiles > 1) hipLaunchKernelGGL(k_cc_merge, dim3((unsigned)tiles), dim3(kMergeThreads), 0, s, a);
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)p.chunks), dim3(256), 0, s, d_labels, p.n, t.rb, t.wr, t.cc);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(kRankScanThreads), 0, s, (const uint32_t*)t.cc, t.co, p.chunks, cc_count_word(p, d_scratch));
    const uint64_t rblocks = (p.n + 256 * kRelabelPerThread - 1) / (256 * kRelabelPerThread);
    hipLaunchKernelGGL(k_cc_relabel, dim3((unsigned)rblocks), dim3(256), 0, s, d_labels, p.n, (const uint32_t*)t.rb,
                       (const uint32_t*)t.wr, (const uint32_t*)t.co);
    return hipGetLastError();
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

// ---- connected components (sdfgpu_components.hpp) ------------------------------------------------------------------------------
// Uses only cc_scratch (and, in the host forms, the bit / output staging and the pinned chunks, which every host-buffer call
// owns while it runs): the SDF builds' scratch, status block and policy are not touched.

// bits (device) -> labels (device), K -> *out_count; synchronises `st` (K is read back)
int components_impl(sdfgpu_handle h, const uint32_t* d_bits, int64_t nx, int64_t ny, int64_t nz, uint32_t* d_labels, uint32_t* out_count,
                    hipStream_t st) {
    const CcPlan plan = cc_plan(nx, ny, nz);
    if (int rc = ensure(h, h->cc_scratch, plan.scratch_bytes, "components scratch")) return rc;
    HIP_TRY(h, cc_launch(plan, d_bits, d_labels, h->cc_scratch.ptr, st));
    uint32_t k = 0;
    HIP_TRY(h, hipMemcpyAsync(&k, cc_count_word(plan, h->cc_scratch.ptr), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (out_count) *out_count = k;
    return SDFGPU_OK;
}

// host mask / cell records -> bits (host team, 1 bit per voxel over PCIe) -> labels in the output staging
int components_host(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, uint32_t* out_count) {
    const int64_t n = nx * ny * nz;
    if (int rc = upload_packed(h, occ, n, kNullStream)) return rc;
    if (int rc = ensure(h, h->stage_out, (size_t)n * 4, "output staging")) return rc;
    return components_impl(h, (const uint32_t*)h->stage_bits.ptr, nx, ny, nz, (uint32_t*)h->stage_out.ptr, out_count, nullptr);
}

// bits + labels (device) -> the records of the labels with a set voxel, in label order; synchronises `st` (the total is read back)
int component_stats_impl(sdfgpu_handle h, const uint32_t* d_bits, const uint32_t* d_labels, int64_t nx, int64_t ny, int64_t nz, uint32_t label_count,
                         sdfgpu_component_stats* d_stats, int64_t capacity, int64_t* out_total, hipStream_t st) {
    *out_total = 0;
    if (label_count == 0) return SDFGPU_OK;
    const uint64_t n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz, entries = (uint64_t)label_count + 1;
    constexpr size_t kCounterBytes = 256;                                      // the total, in front of the table
    HIP_TRY(h, h->cs_order.create());
    HIP_TRY(h, h->cs_order.wait(st));
    if (int rc = ensure(h, h->cs_scratch, kCounterBytes + (size_t)entries * sizeof(sdfgpu_component_stats), "component statistics scratch")) return rc;
    StreamOrder::RecordAtExit record{h->cs_order, st};
    unsigned long long* const d_total = static_cast<unsigned long long*>(h->cs_scratch.ptr);
    sdfgpu_component_stats* const table = reinterpret_cast<sdfgpu_component_stats*>(static_cast<char*>(h->cs_scratch.ptr) + kCounterBytes);
    const auto blocks = [](uint64_t items) { return dim3((unsigned)((items + kStatsThreads - 1) / kStatsThreads)); };
    HIP_TRY(h, hipMemsetAsync(d_total, 0, kCounterBytes, st));
    hipLaunchKernelGGL(k_cs_init, blocks(entries), dim3(kStatsThreads), 0, st, table, entries);
    hipLaunchKernelGGL(k_cs_gather, blocks(n), dim3(kStatsThreads), 0, st, d_bits, d_labels, n, (uint32_t)ny, (uint32_t)nz, label_count, table);
    hipLaunchKernelGGL(k_cs_count, blocks(label_count), dim3(kStatsThreads), 0, st, (const sdfgpu_component_stats*)table, label_count, d_total);
    HIP_TRY(h, hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    *out_total = (int64_t)total;
    if (total == 0 || (uint64_t)capacity < total) return SDFGPU_OK;
    hipLaunchKernelGGL(k_cs_compact, dim3(1), dim3(kStatsCompactThreads), 0, st, (const sdfgpu_component_stats*)table, label_count, d_stats);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

}  // namespace

extern "C" {

int sdfgpu_component_stats_device(sdfgpu_handle h, const uint32_t* d_bits, const uint32_t* d_labels, int64_t nx, int64_t ny, int64_t nz,
                                  uint32_t label_count, sdfgpu_component_stats* d_stats, int64_t capacity, int64_t* out_total, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_bits || !d_labels || !out_total) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if ((reinterpret_cast<uintptr_t>(d_bits) | reinterpret_cast<uintptr_t>(d_labels)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_bits and d_labels must be 4-byte aligned");
        if (reinterpret_cast<uintptr_t>(d_stats) & 7) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_stats must be 8-byte aligned");
        if (capacity < 0 || (capacity > 0 && !d_stats)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "component statistics: a capacity without a buffer");
        if (int rc = check_dims_u32(h, nx, ny, nz, kLabelsTail)) return rc;
        if (std::max({nx, ny, nz}) > (int64_t)INT32_MAX)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "component statistics: an axis above 2^31 - 1 voxels (the bounding box is int32)");
        HIP_TRY(h, hipSetDevice(h->device));
        return component_stats_impl(h, d_bits, d_labels, nx, ny, nz, label_count, d_stats, capacity, out_total, (hipStream_t)stream);
    });
}

int sdfgpu_components_bits_device(sdfgpu_handle h, const uint32_t* d_bits, int64_t nx, int64_t ny, int64_t nz, uint32_t* d_labels,
                                  uint32_t* out_count, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_bits || !d_labels || !out_count) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if ((reinterpret_cast<uintptr_t>(d_bits) | reinterpret_cast<uintptr_t>(d_labels)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_bits and d_labels must be 4-byte aligned");
        if (int rc = check_dims_u32(h, nx, ny, nz, kLabelsTail)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return components_impl(h, d_bits, nx, ny, nz, d_labels, out_count, (hipStream_t)stream);
    });
}

int sdfgpu_components(sdfgpu_handle h, const uint8_t* filled, int64_t nx, int64_t ny, int64_t nz, uint32_t* out_labels, uint32_t* out_count) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!filled || !out_labels || !out_count) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_dims_u32(h, nx, ny, nz, kLabelsTail)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = components_host(h, Occupancy::of_mask(filled), nx, ny, nz, out_count)) return rc;
        return copy_to_host(h, out_labels, h->stage_out.ptr, (size_t)(nx * ny * nz) * 4);
    });
}

int sdfgpu_components_cells(sdfgpu_handle h, void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                            int64_t nx, int64_t ny, int64_t nz, uint32_t* out_count) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!cells || !out_count) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_component_layout(h, cell_stride, occupancy_offset, component_offset)) return rc;
        if (int rc = check_dims_u32(h, nx, ny, nz, kLabelsTail)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = components_host(h, Occupancy::of_cells(cells, cell_stride, occupancy_offset, 0), nx, ny, nz, out_count)) return rc;
        char* const rec = static_cast<char*>(cells) + component_offset;
        // the drain team writes each label into its record (download offsets are multiples of 4: whole labels)
        return staged_download_hip(h, h->stage_out.ptr, (size_t)(nx * ny * nz) * 4, nullptr, [=](const char* src, size_t goff, size_t len) {
            char* dst = rec + (goff / 4) * cell_stride;
            for (size_t o = 0; o < len; o += 4, dst += cell_stride) memcpy(dst, src + o, 4);
        });
    });
}

}  // extern "C"
