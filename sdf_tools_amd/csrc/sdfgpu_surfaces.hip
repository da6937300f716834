// sdfgpu_surfaces.hip -- the component-surface kernels (sdfgpu_surfaces.hpp) and their launchers.  Compiled beside sdfgpu.hip and
// linked into the same libsdfgpu.so (sdf_tools_amd/build.py).
// The family's host orchestration and C ABI entry points (sdfgpu_component_surfaces*) are at the end of this file, over the handle of
// sdfgpu_context.hpp.
//
// Launch sizes: every workgroup owns kSfTile voxels or elements, so the largest grid (2^32 - 1 voxels) is 2^20 workgroups of 256
// threads -- far below the 2^32 threads a single launch may have; the scan's table has at most 2^8 x 2^20 entries.
#include "sdfgpu_context.hpp"
#include "sdfgpu_surfaces.hpp"
#include "sdfgpu.h"

#include <algorithm>

namespace sdfgpu {

namespace {

constexpr int kFlagThreads = 256;
constexpr int kTableSlots = 1024;              // k_sf_flag's LDS table of per-label counts (open addressing)
constexpr int kTableProbes = 16;               // (a label that finds no slot goes straight to the global counters)
constexpr int kScanThreads = 256;              // k_sf_scan_reduce / k_sf_scan_apply: 8 entries per thread
constexpr int kTopThreads = 1024;
constexpr uint32_t kFree = 0xFFFFFFFFu;        // free table slot (a counted label is <= max_label < 2^32 - 1)

struct SfArgs {
    const uint32_t* L;                         // labels
    const uint32_t* S;                         // selection bits or nullptr
    uint32_t* bits;                            // surface bit words, tiles * kSfTile / 32
    uint32_t* ubits;                           // the caller's copy (ceil(n / 32) words) or nullptr
    uint64_t uwords;
    uint32_t nx, ny, nz;                       // (each axis is below 2^32: the voxel count is)
    uint64_t n;
    uint32_t max_label;
    uint32_t* cnt;                             // max_label + 1
    SfStatus* st;
};

// ---- k_sf_flag ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFlagThreads) void k_sf_flag(const SfArgs a) {
    __shared__ uint32_t tkey[kTableSlots];                  // label, or kFree
    __shared__ uint32_t tval[kTableSlots];                  // reported voxels of this workgroup (<= kSfTile)
    __shared__ uint32_t btotal;
    const int lane = threadIdx.x & 63;
    for (int t = threadIdx.x; t < kTableSlots; t += kFlagThreads) { tkey[t] = kFree; tval[t] = 0u; }
    if (threadIdx.x == 0) btotal = 0u;
    __syncthreads();
    const uint64_t sy = a.nz, sx = (uint64_t)a.ny * (uint64_t)a.nz;
    uint32_t wtotal = 0;                                    // reported voxels of this wave (same in every lane)
    for (int r = 0; r < kSfTile / kFlagThreads; ++r) {
        const uint64_t v = (uint64_t)blockIdx.x * kSfTile + (uint64_t)r * kFlagThreads + threadIdx.x;
        bool rep = false;
        uint32_t c = 0;
        if (v < a.n) {
            c = a.L[v];
            if (c > a.max_label) {                          // (max_label < 2^32 - 1)
                atomicOr(&a.st->err, kSfErrLabel);
                atomicMax(&a.st->label_over, c);
            } else if (!a.S || ((a.S[v >> 5] >> (v & 31)) & 1u)) {
                const uint32_t v32 = (uint32_t)v, t = v32 / a.nz, z = v32 - t * a.nz, x = t / a.ny, y = t - x * a.ny;   // (v < n < 2^32)
                if (x == 0 || y == 0 || z == 0 || x == a.nx - 1 || y == a.ny - 1 || z == a.nz - 1) {
                    rep = true;                             // an out-of-grid neighbour: component -1
                } else {
                    const uint32_t l0 = a.L[v - 1], l1 = a.L[v + 1], l2 = a.L[v - sy], l3 = a.L[v + sy], l4 = a.L[v - sx], l5 = a.L[v + sx];
                    rep = (l0 != c) | (l1 != c) | (l2 != c) | (l3 != c) | (l4 != c) | (l5 != c);
                }
            }
        }
        const uint64_t bal = __ballot(rep);
        if (lane == 0) {                                    // (v is a multiple of 64 here: two whole words; bits past n are 0)
            const uint64_t w = v >> 5;
            a.bits[w] = (uint32_t)bal;
            a.bits[w + 1] = (uint32_t)(bal >> 32);
            if (a.ubits) {
                if (w < a.uwords) a.ubits[w] = (uint32_t)bal;
                if (w + 1 < a.uwords) a.ubits[w + 1] = (uint32_t)(bal >> 32);
            }
        }
        wtotal += (uint32_t)__popcll(bal);
        // per-label counts: reported lanes that share a label add once per wave
        uint64_t act = bal;
        while (act) {
            const int leader = __ffsll((long long)act) - 1;
            const uint32_t cl = __shfl(c, leader);
            const uint64_t mm = __ballot(rep && c == cl);
            if (lane == leader) {
                const uint32_t add = (uint32_t)__popcll(mm);
                bool placed = false;
                for (int p = 0, h = (int)((cl * 2654435761u) >> 22); p < kTableProbes && !placed; ++p, h = (h + 1) & (kTableSlots - 1)) {
                    const uint32_t old = atomicCAS(&tkey[h], kFree, cl);
                    if (old == kFree || old == cl) { atomicAdd(&tval[h], add); placed = true; }
                }
                if (!placed) atomicAdd(a.cnt + cl, add);
            }
            act &= ~mm;
        }
    }
    if (lane == 0 && wtotal) atomicAdd(&btotal, wtotal);
    __syncthreads();
    if (threadIdx.x == 0 && btotal) atomicAdd(reinterpret_cast<unsigned long long*>(&a.st->total), (unsigned long long)btotal);
    for (int t = threadIdx.x; t < kTableSlots; t += kFlagThreads)
        if (tkey[t] != kFree && tval[t]) atomicAdd(a.cnt + tkey[t], tval[t]);
}

// ---- the sort -------------------------------------------------------------------------------------------------------------------
struct SortArgs {
    const uint32_t* L;                         // first pass: labels and surface bit words
    const uint64_t* bits;
    const uint2* src;                          // later passes: (label, index) pairs
    uint64_t total;
    uint64_t tiles;                            // of this pass
    int shift, nb;                             // digit = (label >> shift) & (2^nb - 1)
    uint32_t* table;                           // [2^nb][tiles]
    uint32_t* sums;                            // the scan's segment sums
    uint2* dst_pairs;                          // or, on the last pass,
    uint32_t* dst_idx;
    uint32_t* dst_key;                         // ... and the labels beside them, or nullptr (sf_launch_sort_pairs)
};

// element (tile, round r, lane) of the pass's input, in order; `any` is wave-uniform: some lane of the round has an element
template <bool FIRST>
__device__ __forceinline__ bool load_elem(const SortArgs& a, uint64_t tile, int r, int lane, uint32_t& lab, uint32_t& idx, bool& any) {
    const uint64_t base = tile * kSfTile + (uint64_t)r * 64;
    if (FIRST) {
        const uint64_t w = a.bits[base >> 6];               // (base is a multiple of 64)
        any = w != 0;
        const bool has = (w >> lane) & 1ull;
        if (has) { lab = a.L[base + lane]; idx = (uint32_t)(base + lane); }
        return has;
    }
    any = base < a.total;
    const bool has = base + lane < a.total;
    if (has) { const uint2 p = a.src[base + lane]; lab = p.x; idx = p.y; }
    return has;
}

// the lanes of the wave that hold an element with this lane's digit (meaningful where `has`)
__device__ __forceinline__ uint64_t match_digit(bool has, uint32_t d, int nb) {
    uint64_t m = __ballot(has);
    for (int b = 0; b < nb; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(has && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

template <bool FIRST>
__global__ __launch_bounds__(64) void k_sf_hist(const SortArgs a) {
    __shared__ uint32_t hist[1 << kSfDigitBits];
    const int lane = threadIdx.x, nd = 1 << a.nb;
    const uint64_t tile = blockIdx.x;
    for (int d = lane; d < nd; d += 64) hist[d] = 0u;
    __syncthreads();
    for (int r = 0; r < kSfTile / 64; ++r) {
        uint32_t lab = 0, idx = 0;
        bool any;
        const bool has = load_elem<FIRST>(a, tile, r, lane, lab, idx, any);
        if (!any) continue;
        const uint32_t d = (lab >> a.shift) & (uint32_t)(nd - 1);
        const uint64_t m = match_digit(has, d, a.nb);
        if (has && lane == __ffsll((long long)m) - 1) atomicAdd(&hist[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    for (int d = lane; d < nd; d += 64) a.table[(uint64_t)d * a.tiles + tile] = hist[d];
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(64) void k_sf_scatter(const SortArgs a) {
    __shared__ uint32_t run[1 << kSfDigitBits];             // per digit: where this tile's next element of the digit goes
    const int lane = threadIdx.x, nd = 1 << a.nb;
    const uint64_t tile = blockIdx.x;
    const uint64_t lt = (1ull << lane) - 1ull;
    for (int d = lane; d < nd; d += 64) run[d] = a.table[(uint64_t)d * a.tiles + tile];
    __syncthreads();
    for (int r = 0; r < kSfTile / 64; ++r) {
        uint32_t lab = 0, idx = 0;
        bool any;
        const bool has = load_elem<FIRST>(a, tile, r, lane, lab, idx, any);
        if (!any) continue;                                 // (uniform: the workgroup is one wave)
        const uint32_t d = (lab >> a.shift) & (uint32_t)(nd - 1);
        const uint64_t m = match_digit(has, d, a.nb);
        const int leader = has ? __ffsll((long long)m) - 1 : lane;
        uint32_t base = 0;
        if (has && lane == leader) {                        // (one leader per digit: no two lanes touch the same word)
            base = run[d];
            run[d] = base + (uint32_t)__popcll(m);
        }
        base = __shfl(base, leader);
        if (has) {
            const uint32_t pos = base + (uint32_t)__popcll(m & lt);       // (< total <= the destination's capacity)
            if (LAST) {
                a.dst_idx[pos] = idx;
                if (a.dst_key) a.dst_key[pos] = lab;
            } else {
                a.dst_pairs[pos] = make_uint2(lab, idx);
            }
        }
        __syncthreads();                                    // (run is read by other lanes in the next round)
    }
}

// ---- exclusive scan of the histogram table (uint32: every partial sum is <= total < 2^32) ----------------------------------------
__global__ __launch_bounds__(kScanThreads) void k_sf_scan_reduce(const uint32_t* __restrict__ t, uint64_t entries, uint32_t* __restrict__ sums) {
    __shared__ uint32_t acc;
    if (threadIdx.x == 0) acc = 0u;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * kSfScanSeg + (uint64_t)threadIdx.x * 8;
    uint32_t s = 0;
    for (int i = 0; i < 8; ++i) s += lo + i < entries ? t[lo + i] : 0u;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&acc, s);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kTopThreads) void k_sf_scan_top(uint32_t* __restrict__ sums, uint64_t segs) {
    __shared__ uint32_t s[kTopThreads];
    const int t = threadIdx.x;
    const uint64_t per = (segs + kTopThreads - 1) / kTopThreads;
    const uint64_t lo = std::min<uint64_t>(segs, per * t), hi = std::min<uint64_t>(segs, lo + per);
    uint32_t sum = 0;
    for (uint64_t i = lo; i < hi; ++i) sum += sums[i];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kTopThreads; d <<= 1) {
        const uint32_t add = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    uint32_t run = s[t] - sum;
    for (uint64_t i = lo; i < hi; ++i) { const uint32_t c = sums[i]; sums[i] = run; run += c; }
}

__global__ __launch_bounds__(kScanThreads) void k_sf_scan_apply(uint32_t* __restrict__ t, uint64_t entries, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * kSfScanSeg + (uint64_t)threadIdx.x * 8;
    uint32_t e[8], s = 0;
    for (int i = 0; i < 8; ++i) { e[i] = lo + i < entries ? t[lo + i] : 0u; s += e[i]; }
    uint32_t inc = s;                                       // inclusive scan of the thread sums over the wave
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t run = sums[blockIdx.x] + inc - s;
    for (int w = 0; w < kScanThreads / 64; ++w) run += w < wave ? wsum[w] : 0u;
    for (int i = 0; i < 8; ++i) {
        if (lo + i < entries) t[lo + i] = run;
        run += e[i];
    }
}

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

}  // namespace

SfPlan sf_plan(int64_t nx, int64_t ny, int64_t nz, uint32_t max_label) {
    SfPlan p;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    p.tiles = (p.n + kSfTile - 1) / kSfTile;
    p.max_label = max_label;
    p.label_bits = 0;
    while (p.label_bits < 32 && ((uint64_t)max_label >> p.label_bits) != 0) ++p.label_bits;
    p.passes = std::max(1, (p.label_bits + kSfDigitBits - 1) / kSfDigitBits);
    p.off_status = align8(((size_t)max_label + 1) * 4);
    p.zero_bytes = p.off_status + sizeof(SfStatus);
    p.off_bits = align8(p.zero_bytes);
    p.scratch_bytes = p.off_bits + (size_t)p.tiles * (kSfTile / 8);
    return p;
}

SfSortPlan sf_sort_plan(const SfPlan& p, uint64_t total) {
    SfSortPlan sp;
    sp.total = total;
    const int nb0 = std::min(p.label_bits, kSfDigitBits);
    sp.table_entries = p.tiles << nb0;
    if (p.passes > 1) sp.table_entries = std::max<uint64_t>(sp.table_entries, ((total + kSfTile - 1) / kSfTile) << kSfDigitBits);
    const size_t pair_bytes = p.passes > 1 ? (size_t)total * 8 : 0;
    sp.off_b = pair_bytes;
    sp.off_table = 2 * pair_bytes;
    sp.off_sums = sp.off_table + align8((size_t)sp.table_entries * 4);
    sp.bytes = sp.off_sums + (size_t)((sp.table_entries + kSfScanSeg - 1) / kSfScanSeg) * 4;
    return sp;
}

hipError_t sf_launch_flag(const SfPlan& p, const uint32_t* d_labels, const uint32_t* d_select, uint32_t* d_user_bits, void* d_scratch,
                          hipStream_t s) {
    char* b = static_cast<char*>(d_scratch);
    SfArgs a;
    a.L = d_labels;
    a.S = d_select;
    a.bits = reinterpret_cast<uint32_t*>(b + p.off_bits);
    a.ubits = d_user_bits;
    a.uwords = (p.n + 31) / 32;
    a.nx = (uint32_t)p.nx; a.ny = (uint32_t)p.ny; a.nz = (uint32_t)p.nz;
    a.n = p.n;
    a.max_label = p.max_label;
    a.cnt = reinterpret_cast<uint32_t*>(b);
    a.st = reinterpret_cast<SfStatus*>(b + p.off_status);
    hipError_t e = hipMemsetAsync(d_scratch, 0, p.zero_bytes, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sf_flag, dim3((unsigned)p.tiles), dim3(kFlagThreads), 0, s, a);
    return hipGetLastError();
}

void sf_launch_scan(uint32_t* d_table, uint64_t entries, uint32_t* d_sums, hipStream_t s) {
    if (entries == 0) return;
    const uint64_t segs = (entries + kSfScanSeg - 1) / kSfScanSeg;
    hipLaunchKernelGGL(k_sf_scan_reduce, dim3((unsigned)segs), dim3(kScanThreads), 0, s, (const uint32_t*)d_table, entries, d_sums);
    hipLaunchKernelGGL(k_sf_scan_top, dim3(1), dim3(kTopThreads), 0, s, d_sums, segs);
    hipLaunchKernelGGL(k_sf_scan_apply, dim3((unsigned)segs), dim3(kScanThreads), 0, s, d_table, entries, (const uint32_t*)d_sums);
}

namespace {

// one pass of the sort: histogram, scan of the table, scatter
hipError_t launch_pass(const SortArgs& a, bool first, bool last, hipStream_t s) {
    const dim3 grid((unsigned)a.tiles), block(64);
    if (first) hipLaunchKernelGGL(k_sf_hist<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_sf_hist<false>, grid, block, 0, s, a);
    sf_launch_scan(a.table, a.tiles << a.nb, a.sums, s);
    if (first && last) hipLaunchKernelGGL((k_sf_scatter<true, true>), grid, block, 0, s, a);
    else if (first) hipLaunchKernelGGL((k_sf_scatter<true, false>), grid, block, 0, s, a);
    else if (last) hipLaunchKernelGGL((k_sf_scatter<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_sf_scatter<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t sf_launch_sort(const SfPlan& p, const SfSortPlan& sp, const uint32_t* d_labels, const void* d_scratch, void* d_sort,
                          uint32_t* d_indices, hipStream_t s) {
    if (sp.total == 0) return hipSuccess;
    char* q = static_cast<char*>(d_sort);
    uint2* const pairs[2] = {reinterpret_cast<uint2*>(q), reinterpret_cast<uint2*>(q + sp.off_b)};
    for (int k = 0; k < p.passes; ++k) {
        const bool first = k == 0, last = k == p.passes - 1;
        SortArgs a;
        a.L = d_labels;
        a.bits = reinterpret_cast<const uint64_t*>(static_cast<const char*>(d_scratch) + p.off_bits);
        a.src = first ? nullptr : pairs[(k - 1) & 1];
        a.total = sp.total;
        a.tiles = first ? p.tiles : (sp.total + kSfTile - 1) / kSfTile;
        a.shift = k * kSfDigitBits;
        a.nb = std::max(0, std::min(kSfDigitBits, p.label_bits - a.shift));
        a.table = reinterpret_cast<uint32_t*>(q + sp.off_table);
        a.sums = reinterpret_cast<uint32_t*>(q + sp.off_sums);
        a.dst_pairs = last ? nullptr : pairs[k & 1];
        a.dst_idx = last ? d_indices : nullptr;
        a.dst_key = nullptr;
        const hipError_t e = launch_pass(a, first, last, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

SfPairSortPlan sf_pair_sort_plan(uint64_t total, int key_bits) {
    SfPairSortPlan sp;
    sp.total = total;
    sp.passes = (key_bits + kSfDigitBits - 1) / kSfDigitBits;
    const uint64_t entries = ((total + kSfTile - 1) / kSfTile) << std::min(key_bits, kSfDigitBits);
    sp.off_b = (size_t)total * 8;
    sp.off_table = 2 * sp.off_b;
    sp.off_sums = sp.off_table + align8((size_t)entries * 4);
    sp.bytes = sp.off_sums + align8((size_t)((entries + kSfScanSeg - 1) / kSfScanSeg) * 4);
    return sp;
}

hipError_t sf_launch_sort_pairs(const SfPairSortPlan& sp, int key_bits, void* d_sort, uint32_t* d_indices, uint32_t* d_keys, hipStream_t s) {
    if (sp.total == 0) return hipSuccess;
    char* q = static_cast<char*>(d_sort);
    uint2* const pairs[2] = {reinterpret_cast<uint2*>(q), reinterpret_cast<uint2*>(q + sp.off_b)};
    for (int k = 0; k < sp.passes; ++k) {
        const bool last = k == sp.passes - 1;
        SortArgs a;
        a.L = nullptr;
        a.bits = nullptr;
        a.src = pairs[k & 1];
        a.total = sp.total;
        a.tiles = (sp.total + kSfTile - 1) / kSfTile;
        a.shift = k * kSfDigitBits;
        a.nb = std::min(kSfDigitBits, key_bits - a.shift);
        a.table = reinterpret_cast<uint32_t*>(q + sp.off_table);
        a.sums = reinterpret_cast<uint32_t*>(q + sp.off_sums);
        a.dst_pairs = last ? nullptr : pairs[(k + 1) & 1];
        a.dst_idx = last ? d_indices : nullptr;
        a.dst_key = last ? d_keys : nullptr;
        const hipError_t e = launch_pass(a, false, last, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

// ---- component surfaces (sdfgpu_surfaces.hpp) -----------------------------------------------------------------------------------
// Like the topology: only sf_scratch, sf_sort and sf_indices (and, in the host forms, the label / bit staging and the pinned
// chunks) are used; the SDF builds' scratch, status block and policy are not touched.
int check_surfaces_args(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, const int64_t* out_counts, bool want_indices,
                        int64_t capacity, const int64_t* out_total) {
    if (!out_counts || !out_total) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = check_dims_u32(h, nx, ny, nz, kLabelsTail)) return rc;
    if (max_label == 0xFFFFFFFFu) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "max_label must be below 2^32 - 1");
    if (want_indices && capacity < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "capacity must not be negative (got %lld)", (long long)capacity);
    return SDFGPU_OK;
}

// labels (device) + selection bits (device or null) -> counts (host) and, when asked, the grouped indices: into d_indices
// (device) or, through sf_indices, into host_indices.  Synchronises `st`.
int surfaces_impl(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label,
                  int64_t* out_counts, uint32_t* d_indices, uint32_t* host_indices, int64_t capacity, int64_t* out_total,
                  uint32_t* d_surface_bits, hipStream_t st) {
    const SfPlan plan = sf_plan(nx, ny, nz, max_label);
    if (int rc = ensure(h, h->sf_scratch, plan.scratch_bytes, "surfaces scratch")) return rc;
    HIP_TRY(h, sf_launch_flag(plan, d_labels, d_select, d_surface_bits, h->sf_scratch.ptr, st));
    SfStatus status;
    HIP_TRY(h, hipMemcpyAsync(&status, static_cast<char*>(h->sf_scratch.ptr) + plan.off_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (status.err & kSfErrLabel)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "label %u exceeds max_label %u", status.label_over, max_label);
    *out_total = (int64_t)status.total;
    {                                                           // (uint32 counters, widened: every count is below 2^32)
        std::vector<uint32_t> c32((size_t)max_label + 1);
        if (int rc = copy_to_host(h, c32.data(), h->sf_scratch.ptr, c32.size() * 4, st)) return rc;
        for (size_t c = 0; c < c32.size(); ++c) out_counts[c] = (int64_t)c32[c];
    }
    if (!d_indices && !host_indices) return SDFGPU_OK;          // counts only
    if ((uint64_t)capacity < status.total)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "the index buffer holds %lld indices, the surfaces have %llu (counts and total are valid)",
                    (long long)capacity, (unsigned long long)status.total);
    if (status.total == 0) return SDFGPU_OK;
    if (host_indices) {
        if (int rc = ensure(h, h->sf_indices, (size_t)status.total * 4, "surfaces indices")) return rc;
        d_indices = (uint32_t*)h->sf_indices.ptr;
    }
    const SfSortPlan sp = sf_sort_plan(plan, status.total);
    if (int rc = ensure(h, h->sf_sort, sp.bytes, "surfaces sort scratch")) return rc;
    HIP_TRY(h, sf_launch_sort(plan, sp, d_labels, h->sf_scratch.ptr, h->sf_sort.ptr, d_indices, st));
    if (host_indices) return copy_to_host(h, host_indices, d_indices, (size_t)status.total * 4, st);
    HIP_TRY(h, hipStreamSynchronize(st));
    return SDFGPU_OK;
}

int surfaces_host(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select, const void* cells, size_t stride, size_t occ_off,
                  size_t comp_off, int class_mask, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, int64_t* out_counts,
                  uint32_t* out_indices, int64_t capacity, int64_t* out_total) {
    bool selected = false;
    if (int rc = stage_labels_selection(h, labels, select, cells, stride, occ_off, comp_off, class_mask, nx * ny * nz, &selected)) return rc;
    return surfaces_impl(h, (const uint32_t*)h->stage_out.ptr, selected ? (const uint32_t*)h->stage_bits.ptr : nullptr, nx, ny, nz,
                         max_label, out_counts, nullptr, out_indices, capacity, out_total, nullptr, nullptr);
}

}  // namespace

extern "C" {

int sdfgpu_component_surfaces_device(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select_bits, int64_t nx, int64_t ny,
                                     int64_t nz, uint32_t max_label, int64_t* out_counts, uint32_t* d_indices, int64_t capacity,
                                     int64_t* out_total, uint32_t* d_surface_bits, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_labels) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if ((reinterpret_cast<uintptr_t>(d_labels) | reinterpret_cast<uintptr_t>(d_select_bits) | reinterpret_cast<uintptr_t>(d_indices) |
             reinterpret_cast<uintptr_t>(d_surface_bits)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_labels, d_select_bits, d_indices and d_surface_bits must be 4-byte aligned");
        if (int rc = check_surfaces_args(h, nx, ny, nz, max_label, out_counts, d_indices != nullptr, capacity, out_total)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return surfaces_impl(h, d_labels, d_select_bits, nx, ny, nz, max_label, out_counts, d_indices, nullptr, capacity, out_total,
                             d_surface_bits, (hipStream_t)stream);
    });
}

int sdfgpu_component_surfaces(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select_mask, int64_t nx, int64_t ny, int64_t nz,
                              uint32_t max_label, int64_t* out_counts, uint32_t* out_indices, int64_t capacity, int64_t* out_total) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!labels) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_surfaces_args(h, nx, ny, nz, max_label, out_counts, out_indices != nullptr, capacity, out_total)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return surfaces_host(h, labels, select_mask, nullptr, 0, 0, 0, 7, nx, ny, nz, max_label, out_counts, out_indices, capacity, out_total);
    });
}

int sdfgpu_component_surfaces_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                                    int64_t nx, int64_t ny, int64_t nz, int class_mask, uint32_t max_label, int64_t* out_counts,
                                    uint32_t* out_indices, int64_t capacity, int64_t* out_total) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_component_layout(h, cell_stride, occupancy_offset, component_offset)) return rc;
        if (class_mask < 1 || class_mask > 7)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "class_mask must be a nonzero combination of FILLED (1), EMPTY (2) and UNKNOWN (4)");
        if (int rc = check_surfaces_args(h, nx, ny, nz, max_label, out_counts, out_indices != nullptr, capacity, out_total)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return surfaces_host(h, nullptr, nullptr, cells, cell_stride, occupancy_offset, component_offset, class_mask, nx, ny, nz, max_label,
                             out_counts, out_indices, capacity, out_total);
    });
}

}  // extern "C"
