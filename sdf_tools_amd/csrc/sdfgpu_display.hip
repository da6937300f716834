// sdfgpu_display.hip -- the display-export kernels (sdfgpu_display.hpp) and their launchers.  Compiled beside sdfgpu.hip and linked
// into the same libsdfgpu.so (sdf_tools_amd/build.py).
// The family's host orchestration and C ABI entry points (sdfgpu_display_*) are at the end of this file, over the handle of
// sdfgpu_context.hpp.
//
// The SDF colour map restates the host's `fabs(d / extremum) * 0.8 + 0.2` in double with the product and the sum rounded
// separately, so nothing in this file may be contracted into an FMA (hipcc contracts by default), as in sdfgpu_resample.hip.
//
// Launch sizes: every workgroup owns kDpTile voxels or elements, so the largest grid (2^32 - 1 voxels) is 2^20 workgroups -- no
// launch comes near 2^32 threads.
// The host code at the end of this file falls under the pragma too.  It is compiled for baseline x86-64, which has no FMA to
// contract into, so the pragma changes nothing there -- look again before giving the host pass a -march.
#pragma clang fp contract(off)
#include "sdfgpu_context.hpp"
#include "sdfgpu_display.hpp"
#include "sdfgpu.h"

namespace sdfgpu {

namespace {

constexpr int kDpThreads = 256;
constexpr int kDpRounds = kDpTile / kDpThreads;

__device__ __forceinline__ uint32_t load_word(const DpSource& s, uint64_t v, uint32_t off) {
    return *reinterpret_cast<const uint32_t*>(s.cells + v * s.stride + off);
}

// the reference's literal comparisons on the float: 0 F, 1 E, 2 U, 3 N (NaN: none of the three)
__device__ __forceinline__ uint32_t occ_class(float o) { return o > 0.5f ? 0u : o < 0.5f ? 1u : o == 0.5f ? 2u : 3u; }
__device__ __forceinline__ uint32_t occ_class_at(const DpSource& s, uint64_t v) { return occ_class(__uint_as_float(load_word(s, v, s.occ_off))); }
__device__ __forceinline__ uint32_t class_key(uint32_t cls) { return cls < 2u ? cls : 2u; }       // (NaN falls into the reference's `else`)

// The 26-neighbour rule.  Classes as bits (F 1, E 2, U 4, N 8): a cell is a surface iff some in-bounds neighbour's class is in the
// set its own class asks for -- E: {F, U}; F: {E, U}; U: {F, E, N}; N: nothing.  No class asks for itself, so the cell may stay in
// the loop.  The loop bounds are clamped to the grid: no out-of-grid value is read.
__device__ __forceinline__ bool occ_surface(const DpSelect& a, uint64_t v, uint32_t cls) {
    const uint32_t want = cls == 0u ? 6u : cls == 1u ? 5u : cls == 2u ? 11u : 0u;
    if (!want) return false;
    const uint32_t v32 = (uint32_t)v, t = v32 / a.nz, z = v32 - t * a.nz, x = t / a.ny, y = t - x * a.ny;   // (v < n < 2^32)
    const uint32_t x0 = x ? x - 1 : 0u, x1 = x + 1 < a.nx ? x + 1 : x;
    const uint32_t y0 = y ? y - 1 : 0u, y1 = y + 1 < a.ny ? y + 1 : y;
    const uint32_t z0 = z ? z - 1 : 0u, z1 = z + 1 < a.nz ? z + 1 : z;
    uint32_t seen = 0;
    for (uint32_t xx = x0; xx <= x1; ++xx)
        for (uint32_t yy = y0; yy <= y1; ++yy) {
            const uint64_t row = ((uint64_t)xx * a.ny + yy) * a.nz;
            for (uint32_t zz = z0; zz <= z1; ++zz) seen |= 1u << occ_class_at(a.src, row + zz);
        }
    return (seen & want) != 0u;
}

// draw_keys is ascending: lower bound, then compare
__device__ __forceinline__ bool key_listed(const DpSelect& a, uint32_t key) {
    uint32_t lo = 0, hi = a.n_draw;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.draw_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < a.n_draw && a.draw_keys[lo] == key;
}

template <int RULE>
__device__ __forceinline__ bool evaluate(const DpSelect& a, uint64_t v, uint32_t& key) {
    if (RULE == kDpRuleOccupancy) {
        const uint32_t cls = occ_class_at(a.src, v);
        key = class_key(cls);
        bool drawn = (a.class_mask >> key) & 1u;
        if (drawn && a.surface_only) drawn = occ_surface(a, v, cls);
        return drawn;
    }
    if (RULE == kDpRuleKeyField) {
        key = load_word(a.src, v, a.src.key_off);
        bool drawn = a.draw_zero || key != 0u;
        if (drawn && a.filter) drawn = key_listed(a, key);
        if (drawn && a.class_mask != 7u) drawn = (a.class_mask >> class_key(occ_class_at(a.src, v))) & 1u;
        return drawn;
    }
    if (RULE == kDpRuleSdfNonPositive) {
        key = 0u;
        return __uint_as_float(load_word(a.src, v, 0u)) <= 0.0f;       // (NaN: not drawn)
    }
    key = load_word(a.src, v, 0u);                                      // kDpRuleGroupStart
    return v == 0 || load_word(a.src, v - 1, 0u) != key;
}

// ---- k_dp_select ----------------------------------------------------------------------------------------------------------------
template <int RULE>
__global__ __launch_bounds__(kDpThreads) void k_dp_select(const DpSelect a) {
    __shared__ uint32_t s_total, s_kmax, s_kinv;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) { s_total = 0u; s_kmax = 0u; s_kinv = 0u; }
    __syncthreads();
    uint32_t wtotal = 0, kmax = 0, kinv = 0;                    // drawn voxels of this wave (same in every lane); this lane's keys
    for (int r = 0; r < kDpRounds; ++r) {
        const uint64_t v = (uint64_t)blockIdx.x * kDpTile + (uint64_t)r * kDpThreads + threadIdx.x;
        uint32_t key = 0;
        const bool drawn = v < a.n && evaluate<RULE>(a, v, key);
        const uint64_t bal = __ballot(drawn);
        if (lane == 0) {                                        // (v is a multiple of 64 here: two whole words; bits past n are 0)
            a.bits[v >> 5] = (uint32_t)bal;
            a.bits[(v >> 5) + 1] = (uint32_t)(bal >> 32);
        }
        wtotal += (uint32_t)__popcll(bal);
        if (drawn) { kmax = max(kmax, key); kinv = max(kinv, ~key); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        kmax = max(kmax, (uint32_t)__shfl_down(kmax, o));
        kinv = max(kinv, (uint32_t)__shfl_down(kinv, o));
    }
    if (lane == 0 && wtotal) { atomicAdd(&s_total, wtotal); atomicMax(&s_kmax, kmax); atomicMax(&s_kinv, kinv); }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.tile_counts[blockIdx.x] = s_total;
        if (s_total) {
            atomicAdd(a.total, s_total);
            if (a.key_max) { atomicMax(a.key_max, s_kmax); atomicMax(a.key_max + 1, s_kinv); }
        }
    }
}

// ---- k_dp_contour ---------------------------------------------------------------------------------------------------------------
// The object contours: a cell that is filled for its own key is drawn iff some in-bounds cell n of the 26
// around it is NOT filled for that key (filled: occ > 0.5, or occ == 0.5 with unknown_is_filled; NaN never) at a squared offset
// |n - c|^2 <= reach.  Output contract of k_dp_select (bit words, tile counts, total, smallest and largest drawn key).
// A wave round is 64 consecutive cells of the scan order, so 64 consecutive z (of one row or of several short ones).  A round without
// a candidate loads nothing more.  Otherwise the nine (dx, dy) rows come in three phases -- the cell's own row, the four rows at
// dx^2 + dy^2 = 1, the four at 2 -- and a phase starts only while some candidate of the wave is undecided and the reach admits it.
// Within a phase all loads are issued before any is used: per row every in-grid lane loads the record (x + dx, y + dy, z) -- the
// lanes' addresses are consecutive records -- and z - 1 / z + 1 of that row come from lanes - 1 / + 1, which hold exactly those cells
// whenever they lie in the lane's own row; only lane 0 (z - 1) and lane 63 (z + 1) lack such a lane, and ONE more load per row serves
// both.  Indices are clamped at the grid faces: nothing outside the grid is read.
struct CtTag { uint32_t key, filled; };

__device__ __forceinline__ CtTag ct_load(const DpSelect& a, uint64_t v) {
    const float o = __uint_as_float(load_word(a.src, v, a.src.occ_off));
    CtTag t;
    t.key = load_word(a.src, v, a.src.key_off);                 // (not behind the occupancy: two independent loads of one record)
    t.filled = (o > 0.5f || (a.unknown_is_filled && o == 0.5f)) ? 1u : 0u;
    return t;
}

struct CtRow { CtTag c, e; bool ok; };                          // the row's cell at this lane's z; lane 0 / 63: the cell at z - 1 / z + 1

struct CtLane { uint32_t x, y, z, key; bool in, has_lo, has_hi; int lane; };

template <bool OWN>
__device__ __forceinline__ CtRow ct_row_load(const DpSelect& a, const CtLane& l, uint64_t v, CtTag own, int dx, int dy, bool with_dz) {
    CtRow r;
    r.ok = l.in && (dx < 0 ? l.x > 0u : dx > 0 ? l.x + 1u < a.nx : true) && (dy < 0 ? l.y > 0u : dy > 0 ? l.y + 1u < a.ny : true);
    r.c.key = 0u; r.c.filled = 0u;
    r.e = r.c;
    const uint64_t nb = OWN ? v : ((uint64_t)(l.x + dx) * a.ny + (uint64_t)(l.y + dy)) * a.nz + l.z;
    if (OWN) r.c = own;
    else if (r.ok) r.c = ct_load(a, nb);
    if (with_dz && r.ok && ((l.lane == 0 && l.has_lo) || (l.lane == 63 && l.has_hi))) r.e = ct_load(a, l.lane == 0 ? nb - 1 : nb + 1);
    return r;
}

// does the row show this lane a cell that is not filled for its key?  (whole waves: a ballot and two shuffles)
template <bool OWN>
__device__ __forceinline__ bool ct_row_foreign(const CtLane& l, const CtRow& r, bool with_dz) {
    bool foreign = !OWN && r.ok && !(r.c.filled && r.c.key == l.key);
    if (with_dz) {                                              // (uniform)
        const uint64_t fb = __ballot(r.c.filled != 0u);
        CtTag lo, hi;
        lo.key = __shfl_up(r.c.key, 1); hi.key = __shfl_down(r.c.key, 1);
        lo.filled = (uint32_t)(fb >> ((l.lane + 63) & 63)) & 1u; hi.filled = (uint32_t)(fb >> ((l.lane + 1) & 63)) & 1u;
        if (l.lane == 0) lo = r.e;
        if (l.lane == 63) hi = r.e;
        if (r.ok && l.has_lo && !(lo.filled && lo.key == l.key)) foreign = true;
        if (r.ok && l.has_hi && !(hi.filled && hi.key == l.key)) foreign = true;
    }
    return foreign;
}

// `v` < n in the lanes that are `in`; cand: this lane's cell is filled, listed and not the undrawn key 0.  Called by whole waves
// with reach >= 1.
__device__ __forceinline__ bool ct_round(const DpSelect& a, uint64_t v, bool in, CtTag own, bool cand, int lane) {
    constexpr int kDx[8] = {-1, 1, 0, 0, -1, -1, 1, 1}, kDy[8] = {0, 0, -1, 1, -1, 1, -1, 1};
    const uint32_t v32 = in ? (uint32_t)v : 0u, t = v32 / a.nz, z = v32 - t * a.nz, x = t / a.ny;     // (v < n < 2^32)
    CtLane l;
    l.x = x; l.y = t - x * a.ny; l.z = z; l.key = own.key; l.in = in; l.has_lo = in && z > 0u; l.has_hi = in && z + 1u < a.nz; l.lane = lane;
    const int reach = a.reach;
    bool drawn = ct_row_foreign<true>(l, ct_row_load<true>(a, l, v, own, 0, 0, true), true);
#pragma unroll
    for (int phase = 0; phase < 2; ++phase) {                   // rows at dx^2 + dy^2 = 1, then 2
        if (reach < phase + 1 || !__any(cand && !drawn)) break; // (uniform)
        const bool with_dz = reach >= phase + 2;
        CtRow r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = ct_row_load<false>(a, l, v, own, kDx[phase * 4 + j], kDy[phase * 4 + j], with_dz);
#pragma unroll
        for (int j = 0; j < 4; ++j) drawn |= ct_row_foreign<false>(l, r[j], with_dz);
    }
    return cand && drawn;
}

__global__ __launch_bounds__(kDpThreads) void k_dp_contour(const DpSelect a) {
    __shared__ uint32_t s_total, s_kmax, s_kinv;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) { s_total = 0u; s_kmax = 0u; s_kinv = 0u; }
    __syncthreads();
    uint32_t wtotal = 0, kmax = 0, kinv = 0;
    for (int r = 0; r < kDpRounds; ++r) {
        const uint64_t v = (uint64_t)blockIdx.x * kDpTile + (uint64_t)r * kDpThreads + threadIdx.x;
        const bool in = v < a.n;
        CtTag own;
        own.key = 0u; own.filled = 0u;
        if (in) own = ct_load(a, v);
        bool cand = in && own.filled && a.reach > 0 && (a.draw_zero || own.key != 0u);
        if (cand && a.filter) cand = key_listed(a, own.key);
        bool drawn = false;
        if (__any(cand)) drawn = ct_round(a, v, in, own, cand, lane);     // (uniform in the wave)
        const uint64_t bal = __ballot(drawn);
        if (lane == 0) {                                        // (as in k_dp_select)
            a.bits[v >> 5] = (uint32_t)bal;
            a.bits[(v >> 5) + 1] = (uint32_t)(bal >> 32);
        }
        wtotal += (uint32_t)__popcll(bal);
        if (drawn) { kmax = max(kmax, own.key); kinv = max(kinv, ~own.key); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        kmax = max(kmax, (uint32_t)__shfl_down(kmax, o));
        kinv = max(kinv, (uint32_t)__shfl_down(kinv, o));
    }
    if (lane == 0 && wtotal) { atomicAdd(&s_total, wtotal); atomicMax(&s_kmax, kmax); atomicMax(&s_kinv, kinv); }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.tile_counts[blockIdx.x] = s_total;
        if (s_total) {
            atomicAdd(a.total, s_total);
            if (a.key_max) { atomicMax(a.key_max, s_kmax); atomicMax(a.key_max + 1, s_kinv); }
        }
    }
}

// ---- k_dp_compact ---------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per tile.  Every wave loads the tile's 64 bit words (lane l: word l) and scans their popcounts, so
// each word's offset is known before any element moves; wave w then places the voxels of words 16 w .. 16 w + 15, one word a round,
// and no round waits for the one before.
constexpr int kCompactThreads = 256;
constexpr int kCompactWords = kDpTile / 64;                     // 64-bit words per tile: one per lane
static_assert(kCompactWords == 64, "k_dp_compact holds one bit word of the tile per lane");

__global__ __launch_bounds__(kCompactThreads) void k_dp_compact(const DpCompact a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x, lt = (1ull << lane) - 1ull;
    const uint64_t mine = reinterpret_cast<const uint64_t*>(a.bits)[tile * kCompactWords + lane];
    const uint32_t cnt = (uint32_t)__popcll(mine);
    uint32_t inc = cnt;                                         // inclusive scan of the words' counts over the wave
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    const uint64_t first = (uint64_t)a.tile_offsets[tile] + (inc - cnt);     // of this lane's word
    constexpr int kPerWave = kCompactWords / (kCompactThreads / 64);
    for (int r = wave * kPerWave; r < (wave + 1) * kPerWave; ++r) {
        const uint64_t w = __shfl(mine, r), base = __shfl(first, r);
        if (!w) continue;                                       // (uniform in the wave)
        if ((w >> lane) & 1ull) {
            const uint64_t v = tile * kDpTile + (uint64_t)r * 64 + lane, pos = base + (uint64_t)__popcll(w & lt);
            if (pos < a.capacity) {
                const uint32_t key = a.key_mode == kDpKeyZero   ? 0u
                                     : a.key_mode == kDpKeyWord ? load_word(a.src, v, a.src.key_off)
                                                                : class_key(occ_class_at(a.src, v));
                if (a.pairs) {
                    a.pairs[pos] = make_uint2(key, (uint32_t)v);
                } else {
                    a.idx[pos] = (uint32_t)v;
                    if (a.keys) a.keys[pos] = key;
                }
            }
        }
    }
}

// ---- k_dp_expand ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_double(uint32_t* p, double d) {
    p[0] = (uint32_t)__double2loint(d);
    p[1] = (uint32_t)__double2hiint(d);
}

__global__ __launch_bounds__(kDpThreads) void k_dp_expand(const DpExpand a) {
    for (int r = 0; r < kDpRounds; ++r) {
        const uint64_t e = (uint64_t)blockIdx.x * kDpTile + (uint64_t)r * kDpThreads + threadIdx.x;
        if (e >= a.count) return;
        const uint32_t i = a.idx[e], t = i / a.nz, z = i - t * a.nz, x = t / a.ny, y = t - x * a.ny;
        if (a.points) {                                         // cell * (i + 0.5): the sum is exact, the product rounds once
            uint32_t* p = a.points + e * 6;
            store_double(p, a.cell[0] * ((double)x + 0.5));
            store_double(p + 2, a.cell[1] * ((double)y + 0.5));
            store_double(p + 4, a.cell[2] * ((double)z + 0.5));
        }
        if (a.colors) {
            const uint32_t key = a.keys ? a.keys[e] : 0u;
            float* c = a.colors + e * 4;
            if (key < a.table_len) {
                const float* q = a.table + (uint64_t)key * 4;
                c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; c[3] = q[3];
            } else {
                c[0] = a.fallback[0]; c[1] = a.fallback[1]; c[2] = a.fallback[2]; c[3] = a.fallback[3];
            }
        }
    }
}

// ---- the SDF colour map ---------------------------------------------------------------------------------------------------------
// max starts at 0.0 and moves on d > max, min on d < min: NaN moves neither.  Positive floats order like their bits, so the maximum
// is an atomicMax of bits; the minimum is the negative value of the largest magnitude, an atomicMax of the bits without the sign.
__global__ __launch_bounds__(kDpThreads) void k_dp_minmax(const float* __restrict__ d, uint64_t n, DpStatus* st) {
    __shared__ uint32_t s_pos, s_neg;
    if (threadIdx.x == 0) { s_pos = 0u; s_neg = 0u; }
    __syncthreads();
    uint32_t pos = 0, neg = 0;
    for (int r = 0; r < kDpRounds; ++r) {
        const uint64_t v = (uint64_t)blockIdx.x * kDpTile + (uint64_t)r * kDpThreads + threadIdx.x;
        if (v >= n) break;
        const float f = d[v];
        const uint32_t u = __float_as_uint(f);
        if (f > 0.0f) pos = max(pos, u);
        else if (f < 0.0f) neg = max(neg, u & 0x7FFFFFFFu);
    }
    for (int o = 32; o > 0; o >>= 1) {
        pos = max(pos, (uint32_t)__shfl_down(pos, o));
        neg = max(neg, (uint32_t)__shfl_down(neg, o));
    }
    if ((threadIdx.x & 63) == 0) { if (pos) atomicMax(&s_pos, pos); if (neg) atomicMax(&s_neg, neg); }
    __syncthreads();
    if (threadIdx.x == 0) { if (s_pos) atomicMax(&st->pos_bits, s_pos); if (s_neg) atomicMax(&st->neg_bits, s_neg); }
}

__global__ __launch_bounds__(kDpThreads) void k_dp_sdf_colors(const float* __restrict__ d, uint64_t n, float alpha, const DpStatus* st,
                                                              float* colors) {
    const double dmax = (double)__uint_as_float(st->pos_bits), dmin = -(double)__uint_as_float(st->neg_bits);
    for (int r = 0; r < kDpRounds; ++r) {
        const uint64_t v = (uint64_t)blockIdx.x * kDpTile + (uint64_t)r * kDpThreads + threadIdx.x;
        if (v >= n) return;
        const float f = d[v];
        float cr = 0.0f, cg = 0.0f, cb = 0.0f;
        if (f > 0.0f) {
            const double q = fabs((double)f / dmax), m = q * 0.8;
            cg = (float)(m + 0.2);
        } else if (f < 0.0f) {
            const double q = fabs((double)f / dmin), m = q * 0.8;
            cr = (float)(m + 0.2);
        } else {
            cb = 1.0f;                                          // 0 and NaN
        }
        float* c = colors + v * 4;
        c[0] = cr; c[1] = cg; c[2] = cb; c[3] = alpha;
    }
}

unsigned grid_of(uint64_t n) { return (unsigned)dp_tiles(n); }

}  // namespace

hipError_t dp_launch_select(int rule, const DpSelect& a, hipStream_t s) {
    const dim3 grid(grid_of(a.n)), block(kDpThreads);
    switch (rule) {
        case kDpRuleOccupancy: hipLaunchKernelGGL(k_dp_select<kDpRuleOccupancy>, grid, block, 0, s, a); break;
        case kDpRuleKeyField: hipLaunchKernelGGL(k_dp_select<kDpRuleKeyField>, grid, block, 0, s, a); break;
        case kDpRuleSdfNonPositive: hipLaunchKernelGGL(k_dp_select<kDpRuleSdfNonPositive>, grid, block, 0, s, a); break;
        case kDpRuleGroupStart: hipLaunchKernelGGL(k_dp_select<kDpRuleGroupStart>, grid, block, 0, s, a); break;
        case kDpRuleContour: hipLaunchKernelGGL(k_dp_contour, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t dp_launch_compact(const DpCompact& a, hipStream_t s) {
    hipLaunchKernelGGL(k_dp_compact, dim3(grid_of(a.n)), dim3(kCompactThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t dp_launch_expand(const DpExpand& a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dp_expand, dim3(grid_of(a.count)), dim3(kDpThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t dp_launch_minmax(const float* d_sdf, uint64_t n, DpStatus* st, hipStream_t s) {
    hipLaunchKernelGGL(k_dp_minmax, dim3(grid_of(n)), dim3(kDpThreads), 0, s, d_sdf, n, st);
    return hipGetLastError();
}

hipError_t dp_launch_sdf_colors(const float* d_sdf, uint64_t n, float alpha, const DpStatus* st, float* d_colors, hipStream_t s) {
    hipLaunchKernelGGL(k_dp_sdf_colors, dim3(grid_of(n)), dim3(kDpThreads), 0, s, d_sdf, n, alpha, st, d_colors);
    return hipGetLastError();
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

// ---- display export (sdfgpu_display.hpp) --------------------------------------------------------------------------------------------
// Only dp_scratch, dp_sort and dp_out (and, in the host forms, the cell / field staging and the pinned chunks) are used.
constexpr const char* kDisplayTail = "the display export's uint32 indices cannot number it";

struct DisplayRequest {
    int rule = kDpRuleOccupancy;
    const uint32_t* draw_keys = nullptr;       // host, ascending; nullptr = no list
    int64_t n_draw_keys = 0;
    bool grouped = false;
    bool to_host = false;                      // the four result pointers are host memory (filled through dp_out)
    uint32_t* indices = nullptr;               // nullptr = the total only
    uint32_t* keys = nullptr;
    int64_t capacity = 0;
    uint32_t* group_keys = nullptr;
    uint32_t* group_offsets = nullptr;
    int64_t group_capacity = 0;
    int64_t* out_total = nullptr;
    int64_t* out_groups = nullptr;
};

int check_display_request(sdfgpu_handle h, const DisplayRequest& rq) {
    if (!rq.out_total) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
    if (rq.n_draw_keys < 0 || rq.n_draw_keys > (int64_t)0xFFFFFFFFll || (rq.n_draw_keys > 0 && !rq.draw_keys))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: n_draw_keys must be in [0, 2^32) and come with a list (got %lld)", (long long)rq.n_draw_keys);
    for (int64_t i = 1; rq.draw_keys && i < rq.n_draw_keys; ++i)
        if (rq.draw_keys[i] < rq.draw_keys[i - 1])
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: draw_keys must be ascending (entry %lld is %u after %u)", (long long)i,
                        rq.draw_keys[i], rq.draw_keys[i - 1]);
    if (rq.indices && rq.capacity < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: capacity must not be negative (got %lld)", (long long)rq.capacity);
    if (rq.grouped && (!rq.indices || !rq.group_keys || !rq.group_offsets || !rq.out_groups || rq.group_capacity < 0))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: the grouped form needs indices, group_keys, group_offsets, out_groups and a group capacity >= 0");
    if (!rq.to_host && ((reinterpret_cast<uintptr_t>(rq.indices) | reinterpret_cast<uintptr_t>(rq.keys) | reinterpret_cast<uintptr_t>(rq.group_keys) |
                         reinterpret_cast<uintptr_t>(rq.group_offsets)) & 3))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: device pointers must be 4-byte aligned");
    return SDFGPU_OK;
}

size_t dp_align8(size_t x) { return (x + 7) & ~(size_t)7; }
int dp_bit_length(uint32_t x) { int b = 0; while (b < 32 && (x >> b) != 0) ++b; return b; }

// sel: the source, the rule's options and the shape (device records).  Synchronises `st`.
int display_select_impl(sdfgpu_handle h, DpSelect sel, const DisplayRequest& rq, hipStream_t st) {
    const uint64_t n = sel.n, tiles = dp_tiles(n);
    const size_t key_bytes = dp_align8((size_t)rq.n_draw_keys * 4);
    const size_t off_keys = sizeof(DpStatus), off_bits = off_keys + key_bytes, off_counts = off_bits + (size_t)tiles * (kDpTile / 8),
                 off_sums = off_counts + dp_align8((size_t)tiles * 4),
                 bytes = off_sums + dp_align8((size_t)((tiles + kDpScanSeg - 1) / kDpScanSeg) * 4);
    if (int rc = ensure(h, h->dp_scratch, bytes, "display scratch")) return rc;
    char* const b = static_cast<char*>(h->dp_scratch.ptr);
    DpStatus* const d_st = reinterpret_cast<DpStatus*>(b);
    uint32_t* const bits = reinterpret_cast<uint32_t*>(b + off_bits);
    uint32_t* const counts = reinterpret_cast<uint32_t*>(b + off_counts);
    uint32_t* const sums = reinterpret_cast<uint32_t*>(b + off_sums);
    HIP_TRY(h, hipMemsetAsync(d_st, 0, sizeof(DpStatus), st));
    if (rq.n_draw_keys) HIP_TRY(h, hipMemcpyAsync(b + off_keys, rq.draw_keys, (size_t)rq.n_draw_keys * 4, hipMemcpyHostToDevice, st));
    sel.draw_keys = reinterpret_cast<const uint32_t*>(b + off_keys);
    sel.n_draw = (uint32_t)rq.n_draw_keys;
    sel.filter = rq.draw_keys != nullptr;
    sel.bits = bits;
    sel.tile_counts = counts;
    sel.total = &d_st->total;
    sel.key_max = &d_st->key_max;
    HIP_TRY(h, dp_launch_select(rq.rule, sel, st));
    DpStatus status;
    HIP_TRY(h, hipMemcpyAsync(&status, d_st, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t total = status.total;
    *rq.out_total = (int64_t)total;
    if (rq.out_groups) *rq.out_groups = 0;
    if (!rq.indices) return SDFGPU_OK;                          // the total only
    if ((uint64_t)rq.capacity < total)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: the buffers hold %lld elements, %llu voxels are drawn (the total is valid)",
                    (long long)rq.capacity, (unsigned long long)total);
    // where the results are built: the caller's device arrays or dp_out
    const uint64_t gmax = std::min<uint64_t>(total, rq.grouped ? (uint64_t)rq.group_capacity : 0);
    uint32_t *d_idx = rq.indices, *d_keys = rq.keys, *d_gkeys = rq.group_keys, *d_goffs = rq.group_offsets;
    if (rq.to_host) {                                           // indices | keys (only when someone reads them) | group keys | group offsets
        const size_t key_words = rq.keys || rq.grouped ? (size_t)total : 0;
        if (int rc = ensure(h, h->dp_out, ((size_t)total + key_words + (size_t)gmax * 2 + 1) * 4, "display results")) return rc;
        d_idx = static_cast<uint32_t*>(h->dp_out.ptr);
        d_keys = key_words ? d_idx + total : nullptr;
        d_gkeys = d_idx + total + key_words;
        d_goffs = d_gkeys + gmax;
    }
    // sort only the bits in which the drawn keys differ: all of them agree above bit_length(max ^ min)
    const int key_bits = rq.grouped && total ? dp_bit_length(status.key_max ^ ~status.key_inv_max) : 0;
    const SfPairSortPlan sp = key_bits ? sf_pair_sort_plan(total, key_bits) : SfPairSortPlan();
    const bool own_keys = rq.grouped && !d_keys;               // the group boundaries are read from the sorted keys
    if (sp.bytes || own_keys) {
        if (int rc = ensure(h, h->dp_sort, sp.bytes + (own_keys ? (size_t)total * 4 : 0), "display sort scratch")) return rc;
        if (own_keys) d_keys = reinterpret_cast<uint32_t*>(static_cast<char*>(h->dp_sort.ptr) + sp.bytes);
    }
    if (total) {
        sf_launch_scan(counts, tiles, sums, st);
        DpCompact c;
        c.src = sel.src;
        c.key_mode = rq.rule == kDpRuleOccupancy ? kDpKeyClass : rq.rule == kDpRuleKeyField || rq.rule == kDpRuleContour ? kDpKeyWord : kDpKeyZero;
        c.n = n;
        c.bits = bits;
        c.tile_offsets = counts;
        c.capacity = total;
        if (key_bits) c.pairs = static_cast<uint2*>(h->dp_sort.ptr);
        else { c.idx = d_idx; c.keys = d_keys; }
        HIP_TRY(h, dp_launch_compact(c, st));
        if (key_bits) HIP_TRY(h, sf_launch_sort_pairs(sp, key_bits, h->dp_sort.ptr, d_idx, d_keys, st));
    }
    uint64_t groups = 0;
    if (rq.grouped) {
        if (total) {                                            // the same three steps over the sorted keys (their tiles fit the main pass's scratch)
            DpSelect g;
            g.src.cells = reinterpret_cast<const char*>(d_keys);
            g.src.stride = 4;
            g.src.occ_off = 0;                                  // (not read by this rule)
            g.src.key_off = 0;                                  // the key IS the record: k_dp_compact reads it at offset 0
            g.n = total;
            g.bits = bits;
            g.tile_counts = counts;
            g.total = &d_st->groups;
            HIP_TRY(h, dp_launch_select(kDpRuleGroupStart, g, st));
            HIP_TRY(h, hipMemcpyAsync(&status, d_st, sizeof status, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            groups = status.groups;
            *rq.out_groups = (int64_t)groups;
            if ((uint64_t)rq.group_capacity < groups)
                return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: the group arrays hold %lld groups, the drawn voxels have %llu keys (total and groups are valid)",
                            (long long)rq.group_capacity, (unsigned long long)groups);
            sf_launch_scan(counts, dp_tiles(total), sums, st);
            // the same kernel with other meanings: its "voxels" are the positions in the sorted key array (records of one word,
            // stride 4, key at offset 0), so c.idx receives the positions of the group starts = the group offsets, and c.keys
            // load_word(sorted keys, position) = the group keys
            DpCompact c;
            c.src = g.src;
            c.key_mode = kDpKeyWord;
            c.n = total;
            c.bits = bits;
            c.tile_offsets = counts;
            c.capacity = groups;
            c.idx = d_goffs;
            c.keys = d_gkeys;
            HIP_TRY(h, dp_launch_compact(c, st));
        }
        HIP_TRY(h, hipMemcpyAsync(d_goffs + groups, &d_st->total, 4, hipMemcpyDeviceToDevice, st));      // group_offsets[groups] = total
    }
    HIP_TRY(h, hipGetLastError());
    if (rq.to_host) {
        if (int rc = copy_to_host(h, rq.indices, d_idx, (size_t)total * 4, st)) return rc;
        if (rq.keys) if (int rc = copy_to_host(h, rq.keys, d_keys, (size_t)total * 4, st)) return rc;
        if (rq.grouped) {
            if (int rc = copy_to_host(h, rq.group_keys, d_gkeys, (size_t)groups * 4, st)) return rc;
            if (int rc = copy_to_host(h, rq.group_offsets, d_goffs, ((size_t)groups + 1) * 4, st)) return rc;
        }
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    return SDFGPU_OK;
}

int check_display_cells(sdfgpu_handle h, const void* cells, size_t stride, size_t occ_off, size_t key_off, int64_t nx, int64_t ny, int64_t nz,
                        int rule, int class_mask, DpSelect& sel) {
    if (!cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
    if (rule != SDFGPU_DISPLAY_OCCUPANCY && rule != SDFGPU_DISPLAY_KEY_FIELD)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: rule must be SDFGPU_DISPLAY_OCCUPANCY (0) or SDFGPU_DISPLAY_KEY_FIELD (1), got %d", rule);
    if (int rc = check_cell_layout(h, stride, occ_off)) return rc;
    if (rule == SDFGPU_DISPLAY_KEY_FIELD && ((key_off % 4) || key_off + 4 > stride))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: key_offset must be 4-byte aligned and inside the record");
    if (class_mask < 0 || class_mask > 7)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: class_mask must be a combination of FILLED (1), EMPTY (2) and UNKNOWN (4)");
    if (int rc = check_dims_u32(h, nx, ny, nz, kDisplayTail)) return rc;
    sel.src.stride = stride;
    sel.src.occ_off = (uint32_t)occ_off;
    sel.src.key_off = (uint32_t)key_off;
    sel.class_mask = (uint32_t)class_mask;
    sel.nx = (uint32_t)nx; sel.ny = (uint32_t)ny; sel.nz = (uint32_t)nz;
    sel.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    return SDFGPU_OK;
}

// the contour's records: the layout checks of the key-field rule, and a reach of 0 .. 3
int check_display_contour(sdfgpu_handle h, const void* cells, size_t stride, size_t occ_off, size_t key_off, int64_t nx, int64_t ny, int64_t nz,
                          int reach, DpSelect& sel) {
    if (int rc = check_display_cells(h, cells, stride, occ_off, key_off, nx, ny, nz, SDFGPU_DISPLAY_KEY_FIELD, 7, sel)) return rc;
    if (reach < 0 || reach > 3)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: the contour's reach must be 0 .. 3 (sdfgpu_display_contour_reach), got %d", reach);
    sel.reach = reach;
    return SDFGPU_OK;
}

int check_display_sdf(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, DpSelect& sel) {
    if (!sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
    if (int rc = check_dims_u32(h, nx, ny, nz, kDisplayTail)) return rc;
    sel.src.stride = 4;
    sel.nx = (uint32_t)nx; sel.ny = (uint32_t)ny; sel.nz = (uint32_t)nz;
    sel.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    return SDFGPU_OK;
}

// a = min(max(alpha, 0), 1); the extrema into dp_scratch's status words, then one rgba per voxel.  Synchronises `st` (the status
// words are scratch of the handle).
int display_sdf_colors_impl(sdfgpu_handle h, const float* d_sdf, uint64_t n, float alpha, float* d_colors, hipStream_t st) {
    if (int rc = ensure(h, h->dp_scratch, sizeof(DpStatus), "display scratch")) return rc;
    DpStatus* const d_st = static_cast<DpStatus*>(h->dp_scratch.ptr);
    HIP_TRY(h, hipMemsetAsync(d_st, 0, sizeof(DpStatus), st));
    HIP_TRY(h, dp_launch_minmax(d_sdf, n, d_st, st));
    HIP_TRY(h, dp_launch_sdf_colors(d_sdf, n, std::min(std::max(alpha, 0.0f), 1.0f), d_st, d_colors, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return SDFGPU_OK;
}

}  // namespace

extern "C" {

int sdfgpu_display_select_cells_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset,
                                       int64_t nx, int64_t ny, int64_t nz, int rule, int class_mask, int surface_only,
                                       const uint32_t* draw_keys, int64_t n_draw_keys, int draw_zero, int grouped, uint32_t* d_indices,
                                       uint32_t* d_keys, int64_t capacity, int64_t* out_total, uint32_t* d_group_keys,
                                       uint32_t* d_group_offsets, int64_t group_capacity, int64_t* out_groups, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        DpSelect sel;
        if (int rc = check_display_cells(h, d_cells, cell_stride, occupancy_offset, key_offset, nx, ny, nz, rule, class_mask, sel)) return rc;
        if (reinterpret_cast<uintptr_t>(d_cells) & 3) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: d_cells must be 4-byte aligned");
        DisplayRequest rq;
        rq.rule = rule == SDFGPU_DISPLAY_OCCUPANCY ? kDpRuleOccupancy : kDpRuleKeyField;
        rq.draw_keys = draw_keys; rq.n_draw_keys = n_draw_keys; rq.grouped = grouped != 0;
        rq.indices = d_indices; rq.keys = d_keys; rq.capacity = capacity; rq.out_total = out_total;
        rq.group_keys = d_group_keys; rq.group_offsets = d_group_offsets; rq.group_capacity = group_capacity; rq.out_groups = out_groups;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        sel.src.cells = static_cast<const char*>(d_cells);
        sel.surface_only = surface_only != 0;
        sel.draw_zero = draw_zero != 0;
        return display_select_impl(h, sel, rq, (hipStream_t)stream);
    });
}

int sdfgpu_display_select_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset, int64_t nx,
                                int64_t ny, int64_t nz, int rule, int class_mask, int surface_only, const uint32_t* draw_keys,
                                int64_t n_draw_keys, int draw_zero, int grouped, uint32_t* out_indices, uint32_t* out_keys, int64_t capacity,
                                int64_t* out_total, uint32_t* out_group_keys, uint32_t* out_group_offsets, int64_t group_capacity,
                                int64_t* out_groups) {
    return rz_wrap(h, nullptr, [&]() -> int {
        DpSelect sel;
        if (int rc = check_display_cells(h, cells, cell_stride, occupancy_offset, key_offset, nx, ny, nz, rule, class_mask, sel)) return rc;
        DisplayRequest rq;
        rq.rule = rule == SDFGPU_DISPLAY_OCCUPANCY ? kDpRuleOccupancy : kDpRuleKeyField;
        rq.draw_keys = draw_keys; rq.n_draw_keys = n_draw_keys; rq.grouped = grouped != 0; rq.to_host = true;
        rq.indices = out_indices; rq.keys = out_keys; rq.capacity = capacity; rq.out_total = out_total;
        rq.group_keys = out_group_keys; rq.group_offsets = out_group_offsets; rq.group_capacity = group_capacity; rq.out_groups = out_groups;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const size_t bytes = (size_t)sel.n * cell_stride;       // the null stream throughout: records through the cell staging
        if (int rc = stage_input(h, bytes)) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, cells, bytes)) return rc;
        sel.src.cells = static_cast<const char*>(h->stage_in.ptr);
        sel.surface_only = surface_only != 0;
        sel.draw_zero = draw_zero != 0;
        return display_select_impl(h, sel, rq, nullptr);
    });
}

int sdfgpu_display_contour_reach(double cell_size, int* out_reach) {
    if (!out_reach) return SDFGPU_ERR_INVALID_ARGUMENT;
    // the reference's own lines: `const float bdy = -1.9 * GetResolution()`, dist = the finished field of a filled cell at squared
    // distance D, drawn iff `dist < 0.0 && dist > bdy`.  NaN, zero and negative sizes fail every comparison: reach 0.
    const float bdy = -1.9 * cell_size;
    int reach = 0;
    for (int d = 1; d <= 3; ++d) {
        const float dist = -(float)(std::sqrt((double)d) * cell_size);
        if (dist < 0.0 && dist > bdy) reach = d;
    }
    *out_reach = reach;
    return SDFGPU_OK;
}

int sdfgpu_display_select_contour_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset,
                                         int64_t nx, int64_t ny, int64_t nz, int reach, int unknown_is_filled, const uint32_t* draw_keys,
                                         int64_t n_draw_keys, int draw_zero, int grouped, uint32_t* d_indices, uint32_t* d_keys,
                                         int64_t capacity, int64_t* out_total, uint32_t* d_group_keys, uint32_t* d_group_offsets,
                                         int64_t group_capacity, int64_t* out_groups, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        DpSelect sel;
        if (int rc = check_display_contour(h, d_cells, cell_stride, occupancy_offset, key_offset, nx, ny, nz, reach, sel)) return rc;
        if (reinterpret_cast<uintptr_t>(d_cells) & 3) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: d_cells must be 4-byte aligned");
        DisplayRequest rq;
        rq.rule = kDpRuleContour;
        rq.draw_keys = draw_keys; rq.n_draw_keys = n_draw_keys; rq.grouped = grouped != 0;
        rq.indices = d_indices; rq.keys = d_keys; rq.capacity = capacity; rq.out_total = out_total;
        rq.group_keys = d_group_keys; rq.group_offsets = d_group_offsets; rq.group_capacity = group_capacity; rq.out_groups = out_groups;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        sel.src.cells = static_cast<const char*>(d_cells);
        sel.unknown_is_filled = unknown_is_filled != 0;
        sel.draw_zero = draw_zero != 0;
        return display_select_impl(h, sel, rq, (hipStream_t)stream);
    });
}

int sdfgpu_display_select_contour(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset, int64_t nx,
                                  int64_t ny, int64_t nz, int reach, int unknown_is_filled, const uint32_t* draw_keys, int64_t n_draw_keys,
                                  int draw_zero, int grouped, uint32_t* out_indices, uint32_t* out_keys, int64_t capacity, int64_t* out_total,
                                  uint32_t* out_group_keys, uint32_t* out_group_offsets, int64_t group_capacity, int64_t* out_groups) {
    return rz_wrap(h, nullptr, [&]() -> int {
        DpSelect sel;
        if (int rc = check_display_contour(h, cells, cell_stride, occupancy_offset, key_offset, nx, ny, nz, reach, sel)) return rc;
        DisplayRequest rq;
        rq.rule = kDpRuleContour;
        rq.draw_keys = draw_keys; rq.n_draw_keys = n_draw_keys; rq.grouped = grouped != 0; rq.to_host = true;
        rq.indices = out_indices; rq.keys = out_keys; rq.capacity = capacity; rq.out_total = out_total;
        rq.group_keys = out_group_keys; rq.group_offsets = out_group_offsets; rq.group_capacity = group_capacity; rq.out_groups = out_groups;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const size_t bytes = (size_t)sel.n * cell_stride;       // the null stream throughout: records through the cell staging
        if (int rc = stage_input(h, bytes)) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, cells, bytes)) return rc;
        sel.src.cells = static_cast<const char*>(h->stage_in.ptr);
        sel.unknown_is_filled = unknown_is_filled != 0;
        sel.draw_zero = draw_zero != 0;
        return display_select_impl(h, sel, rq, nullptr);
    });
}

int sdfgpu_display_select_sdf_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, uint32_t* d_indices,
                                     int64_t capacity, int64_t* out_total, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        DpSelect sel;
        if (int rc = check_display_sdf(h, d_sdf, nx, ny, nz, sel)) return rc;
        if (reinterpret_cast<uintptr_t>(d_sdf) & 3) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: d_sdf must be 4-byte aligned");
        DisplayRequest rq;
        rq.rule = kDpRuleSdfNonPositive;
        rq.indices = d_indices; rq.capacity = capacity; rq.out_total = out_total;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        sel.src.cells = reinterpret_cast<const char*>(d_sdf);
        return display_select_impl(h, sel, rq, (hipStream_t)stream);
    });
}

int sdfgpu_display_select_sdf(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, uint32_t* out_indices, int64_t capacity,
                              int64_t* out_total) {
    return rz_wrap(h, nullptr, [&]() -> int {
        DpSelect sel;
        if (int rc = check_display_sdf(h, sdf, nx, ny, nz, sel)) return rc;
        DisplayRequest rq;
        rq.rule = kDpRuleSdfNonPositive;
        rq.to_host = true;
        rq.indices = out_indices; rq.capacity = capacity; rq.out_total = out_total;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = stage_input(h, (size_t)sel.n * 4)) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, sdf, (size_t)sel.n * 4)) return rc;
        sel.src.cells = static_cast<const char*>(h->stage_in.ptr);
        return display_select_impl(h, sel, rq, nullptr);
    });
}

int sdfgpu_display_expand_device(sdfgpu_handle h, const uint32_t* d_indices, const uint32_t* d_keys, int64_t count, int64_t nx, int64_t ny,
                                 int64_t nz, const double cell_sizes[3], double* d_points, float* d_colors, const float* d_color_table,
                                 int64_t table_entries, const float default_color[4], void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_indices || !cell_sizes || (!d_points && !d_colors)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
        if (d_colors && (!default_color || table_entries < 0 || table_entries > (int64_t)0xFFFFFFFFll || (table_entries > 0 && !d_color_table)))
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: colours need a default colour and a table of [0, 2^32) entries");
        if (count < 0 || count > (int64_t)0xFFFFFFFFll)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: count must be in [0, 2^32) (got %lld)", (long long)count);
        if (int rc = check_dims_u32(h, nx, ny, nz, kDisplayTail)) return rc;
        if ((reinterpret_cast<uintptr_t>(d_indices) | reinterpret_cast<uintptr_t>(d_keys) | reinterpret_cast<uintptr_t>(d_points) |
             reinterpret_cast<uintptr_t>(d_colors) | reinterpret_cast<uintptr_t>(d_color_table)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: device pointers must be 4-byte aligned");
        HIP_TRY(h, hipSetDevice(h->device));
        DpExpand a;
        a.idx = d_indices; a.keys = d_keys; a.count = (uint64_t)count;
        a.ny = (uint32_t)ny; a.nz = (uint32_t)nz;
        for (int i = 0; i < 3; ++i) a.cell[i] = cell_sizes[i];
        a.points = reinterpret_cast<uint32_t*>(d_points);
        a.colors = d_colors;
        if (d_colors) {
            a.table = d_color_table; a.table_len = (uint32_t)table_entries;
            for (int i = 0; i < 4; ++i) a.fallback[i] = default_color[i];
        }
        HIP_TRY(h, dp_launch_expand(a, (hipStream_t)stream));
        return SDFGPU_OK;
    });
}

int sdfgpu_display_sdf_colors_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, float alpha, float* d_colors,
                                     void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        DpSelect sel;
        if (!d_colors) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
        if (int rc = check_display_sdf(h, d_sdf, nx, ny, nz, sel)) return rc;
        if (std::isnan(alpha)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: alpha must not be NaN");
        if ((reinterpret_cast<uintptr_t>(d_sdf) | reinterpret_cast<uintptr_t>(d_colors)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: d_sdf and d_colors must be 4-byte aligned");
        HIP_TRY(h, hipSetDevice(h->device));
        return display_sdf_colors_impl(h, d_sdf, sel.n, alpha, d_colors, (hipStream_t)stream);
    });
}

int sdfgpu_display_sdf_colors(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, float alpha, float* out_colors) {
    return rz_wrap(h, nullptr, [&]() -> int {
        DpSelect sel;
        if (!out_colors) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
        if (int rc = check_display_sdf(h, sdf, nx, ny, nz, sel)) return rc;
        if (std::isnan(alpha)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: alpha must not be NaN");
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = stage_input(h, (size_t)sel.n * 4)) return rc;
        if (int rc = ensure(h, h->stage_out, (size_t)sel.n * 16, "output staging")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, sdf, (size_t)sel.n * 4)) return rc;
        if (int rc = display_sdf_colors_impl(h, (const float*)h->stage_in.ptr, sel.n, alpha, (float*)h->stage_out.ptr, nullptr)) return rc;
        return copy_to_host(h, out_colors, h->stage_out.ptr, (size_t)sel.n * 16);
    });
}

}  // extern "C"
