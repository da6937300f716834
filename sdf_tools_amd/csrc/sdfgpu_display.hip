// sdfgpu_display.hip -- the display-export kernels (sdfgpu_display.hpp) and their launchers.  Compiled beside sdfgpu.hip and linked
// into the same libsdfgpu.so (sdf_tools_amd/build.py); the C ABI entry points live in sdfgpu.hip.
//
// The SDF colour map restates the host's `fabs(d / extremum) * 0.8 + 0.2` in double with the product and the sum rounded
// separately, so nothing in this file may be contracted into an FMA (hipcc contracts by default), as in sdfgpu_resample.hip.
//
// Launch sizes: every workgroup owns kDpTile voxels or elements, so the largest grid (2^32 - 1 voxels) is 2^20 workgroups -- no
// launch comes near 2^32 threads.
#pragma clang fp contract(off)
#include "sdfgpu_display.hpp"

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
