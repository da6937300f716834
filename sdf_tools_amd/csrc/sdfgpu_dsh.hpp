// sdfgpu_dsh.hpp -- the chunk-hashed sparse collision map (include/sdfgpu.h "Dynamic spatial hashed map"): its
// constants, the packing of a chunk coordinate into a table key, the hash, and the planning of the table's and the pool's sizes.
// Plain C++ without a HIP header, as sdfgpu_plan.hpp and sdfgpu_policy.hpp are: sdfgpu_dsh.hip includes it for its kernels and its host
// code, and tests/dsh_plan_harness.cpp, tests/dsh_rays_plan_harness.cpp, tests/dsh_fusion_plan_harness.cpp and
// tests/dsh_remove_plan_harness.cpp (and the later dsh_*_plan_harness.cpp) drive the arithmetic on the CPU under -fsanitize=address,undefined.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SDFGPU_DSH_HD __host__ __device__ __forceinline__
#else
#define SDFGPU_DSH_HD inline
#endif

namespace sdfgpu {

// ---- the contract's numbers ----------------------------------------------------------------------------------------------------------
constexpr int64_t kDshChunkBias = (int64_t)1 << 20;        // a chunk coordinate lies in [-2^20, 2^20): 21 bits once biased
constexpr int64_t kDshMaxChunkCells = 32768;               // n_x * n_y * n_z of a chunk
constexpr uint64_t kDshEmptyKey = ~(uint64_t)0;            // three 21-bit coordinates fill 63 bits: all ones is no key
constexpr uint32_t kDshChunkFilled = 1, kDshCellFilled = 2;   // a live chunk's state (SDFGPU_DSH_FOUND_IN_CHUNK / _IN_CELL)
constexpr uint32_t kDshStateMask = 3;
constexpr uint32_t kDshTouched = 0x80000000u;              // set in a chunk's state word between k_dsh_touch and k_dsh_expand (and, in a fused
                                                           // frame, again between k_dsh_ray_touch and k_dsh_ray_fuse) only
constexpr uint64_t kDshMinTable = 16;                      // entries; the table's capacity is a power of two
constexpr int64_t kDshMaxBatch = (int64_t)1 << 31;         // operations of one batch (their table positions are uint32)

// What the pool keeps per chunk beside its cells.
struct DshChunkHead {
    uint64_t key;       // the packed chunk coordinate (what the rehash and the export read)
    uint64_t record;    // the chunk's record while it is chunk-filled
    uint32_t state;     // kDshChunkFilled / kDshCellFilled (0 only between k_dsh_init_new and the kernel that fills the chunk)
    uint32_t reserved;
};
static_assert(sizeof(DshChunkHead) == 24, "DshChunkHead is 24 bytes");

// ---- keys ----------------------------------------------------------------------------------------------------------------------------
SDFGPU_DSH_HD bool dsh_chunk_in_range(int64_t c) { return c >= -kDshChunkBias && c < kDshChunkBias; }

// (c_x, c_y, c_z), each in range -> key.  x takes the high bits, so keys ascend as (c_x, c_y, c_z) ascends lexicographically.
SDFGPU_DSH_HD uint64_t dsh_pack_key(int64_t cx, int64_t cy, int64_t cz) {
    return ((uint64_t)(cx + kDshChunkBias) << 42) | ((uint64_t)(cy + kDshChunkBias) << 21) | (uint64_t)(cz + kDshChunkBias);
}
SDFGPU_DSH_HD void dsh_unpack_key(uint64_t key, int64_t& cx, int64_t& cy, int64_t& cz) {
    cx = (int64_t)(key >> 42) - kDshChunkBias;
    cy = (int64_t)((key >> 21) & 0x1FFFFF) - kDshChunkBias;
    cz = (int64_t)(key & 0x1FFFFF) - kDshChunkBias;
}

// floor(i / n) for n > 0 (C++ division truncates)
SDFGPU_DSH_HD int64_t dsh_floor_div(int64_t i, int64_t n) {
    const int64_t q = i / n;
    return (i % n != 0 && i < 0) ? q - 1 : q;
}

// the finaliser of splitmix64: every key bit reaches the low bits that index the table
SDFGPU_DSH_HD uint64_t dsh_hash(uint64_t k) {
    k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 27; k *= 0x94D049BB133111EBull;
    return k ^ (k >> 31);
}

// ---- sizes (64-bit throughout) ----------------------------------------------------------------------------------------------------------
// The smallest table in which `chunks` keys fill at most half the entries: a probe always meets an empty entry, and a batch that is
// sized for (live chunks + operations) cannot fill the table while it inserts.
inline uint64_t dsh_table_capacity(uint64_t chunks) {
    uint64_t cap = kDshMinTable;
    while (cap < 2 * chunks) cap <<= 1;
    return cap;
}
inline uint64_t dsh_table_bytes(uint64_t capacity) { return capacity * (8 + 4); }        // keys | slots
inline uint64_t dsh_pool_bytes(uint64_t chunks, uint64_t cells_per_chunk) { return chunks * (sizeof(DshChunkHead) + 8 * cells_per_chunk); }

// The pool's capacity for `needed` chunks when it holds `capacity`: unchanged while it suffices; otherwise twice the old one (at least
// `needed`), or exactly `needed` where the doubling would pass the byte limit (0 = none).  False when even that passes the limit.
inline bool dsh_plan_pool(uint64_t capacity, uint64_t needed, uint64_t cells_per_chunk, uint64_t table_bytes, uint64_t byte_limit,
                          uint64_t* out_capacity) {
    *out_capacity = capacity;
    if (needed <= capacity) return true;
    uint64_t want = capacity * 2 > needed ? capacity * 2 : needed;
    if (byte_limit && table_bytes + dsh_pool_bytes(want, cells_per_chunk) > byte_limit) want = needed;
    if (byte_limit && table_bytes + dsh_pool_bytes(want, cells_per_chunk) > byte_limit) return false;
    *out_capacity = want;
    return true;
}

// ---- removal ----------------------------------------------------------------------------------------------------------
constexpr int64_t kDshMaxBoxCell = (int64_t)1 << 40;       // |lower| and extent of a box of cells are at most this
constexpr uint32_t kDshKept = 0xFFFFFFFFu;                 // a slot's word in the removal's flag array while nothing removes it
constexpr uint32_t kDshPairItems = 16;                     // slots per thread of the pairing scan: a tile is kDshPairTile slots
constexpr uint32_t kDshPairTile = 256 * kDshPairItems;

// A box of cells as a closed range of chunk coordinates per axis, clamped to the key range; `empty` when it holds no chunk.
struct DshChunkRange {
    int64_t lo[3], hi[3];
    int empty;
};

inline bool dsh_box_ok(const int64_t lower[3], const int64_t extent[3]) {
    for (int a = 0; a < 3; ++a)
        if (lower[a] < -kDshMaxBoxCell || lower[a] > kDshMaxBoxCell || extent[a] < 0 || extent[a] > kDshMaxBoxCell) return false;
    return true;
}

// The chunks that hold at least one of the cells lower[a] .. lower[a] + extent[a] - 1 (dsh_box_ok holds: no sum passes 2^41).
inline DshChunkRange dsh_box_chunk_range(const int64_t lower[3], const int64_t extent[3], const int64_t n[3]) {
    DshChunkRange r{};
    for (int a = 0; a < 3; ++a) {
        if (extent[a] == 0) { r.empty = 1; r.lo[a] = 0; r.hi[a] = -1; continue; }
        const int64_t lo = dsh_floor_div(lower[a], n[a]), hi = dsh_floor_div(lower[a] + extent[a] - 1, n[a]);
        r.lo[a] = lo < -kDshChunkBias ? -kDshChunkBias : lo;
        r.hi[a] = hi > kDshChunkBias - 1 ? kDshChunkBias - 1 : hi;
        if (r.lo[a] > r.hi[a]) r.empty = 1;
    }
    return r;
}

// whether the chunk of `key` holds a cell of the box (unpacked coordinates only)
SDFGPU_DSH_HD bool dsh_key_in_range(uint64_t key, const DshChunkRange& r) {
    int64_t c[3];
    dsh_unpack_key(key, c[0], c[1], c[2]);
    bool in = !r.empty;
    for (int a = 0; a < 3; ++a) in = in && c[a] >= r.lo[a] && c[a] <= r.hi[a];
    return in;
}

// The pairing of a removal, on the host (tests/dsh_remove_plan_harness.cpp holds the kernels' scan against it): with `keep` slots
// unflagged, the j-th flagged slot below `keep` (a hole) takes the j-th unflagged slot at or above it (a mover), both ascending.
// Returns the number of pairs; holes / movers need room for min(keep, n - keep) entries.
inline uint64_t dsh_pair_model(const uint8_t* flagged, uint64_t n, uint64_t keep, uint32_t* holes, uint32_t* movers) {
    uint64_t n_holes = 0, n_movers = 0;
    for (uint64_t s = 0; s < n; ++s) {
        if (s < keep && flagged[s]) holes[n_holes++] = (uint32_t)s;
        if (s >= keep && !flagged[s]) movers[n_movers++] = (uint32_t)s;
    }
    return n_holes == n_movers ? n_holes : ~(uint64_t)0;
}
inline uint64_t dsh_pair_tiles(uint64_t n) { return (n + kDshPairTile - 1) / kDshPairTile; }

// What shrink leaves: the pool at max(live + spare, 1) chunks and the table at dsh_table_capacity(live + spare), each only where
// that is smaller than what the map holds.  (spare is clamped where it cannot matter: no sum overflows.)
inline void dsh_plan_shrink(uint64_t live, uint64_t spare, uint64_t pool_cap, uint64_t table_cap, uint64_t* out_pool, uint64_t* out_table) {
    if (spare > ((uint64_t)1 << 32)) spare = (uint64_t)1 << 32;
    const uint64_t chunks = live + spare;
    const uint64_t pool = chunks > 1 ? chunks : 1, table = dsh_table_capacity(chunks);
    *out_pool = pool < pool_cap ? pool : pool_cap;
    *out_table = table < table_cap ? table : table_cap;
}

// ---- frontier cells ---------------------------------------------------------------------------------------------
constexpr uint32_t kDshFrontier26 = 1;                     // SDFGPU_DSH_FRONTIER_26

// The candidates of a frontier list: a closed range of global cells per axis, clamped to the cells of the chunks in [-2^20, 2^20)
// (no cell outside them belongs to a live chunk), and the chunks that hold them.  `chunks.empty` when the box holds no such cell.
struct DshFrontierBox {
    DshChunkRange chunks;
    int64_t lo[3], hi[3];
};

// extent >= 1 on every axis and lower + extent - 1 is an int64
inline bool dsh_frontier_box_ok(const int64_t lower[3], const int64_t extent[3]) {
    for (int a = 0; a < 3; ++a)
        if (extent[a] < 1 || lower[a] > INT64_MAX - (extent[a] - 1)) return false;
    return true;
}

// The box lower .. lower + extent - 1 (dsh_frontier_box_ok holds), or with both null every cell a chunk can hold.
inline DshFrontierBox dsh_frontier_box(const int64_t* lower, const int64_t* extent, const int64_t n[3]) {
    DshFrontierBox b{};
    for (int a = 0; a < 3; ++a) {
        const int64_t first = -kDshChunkBias * n[a], last = kDshChunkBias * n[a] - 1;      // |.| <= 2^35
        const int64_t lo = lower ? lower[a] : first, hi = lower ? lower[a] + (extent[a] - 1) : last;
        b.lo[a] = lo < first ? first : lo;
        b.hi[a] = hi > last ? last : hi;
        if (b.lo[a] > b.hi[a]) { b.chunks.empty = 1; b.chunks.lo[a] = 0; b.chunks.hi[a] = -1; continue; }
        b.chunks.lo[a] = dsh_floor_div(b.lo[a], n[a]);
        b.chunks.hi[a] = dsh_floor_div(b.hi[a], n[a]);
    }
    return b;
}

// 64-bit words of a chunk's frontier mask (one bit per cell slot) in the list form's scratch
SDFGPU_DSH_HD uint64_t dsh_frontier_mask_words(uint64_t cells_per_chunk) { return (cells_per_chunk + 63) / 64; }

// The steps d in {-1, 0, 1} along one axis that lead from the cell at `l` of a chunk of n cells into the chunk `o` chunks further
// (o in {-1, 0, 1}): the closed range lo .. hi, empty (lo > hi) where no step does.
SDFGPU_DSH_HD void dsh_axis_steps(int64_t l, int64_t n, int o, int& lo, int& hi) {
    if (o < 0) { lo = -1; hi = l == 0 ? -1 : -2; }
    else if (o > 0) { lo = 1; hi = l == n - 1 ? 1 : 0; }
    else { lo = l > 0 ? -1 : 0; hi = l < n - 1 ? 1 : 0; }
}

// ---- connected components ----------------------------------------------------------------------------------------
// A node is a cell of a cell-filled chunk or a whole chunk-filled chunk.  Nodes are numbered in export order: a chunk's node base is
// the number of nodes of the live chunks with a smaller key, its cells follow in slot order.  N nodes must stay below 2^32 - 1.
constexpr uint32_t kDshComponentsUnknownApart = 1;         // SDFGPU_DSH_COMPONENTS_UNKNOWN_APART
constexpr uint32_t kDshCcTile = 8192;                      // cell slots one workgroup of k_dsh_cc_local labels in LDS
constexpr uint32_t kDshCcRankChunk = 8192;                 // kRankChunk of sdfgpu_unionfind.hpp (a device header this one cannot include)
constexpr uint64_t kDshCcMaxNodes = 0xFFFFFFFFull;         // N < this

// weight of a live chunk in the node numbering, and N from the counts by state (64-bit: 2^31 chunks of 2^15 cells stay below 2^47)
SDFGPU_DSH_HD uint64_t dsh_cc_weight(uint32_t state, uint64_t cells_per_chunk) { return (state & kDshStateMask) == kDshCellFilled ? cells_per_chunk : 1; }
SDFGPU_DSH_HD uint64_t dsh_cc_nodes(uint64_t cell_filled, uint64_t chunk_filled, uint64_t cells_per_chunk) { return cell_filled * cells_per_chunk + chunk_filled; }
SDFGPU_DSH_HD bool dsh_cc_nodes_ok(uint64_t nodes) { return nodes < kDshCcMaxNodes; }
SDFGPU_DSH_HD uint64_t dsh_cc_tiles(uint64_t cells_per_chunk) { return (cells_per_chunk + kDshCcTile - 1) / kDshCcTile; }
// the node of cell slot k of a chunk with node base `base` (a chunk-filled chunk is its base alone)
SDFGPU_DSH_HD uint64_t dsh_cc_node(uint64_t base, bool has_cells, uint32_t k) { return base + (has_cells ? (uint64_t)k : 0); }

// The class of an occupancy: filled (1) is > 0.5; everything else is free (0), or with `apart` free is < 0.5 and the rest -- 0.5 and
// NaN -- is unknown (2).
SDFGPU_DSH_HD uint32_t dsh_cc_class(float occupancy, bool apart) { return occupancy > 0.5f ? 1u : (apart && !(occupancy < 0.5f)) ? 2u : 0u; }

// The idx-th pair of cells across a chunk's low face along `axis`: cell slot k of the chunk, slot k2 of the chunk one lower along the
// axis, and `back`, the step to the pair before it along z (x and y faces) or y (z faces), 0 where there is none.  A pair whose
// predecessor pair is of its own class on both sides is joined through that pair and needs no link.
SDFGPU_DSH_HD void dsh_cc_face_pair(int axis, uint32_t idx, const int64_t n[3], uint32_t& k, uint32_t& k2, uint32_t& back) {
    const uint32_t nx = (uint32_t)n[0], ny = (uint32_t)n[1], nz = (uint32_t)n[2];
    if (axis == 0) { k = idx; k2 = idx + (nx - 1) * ny * nz; back = idx % nz ? 1u : 0u; }
    else if (axis == 1) { const uint32_t ix = idx / nz, iz = idx - ix * nz; k = ix * ny * nz + iz; k2 = k + (ny - 1) * nz; back = iz ? 1u : 0u; }
    else { k = idx * nz; k2 = k + nz - 1; back = idx % ny ? nz : 0u; }
}
// candidate pairs of one face: its cells, but ONE where both chunks are chunk-filled (two nodes, one link)
SDFGPU_DSH_HD uint64_t dsh_cc_face_pairs(bool own_cells, bool other_cells, uint64_t face_cells) { return own_cells || other_cells ? face_cells : 1; }

// the update's scratch behind the counters: per-chunk node bases | one label word per node | the rank tables (rb | wr | cc | co of
// sdfgpu_unionfind.hpp), each section rounded up to 256 bytes
inline uint64_t dsh_cc_rank_bytes(uint64_t nodes) {
    const uint64_t chunks = (nodes + kDshCcRankChunk - 1) / kDshCcRankChunk;
    return (2 * chunks * (kDshCcRankChunk / 32) + 2 * chunks) * 4;
}
inline uint64_t dsh_cc_bases_bytes(uint64_t live) { return live * 4; }
inline uint64_t dsh_cc_label_bytes(uint64_t nodes) { return nodes * 4; }
// (dsh_components_impl cuts its sections by the three functions above and refuses to run where its cut's total is not this)
inline uint64_t dsh_cc_scratch_bytes(uint64_t live, uint64_t nodes) {
    const auto up = [](uint64_t b) { return (b + 255) & ~(uint64_t)255; };
    return up(dsh_cc_bases_bytes(live)) + up(dsh_cc_label_bytes(nodes)) + up(dsh_cc_rank_bytes(nodes));
}

// ---- a frame of sensor rays ------------------------------------------------------------------------------------------
constexpr double kDshMaxRangeCells = 65536.0;              // R = max_range / cell_size lies in (0, 65536]
constexpr uint64_t kDshRayBoundCap = (uint64_t)1 << 62;    // where the bound below saturates

// Along one axis a ray writes cells whose boundary lies within R (1 + a few ulp) cells of the sensor, and one more: at most
// ceil(R) + 2 steps.  `range_cells` is that ceil(R), at most 65536.
SDFGPU_DSH_HD uint64_t dsh_ray_axis_steps(uint64_t range_cells) { return range_cells + 2; }

// How many chunks one ray from global cell i0 to i1 can write into.  Its walk is monotone along every axis, so it crosses each chunk
// boundary between its two ends once: a ray that is not long enters exactly this many chunks.  A long ray stops inside the range.
SDFGPU_DSH_HD uint64_t dsh_ray_chunks(const int64_t i0[3], const int64_t i1[3], const int64_t n[3], bool is_long, uint64_t range_cells) {
    uint64_t chunks = 1;
    for (int a = 0; a < 3; ++a) {
        const int64_t c0 = dsh_floor_div(i0[a], n[a]), c1 = dsh_floor_div(i1[a], n[a]);
        uint64_t across = (uint64_t)(c1 > c0 ? c1 - c0 : c0 - c1);                          // at most 2^21
        const uint64_t within = dsh_ray_axis_steps(range_cells) / (uint64_t)n[a] + 1;
        if (is_long && across > within) across = within;
        chunks += across;
    }
    return chunks;
}

// Steps of one ray's walk that cannot be passed (the kernels' loop guard; the walk ends earlier by itself).
inline uint64_t dsh_ray_max_steps(uint64_t range_cells) { return 3 * dsh_ray_axis_steps(range_cells) + 2; }

// How many chunks a frame of `rays` rays of at most `range_cells` cells can enter, whatever the map holds: the smaller of
//   rays * (1 + sum over the axes of (steps / n_a + 1))    a ray changes chunk along an axis once per n_a steps, and once more
//   product over the axes of ((2 steps) / n_a + 2)         every cell lies within `steps` cells of the sensor's cell
// saturating at kDshRayBoundCap.  The table of a frame is sized for the live chunks plus this; where that would make the table
// grow, the frame's rays are counted first (the sum of dsh_ray_chunks) and the smaller of the two numbers sizes it.
inline uint64_t dsh_ray_chunk_bound(uint64_t rays, uint64_t range_cells, const int64_t n[3]) {
    const uint64_t steps = dsh_ray_axis_steps(range_cells);
    uint64_t per_ray = 1, box = 1;
    for (int a = 0; a < 3; ++a) {
        per_ray += steps / (uint64_t)n[a] + 1;                                 // at most 1 + 3 * 65539
        const uint64_t across = (2 * steps) / (uint64_t)n[a] + 2;               // at most 131078: three of them stay below 2^52
        box *= across;
    }
    const uint64_t by_rays = rays > kDshRayBoundCap / per_ray ? kDshRayBoundCap : rays * per_ray;
    return by_rays < box ? by_rays : box;
}

// ---- a fused frame of sensor rays -----------------------------------------------------------------------------------
constexpr float kDshFuseLow = 0.001f, kDshFuseHigh = 0.999f;   // the domain of the sensor model's four numbers
constexpr uint8_t kDshMarkMiss = 1, kDshMarkHit = 2;           // a cell's byte in the mark plane while a frame is in flight (else 0)

// prob_hit, prob_miss, clamp_min and clamp_max all lie in [0.001, 0.999] and clamp_min <= clamp_max (a NaN fails every comparison)
SDFGPU_DSH_HD bool dsh_fuse_model_ok(float prob_hit, float prob_miss, float clamp_min, float clamp_max) {
    const float v[4] = {prob_hit, prob_miss, clamp_min, clamp_max};
    for (int k = 0; k < 4; ++k)
        if (!(v[k] >= kDshFuseLow && v[k] <= kDshFuseHigh)) return false;
    return clamp_min <= clamp_max;
}

// One measurement m (prob_hit or prob_miss; one_minus_m = 1.0f - m, worked out once on the host) folded into the occupancy p: Bayes'
// rule on the clamped prior, clamped again.  IEEE float32, every operation rounded by itself (nothing contracted: the pragma for
// clang, -ffp-contract=off for the CPU harness), the division correctly rounded.  Inside the model's domain no operand is denormal
// and a + b > 0.  A NaN prior becomes clamp_min.
SDFGPU_DSH_HD float dsh_fuse_update(float p, float m, float one_minus_m, float clamp_min, float clamp_max) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float q = p >= clamp_min ? p : clamp_min;
    q = q <= clamp_max ? q : clamp_max;
    const float a = q * m;
    const float b = (1.0f - q) * one_minus_m;
    float r = a / (a + b);
    r = r >= clamp_min ? r : clamp_min;
    r = r <= clamp_max ? r : clamp_max;
    return r;
}

// The mark plane of a fused map: one byte per cell of the pool's capacity, indexed like the cells.  64-bit: a pool of 2^17 chunks of
// 32768 cells has 2^32 of them.
inline uint64_t dsh_mark_bytes(uint64_t pool_chunks, uint64_t cells_per_chunk) { return pool_chunks * cells_per_chunk; }
SDFGPU_DSH_HD uint64_t dsh_mark_offset(uint64_t slot, uint64_t cells_per_chunk, uint32_t cell) { return slot * cells_per_chunk + (uint64_t)cell; }

// what k_dsh_ray_fuse is told about the model
struct DshFuse {
    float hit, one_minus_hit, miss, one_minus_miss, clamp_min, clamp_max;
};

// ---- what the kernels are told ----------------------------------------------------------------------------------------------------------
struct DshGeometry {
    double inverse[12];         // rows 0 - 2 of the inverse origin transform, row-major
    double inv_cell;            // 1 / cell_size
    int64_t n[3];               // chunk dimensions in cells
    int64_t cells_per_chunk;
    uint64_t default_record;
};

struct DshTable {
    uint64_t* keys;             // [capacity] kDshEmptyKey or a key
    uint32_t* slots;            // [capacity] the pool slot of the key at the same position
    uint64_t mask;              // capacity - 1
};

struct DshPool {
    DshChunkHead* heads;        // [capacity in chunks]
    uint64_t* cells;            // [capacity in chunks][cells_per_chunk]
};

// A frame of sensor rays: what the host worked out about the sensor, once for all rays.
struct DshRayFrame {
    double gs[3];               // the sensor in grid coordinates (cells, before the floor)
    int64_t i0[3];              // floor(gs): the sensor's global cell
    int64_t c0[3];              // its chunk
    int64_t l0[3];              // its cell inside the chunk
    double range2;              // R * R, R in cells
    uint64_t range_cells;       // ceil(R)
    uint64_t max_steps;         // dsh_ray_max_steps
};

constexpr int kDshThreads = 256;
constexpr int64_t kDshGridX = 1 << 20;    // workgroups per grid row (a launch dimension takes fewer than 2^32 threads)

}  // namespace sdfgpu
