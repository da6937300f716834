// sdfgpu_dsh.hip -- the chunk-hashed sparse collision map (sdfgpu_dsh.hpp, include/sdfgpu.h "Dynamic spatial hashed map", DESIGN.md
// sections 29 to 33): its kernels, the host orchestration of a batch, of a frame of sensor rays (carved or fused), of a removal and of a
// ray cast, growth and shrinking, and the C ABI entry points sdfgpu_dsh_*.  Compiled beside
// sdfgpu.hip and linked into the same libsdfgpu.so (sdf_tools_amd/build.py).
//
// How the kernels of one call talk to each other: through kernel boundaries, and inside a launch through atomics only.
//   - the table's keys are claimed by 64-bit compare-and-swap and looked at, inside the inserting launch, by atomic loads; every other
//     word a kernel reads was written by an EARLIER launch (or by the reading thread itself)
//   - no kernel waits for another workgroup, and every probe loop ends after `capacity` steps
//   - the order rule of a batch with one value per operation is a winner stamp by 64-bit atomic max (operation index + 1) that lives,
//     between two launches, in the 8 bytes it is about to overwrite: zero the targets | stamp | decide (one flag per operation) | apply
//   - a frame of sensor rays marks the chunks it writes into in a byte map by table position, and carves with one record: wherever
//     several threads of a launch store to one address, they store the same value
//   - a fused frame tells its cells to a mark plane the same way (one byte value per launch), and one workgroup per touched chunk then
//     updates each marked record once and clears its mark
//   - a ray cast reads only: one kernel, no scratch, and nothing another thread of the launch wrote
//   - a removal flags slots by a 32-bit atomic min of the operation index, and moves chunks from slots at or above `keep` into
//     flagged slots below it: the sources and the destinations of the one launch are disjoint
//
// Arithmetic: a location on a cell boundary is placed by the rounding of g = inverse_origin * p alone, and tests/dsh_restated.py states
// that product in numpy (separate products and sums), so nothing here may be contracted into an FMA (hipcc contracts by default).  The
// product, its floor and range check, and the split into chunk and cell are written once (dsh_axis_cell, dsh_split_cell,
// dsh_cell_index) for the lanes and for the host, which works a frame's sensor out with them: the host code below falls under the
// pragma too; it is compiled for baseline x86-64, which has no FMA to contract into.
#pragma clang fp contract(off)
#include "sdfgpu_context.hpp"
#include "sdfgpu_dsh.hpp"
#include "sdfgpu_unionfind.hpp"
#include "sdfgpu.h"

namespace sdfgpu {

namespace {

constexpr uint32_t kDshNoPos = 0xFFFFFFFFu;       // an operation at an invalid location

dim3 dsh_grid(int64_t items) {
    const int64_t workgroups = std::max<int64_t>(1, (items + kDshThreads - 1) / kDshThreads);
    if (workgroups <= kDshGridX) return dim3((unsigned)workgroups);
    return dim3((unsigned)kDshGridX, (unsigned)((workgroups + kDshGridX - 1) / kDshGridX));
}
__device__ __forceinline__ int64_t dsh_item() { return ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kDshThreads + threadIdx.x; }

// ---- the cell arithmetic, stated once for the device and the host ---------------------------------------------------------------------
// One axis of one point (x, y, z): `row` of the inverse origin transform gives the grid coordinate in cells `coord` (products and sums
// in exactly this order, then the scale), its floor the global cell; false where that is no cell of a chunk in [-2^20, 2^20).
__host__ __device__ __forceinline__ bool dsh_axis_cell(const double* row, double inv_cell, int64_t n_a, double x, double y, double z, double& coord,
                                                       int64_t& cell) {
    const double ga = ((row[0] * x + row[1] * y) + row[2] * z) + row[3];
    coord = ga * inv_cell;
    const double v = floor(coord);
    const double lim = (double)(kDshChunkBias * n_a);                          // exact: at most 2^35
    if (!(v >= -lim && v < lim)) return false;                                 // (NaN and the infinities fail: no cast of such a double)
    cell = (int64_t)v;
    return true;
}
// a global cell along one axis -> its chunk and the cell inside the chunk
__host__ __device__ __forceinline__ void dsh_split_cell(int64_t i, int64_t n_a, int64_t& chunk, int64_t& local) {
    chunk = dsh_floor_div(i, n_a);
    local = i - chunk * n_a;
}
// the cell slot of (l_x, l_y, l_z) in a chunk of n cells
__host__ __device__ __forceinline__ uint32_t dsh_cell_index(const int64_t l[3], const int64_t n[3]) { return (uint32_t)((l[0] * n[1] + l[1]) * n[2] + l[2]); }

// location -> (key, cell slot); false for an invalid location
__device__ __forceinline__ bool dsh_locate(const DshGeometry& g, double px, double py, double pz, uint64_t& key, uint32_t& cell) {
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return false;
    int64_t c[3], l[3];
    for (int a = 0; a < 3; ++a) {
        double coord;
        int64_t i;
        if (!dsh_axis_cell(g.inverse + 4 * a, g.inv_cell, g.n[a], px, py, pz, coord, i)) return false;
        dsh_split_cell(i, g.n[a], c[a], l[a]);
    }
    key = dsh_pack_key(c[0], c[1], c[2]);
    cell = dsh_cell_index(l, g.n);
    return true;
}

// whether a cell with this record stops a ray and counts as filled in a window (COLLISION_CELL: occupancy in the low word; a NaN
// fails both comparisons)
__device__ __forceinline__ bool dsh_record_blocks(uint64_t record, bool unknown_is_filled) {
    const float occ = __uint_as_float((uint32_t)record);
    return occ > 0.5f || (unknown_is_filled && occ == 0.5f);
}

// the position of `key` in a table no launch is inserting into, or kDshNoPos
__device__ __forceinline__ uint32_t dsh_find(const DshTable& t, uint64_t key) {
    uint64_t pos = dsh_hash(key) & t.mask;
    for (uint64_t probe = 0; probe <= t.mask; ++probe) {
        const uint64_t k = t.keys[pos];
        if (k == key) return (uint32_t)pos;
        if (k == kDshEmptyKey) return kDshNoPos;
        pos = (pos + 1) & t.mask;
    }
    return kDshNoPos;
}

// ---- a batch: insert keys ------------------------------------------------------------------------------------------------------------
// counters[0] = new chunks of this batch, counters[1] = operations that found no entry (cannot happen in a table sized for the batch),
// counters[2] = 1 once an operation of a batch named a valid location (every writer stores the same value)
// The position of `key` in a table this launch inserts into: the thread that makes the entry numbers the chunk and lists it.
__device__ __forceinline__ uint32_t dsh_claim(const DshTable& t, uint64_t key, uint32_t n_live, uint32_t* __restrict__ newlist, uint32_t* counters) {
    uint64_t pos = dsh_hash(key) & t.mask;
    unsigned long long* const keys = reinterpret_cast<unsigned long long*>(t.keys);
    for (uint64_t probe = 0; probe <= t.mask; ++probe) {
        unsigned long long k = __hip_atomic_load(keys + pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kDshEmptyKey) {
            k = atomicCAS(keys + pos, (unsigned long long)kDshEmptyKey, (unsigned long long)key);
            if (k == kDshEmptyKey) {                                         // this thread made the entry: it numbers the chunk
                const uint32_t fresh = atomicAdd(&counters[0], 1u);
                newlist[fresh] = (uint32_t)pos;
                t.slots[pos] = n_live + fresh;                               // (read by later launches only)
                k = key;
            }
        }
        if (k == key) return (uint32_t)pos;
        pos = (pos + 1) & t.mask;
    }
    atomicAdd(&counters[1], 1u);
    return kDshNoPos;
}

template <typename LOC>
__global__ __launch_bounds__(kDshThreads) void k_dsh_insert(const DshGeometry g, const DshTable t, const LOC* __restrict__ loc, int64_t n,
                                                            uint32_t n_live, uint32_t* __restrict__ op_pos, uint32_t* __restrict__ op_cell,
                                                            uint32_t* __restrict__ newlist, uint32_t* counters, uint8_t* __restrict__ statuses,
                                                            uint8_t set_status) {
    const int64_t i = dsh_item();
    if (i >= n) return;
    uint64_t key = 0;
    uint32_t cell = 0, found = kDshNoPos;
    if (dsh_locate(g, (double)loc[3 * i], (double)loc[3 * i + 1], (double)loc[3 * i + 2], key, cell))
        found = dsh_claim(t, key, n_live, newlist, counters);
    op_pos[i] = found;
    op_cell[i] = cell;
    if (found != kDshNoPos) counters[2] = 1u;
    if (statuses) statuses[i] = found != kDshNoPos ? set_status : (uint8_t)SDFGPU_DSH_NOT_SET;
}

// a refused batch: the entries it made become empty again.  Every other key sits where it sat before the batch (an insert moves
// nothing), so the table is exactly the one the batch found.
__global__ __launch_bounds__(kDshThreads) void k_dsh_rollback(const DshTable t, const uint32_t* __restrict__ newlist, uint32_t n_new) {
    const int64_t i = dsh_item();
    if (i < n_new) t.keys[newlist[i]] = kDshEmptyKey;
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_init_new(const DshTable t, DshChunkHead* __restrict__ heads,
                                                              const uint32_t* __restrict__ newlist, uint32_t n_new, uint32_t n_live) {
    const int64_t i = dsh_item();
    if (i >= n_new) return;
    DshChunkHead hd;
    hd.key = t.keys[newlist[i]];
    hd.record = 0; hd.state = 0; hd.reserved = 0;
    heads[n_live + i] = hd;
}

// the table after it grew: every live chunk's key goes into the new (empty) table
__global__ __launch_bounds__(kDshThreads) void k_dsh_rehash(const DshTable t, const DshChunkHead* __restrict__ heads, uint32_t n_live,
                                                            uint32_t* counters) {
    const int64_t s = dsh_item();
    if (s >= n_live) return;
    const uint64_t key = heads[s].key;
    uint64_t pos = dsh_hash(key) & t.mask;
    unsigned long long* const keys = reinterpret_cast<unsigned long long*>(t.keys);
    for (uint64_t probe = 0; probe <= t.mask; ++probe) {
        if (atomicCAS(keys + pos, (unsigned long long)kDshEmptyKey, (unsigned long long)key) == kDshEmptyKey) {
            t.slots[pos] = (uint32_t)s;
            return;
        }
        pos = (pos + 1) & t.mask;
    }
    atomicAdd(&counters[1], 1u);
}

// ---- a batch of cell sets: which chunks must hold cells ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kDshThreads) void k_dsh_touch(const DshTable t, DshChunkHead* heads, const uint32_t* __restrict__ op_pos, int64_t n) {
    const int64_t i = dsh_item();
    const uint32_t pos = i < n ? op_pos[i] : kDshNoPos;
    // neighbouring operations mostly share a chunk: a lane whose predecessor in the wave names the same entry leaves the flag to it
    const uint32_t before = (uint32_t)__shfl_up((int)pos, 1);
    if (pos != kDshNoPos && ((threadIdx.x & 63) == 0 || before != pos)) atomicOr(&heads[t.slots[pos]].state, kDshTouched);
}

// one workgroup per chunk: a touched chunk that holds no cells yet gets them (the default, or the chunk's record in every cell)
__global__ __launch_bounds__(kDshThreads) void k_dsh_expand(const DshPool p, uint64_t n_live, uint64_t cells_per_chunk, uint64_t default_record) {
    const uint64_t slot = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (slot >= n_live) return;                                                // (the last row of a two-dimensional launch)
    DshChunkHead* const hd = p.heads + slot;
    const uint32_t state = hd->state;
    if (!(state & kDshTouched)) return;                                        // (uniform over the workgroup)
    if ((state & kDshStateMask) != kDshCellFilled) {
        const uint64_t fill = (state & kDshStateMask) == kDshChunkFilled ? hd->record : default_record;
        uint64_t* const cells = p.cells + slot * cells_per_chunk;
        for (uint64_t k = threadIdx.x; k < cells_per_chunk; k += kDshThreads) cells[k] = fill;
    }
    __syncthreads();                                                           // every thread has read the state word
    if (threadIdx.x == 0) { hd->state = kDshCellFilled; hd->record = 0; }
}

// ---- a batch: write ------------------------------------------------------------------------------------------------------------------
// what operation i writes: a cell of its chunk, or (CHUNK) the chunk's record
template <bool CHUNK>
__device__ __forceinline__ uint64_t* dsh_target(const DshTable& t, const DshPool& p, uint64_t cells_per_chunk, uint32_t pos, uint32_t cell) {
    const uint64_t slot = t.slots[pos];
    return CHUNK ? &p.heads[slot].record : p.cells + slot * cells_per_chunk + cell;
}

// every valid operation stores `value` (the one-value batch, whose order cannot matter; and, with 0, the first step of the order rule)
template <bool CHUNK>
__global__ __launch_bounds__(kDshThreads) void k_dsh_store_one(const DshTable t, const DshPool p, uint64_t cells_per_chunk,
                                                               const uint32_t* __restrict__ op_pos, const uint32_t* __restrict__ op_cell,
                                                               int64_t n, uint64_t value) {
    const int64_t i = dsh_item();
    if (i >= n || op_pos[i] == kDshNoPos) return;
    *dsh_target<CHUNK>(t, p, cells_per_chunk, op_pos[i], op_cell[i]) = value;
    if (CHUNK) p.heads[t.slots[op_pos[i]]].state = kDshChunkFilled;
}

template <bool CHUNK>
__global__ __launch_bounds__(kDshThreads) void k_dsh_stamp(const DshTable t, const DshPool p, uint64_t cells_per_chunk,
                                                           const uint32_t* __restrict__ op_pos, const uint32_t* __restrict__ op_cell, int64_t n) {
    const int64_t i = dsh_item();
    if (i >= n || op_pos[i] == kDshNoPos) return;
    atomicMax(reinterpret_cast<unsigned long long*>(dsh_target<CHUNK>(t, p, cells_per_chunk, op_pos[i], op_cell[i])), (unsigned long long)(i + 1));
}

template <bool CHUNK>
__global__ __launch_bounds__(kDshThreads) void k_dsh_decide(const DshTable t, const DshPool p, uint64_t cells_per_chunk,
                                                            const uint32_t* __restrict__ op_pos, const uint32_t* __restrict__ op_cell, int64_t n,
                                                            uint8_t* __restrict__ wins) {
    const int64_t i = dsh_item();
    if (i >= n) return;
    wins[i] = op_pos[i] != kDshNoPos && *dsh_target<CHUNK>(t, p, cells_per_chunk, op_pos[i], op_cell[i]) == (uint64_t)(i + 1);
}

template <bool CHUNK>
__global__ __launch_bounds__(kDshThreads) void k_dsh_apply(const DshTable t, const DshPool p, uint64_t cells_per_chunk,
                                                           const uint32_t* __restrict__ op_pos, const uint32_t* __restrict__ op_cell, int64_t n,
                                                           const uint8_t* __restrict__ wins, const uint64_t* __restrict__ values) {
    const int64_t i = dsh_item();
    if (i >= n || !wins[i]) return;
    *dsh_target<CHUNK>(t, p, cells_per_chunk, op_pos[i], op_cell[i]) = values[i];
}

// ---- reads ---------------------------------------------------------------------------------------------------------------------------
// what Get returns for (key, cell) of a valid location
__device__ __forceinline__ uint32_t dsh_read(const DshTable& t, const DshPool& p, uint64_t cells_per_chunk, uint64_t key, uint32_t cell,
                                             uint64_t& record) {
    const uint32_t pos = dsh_find(t, key);
    if (pos == kDshNoPos) return SDFGPU_DSH_NOT_FOUND;
    const uint64_t slot = t.slots[pos];
    const uint32_t state = p.heads[slot].state & kDshStateMask;
    if (state == kDshChunkFilled) record = p.heads[slot].record;
    else if (state == kDshCellFilled) record = p.cells[slot * cells_per_chunk + cell];
    return state;
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_get(const DshGeometry g, const DshTable t, const DshPool p, const double* __restrict__ loc,
                                                         int64_t n, uint64_t* __restrict__ records, uint8_t* __restrict__ statuses) {
    const int64_t i = dsh_item();
    if (i >= n) return;
    uint64_t key = 0, record = g.default_record;
    uint32_t cell = 0, status = SDFGPU_DSH_NOT_FOUND;
    if (dsh_locate(g, loc[3 * i], loc[3 * i + 1], loc[3 * i + 2], key, cell)) status = dsh_read(t, p, (uint64_t)g.cells_per_chunk, key, cell, record);
    if (records) records[i] = record;
    if (statuses) statuses[i] = (uint8_t)status;
}

struct DshWindow {
    int64_t lower[3];
    uint32_t ny, nz;
    uint64_t n;             // voxels (< 2^32)
    int unknown_is_filled;
    uint64_t* records;      // either may be null
    uint32_t* bits;
};

// One thread per voxel, a wave per two bit words: the words' bits come out of a ballot, lanes 0 and 32 store them whole.
__global__ __launch_bounds__(kDshThreads) void k_dsh_window(const DshGeometry g, const DshTable t, const DshPool p, const DshWindow w) {
    const uint64_t v = (uint64_t)dsh_item();
    if (v - threadIdx.x >= w.n) return;                                        // (the last row of a two-dimensional launch)
    bool filled = false;
    if (v < w.n) {
        const uint32_t u = (uint32_t)v, q = u / w.nz;
        const uint32_t z = u - q * w.nz, x = q / w.ny, y = q - x * w.ny;
        const int64_t i[3] = {w.lower[0] + (int64_t)x, w.lower[1] + (int64_t)y, w.lower[2] + (int64_t)z};
        int64_t c[3], l[3];
        bool valid = true;
        for (int a = 0; a < 3; ++a) {
            dsh_split_cell(i[a], g.n[a], c[a], l[a]);
            valid = valid && dsh_chunk_in_range(c[a]);
        }
        uint64_t record = g.default_record;
        if (valid) (void)dsh_read(t, p, (uint64_t)g.cells_per_chunk, dsh_pack_key(c[0], c[1], c[2]), dsh_cell_index(l, g.n), record);
        if (w.records) w.records[v] = record;
        filled = dsh_record_blocks(record, w.unknown_is_filled != 0);
    }
    if (w.bits) {                                                             // (uniform)
        const unsigned long long b = __ballot(filled);
        const int lane = threadIdx.x & 63;
        if (v < w.n && (lane == 0 || lane == 32)) w.bits[v >> 5] = (uint32_t)(b >> lane);
    }
}

// ---- export and counts -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDshThreads) void k_dsh_count(const DshChunkHead* __restrict__ heads, uint32_t n_live, unsigned long long* counts) {
    const int64_t s = dsh_item();
    const uint32_t state = s < n_live ? heads[s].state & kDshStateMask : 0;
    const unsigned long long chunk = __ballot(state == kDshChunkFilled), cell = __ballot(state == kDshCellFilled);
    if ((threadIdx.x & 63) == 0) {
        if (chunk) atomicAdd(&counts[0], (unsigned long long)__popcll(chunk));
        if (cell) atomicAdd(&counts[1], (unsigned long long)__popcll(cell));
    }
}

// A chunk's place in the export is the number of live keys below its own, and its cells start behind those of the cell-filled chunks
// among them: every thread counts over all chunks, a tile of kDshThreads heads at a time through LDS.  Quadratic in the number of
// chunks and free of scratch, atomics and order effects; the export feeds a display or a test, not a frame.
__global__ __launch_bounds__(kDshThreads) void k_dsh_rank(const DshChunkHead* __restrict__ heads, uint32_t n_live, uint64_t cells_per_chunk,
                                                          sdfgpu_dsh_chunk* __restrict__ out, uint32_t* __restrict__ slot_of_rank) {
    __shared__ uint64_t tile_key[kDshThreads];
    __shared__ uint32_t tile_cell[kDshThreads];
    const int64_t s = dsh_item();
    const bool live = s < n_live;
    const DshChunkHead mine = live ? heads[s] : DshChunkHead{kDshEmptyKey, 0, 0, 0};
    uint32_t below = 0, cells_below = 0;
    for (uint32_t base = 0; base < n_live; base += kDshThreads) {
        const uint32_t j = base + threadIdx.x;
        tile_key[threadIdx.x] = j < n_live ? heads[j].key : kDshEmptyKey;      // (no key is above the empty key's value)
        tile_cell[threadIdx.x] = j < n_live && (heads[j].state & kDshStateMask) == kDshCellFilled;
        __syncthreads();
        for (int k = 0; k < kDshThreads; ++k) {
            const uint32_t lt = tile_key[k] < mine.key;
            below += lt;
            cells_below += lt & tile_cell[k];
        }
        __syncthreads();
    }
    if (!live) return;
    sdfgpu_dsh_chunk c;
    dsh_unpack_key(mine.key, c.c[0], c.c[1], c.c[2]);
    c.state = mine.state & kDshStateMask;
    c.reserved = 0;
    c.record = c.state == kDshChunkFilled ? mine.record : 0;
    c.first_cell = c.state == kDshCellFilled ? (int64_t)((uint64_t)cells_below * cells_per_chunk) : -1;
    out[below] = c;
    slot_of_rank[below] = (uint32_t)s;
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_export_cells(const DshPool p, uint64_t n_live, uint64_t cells_per_chunk,
                                                                  const sdfgpu_dsh_chunk* __restrict__ chunks, const uint32_t* __restrict__ slot_of_rank,
                                                                  uint64_t* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (r >= n_live) return;
    const int64_t first = chunks[r].first_cell;
    if (first < 0) return;
    const uint64_t* const cells = p.cells + (uint64_t)slot_of_rank[r] * cells_per_chunk;
    for (uint64_t k = threadIdx.x; k < cells_per_chunk; k += kDshThreads) out[(uint64_t)first + k] = cells[k];
}

// ---- a frame of sensor rays (include/sdfgpu.h "Sensor rays") ---------------------------------------------------------
// One lane per ray.  A ray's walk is stated once (dsh_ray_begin, dsh_ray_step, dsh_ray_walk) and run twice: k_dsh_ray_insert claims
// the key of every chunk the walk writes into, k_dsh_ray_carve repeats it and stores.  Nothing is kept per cell between the two.
// Every array below is indexed by unrolled constants only (a == axis), so the walk's state stays in registers.
struct DshRayWalk {
    double gs[3], d[3];         // the sensor and end - sensor, in cells
    double t[3];                // the parameter at which the ray crosses into the next cell along each axis (+inf: no step left)
    double bound[3];            // that crossing's coordinate: the next cell boundary along the axis
    double len2;
    int64_t rem[3];             // steps left along each axis
    int64_t c[3];               // the current cell: chunk, and cell inside the chunk
    int32_t l[3];
    int32_t sg[3];
    bool is_long;
};

// Where a ray starts: its grid coordinates, their floors, and the floors' chunk and cell inside the chunk.  A frame's rays share the
// host's (dsh_ray_frame); a cast segment works its own out in the lane (dsh_ray_start).
struct DshRayStart {
    double gs[3];
    int64_t i0[3], c0[3], l0[3];
};

// SDFGPU_DSH_RAY_SKIPPED for a point that is no valid location; else _HIT or _TRUNCATED, and the walk stands on the start's cell
template <class Start>
__device__ __forceinline__ uint32_t dsh_ray_begin(const DshGeometry& g, const Start& f, double range2, double px, double py, double pz, DshRayWalk& w) {
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return SDFGPU_DSH_RAY_SKIPPED;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double ge;
        int64_t i1;
        if (!dsh_axis_cell(g.inverse + 4 * a, g.inv_cell, g.n[a], px, py, pz, ge, i1)) return SDFGPU_DSH_RAY_SKIPPED;
        const int64_t diff = i1 - f.i0[a];
        w.sg[a] = diff > 0 ? 1 : diff < 0 ? -1 : 0;
        w.rem[a] = diff < 0 ? -diff : diff;
        w.gs[a] = f.gs[a];
        w.d[a] = ge - f.gs[a];
        w.bound[a] = (double)(f.i0[a] + (diff > 0 ? 1 : 0));                   // exact: below 2^36
        w.t[a] = diff != 0 ? (w.bound[a] - w.gs[a]) / w.d[a] : INFINITY;       // (the floors differ, so d is not 0)
        w.c[a] = f.c0[a];
        w.l[a] = (int32_t)f.l0[a];
    }
    w.len2 = (w.d[0] * w.d[0] + w.d[1] * w.d[1]) + w.d[2] * w.d[2];
    w.is_long = w.len2 > range2;
    return w.is_long ? SDFGPU_DSH_RAY_TRUNCATED : SDFGPU_DSH_RAY_HIT;
}
__device__ __forceinline__ uint32_t dsh_ray_begin(const DshGeometry& g, const DshRayFrame& f, double px, double py, double pz, DshRayWalk& w) {
    return dsh_ray_begin(g, f, f.range2, px, py, pz, w);
}

// Where a ray starts, worked out from a finite point: by the host for a frame's sensor (dsh_ray_frame), in the lane for a segment
// (dsh_ray_start).  False where the point is no valid location.
template <class Start>
__host__ __device__ __forceinline__ bool dsh_start_cell(const DshGeometry& g, double sx, double sy, double sz, Start& s) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!dsh_axis_cell(g.inverse + 4 * a, g.inv_cell, g.n[a], sx, sy, sz, s.gs[a], s.i0[a])) return false;
        dsh_split_cell(s.i0[a], g.n[a], s.c0[a], s.l0[a]);
    }
    return true;
}
__device__ __forceinline__ bool dsh_ray_start(const DshGeometry& g, double sx, double sy, double sz, DshRayStart& s) {
    return isfinite(sx) && isfinite(sy) && isfinite(sz) && dsh_start_cell(g, sx, sy, sz, s);
}

// One step: along the axis with the smallest crossing parameter, x before y before z.  Returns that parameter, the entry parameter
// of the cell the walk now stands on; `chunk_changed` says whether that cell lies in another chunk.
__device__ __forceinline__ double dsh_ray_step(const DshGeometry& g, DshRayWalk& w, bool& chunk_changed) {
    int axis = 0;
    double tk = w.t[0];
    if (w.t[1] < tk) { axis = 1; tk = w.t[1]; }
    if (w.t[2] < tk) { axis = 2; tk = w.t[2]; }
    chunk_changed = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (a != axis) continue;
        w.bound[a] += (double)w.sg[a];
        w.rem[a] -= 1;
        w.t[a] = w.rem[a] != 0 ? (w.bound[a] - w.gs[a]) / w.d[a] : INFINITY;
        w.l[a] += w.sg[a];
        if (w.l[a] < 0) { w.l[a] = (int32_t)g.n[a] - 1; w.c[a] -= 1; chunk_changed = true; }
        else if (w.l[a] >= (int32_t)g.n[a]) { w.l[a] = 0; w.c[a] += 1; chunk_changed = true; }
    }
    return tk;
}

__device__ __forceinline__ uint32_t dsh_ray_cell(const DshGeometry& g, const DshRayWalk& w) {
    return (uint32_t)((w.l[0] * (int32_t)g.n[1] + w.l[1]) * (int32_t)g.n[2] + w.l[2]);
}

// The cells a ray writes, in walk order: cell(chunk_changed, is_hit) for each.  A ray that is not long carves c_0 .. c_(N-1) and
// hits c_N; a long one carves the prefix of c_0 .. c_N whose entry parameters are in range.  Returns how many cells it carved.
// The loop ends with the steps left (rem) or the range; max_steps is a guard that neither can pass.
template <class Cell>
__device__ __forceinline__ uint32_t dsh_ray_walk(const DshGeometry& g, const DshRayFrame& f, DshRayWalk& w, Cell&& cell) {
    uint32_t carved = 0;
    bool chunk_changed = true;                                                // (the first cell: its chunk has not been looked up)
    for (uint64_t step = 0; step <= f.max_steps; ++step) {
        const bool last = (w.rem[0] | w.rem[1] | w.rem[2]) == 0;
        if (last && !w.is_long) { cell(chunk_changed, true); break; }
        cell(chunk_changed, false);
        ++carved;
        if (last) break;
        const double tk = dsh_ray_step(g, w, chunk_changed);
        if (w.is_long && !((tk * tk) * w.len2 <= f.range2)) break;
    }
    return carved;
}

// counters: [0] new chunks, [1] lost operations (uint32); from byte 8 on, four uint64: rays hit, truncated, skipped, cells carved
constexpr int kDshRayCounts = 4;

__device__ __forceinline__ uint32_t dsh_wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_down((int)v, off);
    return v;                                                                 // (lane 0 holds the sum)
}

// The chunks the frame's rays can enter, summed over the rays (dsh_ray_chunks: arithmetic on a ray's two ends, no walk) into the
// uint64 at byte 8 of the counters.  Run only where the bound that needs no ray would make the table grow.
__global__ __launch_bounds__(kDshThreads) void k_dsh_ray_count(const DshGeometry g, const DshRayFrame f, const float* __restrict__ points, int64_t n,
                                                               uint32_t* counters) {
    const int64_t i = dsh_item();
    uint32_t chunks = 0;
    if (i < n) {
        DshRayWalk w;
        if (dsh_ray_begin(g, f, (double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2], w) != SDFGPU_DSH_RAY_SKIPPED) {
            const int64_t i1[3] = {f.i0[0] + w.sg[0] * w.rem[0], f.i0[1] + w.sg[1] * w.rem[1], f.i0[2] + w.sg[2] * w.rem[2]};
            chunks = (uint32_t)dsh_ray_chunks(f.i0, i1, g.n, w.is_long, f.range_cells);      // at most 1 + 3 * 2^21
        }
    }
    const uint32_t sum = dsh_wave_sum(chunks);                               // at most 64 * (1 + 3 * 2^21): fits
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(reinterpret_cast<unsigned long long*>(counters + 2), (unsigned long long)sum);
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_ray_insert(const DshGeometry g, const DshTable t, const DshRayFrame f,
                                                                const float* __restrict__ points, int64_t n, uint32_t n_live,
                                                                uint32_t* __restrict__ op_pos, uint32_t* __restrict__ op_cell,
                                                                uint32_t* __restrict__ newlist, uint8_t* __restrict__ marks, uint32_t* counters,
                                                                uint8_t* __restrict__ statuses) {
    const int64_t i = dsh_item();
    uint32_t status = SDFGPU_DSH_RAY_SKIPPED, carved = 0;
    if (i < n) {
        DshRayWalk w;
        uint32_t pos = kDshNoPos, hit_pos = kDshNoPos, hit_cell = 0;
        status = dsh_ray_begin(g, f, (double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2], w);
        if (status != SDFGPU_DSH_RAY_SKIPPED)
            carved = dsh_ray_walk(g, f, w, [&](bool chunk_changed, bool is_hit) {
                if (chunk_changed) {
                    pos = dsh_claim(t, dsh_pack_key(w.c[0], w.c[1], w.c[2]), n_live, newlist, counters);
                    if (pos != kDshNoPos) marks[pos] = 1;                      // (every writer stores the same byte)
                }
                if (is_hit) { hit_pos = pos; hit_cell = dsh_ray_cell(g, w); }
            });
        op_pos[i] = hit_pos;
        op_cell[i] = hit_cell;
        if (statuses) statuses[i] = (uint8_t)status;
    }
    // the frame's counts: one atomic per wave and count (lanes behind the last ray count as nothing)
    const bool live = i < n;
    const unsigned long long hit = __ballot(live && status == SDFGPU_DSH_RAY_HIT), cut = __ballot(live && status == SDFGPU_DSH_RAY_TRUNCATED),
                             skipped = __ballot(live && status == SDFGPU_DSH_RAY_SKIPPED);
    const uint32_t sum = dsh_wave_sum(carved);                               // at most 64 * (3 * 65538 + 3): fits
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* const counts = reinterpret_cast<unsigned long long*>(counters + 2);
        if (hit) atomicAdd(&counts[0], (unsigned long long)__popcll(hit));
        if (cut) atomicAdd(&counts[1], (unsigned long long)__popcll(cut));
        if (skipped) atomicAdd(&counts[2], (unsigned long long)__popcll(skipped));
        if (sum) atomicAdd(&counts[3], (unsigned long long)sum);
    }
}

// the chunks the frame writes into, by table position -> the touched flag k_dsh_expand reads (one thread per position)
__global__ __launch_bounds__(kDshThreads) void k_dsh_ray_touch(const DshTable t, DshChunkHead* heads, const uint8_t* __restrict__ marks) {
    const uint64_t pos = (uint64_t)dsh_item();
    if (pos <= t.mask && marks[pos]) heads[t.slots[pos]].state |= kDshTouched;
}

// the walk again: every carved cell gets `free_value`.  All writers store the same record, so their order cannot matter; the hits
// follow behind a kernel boundary (k_dsh_store_one).
__global__ __launch_bounds__(kDshThreads) void k_dsh_ray_carve(const DshGeometry g, const DshTable t, const DshPool p, const DshRayFrame f,
                                                               const float* __restrict__ points, int64_t n, uint64_t free_value) {
    const int64_t i = dsh_item();
    if (i >= n) return;
    DshRayWalk w;
    if (dsh_ray_begin(g, f, (double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2], w) == SDFGPU_DSH_RAY_SKIPPED) return;
    uint64_t* cells = nullptr;
    (void)dsh_ray_walk(g, f, w, [&](bool chunk_changed, bool is_hit) {
        if (chunk_changed) {
            const uint32_t pos = dsh_find(t, dsh_pack_key(w.c[0], w.c[1], w.c[2]));
            cells = pos != kDshNoPos ? p.cells + (uint64_t)t.slots[pos] * (uint64_t)g.cells_per_chunk : nullptr;
        }
        if (!is_hit && cells) cells[dsh_ray_cell(g, w)] = free_value;
    });
}

// ---- a fused frame (include/sdfgpu.h "Sensor rays: fusion") ------------------------------------------------------------
// Behind walk A the frame is told to the mark plane, one byte per cell, and then folded into the records chunk by chunk, so that a
// cell is updated once however many rays cross it: walk B stores kDshMarkMiss for every carved cell (all writers store the same
// byte), the hits store kDshMarkHit behind a kernel boundary (a hit beats a miss by launch order), and k_dsh_ray_fuse reads each
// touched chunk's marks, updates the marked records and clears the marks.  No atomics, and nothing depends on the order of lanes.
__global__ __launch_bounds__(kDshThreads) void k_dsh_ray_mark(const DshGeometry g, const DshTable t, uint8_t* __restrict__ plane, const DshRayFrame f,
                                                              const float* __restrict__ points, int64_t n) {
    const int64_t i = dsh_item();
    if (i >= n) return;
    DshRayWalk w;
    if (dsh_ray_begin(g, f, (double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2], w) == SDFGPU_DSH_RAY_SKIPPED) return;
    uint8_t* marks = nullptr;
    (void)dsh_ray_walk(g, f, w, [&](bool chunk_changed, bool is_hit) {
        if (chunk_changed) {
            const uint32_t pos = dsh_find(t, dsh_pack_key(w.c[0], w.c[1], w.c[2]));
            marks = pos != kDshNoPos ? plane + dsh_mark_offset(t.slots[pos], (uint64_t)g.cells_per_chunk, 0) : nullptr;
        }
        if (!is_hit && marks) marks[dsh_ray_cell(g, w)] = kDshMarkMiss;
    });
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_ray_mark_hits(const DshTable t, uint8_t* __restrict__ plane, uint64_t cells_per_chunk,
                                                                   const uint32_t* __restrict__ op_pos, const uint32_t* __restrict__ op_cell, int64_t n) {
    const int64_t i = dsh_item();
    if (i >= n || op_pos[i] == kDshNoPos) return;
    plane[dsh_mark_offset(t.slots[op_pos[i]], cells_per_chunk, op_cell[i])] = kDshMarkHit;
}

__device__ __forceinline__ void dsh_fuse_cell(uint64_t* cell, uint32_t mark, const DshFuse& u) {
    uint32_t* const occupancy = reinterpret_cast<uint32_t*>(cell);            // COLLISION_CELL: occupancy in the low word; the component stays
    const bool hit = mark == kDshMarkHit;
    *occupancy = __float_as_uint(dsh_fuse_update(__uint_as_float(*occupancy), hit ? u.hit : u.miss, hit ? u.one_minus_hit : u.one_minus_miss,
                                                 u.clamp_min, u.clamp_max));
}

// One workgroup per chunk; the chunks the frame touched carry kDshTouched again (k_dsh_ray_touch a second time: k_dsh_expand consumed
// the first).  The chunk's marks go through LDS (dsh_fuse_lds_bytes per workgroup), so that both sides are coalesced: a lane loads 16
// marks in one load where the chunk's marks are 16-byte aligned (cells_per_chunk a multiple of 16: the plane's base is), else the
// lanes take a byte each; whoever loaded a mark clears it.  Then the lanes sweep the cells in lane order, and a marked record's
// occupancy word is loaded, updated and stored beside its neighbours'.
__global__ __launch_bounds__(kDshThreads) void k_dsh_ray_fuse(const DshPool p, uint8_t* __restrict__ plane, uint64_t n_live, uint32_t cells_per_chunk,
                                                              const DshFuse u) {
    extern __shared__ uint4 staged_vectors[];                                  // ceil(cells_per_chunk / 16) of them
    const uint64_t slot = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (slot >= n_live) return;                                                // (the last row of a two-dimensional launch)
    DshChunkHead* const hd = p.heads + slot;
    const uint32_t state = hd->state;
    if (!(state & kDshTouched)) return;                                        // (uniform over the workgroup)
    uint64_t* const cells = p.cells + slot * (uint64_t)cells_per_chunk;
    uint8_t* const marks = plane + dsh_mark_offset(slot, cells_per_chunk, 0);
    uint8_t* const staged = reinterpret_cast<uint8_t*>(staged_vectors);
    if ((cells_per_chunk & 15u) == 0) {
        for (uint32_t k = threadIdx.x * 16u; k < cells_per_chunk; k += kDshThreads * 16u) {
            const uint4 v = *reinterpret_cast<const uint4*>(marks + k);
            staged_vectors[k >> 4] = v;
            if ((v.x | v.y | v.z | v.w) != 0) *reinterpret_cast<uint4*>(marks + k) = make_uint4(0, 0, 0, 0);
        }
    } else {
        for (uint32_t k = threadIdx.x; k < cells_per_chunk; k += kDshThreads) {
            const uint8_t mark = marks[k];
            staged[k] = mark;
            if (mark) marks[k] = 0;
        }
    }
    __syncthreads();                                                           // the marks are staged, and every thread has read the state word
    if (threadIdx.x == 0) hd->state = state & ~kDshTouched;
    for (uint32_t k = threadIdx.x; k < cells_per_chunk; k += kDshThreads) {
        const uint32_t mark = staged[k];
        if (mark) dsh_fuse_cell(cells + k, mark, u);
    }
}

// ---- ray casts (include/sdfgpu.h "Ray casts") ------------------------------------------------------------------------------
// One lane per ray, read-only: the walk of a frame (dsh_ray_begin, dsh_ray_step), stopped at the first tested cell whose record
// satisfies the window predicate.  A chunk is looked up once, when the walk enters it; an absent or chunk-filled one is decided there
// and then stepped through without a memory access, a cell-filled one costs one 8-byte load per tested cell.  No atomics, no LDS.
template <bool SEGMENTS>
__global__ __launch_bounds__(kDshThreads) void k_dsh_cast(const DshGeometry g, const DshTable t, const DshPool p, const DshRayFrame f,
                                                          const float* __restrict__ points, const double* __restrict__ starts,
                                                          const double* __restrict__ ends, int64_t n, uint32_t flags,
                                                          uint8_t* __restrict__ statuses, sdfgpu_dsh_cast_hit* __restrict__ hits) {
    const int64_t i = dsh_item();
    if (i >= n) return;
    const bool skip_first = (flags & SDFGPU_DSH_CAST_SKIP_FIRST) != 0, skip_last = (flags & SDFGPU_DSH_CAST_SKIP_LAST) != 0;
    const bool unknown_is_filled = (flags & SDFGPU_DSH_CAST_UNKNOWN_IS_FILLED) != 0;
    DshRayWalk w;
    uint32_t status;
    if (SEGMENTS) {
        DshRayStart s;
        status = dsh_ray_start(g, starts[3 * i], starts[3 * i + 1], starts[3 * i + 2], s)
                     ? dsh_ray_begin(g, s, f.range2, ends[3 * i], ends[3 * i + 1], ends[3 * i + 2], w) : (uint32_t)SDFGPU_DSH_RAY_SKIPPED;
    } else {
        status = dsh_ray_begin(g, f, (double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2], w);
    }
    sdfgpu_dsh_cast_hit hit{};
    uint32_t out = SDFGPU_DSH_CAST_SKIPPED;
    if (status != SDFGPU_DSH_RAY_SKIPPED) {
        out = w.is_long ? SDFGPU_DSH_CAST_CLEAR_IN_RANGE : SDFGPU_DSH_CAST_CLEAR;
        const uint64_t* cells = nullptr;                                       // the current chunk's cells while it is cell-filled
        uint64_t record = g.default_record;                                    // the current cell's record where it was read or is uniform
        uint32_t found = SDFGPU_DSH_NOT_FOUND, k = 0;
        double tk = 0.0;
        bool chunk_changed = true, uniform_blocks = false, have_record = false;
        for (uint64_t step = 0; step <= f.max_steps; ++step) {
            const bool last = (w.rem[0] | w.rem[1] | w.rem[2]) == 0;
            if (chunk_changed) {
                const uint32_t pos = dsh_find(t, dsh_pack_key(w.c[0], w.c[1], w.c[2]));
                cells = nullptr;
                record = g.default_record;
                found = SDFGPU_DSH_NOT_FOUND;
                if (pos != kDshNoPos) {
                    const uint64_t slot = t.slots[pos];
                    found = p.heads[slot].state & kDshStateMask;
                    if (found == kDshCellFilled) cells = p.cells + slot * (uint64_t)g.cells_per_chunk;
                    else record = p.heads[slot].record;
                }
                uniform_blocks = !cells && dsh_record_blocks(record, unknown_is_filled);
            }
            have_record = !cells;
            if (!(skip_first && step == 0) && !(skip_last && last)) {
                bool blocks = uniform_blocks;
                if (cells) {
                    record = cells[dsh_ray_cell(g, w)];
                    have_record = true;
                    blocks = dsh_record_blocks(record, unknown_is_filled);
                }
                if (blocks) { out = SDFGPU_DSH_CAST_BLOCKED; break; }
            }
            if (last) break;
            if (w.is_long) {                                                   // the next cell's entry parameter: what dsh_ray_step is about to return
                double tn = w.t[0];
                if (w.t[1] < tn) tn = w.t[1];
                if (w.t[2] < tn) tn = w.t[2];
                if (!((tn * tn) * w.len2 <= f.range2)) break;                  // it is out of range: this cell is the last of W
            }
            tk = dsh_ray_step(g, w, chunk_changed);
            ++k;
        }
        if (hits) {
            if (!have_record) record = cells[dsh_ray_cell(g, w)];             // (an untested cell of a cell-filled chunk)
#pragma unroll
            for (int a = 0; a < 3; ++a) hit.cell[a] = w.c[a] * g.n[a] + (int64_t)w.l[a];
            hit.record = record;
            hit.t = tk;
            hit.step = k;
            hit.found = found;
        }
    }
    if (statuses) statuses[i] = (uint8_t)out;
    if (hits) hits[i] = hit;
}

// ---- removal (include/sdfgpu.h "Removal") --------------------------------------------------------------------------------
// One uint32 per live slot says whether the chunk goes: kDshKept, or the smallest index of an operation that names it (by box: 0).
// The pool keeps its invariant (slots 0 .. n_live - 1 in use) by hole filling: with `keep` survivors, the j-th flagged slot below
// `keep` takes the j-th unflagged slot at or above it.  Their ranks come out of a two-level scan of linear work over tiles of
// kDshPairTile slots (count per tile | one workgroup scans the tiles' counts | list), so the pairing depends on the flags alone.
__global__ __launch_bounds__(kDshThreads) void k_dsh_remove_stamp(const DshGeometry g, const DshTable t, const double* __restrict__ loc, int64_t n,
                                                                  uint32_t* flags, uint32_t* __restrict__ op_slot) {
    const int64_t i = dsh_item();
    if (i >= n) return;
    uint64_t key = 0;
    uint32_t cell = 0, slot = kDshNoPos;
    if (dsh_locate(g, loc[3 * i], loc[3 * i + 1], loc[3 * i + 2], key, cell)) {
        const uint32_t pos = dsh_find(t, key);
        if (pos != kDshNoPos) {
            slot = t.slots[pos];
            atomicMin(&flags[slot], (uint32_t)i);
        }
    }
    op_slot[i] = slot;
}

// (behind a kernel boundary) the first operation in list order that names a live chunk removed it
__global__ __launch_bounds__(kDshThreads) void k_dsh_remove_decide(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ op_slot, int64_t n,
                                                                   uint8_t* __restrict__ statuses) {
    const int64_t i = dsh_item();
    if (i >= n) return;
    const uint32_t slot = op_slot[i];
    statuses[i] = slot != kDshNoPos && flags[slot] == (uint32_t)i ? SDFGPU_DSH_CHUNK_REMOVED : SDFGPU_DSH_CHUNK_NOT_REMOVED;
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_remove_box(const DshChunkHead* __restrict__ heads, uint32_t n_live, const DshChunkRange range,
                                                                int invert, uint32_t* __restrict__ flags) {
    const int64_t s = dsh_item();
    if (s >= n_live) return;
    const bool in = dsh_key_in_range(heads[s].key, range);
    flags[s] = in == (invert != 0) ? 0u : kDshKept;
}

// counters[0] = flagged slots, one atomic per wave
__global__ __launch_bounds__(kDshThreads) void k_dsh_remove_count(const uint32_t* __restrict__ flags, uint32_t n_live, uint32_t* counters) {
    const int64_t s = dsh_item();
    const unsigned long long gone = __ballot(s < n_live && flags[s] != kDshKept);
    if ((threadIdx.x & 63) == 0 && gone) atomicAdd(&counters[0], (uint32_t)__popcll(gone));
}

// the holes (low 16 bits) and the movers (high 16 bits) among the thread's kDshPairItems slots from `first` on
__device__ __forceinline__ uint32_t dsh_pair_local(const uint32_t* __restrict__ flags, uint32_t n_live, uint32_t keep, uint32_t first) {
    uint32_t both = 0;
    for (uint32_t k = 0; k < kDshPairItems; ++k) {
        const uint32_t s = first + k;
        if (s >= n_live) break;
        const bool gone = flags[s] != kDshKept;
        both += (s < keep && gone ? 1u : 0u) + (s >= keep && !gone ? 0x10000u : 0u);
    }
    return both;
}

// exclusive prefix of v over the workgroup's threads and the workgroup's total (v's sums stay below 2^32)
__device__ __forceinline__ uint32_t dsh_block_exclusive(uint32_t v, uint32_t* wave_sum, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inclusive = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t other = (uint32_t)__shfl_up((int)inclusive, d);
        if (lane >= d) inclusive += other;
    }
    __syncthreads();                                                           // (wave_sum may still be read from an earlier call)
    if (lane == 63) wave_sum[wave] = inclusive;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    for (uint32_t w = 0; w < kDshThreads / 64; ++w) {
        if (w < wave) base += wave_sum[w];
        total += wave_sum[w];
    }
    return base + inclusive - v;
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_pair_count(const uint32_t* __restrict__ flags, uint32_t n_live, uint32_t keep,
                                                                uint32_t* __restrict__ tile_counts) {
    __shared__ uint32_t wave_sum[kDshThreads / 64];
    uint32_t total = 0;
    (void)dsh_block_exclusive(dsh_pair_local(flags, n_live, keep, blockIdx.x * kDshPairTile + threadIdx.x * kDshPairItems), wave_sum, total);
    if (threadIdx.x == 0) { tile_counts[2 * blockIdx.x] = total & 0xFFFFu; tile_counts[2 * blockIdx.x + 1] = total >> 16; }
}

// One workgroup: the tiles' counts become their exclusive prefixes, in place; counters[2] = the number of holes.
__global__ __launch_bounds__(kDshThreads) void k_dsh_pair_scan(uint32_t* __restrict__ tile_counts, uint32_t tiles, uint32_t* counters) {
    __shared__ uint32_t wave_sum[kDshThreads / 64];
    const uint32_t per = (tiles + kDshThreads - 1) / kDshThreads;
    const uint32_t begin = min(threadIdx.x * per, tiles), end = min(begin + per, tiles);
    uint32_t sum[2] = {0, 0};
    for (uint32_t k = begin; k < end; ++k) { sum[0] += tile_counts[2 * k]; sum[1] += tile_counts[2 * k + 1]; }
    uint32_t total = 0;
    uint32_t holes = dsh_block_exclusive(sum[0], wave_sum, total);
    if (threadIdx.x == 0) counters[2] = total;
    uint32_t movers = dsh_block_exclusive(sum[1], wave_sum, total);
    for (uint32_t k = begin; k < end; ++k) {
        const uint32_t h = tile_counts[2 * k], m = tile_counts[2 * k + 1];
        tile_counts[2 * k] = holes; tile_counts[2 * k + 1] = movers;
        holes += h; movers += m;
    }
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_pair_list(const uint32_t* __restrict__ flags, uint32_t n_live, uint32_t keep,
                                                               const uint32_t* __restrict__ tile_counts, uint32_t* __restrict__ holes,
                                                               uint32_t* __restrict__ movers) {
    __shared__ uint32_t wave_sum[kDshThreads / 64];
    const uint32_t first = blockIdx.x * kDshPairTile + threadIdx.x * kDshPairItems;
    uint32_t total = 0;
    const uint32_t before = dsh_block_exclusive(dsh_pair_local(flags, n_live, keep, first), wave_sum, total);
    uint32_t hole = tile_counts[2 * blockIdx.x] + (before & 0xFFFFu), mover = tile_counts[2 * blockIdx.x + 1] + (before >> 16);
    for (uint32_t k = 0; k < kDshPairItems; ++k) {
        const uint32_t s = first + k;
        if (s >= n_live) break;
        const bool gone = flags[s] != kDshKept;
        if (s < keep && gone) holes[hole++] = s;
        if (s >= keep && !gone) movers[mover++] = s;
    }
}

// One workgroup per pair: the mover's head, and its cells when it holds any, go into the hole.  Sources lie at or above `keep`,
// destinations below it: the moves of one launch are disjoint.  Two records per lane where the chunk's cells are 16-byte aligned
// (a slot's cells start at slot * cells_per_chunk * 8: an even cells_per_chunk).  The launch is sized by a bound on the pairs;
// counters[2] holds their number.
__global__ __launch_bounds__(kDshThreads) void k_dsh_remove_move(const DshPool p, uint64_t cells_per_chunk, const uint32_t* __restrict__ holes,
                                                                 const uint32_t* __restrict__ movers, const uint32_t* __restrict__ counters) {
    const uint64_t j = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (j >= counters[2]) return;
    const uint64_t src = movers[j], dst = holes[j];
    const DshChunkHead hd = p.heads[src];
    if (threadIdx.x == 0) p.heads[dst] = hd;
    if ((hd.state & kDshStateMask) != kDshCellFilled) return;                   // (uniform over the workgroup)
    const uint64_t* const from = p.cells + src * cells_per_chunk;
    uint64_t* const to = p.cells + dst * cells_per_chunk;
    if ((cells_per_chunk & 1) == 0) {
        const ulonglong2* const from2 = reinterpret_cast<const ulonglong2*>(from);
        ulonglong2* const to2 = reinterpret_cast<ulonglong2*>(to);
        for (uint64_t k = threadIdx.x; k < cells_per_chunk / 2; k += kDshThreads) to2[k] = from2[k];
    } else {
        for (uint64_t k = threadIdx.x; k < cells_per_chunk; k += kDshThreads) to[k] = from[k];
    }
}

// ---- frontier cells (include/sdfgpu.h "Frontier cells") ---------------------------------------------------------------
// A frontier cell is a free cell of a live chunk with an unknown neighbour.  The stencil is stated once (dsh_unknown_neighbour) and
// walks the neighbouring CHUNKS, not the neighbours: for each of the up to 27 chunk offsets it asks `lookup` once what that chunk
// shows, then reads the neighbours that lie there.  The window form answers a lookup with a dsh_find, the list form out of LDS.
// The loops index l[] and g.n[] by constants only: nothing is kept in scratch.
__device__ __forceinline__ bool dsh_record_free(uint64_t record) { return __uint_as_float((uint32_t)record) < 0.5f; }
__device__ __forceinline__ bool dsh_record_unknown(uint64_t record) { return __uint_as_float((uint32_t)record) == 0.5f; }

// What a chunk shows to a reader: its cells (cell-filled), else one record for every cell (the chunk's own when chunk-filled, the
// default when it is absent or its coordinate is out of range).
struct DshChunkView {
    const uint64_t* cells;
    uint64_t record;
};

__device__ __forceinline__ DshChunkView dsh_view_slot(const DshPool& p, uint64_t cells_per_chunk, uint64_t slot, uint64_t default_record) {
    const uint32_t state = p.heads[slot].state & kDshStateMask;
    DshChunkView v{nullptr, default_record};
    if (state == kDshChunkFilled) v.record = p.heads[slot].record;
    else if (state == kDshCellFilled) v.cells = p.cells + slot * cells_per_chunk;
    return v;
}

__device__ __forceinline__ DshChunkView dsh_view_chunk(const DshGeometry& g, const DshTable& t, const DshPool& p, int64_t cx, int64_t cy, int64_t cz) {
    if (!(dsh_chunk_in_range(cx) && dsh_chunk_in_range(cy) && dsh_chunk_in_range(cz))) return DshChunkView{nullptr, g.default_record};
    const uint32_t pos = dsh_find(t, dsh_pack_key(cx, cy, cz));
    if (pos == kDshNoPos) return DshChunkView{nullptr, g.default_record};
    return dsh_view_slot(p, (uint64_t)g.cells_per_chunk, t.slots[pos], g.default_record);
}

// whether a neighbour (6 face neighbours, or all 26) of the cell at l[] of a chunk is unknown; lookup(ox, oy, oz) -> DshChunkView of
// the chunk at that offset from the cell's own ((0, 0, 0) is its own chunk)
template <class Lookup>
__device__ __forceinline__ bool dsh_unknown_neighbour(const DshGeometry& g, const int64_t l[3], bool use_26, Lookup&& lookup) {
    for (int ox = -1; ox <= 1; ++ox) {
        int x0, x1;
        dsh_axis_steps(l[0], g.n[0], ox, x0, x1);
        if (x0 > x1) continue;
        for (int oy = -1; oy <= 1; ++oy) {
            int y0, y1;
            dsh_axis_steps(l[1], g.n[1], oy, y0, y1);
            if (y0 > y1) continue;
            for (int oz = -1; oz <= 1; ++oz) {
                int z0, z1;
                dsh_axis_steps(l[2], g.n[2], oz, z0, z1);
                if (z0 > z1) continue;
                if (!use_26 && (ox != 0) + (oy != 0) + (oz != 0) > 1) continue;       // a face neighbour crosses at most one chunk face
                const DshChunkView view = lookup(ox, oy, oz);
                if (!view.cells && !dsh_record_unknown(view.record)) continue;         // one record for all its cells, and not unknown
                for (int dx = x0; dx <= x1; ++dx)
                    for (int dy = y0; dy <= y1; ++dy)
                        for (int dz = z0; dz <= z1; ++dz) {
                            const int steps = (dx != 0) + (dy != 0) + (dz != 0);
                            if (steps == 0 || (!use_26 && steps != 1)) continue;
                            if (!view.cells) return true;
                            const int64_t m[3] = {l[0] + dx - ox * g.n[0], l[1] + dy - oy * g.n[1], l[2] + dz - oz * g.n[2]};
                            if (dsh_record_unknown(view.cells[dsh_cell_index(m, g.n)])) return true;
                        }
            }
        }
    }
    return false;
}

struct DshFrontierWindow {
    int64_t lower[3];
    uint32_t ny, nz;
    uint64_t n;             // voxels (< 2^32)
    uint32_t use_26;
    uint32_t* bits;
};

// k_dsh_window's shape: one thread per voxel, the words out of a ballot.  A lane decides its own cell first; only a free cell of a
// live chunk reads neighbours, those of its own chunk from the slot it has found.
__global__ __launch_bounds__(kDshThreads) void k_dsh_frontier_window(const DshGeometry g, const DshTable t, const DshPool p, const DshFrontierWindow w) {
    const uint64_t v = (uint64_t)dsh_item();
    if (v - threadIdx.x >= w.n) return;                                        // (the last row of a two-dimensional launch)
    bool frontier = false;
    if (v < w.n) {
        const uint32_t u = (uint32_t)v, q = u / w.nz;
        const uint32_t z = u - q * w.nz, x = q / w.ny, y = q - x * w.ny;
        const int64_t i[3] = {w.lower[0] + (int64_t)x, w.lower[1] + (int64_t)y, w.lower[2] + (int64_t)z};
        int64_t c[3], l[3];
        bool valid = true;
        for (int a = 0; a < 3; ++a) {
            dsh_split_cell(i[a], g.n[a], c[a], l[a]);
            valid = valid && dsh_chunk_in_range(c[a]);
        }
        const uint32_t pos = valid ? dsh_find(t, dsh_pack_key(c[0], c[1], c[2])) : kDshNoPos;
        if (pos != kDshNoPos) {
            const DshChunkView own = dsh_view_slot(p, (uint64_t)g.cells_per_chunk, t.slots[pos], g.default_record);
            if (dsh_record_free(own.cells ? own.cells[dsh_cell_index(l, g.n)] : own.record))
                frontier = dsh_unknown_neighbour(g, l, w.use_26 != 0, [&](int ox, int oy, int oz) {
                    return (ox | oy | oz) ? dsh_view_chunk(g, t, p, c[0] + ox, c[1] + oy, c[2] + oz) : own;
                });
        }
    }
    const unsigned long long b = __ballot(frontier);
    const int lane = threadIdx.x & 63;
    if (v < w.n && (lane == 0 || lane == 32)) w.bits[v >> 5] = (uint32_t)(b >> lane);
}

// The list form, first pass: one workgroup per live chunk.  A chunk that holds no cell of the box counts 0 and writes no mask.
// Lanes 0 .. 26 look the 27 chunks around (and including) it up once; then a thread per cell slot, 256 slots a round: each wave's
// ballot is one 64-bit word of the chunk's mask (bit k of word j: cell slot 64 j + k), written whole.  counts[slot] = the chunk's
// frontier cells, *total += them.
__global__ __launch_bounds__(kDshThreads) void k_dsh_frontier_count(const DshGeometry g, const DshTable t, const DshPool p, uint64_t n_live,
                                                                    const DshFrontierBox box, uint32_t use_26, uint32_t* __restrict__ counts,
                                                                    unsigned long long* __restrict__ masks, unsigned long long* total) {
    __shared__ DshChunkView around[27];
    __shared__ uint32_t wave_count[kDshThreads / 64];
    const uint64_t slot = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (slot >= n_live) return;                                                // (the last row of a two-dimensional launch)
    const uint64_t key = p.heads[slot].key;
    if (!dsh_key_in_range(key, box.chunks)) {                                  // (uniform over the workgroup)
        if (threadIdx.x == 0) counts[slot] = 0;
        return;
    }
    int64_t c[3];
    dsh_unpack_key(key, c[0], c[1], c[2]);
    const uint64_t cpc = (uint64_t)g.cells_per_chunk, words = dsh_frontier_mask_words(cpc);
    if (threadIdx.x < 27) {
        const int k = (int)threadIdx.x, ox = k / 9 - 1, oy = (k / 3) % 3 - 1, oz = k % 3 - 1;
        around[k] = k == 13 ? dsh_view_slot(p, cpc, slot, g.default_record) : dsh_view_chunk(g, t, p, c[0] + ox, c[1] + oy, c[2] + oz);
    }
    __syncthreads();
    const DshChunkView own = around[13];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t mine = 0;
    for (uint64_t base = 0; base < cpc; base += kDshThreads) {                 // (every thread runs every round: the ballots are whole)
        const uint64_t k = base + threadIdx.x;
        bool frontier = false;
        if (k < cpc) {
            const uint64_t q = k / (uint64_t)g.n[2];
            const int64_t l[3] = {(int64_t)(q / (uint64_t)g.n[1]), (int64_t)(q % (uint64_t)g.n[1]), (int64_t)(k % (uint64_t)g.n[2])};
            bool in = true;
            for (int a = 0; a < 3; ++a) {
                const int64_t i = c[a] * g.n[a] + l[a];
                in = in && i >= box.lo[a] && i <= box.hi[a];
            }
            if (in && dsh_record_free(own.cells ? own.cells[k] : own.record))
                frontier = dsh_unknown_neighbour(g, l, use_26 != 0, [&](int ox, int oy, int oz) { return around[(ox + 1) * 9 + (oy + 1) * 3 + (oz + 1)]; });
        }
        const unsigned long long b = __ballot(frontier);
        const uint64_t first = base + 64 * (uint64_t)wave;                     // the wave's first cell slot of this round
        if (lane == 0 && first < cpc) {
            masks[slot * words + (first >> 6)] = b;
            mine += (uint32_t)__popcll(b);
        }
    }
    if (lane == 0) wave_count[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int k = 0; k < kDshThreads / 64; ++k) sum += wave_count[k];
        counts[slot] = sum;
        if (sum) atomicAdd(total, (unsigned long long)sum);
    }
}

// Where a chunk's cells start in the list: the frontier cells of the live chunks with a smaller key.  k_dsh_rank's counting (every
// thread over all chunks, a tile of heads at a time through LDS) with the counts as weights: the rank and the scan over the chunks
// in key order in one pass, free of scratch, atomics and order effects.
// The counting itself, for every thread of the workgroup: the sum of weight(j) over the live chunks j with a key below `mine`.
template <class Weight>
__device__ __forceinline__ uint64_t dsh_weight_below(const DshChunkHead* __restrict__ heads, uint32_t n_live, uint64_t mine, Weight&& weight) {
    __shared__ uint64_t tile_key[kDshThreads];
    __shared__ uint32_t tile_weight[kDshThreads];
    uint64_t before = 0;
    for (uint32_t base = 0; base < n_live; base += kDshThreads) {
        const uint32_t j = base + threadIdx.x;
        tile_key[threadIdx.x] = j < n_live ? heads[j].key : kDshEmptyKey;      // (no key is above the empty key's value)
        tile_weight[threadIdx.x] = j < n_live ? weight(j) : 0u;
        __syncthreads();
        for (int k = 0; k < kDshThreads; ++k) before += tile_key[k] < mine ? tile_weight[k] : 0u;
        __syncthreads();
    }
    return before;
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_frontier_offsets(const DshChunkHead* __restrict__ heads, uint32_t n_live,
                                                                      const uint32_t* __restrict__ counts, uint64_t* __restrict__ offsets) {
    const int64_t s = dsh_item();
    const bool live = s < n_live;
    const uint64_t before = dsh_weight_below(heads, n_live, live ? heads[s].key : kDshEmptyKey, [&](uint32_t j) { return counts[j]; });
    if (live) offsets[s] = before;
}

// The list form, second pass: one workgroup per live chunk with frontier cells writes them, in cell slot order, from offsets[slot]
// on.  A thread per mask word: the words' popcounts are scanned over the workgroup, and a thread writes the cells of its word.
__global__ __launch_bounds__(kDshThreads) void k_dsh_frontier_write(const DshGeometry g, const DshChunkHead* __restrict__ heads, uint64_t n_live,
                                                                    const uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets,
                                                                    const unsigned long long* __restrict__ masks, int64_t* __restrict__ out) {
    __shared__ uint32_t wave_sum[kDshThreads / 64];
    const uint64_t slot = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (slot >= n_live || counts[slot] == 0) return;                           // (uniform over the workgroup)
    int64_t c[3];
    dsh_unpack_key(heads[slot].key, c[0], c[1], c[2]);
    const uint64_t words = dsh_frontier_mask_words((uint64_t)g.cells_per_chunk);
    uint64_t at = offsets[slot];
    for (uint64_t base = 0; base < words; base += kDshThreads) {
        const uint64_t j = base + threadIdx.x;
        unsigned long long word = j < words ? masks[slot * words + j] : 0ull;
        uint32_t total = 0;
        uint64_t o = at + dsh_block_exclusive((uint32_t)__popcll(word), wave_sum, total);
        while (word) {
            const uint64_t k = 64 * j + (uint64_t)(__ffsll(word) - 1), q = k / (uint64_t)g.n[2];
            word &= word - 1;
            out[3 * o] = c[0] * g.n[0] + (int64_t)(q / (uint64_t)g.n[1]);
            out[3 * o + 1] = c[1] * g.n[1] + (int64_t)(q % (uint64_t)g.n[1]);
            out[3 * o + 2] = c[2] * g.n[2] + (int64_t)(k % (uint64_t)g.n[2]);
            ++o;
        }
        at += total;
    }
}

// ---- connected components (include/sdfgpu.h "Dynamic spatial hashed map: connected components") ---------------------
// Nodes are numbered in export order (k_dsh_cc_bases: the weighted counting above), so a set's minimum node index is its first node
// in that order and the union-find and the root ranking of sdfgpu_unionfind.hpp give 1..K directly.  One label word per node in the
// scratch: k_dsh_cc_local writes every word once (plain stores), k_dsh_cc_merge joins across tiles and chunks with the agent-scope
// union-find only, the flatten, the scan and the relabel follow behind kernel boundaries.  Nothing but the relabel writes the map.
static_assert(kDshCcRankChunk == kRankChunk && kRankWords == kDshThreads, "the rank tables' layout as sdfgpu_dsh.hpp sizes it");

__device__ __forceinline__ uint32_t dsh_cc_record_class(uint64_t record, bool apart) { return dsh_cc_class(__uint_as_float((uint32_t)record), apart); }
__device__ __forceinline__ uint32_t dsh_cc_view_class(const DshChunkView& v, uint32_t k, bool apart) {
    return dsh_cc_record_class(v.cells ? v.cells[k] : v.record, apart);
}

__global__ __launch_bounds__(kDshThreads) void k_dsh_cc_bases(const DshChunkHead* __restrict__ heads, uint32_t n_live, uint32_t cells_per_chunk,
                                                              uint32_t* __restrict__ bases) {
    const int64_t s = dsh_item();
    const bool live = s < n_live;
    const uint64_t before = dsh_weight_below(heads, n_live, live ? heads[s].key : kDshEmptyKey,
                                             [&](uint32_t j) { return (uint32_t)dsh_cc_weight(heads[j].state, cells_per_chunk); });
    if (live) bases[s] = (uint32_t)before;                                     // (N < 2^32 - 1: the host has seen to it)
}

// One workgroup per tile of kDshCcTile consecutive cell slots of a cell-filled chunk (a chunk-filled chunk: its one word).  Slots
// ascend with the node index, so the tile-local minimum is the minimum of the tile's part of a component.  Class codes go into LDS,
// a cell starts under the first cell of its z run inside the tile (run-start bits out of ballots, then the highest start bit at or
// below the cell), y and x neighbours inside the tile are joined by union-find in LDS, and every cell's word becomes
// node base + tile start + local root.  Pairs that straddle a tile are k_dsh_cc_merge's.
__global__ __launch_bounds__(kDshThreads) void k_dsh_cc_local(const DshPool p, uint64_t n_live, uint32_t cells_per_chunk, uint32_t ny, uint32_t nz,
                                                              uint32_t tiles, uint32_t apart, const uint32_t* __restrict__ bases, uint32_t* __restrict__ L) {
    __shared__ uint32_t lab[kDshCcTile];
    __shared__ uint32_t starts[kDshCcTile / 32];
    __shared__ uint8_t cls[kDshCcTile];
    const uint64_t w = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (w >= n_live * tiles) return;                                           // (the last row of a two-dimensional launch)
    const uint64_t slot = w / tiles;
    const uint32_t tile = (uint32_t)(w - slot * tiles), base = bases[slot];
    if ((p.heads[slot].state & kDshStateMask) != kDshCellFilled) {             // (uniform over the workgroup)
        if (tile == 0 && threadIdx.x == 0) L[base] = base;
        return;
    }
    const uint32_t k0 = tile * kDshCcTile, nv = min(kDshCcTile, cells_per_chunk - k0), plane = ny * nz;
    const uint64_t* const cells = p.cells + slot * (uint64_t)cells_per_chunk + k0;
    for (uint32_t i = threadIdx.x; i < nv; i += kDshThreads) cls[i] = (uint8_t)dsh_cc_record_class(cells[i], apart != 0);
    __syncthreads();
    for (uint32_t b = 0; b < nv; b += kDshThreads) {                           // (every thread runs every round: the ballots are whole)
        const uint32_t i = b + threadIdx.x;
        const bool start = i < nv && (i == 0 || (k0 + i) % nz == 0 || cls[i - 1] != cls[i]);
        const unsigned long long m = __ballot(start);
        if ((threadIdx.x & 63) == 0) { starts[i >> 5] = (uint32_t)m; starts[(i >> 5) + 1] = (uint32_t)(m >> 32); }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nv; i += kDshThreads) {
        uint32_t word = i >> 5, d = starts[word] & (0xFFFFFFFFu >> (31 - (i & 31)));
        while (!d) d = starts[--word];                                         // (bit 0 of word 0 is set: the tile's first cell starts a run)
        lab[i] = 32 * word + (31 - (uint32_t)__clz(d));
    }
    __syncthreads();
    // y and x faces inside the tile.  A pair whose z predecessors are a same-class pair too is already joined through them.
    for (uint32_t i = threadIdx.x; i < nv; i += kDshThreads) {
        const uint32_t k = k0 + i, row = k / nz, iz = k - row * nz, ix = row / ny, iy = row - ix * ny, c = cls[i];
        const bool zp = iz > 0 && i > 0 && cls[i - 1] == c;
        if (iy > 0 && i >= nz && cls[i - nz] == c && !(zp && i > nz && cls[i - nz - 1] == c)) lds_union(lab, i, i - nz);
        if (ix > 0 && i >= plane && cls[i - plane] == c && !(zp && i > plane && cls[i - plane - 1] == c)) lds_union(lab, i, i - plane);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nv; i += kDshThreads) L[base + k0 + i] = base + k0 + lds_find(lab, i);
}

// One workgroup per live chunk joins what k_dsh_cc_local could not: the pairs of the chunk's own cells that straddle a tile, and the
// chunk's low x, y and z faces with the chunk beyond each -- three table lookups per chunk (lanes 0 .. 2), all four state pairs by
// one loop over a face's pairs (dsh_cc_face_pair), two chunk-filled chunks by one link.  A pair is skipped where its predecessor
// pair is of its class on both sides: that pair is linked (or skipped in turn), and each side's two cells are joined inside their
// chunk by the end of this launch.  Every label word is read and written through uf_union alone.
__global__ __launch_bounds__(kDshThreads) void k_dsh_cc_merge(const DshGeometry g, const DshTable t, const DshPool p, uint64_t n_live, uint32_t apart_flag,
                                                              const uint32_t* __restrict__ bases, uint32_t* L) {
    __shared__ DshChunkView beyond[3];
    __shared__ uint32_t beyond_base[3];
    __shared__ uint32_t beyond_live[3];
    const uint64_t slot = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (slot >= n_live) return;                                                // (the last row of a two-dimensional launch)
    const bool apart = apart_flag != 0;
    const uint32_t cpc = (uint32_t)g.cells_per_chunk, ny = (uint32_t)g.n[1], nz = (uint32_t)g.n[2], plane = ny * nz;
    if (threadIdx.x < 3) {
        const int a = (int)threadIdx.x;
        int64_t c[3];
        dsh_unpack_key(p.heads[slot].key, c[0], c[1], c[2]);
        const int64_t cx = c[0] - (a == 0), cy = c[1] - (a == 1), cz = c[2] - (a == 2);
        uint32_t live = 0;
        if (dsh_chunk_in_range(cx) && dsh_chunk_in_range(cy) && dsh_chunk_in_range(cz)) {
            const uint32_t pos = dsh_find(t, dsh_pack_key(cx, cy, cz));
            if (pos != kDshNoPos) {
                const uint64_t other = t.slots[pos];
                beyond[a] = dsh_view_slot(p, cpc, other, g.default_record);
                beyond_base[a] = bases[other];
                live = 1;
            }
        }
        beyond_live[a] = live;
    }
    __syncthreads();
    const DshChunkView own = dsh_view_slot(p, cpc, slot, g.default_record);
    const uint32_t base = bases[slot];

    if (own.cells)                                                             // (uniform over the workgroup)
        for (uint32_t k = kDshCcTile + threadIdx.x; k < cpc; k += kDshThreads) {
            const uint32_t first = k - k % kDshCcTile, row = k / nz, iz = k - row * nz, ix = row / ny, iy = row - ix * ny;
            const uint32_t c = dsh_cc_record_class(own.cells[k], apart);
            const bool zp = iz > 0 && dsh_cc_record_class(own.cells[k - 1], apart) == c;
            if (zp && k == first) uf_union<RootIsSelf>(L, base + k, base + k - 1);
            if (iy > 0 && k - nz < first && dsh_cc_record_class(own.cells[k - nz], apart) == c &&
                !(zp && dsh_cc_record_class(own.cells[k - nz - 1], apart) == c))
                uf_union<RootIsSelf>(L, base + k, base + k - nz);
            if (ix > 0 && k - plane < first && dsh_cc_record_class(own.cells[k - plane], apart) == c &&
                !(zp && dsh_cc_record_class(own.cells[k - plane - 1], apart) == c))
                uf_union<RootIsSelf>(L, base + k, base + k - plane);
        }

#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!beyond_live[a]) continue;                                         // (uniform over the workgroup)
        const DshChunkView other = beyond[a];
        const uint32_t other_base = beyond_base[a];
        const uint32_t pairs = (uint32_t)dsh_cc_face_pairs(own.cells != nullptr, other.cells != nullptr, cpc / (uint32_t)g.n[a]);
        for (uint32_t idx = threadIdx.x; idx < pairs; idx += kDshThreads) {
            uint32_t k, k2, back;
            dsh_cc_face_pair(a, idx, g.n, k, k2, back);
            const uint32_t c = dsh_cc_view_class(own, k, apart);
            if (dsh_cc_view_class(other, k2, apart) != c) continue;
            if (back && dsh_cc_view_class(own, k - back, apart) == c && dsh_cc_view_class(other, k2 - back, apart) == c) continue;
            uf_union<RootIsSelf>(L, (uint32_t)dsh_cc_node(base, own.cells != nullptr, k), (uint32_t)dsh_cc_node(other_base, other.cells != nullptr, k2));
        }
    }
}

// The root ranking of sdfgpu_unionfind.hpp over the N label words; every self-labelled node is a root.
__global__ __launch_bounds__(kRankWords) void k_dsh_cc_flatten(uint32_t* __restrict__ L, uint64_t n, uint32_t* __restrict__ rb, uint32_t* __restrict__ wr,
                                                               uint32_t* __restrict__ cc) {
    rank_flatten(L, n, RankTables{rb, wr, cc, nullptr}, [](uint64_t) { return true; });
}

__global__ __launch_bounds__(kRankScanThreads) void k_dsh_cc_scan(const uint32_t* __restrict__ cc, uint32_t* __restrict__ co, uint64_t chunks,
                                                                  uint32_t* __restrict__ count) {
    rank_scan(cc, co, chunks, count);
}

// k_dsh_cc_local's grid again: a node's rank goes into the component word of its record, the high 4 bytes of the 8 (COLLISION_CELL:
// occupancy | component), and of a chunk-filled chunk's head record.  Reads the node's own label word and the tables only.
__global__ __launch_bounds__(kDshThreads) void k_dsh_cc_relabel(const DshPool p, uint64_t n_live, uint32_t cells_per_chunk, uint32_t tiles,
                                                                const uint32_t* __restrict__ bases, const uint32_t* __restrict__ L,
                                                                const uint32_t* __restrict__ rb, const uint32_t* __restrict__ wr, const uint32_t* __restrict__ co) {
    const uint64_t w = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (w >= n_live * tiles) return;                                           // (the last row of a two-dimensional launch)
    const uint64_t slot = w / tiles;
    const uint32_t tile = (uint32_t)(w - slot * tiles), base = bases[slot];
    if ((p.heads[slot].state & kDshStateMask) != kDshCellFilled) {             // (uniform over the workgroup)
        if (tile == 0 && threadIdx.x == 0) reinterpret_cast<uint32_t*>(&p.heads[slot].record)[1] = rank_of(L[base], rb, wr, co);
        return;
    }
    const uint32_t k0 = tile * kDshCcTile, nv = min(kDshCcTile, cells_per_chunk - k0);
    uint32_t* const words = reinterpret_cast<uint32_t*>(p.cells + slot * (uint64_t)cells_per_chunk + k0);
    for (uint32_t i = threadIdx.x; i < nv; i += kDshThreads) words[2 * i + 1] = rank_of(L[base + k0 + i], rb, wr, co);
}

size_t dsh_fuse_lds_bytes(uint64_t cells_per_chunk) { return (size_t)((cells_per_chunk + 15) / 16 * 16); }   // at most 32 KiB

dim3 dsh_chunk_grid(uint64_t chunks) {                                        // one workgroup per chunk
    if (chunks <= (uint64_t)kDshGridX) return dim3((unsigned)std::max<uint64_t>(chunks, 1));
    return dim3((unsigned)kDshGridX, (unsigned)((chunks + kDshGridX - 1) / kDshGridX));
}

}  // namespace

}  // namespace sdfgpu

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
using namespace sdfgpu;

struct sdfgpu_dsh_map_object {
    sdfgpu_handle h = nullptr;
    DshGeometry g{};
    DshTable table{};
    uint64_t table_cap = 0;
    DshPool pool{};
    uint64_t pool_cap = 0;          // chunks
    uint64_t n_live = 0;            // chunks in use: slots 0 .. n_live - 1, every one chunk-filled or cell-filled
    uint64_t byte_limit = 0;
    DeviceBuffer scratch;           // per batch: table position, cell slot, new entries, winner flags, counters; the export's order
    DeviceBuffer stage;             // host forms: locations | values | records | statuses
    uint8_t* marks = nullptr;       // the mark plane of fused frames (null until the first): all zero between frames
    uint64_t marks_cap = 0;         // chunks it covers: at least pool_cap while a fused frame runs
    StreamOrder order;             // recorded behind every call: one on another stream waits for it first
    uint32_t cc_count = 0;          // connected components: K of the last update, the flags it ran under, and whether nothing has
    uint32_t cc_flags = 0;          // changed the map's content since
    bool cc_valid = false;
};

namespace {

constexpr size_t kDshCounterBytes = 256;

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

uint64_t dsh_bytes_held(const sdfgpu_dsh_map_object* m) { return dsh_table_bytes(m->table_cap) + dsh_pool_bytes(m->pool_cap, (uint64_t)m->g.cells_per_chunk); }

int dsh_alloc_table(sdfgpu_handle h, uint64_t cap, DshTable& t, hipStream_t st) {
    void* base = nullptr;
    if (int rc = rz_malloc(h, "dsh table", (size_t)dsh_table_bytes(cap), &base)) return rc;
    t.keys = static_cast<uint64_t*>(base);
    t.slots = reinterpret_cast<uint32_t*>(t.keys + cap);
    t.mask = cap - 1;
    HIP_TRY(h, hipMemsetAsync(t.keys, 0xFF, (size_t)cap * 8, st));
    return SDFGPU_OK;
}

int dsh_alloc_pool(sdfgpu_handle h, uint64_t chunks, uint64_t cells_per_chunk, DshPool& p) {
    p = DshPool{};
    if (int rc = rz_malloc(h, "dsh chunk heads", (size_t)(chunks * sizeof(DshChunkHead)), (void**)&p.heads)) return rc;
    if (int rc = rz_malloc(h, "dsh chunk cells", (size_t)(chunks * cells_per_chunk * 8), (void**)&p.cells)) {
        (void)rz_free(h, p.heads);
        p = DshPool{};
        return rc;
    }
    return SDFGPU_OK;
}

uint32_t* dsh_counters(sdfgpu_dsh_map_object* m) { return static_cast<uint32_t*>(m->scratch.ptr); }

// What every call does before it touches the map: the context's device, the map's event, and `st` behind the call before this one
// wherever that ran.
int dsh_wait(sdfgpu_dsh_map_object* m, hipStream_t st) {
    sdfgpu_handle h = m->h;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, m->order.create());
    HIP_TRY(h, m->order.wait(st));
    return SDFGPU_OK;
}

// The scope of one device body on `st`: open() is dsh_wait, and the map's event is recorded on `st` on every path out of the scope
// that open() did not refuse (a refused call has enqueued nothing).
struct DshCall {
    sdfgpu_dsh_map_object* m;
    hipStream_t st;
    bool armed = false;
    int open() { const int rc = dsh_wait(m, st); armed = rc == SDFGPU_OK; return rc; }
    ~DshCall() { if (armed) (void)m->order.record(st); }
};

// A buffer cut into 256-byte aligned sections: a running total, and each section as a typed pointer (null for an absent optional
// one, which takes no room).  dsh_cut runs a layout twice, to size the buffer and then, in the buffer, to hand the sections out.
struct DshCut {
    char* base;             // null while the layout is only measured
    size_t total;
    template <class T>
    T* take(size_t bytes, bool present = true) {
        if (!present) return nullptr;
        T* const at = base ? reinterpret_cast<T*>(base + total) : nullptr;
        total += align256(bytes);
        return at;
    }
};

template <class Layout>
int dsh_cut(sdfgpu_handle h, DeviceBuffer& b, const char* name, size_t first, Layout&& layout) {
    DshCut cut{nullptr, first};
    layout(cut);
    if (int rc = ensure(h, b, cut.total, name)) return rc;
    cut = DshCut{static_cast<char*>(b.ptr), first};
    layout(cut);
    return SDFGPU_OK;
}

// the per-call scratch: the counters are its first kDshCounterBytes, the call's sections follow
template <class Layout>
int dsh_scratch(sdfgpu_dsh_map_object* m, Layout&& layout) { return dsh_cut(m->h, m->scratch, "dsh batch scratch", kDshCounterBytes, layout); }

// every live chunk's key into `table` (empty, or holding none of them) and the count of keys that found no entry on its way to
// `lost`: enqueued, not waited for.  The counters are the caller's to clear.
int dsh_rehash_into(sdfgpu_dsh_map_object* m, const DshTable& table, uint64_t n_live, hipStream_t st, uint32_t* lost) {
    hipLaunchKernelGGL(k_dsh_rehash, dsh_grid((int64_t)n_live), dim3(kDshThreads), 0, st, table, m->pool.heads, (uint32_t)n_live, dsh_counters(m));
    HIP_TRY(m->h, hipGetLastError());
    HIP_TRY(m->h, hipMemcpyAsync(lost, dsh_counters(m) + 1, 4, hipMemcpyDeviceToHost, st));
    return SDFGPU_OK;
}

// the heads and the cells of the chunks in use into another pool: enqueued, not waited for
int dsh_copy_pool(sdfgpu_dsh_map_object* m, const DshPool& dst, hipStream_t st) {
    if (!m->n_live) return SDFGPU_OK;
    HIP_TRY(m->h, hipMemcpyAsync(dst.heads, m->pool.heads, (size_t)(m->n_live * sizeof(DshChunkHead)), hipMemcpyDeviceToDevice, st));
    HIP_TRY(m->h, hipMemcpyAsync(dst.cells, m->pool.cells, (size_t)(m->n_live * (uint64_t)m->g.cells_per_chunk * 8), hipMemcpyDeviceToDevice, st));
    return SDFGPU_OK;
}

// the table for `chunks` keys: grown (new table, rehash kernel) when it is too small.  Refused before anything changes when the
// larger table would pass the byte limit.  With `kept`, a table that was replaced is handed to the caller instead of being freed
// (kept->keys stays null when the table did not grow): a call that may still be refused puts it back, and nothing has changed.
int dsh_reserve_table(sdfgpu_dsh_map_object* m, uint64_t chunks, hipStream_t st, DshTable* kept = nullptr, uint64_t* kept_cap = nullptr) {
    sdfgpu_handle h = m->h;
    const uint64_t want = dsh_table_capacity(chunks);
    if (want <= m->table_cap) return SDFGPU_OK;
    if (want > ((uint64_t)1 << 31)) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dsh: a table of %llu entries is not supported", (unsigned long long)want);
    if (m->byte_limit && dsh_table_bytes(want) + dsh_pool_bytes(m->pool_cap, (uint64_t)m->g.cells_per_chunk) > m->byte_limit)
        return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dsh: the table for %llu chunks would pass the map's byte limit of %llu", (unsigned long long)chunks,
                    (unsigned long long)m->byte_limit);
    DshTable grown{};
    if (int rc = dsh_alloc_table(h, want, grown, st)) return rc;
    uint32_t lost = 0;
    if (m->n_live) {
        HIP_TRY(h, hipMemsetAsync(dsh_counters(m), 0, kDshCounterBytes, st));
        if (int rc = dsh_rehash_into(m, grown, m->n_live, st, &lost)) return rc;
    }
    HIP_TRY(h, hipStreamSynchronize(st));                                       // (the old table may still be read by pending work)
    if (lost) { (void)rz_free(h, grown.keys); return fail(h, SDFGPU_ERR_HIP, "dsh: the rehash lost %u keys (internal error)", lost); }
    if (kept) { *kept = m->table; *kept_cap = m->table_cap; }
    else if (int rc = rz_free(h, m->table.keys)) return rc;
    m->table = grown;
    m->table_cap = want;
    return SDFGPU_OK;
}

// the pool for `needed` chunks: grown (new allocations, device-to-device copies of the chunks in use) when it is too small
int dsh_reserve_pool(sdfgpu_dsh_map_object* m, uint64_t needed, hipStream_t st) {
    sdfgpu_handle h = m->h;
    const uint64_t cpc = (uint64_t)m->g.cells_per_chunk;
    uint64_t want = 0;
    if (!dsh_plan_pool(m->pool_cap, needed, cpc, dsh_table_bytes(m->table_cap), m->byte_limit, &want))
        return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dsh: a pool of %llu chunks would pass the map's byte limit of %llu", (unsigned long long)needed,
                    (unsigned long long)m->byte_limit);
    if (want == m->pool_cap) return SDFGPU_OK;
    DshPool grown{};
    if (int rc = dsh_alloc_pool(h, want, cpc, grown)) {
        if (want == needed) return rc;
        (void)hipGetLastError();                                                // the doubling does not fit the device: exactly what is needed
        want = needed;
        if (int rc2 = dsh_alloc_pool(h, want, cpc, grown)) return rc2;
    }
    if (int rc = dsh_copy_pool(m, grown, st)) return rc;
    HIP_TRY(h, hipStreamSynchronize(st));
    (void)rz_free(h, m->pool.heads);
    (void)rz_free(h, m->pool.cells);
    m->pool = grown;
    m->pool_cap = want;
    return SDFGPU_OK;
}

// the mark plane for the pool dsh_reserve_pool(needed) will leave: made, or replaced by a larger one, and cleared.  Nothing is copied
// (it is all zero between frames).  Called in front of dsh_reserve_pool, so a frame this refuses has grown nothing; a pool that a
// batch grew in between is caught up with here, at the next fused frame.
int dsh_reserve_marks(sdfgpu_dsh_map_object* m, uint64_t needed, hipStream_t st) {
    sdfgpu_handle h = m->h;
    const uint64_t cpc = (uint64_t)m->g.cells_per_chunk;
    uint64_t want = m->pool_cap;
    (void)dsh_plan_pool(m->pool_cap, needed, cpc, dsh_table_bytes(m->table_cap), m->byte_limit, &want);   // (refused: dsh_reserve_pool says so)
    if (want <= m->marks_cap) return SDFGPU_OK;
    void* grown = nullptr;
    if (int rc = rz_malloc(h, "dsh fusion marks", (size_t)dsh_mark_bytes(want, cpc), &grown)) {
        const uint64_t least = std::max(needed, m->pool_cap);
        if (want == least) return rc;
        (void)hipGetLastError();                                                // as the pool does: exactly what is needed
        want = least;
        if (int rc2 = rz_malloc(h, "dsh fusion marks", (size_t)dsh_mark_bytes(want, cpc), &grown)) return rc2;
    }
    if (hipMemsetAsync(grown, 0, (size_t)dsh_mark_bytes(want, cpc), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        (void)rz_free(h, grown);
        return fail(h, SDFGPU_ERR_HIP, "dsh: clearing the fusion marks failed");
    }
    if (m->marks) (void)rz_free(h, m->marks);
    m->marks = static_cast<uint8_t*>(grown);
    m->marks_cap = want;
    return SDFGPU_OK;
}

// What follows an inserting kernel, its read-back and their synchronisation: the `n_new` chunks of `newlist` are committed or refused.
// `rc` says what the caller made of the read-back (lost operations, a HIP error).  The mark plane (fused frames only) is reserved in
// front of the pool.  Refused, the table is the one the call found: a frame hands over the table it replaced (`kept`; kept->keys is
// null where it did not grow) and gets it back, where none was handed over the new entries become empty again -- so a refused
// batch, which hands nothing over, keeps a table it grew.  A frame's work is waited for before its table goes (its HIP calls may
// have failed half way), a batch's rollback is waited for.
int dsh_commit_new(sdfgpu_dsh_map_object* m, int rc, uint32_t n_new, const uint32_t* newlist, bool marks, DshTable* kept, uint64_t kept_cap, hipStream_t st) {
    sdfgpu_handle h = m->h;
    const dim3 block(kDshThreads);
    if (rc == SDFGPU_OK && marks) rc = dsh_reserve_marks(m, m->n_live + n_new, st);
    if (rc == SDFGPU_OK) rc = dsh_reserve_pool(m, m->n_live + n_new, st);
    if (rc != SDFGPU_OK) {
        if (kept) (void)hipStreamSynchronize(st);
        if (kept && kept->keys) {
            (void)rz_free(h, m->table.keys);
            m->table = *kept;
            m->table_cap = kept_cap;
            return rc;
        }
        if (n_new) hipLaunchKernelGGL(k_dsh_rollback, dsh_grid(n_new), block, 0, st, m->table, newlist, n_new);
        if (n_new || !kept) (void)hipStreamSynchronize(st);
        return rc;
    }
    if (kept && kept->keys) (void)rz_free(h, kept->keys);
    if (n_new) hipLaunchKernelGGL(k_dsh_init_new, dsh_grid(n_new), block, 0, st, m->table, m->pool.heads, newlist, n_new, (uint32_t)m->n_live);
    m->n_live += n_new;
    return SDFGPU_OK;
}

int dsh_check_map(sdfgpu_dsh_map m) { return m && m->h ? SDFGPU_OK : SDFGPU_ERR_INVALID_ARGUMENT; }

int dsh_aligned8(sdfgpu_handle h, const void* p, const char* what) {
    if (reinterpret_cast<uintptr_t>(p) & 7) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: %s must be 8-byte aligned", what);
    return SDFGPU_OK;
}

// the writes of a batch into the cells (or, CHUNK, the chunk records) its operations name: one record for all of them, or the order rule
template <bool CHUNK>
void dsh_write(sdfgpu_dsh_map_object* m, const uint32_t* op_pos, const uint32_t* op_cell, int64_t n, uint8_t* wins, const void* d_values,
               const void* one_value, hipStream_t st) {
    const dim3 grid = dsh_grid(n), block(kDshThreads);
    const uint64_t cpc = (uint64_t)m->g.cells_per_chunk;
    uint64_t value = 0;
    if (one_value) memcpy(&value, one_value, 8);
    hipLaunchKernelGGL((k_dsh_store_one<CHUNK>), grid, block, 0, st, m->table, m->pool, cpc, op_pos, op_cell, n, value);
    if (one_value) return;
    hipLaunchKernelGGL((k_dsh_stamp<CHUNK>), grid, block, 0, st, m->table, m->pool, cpc, op_pos, op_cell, n);
    hipLaunchKernelGGL((k_dsh_decide<CHUNK>), grid, block, 0, st, m->table, m->pool, cpc, op_pos, op_cell, n, wins);
    hipLaunchKernelGGL((k_dsh_apply<CHUNK>), grid, block, 0, st, m->table, m->pool, cpc, op_pos, op_cell, n, wins, static_cast<const uint64_t*>(d_values));
}

// One batch on `st`: cell sets (locations as doubles, or points as floats) or chunk sets.
template <typename LOC>
int dsh_batch(sdfgpu_dsh_map_object* m, bool chunk_sets, const LOC* d_loc, int64_t n, const void* d_values, const void* one_value,
              uint8_t* d_statuses, hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (n < 0 || n >= kDshMaxBatch) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a batch holds 0 .. 2^31 - 1 operations (got %lld)", (long long)n);
    if ((d_values != nullptr) == (one_value != nullptr))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: give one record for the batch or one per operation, not both and not neither");
    if (n == 0) return SDFGPU_OK;
    if (!d_loc) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null locations");
    if (int rc = dsh_aligned8(h, d_values, "the values")) return rc;
    if (reinterpret_cast<uintptr_t>(d_loc) & (sizeof(LOC) - 1)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the locations are not aligned for their type");
    DshCall call{m, st};
    if (int rc = call.open()) return rc;

    const size_t un = (size_t)n;
    uint32_t *op_pos = nullptr, *op_cell = nullptr, *newlist = nullptr;
    uint8_t* wins = nullptr;
    if (int rc = dsh_scratch(m, [&](DshCut& c) {
            op_pos = c.take<uint32_t>(un * 4); op_cell = c.take<uint32_t>(un * 4); newlist = c.take<uint32_t>(un * 4); wins = c.take<uint8_t>(un);
        })) return rc;
    uint32_t* const counters = dsh_counters(m);

    // the table cannot fill while the batch inserts: the number of operations bounds the number of new chunks
    if (int rc = dsh_reserve_table(m, m->n_live + (uint64_t)n, st)) return rc;
    const dim3 grid = dsh_grid(n), block(kDshThreads);
    HIP_TRY(h, hipMemsetAsync(counters, 0, kDshCounterBytes, st));
    hipLaunchKernelGGL((k_dsh_insert<LOC>), grid, block, 0, st, m->g, m->table, d_loc, n, (uint32_t)m->n_live, op_pos, op_cell, newlist, counters, d_statuses,
                       (uint8_t)(chunk_sets ? SDFGPU_DSH_SET_CHUNK : SDFGPU_DSH_SET_CELL));
    HIP_TRY(h, hipGetLastError());
    uint32_t back[3] = {0, 0, 0};                                               // new chunks, lost operations, whether any operation was valid
    HIP_TRY(h, hipMemcpyAsync(back, counters, sizeof back, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const int lost = back[1] ? fail(h, SDFGPU_ERR_HIP, "dsh: %u operations found no table entry (internal error)", back[1]) : SDFGPU_OK;
    if (int rc = dsh_commit_new(m, lost, back[0], newlist, false, nullptr, 0, st)) return rc;
    if (back[2]) m->cc_valid = false;                                           // (a batch of invalid locations alone sets nothing)
    if (!chunk_sets) {
        hipLaunchKernelGGL(k_dsh_touch, grid, block, 0, st, m->table, m->pool.heads, op_pos, n);
        hipLaunchKernelGGL(k_dsh_expand, dsh_chunk_grid(m->n_live), block, 0, st, m->pool, m->n_live, (uint64_t)m->g.cells_per_chunk, m->g.default_record);
        dsh_write<false>(m, op_pos, op_cell, n, wins, d_values, one_value, st);
    } else {
        dsh_write<true>(m, op_pos, op_cell, n, wins, d_values, one_value, st);
    }
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

constexpr char kDshFrameNeeds[] = "dsh: insert_rays needs the sensor, the free record and the hit record";

// the range of a frame or a cast, R = max_range in cells with 0 < R <= 65536, in what the kernels are told
int dsh_ray_range(sdfgpu_dsh_map_object* m, double max_range, DshRayFrame& f) {
    const double range = max_range * m->g.inv_cell;
    if (!(range > 0.0 && range <= kDshMaxRangeCells))
        return fail(m->h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: max_range must span more than 0 and at most 65536 cells (got %g, %g cells)", max_range, range);
    f.range2 = range * range;
    f.range_cells = (uint64_t)std::ceil(range);
    f.max_steps = dsh_ray_max_steps(f.range_cells);
    return SDFGPU_OK;
}

// What a frame of rays is refused for before anything is enqueued, and what the host works out about the sensor (dsh_start_cell: the
// arithmetic of the lanes, compiled without contraction here too).
int dsh_ray_frame(sdfgpu_dsh_map_object* m, const double* sensor, int64_t n, double max_range, DshRayFrame& f) {
    sdfgpu_handle h = m->h;
    if (n < 0 || n >= kDshMaxBatch) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a frame holds 0 .. 2^31 - 1 rays (got %lld)", (long long)n);
    if (!sensor) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "%s", kDshFrameNeeds);
    if (int rc = dsh_ray_range(m, max_range, f)) return rc;
    if (!(std::isfinite(sensor[0]) && std::isfinite(sensor[1]) && std::isfinite(sensor[2])))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the sensor position is not finite");
    if (!dsh_start_cell(m->g, sensor[0], sensor[1], sensor[2], f))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the sensor position is not a valid location of the map");
    return SDFGPU_OK;
}

// What the carve entry points, device and host form, check: the two records every ray stores, then the frame.
int dsh_carve_frame(sdfgpu_dsh_map_object* m, const double* sensor, int64_t n, double max_range, const void* free_value, const void* hit_value, DshRayFrame& f) {
    if (!free_value || !hit_value) return fail(m->h, SDFGPU_ERR_INVALID_ARGUMENT, "%s", kDshFrameNeeds);
    return dsh_ray_frame(m, sensor, n, max_range, f);
}

// The sensor model of a fused frame, checked and turned into what k_dsh_ray_fuse is told.
int dsh_fuse_model(sdfgpu_handle h, const sdfgpu_dsh_sensor_model* model, DshFuse& u) {
    if (!model) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: fuse_rays needs the sensor model");
    if (!dsh_fuse_model_ok(model->prob_hit, model->prob_miss, model->clamp_min, model->clamp_max))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the sensor model's numbers must lie in [0.001, 0.999] with clamp_min <= clamp_max (got %g, %g, %g, %g)",
                    (double)model->prob_hit, (double)model->prob_miss, (double)model->clamp_min, (double)model->clamp_max);
    u.hit = model->prob_hit;
    u.one_minus_hit = 1.0f - model->prob_hit;
    u.miss = model->prob_miss;
    u.one_minus_miss = 1.0f - model->prob_miss;
    u.clamp_min = model->clamp_min;
    u.clamp_max = model->clamp_max;
    return SDFGPU_OK;
}

// One frame of rays on `st` (the frame was checked by dsh_ray_frame): carved with the two records, or (fuse) fused with the model.
int dsh_rays_impl(sdfgpu_dsh_map_object* m, const DshRayFrame& f, const float* d_points, int64_t n, const void* free_value, const void* hit_value,
                  const DshFuse* fuse, uint8_t* d_statuses, sdfgpu_dsh_ray_counts* out_counts, hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (out_counts) *out_counts = sdfgpu_dsh_ray_counts{};
    if (n == 0) return SDFGPU_OK;
    if (!d_points) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null points");
    if (reinterpret_cast<uintptr_t>(d_points) & 3) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the points are not aligned for their type");
    DshCall call{m, st};
    if (int rc = call.open()) return rc;

    // the table cannot fill while the frame inserts: it is sized for every chunk the rays can enter.  Where the bound that needs no
    // ray would make it grow, the rays are counted first (one more read-back)
    uint64_t bound = dsh_ray_chunk_bound((uint64_t)n, f.range_cells, m->g.n);
    if (bound > ((uint64_t)1 << 30) || dsh_table_capacity(m->n_live + bound) > m->table_cap) {
        unsigned long long by_rays = 0;
        HIP_TRY(h, hipMemsetAsync(dsh_counters(m), 0, kDshCounterBytes, st));
        hipLaunchKernelGGL(k_dsh_ray_count, dsh_grid(n), dim3(kDshThreads), 0, st, m->g, f, d_points, n, dsh_counters(m));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(&by_rays, dsh_counters(m) + 2, sizeof by_rays, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        bound = std::min<uint64_t>(bound, by_rays);
    }
    if (m->n_live + bound > ((uint64_t)1 << 30))
        return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dsh: a frame of %lld rays of %llu cells may enter %llu chunks: more than a table holds", (long long)n,
                    (unsigned long long)f.range_cells, (unsigned long long)bound);
    const size_t un = (size_t)n, table_cap = (size_t)std::max(m->table_cap, dsh_table_capacity(m->n_live + bound));
    uint32_t *op_pos = nullptr, *op_cell = nullptr, *newlist = nullptr;
    uint8_t* marks = nullptr;
    if (int rc = dsh_scratch(m, [&](DshCut& c) {
            op_pos = c.take<uint32_t>(un * 4); op_cell = c.take<uint32_t>(un * 4); newlist = c.take<uint32_t>(table_cap * 4); marks = c.take<uint8_t>(table_cap);
        })) return rc;
    uint32_t* const counters = dsh_counters(m);
    DshTable old_table{};
    uint64_t old_cap = 0;
    if (int rc = dsh_reserve_table(m, m->n_live + bound, st, &old_table, &old_cap)) return rc;
    const dim3 grid = dsh_grid(n), block(kDshThreads);
    const uint64_t cpc = (uint64_t)m->g.cells_per_chunk;

    struct { uint32_t n_new, lost; unsigned long long counts[kDshRayCounts]; } back{};
    static_assert(sizeof back == 8 + 8 * kDshRayCounts && sizeof back <= kDshCounterBytes, "the counters' layout");
    // walk A and the read-back of the new-chunk count: until dsh_commit_new has reserved the pool the frame can still be refused
    const int walked = [&]() -> int {
        HIP_TRY(h, hipMemsetAsync(counters, 0, kDshCounterBytes, st));
        HIP_TRY(h, hipMemsetAsync(marks, 0, (size_t)m->table_cap, st));
        hipLaunchKernelGGL(k_dsh_ray_insert, grid, block, 0, st, m->g, m->table, f, d_points, n, (uint32_t)m->n_live, op_pos, op_cell, newlist, marks, counters,
                           d_statuses);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(&back, counters, sizeof back, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        if (back.lost) return fail(h, SDFGPU_ERR_HIP, "dsh: %u chunk keys found no table entry (internal error)", back.lost);
        return SDFGPU_OK;
    }();
    if (int rc = dsh_commit_new(m, walked, back.n_new, newlist, fuse != nullptr, &old_table, old_cap, st)) return rc;
    if (back.counts[0] + back.counts[1]) m->cc_valid = false;                   // (a ray that is hit or truncated writes at least its first cell)
    hipLaunchKernelGGL(k_dsh_ray_touch, dsh_grid((int64_t)m->table_cap), block, 0, st, m->table, m->pool.heads, marks);
    hipLaunchKernelGGL(k_dsh_expand, dsh_chunk_grid(m->n_live), block, 0, st, m->pool, m->n_live, cpc, m->g.default_record);
    if (!fuse) {
        uint64_t free_record = 0, hit_record = 0;
        memcpy(&free_record, free_value, 8);
        memcpy(&hit_record, hit_value, 8);
        hipLaunchKernelGGL(k_dsh_ray_carve, grid, block, 0, st, m->g, m->table, m->pool, f, d_points, n, free_record);
        hipLaunchKernelGGL((k_dsh_store_one<false>), grid, block, 0, st, m->table, m->pool, cpc, op_pos, op_cell, n, hit_record);
    } else {                                                                    // walk B into the mark plane, the hits behind it, then one update per marked cell
        hipLaunchKernelGGL(k_dsh_ray_mark, grid, block, 0, st, m->g, m->table, m->marks, f, d_points, n);
        hipLaunchKernelGGL(k_dsh_ray_mark_hits, grid, block, 0, st, m->table, m->marks, cpc, op_pos, op_cell, n);
        hipLaunchKernelGGL(k_dsh_ray_touch, dsh_grid((int64_t)m->table_cap), block, 0, st, m->table, m->pool.heads, marks);
        hipLaunchKernelGGL(k_dsh_ray_fuse, dsh_chunk_grid(m->n_live), block, dsh_fuse_lds_bytes(cpc), st, m->pool, m->marks, m->n_live, (uint32_t)cpc, *fuse);
    }
    HIP_TRY(h, hipGetLastError());
    if (out_counts) {
        out_counts->rays_hit = back.counts[0];
        out_counts->rays_truncated = back.counts[1];
        out_counts->rays_skipped = back.counts[2];
        out_counts->cells_carved = back.counts[3];
        out_counts->new_chunks = back.n_new;
    }
    return SDFGPU_OK;
}

int dsh_get_impl(sdfgpu_dsh_map_object* m, const double* d_loc, int64_t n, void* d_records, uint8_t* d_statuses, hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (n < 0 || n >= kDshMaxBatch) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a batch holds 0 .. 2^31 - 1 locations (got %lld)", (long long)n);
    if (!d_records && !d_statuses) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: get needs an output");
    if (n == 0) return SDFGPU_OK;
    if (!d_loc) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null locations");
    if (int rc = dsh_aligned8(h, d_records, "the records")) return rc;
    if (int rc = dsh_aligned8(h, d_loc, "the locations")) return rc;
    DshCall call{m, st};
    if (int rc = call.open()) return rc;
    hipLaunchKernelGGL(k_dsh_get, dsh_grid(n), dim3(kDshThreads), 0, st, m->g, m->table, m->pool, d_loc, n, static_cast<uint64_t*>(d_records), d_statuses);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// What a cast is refused for before anything is enqueued; the range of a cast in what the kernel is told (and, with a sensor, the
// sensor as dsh_ray_frame works it out).
int dsh_cast_frame(sdfgpu_dsh_map_object* m, const double* sensor, bool segments, int64_t n, double max_range, uint32_t flags, const void* statuses,
                   const void* hits, DshRayFrame& f) {
    sdfgpu_handle h = m->h;
    if (segments) {                                                            // (every start is the lane's own: only the range is the frame's)
        if (n < 0 || n >= kDshMaxBatch) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a cast holds 0 .. 2^31 - 1 segments (got %lld)", (long long)n);
        f = DshRayFrame{};
        if (int rc = dsh_ray_range(m, max_range, f)) return rc;
    } else {
        if (!sensor) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: cast_rays needs the sensor");
        if (int rc = dsh_ray_frame(m, sensor, n, max_range, f)) return rc;
    }
    if (flags & ~(uint32_t)(SDFGPU_DSH_CAST_SKIP_FIRST | SDFGPU_DSH_CAST_SKIP_LAST | SDFGPU_DSH_CAST_UNKNOWN_IS_FILLED))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a cast knows the flags SKIP_FIRST, SKIP_LAST and UNKNOWN_IS_FILLED (got 0x%x)", flags);
    if (!statuses && !hits) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a cast needs an output");
    return SDFGPU_OK;
}

// One cast on `st` (checked by dsh_cast_frame): rays from the frame's sensor to d_points, or the segments d_starts -> d_ends.
int dsh_cast_impl(sdfgpu_dsh_map_object* m, const DshRayFrame& f, bool segments, const float* d_points, const double* d_starts, const double* d_ends,
                  int64_t n, uint32_t flags, uint8_t* d_statuses, sdfgpu_dsh_cast_hit* d_hits, hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (n == 0) return SDFGPU_OK;
    if (segments ? !d_starts || !d_ends : !d_points) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a cast needs its %s", segments ? "starts and ends" : "points");
    if (segments) {
        if (int rc = dsh_aligned8(h, d_starts, "the starts")) return rc;
        if (int rc = dsh_aligned8(h, d_ends, "the ends")) return rc;
    } else if (reinterpret_cast<uintptr_t>(d_points) & 3) {
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the points must be 4-byte aligned");
    }
    if (int rc = dsh_aligned8(h, d_hits, "the hits")) return rc;
    DshCall call{m, st};
    if (int rc = call.open()) return rc;
    const auto kernel = segments ? k_dsh_cast<true> : k_dsh_cast<false>;
    hipLaunchKernelGGL(kernel, dsh_grid(n), dim3(kDshThreads), 0, st, m->g, m->table, m->pool, f, d_points, d_starts, d_ends, n, flags, d_statuses, d_hits);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

int dsh_check_window(sdfgpu_handle h, const int64_t* lower, int64_t nx, int64_t ny, int64_t nz, const void* records, const void* bits) {
    if (!lower) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null lower corner");
    if (!records && !bits) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a window needs an output");
    if (int rc = check_dims_u32(h, nx, ny, nz, "the window's voxels are numbered by uint32")) return rc;
    const int64_t far = (int64_t)1 << 61;                                      // lower + extent cannot overflow; anything near is out of range anyway
    for (int a = 0; a < 3; ++a)
        if (lower[a] < -far || lower[a] > far) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the window's lower corner is beyond +-2^61 cells");
    return SDFGPU_OK;
}

int dsh_window_impl(sdfgpu_dsh_map_object* m, const int64_t* lower, int64_t nx, int64_t ny, int64_t nz, int unknown_is_filled, void* d_records,
                    uint32_t* d_bits, hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (int rc = dsh_aligned8(h, d_records, "the records")) return rc;
    if (reinterpret_cast<uintptr_t>(d_bits) & 3) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the bit field must be 4-byte aligned");
    DshCall call{m, st};
    if (int rc = call.open()) return rc;
    DshWindow w{};
    for (int a = 0; a < 3; ++a) w.lower[a] = lower[a];
    w.ny = (uint32_t)ny; w.nz = (uint32_t)nz;
    w.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    w.unknown_is_filled = unknown_is_filled != 0;
    w.records = static_cast<uint64_t*>(d_records);
    w.bits = d_bits;
    hipLaunchKernelGGL(k_dsh_window, dsh_grid((int64_t)w.n), dim3(kDshThreads), 0, st, m->g, m->table, m->pool, w);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

int dsh_check_frontier_flags(sdfgpu_handle h, uint32_t flags) {
    if (flags & ~(uint32_t)SDFGPU_DSH_FRONTIER_26) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a frontier call knows the flag FRONTIER_26 (got 0x%x)", flags);
    return SDFGPU_OK;
}

// The frontier bits of a window on `st` (checked by dsh_check_window and dsh_check_frontier_flags): one kernel, nothing allocated.
int dsh_frontier_window_impl(sdfgpu_dsh_map_object* m, const int64_t* lower, int64_t nx, int64_t ny, int64_t nz, uint32_t flags, uint32_t* d_bits,
                             hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (reinterpret_cast<uintptr_t>(d_bits) & 3) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the bit field must be 4-byte aligned");
    DshCall call{m, st};
    if (int rc = call.open()) return rc;
    DshFrontierWindow w{};
    for (int a = 0; a < 3; ++a) w.lower[a] = lower[a];
    w.ny = (uint32_t)ny; w.nz = (uint32_t)nz;
    w.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    w.use_26 = (flags & SDFGPU_DSH_FRONTIER_26) != 0;
    w.bits = d_bits;
    hipLaunchKernelGGL(k_dsh_frontier_window, dsh_grid((int64_t)w.n), dim3(kDshThreads), 0, st, m->g, m->table, m->pool, w);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// What a frontier list is refused for before anything is enqueued, and its box.
int dsh_frontier_cells_check(sdfgpu_dsh_map_object* m, const int64_t* lower, const int64_t* extent, uint32_t flags, const void* cells, int64_t capacity,
                             const int64_t* out_total, DshFrontierBox& box) {
    sdfgpu_handle h = m->h;
    if (int rc = dsh_check_frontier_flags(h, flags)) return rc;
    if (!out_total) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: frontier_cells needs out_total");
    if (capacity < 0 || (capacity > 0 && !cells)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: frontier_cells: a capacity without a buffer");
    if (!lower != !extent) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: frontier_cells takes lower and extent, or neither (the whole map)");
    if (lower && !dsh_frontier_box_ok(lower, extent))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a frontier box has extent >= 1 on every axis and lower + extent - 1 within int64");
    box = dsh_frontier_box(lower, extent, m->g.n);
    return SDFGPU_OK;
}

// The frontier cells of the box on `st` (checked by dsh_frontier_cells_check): count and mask per chunk | the total read back | offsets
// in key order | write.  The list is written iff capacity suffices.
int dsh_frontier_cells_impl(sdfgpu_dsh_map_object* m, const DshFrontierBox& box, uint32_t flags, int64_t* d_cells, int64_t capacity, int64_t* out_total,
                            hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (int rc = dsh_aligned8(h, d_cells, "the cell list")) return rc;
    DshCall call{m, st};
    if (int rc = call.open()) return rc;
    *out_total = 0;
    if (!m->n_live || box.chunks.empty) return SDFGPU_OK;
    const size_t live = (size_t)m->n_live, words = (size_t)dsh_frontier_mask_words((uint64_t)m->g.cells_per_chunk);
    uint32_t* counts = nullptr;
    uint64_t* offsets = nullptr;
    unsigned long long* masks = nullptr;
    if (int rc = dsh_scratch(m, [&](DshCut& c) {
            counts = c.take<uint32_t>(live * 4); offsets = c.take<uint64_t>(live * 8); masks = c.take<unsigned long long>(live * words * 8);
        })) return rc;
    unsigned long long* const d_total = static_cast<unsigned long long*>(m->scratch.ptr);
    const uint32_t use_26 = (flags & SDFGPU_DSH_FRONTIER_26) != 0;
    HIP_TRY(h, hipMemsetAsync(d_total, 0, kDshCounterBytes, st));
    hipLaunchKernelGGL(k_dsh_frontier_count, dsh_chunk_grid(m->n_live), dim3(kDshThreads), 0, st, m->g, m->table, m->pool, m->n_live, box, use_26, counts, masks,
                       d_total);
    HIP_TRY(h, hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));                                       // the call's one synchronisation
    *out_total = (int64_t)total;
    if (total == 0 || (uint64_t)capacity < total) return SDFGPU_OK;
    hipLaunchKernelGGL(k_dsh_frontier_offsets, dsh_grid((int64_t)live), dim3(kDshThreads), 0, st, m->pool.heads, (uint32_t)m->n_live, counts, offsets);
    hipLaunchKernelGGL(k_dsh_frontier_write, dsh_chunk_grid(m->n_live), dim3(kDshThreads), 0, st, m->g, m->pool.heads, m->n_live, counts, offsets, masks, d_cells);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// live chunks by state (synchronises st)
int dsh_count(sdfgpu_dsh_map_object* m, uint64_t* chunk_filled, uint64_t* cell_filled, hipStream_t st) {
    sdfgpu_handle h = m->h;
    *chunk_filled = *cell_filled = 0;
    if (!m->n_live) return SDFGPU_OK;
    if (int rc = ensure(h, m->scratch, kDshCounterBytes, "dsh batch scratch")) return rc;
    unsigned long long* const counts = static_cast<unsigned long long*>(m->scratch.ptr);
    HIP_TRY(h, hipMemsetAsync(counts, 0, kDshCounterBytes, st));
    hipLaunchKernelGGL(k_dsh_count, dsh_grid((int64_t)m->n_live), dim3(kDshThreads), 0, st, m->pool.heads, (uint32_t)m->n_live, counts);
    HIP_TRY(h, hipGetLastError());
    unsigned long long back[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(back, counts, sizeof back, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    *chunk_filled = back[0];
    *cell_filled = back[1];
    return SDFGPU_OK;
}

// The components of the whole map on `st`: the chunks counted by state and read back (N sizes the scratch, and a map of 2^32 - 1
// nodes or more is refused before anything is written) | node bases | labels inside tiles | joins across tiles and chunks | flatten |
// scan | relabel into the records | K read back.  Two synchronisations: behind the count and at the end.
int dsh_components_impl(sdfgpu_dsh_map_object* m, uint32_t flags, uint32_t* out_count, hipStream_t st) {
    sdfgpu_handle h = m->h;
    static_assert(kDshComponentsUnknownApart == SDFGPU_DSH_COMPONENTS_UNKNOWN_APART, "the flag as sdfgpu_dsh.hpp states it");
    if (flags & ~kDshComponentsUnknownApart)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: update_components knows the flag COMPONENTS_UNKNOWN_APART (got 0x%x)", flags);
    DshCall call{m, st};
    if (int rc = call.open()) return rc;
    const uint64_t cpc = (uint64_t)m->g.cells_per_chunk;
    uint64_t chunk_filled = 0, cell_filled = 0;
    if (int rc = dsh_count(m, &chunk_filled, &cell_filled, st)) return rc;
    const uint64_t nodes = dsh_cc_nodes(cell_filled, chunk_filled, cpc);
    if (!dsh_cc_nodes_ok(nodes))
        return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dsh: update_components numbers fewer than 2^32 - 1 nodes (the map has %llu)", (unsigned long long)nodes);
    uint32_t count = 0;
    if (m->n_live) {
        const size_t live = (size_t)m->n_live;
        const uint64_t rank = rank_chunks(nodes);
        const uint32_t tiles = (uint32_t)dsh_cc_tiles(cpc), apart = (flags & kDshComponentsUnknownApart) != 0;
        uint32_t *bases = nullptr, *labels = nullptr;
        void* tables = nullptr;
        size_t cut_bytes = 0;
        if (int rc = dsh_scratch(m, [&](DshCut& c) {
                bases = c.take<uint32_t>((size_t)dsh_cc_bases_bytes(live)); labels = c.take<uint32_t>((size_t)dsh_cc_label_bytes(nodes));
                tables = c.take<char>((size_t)dsh_cc_rank_bytes(nodes));
                cut_bytes = c.total - kDshCounterBytes;
            })) return rc;
        if (cut_bytes != dsh_cc_scratch_bytes(live, nodes) || rank_tables_bytes(rank) != dsh_cc_rank_bytes(nodes))
            return fail(h, SDFGPU_ERR_HIP, "dsh: the components' scratch is not laid out as sdfgpu_dsh.hpp sizes it (internal error)");
        const RankTables t = rank_tables_at(tables, rank);
        uint32_t* const d_count = dsh_counters(m);                              // K
        const dim3 block(kDshThreads), live_grid = dsh_grid((int64_t)live), chunk_grid = dsh_chunk_grid(m->n_live), tile_grid = dsh_chunk_grid(m->n_live * tiles);
        m->cc_valid = false;                                                    // (until K is back: a call that fails half way leaves no claim)
        hipLaunchKernelGGL(k_dsh_cc_bases, live_grid, block, 0, st, m->pool.heads, (uint32_t)m->n_live, (uint32_t)cpc, bases);
        hipLaunchKernelGGL(k_dsh_cc_local, tile_grid, block, 0, st, m->pool, m->n_live, (uint32_t)cpc, (uint32_t)m->g.n[1], (uint32_t)m->g.n[2], tiles, apart, bases,
                           labels);
        hipLaunchKernelGGL(k_dsh_cc_merge, chunk_grid, block, 0, st, m->g, m->table, m->pool, m->n_live, apart, bases, labels);
        hipLaunchKernelGGL(k_dsh_cc_flatten, dim3((unsigned)rank), dim3(kRankWords), 0, st, labels, nodes, t.rb, t.wr, t.cc);
        hipLaunchKernelGGL(k_dsh_cc_scan, dim3(1), dim3(kRankScanThreads), 0, st, (const uint32_t*)t.cc, t.co, rank, d_count);
        hipLaunchKernelGGL(k_dsh_cc_relabel, tile_grid, block, 0, st, m->pool, m->n_live, (uint32_t)cpc, tiles, bases, (const uint32_t*)labels, (const uint32_t*)t.rb,
                           (const uint32_t*)t.wr, (const uint32_t*)t.co);
        HIP_TRY(h, hipGetLastError());
        const hipError_t copied = hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, st);
        const hipError_t waited = hipStreamSynchronize(st);                     // (whatever the copy said: `count` is not left to a pending copy)
        HIP_TRY(h, copied);
        HIP_TRY(h, waited);
    }
    m->cc_count = count;
    m->cc_flags = flags;
    m->cc_valid = true;
    if (out_count) *out_count = count;
    return SDFGPU_OK;
}

int dsh_export_impl(sdfgpu_dsh_map_object* m, sdfgpu_dsh_chunk* d_chunks, int64_t chunk_capacity, void* d_cells, int64_t cell_capacity,
                    int64_t* out_chunks, int64_t* out_cells, hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (chunk_capacity < 0 || cell_capacity < 0 || (chunk_capacity > 0 && !d_chunks) || (cell_capacity > 0 && !d_cells))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: export: a capacity without a buffer");
    if (int rc = dsh_aligned8(h, d_chunks, "the chunk list")) return rc;
    if (int rc = dsh_aligned8(h, d_cells, "the cell list")) return rc;
    DshCall call{m, st};
    if (int rc = call.open()) return rc;
    uint64_t chunk_filled = 0, cell_filled = 0;
    if (int rc = dsh_count(m, &chunk_filled, &cell_filled, st)) return rc;
    const uint64_t cpc = (uint64_t)m->g.cells_per_chunk, total_cells = cell_filled * cpc;
    if (out_chunks) *out_chunks = (int64_t)m->n_live;
    if (out_cells) *out_cells = (int64_t)total_cells;
    if (!m->n_live || (uint64_t)chunk_capacity < m->n_live || (uint64_t)cell_capacity < total_cells) return SDFGPU_OK;
    uint32_t* slot_of_rank = nullptr;
    if (int rc = dsh_scratch(m, [&](DshCut& c) { slot_of_rank = c.take<uint32_t>((size_t)m->n_live * 4); })) return rc;
    hipLaunchKernelGGL(k_dsh_rank, dsh_grid((int64_t)m->n_live), dim3(kDshThreads), 0, st, m->pool.heads, (uint32_t)m->n_live, cpc, d_chunks, slot_of_rank);
    if (total_cells)
        hipLaunchKernelGGL(k_dsh_export_cells, dsh_chunk_grid(m->n_live), dim3(kDshThreads), 0, st, m->pool, m->n_live, cpc, d_chunks, slot_of_rank, static_cast<uint64_t*>(d_cells));
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// One removal on `st`: by list (d_loc, n) or, with `range`, by box.  Flag | count and read back | pair | move | rebuild the table.
int dsh_remove_impl(sdfgpu_dsh_map_object* m, const double* d_loc, int64_t n, const DshChunkRange* range, int invert, uint8_t* d_statuses,
                    int64_t* out_removed, hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (out_removed) *out_removed = 0;
    if (!range) {
        if (n < 0 || n >= kDshMaxBatch) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a batch holds 0 .. 2^31 - 1 operations (got %lld)", (long long)n);
        if (n == 0) return SDFGPU_OK;
        if (!d_loc) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null locations");
        if (int rc = dsh_aligned8(h, d_loc, "the locations")) return rc;
    }
    DshCall call{m, st};
    if (int rc = call.open()) return rc;

    const size_t live = (size_t)m->n_live, ops = range ? 0 : (size_t)n, tiles = (size_t)dsh_pair_tiles(m->n_live), half = live / 2 + 1;
    uint32_t *flags = nullptr, *op_slot = nullptr, *tile_counts = nullptr, *holes = nullptr, *movers = nullptr;
    if (int rc = dsh_scratch(m, [&](DshCut& c) {
            flags = c.take<uint32_t>(live * 4); op_slot = c.take<uint32_t>(ops * 4); tile_counts = c.take<uint32_t>(tiles * 8);
            holes = c.take<uint32_t>(half * 4); movers = c.take<uint32_t>(half * 4);
        })) return rc;
    uint32_t* const counters = dsh_counters(m);
    const dim3 block(kDshThreads), live_grid = dsh_grid((int64_t)live);
    const uint32_t n_live = (uint32_t)m->n_live;

    HIP_TRY(h, hipMemsetAsync(counters, 0, kDshCounterBytes, st));
    if (range) {
        if (live) hipLaunchKernelGGL(k_dsh_remove_box, live_grid, block, 0, st, m->pool.heads, n_live, *range, invert, flags);
    } else {
        if (live) HIP_TRY(h, hipMemsetAsync(flags, 0xFF, live * 4, st));
        hipLaunchKernelGGL(k_dsh_remove_stamp, dsh_grid(n), block, 0, st, m->g, m->table, d_loc, n, flags, op_slot);
        if (d_statuses) hipLaunchKernelGGL(k_dsh_remove_decide, dsh_grid(n), block, 0, st, flags, op_slot, n, d_statuses);
    }
    if (live) hipLaunchKernelGGL(k_dsh_remove_count, live_grid, block, 0, st, flags, n_live, counters);
    HIP_TRY(h, hipGetLastError());
    uint32_t removed = 0;
    HIP_TRY(h, hipMemcpyAsync(&removed, counters, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));                                       // the call's one synchronisation while nothing is lost
    if (removed == 0) return SDFGPU_OK;
    if (removed > n_live) return fail(h, SDFGPU_ERR_HIP, "dsh: %u of %u chunks flagged (internal error)", removed, n_live);
    const uint32_t keep = n_live - removed;
    m->cc_valid = false;
    if (keep) {
        hipLaunchKernelGGL(k_dsh_pair_count, dim3((unsigned)tiles), block, 0, st, flags, n_live, keep, tile_counts);
        hipLaunchKernelGGL(k_dsh_pair_scan, dim3(1), block, 0, st, tile_counts, (uint32_t)tiles, counters);
        hipLaunchKernelGGL(k_dsh_pair_list, dim3((unsigned)tiles), block, 0, st, flags, n_live, keep, tile_counts, holes, movers);
        hipLaunchKernelGGL(k_dsh_remove_move, dsh_chunk_grid(std::min(removed, keep)), block, 0, st, m->pool, (uint64_t)m->g.cells_per_chunk, holes, movers,
                           counters);
    }
    // linear probing has no parallel deletion: the table is made again from the heads that stay
    HIP_TRY(h, hipMemsetAsync(m->table.keys, 0xFF, (size_t)m->table_cap * 8, st));
    m->n_live = keep;
    if (out_removed) *out_removed = (int64_t)removed;
    if (!keep) return SDFGPU_OK;
    uint32_t lost = 0;
    if (int rc = dsh_rehash_into(m, m->table, keep, st, &lost)) return rc;    // (counters[1] is still the zero the call began with)
    HIP_TRY(h, hipStreamSynchronize(st));
    if (lost) return fail(h, SDFGPU_ERR_HIP, "dsh: the rehash lost %u keys (internal error)", lost);
    return SDFGPU_OK;
}

// shrink-to-fit: dsh_reserve_pool and dsh_reserve_table run downwards.  Both new allocations are made before anything is copied,
// so a failure leaves the map as it was; the mark plane is given up (dsh_reserve_marks makes it again).
int dsh_shrink_impl(sdfgpu_dsh_map_object* m, int64_t spare_chunks, hipStream_t st) {
    sdfgpu_handle h = m->h;
    if (spare_chunks < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: spare_chunks must not be negative (got %lld)", (long long)spare_chunks);
    DshCall call{m, st};
    if (int rc = call.open()) return rc;
    const uint64_t cpc = (uint64_t)m->g.cells_per_chunk;
    uint64_t pool_cap = 0, table_cap = 0;
    dsh_plan_shrink(m->n_live, (uint64_t)spare_chunks, m->pool_cap, m->table_cap, &pool_cap, &table_cap);
    DshTable table{};
    DshPool pool{};
    uint32_t lost = 0;
    int rc = SDFGPU_OK;
    if (table_cap < m->table_cap) rc = dsh_alloc_table(h, table_cap, table, st);
    if (rc == SDFGPU_OK && pool_cap < m->pool_cap) rc = dsh_alloc_pool(h, pool_cap, cpc, pool);
    if (rc == SDFGPU_OK) rc = [&]() -> int {
        if (table.keys && m->n_live) {
            HIP_TRY(h, hipMemsetAsync(dsh_counters(m), 0, kDshCounterBytes, st));
            if (int rc_rehash = dsh_rehash_into(m, table, m->n_live, st, &lost)) return rc_rehash;
        }
        if (pool.heads) if (int rc_copy = dsh_copy_pool(m, pool, st)) return rc_copy;
        HIP_TRY(h, hipStreamSynchronize(st));                                   // (what is replaced may still be read by pending work)
        if (lost) return fail(h, SDFGPU_ERR_HIP, "dsh: the rehash lost %u keys (internal error)", lost);
        return SDFGPU_OK;
    }();
    if (rc != SDFGPU_OK) {
        (void)hipStreamSynchronize(st);
        if (table.keys) (void)rz_free(h, table.keys);
        if (pool.heads) { (void)rz_free(h, pool.heads); (void)rz_free(h, pool.cells); }
        return rc;
    }
    if (table.keys) {
        (void)rz_free(h, m->table.keys);
        m->table = table;
        m->table_cap = table_cap;
    }
    if (pool.heads) {
        (void)rz_free(h, m->pool.heads);
        (void)rz_free(h, m->pool.cells);
        m->pool = pool;
        m->pool_cap = pool_cap;
    }
    if (m->marks) {
        (void)rz_free(h, m->marks);
        m->marks = nullptr;
        m->marks_cap = 0;
    }
    return SDFGPU_OK;
}

template <class Body>
int dsh_entry(sdfgpu_dsh_map m, void* stream, Body&& body) {
    if (dsh_check_map(m)) return SDFGPU_ERR_INVALID_ARGUMENT;
    return rz_wrap(m->h, stream, body);
}

// What a host form says about its arrays while dsh_staged lays the map's stage buffer out: in() and out() give the array's section
// (null for an absent array) and note the copy.
struct DshStaging {
    struct Copy { void* host; void* dev; size_t bytes; };
    DshCut* cut = nullptr;
    Copy ins[2], outs[2];
    int n_in = 0, n_out = 0;
    void* take(const void* host, size_t bytes, Copy* list, int& count) {
        void* const dev = cut->take<char>(bytes, host && bytes);
        if (dev) list[count++] = Copy{const_cast<void*>(host), dev, bytes};
        return dev;
    }
    template <class T> const T* in(const T* host, size_t bytes) { return static_cast<const T*>(take(host, bytes, ins, n_in)); }
    template <class T> T* out(T* host, size_t bytes) { return static_cast<T*>(take(host, bytes, outs, n_out)); }
};

// A host form on the null stream: behind the call before it (dsh_wait) the stage buffer is sized and cut as `layout` says, the inputs
// go up in the order they were named, `body` (the device form, on the staged arrays) runs, and the outputs come down in theirs.
template <class Layout, class Body>
int dsh_staged(sdfgpu_dsh_map_object* m, Layout&& layout, Body&& body) {
    sdfgpu_handle h = m->h;
    if (int rc = dsh_wait(m, nullptr)) return rc;
    DshStaging s;
    if (int rc = dsh_cut(h, m->stage, "dsh staging", 0, [&](DshCut& c) { s = DshStaging{}; s.cut = &c; layout(s); })) return rc;
    for (int k = 0; k < s.n_in; ++k) if (int rc = copy_from_host(h, s.ins[k].dev, s.ins[k].host, s.ins[k].bytes)) return rc;
    if (int rc = body()) return rc;
    for (int k = 0; k < s.n_out; ++k) if (int rc = copy_to_host(h, s.outs[k].host, s.outs[k].dev, s.outs[k].bytes)) return rc;
    return SDFGPU_OK;
}

int dsh_set_host(sdfgpu_dsh_map m, bool chunk_sets, const double* locations, int64_t n, const void* values, const void* one_value, uint8_t* statuses) {
    return dsh_entry(m, nullptr, [&]() -> int {
        if (n <= 0 || n >= kDshMaxBatch) return dsh_batch<double>(m, chunk_sets, nullptr, n, values, one_value, nullptr, nullptr);   // (its refusals, or nothing to do)
        if (!locations) return fail(m->h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null locations");
        const size_t un = (size_t)n;
        const double* d_loc = nullptr;
        const void* d_values = nullptr;
        uint8_t* d_statuses = nullptr;
        return dsh_staged(m, [&](DshStaging& s) { d_loc = s.in(locations, un * 24); d_values = s.in(values, un * 8); d_statuses = s.out(statuses, un); },
                          [&] { return dsh_batch<double>(m, chunk_sets, d_loc, n, d_values, one_value, d_statuses, nullptr); });
    });
}

// The host form of a frame: the points are staged, the statuses copied back.
int dsh_rays_host(sdfgpu_dsh_map m, const DshRayFrame& f, const float* points, int64_t n, const void* free_value, const void* hit_value, const DshFuse* fuse,
                  uint8_t* statuses, sdfgpu_dsh_ray_counts* out_counts) {
    if (n == 0) return dsh_rays_impl(m, f, nullptr, 0, free_value, hit_value, fuse, nullptr, out_counts, nullptr);
    if (!points) return fail(m->h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null points");
    const float* d_points = nullptr;
    uint8_t* d_statuses = nullptr;
    return dsh_staged(m, [&](DshStaging& s) { d_points = s.in(points, (size_t)n * 12); d_statuses = s.out(statuses, (size_t)n); },
                      [&] { return dsh_rays_impl(m, f, d_points, n, free_value, hit_value, fuse, d_statuses, out_counts, nullptr); });
}

// The host form of a cast: the points (12 bytes a ray), or the starts and the ends (24 each), are staged; statuses and hits copied back.
int dsh_cast_host(sdfgpu_dsh_map m, const DshRayFrame& f, bool segments, const void* first, const void* second, int64_t n, uint32_t flags, uint8_t* statuses,
                  sdfgpu_dsh_cast_hit* hits) {
    if (n == 0) return SDFGPU_OK;
    if (!first || (segments && !second)) return fail(m->h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a cast needs its %s", segments ? "starts and ends" : "points");
    const size_t un = (size_t)n, each = segments ? un * 24 : un * 12;
    const void *d_first = nullptr, *d_second = nullptr;
    uint8_t* d_statuses = nullptr;
    sdfgpu_dsh_cast_hit* d_hits = nullptr;
    return dsh_staged(m, [&](DshStaging& s) {
            d_first = s.in(first, each); d_second = s.in(segments ? second : nullptr, each);
            d_statuses = s.out(statuses, un); d_hits = s.out(hits, un * sizeof(sdfgpu_dsh_cast_hit));
        }, [&] {
            return dsh_cast_impl(m, f, segments, segments ? nullptr : static_cast<const float*>(d_first), segments ? static_cast<const double*>(d_first) : nullptr,
                                 static_cast<const double*>(d_second), n, flags, d_statuses, d_hits, nullptr);
        });
}

}  // namespace

extern "C" {

int sdfgpu_dsh_create(sdfgpu_handle h, const double inverse_origin[16], double cell_size, int64_t chunk_nx, int64_t chunk_ny, int64_t chunk_nz,
                      const void* default_cell, int64_t initial_chunks, uint64_t byte_limit, sdfgpu_dsh_map* out_map) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!out_map) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: out_map is null");
    *out_map = nullptr;
    if (!inverse_origin || !default_cell) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null pointer");
    if (!(cell_size > 0.0) || !std::isfinite(cell_size)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: cell_size must be positive and finite (got %g)", cell_size);
    if (chunk_nx < 1 || chunk_ny < 1 || chunk_nz < 1 || chunk_nx > kDshMaxChunkCells || chunk_ny > kDshMaxChunkCells || chunk_nz > kDshMaxChunkCells ||
        chunk_nx * chunk_ny * chunk_nz > kDshMaxChunkCells)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: chunk dimensions must be at least 1 with a product of at most 32768 (got %lld x %lld x %lld)",
                    (long long)chunk_nx, (long long)chunk_ny, (long long)chunk_nz);
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(inverse_origin[i])) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: the inverse origin transform is not finite");
    if (initial_chunks < 0 || initial_chunks >= kDshMaxBatch) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: initial_chunks out of range");
    return rz_wrap(h, nullptr, [&]() -> int {
        HIP_TRY(h, hipSetDevice(h->device));
        sdfgpu_dsh_map_object* m = new (std::nothrow) sdfgpu_dsh_map_object();
        if (!m) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "out of host memory");
        m->h = h;
        for (int i = 0; i < 12; ++i) m->g.inverse[i] = inverse_origin[i];
        m->g.inv_cell = 1.0 / cell_size;
        m->g.n[0] = chunk_nx; m->g.n[1] = chunk_ny; m->g.n[2] = chunk_nz;
        m->g.cells_per_chunk = chunk_nx * chunk_ny * chunk_nz;
        memcpy(&m->g.default_record, default_cell, 8);
        m->byte_limit = byte_limit;
        const uint64_t chunks = initial_chunks ? (uint64_t)initial_chunks : 64, table = dsh_table_capacity(chunks);
        int rc = SDFGPU_OK;
        if (byte_limit && dsh_table_bytes(table) + dsh_pool_bytes(chunks, (uint64_t)m->g.cells_per_chunk) > byte_limit)
            rc = fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dsh: a map of %llu chunks would pass its byte limit of %llu", (unsigned long long)chunks,
                      (unsigned long long)byte_limit);
        if (rc == SDFGPU_OK) rc = dsh_alloc_table(h, table, m->table, nullptr);
        if (rc == SDFGPU_OK) { m->table_cap = table; rc = dsh_alloc_pool(h, chunks, (uint64_t)m->g.cells_per_chunk, m->pool); }
        if (rc == SDFGPU_OK) { m->pool_cap = chunks; rc = ensure(h, m->scratch, kDshCounterBytes, "dsh batch scratch"); }
        if (rc == SDFGPU_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(h, SDFGPU_ERR_HIP, "dsh: clearing the table failed");
        if (rc != SDFGPU_OK) {
            if (m->table.keys) (void)rz_free(h, m->table.keys);
            if (m->pool.heads) { (void)rz_free(h, m->pool.heads); (void)rz_free(h, m->pool.cells); }
            delete m;
            return rc;
        }
        *out_map = m;
        return SDFGPU_OK;
    });
}

int sdfgpu_dsh_destroy(sdfgpu_dsh_map map) {
    if (!map) return SDFGPU_OK;
    sdfgpu_handle h = map->h;
    (void)hipSetDevice(h->device);
    (void)map->order.host_wait();
    for (void* p : {(void*)map->table.keys, (void*)map->pool.heads, (void*)map->pool.cells, map->scratch.ptr, map->stage.ptr, (void*)map->marks}) (void)rz_free(h, p);
    map->order.destroy();
    delete map;
    return SDFGPU_OK;
}

int sdfgpu_dsh_info(sdfgpu_dsh_map map, sdfgpu_dsh_counts* out_counts) {
    return dsh_entry(map, nullptr, [&]() -> int {
        sdfgpu_handle h = map->h;
        if (!out_counts) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: out_counts is null");
        DshCall call{map, nullptr};
        if (int rc = call.open()) return rc;
        sdfgpu_dsh_counts c{};
        if (int rc = dsh_count(map, &c.chunk_filled, &c.cell_filled, nullptr)) return rc;
        c.capacity_chunks = map->pool_cap;
        c.table_capacity = map->table_cap;
        c.bytes_held = dsh_bytes_held(map);
        c.scratch_bytes = map->scratch.bytes + map->stage.bytes + (map->marks ? dsh_mark_bytes(map->marks_cap, (uint64_t)map->g.cells_per_chunk) : 0);
        c.byte_limit = map->byte_limit;
        *out_counts = c;
        return SDFGPU_OK;
    });
}

int sdfgpu_dsh_set_cells_device(sdfgpu_dsh_map map, const double* d_locations, int64_t n, const void* d_values, const void* one_value,
                                uint8_t* d_statuses, void* stream) {
    return dsh_entry(map, stream, [&]() -> int { return dsh_batch<double>(map, false, d_locations, n, d_values, one_value, d_statuses, (hipStream_t)stream); });
}

int sdfgpu_dsh_set_chunks_device(sdfgpu_dsh_map map, const double* d_locations, int64_t n, const void* d_values, const void* one_value,
                                 uint8_t* d_statuses, void* stream) {
    return dsh_entry(map, stream, [&]() -> int { return dsh_batch<double>(map, true, d_locations, n, d_values, one_value, d_statuses, (hipStream_t)stream); });
}

int sdfgpu_dsh_insert_points_device(sdfgpu_dsh_map map, const float* d_points, int64_t n, const void* one_value, uint8_t* d_statuses, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        if (!one_value) return fail(map->h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: insert_points needs its one record");
        return dsh_batch<float>(map, false, d_points, n, nullptr, one_value, d_statuses, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_insert_rays_device(sdfgpu_dsh_map map, const double sensor[3], const float* d_points, int64_t n, double max_range, const void* free_value,
                                  const void* hit_value, uint8_t* d_statuses, sdfgpu_dsh_ray_counts* out_counts, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        DshRayFrame f{};
        if (int rc = dsh_carve_frame(map, sensor, n, max_range, free_value, hit_value, f)) return rc;
        return dsh_rays_impl(map, f, d_points, n, free_value, hit_value, nullptr, d_statuses, out_counts, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_fuse_rays_device(sdfgpu_dsh_map map, const double sensor[3], const float* d_points, int64_t n, double max_range,
                                const sdfgpu_dsh_sensor_model* model, uint8_t* d_statuses, sdfgpu_dsh_ray_counts* out_counts, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        DshRayFrame f{};
        DshFuse u{};
        if (int rc = dsh_fuse_model(map->h, model, u)) return rc;
        if (int rc = dsh_ray_frame(map, sensor, n, max_range, f)) return rc;
        return dsh_rays_impl(map, f, d_points, n, nullptr, nullptr, &u, d_statuses, out_counts, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_insert_rays(sdfgpu_dsh_map map, const double sensor[3], const float* points, int64_t n, double max_range, const void* free_value,
                           const void* hit_value, uint8_t* statuses, sdfgpu_dsh_ray_counts* out_counts) {
    return dsh_entry(map, nullptr, [&]() -> int {
        DshRayFrame f{};
        if (int rc = dsh_carve_frame(map, sensor, n, max_range, free_value, hit_value, f)) return rc;
        return dsh_rays_host(map, f, points, n, free_value, hit_value, nullptr, statuses, out_counts);
    });
}

int sdfgpu_dsh_fuse_rays(sdfgpu_dsh_map map, const double sensor[3], const float* points, int64_t n, double max_range,
                         const sdfgpu_dsh_sensor_model* model, uint8_t* statuses, sdfgpu_dsh_ray_counts* out_counts) {
    return dsh_entry(map, nullptr, [&]() -> int {
        DshRayFrame f{};
        DshFuse u{};
        if (int rc = dsh_fuse_model(map->h, model, u)) return rc;
        if (int rc = dsh_ray_frame(map, sensor, n, max_range, f)) return rc;
        return dsh_rays_host(map, f, points, n, nullptr, nullptr, &u, statuses, out_counts);
    });
}

int sdfgpu_dsh_set_cells(sdfgpu_dsh_map map, const double* locations, int64_t n, const void* values, const void* one_value, uint8_t* statuses) {
    return dsh_set_host(map, false, locations, n, values, one_value, statuses);
}

int sdfgpu_dsh_set_chunks(sdfgpu_dsh_map map, const double* locations, int64_t n, const void* values, const void* one_value, uint8_t* statuses) {
    return dsh_set_host(map, true, locations, n, values, one_value, statuses);
}

int sdfgpu_dsh_remove_chunks_device(sdfgpu_dsh_map map, const double* d_locations, int64_t n, uint8_t* d_statuses, int64_t* out_removed, void* stream) {
    return dsh_entry(map, stream, [&]() -> int { return dsh_remove_impl(map, d_locations, n, nullptr, 0, d_statuses, out_removed, (hipStream_t)stream); });
}

int sdfgpu_dsh_remove_chunks(sdfgpu_dsh_map map, const double* locations, int64_t n, uint8_t* statuses, int64_t* out_removed) {
    return dsh_entry(map, nullptr, [&]() -> int {
        sdfgpu_handle h = map->h;
        if (n <= 0 || n >= kDshMaxBatch) return dsh_remove_impl(map, nullptr, n, nullptr, 0, nullptr, out_removed, nullptr);
        if (!locations) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null locations");
        const double* d_loc = nullptr;
        uint8_t* d_statuses = nullptr;
        return dsh_staged(map, [&](DshStaging& s) { d_loc = s.in(locations, (size_t)n * 24); d_statuses = s.out(statuses, (size_t)n); },
                          [&] { return dsh_remove_impl(map, d_loc, n, nullptr, 0, d_statuses, out_removed, nullptr); });
    });
}

int sdfgpu_dsh_retain_box(sdfgpu_dsh_map map, const int64_t lower[3], const int64_t extent[3], int invert, int64_t* out_removed, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        sdfgpu_handle h = map->h;
        if (!lower || !extent) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: retain_box needs the box");
        if (!dsh_box_ok(lower, extent))
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: a box has |lower| <= 2^40 and 0 <= extent <= 2^40 on every axis");
        const DshChunkRange range = dsh_box_chunk_range(lower, extent, map->g.n);
        return dsh_remove_impl(map, nullptr, 0, &range, invert, nullptr, out_removed, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_shrink(sdfgpu_dsh_map map, int64_t spare_chunks, void* stream) {
    return dsh_entry(map, stream, [&]() -> int { return dsh_shrink_impl(map, spare_chunks, (hipStream_t)stream); });
}

int sdfgpu_dsh_get_device(sdfgpu_dsh_map map, const double* d_locations, int64_t n, void* d_records, uint8_t* d_statuses, void* stream) {
    return dsh_entry(map, stream, [&]() -> int { return dsh_get_impl(map, d_locations, n, d_records, d_statuses, (hipStream_t)stream); });
}

int sdfgpu_dsh_get(sdfgpu_dsh_map map, const double* locations, int64_t n, void* records, uint8_t* statuses) {
    return dsh_entry(map, nullptr, [&]() -> int {
        if (n <= 0 || n >= kDshMaxBatch || (!records && !statuses)) return dsh_get_impl(map, nullptr, n, records, statuses, nullptr);   // (its refusals, or nothing to do)
        if (!locations) return fail(map->h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: null locations");
        const size_t un = (size_t)n;
        const double* d_loc = nullptr;
        void* d_records = nullptr;
        uint8_t* d_statuses = nullptr;
        return dsh_staged(map, [&](DshStaging& s) { d_loc = s.in(locations, un * 24); d_records = s.out(records, un * 8); d_statuses = s.out(statuses, un); },
                          [&] { return dsh_get_impl(map, d_loc, n, d_records, d_statuses, nullptr); });
    });
}

int sdfgpu_dsh_cast_rays_device(sdfgpu_dsh_map map, const double sensor[3], const float* d_points, int64_t n, double max_range, uint32_t flags,
                                uint8_t* d_statuses, sdfgpu_dsh_cast_hit* d_hits, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        DshRayFrame f{};
        if (int rc = dsh_cast_frame(map, sensor, false, n, max_range, flags, d_statuses, d_hits, f)) return rc;
        return dsh_cast_impl(map, f, false, d_points, nullptr, nullptr, n, flags, d_statuses, d_hits, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_cast_segments_device(sdfgpu_dsh_map map, const double* d_starts, const double* d_ends, int64_t n, double max_range, uint32_t flags,
                                    uint8_t* d_statuses, sdfgpu_dsh_cast_hit* d_hits, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        DshRayFrame f{};
        if (int rc = dsh_cast_frame(map, nullptr, true, n, max_range, flags, d_statuses, d_hits, f)) return rc;
        return dsh_cast_impl(map, f, true, nullptr, d_starts, d_ends, n, flags, d_statuses, d_hits, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_cast_rays(sdfgpu_dsh_map map, const double sensor[3], const float* points, int64_t n, double max_range, uint32_t flags, uint8_t* statuses,
                         sdfgpu_dsh_cast_hit* hits) {
    return dsh_entry(map, nullptr, [&]() -> int {
        DshRayFrame f{};
        if (int rc = dsh_cast_frame(map, sensor, false, n, max_range, flags, statuses, hits, f)) return rc;
        return dsh_cast_host(map, f, false, points, nullptr, n, flags, statuses, hits);
    });
}

int sdfgpu_dsh_cast_segments(sdfgpu_dsh_map map, const double* starts, const double* ends, int64_t n, double max_range, uint32_t flags, uint8_t* statuses,
                             sdfgpu_dsh_cast_hit* hits) {
    return dsh_entry(map, nullptr, [&]() -> int {
        DshRayFrame f{};
        if (int rc = dsh_cast_frame(map, nullptr, true, n, max_range, flags, statuses, hits, f)) return rc;
        return dsh_cast_host(map, f, true, starts, ends, n, flags, statuses, hits);
    });
}

int sdfgpu_dsh_extract_window_device(sdfgpu_dsh_map map, const int64_t lower[3], int64_t nx, int64_t ny, int64_t nz, int unknown_is_filled,
                                     void* d_records, uint32_t* d_bits, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        if (int rc = dsh_check_window(map->h, lower, nx, ny, nz, d_records, d_bits)) return rc;
        return dsh_window_impl(map, lower, nx, ny, nz, unknown_is_filled, d_records, d_bits, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_extract_window(sdfgpu_dsh_map map, const int64_t lower[3], int64_t nx, int64_t ny, int64_t nz, int unknown_is_filled, void* records,
                              uint32_t* bits) {
    return dsh_entry(map, nullptr, [&]() -> int {
        sdfgpu_handle h = map->h;
        if (int rc = dsh_check_window(h, lower, nx, ny, nz, records, bits)) return rc;
        const size_t n = (size_t)nx * (size_t)ny * (size_t)nz, words = (n + 31) / 32;
        void* d_records = nullptr;
        uint32_t* d_bits = nullptr;
        return dsh_staged(map, [&](DshStaging& s) { d_records = s.out(records, n * 8); d_bits = s.out(bits, words * 4); },
                          [&] { return dsh_window_impl(map, lower, nx, ny, nz, unknown_is_filled, d_records, d_bits, nullptr); });
    });
}

int sdfgpu_dsh_frontier_window_device(sdfgpu_dsh_map map, const int64_t lower[3], int64_t nx, int64_t ny, int64_t nz, uint32_t flags, uint32_t* d_bits,
                                      void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        if (int rc = dsh_check_window(map->h, lower, nx, ny, nz, nullptr, d_bits)) return rc;
        if (int rc = dsh_check_frontier_flags(map->h, flags)) return rc;
        return dsh_frontier_window_impl(map, lower, nx, ny, nz, flags, d_bits, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_frontier_window(sdfgpu_dsh_map map, const int64_t lower[3], int64_t nx, int64_t ny, int64_t nz, uint32_t flags, uint32_t* bits) {
    return dsh_entry(map, nullptr, [&]() -> int {
        if (int rc = dsh_check_window(map->h, lower, nx, ny, nz, nullptr, bits)) return rc;
        if (int rc = dsh_check_frontier_flags(map->h, flags)) return rc;
        const size_t words = ((size_t)nx * (size_t)ny * (size_t)nz + 31) / 32;
        uint32_t* d_bits = nullptr;
        return dsh_staged(map, [&](DshStaging& s) { d_bits = s.out(bits, words * 4); },
                          [&] { return dsh_frontier_window_impl(map, lower, nx, ny, nz, flags, d_bits, nullptr); });
    });
}

int sdfgpu_dsh_frontier_cells_device(sdfgpu_dsh_map map, const int64_t lower[3], const int64_t extent[3], uint32_t flags, int64_t* d_cells,
                                     int64_t capacity, int64_t* out_total, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        DshFrontierBox box{};
        if (int rc = dsh_frontier_cells_check(map, lower, extent, flags, d_cells, capacity, out_total, box)) return rc;
        return dsh_frontier_cells_impl(map, box, flags, d_cells, capacity, out_total, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_frontier_cells(sdfgpu_dsh_map map, const int64_t lower[3], const int64_t extent[3], uint32_t flags, int64_t* cells, int64_t capacity,
                              int64_t* out_total) {
    return dsh_entry(map, nullptr, [&]() -> int {
        DshFrontierBox box{};
        if (int rc = dsh_frontier_cells_check(map, lower, extent, flags, cells, capacity, out_total, box)) return rc;
        if (int rc = dsh_wait(map, nullptr)) return rc;
        if (int rc = dsh_frontier_cells_impl(map, box, flags, nullptr, 0, out_total, nullptr)) return rc;
        const int64_t total = *out_total;
        if (total == 0 || capacity < total) return SDFGPU_OK;
        int64_t* d_cells = nullptr;
        return dsh_staged(map, [&](DshStaging& s) { d_cells = s.out(cells, (size_t)total * 24); },
                          [&] { return dsh_frontier_cells_impl(map, box, flags, d_cells, total, out_total, nullptr); });
    });
}

int sdfgpu_dsh_update_components(sdfgpu_dsh_map map, uint32_t flags, uint32_t* out_count, void* stream) {
    return dsh_entry(map, stream, [&]() -> int { return dsh_components_impl(map, flags, out_count, (hipStream_t)stream); });
}

int sdfgpu_dsh_components_info(sdfgpu_dsh_map map, uint32_t* out_count, uint32_t* out_flags, int* out_valid) {
    if (dsh_check_map(map)) return SDFGPU_ERR_INVALID_ARGUMENT;                // (the host's record of the map: no GPU call)
    if (out_count) *out_count = map->cc_count;
    if (out_flags) *out_flags = map->cc_flags;
    if (out_valid) *out_valid = map->cc_valid ? 1 : 0;
    return SDFGPU_OK;
}

int sdfgpu_dsh_export_device(sdfgpu_dsh_map map, sdfgpu_dsh_chunk* d_chunks, int64_t chunk_capacity, void* d_cells, int64_t cell_capacity,
                             int64_t* out_chunks, int64_t* out_cells, void* stream) {
    return dsh_entry(map, stream, [&]() -> int {
        return dsh_export_impl(map, d_chunks, chunk_capacity, d_cells, cell_capacity, out_chunks, out_cells, (hipStream_t)stream);
    });
}

int sdfgpu_dsh_export(sdfgpu_dsh_map map, sdfgpu_dsh_chunk* chunks, int64_t chunk_capacity, void* cells, int64_t cell_capacity, int64_t* out_chunks,
                      int64_t* out_cells) {
    return dsh_entry(map, nullptr, [&]() -> int {
        sdfgpu_handle h = map->h;
        if (chunk_capacity < 0 || cell_capacity < 0 || (chunk_capacity > 0 && !chunks) || (cell_capacity > 0 && !cells))
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "dsh: export: a capacity without a buffer");
        if (int rc = dsh_wait(map, nullptr)) return rc;
        int64_t n_chunks = 0, n_cells = 0;
        if (int rc = dsh_export_impl(map, nullptr, 0, nullptr, 0, &n_chunks, &n_cells, nullptr)) return rc;
        if (out_chunks) *out_chunks = n_chunks;
        if (out_cells) *out_cells = n_cells;
        if (n_chunks == 0 || chunk_capacity < n_chunks || cell_capacity < n_cells) return SDFGPU_OK;
        sdfgpu_dsh_chunk* d_chunks = nullptr;
        void* d_cells = nullptr;
        return dsh_staged(map, [&](DshStaging& s) { d_chunks = s.out(chunks, (size_t)n_chunks * sizeof(sdfgpu_dsh_chunk)); d_cells = s.out(cells, (size_t)n_cells * 8); },
                          [&] { return dsh_export_impl(map, d_chunks, n_chunks, d_cells, n_cells, nullptr, nullptr, nullptr); });
    });
}

}  // extern "C"
