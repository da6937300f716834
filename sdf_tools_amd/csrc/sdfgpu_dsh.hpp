// sdfgpu_dsh.hpp -- the chunk-hashed sparse collision map (include/sdfgpu.h "Dynamic spatial hashed map"): its
// constants, the packing of a chunk coordinate into a table key, the hash, and the planning of the table's and the pool's sizes.
// Plain C++ without a HIP header, as sdfgpu_plan.hpp and sdfgpu_policy.hpp are: sdfgpu_dsh.hip includes it for its kernels and its host
// code, and tests/dsh_plan_harness.cpp drives the arithmetic on the CPU under -fsanitize=address,undefined.
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
constexpr uint32_t kDshTouched = 0x80000000u;              // set in a chunk's state word between k_dsh_touch and k_dsh_expand only
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

constexpr int kDshThreads = 256;
constexpr int64_t kDshGridX = 1 << 20;    // workgroups per grid row (a launch dimension takes fewer than 2^32 threads)

}  // namespace sdfgpu
