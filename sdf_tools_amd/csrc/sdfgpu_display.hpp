// sdfgpu_display.hpp -- the display export of the grid classes and the SDF (the reference's ExportForDisplay family,
// src/sdf_tools/collision_map.cpp, tagged_object_collision_map.cpp, sdf.cpp): which voxels are drawn, in which order, where and in
// which colour.  The interface between the kernels in sdfgpu_display.hip and the host code at the end of that file (which owns the scratch and
// reads the status words back).  Contract: include/sdfgpu.h "Display export", DESIGN.md section 23.  Launches:
//   k_dp_select  one lane per voxel, kDpTile voxels per workgroup: the rule (drawn?, key), one ballot per wave = two bit words, the
//                workgroup's count -> tile_counts[tile], one atomic each for the total and the smallest / largest drawn key
//   -- the host reads the status words, refuses a short buffer, sizes the sort buffers; a count-only call ends here --
//   sf_launch_scan   (sdfgpu_surfaces.hpp) exclusive scan of the tile counts
//   k_dp_compact four waves per tile: the tile's 64 bit words scanned in the wave, then 64 voxels a round: rank = popcount of the lower
//                drawn lanes -> (index, key) in scan order, into the caller's arrays or, when a sort follows, into its pair buffer
//   sf_launch_sort_pairs   (sdfgpu_surfaces.hpp) the stable radix sort of section 19 on the key bits in which the drawn keys differ
//   group boundaries: k_dp_select<kDpRuleGroupStart> over the sorted keys (element i starts a group iff i = 0 or its key differs
//                from the one before), scan, k_dp_compact -> group offsets and group keys: the same three steps once more
//   k_dp_contour the object contours (kDpRuleContour) under k_dp_select's output contract: a wave round holds 64
//                consecutive z cells; each lane loads the record at its own z of the nine (dx, dy) rows and takes z - 1 / z + 1 from
//                the lanes beside it
//   k_dp_expand  indices (+ keys) -> points (3 doubles) and colours (4 floats) per element
//   k_dp_minmax, k_dp_sdf_colors   the SDF colour map
// Voxel indices are uint64 wherever they are formed; counts, offsets and totals fit uint32 (at most 2^32 - 1 voxels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdfgpu_surfaces.hpp"

namespace sdfgpu {

constexpr int kDpTile = kSfTile;               // voxels per k_dp_select and k_dp_compact workgroup: the sort's tile
constexpr int kDpScanSeg = kSfScanSeg;         // tile counts per workgroup of the scan

constexpr int kDpRuleOccupancy = 0;            // SDFGPU_DISPLAY_OCCUPANCY
constexpr int kDpRuleKeyField = 1;             // SDFGPU_DISPLAY_KEY_FIELD
constexpr int kDpRuleSdfNonPositive = 2;       // sdfgpu_display_select_sdf*
constexpr int kDpRuleGroupStart = 3;           // internal: first elements of the runs of a sorted key array
constexpr int kDpRuleContour = 4;              // sdfgpu_display_select_contour*: k_dp_contour

constexpr int kDpKeyZero = 0, kDpKeyWord = 1, kDpKeyClass = 2;   // how k_dp_compact finds an element's key again

struct DpStatus {                              // zeroed at the start of every call
    uint32_t total;                            // drawn voxels
    uint32_t groups;                           // distinct keys among them (grouped form)
    uint32_t key_max, key_inv_max;             // largest drawn key; largest ~key = ~(smallest drawn key)
    uint32_t pos_bits, neg_bits;               // SDF colour map: bits of the largest d > 0 / of the largest -d with d < 0 (0: none)
    uint32_t pad[2];
};

struct DpSource {                              // records of `stride` bytes; every field is a 4-byte word at its offset
    const char* cells = nullptr;
    uint64_t stride = 0;
    uint32_t occ_off = 0, key_off = 0;
};

struct DpSelect {
    DpSource src;
    uint32_t class_mask = 7;                   // bit 0 F (occ > 0.5), bit 1 E (occ < 0.5), bit 2 U and NaN
    int surface_only = 0;
    int draw_zero = 1;
    const uint32_t* draw_keys = nullptr;       // device, ascending
    uint32_t n_draw = 0;
    int filter = 0;                            // draw_keys given (an empty list draws nothing)
    uint32_t nx = 0, ny = 0, nz = 0;
    uint64_t n = 0;
    uint32_t* bits = nullptr;                  // tiles * kDpTile / 32 words
    uint32_t* tile_counts = nullptr;           // tiles
    uint32_t* total = nullptr;                 // DpStatus::total or ::groups
    uint32_t* key_max = nullptr;               // DpStatus::key_max (key_inv_max follows it) or nullptr
    int reach = 0;                             // kDpRuleContour: the largest squared offset (0 .. 3) at which a foreign cell draws
    int unknown_is_filled = 0;                 // kDpRuleContour: occ == 0.5 counts as filled
};

struct DpCompact {
    DpSource src;
    int key_mode = kDpKeyZero;
    uint64_t n = 0;
    const uint32_t* bits = nullptr;            // (8-byte aligned: read as 64-bit words)
    const uint32_t* tile_offsets = nullptr;    // the scanned tile counts
    uint64_t capacity = 0;                     // nothing is stored at or past it
    uint32_t* idx = nullptr;                   // either idx (+ keys, optional)
    uint32_t* keys = nullptr;
    uint2* pairs = nullptr;                    // or (key, index) pairs for sf_launch_sort_pairs
};

struct DpExpand {
    const uint32_t* idx = nullptr;
    const uint32_t* keys = nullptr;            // nullptr: every key is 0
    uint64_t count = 0;
    uint32_t ny = 0, nz = 0;
    double cell[3] = {0.0, 0.0, 0.0};
    uint32_t* points = nullptr;                // 3 doubles per element, stored as 6 words (the caller's pointer is 4-byte aligned)
    float* colors = nullptr;                   // 4 floats per element or nullptr
    const float* table = nullptr;              // table_len rgba entries
    uint32_t table_len = 0;
    float fallback[4] = {0.0f, 0.0f, 0.0f, 0.0f};
};

inline uint64_t dp_tiles(uint64_t n) { return (n + kDpTile - 1) / kDpTile; }

hipError_t dp_launch_select(int rule, const DpSelect& a, hipStream_t s);
hipError_t dp_launch_compact(const DpCompact& a, hipStream_t s);
hipError_t dp_launch_expand(const DpExpand& a, hipStream_t s);
// pos_bits / neg_bits of `st` (zeroed by the caller) from n floats; then one rgba per voxel from them
hipError_t dp_launch_minmax(const float* d_sdf, uint64_t n, DpStatus* st, hipStream_t s);
hipError_t dp_launch_sdf_colors(const float* d_sdf, uint64_t n, float alpha, const DpStatus* st, float* d_colors, hipStream_t s);

}  // namespace sdfgpu
