// sdfgpu_surfaces.hpp -- the surface voxels of every connected component, grouped by component (CollisionMapGrid /
// TaggedObjectCollisionMapGrid::ExtractComponentSurfaces, reference src/sdf_tools/collision_map.cpp:697-754,
// tagged_object_collision_map.cpp:492-550), the interface between the kernels in sdfgpu_surfaces.hip and the host code at the end
// of that file (which owns the scratch and the ordering).
//
// Contract (include/sdfgpu.h "Component surfaces"): voxel v of label c is REPORTED iff it is selected and one of its six face
// neighbours has another label (out-of-grid voxels are component -1).  Result: per-label counts, and the reported indices
// grouped by ascending label, ascending inside each group.  Launches:
//   k_sf_flag    one lane per voxel, kSfTile voxels per workgroup: the six comparisons, the label check, the surface bit words
//                (one ballot per wave = two words), per-label counts pre-reduced in the wave, then in a per-workgroup LDS table
//                (one global atomic per label and workgroup), the workgroup's reported total (one atomic)
//   -- the host reads the total and the error words, refuses, sizes the sort buffers; a counts-only call ends here --
//   then a stable least-significant-digit radix sort of the reported voxels on their label, kSfDigitBits bits per pass, over the
//   ceil(log2(max_label + 1)) bits that exist (at least one pass: with no bits it is a plain ordered compaction).  Per pass:
//   k_sf_hist    one wave per tile: digit histogram -> table[digit][tile]
//   k_sf_scan_*  exclusive scan of the table (segment sums, one workgroup over the sums, segment scans)
//   k_sf_scatter one wave per tile, 64 elements a round in tile order: rank among the wave's lanes of the same digit (one ballot
//                per digit bit), the digit's running offset in LDS -> destination
//   The first pass reads the surface bit words and the labels (tile = kSfTile voxels: no separate compaction), the later ones
//   the (label, index) pairs of the pass before; the last pass stores indices only, into the caller's buffer.
// Voxel indices are uint64 wherever they are formed; counts, offsets and the total fit uint32 (at most 2^32 - 1 voxels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfgpu {

constexpr int kSfTile = 4096;                  // voxels per k_sf_flag workgroup; elements per sort tile
constexpr int kSfDigitBits = 8;
constexpr int kSfScanSeg = 2048;               // table entries per k_sf_scan_* workgroup
constexpr uint32_t kSfErrLabel = 1u;           // status err flag: a label above max_label

struct SfStatus {
    uint64_t total;                            // reported voxels
    uint32_t err, label_over;                  // one offending label (the largest)
};

struct SfPlan {
    int64_t nx = 0, ny = 0, nz = 0;
    uint64_t n = 0;                            // voxels
    uint64_t tiles = 0;                        // ceil(n / kSfTile)
    uint32_t max_label = 0;
    int label_bits = 0;                        // ceil(log2(max_label + 1))
    int passes = 1;                            // max(1, ceil(label_bits / kSfDigitBits))
    // scratch layout (bytes): counts u32 [max_label + 1] | status | surface bit words u32 [tiles * kSfTile / 32]
    size_t off_status = 0, off_bits = 0;
    size_t zero_bytes = 0;                     // counts and status: zeroed at the start of every call
    size_t scratch_bytes = 0;
};

// sort scratch for `total` reported voxels: pairs A | pairs B (uint2 [total] each, only when passes > 1) | table u32 | segment sums u32
struct SfSortPlan {
    uint64_t total = 0;
    uint64_t table_entries = 0;                // the largest pass's digits x tiles
    size_t off_b = 0, off_table = 0, off_sums = 0;
    size_t bytes = 0;
};

SfPlan sf_plan(int64_t nx, int64_t ny, int64_t nz, uint32_t max_label);
SfSortPlan sf_sort_plan(const SfPlan& p, uint64_t total);

// d_labels: n uint32 [nx][ny][nz]; d_select: ceil(n / 32) words or nullptr (every voxel selected); d_user_bits: ceil(n / 32)
// words or nullptr.  Zeroes the counts and the status, runs k_sf_flag on `s`; the SfStatus at plan.off_status and the counts at
// offset 0 are then valid.
hipError_t sf_launch_flag(const SfPlan& p, const uint32_t* d_labels, const uint32_t* d_select, uint32_t* d_user_bits, void* d_scratch,
                          hipStream_t s);
// After sf_launch_flag, with no refusal: d_indices holds at least `total` uint32; d_sort sf_sort_plan(p, total).bytes.
hipError_t sf_launch_sort(const SfPlan& p, const SfSortPlan& sp, const uint32_t* d_labels, const void* d_scratch, void* d_sort,
                          uint32_t* d_indices, hipStream_t s);


// ---- the scan and the sort on their own (sdfgpu_display.hpp: the display export compacts and groups with them) ---------------------
// In-place exclusive scan of `entries` uint32 on `s`; d_sums: ceil(entries / kSfScanSeg) words of scratch.
void sf_launch_scan(uint32_t* d_table, uint64_t entries, uint32_t* d_sums, hipStream_t s);

// The later passes of the sort without the first: `total` (key, index) pairs that stand in index order at the start of d_sort are
// ordered stably on key bits [0, key_bits), key_bits >= 1 (keys must agree in every bit above).  Scratch: pairs A | pairs B |
// table | segment sums.  The last pass stores the indices into d_indices and the keys into d_keys (both hold `total`).
struct SfPairSortPlan {
    uint64_t total = 0;
    int passes = 0;                            // ceil(key_bits / kSfDigitBits)
    size_t off_b = 0, off_table = 0, off_sums = 0;
    size_t bytes = 0;
};
SfPairSortPlan sf_pair_sort_plan(uint64_t total, int key_bits);
hipError_t sf_launch_sort_pairs(const SfPairSortPlan& sp, int key_bits, void* d_sort, uint32_t* d_indices, uint32_t* d_keys, hipStream_t s);

}  // namespace sdfgpu
