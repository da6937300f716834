// sdfgpu_convex.hpp -- local extrema maps (SignedDistanceField::ComputeLocalExtremaMap, reference src/sdf_tools/sdf.cpp:23-207)
// and convex segments (TaggedObjectCollisionMapGrid::UpdateConvexSegments, tagged_object_collision_map.cpp:552-654), the interface
// between the kernels in sdfgpu_convex.hip and the host code at the end of that file (which owns the scratch and the ordering;
// the SDF build is sdfgpu.hip's).
//
// Contract (include/sdfgpu.h "Local extrema and convex segments"): next(v) is the cell the reference's walk steps to from v (v itself
// when no axis steps, kCxOff when the step leaves the grid); the extremum of v is the terminal of its forward orbit (a fixed point,
// or kCxOff) or, for an orbit that ends in a cycle C, the first node of C on the orbit of the minimum-index voxel of C's basin.
// Launches:
//   k_cx_next     one lane per voxel: gradient (gradient_one), rotation, step -> next[v]; the doubling state S_0
//   k_cx_round    pointer doubling, one launch per round: S = (p_k(v), m_k(v)) packed in a uint64; a node resolves when the node
//                 2^k ahead, or the successor of the minimum of its window, is resolved, or when the cycle test
//                 m_k(next(c)) == c holds for c = m_k(p_k(v)); the host reads each round's count of unresolved nodes
//   k_cx_basin    every cycle-bound voxel: atomicMin of its index into the slot of its cycle (indexed by the cycle's minimum)
//   k_cx_entry    one lane per cycle: marks the cycle's nodes, walks next from the basin minimum to the first marked node
//   k_cx_final    extremum index per voxel
// Segments:
//   k_cx_key      per voxel (object id, extremum or kCxOff when the cell does not take part)
//   k_cx_uf_init  union-find labels: the start of the voxel's run of joined z neighbours inside its wave
//   k_cx_uf_link  global union-find over the remaining joined face pairs (sdfgpu_unionfind.hpp, as k_cc_merge)
//   k_cx_flatten / k_cx_scan / k_cx_relabel   roots of taking-part cells -> 1..K in scan order, everything else 0 (the root
//                 ranking of sdfgpu_unionfind.hpp)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfgpu {

constexpr uint32_t kCxOff = 0xFFFFFFFFu;       // "the walk leaves the grid"; also the extremum index of such a voxel
constexpr int kCxMaxRounds = 40;               // > ceil(log2(2^32)) + 1

struct CxRot {
    double q[4], qi[4];                        // (w, x, y, z) of the origin rotation and of its inverse (eigen_lite arithmetic)
};

// Counters that every workgroup adds to are spread over kCxSpread slots, one 128-byte line each (a single word took one
// same-address atomic per wave: 2 M of them at 512^3, about 24 ms per doubling round); a total is the sum of a row's slots.
constexpr int kCxSpread = 64;
constexpr int kCxLine = 32;                    // words per slot

struct CxStats {
    uint32_t open[kCxMaxRounds][kCxSpread * kCxLine];   // nodes still unresolved after round k
    uint32_t cycles[kCxSpread * kCxLine];               // cycles (of length >= 2) found
    uint32_t longest_cycle[kCxLine];                    // [0]: nodes of the longest cycle
    uint32_t longest_entry[kCxLine];                    // [0]: steps of the longest basin-minimum -> cycle walk
    uint32_t count[kCxLine];                            // [0]: K of the segments
};

inline uint32_t cx_row_sum(const uint32_t* row) {
    uint32_t s = 0;
    for (int i = 0; i < kCxSpread; ++i) s += row[i * kCxLine];
    return s;
}

struct CxPlan {
    int64_t nx = 0, ny = 0, nz = 0;
    uint64_t n = 0;                            // voxels (<= 2^32 - 3: indices stay below the doubling markers)
    uint64_t chunks = 0;                       // k_cx_flatten's chunks of 8192 voxels (kRankChunk, sdfgpu_unionfind.hpp)
    // scratch layout (bytes): A u64 [n] | B u64 [n] | next u32 [n] | pad | stats | the rank tables of `chunks` chunks (root bits
    // u32 [chunks * 256] | word ranks u32 [chunks * 256] | chunk counts u32 [chunks] | chunk offsets u32 [chunks])
    size_t off_b = 0, off_next = 0, off_stats = 0, off_ranks = 0;
    size_t scratch_bytes = 0;
};

// nx, ny, nz positive, nx * ny * nz <= 2^32 - 3 (checked by the caller)
CxPlan cx_plan(int64_t nx, int64_t ny, int64_t nz);

// d_sdf: n floats [nx][ny][nz]; d_ext: n uint32 out.  Enqueued on `s`, with one synchronisation per doubling round (the host
// reads the round's unresolved count); on return the extremum indices are complete in stream order and *rounds holds the rounds
// used.
// The CxStats at plan.off_stats are valid once `s` has drained.
hipError_t cx_extrema(const CxPlan& p, const float* d_sdf, double res, const CxRot& rot, uint32_t* d_ext, void* d_scratch,
                      hipStream_t s, int* rounds);

// d_ext: the extremum indices; d_cells: n records of `stride` bytes (float occupancy at occ_off, uint32 object id at obj_off);
// d_labels: n uint32 out (segments 1..K, 0 for cells that take no part).  Enqueued on `s`; K lands in CxStats::count.
hipError_t cx_segments(const CxPlan& p, const uint32_t* d_ext, const char* d_cells, size_t stride, size_t occ_off, size_t obj_off,
                       double res, double threshold, uint32_t* d_labels, void* d_scratch, hipStream_t s);

// ExtractFreeAndNamedObjectsSignedDistanceField's combine, in place in `free_sdf`: free >= 0 -> free; named <= -0 -> named; else 0
hipError_t cx_combine(float* free_sdf, const float* named_sdf, uint64_t n, hipStream_t s);

}  // namespace sdfgpu
