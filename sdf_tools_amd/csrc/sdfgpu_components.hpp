// sdfgpu_components.hpp -- connected components of a two-class occupancy grid (CollisionMapGrid::UpdateConnectedComponents,
// reference src/sdf_tools/collision_map.cpp:564-618 over topology_computation.hpp:25-150), the interface between the kernels in
// sdfgpu_components.hip and the host code at the end of that file (which owns the scratch and the ordering).
//
// Contract: a voxel's class is its bit of the linear bit field (bit v & 31 of word v >> 5); two voxels are in one component iff a
// path of face neighbours of their class joins them; components are numbered 1..K by their minimum linear index (the reference's
// x -> y -> z scan meets a component first at that voxel).  Four launches plus a one-block scan:
//   k_cc_local    one workgroup per tile (tx x ty x tz voxels, at most 16384): z runs from the bit words, union-find in LDS on
//                 the y / x faces inside the tile, provisional label = global index of the tile-local minimum
//   k_cc_merge    the tile faces: global union-find on the label words (sdfgpu_unionfind.hpp: larger root under smaller)
//   k_cc_flatten  every label -> its root (= the component's minimum index); root flags as bits, per-word ranks inside a chunk
//   k_cc_scan     exclusive scan of the chunk counts (one workgroup) and K
//   k_cc_relabel  label = rank of its root among the roots + 1
// (the last three are the root ranking of sdfgpu_unionfind.hpp, which also lays out its tables in the scratch)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfgpu {

constexpr int kCcTileVoxels = 16384;    // LDS labels of one k_cc_local tile (64 KiB)

struct CcPlan {
    int64_t nx = 0, ny = 0, nz = 0;     // the grid with singleton axes moved to the front (same linear layout, same adjacency)
    int tx = 0, ty = 0, tz = 0;         // tile extents; tz a multiple of 32
    int64_t ntx = 0, nty = 0, ntz = 0;  // tiles per axis
    uint64_t n = 0;                     // voxels (< 2^32)
    uint64_t chunks = 0;                // k_cc_flatten's chunks of 8192 voxels (kRankChunk, sdfgpu_unionfind.hpp)
    size_t scratch_bytes = 0;           // the rank tables of `chunks` chunks (root bits, word ranks, chunk counts, offsets) + K
};

// nx, ny, nz: positive, nx * ny * nz < 2^32 (checked by the caller)
CcPlan cc_plan(int64_t nx, int64_t ny, int64_t nz);

// d_bits: ceil(n / 32) words; d_labels: n words; d_scratch: plan.scratch_bytes, 4-byte aligned.  Enqueued on `s`; K lands in
// the word behind the rank tables (cc_count_word).
hipError_t cc_launch(const CcPlan& p, const uint32_t* d_bits, uint32_t* d_labels, void* d_scratch, hipStream_t s);
uint32_t* cc_count_word(const CcPlan& p, void* d_scratch);

}  // namespace sdfgpu
