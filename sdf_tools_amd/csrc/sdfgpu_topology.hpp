// sdfgpu_topology.hpp -- holes and voids of every connected component (CollisionMapGrid::ComputeComponentTopology, reference
// src/sdf_tools/collision_map.cpp:620-671 over topology_computation.hpp:297-672), the interface between the kernels in
// sdfgpu_topology.hip and the host code at the end of that file (which owns the scratch, the node buffer and the ordering).
//
// Contract (include/sdfgpu.h "Component topology"): vertex (i, j, k), 0 <= i <= nx ..., is the corner of the voxels
// (i-1..i, j-1..j, k-1..k), its cube, slot s = 4 dx + 2 dy + dz; out-of-grid voxels are component -1.  A NODE is a pair
// (vertex, label c) such that the cube holds a selected voxel of c with a face neighbour inside the cube whose label is not c;
// it is stored as bit s of the vertex's node byte, s being c's first slot in the cube.  Launches:
//   k_tp_vertex  one lane per vertex: node byte, 6-bit edge masks -> per-label counts (vertices, M3, M5, M6) pre-reduced in the
//                wave, then in a per-workgroup LDS table (one global atomic per label and workgroup: a room's free space or a
//                percolating Bernoulli component is one label for most of the grid); the label / selection checks; the node
//                bytes' running counts inside the workgroup's chunk of kTpChunk vertices
//   k_tp_scan    exclusive scan of the chunk counts (one workgroup) and the node total (uint64): sdfgpu_unionfind.hpp's scan
//   -- the host reads the total and the error words, refuses, sizes the node buffer --
//   k_tp_link    one lane per vertex: every exposed +x / +y / +z edge of a node joins it with the node of the same label at the
//                far vertex (the global union-find of sdfgpu_unionfind.hpp, a root's word being 0xFFFFFFFF)
//   k_tp_roots   per-label count of the union-find roots = surfaces
// Node id of (v, slot s) = co[chunk] + gb[v / 8] + popcount of the node bits of vertices 8 (v / 8) .. v - 1 and of v's bits below s.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfgpu {

constexpr int kTpChunk = 8192;                 // vertices per k_tp_vertex workgroup (32 rounds of 256)
constexpr int kTpCounters = 5;                 // per label: surface vertices, M3, M5, M6, surfaces
constexpr uint32_t kTpErrLabel = 1u;           // status err flag: a label above max_label
constexpr uint32_t kTpErrMixed = 2u;           // status err flag: a label with selected and unselected voxels

struct TpPlan {
    int64_t nx = 0, ny = 0, nz = 0;
    uint64_t nv = 0;                           // vertices (nx + 1)(ny + 1)(nz + 1)
    uint64_t chunks = 0;                       // ceil(nv / kTpChunk)
    uint32_t max_label = 0;
    bool select = false;
    // scratch layout (bytes): counters u64 [(max_label + 1) * 5] | status u64 [2] (node total; err flags, 0) | err labels u32 [2]
    // (over max_label, mixed) | selection flags u32 [max_label + 1] | node bytes u8 [chunks * kTpChunk] | gb u32 [chunks * kTpChunk / 8]
    // | chunk counts u32 [chunks] | chunk offsets u32 [chunks]
    size_t off_status = 0, off_flags = 0, off_nm = 0, off_gb = 0, off_cc = 0, off_co = 0;
    size_t zero_bytes = 0;                     // counters .. selection flags: zeroed at the start of every call
    size_t scratch_bytes = 0;
};

struct TpStatus {
    uint64_t nodes;
    uint32_t err, pad;
    uint32_t label_over, label_mixed;          // one offending label of each kind (the largest)
};

TpPlan tp_plan(int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, bool select);

// d_labels: n uint32 [nx][ny][nz]; d_select: ceil(n / 32) words or nullptr (every voxel selected).  Zeroes the counters, runs
// k_tp_vertex and k_tp_scan on `s`; the TpStatus at plan.off_status is then valid.
hipError_t tp_launch_count(const TpPlan& p, const uint32_t* d_labels, const uint32_t* d_select, void* d_scratch, hipStream_t s);
// After tp_launch_count, with no refusal: d_nodes holds status.nodes uint32 (its contents are overwritten).  Runs the
// union-find and the root count; the counters at offset 0 of the scratch are then final.
hipError_t tp_launch_surfaces(const TpPlan& p, const uint32_t* d_labels, void* d_scratch, uint32_t* d_nodes, uint64_t nodes, hipStream_t s);

}  // namespace sdfgpu
