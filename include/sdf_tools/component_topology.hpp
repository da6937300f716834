// component_topology -- the shared body of CollisionMapGrid / TaggedObjectCollisionMapGrid::ComputeComponentTopology (reference
// src/sdf_tools/collision_map.cpp:620-671, tagged_object_collision_map.cpp:424-490): the per-label counters come from the GPU
// (sdfgpu_component_topology_cells, include/sdfgpu.h "Component topology"), holes and voids are derived here in the reference's
// int32 arithmetic (topology_computation.hpp:624-630).
#pragma once
#include <cstddef>
#include <cstdint>
#include <iostream>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "sdf_tools/gpu_context.hpp"

namespace sdf_tools {

// cells: nx * ny * nz records of `stride` bytes holding the float occupancy at occ_off and the uint32 label at comp_off;
// class_mask: FILLED (1) | EMPTY (2) | UNKNOWN (4).  Throws std::invalid_argument on a refusal (a label above max_label, a label
// with selected and unselected voxels, more nodes than the union-find numbers) and std::runtime_error on a HIP failure.
inline std::map<uint32_t, std::pair<int32_t, int32_t>> ComputeComponentTopologyFromCells(
    const void* cells, const size_t stride, const size_t occ_off, const size_t comp_off, const int64_t nx, const int64_t ny, const int64_t nz,
    const int class_mask, const uint32_t max_label, const bool verbose) {
    std::map<uint32_t, std::pair<int32_t, int32_t>> result;
    if (nx <= 0 || ny <= 0 || nz <= 0 || (class_mask & 7) == 0) return result;      // (nothing selected: an empty map)
    std::vector<int64_t> counts(((size_t)max_label + 1) * 5, 0);
    {
        const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
        const std::lock_guard<std::mutex> lock(ctx->mutex);
        sdf_generation::ThrowOnStatus(ctx->handle, sdfgpu_component_topology_cells(ctx->handle, cells, stride, occ_off, comp_off, nx, ny, nz,
                                                                                   class_mask, max_label, counts.data()));
    }
    for (size_t c = 0; c <= (size_t)max_label; ++c) {
        const int64_t* q = counts.data() + c * 5;
        if (q[0] == 0) continue;                            // no surface vertex: not in the reference's map
        const int32_t m3 = (int32_t)q[1], m5 = (int32_t)q[2], m6 = (int32_t)q[3], surfaces = (int32_t)q[4];
        const int32_t voids = surfaces - 1;
        const int32_t holes = 1 + ((m5 + (2 * m6) - m3) / 8) + voids;
        if (verbose)
            std::cout << "Processing surface with M3 = " << m3 << " M5 = " << m5 << " M6 = " << m6 << " holes = " << holes
                      << " surfaces = " << surfaces << " voids = " << voids << std::endl;
        result[(uint32_t)c] = std::make_pair(holes, voids);
    }
    return result;
}

}  // namespace sdf_tools
