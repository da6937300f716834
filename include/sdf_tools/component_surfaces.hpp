// component_surfaces -- the shared body of CollisionMapGrid / TaggedObjectCollisionMapGrid::ExtractComponentSurfaces (reference
// src/sdf_tools/collision_map.cpp:697-754, tagged_object_collision_map.cpp:492-550) and of CheckIfCandidateCorner
// (collision_map.hpp:508-619).  The surface voxels come from the GPU grouped by component (sdfgpu_component_surfaces_cells,
// include/sdfgpu.h "Component surfaces": the contract and its two deviations from the reference as written); the reference's
// map of hash maps is built from them here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

#include "arc_utilities/voxel_grid.hpp"
#include "sdf_tools/gpu_context.hpp"

namespace sdf_tools {

// The fast form of ExtractComponentSurfaces: the surface voxels of component c are indices[offsets[c] .. offsets[c + 1]), linear
// indices (x ny + y) nz + z in ascending order; offsets has max_label + 2 entries.
struct ComponentSurfaceIndices {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> indices;
};

// cells: nx * ny * nz records of `stride` bytes holding the float occupancy at occ_off and the uint32 label at comp_off;
// class_mask: FILLED (1) | EMPTY (2) | UNKNOWN (4).  Throws std::invalid_argument on a refusal (a label above max_label, more
// than 2^32 - 1 voxels) and std::runtime_error on a HIP failure.
inline ComponentSurfaceIndices ExtractComponentSurfaceIndicesFromCells(const void* cells, const size_t stride, const size_t occ_off,
                                                                       const size_t comp_off, const int64_t nx, const int64_t ny,
                                                                       const int64_t nz, const int class_mask, const uint32_t max_label) {
    ComponentSurfaceIndices result;
    result.offsets.assign((size_t)max_label + 2, 0);
    if (nx <= 0 || ny <= 0 || nz <= 0 || (class_mask & 7) == 0) return result;      // (nothing selected: no surface voxel)
    std::vector<int64_t> counts((size_t)max_label + 1, 0);
    result.indices.resize((size_t)(nx * ny * nz));                                  // (every voxel can be a surface voxel)
    int64_t total = 0;
    {
        const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
        const std::lock_guard<std::mutex> lock(ctx->mutex);
        sdf_generation::ThrowOnStatus(ctx->handle, sdfgpu_component_surfaces_cells(ctx->handle, cells, stride, occ_off, comp_off, nx, ny, nz,
                                                                                   class_mask & 7, max_label, counts.data(),
                                                                                   result.indices.data(), (int64_t)result.indices.size(), &total));
    }
    result.indices.resize((size_t)total);
    result.indices.shrink_to_fit();
    for (size_t c = 0; c <= (size_t)max_label; ++c) result.offsets[c + 1] = result.offsets[c] + (uint64_t)counts[c];
    return result;
}

// {component: {index: 1}} for every component with a surface voxel, as the reference returns it
inline std::map<uint32_t, std::unordered_map<VoxelGrid::GRID_INDEX, uint8_t>> ComponentSurfacesToMap(const ComponentSurfaceIndices& s,
                                                                                                     const int64_t ny, const int64_t nz) {
    std::map<uint32_t, std::unordered_map<VoxelGrid::GRID_INDEX, uint8_t>> surfaces;
    for (size_t c = 0; c + 1 < s.offsets.size(); ++c) {
        if (s.offsets[c + 1] == s.offsets[c]) continue;
        std::unordered_map<VoxelGrid::GRID_INDEX, uint8_t>& cells = surfaces[(uint32_t)c];
        cells.reserve((size_t)(s.offsets[c + 1] - s.offsets[c]));
        for (uint64_t i = s.offsets[c]; i < s.offsets[c + 1]; ++i) {
            const int64_t v = (int64_t)s.indices[(size_t)i], t = v / nz;
            cells[VoxelGrid::GRID_INDEX(t / ny, t % ny, v % nz)] = 1;
        }
    }
    return surfaces;
}

// CheckIfCandidateCorner (collision_map.hpp:549-619) on the stored labels: (candidate corner, index in the grid).  A cell is a
// candidate corner when two or more of its in-grid face neighbours belong to another component.
template <typename Grid>
inline std::pair<bool, bool> CheckIfCandidateCornerOnGrid(const Grid& grid, const int64_t x_index, const int64_t y_index, const int64_t z_index) {
    const auto current_cell = grid.GetImmutable(x_index, y_index, z_index);
    if (!current_cell.second) return std::pair<bool, bool>(false, false);
    static const int64_t kSteps[6][3] = {{-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
    uint32_t different_neighbors = 0u;
    for (const auto& d : kSteps) {
        const auto neighbor = grid.GetImmutable(x_index + d[0], y_index + d[1], z_index + d[2]);
        if (neighbor.second && (neighbor.first.component != current_cell.first.component)) different_neighbors++;
    }
    return std::pair<bool, bool>(different_neighbors > 1u, true);
}

}  // namespace sdf_tools
