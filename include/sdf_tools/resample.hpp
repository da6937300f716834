// resample -- the shared body of CollisionMapGrid / TaggedObjectCollisionMapGrid::Resample (reference
// src/sdf_tools/collision_map.cpp:673-695, tagged_object_collision_map.cpp:399-422).  The result grid is built here by the grid's
// own metric-size constructor (the source's origin transform, frame and metric sizes, ceil(size / new_resolution) cells per axis,
// the source's OOB value as default and OOB value), so its cell counts and inverse transform are VoxelGrid's; the cell records
// are moved on the GPU by sdfgpu_resample_cells (include/sdfgpu.h "Resample"), straight into the result's storage.
//
// What the reference's loop does, and what is kept: every source cell, in x -> y -> z order, overwrites the result cell that holds
// its centre.  Coarsening therefore keeps, per result cell, the LAST source cell of the scan that lands in it; refining leaves
// every result cell that holds no source centre at the OOB value -- holes, not interpolation.  Components and convex segments of
// the result are invalid and counted 0, as for a freshly constructed grid.
#pragma once
#include <cmath>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <utility>

#include "arc_utilities/voxel_grid.hpp"
#include "sdf_tools/gpu_context.hpp"

namespace sdf_tools {

// Grid: a VoxelGrid of 4-, 8- or 16-byte records with GetFrame() and the constructor (origin, frame, resolution, x_size, y_size,
// z_size, oob_default_value).  Throws std::invalid_argument when new_resolution is not positive and finite (or the library refuses),
// std::runtime_error on a HIP failure.
template <typename Grid>
inline Grid ResampleGridFromCells(const Grid& source, const double new_resolution) {
    if (!(new_resolution > 0.0) || !std::isfinite(new_resolution)) throw std::invalid_argument("new_resolution must be positive and finite");
    Grid resampled(source.GetOriginTransform(), source.GetFrame(), new_resolution, source.GetXSize(), source.GetYSize(), source.GetZSize(),
                   source.GetOOBValue());
    const auto& cells = source.GetImmutableRawData();
    auto& result_cells = resampled.GetMutableRawData();
    static_assert(sizeof(cells[0]) == 4 || sizeof(cells[0]) == 8 || sizeof(cells[0]) == 16, "cell records are 4, 8 or 16 bytes");
    double origin[16], inverse[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            origin[4 * r + c] = source.GetOriginTransform().matrix()(r, c);
            inverse[4 * r + c] = resampled.GetInverseOriginTransform().matrix()(r, c);
        }
    const Eigen::Vector3d cell = source.GetCellSizes(), new_cell = resampled.GetCellSizes();
    const double src_cell[3] = {cell.x(), cell.y(), cell.z()};
    const double inv_cell[3] = {1.0 / new_cell.x(), 1.0 / new_cell.y(), 1.0 / new_cell.z()};       // (VoxelGrid's inv_cell_*_size_)
    const auto fill = source.GetOOBValue();
    const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
    const std::lock_guard<std::mutex> lock(ctx->mutex);
    sdf_generation::ThrowOnStatus(
        ctx->handle, sdfgpu_resample_cells(ctx->handle, cells.data(), sizeof(cells[0]), source.GetNumXCells(), source.GetNumYCells(),
                                           source.GetNumZCells(), src_cell, origin, inverse, inv_cell, result_cells.data(),
                                           resampled.GetNumXCells(), resampled.GetNumYCells(), resampled.GetNumZCells(), &fill, nullptr));
    return resampled;
}

}  // namespace sdf_tools
