// The yardstick of Resample: the loop of the contract (include/sdfgpu.h "Resample") written against VoxelGrid's public members
// alone -- a result grid from the metric-size constructor, then, for every source cell in x -> y -> z order,
// result.SetValue4d(source.GridIndexToLocation(x, y, z), cell).  Host code only: no GPU library is linked.  Instantiated for 4-byte
// (float), 8-byte and 16-byte cells.  tests/resample_restated.py compiles this with g++ -O2 -ffp-contract=off and loads it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "arc_utilities/voxel_grid.hpp"

namespace {

struct Cell8 { uint32_t w[2]; };
struct Cell16 { uint32_t w[4]; };
static_assert(sizeof(float) == 4 && sizeof(Cell8) == 8 && sizeof(Cell16) == 16, "record sizes");

// The restatement.  *out_hit[i] = result cell i received a source cell.
template <typename T>
VoxelGrid::VoxelGrid<T> Resample(const VoxelGrid::VoxelGrid<T>& source, const double new_resolution, std::vector<uint8_t>* out_hit) {
    VoxelGrid::VoxelGrid<T> resampled(source.GetOriginTransform(), new_resolution, source.GetXSize(), source.GetYSize(), source.GetZSize(),
                                      source.GetOOBValue(), source.GetOOBValue());
    out_hit->assign((size_t)(resampled.GetNumXCells() * resampled.GetNumYCells() * resampled.GetNumZCells()), 0);
    for (int64_t x = 0; x < source.GetNumXCells(); x++)
        for (int64_t y = 0; y < source.GetNumYCells(); y++)
            for (int64_t z = 0; z < source.GetNumZCells(); z++) {
                const Eigen::Vector4d location = source.GridIndexToLocation(x, y, z);
                if (resampled.SetValue4d(location, source.GetImmutable(x, y, z).first))
                    (*out_hit)[(size_t)resampled.GetDataIndex(resampled.LocationToGridIndex4d(location))] = 1;
            }
    return resampled;
}

template <typename T>
int Run(const int64_t nx, const int64_t ny, const int64_t nz, const double cell, const double* origin, const double new_resolution,
        const void* src, const void* oob, int64_t* out_dims, double* out_inverse, double* out_inv_cell, void* dst,
        const int64_t dst_capacity, uint64_t* out_written) {
    Eigen::Isometry3d o = Eigen::Isometry3d::Identity();
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) o.matrix()(r, c) = origin[4 * r + c];
    T oob_value;
    std::memcpy(&oob_value, oob, sizeof(T));
    VoxelGrid::VoxelGrid<T> source(o, cell, nx, ny, nz, oob_value, oob_value);
    std::memcpy(static_cast<void*>(source.GetMutableRawData().data()), src, (size_t)(nx * ny * nz) * sizeof(T));
    std::vector<uint8_t> hit;
    const VoxelGrid::VoxelGrid<T> result = Resample(source, new_resolution, &hit);
    out_dims[0] = result.GetNumXCells(); out_dims[1] = result.GetNumYCells(); out_dims[2] = result.GetNumZCells();
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) out_inverse[4 * r + c] = result.GetInverseOriginTransform().matrix()(r, c);
    const Eigen::Vector3d sizes = result.GetCellSizes();
    out_inv_cell[0] = 1.0 / sizes.x(); out_inv_cell[1] = 1.0 / sizes.y(); out_inv_cell[2] = 1.0 / sizes.z();
    uint64_t written = 0;
    for (const uint8_t h : hit) written += h;
    *out_written = written;
    const int64_t n = out_dims[0] * out_dims[1] * out_dims[2];
    if (!dst) return 0;
    if (dst_capacity < n) return 2;
    std::memcpy(dst, static_cast<const void*>(result.GetImmutableRawData().data()), (size_t)n * sizeof(T));
    return 0;
}

}  // namespace

// 0: done (dst == nullptr: dimensions, matrices and the count only); 1: std::invalid_argument (message in msg); 2: dst_capacity
// (in cells) is below the result's size; 3: cell_bytes is not 4, 8 or 16.  origin and out_inverse are row-major 4 x 4.
extern "C" int rr_resample(int cell_bytes, int64_t nx, int64_t ny, int64_t nz, double cell, const double* origin, double new_resolution,
                           const void* src, const void* oob, int64_t* out_dims, double* out_inverse, double* out_inv_cell, void* dst,
                           int64_t dst_capacity, uint64_t* out_written, char* msg, int msg_len) {
    try {
        if (cell_bytes == 4) return Run<float>(nx, ny, nz, cell, origin, new_resolution, src, oob, out_dims, out_inverse, out_inv_cell, dst, dst_capacity, out_written);
        if (cell_bytes == 8) return Run<Cell8>(nx, ny, nz, cell, origin, new_resolution, src, oob, out_dims, out_inverse, out_inv_cell, dst, dst_capacity, out_written);
        if (cell_bytes == 16) return Run<Cell16>(nx, ny, nz, cell, origin, new_resolution, src, oob, out_dims, out_inverse, out_inv_cell, dst, dst_capacity, out_written);
        return 3;
    } catch (const std::invalid_argument& e) {
        if (msg && msg_len > 0) std::snprintf(msg, (size_t)msg_len, "%s", e.what());
        return 1;
    }
}
