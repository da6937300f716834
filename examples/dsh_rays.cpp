// dsh_rays -- a sensed world map that forgets, on sdf_tools::DynamicSpatialHashedCollisionMapGrid::InsertPointCloudRays: a depth
// camera looks along +x at a wall; in the first frame a box stands in front of the wall and is seen from one side, in the second
// frame the box is gone.  The rays of the second frame pass through the box's old place and carve it free, so the signed distance
// field of the window around it no longer shows an obstacle there: the nearest one is the wall.
// Usage: dsh_rays_example [output directory]
// With a directory, what the example saw is written there as raw arrays for tests/test_gpu_dsh_rays_cpp.py:
//   frame_<k>.f32 (the points of frame k, x y z), window_<k>.cells (the window's 8-byte records after frame k, x -> y -> z),
//   window_<k>_sdf.f32
// The map's numbers (cell size, chunk size, sensor, range, window) are repeated in that test.
#include <cmath>
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "sdf_tools/dynamic_spatial_hashed_collision_map.hpp"

namespace {

template <typename T>
void Write(const std::string& dir, const std::string& name, const T* data, size_t count) {
    if (dir.empty()) return;
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f || std::fwrite(data, sizeof(T), count, f) != count) throw std::runtime_error("cannot write " + name);
    std::fclose(f);
}

const double kSensor[3] = {0.025, 1.225, 1.225};

// A 48 x 48 image of the wall x = 3.0: each pixel's ray ends on the wall, or, while the box [1.5, 2.0] x [0.9, 1.5] x [0.9, 1.5]
// stands there, on the box's face x = 1.5 where it crosses that face inside the box.  Every 97th pixel has no return (NaN).
std::vector<float> Frame(const bool box) {
    std::vector<float> points;
    for (int i = 0; i < 48; ++i)
        for (int j = 0; j < 48; ++j) {
            const double wall[3] = {3.0, 0.025 + 0.05 * i, 0.025 + 0.05 * j};
            double end[3] = {wall[0], wall[1], wall[2]};
            const double at = (1.5 - kSensor[0]) / (wall[0] - kSensor[0]);
            const double y = kSensor[1] + at * (wall[1] - kSensor[1]), z = kSensor[2] + at * (wall[2] - kSensor[2]);
            if (box && y >= 0.9 && y <= 1.5 && z >= 0.9 && z <= 1.5) { end[0] = 1.5; end[1] = y; end[2] = z; }
            const bool no_return = (i * 48 + j) % 97 == 96;
            for (int a = 0; a < 3; ++a) points.push_back(no_return ? NAN : (float)end[a]);
        }
    return points;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "";
    try {
        // unknown space (occupancy 0.5) is the default: what no ray has looked through stays unknown
        sdf_tools::DynamicSpatialHashedCollisionMapGrid map("world", 0.05, 8, 8, 8, sdf_tools::COLLISION_CELL(0.5f));
        const sdf_tools::COLLISION_CELL free_cell(0.0f), filled_cell(1.0f);
        const Eigen::Vector3d sensor(kSensor[0], kSensor[1], kSensor[2]);
        const VoxelGrid::GRID_INDEX lower(20, 12, 12);                 // 48 x 24 x 24 cells: the box's place and the wall behind it
        double centre_distance[2] = {0.0, 0.0};
        for (int k = 0; k < 2; ++k) {
            const std::vector<float> points = Frame(k == 0);
            const sdfgpu_dsh_ray_counts counts = map.InsertPointCloudRays(points, sensor, 4.0, free_cell, filled_cell);
            std::cout << "frame " << k << (k == 0 ? " (box)" : " (box gone)") << ": " << counts.rays_hit << " hits, " << counts.rays_truncated << " beyond the range, "
                      << counts.rays_skipped << " without a return, " << counts.cells_carved << " cells carved, " << counts.new_chunks << " new chunks" << std::endl;
            const sdf_tools::CollisionMapGrid window = map.ExtractCollisionMapGrid(lower, 48, 24, 24);
            auto sdf = map.ExtractSignedDistanceFieldDevice(lower, 48, 24, 24, 1e6f, false, false);
            const double query[3] = {1.525, 1.225, 1.225};             // the middle of the face the camera saw
            sdf.first.QueryBatch(query, 1, true, &centre_distance[k], nullptr, nullptr);
            const auto cell = map.Get(query[0], query[1], query[2]);
            std::cout << "  the box's face: occupancy " << cell.first.occupancy << ", distance " << centre_distance[k] << std::endl;
            Write(dir, "frame_" + std::to_string(k) + ".f32", points.data(), points.size());
            Write(dir, "window_" + std::to_string(k) + ".cells", window.GetImmutableRawData().data(), window.GetImmutableRawData().size());
            Write(dir, "window_" + std::to_string(k) + "_sdf.f32", sdf.first.Host().GetImmutableRawData().data(), sdf.first.Host().GetImmutableRawData().size());
        }
        if (!(centre_distance[0] <= 0.0 && centre_distance[1] > 0.0)) throw std::runtime_error("the box is still in the map after the frame without it");
    } catch (const std::exception& e) {
        std::cerr << "dsh_rays example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "dsh_rays example done" << std::endl;
    return 0;
}
