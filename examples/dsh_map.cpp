// dsh_map -- a map server in miniature on sdf_tools::DynamicSpatialHashedCollisionMapGrid: frames of points go into a sparse map that
// stays on the GPU, a dense window comes out as a CollisionMapGrid and as a signed distance field, and a few queries are answered.
// Usage: dsh_map_example [output directory]
// With a directory, what the example saw is written there as raw arrays for tests/test_gpu_dsh_cpp.py:
//   frame_<k>.f32 (the points of frame k, x y z), window.cells (the window's 8-byte records, x -> y -> z), window_sdf.f32
// The map's numbers (origin, cell size, chunk size, window) are repeated in that test.
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

// what a depth camera at `eye` sees of a sphere of radius 0.6 around (0.2, -0.1, 0.5): the cap that faces it, 20 000 points
std::vector<float> Frame(const double eye_angle) {
    std::vector<float> points;
    const double ex = std::cos(eye_angle), ey = std::sin(eye_angle);
    for (int i = 0; i < 200; ++i)
        for (int j = 0; j < 100; ++j) {
            const double phi = 2.0 * M_PI * i / 200.0, theta = M_PI * (j + 0.5) / 100.0;
            const double nx = std::sin(theta) * std::cos(phi), ny = std::sin(theta) * std::sin(phi), nz = std::cos(theta);
            if (nx * ex + ny * ey < 0.2) continue;
            points.push_back((float)(0.2 + 0.6 * nx));
            points.push_back((float)(-0.1 + 0.6 * ny));
            points.push_back((float)(0.5 + 0.6 * nz));
        }
    return points;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "";
    try {
        Eigen::Isometry3d origin;
        origin.setTranslation(-1.6, -1.6, -0.4);                      // whole cells of 0.05 away from the world's origin
        sdf_tools::DynamicSpatialHashedCollisionMapGrid map(origin, "world", 0.05, 16, 16, 16, sdf_tools::COLLISION_CELL(0.0f));

        for (int k = 0; k < 3; ++k) {
            const std::vector<float> points = Frame(0.9 * k);
            const size_t set = map.InsertPointCloud(points, sdf_tools::COLLISION_CELL(1.0f));
            const sdfgpu_dsh_counts counts = map.GetCounts();
            std::cout << "frame " << k << ": " << points.size() / 3 << " points, " << set << " set, " << counts.cell_filled << " cell-filled chunks, "
                      << counts.bytes_held << " bytes held" << std::endl;
            Write(dir, "frame_" + std::to_string(k) + ".f32", points.data(), points.size());
        }
        // a region the planner knows to be free, as one record per chunk
        map.SetChunks({-0.9, -0.9, 0.1, -0.9, 0.9, 0.1}, {sdf_tools::COLLISION_CELL(0.0f, 7u)});

        // the 64 x 64 x 48 cells around the robot, as a grid and as a signed distance field that stays on the GPU
        const VoxelGrid::GRID_INDEX lower(4, 4, -2);
        const sdf_tools::CollisionMapGrid window = map.ExtractCollisionMapGrid(lower, 64, 64, 48);
        size_t filled = 0;
        for (const sdf_tools::COLLISION_CELL& cell : window.GetImmutableRawData()) filled += cell.occupancy > 0.5f;
        auto sdf = map.ExtractSignedDistanceFieldDevice(lower, 64, 64, 48, 1e6f, false, false);
        std::cout << "window: " << filled << " filled cells, SDF extrema " << sdf.second.first << " " << sdf.second.second << std::endl;
        const auto from_grid = window.ExtractSignedDistanceField(1e6f, false, false);
        if (from_grid.first.GetImmutableRawData() != sdf.first.Host().GetImmutableRawData())
            throw std::runtime_error("the window's SDF differs from the SDF of the window's grid");
        Write(dir, "window.cells", window.GetImmutableRawData().data(), window.GetImmutableRawData().size());
        Write(dir, "window_sdf.f32", sdf.first.Host().GetImmutableRawData().data(), sdf.first.Host().GetImmutableRawData().size());

        const double queries[9] = {0.2, -0.1, 0.5, 0.2, -0.1, 1.3, 0.9, -0.1, 0.5};
        double distance[3];
        sdf.first.QueryBatch(queries, 3, true, distance, nullptr, nullptr);
        for (int i = 0; i < 3; ++i) {
            const auto cell = map.Get(queries[3 * i], queries[3 * i + 1], queries[3 * i + 2]);
            std::cout << "(" << queries[3 * i] << ", " << queries[3 * i + 1] << ", " << queries[3 * i + 2] << "): distance " << distance[i] << ", occupancy "
                      << cell.first.occupancy << ", found status " << cell.second << std::endl;
        }
        std_msgs::ColorRGBA red, green, blue;
        red.r = red.a = green.g = green.a = blue.b = blue.a = 1.0f;
        for (const visualization_msgs::Marker& m : map.ExportForDisplay(red, green, blue))
            std::cout << "marker " << m.ns << ": " << m.points.size() << " cubes of " << m.scale.x << " m" << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "dsh_map example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "dsh_map example done" << std::endl;
    return 0;
}
