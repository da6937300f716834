// dsh_frontier -- asking a sensed map where it ends, on sdf_tools::DynamicSpatialHashedCollisionMapGrid::ExtractFrontierCells /
// ExtractFrontierWindowBits / ExtractFrontierClusters: a depth camera looks along +x at a wall with a box in front of it (the scene
// of dsh_cast) and one frame is carved into the map.  The frontier is the seen-free space that borders never-seen space: the sides of
// the viewing frustum and the shadow behind the box.  The example lists it under both neighbour rules, groups the part of it around
// the sensor into clusters, and casts a ray from the sensor to the largest cluster's centroid, as a planner that picks its next
// view would.
// Usage: dsh_frontier_example [output directory]
// With a directory, what the example asked and got is written there as raw arrays for tests/test_gpu_dsh_frontier_cpp.py:
//   frame.f32 (the carved frame's points, x y z), cells_6.i64 / cells_26.i64 (the frontier cells of the whole map, x y z),
//   window_bits.u32 (the 26-rule frontier of the window), cluster_label.u32, cluster_cells.i64, cluster_lower.i64, cluster_upper.i64,
//   cluster_centroid.f64 (the window's clusters), cast_status.u8 / cast_cell.i64 (the ray to the largest cluster's centroid)
// The map's numbers (cell size, chunk size, the sensor, the window) are repeated in that test.
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "sdf_tools/dynamic_spatial_hashed_collision_map.hpp"

namespace {

using Map = sdf_tools::DynamicSpatialHashedCollisionMapGrid;

template <typename T>
void Write(const std::string& dir, const std::string& name, const T* data, size_t count) {
    if (dir.empty()) return;
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f || std::fwrite(data, sizeof(T), count, f) != count) throw std::runtime_error("cannot write " + name);
    std::fclose(f);
}

const double kSensor[3] = {0.025, 1.225, 1.225};

// The frame of dsh_cast: a 48 x 48 image of the wall x = 3.0, the box [1.5, 2.0] x [0.9, 1.5] x [0.9, 1.5] in front.
std::vector<float> Frame() {
    std::vector<float> points;
    for (int i = 0; i < 48; ++i)
        for (int j = 0; j < 48; ++j) {
            const double wall[3] = {3.0, 0.025 + 0.05 * i, 0.025 + 0.05 * j};
            double end[3] = {wall[0], wall[1], wall[2]};
            const double at = (1.5 - kSensor[0]) / (wall[0] - kSensor[0]);
            const double y = kSensor[1] + at * (wall[1] - kSensor[1]), z = kSensor[2] + at * (wall[2] - kSensor[2]);
            if (y >= 0.9 && y <= 1.5 && z >= 0.9 && z <= 1.5) { end[0] = 1.5; end[1] = y; end[2] = z; }
            for (int a = 0; a < 3; ++a) points.push_back((float)end[a]);
        }
    return points;
}

std::vector<int64_t> Flat(const std::vector<VoxelGrid::GRID_INDEX>& cells) {
    std::vector<int64_t> flat;
    for (const VoxelGrid::GRID_INDEX& c : cells) { flat.push_back(c.x); flat.push_back(c.y); flat.push_back(c.z); }
    return flat;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "";
    try {
        sdf_tools::DynamicSpatialHashedCollisionMapGrid seen("world", 0.05, 8, 8, 8, sdf_tools::COLLISION_CELL(0.5f));
        const std::vector<float> frame = Frame();
        const Eigen::Vector3d sensor(kSensor[0], kSensor[1], kSensor[2]);
        const sdfgpu_dsh_ray_counts counts = seen.InsertPointCloudRays(frame, sensor, 4.0, sdf_tools::COLLISION_CELL(0.0f), sdf_tools::COLLISION_CELL(1.0f));
        std::cout << "frame: " << counts.rays_hit << " hits, " << counts.cells_carved << " cells carved" << std::endl;
        Write(dir, "frame.f32", frame.data(), frame.size());
        const Map& map = seen;                                          // every frontier call is const: the map is read, not written

        const std::vector<int64_t> six = Flat(map.ExtractFrontierCells(false)), all_26 = Flat(map.ExtractFrontierCells(true));
        std::cout << "frontier cells: " << six.size() / 3 << " with an unknown face neighbour, " << all_26.size() / 3 << " with an unknown neighbour among all 26"
                  << std::endl;
        Write(dir, "cells_6.i64", six.data(), six.size());
        Write(dir, "cells_26.i64", all_26.data(), all_26.size());

        // the 40^3 cells around the sensor (its cell is (0, 24, 24)): the near end of the frustum
        const VoxelGrid::GRID_INDEX lower(-4, 4, 4);
        const std::vector<uint32_t> bits = map.ExtractFrontierWindowBits(lower, 40, 40, 40, true);
        Write(dir, "window_bits.u32", bits.data(), bits.size());
        const std::vector<Map::FrontierCluster> clusters = map.ExtractFrontierClusters(lower, 40, 40, 40);
        std::vector<uint32_t> label;
        std::vector<int64_t> cells, low, high;
        std::vector<double> centroid;
        size_t largest = 0;
        for (size_t k = 0; k < clusters.size(); ++k) {
            const Map::FrontierCluster& c = clusters[k];
            std::cout << "cluster " << c.label << ": " << c.cells << " cells in (" << c.lower.x << ", " << c.lower.y << ", " << c.lower.z << ") .. (" << c.upper.x
                      << ", " << c.upper.y << ", " << c.upper.z << "), centroid (" << c.centroid.x() << ", " << c.centroid.y() << ", " << c.centroid.z() << ")"
                      << std::endl;
            label.push_back(c.label);
            cells.push_back(c.cells);
            low.push_back(c.lower.x); low.push_back(c.lower.y); low.push_back(c.lower.z);
            high.push_back(c.upper.x); high.push_back(c.upper.y); high.push_back(c.upper.z);
            for (int a = 0; a < 3; ++a) centroid.push_back(c.centroid(a));
            if (c.cells > clusters[largest].cells) largest = k;
        }
        Write(dir, "cluster_label.u32", label.data(), label.size());
        Write(dir, "cluster_cells.i64", cells.data(), cells.size());
        Write(dir, "cluster_lower.i64", low.data(), low.size());
        Write(dir, "cluster_upper.i64", high.data(), high.size());
        Write(dir, "cluster_centroid.f64", centroid.data(), centroid.size());
        if (clusters.empty()) throw std::runtime_error("the window around the sensor holds no frontier");

        // what a ray from the sensor to the largest cluster's centroid meets: unknown space blocks, the start's cell is left out
        const Map::RayCast to_centroid = map.CastRay(sensor, clusters[largest].centroid, 4.0, true, true, false);
        std::cout << "the sensor " << (to_centroid.status == Map::CAST_BLOCKED ? "does not see" : "sees") << " the centroid of cluster " << clusters[largest].label
                  << " (" << to_centroid.step << " cells walked, " << to_centroid.distance << " m)" << std::endl;
        const uint8_t status = (uint8_t)to_centroid.status;
        const int64_t cast_cell[3] = {to_centroid.cell.x, to_centroid.cell.y, to_centroid.cell.z};
        Write(dir, "cast_status.u8", &status, 1);
        Write(dir, "cast_cell.i64", cast_cell, 3);
        if (six.empty() || six.size() > all_26.size()) throw std::runtime_error("the 26-rule must find every cell the 6-rule finds");
    } catch (const std::exception& e) {
        std::cerr << "dsh_frontier example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "dsh_frontier example done" << std::endl;
    return 0;
}
