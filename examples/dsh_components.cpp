// dsh_components -- asking a sensed map which of its frontiers can be reached, on
// sdf_tools::DynamicSpatialHashedCollisionMapGrid::UpdateConnectedComponents: a robot stands in a room (the box [0, 3] x [0, 2.4] x
// [0, 2.4] m) beside a closed-off closet (the box [3.2, 4.2] x [0.6, 1.8] x [0, 2.4] m behind the room's x = 3 wall).  Three frames
// of a depth camera are fused into the map: two from the robot, looking along +x and +y, and one taken inside the closet before
// its door was shut.  Each frame sees a part of its box only, so each box holds free space that borders never-seen space.  The
// example labels the connected components of the whole map with unknown space kept apart from free space, lists the frontier cells,
// reads their labels with GetBatch at the cell centres, and prints how many share the robot's component (the robot can drive
// there) and how many do not (the closet's).
// Usage: dsh_components_example [output directory]
// With a directory, what the example asked and got is written there as raw arrays for tests/test_gpu_dsh_components_cpp.py:
//   frame_0.f32 .. frame_2.f32 (the frames' points, x y z), sensors.f64 (their sensors), frontier.i64 (the frontier cells, x y z),
//   labels.u32 (their component labels), summary.u32 (K, the robot's label, frontier cells in its component, frontier cells elsewhere)
// The map's numbers (cell size, chunk size, range) are repeated in that test.
#include <algorithm>
#include <cmath>
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

const double kCell = 0.05, kRange = 6.0;
const double kRoom[6] = {0.0, 0.0, 0.0, 3.0, 2.4, 2.4}, kCloset[6] = {3.2, 0.6, 0.0, 4.2, 1.8, 2.4};   // lower corner, upper corner

// A 48 x 48 image of a camera at `sensor` inside `box`, looking along `forward` with `side` to its right (both unit vectors along
// axes; up is z) over +-0.6 in both image directions: every pixel's ray ends where it leaves the box.
std::vector<float> Frame(const double sensor[3], const double forward[3], const double side[3], const double box[6]) {
    std::vector<float> points;
    for (int i = 0; i < 48; ++i)
        for (int j = 0; j < 48; ++j) {
            const double u = -0.6 + 1.2 * (i + 0.5) / 48.0, v = -0.6 + 1.2 * (j + 0.5) / 48.0;
            const double d[3] = {forward[0] + u * side[0], forward[1] + u * side[1], v};
            double t = 1e30;
            for (int a = 0; a < 3; ++a) {
                if (d[a] > 0.0) t = std::min(t, (box[3 + a] - sensor[a]) / d[a]);
                if (d[a] < 0.0) t = std::min(t, (box[a] - sensor[a]) / d[a]);
            }
            for (int a = 0; a < 3; ++a) points.push_back((float)(sensor[a] + t * d[a]));
        }
    return points;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "";
    try {
        Map seen("world", kCell, 8, 8, 8, sdf_tools::COLLISION_CELL(0.5f));
        const double robot[3] = {0.525, 0.525, 1.225}, in_closet[3] = {3.325, 1.225, 1.225};
        const double plus_x[3] = {1.0, 0.0, 0.0}, plus_y[3] = {0.0, 1.0, 0.0}, minus_x[3] = {-1.0, 0.0, 0.0};
        const std::vector<float> frames[3] = {Frame(robot, plus_x, plus_y, kRoom), Frame(robot, plus_y, minus_x, kRoom), Frame(in_closet, plus_x, plus_y, kCloset)};
        const double* sensors[3] = {robot, robot, in_closet};
        std::vector<double> sensor_dump;
        for (int k = 0; k < 3; ++k) {
            const sdfgpu_dsh_ray_counts counts = seen.FusePointCloudRays(frames[k], Eigen::Vector3d(sensors[k][0], sensors[k][1], sensors[k][2]), kRange);
            std::cout << "frame " << k << ": " << counts.rays_hit << " hits, " << counts.new_chunks << " new chunks" << std::endl;
            Write(dir, "frame_" + std::to_string(k) + ".f32", frames[k].data(), frames[k].size());
            sensor_dump.insert(sensor_dump.end(), sensors[k], sensors[k] + 3);
        }
        Write(dir, "sensors.f64", sensor_dump.data(), sensor_dump.size());
        if (seen.AreComponentsValid()) throw std::runtime_error("no update has run yet");

        // unknown space apart: free space the robot has seen is not joined with never-seen cells of the chunks it has touched
        const uint32_t count = seen.UpdateConnectedComponents(true);
        const Map same_map = seen;                                       // a copy is another name for the same map: it agrees on the validity
        if (!seen.AreComponentsValid() || !same_map.AreComponentsValid() || same_map.GetNumConnectedComponents() != std::make_pair(count, true))
            throw std::runtime_error("the map and its copy disagree about the components");
        if (seen.UpdateConnectedComponents(true) != count) throw std::runtime_error("a valid map answers with the stored count");
        const uint32_t robot_label = seen.Get(robot[0], robot[1], robot[2]).first.component;
        std::cout << count << " components; the robot stands in component " << robot_label << std::endl;

        const std::vector<VoxelGrid::GRID_INDEX> frontier = seen.ExtractFrontierCells(false);
        std::vector<double> centres;
        std::vector<int64_t> flat;
        for (const VoxelGrid::GRID_INDEX& c : frontier) {
            const int64_t i[3] = {c.x, c.y, c.z};
            for (int a = 0; a < 3; ++a) { centres.push_back(((double)i[a] + 0.5) * kCell); flat.push_back(i[a]); }
        }
        const std::vector<sdf_tools::COLLISION_CELL> cells = seen.GetBatch(centres).first;
        std::vector<uint32_t> labels;
        uint32_t reachable = 0, elsewhere = 0;
        for (const sdf_tools::COLLISION_CELL& cell : cells) {
            labels.push_back(cell.component);
            (cell.component == robot_label ? reachable : elsewhere) += 1;
        }
        std::cout << "frontier cells: " << frontier.size() << ", " << reachable << " in the robot's component, " << elsewhere << " elsewhere" << std::endl;
        const uint32_t summary[4] = {count, robot_label, reachable, elsewhere};
        Write(dir, "frontier.i64", flat.data(), flat.size());
        Write(dir, "labels.u32", labels.data(), labels.size());
        Write(dir, "summary.u32", summary, 4);
        if (robot_label == 0 || reachable == 0 || elsewhere == 0) throw std::runtime_error("both the room and the closet hold frontier cells");

        // a fourth frame changes the map: the labels are stale until the next update
        (void)seen.FusePointCloudRays(frames[0], Eigen::Vector3d(robot[0], robot[1], robot[2]), kRange);
        if (seen.AreComponentsValid() || same_map.AreComponentsValid()) throw std::runtime_error("a fused frame clears the validity, for every copy");
        std::cout << "after another frame: " << seen.UpdateConnectedComponents(true) << " components" << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "dsh_components example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "dsh_components example done" << std::endl;
    return 0;
}
