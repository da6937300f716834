// dsh_fusion -- a sensed world map that weighs its evidence, on sdf_tools::DynamicSpatialHashedCollisionMapGrid::FusePointCloudRays:
// the scene of dsh_rays (a depth camera looks along +x at a wall, a box stands in front of it) seen for four frames, then the box is
// gone.  Each frame updates every cell it looks through once with prob_miss and every cell a return falls into once with prob_hit, so
// the box's face grows more certain while it is seen and fades over several frames once it is not; the example prints the frame at
// which its occupancy falls to 0.5 or below and the signed distance field stops showing an obstacle there.  Frame 3 carries one
// spurious return in space that three frames have seen free: that cell never passes 0.5, where InsertPointCloudRays would have put an
// obstacle into the planner's window.
// Usage: dsh_fusion_example [output directory]
// With a directory, what the example saw is written there as raw arrays for tests/test_gpu_dsh_fusion_cpp.py:
//   frame_<k>.f32 (the points of frame k, x y z), window_<k>.cells (the window's 8-byte records after frame k, x -> y -> z),
//   window_<k>_sdf.f32
// The map's numbers (cell size, chunk size, sensor, range, window, the two watched cells) are repeated in that test.
#include <algorithm>
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
const double kFace[3] = {1.525, 1.23125, 1.23125};         // inside the cell of the box's face that the middle pixel's ray ends in
const double kSpurious[3] = {1.225, 1.225, 1.225};         // free space in front of the box
const int kPixels = 32, kBoxFrames = 4, kFrames = 14, kSpuriousFrame = 3;

// A 32 x 32 image of the wall x = 3.0: each pixel's ray ends on the wall, or, while the box [1.5, 2.0] x [0.9, 1.5] x [0.9, 1.5]
// stands there, on the box's face x = 1.5 where it crosses that face inside the box.  Every 97th pixel has no return (NaN).
std::vector<float> Frame(const bool box, const bool spurious) {
    std::vector<float> points;
    for (int i = 0; i < kPixels; ++i)
        for (int j = 0; j < kPixels; ++j) {
            const double wall[3] = {3.0, 0.0375 + 0.075 * i, 0.0375 + 0.075 * j};
            double end[3] = {wall[0], wall[1], wall[2]};
            const double at = (1.5 - kSensor[0]) / (wall[0] - kSensor[0]);
            const double y = kSensor[1] + at * (wall[1] - kSensor[1]), z = kSensor[2] + at * (wall[2] - kSensor[2]);
            if (box && y >= 0.9 && y <= 1.5 && z >= 0.9 && z <= 1.5) { end[0] = 1.5; end[1] = y; end[2] = z; }
            const bool no_return = (i * kPixels + j) % 97 == 96;
            for (int a = 0; a < 3; ++a) points.push_back(no_return ? NAN : (float)end[a]);
        }
    if (spurious) for (int a = 0; a < 3; ++a) points.push_back((float)kSpurious[a]);
    return points;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "";
    try {
        // unknown space (occupancy 0.5) is the default: what no ray has looked through stays unknown
        sdf_tools::DynamicSpatialHashedCollisionMapGrid map("world", 0.05, 8, 8, 8, sdf_tools::COLLISION_CELL(0.5f));
        const Eigen::Vector3d sensor(kSensor[0], kSensor[1], kSensor[2]);
        const VoxelGrid::GRID_INDEX lower(20, 12, 12);                 // 48 x 24 x 24 cells: the box's place and the wall behind it
        int faded_at = -1;
        float spurious_most = 0.0f;
        for (int k = 0; k < kFrames; ++k) {
            const std::vector<float> points = Frame(k < kBoxFrames, k == kSpuriousFrame);
            const sdfgpu_dsh_ray_counts counts = map.FusePointCloudRays(points, sensor, 4.0);        // the default sensor model
            const sdf_tools::CollisionMapGrid window = map.ExtractCollisionMapGrid(lower, 48, 24, 24);
            auto sdf = map.ExtractSignedDistanceFieldDevice(lower, 48, 24, 24, 1e6f, false, false);
            double distance = 0.0;
            sdf.first.QueryBatch(kFace, 1, true, &distance, nullptr, nullptr);
            const float face = map.Get(kFace[0], kFace[1], kFace[2]).first.occupancy;
            const float stray = map.Get(kSpurious[0], kSpurious[1], kSpurious[2]).first.occupancy;
            spurious_most = std::max(spurious_most, stray);
            std::cout << "frame " << k << (k < kBoxFrames ? " (box)" : " (box gone)") << (k == kSpuriousFrame ? " (one spurious return)" : "") << ": " << counts.rays_hit
                      << " hits, " << counts.cells_carved << " cells carved, " << counts.new_chunks << " new chunks; the box's face: occupancy " << face << ", distance "
                      << distance << "; the spurious return's cell: occupancy " << stray << std::endl;
            if (k < kBoxFrames && !(face > 0.5f && distance <= 0.0)) throw std::runtime_error("the box's face is not an obstacle while it is seen");
            if (k >= kBoxFrames && faded_at < 0 && !(face > 0.5f)) {
                faded_at = k;
                if (!(distance > 0.0)) throw std::runtime_error("the box's face faded but the signed distance field still shows it");
            }
            if (k >= kBoxFrames && faded_at < 0 && !(distance <= 0.0)) throw std::runtime_error("the box's face is gone from the field before it faded");
            Write(dir, "frame_" + std::to_string(k) + ".f32", points.data(), points.size());
            Write(dir, "window_" + std::to_string(k) + ".cells", window.GetImmutableRawData().data(), window.GetImmutableRawData().size());
            Write(dir, "window_" + std::to_string(k) + "_sdf.f32", sdf.first.Host().GetImmutableRawData().data(), sdf.first.Host().GetImmutableRawData().size());
        }
        if (faded_at < 0) throw std::runtime_error("the box's face never faded");
        if (faded_at == kBoxFrames) throw std::runtime_error("one frame without the box erased it: evidence did not accumulate");
        if (!(spurious_most <= 0.5f)) throw std::runtime_error("a single spurious return became an obstacle");
        std::cout << "the box's face crosses 0.5 at frame " << faded_at << std::endl;
        std::cout << "the spurious return's cell never passes 0.5 (at most " << spurious_most << ")" << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "dsh_fusion example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "dsh_fusion example done" << std::endl;
    return 0;
}
