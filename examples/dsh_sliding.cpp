// dsh_sliding -- a local map that slides with the robot, on sdf_tools::DynamicSpatialHashedCollisionMapGrid::RetainBox: a depth
// camera moves along +x through a corridor (walls at y = +-1.25 and z = +-1.25) in which boxes stand, one chunk (0.8 m) per frame,
// and fuses what it sees into a map whose byte_limit is sized for the region around it, not for the corridor.
//   - without RetainBox the pool fills up and a later frame is refused, for as long as the map lives
//   - with RetainBox around the sensor in front of every frame, every frame goes in; what lies behind the robot is forgotten
//     (GetBatch there says NOT_FOUND), and the window at the robot -- records and signed distance field -- is byte for byte that
//     of a map without a limit that forgot nothing
// Usage: dsh_sliding_example [output directory]
// With a directory, what the example saw is written there as raw arrays for tests/test_gpu_dsh_remove_cpp.py:
//   frame_<k>.f32 (the points of frame k, x y z), window.cells and window_sdf.f32 (the last window of the sliding map, x -> y -> z)
// The map's numbers (cell size, chunk size, the sensor's path, range, the region, the window, the byte limit) are repeated in that test.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

const double kCell = 0.1, kRange = 4.0, kWall = 1.25, kStep = 0.8;
const int kFrames = 16, kPixels = 24;
// the region kept around the sensor's cell: 16 cells behind it, 48 in front (the range is 40), 16 to each side
const int64_t kBehind = 16, kAhead = 48, kSide = 16;
// a table for the region's chunks and a frame's worst case (4 096 entries) and a pool of 192 chunks of 8^3 cells
const uint64_t kByteLimit = 4096 * 12 + 192 * (24 + 8 * 512);

double SensorX(const int k) { return 0.45 + kStep * k; }

// where the ray from s along d leaves the corridor or meets a box (every 2.4 m one stands on the floor, left and right in turn)
void Cast(const double s[3], const double d[3], double end[3]) {
    double t = 1e30;
    for (int a = 1; a < 3; ++a)
        if (d[a] != 0.0) t = std::min(t, ((d[a] > 0.0 ? kWall : -kWall) - s[a]) / d[a]);
    for (int b = 0; b < 12; ++b) {
        const double lo[3] = {2.0 + 2.4 * b, b % 2 ? 0.35 : -0.95, -kWall}, hi[3] = {lo[0] + 0.6, lo[1] + 0.6, -0.25};
        double t0 = 0.0, t1 = t;
        for (int a = 0; a < 3 && t0 <= t1; ++a) {
            if (d[a] == 0.0) { if (s[a] < lo[a] || s[a] > hi[a]) t1 = -1.0; continue; }
            const double ta = (lo[a] - s[a]) / d[a], tb = (hi[a] - s[a]) / d[a];
            t0 = std::max(t0, std::min(ta, tb));
            t1 = std::min(t1, std::max(ta, tb));
        }
        if (t0 <= t1 && t0 > 0.0) t = std::min(t, t0);
    }
    for (int a = 0; a < 3; ++a) end[a] = s[a] + t * d[a];
}

// a 24 x 24 image looking along +x with a 90 degree field of view; returns beyond the range come back truncated by the map
std::vector<float> Frame(const int k) {
    const double s[3] = {SensorX(k), 0.0, 0.0};
    std::vector<float> points;
    for (int i = 0; i < kPixels; ++i)
        for (int j = 0; j < kPixels; ++j) {
            const double d[3] = {1.0, (i + 0.5) / kPixels * 2.0 - 1.0, (j + 0.5) / kPixels * 2.0 - 1.0};
            double end[3];
            Cast(s, d, end);
            for (int a = 0; a < 3; ++a) points.push_back((float)(end[a] - 1e-3 * d[a]));       // just inside the corridor
        }
    return points;
}

int64_t CellOf(const double x) { return (int64_t)std::floor(x / kCell); }

VoxelGrid::GRID_INDEX RegionLower(const int k) { return VoxelGrid::GRID_INDEX(CellOf(SensorX(k)) - kBehind, -kSide, -kSide); }

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "";
    try {
        const sdf_tools::COLLISION_CELL unknown(0.5f);
        // 1. a limited map that never forgets: refused once the pool is full
        int refused_at = -1;
        {
            Map stuck(Eigen::Isometry3d::Identity(), "world", kCell, 8, 8, 8, unknown, kByteLimit);
            for (int k = 0; k < kFrames && refused_at < 0; ++k) {
                try {
                    stuck.FusePointCloudRays(Frame(k), Eigen::Vector3d(SensorX(k), 0.0, 0.0), kRange);
                } catch (const std::runtime_error& e) {
                    refused_at = k;
                    std::cout << "without RetainBox frame " << k << " is refused: " << e.what() << std::endl;
                }
            }
            if (refused_at < 0) throw std::runtime_error("the limited map took every frame without forgetting: the limit is not one");
            bool again = false;
            try { stuck.FusePointCloudRays(Frame(refused_at), Eigen::Vector3d(SensorX(refused_at), 0.0, 0.0), kRange); } catch (const std::runtime_error&) { again = true; }
            if (!again) throw std::runtime_error("the stuck map took the frame it had refused");
        }
        // 2. the same limit with RetainBox in front of every frame, beside a map without a limit
        Map sliding(Eigen::Isometry3d::Identity(), "world", kCell, 8, 8, 8, unknown, kByteLimit);
        Map whole("world", kCell, 8, 8, 8, unknown);
        uint64_t most_held = 0;
        for (int k = 0; k < kFrames; ++k) {
            const std::vector<float> points = Frame(k);
            const Eigen::Vector3d sensor(SensorX(k), 0.0, 0.0);
            const int64_t forgotten = sliding.RetainBox(RegionLower(k), kBehind + kAhead, 2 * kSide, 2 * kSide);
            const sdfgpu_dsh_ray_counts counts = sliding.FusePointCloudRays(points, sensor, kRange);
            whole.FusePointCloudRays(points, sensor, kRange);
            const sdfgpu_dsh_counts held = sliding.GetCounts();
            most_held = std::max(most_held, (uint64_t)held.bytes_held);
            std::cout << "frame " << k << ": " << forgotten << " chunks forgotten, " << counts.new_chunks << " new chunks, " << held.chunk_filled + held.cell_filled
                      << " chunks live, " << held.bytes_held << " bytes held" << std::endl;
            if (held.bytes_held > kByteLimit) throw std::runtime_error("the sliding map passed its byte limit");
            Write(dir, "frame_" + std::to_string(k) + ".f32", points.data(), points.size());
        }
        const int last = kFrames - 1;
        // behind the robot: nothing is found any more (the whole map still knows the place)
        std::vector<double> behind;
        for (int k = 0; k < 8; ++k) { behind.push_back(SensorX(k)); behind.push_back(0.05); behind.push_back(0.05); }
        const auto forgotten = sliding.GetBatch(behind);
        const auto remembered = whole.GetBatch(behind);
        for (size_t i = 0; i < forgotten.second.size(); ++i) {
            if (forgotten.second[i] != VoxelGrid::NOT_FOUND) throw std::runtime_error("the sliding map still finds a cell behind the robot");
            if (remembered.second[i] == VoxelGrid::NOT_FOUND) throw std::runtime_error("the whole map lost a cell it had seen");
        }
        // at the robot: the window of the sliding map is the window of the whole map, records and signed distance field
        const VoxelGrid::GRID_INDEX lower(CellOf(SensorX(last)) - 8, -14, -14);              // 48 x 28 x 28 cells: the walls are inside
        const sdf_tools::CollisionMapGrid a = sliding.ExtractCollisionMapGrid(lower, 48, 28, 28), b = whole.ExtractCollisionMapGrid(lower, 48, 28, 28);
        const auto sdf_a = sliding.ExtractSignedDistanceField(lower, 48, 28, 28, 1e6f, false, false);
        const auto sdf_b = whole.ExtractSignedDistanceField(lower, 48, 28, 28, 1e6f, false, false);
        const auto& cells_a = a.GetImmutableRawData();
        const auto& cells_b = b.GetImmutableRawData();
        const auto& dist_a = sdf_a.first.GetImmutableRawData();
        const auto& dist_b = sdf_b.first.GetImmutableRawData();
        if (cells_a.size() != cells_b.size() || std::memcmp(static_cast<const void*>(cells_a.data()), static_cast<const void*>(cells_b.data()), cells_a.size() * sizeof(cells_a[0])) != 0)
            throw std::runtime_error("the sliding map's window differs from the whole map's");
        if (dist_a.size() != dist_b.size() || std::memcmp(dist_a.data(), dist_b.data(), dist_a.size() * sizeof(dist_a[0])) != 0)
            throw std::runtime_error("the sliding map's signed distance field differs from the whole map's");
        size_t obstacle = 0;
        for (const float d : dist_a) obstacle += d < 0.0f;
        if (!obstacle || obstacle == dist_a.size()) throw std::runtime_error("the window shows no obstacle, or nothing else");
        Write(dir, "window.cells", cells_a.data(), cells_a.size());
        Write(dir, "window_sdf.f32", dist_a.data(), dist_a.size());
        const sdfgpu_dsh_counts kept = sliding.GetCounts(), all = whole.GetCounts();
        std::cout << "the sliding map ends with " << kept.chunk_filled + kept.cell_filled << " chunks in " << kept.bytes_held << " bytes (at most " << most_held
                  << ", limit " << kByteLimit << "); the whole map holds " << all.chunk_filled + all.cell_filled << " chunks in " << all.bytes_held << " bytes" << std::endl;
        std::cout << "without RetainBox the limited map was stuck from frame " << refused_at << " on" << std::endl;
        sliding.ShrinkToFit(16);
        std::cout << "after ShrinkToFit(16) the sliding map holds " << sliding.GetCounts().bytes_held << " bytes" << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "dsh_sliding example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "dsh_sliding example done" << std::endl;
    return 0;
}
