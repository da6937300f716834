// dsh_cast -- asking a sensed map what a ray meets first, on sdf_tools::DynamicSpatialHashedCollisionMapGrid::CastRays / CastSegments /
// CastRay: a depth camera looks along +x at a wall with a box in front of it (the scene of dsh_rays) and one frame is carved into the
// map.  Then the map predicts the scan of a camera at a second pose: each ray stops at the first filled cell, runs out of range, or
// ends in free or unknown space.  Last, line of sight between surface cells: the segment between two cells' centres with both of
// its end cells left out of the test.
// Usage: dsh_cast_example [output directory]
// With a directory, what the example asked and got is written there as raw arrays for tests/test_gpu_dsh_cast_cpp.py:
//   frame.f32 (the carved frame's points, x y z), scan.f32 (the predicted scan's points), los_starts.f64 / los_ends.f64, and per query
//   <name>_status.u8, _cell.i64, _record.u64, _t.f64, _step.u32, _found.u32, _distance.f64 for name in scan, los, los_unknown
// The map's numbers (cell size, chunk size, the two sensors, the ranges) are repeated in that test.
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

const double kSensor[3] = {0.025, 1.225, 1.225};
const double kSecondSensor[3] = {0.025, 0.375, 1.875};

// The frame of dsh_rays with the box: a 48 x 48 image of the wall x = 3.0, the box [1.5, 2.0] x [0.9, 1.5] x [0.9, 1.5] in front.
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

// The second camera's image, 40 x 40 pixels: four rows in five look at the plane x = 3.6 behind the wall, every fifth row ends at
// x = 1.2 in front of the box; every 89th pixel has no return to predict (NaN).
std::vector<float> Scan() {
    std::vector<float> points;
    for (int i = 0; i < 40; ++i)
        for (int j = 0; j < 40; ++j) {
            const double end[3] = {i % 5 == 0 ? 1.2 : 3.6, -0.4 + 0.07 * i, -0.2 + 0.07 * j};
            const bool no_pixel = (i * 40 + j) % 89 == 88;
            for (int a = 0; a < 3; ++a) points.push_back(no_pixel ? NAN : (float)end[a]);
        }
    return points;
}

void Report(const std::string& dir, const std::string& name, const std::vector<Map::RayCast>& casts) {
    size_t by_status[4] = {0, 0, 0, 0};
    std::vector<uint8_t> status;
    std::vector<int64_t> cell;
    std::vector<sdf_tools::COLLISION_CELL> record;
    std::vector<double> t, distance;
    std::vector<uint32_t> step, found;
    for (const Map::RayCast& c : casts) {
        by_status[c.status] += 1;
        status.push_back((uint8_t)c.status);
        cell.push_back(c.cell.x); cell.push_back(c.cell.y); cell.push_back(c.cell.z);
        record.push_back(c.value);
        t.push_back(c.t);
        distance.push_back(c.distance);
        step.push_back(c.step);
        found.push_back((uint32_t)c.found);
    }
    std::cout << name << ": " << by_status[Map::CAST_BLOCKED] << " blocked, " << by_status[Map::CAST_CLEAR] << " clear, " << by_status[Map::CAST_CLEAR_IN_RANGE]
              << " clear in range, " << by_status[Map::CAST_SKIPPED] << " skipped" << std::endl;
    Write(dir, name + "_status.u8", status.data(), status.size());
    Write(dir, name + "_cell.i64", cell.data(), cell.size());
    Write(dir, name + "_record.u64", record.data(), record.size());
    Write(dir, name + "_t.f64", t.data(), t.size());
    Write(dir, name + "_distance.f64", distance.data(), distance.size());
    Write(dir, name + "_step.u32", step.data(), step.size());
    Write(dir, name + "_found.u32", found.data(), found.size());
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "";
    try {
        sdf_tools::DynamicSpatialHashedCollisionMapGrid seen("world", 0.05, 8, 8, 8, sdf_tools::COLLISION_CELL(0.5f));
        const std::vector<float> frame = Frame();
        const sdfgpu_dsh_ray_counts counts = seen.InsertPointCloudRays(frame, Eigen::Vector3d(kSensor[0], kSensor[1], kSensor[2]), 4.0,
                                                                       sdf_tools::COLLISION_CELL(0.0f), sdf_tools::COLLISION_CELL(1.0f));
        std::cout << "frame: " << counts.rays_hit << " hits, " << counts.cells_carved << " cells carved" << std::endl;
        Write(dir, "frame.f32", frame.data(), frame.size());
        const Map& map = seen;                                          // every cast is const: the map is read, not written

        // the predicted scan from the second pose: unknown space does not block, the range ends some rays in front of the wall
        const std::vector<float> scan = Scan();
        const std::vector<Map::RayCast> predicted = map.CastRays(scan, Eigen::Vector3d(kSecondSensor[0], kSecondSensor[1], kSecondSensor[2]), 3.2, false);
        Write(dir, "scan.f32", scan.data(), scan.size());
        Report(dir, "scan", predicted);

        // line of sight between surface cells, both end cells excepted: box face -> box face (the face's own cells are in the way),
        // box face -> first camera (free), box face -> wall beside the box's shadow, wall -> wall along the wall
        const double face[3] = {1.525, 1.225, 1.225}, face_corner[3] = {1.525, 0.925, 1.475}, wall_a[3] = {3.025, 0.225, 0.225}, wall_b[3] = {3.025, 2.225, 0.225};
        std::vector<double> starts, ends;
        const double* pairs[][2] = {{face, face_corner}, {face, kSensor}, {face, wall_a}, {wall_a, wall_b}, {kSecondSensor, wall_a}, {face_corner, wall_b}};
        for (const auto& pair : pairs)
            for (int a = 0; a < 3; ++a) { starts.push_back(pair[0][a]); ends.push_back(pair[1][a]); }
        Write(dir, "los_starts.f64", starts.data(), starts.size());
        Write(dir, "los_ends.f64", ends.data(), ends.size());
        const std::vector<Map::RayCast> sight = map.CastSegments(starts, ends, 4.0, false, true, true);
        Report(dir, "los", sight);
        Report(dir, "los_unknown", map.CastSegments(starts, ends, 4.0, true, true, true));     // the same, with unknown space in the way

        const Map::RayCast one = map.CastRay(Eigen::Vector3d(face[0], face[1], face[2]), Eigen::Vector3d(kSensor[0], kSensor[1], kSensor[2]), 4.0, false, true, true);
        std::cout << "the box's face sees the first camera: " << (one.status == Map::CAST_CLEAR ? "yes" : "no") << ", " << one.step << " cells, " << one.distance
                  << " m to the last one" << std::endl;
        if (one.status != Map::CAST_CLEAR || sight[1].status != Map::CAST_CLEAR) throw std::runtime_error("the carved rays' own path is not clear");
        if (sight[0].status != Map::CAST_BLOCKED) throw std::runtime_error("the box's face does not block the segment along it");
        size_t blocked = 0;
        for (const Map::RayCast& c : predicted) blocked += c.status == Map::CAST_BLOCKED;
        if (blocked == 0) throw std::runtime_error("the predicted scan meets neither the box nor the wall");
    } catch (const std::exception& e) {
        std::cerr << "dsh_cast example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "dsh_cast example done" << std::endl;
    return 0;
}
