// dsh_class_check.cpp -- sdf_tools::DynamicSpatialHashedCollisionMapGrid as a C++ client sees it: the reference's signatures (compile
// time), what an uninitialised map answers (no GPU needed: `dsh_class_check cpu` stops there), and, on a GPU, the state changes
// through the single-call methods and the fields of ExportForDisplay's markers.  Prints "dsh class OK" and returns 0, or says what
// failed and returns 1.  tests/test_dsh_cpu.py and tests/test_gpu_dsh_cpp.py build and run it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>

#include "sdf_tools/dynamic_spatial_hashed_collision_map.hpp"

using sdf_tools::COLLISION_CELL;
using Map = sdf_tools::DynamicSpatialHashedCollisionMapGrid;

// ---- the reference's signatures (include/sdf_tools/dynamic_spatial_hashed_collision_map.hpp:27-51) ------------------------------------------
static_assert(std::is_constructible<Map, std::string, double, int64_t, int64_t, int64_t, COLLISION_CELL>::value, "frame constructor");
static_assert(std::is_constructible<Map, Eigen::Isometry3d, std::string, double, int64_t, int64_t, int64_t, COLLISION_CELL>::value, "origin constructor");
static_assert(std::is_default_constructible<Map>::value, "default constructor");
using GetResult = std::pair<COLLISION_CELL, VoxelGrid::FOUND_STATUS>;
static_assert(std::is_same<decltype(static_cast<bool (Map::*)() const>(&Map::IsInitialized)), bool (Map::*)() const>::value, "IsInitialized");
static_assert(std::is_same<decltype(static_cast<bool (Map::*)() const>(&Map::AreComponentsValid)), bool (Map::*)() const>::value, "AreComponentsValid");
static_assert(std::is_same<decltype(std::declval<const Map&>().Get(0.0, 0.0, 0.0)), GetResult>::value, "Get(x, y, z)");
static_assert(std::is_same<decltype(std::declval<const Map&>().Get(std::declval<const Eigen::Vector3d&>())), GetResult>::value, "Get(location)");
static_assert(std::is_same<decltype(std::declval<Map&>().SetCell(0.0, 0.0, 0.0, COLLISION_CELL())), VoxelGrid::SET_STATUS>::value, "SetCell(x, y, z)");
static_assert(std::is_same<decltype(std::declval<Map&>().SetCell(std::declval<const Eigen::Vector3d&>(), COLLISION_CELL())), VoxelGrid::SET_STATUS>::value, "SetCell");
static_assert(std::is_same<decltype(std::declval<Map&>().SetChunk(0.0, 0.0, 0.0, COLLISION_CELL())), VoxelGrid::SET_STATUS>::value, "SetChunk(x, y, z)");
static_assert(std::is_same<decltype(std::declval<Map&>().SetChunk(std::declval<const Eigen::Vector3d&>(), COLLISION_CELL())), VoxelGrid::SET_STATUS>::value, "SetChunk");
static_assert(std::is_same<decltype(std::declval<const Map&>().GetOriginTransform()), Eigen::Isometry3d>::value, "GetOriginTransform");
static_assert(std::is_same<decltype(std::declval<const Map&>().ExportForDisplay(std::declval<const std_msgs::ColorRGBA&>(), std::declval<const std_msgs::ColorRGBA&>(),
                                                                                std::declval<const std_msgs::ColorRGBA&>())),
                           std::vector<visualization_msgs::Marker>>::value, "ExportForDisplay");
static_assert(VoxelGrid::NOT_FOUND == 0 && VoxelGrid::FOUND_IN_CHUNK == 1 && VoxelGrid::FOUND_IN_CELL == 2, "FOUND_STATUS");
static_assert(VoxelGrid::NOT_SET == 0 && VoxelGrid::SET_CHUNK == 1 && VoxelGrid::SET_CELL == 2, "SET_STATUS");

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

template <typename Call>
static bool Throws(Call call) {
    try { call(); } catch (const std::runtime_error&) { return true; }
    return false;
}

static bool Same(const std_msgs::ColorRGBA& a, const std_msgs::ColorRGBA& b) { return a.r == b.r && a.g == b.g && a.b == b.b && a.a == b.a; }

static void Uninitialised() {
    Map map;
    std_msgs::ColorRGBA c;
    CHECK(!map.IsInitialized() && !map.AreComponentsValid());
    CHECK(map.Get(0.0, 0.0, 0.0).second == VoxelGrid::NOT_FOUND && map.Get(Eigen::Vector3d(1, 2, 3)).first.occupancy == 0.0f);
    CHECK(map.SetCell(0.0, 0.0, 0.0, COLLISION_CELL(1.0f)) == VoxelGrid::NOT_SET && map.SetChunk(Eigen::Vector3d(1, 2, 3), COLLISION_CELL(1.0f)) == VoxelGrid::NOT_SET);
    CHECK(map.ExportForDisplay(c, c, c).empty());
    CHECK(Throws([&] { map.SetCells({0.0, 0.0, 0.0}, {COLLISION_CELL(1.0f)}); }));
    CHECK(Throws([&] { map.SetChunks({0.0, 0.0, 0.0}, {COLLISION_CELL(1.0f)}); }));
    CHECK(Throws([&] { map.GetBatch({0.0, 0.0, 0.0}); }));
    CHECK(Throws([&] { map.InsertPointCloud({0.0f, 0.0f, 0.0f}, COLLISION_CELL(1.0f)); }));
    CHECK(Throws([&] { map.ExtractCollisionMapGrid(VoxelGrid::GRID_INDEX(0, 0, 0), 2, 2, 2); }));
    CHECK(Throws([&] { map.ExtractSignedDistanceField(VoxelGrid::GRID_INDEX(0, 0, 0), 2, 2, 2, 1.0f, false, false); }));
    CHECK(Throws([&] { map.ExtractSignedDistanceFieldDevice(VoxelGrid::GRID_INDEX(0, 0, 0), 2, 2, 2, 1.0f, false, false); }));
    CHECK(map.DeviceMapHandle() == nullptr);
}

static void OnTheGpu() {
    Eigen::Isometry3d origin;
    origin.setTranslation(1.0, -2.0, 0.5);
    Map map(origin, "map_frame", 0.25, 2, 3, 4, COLLISION_CELL(0.5f, 9u));
    CHECK(map.IsInitialized() && !map.AreComponentsValid() && map.GetOriginTransform().translation().y() == -2.0);
    std_msgs::ColorRGBA red, green, blue;
    red.r = red.a = 1.0f; green.g = green.a = 1.0f; blue.b = 1.0f; blue.a = 0.5f;
    CHECK(map.ExportForDisplay(red, green, blue).empty());                                   // an empty map: no marker
    CHECK(map.Get(1.1, -1.9, 0.6).second == VoxelGrid::NOT_FOUND && map.Get(1.1, -1.9, 0.6).first.component == 9u);
    CHECK(map.SetCell(NAN, 0.0, 0.0, COLLISION_CELL(1.0f)) == VoxelGrid::NOT_SET && map.ExportForDisplay(red, green, blue).empty());
    // chunk (0, 0, 0) chunk-filled and free, chunk (-1, 0, 0) chunk-filled and unknown: one marker
    CHECK(map.SetChunk(1.1, -1.9, 0.6, COLLISION_CELL(0.0f, 1u)) == VoxelGrid::SET_CHUNK);
    CHECK(map.SetChunk(Eigen::Vector3d(0.9, -1.9, 0.6), COLLISION_CELL(0.5f, 2u)) == VoxelGrid::SET_CHUNK);
    CHECK(map.Get(1.4, -1.3, 1.4).second == VoxelGrid::FOUND_IN_CHUNK && map.Get(1.4, -1.3, 1.4).first.component == 1u);
    std::vector<visualization_msgs::Marker> markers = map.ExportForDisplay(red, green, blue);
    CHECK(markers.size() == 1);
    if (markers.size() == 1) {
        const visualization_msgs::Marker& m = markers[0];
        CHECK(m.ns == "dynamic_spatial_hashed_collision_map_chunks_display" && m.id == 1 && m.type == visualization_msgs::Marker::CUBE_LIST);
        CHECK(m.action == visualization_msgs::Marker::ADD && m.lifetime == 0.0 && !m.frame_locked && m.header.frame_id == "map_frame");
        CHECK(m.scale.x == 0.5 && m.scale.y == 0.75 && m.scale.z == 1.0);
        CHECK(m.pose.position.x == 0.0 && m.pose.position.y == 0.0 && m.pose.position.z == 0.0 && m.pose.orientation.w == 1.0 && m.pose.orientation.x == 0.0);
        CHECK(m.points.size() == 2 && m.colors.size() == 2);
        if (m.points.size() == 2) {                                                          // ascending chunk order: (-1, 0, 0) first; centres
            CHECK(m.points[0].x == 1.0 - 0.25 && m.points[0].y == -2.0 + 0.375 && m.points[0].z == 0.5 + 0.5 && Same(m.colors[0], blue));
            CHECK(m.points[1].x == 1.0 + 0.25 && m.points[1].y == -2.0 + 0.375 && m.points[1].z == 0.5 + 0.5 && Same(m.colors[1], green));
        }
    }
    // a cell set turns chunk (0, 0, 0) into cells: the other 23 keep the chunk's record; two markers
    CHECK(map.SetCell(1.3, -1.4, 0.8, COLLISION_CELL(1.0f, 3u)) == VoxelGrid::SET_CELL);     // cell (1, 2, 1)
    CHECK(map.Get(1.3, -1.4, 0.8).second == VoxelGrid::FOUND_IN_CELL && map.Get(1.3, -1.4, 0.8).first.occupancy == 1.0f);
    CHECK(map.Get(1.1, -1.9, 0.6).second == VoxelGrid::FOUND_IN_CELL && map.Get(1.1, -1.9, 0.6).first.component == 1u);
    markers = map.ExportForDisplay(red, green, blue);
    CHECK(markers.size() == 2);
    if (markers.size() == 2) {
        const visualization_msgs::Marker& m = markers[1];
        CHECK(markers[0].points.size() == 1 && Same(markers[0].colors[0], blue));
        CHECK(m.ns == "dynamic_spatial_hashed_collision_map_cells_display" && m.id == 1 && m.type == visualization_msgs::Marker::CUBE_LIST && m.header.frame_id == "map_frame");
        CHECK(m.scale.x == 0.25 && m.scale.y == 0.25 && m.scale.z == 0.25 && m.points.size() == 24 && m.colors.size() == 24);
        size_t reds = 0, greens = 0;
        for (const std_msgs::ColorRGBA& c : m.colors) { reds += Same(c, red); greens += Same(c, green); }
        CHECK(reds == 1 && greens == 23);
        const size_t at = (1 * 3 + 2) * 4 + 1;                                               // x -> y -> z inside the chunk
        if (m.points.size() == 24) {
            CHECK(Same(m.colors[at], red) && m.points[at].x == 1.0 + 1.5 * 0.25 && m.points[at].y == -2.0 + 2.5 * 0.25 && m.points[at].z == 0.5 + 1.5 * 0.25);
            CHECK(m.points[0].x == 1.125 && m.points[0].y == -1.875 && m.points[0].z == 0.625);
        }
    }
    // batches and the window through the class
    const std::vector<VoxelGrid::SET_STATUS> st = map.SetCells({1.3, -1.4, 0.8, INFINITY, 0.0, 0.0, 1.3, -1.4, 0.8}, {COLLISION_CELL(0.0f, 4u), COLLISION_CELL(0.0f, 5u), COLLISION_CELL(0.75f, 6u)});
    CHECK(st.size() == 3 && st[0] == VoxelGrid::SET_CELL && st[1] == VoxelGrid::NOT_SET && st[2] == VoxelGrid::SET_CELL);
    CHECK(map.Get(1.3, -1.4, 0.8).first.component == 6u);
    const sdf_tools::CollisionMapGrid grid = map.ExtractCollisionMapGrid(VoxelGrid::GRID_INDEX(-1, 0, 0), 3, 3, 4);
    CHECK(grid.GetImmutable((int64_t)2, (int64_t)2, (int64_t)1).first.component == 6u && grid.GetImmutable((int64_t)0, (int64_t)0, (int64_t)0).first.component == 2u);
    CHECK(grid.GetOriginTransform().translation().x() == 0.75 && grid.GetOriginTransform().translation().y() == -2.0);
    const auto got = map.GetBatch({1.3, -1.4, 0.8, 100.0, 100.0, 100.0});
    CHECK(got.second.size() == 2 && got.second[0] == VoxelGrid::FOUND_IN_CELL && got.second[1] == VoxelGrid::NOT_FOUND && got.first[1].component == 9u);
    CHECK(map.InsertPointCloud({1.1f, -1.9f, 0.6f, NAN, 0.0f, 0.0f}, COLLISION_CELL(1.0f, 8u)) == 1 && map.Get(1.1, -1.9, 0.6).first.component == 8u);
    const Map alias = map;                                                                   // a copy names the same device map
    CHECK(alias.Get(1.1, -1.9, 0.6).first.component == 8u && alias.DeviceMapHandle() == map.DeviceMapHandle());
}

int main(int argc, char** argv) {
    Uninitialised();
    if (!(argc > 1 && std::string(argv[1]) == "cpu")) {
        try {
            OnTheGpu();
        } catch (const std::exception& e) {
            std::printf("FAILED: %s\n", e.what());
            ++failures;
        }
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("dsh class OK\n");
    return 0;
}
