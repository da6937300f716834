// dsh_remove_class_check.cpp -- the removal methods of sdf_tools::DynamicSpatialHashedCollisionMapGrid (additions of this project;
// DESIGN.md section 32) as a C++ client sees them: their signatures (compile time), what an uninitialised map answers (no GPU
// needed: `dsh_remove_class_check cpu` stops there), and, on a GPU, each of them once.  Prints "dsh remove class OK" and returns 0,
// or says what failed and returns 1.  tests/test_dsh_remove_cpu.py and tests/test_gpu_dsh_remove_cpp.py build and run it.
#include <cmath>
#include <cstdio>
#include <string>
#include <type_traits>

#include "sdf_tools/dynamic_spatial_hashed_collision_map.hpp"

using sdf_tools::COLLISION_CELL;
using Map = sdf_tools::DynamicSpatialHashedCollisionMapGrid;

static_assert(std::is_same<decltype(std::declval<Map&>().RemoveChunk(0.0, 0.0, 0.0)), bool>::value, "RemoveChunk(x, y, z)");
static_assert(std::is_same<decltype(std::declval<Map&>().RemoveChunk(std::declval<const Eigen::Vector3d&>())), bool>::value, "RemoveChunk(location)");
static_assert(std::is_same<decltype(std::declval<Map&>().RemoveChunks(std::declval<const std::vector<double>&>())), std::vector<bool>>::value, "RemoveChunks");
static_assert(std::is_same<decltype(std::declval<Map&>().RetainBox(VoxelGrid::GRID_INDEX(), 1, 1, 1)), int64_t>::value, "RetainBox");
static_assert(std::is_same<decltype(std::declval<Map&>().RemoveBox(VoxelGrid::GRID_INDEX(), 1, 1, 1)), int64_t>::value, "RemoveBox");
static_assert(std::is_same<decltype(std::declval<Map&>().Clear()), int64_t>::value, "Clear");
static_assert(std::is_same<decltype(std::declval<Map&>().ShrinkToFit()), void>::value, "ShrinkToFit()");
static_assert(std::is_same<decltype(std::declval<Map&>().ShrinkToFit((int64_t)3)), void>::value, "ShrinkToFit(spare)");
static_assert(SDFGPU_DSH_CHUNK_NOT_REMOVED == 0 && SDFGPU_DSH_CHUNK_REMOVED == 1, "the removal's status byte");

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

template <typename Call>
static bool Refuses(Call call) {                                                 // SDFGPU_ERR_INVALID_ARGUMENT arrives as std::invalid_argument
    try { call(); } catch (const std::invalid_argument&) { return true; }
    return false;
}

static void Uninitialised() {
    Map map;
    CHECK(!map.IsInitialized() && !map.AreComponentsValid());
    CHECK(!map.RemoveChunk(0.0, 0.0, 0.0) && !map.RemoveChunk(Eigen::Vector3d(1, 2, 3)) && map.Clear() == 0);
    CHECK(Throws([&] { map.RemoveChunks({0.0, 0.0, 0.0}); }));
    CHECK(Throws([&] { map.RetainBox(VoxelGrid::GRID_INDEX(0, 0, 0), 2, 2, 2); }));
    CHECK(Throws([&] { map.RemoveBox(VoxelGrid::GRID_INDEX(0, 0, 0), 2, 2, 2); }));
    CHECK(Throws([&] { map.ShrinkToFit(); }));
    CHECK(map.DeviceMapHandle() == nullptr);
}

static void OnTheGpu() {
    Map map("map_frame", 1.0, 2, 2, 2, COLLISION_CELL(0.5f, 99u));
    // chunks 0 .. 9 along x: even ones cell-filled, odd ones chunk-filled
    for (int k = 0; k < 10; ++k) {
        if (k % 2) CHECK(map.SetChunk(2.0 * k + 0.5, 0.5, 0.5, COLLISION_CELL(1.0f, (uint32_t)k)) == VoxelGrid::SET_CHUNK);
        else CHECK(map.SetCell(2.0 * k + 0.5, 0.5, 0.5, COLLISION_CELL(1.0f, (uint32_t)k)) == VoxelGrid::SET_CELL);
    }
    CHECK(map.GetCounts().chunk_filled == 5 && map.GetCounts().cell_filled == 5);
    CHECK(map.RemoveChunk(0.5, 0.5, 0.5) && !map.RemoveChunk(0.5, 0.5, 0.5) && !map.RemoveChunk(NAN, 0.0, 0.0) && !map.RemoveChunk(Eigen::Vector3d(100.5, 0.5, 0.5)));
    CHECK(map.Get(0.5, 0.5, 0.5).second == VoxelGrid::NOT_FOUND && map.Get(0.5, 0.5, 0.5).first.component == 99u);
    CHECK(map.Get(18.5, 0.5, 0.5).second == VoxelGrid::FOUND_IN_CHUNK && map.Get(18.5, 0.5, 0.5).first.component == 9u);   // chunk 9 moved into the hole: still found
    CHECK(map.Get(16.5, 0.5, 0.5).second == VoxelGrid::FOUND_IN_CELL && map.Get(16.5, 0.5, 0.5).first.component == 8u);
    const std::vector<bool> st = map.RemoveChunks({2.5, 0.5, 0.5, 2.5, 1.5, 1.5, INFINITY, 0.0, 0.0, 4.5, 0.5, 0.5, 0.5, 0.5, 0.5});
    CHECK(st.size() == 5 && st[0] && !st[1] && !st[2] && st[3] && !st[4]);
    CHECK(map.GetCounts().chunk_filled == 4 && map.GetCounts().cell_filled == 3);
    // a fresh cell-filled chunk where one was removed: its other cells are the default
    CHECK(map.SetCell(4.5, 0.5, 0.5, COLLISION_CELL(0.0f, 77u)) == VoxelGrid::SET_CELL);
    CHECK(map.Get(5.5, 1.5, 1.5).second == VoxelGrid::FOUND_IN_CELL && map.Get(5.5, 1.5, 1.5).first.component == 99u && map.Get(4.5, 0.5, 0.5).first.component == 77u);
    // cells 13 .. 16 along x: chunks 6, 7 and 8 hold one; everything else goes (chunks 2, 3, 4, 5, 9)
    CHECK(map.RetainBox(VoxelGrid::GRID_INDEX(13, -5, 0), 4, 10, 1) == 5);
    CHECK(map.GetCounts().chunk_filled == 1 && map.GetCounts().cell_filled == 2);
    CHECK(map.RemoveBox(VoxelGrid::GRID_INDEX(15, 1, 1), 1, 1, 1) == 1 && map.Get(14.5, 0.5, 0.5).second == VoxelGrid::NOT_FOUND);
    CHECK(map.Get(12.5, 0.5, 0.5).first.component == 6u && map.Get(16.5, 0.5, 0.5).first.component == 8u);
    const sdfgpu_dsh_counts before = map.GetCounts();
    map.ShrinkToFit(3);
    const sdfgpu_dsh_counts after = map.GetCounts();
    CHECK(before.capacity_chunks == 64 && after.capacity_chunks == 5 && after.table_capacity == 16 && after.bytes_held == 16 * 12 + 5 * (24 + 8 * 8));
    CHECK(map.Get(12.5, 0.5, 0.5).first.component == 6u && map.Get(16.5, 0.5, 0.5).first.component == 8u);
    CHECK(map.Clear() == 2 && map.Clear() == 0 && map.GetCounts().chunk_filled + map.GetCounts().cell_filled == 0);
    CHECK(map.Get(12.5, 0.5, 0.5).second == VoxelGrid::NOT_FOUND && !map.AreComponentsValid());
    CHECK(Refuses([&] { map.RetainBox(VoxelGrid::GRID_INDEX(((int64_t)1 << 40) + 1, 0, 0), 1, 1, 1); }));
    CHECK(Refuses([&] { map.RemoveBox(VoxelGrid::GRID_INDEX(0, 0, 0), 1, -1, 1); }));
    CHECK(Refuses([&] { map.ShrinkToFit(-1); }));
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
    std::printf("dsh remove class OK\n");
    return 0;
}
