// dsh_frontier_class_check.cpp -- the frontier methods of sdf_tools::DynamicSpatialHashedCollisionMapGrid (additions of this project;
// DESIGN.md section 34) as a C++ client sees them: their signatures (compile time), what an uninitialised map answers (no GPU
// needed: `dsh_frontier_class_check cpu` stops there), and, on a GPU, each of them once on a hand-worked map.  Prints
// "dsh frontier class OK" and returns 0, or says what failed and returns 1.  tests/test_dsh_frontier_cpu.py and
// tests/test_gpu_dsh_frontier_cpp.py build and run it.
#include <cstdio>
#include <string>
#include <type_traits>

#include "sdf_tools/dynamic_spatial_hashed_collision_map.hpp"

using sdf_tools::COLLISION_CELL;
using Map = sdf_tools::DynamicSpatialHashedCollisionMapGrid;
using Index = VoxelGrid::GRID_INDEX;

// all three are const, and their defaults are the stated ones (use_26 false for the lists and the bits, min_cells 1 and use_26 true for the clusters)
static_assert(std::is_same<decltype(std::declval<const Map&>().ExtractFrontierCells()), std::vector<Index>>::value, "ExtractFrontierCells()");
static_assert(std::is_same<decltype(std::declval<const Map&>().ExtractFrontierCells(true)), std::vector<Index>>::value, "ExtractFrontierCells(use_26)");
static_assert(std::is_same<decltype(std::declval<const Map&>().ExtractFrontierCells(Index(), (int64_t)1, (int64_t)1, (int64_t)1)), std::vector<Index>>::value,
              "ExtractFrontierCells(lower_index, nx, ny, nz)");
static_assert(std::is_same<decltype(std::declval<const Map&>().ExtractFrontierCells(Index(), (int64_t)1, (int64_t)1, (int64_t)1, true)), std::vector<Index>>::value,
              "ExtractFrontierCells(lower_index, nx, ny, nz, use_26)");
static_assert(std::is_same<decltype(std::declval<const Map&>().ExtractFrontierWindowBits(Index(), (int64_t)1, (int64_t)1, (int64_t)1)), std::vector<uint32_t>>::value,
              "ExtractFrontierWindowBits");
static_assert(std::is_same<decltype(std::declval<const Map&>().ExtractFrontierClusters(Index(), (int64_t)1, (int64_t)1, (int64_t)1)), std::vector<Map::FrontierCluster>>::value,
              "ExtractFrontierClusters(lower_index, nx, ny, nz)");
static_assert(std::is_same<decltype(std::declval<const Map&>().ExtractFrontierClusters(Index(), (int64_t)1, (int64_t)1, (int64_t)1, (int64_t)2, false)),
                           std::vector<Map::FrontierCluster>>::value, "ExtractFrontierClusters(lower_index, nx, ny, nz, min_cells, use_26)");
static_assert(std::is_same<decltype(Map::FrontierCluster::label), uint32_t>::value && std::is_same<decltype(Map::FrontierCluster::cells), int64_t>::value &&
                  std::is_same<decltype(Map::FrontierCluster::lower), Index>::value && std::is_same<decltype(Map::FrontierCluster::upper), Index>::value &&
                  std::is_same<decltype(Map::FrontierCluster::centroid), Eigen::Vector3d>::value, "FrontierCluster {label, cells, lower, upper, centroid}");
static_assert(SDFGPU_DSH_FRONTIER_26 == 1 && sizeof(sdfgpu_component_stats) == 64, "the flag and the statistics record");

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

template <typename Call>
static bool Throws(Call call) {
    try { call(); } catch (const std::invalid_argument&) { return false; } catch (const std::runtime_error&) { return true; }
    return false;
}

template <typename Call>
static bool Refuses(Call call) {                                                 // SDFGPU_ERR_INVALID_ARGUMENT arrives as std::invalid_argument
    try { call(); } catch (const std::invalid_argument&) { return true; }
    return false;
}

static void Uninitialised() {
    const Map map;
    CHECK(!map.IsInitialized());
    CHECK(Throws([&] { map.ExtractFrontierCells(); }));
    CHECK(Throws([&] { map.ExtractFrontierCells(Index(0, 0, 0), 2, 2, 2, true); }));
    CHECK(Throws([&] { map.ExtractFrontierWindowBits(Index(0, 0, 0), 2, 2, 2); }));
    CHECK(Throws([&] { map.ExtractFrontierClusters(Index(0, 0, 0), 2, 2, 2); }));
}

static bool Is(const Index& i, int64_t x, int64_t y, int64_t z) { return i.x == x && i.y == y && i.z == z; }

static void OnTheGpu() {
    // Unit cells, chunks of 4^3, everything unknown but two free rows along x in chunk (0, 0, 0): cells (0 .. 3, 1, 1) and, touching
    // the first only across an edge, (0 .. 1, 2, 2).
    Map writable("map_frame", 1.0, 4, 4, 4, COLLISION_CELL(0.5f, 7u));
    for (int x = 0; x < 4; ++x) CHECK(writable.SetCell(x + 0.5, 1.5, 1.5, COLLISION_CELL(0.0f)) == VoxelGrid::SET_CELL);
    for (int x = 0; x < 2; ++x) CHECK(writable.SetCell(x + 0.5, 2.5, 2.5, COLLISION_CELL(0.0f)) == VoxelGrid::SET_CELL);
    const Map& map = writable;
    const sdfgpu_dsh_counts before = map.GetCounts();
    const std::vector<Index> cells = map.ExtractFrontierCells();
    CHECK(cells.size() == 6 && Is(cells[0], 0, 1, 1) && Is(cells[1], 0, 2, 2) && Is(cells[2], 1, 1, 1) && Is(cells[5], 3, 1, 1));    // cell slot order: x slowest
    CHECK(map.ExtractFrontierCells(true).size() == 6);
    const std::vector<Index> boxed = map.ExtractFrontierCells(Index(1, 0, 0), 2, 2, 4);
    CHECK(boxed.size() == 2 && Is(boxed[0], 1, 1, 1) && Is(boxed[1], 2, 1, 1));
    const std::vector<uint32_t> bits = map.ExtractFrontierWindowBits(Index(0, 0, 0), 4, 4, 4);
    CHECK(bits.size() == 2 && bits[0] == ((1u << 5) | (1u << 10) | (1u << 21) | (1u << 26)) && bits[1] == ((1u << 5) | (1u << 21)));
    // two 6-connected pieces, whichever rule found the cells; the window's lower corner moves the coordinates, not the clusters
    for (const bool use_26 : {true, false}) {
        const std::vector<Map::FrontierCluster> clusters = map.ExtractFrontierClusters(Index(-1, -1, -1), 6, 5, 5, 1, use_26);
        CHECK(clusters.size() == 2);
        if (clusters.size() != 2) continue;
        CHECK(clusters[0].cells == 4 && Is(clusters[0].lower, 0, 1, 1) && Is(clusters[0].upper, 3, 1, 1) && clusters[0].label < clusters[1].label);
        CHECK(clusters[1].cells == 2 && Is(clusters[1].lower, 0, 2, 2) && Is(clusters[1].upper, 1, 2, 2));
        CHECK(clusters[0].centroid.x() == 2.0 && clusters[0].centroid.y() == 1.5 && clusters[0].centroid.z() == 1.5);
        CHECK(clusters[1].centroid.x() == 1.0 && clusters[1].centroid.y() == 2.5 && clusters[1].centroid.z() == 2.5);
    }
    const std::vector<Map::FrontierCluster> big = map.ExtractFrontierClusters(Index(-1, -1, -1), 6, 5, 5, 3);
    CHECK(big.size() == 1 && big[0].cells == 4);
    CHECK(map.ExtractFrontierClusters(Index(10, 10, 10), 3, 3, 3).empty());
    const sdfgpu_dsh_counts after = map.GetCounts();
    CHECK(before.chunk_filled == after.chunk_filled && before.cell_filled == after.cell_filled && before.bytes_held == after.bytes_held);
    CHECK(Refuses([&] { map.ExtractFrontierCells(Index(0, 0, 0), 1, 0, 1); }));
    CHECK(Refuses([&] { map.ExtractFrontierWindowBits(Index(0, 0, 0), 1, -1, 1); }));
    CHECK(Refuses([&] { map.ExtractFrontierWindowBits(Index(0, 0, 0), (int64_t)1 << 16, (int64_t)1 << 16, 1); }));
    CHECK(Refuses([&] { map.ExtractFrontierClusters(Index(0, 0, 0), 0, 1, 1); }));
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
    std::printf("dsh frontier class OK\n");
    return 0;
}
