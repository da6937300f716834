// dsh_rays_plan_harness.cpp -- the host-side sizing arithmetic of a frame of sensor rays (sdf_tools_amd/csrc/sdfgpu_dsh.hpp:
// dsh_ray_axis_steps, dsh_ray_max_steps, dsh_ray_chunks, dsh_ray_chunk_bound) driven on the CPU: the saturation of the 64-bit bound at
// its ends, and a model of the walk (in doubles as the kernels state it) whose steps and distinct chunks must stay inside the
// bounds for frames at many ranges, chunk shapes and sensor positions.  tests/test_dsh_rays_cpu.py builds it with
// -fsanitize=address,undefined and runs it; it prints "dsh rays plan OK" and returns 0, or says what failed and returns 1.
#include "../sdf_tools_amd/csrc/sdfgpu_dsh.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <set>

using namespace sdfgpu;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static void test_bound_arithmetic() {
    const int64_t one[3] = {1, 1, 1}, big[3] = {32768, 1, 1}, cube[3] = {16, 16, 16};
    CHECK(dsh_ray_axis_steps(65536) == 65538 && dsh_ray_max_steps(65536) == 3 * 65538 + 2);
    // one ray of one cell in chunks of one cell: 1 + 3 * (3 + 1) chunks by the ray count, 8^3 by the box
    CHECK(dsh_ray_chunk_bound(1, 1, one) == 13);
    CHECK(dsh_ray_chunk_bound(1000, 1, one) == 512);
    CHECK(dsh_ray_chunk_bound(0, 65536, one) == 0);
    // the largest range in the smallest chunks: the box is (2 * 65538 + 2)^3 < 2^52, the ray count takes over below it
    const uint64_t across = 2 * 65538 + 2, box = across * across * across;
    CHECK(box < (1ull << 52));
    CHECK(dsh_ray_chunk_bound(~0ull, 65536, one) == box);                                   // (the product by rays saturates, the box wins)
    CHECK(dsh_ray_chunk_bound((1ull << 31) - 1, 65536, one) == ((1ull << 31) - 1) * (1 + 3 * 65539ull));
    CHECK(dsh_ray_chunk_bound(1ull << 40, 65536, one) == box);
    CHECK(dsh_ray_chunk_bound(1000, 65536, one) == 1000ull * (1 + 3 * 65539ull));
    // 200 000 rays of 256 cells in 16^3 chunks: the box of (516 / 16 + 2)^3 chunks
    CHECK(dsh_ray_chunk_bound(200000, 256, cube) == 34ull * 34 * 34);
    CHECK(dsh_ray_chunk_bound(3, 256, cube) == 3 * (1 + 3 * (258 / 16 + 1)));
    CHECK(dsh_ray_chunk_bound(5, 10, big) == 5 * (1 + 1 + 13 + 13));
    for (uint64_t rays : {1ull, 77ull, 1ull << 20, 1ull << 40, ~0ull})
        for (uint64_t r : {1ull, 2ull, 100ull, 65536ull})
            CHECK(dsh_ray_chunk_bound(rays, r, cube) <= kDshRayBoundCap && dsh_ray_chunk_bound(rays, r, one) >= dsh_ray_chunk_bound(rays, r, cube));
}

// the walk of the contract for one ray: the distinct chunks it writes into go to `chunks`; returns the steps it took
static uint64_t model_walk(const double gs[3], const double ge[3], double range, const int64_t n[3], std::set<uint64_t>& chunks, bool& is_long) {
    int64_t cur[3], rem[3];
    int sg[3];
    double d[3], t[3];
    const double inf = std::numeric_limits<double>::infinity();
    for (int a = 0; a < 3; ++a) {
        const int64_t i0 = (int64_t)std::floor(gs[a]), i1 = (int64_t)std::floor(ge[a]);
        cur[a] = i0;
        sg[a] = i1 > i0 ? 1 : i1 < i0 ? -1 : 0;
        rem[a] = i1 > i0 ? i1 - i0 : i0 - i1;
        d[a] = ge[a] - gs[a];
        t[a] = rem[a] ? ((double)(cur[a] + (sg[a] > 0 ? 1 : 0)) - gs[a]) / d[a] : inf;
    }
    const double len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], range2 = range * range;
    is_long = len2 > range2;
    uint64_t steps = 0;
    for (;;) {
        chunks.insert(dsh_pack_key(dsh_floor_div(cur[0], n[0]), dsh_floor_div(cur[1], n[1]), dsh_floor_div(cur[2], n[2])));
        if (!(rem[0] | rem[1] | rem[2])) break;
        int a = 0;
        if (t[1] < t[a]) a = 1;
        if (t[2] < t[a]) a = 2;
        const double tk = t[a];
        cur[a] += sg[a];
        rem[a] -= 1;
        t[a] = rem[a] ? ((double)(cur[a] + (sg[a] > 0 ? 1 : 0)) - gs[a]) / d[a] : inf;
        if (is_long && !((tk * tk) * len2 <= range2)) break;
        ++steps;
    }
    return steps;
}

static void test_walks_stay_inside_the_bounds() {
    std::mt19937_64 rng(30);
    std::uniform_real_distribution<double> unit(-1.0, 1.0);
    const int64_t shapes[][3] = {{1, 1, 1}, {3, 2, 5}, {4, 4, 4}, {8, 8, 32}, {16, 16, 16}};
    const double ranges[] = {0.3, 1.0, 2.5, 7.0, 40.0, 300.0};
    for (const auto& n : shapes)
        for (const double range : ranges) {
            const uint64_t range_cells = (uint64_t)std::ceil(range);
            for (int frame = 0; frame < 3; ++frame) {
                // the sensor on a chunk corner, just below one, and anywhere
                double gs[3];
                for (int a = 0; a < 3; ++a) gs[a] = frame == 0 ? (double)(-2 * n[a]) : frame == 1 ? std::nextafter((double)n[a], 0.0) : 1000.0 * unit(rng);
                const uint64_t rays = range < 100.0 ? 400 : 60;
                std::set<uint64_t> chunks;
                uint64_t entered_by_rays = 0;
                for (uint64_t r = 0; r < rays; ++r) {
                    // ends on and beyond the range sphere, along the axes and the diagonals among them
                    double dir[3] = {unit(rng), unit(rng), unit(rng)};
                    if (r % 7 == 0) dir[r % 3] = 0.0;
                    if (r % 11 == 0) { dir[0] = dir[1] = dir[2] = (r & 1) ? 1.0 : -1.0; }
                    const double norm = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
                    if (norm == 0.0) continue;
                    const double reach = range * (r % 3 == 0 ? 1.0 : r % 3 == 1 ? 0.999 * unit(rng) : 1.0 + 3.0 * std::fabs(unit(rng)));
                    double ge[3];
                    for (int a = 0; a < 3; ++a) ge[a] = gs[a] + dir[a] / norm * reach;
                    std::set<uint64_t> mine;
                    bool is_long = false;
                    const uint64_t steps = model_walk(gs, ge, range, n, mine, is_long);
                    CHECK(steps <= dsh_ray_max_steps(range_cells));
                    CHECK(mine.size() <= dsh_ray_chunk_bound(1, range_cells, n));
                    // the count from the ray's two ends: exact for a ray that is not long, a bound for a long one
                    const int64_t i0[3] = {(int64_t)std::floor(gs[0]), (int64_t)std::floor(gs[1]), (int64_t)std::floor(gs[2])};
                    const int64_t i1[3] = {(int64_t)std::floor(ge[0]), (int64_t)std::floor(ge[1]), (int64_t)std::floor(ge[2])};
                    const uint64_t counted = dsh_ray_chunks(i0, i1, n, is_long, range_cells);
                    CHECK(is_long ? mine.size() <= counted : mine.size() == counted);
                    CHECK(counted <= dsh_ray_chunk_bound(1, range_cells, n));
                    entered_by_rays += mine.size();
                    chunks.insert(mine.begin(), mine.end());
                }
                CHECK(chunks.size() <= dsh_ray_chunk_bound(rays, range_cells, n));
                CHECK(entered_by_rays >= chunks.size());
            }
        }
}

int main() {
    test_bound_arithmetic();
    test_walks_stay_inside_the_bounds();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("dsh rays plan OK\n");
    return 0;
}
