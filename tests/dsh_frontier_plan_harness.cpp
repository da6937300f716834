// dsh_frontier_plan_harness.cpp -- the host arithmetic of the frontier calls (sdf_tools_amd/csrc/sdfgpu_dsh.hpp, DESIGN.md section
// 34) on the CPU, meant for -fsanitize=address,undefined: the box of a list (dsh_frontier_box_ok, dsh_frontier_box) at and beyond the
// ends of int64 and of the chunk range, against the cells counted one by one; the steps of the stencil (dsh_axis_steps) against
// every neighbour of every cell of small chunks; the mask's word count.  Prints "dsh frontier plan OK" and returns 0, or says what
// failed and returns 1.  tests/test_dsh_frontier_cpu.py builds and runs it.
#include <cstdio>
#include <set>
#include <tuple>

#include "../sdf_tools_amd/csrc/sdfgpu_dsh.hpp"

using namespace sdfgpu;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static void Boxes() {
    const int64_t n[3] = {3, 2, 5};
    const int64_t most = INT64_MAX, least = INT64_MIN;
    // what is refused: an extent below 1, an upper corner beyond int64
    const int64_t zero[3] = {0, 0, 0}, one[3] = {1, 1, 1};
    CHECK(dsh_frontier_box_ok(zero, one));
    for (int a = 0; a < 3; ++a) {
        int64_t lower[3] = {0, 0, 0}, extent[3] = {1, 1, 1};
        extent[a] = 0;
        CHECK(!dsh_frontier_box_ok(lower, extent));
        extent[a] = -1;
        CHECK(!dsh_frontier_box_ok(lower, extent));
        extent[a] = most;                                  // 0 .. INT64_MAX - 1
        CHECK(dsh_frontier_box_ok(lower, extent));
        lower[a] = 1;                                      // 1 .. INT64_MAX
        CHECK(dsh_frontier_box_ok(lower, extent));
        lower[a] = 2;
        CHECK(!dsh_frontier_box_ok(lower, extent));
        lower[a] = least; extent[a] = most;                // INT64_MIN .. -2
        CHECK(dsh_frontier_box_ok(lower, extent));
        lower[a] = most; extent[a] = 1;
        CHECK(dsh_frontier_box_ok(lower, extent));
        extent[a] = 2;
        CHECK(!dsh_frontier_box_ok(lower, extent));
    }
    // the whole map: every cell a chunk can hold
    const DshFrontierBox whole = dsh_frontier_box(nullptr, nullptr, n);
    CHECK(!whole.chunks.empty);
    for (int a = 0; a < 3; ++a) {
        CHECK(whole.lo[a] == -kDshChunkBias * n[a] && whole.hi[a] == kDshChunkBias * n[a] - 1);
        CHECK(whole.chunks.lo[a] == -kDshChunkBias && whole.chunks.hi[a] == kDshChunkBias - 1);
    }
    // boxes at the extremes are clamped, not overflowed
    {
        const int64_t lower[3] = {least, least, least}, extent[3] = {most, most, most};
        const DshFrontierBox b = dsh_frontier_box(lower, extent, n);
        CHECK(!b.chunks.empty && b.lo[0] == -kDshChunkBias * 3 && b.hi[0] == -2 && b.chunks.hi[0] == -1 && b.chunks.hi[1] == -1 && b.chunks.hi[2] == -1);
        const int64_t far[3] = {most, 0, 0};
        const DshFrontierBox c = dsh_frontier_box(far, one, n);
        CHECK(c.chunks.empty);
        const int64_t below[3] = {least, 0, 0};
        CHECK(dsh_frontier_box(below, one, n).chunks.empty);
    }
    // small boxes around zero and around both ends of the chunk range: the chunk range holds exactly the chunks of the box's cells
    const int64_t ends[3] = {0, -kDshChunkBias, kDshChunkBias - 1};
    for (int e = 0; e < 3; ++e)
        for (int64_t off = -7; off <= 7; ++off)
            for (int64_t len = 1; len <= 9; ++len)
                for (int a = 0; a < 3; ++a) {
                    int64_t lower[3] = {0, 0, 0}, extent[3] = {1, 1, 1};
                    lower[a] = ends[e] * n[a] + off;
                    extent[a] = len;
                    const DshFrontierBox b = dsh_frontier_box(lower, extent, n);
                    int64_t lo = INT64_MAX, hi = INT64_MIN, clo = INT64_MAX, chi = INT64_MIN;
                    for (int64_t i = lower[a]; i < lower[a] + len; ++i) {
                        const int64_t c = dsh_floor_div(i, n[a]);
                        if (!dsh_chunk_in_range(c)) continue;
                        lo = i < lo ? i : lo; hi = i > hi ? i : hi; clo = c < clo ? c : clo; chi = c > chi ? c : chi;
                    }
                    if (lo > hi) { CHECK(b.chunks.empty); continue; }
                    CHECK(!b.chunks.empty && b.lo[a] == lo && b.hi[a] == hi && b.chunks.lo[a] == clo && b.chunks.hi[a] == chi);
                    CHECK(dsh_key_in_range(dsh_pack_key(a == 0 ? clo : 0, a == 1 ? clo : 0, a == 2 ? clo : 0), b.chunks));
                }
}

// every (chunk offset, step) pair the three axis ranges produce, against the neighbours of the cell counted one by one
static void Steps() {
    const int64_t shapes[][3] = {{1, 1, 1}, {3, 2, 5}, {4, 4, 4}, {2, 1, 3}};
    for (const auto& n : shapes)
        for (int64_t lx = 0; lx < n[0]; ++lx)
            for (int64_t ly = 0; ly < n[1]; ++ly)
                for (int64_t lz = 0; lz < n[2]; ++lz) {
                    const int64_t l[3] = {lx, ly, lz};
                    std::set<std::tuple<int, int, int>> seen;
                    for (int ox = -1; ox <= 1; ++ox)
                        for (int oy = -1; oy <= 1; ++oy)
                            for (int oz = -1; oz <= 1; ++oz) {
                                const int o[3] = {ox, oy, oz};
                                int lo[3], hi[3];
                                for (int a = 0; a < 3; ++a) dsh_axis_steps(l[a], n[a], o[a], lo[a], hi[a]);
                                for (int dx = lo[0]; dx <= hi[0]; ++dx)
                                    for (int dy = lo[1]; dy <= hi[1]; ++dy)
                                        for (int dz = lo[2]; dz <= hi[2]; ++dz) {
                                            const int d[3] = {dx, dy, dz};
                                            for (int a = 0; a < 3; ++a) {
                                                CHECK(d[a] >= -1 && d[a] <= 1 && dsh_floor_div(l[a] + d[a], n[a]) == o[a]);    // the step leads into that chunk
                                                const int64_t m = l[a] + d[a] - o[a] * n[a];
                                                CHECK(m >= 0 && m < n[a]);                                                       // ... and to a cell of it
                                            }
                                            CHECK(seen.insert(std::make_tuple(dx, dy, dz)).second);                            // once
                                        }
                            }
                    CHECK(seen.size() == 27);                                                                                   // every step, the cell itself included
                }
}

int main() {
    Boxes();
    Steps();
    CHECK(dsh_frontier_mask_words(1) == 1 && dsh_frontier_mask_words(64) == 1 && dsh_frontier_mask_words(65) == 2 && dsh_frontier_mask_words(32768) == 512);
    CHECK(kDshFrontier26 == 1);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("dsh frontier plan OK\n");
    return 0;
}
