// dsh_remove_plan_harness.cpp -- the host-side arithmetic of removal from the dynamic spatial hashed map (sdf_tools_amd/csrc/
// sdfgpu_dsh.hpp) driven on the CPU: a box of cells as a range of chunk coordinates against a brute-force loop
// over chunks, the hole-filling pairing (the plain statement dsh_pair_model, and the kernels' two-level scan over tiles restated in
// host memory) over every flag pattern of length <= 12 and random ones up to 70 000, and the sizes that shrink plans.
// tests/test_dsh_remove_cpu.py builds it with -fsanitize=address,undefined and runs it; it prints "dsh remove plan OK" and returns
// 0, or says what failed and returns 1.
#include "../sdf_tools_amd/csrc/sdfgpu_dsh.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace sdfgpu;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// ---- the box ---------------------------------------------------------------------------------------------------------------------------
// whether chunk c holds a cell of the box along one axis, by its cell range (128-bit: no assumption about the sizes)
static bool axis_overlap(int64_t c, int64_t n, int64_t lower, int64_t extent) {
    const __int128 first = (__int128)c * n, last = first + n - 1, box_first = lower, box_last = (__int128)lower + extent - 1;
    return box_last >= box_first && last >= box_first && first <= box_last;
}

static void check_box(const int64_t lower[3], const int64_t extent[3], const int64_t n[3], const std::vector<int64_t>& probes) {
    CHECK(dsh_box_ok(lower, extent));
    const DshChunkRange r = dsh_box_chunk_range(lower, extent, n);
    for (int a = 0; a < 3; ++a)
        if (!r.empty) CHECK(r.lo[a] >= -kDshChunkBias && r.hi[a] < kDshChunkBias && r.lo[a] <= r.hi[a]);
    for (int64_t cx : probes)
        for (int64_t cy : probes)
            for (int64_t cz : probes) {
                const bool want = axis_overlap(cx, n[0], lower[0], extent[0]) && axis_overlap(cy, n[1], lower[1], extent[1]) &&
                                  axis_overlap(cz, n[2], lower[2], extent[2]);
                CHECK(dsh_key_in_range(dsh_pack_key(cx, cy, cz), r) == want);
            }
}

static void test_box() {
    const int64_t lo = -kDshChunkBias, hi = kDshChunkBias - 1, big = kDshMaxBoxCell;
    {   // a small box around the origin, every chunk near it by brute force
        const int64_t n[3] = {3, 2, 5};
        std::vector<int64_t> near;
        for (int64_t c = -6; c <= 6; ++c) near.push_back(c);
        for (int64_t l = -7; l <= 7; l += 1)
            for (int64_t e = 0; e <= 7; ++e) {
                const int64_t lower[3] = {l, -l, l + 1}, extent[3] = {e, 7 - e + 1, e + 1};
                check_box(lower, extent, n, near);
            }
    }
    {   // the faces one cell to each side of a chunk boundary
        const int64_t n[3] = {4, 4, 4};
        const std::vector<int64_t> near = {-3, -2, -1, 0, 1, 2, 3};
        for (int64_t d = -1; d <= 1; ++d)
            for (int64_t e = 3; e <= 5; ++e) {
                const int64_t lower[3] = {-4 + d, 0 + d, 4 + d}, extent[3] = {e, e + 4, e};
                check_box(lower, extent, n, near);
            }
    }
    {   // the clamps at +-2^20 and the box bounds at +-2^40
        const int64_t dims[4][3] = {{1, 1, 1}, {3, 2, 5}, {16, 16, 16}, {32768, 1, 1}};
        const std::vector<int64_t> edge = {lo, lo + 1, -1, 0, 1, hi - 1, hi};
        for (const auto& n : dims) {
            const int64_t lowers[] = {-big, -big + 1, lo * n[0], lo * n[0] - 1, lo * n[0] + 1, -1, 0, hi * n[0], hi * n[0] + n[0] - 1, hi * n[0] + n[0], big - 1, big};
            const int64_t extents[] = {0, 1, 2, n[0], big - 1, big};
            for (int64_t l : lowers)
                for (int64_t e : extents) {
                    if (l < -big || l > big) continue;
                    const int64_t lower[3] = {l, -big, l}, extent[3] = {e, big, e == 0 ? 1 : e};
                    check_box(lower, extent, n, edge);
                }
        }
        const int64_t n[3] = {1, 1, 1};
        const int64_t all_lower[3] = {-big, -big, -big}, all_extent[3] = {big, big, big};
        const DshChunkRange r = dsh_box_chunk_range(all_lower, all_extent, n);
        CHECK(!r.empty && r.lo[0] == lo && r.hi[0] == -1);
        const int64_t beyond[3] = {hi + 1, 0, 0}, one[3] = {1, 1, 1};
        CHECK(dsh_box_chunk_range(beyond, one, n).empty);                      // a box beyond the key range holds no chunk
        const int64_t below[3] = {lo - 5, 0, 0}, four[3] = {4, 1, 1};
        CHECK(dsh_box_chunk_range(below, four, n).empty);
    }
    {   // refusals
        const int64_t ok[3] = {0, 0, 0};
        for (int a = 0; a < 3; ++a) {
            int64_t lower[3] = {0, 0, 0}, extent[3] = {1, 1, 1};
            lower[a] = big + 1; CHECK(!dsh_box_ok(lower, extent));
            lower[a] = -big - 1; CHECK(!dsh_box_ok(lower, extent));
            lower[a] = INT64_MIN; CHECK(!dsh_box_ok(lower, extent));
            lower[a] = big; CHECK(dsh_box_ok(lower, extent));
            lower[a] = -big; CHECK(dsh_box_ok(lower, extent));
            extent[a] = -1; CHECK(!dsh_box_ok(ok, extent));
            extent[a] = big + 1; CHECK(!dsh_box_ok(ok, extent));
            extent[a] = INT64_MAX; CHECK(!dsh_box_ok(ok, extent));
            extent[a] = big; CHECK(dsh_box_ok(ok, extent));
            extent[a] = 0; CHECK(dsh_box_ok(ok, extent));
        }
    }
}

// ---- the pairing -----------------------------------------------------------------------------------------------------------------------
// The kernels' scan in host memory: k_dsh_pair_count (a count per tile), k_dsh_pair_scan (exclusive prefixes over the tiles, each
// of 256 "threads" taking a run of consecutive tiles), k_dsh_pair_list (each thread's kDshPairItems slots behind its rank).
static uint64_t tiled_pairing(const std::vector<uint8_t>& flagged, uint64_t keep, std::vector<uint32_t>& holes, std::vector<uint32_t>& movers) {
    const uint64_t n = flagged.size(), tiles = dsh_pair_tiles(n);
    std::vector<uint32_t> counts(2 * tiles + 2, 0);
    for (uint64_t s = 0; s < n; ++s) {
        counts[2 * (s / kDshPairTile)] += s < keep && flagged[s];
        counts[2 * (s / kDshPairTile) + 1] += s >= keep && !flagged[s];
    }
    const uint64_t per = (tiles + 255) / 256;
    uint32_t run_holes = 0, run_movers = 0;
    for (uint64_t t = 0; t < 256; ++t)
        for (uint64_t k = std::min(t * per, tiles); k < std::min(std::min(t * per, tiles) + per, tiles); ++k) {
            const uint32_t h = counts[2 * k], m = counts[2 * k + 1];
            counts[2 * k] = run_holes; counts[2 * k + 1] = run_movers;
            run_holes += h; run_movers += m;
        }
    if (run_holes != run_movers) return ~(uint64_t)0;
    for (uint64_t tile = 0; tile < tiles; ++tile) {
        uint32_t hole = counts[2 * tile], mover = counts[2 * tile + 1];
        for (uint64_t thread = 0; thread < 256; ++thread)
            for (uint64_t k = 0; k < kDshPairItems; ++k) {
                const uint64_t s = tile * kDshPairTile + thread * kDshPairItems + k;
                if (s >= n) break;
                if (s < keep && flagged[s]) holes.at(hole++) = (uint32_t)s;
                if (s >= keep && !flagged[s]) movers.at(mover++) = (uint32_t)s;
            }
    }
    return run_holes;
}

static void check_pairing(const std::vector<uint8_t>& flagged) {
    const uint64_t n = flagged.size();
    uint64_t removed = 0;
    for (uint8_t f : flagged) removed += f != 0;
    const uint64_t keep = n - removed, room = std::min(keep, removed);
    std::vector<uint32_t> holes(room + 1, 0xFFFFFFFFu), movers(room + 1, 0xFFFFFFFFu), holes2(room + 1, 0xFFFFFFFFu), movers2(room + 1, 0xFFFFFFFFu);
    const uint64_t pairs = dsh_pair_model(flagged.data(), n, keep, holes.data(), movers.data());
    CHECK(pairs != ~(uint64_t)0 && pairs <= room);                              // as many holes as movers
    if (pairs == ~(uint64_t)0) return;
    CHECK(tiled_pairing(flagged, keep, holes2, movers2) == pairs && holes2 == holes && movers2 == movers);
    std::vector<uint32_t> owner(n);                                             // which survivor a slot holds once the moves have run
    for (uint64_t s = 0; s < n; ++s) owner[s] = flagged[s] ? 0xFFFFFFFFu : (uint32_t)s;
    for (uint64_t j = 0; j < pairs; ++j) {
        CHECK(holes[j] < keep && flagged[holes[j]] && movers[j] >= keep && movers[j] < n && !flagged[movers[j]]);   // disjoint: below / at or above keep
        if (j) CHECK(holes[j] > holes[j - 1] && movers[j] > movers[j - 1]);      // ascending: the j-th takes the j-th
        owner[holes[j]] = movers[j];
        owner[movers[j]] = 0xFFFFFFFFu;
    }
    std::vector<uint8_t> seen(n, 0);
    for (uint64_t s = 0; s < n; ++s) {
        if (s < keep) {
            CHECK(owner[s] != 0xFFFFFFFFu && !flagged[owner[s]] && !seen[owner[s]]);
            if (owner[s] != 0xFFFFFFFFu) seen[owner[s]] = 1;
        } else {
            CHECK(owner[s] == 0xFFFFFFFFu);
        }
    }
    uint64_t survivors = 0;
    for (uint8_t v : seen) survivors += v;
    CHECK(survivors == keep);                                                   // every survivor ends below keep exactly once
}

static void test_pairing() {
    for (uint32_t n = 0; n <= 12; ++n)
        for (uint32_t bits = 0; bits < (1u << n); ++bits) {
            std::vector<uint8_t> flagged(n);
            for (uint32_t s = 0; s < n; ++s) flagged[s] = (bits >> s) & 1;
            check_pairing(flagged);
        }
    std::mt19937_64 rng(32);
    const uint64_t sizes[] = {13, 255, 256, 257, 513, 4095, 4096, 4097, 8000, 8192, 12289, 65537, 70000};
    const double shares[] = {0.0, 0.01, 0.5, 0.99, 1.0};
    for (uint64_t n : sizes)
        for (double share : shares) {
            std::vector<uint8_t> flagged(n);
            for (auto& f : flagged) f = std::uniform_real_distribution<double>(0, 1)(rng) < share;
            check_pairing(flagged);
        }
    for (uint64_t n : sizes) {                                                  // head only, tail only, alternating
        std::vector<uint8_t> head(n, 0), tail(n, 0), alt(n, 0);
        for (uint64_t s = 0; s < n; ++s) { head[s] = s < n / 2; tail[s] = s >= n / 2; alt[s] = s & 1; }
        check_pairing(head); check_pairing(tail); check_pairing(alt);
    }
}

// ---- shrink -----------------------------------------------------------------------------------------------------------------------------
static void test_shrink() {
    uint64_t pool = 0, table = 0;
    dsh_plan_shrink(100, 0, 8192, 16384, &pool, &table);
    CHECK(pool == 100 && table == 256);
    dsh_plan_shrink(100, 10, 8192, 16384, &pool, &table);
    CHECK(pool == 110 && table == 256);
    dsh_plan_shrink(100, 28, 8192, 16384, &pool, &table);
    CHECK(pool == 128 && table == 256);
    dsh_plan_shrink(100, 29, 8192, 16384, &pool, &table);
    CHECK(pool == 129 && table == 512);
    dsh_plan_shrink(0, 0, 64, 128, &pool, &table);
    CHECK(pool == 1 && table == kDshMinTable);
    dsh_plan_shrink(0, 0, 1, 16, &pool, &table);
    CHECK(pool == 1 && table == 16);
    dsh_plan_shrink(100, 0, 100, 256, &pool, &table);                           // already tight: nothing changes
    CHECK(pool == 100 && table == 256);
    dsh_plan_shrink(100, 1000, 200, 256, &pool, &table);                        // an allocation is replaced only where the new size is smaller
    CHECK(pool == 200 && table == 256);
    dsh_plan_shrink(100, 0, 50000, 256, &pool, &table);
    CHECK(pool == 100 && table == 256);
    dsh_plan_shrink((uint64_t)1 << 30, (uint64_t)INT64_MAX, (uint64_t)1 << 30, (uint64_t)1 << 31, &pool, &table);   // no sum overflows
    CHECK(pool == (uint64_t)1 << 30 && table == (uint64_t)1 << 31);
    for (uint64_t live = 0; live < 300; ++live)
        for (uint64_t spare = 0; spare < 40; spare += 3) {
            dsh_plan_shrink(live, spare, 1000, 4096, &pool, &table);
            CHECK(pool == std::max<uint64_t>(live + spare, 1) && table == dsh_table_capacity(live + spare) && table >= 2 * (live + spare) && pool >= live);
        }
}

int main() {
    test_box();
    test_pairing();
    test_shrink();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("dsh remove plan OK\n");
    return 0;
}
