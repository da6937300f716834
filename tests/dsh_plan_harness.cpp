// dsh_plan_harness.cpp -- the host-side arithmetic of the dynamic spatial hashed map (sdf_tools_amd/csrc/sdfgpu_dsh.hpp) driven on the
// CPU: key packing, floor division, table sizing, pool growth with 64-bit sizes, and a model of the open-addressing table (insert,
// rehash into a grown table, roll-back of a refused batch) in host memory.  tests/test_dsh_cpu.py builds it with
// -fsanitize=address,undefined and runs it; it prints "dsh plan OK" and returns 0, or says what failed and returns 1.
#include "../sdf_tools_amd/csrc/sdfgpu_dsh.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

using namespace sdfgpu;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// the table of the kernels, in host memory: the same hash, the same bounded linear probe
struct Table {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> slots;
    uint64_t mask;
    explicit Table(uint64_t cap) : keys(cap, kDshEmptyKey), slots(cap, 0), mask(cap - 1) {}
    // the position of key, inserted with `slot` when absent (*fresh says which); -1 when the probe found no room
    int64_t insert(uint64_t key, uint32_t slot, bool* fresh) {
        uint64_t pos = dsh_hash(key) & mask;
        for (uint64_t probe = 0; probe <= mask; ++probe) {
            if (keys[pos] == kDshEmptyKey) { keys[pos] = key; slots[pos] = slot; *fresh = true; return (int64_t)pos; }
            if (keys[pos] == key) { *fresh = false; return (int64_t)pos; }
            pos = (pos + 1) & mask;
        }
        return -1;
    }
    int64_t find(uint64_t key) const {
        uint64_t pos = dsh_hash(key) & mask;
        for (uint64_t probe = 0; probe <= mask; ++probe) {
            if (keys[pos] == key) return (int64_t)pos;
            if (keys[pos] == kDshEmptyKey) return -1;
            pos = (pos + 1) & mask;
        }
        return -1;
    }
};

static void test_keys() {
    const int64_t lo = -kDshChunkBias, hi = kDshChunkBias - 1;
    const int64_t edge[] = {lo, lo + 1, -1, 0, 1, hi - 1, hi};
    std::vector<uint64_t> seen;
    for (int64_t x : edge) for (int64_t y : edge) for (int64_t z : edge) {
        const uint64_t k = dsh_pack_key(x, y, z);
        CHECK(k != kDshEmptyKey && (k >> 63) == 0);
        int64_t bx, by, bz;
        dsh_unpack_key(k, bx, by, bz);
        CHECK(bx == x && by == y && bz == z);
        seen.push_back(k);
    }
    CHECK(std::is_sorted(seen.begin(), seen.end()));                   // keys ascend as (x, y, z) ascends lexicographically
    CHECK(std::set<uint64_t>(seen.begin(), seen.end()).size() == seen.size());
    CHECK(dsh_pack_key(hi, hi, hi) == (kDshEmptyKey >> 1));            // 63 ones: the largest key, one bit short of the empty word
    CHECK(!dsh_chunk_in_range(lo - 1) && dsh_chunk_in_range(lo) && dsh_chunk_in_range(hi) && !dsh_chunk_in_range(hi + 1));
}

static void test_floor_div() {
    for (int64_t n : {1, 2, 3, 5, 16, 32768})
        for (int64_t i = -3 * n - 2; i <= 3 * n + 2; ++i) {
            const int64_t q = dsh_floor_div(i, n), r = i - q * n;
            CHECK(r >= 0 && r < n);
        }
    CHECK(dsh_floor_div(-1, 16) == -1 && dsh_floor_div(-16, 16) == -1 && dsh_floor_div(-17, 16) == -2 && dsh_floor_div(15, 16) == 0);
    // the ends of the valid global cell range with the largest chunk axis
    CHECK(dsh_floor_div(-kDshChunkBias * 32768, 32768) == -kDshChunkBias && dsh_floor_div(kDshChunkBias * 32768 - 1, 32768) == kDshChunkBias - 1);
}

static void test_sizes() {
    CHECK(dsh_table_capacity(0) == kDshMinTable && dsh_table_capacity(8) == 16 && dsh_table_capacity(9) == 32);
    for (uint64_t chunks : {1ull, 7ull, 5000ull, 65537ull, (1ull << 30)}) {
        const uint64_t cap = dsh_table_capacity(chunks);
        CHECK((cap & (cap - 1)) == 0 && cap >= 2 * chunks && (cap == kDshMinTable || cap < 4 * chunks));
    }
    // 65537 chunks of 32^3 cells: the cell index passes 2^31 and the byte offset 2^34
    const uint64_t cpc = 32768, chunks = 65537;
    CHECK(chunks * cpc > (1ull << 31) && dsh_pool_bytes(chunks, cpc) > (1ull << 34));
    CHECK(dsh_pool_bytes(chunks, cpc) == chunks * 24 + chunks * cpc * 8);
    CHECK(dsh_table_bytes(1ull << 31) == 12ull << 31);
    uint64_t cap = 0;
    CHECK(dsh_plan_pool(64, 10, 4096, 0, 0, &cap) && cap == 64);                          // room: unchanged
    CHECK(dsh_plan_pool(64, 65, 4096, 0, 0, &cap) && cap == 128);                         // doubling
    CHECK(dsh_plan_pool(1, 5000, 64, 0, 0, &cap) && cap == 5000);                         // at least what is needed
    const uint64_t table = dsh_table_bytes(256);
    const uint64_t limit = table + dsh_pool_bytes(100, 4096);
    CHECK(dsh_plan_pool(64, 65, 4096, table, limit, &cap) && cap == 65);                  // the doubling would pass the limit: exactly 65
    CHECK(dsh_plan_pool(64, 100, 4096, table, limit, &cap) && cap == 100);
    CHECK(!dsh_plan_pool(64, 101, 4096, table, limit, &cap) && cap == 64);                // refused: the capacity stays
    CHECK(dsh_plan_pool(1ull << 20, (1ull << 20) + 1, cpc, 0, 0, &cap) && cap == (1ull << 21) && dsh_pool_bytes(cap, cpc) > (1ull << 39));
}

static void test_table_model() {
    std::mt19937_64 rng(7);
    // lines through negative coordinates and a block: the keys differ in few bits, the probe chains must stay short of the capacity
    std::vector<uint64_t> keys;
    for (int64_t i = -1500; i < 1500; ++i) { keys.push_back(dsh_pack_key(i, 0, 0)); keys.push_back(dsh_pack_key(0, i, -1)); keys.push_back(dsh_pack_key(-1, -1, i)); }
    for (int64_t x = 0; x < 12; ++x) for (int64_t y = 0; y < 12; ++y) for (int64_t z = 0; z < 12; ++z) keys.push_back(dsh_pack_key(x - 6, y + 100, z - 1000));
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::shuffle(keys.begin(), keys.end(), rng);
    Table small(dsh_table_capacity(keys.size() / 2));
    std::vector<uint64_t> by_slot;
    for (size_t k = 0; k < keys.size() / 2; ++k) {
        bool fresh = false;
        CHECK(small.insert(keys[k], (uint32_t)by_slot.size(), &fresh) >= 0 && fresh);
        by_slot.push_back(keys[k]);
        CHECK(small.insert(keys[k], 0xFFFFFFFFu, &fresh) >= 0 && !fresh);                 // a second insert finds the first
    }
    // a refused batch: its entries become empty again and the table is the one it found
    const Table before = small;
    std::vector<int64_t> made;
    for (size_t k = keys.size() / 2; k < keys.size() / 2 + small.keys.size() / 8; ++k) {
        bool fresh = false;
        const int64_t pos = small.insert(keys[k], 0, &fresh);
        CHECK(pos >= 0 && fresh);
        made.push_back(pos);
    }
    for (int64_t pos : made) { small.keys[(size_t)pos] = kDshEmptyKey; small.slots[(size_t)pos] = before.slots[(size_t)pos]; }
    CHECK(small.keys == before.keys && small.slots == before.slots);
    // growth: rehash by slot into the table for all keys, then the rest
    Table grown(dsh_table_capacity(keys.size()));
    for (size_t s = 0; s < by_slot.size(); ++s) { bool fresh = false; CHECK(grown.insert(by_slot[s], (uint32_t)s, &fresh) >= 0 && fresh); }
    for (size_t k = keys.size() / 2; k < keys.size(); ++k) {
        bool fresh = false;
        CHECK(grown.insert(keys[k], (uint32_t)by_slot.size(), &fresh) >= 0 && fresh);
        by_slot.push_back(keys[k]);
    }
    for (size_t s = 0; s < by_slot.size(); ++s) {
        const int64_t pos = grown.find(by_slot[s]);
        CHECK(pos >= 0 && grown.slots[(size_t)pos] == s);
    }
    CHECK(grown.find(dsh_pack_key(5000, 5000, 5000)) == -1);
    // a full table ends its probe: capacity steps, no more
    Table full(kDshMinTable);
    for (uint64_t k = 0; k < kDshMinTable; ++k) { bool fresh = false; CHECK(full.insert(dsh_pack_key((int64_t)k, 1, 2), 0, &fresh) >= 0); }
    bool fresh = false;
    CHECK(full.insert(dsh_pack_key(-7, -7, -7), 0, &fresh) == -1 && full.find(dsh_pack_key(-7, -7, -7)) == -1);
}

int main() {
    test_keys();
    test_floor_div();
    test_sizes();
    test_table_model();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("dsh plan OK\n");
    return 0;
}
