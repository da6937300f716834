// dsh_components_plan_harness.cpp -- the host arithmetic of the sparse map's connected components (sdf_tools_amd/csrc/sdfgpu_dsh.hpp,
// DESIGN.md section 35) on the CPU, meant for -fsanitize=address,undefined: the node bases in 64 bits, the N < 2^32 - 1 refusal at
// its exact edge, the scratch's size, the class of an occupancy, and a host model of the face pairing for the four state pairs
// (dsh_cc_face_pair, dsh_cc_face_pairs, dsh_cc_node) against the neighbours counted cell by cell.  Prints "dsh components plan OK"
// and returns 0, or says what failed and returns 1.  tests/test_dsh_components_cpu.py builds and runs it.
#include <cmath>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../sdf_tools_amd/csrc/sdfgpu_dsh.hpp"

using namespace sdfgpu;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static void NodeBases() {
    // bases are a running sum of the weights in key order, in 64 bits: 131 071 cell-filled chunks of 32^3 and a chunk-filled one
    const uint64_t cpc = 32768;
    CHECK(dsh_cc_weight(kDshCellFilled, cpc) == cpc && dsh_cc_weight(kDshChunkFilled, cpc) == 1);
    CHECK(dsh_cc_weight(kDshCellFilled | kDshTouched, cpc) == cpc);
    uint64_t base = 0;
    for (uint64_t c = 0; c < 131071; ++c) base += dsh_cc_weight(kDshCellFilled, cpc);
    CHECK(base == 131071ull * 32768ull && base > 0xFFFF0000ull);               // past what a 32-bit product of (chunks, cells) keeps
    base += dsh_cc_weight(kDshChunkFilled, cpc);
    CHECK(base == dsh_cc_nodes(131071, 1, cpc));
    CHECK(dsh_cc_nodes((uint64_t)1 << 31, (uint64_t)1 << 31, cpc) == ((uint64_t)1 << 46) + ((uint64_t)1 << 31));
    CHECK(dsh_cc_node(base, true, 7) == base + 7 && dsh_cc_node(base, false, 7) == base);
}

static void SizeEdge() {
    const uint64_t cpc = 32768;
    CHECK(!dsh_cc_nodes_ok(dsh_cc_nodes(131072, 0, cpc)));                     // 2^32: refused
    CHECK(dsh_cc_nodes_ok(dsh_cc_nodes(131071, 0, cpc)));                      // 2^32 - 32768: accepted
    // mixed states: 131 071 cell-filled chunks leave room for 32 766 chunk-filled ones
    CHECK(dsh_cc_nodes(131071, 32766, cpc) == 0xFFFFFFFEull && dsh_cc_nodes_ok(0xFFFFFFFEull));
    CHECK(dsh_cc_nodes(131071, 32767, cpc) == 0xFFFFFFFFull && !dsh_cc_nodes_ok(0xFFFFFFFFull));
    CHECK(!dsh_cc_nodes_ok(dsh_cc_nodes(131071, 32768, cpc)));
    CHECK(dsh_cc_nodes_ok(0) && dsh_cc_nodes_ok(1));
    CHECK(dsh_cc_nodes_ok(dsh_cc_nodes(0, 0xFFFFFFFEull, 1)) && !dsh_cc_nodes_ok(dsh_cc_nodes(0xFFFFFFFFull, 0, 1)));
}

static void Scratch() {
    CHECK(dsh_cc_tiles(1) == 1 && dsh_cc_tiles(8192) == 1 && dsh_cc_tiles(8193) == 2 && dsh_cc_tiles(16400) == 3 && dsh_cc_tiles(32768) == 4);
    // (the functions dsh_components_impl cuts its scratch by; it refuses to run where its cut's total is not dsh_cc_scratch_bytes)
    CHECK(dsh_cc_bases_bytes(3) == 12 && dsh_cc_label_bytes(0xFFFFFFFEull) == 0x3FFFFFFF8ull);
    CHECK(dsh_cc_rank_bytes(0) == 0);
    CHECK(dsh_cc_rank_bytes(1) == (2 * 256 + 2) * 4 && dsh_cc_rank_bytes(8192) == dsh_cc_rank_bytes(1) && dsh_cc_rank_bytes(8193) == 2 * dsh_cc_rank_bytes(1));
    CHECK(dsh_cc_scratch_bytes(1, 1) == 256 + 256 + 2304);                     // 2056 bytes of tables, rounded up
    const uint64_t most = 0xFFFFFFFEull;                                       // the largest N: 16 GiB of labels, 524 288 rank chunks
    CHECK(dsh_cc_rank_bytes(most) == 524288ull * 514 * 4);
    CHECK(dsh_cc_scratch_bytes(131072, most) == 131072ull * 4 + (((most * 4) + 255) & ~255ull) + 524288ull * 514 * 4);
    for (uint64_t n : {1ull, 255ull, 256ull, 8191ull, 8192ull, 8193ull, 1000003ull})
        CHECK(dsh_cc_scratch_bytes(3, n) % 256 == 0 && dsh_cc_scratch_bytes(3, n) >= 12 + 4 * n + dsh_cc_rank_bytes(n));
}

static void Classes() {
    const float below = std::nextafterf(0.5f, 0.0f), above = std::nextafterf(0.5f, 1.0f), nan = std::nanf("");
    for (int apart = 0; apart < 2; ++apart) {
        CHECK(dsh_cc_class(above, apart) == 1 && dsh_cc_class(1.0f, apart) == 1 && dsh_cc_class(INFINITY, apart) == 1);
        CHECK(dsh_cc_class(below, apart) == 0 && dsh_cc_class(0.0f, apart) == 0 && dsh_cc_class(-0.0f, apart) == 0 && dsh_cc_class(-INFINITY, apart) == 0);
        CHECK(dsh_cc_class(0.5f, apart) == (apart ? 2u : 0u) && dsh_cc_class(nan, apart) == (apart ? 2u : 0u));
    }
}

// The links of one face for a state pair, by the model the kernel runs (every candidate pair of the same class that its predecessor
// pair does not cover), closed transitively together with each side's own joins along the face; against the pairs of face
// neighbours of the same class counted cell by cell.  What must agree is which nodes end up joined.
struct Sets {
    std::vector<uint32_t> parent;
    explicit Sets(size_t n) : parent(n) { for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i; }
    uint32_t find(uint32_t a) { while (parent[a] != a) a = parent[a] = parent[parent[a]]; return a; }
    void join(uint32_t a, uint32_t b) { a = find(a); b = find(b); if (a != b) parent[a > b ? a : b] = a > b ? b : a; }
};

static void joins_inside(Sets& s, uint32_t base, const std::vector<uint32_t>& cls, const int64_t n[3]) {
    const uint32_t ny = (uint32_t)n[1], nz = (uint32_t)n[2];
    for (uint32_t k = 0; k < cls.size(); ++k) {
        const uint32_t iz = k % nz, iy = (k / nz) % ny, ix = k / (ny * nz);
        if (iz && cls[k - 1] == cls[k]) s.join(base + k, base + k - 1);
        if (iy && cls[k - nz] == cls[k]) s.join(base + k, base + k - nz);
        if (ix && cls[k - ny * nz] == cls[k]) s.join(base + k, base + k - ny * nz);
    }
}

static void FacePairs() {
    const int64_t shapes[][3] = {{1, 1, 1}, {3, 2, 5}, {4, 4, 4}, {1, 1, 7}, {7, 1, 1}, {2, 5, 3}};
    uint32_t seed = 12345;
    const auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 16; };
    for (const auto& n : shapes) {
        const uint32_t cpc = (uint32_t)(n[0] * n[1] * n[2]);
        for (int axis = 0; axis < 3; ++axis)
            for (int own_cells = 0; own_cells < 2; ++own_cells)
                for (int other_cells = 0; other_cells < 2; ++other_cells)
                    for (int round = 0; round < 8; ++round) {
                        // classes: three values, so that runs of equal class are short and long
                        std::vector<uint32_t> own(own_cells ? cpc : 1), other(other_cells ? cpc : 1);
                        for (uint32_t& c : own) c = next() % 3 % (1 + round % 3);
                        for (uint32_t& c : other) c = next() % 3 % (1 + round % 3);
                        const uint32_t own_base = 0, other_base = (uint32_t)own.size(), nodes = other_base + (uint32_t)other.size();
                        Sets model(nodes), truth(nodes);
                        if (own_cells) { joins_inside(model, own_base, own, n); joins_inside(truth, own_base, own, n); }
                        if (other_cells) { joins_inside(model, other_base, other, n); joins_inside(truth, other_base, other, n); }
                        const uint64_t face = cpc / (uint64_t)n[axis], pairs = dsh_cc_face_pairs(own_cells, other_cells, face);
                        CHECK(pairs == (own_cells || other_cells ? face : 1));
                        uint64_t links = 0;
                        std::set<std::pair<uint32_t, uint32_t>> seen;
                        for (uint32_t idx = 0; idx < pairs; ++idx) {
                            uint32_t k = 0, k2 = 0, back = 0;
                            dsh_cc_face_pair(axis, idx, n, k, k2, back);
                            CHECK(k < cpc && k2 < cpc && back <= k && back <= k2);
                            // k lies on the low face, k2 on the high face, and they differ along the axis alone
                            const uint32_t l[3] = {k / (uint32_t)(n[1] * n[2]), (k / (uint32_t)n[2]) % (uint32_t)n[1], k % (uint32_t)n[2]};
                            const uint32_t l2[3] = {k2 / (uint32_t)(n[1] * n[2]), (k2 / (uint32_t)n[2]) % (uint32_t)n[1], k2 % (uint32_t)n[2]};
                            for (int a = 0; a < 3; ++a) CHECK(a == axis ? l[a] == 0 && l2[a] == (uint32_t)n[a] - 1 : l[a] == l2[a]);
                            CHECK(seen.insert({k, k2}).second);
                            const uint32_t c = own[own_cells ? k : 0], c2 = other[other_cells ? k2 : 0];
                            if (c == c2) truth.join((uint32_t)dsh_cc_node(own_base, own_cells, k), (uint32_t)dsh_cc_node(other_base, other_cells, k2));
                            if (c != c2) continue;
                            if (back && own[own_cells ? k - back : 0] == c && other[other_cells ? k2 - back : 0] == c) continue;
                            model.join((uint32_t)dsh_cc_node(own_base, own_cells, k), (uint32_t)dsh_cc_node(other_base, other_cells, k2));
                            ++links;
                        }
                        if (own_cells || other_cells) CHECK(seen.size() == face);
                        if (!own_cells && !other_cells) CHECK(links == (own[0] == other[0] ? 1u : 0u));
                        for (uint32_t v = 0; v < nodes; ++v) CHECK(model.find(v) == truth.find(v));
                    }
    }
}

int main() {
    NodeBases();
    SizeEdge();
    Scratch();
    Classes();
    FacePairs();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("dsh components plan OK\n");
    return 0;
}
