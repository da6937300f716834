// topology_restated.cpp -- test infrastructure, never on the product path: a plain restatement of the reference's
// ComputeComponentTopology (src/sdf_tools/collision_map.cpp:620-671 over include/sdf_tools/topology_computation.hpp:297-672:
// ExtractComponentSurfaces, ComputeHolesInSurface, ComputeConnectivityOfSurfaceVertices) that the GPU counters are compared
// with bit for bit.
//
// The reference, per component c:
//   1. surface voxels: every voxel of c the caller's is_surface_index_fn accepts (a selected voxel with a face neighbour of
//      another component; grid-edge voxels count as surface);
//   2. surface vertices: for each surface voxel and each of its 8 corners, the corner is added when one of the three face
//      neighbours of the voxel towards that corner is not c;
//   3. per surface vertex: the 6-bit edge mask (an edge is exposed when the 4 voxels around it hold c and something else),
//      edge count e, tallies M3 / M5 / M6;
//   4. surfaces = connected components of the surface vertices along the exposed edges (breadth-first search, whose lookup of
//      a reached vertex throws std::out_of_range when the vertex is not in the set);
//   5. voids = surfaces - 1, holes = 1 + (M5 + 2 M6 - M3) / 8 + voids (int32, C truncation).
// Here the per-component hash maps are flat per-vertex bytes: vertex (i, j, k) (0 <= i <= nx ...) is the corner shared by the
// voxels (i-1..i, j-1..j, k-1..k), its "cube", at slots s = 4 dx + 2 dy + dz; the pair (vertex, c) is bit s of the vertex's
// byte, s being the first slot of the cube that holds c.  Same sets, same graph, same counts; no hashing, so 512^3 runs on one
// core in seconds.
//
// literal = 0 (the library's contract, include/sdfgpu.h): the corner test reads the +z neighbour at z + 1, and the surface-voxel
//   test sees every out-of-grid voxel as component -1.
// literal = 1 (the reference as written): the "+z" neighbour is read at z - 1 (topology_computation.hpp:383-386), and the
//   surface-voxel test (collision_map.hpp:96-152) treats z == nz - 1 as interior (its "z_index == GetNumZCells()" slip) and
//   compares against the out-of-grid cell's component, oob_component.  Where the reference would throw, this returns 1 and the
//   vertex the search reached in throw_at[0..2].
// Returns 0, 1 (would throw), or -1 when a label exceeds max_label.  out: (max_label + 1) x 5 int64:
//   surface vertices, M3, M5, M6, surfaces.
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

struct Grid {
    const uint32_t* labels;
    int64_t nx, ny, nz;
    bool in(int64_t x, int64_t y, int64_t z) const { return x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz; }
    int64_t comp(int64_t x, int64_t y, int64_t z) const { return in(x, y, z) ? (int64_t)labels[(x * ny + y) * nz + z] : -1; }
    // the eight voxels around vertex (i, j, k), slot s = 4 dx + 2 dy + dz
    void cube(int64_t i, int64_t j, int64_t k, int64_t out[8]) const {
        for (int s = 0; s < 8; ++s) out[s] = comp(i - 1 + (s >> 2), j - 1 + ((s >> 1) & 1), k - 1 + (s & 1));
    }
};

int first_slot(const int64_t cube[8], int64_t c) {
    for (int s = 0; s < 8; ++s)
        if (cube[s] == c) return s;
    return -1;
}

// the reference's edge mask of (vertex, c): bit 0 z-, 1 z+, 2 y-, 3 y+, 4 x-, 5 x+ (topology_computation.hpp:531-608)
int edge_mask(const int64_t cube[8], int64_t c) {
    static const int faces[6][4] = {{0, 2, 4, 6}, {1, 3, 5, 7}, {0, 1, 4, 5}, {2, 3, 6, 7}, {0, 1, 2, 3}, {4, 5, 6, 7}};
    int m = 0;
    for (int e = 0; e < 6; ++e) {
        int in = 0;
        for (int q = 0; q < 4; ++q) in += cube[faces[e][q]] == c;
        if (in > 0 && in < 4) m |= 1 << e;
    }
    return m;
}

}  // namespace

extern "C" int topo_restated(const uint32_t* labels, const uint8_t* select, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label,
                             int literal, uint32_t oob_component, int64_t* out, int64_t* throw_at) {
    const Grid g{labels, nx, ny, nz};
    const int64_t n = nx * ny * nz;
    for (int64_t v = 0; v < n; ++v)
        if (labels[v] > max_label) return -1;
    for (int64_t i = 0; i < ((int64_t)max_label + 1) * 5; ++i) out[i] = 0;
    const int64_t vx = nx + 1, vy = ny + 1, vz = nz + 1, nv = vx * vy * vz;
    auto vid = [=](int64_t i, int64_t j, int64_t k) { return (i * vy + j) * vz + k; };
    std::vector<uint8_t> node(nv, 0);
    int64_t cb[8];

    auto add = [&](int64_t i, int64_t j, int64_t k, int64_t c) {
        g.cube(i, j, k, cb);
        node[vid(i, j, k)] |= (uint8_t)(1u << first_slot(cb, c));
    };
    auto is_surface = [&](int64_t x, int64_t y, int64_t z, int64_t c) {
        if (select && !select[(x * ny + y) * nz + z]) return false;
        if (!literal) {
            return g.comp(x - 1, y, z) != c || g.comp(x + 1, y, z) != c || g.comp(x, y - 1, z) != c || g.comp(x, y + 1, z) != c ||
                   g.comp(x, y, z - 1) != c || g.comp(x, y, z + 1) != c;
        }
        if (x == 0 || y == 0 || z == 0 || x == nx - 1 || y == ny - 1) return true;          // (no z == nz - 1 here: the slip)
        auto cell = [&](int64_t a, int64_t b, int64_t d) { return g.in(a, b, d) ? g.comp(a, b, d) : (int64_t)oob_component; };
        return cell(x, y, z - 1) != c || cell(x, y, z + 1) != c || cell(x, y - 1, z) != c || cell(x, y + 1, z) != c ||
               cell(x - 1, y, z) != c || cell(x + 1, y, z) != c;
    };

    // 1 + 2: surface voxels -> surface vertices
    for (int64_t x = 0; x < nx; ++x)
        for (int64_t y = 0; y < ny; ++y)
            for (int64_t z = 0; z < nz; ++z) {
                const int64_t c = g.comp(x, y, z);
                if (!is_surface(x, y, z, c)) continue;
                const bool zm = g.comp(x, y, z - 1) != c, zp = g.comp(x, y, literal ? z - 1 : z + 1) != c;
                const bool ym = g.comp(x, y - 1, z) != c, yp = g.comp(x, y + 1, z) != c;
                const bool xm = g.comp(x - 1, y, z) != c, xp = g.comp(x + 1, y, z) != c;
                for (int s = 0; s < 8; ++s) {
                    const int dx = s >> 2, dy = (s >> 1) & 1, dz = s & 1;
                    if ((dz ? zp : zm) || (dy ? yp : ym) || (dx ? xp : xm)) add(x + dx, y + dy, z + dz, c);
                }
            }

    // 3: edge counts
    for (int64_t i = 0; i < vx; ++i)
        for (int64_t j = 0; j < vy; ++j)
            for (int64_t k = 0; k < vz; ++k) {
                const uint8_t m = node[vid(i, j, k)];
                if (!m) continue;
                g.cube(i, j, k, cb);
                for (int s = 0; s < 8; ++s) {
                    if (!((m >> s) & 1)) continue;
                    const int64_t c = cb[s];
                    int e = 0;
                    for (int em = edge_mask(cb, c); em; em &= em - 1) ++e;
                    out[c * 5 + 0] += 1;
                    if (e == 3) out[c * 5 + 1] += 1;
                    if (e == 5) out[c * 5 + 2] += 1;
                    if (e == 6) out[c * 5 + 3] += 1;
                }
            }

    // 4: surfaces by breadth-first search along the exposed edges
    std::vector<uint8_t> seen(nv, 0);
    std::vector<int64_t> queue;
    static const int step[6][3] = {{0, 0, -1}, {0, 0, 1}, {0, -1, 0}, {0, 1, 0}, {-1, 0, 0}, {1, 0, 0}};
    for (int64_t i = 0; i < vx; ++i)
        for (int64_t j = 0; j < vy; ++j)
            for (int64_t k = 0; k < vz; ++k) {
                const int64_t v0 = vid(i, j, k);
                for (int s0 = 0; s0 < 8; ++s0) {
                    if (!((node[v0] >> s0) & 1) || ((seen[v0] >> s0) & 1)) continue;
                    g.cube(i, j, k, cb);
                    const int64_t c = cb[s0];
                    out[c * 5 + 4] += 1;
                    queue.clear();
                    queue.push_back(v0 * 8 + s0);
                    seen[v0] |= (uint8_t)(1u << s0);
                    for (size_t head = 0; head < queue.size(); ++head) {
                        const int64_t v = queue[head] >> 3;
                        const int s = (int)(queue[head] & 7);
                        const int64_t a = v / (vy * vz), b = (v / vz) % vy, d = v % vz;
                        if (!((node[v] >> s) & 1)) {             // surface_vertex_connectivity.at(...) would throw here
                            if (throw_at) { throw_at[0] = a; throw_at[1] = b; throw_at[2] = d; }
                            return 1;
                        }
                        g.cube(a, b, d, cb);
                        const int em = edge_mask(cb, c);
                        for (int e = 0; e < 6; ++e) {
                            if (!((em >> e) & 1)) continue;
                            const int64_t a2 = a + step[e][0], b2 = b + step[e][1], d2 = d + step[e][2];
                            int64_t cb2[8];
                            g.cube(a2, b2, d2, cb2);
                            const int s2 = first_slot(cb2, c);             // (an exposed edge's 4 voxels hold c: s2 >= 0)
                            const int64_t v2 = vid(a2, b2, d2);
                            if ((seen[v2] >> s2) & 1) continue;
                            seen[v2] |= (uint8_t)(1u << s2);
                            queue.push_back(v2 * 8 + s2);
                        }
                    }
                }
            }
    return 0;
}
