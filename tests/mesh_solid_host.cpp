// The solid fill's decision procedure (sdf_tools_amd/csrc/sdfgpu_mesh_solid.hpp: the text the kernels compile) run on the CPU, so that
// tests/test_mesh_solid_cpu.py can compare it bit for bit with the numpy restatement, and its exact orientation sign with
// fractions.Fraction, without a GPU.  Also built with -fsanitize=address,undefined.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I include -I sdf_tools_amd/csrc tests/mesh_solid_host.cpp
//   mesh_solid_host orient IN OUT   IN: int64 n | n x 6 doubles (P, Q, C).  OUT: per case two int8: ms_orient_exact, ms_orient
//   mesh_solid_host fill IN OUT     IN: int64 n_meshes, n_vertices, n_triangles, nx, ny, nz | double res | 16 doubles origin |
//                                       sdfgpu_mesh records | n_vertices x 3 doubles | n_triangles x 3 uint32
//                                   OUT: int64: the lowest refused mesh index, -1 for none, -2 for an origin without an inverse; per
//                                       voxel one uint32: the smallest object id among the meshes that fill it, 0 for none
//   mesh_solid_host cull IN OUT     IN: int64 n, nx, ny | double res | n x 9 doubles: triangles in GRID coordinates (ms_grid's output)
//                                   OUT: per triangle seven int64: ms_column_box's lo[0], lo[1], hi[0], hi[1], then ms_tiles' per[0],
//                                       per[1] and its count
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sdfgpu_mesh_solid.hpp"

using namespace sdfgpu;

static int run_orient(FILE* in, FILE* out) {
    int64_t n = 0;
    if (fread(&n, 8, 1, in) != 1 || n < 0) return 4;
    std::vector<double> v((size_t)n * 6);
    if (n && fread(v.data(), 8, v.size(), in) != v.size()) return 4;
    std::vector<signed char> sign((size_t)n * 2);
    for (int64_t i = 0; i < n; ++i) {
        const double* p = &v[6 * i];
        double det;
        sign[2 * i] = (signed char)ms_orient_exact(p, p + 2, p + 4);
        sign[2 * i + 1] = (signed char)ms_orient(p, p + 2, p + 4, det);
    }
    if (n) fwrite(sign.data(), 1, sign.size(), out);
    return 0;
}

static int run_fill(FILE* in, FILE* out) {
    int64_t count[6];
    double res = 0.0, origin[16];
    if (fread(count, 8, 6, in) != 6 || fread(&res, 8, 1, in) != 1 || fread(origin, 8, 16, in) != 16) return 4;
    const int64_t n_meshes = count[0], n_vertices = count[1], n_triangles = count[2], nx = count[3], ny = count[4], nz = count[5];
    std::vector<sdfgpu_mesh> meshes((size_t)n_meshes);
    std::vector<double> vertices((size_t)n_vertices * 3);
    std::vector<uint32_t> triangles((size_t)n_triangles * 3);
    if (n_meshes && fread(meshes.data(), sizeof(sdfgpu_mesh), meshes.size(), in) != meshes.size()) return 4;
    if (n_vertices && fread(vertices.data(), 8, vertices.size(), in) != vertices.size()) return 4;
    if (n_triangles && fread(triangles.data(), 4, triangles.size(), in) != triangles.size()) return 4;

    MeshArgs a{};
    for (int i = 0; i < 12; ++i) a.origin[i] = origin[i];
    a.no_inverse = ms_inverse(origin, a.inverse) ? 0 : 1;
    a.res = res; a.half = res * 0.5;
    a.nx = nx; a.ny = ny; a.nz = nz; a.n = nx * ny * nz;
    int64_t bad = a.no_inverse ? -2 : -1, slots = 0;
    std::vector<uint32_t> ids((size_t)a.n, 0);
    std::vector<std::vector<double>> world((size_t)n_meshes);
    for (int64_t m = 0; m < n_meshes && bad == -1; ++m) {
        bool ok = mr_mesh_valid(meshes[m], n_vertices, n_triangles, true);
        if (ok) { slots += meshes[m].n_triangles; ok = slots <= n_triangles; }
        for (int64_t j = 0; ok && j < meshes[m].n_triangles; ++j) {
            double W[9], G[3][3];
            ok = mr_triangle_valid(meshes[m], vertices.data(), triangles.data() + 3 * (meshes[m].first_triangle + j), W) && ms_grid_triangle(a, W, G);
            world[m].insert(world[m].end(), W, W + 9);
        }
        if (!ok) bad = m;
    }
    auto take = [&](int64_t v, uint32_t id) { if (ids[v] == 0 || id < ids[v]) ids[v] = id; };
    std::vector<unsigned char> toggle((size_t)nz + 1);
    for (int64_t m = 0; m < n_meshes && bad == -1; ++m) {
        const uint32_t id = meshes[m].object_id;
        const int64_t nt = meshes[m].n_triangles;
        std::vector<MrTriangle> tris((size_t)nt);
        std::vector<double> grid((size_t)nt * 9);
        for (int64_t j = 0; j < nt; ++j) {
            const double* W = &world[m][9 * j];
            mr_triangle(W, W + 3, W + 6, tris[j]);
            double G[3][3];
            ms_grid_triangle(a, W, G);
            std::memcpy(&grid[9 * j], G, sizeof G);
        }
        for (int64_t x = 0; x < nx; ++x)
            for (int64_t y = 0; y < ny; ++y) {
                // (a): every triangle against every probe of the column
                for (int64_t z = 0; z < nz; ++z) {
                    double c[3];
                    sc_centre(a.origin, res, x, y, z, c);
                    for (int64_t j = 0; j < nt; ++j)
                        if (mr_hit(tris[j], c, a.half)) { take((x * ny + y) * nz + z, id); break; }
                }
                // (b): the crossings of the column, then the prefix parity
                std::fill(toggle.begin(), toggle.end(), 0);
                const double C[2] = {res * ((double)x + 0.5), res * ((double)y + 0.5)};
                for (int64_t j = 0; j < nt; ++j) {
                    double G[3][3], zc;
                    std::memcpy(G, &grid[9 * j], sizeof G);
                    if (ms_crossing(G, C, zc)) toggle[(size_t)ms_first_above(res, nz, zc)] ^= 1;
                }
                unsigned char inside = 0;
                for (int64_t z = 0; z < nz; ++z) {
                    inside ^= toggle[z];
                    if (inside) take((x * ny + y) * nz + z, id);
                }
            }
    }
    if (bad != -1) std::fill(ids.begin(), ids.end(), 0);
    fwrite(&bad, 8, 1, out);
    if (!ids.empty()) fwrite(ids.data(), 4, ids.size(), out);
    return 0;
}

// the culling, which run_fill never calls: ms_column_box and ms_tiles per triangle, given in grid coordinates
static int run_cull(FILE* in, FILE* out) {
    int64_t count[3];
    double res = 0.0;
    if (fread(count, 8, 3, in) != 3 || fread(&res, 8, 1, in) != 1 || count[0] < 0) return 4;
    std::vector<double> grid((size_t)count[0] * 9);
    if (count[0] && fread(grid.data(), 8, grid.size(), in) != grid.size()) return 4;
    MeshArgs a{};
    a.res = res; a.half = res * 0.5;
    a.nx = count[1]; a.ny = count[2];
    std::vector<int64_t> rows((size_t)count[0] * 7);
    for (int64_t j = 0; j < count[0]; ++j) {
        double G[3][3];
        std::memcpy(G, &grid[9 * j], sizeof G);
        int64_t* r = &rows[7 * j];
        ms_column_box(a, G, r, r + 2);
        r[6] = ms_tiles(r, r + 2, r + 4);
    }
    if (!rows.empty()) fwrite(rows.data(), 8, rows.size(), out);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 3;
    const int rc = std::strcmp(argv[1], "orient") == 0 ? run_orient(in, out) : std::strcmp(argv[1], "fill") == 0 ? run_fill(in, out)
                   : std::strcmp(argv[1], "cull") == 0 ? run_cull(in, out) : 2;
    fclose(in);
    fclose(out);
    return rc;
}
