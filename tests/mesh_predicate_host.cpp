// The mesh rasteriser's and the plane's decision procedure (sdf_tools_amd/csrc/sdfgpu_mesh.hpp and sc_plane of sdfgpu_scene.hpp: the
// text the kernels compile) run on the CPU, so that tests/test_mesh_raster_cpu.py can compare it bit for bit with the numpy
// restatement without a GPU.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I include -I sdf_tools_amd/csrc tests/mesh_predicate_host.cpp
// Input file:  int64 n_meshes, n_vertices, n_triangles, n_shapes, n_points, double h | sdfgpu_mesh records | n_vertices x 3 doubles |
//              n_triangles x 3 uint32 | sdfgpu_shape records | n_points x 3 doubles (probe centres)
// Output file: int64: the lowest refused mesh index (ids asked for), or -1; per point one uint32: the smallest object id among the
//              meshes with a triangle that meets the probe, 0 for none (all 0 when a mesh is refused); per point one uint32: 0, or
//              1 + the index of the first valid shape in list order that meets the probe; per shape one byte: sc_shape_valid
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sdfgpu_mesh.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    int64_t count[5] = {0, 0, 0, 0, 0};
    double h = 0.0;
    if (fread(count, 8, 5, in) != 5 || fread(&h, 8, 1, in) != 1) return 4;
    const int64_t n_meshes = count[0], n_vertices = count[1], n_triangles = count[2], n_shapes = count[3], n_points = count[4];
    std::vector<sdfgpu_mesh> meshes((size_t)n_meshes);
    std::vector<double> vertices((size_t)n_vertices * 3), points((size_t)n_points * 3);
    std::vector<uint32_t> triangles((size_t)n_triangles * 3);
    std::vector<sdfgpu_shape> shapes((size_t)n_shapes);
    if (n_meshes && fread(meshes.data(), sizeof(sdfgpu_mesh), meshes.size(), in) != meshes.size()) return 4;
    if (n_vertices && fread(vertices.data(), 8, vertices.size(), in) != vertices.size()) return 4;
    if (n_triangles && fread(triangles.data(), 4, triangles.size(), in) != triangles.size()) return 4;
    if (n_shapes && fread(shapes.data(), sizeof(sdfgpu_shape), shapes.size(), in) != shapes.size()) return 4;
    if (n_points && fread(points.data(), 8, points.size(), in) != points.size()) return 4;
    fclose(in);

    int64_t bad = -1, slots = 0;
    std::vector<sdfgpu::MrTriangle> tris;
    std::vector<uint32_t> tri_id;
    for (int64_t m = 0; m < n_meshes && bad < 0; ++m) {
        bool ok = sdfgpu::mr_mesh_valid(meshes[m], n_vertices, n_triangles, true);
        if (ok) { slots += meshes[m].n_triangles; ok = slots <= n_triangles; }
        for (int64_t j = 0; ok && j < meshes[m].n_triangles; ++j) {
            double W[9];
            ok = sdfgpu::mr_triangle_valid(meshes[m], vertices.data(), triangles.data() + 3 * (meshes[m].first_triangle + j), W);
            if (ok) {
                sdfgpu::MrTriangle t;
                sdfgpu::mr_triangle(W, W + 3, W + 6, t);
                tris.push_back(t);
                tri_id.push_back(meshes[m].object_id);
            }
        }
        if (!ok) bad = m;
    }
    std::vector<uint32_t> ids((size_t)n_points, 0), first((size_t)n_points, 0);
    if (bad < 0)
        for (int64_t i = 0; i < n_points; ++i)
            for (size_t k = 0; k < tris.size(); ++k)
                if ((ids[i] == 0 || tri_id[k] < ids[i]) && sdfgpu::mr_hit(tris[k], &points[3 * i], h)) ids[i] = tri_id[k];
    std::vector<unsigned char> valid((size_t)n_shapes);
    for (int64_t s = 0; s < n_shapes; ++s) valid[s] = sdfgpu::sc_shape_valid(shapes[s]) ? 1 : 0;
    for (int64_t i = 0; i < n_points; ++i)
        for (int64_t s = 0; s < n_shapes && !first[i]; ++s)
            if (valid[s] && sdfgpu::sc_hit(shapes[s], &points[3 * i], h)) first[i] = (uint32_t)(s + 1);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    fwrite(&bad, 8, 1, out);
    if (!ids.empty()) fwrite(ids.data(), 4, ids.size(), out);
    if (!first.empty()) fwrite(first.data(), 4, first.size(), out);
    if (!valid.empty()) fwrite(valid.data(), 1, valid.size(), out);
    fclose(out);
    return 0;
}
