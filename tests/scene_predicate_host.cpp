// The shape rasteriser's decision procedure (sdf_tools_amd/csrc/sdfgpu_scene.hpp: the text the kernels compile) run on the CPU,
// so that tests/test_scene_raster_cpu.py can compare it bit for bit with the numpy restatement without a GPU.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I include -I sdf_tools_amd/csrc tests/scene_predicate_host.cpp
// Input file:  int64 n_shapes, int64 n_points, double h | n_shapes sdfgpu_shape records | n_points x 3 doubles (probe centres)
// Output file: per point one uint32: 0, or 1 + the index of the first shape in list order whose solid meets the probe;
//              then per shape one byte: sc_shape_valid; then per shape 3 doubles: sc_half_extents (zeros for a refused shape)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sdfgpu_scene.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    int64_t n_shapes = 0, n_points = 0;
    double h = 0.0;
    if (fread(&n_shapes, 8, 1, in) != 1 || fread(&n_points, 8, 1, in) != 1 || fread(&h, 8, 1, in) != 1) return 4;
    std::vector<sdfgpu_shape> shapes((size_t)n_shapes);
    std::vector<double> points((size_t)n_points * 3);
    if (n_shapes && fread(shapes.data(), sizeof(sdfgpu_shape), shapes.size(), in) != shapes.size()) return 4;
    if (n_points && fread(points.data(), 8, points.size(), in) != points.size()) return 4;
    fclose(in);
    std::vector<uint32_t> first((size_t)n_points, 0);
    std::vector<unsigned char> valid((size_t)n_shapes);
    std::vector<double> extents((size_t)n_shapes * 3, 0.0);
    for (int64_t s = 0; s < n_shapes; ++s) {
        valid[s] = sdfgpu::sc_shape_valid(shapes[s]) ? 1 : 0;
        if (valid[s]) sdfgpu::sc_half_extents(shapes[s], &extents[3 * s]);
    }
    for (int64_t i = 0; i < n_points; ++i)
        for (int64_t s = 0; s < n_shapes && !first[i]; ++s)
            if (valid[s] && sdfgpu::sc_hit(shapes[s], &points[3 * i], h)) first[i] = (uint32_t)(s + 1);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    fwrite(first.data(), 4, first.size(), out);
    fwrite(valid.data(), 1, valid.size(), out);
    fwrite(extents.data(), 8, extents.size(), out);
    fclose(out);
    return 0;
}
