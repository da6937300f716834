// sdfgpu_mesh.hpp -- rasterising the triangle meshes of a planning scene into occupancy: the decision procedure of include/sdfgpu.h
// "Planes and triangle meshes" (DESIGN.md section 27), the arguments of its kernels and the layout of its scratch.  As in
// sdfgpu_scene.hpp the procedure is plain C++ (SC_HD functions of doubles): tests/mesh_predicate_host.cpp runs the very same text on
// the CPU against the numpy restatement (tests/mesh_raster_restated.py); the kernels are in sdfgpu_mesh.hip.
//
// The plane of the same section is a member of the shape list and is decided by sc_plane in sdfgpu_scene.hpp (included here):
//   N_a = (r_a0 n_0 + r_a1 n_1) + r_a2 n_2,  s = (N_0 (c_0 - t_0) + N_1 (c_1 - t_1)) + N_2 (c_2 - t_2),  filled iff
//   |s| <= h ((|N_0| + |N_1|) + |N_2|).
//
// Arithmetic: doubles, separate products and sums in the order written, no FMA: every unit that includes this header must
// compile it under `#pragma clang fp contract(off)` (or -ffp-contract=off).
#pragma once
#include "sdfgpu_scene.hpp"

namespace sdfgpu {

constexpr int64_t kMrMaxMeshes = 65536;            // SDFGPU_MAX_MESHES
constexpr int64_t kMrMaxTriangles = 1 << 24;       // SDFGPU_MAX_TRIANGLES
constexpr int kMrThreads = 256;
constexpr int kMrScanBlock = 1024;                 // slots of one k_mr_scan_blocks workgroup: four per thread
constexpr int kMrTile = 16;                        // a work item: one 16 x 16 x 16 tile of a triangle's index box, one wave;
constexpr int kMrSub = 4;                          //   its 64 lanes first judge the tile's 64 sub-tiles of 4 x 4 x 4, then voxels
constexpr int kMrChunk = 16;                       // consecutive work items a wave takes at a time (one binary search for them)
constexpr int kMrScatterGroups = 2048;             // workgroups of k_mr_scatter, whatever the work: they stride over the chunks
constexpr uint32_t kMrNoBadMesh = 0xFFFFFFFFu;

// scratch: status block | first slot per mesh (n_meshes + 1) | tile sums per scan block (+ 1) | tile counts, then their exclusive
// scan within the block, per slot | world vertices per slot (9 doubles) | object id per slot.  A slot is one triangle of one mesh;
// there are at most n_triangles of them.
inline size_t mr_round(size_t b) { return (b + 255) & ~(size_t)255; }
SC_HD int64_t mr_scan_blocks(int64_t n_triangles) { return (n_triangles + kMrScanBlock - 1) / kMrScanBlock; }
inline size_t mr_first_offset() { return kScStatusBytes; }
inline size_t mr_top_offset(int64_t n_meshes) { return mr_first_offset() + mr_round((size_t)(n_meshes + 1) * 8); }
inline size_t mr_scan_offset(int64_t n_meshes, int64_t n_triangles) { return mr_top_offset(n_meshes) + mr_round((size_t)(mr_scan_blocks(n_triangles) + 1) * 8); }
inline size_t mr_world_offset(int64_t n_meshes, int64_t n_triangles) { return mr_scan_offset(n_meshes, n_triangles) + mr_round((size_t)n_triangles * 8); }
inline size_t mr_id_offset(int64_t n_meshes, int64_t n_triangles) { return mr_world_offset(n_meshes, n_triangles) + mr_round((size_t)n_triangles * 72); }
inline size_t mesh_scratch_bytes(int64_t n_meshes, int64_t n_triangles) { return mr_id_offset(n_meshes, n_triangles) + mr_round((size_t)n_triangles * 4); }

struct MeshArgs {
    const sdfgpu_mesh* meshes;
    const double* vertices;
    const uint32_t* triangles;
    int64_t n_meshes, n_vertices, n_triangles;
    double origin[12];
    double inverse[9];                 // of the origin's 3 x 3 block (culling only); all zero with `no_inverse` when it has none
    int no_inverse;
    double res, half;
    int64_t nx, ny, nz, n;
    uint32_t* status;                  // [0]: the lowest refused mesh index, or kMrNoBadMesh; bytes 8 .. 15: the number of work items
    int64_t* first;                    // [n_meshes + 1] exclusive scan of the meshes' triangle counts: the first slot of each
    int64_t* top;                      // [scan blocks + 1] exclusive scan of the blocks' tile sums
    int64_t* scan;                     // [n_triangles] per slot
    double* world;                     // [n_triangles][9] W_0, W_1, W_2
    uint32_t* slot_id;                 // [n_triangles]
    uint32_t* bits;
    uint8_t* mask;
    uint32_t* ids;
    int accumulate;
};

// ---- the decision procedure ----------------------------------------------------------------------------------------------------------
// W = pose * v, rows as ((m0 v0 + m1 v1) + m2 v2) + m3
SC_HD void mr_world(const double* p, const double* v, double w[3]) {
    for (int r = 0; r < 3; ++r) w[r] = ((p[4 * r] * v[0] + p[4 * r + 1] * v[1]) + p[4 * r + 2] * v[2]) + p[4 * r + 3];
}

// what a triangle contributes that does not depend on the voxel: world vertices, edges f_j = W_{j+1} - W_j and n = f_0 x f_1
struct MrTriangle {
    double W[3][3], f[3][3], n[3];
};

SC_HD void mr_triangle(const double W0[3], const double W1[3], const double W2[3], MrTriangle& t) {
    for (int k = 0; k < 3; ++k) {
        t.W[0][k] = W0[k]; t.W[1][k] = W1[k]; t.W[2][k] = W2[k];
        t.f[0][k] = W1[k] - W0[k];
        t.f[1][k] = W2[k] - W1[k];
        t.f[2][k] = W0[k] - W2[k];
    }
    t.n[0] = t.f[0][1] * t.f[1][2] - t.f[0][2] * t.f[1][1];
    t.n[1] = t.f[0][2] * t.f[1][0] - t.f[0][0] * t.f[1][2];
    t.n[2] = t.f[0][0] * t.f[1][1] - t.f[0][1] * t.f[1][0];
}

// an axis with projections p_0, p_1, p_2 of the triangle and radius r of the cube separates only when all of the triangle lies
// strictly beyond the cube: an axis that degenerates to 0 has p = 0 and r = 0 and never does
SC_HD bool mr_separates(double p0, double p1, double p2, double r) {
    return sc_min(sc_min(p0, p1), p2) > r || sc_max(sc_max(p0, p1), p2) < -r;
}

// TRIANGLE against the probe cube of half side h about c: thirteen axes, in this order: e_x, e_y, e_z; n; e_a x f_j for a = x, y, z
// (outer) and j = 0, 1, 2 (inner), with a1 = a + 1 and a2 = a + 2 (mod 3): (e_a x f)_a1 = -f_a2, (e_a x f)_a2 = f_a1.
SC_HD bool mr_hit(const MrTriangle& t, const double c[3], double h) {
    double u[3][3];
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) u[i][k] = t.W[i][k] - c[k];
    for (int a = 0; a < 3; ++a)
        if (mr_separates(u[0][a], u[1][a], u[2][a], h)) return false;
    {
        const double p0 = (t.n[0] * u[0][0] + t.n[1] * u[0][1]) + t.n[2] * u[0][2];
        const double p1 = (t.n[0] * u[1][0] + t.n[1] * u[1][1]) + t.n[2] * u[1][2];
        const double p2 = (t.n[0] * u[2][0] + t.n[1] * u[2][1]) + t.n[2] * u[2][2];
        if (mr_separates(p0, p1, p2, h * ((sc_abs(t.n[0]) + sc_abs(t.n[1])) + sc_abs(t.n[2])))) return false;
    }
    for (int a = 0; a < 3; ++a) {
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
        for (int j = 0; j < 3; ++j) {
            const double fa1 = t.f[j][a1], fa2 = t.f[j][a2];
            const double p0 = u[0][a2] * fa1 - u[0][a1] * fa2;
            const double p1 = u[1][a2] * fa1 - u[1][a1] * fa2;
            const double p2 = u[2][a2] * fa1 - u[2][a1] * fa2;
            if (mr_separates(p0, p1, p2, h * (sc_abs(fa2) + sc_abs(fa1)))) return false;
        }
    }
    return true;
}

// ---- culling (not part of the restatement) ---------------------------------------------------------------------------------------------
// The same thirteen axes against a box of half sides H[3] (world axes) about c, every radius padded by a relative 2^-20 and by
// 2^-30 of the magnitudes that went into the projections: false only when the exact test is false for every probe inside the box.
SC_HD bool mr_may_hit(const MrTriangle& t, const double c[3], const double H[3]) {
    double u[3][3], big = 0.0;
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) { u[i][k] = t.W[i][k] - c[k]; big = sc_max(big, sc_abs(u[i][k])); }
    big = big + (sc_abs(c[0]) + sc_abs(c[1]) + sc_abs(c[2]));                  // (the rounding of u itself is relative to W and c)
    const double rel = 9.5367431640625e-07, tiny = 9.313225746154785e-10;
    for (int a = 0; a < 3; ++a)
        if (mr_separates(u[0][a], u[1][a], u[2][a], H[a] + (rel * H[a] + tiny * big))) return false;
    {
        const double A[3] = {sc_abs(t.n[0]), sc_abs(t.n[1]), sc_abs(t.n[2])};
        const double r = H[0] * A[0] + H[1] * A[1] + H[2] * A[2];
        const double p0 = t.n[0] * u[0][0] + t.n[1] * u[0][1] + t.n[2] * u[0][2];
        const double p1 = t.n[0] * u[1][0] + t.n[1] * u[1][1] + t.n[2] * u[1][2];
        const double p2 = t.n[0] * u[2][0] + t.n[1] * u[2][1] + t.n[2] * u[2][2];
        if (mr_separates(p0, p1, p2, r + (rel * r + tiny * (big * (A[0] + A[1] + A[2]))))) return false;
    }
    for (int a = 0; a < 3; ++a) {
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
        for (int j = 0; j < 3; ++j) {
            const double fa1 = t.f[j][a1], fa2 = t.f[j][a2];
            const double r = H[a1] * sc_abs(fa2) + H[a2] * sc_abs(fa1);
            const double p0 = u[0][a2] * fa1 - u[0][a1] * fa2;
            const double p1 = u[1][a2] * fa1 - u[1][a1] * fa2;
            const double p2 = u[2][a2] * fa1 - u[2][a1] * fa2;
            if (mr_separates(p0, p1, p2, r + (rel * r + tiny * (big * (sc_abs(fa1) + sc_abs(fa2)))))) return false;
        }
    }
    return true;
}

// The index box lo[k] .. hi[k] (inclusive, clipped to the grid; lo > hi on some axis: empty) that holds every voxel whose probe can
// meet the triangle.  A point P of the triangle within the probe of centre c has |inverse (P - c)|_k <= h sum_j |inverse_kj|, and
// inverse (c - t) = res (index + 1/2): so res (index_k + 1/2) lies within that of the triangle's extent in grid coordinate k.  The
// reach is taken 1.25 times as large and padded by 2^-30 of the magnitudes involved; an origin without an inverse, or any value
// that is not finite, gives the whole grid.
SC_HD void mr_index_box(const MeshArgs& a, const MrTriangle& t, int64_t lo[3], int64_t hi[3]) {
    const int64_t dims[3] = {a.nx, a.ny, a.nz};
    for (int k = 0; k < 3; ++k) {
        lo[k] = 0; hi[k] = dims[k] - 1;
        if (a.no_inverse) continue;
        const double* inv = a.inverse + 3 * k;
        const double row = (sc_abs(inv[0]) + sc_abs(inv[1])) + sc_abs(inv[2]);
        double gmin = 0.0, gmax = 0.0, mag = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double d0 = t.W[i][0] - a.origin[3], d1 = t.W[i][1] - a.origin[7], d2 = t.W[i][2] - a.origin[11];
            const double g = inv[0] * d0 + inv[1] * d1 + inv[2] * d2;
            mag = sc_max(mag, sc_abs(inv[0]) * (sc_abs(t.W[i][0]) + sc_abs(a.origin[3])) + sc_abs(inv[1]) * (sc_abs(t.W[i][1]) + sc_abs(a.origin[7])) +
                                  sc_abs(inv[2]) * (sc_abs(t.W[i][2]) + sc_abs(a.origin[11])));
            if (i == 0) { gmin = g; gmax = g; }
            else { gmin = sc_min(gmin, g); gmax = sc_max(gmax, g); }
        }
        const double reach = 1.25 * (a.half * row) + 9.313225746154785e-10 * (mag + a.res);
        const double below = (gmin - reach) / a.res - 0.5, above = (gmax + reach) / a.res - 0.5;
        const double top = (double)(dims[k] - 1);
        if (below > top) { lo[k] = 1; hi[k] = 0; continue; }               // (false for a NaN: the whole axis stays)
        if (above < 0.0) { lo[k] = 1; hi[k] = 0; continue; }
        if (below > 0.0) lo[k] = (int64_t)below;                             // floor
        if (above < top) hi[k] = (int64_t)above + 1 < dims[k] - 1 ? (int64_t)above + 1 : dims[k] - 1;    // at least the ceiling
    }
}

// the number of kMrTile^3 tiles the box splits into, counted from its low corner
SC_HD int64_t mr_tiles(const int64_t lo[3], const int64_t hi[3], int64_t per[3]) {
    int64_t count = 1;
    for (int k = 0; k < 3; ++k) {
        per[k] = hi[k] < lo[k] ? 0 : (hi[k] - lo[k]) / kMrTile + 1;
        count *= per[k];
    }
    return count;
}

// one mesh record by itself: runs inside the arrays, a finite pose and (for ids) an id that is neither 0 nor 0xFFFFFFFF
SC_HD bool mr_mesh_valid(const sdfgpu_mesh& m, int64_t n_vertices, int64_t n_triangles, bool ids) {
    if (m.first_triangle < 0 || m.n_triangles < 0 || m.first_triangle > n_triangles || m.n_triangles > n_triangles - m.first_triangle) return false;
    if (m.first_vertex < 0 || m.n_vertices < 0 || m.first_vertex > n_vertices || m.n_vertices > n_vertices - m.first_vertex) return false;
    for (int i = 0; i < 12; ++i) if (!sc_finite(m.pose[i])) return false;
    if (ids && (m.object_id == 0 || m.object_id == 0xFFFFFFFFu)) return false;
    return true;
}

// one triangle of a valid mesh: indices below the mesh's n_vertices, finite vertices, finite world vertices; W[9] is written
SC_HD bool mr_triangle_valid(const sdfgpu_mesh& m, const double* vertices, const uint32_t* tri, double* W) {
    for (int i = 0; i < 3; ++i) {
        if ((int64_t)tri[i] >= m.n_vertices) return false;
        const double* v = vertices + 3 * (m.first_vertex + (int64_t)tri[i]);
        if (!(sc_finite(v[0]) && sc_finite(v[1]) && sc_finite(v[2]))) return false;
        mr_world(m.pose, v, W + 3 * i);
        if (!(sc_finite(W[3 * i]) && sc_finite(W[3 * i + 1]) && sc_finite(W[3 * i + 2]))) return false;
    }
    return true;
}

}  // namespace sdfgpu
