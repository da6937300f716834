// sdfgpu_mesh_solid.hpp -- solid fill of closed triangle meshes: the decision procedure of include/sdfgpu.h "Solid meshes"
// (DESIGN.md section 28), the arguments of its kernels and the layout of its scratch.  As in sdfgpu_mesh.hpp the procedure is plain
// C++ (SC_HD functions of doubles): tests/mesh_solid_host.cpp runs the very same text on the CPU against the numpy restatement
// (tests/mesh_solid_restated.py); the kernels are in sdfgpu_mesh_solid.hip.
//
// A voxel is filled by a solid mesh when (a) its probe cube meets a triangle (mr_hit, unchanged) or (b) its centre is inside the mesh
// by the even-odd rule along the grid's z axis.  (b), per mesh and per column (x, y):
//   G_i = inverse * (W_i - t), rows as (i0 d0 + i1 d1) + i2 d2: the triangle's vertices in grid coordinates (metres)
//   C   = (res (x + 1/2), res (y + 1/2)): the column's centre
//   s_j = the EXACT sign of orient(P, Q, C) = (P_x - C_x)(Q_y - C_y) - (P_y - C_y)(Q_x - C_x) over the doubles P, Q, C, for the edges
//         (G_1, G_2), (G_2, G_0), (G_0, G_1); a zero is resolved as if C were displaced by (eps, eps^2): by the sign of P_y - Q_y, then
//         of Q_x - P_x (the top-left rule: orient is linear in C, so these are its derivatives), 0 only when P = Q in projection
//   the triangle covers the column iff s_0 = s_1 = s_2 != 0 (a triangle of projected area 0 never does: its edge values sum to 0)
//   z_c = ((w_0 z_0 + w_1 z_1) + w_2 z_2) / ((w_0 + w_1) + w_2) with w_j the edge values in doubles, clamped to the triangle's z range
//         (a NaN gives its lower end); the crossing toggles the first cell k of the column with res (k + 1/2) > z_c, k = 0 when it is
//         below the grid, nothing when there is no such cell
//   cell k is inside iff the number of toggles at cells <= k is odd.
// An edge is always evaluated from its endpoints in lexicographic order and negated when that swaps them, so that two triangles
// sharing an edge see the same doubles.
//
// Arithmetic: doubles, separate products and sums in the order written, no contraction: every unit that includes this header
// compiles it under `#pragma clang fp contract(off)` (or -ffp-contract=off).  The only fused operations are the explicit
// __builtin_fma calls of ms_two_prod, whose rounding error term they make exact.
#pragma once
#include <cmath>

#include "sdfgpu_mesh.hpp"

namespace sdfgpu {

constexpr int64_t kMsMaxMeshes = 256;              // SDFGPU_MAX_SOLID_MESHES
constexpr int kMsTile = 16;                        // a work item: 16 x 16 columns of a triangle's xy index box, one wave, four rows a pass
constexpr int kMsScatterGroups = 512;              // workgroups of k_ms_scatter, whatever the work: they stride over the chunks
constexpr int kMsMergeGroups = 1024;               // workgroups of k_ms_merge: they stride over the columns of the mesh's column box

// scratch behind the mesh rasteriser's (mesh_scratch_bytes): column-tile counts per slot, then their scan within the block | sums
// per scan block (+ 1) | per mesh the xy column box: [n_meshes][2] lows (unsigned minimum), then [n_meshes][2] highs + 1 (maximum)
inline size_t ms_scan_offset(int64_t n_meshes, int64_t n_triangles) { return mesh_scratch_bytes(n_meshes, n_triangles); }
inline size_t ms_top_offset(int64_t n_meshes, int64_t n_triangles) { return ms_scan_offset(n_meshes, n_triangles) + mr_round((size_t)n_triangles * 8); }
inline size_t ms_box_offset(int64_t n_meshes, int64_t n_triangles) { return ms_top_offset(n_meshes, n_triangles) + mr_round((size_t)(mr_scan_blocks(n_triangles) + 1) * 8); }
inline size_t ms_box_bytes(int64_t n_meshes) { return mr_round((size_t)n_meshes * 16); }                 // of the lows; as much for the highs
inline size_t mesh_solid_scratch_bytes(int64_t n_meshes, int64_t n_triangles) { return ms_box_offset(n_meshes, n_triangles) + 2 * ms_box_bytes(n_meshes); }
// the toggle field: one bit per cell, every column padded to whole words
SC_HD int64_t ms_row_words(int64_t nz) { return (nz + 31) / 32; }

struct SolidArgs {
    MeshArgs m;                        // scan and top are the surface pass's; everything else is shared
    int64_t* scan;                     // [n_triangles] column tiles per slot, then their exclusive scan within the block
    int64_t* top;                      // [scan blocks + 1] exclusive scan of the blocks' sums; the last is the total
    unsigned long long* box_lo;        // [n_meshes][2]
    unsigned long long* box_hi;        // [n_meshes][2], one past
    uint32_t* toggle;                  // [nx ny][wz], all zero outside a call
    int64_t wz;
    int64_t mesh;                      // the mesh of this scatter and merge pair
};

// ---- the decision procedure ----------------------------------------------------------------------------------------------------------
// the inverse of the 3 x 3 block of the row-major 4 x 4 origin by cofactors (host); false, and all zero, when it has none
inline bool ms_inverse(const double* o, double inverse[9]) {
    const double c00 = o[5] * o[10] - o[6] * o[9], c01 = o[6] * o[8] - o[4] * o[10], c02 = o[4] * o[9] - o[5] * o[8];
    const double det = o[0] * c00 + o[1] * c01 + o[2] * c02;
    const double inv[9] = {c00 / det, (o[2] * o[9] - o[1] * o[10]) / det, (o[1] * o[6] - o[2] * o[5]) / det,
                           c01 / det, (o[0] * o[10] - o[2] * o[8]) / det, (o[2] * o[4] - o[0] * o[6]) / det,
                           c02 / det, (o[1] * o[8] - o[0] * o[9]) / det, (o[0] * o[5] - o[1] * o[4]) / det};
    bool ok = sc_finite(det) && det != 0.0;
    for (int i = 0; i < 9; ++i) ok = ok && sc_finite(inv[i]);
    for (int i = 0; i < 9; ++i) inverse[i] = ok ? inv[i] : 0.0;
    return ok;
}

SC_HD void ms_grid(const double* inv, const double* o, const double W[3], double g[3]) {
    const double d0 = W[0] - o[3], d1 = W[1] - o[7], d2 = W[2] - o[11];
    for (int k = 0; k < 3; ++k) g[k] = (inv[3 * k] * d0 + inv[3 * k + 1] * d1) + inv[3 * k + 2] * d2;
}

// s + e = a + b exactly
SC_HD void ms_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// p + e = a * b exactly (while the product neither overflows nor falls below 2^-968)
SC_HD void ms_two_prod(double a, double b, double& p, double& e) {
    p = a * b;
    e = __builtin_fma(a, b, -p);
}

// The exact sign of orient(P, Q, C) = P_x Q_y - P_x C_y - C_x Q_y - P_y Q_x + P_y C_x + C_y Q_x: six two-products summed into a
// non-overlapping expansion (Shewchuk's GROW-EXPANSION), whose sign is that of its last non-zero component.  The sign does not
// change when all six inputs are scaled by a power of two: they are scaled so that the largest lies in [2^499, 2^500), and the
// result is exact whenever every non-zero input is at least 2^-980 of the largest.  Smaller inputs are not refused: their scaled
// values or products underflow and the sign may be wrong (include/sdfgpu.h says that the evenness of the coverage depends on this).
SC_HD int ms_orient_exact(const double P[2], const double Q[2], const double C[2]) {
    double v[6] = {P[0], P[1], Q[0], Q[1], C[0], C[1]};
    double big = 0.0;
    for (int i = 0; i < 6; ++i) big = sc_max(big, sc_abs(v[i]));
    if (!(big > 0.0)) return 0;
    int ex = 0;
    (void)frexp(big, &ex);
    for (int i = 0; i < 6; ++i) v[i] = ldexp(v[i], 500 - ex);
    const double a[6] = {v[0], -v[0], -v[4], -v[1], v[1], v[5]}, b[6] = {v[3], v[5], v[3], v[2], v[4], v[2]};
    double e[12];
    for (int i = 0; i < 12; ++i) e[i] = 0.0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        double term[2];
        ms_two_prod(a[t], b[t], term[1], term[0]);
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const int n = 2 * t + part;                                      // components so far
            double q = term[part];
#pragma unroll
            for (int i = 0; i < n; ++i) {
                double s, h;
                ms_two_sum(q, e[i], s, h);
                e[i] = h;
                q = s;
            }
            e[n] = q;
        }
    }
    for (int i = 11; i >= 0; --i)
        if (e[i] != 0.0) return e[i] > 0.0 ? 1 : -1;
    return 0;
}

// The exact sign of orient(P, Q, C), and its value in doubles.  The filter: three roundings per product and one of the difference
// keep the computed value within 4 * 2^-53 (|l| + |r|) (1 + O(2^-53)) of the exact one, so a magnitude above 2^-50 (|l| + |r|)
// carries the sign; a sum that is not finite or is below 2^-900 (where a product may have underflowed) goes to the exact path.
SC_HD int ms_orient(const double P[2], const double Q[2], const double C[2], double& det) {
    const double l = (P[0] - C[0]) * (Q[1] - C[1]), r = (P[1] - C[1]) * (Q[0] - C[0]);
    det = l - r;
    const double sum = sc_abs(l) + sc_abs(r);
    if (sum >= 0x1p-900 && sum <= 0x1p1000 && sc_abs(det) > 0x1p-50 * sum) return det > 0.0 ? 1 : -1;
    return ms_orient_exact(P, Q, C);
}

// one edge from P to Q at the column centre C: the sign under the top-left rule, and the value w in doubles
SC_HD int ms_edge(const double P[2], const double Q[2], const double C[2], double& w) {
    const bool swap = Q[0] < P[0] || (Q[0] == P[0] && Q[1] < P[1]);
    const double* a = swap ? Q : P;
    const double* b = swap ? P : Q;
    int s = ms_orient(a, b, C, w);
    if (s == 0) s = a[1] > b[1] ? 1 : a[1] < b[1] ? -1 : b[0] > a[0] ? 1 : 0;     // (b_x >= a_x in this order)
    if (swap) { s = -s; w = -w; }
    return s;
}

// does the triangle with grid vertices G[3] cover the column centre C, and at which z does the column cross it
SC_HD bool ms_crossing(const double G[3][3], const double C[2], double& zc) {
    double w[3];
    const int s0 = ms_edge(G[1], G[2], C, w[0]);
    const int s1 = ms_edge(G[2], G[0], C, w[1]);
    const int s2 = ms_edge(G[0], G[1], C, w[2]);
    if (!(s0 != 0 && s0 == s1 && s1 == s2)) return false;
    const double zmin = sc_min(sc_min(G[0][2], G[1][2]), G[2][2]), zmax = sc_max(sc_max(G[0][2], G[1][2]), G[2][2]);
    double z = ((w[0] * G[0][2] + w[1] * G[1][2]) + w[2] * G[2][2]) / ((w[0] + w[1]) + w[2]);
    z = z >= zmin ? z : zmin;
    zc = z <= zmax ? z : zmax;
    return true;
}

// the number of cells of a column whose centres are not above zc: the first cell above it, nz when there is none
SC_HD int64_t ms_first_above(double res, int64_t nz, double zc) {
    int64_t lo = 0, hi = nz;
    for (int step = 0; step < 64 && lo < hi; ++step) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (res * ((double)mid + 0.5) <= zc) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- culling (not part of the restatement) ---------------------------------------------------------------------------------------------
// The xy index box lo[k] .. hi[k] (inclusive, clipped; lo > hi: empty) of the columns whose centres lie within the triangle's
// bounding rectangle, one column further each way: a centre strictly outside that rectangle is covered under no tie rule.
SC_HD void ms_column_box(const MeshArgs& a, const double G[3][3], int64_t lo[2], int64_t hi[2]) {
    const int64_t dims[2] = {a.nx, a.ny};
    for (int k = 0; k < 2; ++k) {
        const double gmin = sc_min(sc_min(G[0][k], G[1][k]), G[2][k]), gmax = sc_max(sc_max(G[0][k], G[1][k]), G[2][k]);
        const double below = gmin / a.res - 1.5, above = gmax / a.res + 0.5, top = (double)(dims[k] - 1);
        lo[k] = 0; hi[k] = dims[k] - 1;
        if (!(below <= top) || !(above >= 0.0)) { lo[k] = 1; hi[k] = 0; continue; }       // (also for a NaN)
        if (below > 0.0) lo[k] = (int64_t)below;
        if (above < top) hi[k] = (int64_t)above + 1 < dims[k] - 1 ? (int64_t)above + 1 : dims[k] - 1;
    }
}

SC_HD int64_t ms_tiles(const int64_t lo[2], const int64_t hi[2], int64_t per[2]) {
    int64_t count = 1;
    for (int k = 0; k < 2; ++k) {
        per[k] = hi[k] < lo[k] ? 0 : (hi[k] - lo[k]) / kMsTile + 1;
        count *= per[k];
    }
    return count;
}

SC_HD bool ms_grid_triangle(const MeshArgs& a, const double* W, double G[3][3]) {
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
        ms_grid(a.inverse, a.origin, W + 3 * i, G[i]);
        ok = ok && sc_finite(G[i][0]) && sc_finite(G[i][1]) && sc_finite(G[i][2]);
    }
    return ok;
}

#if defined(__HIPCC__)
// the launches of sdfgpu_mesh.hip that the solid call shares, and its own (sdfgpu_mesh_solid.hip)
hipError_t mesh_launch_setup(const MeshArgs& a, hipStream_t s);
hipError_t mesh_launch_scan(const MeshArgs& a, hipStream_t s);
hipError_t mesh_launch_scatter(const MeshArgs& a, hipStream_t s);
hipError_t mesh_solid_launch(const SolidArgs& a, hipStream_t s);
#endif

}  // namespace sdfgpu
