// sdfgpu_scene.hpp -- rasterising planning-scene shapes (boxes, spheres, cylinders with poses) into occupancy: the decision
// procedure of include/sdfgpu.h "Shape rasteriser" (DESIGN.md section 26), the arguments of its kernels and the layout of its
// scratch.  The procedure is plain C++ (SC_HD functions of doubles), so that tests/scene_predicate_host.cpp runs the very same
// text on the CPU against the numpy restatement (tests/scene_raster_restated.py); the kernels are in sdfgpu_scene.hip.
//
// Arithmetic: doubles, separate products and sums in the order written, no FMA: every unit that includes this header must
// compile it under `#pragma clang fp contract(off)` (or -ffp-contract=off).
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "sdfgpu.h"

#if defined(__HIPCC__)
#define SC_HD __host__ __device__ __forceinline__
#else
#define SC_HD inline
#endif

namespace sdfgpu {

constexpr int kScThreads = 256;                    // voxels of a fine region: one workgroup, four waves of two bit words each
constexpr int64_t kScMaxShapes = 65536;            // SDFGPU_MAX_SHAPES
constexpr int64_t kScMaxCoarse = 4096;             // coarse regions of a call, at most
constexpr int64_t kScGridX = 1 << 20;              // workgroups per grid row (a launch dimension stays far below 2^32 threads)
constexpr size_t kScStatusBytes = 256;

// Voxels per coarse region: a multiple of the fine region, at least 16 of them, and few enough regions that the candidate bits
// (one per coarse region and shape) stay small: kScMaxCoarse * kScMaxShapes / 8 = 32 MiB at the most.
inline int64_t scene_coarse_voxels(int64_t n) {
    const int64_t per = (n + kScMaxCoarse - 1) / kScMaxCoarse;
    const int64_t fine = (per + kScThreads - 1) / kScThreads;
    return (fine < 16 ? 16 : fine) * kScThreads;
}
inline int64_t scene_coarse_count(int64_t n) { const int64_t c = scene_coarse_voxels(n); return (n + c - 1) / c; }
inline int64_t scene_shape_words(int64_t n_shapes) { return (n_shapes + 31) / 32; }
// scratch: status block | 6 doubles of world bounds per shape | candidate words [coarse][shape words]
inline size_t scene_bounds_offset() { return kScStatusBytes; }
inline size_t scene_cand_offset(int64_t n_shapes) { return kScStatusBytes + (((size_t)n_shapes * 48 + 255) & ~(size_t)255); }
inline size_t scene_scratch_bytes(int64_t n, int64_t n_shapes) {
    return scene_cand_offset(n_shapes) + (size_t)scene_coarse_count(n) * (size_t)scene_shape_words(n_shapes) * 4;
}

struct SceneArgs {
    const sdfgpu_shape* shapes;
    int64_t n_shapes, n_words;
    double origin[12];
    double res, half;                  // half = res * 0.5, the probe cube's half side
    int64_t nx, ny, nz, n;
    int64_t coarse_voxels, n_coarse;
    uint32_t* status;                  // [0]: 0, or 1 + the index of the first shape that was refused
    double* bounds;                    // [n_shapes][6]: lo x y z, hi x y z of the shape in the world, inflated by res
    uint32_t* cand;                    // [n_coarse][n_words]
    uint32_t* bits;
    uint8_t* mask;
    uint32_t* ids;
};

// ---- the decision procedure ----------------------------------------------------------------------------------------------------------
SC_HD double sc_abs(double v) { return v < 0.0 ? -v : v; }
SC_HD double sc_min(double a, double b) { return b < a ? b : a; }
SC_HD double sc_max(double a, double b) { return b > a ? b : a; }
SC_HD bool sc_finite(double v) { return v - v == 0.0; }

// the centre of voxel (x, y, z): origin * (res (x + 0.5), res (y + 0.5), res (z + 0.5), 1), rows as ((m0 v0 + m1 v1) + m2 v2) + m3
SC_HD void sc_centre(const double* o, double res, int64_t x, int64_t y, int64_t z, double c[3]) {
    const double g0 = res * ((double)x + 0.5), g1 = res * ((double)y + 0.5), g2 = res * ((double)z + 0.5);
    for (int r = 0; r < 3; ++r) c[r] = o[4 * r] * g0 + o[4 * r + 1] * g1 + o[4 * r + 2] * g2 + o[4 * r + 3];
}

// type known, dims finite and >= 0 (those the type uses), the 12 used pose entries finite; a plane's dims are its normal: finite,
// of either sign, not all zero
SC_HD bool sc_shape_valid(const sdfgpu_shape& s) {
    if (s.type == SDFGPU_SHAPE_PLANE) {
        for (int i = 0; i < 3; ++i) if (!sc_finite(s.dims[i])) return false;
        if (s.dims[0] == 0.0 && s.dims[1] == 0.0 && s.dims[2] == 0.0) return false;
        for (int i = 0; i < 12; ++i) if (!sc_finite(s.pose[i])) return false;
        return true;
    }
    const int nd = s.type == SDFGPU_SHAPE_BOX ? 3 : s.type == SDFGPU_SHAPE_SPHERE ? 1 : s.type == SDFGPU_SHAPE_CYLINDER ? 2 : -1;
    if (nd < 0) return false;
    for (int i = 0; i < nd; ++i) if (!(sc_finite(s.dims[i]) && s.dims[i] >= 0.0)) return false;
    for (int i = 0; i < 12; ++i) if (!sc_finite(s.pose[i])) return false;
    return true;
}

// Half extents of the shape's world bounds about its translation, per world axis: the box's own, a sphere's radius, a cylinder as
// the box 2r x 2r x height around it.
SC_HD void sc_half_extents(const sdfgpu_shape& s, double e[3]) {
    const double* p = s.pose;
    if (s.type == SDFGPU_SHAPE_SPHERE) { e[0] = e[1] = e[2] = s.dims[0]; return; }
    double d0, d1, d2;
    if (s.type == SDFGPU_SHAPE_BOX) { d0 = s.dims[0] * 0.5; d1 = s.dims[1] * 0.5; d2 = s.dims[2] * 0.5; }
    else { d0 = d1 = s.dims[1]; d2 = s.dims[0] * 0.5; }
    for (int a = 0; a < 3; ++a) e[a] = sc_abs(p[4 * a]) * d0 + sc_abs(p[4 * a + 1]) * d1 + sc_abs(p[4 * a + 2]) * d2;
}

// SPHERE: the squared distance from the sphere's centre to the cube against r^2
SC_HD bool sc_sphere(const sdfgpu_shape& s, const double c[3], double h) {
    double sum = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double d = sc_max(sc_abs(c[a] - s.pose[4 * a + 3]) - h, 0.0);
        sum = sum + d * d;
    }
    return sum <= s.dims[0] * s.dims[0];
}

// BOX: the 15 separating axes of the cube (half side h, world axes) and the box (half extents b along the pose's columns), with the
// pose's rotation block taken as orthonormal.  Closed: an axis separates only when |t . L| > r_cube + r_box, so a cross axis that
// degenerates to L = 0 (0 > 0) never does.
SC_HD bool sc_box(const sdfgpu_shape& s, const double c[3], double h) {
    const double* p = s.pose;
    const double b[3] = {s.dims[0] * 0.5, s.dims[1] * 0.5, s.dims[2] * 0.5};
    double t[3], R[3][3], A[3][3];
    for (int a = 0; a < 3; ++a) {
        t[a] = p[4 * a + 3] - c[a];
        for (int j = 0; j < 3; ++j) { R[a][j] = p[4 * a + j]; A[a][j] = sc_abs(R[a][j]); }
    }
    // the cube's axes
    for (int a = 0; a < 3; ++a)
        if (sc_abs(t[a]) > h + ((b[0] * A[a][0] + b[1] * A[a][1]) + b[2] * A[a][2])) return false;
    // the box's axes
    for (int j = 0; j < 3; ++j) {
        const double tl = (t[0] * R[0][j] + t[1] * R[1][j]) + t[2] * R[2][j];
        if (sc_abs(tl) > h * ((A[0][j] + A[1][j]) + A[2][j]) + b[j]) return false;
    }
    // e_a x u_j, with a1 = a + 1, a2 = a + 2 and j1 = j + 1, j2 = j + 2 (mod 3)
    for (int a = 0; a < 3; ++a) {
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            const double tl = t[a2] * R[a1][j] - t[a1] * R[a2][j];
            const double rc = h * (A[a2][j] + A[a1][j]);
            const double rb = b[j1] * A[a][j2] + b[j2] * A[a][j1];
            if (sc_abs(tl) > rc + rb) return false;
        }
    }
    return true;
}

// the squared distance from the origin to the segment a -> b in the plane
SC_HD double sc_segment_dsq(double ax, double ay, double bx, double by) {
    const double ex = bx - ax, ey = by - ay;
    const double ee = ex * ex + ey * ey;
    double t = 0.0;
    if (ee > 0.0) t = sc_min(sc_max(-(ax * ex + ay * ey) / ee, 0.0), 1.0);
    const double qx = ax + t * ex, qy = ay + t * ey;
    return qx * qx + qy * qy;
}

// One Sutherland-Hodgman pass: keep sign * z <= bound (sign = +1: z <= bound, sign = -1: z >= -bound).  A cut point takes the
// plane's z exactly.  Returns the number of vertices written to `out` (at most n + 1).
SC_HD int sc_clip(const double (*in)[3], int n, double sign, double bound, double (*out)[3]) {
    int m = 0;
    const double plane = sign * bound;
    for (int k = 0; k < n; ++k) {
        const double* cur = in[k];
        const double* prv = in[k == 0 ? n - 1 : k - 1];
        const bool cin = sign * cur[2] <= bound, pin = sign * prv[2] <= bound;
        if (cin != pin) {
            const double u = (plane - prv[2]) / (cur[2] - prv[2]);
            out[m][0] = prv[0] + u * (cur[0] - prv[0]);
            out[m][1] = prv[1] + u * (cur[1] - prv[1]);
            out[m][2] = plane;
            ++m;
        }
        if (cin) { out[m][0] = cur[0]; out[m][1] = cur[1]; out[m][2] = cur[2]; ++m; }
    }
    return m;
}

// CYLINDER (height H along the pose's z column, radius r), the rotation block taken as orthonormal.
//   q = R^T (c - T), the centre in the shape frame; rho2 = qx^2 + qy^2; hz = H / 2.
//   1. reject when |qz| - hz > 1.75 h or rho2 > (r + 1.75 h)^2   (1.75 h > sqrt(3) h, the probe's circum-radius)
//   2. accept when |qz| <= hz and rho2 <= r^2                    (the centre is in the solid)
//   3. the eight corners c + (+-h, +-h, +-h) in the shape frame; each of the six faces clipped to |z| <= hz (two passes); the
//      minimum over the clipped faces' edges of the squared distance from the axis to the edge's xy projection; accept when it is <= r^2
//   4. accept when the axis segment T -+ hz u_z passes through the cube (slab test in the world's axes), else reject
SC_HD bool sc_cylinder(const sdfgpu_shape& s, const double c[3], double h) {
    const double* p = s.pose;
    const double hz = s.dims[0] * 0.5, r = s.dims[1];
    const double r2 = r * r;
    double d[3], q[3];
    for (int a = 0; a < 3; ++a) d[a] = c[a] - p[4 * a + 3];
    for (int j = 0; j < 3; ++j) q[j] = (p[j] * d[0] + p[4 + j] * d[1]) + p[8 + j] * d[2];
    const double rho2 = q[0] * q[0] + q[1] * q[1];
    const double reach = 1.75 * h, rr = r + reach;
    if (sc_abs(q[2]) - hz > reach || rho2 > rr * rr) return false;
    if (sc_abs(q[2]) <= hz && rho2 <= r2) return true;
    // corner k: bit a of k set = +h along world axis a
    double v[8][3];
    for (int k = 0; k < 8; ++k) {
        double w[3];
        for (int a = 0; a < 3; ++a) w[a] = (c[a] + ((k >> a) & 1 ? h : -h)) - p[4 * a + 3];
        for (int j = 0; j < 3; ++j) v[k][j] = (p[j] * w[0] + p[4 + j] * w[1]) + p[8 + j] * w[2];
    }
    double best = 1.0e300;
    for (int f = 0; f < 6; ++f) {
        // face f: axis a = f / 2 fixed at side f & 1; its corners in cyclic order over the other two axes
        const int a = f >> 1, a1 = (a + 1) % 3, a2 = (a + 2) % 3, base = (f & 1) << a;
        const int corner[4] = {base, base | (1 << a1), base | (1 << a1) | (1 << a2), base | (1 << a2)};
        double quad[4][3], one[5][3], two[6][3];
        for (int k = 0; k < 4; ++k) for (int j = 0; j < 3; ++j) quad[k][j] = v[corner[k]][j];
        const int n1 = sc_clip(quad, 4, -1.0, hz, one);
        const int n2 = sc_clip(one, n1, 1.0, hz, two);
        for (int k = 0; k < n2; ++k) {
            const int l = k == 0 ? n2 - 1 : k - 1;
            best = sc_min(best, sc_segment_dsq(two[l][0], two[l][1], two[k][0], two[k][1]));
        }
    }
    if (best <= r2) return true;
    // the axis segment P(s) = T + s hz u_z, s in [-1, 1], against |P_a - c_a| <= h
    double lo = -1.0, hi = 1.0;
    for (int a = 0; a < 3; ++a) {
        const double g = hz * p[4 * a + 2];
        if (g == 0.0) {
            if (sc_abs(d[a]) > h) return false;
        } else {
            const double s1 = (d[a] - h) / g, s2 = (d[a] + h) / g;
            lo = sc_max(lo, sc_min(s1, s2));
            hi = sc_min(hi, sc_max(s1, s2));
        }
    }
    return lo <= hi;
}

// PLANE (through the shape frame's origin, normal dims[0..2] in the shape frame; infinite, no thickness): N = R n, s = N . (c - T),
// filled iff |s| <= h (|N_0| + |N_1| + |N_2|).  It belongs to the shape list, so it lives here; sdfgpu_mesh.hpp states it beside
// the triangle's axes.
SC_HD bool sc_plane(const sdfgpu_shape& s, const double c[3], double h) {
    const double* p = s.pose;
    double N[3];
    for (int a = 0; a < 3; ++a) N[a] = (p[4 * a] * s.dims[0] + p[4 * a + 1] * s.dims[1]) + p[4 * a + 2] * s.dims[2];
    const double d = (N[0] * (c[0] - p[3]) + N[1] * (c[1] - p[7])) + N[2] * (c[2] - p[11]);
    return sc_abs(d) <= h * ((sc_abs(N[0]) + sc_abs(N[1])) + sc_abs(N[2]));
}

// a valid shape against the probe cube of half side h about c
SC_HD bool sc_hit(const sdfgpu_shape& s, const double c[3], double h) {
    if (s.type == SDFGPU_SHAPE_PLANE) return sc_plane(s, c, h);
    if (s.type == SDFGPU_SHAPE_SPHERE) return sc_sphere(s, c, h);
    if (s.type == SDFGPU_SHAPE_BOX) return sc_box(s, c, h);
    return sc_cylinder(s, c, h);
}

}  // namespace sdfgpu
