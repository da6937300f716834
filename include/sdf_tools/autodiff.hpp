// autodiff.hpp -- AutoDiff3, a forward-mode dual number (a value and the derivatives with respect to the three world-frame
// coordinates) for SignedDistanceField::GetAutoDiffGradient*, in place of the reference's Eigen::AutoDiffScalar<Vector4d>
// (reference include/sdf_tools/sdf.hpp:600-653).  The reference's 4th (homogeneous) derivative component never feeds the
// first three, so it is left out.
//
// The operators follow Eigen::AutoDiffScalar's literally, zero terms included (a zero derivative times an infinite value is
// NaN, as in Eigen):
//   AD * AD        value a * b, derivatives (a.d * b) + (b.d * a)
//   double * AD    derivatives b.d * a (and AD * double alike)
//   AD +- AD       derivatives a.d +- b.d;  AD - double keeps a.d;  double - AD gives -b.d
//   AD(double)     zero derivatives
// The same header is compiled by the host compiler (include/sdf_tools/sdf.hpp) and by hipcc (sdf_tools_amd/csrc/
// sdfgpu_query.hip); neither build may contract a product and a sum into an FMA.
#pragma once

#if defined(__HIPCC__)
#define SDF_TOOLS_HD __host__ __device__ __forceinline__
#else
#define SDF_TOOLS_HD inline
#endif

namespace sdf_tools {

struct AutoDiff3 {
    double v;
    double d[3];

    SDF_TOOLS_HD AutoDiff3() : v(0.0), d{0.0, 0.0, 0.0} {}
    SDF_TOOLS_HD AutoDiff3(const double value) : v(value), d{0.0, 0.0, 0.0} {}       // NOLINT: implicit, like Eigen's
    SDF_TOOLS_HD AutoDiff3(const double value, const double d0, const double d1, const double d2) : v(value), d{d0, d1, d2} {}
    // the seed of coordinate `axis` (0, 1, 2): derivative Unit(axis)
    SDF_TOOLS_HD static AutoDiff3 Seed(const double value, const int axis) {
        return AutoDiff3(value, axis == 0 ? 1.0 : 0.0, axis == 1 ? 1.0 : 0.0, axis == 2 ? 1.0 : 0.0);
    }
};

SDF_TOOLS_HD AutoDiff3 operator*(const AutoDiff3& a, const AutoDiff3& b) {
    return AutoDiff3(a.v * b.v, (a.d[0] * b.v) + (b.d[0] * a.v), (a.d[1] * b.v) + (b.d[1] * a.v), (a.d[2] * b.v) + (b.d[2] * a.v));
}
SDF_TOOLS_HD AutoDiff3 operator*(const double a, const AutoDiff3& b) {
    return AutoDiff3(a * b.v, b.d[0] * a, b.d[1] * a, b.d[2] * a);
}
SDF_TOOLS_HD AutoDiff3 operator*(const AutoDiff3& a, const double b) {
    return AutoDiff3(a.v * b, a.d[0] * b, a.d[1] * b, a.d[2] * b);
}
SDF_TOOLS_HD AutoDiff3 operator+(const AutoDiff3& a, const AutoDiff3& b) {
    return AutoDiff3(a.v + b.v, a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2]);
}
SDF_TOOLS_HD AutoDiff3 operator-(const AutoDiff3& a, const AutoDiff3& b) {
    return AutoDiff3(a.v - b.v, a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2]);
}
SDF_TOOLS_HD AutoDiff3 operator-(const AutoDiff3& a, const double b) { return AutoDiff3(a.v - b, a.d[0], a.d[1], a.d[2]); }
SDF_TOOLS_HD AutoDiff3 operator-(const double a, const AutoDiff3& b) { return AutoDiff3(a - b.v, -b.d[0], -b.d[1], -b.d[2]); }

SDF_TOOLS_HD double ValueOf(const double x) { return x; }
SDF_TOOLS_HD double ValueOf(const AutoDiff3& x) { return x.v; }

// The reference's trilinear estimate (TrilinearInterpolateDistance and BilinearInterpolate, :699-771, with the corrected
// centre distances of EstimateDistanceInterpolateFromNeighborsGridFrame, :836-915) as a template over T = double or AutoDiff3,
// in the evaluation order the host and the GPU share: ((multiplier * d1_offsets) * values) * d2_offsets, left-to-right sums.
// multiplier and values are T (full product rule for AutoDiff3), inv_resolution is a double.
template <typename T>
SDF_TOOLS_HD T BilinearT(const double l1, const double h1, const double l2, const double h2, const T& q1, const T& q2, const double ll,
                         const double lh, const double hl, const double hh) {
    const T multiplier = T(1.0 / ((h1 - l1) * (h2 - l2)));
    const T a0 = multiplier * (h1 - q1), a1 = multiplier * (q1 - l1);
    const T r0 = a0 * T(ll) + a1 * T(hl), r1 = a0 * T(lh) + a1 * T(hh);
    return r0 * (h2 - q2) + r1 * (q2 - l2);
}

// lo = the lower corner's grid-frame location; the eight distances are the corrected centre distances, [x][y][z] lower/upper
template <typename T>
SDF_TOOLS_HD T TrilinearT(const double lo0, const double lo1, const double lo2, const double res, const T& q0, const T& q1, const T& q2,
                          const double mxmymz, const double mxmypz, const double mxpymz, const double mxpypz, const double pxmymz,
                          const double pxmypz, const double pxpymz, const double pxpypz) {
    const T mz = BilinearT(lo0, lo0 + res, lo1, lo1 + res, q0, q1, mxmymz, mxpymz, pxmymz, pxpymz);
    const T pz = BilinearT(lo0, lo0 + res, lo1, lo1 + res, q0, q1, mxmypz, mxpypz, pxmypz, pxpypz);
    const double inv_resolution = 1.0 / res;
    const T slope = (pz - mz) * inv_resolution;
    const T query_z_delta = q2 - T(lo2);
    return mz + (query_z_delta * slope);
}

// Row r of a row-major 3x4 world -> grid transform applied to (p0, p1, p2, 1) in eigen_lite's order, ((m0 p0 + m1 p1) + m2 p2)
// + m3 p3, where p3 is the constant 1 (an AutoDiff3 with zero derivatives).
template <typename T>
SDF_TOOLS_HD T TransformRowT(const double* m, const T& p0, const T& p1, const T& p2) {
    const T p3 = T(1.0);
    return m[0] * p0 + m[1] * p1 + m[2] * p2 + m[3] * p3;
}

}  // namespace sdf_tools
