// sdfgpu_query.hip -- the interpolated-gradient kernel (sdfgpu_query.hpp) and its launcher.  Compiled beside sdfgpu.hip and
// linked into the same libsdfgpu.so (sdf_tools_amd/build.py).
// The family's host orchestration and C ABI entry points (sdfgpu_query_gradients*) are at the end of this file, over the handle of
// sdfgpu_context.hpp.
//
// Arithmetic: every estimate, difference, derivative and displacement must round exactly as the host core
// (SignedDistanceField::QueryGradient4d) does -- separate products and sums in eigen_lite order, the AutoDiff3 operators of
// include/sdf_tools/autodiff.hpp, correctly rounded division -- so nothing in this file (nor in that header, included below) may
// be contracted into an FMA (hipcc contracts by default).
// The host code at the end of this file falls under the pragma too.  It is compiled for baseline x86-64, which has no FMA to
// contract into, so the pragma changes nothing there -- look again before giving the host pass a -march.
#pragma clang fp contract(off)
#define SDFGPU_AUX_TU
#include "sdfgpu_kernels.hpp"
#include "sdfgpu_context.hpp"
#include "sdfgpu_query.hpp"
#include "sdfgpu.h"
#include "sdf_tools/autodiff.hpp"

#include <cmath>

namespace sdfgpu {

namespace {

constexpr int kThreads = 256;
using sdf_tools::AutoDiff3;

// PointInFrameToGridIndex4d + IndexInBounds on the floored doubles (no int64 cast of a coordinate outside the grid)
__device__ __forceinline__ bool cell_of(const GradientQueryArgs& a, double q0, double q1, double q2, int64_t& x, int64_t& y, int64_t& z) {
    const double fx = floor(q0 * a.inv_res), fy = floor(q1 * a.inv_res), fz = floor(q2 * a.inv_res);
    if (!(fx >= 0.0 && fy >= 0.0 && fz >= 0.0 && fx < (double)a.nx && fy < (double)a.ny && fz < (double)a.nz)) return false;
    x = (int64_t)fx; y = (int64_t)fy; z = (int64_t)fz;
    return true;
}

// row-major 3x4 transform of (p0, p1, p2, 1): ((m0 p0 + m1 p1) + m2 p2) + m3 (m3 * 1.0 == m3 exactly)
__device__ __forceinline__ void transform(const double* m, double p0, double p1, double p2, double& r0, double& r1, double& r2) {
    r0 = m[0] * p0 + m[1] * p1 + m[2] * p2 + m[3];
    r1 = m[4] * p0 + m[5] * p1 + m[6] * p2 + m[7];
    r2 = m[8] * p0 + m[9] * p1 + m[10] * p2 + m[11];
}

// SignedDistanceField::EstimateFromNeighborsGridFrame, as k_query_points computes it; the cell (x, y, z) is inside the grid
__device__ __forceinline__ double estimate(const GradientQueryArgs& a, double q0, double q1, double q2, int64_t x, int64_t y, int64_t z) {
    const int64_t sx = a.ny * a.nz, sy = a.nz;
    const float* f = a.sdf;
    auto D = [&](int64_t xi, int64_t yi, int64_t zi) -> double {
        const double d = (double)f[xi * sx + yi * sy + zi];
        return d >= 0.0 ? d - a.half : d + a.half;
    };
    int64_t x0, x1, y0, y1, z0, z1;
    query_axis_pair(x, a.nx, q0 - a.res * ((double)x + 0.5), x0, x1);
    query_axis_pair(y, a.ny, q1 - a.res * ((double)y + 0.5), y0, y1);
    query_axis_pair(z, a.nz, q2 - a.res * ((double)z + 0.5), z0, z1);
    const double lx = a.res * ((double)x0 + 0.5), ly = a.res * ((double)y0 + 0.5), lz = a.res * ((double)z0 + 0.5);
    const double mz = query_bilinear(lx, lx + a.res, ly, ly + a.res, q0, q1, D(x0, y0, z0), D(x0, y1, z0), D(x1, y0, z0), D(x1, y1, z0));
    const double pz = query_bilinear(lx, lx + a.res, ly, ly + a.res, q0, q1, D(x0, y0, z1), D(x0, y1, z1), D(x1, y0, z1), D(x1, y1, z1));
    const double slope = (pz - mz) * (1.0 / a.res);
    return mz + ((q2 - lz) * slope);
}

// EstimateDistance(p) with the cell decided on the doubles: false (the reference's .second) outside the grid
__device__ __forceinline__ bool estimate_world(const GradientQueryArgs& a, double p0, double p1, double p2, double& d) {
    double q0, q1, q2;
    int64_t x, y, z;
    transform(a.w2g, p0, p1, p2, q0, q1, q2);
    if (!cell_of(a, q0, q1, q2, x, y, z)) return false;
    d = estimate(a, q0, q1, q2, x, y, z);
    return true;
}

// The same estimate over AutoDiff3 (autodiff.hpp's TrilinearT, the host core's template); the cell is chosen from the values
__device__ __forceinline__ AutoDiff3 estimate_ad(const GradientQueryArgs& a, const AutoDiff3& q0, const AutoDiff3& q1, const AutoDiff3& q2,
                                                 int64_t x, int64_t y, int64_t z) {
    const int64_t sx = a.ny * a.nz, sy = a.nz;
    const float* f = a.sdf;
    auto D = [&](int64_t xi, int64_t yi, int64_t zi) -> double {
        const double d = (double)f[xi * sx + yi * sy + zi];
        return d >= 0.0 ? d - a.half : d + a.half;
    };
    int64_t x0, x1, y0, y1, z0, z1;
    query_axis_pair(x, a.nx, q0.v - a.res * ((double)x + 0.5), x0, x1);
    query_axis_pair(y, a.ny, q1.v - a.res * ((double)y + 0.5), y0, y1);
    query_axis_pair(z, a.nz, q2.v - a.res * ((double)z + 0.5), z0, z1);
    const double lx = a.res * ((double)x0 + 0.5), ly = a.res * ((double)y0 + 0.5), lz = a.res * ((double)z0 + 0.5);
    return sdf_tools::TrilinearT<AutoDiff3>(lx, ly, lz, a.res, q0, q1, q2, D(x0, y0, z0), D(x0, y0, z1), D(x0, y1, z0), D(x0, y1, z1),
                                            D(x1, y0, z0), D(x1, y0, z1), D(x1, y1, z0), D(x1, y1, z1));
}

// std::min(a, b) as libstdc++ evaluates it
__device__ __forceinline__ double min_ref(double a, double b) { return (b < a) ? b : a; }

// One lane per point; KIND is fixed per instantiation, so no lane branches on the mode.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_query_gradients(const GradientQueryArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const double nan = __builtin_nan("");
    const double p0 = a.points[3 * i], p1 = a.points[3 * i + 1], p2 = a.points[3 * i + 2];
    double v = nan, g0 = nan, g1 = nan, g2 = nan;
    uint8_t st = SDFGPU_QUERY_OK;
    if constexpr (KIND == SDFGPU_QUERY_DISTANCE_TO_BOUNDARY) {
        double q0, q1, q2;
        transform(a.w2g, p0, p1, p2, q0, q1, q2);
        const double d0 = min_ref(q0, a.size[0] - q0), d1 = min_ref(q1, a.size[1] - q1), d2 = min_ref(q2, a.size[2] - q2);
        st = (d0 >= 0.0 && d1 >= 0.0 && d2 >= 0.0) ? SDFGPU_QUERY_OK : SDFGPU_QUERY_OUTSIDE;
        double least = fabs(d0);
        v = d0;
        if (fabs(d1) < least) { least = fabs(d1); v = d1; }
        if (fabs(d2) < least) { v = d2; }
    } else if (!isfinite(p0) || !isfinite(p1) || !isfinite(p2)) {
        st = SDFGPU_QUERY_NON_FINITE;
    } else {
        int64_t x = 0, y = 0, z = 0;
        double q0, q1, q2;
        transform(a.w2g, p0, p1, p2, q0, q1, q2);
        if (!cell_of(a, q0, q1, q2, x, y, z)) {
            st = SDFGPU_QUERY_OUTSIDE;
            v = a.oob;
        } else if constexpr (KIND == SDFGPU_QUERY_AUTODIFF_GRADIENT) {
            // (x, y, z, 1) seeded with Unit(0..2) through W; the values repeat transform() above bit for bit
            const AutoDiff3 s0 = AutoDiff3::Seed(p0, 0), s1 = AutoDiff3::Seed(p1, 1), s2 = AutoDiff3::Seed(p2, 2);
            const AutoDiff3 r0 = sdf_tools::TransformRowT(a.w2g, s0, s1, s2);
            const AutoDiff3 r1 = sdf_tools::TransformRowT(a.w2g + 4, s0, s1, s2);
            const AutoDiff3 r2 = sdf_tools::TransformRowT(a.w2g + 8, s0, s1, s2);
            const AutoDiff3 d = estimate_ad(a, r0, r1, r2, x, y, z);
            v = d.v; g0 = d.d[0]; g1 = d.d[1]; g2 = d.d[2];
        } else {
            // ComputeAxisSmoothGradient per axis; the query point itself is inside the grid here
            v = estimate(a, q0, q1, q2, x, y, z);
            const double w = a.window;
            double g[3];
            const double p[3] = {p0, p1, p2};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double lo = p[k] - w, hi = p[k] + w;
                double dm = 0.0, dp = 0.0;
                const bool am = estimate_world(a, k == 0 ? lo : p0, k == 1 ? lo : p1, k == 2 ? lo : p2, dm);
                const bool ap = estimate_world(a, k == 0 ? hi : p0, k == 1 ? hi : p1, k == 2 ? hi : p2, dp);
                if (am && ap) g[k] = (dp - dm) / (hi - lo);
                else if (am) g[k] = (v - dm) / (p[k] - lo);
                else if (ap) g[k] = (dp - v) / (hi - p[k]);
                else { st = SDFGPU_QUERY_WINDOW_TOO_LARGE; g[k] = nan; }
            }
            if (st == SDFGPU_QUERY_OK) { g0 = g[0]; g1 = g[1]; g2 = g[2]; }
        }
    }
    if (a.value) a.value[i] = v;
    if (a.gradient) { a.gradient[3 * i] = g0; a.gradient[3 * i + 1] = g1; a.gradient[3 * i + 2] = g2; }
    if (a.status) a.status[i] = st;
}

}  // namespace

void query_gradients_prepare(GradientQueryArgs& a, double resolution, double window, float oob_value) {
    // the expressions of SignedDistanceField (VoxelGrid's inv_cell_x_size_ = 1.0 / cx, x_size_ = nx * cx, CorrectedCenterDistance)
    a.res = resolution;
    a.inv_res = 1.0 / resolution;
    a.half = resolution * 0.5;
    a.window = std::fabs(window);
    a.oob = (double)oob_value;
    a.size[0] = (double)a.nx * resolution;
    a.size[1] = (double)a.ny * resolution;
    a.size[2] = (double)a.nz * resolution;
}

hipError_t query_gradients_launch(const GradientQueryArgs& a, hipStream_t s) {
    const int64_t blocks = (a.n + kThreads - 1) / kThreads;
    if (a.kind == SDFGPU_QUERY_SMOOTH_GRADIENT)
        hipLaunchKernelGGL(k_query_gradients<SDFGPU_QUERY_SMOOTH_GRADIENT>, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
    else if (a.kind == SDFGPU_QUERY_AUTODIFF_GRADIENT)
        hipLaunchKernelGGL(k_query_gradients<SDFGPU_QUERY_AUTODIFF_GRADIENT>, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL(k_query_gradients<SDFGPU_QUERY_DISTANCE_TO_BOUNDARY>, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

int check_query_gradients_args(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                               const double* world_to_grid, int kind, double window, const double* points, int64_t n_points,
                               GradientQueryArgs& a) {
    if (!d_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "gradient query: null field pointer");
    if (n_points < 0 || n_points > ((int64_t)1 << 40)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "gradient query: point count %lld out of range [0, 2^40]", (long long)n_points);
    if (n_points > 0 && !points) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "gradient query: null points");
    if (!world_to_grid) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "gradient query: world_to_grid is required");
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx > INT64_MAX / ny || nx * ny > INT64_MAX / nz)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "gradient query: unsupported grid %lld x %lld x %lld", (long long)nx, (long long)ny, (long long)nz);
    if (!(resolution > 0.0) || !std::isfinite(resolution)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "gradient query: resolution must be positive and finite");
    if (kind != SDFGPU_QUERY_SMOOTH_GRADIENT && kind != SDFGPU_QUERY_AUTODIFF_GRADIENT && kind != SDFGPU_QUERY_DISTANCE_TO_BOUNDARY)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "gradient query: unknown kind %d", kind);
    if (!std::isfinite(window)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "gradient query: the window must be finite");
    a = GradientQueryArgs{};
    a.sdf = d_sdf; a.n = n_points; a.nx = nx; a.ny = ny; a.nz = nz; a.kind = kind;
    for (int i = 0; i < 12; ++i) a.w2g[i] = world_to_grid[i];
    return SDFGPU_OK;
}

}  // namespace

extern "C" {

int sdfgpu_query_gradients_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                  const double world_to_grid[12], float oob_value, int kind, double window, const double* d_points,
                                  int64_t n_points, double* d_value, double* d_gradient, uint8_t* d_status, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        GradientQueryArgs a;
        if (int rc = check_query_gradients_args(h, d_sdf, nx, ny, nz, resolution, world_to_grid, kind, window, d_points, n_points, a)) return rc;
        if (n_points == 0 || (!d_value && !d_gradient && !d_status)) return SDFGPU_OK;
        HIP_TRY(h, hipSetDevice(h->device));
        a.points = d_points; a.value = d_value; a.gradient = d_gradient; a.status = d_status;
        query_gradients_prepare(a, resolution, window, oob_value);
        HIP_TRY(h, query_gradients_launch(a, (hipStream_t)stream));
        return SDFGPU_OK;
    });
}

int sdfgpu_query_gradients(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                           const double world_to_grid[12], float oob_value, int kind, double window, const double* points,
                           int64_t n_points, double* out_value, double* out_gradient, uint8_t* out_status) {
    return rz_wrap(h, nullptr, [&]() -> int {
        GradientQueryArgs a;
        if (int rc = check_query_gradients_args(h, d_sdf, nx, ny, nz, resolution, world_to_grid, kind, window, points, n_points, a)) return rc;
        if (n_points == 0 || (!out_value && !out_gradient && !out_status)) return SDFGPU_OK;
        HIP_TRY(h, hipSetDevice(h->device));
        // points | gradient | value | status
        return with_staged_points(h, points, n_points, {24, 8, 1}, {out_gradient, out_value, out_status}, [&](const double* d_points, char* const (&d)[3]) -> int {
            a.points = d_points; a.gradient = (double*)d[0]; a.value = (double*)d[1]; a.status = (uint8_t*)d[2];
            query_gradients_prepare(a, resolution, window, oob_value);
            HIP_TRY(h, query_gradients_launch(a, nullptr));
            return SDFGPU_OK;
        });
    });
}

}  // extern "C"
