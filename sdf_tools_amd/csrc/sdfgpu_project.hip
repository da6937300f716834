// sdfgpu_project.hip -- the projection kernel (sdfgpu_project.hpp) and its launcher.  Compiled beside sdfgpu.hip and linked into
// the same libsdfgpu.so (sdf_tools_amd/build.py).
// The family's host orchestration and C ABI entry points (sdfgpu_project_*) are at the end of this file, over the handle of
// sdfgpu_context.hpp.
//
// Arithmetic: every location, distance and step must round exactly as the host walk does (separate products and sums in
// eigen_lite order, correctly rounded division and square root), so nothing in this file may be contracted into an FMA (hipcc
// contracts by default).
// The host code at the end of this file falls under the pragma too.  It is compiled for baseline x86-64, which has no FMA to
// contract into, so the pragma changes nothing there -- look again before giving the host pass a -march.
#pragma clang fp contract(off)
#define SDFGPU_AUX_TU
#include "sdfgpu_kernels.hpp"
#include "sdfgpu_context.hpp"
#include "sdfgpu_project.hpp"
#include "sdfgpu.h"

#include <cmath>

namespace sdfgpu {

namespace {

constexpr int kThreads = 256;

// PointInFrameToGridIndex4d + IndexInBounds on the floored doubles (no int64 cast of a coordinate outside the grid)
__device__ __forceinline__ bool cell_of(const ProjectArgs& a, double q0, double q1, double q2, int64_t& x, int64_t& y, int64_t& z) {
    const double fx = floor(q0 * a.inv_res), fy = floor(q1 * a.inv_res), fz = floor(q2 * a.inv_res);
    if (!(fx >= 0.0 && fy >= 0.0 && fz >= 0.0 && fx < (double)a.nx && fy < (double)a.ny && fz < (double)a.nz)) return false;
    x = (int64_t)fx; y = (int64_t)fy; z = (int64_t)fz;
    return true;
}

// SignedDistanceField::EstimateFromNeighborsGridFrame, as k_query_points computes it; the cell (x, y, z) is inside the grid
__device__ __forceinline__ double estimate(const ProjectArgs& a, double q0, double q1, double q2, int64_t x, int64_t y, int64_t z) {
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

// GetGridAlignedGradient(x, y, z, enable_edge_gradients = true) of a cell inside the grid
__device__ __forceinline__ void gradient(const ProjectArgs& a, int64_t x, int64_t y, int64_t z, double& g0, double& g1, double& g2) {
    const int64_t sx = a.ny * a.nz, sy = a.nz;
    const int64_t i = x * sx + y * sy + z;
    const float* f = a.sdf;
    if (x > 0 && y > 0 && z > 0 && x < a.nx - 1 && y < a.ny - 1 && z < a.nz - 1) {
        g0 = (double)(f[i + sx] - f[i - sx]) * a.inv2;          // float subtraction, double scale
        g1 = (double)(f[i + sy] - f[i - sy]) * a.inv2;
        g2 = (double)(f[i + 1] - f[i - 1]) * a.inv2;
        return;
    }
    const int64_t lx = max((int64_t)0, x - 1), hx = min(a.nx - 1, x + 1);
    const int64_t ly = max((int64_t)0, y - 1), hy = min(a.ny - 1, y + 1);
    const int64_t lz = max((int64_t)0, z - 1), hz = min(a.nz - 1, z + 1);
    const double ix = (double)(hx - lx) * a.res, iy = (double)(hy - ly) * a.res, iz = (double)(hz - lz) * a.res;
    g0 = g1 = g2 = 0.0;
    if (ix > 0.0) g0 = ((double)f[i + (hx - x) * sx] - (double)f[i - (x - lx) * sx]) * (1.0 / ix);
    if (iy > 0.0) g1 = ((double)f[i + (hy - y) * sy] - (double)f[i - (y - ly) * sy]) * (1.0 / iy);
    if (iz > 0.0) g2 = ((double)f[i + (hz - z)] - (double)f[i - (z - lz)]) * (1.0 / iz);
}

// row-major 3x4 transform of (p0, p1, p2, 1): ((m0 p0 + m1 p1) + m2 p2) + m3 (m3 * 1.0 == m3 exactly)
__device__ __forceinline__ void transform(const double* m, double p0, double p1, double p2, double& r0, double& r1, double& r2) {
    r0 = m[0] * p0 + m[1] * p1 + m[2] * p2 + m[3];
    r1 = m[4] * p0 + m[5] * p1 + m[6] * p2 + m[7];
    r2 = m[8] * p0 + m[9] * p1 + m[10] * p2 + m[11];
}

// std::min(hi, std::max(lo, v)) as libstdc++ evaluates it
__device__ __forceinline__ double clamp_ref(double v, double lo, double hi) {
    const double m = (lo < v) ? v : lo;
    return (m < hi) ? m : hi;
}

// One point's walk: the state a lane carries between steps.
struct Walk {
    double q0, q1, q2;                 // grid frame (or the world-frame answer once `done` is set by start())
    int64_t x, y, z;
    double d;
    int32_t steps;
    uint8_t status;
    bool done;
    bool world;                        // q holds the world-frame answer already (no final transform)

    // Step 1 (or the whole valid-volume call), step 2 and the first estimate.
    __device__ __forceinline__ void start(const ProjectArgs& a, int64_t i) {
        const double p0 = a.points[3 * i], p1 = a.points[3 * i + 1], p2 = a.points[3 * i + 2];
        steps = 0;
        status = SDFGPU_PROJECT_CONVERGED;
        done = true;
        world = true;
        q0 = p0; q1 = p1; q2 = p2;
        if (!isfinite(p0) || !isfinite(p1) || !isfinite(p2)) { status = SDFGPU_PROJECT_NON_FINITE; return; }
        double g0, g1, g2;
        transform(a.w2g, p0, p1, p2, g0, g1, g2);
        const bool clamp = a.mode == SDFGPU_PROJECT_INTO_VALID_VOLUME || !cell_of(a, g0, g1, g2, x, y, z);
        if (clamp) {
            const double c0 = clamp_ref(g0, a.clamp_m, a.size[0] - a.clamp_m);
            const double c1 = clamp_ref(g1, a.clamp_m, a.size[1] - a.clamp_m);
            const double c2 = clamp_ref(g2, a.clamp_m, a.size[2] - a.clamp_m);
            if (c0 != g0 || c1 != g1 || c2 != g2) {
                transform(a.g2w, c0, c1, c2, q0, q1, q2);
                if (a.mode != SDFGPU_PROJECT_INTO_VALID_VOLUME) transform(a.w2g, q0, q1, q2, g0, g1, g2);
            }
            if (a.mode == SDFGPU_PROJECT_INTO_VALID_VOLUME) return;
        }
        world = false;
        q0 = g0; q1 = g1; q2 = g2;
        if (!cell_of(a, q0, q1, q2, x, y, z)) { status = SDFGPU_PROJECT_LEFT_GRID; return; }
        d = estimate(a, q0, q1, q2, x, y, z);
        done = !(d <= a.min_dist);
    }

    // One pass of the reference's loop body; sets `done` when the walk ends.
    __device__ __forceinline__ void step(const ProjectArgs& a) {
        if (steps >= a.step_limit) { status = SDFGPU_PROJECT_STEP_LIMIT; done = true; return; }
        double g0, g1, g2;
        gradient(a, x, y, z, g0, g1, g2);
        // Vector4d(g0, g1, g2, 0).norm(): ((0 + g0 g0) + g1 g1) + g2 g2, then + 0 * 0 (which changes no sum >= +0 or NaN)
        double s = 0.0;
        s = s + g0 * g0;
        s = s + g1 * g1;
        s = s + g2 * g2;
        const double nrm = __dsqrt_rn(s);
        if (!(nrm > a.flat)) { status = SDFGPU_PROJECT_FLAT_GRADIENT; done = true; return; }
        const double rem = a.margin - d;
        const double step_distance = (rem < a.max_step) ? rem : a.max_step;      // std::min(max_step, margin - d)
        q0 = q0 + (g0 / nrm) * step_distance;                                    // normalized(): s > 0 here
        q1 = q1 + (g1 / nrm) * step_distance;
        q2 = q2 + (g2 / nrm) * step_distance;
        ++steps;
        if (!cell_of(a, q0, q1, q2, x, y, z)) { status = SDFGPU_PROJECT_LEFT_GRID; done = true; return; }
        d = estimate(a, q0, q1, q2, x, y, z);
        done = !(d <= a.min_dist);
    }

    __device__ __forceinline__ void finish(const ProjectArgs& a, int64_t i) const {
        double r0 = q0, r1 = q1, r2 = q2;
        if (!world) transform(a.g2w, q0, q1, q2, r0, r1, r2);
        a.out[3 * i] = r0;
        a.out[3 * i + 1] = r1;
        a.out[3 * i + 2] = r2;
        if (a.status) a.status[i] = status;
        if (a.steps) a.steps[i] = steps;
    }
};

// One lane per point; the loop is bounded by step_limit (the host caps it at SDFGPU_PROJECT_MAX_STEPS_CEILING or the caller's
// max_steps).
__global__ __launch_bounds__(kThreads) void k_project(const ProjectArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    Walk w;
    w.start(a, i);
    while (!w.done) w.step(a);
    w.finish(a, i);
}

}  // namespace

int project_step_limit(int64_t nx, int64_t ny, int64_t nz, double stepsize_multiplier, int max_steps) {
    if (max_steps < 0 || !(stepsize_multiplier > 0.0) || !std::isfinite(stepsize_multiplier)) return -1;
    if (max_steps > 0) return max_steps;
    const double diagonal = std::sqrt((double)nx * (double)nx + (double)ny * (double)ny + (double)nz * (double)nz);
    const double limit = 4.0 * std::ceil(diagonal / stepsize_multiplier) + 64.0;
    return limit < (double)SDFGPU_PROJECT_MAX_STEPS_CEILING ? (int)limit : SDFGPU_PROJECT_MAX_STEPS_CEILING;
}

void project_prepare(ProjectArgs& a, double resolution, double minimum_distance, double stepsize_multiplier) {
    // the expressions of SignedDistanceField::ProjectOutOfCollisionToMinimumDistanceGridFrameCounted / ClampIntoValidVolume
    a.res = resolution;
    a.inv_res = 1.0 / resolution;
    a.half = resolution * 0.5;
    a.inv2 = 1.0 / (2.0 * resolution);
    a.flat = resolution * 0.25;
    a.min_dist = minimum_distance;
    a.margin = minimum_distance + resolution * stepsize_multiplier * 1e-4;
    a.max_step = resolution * stepsize_multiplier;
    a.clamp_m = (a.mode == SDFGPU_PROJECT_INTO_VALID_VOLUME ? minimum_distance : 0.0) + resolution * 1e-4;
    a.size[0] = (double)a.nx * resolution;
    a.size[1] = (double)a.ny * resolution;
    a.size[2] = (double)a.nz * resolution;
}

hipError_t project_launch(const ProjectArgs& a, hipStream_t s) {
    const int64_t blocks = (a.n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_project, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

int check_project_args(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                       const double* world_to_grid, const double* grid_to_world, double stepsize_multiplier, int max_steps, int mode,
                       const double* points, int64_t n_points, const double* out_points, ProjectArgs& a) {
    if (!d_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "projection: null field pointer");
    if (n_points < 0 || n_points > ((int64_t)1 << 40)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "projection: point count %lld out of range [0, 2^40]", (long long)n_points);
    if (n_points > 0 && (!points || !out_points)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "projection: null points or out_points");
    if (!world_to_grid || !grid_to_world) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "projection: world_to_grid and grid_to_world are required");
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx > INT64_MAX / ny || nx * ny > INT64_MAX / nz)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "projection: unsupported grid %lld x %lld x %lld", (long long)nx, (long long)ny, (long long)nz);
    if (!(resolution > 0.0) || !std::isfinite(resolution)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "projection: resolution must be positive and finite");
    if (mode != SDFGPU_PROJECT_OUT_OF_COLLISION && mode != SDFGPU_PROJECT_INTO_VALID_VOLUME)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "projection: unknown mode %d", mode);
    const int limit = project_step_limit(nx, ny, nz, stepsize_multiplier, max_steps);
    if (limit < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "projection: stepsize_multiplier must be positive and finite and max_steps >= 0");
    a = ProjectArgs{};
    a.sdf = d_sdf; a.n = n_points; a.nx = nx; a.ny = ny; a.nz = nz;
    a.step_limit = limit; a.mode = mode;
    for (int i = 0; i < 12; ++i) { a.w2g[i] = world_to_grid[i]; a.g2w[i] = grid_to_world[i]; }
    return SDFGPU_OK;
}

}  // namespace

extern "C" {

int sdfgpu_project_step_limit(int64_t nx, int64_t ny, int64_t nz, double stepsize_multiplier, int max_steps, int* out_limit) {
    if (!out_limit || nx <= 0 || ny <= 0 || nz <= 0) return SDFGPU_ERR_INVALID_ARGUMENT;
    const int limit = project_step_limit(nx, ny, nz, stepsize_multiplier, max_steps);
    if (limit < 0) return SDFGPU_ERR_INVALID_ARGUMENT;
    *out_limit = limit;
    return SDFGPU_OK;
}

int sdfgpu_project_points_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 const double world_to_grid[12], const double grid_to_world[12], double minimum_distance,
                                 double stepsize_multiplier, int max_steps, int mode, const double* d_points, int64_t n_points,
                                 double* d_out_points, uint8_t* d_out_status, int32_t* d_out_steps, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        ProjectArgs a;
        if (int rc = check_project_args(h, d_sdf, nx, ny, nz, resolution, world_to_grid, grid_to_world, stepsize_multiplier, max_steps,
                                        mode, d_points, n_points, d_out_points, a)) return rc;
        if (n_points == 0) return SDFGPU_OK;
        HIP_TRY(h, hipSetDevice(h->device));
        a.points = d_points; a.out = d_out_points; a.status = d_out_status; a.steps = d_out_steps;
        project_prepare(a, resolution, minimum_distance, stepsize_multiplier);
        HIP_TRY(h, project_launch(a, (hipStream_t)stream));
        return SDFGPU_OK;
    });
}

int sdfgpu_project_points(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                          const double world_to_grid[12], const double grid_to_world[12], double minimum_distance,
                          double stepsize_multiplier, int max_steps, int mode, const double* points, int64_t n_points,
                          double* out_points, uint8_t* out_status, int32_t* out_steps) {
    return rz_wrap(h, nullptr, [&]() -> int {
        ProjectArgs a;
        if (int rc = check_project_args(h, d_sdf, nx, ny, nz, resolution, world_to_grid, grid_to_world, stepsize_multiplier, max_steps,
                                        mode, points, n_points, out_points, a)) return rc;
        if (n_points == 0) return SDFGPU_OK;
        HIP_TRY(h, hipSetDevice(h->device));
        // points | out points | steps | status
        return with_staged_points(h, points, n_points, {24, 4, 1}, {out_points, out_steps, out_status}, [&](const double* d_points, char* const (&d)[3]) -> int {
            a.points = d_points; a.out = (double*)d[0]; a.steps = (int32_t*)d[1]; a.status = (uint8_t*)d[2];
            project_prepare(a, resolution, minimum_distance, stepsize_multiplier);
            HIP_TRY(h, project_launch(a, nullptr));
            return SDFGPU_OK;
        });
    });
}

}  // extern "C"
