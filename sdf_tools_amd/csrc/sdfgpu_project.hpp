// sdfgpu_project.hpp -- projection out of collision / into the valid volume (SignedDistanceField::ProjectOutOfCollision*,
// ProjectIntoValidVolume*, reference include/sdf_tools/sdf.hpp:996-1190), the interface between the kernel in sdfgpu_project.hip
// and the host code at the end of that file (which checks the arguments, precomputes the constants below and owns the staging).
//
// Contract: include/sdfgpu.h "Projection".  One lane per point walks the reference's loop in double, bounded by step_limit; the
// constants are computed once on the host with the host walk's expressions (SignedDistanceField::
// ProjectOutOfCollisionToMinimumDistanceGridFrameCounted), so that the device repeats its arithmetic operation for operation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfgpu {

struct ProjectArgs {
    const float* sdf;
    const double* points;      // [n][3] world frame
    double* out;               // [n][3] world frame
    uint8_t* status;           // [n] or null
    int32_t* steps;            // [n] or null
    int64_t n, nx, ny, nz;
    double res, inv_res;       // res, 1.0 / res
    double half;               // res * 0.5 (the centre-distance correction)
    double inv2;               // 1.0 / (2.0 * res) (central differences)
    double flat;               // res * 0.25 (the "flat gradient" test)
    double min_dist;           // minimum_distance
    double margin;             // minimum_distance + res * stepsize_multiplier * 1e-4
    double max_step;           // res * stepsize_multiplier
    double clamp_m;            // the clamp margin: res * 1e-4 (out of collision), minimum_distance + res * 1e-4 (valid volume)
    double size[3];            // cells * res per axis
    double w2g[12], g2w[12];   // row-major 3x4 world -> grid, grid -> world
    int32_t step_limit;
    int mode;                  // SDFGPU_PROJECT_OUT_OF_COLLISION / SDFGPU_PROJECT_INTO_VALID_VOLUME
};

// The step limit of a walk (include/sdfgpu.h): max_steps, or for 0 the default 4 * ceil(sqrt(nx^2 + ny^2 + nz^2) /
// stepsize_multiplier) + 64 capped at SDFGPU_PROJECT_MAX_STEPS_CEILING; -1 for max_steps < 0 or a stepsize_multiplier that is
// not positive and finite.
int project_step_limit(int64_t nx, int64_t ny, int64_t nz, double stepsize_multiplier, int max_steps);

// The derived constants of `a` (res .. size, from a.nx, a.ny, a.nz and the arguments), computed in this translation unit so that
// no host compiler contracts them either.
void project_prepare(ProjectArgs& a, double resolution, double minimum_distance, double stepsize_multiplier);

// Enqueue the walk of a.n > 0 points on `s`.
hipError_t project_launch(const ProjectArgs& a, hipStream_t s);

}  // namespace sdfgpu
