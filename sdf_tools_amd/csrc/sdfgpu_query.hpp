// sdfgpu_query.hpp -- the interpolated gradients (SignedDistanceField::GetSmoothGradient*, GetAutoDiffGradient*,
// DistanceToBoundary*, reference include/sdf_tools/sdf.hpp:528-653, 963-988), the interface between the kernel in
// sdfgpu_query.hip and the host code at the end of that file (which checks the arguments and owns the staging).
//
// Contract: include/sdfgpu.h "Interpolated gradients".  One lane per point, in double; the constants are computed once on the
// host with the host core's expressions (SignedDistanceField::QueryGradient4d) so that the device repeats its arithmetic
// operation for operation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfgpu {

struct GradientQueryArgs {
    const float* sdf;
    const double* points;      // [n][3] world frame
    double* value;             // [n] or null
    double* gradient;          // [n][3] or null
    uint8_t* status;           // [n] or null
    int64_t n, nx, ny, nz;
    double res, inv_res;       // res, 1.0 / res
    double half;               // res * 0.5 (the centre-distance correction)
    double window;             // |window| (smooth)
    double oob;                // (double)oob_value
    double size[3];            // cells * res per axis
    double w2g[12];            // row-major 3x4 world -> grid
    int kind;                  // SDFGPU_QUERY_SMOOTH_GRADIENT / _AUTODIFF_GRADIENT / _DISTANCE_TO_BOUNDARY
};

// The derived constants of `a` (res .. size, from a.nx, a.ny, a.nz and the arguments), computed in this translation unit so that
// no host compiler contracts them either.
void query_gradients_prepare(GradientQueryArgs& a, double resolution, double window, float oob_value);

// Enqueue the query of a.n > 0 points on `s`.
hipError_t query_gradients_launch(const GradientQueryArgs& a, hipStream_t s);

}  // namespace sdfgpu
