// sdfgpu_batch.hpp -- B grids of one small shape in one launch sequence (include/sdfgpu.h "Batches of same-shape grids"), the
// interface between the kernels in sdfgpu_batch.hip and the C ABI in sdfgpu.hip (which checks the arguments, owns the scratch
// and the staging, and falls back to one single build per grid for shapes the kernels do not take).  DESIGN.md section 18.
//
// Layout: grid b at offset b * nx * ny * nz of the input and of the output, each [nx][ny][nz] (z fastest).  The kernels compute the
// same signed d^2 field as the single build (sdfgpu_kernels.hpp: + free / - filled, exact separable squared EDT) by an exact
// min-plus over whole lines: every axis is at most kBatchMaxAxis cells, so a line has at most 128 candidates and a plane fits
// in LDS.  No tier, no probe, no guard: two launches whatever the scenes are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfgpu {

constexpr int kBatchMaxAxis = 128;     // 2 * 127^2 < 32767: the in-plane d^2 of such a grid fits the int16 scratch field
constexpr int kBatchTileCols = 128;    // y.z columns per workgroup of the x pass

struct BatchArgs {
    const uint8_t* mask;       // [batch][n] occupancy bytes, or null (tagged)
    const char* cells;         // tagged: the records of ONE grid [n], read for every b (filled iff occupied and object id == ids[b])
    int64_t stride, occ_off, obj_off;
    int unknown_is_filled;
    const uint32_t* ids;       // tagged: [batch] (device)
    int16_t* plane;            // [batch][n] scratch: signed in-plane d^2 (+ free / - filled, magnitude 32767 = none in the plane)
    float* out;                // [batch][n]
    const double* res;         // [batch] (device) per-grid resolutions, or null: res_uniform for every grid
    double res_uniform;
    uint32_t* ext;             // [batch][2] max d^2 over free, over filled voxels (zeroed by the first kernel)
    int batch, nx, ny, nz;     // canonical dims (singleton axes in front), each <= kBatchMaxAxis
    int vb;
};

inline bool batch_fast_shape(int64_t nx, int64_t ny, int64_t nz) {
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= kBatchMaxAxis && ny <= kBatchMaxAxis && nz <= kBatchMaxAxis;
}

// Enqueue k_batch_zy and k_batch_x_finish on `s`; *launches = kernels launched.
hipError_t batch_launch(const BatchArgs& a, hipStream_t s, int* launches);

// sdfgpu_gradient_device's definition on every grid of a batch: one launch.  scales: [batch] GradScale records (device; see
// sdfgpu_kernels.hpp) or null, in which case `uniform` (4 doubles' worth: inv2, inv_w1, inv_w2, inv2f) holds for every grid.
struct BatchGradArgs {
    const float* sdf;          // [batch][n]
    void* out;                 // [batch][n][3] float64 (f64) or float32
    const void* scales;        // device GradScale[batch], or null
    double inv2, inv_w1, inv_w2;
    int64_t nx, ny, nz;
    int batch, edge, f64;
};
hipError_t batch_gradient_launch(const BatchGradArgs& a, hipStream_t s);

}  // namespace sdfgpu
