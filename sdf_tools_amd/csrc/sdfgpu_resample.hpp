// sdfgpu_resample.hpp -- CollisionMapGrid / TaggedObjectCollisionMapGrid::Resample (reference src/sdf_tools/collision_map.cpp:673-695,
// tagged_object_collision_map.cpp:399-422) on the GPU: the interface between the kernels in sdfgpu_resample.hip and the host code
// at the end of that file (which owns the scratch and the ordering).
//
// Contract (include/sdfgpu.h "Resample"): every source cell (x, y, z), in x -> y -> z order, goes to
//   loc = origin * (cell * (i + 0.5), 1),  p = dst_inverse_origin * loc,  idx = floor(p * dst_inv_cell) per axis
// and, when idx is inside the result, overwrites result cell idx with its whole record.  So the source cell with the LARGEST
// linear index among those that land in a result cell stays, and a result cell on which none lands keeps the fill record (any
// upsampling leaves such holes: the reference's behaviour, kept).  Launches, all on the caller's stream:
//   memset          the winner words (and the counter) to 0
//   k_rs_winner     one lane per source cell, z fastest; reads no cell data; the arithmetic above in double precision, in the
//                   product order of eigen_lite.hpp's Isometry3d * Vector4d, uncontracted; atomicMax(winner[dst], src + 1).
//                   Lanes of a wave are ascending in the source index, so of a run of neighbouring lanes with one destination
//                   only the last issues the atomic (the pre-reduced form; kRsPlain issues one per lane)
//   k_rs_gather     one lane per result cell: w = winner[d]; dst[d] = w ? src[w - 1] : fill; counts the cells with w != 0 when
//                   asked (one atomic per workgroup)
// winner words are uint32 while the source has fewer than 2^32 - 1 cells, unsigned long long otherwise.  Every index is int64;
// launches of more than kRsGridX workgroups go over two grid dimensions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfgpu {

constexpr int kRsThreads = 256;
constexpr int64_t kRsGridX = (int64_t)1 << 22;

struct ResampleArgs {
    const void* src = nullptr;         // n_src records of cell_bytes, 4-byte aligned
    void* dst = nullptr;               // n_dst records
    void* winner = nullptr;            // n_dst words of winner_bytes, zeroed
    unsigned long long* written = nullptr;   // zeroed counter, or nullptr: not wanted
    int64_t nx = 0, ny = 0, nz = 0;    // source cells
    int64_t mx = 0, my = 0, mz = 0;    // result cells
    int64_t n_src = 0, n_dst = 0;
    double cell[3] = {0, 0, 0};        // source cell sizes
    double origin[16] = {};            // row-major 4 x 4
    double inverse[16] = {};           // the result's inverse origin transform, row-major 4 x 4
    double inv_cell[3] = {0, 0, 0};    // 1.0 / the result's cell sizes
    uint32_t fill[4] = {0, 0, 0, 0};   // the fill record
    int cell_bytes = 0;                // 4, 8 or 16
    int winner_bytes = 4;              // 4 or 8
    bool plain_atomics = false;        // one atomic per lane (measurement only)
};

// 4 while every src + 1 fits a uint32 word, else 8
inline int resample_winner_bytes(int64_t n_src) { return n_src < (int64_t)0xFFFFFFFFll ? 4 : 8; }
// winner words | counter (8 bytes, 8-byte aligned)
inline size_t resample_counter_offset(int64_t n_dst, int winner_bytes) { return (((size_t)n_dst * (size_t)winner_bytes) + 7) & ~(size_t)7; }
inline size_t resample_scratch_bytes(int64_t n_dst, int winner_bytes) { return resample_counter_offset(n_dst, winner_bytes) + 8; }

// memset + k_rs_winner + k_rs_gather on `s`; a.winner holds resample_scratch_bytes(a.n_dst, a.winner_bytes) bytes and a.written,
// when wanted, points at its counter.  after_winner (optional) is recorded between the two kernels (tools/resample_bench.py).
hipError_t resample_launch(const ResampleArgs& a, hipStream_t s, hipEvent_t after_winner = nullptr);

}  // namespace sdfgpu
