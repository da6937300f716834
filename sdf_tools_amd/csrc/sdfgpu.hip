// sdfgpu.hip -- the SDF build: C ABI (include/sdfgpu.h) over the gfx950 kernels in sdfgpu_kernels.hpp and its sibling build
// headers, and the one unit that launches them.  Host side of the drop-in boundary for
// sdf_generation::ExtractSignedDistanceField (reference include/sdf_tools/sdf_generation.hpp:209-420).  No CPU fallback.
// The handle and its helpers are in sdfgpu_context.hpp / .hip; the analysis families (components, topology, surfaces, local
// extrema, projection, query gradients, resample, display) keep their host code and entry points in their own units.
#include "sdfgpu_kernels.hpp"
#include "sdfgpu_sweep_x16.hpp"
#include "sdfgpu_sweep_y16.hpp"
#include "sdfgpu_dense3.hpp"
#include "sdfgpu_dense6.hpp"
#include "sdfgpu_fused_zy.hpp"
#include "sdfgpu_dense.hpp"
#include "sdfgpu_envelope_dc.hpp"
#include "sdfgpu_convex.hpp"
#include "sdfgpu_batch.hpp"
#include "sdfgpu_context.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

using namespace sdfgpu;

namespace {

constexpr int kH = 3;            // register-window radius of the marching sweeps

// the cell records of `occ` as the kernels read them
CellLoader cell_loader(const Occupancy& occ) {
    return CellLoader{reinterpret_cast<const char*>(occ.cells), (int64_t)occ.stride, (int64_t)occ.off, occ.unknown};
}
// (kShellMinWords is the default of a host option and lives with BuildOptions; its unit is the words of one KD6 group)
static_assert(kShellMinWords <= kShellGroup * 256, "shell_min_words counts active words of a group of kShellGroup x 256");

int rows_per_block(int nz) {
    const int W = (nz + 63) / 64;
    return std::max(1, 4096 / (W * 64));
}

// K1 launch.  cells == nullptr -> uint8 mask.
bool z_wave16_shape(const sdfgpu_context* h, int64_t nz) {
    return h->opt.z_wave_on && (nz == 64 || nz == 128 || nz == 256 || nz == 512 || nz == 1024);
}

// whole rows per wave (16 nz-lanes): no workgroup barrier; 32 workgroups per CU's worth of persistent waves (measured
// at 512^3: 8 per CU 0.099 ms, 16 0.093, 32 0.088, one step per wave 0.100).  BITS (round 6): a wave reads its 16 voxels as one
// 16-bit piece of the bit field.
template <bool BITS>
void launch_z_wave16(const uint8_t* d_in, int16_t* d_out, int64_t nrows, int64_t nz, const uint32_t* guard, uint8_t* d_row_any, hipStream_t s) {
    const int rw = 1024 / (int)nz;                                  // rows per wave step
    const int64_t ngroups = (nrows + rw - 1) / rw;
    const dim3 gw((unsigned)std::min<int64_t>((ngroups + kBlock / 64 - 1) / (kBlock / 64), 8192)), block(kBlock);
    switch ((int)nz) {
        case 64: hipLaunchKernelGGL((k_sweep_z_wave16<4, BITS>), gw, block, 0, s, d_in, d_out, nrows, guard, d_row_any); break;
        case 128: hipLaunchKernelGGL((k_sweep_z_wave16<8, BITS>), gw, block, 0, s, d_in, d_out, nrows, guard, d_row_any); break;
        case 256: hipLaunchKernelGGL((k_sweep_z_wave16<16, BITS>), gw, block, 0, s, d_in, d_out, nrows, guard, d_row_any); break;
        case 512: hipLaunchKernelGGL((k_sweep_z_wave16<32, BITS>), gw, block, 0, s, d_in, d_out, nrows, guard, d_row_any); break;
        default: hipLaunchKernelGGL((k_sweep_z_wave16<64, BITS>), gw, block, 0, s, d_in, d_out, nrows, guard, d_row_any); break;
    }
}

// d_row_any != nullptr (callers check z_wave16_shape and, for masks, the alignment first): the kernel also writes one "holds a filled voxel" byte per z row
int launch_sweep_z(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, int16_t* d_out, const uint32_t* guard,
                   hipStream_t s, uint8_t* d_row_any = nullptr) {
    const int64_t nrows = nx * ny;
    const int rpb = rows_per_block((int)nz);
    const int W = ((int)nz + 63) / 64;
    const size_t lds = (size_t)rpb * W * 8 + (size_t)rpb * 4;     // bitmap + one class word per row (vec16 kernel)
    const int64_t nblocks = (nrows + rpb - 1) / rpb;
    // persistent row-group loop inside the kernel: 8 workgroups per CU are plenty, and a small grid
    // makes the guard early-exit (dense path certified) a ~2 us launch instead of ~10 us
    dim3 grid((unsigned)std::min<int64_t>(nblocks, 2048)), block(kBlock);
    const bool mask16 = occ.mask && (reinterpret_cast<uintptr_t>(occ.mask) % 16) == 0;
    if (mask16 && (nz % 16) == 0) {
        // the persistent grid must fit the device in ONE round: at 70 VGPRs 7 workgroups are resident per CU, and a grid of 8
        // per CU left 256 workgroups to run their 16 row groups alone after the others had finished
        if (h->k1_resident <= 0) {
            int per_cu = 0, cus = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sweep_z_vec16, kBlock, lds) != hipSuccess || per_cu <= 0) per_cu = 4;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus <= 0) cus = 256;
            h->k1_resident = per_cu * cus;
        }
        grid.x = (unsigned)std::min<int64_t>(nblocks, h->k1_resident);
    }
    if (occ.bits) {
        // every shape but the wave-private ones goes through the generic kernel with a bit loader
        if (z_wave16_shape(h, nz)) launch_z_wave16<true>(reinterpret_cast<const uint8_t*>(occ.bits), d_out, nrows, nz, guard, d_row_any, s);
        else hipLaunchKernelGGL(k_sweep_z_generic<BitsLoader>, grid, block, lds, s, BitsLoader{occ.bits}, d_out, nrows, (int)nz, rpb, guard);
    } else if (occ.cells) {
        hipLaunchKernelGGL(k_sweep_z_generic<CellLoader>, grid, block, lds, s, cell_loader(occ), d_out, nrows, (int)nz, rpb, guard);
    } else if (mask16 && z_wave16_shape(h, nz)) {
        launch_z_wave16<false>(occ.mask, d_out, nrows, nz, guard, d_row_any, s);
    } else if (mask16 && (nz % 16) == 0) {
        hipLaunchKernelGGL(k_sweep_z_vec16, grid, block, lds, s, occ.mask, d_out, nrows, (int)nz, rpb, guard);
    } else {
        hipLaunchKernelGGL(k_sweep_z_generic<MaskLoader>, grid, block, lds, s, MaskLoader{occ.mask}, d_out, nrows, (int)nz, rpb, guard);
    }
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

int pick_T(int user, int span) {
    int T = user > 0 ? user : 64;
    T = std::max(T, 2 * 8 + 1);
    return std::min(T, std::max(span, 1));
}

template <int STAGE, bool VB>
int launch_march(sdfgpu_handle h, SweepArgs a, bool vec4, hipStream_t s, bool wide_window = false) {
    const int span = a.out_hi - a.out_lo;
    const int nchunks = (span + a.T - 1) / a.T;
    const int64_t nbx = (a.ncols + kBlock - 1) / kBlock;
    if (nbx > 0x7fffffffLL || nchunks > 65535) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "sweep grid too large");
    dim3 grid((unsigned)nbx, (unsigned)nchunks), block(kBlock);
    bool wide = false;
    if constexpr (STAGE == 2 && !VB) {                       // radius-8 window: y sweep only
        if (vec4 && wide_window) {
            hipLaunchKernelGGL((k_sweep_march<2, 4, 8, false>), grid, block, 0, s, a);
            wide = true;
        }
    }
    if (wide) {}
    else if (STAGE == 2 && vec4 && a.out16 && kH == 3)      // y sweep into the 16-bit plane field: packed 16-bit window
        hipLaunchKernelGGL((k_sweep_y16<3>), grid, block, 0, s, a);
    else if (vec4) hipLaunchKernelGGL((k_sweep_march<STAGE, 4, kH, VB>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_sweep_march<STAGE, 1, kH, VB>), grid, block, 0, s, a);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// K2 launch: int16 z field -> int32 in-plane signed d^2
// (d_side != kNoSideTable: write the int16 plane field to d_out and exact saturated groups to d_side;
//  requires the vec4 path)
enum class YWindow { r3, r8 };       // register-window radius of the marching y sweep (r8: 4-voxel lanes only)
int launch_sweep_y(sdfgpu_handle h, const int16_t* d_in, void* d_out, int32_t* d_side, int64_t nx, int64_t ny,
                   int64_t nz, const uint32_t* guard, uint32_t* far_flag, hipStream_t s, YWindow window = YWindow::r3) {
    const bool vec4 = (nz % 4) == 0 && (reinterpret_cast<uintptr_t>(d_in) % 8) == 0 &&
                      (reinterpret_cast<uintptr_t>(d_out) % 16) == 0;
    if (d_side && !vec4) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "16-bit plane output needs nz % 4 == 0");
    const int V = vec4 ? 4 : 1;
    SweepArgs a{};
    a.in = d_in; a.out = d_out;
    a.out16 = d_side ? 1 : 0; a.side = d_side;
    a.guard = guard;
    if (far_flag) { a.max_scan = kScanExpectNear; a.far_flag = far_flag; }
    a.cpl = nz / V;
    a.ncols = nx * a.cpl;
    a.outer_stride = ny * nz;
    a.line_stride = nz;
    a.L = (int)ny; a.out_lo = 0; a.out_hi = (int)ny;
    a.T = pick_T(h->opt.tune_ty, (int)ny);
    if (h->opt.tune_ty <= 0 && vec4 && d_side) {
        // K2/16: chunks of 16 batches of 7 rows while the launch still fills the device.  Measured at 512^3 (rocprofv3):
        // 56 rows 131 us, 64 rows 138, 112 rows 122, 119 / 126 rows 123 - 125, 128 rows 132 -- with a power-of-two chunk the
        // workgroups, which march in step, read addresses that differ by multiples of 64 KB only.
        const int64_t nbx = (a.ncols + kBlock - 1) / kBlock;
        for (int t : {112, 56, 28}) {
            a.T = std::min(t, (int)ny);
            if (nbx * ((ny + t - 1) / t) >= 1024) break;
        }
    }
    return launch_march<2, false>(h, a, vec4, s, window == YWindow::r8);
}

// K12 launch: mask -> int32 in-plane signed d^2 in one kernel (nz = 512 or 1024, 16-B aligned mask)
bool fused_zy_nz(int64_t nz) { return nz == 512 || nz == 1024; }       // the kernel's instances
// (a stage call's test; a whole build's is plan_build's)
bool fused_zy_eligible(const sdfgpu_context* h, const uint8_t* d_mask, const void* d_out, int64_t nz) {
    return h->opt.fused_zy && d_mask && fused_zy_nz(nz) &&
           (reinterpret_cast<uintptr_t>(d_mask) % 16) == 0 && (reinterpret_cast<uintptr_t>(d_out) % 16) == 0;
}

template <int V, int H>
void launch_fused_variant(const FusedZyArgs& a0, int T, int64_t nx, int64_t ny, bool out16, hipStream_t s) {
    constexpr int R = 2 * H + 1;
    FusedZyArgs a = a0;
    a.T = std::min(std::max(T, R), (int)ny);
    const int wpb = kBlock / 64;
    dim3 grid((unsigned)((nx + wpb - 1) / wpb), (unsigned)((ny + a.T - 1) / a.T)), block(kBlock);
    const size_t lds = (size_t)wpb * (R + 1) * (8 + 64 * (V / 8) + 8);
    if (out16) hipLaunchKernelGGL((k_sweep_zy_fused<V, H, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_sweep_zy_fused<V, H, false>), grid, block, lds, s, a);
}

// d_side != kNoSideTable: d_out is the int16 plane field, saturated groups go to d_side
int launch_sweep_zy_fused(sdfgpu_handle h, const uint8_t* d_mask, void* d_out, int32_t* d_side, int64_t nx,
                          int64_t ny, int64_t nz, const uint32_t* guard, hipStream_t s) {
    FusedZyArgs a{};
    a.mask = d_mask; a.out = d_out; a.side = d_side; a.nx = (int)nx; a.ny = (int)ny;
    a.guard = guard;
    const int T = 64;
    const bool o16 = d_side != nullptr;
    if (nz == 512 && h->opt.fused_h == 3) launch_fused_variant<8, 3>(a, T, nx, ny, o16, s);
    else if (nz == 512) launch_fused_variant<8, 2>(a, T, nx, ny, o16, s);
    else launch_fused_variant<16, 2>(a, T, nx, ny, o16, s);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// K3/16 launch: int16 plane field + side table (optionally with x halo) -> fp32 sdf
template <int V, int H>
void launch_x16_variant(const SweepX16Args& a, dim3 grid, dim3 block, bool vb, bool slab, hipStream_t s) {
    if (vb && slab) hipLaunchKernelGGL((k_sweep_x16<V, H, true, true>), grid, block, 0, s, a);
    else if (vb) hipLaunchKernelGGL((k_sweep_x16<V, H, true, false>), grid, block, 0, s, a);
    else if (slab) hipLaunchKernelGGL((k_sweep_x16<V, H, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_sweep_x16<V, H, false, false>), grid, block, 0, s, a);
}

// The part of a grid an x sweep is launched on: planes [x_global, x_global + nxs) of nx_global with halo planes in front and behind,
// rows [y_off, y_off + ny) of ny_glob.
struct XSlab {
    int64_t halo_lo = 0, nxs = 0, halo_hi = 0;
    int lo_trunc = 0, hi_trunc = 0;         // the grid goes on beyond the halo on that side
    int64_t x_global = 0, nx_global = 0;
    int64_t y_off = 0, ny_glob = -1;        // K3 only; -1: the launch's own ny
    int64_t side_lo = 0, side_hi = 0;       // K3/16 only: the planes the side table covers
    uint32_t* status = nullptr;             // raised when a truncated halo was too short for a voxel (optional)
    static XSlab whole(int64_t nx) { XSlab g; g.nxs = g.nx_global = g.side_hi = nx; return g; }
};

int launch_sweep_x16(sdfgpu_handle h, const int16_t* d_in16, const int32_t* d_side, float* d_out, const XSlab& g, int64_t ny,
                     int64_t nz, double resolution, int vb, const uint32_t* guard, uint32_t* far_flag, hipStream_t s) {
    const int64_t plane = ny * nz;
    const int V = (h->opt.x16_v == 8) ? 8 : 4;
    SweepX16Args a{};
    a.in16 = d_in16; a.side32 = d_side; a.out = d_out;
    a.ncols = plane / V; a.plane = plane;
    a.L = (int)(g.halo_lo + g.nxs + g.halo_hi);
    a.out_lo = (int)g.halo_lo; a.out_hi = (int)(g.halo_lo + g.nxs);
    a.T = pick_T(h->opt.tune_tx, (int)g.nxs);
    a.side_lo = (int)g.side_lo; a.side_hi = (int)g.side_hi;
    a.resolution = resolution;
    a.lo_truncated = g.lo_trunc; a.hi_truncated = g.hi_trunc;
    a.x_global = g.x_global; a.nx_global = g.nx_global; a.ny = ny; a.nz = nz;
    a.maxdsq = h->d_slots; a.status = g.status;                 // maxima go to the slot array; the caller folds them (fold_slots)
    a.guard = guard;
    if (far_flag) { a.max_scan = kScanExpectNear; a.far_flag = far_flag; }
    const int span = a.out_hi - a.out_lo;
    const int nchunks = (span + a.T - 1) / a.T;
    const int64_t nbx = (a.ncols + kBlock - 1) / kBlock;
    if (nbx > 0x7fffffffLL || nchunks > 65535) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "sweep grid too large");
    dim3 grid((unsigned)nbx, (unsigned)nchunks), block(kBlock);
    const bool slab = g.lo_trunc || g.hi_trunc || g.side_lo > 0 || g.side_hi < a.L;
    if (V == 8) launch_x16_variant<8, 3>(a, grid, block, vb != 0, slab, s);
    else if (h->opt.x16_h == 2) launch_x16_variant<4, 2>(a, grid, block, vb != 0, slab, s);
    else if (h->opt.x16_h == 8 && !vb && !slab)      // wide window (option only): plain grids
        hipLaunchKernelGGL((k_sweep_x16<4, 8, false, false>), grid, block, 0, s, a);
    else launch_x16_variant<4, 3>(a, grid, block, vb != 0, slab, s);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// K3 launch: int32 plane field (optionally with x halo) -> fp32 sdf
int launch_sweep_x(sdfgpu_handle h, const int32_t* d_in, float* d_out, const XSlab& g, int64_t ny, int64_t nz, double resolution,
                   int vb, const uint32_t* guard, uint32_t* far_flag, hipStream_t s) {
    const int64_t plane = ny * nz;
    const bool vec4 = (plane % 4) == 0 && (reinterpret_cast<uintptr_t>(d_in) % 16) == 0 &&
                      (reinterpret_cast<uintptr_t>(d_out) % 16) == 0;
    const int V = vec4 ? 4 : 1;
    SweepArgs a{};
    a.in = d_in; a.out = d_out;
    a.ncols = plane / V;
    a.cpl = a.ncols;
    a.outer_stride = 0;
    a.line_stride = plane;
    a.L = (int)(g.halo_lo + g.nxs + g.halo_hi);
    a.out_lo = (int)g.halo_lo; a.out_hi = (int)(g.halo_lo + g.nxs);
    a.T = pick_T(h->opt.tune_tx, (int)g.nxs);
    a.resolution = resolution;
    a.lo_truncated = g.lo_trunc; a.hi_truncated = g.hi_trunc;
    a.x_global = g.x_global; a.nx_global = g.nx_global; a.ny = ny; a.nz = nz;
    a.y_off = g.y_off; a.ny_glob = g.ny_glob < 0 ? ny : g.ny_glob;
    if (far_flag) { a.max_scan = kScanExpectNear; a.far_flag = far_flag; }
    a.maxdsq = h->d_slots; a.status = g.status;                 // maxima go to the slot array; the caller folds them (fold_slots)
    a.guard = guard;
    return vb ? launch_march<3, true>(h, a, vec4, s) : launch_march<3, false>(h, a, vec4, s);
}

// Shapes the far-field kernel takes (any line count; keys must fit 32 bits: finf + (L + 2)^2 < 2^(32 - B)).
struct DcGeometry { bool ok; int B; uint32_t finf; int pitch; int M, Kp; };
// dynamic LDS a far-field launch may ask for: the CU's 160 KB less the kernel's few static words (the fold of the stand-by x sweep)
constexpr size_t kDcMaxDynamicLds = 160 * 1024 - 256;
// What a far-field launch (sweep or probe) reads and writes.  Stage 2 reads the z field (in16) or the dense tier's bit field and
// writes the int16 plane field + side table (out, side_out) or an int32 plane field (out_i32); stage 3 reads either pair and
// writes the fp32 field (out).
struct DcIo {
    const int16_t* in16 = nullptr;
    const int32_t* side_in = nullptr;
    void* out = nullptr;
    int32_t* side_out = nullptr;
    const int32_t* in_i32 = nullptr;
    int32_t* out_i32 = nullptr;
    const uint32_t* i32_flag = nullptr;     // device word: use the int32 fields only when it is non-zero (nullptr: always)
    int64_t y_off = 0, ny_glob = -1;        // y-slab geometry (-1: the launch's own ny)
    const uint32_t* bits = nullptr;         // stage 2: z distances from the dense tier's bit field instead of the z field (forces the scalar form)
    int nzw = 0;
    // sweeps only
    bool loop = false;                      // LOOP form of the kernel: a small grid whose workgroups walk the tiles (stand-by launches)
    uint32_t* ran_flag = nullptr;           // status word raised by a launch that does work
    const uint32_t* row_bits = nullptr;     // plane sparsity (see EnvDcArgs); nullptr: every plane is processed
    int row_words = 0;
    const uint8_t* plane_any = nullptr;
    uint32_t* fold_result = nullptr;        // stage 3, LOOP form: the launch also does the end-of-build fold (fold_ticket = a free status word)
    uint32_t* fold_report = nullptr;
    uint32_t* fold_ticket = nullptr;
};
// The probes' fixed fractions (BuildOptions::far_thr holds the thresholds): an axis is far-field when more than 1 / kFarDen of the
// probed voxels reach its threshold (y, x); the y sweep takes radius-8 windows when more than 1 / kMidDenY of them have d^2 >= kMidThrY.
constexpr int kFarDen[2] = {5, 24};
constexpr int kMidThrY = 16, kMidDenY = 24;
struct DcDecide {                // a probe launch turns its counters into the tier decision itself (last workgroup)
    int stage = 0; bool dense_tried = false, handoff = false, window_choice = false;
};
// Shapes refused here (keys wider than 32 bits: finf + (L + 2)^2 >= 2^(32 - B); 2^31 voxels or more) take the marching sweeps
// with unbounded scans.  In practice the key gate decides for every line longer than 1024: from L = 1025 on, B = 11 and
// (L - 1)^2 + (L + 2)^2 alone exceed 2^21, so the L > 2048, 24-bit and LDS tests below never turn a shape away by themselves.
DcGeometry envelope_dc_geometry(const sdfgpu_context* h, int stage, int64_t nx, int64_t ny, int64_t nz, int64_t ny_full = -1) {
    DcGeometry g{};
    if (ny_full < 0) ny_full = ny;
    const int64_t L = stage == 2 ? ny : nx;
    if (!h->opt.envelope_dc || L < 1 || L > 2048 || nx * ny * nz >= (1ll << 31)) return g;
    int B = 1;
    while ((1ll << B) < L) ++B;
    const int64_t finf = (nx - 1) * (nx - 1) + (ny_full - 1) * (ny_full - 1) + (nz - 1) * (nz - 1) + 1;   // > every real d^2
    if (finf + (L + 2) * (L + 2) >= (1ll << (32 - B))) return g;
    if ((L + 2) * (2ll << B) >= (1ll << 23)) return g;            // 24-bit multiplier operands
    if (envelope_dc_lds_bytes((int)L) > kDcMaxDynamicLds) return g;
    g.ok = true; g.B = B; g.finf = (uint32_t)finf;
    g.pitch = envelope_dc_pitch((int)L);
    g.M = (int)((L + 7) / 8);
    g.Kp = 0;
    return g;
}

bool far_geometry_ok(const sdfgpu_context* h, int stage, int64_t nx, int64_t ny, int64_t nz, int64_t ny_full = -1) {
    return envelope_dc_geometry(h, stage, nx, ny, nz, ny_full).ok;
}

// probe counters -> guard words, for a build whose tier is forced or whose probe has no tile to sample
int launch_decide(sdfgpu_handle h, const DcDecide& dec, hipStream_t s) {
    hipLaunchKernelGGL(k_decide_tier, dim3(1), dim3(1), 0, s, h->d_small, dec.stage, dec.dense_tried ? 1 : 0, h->opt.force_env,
                       1, kFarDen[dec.stage], dec.handoff ? 1 : 0, (dec.stage == 0 && dec.window_choice) ? kMidDenY : 0);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// What the far-field sweep and its tile probe share: the line geometry and the fields of `io` both read.
int envelope_args(sdfgpu_handle h, int stage, const DcIo& io, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                  const uint32_t* guard, EnvDcArgs& a) {
    const DcGeometry g = envelope_dc_geometry(h, stage, nx, ny, nz, io.ny_glob);
    if (!g.ok) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "shape not taken by the far-field kernel (internal: callers check the geometry first)");
    a.in16 = io.in16; a.side_in = io.side_in; a.out = io.out; a.side_out = io.side_out;
    constexpr int NL = kDcLines;
    if (stage == 2) { a.group_lines = nz; a.tiles_per_outer = (nz + NL - 1) / NL; a.ntiles = nx * a.tiles_per_outer; a.outer_stride = ny * nz; a.line_stride = nz; a.L = (int)ny; }
    else { a.group_lines = ny * nz; a.tiles_per_outer = (ny * nz + NL - 1) / NL; a.ntiles = a.tiles_per_outer; a.outer_stride = 0; a.line_stride = ny * nz; a.L = (int)nx; }
    a.B = g.B; a.finf = g.finf; a.pitch = g.pitch; a.M = g.M; a.Kp = 0; a.h = (a.L + 1) / 2;
    a.resolution = resolution; a.vb = vb; a.nx = nx; a.ny = ny; a.nz = nz;
    a.in_i32 = io.in_i32; a.out_i32 = io.out_i32; a.y_off = io.y_off; a.i32_flag = io.i32_flag;
    a.ny_glob = io.ny_glob >= 0 ? io.ny_glob : ny;
    a.ran_flag = io.ran_flag;
    if (stage == 2) { a.bits = io.bits; a.nzw = io.nzw; }
    a.maxdsq = h->d_slots; a.guard = guard;
    if (a.ntiles > 0x7fffffffLL) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "envelope grid too large");
    return SDFGPU_OK;
}

// vector loads: 4 consecutive lines per load, whole tiles, aligned rows
bool envelope_vector_form(const EnvDcArgs& a) {
    auto al = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; };
    return !a.bits && (a.nz % 4) == 0 && (a.group_lines % kDcLines) == 0 && al(a.in16, 8) && al(a.side_in, 16) && al(a.in_i32, 16);
}

// Picks the kernel instance for `a` (a.ntiles = the tiles of this launch) and launches it.
int launch_envelope_kernel(sdfgpu_handle h, int stage, EnvDcArgs& a, bool loop, bool probe, hipStream_t s) {
    constexpr int NL = kDcLines;
    const bool vec = envelope_vector_form(a);
    const size_t lds = envelope_dc_lds_bytes(a.L, NL);
    // (the kernel is a template over lines per tile and lanes; measured at 512^3: 8-line tiles -- 20 KB of LDS, 7 - 8
    //  workgroups per CU -- with 128 or 256 lanes are 12 - 25 % slower than 16 lines x 256 lanes, 16 lines x 512 lanes
    //  +-5 %, 32 lines x 512 lanes +-3 %; 2 instead of 4 workgroups per CU is 1.55x slower)
    // lines above 512: the tile's keys take 66 KB and more, two workgroups per CU -- of 512 lanes then (round 4: with 256 they
    // left the CU at 2 waves per SIMD, and 1024-voxel lines cost 1.5 - 2x their share).  Round 5 tried the other way out, 8 lines
    // x 256 lanes (38 KB: four workgroups per CU again) on the 1024^3 scenes: same fields bit for bit, room 18.1 ms instead of
    // 16.0, boxes / shells / spheres within 2 % -- the long lines are not short of resident workgroups
    const bool big = a.L > 512 && !loop;
    const int NT = big ? 512 : 256;
    // LOOP form: at most 2048 workgroups (a guarded exit costs 1.7 us up to there and grows with the grid), a multiple of 8
    // so that a workgroup's tiles stay on its XCD
    const int64_t nwg = loop ? std::min<int64_t>(a.ntiles, h->opt.standby_grid) : a.ntiles;
    // 512-voxel lines, vector loads, one tile per workgroup: the instances with the line's geometry as compile-time constants (option "dc_fixed")
    const bool fixed512 = h->opt.dc_fixed && a.L == 512 && vec && !loop && !big && a.B == 9 && a.pitch == 514 && a.M == 64 && a.h == 256;
    const bool fixed1024 = h->opt.dc_fixed && a.L == 1024 && vec && big && a.B == 10 && a.pitch == 1026 && a.M == 128 && a.h == 512;
    const int which = fixed512 ? 12 + (stage == 3 ? 1 : 0) : fixed1024 ? 14 + (stage == 3 ? 1 : 0) :
                      (stage == 3 ? 1 : 0) + (vec ? 2 : 0) + (loop ? 4 : 0) + (big ? 8 : 0);
    if (stage == 3 && !probe) h->last.last_dc_x = which + 1;
    // the instances by `which`: stage 2 / 3, scalar / vector loads, LOOP form, 512 lanes, fixed 512- / 1024-voxel lines
    static void (*const kKernels[16])(const EnvDcArgs) = {
        k_envelope_dc<2, false, 256, 16>, k_envelope_dc<3, false, 256, 16>, k_envelope_dc<2, true, 256, 16>, k_envelope_dc<3, true, 256, 16>,
        k_envelope_dc<2, false, 256, 16, true>, k_envelope_dc<3, false, 256, 16, true>,
        k_envelope_dc<2, true, 256, 16, true>, k_envelope_dc<3, true, 256, 16, true>,
        k_envelope_dc<2, false, 512, 16, false, 4>, k_envelope_dc<3, false, 512, 16, false, 4>,
        k_envelope_dc<2, true, 512, 16, false, 4>, k_envelope_dc<3, true, 512, 16, false, 4>,
        k_envelope_dc<2, true, 256, 16, false, 4, 512>, k_envelope_dc<3, true, 256, 16, false, 4, 512>,
        k_envelope_dc<2, true, 512, 16, false, 4, 1024>, k_envelope_dc<3, true, 512, 16, false, 4, 1024>};
    // (the attribute is per kernel: raised once per instantiation, not on every launch -- ADVICE r3)
    if (lds > 64 * 1024 && !h->dc_attr_set[which]) {
        HIP_TRY(h, hipFuncSetAttribute((const void*)kKernels[which], hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDcMaxDynamicLds));
        h->dc_attr_set[which] = true;
    }
    hipLaunchKernelGGL(kKernels[which], dim3((unsigned)nwg), dim3((unsigned)NT), lds, s, a);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// KE2 / KE3: exact far-field sweeps.  guard: run iff *guard != 0 (kUnguarded: always).
int launch_envelope(sdfgpu_handle h, int stage, const DcIo& io, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                    const uint32_t* guard, hipStream_t s) {
    EnvDcArgs a{};
    if (int rc = envelope_args(h, stage, io, nx, ny, nz, resolution, vb, guard, a)) return rc;
    if (io.row_bits || io.plane_any) {                              // plane sparsity, and the flat tiles that go with the row masks
        a.row_bits = io.row_bits; a.row_words = io.row_words; a.plane_any = io.plane_any;
        a.some_empty = h->d_small + kSwPlaneEmpty; a.flat_on = h->opt.flat_tiles; a.flat_score = h->d_small + kSwFlatScore;
    }
    if (stage == 3 && io.loop && io.fold_ticket) {
        a.fold_status = h->d_small; a.fold_result = io.fold_result; a.fold_report = io.fold_report; a.fold_ticket = io.fold_ticket;
        a.fold_report_mask = kReportDense;
    }
    return launch_envelope_kernel(h, stage, a, io.loop, false, s);
}

// The stand-by pair behind a trusted dense tier as ONE launch (k_envelope_standby; option "standby_single"): the LOOP-form y sweep
// (`ke2`), the LOOP-form x sweep (`ke3`) and, when ke3 carries a fold ticket, the end-of-build fold.  The workgroups take the tiles
// of both stages by ticket (sdfgpu_tickets.hpp); the ticket words live in the status block and the fold clears them with the rest.
int launch_envelope_standby(sdfgpu_handle h, const DcIo& ke2, const DcIo& ke3, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                            const uint32_t* guard, hipStream_t s) {
    if (guard == kUnguarded) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "the single stand-by launch stands behind a guard word (internal)");
    EnvDcArgs ay{}, ax{};
    if (int rc = envelope_args(h, 2, ke2, nx, ny, nz, resolution, vb, guard, ay)) return rc;
    if (int rc = envelope_args(h, 3, ke3, nx, ny, nz, resolution, vb, guard, ax)) return rc;
    if (ke3.fold_ticket) {
        ax.fold_status = h->d_small; ax.fold_result = ke3.fold_result; ax.fold_report = ke3.fold_report; ax.fold_ticket = ke3.fold_ticket;
        ax.fold_report_mask = kReportDense;
    }
    StandbyTickets tk{};
    tk.next = h->d_small + kSwTicketNext; tk.done_y = h->d_small + kSwTicketDoneY; tk.failed = h->d_small + kSwStandbyFailed;
    tk.t2 = (uint32_t)((ay.ntiles + kStandbyRun - 1) / kStandbyRun); tk.t3 = (uint32_t)((ax.ntiles + kStandbyRun - 1) / kStandbyRun);
    if (ay.ntiles + ax.ntiles > 0x7fffffffLL) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "envelope grid too large");
    // an x tile waits for the y sweep at most this long (100 MHz ticks): the y sweep of the largest grid the kernel takes is tens of ms
    tk.budget = 2ull * 100000000ull;
    const bool vec3 = envelope_vector_form(ax);
    const int which = vec3 ? 1 : 0;
    h->last.last_dc_x = (1 + (vec3 ? 2 : 0) + 4) + 1;             // (what the x sweep's own LOOP-form launch would have reported)
    // dynamic LDS: the larger of the two stages' needs (their line lengths differ)
    const size_t lds = std::max(envelope_dc_lds_bytes(ay.L, kDcLines), envelope_dc_lds_bytes(ax.L, kDcLines));
    static void (*const kKernels[2])(const EnvDcArgs, const EnvDcArgs, const StandbyTickets) = {k_envelope_standby<false>, k_envelope_standby<true>};
    if (lds > 64 * 1024 && !h->standby_attr_set[which]) {
        HIP_TRY(h, hipFuncSetAttribute((const void*)kKernels[which], hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDcMaxDynamicLds));
        h->standby_attr_set[which] = true;
    }
    const int64_t nwg = std::min<int64_t>((int64_t)tk.t2 + tk.t3, h->opt.standby_grid);
    hipLaunchKernelGGL(kKernels[which], dim3((unsigned)nwg), dim3(256), lds, s, ay, ax, tk);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// The tier probe of a far-field sweep: counts, on a sample of the sweep's own input, the voxels whose d^2 reaches the axis'
// thresholds into the status block's probe counters; its last workgroup turns them into the tier decision `dec`.  Stores no field.
// The window statistic (k_probe_window) where the thresholds allow it, else the far-field kernel itself on ~256 sampled tiles.
int launch_envelope_probe(sdfgpu_handle h, int stage, const DcIo& io, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                          const uint32_t* guard, const DcDecide& dec, hipStream_t s) {
    EnvDcArgs a{};
    if (int rc = envelope_args(h, stage, io, nx, ny, nz, resolution, vb, guard, a)) return rc;
    uint32_t* const probe_out = h->d_small + kSwProbeFar;
    auto set_decision = [&](auto& args) {                           // what the launch's last workgroup passes to decide_tier
        args.decide_small = h->d_small; args.decide_stage = dec.stage; args.decide_dense_tried = dec.dense_tried ? 1 : 0;
        args.decide_force = h->opt.force_env; args.decide_den = kFarDen[dec.stage]; args.decide_handoff = dec.handoff ? 1 : 0;
        args.decide_mid_den = (dec.stage == 0 && dec.window_choice) ? kMidDenY : 0;
        args.decide_xden = kFarDen[1];
    };
    if (h->opt.probe_window) {
        // thresholds up to 81 = windows up to radius 8
        const int thr = h->opt.far_thr[stage - 2], thr2 = stage == 2 ? kMidThrY : 0, thr3 = stage == 2 ? h->opt.far_thr[1] : 0;
        int W = 0;
        while ((W + 1) * (W + 1) < std::max(thr, std::max(thr2, thr3))) ++W;
        const bool handoff_in = io.i32_flag != nullptr;                 // p16 shape: int32 values only behind the flag, which ends the probe
        const int32_t* in32 = (stage == 3 && io.in_i32 && !handoff_in) ? io.in_i32 : nullptr;
        const int16_t* in16 = in32 ? nullptr : io.in16;
        if (W <= 8 && (in16 || in32)) {
            ProbeArgs pa{};
            pa.in16 = in16; pa.in32 = in32;
            pa.n = nx * ny * nz; pa.ls = a.line_stride; pa.L = a.L; pa.W = W;
            pa.thr = thr; pa.thr2 = thr2; pa.thr3 = thr3;
            pa.nsamples = (uint32_t)std::min<int64_t>(pa.n, 32768);
            pa.step = std::max<int64_t>(1, pa.n / pa.nsamples);
            if (pa.step > 0xffffff) pa.step = 0xffffff;                 // (the kernel hashes the offset inside a stretch in 24 bits)
            pa.probe_out = probe_out; pa.guard = guard; pa.i32_flag = io.i32_flag;
            set_decision(pa);
            const unsigned nb = (pa.nsamples + 255u) / 256u;
            if (stage == 2 && W <= 3) hipLaunchKernelGGL((k_probe_window<2, 3>), dim3(nb), dim3(256), 0, s, pa);
            else if (stage == 2) hipLaunchKernelGGL((k_probe_window<2, 8>), dim3(nb), dim3(256), 0, s, pa);
            else if (W <= 3) hipLaunchKernelGGL((k_probe_window<3, 3>), dim3(nb), dim3(256), 0, s, pa);
            else hipLaunchKernelGGL((k_probe_window<3, 8>), dim3(nb), dim3(256), 0, s, pa);
            HIP_TRY(h, hipGetLastError());
            return SDFGPU_OK;
        }
    }
    // sample ~256 tiles spread over the grid, store nothing
    const int64_t all = a.ntiles;
    a.probe_stride = (int)std::max<int64_t>(1, std::min<int64_t>(64, all / 256));
    a.probe_thr = h->opt.far_thr[stage - 2];
    a.probe_thr2 = stage == 2 ? kMidThrY : 0;
    a.probe_thr3 = stage == 2 ? h->opt.far_thr[1] : 0;
    a.probe_out = probe_out;
    set_decision(a);
    a.ntiles = (all + a.probe_stride - 1) / a.probe_stride;
    while (a.ntiles > 0 && (a.ntiles - 1) * a.probe_stride + ((a.ntiles - 1) * 7) % a.probe_stride >= all) --a.ntiles;
    if (a.ntiles == 0) return launch_decide(h, dec, s);
    return launch_envelope_kernel(h, stage, a, false, true, s);
}

// What stands in front of a sweep whose tier is chosen on the device: probe + decision in one launch (the probe's last workgroup
// decides), or the decision alone when an option forces the tier (nothing to probe).
int launch_probe_or_decide(sdfgpu_handle h, int stage, const DcIo& io, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                           const uint32_t* guard, const DcDecide& dec, hipStream_t s) {
    if (h->opt.force_env < 0) return launch_envelope_probe(h, stage, io, nx, ny, nz, resolution, vb, guard, dec, s);
    return launch_decide(h, dec, s);
}

// K0 + KD: pack to bits, then the bit-parallel ball kernel (sdfgpu_dense.hpp)
constexpr int kBallLanes = 256;                   // lanes per workgroup of KD, KD3, KD6 and KF
constexpr int kDenseMaxRowWords = 64;             // longest z-row the tuned dense kernels take, in 32-voxel words (DenseArgs::nzw)
static_assert(kDenseMaxRowWords <= kBallLanes, "a ball-kernel tile holds at least one z-row: launch_ball_dense divides by kBallLanes / nzw");
bool dense_shape_ok(int64_t nz) {                                // (with or without virtual border: the tuned ball kernel folds it itself)
    const int64_t nzw = nz / 32;
    return (nz % 32) == 0 && nzw >= 1 && nzw <= kDenseMaxRowWords && (nzw & (nzw - 1)) == 0;
}
bool dense_eligible(const sdfgpu_context* h, int64_t nz) { return h->opt.dense_on && dense_shape_ok(nz); }   // (a stage call's test; a whole build's is plan_build's)

// K0: byte mask or cell records -> bits (a bit field needs no packing: callers do not come here with one)
int launch_pack_bits(sdfgpu_handle h, const Occupancy& occ, int64_t n, uint32_t* d_bits, hipStream_t s) {
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    if (occ.cells) {
        hipLaunchKernelGGL(k_pack_bits_generic<CellLoader>, grid, block, 0, s, cell_loader(occ), d_bits, n);
    } else if ((reinterpret_cast<uintptr_t>(occ.mask) % 16) == 0) {
        const int64_t n16 = n / 16;
        const int64_t pb = (int64_t)kBlock * 4;                     // 4 chunks of 16 voxels per lane
        hipLaunchKernelGGL((k_pack_bits_mask<4, true>), dim3((unsigned)((n16 + pb - 1) / pb)), block, 0, s, occ.mask, d_bits, n16);
    } else {
        hipLaunchKernelGGL(k_pack_bits_generic<MaskLoader>, grid, block, 0, s, MaskLoader{occ.mask}, d_bits, n);
    }
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// Folds the per-slot maxima of the final-stage kernels launched so far into d_maxdsq[0..1] and clears the slots.
int fold_slots(sdfgpu_handle h, uint32_t* d_maxdsq, hipStream_t s, uint32_t* result = nullptr, uint32_t* report = nullptr,
               uint32_t report_mask = kReportDense) {
    hipLaunchKernelGGL(k_fold_slots, dim3(1), dim3(kSlots), 0, s, h->d_slots, d_maxdsq, result, report, report_mask);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// KD6 is for scenes with at most 1 / 8 of their voxels undecided behind KD3: Bernoulli p = 0.01 leaves 8 % (0.78 ms against the
// far-field pair's 0.96), p = 0.007 17 % (1.07 ms against 0.97)
constexpr int kShellBudgetDen = 8;

// The ball kernels' level magnitudes, float(sqrt(double(d^2)) * resolution): the 7 levels of KD and the generic kernel (mag[7] = 0:
// not found) and, where asked for, the 13 levels of KD3 (mag3[13..15] = 0).
void fill_ball_magnitudes(double resolution, float (&mag)[8], float* mag3 = nullptr) {
    static const int level3_d2[13] = {1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14};          // (KD's levels are the first seven)
    for (int l = 0; l < 8; ++l) mag[l] = l < 7 ? (float)(std::sqrt((double)level3_d2[l]) * resolution) : 0.0f;
    if (mag3) for (int l = 0; l < 16; ++l) mag3[l] = l < 13 ? (float)(std::sqrt((double)level3_d2[l]) * resolution) : 0.0f;
}

// How launch_ball_dense runs the dense tier.  The defaults are a stage call's: KD alone on a slab without virtual border, raising
// *d_uncert itself for what it cannot decide.
struct BallMode {
    uint32_t* fix_needed = nullptr;  // non-null: fix-up mode -- the ball kernel raises this word instead and hands its undecided voxels to
                                     // KF (behind KD3: to KD6 first), which raises *d_uncert only for what it cannot decide either
    bool early_out = false;          // whole builds: a scene the tier will not certify is left early, the reason goes to the status block
    int vb = 0;                      // virtual border around a grid of nx_glob planes
    int64_t nx_glob = 0;
    int radius = 2;                  // 3: KD3 (sdfgpu_dense3.hpp; whole-grid builds without virtual border only)
    const uint32_t* guard = kUnguarded;
    int flip = 0;                    // KD walks its tiles in the opposite order (option "ball_serpentine")
    uint32_t* unc = nullptr;         // fix-up mode: storage of unc_bytes for the undecided bits (and, if it is large enough, the tile
    size_t unc_bytes = 0;            // flags behind them) in place of the context's own buffers
};

int launch_ball_dense(sdfgpu_handle h, const uint32_t* d_bits, float* d_out, int64_t rows_x, int64_t out_lo, int64_t out_hi,
                      int64_t ny, int64_t nz, double resolution, uint32_t* d_uncert, const BallMode& m, hipStream_t s) {
    const int R = m.radius == 3 ? kBall3R : kBallR;                   // 3: KD3 (sdfgpu_dense3.hpp; whole-grid builds without virtual border only)
    // The ball kernels stage bit rows with 16-byte loads and store 4 floats per lane.  Whole builds come here with the library's own
    // bit field and a 16-byte-aligned field (build_device_impl); the stage entry points pass the caller's pointers, which need
    // element alignment only (sdfgpu.h "Conventions"): planes off 16 bytes are copied into scratch first, and a field off 16 bytes
    // is built in scratch and copied out behind the last kernel.  Both copies are on `s`.
    float* const d_out_caller = d_out;
    const size_t out_bytes = (size_t)(out_hi - out_lo) * (size_t)ny * (size_t)nz * 4;
    const bool out_staged = (reinterpret_cast<uintptr_t>(d_out) % 16) != 0;
    if (out_staged) {
        if (int rc = ensure(h, h->ball_out, out_bytes, "dense stage field (caller's is off 16 bytes)")) return rc;
        d_out = (float*)h->ball_out.ptr;
    }
    if ((reinterpret_cast<uintptr_t>(d_bits) % 16) != 0) {
        const size_t bits_bytes = (size_t)rows_x * (size_t)ny * (size_t)(nz / 32) * 4;
        if (int rc = ensure(h, h->ball_bits, bits_bytes, "dense stage bit planes (caller's are off 16 bytes)")) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->ball_bits.ptr, d_bits, bits_bytes, hipMemcpyDeviceToDevice, s));
        d_bits = (const uint32_t*)h->ball_bits.ptr;
    }
    DenseArgs a{};
    a.early_out = m.early_out ? 1 : 0;
    a.vb = m.vb; a.nx_glob = (int)m.nx_glob;
    a.bits = d_bits; a.out = d_out;
    a.nzw = (int)(nz / 32);
    a.log2_nzw = 0;
    while ((1 << a.log2_nzw) < a.nzw) ++a.log2_nzw;
    a.ny = (int)ny; a.rows_x = (int)rows_x; a.out_lo = (int)out_lo; a.out_hi = (int)out_hi;
    constexpr int bd = kBallLanes;                         // (every caller checks dense_eligible first: nzw <= kDenseMaxRowWords, 4 rows or more per tile)
    const int rows = bd / a.nzw;                           // tile rows per workgroup
    int best_tx = 1, best_ty = rows, best_cost = 1 << 30;
    for (int ty = 1; ty <= rows; ty *= 2) {                // smallest halo-inclusive footprint
        const int tx = rows / ty;
        const int cost = (tx + 2 * R) * (ty + 2 * R);
        if (cost < best_cost || (cost == best_cost && ty > best_ty)) { best_cost = cost; best_tx = tx; best_ty = ty; }
    }
    a.tx = best_tx; a.ty = best_ty;
    a.log2_ty = 0;
    while ((1 << a.log2_ty) < a.ty) ++a.log2_ty;
    a.inv_hy = (65536 + (a.ty + 2 * R) - 1) / (a.ty + 2 * R);
    fill_ball_magnitudes(resolution, a.mag, a.mag3);
    a.slots = h->d_slots; a.uncertified = d_uncert;
    a.reason = m.early_out ? h->d_small + kSwReason : nullptr;                // (whole builds: the context's status block; stage calls have none)
    a.flip = m.radius == 3 ? 0 : m.flip;
    a.guard = m.guard;
    // KD3 gives up at once when a wave holds more undecided voxels than the stage behind it takes: KF's per-tile cap -- or, with
    // the shell pass in between (which turns words, not voxels, around and leaves KF what lies beyond d^2 = 36), three quarters
    // of the wave: the faces of a sparse noise grid, where a voxel sees a fraction of the ball, used to end the tier there
    const bool shell = m.radius == 3 && h->opt.shell_on && m.fix_needed && m.early_out;      // (whole builds: the status block carries the sample)
    a.max_undecided = shell ? 1536 : kBall3MaxUndecided;
    a.und_sample = shell ? h->d_slots : nullptr;
    const int64_t gx = (ny + a.ty - 1) / a.ty, gy = (out_hi - out_lo + a.tx - 1) / a.tx;
    if (gx > 0x7fffffffLL || gy > 65535) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dense grid too large");
    const size_t pitch = a.nzw < 32 ? a.nzw + 32 : a.nzw + 2;        // must match k_ball_dense
    const size_t tile_words = ((size_t)(a.tx + 2 * R) * (a.ty + 2 * R) * pitch + 3) & ~(size_t)3;
    const size_t lds = m.radius == 3 ? tile_words * 4 + (size_t)bd * 20 + 1024 * 8 + 128 : tile_words * 4 + (size_t)bd * 16 + 256 * 8 + 64;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (m.fix_needed) {                                              // fix-up mode: hand the undecided voxels to KF
        const size_t tiles = (size_t)gx * gy;
        // (the undecided bits of a STAGED fix-up stage live in the z field's storage, which the general pipeline only writes
        //  after KF has consumed them: a fresh context's first build does not pay a 17 MB allocation for a stage that a
        //  far-field scene leaves at once)
        if (!m.unc) if (int rc = ensure(h, h->unc, (size_t)(out_hi - out_lo) * ny * a.nzw * 4, "undecided words")) return rc;
        uint32_t* tileflag = nullptr;
        if (m.unc && m.unc_bytes >= (size_t)(out_hi - out_lo) * ny * a.nzw * 4 + 256 + tiles * 4) {
            // ... and so do its tile flags (behind the bits; cleared here: the storage is not ours between builds)
            tileflag = m.unc + ((size_t)(out_hi - out_lo) * ny * a.nzw + 63) / 64 * 64;
            HIP_TRY(h, hipMemsetAsync(tileflag, 0, tiles * 4, s));
        } else {
            if (h->tileflag.bytes < tiles * 4 || !h->tileflag.ptr) {
                if (int rc = ensure(h, h->tileflag, tiles * 4, "tile flags")) return rc;
                HIP_TRY(h, hipMemsetAsync(h->tileflag.ptr, 0, h->tileflag.bytes, s));     // afterwards KF keeps it zero
            }
            tileflag = (uint32_t*)h->tileflag.ptr;
        }
        a.unc = m.unc ? m.unc : (uint32_t*)h->unc.ptr; a.tileflag = tileflag; a.fix_needed = m.fix_needed;
    }
    const bool zinv = nz <= (int64_t)bd * 4;   // an expansion pass covers whole z-rows
    if (m.radius == 3) {
        if (m.vb) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "KD3: grids without virtual border only (internal)");
        // nz = 512 (16 words per row, 4 x 4-row tiles): the instance with compile-time row pitch and halo width (option "dense3_fixed")
        if (zinv && a.nzw == 16 && a.ty == 4 && a.tx == 4 && h->opt.dense3_fixed) hipLaunchKernelGGL((k_ball_dense3<256, true, 16, 4>), grid, dim3(256), lds, s, a);
        else if (zinv) hipLaunchKernelGGL((k_ball_dense3<256, true>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((k_ball_dense3<256, false>), grid, dim3(256), lds, s, a);
    }
    else if (zinv) hipLaunchKernelGGL((k_ball_dense<256, true>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((k_ball_dense<256, false>), grid, dim3(256), lds, s, a);
    if (m.fix_needed) {
        HIP_TRY(h, hipGetLastError());
        if (!h->fix_order.ptr) {                                     // (dx, dy) rows by increasing dx^2 + dy^2, built once
            std::vector<uint32_t> order;
            for (int dx = -kFixR; dx <= kFixR; ++dx)
                for (int dy = -kFixR; dy <= kFixR; ++dy)
                    order.push_back((uint32_t)(dx + kFixR) | ((uint32_t)(dy + kFixR) << 8) | ((uint32_t)(dx * dx + dy * dy) << 16));
            std::stable_sort(order.begin(), order.end(), [](uint32_t x, uint32_t y) { return (x >> 16) < (y >> 16); });
            if (int rc = ensure(h, h->fix_order, order.size() * 4, "fix-up row order")) return rc;
            HIP_TRY(h, hipMemcpy(h->fix_order.ptr, order.data(), order.size() * 4, hipMemcpyHostToDevice));
        }
        // KD6 (round 5): the bit-parallel shell pass 16 <= d^2 <= 36 over the words KD3 left undecided voxels in, in front of KF
        // (which then only sees what lies beyond d^2 = 36) -- sdfgpu_dense6.hpp.  Behind KD3 only: KD's undecided voxels start
        // at d^2 = 9, below the shell.
        if (shell) {
            ShellArgs sa{};
            sa.bits = d_bits; sa.out = d_out; sa.unc = a.unc; sa.tileflag = a.tileflag; sa.fix_needed = m.fix_needed;
            sa.uncertified = d_uncert;
            // budget: 1 / kShellBudgetDen of the voxels undecided behind KD3 (the sample holds 1 / 16 of them; small grids: at least
            // one wave's worth)
            const uint32_t budget = (uint32_t)std::max<int64_t>((out_hi - out_lo) * ny * nz / kShellBudgetDen / 16, 2048);
            hipLaunchKernelGGL(k_shell_budget, dim3(1), dim3(kSlots), 0, s, h->d_slots, m.fix_needed, d_uncert, a.reason, budget);
            sa.nzw = a.nzw; sa.log2_nzw = a.log2_nzw; sa.ny = a.ny; sa.rows_x = a.rows_x; sa.out_lo = a.out_lo; sa.out_hi = a.out_hi;
            sa.tx = a.tx; sa.ty = a.ty; sa.log2_ty = a.log2_ty; sa.resolution = resolution; sa.slots = h->d_slots; sa.min_words = h->opt.shell_min_words;
            const size_t slds = shell_lds_bytes(256, a.tx, a.ty, a.nzw);
            if (slds <= 64 * 1024) {
                const dim3 sgrid((unsigned)((gx + kShellGroup - 1) / kShellGroup), (unsigned)gy);       // kShellGroup tiles (along y) per workgroup
                hipLaunchKernelGGL(k_ball_shell<256>, sgrid, dim3(256), slds, s, sa);
                HIP_TRY(h, hipGetLastError());
            }
        }
        FixArgs f{};
        f.bits = d_bits; f.out = d_out; f.unc = a.unc; f.tileflag = a.tileflag; f.fix_needed = m.fix_needed;
        f.order = (const uint32_t*)h->fix_order.ptr;
        f.nzw = a.nzw; f.log2_nzw = a.log2_nzw; f.ny = a.ny; f.rows_x = a.rows_x; f.out_lo = a.out_lo; f.out_hi = a.out_hi;
        f.tx = a.tx; f.ty = a.ty; f.log2_ty = a.log2_ty; f.resolution = resolution;
        f.slots = h->d_slots; f.uncertified = d_uncert; f.reason = a.reason;
        const size_t flds = (size_t)(2 * kFixOrderPad + kFixCap + 4) * 4 +
                            (size_t)(a.tx + 2 * kFixTileR) * (a.ty + 2 * kFixTileR) * (a.nzw + 2) * 4;
        hipLaunchKernelGGL(k_ball_fixup<256>, grid, dim3(256), flds, s, f);
    }
    HIP_TRY(h, hipGetLastError());
    if (out_staged) HIP_TRY(h, hipMemcpyAsync(d_out_caller, d_out, out_bytes, hipMemcpyDeviceToDevice, s));
    return SDFGPU_OK;
}

// Generic dense tier (any nz, virtual border): k_pack_bits_rows + k_ball_dense_generic.  `rows`: storage for the bit field, every
// z-row padded to whole words (BuildPlan::bits_bytes).
int launch_dense_generic(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                         uint32_t* rows, float* d_out, uint32_t* d_uncert, hipStream_t s) {
    const int64_t nzw = (nz + 31) / 32, nrows = nx * ny, nwords = nrows * nzw;
    if (nwords > 0x7fffffffLL * (int64_t)kBlock) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dense grid too large");
    const dim3 grid((unsigned)((nwords + kBlock - 1) / kBlock)), block(kBlock);
    if (occ.bits)                                               // (linear bits -> rows padded to whole words)
        hipLaunchKernelGGL(k_pack_bits_rows<BitsLoader>, grid, block, 0, s, BitsLoader{occ.bits}, rows, nrows, (int)nz, (int)nzw);
    else if (occ.cells)
        hipLaunchKernelGGL(k_pack_bits_rows<CellLoader>, grid, block, 0, s, cell_loader(occ), rows, nrows, (int)nz, (int)nzw);
    else
        hipLaunchKernelGGL(k_pack_bits_rows<MaskLoader>, grid, block, 0, s, MaskLoader{occ.mask}, rows, nrows, (int)nz, (int)nzw);
    HIP_TRY(h, hipGetLastError());
    DenseGenArgs a{};
    a.bits = rows; a.out = d_out;
    a.nx = (int)nx; a.ny = (int)ny; a.nz = (int)nz; a.nzw = (int)nzw; a.vb = vb;
    fill_ball_magnitudes(resolution, a.mag);
    a.slots = h->d_slots; a.uncertified = d_uncert;
    hipLaunchKernelGGL(k_ball_dense_generic, grid, block, 0, s, a);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// ---- a whole build: plan (sdfgpu_plan.hpp), allocate, enqueue ---------------------------------------------------------------------

// Profiling marks of one build: eight event slots (start, after pack, ball, K1, K2 / K12, KE2, K3, KE3), seven intervals for
// sdfgpu_get_stage_times.  An event is recorded only behind a stage that launched something; a stage that launched nothing shares
// the previous mark (elapsed 0), so profiling adds as few packets as possible.  Events come from the handle's pool.
struct StageMarks {
    sdfgpu_handle h;
    hipStream_t s;
    int prof = 0;                    // 0 off, 1 every stage, 2 only the dominant kernel of the dense path: stage 1 = [ev1, ev2], every
                                     // other stage shares a mark with its neighbour (builds without the dense tier: like 1)
    bool dense = false;
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool launched_since_mark = true;

    StageMarks(sdfgpu_handle h_, hipStream_t s_, bool dense_) : h(h_), s(s_), prof(h_->profiling), dense(dense_) {
        // level 3 = level 2 on every 4th build (a sampled timing costs the loop a quarter of the event overhead)
        if (prof == 3) prof = ((h->profiled_builds++ & 3u) == 0 && dense) ? 2 : 0;
    }
    void launched() { launched_since_mark = true; }
    hipError_t mark(int k) {
        if (!prof) return hipSuccess;
        if (prof == 2 && dense) {
            if (k == 0) return hipSuccess;
            if (k > 2) { ev[k] = ev[k - 1]; return hipSuccess; }
        } else if (k > 0 && !launched_since_mark) {
            ev[k] = ev[k - 1];
            return hipSuccess;
        }
        if (h->event_pool.empty()) {
            hipError_t e = hipEventCreate(&ev[k]);
            if (e != hipSuccess) return e;
        } else {
            ev[k] = h->event_pool.back();
            h->event_pool.pop_back();
        }
        if (k == 1 && ev[0] == nullptr) ev[0] = ev[1];
        launched_since_mark = false;
        return hipEventRecord(ev[k], s);
    }
    hipError_t finish() {                                        // the last mark; the build's events go to the handle
        if (!prof) return hipSuccess;
        const hipError_t e = mark(7);
        if (e == hipSuccess) for (auto x : ev) h->events.push_back(x);
        return e;
    }
};

// What the stages of one build share: the grid, the caller's buffers, the handle's scratch fields (allocated before the first
// launch) and the device words that steer the launches.
struct BuildIo {
    const Occupancy& occ;
    int64_t nx, ny, nz;
    double resolution;
    int vb;
    float* d_out;
    hipStream_t s;
    uint32_t* sw;                    // the status block, indexed by StatusWord
    const uint32_t* general_guard;   // what guards every launch of the general pipeline: "the dense tier left voxels undecided"
    int16_t* zf;                     // z field
    int32_t* yz;                     // int32 plane field / side table
    int16_t* p16;                    // 16-bit plane field (BuildPlan::p16)
    const uint32_t* dense_bits;      // the bit field the dense kernels (and the stand-by y sweep) read
    uint8_t* row_any;                // plane sparsity: one byte per z row, one per x-plane behind them (BuildPlan::plane_skip)
};

// What plan_build needs and only this unit can know, but for the report slots (nx, ny, nz: canonical)
BuildFacts shape_and_pointer_facts(const sdfgpu_context* h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, int vb, const float* d_out) {
    // (the caller's pointers need element alignment only, sdfgpu.h "Conventions")
    auto aligned16 = [](const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) % 16) == 0; };
    BuildFacts f;
    f.nx = nx; f.ny = ny; f.nz = nz; f.vb = vb != 0;
    f.occ = occ.bits ? BuildFacts::Occ::bits : occ.cells ? BuildFacts::Occ::cells : BuildFacts::Occ::mask;
    f.occ16 = aligned16(occ.bits ? (const void*)occ.bits : occ.cells ? occ.cells : (const void*)occ.mask);
    f.out16 = aligned16(d_out);
    f.dense_shape = dense_shape_ok(nz);
    f.far_shape[0] = far_geometry_ok(h, 2, nx, ny, nz); f.far_shape[1] = far_geometry_ok(h, 3, nx, ny, nz);
    f.z_wave_shape = z_wave16_shape(h, nz);
    f.fused_nz = fused_zy_nz(nz);
    return f;
}

// Learn from an earlier build on this handle, if its status block has arrived (never a wait): sdfgpu_policy.hpp.  Every
// outcome is exact; the policy only decides whether and in which form the DENSE tier is enqueued and whether the pipeline
// behind it may be the two-launch stand-by (which tier does a sweep is decided on the device inside the build).
void consume_arrived_reports(sdfgpu_handle h) {
    if (h->flags_pending && hipEventQuery(h->flags_ev) == hipSuccess) {
        h->flags_pending = false;
        //   (a staged build -- KD, then KD3 + KF on KD's verdict -- reports KD's own verdict, kSwDenseVerdict, as word kSwReportVerdict)
        h->pol.consume_report(h->h_flags[kSwUncertified] != 0, h->h_flags[kSwFixNeeded] != 0, h->h_flags[kSwReportVerdict] != 0);
        // (a predicted build's flags are raised by the launches themselves: they teach the habit nothing, and a near-field scene would
        //  keep a stale "far" alive through them -- ADVICE r5)
        if (!h->pol.prev.predicted) h->far.consume_report(h->h_flags[kSwFarY] != 0, h->h_flags[kSwFarX] != 0);
    }
    if (h->far_pending && hipEventQuery(h->far_ev) == hipSuccess) {
        h->far_pending = false;
        h->far.consume_report(h->h_far[kSwFarY] != 0, h->h_far[kSwFarX] != 0);
    }
}

// The dense tier, with the profiling mark between its bit field and its kernels: generic, or KD (KD3 in fix-up mode) with KD3 + KF
// staged behind it.  Exact wherever the nearest opposite voxel is within d^2 <= 8; raises kSwUncertified otherwise.
int enqueue_dense_tier(sdfgpu_handle h, const BuildPlan& p, const BuildIo& b, StageMarks& marks) {
    const int64_t n = b.nx * b.ny * b.nz;
    uint32_t* const sw = b.sw;
    if (p.bits == BuildPlan::Bits::copy) {                      // (the dense kernels stage bit rows with 16-byte loads)
        HIP_TRY(h, hipMemcpyAsync(h->bits.ptr, b.occ.bits, (size_t)n / 8, hipMemcpyDeviceToDevice, b.s));
    } else if (p.bits == BuildPlan::Bits::pack) {
        if (int rc = launch_pack_bits(h, b.occ, n, (uint32_t*)h->bits.ptr, b.s)) return rc;
        marks.launched();
    }
    HIP_TRY(h, marks.mark(1));
    if (!p.dense) return SDFGPU_OK;
    if (p.dense_generic) {
        if (int rc = launch_dense_generic(h, b.occ, b.nx, b.ny, b.nz, b.resolution, b.vb, (uint32_t*)h->bits.ptr, b.d_out, sw + kSwUncertified, b.s)) return rc;
        marks.launched();
        return SDFGPU_OK;
    }
    // fix-up mode (policy): undecided voxels go to the fix-up kernel, which raises `uncertified` only for what it
    // cannot decide either; otherwise the ball kernel raises it directly and nothing extra is launched
    // (with a virtual border the fix-up kernel stays out: a voxel it would finish may still be bound by b >= 3)
    // (fix-up mode, KD3 in KD's place, the fix-up stage staged behind KD: DensePolicy::plan)
    BallMode kd;
    kd.early_out = true; kd.vb = b.vb; kd.nx_glob = b.nx; kd.radius = p.tier.dense3 ? 3 : 2;
    if (p.tier.fix_mode_build()) kd.fix_needed = sw + kSwFixNeeded;
    if (!p.tier.dense3) {                                       // (KD; see ball_serpentine)
        kd.flip = (h->opt.ball_serpentine && b.d_out == h->serp_out && n == h->serp_n) ? !h->serp_flip : 0;
        h->serp_out = b.d_out; h->serp_n = n; h->serp_flip = kd.flip;
    }
    if (int rc = launch_ball_dense(h, b.dense_bits, b.d_out, b.nx, 0, b.nx, b.ny, b.nz, b.resolution,
                                   p.tier.staged ? sw + kSwDenseVerdict : sw + kSwUncertified, kd, b.s)) return rc;
    if (p.tier.staged) {                                        // KD3 + KF behind KD, guarded on its verdict
        BallMode kd3;
        kd3.early_out = true; kd3.nx_glob = b.nx; kd3.radius = 3; kd3.fix_needed = sw + kSwFixNeeded; kd3.guard = sw + kSwDenseVerdict;
        // (the undecided bits of this stage live in the z field's storage: launch_ball_dense.  Every build that sweeps z has
        //  allocated the field by now, so the stage finds it on a fresh context too)
        if (!p.fused && h->zfield.ptr && h->zfield.bytes >= (size_t)n / 8) { kd3.unc = (uint32_t*)h->zfield.ptr; kd3.unc_bytes = h->zfield.bytes; }
        if (int rc = launch_ball_dense(h, b.dense_bits, b.d_out, b.nx, 0, b.nx, b.ny, b.nz, b.resolution, sw + kSwUncertified, kd3, b.s)) return rc;
    }
    marks.launched();
    return SDFGPU_OK;
}

// K1, unless the build's y sweep computes the z distances itself (K12; the stand-by pair reads the bit field)
int enqueue_z_sweep(sdfgpu_handle h, const BuildPlan& p, const BuildIo& b, StageMarks& marks) {
    if (!p.z_sweep()) return SDFGPU_OK;
    if (int rc = launch_sweep_z(h, b.occ, b.nx, b.ny, b.nz, b.zf, b.general_guard, b.s, b.row_any)) return rc;
    marks.launched();
    return SDFGPU_OK;
}

// Stand-by and predicted builds: KE2 [general guard] -> KE3 [general guard], exact int32 plane values in between, each launch
// raising its far flag itself: no probes, no marching launches.
int enqueue_far_pair(sdfgpu_handle h, const BuildPlan& p, const BuildIo& b, StageMarks& marks) {
    const int64_t nx = b.nx, ny = b.ny, nz = b.nz;
    uint32_t* const sw = b.sw;
    DcIo ke2, ke3;
    ke2.out_i32 = b.yz; ke2.ran_flag = sw + kSwFarY;
    ke3.in_i32 = b.yz; ke3.out = b.d_out; ke3.ran_flag = sw + kSwFarX;
    if (p.standby) {                                            // LOOP form, z distances from the dense tier's bit field, self-reporting
        ke2.loop = ke3.loop = true;
        ke2.bits = b.dense_bits; ke2.nzw = (int)((nz + 31) / 32);
        if (p.standby_folds) {
            ke3.fold_result = h->d_result; ke3.fold_report = p.report == BuildPlan::Report::dense ? h->h_flags_dev : nullptr;
            ke3.fold_ticket = sw + kSwFoldTicket;
        }
    } else {
        ke2.in16 = b.zf;
        if (b.row_any) {
            // row bytes -> one bit per row, one byte per x-plane, "some plane is empty" (kSwPlaneEmpty)
            uint8_t* plane_any = b.row_any + nx * ny;
            uint32_t* row_bits = (uint32_t*)(b.row_any + plane_row_bits_offset(nx, ny));
            const int row_words = (int)((ny + 31) / 32);
            if (h->flat_score_reset) { h->flat_score_reset = false; HIP_TRY(h, hipMemsetAsync(sw + kSwFlatScore, 0, 8, b.s)); }
            hipLaunchKernelGGL(k_pack_row_flags, dim3((unsigned)std::min<int64_t>((nx + 15) / 16, 16)), dim3(1024), 0, b.s, b.row_any, (int)nx, (int)ny, row_words, row_bits, plane_any, sw + kSwPlaneEmpty, sw + kSwFlatScore);
            HIP_TRY(h, hipGetLastError());
            ke2.row_bits = row_bits; ke2.row_words = row_words; ke2.plane_any = ke3.plane_any = plane_any;
        }
    }
    HIP_TRY(h, marks.mark(4));                                  // (stage slot 3, the marching y sweep: nothing launched)
    if (p.standby_single) {
        // ONE launch: its time goes to the y-envelope slot, the x-envelope slot shares its mark
        if (int rc = launch_envelope_standby(h, ke2, ke3, nx, ny, nz, b.resolution, b.vb, b.general_guard, b.s)) return rc;
        marks.launched();
        HIP_TRY(h, marks.mark(5));
        HIP_TRY(h, marks.mark(6));
        return SDFGPU_OK;
    }
    if (int rc = launch_envelope(h, 2, ke2, nx, ny, nz, b.resolution, b.vb, b.general_guard, b.s)) return rc;
    marks.launched();
    HIP_TRY(h, marks.mark(5));
    HIP_TRY(h, marks.mark(6));                                  // (stage slot 5, the marching x sweep: nothing launched)
    if (int rc = launch_envelope(h, 3, ke3, nx, ny, nz, b.resolution, b.vb, b.general_guard, b.s)) return rc;
    marks.launched();
    return SDFGPU_OK;
}

// Every other build.  A probe-selected one (`select`): per axis a probe that decides, the marching sweep behind its guard word with
// bounded scans, and the far-field sweep behind the axis' far flag.  The rest: one sweep per axis (K12 for z and y where the plan
// says so), unbounded scans, no far flag.
int enqueue_swept_axes(sdfgpu_handle h, const BuildPlan& p, const BuildIo& b, StageMarks& marks) {
    const int64_t nx = b.nx, ny = b.ny, nz = b.nz;
    uint32_t* const sw = b.sw;
    void* const zy_out = p.p16 ? (void*)b.p16 : (void*)b.yz;
    int32_t* const zy_side = p.p16 ? b.yz : kNoSideTable;
    uint32_t* const far_y = p.select ? sw + kSwFarY : kUnbounded;
    uint32_t* const far_x = p.select ? sw + kSwFarX : kUnbounded;
    // the far-field pair: p16 + side table in between, or exact int32 values (always on shapes without the 16-bit plane
    // field; behind kSwHandoff on the others)
    DcIo ke2, ke3;
    ke2.in16 = b.zf; ke3.out = b.d_out;
    if (p.p16) { ke2.out = b.p16; ke2.side_out = b.yz; ke3.in16 = b.p16; ke3.side_in = b.yz; }
    if (!p.p16 || p.handoff) { ke2.out_i32 = b.yz; ke3.in_i32 = b.yz; }
    if (p.p16 && p.handoff) ke2.i32_flag = ke3.i32_flag = sw + kSwHandoff;
    DcIo probe2;                                                // the y probe reads what KE2 reads (no hand-off flag: its own decision raises it)
    probe2.in16 = b.zf; probe2.out = b.p16; probe2.side_out = b.yz;
    if (!p.p16) probe2.out_i32 = b.yz;
    DcDecide dy, dx;
    dy.stage = 0; dx.stage = 1;
    dy.dense_tried = dx.dense_tried = p.dense; dy.handoff = dx.handoff = p.handoff; dy.window_choice = dx.window_choice = p.window_choice;
    XSlab whole = XSlab::whole(nx);
    whole.status = sw + kSwSlabStatus;
    // y sweep
    if (p.select) {
        if (int rc = launch_probe_or_decide(h, 2, probe2, nx, ny, nz, b.resolution, b.vb, b.general_guard, dy, b.s)) return rc;
        // marching y sweep: general pipeline needed AND near-field; the probe also picks the window (radius 3 / radius 8)
        if (int rc = launch_sweep_y(h, b.zf, zy_out, zy_side, nx, ny, nz, sw + kSwMarchY, far_y, b.s)) return rc;
        if (p.window_choice)
            if (int rc = launch_sweep_y(h, b.zf, zy_out, zy_side, nx, ny, nz, sw + kSwMarchYWide, far_y, b.s, YWindow::r8)) return rc;
    } else if (p.fused) {
        if (int rc = launch_sweep_zy_fused(h, b.occ.mask, zy_out, zy_side, nx, ny, nz, b.general_guard, b.s)) return rc;
    } else {                                                    // (no far-field kernel for this shape / switched off: unbounded scans)
        if (int rc = launch_sweep_y(h, b.zf, zy_out, zy_side, nx, ny, nz, b.general_guard, kUnbounded, b.s)) return rc;
    }
    marks.launched();
    HIP_TRY(h, marks.mark(4));
    if (p.select) {
        if (int rc = launch_envelope(h, 2, ke2, nx, ny, nz, b.resolution, b.vb, sw + kSwFarY, b.s)) return rc;
        marks.launched();
    }
    HIP_TRY(h, marks.mark(5));
    // x sweep: same choice
    if (p.select) if (int rc = launch_probe_or_decide(h, 3, ke3, nx, ny, nz, b.resolution, b.vb, b.general_guard, dx, b.s)) return rc;
    const uint32_t* const march_x_guard = p.select ? sw + kSwMarchX : b.general_guard;
    if (p.p16) {
        if (int rc = launch_sweep_x16(h, b.p16, b.yz, b.d_out, whole, ny, nz, b.resolution, b.vb, march_x_guard, far_x, b.s)) return rc;
    } else {
        if (int rc = launch_sweep_x(h, b.yz, b.d_out, whole, ny, nz, b.resolution, b.vb, march_x_guard, far_x, b.s)) return rc;
    }
    marks.launched();
    HIP_TRY(h, marks.mark(6));
    if (p.select) {
        if (int rc = launch_envelope(h, 3, ke3, nx, ny, nz, b.resolution, b.vb, sw + kSwFarX, b.s)) return rc;
        marks.launched();
    }
    return SDFGPU_OK;
}

}  // namespace

// (declared in sdfgpu_context.hpp: the families' host code builds SDFs through it)
int sdfgpu::build_device_impl(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                              float* d_out, hipStream_t s) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (occ.null() || !d_out) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
    if (occ.bits && (reinterpret_cast<uintptr_t>(occ.bits) % 4) != 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "the bit field must be 4-byte aligned");
    if (int rc = check_resolution(h, resolution)) return rc;
    if (int rc = check_dims(h, nx, ny, nz)) return rc;
    if (occ.cells) if (int rc = check_cell_layout(h, occ.stride, occ.off)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    canonical_dims(nx, ny, nz);
    h->last.last_dc_x = 0;                                      // (the far-field launchers of this build write it)
    h->last.last_lines_tiered = false;
    BuildFacts f = shape_and_pointer_facts(h, occ, nx, ny, nz, vb, d_out);
    consume_arrived_reports(h);
    f.dense_slot_free = h->h_flags_dev && !h->flags_pending;
    f.far_slot_free = h->h_far_dev && !h->far_pending;
    const BuildPlan p = plan_build(h->opt, h->pol, h->far, f);
    // every scratch field of the build: nothing has been enqueued when an allocation fails
    if (int rc = ensure(h, h->yzfield, p.yz_bytes, "int32 plane field / side table")) return rc;
    if (p.plane16_bytes) if (int rc = ensure(h, h->plane16, p.plane16_bytes, "16-bit plane field")) return rc;
    if (p.z_bytes) if (int rc = ensure(h, h->zfield, p.z_bytes, "z field")) return rc;
    if (p.bits_bytes) if (int rc = ensure(h, h->bits, p.bits_bytes, "bit field")) return rc;
    if (p.unc_bytes) if (int rc = ensure(h, h->unc, p.unc_bytes, "undecided words")) return rc;
    if (p.planebits_bytes) if (int rc = ensure(h, h->planebits, p.planebits_bytes, "row / x-plane occupancy flags")) return rc;
    // Builds on one handle share its status block, extrema slots and scratch fields.  On the same stream they are
    // ordered by the stream; a build issued on ANOTHER stream first waits for the previous build's last kernel.
    HIP_TRY(h, h->build_order.wait(s));
    // status block: maxima, status, uncertified, far flags, fix_needed.  Normally still zero from the previous
    // build's fold kernel; cleared here after a build that failed half-way (or before the first one)
    if (!h->small_clean) {
        HIP_TRY(h, hipMemsetAsync(h->d_small, 0, 128, s));
        HIP_TRY(h, hipMemsetAsync(h->d_slots, 0, (size_t)kSlots * kSlotWords * 4, s));   // a failed build may have left maxima behind
    }
    h->small_clean = false;
    uint32_t* const sw = h->d_small;
    const BuildIo b{occ, nx, ny, nz, resolution, vb, d_out, s, sw,
                    p.dense ? sw + kSwUncertified : kUnguarded,
                    (int16_t*)h->zfield.ptr, (int32_t*)h->yzfield.ptr, (int16_t*)h->plane16.ptr,
                    p.bits == BuildPlan::Bits::caller ? occ.bits : (const uint32_t*)h->bits.ptr,
                    p.plane_skip ? (uint8_t*)h->planebits.ptr : nullptr};
    StageMarks marks(h, s, p.dense);
    HIP_TRY(h, marks.mark(0));
    if (int rc = enqueue_dense_tier(h, p, b, marks)) return rc;
    HIP_TRY(h, marks.mark(2));
    if (int rc = enqueue_z_sweep(h, p, b, marks)) return rc;
    HIP_TRY(h, marks.mark(3));
    if (int rc = p.far_pair() ? enqueue_far_pair(h, p, b, marks) : enqueue_swept_axes(h, p, b, marks)) return rc;
    // one kernel folds the maxima, publishes the status block (device copy for get_extrema, pinned host copy for the
    // next build's policy) and clears it for the next build -- unless the stand-by x sweep's launch has done it.  What the
    // reported build was (dense? fix-up? predicted?) is remembered with the report -- not with whatever build happens to be
    // the latest when it is read.
    const bool report = p.report == BuildPlan::Report::dense, report_far = p.report == BuildPlan::Report::far;
    if (!p.standby_folds) if (int rc = fold_slots(h, h->d_small, s, h->d_result, report ? h->h_flags_dev : report_far ? h->h_far_dev : nullptr,
                                                  report ? kReportDense : kReportFar)) return rc;
    if (report_far) {
        HIP_TRY(h, hipEventRecord(h->far_ev, s));
        h->far_pending = true;
    }
    h->small_clean = true;
    if (report) {
        HIP_TRY(h, hipEventRecord(h->flags_ev, s));
        h->flags_pending = true;
        h->pol.prev = ReportedBuild{p.dense, p.dense_generic, p.tier.fix_mode_build(), p.tier.staged, p.predicted};
    }
    HIP_TRY(h, marks.finish());
    HIP_TRY(h, h->build_order.record(s));
    LastBuild& last = h->last;
    last.last_dense = p.dense; last.last_dense3 = p.tier.dense3; last.last_staged = p.tier.staged;
    last.last_fused = p.fused; last.last_standby = p.standby; last.last_standby_single = p.standby_single;
    last.last_predicted = p.predicted; last.last_plane16 = p.p16; last.last_plane_skip = p.plane_skip;
    last.last_dims[0] = nx; last.last_dims[1] = ny; last.last_dims[2] = nz;
    last.last_stream = s;
    last.last_resolution = resolution;
    last.last_n = nx * ny * nz;
    last.have_result = true;
    return SDFGPU_OK;
}

namespace {

// `occ` is host memory (occ.bits: the caller's occupancy is already one bit per voxel, sdfgpu_build_bits).
// d_out_user != nullptr: the field stays on the device in the caller's buffer (no download; out_sdf is unused)
int build_host_impl(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb, float* out_sdf,
                    double* out_max, double* out_min, float* d_out_user = nullptr) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (occ.null() || (!out_sdf && !d_out_user)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = check_resolution(h, resolution)) return rc;                  // (before the upload: nothing is enqueued for a refused call)
    if (int rc = check_dims(h, nx, ny, nz)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t n = nx * ny * nz;
    const size_t in_bytes = occ.cells ? (size_t)n * occ.stride : (size_t)n;
    h->tag_cached_bytes = 0;                        // (every host-buffer build, also one whose input goes up as bits and leaves stage_in alone)
    // Round 5: the host's thread team classifies the caller's buffer into one bit per voxel while it fills the pinned staging
    // chunk, and 1/8 B per voxel crosses PCIe (16 MiB at 512^3 instead of 128 MiB of mask or 1 GiB of COLLISION_CELL records);
    // k_unpack_bits_mask spreads them into the byte mask on the device.  Same predicate as the device classifier
    // (pack_cells_bits); "host_pack" = 0 keeps the upload-and-classify-on-device path (device-resident cells always take it).
    const bool packed = !occ.bits && (h->opt.host_pack == 2 || (h->opt.host_pack == 1 && in_bytes >= kPinMin));
    if (!packed && !occ.bits) if (int rc = stage_input(h, in_bytes)) return rc;
    if (!d_out_user) if (int rc = ensure(h, h->stage_out, (size_t)n * 4, "output staging")) return rc;
    float* const d_out = d_out_user ? d_out_user : (float*)h->stage_out.ptr;
    const bool timing = getenv("SDFGPU_HOST_TIMING") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t1 = now();
    // (out_sdf is scratch from here on: include/sdfgpu.h documents that its contents are undefined when the call fails)
    // (round 6: the uploaded bits ARE the build's input -- no byte mask is spread out on the device and packed again by K0)
    if (packed) { if (int rc0 = upload_packed(h, occ, n, kNullStream)) return rc0; }
    else if (occ.bits) { if (int rc0 = upload_bits(h, occ.bits, n, kNullStream)) return rc0; }
    else if (int rc0 = copy_from_host(h, h->stage_in.ptr, occ.cells ? occ.cells : (const void*)occ.mask, in_bytes)) return rc0;
    // what the upload left on the device (read the staging pointers behind it: the upload may have allocated them)
    const Occupancy d_occ = (packed || occ.bits) ? Occupancy::of_bits((const uint32_t*)h->stage_bits.ptr)
                            : occ.cells ? Occupancy::of_cells(h->stage_in.ptr, occ.stride, occ.off, occ.unknown)
                                        : Occupancy::of_mask((const uint8_t*)h->stage_in.ptr);
    const double t2 = now();
    int rc = build_device_impl(h, d_occ, nx, ny, nz, resolution, vb, d_out, kNullStream);
    if (rc) return rc;
    const double t3 = now();
    if (!d_out_user) if (int rc2 = copy_to_host(h, out_sdf, h->stage_out.ptr, (size_t)n * 4)) return rc2;
    const double t5 = now();
    double mx, mn;
    rc = sdfgpu_get_extrema(h, &mx, &mn);
    if (timing) fprintf(stderr, "[sdfgpu host] h2d %.3f enqueue %.3f build + d2h %.3f extrema %.3f ms\n", t2 - t1, t3 - t2, t5 - t3, now() - t5);
    if (rc) return rc;
    if (out_max) *out_max = mx;
    if (out_min) *out_min = mn;
    return SDFGPU_OK;
}

}  // namespace

// records in stage_in -> SDF in stage_out (float), the virtual-border or the free-and-named-objects form
// (called from sdfgpu_convex.hip; here because it launches k_classify_tagged and builds SDFs)
int sdfgpu::convex_sdf(sdfgpu_handle h, size_t stride, size_t occ_off, size_t obj_off, int64_t nx, int64_t ny, int64_t nz, double resolution,
                       int add_virtual_border) {
    const int64_t n = nx * ny * nz;
    auto classify = [&](int mode) {
        hipLaunchKernelGGL(k_classify_tagged, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                           (const char*)h->stage_in.ptr, (int64_t)stride, (int64_t)occ_off, (int64_t)obj_off, 1, mode,
                           (const uint32_t*)h->tagids.ptr, 0, n, (uint8_t*)h->tagmask.ptr);
        return hipGetLastError();
    };
    // ExtractSignedDistanceField(+inf, {}, true, true): every filled cell (an empty id list is "any object", :826)
    HIP_TRY(h, classify(0));
    const Occupancy tagged = Occupancy::of_mask((const uint8_t*)h->tagmask.ptr);
    if (int rc = build_device_impl(h, tagged, nx, ny, nz, resolution, add_virtual_border ? 1 : 0, (float*)h->stage_out.ptr, kNullStream))
        return rc;
    if (add_virtual_border) return SDFGPU_OK;
    // ExtractFreeAndNamedObjectsSignedDistanceField(+inf, true): the free-space SDF above, the named-object SDF, combined as the
    // host does it (tagged_object_collision_map.hpp)
    HIP_TRY(h, classify(1));
    const int no_border = 0;
    if (int rc = build_device_impl(h, tagged, nx, ny, nz, resolution, no_border, (float*)h->cx_field.ptr, kNullStream))
        return rc;
    HIP_TRY(h, cx_combine((float*)h->stage_out.ptr, (const float*)h->cx_field.ptr, (uint64_t)n, nullptr));
    return SDFGPU_OK;
}

extern "C" {

int sdfgpu_build(sdfgpu_handle h, const uint8_t* filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                 int add_virtual_border, float* out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        return build_host_impl(h, Occupancy::of_mask(filled), nx, ny, nz, resolution, add_virtual_border, out_sdf, out_max, out_min);
    });
}

int sdfgpu_build_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset,
                       int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                       int add_virtual_border, float* out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cells is null");
        if (int rc = check_cell_layout(h, cell_stride, occupancy_offset)) return rc;
        return build_host_impl(h, Occupancy::of_cells(cells, cell_stride, occupancy_offset, unknown_is_filled), nx, ny, nz,
                               resolution, add_virtual_border, out_sdf, out_max, out_min);
    });
}

int sdfgpu_build_to_device(sdfgpu_handle h, const uint8_t* filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                           int add_virtual_border, float* d_out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!d_out_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_out_sdf is null");
        float* const no_host_field = nullptr;
        return build_host_impl(h, Occupancy::of_mask(filled), nx, ny, nz, resolution, add_virtual_border, no_host_field, out_max, out_min,
                               d_out_sdf);
    });
}

int sdfgpu_build_cells_to_device(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset,
                                 int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 int add_virtual_border, float* d_out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cells is null");
        if (!d_out_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_out_sdf is null");
        if (int rc = check_cell_layout(h, cell_stride, occupancy_offset)) return rc;
        float* const no_host_field = nullptr;
        return build_host_impl(h, Occupancy::of_cells(cells, cell_stride, occupancy_offset, unknown_is_filled), nx, ny, nz, resolution,
                               add_virtual_border, no_host_field, out_max, out_min, d_out_sdf);
    });
}

int sdfgpu_build_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t nx, int64_t ny, int64_t nz,
                        double resolution, int add_virtual_border, float* d_out_sdf, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_filled) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_filled is null");
        return build_device_impl(h, Occupancy::of_mask(d_filled), nx, ny, nz, resolution, add_virtual_border, d_out_sdf, (hipStream_t)stream);
    });
}

int sdfgpu_build_cells_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset,
                              int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              int add_virtual_border, float* d_out_sdf, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_cells is null");
        return build_device_impl(h, Occupancy::of_cells(d_cells, cell_stride, occupancy_offset, unknown_is_filled), nx, ny, nz,
                                 resolution, add_virtual_border, d_out_sdf, (hipStream_t)stream);
    });
}

int sdfgpu_build_bits_device(sdfgpu_handle h, const uint32_t* d_bits, int64_t nx, int64_t ny, int64_t nz,
                             double resolution, int add_virtual_border, float* d_out_sdf, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_bits) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_bits is null");
        return build_device_impl(h, Occupancy::of_bits(d_bits), nx, ny, nz, resolution, add_virtual_border, d_out_sdf, (hipStream_t)stream);
    });
}

int sdfgpu_build_bits(sdfgpu_handle h, const uint32_t* bits, int64_t nx, int64_t ny, int64_t nz, double resolution,
                      int add_virtual_border, float* out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!bits) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "bits is null");
        return build_host_impl(h, Occupancy::of_bits(bits), nx, ny, nz, resolution, add_virtual_border, out_sdf, out_max, out_min);
    });
}

int sdfgpu_upload_classified(sdfgpu_handle h, const uint8_t* filled, const void* cells, size_t cell_stride, size_t occupancy_offset,
                             int unknown_is_filled, int64_t n, uint8_t* d_mask, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if ((!filled && !cells) || !d_mask) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (n <= 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "voxel count must be positive");
        if (cells) if (int rc = check_cell_layout(h, cell_stride, occupancy_offset)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const Occupancy occ = cells ? Occupancy::of_cells(cells, cell_stride, occupancy_offset, unknown_is_filled) : Occupancy::of_mask(filled);
        if (int rc = upload_packed(h, occ, n, (hipStream_t)stream)) return rc;
        // bits -> the caller's byte mask, stream-ordered behind the upload
        const int64_t nch = (n + 15) / 16;
        hipLaunchKernelGGL(k_unpack_bits_mask, dim3((unsigned)((nch + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                           (const uint32_t*)h->stage_bits.ptr, d_mask, n);
        HIP_TRY(h, hipGetLastError());
        return SDFGPU_OK;
    });
}

int sdfgpu_extrema_from_dsq(uint32_t max_dsq_free, uint32_t max_dsq_filled, double resolution, double* out_max,
                            double* out_min) {
    if (!(resolution > 0.0) || !std::isfinite(resolution)) return SDFGPU_ERR_INVALID_ARGUMENT;     // (no handle: the code only; outputs untouched)
    const double inf = std::numeric_limits<double>::infinity();
    // sdf_generation.hpp:246-269: max is attained on a free voxel, min on a filled one;
    // an absent class leaves the running value at its -inf / +inf start or at the
    // other class's infinite distance (all-free -> (inf, inf); all-filled -> (-inf, -inf)).
    double mx, mn;
    if (max_dsq_free == 0) mx = -inf;
    else if (max_dsq_free >= (uint32_t)kInf32) mx = inf;
    else mx = std::sqrt((double)max_dsq_free) * resolution;
    if (max_dsq_filled == 0) mn = inf;
    else if (max_dsq_filled >= (uint32_t)kInf32) mn = -inf;
    else mn = 0.0 - std::sqrt((double)max_dsq_filled) * resolution;
    if (out_max) *out_max = mx;
    if (out_min) *out_min = mn;
    return SDFGPU_OK;
}

namespace {
// The single stand-by launch bounds the wait of its x tiles for its y sweep (k_envelope_standby).  A build in which that bound ran
// out has left a field that is not valid: every read of the build's status block says so.
int standby_failed(sdfgpu_handle h, const uint32_t* status) {
    if (status[kSwStandbyFailed] == 0u) return SDFGPU_OK;
    return fail(h, SDFGPU_ERR_HIP, "the stand-by launch of the last build gave up waiting for its y sweep: the field of that build is not valid");
}
}  // namespace

int sdfgpu_get_extrema(sdfgpu_handle h, double* out_max, double* out_min) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!h->last.have_result) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no build has been issued on this handle");
    HIP_TRY(h, hipSetDevice(h->device));
    uint32_t v[kStatusWords];
    // (the build's own event, not its stream: the stream is the caller's and may be gone by now -- ADVICE r4)
    HIP_TRY(h, h->build_order.host_wait());
    HIP_TRY(h, hipMemcpy(v, h->d_result, sizeof v, hipMemcpyDeviceToHost));
    if (int rc = standby_failed(h, v)) return rc;
    return sdfgpu_extrema_from_dsq(v[kSwMaxFree], v[kSwMaxFilled], h->last.last_resolution, out_max, out_min);
}

int sdfgpu_sweep_zy_tiered_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t nxs, int64_t ny, int64_t nz,
                                  int32_t* d_plane_dsq, uint32_t* d_far, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_filled || !d_plane_dsq) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (int rc = check_dims(h, nxs, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const int64_t n = nxs * ny * nz;
        hipStream_t s = (hipStream_t)stream;
        // (this call uses the handle's status block and scratch fields like a whole build does: it takes part in the same
        //  cross-stream ordering -- waits for the handle's previous work when that ran on another stream, and is waited for)
        HIP_TRY(h, h->build_order.wait(s));
        StreamOrder::RecordAtExit order_end{h->build_order, s};
        const bool tiered = h->opt.envelope_on && far_geometry_ok(h, 2, nxs, ny, nz) &&
                            (nz % 4) == 0 && (reinterpret_cast<uintptr_t>(d_plane_dsq) % 16) == 0;
        if (!tiered) {
            if (d_far) HIP_TRY(h, hipMemsetAsync(d_far, 0, 4, s));           // (no probe ran: "else to 0", sdfgpu.h)
            if (fused_zy_eligible(h, d_filled, d_plane_dsq, nz)) return launch_sweep_zy_fused(h, d_filled, d_plane_dsq, kNoSideTable, nxs, ny, nz, kUnguarded, s);
            if (int rc = ensure(h, h->zfield, (size_t)n * 2, "z field")) return rc;
            if (int rc = launch_sweep_z(h, Occupancy::of_mask(d_filled), nxs, ny, nz, (int16_t*)h->zfield.ptr, kUnguarded, s)) return rc;
            return launch_sweep_y(h, (const int16_t*)h->zfield.ptr, d_plane_dsq, kNoSideTable, nxs, ny, nz, kUnguarded, kUnbounded, s);
        }
        // K1, then the y sweep picked on the device: probe -> decide -> marching (bounded scan) / envelope, int32 output
        if (int rc = ensure(h, h->zfield, (size_t)n * 2, "z field")) return rc;
        HIP_TRY(h, hipMemsetAsync(h->d_small, 0, 128, s));
        h->small_clean = false;
        if (int rc = launch_sweep_z(h, Occupancy::of_mask(d_filled), nxs, ny, nz, (int16_t*)h->zfield.ptr, kUnguarded, s)) return rc;
        uint32_t* const sw = h->d_small;
        DcIo ke2;                                                   // z field -> the caller's int32 plane field; no field is finished here:
        ke2.in16 = (const int16_t*)h->zfield.ptr; ke2.out_i32 = d_plane_dsq;
        const double unit = 1.0;                                    // ... no resolution,
        const int no_border = 0;                                    // ... no virtual border
        DcDecide dy; dy.stage = 0;
        if (int rc = launch_probe_or_decide(h, 2, ke2, nxs, ny, nz, unit, no_border, kUnguarded, dy, s)) return rc;
        if (int rc = launch_sweep_y(h, ke2.in16, d_plane_dsq, kNoSideTable, nxs, ny, nz, sw + kSwMarchY, sw + kSwFarY, s)) return rc;
        if (int rc = launch_envelope(h, 2, ke2, nxs, ny, nz, unit, no_border, sw + kSwFarY, s)) return rc;
        if (d_far) HIP_TRY(h, hipMemcpyAsync(d_far, sw + kSwFarY, 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemsetAsync(h->d_small, 0, 128, s));
        h->small_clean = true;
        return SDFGPU_OK;
    });
}

int sdfgpu_sweep_zy_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t nxs, int64_t ny, int64_t nz,
                           int32_t* d_plane_dsq, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        return sdfgpu_sweep_zy_tiered_device(h, d_filled, nxs, ny, nz, d_plane_dsq, nullptr, stream);
    });
}

int sdfgpu_sweep_x_lines_device(sdfgpu_handle h, const int32_t* d_plane_dsq, int64_t nx, int64_t nys, int64_t nz,
                                int64_t y_global, int64_t ny_global, double resolution, int add_virtual_border,
                                float* d_out_sdf, uint32_t* d_maxdsq, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_plane_dsq || !d_out_sdf || !d_maxdsq) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (y_global < 0 || y_global + nys > ny_global) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "inconsistent slab geometry");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, nx, nys, nz)) return rc;
        if (int rc = check_dims(h, nx, ny_global, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        HIP_TRY(h, h->build_order.wait(s));
        StreamOrder::RecordAtExit order_end{h->build_order, s};
        const bool tiered = h->opt.envelope_on && far_geometry_ok(h, 3, nx, nys, nz, ny_global) &&
                            (reinterpret_cast<uintptr_t>(d_plane_dsq) % 16) == 0;
        h->last.last_dc_x = 0;
        h->last.last_lines_tiered = tiered;
        XSlab rows = XSlab::whole(nx);                              // every plane, rows [y_global, y_global + nys) of ny_global
        rows.y_off = y_global; rows.ny_glob = ny_global;
        if (!tiered) {
            if (int rc = launch_sweep_x(h, d_plane_dsq, d_out_sdf, rows, nys, nz, resolution, add_virtual_border, kUnguarded, kUnbounded, s)) return rc;
            return h->opt.defer_fold ? SDFGPU_OK : fold_slots(h, d_maxdsq, s);
        }
        uint32_t* const sw = h->d_small;
        HIP_TRY(h, hipMemsetAsync(sw, 0, 128, s));
        h->small_clean = false;
        DcIo ke3;
        ke3.in_i32 = d_plane_dsq; ke3.out = d_out_sdf; ke3.y_off = y_global; ke3.ny_glob = ny_global;
        DcDecide dx; dx.stage = 1;
        if (int rc = launch_probe_or_decide(h, 3, ke3, nx, nys, nz, resolution, add_virtual_border, kUnguarded, dx, s)) return rc;
        if (int rc = launch_sweep_x(h, d_plane_dsq, d_out_sdf, rows, nys, nz, resolution, add_virtual_border, sw + kSwMarchX, sw + kSwFarX, s)) return rc;
        if (int rc = launch_envelope(h, 3, ke3, nx, nys, nz, resolution, add_virtual_border, sw + kSwFarX, s)) return rc;
        if (!h->opt.defer_fold) if (int rc3 = fold_slots(h, d_maxdsq, s)) return rc3;
        HIP_TRY(h, hipMemsetAsync(h->d_small, 0, 128, s));
        h->small_clean = true;
        return SDFGPU_OK;
    });
}

int sdfgpu_sweep_x_device(sdfgpu_handle h, const int32_t* d_plane_dsq, int64_t halo_lo, int64_t nxs,
                          int64_t halo_hi, int64_t ny, int64_t nz, int lo_truncated, int hi_truncated,
                          int64_t x_global, int64_t nx_global, double resolution, int add_virtual_border,
                          float* d_out_sdf, uint32_t* d_maxdsq, uint32_t* d_status, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_plane_dsq || !d_out_sdf || !d_maxdsq)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (halo_lo < 0 || halo_hi < 0 || x_global < 0 || x_global + nxs > nx_global)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "inconsistent slab geometry");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, halo_lo + nxs + halo_hi, ny, nz)) return rc;
        if (int rc = check_dims(h, nx_global, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        XSlab slab;
        slab.halo_lo = halo_lo; slab.nxs = nxs; slab.halo_hi = halo_hi; slab.lo_trunc = lo_truncated; slab.hi_trunc = hi_truncated;
        slab.x_global = x_global; slab.nx_global = nx_global; slab.status = d_status;
        if (int rc = launch_sweep_x(h, d_plane_dsq, d_out_sdf, slab, ny, nz, resolution, add_virtual_border, kUnguarded, kUnbounded,
                                    (hipStream_t)stream)) return rc;
        return h->opt.defer_fold ? SDFGPU_OK : fold_slots(h, d_maxdsq, (hipStream_t)stream);
    });
}

int sdfgpu_pack_bits_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t n_rows, int64_t nz, uint32_t* d_bits,
                            void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_filled || !d_bits) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (n_rows <= 0 || nz <= 0 || (nz % 32) != 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "pack_bits needs nz % 32 == 0");
        HIP_TRY(h, hipSetDevice(h->device));
        return launch_pack_bits(h, Occupancy::of_mask(d_filled), n_rows * nz, d_bits, (hipStream_t)stream);
    });
}

int sdfgpu_dense_ball_device(sdfgpu_handle h, const uint32_t* d_bits, int64_t rows_x, int64_t out_lo, int64_t out_hi,
                             int64_t ny, int64_t nz, double resolution, float* d_out_sdf, uint32_t* d_maxdsq,
                             uint32_t* d_uncertified, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_bits || !d_out_sdf || !d_maxdsq || !d_uncertified) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (out_lo < 0 || out_hi <= out_lo || out_hi > rows_x) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "inconsistent slab geometry");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, rows_x, ny, nz)) return rc;
        if (!dense_eligible(h, nz)) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dense kernel needs nz = 32 * 2^k <= 2048");
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = launch_ball_dense(h, d_bits, d_out_sdf, rows_x, out_lo, out_hi, ny, nz, resolution, d_uncertified, BallMode{},
                                       (hipStream_t)stream)) return rc;
        return h->opt.defer_fold ? SDFGPU_OK : fold_slots(h, d_maxdsq, (hipStream_t)stream);
    });
}

// One x slab of the dense path in three host calls instead of ten (the per-call cost of the Python binding is what
// limits a rank at ~0.15 ms per build): phase 0 = clear the status words + pack the boundary planes (the caller then
// posts the halo exchange), phase 1 = pack the interior + ball kernel on every plane that needs no neighbour data
// (10 / 11 = only the first / second half of that), phase 2 = ball kernel on the border planes + fold of the maxima
// (after the exchange has been waited for).  Without neighbours, or for slabs too thin to split, phase 0 packs
// everything, phase 1 does nothing and phase 2 runs the ball kernel on the whole slab.
int sdfgpu_slab_dense_phase(sdfgpu_handle h, int phase, const uint8_t* d_mask_slab, int64_t nxs, int64_t ny, int64_t nz,
                            uint32_t* d_bits_ext, int64_t halo_lo, int64_t halo_hi, double resolution, float* d_out,
                            uint32_t* d_small, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_mask_slab || !d_bits_ext || !d_out || !d_small) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        const int64_t hb = kBallR;
        if (nxs <= 0 || (halo_lo != 0 && halo_lo != hb) || (halo_hi != 0 && halo_hi != hb))
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "inconsistent slab geometry");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, halo_lo + nxs + halo_hi, ny, nz)) return rc;
        if (!dense_eligible(h, nz)) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dense kernel needs nz = 32 * 2^k <= 2048");
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        const int64_t plane = ny * nz, wplane = ny * (nz / 32), rows_x = halo_lo + nxs + halo_hi;
        uint32_t* own = d_bits_ext + halo_lo * wplane;
        const bool split = (halo_lo || halo_hi) && 4 * hb < nxs;
        const int64_t i_lo = (split && halo_lo) ? hb : 0, i_hi = (split && halo_hi) ? nxs - hb : nxs;
        auto pack = [&](int64_t p0, int64_t p1) -> int {
            if (p1 <= p0) return SDFGPU_OK;
            return launch_pack_bits(h, Occupancy::of_mask(d_mask_slab + p0 * plane), (p1 - p0) * plane, own + p0 * wplane, s);
        };
        auto ball = [&](int64_t p0, int64_t p1) -> int {
            if (p1 <= p0) return SDFGPU_OK;
            return launch_ball_dense(h, d_bits_ext, d_out + p0 * plane, rows_x, halo_lo + p0, halo_lo + p1, ny, nz, resolution,
                                     d_small + kSwUncertified, BallMode{}, s);
        };
        switch (phase) {
        case 0:
            HIP_TRY(h, hipMemsetAsync(d_small, 0, 16, s));
            if (!split) return pack(0, nxs);
            if (int rc = pack(0, hb)) return rc;
            return pack(nxs - hb, nxs);
        case 1:
        case 10:
        case 11:
            if (!split) return SDFGPU_OK;
            if (phase != 11) if (int rc = pack(hb, nxs - hb)) return rc;
            if (phase != 10) if (int rc = ball(i_lo, i_hi)) return rc;
            return SDFGPU_OK;
        case 2:
            if (!split) {
                if (int rc = ball(0, nxs)) return rc;
            } else {
                if (int rc = ball(0, i_lo)) return rc;
                if (int rc = ball(i_hi, nxs)) return rc;
            }
            return fold_slots(h, d_small, s);
        default:
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "unknown phase %d", phase);
        }
    });
}

int sdfgpu_fold_extrema_device(sdfgpu_handle h, uint32_t* d_maxdsq, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_maxdsq) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        HIP_TRY(h, hipSetDevice(h->device));
        return fold_slots(h, d_maxdsq, (hipStream_t)stream);
    });
}

int sdfgpu_build_tagged_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset,
                              size_t object_id_offset, int object_mode, const uint32_t* object_ids, int64_t n_object_ids,
                              int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              int add_virtual_border, float* out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!out_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null host pointer");
        if (int rc = check_tagged_layout(h, cell_stride, occupancy_offset, object_id_offset)) return rc;
        if (object_mode < 0 || object_mode > 2 || n_object_ids < 0 || n_object_ids > 0x7fffffffLL ||
            (object_mode == 2 && n_object_ids > 0 && !object_ids))
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "bad object filter");
        if (object_mode == 2 && n_object_ids == 0) object_mode = 0;       // "no objects supplied" = any object (:826)
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const int64_t n = nx * ny * nz;
        if (int rc = stage_tagged_records(h, cells, (size_t)n * cell_stride)) return rc;
        if (int rc = ensure(h, h->stage_out, (size_t)n * 4, "output staging")) return rc;
        if (int rc = ensure(h, h->tagmask, (size_t)n, "tagged-object mask")) return rc;
        if (int rc = ensure(h, h->tagids, (size_t)std::max<int64_t>(n_object_ids, 1) * 4, "object id list")) return rc;
        if (n_object_ids > 0) {                        // sorted copy: the classify kernel binary-searches it
            std::vector<uint32_t> sorted_ids(object_ids, object_ids + n_object_ids);
            std::sort(sorted_ids.begin(), sorted_ids.end());
            HIP_TRY(h, hipMemcpy(h->tagids.ptr, sorted_ids.data(), (size_t)n_object_ids * 4, hipMemcpyHostToDevice));
        }
        hipLaunchKernelGGL(k_classify_tagged, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                           (const char*)h->stage_in.ptr, (int64_t)cell_stride, (int64_t)occupancy_offset, (int64_t)object_id_offset,
                           unknown_is_filled, object_mode, (const uint32_t*)h->tagids.ptr, (int)n_object_ids, n,
                           (uint8_t*)h->tagmask.ptr);
        HIP_TRY(h, hipGetLastError());
        int rc = build_device_impl(h, Occupancy::of_mask((const uint8_t*)h->tagmask.ptr), nx, ny, nz, resolution, add_virtual_border,
                                   (float*)h->stage_out.ptr, kNullStream);
        if (rc) return rc;
        if (int rc2 = copy_to_host(h, out_sdf, h->stage_out.ptr, (size_t)n * 4)) return rc2;
        double mx, mn;
        rc = sdfgpu_get_extrema(h, &mx, &mn);
        if (rc) return rc;
        if (out_max) *out_max = mx;
        if (out_min) *out_min = mn;
        return SDFGPU_OK;
    });
}

// ---- batches of same-shape grids (sdfgpu_batch.hpp) ----------------------------------------------------------------------------
namespace {

// `bytes` of per-grid parameters into the pinned ring, then an asynchronous copy to d_dst on `s`: the caller's array is consumed
// before the call returns and the host never waits for the device (only when the ring wraps into parameters that may still be
// in flight: then for the handle's last recorded work).
int batch_stage_params(sdfgpu_handle h, void* d_dst, const void* src, size_t bytes, hipStream_t s) {
    const size_t want = (bytes + 63) & ~(size_t)63;
    if (want > h->batch_pin_cap) {
        HIP_TRY(h, h->build_order.host_wait());
        if (h->batch_pin) HIP_TRY(h, hipHostFree(h->batch_pin));
        h->batch_pin = nullptr; h->batch_pin_cap = 0; h->batch_pin_off = 0;
        const size_t cap = std::max<size_t>(want * 4, (size_t)64 << 10);
        HIP_TRY(h, hipHostMalloc((void**)&h->batch_pin, cap, hipHostMallocDefault));
        h->batch_pin_cap = cap;
    }
    if (h->batch_pin_off + want > h->batch_pin_cap) {
        HIP_TRY(h, h->build_order.host_wait());
        h->batch_pin_off = 0;
    }
    char* p = h->batch_pin + h->batch_pin_off;
    h->batch_pin_off += want;
    memcpy(p, src, bytes);
    HIP_TRY(h, hipMemcpyAsync(d_dst, p, bytes, hipMemcpyHostToDevice, s));
    return SDFGPU_OK;
}

int check_batch_args(sdfgpu_handle h, int64_t batch, int64_t nx, int64_t ny, int64_t nz, double resolution, const double* resolutions) {
    if (batch < 1 || batch > ((int64_t)1 << 24)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "batch must be in 1 .. 2^24 (got %lld)", (long long)batch);
    if (int rc = check_dims(h, nx, ny, nz)) return rc;
    if (nx * ny * nz > (((int64_t)1 << 62) / batch) / 16) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "batch * nx * ny * nz overflows");
    for (int64_t b = 0; b < (resolutions ? batch : 1); ++b) {
        const double r = resolutions ? resolutions[b] : resolution;
        if (!(r > 0.0) || !std::isfinite(r)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resolution must be positive and finite (grid %lld: %g)", (long long)b, r);
    }
    return SDFGPU_OK;
}

struct BatchTagged { const char* d_cells; size_t stride, occ_off, obj_off; int unknown; const uint32_t* d_ids; };

// The batch build on device memory.  Fast path (every axis <= kBatchMaxAxis): two launches on scratch of the batch's own.  Any
// other shape: the single build once per grid on `s`, no host synchronisation in between; the single builds' result block and the
// handle's "last single build" are put back afterwards.
int build_batch_impl(sdfgpu_handle h, const uint8_t* d_filled, const BatchTagged* tg, int64_t batch, int64_t nx, int64_t ny, int64_t nz,
                     double resolution, const double* resolutions, int vb, float* d_out, hipStream_t s) {
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t n = nx * ny * nz;
    int64_t cx = nx, cy = ny, cz = nz;
    canonical_dims(cx, cy, cz);
    const bool fast = batch_fast_shape(cx, cy, cz) && batch * cx < ((int64_t)1 << 31) - 8;
    if (int rc = ensure(h, h->batch_ext, (size_t)(2 * batch + 32) * 4, "batch extrema")) return rc;
    if (fast) if (int rc = ensure(h, h->batch_field, (size_t)batch * n * 2, "batch plane field")) return rc;
    if (fast && resolutions) if (int rc = ensure(h, h->batch_res, (size_t)batch * 8, "batch resolutions")) return rc;
    if (!fast && tg) if (int rc = ensure(h, h->tagmask, (size_t)n, "tagged-object mask")) return rc;
    h->batch_valid = false;
    if (resolutions) h->batch_resolutions.assign(resolutions, resolutions + batch);
    else h->batch_resolutions.assign((size_t)batch, resolution);
    uint32_t* ext = (uint32_t*)h->batch_ext.ptr;
    if (fast) {
        HIP_TRY(h, h->build_order.wait(s));
        if (resolutions) if (int rc = batch_stage_params(h, h->batch_res.ptr, resolutions, (size_t)batch * 8, s)) return rc;
        BatchArgs a{};
        a.mask = tg ? nullptr : d_filled;
        if (tg) { a.cells = tg->d_cells; a.stride = (int64_t)tg->stride; a.occ_off = (int64_t)tg->occ_off; a.obj_off = (int64_t)tg->obj_off;
                  a.unknown_is_filled = tg->unknown; a.ids = tg->d_ids; }
        a.plane = (int16_t*)h->batch_field.ptr; a.out = d_out;
        a.res = resolutions ? (const double*)h->batch_res.ptr : nullptr; a.res_uniform = resolution;
        a.ext = ext; a.batch = (int)batch; a.nx = (int)cx; a.ny = (int)cy; a.nz = (int)cz; a.vb = vb;
        int launches = 0;
        HIP_TRY(h, batch_launch(a, s, &launches));
        h->batch_launches = launches;
    } else {
        const bool had = h->last.have_result;
        const double keep_res = h->last.last_resolution;
        const int64_t keep_n = h->last.last_n;
        uint32_t* keep = ext + 2 * batch;
        HIP_TRY(h, h->build_order.wait(s));
        HIP_TRY(h, hipMemcpyAsync(keep, h->d_result, kStatusWords * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, h->build_order.adopt(s));            // (the single builds below are on `s` too: none of them waits again)
        for (int64_t b = 0; b < batch; ++b) {
            const uint8_t* m = d_filled ? d_filled + b * n : (const uint8_t*)h->tagmask.ptr;
            if (tg) {      // (object_mode 2 with the single id ids[b]: a one-element list is sorted)
                hipLaunchKernelGGL(k_classify_tagged, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tg->d_cells,
                                   (int64_t)tg->stride, (int64_t)tg->occ_off, (int64_t)tg->obj_off, tg->unknown, 2, tg->d_ids + b, 1, n,
                                   (uint8_t*)h->tagmask.ptr);
                HIP_TRY(h, hipGetLastError());
            }
            if (int rc = build_device_impl(h, Occupancy::of_mask(m), nx, ny, nz, h->batch_resolutions[(size_t)b], vb, d_out + b * n, s)) return rc;
            HIP_TRY(h, hipMemcpyAsync(ext + 2 * b, h->d_result, 8, hipMemcpyDeviceToDevice, s));
        }
        HIP_TRY(h, hipMemcpyAsync(h->d_result, keep, kStatusWords * 4, hipMemcpyDeviceToDevice, s));
        h->last.have_result = had; h->last.last_resolution = keep_res; h->last.last_n = keep_n;
        h->batch_launches = -1;
    }
    HIP_TRY(h, h->build_order.record(s));
    h->batch_fast = fast ? 1 : 0;
    h->batch_valid = true;
    return SDFGPU_OK;
}

int get_extrema_batch(sdfgpu_handle h, int64_t batch, double* out_max, double* out_min) {
    if (!h->batch_valid) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no batch build has been issued on this handle");
    if (batch != (int64_t)h->batch_resolutions.size())
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "the last batch build held %lld grids, not %lld", (long long)h->batch_resolutions.size(), (long long)batch);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->build_order.host_wait());
    std::vector<uint32_t> v((size_t)batch * 2);
    HIP_TRY(h, hipMemcpy(v.data(), h->batch_ext.ptr, v.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t b = 0; b < batch; ++b)
        sdfgpu_extrema_from_dsq(v[2 * b], v[2 * b + 1], h->batch_resolutions[(size_t)b], out_max ? out_max + b : nullptr, out_min ? out_min + b : nullptr);
    return SDFGPU_OK;
}

}  // namespace

int sdfgpu_build_batch_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t batch, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              const double* resolutions, int add_virtual_border, float* d_out_sdf, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_filled || !d_out_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (int rc = check_batch_args(h, batch, nx, ny, nz, resolution, resolutions)) return rc;
        return build_batch_impl(h, d_filled, nullptr, batch, nx, ny, nz, resolution, resolutions, add_virtual_border, d_out_sdf, (hipStream_t)stream);
    });
}

int sdfgpu_get_extrema_batch(sdfgpu_handle h, int64_t batch, double* out_max, double* out_min) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    return get_extrema_batch(h, batch, out_max, out_min);
}

int sdfgpu_build_batch(sdfgpu_handle h, const uint8_t* filled, int64_t batch, int64_t nx, int64_t ny, int64_t nz, double resolution,
                       const double* resolutions, int add_virtual_border, float* out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!filled || !out_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null host pointer");
        if (int rc = check_batch_args(h, batch, nx, ny, nz, resolution, resolutions)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const size_t total = (size_t)(batch * nx * ny * nz);
        if (int rc = stage_input(h, total)) return rc;
        if (int rc = ensure(h, h->stage_out, total * 4, "output staging")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, filled, total)) return rc;
        if (int rc = build_batch_impl(h, (const uint8_t*)h->stage_in.ptr, nullptr, batch, nx, ny, nz, resolution, resolutions, add_virtual_border,
                                      (float*)h->stage_out.ptr, nullptr)) return rc;
        if (int rc = copy_to_host(h, out_sdf, h->stage_out.ptr, total * 4)) return rc;
        return get_extrema_batch(h, batch, out_max, out_min);
    });
}

int sdfgpu_build_tagged_objects(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t object_id_offset,
                                const uint32_t* object_ids, int64_t n_object_ids, int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz,
                                double resolution, int add_virtual_border, float* out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!out_sdf || !object_ids) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null host pointer");
        if (int rc = check_tagged_layout(h, cell_stride, occupancy_offset, object_id_offset)) return rc;
        if (int rc = check_batch_args(h, n_object_ids, nx, ny, nz, resolution, nullptr)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const int64_t n = nx * ny * nz;
        if (int rc = stage_tagged_records(h, cells, (size_t)n * cell_stride)) return rc;
        if (int rc = ensure(h, h->stage_out, (size_t)(n_object_ids * n) * 4, "output staging")) return rc;
        if (int rc = ensure(h, h->tagids, (size_t)n_object_ids * 4, "object id list")) return rc;
        HIP_TRY(h, hipMemcpy(h->tagids.ptr, object_ids, (size_t)n_object_ids * 4, hipMemcpyHostToDevice));
        const BatchTagged tg{(const char*)h->stage_in.ptr, cell_stride, occupancy_offset, object_id_offset, unknown_is_filled, (const uint32_t*)h->tagids.ptr};
        if (int rc = build_batch_impl(h, nullptr, &tg, n_object_ids, nx, ny, nz, resolution, nullptr, add_virtual_border, (float*)h->stage_out.ptr, nullptr))
            return rc;
        if (int rc = copy_to_host(h, out_sdf, h->stage_out.ptr, (size_t)(n_object_ids * n) * 4)) return rc;
        return get_extrema_batch(h, n_object_ids, out_max, out_min);
    });
}

int sdfgpu_gradient_batch_device(sdfgpu_handle h, const float* d_sdf, int64_t batch, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 const double* resolutions, int enable_edge_gradients, int f64, void* d_out, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_sdf || !d_out) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (batch < 1 || batch > ((int64_t)1 << 24)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "batch must be in 1 .. 2^24 (got %lld)", (long long)batch);
        for (int64_t b = 0; b < (resolutions ? batch : 1); ++b)
            if (int rc = check_resolution(h, resolutions ? resolutions[b] : resolution)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        // the reference's reciprocals, computed once per grid with its own double operations (sdfgpu_gradient_device)
        auto scale_of = [](double res) {
            GradScale sc{};
            sc.inv2 = 1.0 / (2.0 * res);
            sc.inv_w1 = 1.0 / ((double)1 * res);
            sc.inv_w2 = 1.0 / ((double)2 * res);
            sc.inv2f = (float)sc.inv2;
            return sc;
        };
        BatchGradArgs a{};
        a.sdf = d_sdf; a.out = d_out; a.nx = nx; a.ny = ny; a.nz = nz; a.batch = (int)batch; a.edge = enable_edge_gradients; a.f64 = f64;
        if (resolutions) {
            // (the scale table is the handle's: calls on different streams are ordered like builds)
            std::vector<GradScale> sc((size_t)batch);
            for (int64_t b = 0; b < batch; ++b) sc[(size_t)b] = scale_of(resolutions[b]);
            if (int rc = ensure(h, h->batch_gscale, sc.size() * sizeof(GradScale), "batch gradient scales")) return rc;
            HIP_TRY(h, h->build_order.wait(s));
            if (int rc = batch_stage_params(h, h->batch_gscale.ptr, sc.data(), sc.size() * sizeof(GradScale), s)) return rc;
            a.scales = h->batch_gscale.ptr;
        } else {
            const GradScale sc = scale_of(resolution);
            a.inv2 = sc.inv2; a.inv_w1 = sc.inv_w1; a.inv_w2 = sc.inv_w2;
        }
        HIP_TRY(h, batch_gradient_launch(a, s));
        if (resolutions) {
            HIP_TRY(h, h->build_order.record(s));
        }
        return SDFGPU_OK;
    });
}

int sdfgpu_last_batch_info(sdfgpu_handle h, int* out_fast_path, int* out_launches) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!h->batch_valid) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no batch build has been issued on this handle");
    if (out_fast_path) *out_fast_path = h->batch_fast;
    if (out_launches) *out_launches = h->batch_launches;
    return SDFGPU_OK;
}

int sdfgpu_classify_cells_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset,
                                 int unknown_is_filled, int64_t n_cells, uint8_t* d_mask, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_cells || !d_mask || n_cells < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "bad classify arguments");
        if (int rc = check_cell_layout(h, cell_stride, occupancy_offset)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        if (n_cells == 0) return SDFGPU_OK;
        CellLoader ld{reinterpret_cast<const char*>(d_cells), (int64_t)cell_stride, (int64_t)occupancy_offset, unknown_is_filled};
        hipLaunchKernelGGL(k_classify_cells, dim3((unsigned)((n_cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                           ld, n_cells, d_mask);
        HIP_TRY(h, hipGetLastError());
        return SDFGPU_OK;
    });
}

int sdfgpu_voxelize_points_device(sdfgpu_handle h, const float* d_points, int64_t n_points, const double* origin,
                                  double resolution, int64_t nx, int64_t ny, int64_t nz, uint8_t* d_mask, int clear_first,
                                  void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_mask || !origin || (n_points > 0 && !d_points) || n_points < 0)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "bad voxelize arguments");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        if (clear_first) HIP_TRY(h, hipMemsetAsync(d_mask, 0, (size_t)(nx * ny * nz), s));
        if (n_points > 0) {
            hipLaunchKernelGGL(k_voxelize_points, dim3((unsigned)((n_points + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_points,
                               n_points, origin[0], origin[1], origin[2], resolution, nx, ny, nz, d_mask);
            HIP_TRY(h, hipGetLastError());
        }
        return SDFGPU_OK;
    });
}

int sdfgpu_voxelize_points_bits_device(sdfgpu_handle h, const float* d_points, int64_t n_points, const double* origin,
                                       double resolution, int64_t nx, int64_t ny, int64_t nz, uint32_t* d_bits, int clear_first,
                                       void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_bits || !origin || (n_points > 0 && !d_points) || n_points < 0)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "bad voxelize arguments");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        if (clear_first) HIP_TRY(h, hipMemsetAsync(d_bits, 0, (((size_t)(nx * ny * nz) + 31) / 32) * 4, s));
        if (n_points > 0) {
            hipLaunchKernelGGL(k_voxelize_points_bits, dim3((unsigned)((n_points + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_points,
                               n_points, origin[0], origin[1], origin[2], resolution, nx, ny, nz, d_bits);
            HIP_TRY(h, hipGetLastError());
        }
        return SDFGPU_OK;
    });
}

int sdfgpu_gradient_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz,
                           double resolution, int enable_edge_gradients, void* d_out_grad, int out_is_f64,
                           void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_sdf || !d_out_grad) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const int64_t n = nx * ny * nz;
        dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
        hipStream_t s = (hipStream_t)stream;
        // the reference's reciprocals, computed once with its own double operations (sdf.hpp:447 and :464-512)
        GradScale sc{};
        sc.inv2 = 1.0 / (2.0 * resolution);
        sc.inv_w1 = 1.0 / ((double)1 * resolution);
        sc.inv_w2 = 1.0 / ((double)2 * resolution);
        sc.inv2f = (float)sc.inv2;
        if (out_is_f64)
            hipLaunchKernelGGL(k_gradient<double>, grid, block, 0, s, d_sdf, (double*)d_out_grad, nx, ny, nz, sc, enable_edge_gradients);
        else if ((nz % 4) == 0 && ny * (nz / 4) < ((int64_t)1 << 31) - kBlock &&
                 (reinterpret_cast<uintptr_t>(d_sdf) % 16) == 0 && (reinterpret_cast<uintptr_t>(d_out_grad) % 16) == 0) {
            const bool f32scale = (double)sc.inv2f == sc.inv2 && std::isfinite(sc.inv2) && std::fabs(sc.inv2) < 1e30 && std::fabs(sc.inv2) > 1e-30;
            const int64_t per_plane = ny * (nz / 4);                                  // groups of 4 voxels per x plane
            const dim3 g4((unsigned)((per_plane + kBlock - 1) / kBlock), (unsigned)std::min<int64_t>(nx, 65535));
            int gshift = -1;                                                           // log2(nz / 4) when that is a power of two
            for (int b = 0; b < 31; ++b) if (((int64_t)1 << b) == nz / 4) gshift = b;
            if (f32scale) hipLaunchKernelGGL(k_gradient_f32x4<true>, g4, block, 0, s, d_sdf, (float*)d_out_grad, nx, ny, nz, sc, enable_edge_gradients, gshift);
            else hipLaunchKernelGGL(k_gradient_f32x4<false>, g4, block, 0, s, d_sdf, (float*)d_out_grad, nx, ny, nz, sc, enable_edge_gradients, gshift);
        } else
            hipLaunchKernelGGL(k_gradient<float>, grid, block, 0, s, d_sdf, (float*)d_out_grad, nx, ny, nz, sc, enable_edge_gradients);
        HIP_TRY(h, hipGetLastError());
        return SDFGPU_OK;
    });
}

// Host-buffer form of the full-grid gradient (what SignedDistanceField::GetFullGradient / pysdf_tools'
// GetFullGradientNumpy call instead of N host GetGradient calls): upload the field, one kernel, download.
int sdfgpu_gradient(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                    int enable_edge_gradients, void* out_grad, int out_is_f64) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!sdf || !out_grad) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null host pointer");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const size_t n = (size_t)(nx * ny * nz), esz = out_is_f64 ? 8 : 4;
        // the x axis is cut into chunks (+1 plane of context each side) so that the staging stays <= ~1.5 GiB even
        // for the 24 B/voxel double output of a 512^3 field
        const int64_t plane = ny * nz;
        const int64_t max_rows = std::max<int64_t>(1, ((int64_t)1 << 26) / std::max<int64_t>(plane, 1));   // <= 64 Mi voxels per chunk
        const int64_t rows = std::min<int64_t>(nx, max_rows);
        if (int rc = stage_input(h, (size_t)(rows + 2) * plane * 4)) return rc;
        if (int rc = ensure(h, h->stage_out, (size_t)(rows + 2) * plane * 3 * esz, "output staging")) return rc;
        (void)n;
        for (int64_t x0 = 0; x0 < nx; x0 += rows) {
            const int64_t x1 = std::min(nx, x0 + rows);
            const int64_t lo = std::max<int64_t>(0, x0 - 1), hi = std::min(nx, x1 + 1);     // context planes
            if (int rc0 = copy_from_host(h, h->stage_in.ptr, sdf + lo * plane, (size_t)(hi - lo) * plane * 4)) return rc0;
            // the kernel treats the chunk as a grid of its own: its first / last plane would take the one-sided boundary
            // formula, so those planes are computed only when they ARE grid faces and are otherwise context that is skipped
            if (int rc = sdfgpu_gradient_device(h, (const float*)h->stage_in.ptr, hi - lo, ny, nz, resolution, enable_edge_gradients,
                                                h->stage_out.ptr, out_is_f64, nullptr)) return rc;
            if (int rc = copy_to_host(h, (char*)out_grad + (size_t)x0 * plane * 3 * esz,
                                      (const char*)h->stage_out.ptr + (size_t)(x0 - lo) * plane * 3 * esz,
                                      (size_t)(x1 - x0) * plane * 3 * esz)) return rc;
        }
        return SDFGPU_OK;
    });
}

int sdfgpu_query_points_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                               const double* world_to_grid, const double* grid_to_world_rotation, float oob_value,
                               const double* d_points, int64_t n_points, int enable_edge_gradients, double* d_distance,
                               double* d_gradient, uint8_t* d_flags, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!d_sdf || (n_points > 0 && !d_points)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
        if (n_points < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "bad point count");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;
        if (n_points == 0 || (!d_distance && !d_gradient && !d_flags)) return SDFGPU_OK;
        HIP_TRY(h, hipSetDevice(h->device));
        QueryArgs a{};
        a.sdf = d_sdf; a.points = d_points; a.distance = d_distance; a.gradient = d_gradient; a.flags = d_flags;
        a.n = n_points; a.nx = nx; a.ny = ny; a.nz = nz;
        a.res = resolution; a.inv_res = 1.0 / resolution; a.oob = (double)oob_value;
        static const double ident34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        static const double ident33[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int i = 0; i < 12; ++i) a.w2g[i] = world_to_grid ? world_to_grid[i] : ident34[i];
        for (int i = 0; i < 9; ++i) a.rot[i] = grid_to_world_rotation ? grid_to_world_rotation[i] : ident33[i];
        a.edge = enable_edge_gradients;
        hipLaunchKernelGGL(k_query_points, dim3((unsigned)((n_points + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           (hipStream_t)stream, a);
        HIP_TRY(h, hipGetLastError());
        return SDFGPU_OK;
    });
}

int sdfgpu_query_points(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                        const double* world_to_grid, const double* grid_to_world_rotation, float oob_value,
                        const double* points, int64_t n_points, int enable_edge_gradients, double* out_distance,
                        double* out_gradient, uint8_t* out_flags) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!d_sdf || (n_points > 0 && !points)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (n_points < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "bad point count");
        if (int rc = check_resolution(h, resolution)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;
        if (n_points == 0 || (!out_distance && !out_gradient && !out_flags)) return SDFGPU_OK;
        HIP_TRY(h, hipSetDevice(h->device));
        // points | distance | gradient | flags
        return with_staged_points(h, points, n_points, {8, 24, 1}, {out_distance, out_gradient, out_flags}, [&](const double* d_points, char* const (&d)[3]) {
            return sdfgpu_query_points_device(h, d_sdf, nx, ny, nz, resolution, world_to_grid, grid_to_world_rotation, oob_value, d_points, n_points,
                                              enable_edge_gradients, (double*)d[0], (double*)d[1], (uint8_t*)d[2], nullptr);
        });
    });
}

int sdfgpu_debug_finish_table(sdfgpu_handle h, float* d_out, int64_t n, double resolution, int fast, uint32_t* out_slow_lanes) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!d_out || n <= 0 || n > (1ll << 24)) return SDFGPU_ERR_INVALID_ARGUMENT;
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = ensure(h, h->tagids, 4, "object id list")) return rc;
        h->tag_cached_bytes = 0;
        HIP_TRY(h, hipMemset(h->tagids.ptr, 0, 4));
        const FinishFast fin = make_finish_fast(resolution, (uint64_t)n, fast != 0);
        hipLaunchKernelGGL(k_finish_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d_out, n, resolution, fin, (uint32_t*)h->tagids.ptr);
        HIP_TRY(h, hipGetLastError());
        uint32_t c = 0;
        HIP_TRY(h, hipMemcpy(&c, h->tagids.ptr, 4, hipMemcpyDeviceToHost));
        if (out_slow_lanes) *out_slow_lanes = c;
        return SDFGPU_OK;
    });
}

int sdfgpu_debug_copy_zsweep(sdfgpu_handle h, int16_t* out_host, int64_t n) {
    if (!h || !out_host) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!h->last.have_result || n > h->last.last_n) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no matching build");
    if (h->last.last_fused) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "the last build fused the z sweep into the y sweep: no z field exists");
    if (h->last.last_standby) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "the last build's stand-by pair takes its z distances from the bit field: no z field exists");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->build_order.host_wait());
    HIP_TRY(h, hipMemcpy(out_host, h->zfield.ptr, (size_t)n * 2, hipMemcpyDeviceToHost));
    if (h->last.last_plane_skip && h->planebits.ptr && n == h->last.last_dims[0] * h->last.last_dims[1] * h->last.last_dims[2]) {
        // the z sweep of a build that went straight to the far-field pair does not write rows without a filled voxel
        const int64_t nrows = h->last.last_dims[0] * h->last.last_dims[1], nz = h->last.last_dims[2];
        std::vector<uint8_t> ra((size_t)nrows);
        HIP_TRY(h, hipMemcpy(ra.data(), h->planebits.ptr, ra.size(), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < nrows; ++r)
            if (!ra[(size_t)r]) std::fill(out_host + r * nz, out_host + (r + 1) * nz, (int16_t)kInf16);
    }
    return SDFGPU_OK;
}

int sdfgpu_debug_copy_yzsweep(sdfgpu_handle h, int32_t* out_host, int64_t n) {
    if (!h || !out_host) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!h->last.have_result || n > h->last.last_n) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no matching build");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->build_order.host_wait());
    HIP_TRY(h, hipMemcpy(out_host, h->yzfield.ptr, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (h->last.last_plane_skip && h->planebits.ptr && n == h->last.last_dims[0] * h->last.last_dims[1] * h->last.last_dims[2]) {
        // the y sweep skipped the x-planes without a filled voxel: every voxel of such a plane is "free, no filled voxel in the plane"
        std::vector<uint8_t> pa((size_t)h->last.last_dims[0]);
        HIP_TRY(h, hipMemcpy(pa.data(), (const uint8_t*)h->planebits.ptr + h->last.last_dims[0] * h->last.last_dims[1], pa.size(), hipMemcpyDeviceToHost));
        const int64_t plane = h->last.last_dims[1] * h->last.last_dims[2];
        for (int64_t x = 0; x < h->last.last_dims[0]; ++x)
            if (!pa[(size_t)x]) std::fill(out_host + x * plane, out_host + (x + 1) * plane, (int32_t)kInf32);
    }
    uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};                 // status block of the last build ([7]: int32 hand-off used)
    HIP_TRY(h, hipMemcpy(st, h->d_result, sizeof st, hipMemcpyDeviceToHost));
    if (h->last.last_plane16 && st[7] == 0u && !h->last.last_predicted) {
        // 16-bit pipeline: the int32 buffer is the side table (valid only for saturated groups of 4)
        std::vector<int16_t> p16((size_t)n);
        HIP_TRY(h, hipMemcpy(p16.data(), h->plane16.ptr, (size_t)n * 2, hipMemcpyDeviceToHost));
        for (int64_t g = 0; g + 3 < n; g += 4) {
            bool sat = false;
            for (int k = 0; k < 4; ++k) sat |= std::abs((int)p16[(size_t)(g + k)]) >= 32767;
            if (!sat) for (int k = 0; k < 4; ++k) out_host[g + k] = p16[(size_t)(g + k)];
        }
    }
    return SDFGPU_OK;
}

int sdfgpu_set_profiling(sdfgpu_handle h, int enable) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    h->profiling = enable < 0 ? 0 : (enable > 3 ? 1 : enable);
    h->profiled_builds = 0;
    return SDFGPU_OK;
}

int sdfgpu_get_stage_times(sdfgpu_handle h, double* out_ms_sum, int64_t* out_builds) {
    if (!h || !out_ms_sum || !out_builds) return SDFGPU_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    for (int k = 0; k < 7; ++k) out_ms_sum[k] = 0.0;
    *out_builds = 0;
    if (h->events.empty()) return SDFGPU_OK;
    HIP_TRY(h, hipEventSynchronize(h->events.back()));
    for (size_t i = 0; i + 7 < h->events.size(); i += 8) {
        for (int k = 0; k < 7; ++k) {
            float ms = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&ms, h->events[i + k], h->events[i + k + 1]));
            out_ms_sum[k] += ms;
        }
        ++*out_builds;
    }
    for (size_t i = 0; i < h->events.size(); ++i)
        if (i % 8 == 0 || h->events[i] != h->events[i - 1]) h->event_pool.push_back(h->events[i]);   // marks may be shared
    h->events.clear();
    return SDFGPU_OK;
}

int sdfgpu_set_option(sdfgpu_handle h, const char* name, int value) {
    if (!h || !name) return SDFGPU_ERR_INVALID_ARGUMENT;
    const std::string n(name);
    BuildOptions& o = h->opt;
    // tier selection
    if (n == "dense") o.dense_on = value != 0;
    else if (n == "dense_generic") o.dense_generic_on = value != 0;
    else if (n == "dense_retry") { h->pol.dense_retry = value; h->pol.dense_skip = 0; h->pol.dense_backoff = 0; }
    else if (n == "envelope") o.envelope_on = value != 0;
    else if (n == "envelope_dc") o.envelope_dc = value != 0;
    else if (n == "envelope_mode") { h->flags_pending = false; o.force_env = value != 0 ? 1 : -1; }
    else if (n == "far_predict") h->far.set_mode(value);
    else if (n == "far_threshold_y") o.far_thr[0] = value;
    else if (n == "far_threshold_x") o.far_thr[1] = value;
    else if (n == "probe_window") o.probe_window = value != 0;
    else if (n == "policy_reset") { h->flags_pending = false; h->pol.reset(); h->far.reset(); h->flat_score_reset = true; }
    else if (n == "expect_dense") h->pol.expect_dense = value != 0;      // tests: put the handle into the "dense tier trusted" state
    else if (n == "fixup_mode") h->pol.fix_mode = value != 0;
    else if (n == "dense3_mode") h->pol.dense3_mode = value != 0;
    // dense tier
    else if (n == "dense3") { h->pol.dense3_on = value != 0; h->pol.dense3_mode = false; }
    else if (n == "dense3_staged") h->pol.dense3_staged = value != 0;
    else if (n == "dense3_fixed") o.dense3_fixed = value != 0;
    else if (n == "dense_shell") o.shell_on = value != 0;
    else if (n == "shell_min_words") o.shell_min_words = value >= 0 ? value : kShellMinWords;
    else if (n == "standby_far") o.standby_far = value != 0;
    else if (n == "standby_fold") o.standby_fold = value != 0;
    else if (n == "standby_single") o.standby_single = value != 0;
    else if (n == "standby_grid") o.standby_grid = value >= 32 ? value : 1024;
    else if (n == "ball_serpentine") o.ball_serpentine = value != 0;
    // sweeps
    else if (n == "fused_zy") { o.fused_zy = value != 0; o.fused_always = value == 2; }
    else if (n == "fused_window") o.fused_h = value;
    else if (n == "plane16") o.plane16_on = value != 0;
    else if (n == "z_wave") o.z_wave_on = value != 0;
    else if (n == "x16_voxels_per_lane") o.x16_v = value;
    else if (n == "x16_window") o.x16_h = value;
    else if (n == "i32_handoff") o.i32_handoff = value != 0;
    else if (n == "dc_fixed") o.dc_fixed = value != 0;
    else if (n == "plane_skip") o.plane_skip = value != 0;
    else if (n == "flat_tiles") o.flat_tiles = value < 0 ? 0 : value > 2 ? 2 : value;
    // host side / debugging
    else if (n == "host_pack") o.host_pack = (value >= 0 && value <= 2) ? value : 1;
    else if (n == "defer_fold") o.defer_fold = value != 0;
    else if (n == "redzone") {
        // from now on: every buffer the context holds is released (and comes back with -- or without -- zones when it is next needed);
        // the status block and the slots are replaced at once
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipDeviceSynchronize());
        for (DeviceBuffer& b : *h) if (b.ptr) { (void)rz_free(h, b.ptr); b.ptr = nullptr; b.bytes = 0; }
        // what the handle remembers of their contents goes with them (components, topology, surfaces, cx_field: nothing outlives a call)
        h->tag_cached_bytes = 0;
        h->batch_valid = false;                         // (the batch's extrema words went with batch_ext)
        h->cx_stats_off = 0;                            // (sdfgpu_convex_last_info reads its statistics out of cx_scratch)
        (void)rz_free(h, h->d_small);
        (void)rz_free(h, h->d_slots);
        h->d_small = h->d_slots = nullptr;
        h->redzone = value != 0;
        if (int rc = rz_malloc(h, "extrema slots", (size_t)kSlots * kSlotWords * 4, (void**)&h->d_slots)) return rc;
        if (int rc = rz_malloc(h, "status block", 512, (void**)&h->d_small)) return rc;
        HIP_TRY(h, hipMemset(h->d_slots, 0, (size_t)kSlots * kSlotWords * 4));
        HIP_TRY(h, hipMemset(h->d_small, 0, 512));
        h->d_result = h->d_small + 64;
        h->small_clean = true;
        h->last.have_result = false;
        h->flags_pending = h->far_pending = false;
    }
    else if (n == "resample_plain_atomics") o.rs_plain_atomics = value != 0;
    else if (n == "resample_timing") { o.rs_timing = value != 0; h->rs_timed = false; }
    else return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "unknown option '%s'", name);
    return SDFGPU_OK;
}

int sdfgpu_last_build_info(sdfgpu_handle h, int* out_fused_zy) {
    if (!h || !out_fused_zy) return SDFGPU_ERR_INVALID_ARGUMENT;
    *out_fused_zy = (h->last.last_fused ? 1 : 0) | (h->last.last_plane16 ? 2 : 0) | (h->last.last_dense ? 4 : 0) | (h->last.last_standby ? 8 : 0) |
                    (h->last.last_dense3 ? 16 : 0) | (h->last.last_staged ? 32 : 0) | (h->last.last_predicted ? 64 : 0) |
                    (h->last.last_lines_tiered ? 128 : 0) | ((h->last.last_dc_x & 31) << 8) | (h->last.last_standby_single ? (1 << 13) : 0);
    return SDFGPU_OK;
}

int sdfgpu_last_dense_certified(sdfgpu_handle h, int* out_certified) {
    if (!h || !out_certified) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!h->last.have_result) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no build has been issued on this handle");
    HIP_TRY(h, hipSetDevice(h->device));
    uint32_t v[kStatusWords];
    // (the build's own event, not its stream: the stream is the caller's and may be gone by now -- ADVICE r4)
    HIP_TRY(h, h->build_order.host_wait());
    HIP_TRY(h, hipMemcpy(v, h->d_result, sizeof v, hipMemcpyDeviceToHost));
    if (int rc = standby_failed(h, v)) return rc;
    // bit 0: dense kernel decided everything; bit 1 / 2: the y / x sweep was redone by the envelope kernel
    uint32_t why = 0;
    HIP_TRY(h, hipMemcpy(&why, h->d_result + kSwReason, sizeof why, hipMemcpyDeviceToHost));
    *out_certified = ((h->last.last_dense && v[kSwUncertified] == 0) ? 1 : 0) | (v[kSwFarY] ? 2 : 0) | (v[kSwFarX] ? 4 : 0) | (int)((why & 0xffu) << 8);
    return SDFGPU_OK;
}

int sdfgpu_debug_flat_habit(sdfgpu_handle h, int* out_score, int* out_gate) {
    if (!h || !out_score || !out_gate) return SDFGPU_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->build_order.host_wait());
    int v[2] = {0, 0};                                          // kSwFlatScore, kSwFlatGate
    HIP_TRY(h, hipMemcpy(v, h->d_small + kSwFlatScore, sizeof v, hipMemcpyDeviceToHost));
    *out_score = v[0];
    *out_gate = v[1];
    return SDFGPU_OK;
}

int sdfgpu_set_tuning(sdfgpu_handle h, int rows_per_chunk_y, int rows_per_chunk_x) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    h->opt.tune_ty = rows_per_chunk_y;
    h->opt.tune_tx = rows_per_chunk_x;
    return SDFGPU_OK;
}

}  // extern "C"
