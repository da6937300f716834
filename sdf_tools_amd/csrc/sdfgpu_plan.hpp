// sdfgpu_plan.hpp -- what a build enqueues, decided on the host in one place (no HIP in here: the CPU suite compiles this header
// with g++ and drives plan_build through the situations a GPU test can only reach by building scenes, tests/plan_harness.cpp).
//
// build_device_impl (sdfgpu.hip) fills in BuildFacts -- what only the build unit can know: the shape gates that depend on kernel
// constants, the alignment of the caller's pointers, which report slots are free --, calls plan_build ONCE, allocates every scratch
// field the plan names, and only then enqueues.  Like the policy objects it consults, the plan is exactness-neutral: every
// combination of its flags yields the same field; it decides which kernels stand in front of / behind which guard word.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sdfgpu_policy.hpp"

namespace sdfgpu {

constexpr int kShellMinWords = 128;           // KD6 (sdfgpu_dense6.hpp): active words (of kShellGroup x 256) below which a group is left to KF

// What sdfgpu_set_option and sdfgpu_set_tuning write and a build only reads (include/sdfgpu.h has the table).  The defaults here are
// the documented ones.
struct BuildOptions {
    // tier selection
    bool dense_on = true;            // try the bit-parallel dense kernel first when the shape allows
    bool dense_generic_on = true;    // generic dense kernels for shapes / modes the tuned ones do not take
    bool envelope_on = true;         // bound the outward scans and redo far-field sweeps with the envelope kernels
    bool envelope_dc = true;         // use the divide-and-conquer envelope kernel (sdfgpu_envelope_dc.hpp) when the shape allows
    int force_env = -1;              // -1 automatic, 1 = envelope kernels only (option "envelope_mode")
    // an axis is far-field when more than 1 / kFarDen of the probed voxels have d^2 >= thr.  Per axis, from the measured
    // break-even of the two sweeps at 512^3 (tools/p_sweep.py, tools/ythr_probe.py): the y marching sweep (2 B rows, radius-8
    // windows) against the far-field PAIR (int32 hand-off, no x probe) breaks even at in-plane d^2 ~ 36 on an eighth of the
    // voxels (Bernoulli p = 0.02: 1.31 vs 1.29 ms; p = 0.015: 1.54 vs 1.29 ms; p = 0.025: 1.21 vs 1.28 ms); the x marching sweep falls behind the far-field kernel as soon as its
    // radius-3 window stops deciding nearly every voxel (Bernoulli p = 0.03: 0.65 ms against 0.55; p = 0.04 and denser:
    // marching wins), so its threshold is d^2 >= 9 on 1 / 24 of the voxels (p = 0.03: 6 %, p = 0.04: 2.4 %)
    // (round 3, third-generation far-field kernel: KE2 0.57 -> 0.39 ms moves the y break-even from Bernoulli p ~ 0.018 up to
    //  p ~ 0.035 -- tools/tier_sweep.py: p = 0.03 1.01 vs 0.97 ms, p = 0.02 1.16 vs 0.985, p = 0.04 0.87 vs 0.97 -- i.e. from
    //  "d^2 >= 36 on an eighth" to "d^2 >= 16 on a fifth" of the voxels: (1 - p)^49 = 0.225 at p = 0.03, 0.135 at p = 0.04)
    int far_thr[2] = {16, 9};
    bool probe_window = true;        // tier probes as window statistics (option "probe_window"; 0 = level A of the far-field search on sampled tiles)
    // dense tier
    bool dense3_fixed = true;        // KD3's nz = 512 instance (option "dense3_fixed")
    bool shell_on = true;            // KD6, the bit-parallel shell pass between KD3 and KF (option "dense_shell")
    int shell_min_words = kShellMinWords;   // option "shell_min_words"
    bool standby_far = true;         // stand-by pipeline behind a trusted dense tier = the far-field pair (bounded whatever the scene
                                     // turns into), not fused K12 + K3/16 with unbounded scans (option "standby_far")
    bool standby_fold = true;        // the stand-by x sweep's launch folds the maxima and publishes the status block itself (option "standby_fold")
    bool standby_single = true;      // the stand-by pair and the fold are ONE guarded launch whose workgroups take tiles by ticket (k_envelope_standby;
                                     // option "standby_single"; 0: the y and the x sweep as two launches)
    int standby_grid = 1024;         // workgroups of the stand-by launches (LOOP form; option "standby_grid"): 4 per CU = all resident at once
    // Serpentine tile order (option "ball_serpentine"): a whole build that writes the buffer the handle's last KD launch wrote, at
    // the same size, walks KD's tiles in the opposite order -- it starts on the lines the last one finished with, which are
    // the ones the Infinity Cache still holds; walked the same way round every time, an LRU-like cache has evicted each
    // line just before it is reached.  Speed only: the field, the maxima and the flags do not depend on the order.
    bool ball_serpentine = true;
    // sweeps
    bool fused_zy = true;            // use K12 (z sweep fused into the y sweep) when the shape allows
    bool fused_always = false;       // ... whenever it does (option "fused_zy" = 2)
    int fused_h = 2;                 // its register-window radius at nz = 512: 2 or 3 (option "fused_window")
    bool plane16_on = true;          // use the int16 plane field + side table when the shape allows
    bool z_wave_on = true;           // z sweep with wave-private rows where nz allows it (option "z_wave"; 0 = the workgroup form)
    int x16_v = 4, x16_h = 3;        // K3/16 variant: voxels per lane, window radius
    int tune_ty = 0, tune_tx = 0;    // rows marched per thread by the y / x sweep (sdfgpu_set_tuning; 0 = automatic)
    bool i32_handoff = true;         // far-field pair: int32 plane field between the y and x sweeps (option "i32_handoff")
    bool dc_fixed = true;            // far-field kernel: the 512-voxel-line instances (option "dc_fixed")
    bool plane_skip = true;          // builds that go straight to the far-field pair: the z sweep marks the x-planes that hold a filled voxel,
                                     // the y sweep skips the tiles of the others, the x sweep their row loads (option "plane_skip")
    // ... and y tiles whose 16 lines are all flat-positive (a floor under open space) skip the search (option "flat_tiles")
    int flat_tiles = 1;              // (2: every such tile tries, whatever the habit says -- tests)
    // host side / debugging
    int host_pack = 1;       // host-buffer builds classify on the host and upload bits (option "host_pack"; 0 = upload the
                             // caller's mask / cells and classify on the device, as rounds 1 - 4 did)
    int defer_fold = 0;           // stage entry points leave their maxima in the slot array until sdfgpu_fold_extrema_device
    bool rs_plain_atomics = false;        // option "resample_plain_atomics": one atomic per lane (tools/resample_bench.py)
    bool rs_timing = false;               // option "resample_timing": events around the two kernels (sdfgpu_debug_resample_times)
};

// What the planner needs and only the build unit can know.  The gates come from the predicates beside the kernels' launchers
// (sdfgpu.hip), which also read the options that switch a kernel form off as a whole ("envelope_dc", "z_wave").
struct BuildFacts {
    int64_t nx = 0, ny = 0, nz = 0;  // canonical (canonical_dims)
    bool vb = false;                 // add_virtual_border
    enum class Occ : uint8_t { mask, cells, bits } occ = Occ::mask;
    bool occ16 = false;              // the occupancy pointer is 16-byte aligned
    bool out16 = false;              // d_out is
    bool dense_shape = false;        // the tuned ball kernels take the shape (dense_shape_ok: nz = 32 * 2^k words per row within a tile)
    bool far_shape[2] = {false, false};   // the far-field kernel takes the y / the x lines (far_geometry_ok, stages 2 and 3)
    bool z_wave_shape = false;       // wave-private z sweep (z_wave16_shape)
    bool fused_nz = false;           // K12 has an instance for nz (fused_zy_nz)
    bool dense_slot_free = false;    // the report slot of builds that carry the dense tier can be taken
    bool far_slot_free = false;      // ... of those that do not
};

struct BuildPlan {
    bool out16 = false;              // K3/16 and the tuned ball kernels store 16 bytes per lane: a field off that alignment takes the
    bool p16 = false;                // int32 plane field (p16 = int16 plane field + side table) and the generic dense kernel
    // Dense tier first: exact wherever the nearest opposite voxel is within d^2 <= 8; it raises kSwUncertified otherwise, in which
    // case (and only then) the general pipeline behind it does any work.
    bool dense = false;              // enqueued at all, in either form
    bool dense_generic = false;      // ... in the generic form (any nz, virtual border, any alignment of the field)
    DensePlan tier;                  // ... the tuned form's: fix-up mode, KD3 in KD's place, KD3 + KF staged behind KD (DensePolicy::plan)
    enum class Bits : uint8_t { none, caller, copy, pack, rows };
    Bits bits = Bits::none;          // where the dense tier's bit field comes from: the caller's linear bit field in place (nz % 32 == 0:
                                     // it IS the [x][y][nz / 32] field K0 writes), a 16-byte-aligned copy of it, K0, or the generic
                                     // tier's own rows padded to whole words (launch_dense_generic)
    // Bounded marching scans + the far-field kernel behind them, on every shape that kernel takes; other shapes (lines beyond
    // 2048, keys beyond 32 bits) keep unbounded marching scans.
    bool far_ok = false;
    bool envelope = false;           // ... and this build uses them: not behind a dense tier that is trusted to certify the scene
    // Stand-by behind a TRUSTED dense tier (round 4).  It nearly always exits on its guard, so it must be
    // few launches with small grids -- and since the scene of a stream can change under the handle (dense -> far-field), it
    // must be BOUNDED whatever the scene turns into.  That is the far-field pair with no probes and no marching sweeps:
    // KE2 [guard] -> KE3 [guard], int32 hand-off, LOOP form (1024 workgroups each); KE2 takes its z distances straight from
    // the dense tier's bit field (zdist_from_bits), so no z sweep is launched in front: TWO guarded launches like the
    // K12 + K3/16 pair it replaces (a third one, a guarded K1, cost the dense-certified step 2.6 us: 0.1405 -> 0.1431 ms),
    // O(L log L) per line on any input (the old pair ran unbounded outward scans: tens of ms on the build in which a
    // dense scene turned into the two-box cloud).
    bool standby = false;
    bool standby_single = false;     // ... as ONE launch (k_envelope_standby)
    // K12 (fused z+y) only as the guarded stand-by behind a dense build that is expected to be certified
    // again; everywhere else K1 + K2 (rows from the int16 z field) scan much faster than the fused kernel
    // recomputes, and only they can hand a far-field y sweep to the envelope kernel.
    bool fused = false;
    // Device-side tier selection: the marching-vs-far-field choice of each axis is made INSIDE this build from a probe of the
    // sweep's own input, so a fresh context (the reference's API is one-shot: collision_map.hpp:680-712 builds and returns)
    // never runs a sweep that is thrown away, and a handle's latency does not depend on what it built before.
    bool select = false;
    bool predicted = false;          // the far-field pair without probes: the handle's recent builds were far-field on both axes, or
                                     // the caller forces it (FarHabit::plan)
    // Both axes far-field (decided by the y probe): the y sweep hands the x sweep exact int32 values in the side-table
    // buffer (used whole) instead of p16 + side table -- one store / one load per voxel, no saturation handling, and the
    // x probe is skipped.  kSwHandoff carries the choice on the device.
    bool handoff = false;            // (shapes without the 16-bit plane field hand int32 values over anyway)
    bool window_choice = false;      // the y probe also picks the marching window (the radius-8 one exists for 4-voxel lanes only)
    // a build that goes straight to the far-field pair lets the z sweep mark the x-planes that hold a filled voxel at all: a sensed
    // scene leaves most planes without one, and the pair skips them (y sweep: the planes' tiles; x sweep: their row loads)
    bool plane_skip = false;
    // Who folds the maxima and publishes the status block, and where the report (status block -> pinned host memory + an event)
    // goes.  A report is only taken when the previous one has been consumed: the event is then never re-recorded while the
    // host still waits for it, so even a caller that enqueues builds back to back without ever synchronising keeps feeding the
    // policy (a few builds late), and the builds in between skip the host write.
    // (only a build that carried the dense tier has anything to teach the dense policy: the builds of a pause leave its slot
    //  free, so that the PROBE at its end is the build whose verdict comes back -- with every build reporting, the slot was
    //  usually taken by a paused build when the probe came, its failure went unseen and the pause never grew; tests/policy_harness)
    // (a build without the dense tier reports to the second slot: its far flags teach far_predict -- the builds that probed: a
    //  predicted build's flags say nothing new, and a report is PCIe writes the fold waits for)
    enum class Report : uint8_t { none, dense, far };
    Report report = Report::none;
    bool standby_folds = false;      // the stand-by x sweep's launch folds (one launch less behind the dense kernel); else the fold kernel
    // scratch fields the build needs, in bytes (0: not needed); build_device_impl allocates them all before it enqueues anything
    size_t yz_bytes = 0;             // int32 plane field / side table
    size_t plane16_bytes = 0;        // 16-bit plane field
    size_t z_bytes = 0;              // z field (the stand-by pair takes its z distances from the bit field, K12 computes them itself)
    size_t bits_bytes = 0;           // the library's bit field (Bits::copy, pack, rows)
    size_t unc_bytes = 0;            // undecided words of a fix-up stage that cannot live in the z field's storage
    size_t planebits_bytes = 0;      // row / x-plane occupancy flags (plane_skip)

    bool z_sweep() const { return !fused && !standby; }
    bool far_pair() const { return standby || predicted; }    // KE2 -> KE3 directly: no probes, no marching launches
};

// where the row bits lie behind the row and plane bytes of the plane-skip flags (k_pack_row_flags)
inline size_t plane_row_bits_offset(int64_t nx, int64_t ny) { return ((size_t)(nx * ny + nx) + 255) & ~(size_t)255; }

// One call per build: DensePolicy::plan and FarHabit::plan are called exactly once each, in this order (they count builds).
inline BuildPlan plan_build(const BuildOptions& o, DensePolicy& pol, FarHabit& far, const BuildFacts& f) {
    BuildPlan p;
    const int64_t n = f.nx * f.ny * f.nz;
    p.out16 = f.out16;
    p.p16 = o.plane16_on && (f.nz % 4) == 0 && ((f.ny * f.nz) % 8) == 0 && f.out16;
    const bool tuned = o.dense_on && f.dense_shape && f.ny <= 0x7fffffff && f.out16;
    // shapes / modes the tuned dense kernels do not take go through their generic forms (any nz, virtual border)
    const bool generic = !tuned && o.dense_on && o.dense_generic_on && f.nx <= 0x7fffffff && f.ny <= 0x7fffffff;
    // (d3_shape_ok: KD3's tiles hold whole z-rows of up to 256 words)
    p.tier = pol.plan(tuned || generic, generic, f.nz / 32 <= 256, f.vb);
    p.dense = p.tier.dense;
    p.dense_generic = p.dense && generic;
    const bool trusted = pol.expect_dense && p.dense;
    p.far_ok = o.envelope_on && f.far_shape[0] && f.far_shape[1];
    p.envelope = p.far_ok && !trusted;
    p.standby = p.far_ok && o.standby_far && trusted && !o.fused_always;
    p.standby_single = p.standby && o.standby_single;
    // (both plane fields are the library's own allocations: aligned)
    p.fused = !p.standby && o.fused_zy && f.occ == BuildFacts::Occ::mask && f.fused_nz && f.occ16 &&
              (o.fused_always || trusted || (!p.envelope && !p.dense));
    p.select = p.envelope && !p.fused;
    p.predicted = far.plan(p.select, o.force_env >= 0);
    p.handoff = p.select && p.p16 && o.i32_handoff;
    p.window_choice = p.select && (f.nz % 4) == 0;
    p.plane_skip = p.predicted && o.plane_skip && f.nx >= 8 && f.ny <= 1024 && f.z_wave_shape && f.occ != BuildFacts::Occ::cells &&
                   (f.occ == BuildFacts::Occ::bits || f.occ16);
    if (p.dense_generic) p.bits = BuildPlan::Bits::rows;
    else if (p.dense) p.bits = f.occ != BuildFacts::Occ::bits ? BuildPlan::Bits::pack : f.occ16 ? BuildPlan::Bits::caller : BuildPlan::Bits::copy;
    if (o.envelope_on && f.dense_slot_free && p.dense) p.report = BuildPlan::Report::dense;
    else if (p.select && !p.predicted && f.far_slot_free) p.report = BuildPlan::Report::far;
    p.standby_folds = p.standby && o.standby_fold;
    p.yz_bytes = (size_t)n * 4;
    p.plane16_bytes = p.p16 ? (size_t)n * 2 : 0;
    p.z_bytes = p.z_sweep() ? (size_t)n * 2 : 0;
    if (p.bits == BuildPlan::Bits::rows) p.bits_bytes = (size_t)(f.nx * f.ny * ((f.nz + 31) / 32)) * 4;
    else if (p.bits == BuildPlan::Bits::copy || p.bits == BuildPlan::Bits::pack) p.bits_bytes = (size_t)n / 8;
    // a fix-up stage in KD's place keeps its undecided words in a field of their own; a staged one borrows the z field's storage
    // (which the general pipeline only writes after KF has consumed them) wherever the build has a z field
    if (p.tier.fix_mode_build() || (p.tier.staged && !p.z_sweep())) p.unc_bytes = (size_t)n / 8;
    if (p.plane_skip) p.planebits_bytes = plane_row_bits_offset(f.nx, f.ny) + (size_t)f.nx * ((f.ny + 31) / 32) * 4;
    return p;
}

}  // namespace sdfgpu
