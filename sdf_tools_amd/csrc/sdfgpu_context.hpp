// sdfgpu_context.hpp -- the handle behind include/sdfgpu.h (struct sdfgpu_context) and what the host code of every translation
// unit needs from it: errors, the allocator with its red zones, the argument checks that more than one family shares, the staged
// host transfers.  Host code only.  The non-template functions are defined in sdfgpu_context.hip, except build_device_impl and
// convex_sdf, which sdfgpu.hip (the unit that launches the build kernels) offers to the families.  The options a build reads
// (BuildOptions) and what it decides from them on the host (plan_build) are in sdfgpu_plan.hpp, plain C++ like the policy header.
//
// It includes no kernel header, so that a unit which includes it gains no device code: a kernel defined in sdfgpu_kernels.hpp or
// one of its sibling build headers is launched from sdfgpu.hip only, and a unit that wants those headers' constants defines
// SDFGPU_AUX_TU and includes them itself (its copies of their kernels are then static, and it must not launch them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdfgpu_plan.hpp"
#include "sdfgpu_hostteam.hpp"
#include "sdfgpu.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace sdfgpu {

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
};

// Cross-stream ordering of work that shares state of the handle: an event behind the last such work and the stream it was
// recorded on.  Work on that stream is ordered by the stream itself; work on any other stream waits for the event first.
struct StreamOrder {
    hipEvent_t ev = nullptr;         // created on first use
    hipStream_t stream = nullptr;    // where ev was last recorded
    bool recorded = false;
    hipError_t create() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    hipError_t wait(hipStream_t s) const { return recorded && s != stream ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
    hipError_t record(hipStream_t s) {
        hipError_t e = create();
        if (e == hipSuccess && (e = hipEventRecord(ev, s)) == hipSuccess) { recorded = true; stream = s; }
        return e;
    }
    // `s` becomes the recorded stream WITHOUT a record: for a caller that has just waited on `s` and enqueues a sequence there whose
    // steps would each wait again, ending in record(s).  Until then another stream's wait sees the event as the previous work left it.
    hipError_t adopt(hipStream_t s) { const hipError_t e = create(); if (e == hipSuccess) { recorded = true; stream = s; } return e; }
    hipError_t host_wait() const { return recorded ? hipEventSynchronize(ev) : hipSuccess; }
    void destroy() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; recorded = false; }
    struct RecordAtExit { StreamOrder& order; hipStream_t s; ~RecordAtExit() { (void)order.record(s); } };   // record(s) on every path out of a scope
};

// Every DeviceBuffer of the context, and nothing else: sdfgpu_destroy and the "redzone" switch walk them as an array, so a buffer
// added here is freed by the one and released by the other.
struct ContextBuffers {
    DeviceBuffer zfield;     // int16 [N]   K1 output
    DeviceBuffer yzfield;    // int32 [N]   K2 output (32-bit pipeline) / side table (16-bit pipeline)
    DeviceBuffer plane16;    // int16 [N]   plane field of the 16-bit pipeline
    DeviceBuffer bits;       // uint32 [N/32] packed occupancy of the dense path
    DeviceBuffer unc;        // uint32 [N/32] undecided bits handed from the dense ball kernel to its fix-up kernel
    DeviceBuffer tileflag;   // uint32 [tiles] which waves of a tile wrote unc words (kept zero between builds)
    DeviceBuffer fix_order;  // uint32 [kFixRows] (dx, dy) rows of the fix-up kernel sorted by dx^2 + dy^2
    DeviceBuffer tagmask;    // uint8 [N] mask produced by the tagged-object classify kernel
    DeviceBuffer tagids;     // uint32 object id filter
    DeviceBuffer stage_in;   // host-API staging: mask / cells
    DeviceBuffer stage_bits; // host-API staging: the host-classified bit field (1 bit per voxel, linear order)
    DeviceBuffer stage_out;  // host-API staging: sdf
    DeviceBuffer query_stage;   // host-API staging of the three point calls: points | three result sections (with_staged_points)
    DeviceBuffer cc_scratch;    // sdfgpu_components*: root flags, ranks, chunk counts, K (sdfgpu_components.hpp)
    DeviceBuffer tp_scratch;    // sdfgpu_component_topology*: counters, status, node bytes, node offsets (sdfgpu_topology.hpp)
    DeviceBuffer tp_nodes;      // sdfgpu_component_topology*: one union-find word per surface-vertex node
    DeviceBuffer sf_scratch;    // sdfgpu_component_surfaces*: per-label counts, status, surface bit words (sdfgpu_surfaces.hpp)
    DeviceBuffer sf_sort;       // sdfgpu_component_surfaces*: the sort's pair buffers and histogram table
    DeviceBuffer sf_indices;    // sdfgpu_component_surfaces / _cells: the indices on their way to the caller's host buffer
    DeviceBuffer cx_scratch;    // sdfgpu_local_extrema* / sdfgpu_convex_segments_cells: doubling state, next, stats, ranks (sdfgpu_convex.hpp)
    DeviceBuffer cx_field;      // sdfgpu_local_extrema: the field; sdfgpu_convex_segments_cells: the named-object SDF, then the extrema
    // Batches of same-shape grids (sdfgpu_batch.hpp).  Scratch of their own: a batch build leaves the single builds' fields, status
    // block, result block and policy as they were.
    DeviceBuffer batch_field;   // int16 [batch][N] signed in-plane d^2 between k_batch_zy and k_batch_x_finish
    DeviceBuffer batch_ext;     // uint32 [batch][2] per-grid maxima | 32 words: the single builds' result block while a slow-path batch runs
    DeviceBuffer batch_res;     // double [batch] per-grid resolutions
    DeviceBuffer batch_gscale;  // GradScale [batch] of sdfgpu_gradient_batch_device
    DeviceBuffer planebits;  // row_any [nx * ny] bytes | plane_any [nx] bytes | row_bits [nx][ceil(ny / 32)] words (k_sweep_z_wave16, k_pack_row_flags, EnvDcArgs)
    DeviceBuffer rs_scratch; // sdfgpu_resample_cells*: one winner word per result cell, the counter (sdfgpu_resample.hpp)
    DeviceBuffer ball_bits;  // sdfgpu_dense_ball_device / sdfgpu_slab_dense_phase: copy of a caller's bit planes that are off 16 bytes
    DeviceBuffer ball_out;   // ... and the field of such a call while the caller's is off 16 bytes (launch_ball_dense)
    DeviceBuffer dp_scratch; // sdfgpu_display_*: status, draw keys, drawn bit words, tile counts, segment sums (sdfgpu_display.hpp)
    DeviceBuffer dp_sort;    // sdfgpu_display_select_*: the sort's pair buffers and table; the sorted keys when the caller takes none
    DeviceBuffer dp_out;     // host forms of sdfgpu_display_select_*: indices, keys, group keys and offsets on their way to the caller
    DeviceBuffer sc_scratch; // sdfgpu_rasterize_shapes*: status, world bounds per shape, candidate bits per coarse region (sdfgpu_scene.hpp)
    DeviceBuffer mr_scratch; // sdfgpu_rasterize_meshes*: status, first slot per mesh, tile scan, world vertices and id per triangle (sdfgpu_mesh.hpp)
    DeviceBuffer ms_toggle;  // sdfgpu_rasterize_solid_meshes*: one toggle bit per cell, columns padded to words; all zero between calls (sdfgpu_mesh_solid.hpp)
    DeviceBuffer cs_scratch; // sdfgpu_component_stats_device: the counter, one record per label in 0 .. label_count (sdfgpu_components.hip)
    DeviceBuffer* begin() { return &zfield; }
    DeviceBuffer* end() { return begin() + sizeof(ContextBuffers) / sizeof(DeviceBuffer); }
};
static_assert(sizeof(ContextBuffers) == 36 * sizeof(DeviceBuffer), "ContextBuffers holds DeviceBuffer members only");

// What the sdfgpu_last_* and sdfgpu_debug_* calls report about the most recent build or stage call.
struct LastBuild {
    hipStream_t last_stream = nullptr;
    double last_resolution = 1.0;
    int64_t last_n = 0;
    bool have_result = false;
    int64_t last_dims[3] = {0, 0, 0};
    bool last_fused = false;
    bool last_plane16 = false;
    bool last_dense = false;
    bool last_standby = false;       // the last build carried the far-field stand-by pair behind a trusted dense tier
    bool last_standby_single = false;  // ... as one launch (k_envelope_standby)
    bool last_dense3 = false, last_staged = false;   // ... ran KD3 + KF in KD's place / carried them behind KD, guarded on its verdict
    bool last_predicted = false;     // the last build took the far-field pair on the strength of the handle's recent builds: no probes, no marching launches
    bool last_lines_tiered = false;  // the last sdfgpu_sweep_x_lines_device call chose its tier on the device (probe / forced tier + far-field kernel behind the marching sweep)
    int last_dc_x = 0;               // 1 + the far-field kernel instance (launch_envelope_kernel's `which`) of the last x sweep launched through it; 0: none since the last build / lines call began
    bool last_plane_skip = false;    // the last build skipped the x-planes without a filled voxel (sdfgpu_debug_copy_yzsweep fills them in)
};

// Where a build's occupancy comes from: a byte mask, or cell records (the float occupancy at `off` of every `stride` bytes; 0.5 is
// filled iff `unknown`), or one bit per voxel in linear order (sdfgpu_build_bits*: the tuned dense kernels read it in place, the z
// sweep and the generic dense tier through their bit loaders -- no byte mask exists).  Exactly one of the three pointers is set;
// device memory for the launchers and build_device_impl, host memory for upload_packed and build_host_impl.
struct Occupancy {
    const uint8_t* mask = nullptr;
    const void* cells = nullptr;
    size_t stride = 0, off = 0;
    int unknown = 0;
    const uint32_t* bits = nullptr;
    static Occupancy of_mask(const uint8_t* m) { Occupancy o; o.mask = m; return o; }
    static Occupancy of_cells(const void* c, size_t stride, size_t off, int unknown) {
        Occupancy o; o.cells = c; o.stride = stride; o.off = off; o.unknown = unknown; return o;
    }
    static Occupancy of_bits(const uint32_t* b) { Occupancy o; o.bits = b; return o; }
    bool null() const { return !mask && !cells && !bits; }
};

// What a launcher is told about the device words around its launch, spelt out at the call site.
// guard: the launch does its work iff *guard != 0; kUnguarded: always.
constexpr const uint32_t* kUnguarded = nullptr;
// far_flag of a marching sweep: its outward scans are bounded (kScanExpectNear) and one that gives up raises the word, which guards
// the far-field kernel behind the sweep; kUnbounded: unbounded scans, nothing raised.
constexpr uint32_t* kUnbounded = nullptr;
constexpr hipStream_t kNullStream = nullptr;  // the host-buffer entry points work on the null stream of the context's device
constexpr int32_t* kNoSideTable = nullptr;    // d_side of a y sweep: int32 plane values, not the int16 plane field + side table

}  // namespace sdfgpu

struct sdfgpu_context : sdfgpu::ContextBuffers {
    int device = 0;
    std::string error;
    sdfgpu::BuildOptions opt;
    sdfgpu::LastBuild last;
    size_t cx_stats_off = 0;    // where the last extrema call left its CxStats in cx_scratch (0 = no call yet)
    int cx_rounds = 0;          // doubling rounds of that call
    char* batch_pin = nullptr;  // pinned ring through which per-grid parameters reach the device without a host wait
    size_t batch_pin_cap = 0, batch_pin_off = 0;
    std::vector<double> batch_resolutions;   // of the last batch build (sdfgpu_get_extrema_batch)
    int batch_fast = 0, batch_launches = 0;  // sdfgpu_last_batch_info
    bool batch_valid = false;
    size_t tag_cached_bytes = 0;            // stage_in holds the tagged cell records of the last sdfgpu_build_tagged_cells call
    void* pin[2] = {nullptr, nullptr};      // pinned host staging of copy_to_host (two chunks in flight)
    // Red zones (round 6, VERDICT r5 "next round" 2): with SDFGPU_REDZONE=1 in the environment of sdfgpu_create (or option
    // "redzone") every device allocation of the library -- the scratch fields, the status block, the slots, the staging buffers,
    // what sdfgpu_device_malloc hands out -- carries kRzPad canary bytes in front and behind, and every ABI call that may have
    // launched something ends with one check kernel over all of them (then synchronises): a store outside a buffer fails the
    // call that made it, with the buffer's name (SDFGPU_ERR_REDZONE).  The only net rounds 1 - 5 had was the VALUE of the
    // output, and a store past the end of a field lived in the product for three rounds.
    bool redzone = false;
    int rz_depth = 0;                       // entry points call each other: the outermost one checks
    struct Zone { std::string name; char* base; char* user; size_t bytes, total; };
    std::vector<Zone> zones;
    bool rz_table_dirty = true;
    void* rz_table = nullptr;               // device copy of {base, user bytes, total} per zone + results
    size_t rz_table_cap = 0;
    sdfgpu::HostTeam* team = nullptr;       // the host threads that fill / drain the staging chunks: created with the first staged
                                            // transfer, parked between calls, joined by sdfgpu_destroy (sdfgpu_hostteam.hpp)
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    uint32_t* d_small = nullptr;   // the status block, indexed by StatusWord (sdfgpu_kernels.hpp)
    // "this handle's scene is a far-field scene on both axes": learnt from the status blocks that come back (never a wait).  Such a
    // build skips the two probes and the three guarded marching launches (35 us of a 0.8 - 1.4 ms build) and enqueues KE2 -> KE3
    // directly (int32 hand-off); every 16th build probes again.  The far-field pair is exact on any scene: a wrong prediction costs
    // time, never a voxel.  Option "far_predict" (0 off, 1 on, 2 every build: tests and the fuzz).
    sdfgpu::FarHabit far;            // (sdfgpu_policy.hpp: plain C++, driven on the CPU by tests/policy_harness.cpp)
    uint32_t* h_far = nullptr;       // second report slot (pinned): builds that do not carry the dense tier report their far flags here
    uint32_t* h_far_dev = nullptr;
    hipEvent_t far_ev = nullptr;
    bool far_pending = false;
    sdfgpu::DensePolicy pol;      // what the handle has learned about its scenes' dense tier (sdfgpu_policy.hpp)
    bool flat_score_reset = false;   // "policy_reset": the next build clears the device-side habit of the two-valued tiles (kSwFlatScore)
    const float* serp_out = nullptr; // "ball_serpentine": output buffer and voxel count of the last whole-build KD launch, and its direction
    int64_t serp_n = 0;
    int serp_flip = 0;
    bool dc_attr_set[16] = {};   // MaxDynamicSharedMemorySize raised, per far-field kernel instantiation
    bool standby_attr_set[2] = {};   // ... per instance of the single stand-by launch (k_envelope_standby)
    int k1_resident = 0;             // workgroups of k_sweep_z_vec16 the device holds at once (persistent grid size)
    uint32_t* d_slots = nullptr;     // [kSlots][kSlotWords] extrema / flag slots of the dense kernel (kept zero between launches)
    uint32_t* d_result = nullptr;    // [kStatusWords] the status block of the last finished build (d_small is cleared by its fold)
    bool small_clean = false;        // d_small is all zero (left so by the previous build's fold kernel)
    uint32_t* h_flags_dev = nullptr; // device-side address of h_flags
    uint32_t* h_flags = nullptr;     // pinned host copy of the status block, written by the fold kernel of every build
    hipEvent_t flags_ev = nullptr;
    bool flags_pending = false;
    sdfgpu::StreamOrder build_order;      // recorded behind every build (and every stage call that uses the status block):
                                          // work on another stream waits for it first
    sdfgpu::StreamOrder cx_order;         // recorded behind every local-extrema computation, whose last three kernels are still
                                          // pending on its stream when the call returns: one on another stream waits for it first
    sdfgpu::StreamOrder rs_order;         // recorded behind every resample, which may return with its kernels pending on its
                                          // stream: one on another stream waits for it before it clears the winner words
    sdfgpu::StreamOrder sc_order;         // recorded behind every shape rasterisation (the same rule, for sc_scratch)
    sdfgpu::StreamOrder mr_order;         // recorded behind every mesh rasterisation (the same rule, for mr_scratch)
    sdfgpu::StreamOrder cs_order;         // recorded behind every component statistics call (the same rule, for cs_scratch)
    bool ms_dirty = false;                // a solid mesh call failed between a scatter and its merge: ms_toggle is cleared before its next use
    hipEvent_t rs_time_ev[3] = {nullptr, nullptr, nullptr};   // "resample_timing"
    bool rs_timed = false;
    int profiling = 0;            // 0 off, 1 an event behind every stage, 2 events around the dense ball kernel only,
                                  // 3 like 2 but only on every 4th build
    uint32_t profiled_builds = 0; // builds seen while profiling (level 3 samples every 4th)
    std::vector<hipEvent_t> event_pool;   // recycled profiling events
    std::vector<hipEvent_t> events;   // 8 per profiled build: start, after pack, ball, K1, K2/K12, KE2, K3, KE3
};

namespace sdfgpu {

// ---- errors and allocation ------------------------------------------------------------------------------------------------------
// the message goes to the handle (sdfgpu_last_error), or, without one, to the calling thread's creation error; returns `code`
int fail(sdfgpu_handle h, int code, const char* fmt, ...);

#define HIP_TRY(h, expr)                                                                  \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(h, SDFGPU_ERR_HIP, "HIP error %d (%s) at %s", (int)e_,            \
                        hipGetErrorString(e_), #expr);                                    \
    } while (0)

// every device allocation of the library goes through here (name = what a red-zone report calls it)
int rz_malloc(sdfgpu_handle h, const char* name, size_t bytes, void** out);
int rz_free(sdfgpu_handle h, void* ptr);
// b holds at least `bytes` afterwards (its old contents are gone when it had to grow)
int ensure(sdfgpu_handle h, DeviceBuffer& b, size_t bytes, const char* name = "scratch");
// stage_in for a new input of `bytes`.  Whoever overwrites stage_in drops the tagged cell records cached in it
// (sdfgpu_context::tag_cached_bytes), so every such caller comes through here.
int stage_input(sdfgpu_handle h, size_t bytes);
// One kernel over every zone, then a synchronisation (debug mode: calls become synchronous).  Overwritten zones fail the call
// with the buffer's name and are repaired, so that the next call reports only what IT did.
int redzone_check(sdfgpu_handle h, hipStream_t s);

// What every entry point that may launch something runs its body in: no handle, no call (the body may take h for granted); with
// red zones on, the outermost body is followed by the check of every zone.
template <class F>
int rz_wrap(sdfgpu_handle h, void* stream, F&& body) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!h->redzone) return body();
    ++h->rz_depth;
    int rc = body();
    if (--h->rz_depth == 0) {
        const int rz = redzone_check(h, (hipStream_t)stream);
        if (rz != SDFGPU_OK) rc = rz;
    }
    return rc;
}

// ---- argument checks shared by more than one family --------------------------------------------------------------------------------
// singleton axes to the front (the EDT is symmetric under axis renaming; see the definition)
void canonical_dims(int64_t& nx, int64_t& ny, int64_t& nz);
int check_dims(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz);          // the SDF build's limits
int check_resolution(sdfgpu_handle h, double resolution);
// positive dimensions and at most 2^32 - 1 voxels; `tail` ends the message of the second refusal ("... voxels: <tail>")
int check_dims_u32(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz, const char* tail);
constexpr const char* kLabelsTail = "uint32 component labels cannot number it";     // components, topology, surfaces
int check_cell_layout(sdfgpu_handle h, size_t stride, size_t occ_off);
int check_tagged_layout(sdfgpu_handle h, size_t stride, size_t occ_off, size_t obj_off);
int check_component_layout(sdfgpu_handle h, size_t stride, size_t occ_off, size_t comp_off);

// ---- transfers and staging ----------------------------------------------------------------------------------------------------
int copy_to_host(sdfgpu_handle h, void* dst, const void* d_src, size_t bytes, hipStream_t st = nullptr);
int copy_from_host(sdfgpu_handle h, void* d_dst, const void* src, size_t bytes, hipStream_t st = nullptr);
// host cells / mask (occ) -> one bit per voxel (host team) -> h->stage_bits, enqueued on `st`; the host buffer has been consumed
// when this returns
int upload_packed(sdfgpu_handle h, const Occupancy& occ, int64_t n, hipStream_t st);
// the caller's host bit field (ceil(n / 32) words) -> h->stage_bits
int upload_bits(sdfgpu_handle h, const uint32_t* bits, int64_t n, hipStream_t st);
// The cell records of the two tagged entry points in stage_in: uploaded, or (cells == nullptr) those the previous tagged call on
// this handle left on the device.
int stage_tagged_records(sdfgpu_handle h, const void* cells, size_t bytes);
// host labels / cell records -> stage_out (labels) and, unless every voxel is selected, stage_bits (selection); *out_selected
// says which
int stage_labels_selection(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select, const void* cells, size_t stride, size_t occ_off,
                           size_t comp_off, int class_mask, int64_t n, bool* out_selected);

// ---- what the build unit (sdfgpu.hip) offers the families -------------------------------------------------------------------------
// occ (device) -> d_out (device), enqueued on `s`
int build_device_impl(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                      float* d_out, hipStream_t s);
// records in stage_in -> SDF in stage_out (float), the virtual-border or the free-and-named-objects form
int convex_sdf(sdfgpu_handle h, size_t stride, size_t occ_off, size_t obj_off, int64_t nx, int64_t ny, int64_t nz, double resolution,
               int add_virtual_border);

// ---- templates (their callers pass lambdas) -----------------------------------------------------------------------------------------
// Device -> pageable host memory at PCIe rate, for destinations nobody has touched yet (the std::vector / numpy array
// the reference API returns is fresh: 512^3 floats are 131 072 first-touch page faults, ~40 ms on one thread, and a plain
// hipMemcpy takes them one by one on the runtime's copy thread).  The DMA lands in two pinned staging chunks of the
// context; a small team of host threads copies each chunk out while the next one is in flight, so the faults are spread
// over the team and overlap the transfer.  Enqueued on `st` (ordered after the work already there).  (Round 1 pre-touched the destination from threads running beside the upload:
// the faults and the runtime's pinning of the source pages fought over the address space, and the 128 MiB upload took
// 29 ms instead of 2.5.)  Returns when the data is in dst.
constexpr size_t kPinChunk = (size_t)32 << 20;
constexpr size_t kPinMin = (size_t)4 << 20;      // below this a plain (runtime-staged) copy is as fast as the team

// `drain(src, offset_in_download, len)` consumes bytes [offset, offset + len) of the download from pinned (or, for transfers
// below kPinMin, temporary) host memory: a memcpy for copy_to_host, the scatter of labels into cell records for
// sdfgpu_components_cells.
template <class Drain>
int staged_download_hip(sdfgpu_handle h, const void* d_src, size_t bytes, hipStream_t st, Drain drain) {
    if (bytes == 0) return SDFGPU_OK;
    for (int i = 0; i < 2 && bytes >= kPinMin; ++i) {
        if (!h->pin[i] && hipHostMalloc(&h->pin[i], kPinChunk, hipHostMallocDefault) != hipSuccess) h->pin[i] = nullptr;
        if (h->pin[i] && !h->pin_ev[i] && hipEventCreateWithFlags(&h->pin_ev[i], hipEventDisableTiming) != hipSuccess) h->pin_ev[i] = nullptr;
    }
    if (bytes < kPinMin || !h->pin[0] || !h->pin[1] || !h->pin_ev[0] || !h->pin_ev[1]) {
        (void)hipGetLastError();
        std::vector<char> tmp(std::min(bytes, kPinChunk));
        for (size_t o = 0; o < bytes; o += tmp.size()) {
            const size_t len = std::min(tmp.size(), bytes - o);
            HIP_TRY(h, hipMemcpyAsync(tmp.data(), static_cast<const char*>(d_src) + o, len, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            drain(tmp.data(), o, len);
        }
        return SDFGPU_OK;
    }
    if (!h->team) h->team = new (std::nothrow) HostTeam();
    if (!h->team) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "out of host memory");
    // (the scheduler is host-only code, tests/sched_harness.cpp runs it under -fsanitize=thread: sdfgpu_hostteam.hpp)
    hipError_t herr = hipSuccess;
    const int rc = staged_drain(
        *h->team, bytes, kPinChunk, host_team_size(16),
        [&](int64_t i, int buf, size_t len) -> int {
            herr = hipMemcpyAsync(h->pin[buf], static_cast<const char*>(d_src) + (size_t)i * kPinChunk, len, hipMemcpyDeviceToHost, st);
            if (herr == hipSuccess) herr = hipEventRecord(h->pin_ev[buf], st);
            return herr == hipSuccess ? 0 : 1;
        },
        [&](int buf) -> int { herr = hipEventSynchronize(h->pin_ev[buf]); return herr == hipSuccess ? 0 : 1; },
        [&](int buf, size_t off, size_t goff, size_t len) { drain(static_cast<const char*>(h->pin[buf]) + off, goff, len); });
    if (rc != 0) {
        (void)hipDeviceSynchronize();
        return fail(h, SDFGPU_ERR_HIP, "HIP error %d (%s) in the device-to-host copy", (int)herr, hipGetErrorString(herr));
    }
    return SDFGPU_OK;
}

// Pageable host -> device, the mirror image of copy_to_host: a synchronous hipMemcpy from pageable memory goes through
// the runtime's staging copy on one host thread (measured: 128 MiB in 24 - 30 ms, i.e. 5 GB/s, where the link does 52);
// here a team of threads fills the two pinned chunks and the DMA of one chunk overlaps the filling of the next.
// Enqueued on `st`; returns when the last chunk's DMA has completed.
// `fill(dst, out_offset, len)` produces bytes [out_offset, out_offset + len) of the upload into dst (slices are multiples
// of 4096 bytes except the last): a plain memcpy for copy_from_host, the cells / mask -> bits classification for the
// host-buffer builds (round 5), which is what makes the team worth more than a copy -- it reads 8 or 64 bytes per byte sent.
template <class Fill>
int staged_upload_hip(sdfgpu_handle h, void* d_dst, size_t bytes, hipStream_t st, int team_cap, Fill fill) {
    if (bytes == 0) return SDFGPU_OK;
    for (int i = 0; i < 2; ++i) {
        if (!h->pin[i] && hipHostMalloc(&h->pin[i], kPinChunk, hipHostMallocDefault) != hipSuccess) h->pin[i] = nullptr;
        if (h->pin[i] && !h->pin_ev[i] && hipEventCreateWithFlags(&h->pin_ev[i], hipEventDisableTiming) != hipSuccess) h->pin_ev[i] = nullptr;
    }
    if (!h->pin[0] || !h->pin[1] || !h->pin_ev[0] || !h->pin_ev[1]) {
        // no pinned staging (a locked-memory limit): produce the bytes into a pageable temporary, one runtime-staged copy each
        // (slower, never wrong -- ADVICE r5: rounds 1 - 4 had this fallback, round 5 had dropped it)
        (void)hipGetLastError();
        std::vector<char> tmp(std::min(bytes, kPinChunk));
        for (size_t o = 0; o < bytes; o += tmp.size()) {
            const size_t len = std::min(tmp.size(), bytes - o);
            fill(tmp.data(), o, len);
            HIP_TRY(h, hipMemcpyAsync(static_cast<char*>(d_dst) + o, tmp.data(), len, hipMemcpyHostToDevice, st));
            HIP_TRY(h, hipStreamSynchronize(st));           // (tmp is refilled by the next round)
        }
        return SDFGPU_OK;
    }
    if (!h->team) h->team = new (std::nothrow) HostTeam();
    if (!h->team) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "out of host memory");
    hipError_t herr = hipSuccess;
    const int rc = sdfgpu::staged_upload(
        *h->team, bytes, kPinChunk, host_team_size(team_cap),
        [&](int buf, size_t off, size_t goff, size_t len) { fill(static_cast<char*>(h->pin[buf]) + off, goff, len); },
        [&](int64_t i, int buf, size_t len) -> int {
            herr = hipMemcpyAsync(static_cast<char*>(d_dst) + (size_t)i * kPinChunk, h->pin[buf], len, hipMemcpyHostToDevice, st);
            if (herr == hipSuccess) herr = hipEventRecord(h->pin_ev[buf], st);
            return herr == hipSuccess ? 0 : 1;
        },
        [&](int buf) -> int { herr = hipEventSynchronize(h->pin_ev[buf]); return herr == hipSuccess ? 0 : 1; });
    if (rc != 0) {
        (void)hipDeviceSynchronize();
        return fail(h, SDFGPU_ERR_HIP, "HIP error %d (%s) in the host-to-device copy", (int)herr, hipGetErrorString(herr));
    }
    return SDFGPU_OK;
}

// Host staging of the three point calls (sdfgpu_query_points, sdfgpu_project_points, sdfgpu_query_gradients) in query_stage, which
// grows on demand and is re-used by the next call: points (24 bytes each) | three result sections of per_point[i] bytes per point,
// the last one padded to 256 bytes.  Uploads the points, runs launch(device points, device sections: null where the caller passed
// no out[i]) and downloads the sections that were asked for, in their order.
template <class Launch>
int with_staged_points(sdfgpu_handle h, const double* points, int64_t n_points, const size_t (&per_point)[3], void* const (&out)[3], Launch launch) {
    const size_t n = (size_t)n_points;
    size_t off[4] = {n * 24, 0, 0, 0};
    for (int i = 0; i < 3; ++i) off[i + 1] = off[i] + n * per_point[i];
    if (int rc = ensure(h, h->query_stage, off[2] + ((n * per_point[2] + 255) & ~(size_t)255), "query staging")) return rc;
    char* const base = (char*)h->query_stage.ptr;
    char* const dev[3] = {out[0] ? base + off[0] : nullptr, out[1] ? base + off[1] : nullptr, out[2] ? base + off[2] : nullptr};
    // Round 5: the null stream of the context's device, ordered behind this handle's last build by its event --
    // not h->last.last_stream, which is a handle of the CALLER's (an earlier *_device build's stream may have been destroyed since).
    // A field produced ELSEWHERE (another handle, a caller's kernel) is ordered by the null stream's implicit synchronisation only
    // when its stream is a blocking one: producers on hipStreamNonBlocking streams (PyTorch's are) must be synchronised by the caller
    // before this call -- include/sdfgpu.h says so.
    HIP_TRY(h, h->build_order.wait(nullptr));
    if (int rc = copy_from_host(h, base, points, n * 24, nullptr)) return rc;
    if (int rc = launch((const double*)base, dev)) return rc;
    for (int i = 0; i < 3; ++i) if (out[i]) if (int rc = copy_to_host(h, out[i], dev[i], n * per_point[i], nullptr)) return rc;
    return SDFGPU_OK;
}

}  // namespace sdfgpu
