// sdfgpu.hip -- C ABI (include/sdfgpu.h) over the gfx950 kernels in sdfgpu_kernels.hpp.
// Host side of the drop-in boundary for sdf_generation::ExtractSignedDistanceField
// (reference include/sdf_tools/sdf_generation.hpp:209-420).  No CPU fallback.
#include "sdfgpu_kernels.hpp"
#include "sdfgpu_sweep_x16.hpp"
#include "sdfgpu_sweep_y16.hpp"
#include "sdfgpu_dense3.hpp"
#include "sdfgpu_dense6.hpp"
#include "sdfgpu_fused_zy.hpp"
#include "sdfgpu_dense.hpp"
#include "sdfgpu_envelope_dc.hpp"
#include "sdfgpu_policy.hpp"
#include "sdfgpu_hostteam.hpp"
#include "sdfgpu_components.hpp"
#include "sdfgpu_topology.hpp"
#include "sdfgpu_surfaces.hpp"
#include "sdfgpu_convex.hpp"
#include "sdfgpu_project.hpp"
#include "sdfgpu_query.hpp"
#include "sdfgpu_batch.hpp"
#include "sdfgpu_resample.hpp"
#include "sdfgpu_display.hpp"

#include <sys/mman.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

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

#include "../../include/sdfgpu.h"

using namespace sdfgpu;

namespace {

constexpr int kH = 3;            // register-window radius of the marching sweeps
constexpr int64_t kMaxDim = 16384;

thread_local std::string g_create_error = "";

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
    DeviceBuffer batch_ext;     // uint32 [batch][2] per-grid maxima | 24 words: the single builds' result block while a slow-path batch runs
    DeviceBuffer batch_res;     // double [batch] per-grid resolutions
    DeviceBuffer batch_gscale;  // GradScale [batch] of sdfgpu_gradient_batch_device
    DeviceBuffer planebits;  // row_any [nx * ny] bytes | plane_any [nx] bytes | row_bits [nx][ceil(ny / 32)] words (k_sweep_z_wave16, k_pack_row_flags, EnvDcArgs)
    DeviceBuffer rs_scratch; // sdfgpu_resample_cells*: one winner word per result cell, the counter (sdfgpu_resample.hpp)
    DeviceBuffer ball_bits;  // sdfgpu_dense_ball_device / sdfgpu_slab_dense_phase: copy of a caller's bit planes that are off 16 bytes
    DeviceBuffer ball_out;   // ... and the field of such a call while the caller's is off 16 bytes (launch_ball_dense)
    DeviceBuffer dp_scratch; // sdfgpu_display_*: status, draw keys, drawn bit words, tile counts, segment sums (sdfgpu_display.hpp)
    DeviceBuffer dp_sort;    // sdfgpu_display_select_*: the sort's pair buffers and table; the sorted keys when the caller takes none
    DeviceBuffer dp_out;     // host forms of sdfgpu_display_select_*: indices, keys, group keys and offsets on their way to the caller
    DeviceBuffer* begin() { return &zfield; }
    DeviceBuffer* end() { return begin() + sizeof(ContextBuffers) / sizeof(DeviceBuffer); }
};
static_assert(sizeof(ContextBuffers) == 32 * sizeof(DeviceBuffer), "ContextBuffers holds DeviceBuffer members only");

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
    CellLoader cell_loader() const { return CellLoader{reinterpret_cast<const char*>(cells), (int64_t)stride, (int64_t)off, unknown}; }
};

// What a launcher is told about the device words around its launch, spelt out at the call site.
// guard: the launch does its work iff *guard != 0; kUnguarded: always.
constexpr const uint32_t* kUnguarded = nullptr;
// far_flag of a marching sweep: its outward scans are bounded (kScanExpectNear) and one that gives up raises the word, which guards
// the far-field kernel behind the sweep; kUnbounded: unbounded scans, nothing raised.
constexpr uint32_t* kUnbounded = nullptr;
constexpr hipStream_t kNullStream = nullptr;  // the host-buffer entry points work on the null stream of the context's device
constexpr int32_t* kNoSideTable = nullptr;    // d_side of a y sweep: int32 plane values, not the int16 plane field + side table

}  // namespace

struct sdfgpu_context : ContextBuffers {
    int device = 0;
    std::string error;
    BuildOptions opt;
    LastBuild last;
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
    HostTeam* team = nullptr;               // the host threads that fill / drain the staging chunks: created with the first staged
                                            // transfer, parked between calls, joined by sdfgpu_destroy (sdfgpu_hostteam.hpp)
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    uint32_t* d_small = nullptr;   // the status block, indexed by StatusWord (sdfgpu_kernels.hpp)
    // "this handle's scene is a far-field scene on both axes": learnt from the status blocks that come back (never a wait).  Such a
    // build skips the two probes and the three guarded marching launches (35 us of a 0.8 - 1.4 ms build) and enqueues KE2 -> KE3
    // directly (int32 hand-off); every 16th build probes again.  The far-field pair is exact on any scene: a wrong prediction costs
    // time, never a voxel.  Option "far_predict" (0 off, 1 on, 2 every build: tests and the fuzz).
    FarHabit far;                    // (sdfgpu_policy.hpp: plain C++, driven on the CPU by tests/policy_harness.cpp)
    uint32_t* h_far = nullptr;       // second report slot (pinned): builds that do not carry the dense tier report their far flags here
    uint32_t* h_far_dev = nullptr;
    hipEvent_t far_ev = nullptr;
    bool far_pending = false;
    DensePolicy pol;              // what the handle has learned about its scenes' dense tier (sdfgpu_policy.hpp)
    bool flat_score_reset = false;   // "policy_reset": the next build clears the device-side habit of the two-valued tiles (kSwFlatScore)
    const float* serp_out = nullptr; // "ball_serpentine": output buffer and voxel count of the last whole-build KD launch, and its direction
    int64_t serp_n = 0;
    int serp_flip = 0;
    bool dc_attr_set[16] = {};   // MaxDynamicSharedMemorySize raised, per far-field kernel instantiation
    int k1_resident = 0;             // workgroups of k_sweep_z_vec16 the device holds at once (persistent grid size)
    uint32_t* d_slots = nullptr;     // [kSlots][kSlotWords] extrema / flag slots of the dense kernel (kept zero between launches)
    uint32_t* d_result = nullptr;    // [8] the status block of the last finished build (d_small is cleared by its fold)
    bool small_clean = false;        // d_small is all zero (left so by the previous build's fold kernel)
    uint32_t* h_flags_dev = nullptr; // device-side address of h_flags
    uint32_t* h_flags = nullptr;     // pinned host copy of the status block, written by the fold kernel of every build
    hipEvent_t flags_ev = nullptr;
    bool flags_pending = false;
    StreamOrder build_order;              // recorded behind every build (and every stage call that uses the status block):
                                          // work on another stream waits for it first
    StreamOrder cx_order;                 // recorded behind every local-extrema computation, whose last three kernels are still
                                          // pending on its stream when the call returns: one on another stream waits for it first
    StreamOrder rs_order;                 // recorded behind every resample, which may return with its kernels pending on its
                                          // stream: one on another stream waits for it before it clears the winner words
    hipEvent_t rs_time_ev[3] = {nullptr, nullptr, nullptr};   // "resample_timing"
    bool rs_timed = false;
    int profiling = 0;            // 0 off, 1 an event behind every stage, 2 events around the dense ball kernel only,
                                  // 3 like 2 but only on every 4th build
    uint32_t profiled_builds = 0; // builds seen while profiling (level 3 samples every 4th)
    std::vector<hipEvent_t> event_pool;   // recycled profiling events
    std::vector<hipEvent_t> events;   // 8 per profiled build: start, after pack, ball, K1, K2/K12, KE2, K3, KE3
};

namespace {

int fail(sdfgpu_handle h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->error = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(h, expr)                                                                  \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(h, SDFGPU_ERR_HIP, "HIP error %d (%s) at %s", (int)e_,            \
                        hipGetErrorString(e_), #expr);                                    \
    } while (0)

constexpr size_t kRzPad = 4096;
constexpr int kRzByte = 0xC5;

// every device allocation of the library goes through here (name = what a red-zone report calls it)
int rz_malloc(sdfgpu_handle h, const char* name, size_t bytes, void** out) {
    *out = nullptr;
    if (!h->redzone) {
        HIP_TRY(h, hipMalloc(out, bytes));
        return SDFGPU_OK;
    }
    const size_t total = kRzPad + ((bytes + 255) & ~(size_t)255) + kRzPad;
    char* base = nullptr;
    HIP_TRY(h, hipMalloc((void**)&base, total));
    HIP_TRY(h, hipMemset(base, kRzByte, kRzPad));
    HIP_TRY(h, hipMemset(base + kRzPad + bytes, kRzByte, total - kRzPad - bytes));      // (from the first byte behind the buffer)
    h->zones.push_back({name, base, base + kRzPad, bytes, total});
    h->rz_table_dirty = true;
    *out = base + kRzPad;
    return SDFGPU_OK;
}
int rz_free(sdfgpu_handle h, void* ptr) {
    if (!ptr) return SDFGPU_OK;
    for (size_t i = 0; i < h->zones.size(); ++i)
        if (h->zones[i].user == ptr) {
            char* base = h->zones[i].base;
            h->zones.erase(h->zones.begin() + (long)i);
            h->rz_table_dirty = true;
            HIP_TRY(h, hipFree(base));
            return SDFGPU_OK;
        }
    HIP_TRY(h, hipFree(ptr));               // (allocated before the switch went on)
    return SDFGPU_OK;
}

int ensure(sdfgpu_handle h, DeviceBuffer& b, size_t bytes, const char* name = "scratch") {
    if (b.bytes >= bytes && b.ptr) return SDFGPU_OK;
    if (b.ptr) { if (int rc = rz_free(h, b.ptr)) return rc; b.ptr = nullptr; b.bytes = 0; }
    // (red zones: the buffer is exactly as large as asked for, so that the first byte behind it is canary)
    const size_t want = h->redzone ? std::max<size_t>(bytes, 4) : std::max<size_t>(bytes, 256);
    if (int rc = rz_malloc(h, name, want, &b.ptr)) return rc;
    b.bytes = want;
    return SDFGPU_OK;
}

__global__ __launch_bounds__(256) void k_redzone_check(const uint64_t* __restrict__ table, uint32_t* __restrict__ result) {
    // table[3 z] = base address, [3 z + 1] = user bytes, [3 z + 2] = total bytes; result[2 z] = overwritten bytes, [2 z + 1] = first
    // overwritten byte as an offset from the buffer's start + kRzPad (so that "before the buffer" stays non-negative)
    const int z = blockIdx.x;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(table[3 * z]);
    const size_t bytes = table[3 * z + 1], total = table[3 * z + 2];
    __shared__ uint32_t cnt, first;
    if (threadIdx.x == 0) { cnt = 0u; first = 0xFFFFFFFFu; }
    __syncthreads();
    uint32_t c = 0, f = 0xFFFFFFFFu;
    for (size_t i = threadIdx.x; i < kRzPad; i += 256) if (base[i] != (unsigned char)kRzByte) { ++c; f = min(f, (uint32_t)i); }
    for (size_t i = kRzPad + bytes + threadIdx.x; i < total; i += 256)
        if (base[i] != (unsigned char)kRzByte) { ++c; f = min(f, (uint32_t)min(i - bytes, (size_t)0xFFFFFFFEu)); }
    if (c) { atomicAdd(&cnt, c); atomicMin(&first, f); }
    __syncthreads();
    if (threadIdx.x == 0) { result[2 * z] = cnt; result[2 * z + 1] = first; }
}

// One kernel over every zone, then a synchronisation (debug mode: calls become synchronous).  Overwritten zones fail the call
// with the buffer's name and are repaired, so that the next call reports only what IT did.
int redzone_check(sdfgpu_handle h, hipStream_t s) {
    const size_t nz = h->zones.size();
    if (!h->redzone || nz == 0) return SDFGPU_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t need = nz * 3 * 8 + nz * 2 * 4;
    if (h->rz_table_cap < need) {
        if (h->rz_table) HIP_TRY(h, hipFree(h->rz_table));
        h->rz_table = nullptr;
        h->rz_table_cap = 0;
        HIP_TRY(h, hipMalloc(&h->rz_table, need * 2));
        h->rz_table_cap = need * 2;
        h->rz_table_dirty = true;
    }
    uint32_t* d_res = reinterpret_cast<uint32_t*>(static_cast<char*>(h->rz_table) + nz * 3 * 8);
    if (h->rz_table_dirty) {
        std::vector<uint64_t> t(nz * 3);
        for (size_t i = 0; i < nz; ++i) { t[3 * i] = reinterpret_cast<uint64_t>(h->zones[i].base); t[3 * i + 1] = h->zones[i].bytes; t[3 * i + 2] = h->zones[i].total; }
        HIP_TRY(h, hipStreamSynchronize(s));
        HIP_TRY(h, hipMemcpy(h->rz_table, t.data(), nz * 3 * 8, hipMemcpyHostToDevice));
        h->rz_table_dirty = false;
    }
    hipLaunchKernelGGL(k_redzone_check, dim3((unsigned)nz), dim3(256), 0, s, (const uint64_t*)h->rz_table, d_res);
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> res(nz * 2);
    HIP_TRY(h, hipMemcpyAsync(res.data(), d_res, nz * 2 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    std::string msg;
    for (size_t i = 0; i < nz; ++i) {
        if (res[2 * i] == 0) continue;
        const sdfgpu_context::Zone& z = h->zones[i];
        char buf[256];
        const long long off = (long long)res[2 * i + 1] - (long long)kRzPad;
        snprintf(buf, sizeof buf, "%s'%s' (%zu bytes): %u canary bytes overwritten, the first %lld bytes %s", msg.empty() ? "" : "; ", z.name.c_str(), z.bytes,
                 res[2 * i], off < 0 ? -off : off - (long long)z.bytes, off < 0 ? "BEFORE its start" : "BEHIND its end");
        msg += buf;
        (void)hipMemset(z.base, kRzByte, kRzPad);
        (void)hipMemset(z.base + kRzPad + z.bytes, kRzByte, z.total - kRzPad - z.bytes);
    }
    if (!msg.empty()) return fail(h, SDFGPU_ERR_REDZONE, "red zone: a kernel of this call stored outside %s", msg.c_str());
    return SDFGPU_OK;
}

template <class F>
int rz_wrap(sdfgpu_handle h, void* stream, F&& body) {
    if (!h || !h->redzone) return body();
    ++h->rz_depth;
    int rc = body();
    if (--h->rz_depth == 0) {
        const int rz = redzone_check(h, (hipStream_t)stream);
        if (rz != SDFGPU_OK) rc = rz;
    }
    return rc;
}

// The EDT is symmetric under axis renaming, and a grid with singleton axes has
// the same memory layout when those axes are moved to the front (index =
// x*ny*nz + y*nz + z).  Canonicalising keeps the contiguous axis long, so 2-D
// grids (the reference's test_bindings.py case is 20x40x1) sweep coalesced.
void canonical_dims(int64_t& nx, int64_t& ny, int64_t& nz) {
    if (nz == 1) { nz = ny; ny = nx; nx = 1; }
    if (nz == 1) { nz = ny; ny = nx; nx = 1; }
    if (ny == 1) { ny = nx; nx = 1; }
}

int check_dims(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "grid dimensions must be positive (got %lld x %lld x %lld)",
                    (long long)nx, (long long)ny, (long long)nz);
    if (nx > kMaxDim || ny > kMaxDim || nz > kMaxDim || nx * nx + ny * ny + nz * nz >= (int64_t)kInf32)
        return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE,
                    "grid %lld x %lld x %lld exceeds the supported extent (dims <= 16384, nx^2+ny^2+nz^2 < 2^30)",
                    (long long)nx, (long long)ny, (long long)nz);
    return SDFGPU_OK;
}

// include/sdfgpu.h "Resolutions": positive and finite (subnormal and huge finite values included), refused before anything is enqueued
int check_resolution(sdfgpu_handle h, double resolution) {
    if (!(resolution > 0.0) || !std::isfinite(resolution))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resolution must be positive and finite (got %g)", resolution);
    return SDFGPU_OK;
}

// The record layouts of the cell entry points: every field 4-byte aligned and inside the record.
int check_cell_layout(sdfgpu_handle h, size_t stride, size_t occ_off) {
    if (stride < 4 || (stride % 4) || (occ_off % 4) || occ_off + 4 > stride)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cell_stride/occupancy_offset must be 4-byte aligned and in range");
    return SDFGPU_OK;
}
int check_tagged_layout(sdfgpu_handle h, size_t stride, size_t occ_off, size_t obj_off) {
    if (stride < 8 || (stride % 4) || (occ_off % 4) || (obj_off % 4) || occ_off + 4 > stride || obj_off + 4 > stride)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cell layout must be 4-byte aligned and in range");
    return SDFGPU_OK;
}
int check_component_layout(sdfgpu_handle h, size_t stride, size_t occ_off, size_t comp_off) {
    if (stride < 8 || (stride % 4) || (occ_off % 4) || (comp_off % 4) || occ_off + 4 > stride || comp_off + 4 > stride || occ_off == comp_off)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cell_stride / occupancy_offset / component_offset must be 4-byte aligned, in range and distinct");
    return SDFGPU_OK;
}

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
        hipLaunchKernelGGL(k_sweep_z_generic<CellLoader>, grid, block, lds, s, occ.cell_loader(), d_out, nrows, (int)nz, rpb, guard);
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
bool fused_zy_eligible(const sdfgpu_context* h, const uint8_t* d_mask, const void* d_out, int64_t nz) {
    return h->opt.fused_zy && d_mask && (nz == 512 || nz == 1024) &&
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

bool plane16_eligible(const sdfgpu_context* h, int64_t ny, int64_t nz) {
    return h->opt.plane16_on && (nz % 4) == 0 && ((ny * nz) % 8) == 0;
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

// Picks the kernel instance for `a` (a.ntiles = the tiles of this launch) and launches it.
int launch_envelope_kernel(sdfgpu_handle h, int stage, EnvDcArgs& a, bool loop, bool probe, hipStream_t s) {
    constexpr int NL = kDcLines;
    // vector loads: 4 consecutive lines per load, whole tiles, aligned rows
    auto al = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; };
    const bool vec = !a.bits && (a.nz % 4) == 0 && (a.group_lines % NL) == 0 && al(a.in16, 8) && al(a.side_in, 16) && al(a.in_i32, 16);
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

// K0 + KD: pack to bits, then the bit-parallel ball kernel (sdfgpu_dense.hpp)
constexpr int kBallLanes = 256;                   // lanes per workgroup of KD, KD3, KD6 and KF
constexpr int kDenseMaxRowWords = 64;             // longest z-row the tuned dense kernels take, in 32-voxel words (DenseArgs::nzw)
static_assert(kDenseMaxRowWords <= kBallLanes, "a ball-kernel tile holds at least one z-row: launch_ball_dense divides by kBallLanes / nzw");
bool dense_eligible(const sdfgpu_context* h, int64_t nz) {       // (with or without virtual border: the tuned ball kernel folds it itself)
    const int64_t nzw = nz / 32;
    return h->opt.dense_on && (nz % 32) == 0 && nzw >= 1 && nzw <= kDenseMaxRowWords && (nzw & (nzw - 1)) == 0;
}

// K0: byte mask or cell records -> bits (a bit field needs no packing: callers do not come here with one)
int launch_pack_bits(sdfgpu_handle h, const Occupancy& occ, int64_t n, uint32_t* d_bits, hipStream_t s) {
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    if (occ.cells) {
        hipLaunchKernelGGL(k_pack_bits_generic<CellLoader>, grid, block, 0, s, occ.cell_loader(), d_bits, n);
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
    static const int level_d2[7] = {1, 2, 3, 4, 5, 6, 8};
    for (int l = 0; l < 7; ++l) a.mag[l] = (float)(std::sqrt((double)level_d2[l]) * resolution);
    a.mag[7] = 0.0f;
    static const int level3_d2[13] = {1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14};
    for (int l = 0; l < 16; ++l) a.mag3[l] = l < 13 ? (float)(std::sqrt((double)level3_d2[l]) * resolution) : 0.0f;
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

// Generic dense tier (any nz, virtual border): k_pack_bits_rows + k_ball_dense_generic
int launch_dense_generic(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                         float* d_out, uint32_t* d_uncert, hipStream_t s) {
    const int64_t nzw = (nz + 31) / 32, nrows = nx * ny, nwords = nrows * nzw;
    if (nwords > 0x7fffffffLL * (int64_t)kBlock) return fail(h, SDFGPU_ERR_UNSUPPORTED_SIZE, "dense grid too large");
    if (int rc = ensure(h, h->bits, (size_t)nwords * 4, "bit field")) return rc;
    const dim3 grid((unsigned)((nwords + kBlock - 1) / kBlock)), block(kBlock);
    uint32_t* const rows = (uint32_t*)h->bits.ptr;
    if (occ.bits)                                               // (linear bits -> rows padded to whole words)
        hipLaunchKernelGGL(k_pack_bits_rows<BitsLoader>, grid, block, 0, s, BitsLoader{occ.bits}, rows, nrows, (int)nz, (int)nzw);
    else if (occ.cells)
        hipLaunchKernelGGL(k_pack_bits_rows<CellLoader>, grid, block, 0, s, occ.cell_loader(), rows, nrows, (int)nz, (int)nzw);
    else
        hipLaunchKernelGGL(k_pack_bits_rows<MaskLoader>, grid, block, 0, s, MaskLoader{occ.mask}, rows, nrows, (int)nz, (int)nzw);
    HIP_TRY(h, hipGetLastError());
    DenseGenArgs a{};
    a.bits = (const uint32_t*)h->bits.ptr; a.out = d_out;
    a.nx = (int)nx; a.ny = (int)ny; a.nz = (int)nz; a.nzw = (int)nzw; a.vb = vb;
    static const int level_d2[7] = {1, 2, 3, 4, 5, 6, 8};
    for (int l = 0; l < 7; ++l) a.mag[l] = (float)(std::sqrt((double)level_d2[l]) * resolution);
    a.mag[7] = 0.0f;
    a.slots = h->d_slots; a.uncertified = d_uncert;
    hipLaunchKernelGGL(k_ball_dense_generic, grid, block, 0, s, a);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

int build_device_impl(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, double resolution, int vb,
                      float* d_out, hipStream_t s) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (occ.null() || !d_out) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null device pointer");
    if (occ.bits && (reinterpret_cast<uintptr_t>(occ.bits) % 4) != 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "the bit field must be 4-byte aligned");
    if (int rc = check_resolution(h, resolution)) return rc;
    if (int rc = check_dims(h, nx, ny, nz)) return rc;
    if (occ.cells) if (int rc = check_cell_layout(h, occ.stride, occ.off)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    canonical_dims(nx, ny, nz);
    h->last.last_dc_x = 0;
    h->last.last_lines_tiered = false;
    const int64_t n = nx * ny * nz;
    // (the caller's pointers need element alignment only, sdfgpu.h "Conventions": K3/16 and the tuned ball kernels store 16 bytes
    //  per lane, so a field off that alignment takes the int32 plane field -- launch_sweep_x tests the pointer itself -- and the
    //  generic dense kernel, which store floats)
    const bool out16 = (reinterpret_cast<uintptr_t>(d_out) % 16) == 0;
    const bool p16 = plane16_eligible(h, ny, nz) && out16;
    if (int rc = ensure(h, h->yzfield, (size_t)n * 4, "int32 plane field / side table")) return rc;          // int32 plane field / side table
    if (p16) if (int rc = ensure(h, h->plane16, (size_t)n * 2, "16-bit plane field")) return rc;
    void* zy_out = p16 ? h->plane16.ptr : h->yzfield.ptr;
    int32_t* zy_side = p16 ? (int32_t*)h->yzfield.ptr : nullptr;
    bool dense = dense_eligible(h, nz) && ny <= 0x7fffffff && out16;
    // shapes / modes the tuned dense kernels do not take go through their generic forms (any nz, virtual border)
    const bool dense_generic = !dense && h->opt.dense_on && h->opt.dense_generic_on && nx <= 0x7fffffff && ny <= 0x7fffffff;
    dense = dense || dense_generic;
    // Learn from an earlier build on this handle, if its status block has arrived (never a wait), and plan the dense tier of
    // this one: sdfgpu_policy.hpp.  Every outcome is exact; the policy only decides whether and in which form the DENSE tier is
    // enqueued and whether the pipeline behind it may be the two-launch stand-by (which tier does a sweep is decided on the
    // device inside the build).
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
    const DensePlan plan = h->pol.plan(dense, dense_generic, nz / 32 <= 256, vb != 0);
    dense = plan.dense;
    // bounded marching scans + the far-field kernel behind them, on every shape that kernel takes; other shapes (lines beyond
    // 2048, keys beyond 32 bits) keep unbounded marching scans.  Shapes without the 16-bit plane field (nz % 4 != 0) hand
    // exact int32 plane values from the y to the x sweep.
    const bool far_ok = h->opt.envelope_on && far_geometry_ok(h, 2, nx, ny, nz) && far_geometry_ok(h, 3, nx, ny, nz);
    const bool envelope = far_ok && !(h->pol.expect_dense && dense);
    // Stand-by behind a TRUSTED dense tier (round 4).  It nearly always exits on its guard, so it must be
    // few launches with small grids -- and since the scene of a stream can change under the handle (dense -> far-field), it
    // must be BOUNDED whatever the scene turns into.  That is the far-field pair with no probes and no marching sweeps:
    // KE2 [guard] -> KE3 [guard], int32 hand-off, LOOP form (1024 workgroups each); KE2 takes its z distances straight from
    // the dense tier's bit field (zdist_from_bits), so no z sweep is launched in front: TWO guarded launches like the
    // K12 + K3/16 pair it replaces (a third one, a guarded K1, cost the dense-certified step 2.6 us: 0.1405 -> 0.1431 ms),
    // O(L log L) per line on any input (the old pair ran unbounded outward scans: tens of ms on the build in which a
    // dense scene turned into the two-box cloud).
    const bool standby = far_ok && h->opt.standby_far && h->pol.expect_dense && dense && !h->opt.fused_always;
    // Device-side tier selection: the marching-vs-far-field choice of each axis is made INSIDE this build from a probe of the
    // sweep's own input, so a fresh context (the reference's API is one-shot: collision_map.hpp:680-712 builds and returns)
    // never runs a sweep that is thrown away, and a handle's latency does not depend on what it built before.
    const bool dev_select = envelope;
    // K12 (fused z+y) only as the guarded stand-by behind a dense build that is expected to be certified
    // again; everywhere else K1 + K2 (rows from the int16 z field) scan much faster than the fused kernel
    // recomputes, and only they can hand a far-field y sweep to the envelope kernel.
    const bool fused = !standby && fused_zy_eligible(h, occ.mask, zy_out, nz) &&
                       (h->opt.fused_always || (dense && h->pol.expect_dense) || (!envelope && !dense));
    const bool select = dev_select && !fused;
    // (see far_predict: the handle's recent builds were far-field on both axes -- or the caller forces it)
    const bool predicted = h->far.plan(select, h->opt.force_env >= 0);
    if (!fused && !standby) if (int rc = ensure(h, h->zfield, (size_t)n * 2, "z field")) return rc;
    // status block [0..7]: maxima, status, uncertified, far flags, fix_needed.  Normally still zero from the previous
    // build's fold kernel; cleared here after a build that failed half-way (or before the first one)
    // Builds on one handle share its status block, extrema slots and scratch fields.  On the same stream they are
    // ordered by the stream; a build issued on ANOTHER stream first waits for the previous build's last kernel.
    HIP_TRY(h, h->build_order.wait(s));
    if (!h->small_clean) {
        HIP_TRY(h, hipMemsetAsync(h->d_small, 0, 128, s));
        HIP_TRY(h, hipMemsetAsync(h->d_slots, 0, (size_t)kSlots * kSlotWords * 4, s));   // a failed build may have left maxima behind
    }
    h->small_clean = false;
    // profiling marks: an event is recorded only behind a stage that launched something; a stage that
    // was not launched shares the previous mark (elapsed 0), so profiling adds as few packets as possible
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool launched_since_mark = true;
    // level 3 = level 2 on every 4th build (a sampled timing costs the loop a quarter of the event overhead)
    int prof = h->profiling;
    if (prof == 3) prof = ((h->profiled_builds++ & 3u) == 0 && dense) ? 2 : 0;
    auto mark = [&](int k) -> hipError_t {
        if (!prof) return hipSuccess;
        if (prof == 2 && dense) {
            // only the dominant kernel of the dense path is bracketed: stage 1 = [ev1, ev2], every other stage
            // shares a mark with its neighbour (elapsed 0)
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
    };
    HIP_TRY(h, mark(0));
    // Dense path first: exact wherever the nearest opposite voxel is within d^2 <= 8; raises
    // kSwUncertified otherwise, in which case (and only then) the general pipeline below does any work.
    uint32_t* const sw = h->d_small;                            // the status block, indexed by StatusWord
    bool cur_fix_mode = false, cur_dense3 = false, cur_staged = false;
    const uint32_t* dense_bits = nullptr;                       // the bit field the tuned dense kernels (and the stand-by y sweep) read
    uint8_t* row_any = nullptr;                                 // plane sparsity: one byte per z row, one per x-plane behind them (predicted far-field builds)
    h->last.last_dense = dense;
    if (dense && dense_generic) {
        HIP_TRY(h, mark(1));
        if (int rc = launch_dense_generic(h, occ, nx, ny, nz, resolution, vb, d_out, sw + kSwUncertified, s)) return rc;
        launched_since_mark = true;
    } else if (dense) {
        if (occ.bits && (reinterpret_cast<uintptr_t>(occ.bits) % 16) == 0) {
            dense_bits = occ.bits;                              // (nz % 32 == 0: the caller's linear bit field IS the [x][y][nz / 32] field K0 writes)
        } else if (occ.bits) {                                  // (the dense kernels stage bit rows with 16-byte loads)
            if (int rc = ensure(h, h->bits, (size_t)n / 8, "bit field")) return rc;
            HIP_TRY(h, hipMemcpyAsync(h->bits.ptr, occ.bits, (size_t)n / 8, hipMemcpyDeviceToDevice, s));
            dense_bits = (const uint32_t*)h->bits.ptr;
        } else {
            if (int rc = ensure(h, h->bits, (size_t)n / 8, "bit field")) return rc;
            if (int rc = launch_pack_bits(h, occ, n, (uint32_t*)h->bits.ptr, s)) return rc;
            launched_since_mark = true;
            dense_bits = (const uint32_t*)h->bits.ptr;
        }
        HIP_TRY(h, mark(1));
        // fix-up mode (policy): undecided voxels go to the fix-up kernel, which raises `uncertified` only for what it
        // cannot decide either; otherwise the ball kernel raises it directly and nothing extra is launched
        // (with a virtual border the fix-up kernel stays out: a voxel it would finish may still be bound by b >= 3)
        // (fix-up mode, KD3 in KD's place, the fix-up stage staged behind KD: DensePolicy::plan)
        const bool fix = plan.fix;
        cur_dense3 = plan.dense3;
        cur_staged = plan.staged;
        BallMode kd;
        kd.early_out = true; kd.vb = vb; kd.nx_glob = nx; kd.radius = cur_dense3 ? 3 : 2;
        if (fix || cur_dense3) kd.fix_needed = sw + kSwFixNeeded;
        if (!cur_dense3) {                                      // (KD; see ball_serpentine)
            kd.flip = (h->opt.ball_serpentine && d_out == h->serp_out && n == h->serp_n) ? !h->serp_flip : 0;
            h->serp_out = d_out; h->serp_n = n; h->serp_flip = kd.flip;
        }
        if (int rc = launch_ball_dense(h, dense_bits, d_out, nx, 0, nx, ny, nz, resolution,
                                       cur_staged ? sw + kSwDenseVerdict : sw + kSwUncertified, kd, s)) return rc;
        if (cur_staged) {                                       // KD3 + KF behind KD, guarded on its verdict
            BallMode kd3;
            kd3.early_out = true; kd3.nx_glob = nx; kd3.radius = 3; kd3.fix_needed = sw + kSwFixNeeded; kd3.guard = sw + kSwDenseVerdict;
            // (the undecided bits of this stage live in the z field's storage: launch_ball_dense)
            if (!fused && h->zfield.ptr && h->zfield.bytes >= (size_t)n / 8) { kd3.unc = (uint32_t*)h->zfield.ptr; kd3.unc_bytes = h->zfield.bytes; }
            if (int rc = launch_ball_dense(h, dense_bits, d_out, nx, 0, nx, ny, nz, resolution, sw + kSwUncertified, kd3, s)) return rc;
        }
        launched_since_mark = true;
        cur_fix_mode = fix || cur_dense3;
    } else {
        HIP_TRY(h, mark(1));
    }
    // what guards every launch of the general pipeline: "the dense tier left voxels undecided"
    const uint32_t* const general_guard = dense ? sw + kSwUncertified : kUnguarded;
    h->last.last_dense3 = cur_dense3;
    h->last.last_staged = cur_staged;
    HIP_TRY(h, mark(2));
    h->last.last_fused = fused;
    h->last.last_standby = standby;
    h->last.last_predicted = predicted;
    h->last.last_plane16 = p16;
    if (!fused && !standby) {                                   // (the stand-by pair takes its z distances from the bit field)
        // a build that goes straight to the far-field pair lets the z sweep mark the x-planes that hold a filled voxel at all: a sensed
        // scene leaves most planes without one, and the pair skips them (y sweep: the planes' tiles; x sweep: their row loads)
        if (predicted && h->opt.plane_skip && nx >= 8 && ny <= 1024 && z_wave16_shape(h, nz) && !occ.cells &&
            (occ.bits || (reinterpret_cast<uintptr_t>(occ.mask) % 16) == 0)) {
            const size_t o_bits = ((size_t)(nx * ny + nx) + 255) & ~(size_t)255;
            if (int rc = ensure(h, h->planebits, o_bits + (size_t)nx * ((ny + 31) / 32) * 4, "row / x-plane occupancy flags")) return rc;
            row_any = (uint8_t*)h->planebits.ptr;
        }
        if (int rc = launch_sweep_z(h, occ, nx, ny, nz, (int16_t*)h->zfield.ptr, general_guard, s, row_any)) return rc;
        launched_since_mark = true;
    }
    h->last.last_plane_skip = row_any != nullptr;
    h->last.last_dims[0] = nx; h->last.last_dims[1] = ny; h->last.last_dims[2] = nz;
    HIP_TRY(h, mark(3));
    const int16_t* const zf = (const int16_t*)h->zfield.ptr;
    int32_t* const yz = (int32_t*)h->yzfield.ptr;
    // Both axes far-field (decided by the y probe): the y sweep hands the x sweep exact int32 values in the side-table
    // buffer (used whole) instead of p16 + side table -- one store / one load per voxel, no saturation handling, and the
    // x probe is skipped.  kSwHandoff carries the choice on the device.
    const bool handoff = select && p16 && h->opt.i32_handoff;        // (shapes without the 16-bit plane field hand int32 values over anyway)
    // (the radius-8 y window exists for 4-voxel lanes only)
    const bool window_choice = select && (nz % 4) == 0;
    // (moved up: the stand-by x sweep does the fold itself and needs to know where the report goes)
    const bool report = h->opt.envelope_on && h->h_flags_dev && !h->flags_pending && dense;
    bool folded = false;
    if (standby || predicted) {
        // KE2 [general guard] -> KE3 [general guard], exact int32 plane values in between, each launch raising its far flag itself:
        // no probes, no marching launches
        DcIo ke2, ke3;
        ke2.out_i32 = yz; ke2.ran_flag = sw + kSwFarY;
        ke3.in_i32 = yz; ke3.out = d_out; ke3.ran_flag = sw + kSwFarX;
        if (standby) {                                          // LOOP form, z distances from the dense tier's bit field, self-reporting
            ke2.loop = ke3.loop = true;
            ke2.bits = dense_bits ? dense_bits : (const uint32_t*)h->bits.ptr; ke2.nzw = (int)((nz + 31) / 32);
            if (h->opt.standby_fold) {
                ke3.fold_result = h->d_result; ke3.fold_report = report ? h->h_flags_dev : nullptr; ke3.fold_ticket = sw + kSwFoldTicket;
                folded = true;
            }
        } else {
            ke2.in16 = zf;
            if (row_any) {
                // row bytes -> one bit per row, one byte per x-plane, "some plane is empty" (kSwPlaneEmpty)
                uint8_t* plane_any = row_any + nx * ny;
                uint32_t* row_bits = (uint32_t*)(row_any + (((size_t)(nx * ny + nx) + 255) & ~(size_t)255));
                const int row_words = (int)((ny + 31) / 32);
                if (h->flat_score_reset) { h->flat_score_reset = false; HIP_TRY(h, hipMemsetAsync(sw + kSwFlatScore, 0, 8, s)); }
                hipLaunchKernelGGL(k_pack_row_flags, dim3((unsigned)std::min<int64_t>((nx + 15) / 16, 16)), dim3(1024), 0, s, row_any, (int)nx, (int)ny, row_words, row_bits, plane_any, sw + kSwPlaneEmpty, sw + kSwFlatScore);
                HIP_TRY(h, hipGetLastError());
                ke2.row_bits = row_bits; ke2.row_words = row_words; ke2.plane_any = ke3.plane_any = plane_any;
            }
        }
        HIP_TRY(h, mark(4));                                    // (stage slot 3, the marching y sweep: nothing launched)
        if (int rc = launch_envelope(h, 2, ke2, nx, ny, nz, resolution, vb, general_guard, s)) return rc;
        launched_since_mark = true;
        HIP_TRY(h, mark(5));
        HIP_TRY(h, mark(6));                                    // (stage slot 5, the marching x sweep: nothing launched)
        if (int rc = launch_envelope(h, 3, ke3, nx, ny, nz, resolution, vb, general_guard, s)) return rc;
        launched_since_mark = true;
    } else {
        // A probe-selected build (`select`): per axis a probe that decides, the marching sweep behind its guard word with bounded
        // scans, and the far-field sweep behind the axis' far flag.  Every other build: one sweep per axis, unbounded scans, no far flag.
        uint32_t* const far_y = select ? sw + kSwFarY : kUnbounded;
        uint32_t* const far_x = select ? sw + kSwFarX : kUnbounded;
        // the far-field pair: p16 + side table in between, or exact int32 values (always on shapes without the 16-bit plane
        // field; behind kSwHandoff on the others)
        DcIo ke2, ke3;
        ke2.in16 = zf; ke3.out = d_out;
        if (p16) { ke2.out = h->plane16.ptr; ke2.side_out = yz; ke3.in16 = (const int16_t*)h->plane16.ptr; ke3.side_in = yz; }
        if (!p16 || handoff) { ke2.out_i32 = yz; ke3.in_i32 = yz; }
        if (p16 && handoff) ke2.i32_flag = ke3.i32_flag = sw + kSwHandoff;
        DcIo probe2;                                            // the y probe reads what KE2 reads (no hand-off flag: its own decision raises it)
        probe2.in16 = zf; probe2.out = h->plane16.ptr; probe2.side_out = yz;
        if (!p16) probe2.out_i32 = yz;
        DcDecide dy, dx;
        dy.stage = 0; dx.stage = 1;
        dy.dense_tried = dx.dense_tried = dense; dy.handoff = dx.handoff = handoff; dy.window_choice = dx.window_choice = window_choice;
        XSlab whole = XSlab::whole(nx);
        whole.status = sw + kSwSlabStatus;
        // y sweep
        if (select) {
            // probe + decision in one launch (the probe's last workgroup decides); a forced tier needs no probe
            if (h->opt.force_env < 0) {
                if (int rc = launch_envelope_probe(h, 2, probe2, nx, ny, nz, resolution, vb, general_guard, dy, s)) return rc;
            } else if (int rc = launch_decide(h, dy, s)) return rc;
            // marching y sweep: general pipeline needed AND near-field; the probe also picks the window (radius 3 / radius 8)
            if (int rc = launch_sweep_y(h, zf, zy_out, zy_side, nx, ny, nz, sw + kSwMarchY, far_y, s)) return rc;
            if (window_choice)
                if (int rc = launch_sweep_y(h, zf, zy_out, zy_side, nx, ny, nz, sw + kSwMarchYWide, far_y, s, YWindow::r8)) return rc;
        } else if (fused) {
            if (int rc = launch_sweep_zy_fused(h, occ.mask, zy_out, zy_side, nx, ny, nz, general_guard, s)) return rc;
        } else {                                                // (no far-field kernel for this shape / switched off: unbounded scans)
            if (int rc = launch_sweep_y(h, zf, zy_out, zy_side, nx, ny, nz, general_guard, kUnbounded, s)) return rc;
        }
        launched_since_mark = true;
        HIP_TRY(h, mark(4));
        if (select) {
            if (int rc = launch_envelope(h, 2, ke2, nx, ny, nz, resolution, vb, sw + kSwFarY, s)) return rc;
            launched_since_mark = true;
        }
        HIP_TRY(h, mark(5));
        // x sweep: same choice
        if (select) {
            if (h->opt.force_env < 0) {
                if (int rc = launch_envelope_probe(h, 3, ke3, nx, ny, nz, resolution, vb, general_guard, dx, s)) return rc;
            } else if (int rc = launch_decide(h, dx, s)) return rc;
        }
        const uint32_t* const march_x_guard = select ? sw + kSwMarchX : general_guard;
        if (p16) {
            if (int rc = launch_sweep_x16(h, (const int16_t*)h->plane16.ptr, yz, d_out, whole, ny, nz, resolution, vb, march_x_guard, far_x, s)) return rc;
        } else {
            if (int rc = launch_sweep_x(h, yz, d_out, whole, ny, nz, resolution, vb, march_x_guard, far_x, s)) return rc;
        }
        launched_since_mark = true;
        HIP_TRY(h, mark(6));
        if (select) {
            if (int rc = launch_envelope(h, 3, ke3, nx, ny, nz, resolution, vb, sw + kSwFarX, s)) return rc;
            launched_since_mark = true;
        }
    }
    // one kernel folds the maxima, publishes the status block (device copy for get_extrema, pinned host copy for the
    // next build's policy) and clears it for the next build
    // The report (status block -> pinned host memory + an event) is only taken when the previous report has been
    // consumed: the event is then never re-recorded while the host still waits for it, so even a caller that
    // enqueues builds back to back without ever synchronising keeps feeding the policy (a few builds late), and the
    // builds in between skip the host write.  What the reported build was (dense? fix-up? envelope mode?) is
    // remembered with the report -- not with whatever build happens to be the latest when it is read.
    // (only a build that carried the dense tier has anything to teach the policy: the builds of a pause leave the report slot
    //  free, so that the PROBE at its end is the build whose verdict comes back -- with every build reporting, the slot was
    //  usually taken by a paused build when the probe came, its failure went unseen and the pause never grew; tests/policy_harness)
    // (a stand-by build: the x sweep's launch has done it -- one launch less behind the dense kernel)
    // (a build without the dense tier reports to the second slot: its far flags teach far_predict)
    // (... the builds that probed: a predicted build's flags say nothing new, and a report is PCIe writes the fold waits for)
    const bool report_far = !report && select && !predicted && h->h_far_dev && !h->far_pending;
    if (!folded) if (int rc = fold_slots(h, h->d_small, s, h->d_result, report ? h->h_flags_dev : report_far ? h->h_far_dev : nullptr,
                                         report ? kReportDense : kReportFar)) return rc;
    if (report_far) {
        HIP_TRY(h, hipEventRecord(h->far_ev, s));
        h->far_pending = true;
    }
    h->small_clean = true;
    if (report) {
        HIP_TRY(h, hipEventRecord(h->flags_ev, s));
        h->flags_pending = true;
        h->pol.prev = ReportedBuild{dense, dense_generic, cur_fix_mode, cur_staged, predicted};
    }
    if (prof) {
        HIP_TRY(h, mark(7));
        for (auto e : ev) h->events.push_back(e);
    }
    HIP_TRY(h, h->build_order.record(s));
    h->last.last_stream = s;
    h->last.last_resolution = resolution;
    h->last.last_n = n;
    h->last.have_result = true;
    return SDFGPU_OK;
}

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

int copy_to_host(sdfgpu_handle h, void* dst, const void* d_src, size_t bytes, hipStream_t st = nullptr) {
    if (bytes == 0) return SDFGPU_OK;
    if (bytes < kPinMin) {
        HIP_TRY(h, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return SDFGPU_OK;
    }
    {   // huge pages on the 2 MiB-aligned interior, where the kernel grants them: one fault then maps 512 small pages' worth
        constexpr uintptr_t kHuge = (uintptr_t)2 << 20;
        const uintptr_t lo = (reinterpret_cast<uintptr_t>(dst) + kHuge - 1) & ~(kHuge - 1);
        const uintptr_t hi = (reinterpret_cast<uintptr_t>(dst) + bytes) & ~(kHuge - 1);
        if (hi > lo) (void)madvise(reinterpret_cast<void*>(lo), hi - lo, MADV_HUGEPAGE);
    }
    return staged_download_hip(h, d_src, bytes, st, [dst](const char* src, size_t goff, size_t len) { memcpy(static_cast<char*>(dst) + goff, src, len); });
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

int copy_from_host(sdfgpu_handle h, void* d_dst, const void* src, size_t bytes, hipStream_t st = nullptr) {
    if (bytes == 0) return SDFGPU_OK;
    if (bytes < kPinMin) {
        HIP_TRY(h, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return SDFGPU_OK;
    }
    return staged_upload_hip(h, d_dst, bytes, st, 16, [src](char* dst, size_t o, size_t len) { memcpy(dst, static_cast<const char*>(src) + o, len); });
}

// ---- host-side classification: cells / mask -> one bit per voxel (round 5) ----------------------------------
// Bit (v & 7) of byte (v >> 3) = voxel v is filled, with the predicates of the device classifiers: mask byte != 0;
// occupancy > 0.5f || (unknown_is_filled && occupancy == 0.5f) (collision_map.hpp:689-704 -- the reference compares the float
// with the double 0.5, which is the float 0.5f exactly; NaN is "free" in both).  out[0 .. len) covers voxels
// [8 ob, 8 (ob + len)); bits of voxels >= n are 0.
void pack_mask_bits(const uint8_t* m, int64_t n, size_t ob, size_t len, uint8_t* out) {
    const int64_t v0 = (int64_t)ob * 8, v1 = std::min<int64_t>(n, v0 + (int64_t)len * 8);
    int64_t v = v0;
    size_t o = 0;
#if defined(__SSE2__)
    const __m128i zero = _mm_setzero_si128();
    for (; v + 16 <= v1; v += 16, o += 2) {
        const __m128i x = _mm_loadu_si128(reinterpret_cast<const __m128i*>(m + v));
        const uint32_t nz = ~(uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(x, zero)) & 0xffffu;
        out[o] = (uint8_t)nz; out[o + 1] = (uint8_t)(nz >> 8);
    }
#else       // (hosts without SSE2: eight bytes -> eight bits by the multiply trick)
    for (; v + 8 <= v1; v += 8, ++o) {
        uint64_t x;
        memcpy(&x, m + v, 8);
        x = (x | ((x & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full)) & 0x8080808080808080ull;
        out[o] = (uint8_t)(((x >> 7) * 0x0102040810204080ull) >> 56);
    }
#endif
    for (; o < len; ++o) {
        uint32_t b = 0;
        for (int k = 0; k < 8; ++k, ++v) if (v < v1 && m[v]) b |= 1u << k;
        out[o] = (uint8_t)b;
    }
}
void pack_cells_bits(const char* cells, size_t stride, size_t off, int unknown, int64_t n, size_t ob, size_t len, uint8_t* out) {
    const int64_t v0 = (int64_t)ob * 8, v1 = std::min<int64_t>(n, v0 + (int64_t)len * 8);
    int64_t v = v0;
    size_t o = 0;
#if defined(__SSE2__)
    if (stride == 8 && (off == 0 || off == 4)) {                // COLLISION_CELL {float occupancy; uint32 component}: 4 records per pair of loads
        const __m128 half = _mm_set1_ps(0.5f);
        const __m128 unk = _mm_castsi128_ps(_mm_set1_epi32(unknown ? -1 : 0));
        const char* p = cells + (size_t)v0 * 8;
        for (; v + 8 <= v1; v += 8, ++o, p += 64) {
            uint32_t b = 0;
            for (int g = 0; g < 2; ++g) {
                const __m128 a0 = _mm_loadu_ps(reinterpret_cast<const float*>(p + 32 * g));
                const __m128 a1 = _mm_loadu_ps(reinterpret_cast<const float*>(p + 32 * g + 16));
                const __m128 occ = off == 0 ? _mm_shuffle_ps(a0, a1, _MM_SHUFFLE(2, 0, 2, 0)) : _mm_shuffle_ps(a0, a1, _MM_SHUFFLE(3, 1, 3, 1));
                const __m128 f = _mm_or_ps(_mm_cmpgt_ps(occ, half), _mm_and_ps(_mm_cmpeq_ps(occ, half), unk));
                b |= (uint32_t)_mm_movemask_ps(f) << (4 * g);
            }
            out[o] = (uint8_t)b;
        }
    }
#endif
    for (; o < len; ++o) {
        uint32_t b = 0;
        for (int k = 0; k < 8; ++k, ++v) {
            if (v >= v1) continue;
            float occ;
            memcpy(&occ, cells + (size_t)v * stride + off, 4);
            if (occ > 0.5f || (unknown && occ == 0.5f)) b |= 1u << k;
        }
        out[o] = (uint8_t)b;
    }
}

// Host cells / mask -> bits (team) -> device -> byte mask at d_mask_dst (n bytes), enqueued on `st`; the host buffer has been
// consumed when this returns (the unpack kernel is stream-ordered behind the upload).
// d_mask_dst == kBitsOnly: the bits stay in h->stage_bits and are the caller's input.
constexpr uint8_t* kBitsOnly = nullptr;
int upload_packed(sdfgpu_handle h, const Occupancy& occ, int64_t n, uint8_t* d_mask_dst, hipStream_t st) {
    const size_t nbytes = ((size_t)n + 7) / 8, padded = (nbytes + 3) & ~(size_t)3;
    if (int rc = ensure(h, h->stage_bits, padded, "bit staging")) return rc;
    auto fill = [=](char* dst, size_t o, size_t len) {
        const size_t real = o >= nbytes ? 0 : std::min(len, nbytes - o);
        if (real) {
            if (occ.cells) pack_cells_bits(static_cast<const char*>(occ.cells), occ.stride, occ.off, occ.unknown, n, o, real, reinterpret_cast<uint8_t*>(dst));
            else pack_mask_bits(occ.mask, n, o, real, reinterpret_cast<uint8_t*>(dst));
        }
        if (real < len) memset(dst + real, 0, len - real);
    };
    if (padded >= ((size_t)256 << 10)) {
        if (int rc = staged_upload_hip(h, h->stage_bits.ptr, padded, st, 32, fill)) return rc;
    } else {                                                    // small grids: one thread, one runtime-staged copy
        std::vector<char> tmp(padded);
        fill(tmp.data(), 0, padded);
        HIP_TRY(h, hipMemcpyAsync(h->stage_bits.ptr, tmp.data(), padded, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipStreamSynchronize(st));                   // (tmp goes out of scope)
    }
    if (d_mask_dst == kBitsOnly) return SDFGPU_OK;              // (the host-buffer builds: the bits are the build's input)
    const int64_t nch = (n + 15) / 16;
    hipLaunchKernelGGL(k_unpack_bits_mask, dim3((unsigned)((nch + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       (const uint32_t*)h->stage_bits.ptr, d_mask_dst, n);
    HIP_TRY(h, hipGetLastError());
    return SDFGPU_OK;
}

// the caller's host bit field (ceil(n / 32) words) -> h->stage_bits
int upload_bits(sdfgpu_handle h, const uint32_t* bits, int64_t n, hipStream_t st) {
    const size_t bytes = (((size_t)n + 31) / 32) * 4;
    if (int rc = ensure(h, h->stage_bits, bytes, "bit staging")) return rc;
    return copy_from_host(h, h->stage_bits.ptr, bits, bytes, st);
}

// `occ` is host memory (occ.bits: the caller's occupancy is already one bit per voxel, sdfgpu_build_bits).
// The cell records of the two tagged entry points in stage_in: uploaded, or (cells == nullptr) those the previous tagged call on
// this handle left on the device.
int stage_tagged_records(sdfgpu_handle h, const void* cells, size_t bytes) {
    if (!cells) {
        if (h->tag_cached_bytes == 0 || h->tag_cached_bytes != bytes)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cells is null and the handle holds no cell records of this size");
        return SDFGPU_OK;
    }
    h->tag_cached_bytes = 0;
    if (int rc = ensure(h, h->stage_in, bytes, "input staging")) return rc;
    if (int rc = copy_from_host(h, h->stage_in.ptr, cells, bytes)) return rc;
    h->tag_cached_bytes = bytes;
    return SDFGPU_OK;
}

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
    h->tag_cached_bytes = 0;                        // (stage_in is about to be overwritten)
    // Round 5: the host's thread team classifies the caller's buffer into one bit per voxel while it fills the pinned staging
    // chunk, and 1/8 B per voxel crosses PCIe (16 MiB at 512^3 instead of 128 MiB of mask or 1 GiB of COLLISION_CELL records);
    // k_unpack_bits_mask spreads them into the byte mask on the device.  Same predicate as the device classifier
    // (pack_cells_bits); "host_pack" = 0 keeps the upload-and-classify-on-device path (device-resident cells always take it).
    const bool packed = !occ.bits && (h->opt.host_pack == 2 || (h->opt.host_pack == 1 && in_bytes >= kPinMin));
    if (!packed && !occ.bits) if (int rc = ensure(h, h->stage_in, in_bytes, "input staging")) return rc;
    if (!d_out_user) if (int rc = ensure(h, h->stage_out, (size_t)n * 4, "output staging")) return rc;
    float* const d_out = d_out_user ? d_out_user : (float*)h->stage_out.ptr;
    const bool timing = getenv("SDFGPU_HOST_TIMING") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t1 = now();
    // (out_sdf is scratch from here on: include/sdfgpu.h documents that its contents are undefined when the call fails)
    // (round 6: the uploaded bits ARE the build's input -- no byte mask is spread out on the device and packed again by K0)
    if (packed) { if (int rc0 = upload_packed(h, occ, n, kBitsOnly, kNullStream)) return rc0; }
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

// ---- connected components (sdfgpu_components.hpp) ------------------------------------------------------------------------------
// Uses only cc_scratch (and, in the host forms, the bit / output staging and the pinned chunks, which every host-buffer call
// owns while it runs): the SDF builds' scratch, status block and policy are not touched.
int check_components_dims(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "grid dimensions must be positive (got %lld x %lld x %lld)",
                    (long long)nx, (long long)ny, (long long)nz);
    if ((unsigned __int128)nx * (unsigned __int128)ny * (unsigned __int128)nz > (unsigned __int128)0xFFFFFFFFu)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "grid %lld x %lld x %lld has more than 2^32 - 1 voxels: uint32 component labels cannot number it",
                    (long long)nx, (long long)ny, (long long)nz);
    return SDFGPU_OK;
}

// bits (device) -> labels (device), K -> *out_count; synchronises `st` (K is read back)
int components_impl(sdfgpu_handle h, const uint32_t* d_bits, int64_t nx, int64_t ny, int64_t nz, uint32_t* d_labels, uint32_t* out_count,
                    hipStream_t st) {
    const CcPlan plan = cc_plan(nx, ny, nz);
    if (int rc = ensure(h, h->cc_scratch, plan.scratch_bytes, "components scratch")) return rc;
    HIP_TRY(h, cc_launch(plan, d_bits, d_labels, h->cc_scratch.ptr, st));
    uint32_t k = 0;
    HIP_TRY(h, hipMemcpyAsync(&k, cc_count_word(plan, h->cc_scratch.ptr), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (out_count) *out_count = k;
    return SDFGPU_OK;
}

// host mask / cell records -> bits (host team, 1 bit per voxel over PCIe) -> labels in the output staging
int components_host(sdfgpu_handle h, const Occupancy& occ, int64_t nx, int64_t ny, int64_t nz, uint32_t* out_count) {
    const int64_t n = nx * ny * nz;
    if (int rc = upload_packed(h, occ, n, kBitsOnly, kNullStream)) return rc;
    if (int rc = ensure(h, h->stage_out, (size_t)n * 4, "output staging")) return rc;
    return components_impl(h, (const uint32_t*)h->stage_bits.ptr, nx, ny, nz, (uint32_t*)h->stage_out.ptr, out_count, nullptr);
}

// ---- component topology (sdfgpu_topology.hpp) ----------------------------------------------------------------------------------
// Like the components: only tp_scratch and tp_nodes (and, in the host forms, the label / bit staging and the pinned chunks) are
// used; the SDF builds' scratch, status block and policy are not touched.
int check_topology_args(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, const int64_t* out_counts) {
    if (!out_counts) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = check_components_dims(h, nx, ny, nz)) return rc;
    if (max_label == 0xFFFFFFFFu) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "max_label must be below 2^32 - 1");
    return SDFGPU_OK;
}

// labels (device) + selection bits (device or null) -> (max_label + 1) x 5 counters (host); synchronises `st`
int topology_impl(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label,
                  int64_t* out_counts, hipStream_t st) {
    const TpPlan plan = tp_plan(nx, ny, nz, max_label, d_select != nullptr);
    if (int rc = ensure(h, h->tp_scratch, plan.scratch_bytes, "topology scratch")) return rc;
    HIP_TRY(h, tp_launch_count(plan, d_labels, d_select, h->tp_scratch.ptr, st));
    TpStatus status;
    HIP_TRY(h, hipMemcpyAsync(&status, static_cast<char*>(h->tp_scratch.ptr) + plan.off_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (status.err & kTpErrLabel)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "label %u exceeds max_label %u", status.label_over, max_label);
    if (status.err & kTpErrMixed)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT,
                    "label %u has both selected and unselected voxels: its surface is undefined under this selection "
                    "(labels must come from the connected components of the same occupancy)", status.label_mixed);
    if (status.nodes > 0xFFFFFFFFull)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT,
                    "%llu surface-vertex nodes: more than the 2^32 - 1 that the union-find's 32-bit node ids can number",
                    (unsigned long long)status.nodes);
    if (int rc = ensure(h, h->tp_nodes, (size_t)std::max<uint64_t>(status.nodes, 1) * 4, "topology nodes")) return rc;
    HIP_TRY(h, tp_launch_surfaces(plan, d_labels, h->tp_scratch.ptr, (uint32_t*)h->tp_nodes.ptr, status.nodes, st));
    // (uint64 counters, read as int64: every count is below 2^32)
    return copy_to_host(h, out_counts, h->tp_scratch.ptr, ((size_t)max_label + 1) * kTpCounters * 8, st);
}

// Bit (v & 7) of byte (v >> 3) = voxel v's occupancy class is in class_mask: FILLED (1) occupancy > 0.5f, EMPTY (2) < 0.5f,
// UNKNOWN (4) the rest (0.5 and NaN), as the reference's tagged is_surface_index_fn branches (tagged_object_collision_map.cpp:448-481).
void pack_cells_class_bits(const char* cells, size_t stride, size_t off, int class_mask, int64_t n, size_t ob, size_t len, uint8_t* out) {
    int64_t v = (int64_t)ob * 8;
    for (size_t o = 0; o < len; ++o) {
        uint32_t b = 0;
        for (int k = 0; k < 8; ++k, ++v) {
            if (v >= n) continue;
            float occ;
            memcpy(&occ, cells + (size_t)v * stride + off, 4);
            const int cls = occ > 0.5f ? 1 : occ < 0.5f ? 2 : 4;
            if (cls & class_mask) b |= 1u << k;
        }
        out[o] = (uint8_t)b;
    }
}

// host labels / cell records -> stage_out (labels) and, unless every voxel is selected, stage_bits (selection); *out_selected
// says which
int stage_labels_selection(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select, const void* cells, size_t stride, size_t occ_off,
                           size_t comp_off, int class_mask, int64_t n, bool* out_selected) {
    if (int rc = ensure(h, h->stage_out, (size_t)n * 4, "output staging")) return rc;
    if (labels) {
        if (int rc = copy_from_host(h, h->stage_out.ptr, labels, (size_t)n * 4)) return rc;
    } else {
        const char* const rec = static_cast<const char*>(cells) + comp_off;
        if (int rc = staged_upload_hip(h, h->stage_out.ptr, (size_t)n * 4, nullptr, 32, [=](char* dst, size_t o, size_t len) {
                const char* src = rec + (o / 4) * stride;
                for (size_t q = 0; q < len; q += 4, src += stride) memcpy(dst + q, src, 4);
            }))
            return rc;
    }
    const bool selected = labels ? select != nullptr : (class_mask & 7) != 7;
    if (selected) {
        if (labels || class_mask == 1) {                       // a byte mask, or FILLED: the build's packers (occupancy > 0.5f)
            const Occupancy occ = labels ? Occupancy::of_mask(select) : Occupancy::of_cells(cells, stride, occ_off, 0);
            if (int rc = upload_packed(h, occ, n, kBitsOnly, kNullStream)) return rc;
        } else {
            const size_t nbytes = ((size_t)n + 7) / 8, padded = (nbytes + 3) & ~(size_t)3;
            if (int rc = ensure(h, h->stage_bits, padded, "bit staging")) return rc;
            if (int rc = staged_upload_hip(h, h->stage_bits.ptr, padded, nullptr, 32, [=](char* dst, size_t o, size_t len) {
                    const size_t real = o >= nbytes ? 0 : std::min(len, nbytes - o);
                    if (real) pack_cells_class_bits(static_cast<const char*>(cells), stride, occ_off, class_mask, n, o, real, reinterpret_cast<uint8_t*>(dst));
                    if (real < len) memset(dst + real, 0, len - real);
                }))
                return rc;
        }
    }
    *out_selected = selected;
    return SDFGPU_OK;
}

// host labels / cell records -> counters
int topology_host(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select, const void* cells, size_t stride, size_t occ_off,
                  size_t comp_off, int class_mask, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, int64_t* out_counts) {
    bool selected = false;
    if (int rc = stage_labels_selection(h, labels, select, cells, stride, occ_off, comp_off, class_mask, nx * ny * nz, &selected)) return rc;
    return topology_impl(h, (const uint32_t*)h->stage_out.ptr, selected ? (const uint32_t*)h->stage_bits.ptr : nullptr, nx, ny, nz,
                         max_label, out_counts, nullptr);
}

// ---- component surfaces (sdfgpu_surfaces.hpp) -----------------------------------------------------------------------------------
// Like the topology: only sf_scratch, sf_sort and sf_indices (and, in the host forms, the label / bit staging and the pinned
// chunks) are used; the SDF builds' scratch, status block and policy are not touched.
int check_surfaces_args(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, const int64_t* out_counts, bool want_indices,
                        int64_t capacity, const int64_t* out_total) {
    if (!out_counts || !out_total) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = check_components_dims(h, nx, ny, nz)) return rc;
    if (max_label == 0xFFFFFFFFu) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "max_label must be below 2^32 - 1");
    if (want_indices && capacity < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "capacity must not be negative (got %lld)", (long long)capacity);
    return SDFGPU_OK;
}

// labels (device) + selection bits (device or null) -> counts (host) and, when asked, the grouped indices: into d_indices
// (device) or, through sf_indices, into host_indices.  Synchronises `st`.
int surfaces_impl(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label,
                  int64_t* out_counts, uint32_t* d_indices, uint32_t* host_indices, int64_t capacity, int64_t* out_total,
                  uint32_t* d_surface_bits, hipStream_t st) {
    const SfPlan plan = sf_plan(nx, ny, nz, max_label);
    if (int rc = ensure(h, h->sf_scratch, plan.scratch_bytes, "surfaces scratch")) return rc;
    HIP_TRY(h, sf_launch_flag(plan, d_labels, d_select, d_surface_bits, h->sf_scratch.ptr, st));
    SfStatus status;
    HIP_TRY(h, hipMemcpyAsync(&status, static_cast<char*>(h->sf_scratch.ptr) + plan.off_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (status.err & kSfErrLabel)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "label %u exceeds max_label %u", status.label_over, max_label);
    *out_total = (int64_t)status.total;
    {                                                           // (uint32 counters, widened: every count is below 2^32)
        std::vector<uint32_t> c32((size_t)max_label + 1);
        if (int rc = copy_to_host(h, c32.data(), h->sf_scratch.ptr, c32.size() * 4, st)) return rc;
        for (size_t c = 0; c < c32.size(); ++c) out_counts[c] = (int64_t)c32[c];
    }
    if (!d_indices && !host_indices) return SDFGPU_OK;          // counts only
    if ((uint64_t)capacity < status.total)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "the index buffer holds %lld indices, the surfaces have %llu (counts and total are valid)",
                    (long long)capacity, (unsigned long long)status.total);
    if (status.total == 0) return SDFGPU_OK;
    if (host_indices) {
        if (int rc = ensure(h, h->sf_indices, (size_t)status.total * 4, "surfaces indices")) return rc;
        d_indices = (uint32_t*)h->sf_indices.ptr;
    }
    const SfSortPlan sp = sf_sort_plan(plan, status.total);
    if (int rc = ensure(h, h->sf_sort, sp.bytes, "surfaces sort scratch")) return rc;
    HIP_TRY(h, sf_launch_sort(plan, sp, d_labels, h->sf_scratch.ptr, h->sf_sort.ptr, d_indices, st));
    if (host_indices) return copy_to_host(h, host_indices, d_indices, (size_t)status.total * 4, st);
    HIP_TRY(h, hipStreamSynchronize(st));
    return SDFGPU_OK;
}

int surfaces_host(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select, const void* cells, size_t stride, size_t occ_off,
                  size_t comp_off, int class_mask, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, int64_t* out_counts,
                  uint32_t* out_indices, int64_t capacity, int64_t* out_total) {
    bool selected = false;
    if (int rc = stage_labels_selection(h, labels, select, cells, stride, occ_off, comp_off, class_mask, nx * ny * nz, &selected)) return rc;
    return surfaces_impl(h, (const uint32_t*)h->stage_out.ptr, selected ? (const uint32_t*)h->stage_bits.ptr : nullptr, nx, ny, nz,
                         max_label, out_counts, nullptr, out_indices, capacity, out_total, nullptr, nullptr);
}

// ---- display export (sdfgpu_display.hpp) --------------------------------------------------------------------------------------------
// Only dp_scratch, dp_sort and dp_out (and, in the host forms, the cell / field staging and the pinned chunks) are used.
int check_display_dims(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "grid dimensions must be positive (got %lld x %lld x %lld)",
                    (long long)nx, (long long)ny, (long long)nz);
    if ((unsigned __int128)nx * (unsigned __int128)ny * (unsigned __int128)nz > (unsigned __int128)0xFFFFFFFFu)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "grid %lld x %lld x %lld has more than 2^32 - 1 voxels: the display export's uint32 indices cannot number it",
                    (long long)nx, (long long)ny, (long long)nz);
    return SDFGPU_OK;
}

struct DisplayRequest {
    int rule = kDpRuleOccupancy;
    const uint32_t* draw_keys = nullptr;       // host, ascending; nullptr = no list
    int64_t n_draw_keys = 0;
    bool grouped = false;
    bool to_host = false;                      // the four result pointers are host memory (filled through dp_out)
    uint32_t* indices = nullptr;               // nullptr = the total only
    uint32_t* keys = nullptr;
    int64_t capacity = 0;
    uint32_t* group_keys = nullptr;
    uint32_t* group_offsets = nullptr;
    int64_t group_capacity = 0;
    int64_t* out_total = nullptr;
    int64_t* out_groups = nullptr;
};

int check_display_request(sdfgpu_handle h, const DisplayRequest& rq) {
    if (!rq.out_total) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
    if (rq.n_draw_keys < 0 || rq.n_draw_keys > (int64_t)0xFFFFFFFFll || (rq.n_draw_keys > 0 && !rq.draw_keys))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: n_draw_keys must be in [0, 2^32) and come with a list (got %lld)", (long long)rq.n_draw_keys);
    for (int64_t i = 1; rq.draw_keys && i < rq.n_draw_keys; ++i)
        if (rq.draw_keys[i] < rq.draw_keys[i - 1])
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: draw_keys must be ascending (entry %lld is %u after %u)", (long long)i,
                        rq.draw_keys[i], rq.draw_keys[i - 1]);
    if (rq.indices && rq.capacity < 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: capacity must not be negative (got %lld)", (long long)rq.capacity);
    if (rq.grouped && (!rq.indices || !rq.group_keys || !rq.group_offsets || !rq.out_groups || rq.group_capacity < 0))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: the grouped form needs indices, group_keys, group_offsets, out_groups and a group capacity >= 0");
    if (!rq.to_host && ((reinterpret_cast<uintptr_t>(rq.indices) | reinterpret_cast<uintptr_t>(rq.keys) | reinterpret_cast<uintptr_t>(rq.group_keys) |
                         reinterpret_cast<uintptr_t>(rq.group_offsets)) & 3))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: device pointers must be 4-byte aligned");
    return SDFGPU_OK;
}

size_t dp_align8(size_t x) { return (x + 7) & ~(size_t)7; }
int dp_bit_length(uint32_t x) { int b = 0; while (b < 32 && (x >> b) != 0) ++b; return b; }

// sel: the source, the rule's options and the shape (device records).  Synchronises `st`.
int display_select_impl(sdfgpu_handle h, DpSelect sel, const DisplayRequest& rq, hipStream_t st) {
    const uint64_t n = sel.n, tiles = dp_tiles(n);
    const size_t key_bytes = dp_align8((size_t)rq.n_draw_keys * 4);
    const size_t off_keys = sizeof(DpStatus), off_bits = off_keys + key_bytes, off_counts = off_bits + (size_t)tiles * (kDpTile / 8),
                 off_sums = off_counts + dp_align8((size_t)tiles * 4),
                 bytes = off_sums + dp_align8((size_t)((tiles + kDpScanSeg - 1) / kDpScanSeg) * 4);
    if (int rc = ensure(h, h->dp_scratch, bytes, "display scratch")) return rc;
    char* const b = static_cast<char*>(h->dp_scratch.ptr);
    DpStatus* const d_st = reinterpret_cast<DpStatus*>(b);
    uint32_t* const bits = reinterpret_cast<uint32_t*>(b + off_bits);
    uint32_t* const counts = reinterpret_cast<uint32_t*>(b + off_counts);
    uint32_t* const sums = reinterpret_cast<uint32_t*>(b + off_sums);
    HIP_TRY(h, hipMemsetAsync(d_st, 0, sizeof(DpStatus), st));
    if (rq.n_draw_keys) HIP_TRY(h, hipMemcpyAsync(b + off_keys, rq.draw_keys, (size_t)rq.n_draw_keys * 4, hipMemcpyHostToDevice, st));
    sel.draw_keys = reinterpret_cast<const uint32_t*>(b + off_keys);
    sel.n_draw = (uint32_t)rq.n_draw_keys;
    sel.filter = rq.draw_keys != nullptr;
    sel.bits = bits;
    sel.tile_counts = counts;
    sel.total = &d_st->total;
    sel.key_max = &d_st->key_max;
    HIP_TRY(h, dp_launch_select(rq.rule, sel, st));
    DpStatus status;
    HIP_TRY(h, hipMemcpyAsync(&status, d_st, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t total = status.total;
    *rq.out_total = (int64_t)total;
    if (rq.out_groups) *rq.out_groups = 0;
    if (!rq.indices) return SDFGPU_OK;                          // the total only
    if ((uint64_t)rq.capacity < total)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: the buffers hold %lld elements, %llu voxels are drawn (the total is valid)",
                    (long long)rq.capacity, (unsigned long long)total);
    // where the results are built: the caller's device arrays or dp_out
    const uint64_t gmax = std::min<uint64_t>(total, rq.grouped ? (uint64_t)rq.group_capacity : 0);
    uint32_t *d_idx = rq.indices, *d_keys = rq.keys, *d_gkeys = rq.group_keys, *d_goffs = rq.group_offsets;
    if (rq.to_host) {                                           // indices | keys (only when someone reads them) | group keys | group offsets
        const size_t key_words = rq.keys || rq.grouped ? (size_t)total : 0;
        if (int rc = ensure(h, h->dp_out, ((size_t)total + key_words + (size_t)gmax * 2 + 1) * 4, "display results")) return rc;
        d_idx = static_cast<uint32_t*>(h->dp_out.ptr);
        d_keys = key_words ? d_idx + total : nullptr;
        d_gkeys = d_idx + total + key_words;
        d_goffs = d_gkeys + gmax;
    }
    // sort only the bits in which the drawn keys differ: all of them agree above bit_length(max ^ min)
    const int key_bits = rq.grouped && total ? dp_bit_length(status.key_max ^ ~status.key_inv_max) : 0;
    const SfPairSortPlan sp = key_bits ? sf_pair_sort_plan(total, key_bits) : SfPairSortPlan();
    const bool own_keys = rq.grouped && !d_keys;               // the group boundaries are read from the sorted keys
    if (sp.bytes || own_keys) {
        if (int rc = ensure(h, h->dp_sort, sp.bytes + (own_keys ? (size_t)total * 4 : 0), "display sort scratch")) return rc;
        if (own_keys) d_keys = reinterpret_cast<uint32_t*>(static_cast<char*>(h->dp_sort.ptr) + sp.bytes);
    }
    if (total) {
        sf_launch_scan(counts, tiles, sums, st);
        DpCompact c;
        c.src = sel.src;
        c.key_mode = rq.rule == kDpRuleOccupancy ? kDpKeyClass : rq.rule == kDpRuleKeyField ? kDpKeyWord : kDpKeyZero;
        c.n = n;
        c.bits = bits;
        c.tile_offsets = counts;
        c.capacity = total;
        if (key_bits) c.pairs = static_cast<uint2*>(h->dp_sort.ptr);
        else { c.idx = d_idx; c.keys = d_keys; }
        HIP_TRY(h, dp_launch_compact(c, st));
        if (key_bits) HIP_TRY(h, sf_launch_sort_pairs(sp, key_bits, h->dp_sort.ptr, d_idx, d_keys, st));
    }
    uint64_t groups = 0;
    if (rq.grouped) {
        if (total) {                                            // the same three steps over the sorted keys (their tiles fit the main pass's scratch)
            DpSelect g;
            g.src.cells = reinterpret_cast<const char*>(d_keys);
            g.src.stride = 4;
            g.src.occ_off = 0;                                  // (not read by this rule)
            g.src.key_off = 0;                                  // the key IS the record: k_dp_compact reads it at offset 0
            g.n = total;
            g.bits = bits;
            g.tile_counts = counts;
            g.total = &d_st->groups;
            HIP_TRY(h, dp_launch_select(kDpRuleGroupStart, g, st));
            HIP_TRY(h, hipMemcpyAsync(&status, d_st, sizeof status, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            groups = status.groups;
            *rq.out_groups = (int64_t)groups;
            if ((uint64_t)rq.group_capacity < groups)
                return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: the group arrays hold %lld groups, the drawn voxels have %llu keys (total and groups are valid)",
                            (long long)rq.group_capacity, (unsigned long long)groups);
            sf_launch_scan(counts, dp_tiles(total), sums, st);
            // the same kernel with other meanings: its "voxels" are the positions in the sorted key array (records of one word,
            // stride 4, key at offset 0), so c.idx receives the positions of the group starts = the group offsets, and c.keys
            // load_word(sorted keys, position) = the group keys
            DpCompact c;
            c.src = g.src;
            c.key_mode = kDpKeyWord;
            c.n = total;
            c.bits = bits;
            c.tile_offsets = counts;
            c.capacity = groups;
            c.idx = d_goffs;
            c.keys = d_gkeys;
            HIP_TRY(h, dp_launch_compact(c, st));
        }
        HIP_TRY(h, hipMemcpyAsync(d_goffs + groups, &d_st->total, 4, hipMemcpyDeviceToDevice, st));      // group_offsets[groups] = total
    }
    HIP_TRY(h, hipGetLastError());
    if (rq.to_host) {
        if (int rc = copy_to_host(h, rq.indices, d_idx, (size_t)total * 4, st)) return rc;
        if (rq.keys) if (int rc = copy_to_host(h, rq.keys, d_keys, (size_t)total * 4, st)) return rc;
        if (rq.grouped) {
            if (int rc = copy_to_host(h, rq.group_keys, d_gkeys, (size_t)groups * 4, st)) return rc;
            if (int rc = copy_to_host(h, rq.group_offsets, d_goffs, ((size_t)groups + 1) * 4, st)) return rc;
        }
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    return SDFGPU_OK;
}

int check_display_cells(sdfgpu_handle h, const void* cells, size_t stride, size_t occ_off, size_t key_off, int64_t nx, int64_t ny, int64_t nz,
                        int rule, int class_mask, DpSelect& sel) {
    if (!cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
    if (rule != SDFGPU_DISPLAY_OCCUPANCY && rule != SDFGPU_DISPLAY_KEY_FIELD)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: rule must be SDFGPU_DISPLAY_OCCUPANCY (0) or SDFGPU_DISPLAY_KEY_FIELD (1), got %d", rule);
    if (int rc = check_cell_layout(h, stride, occ_off)) return rc;
    if (rule == SDFGPU_DISPLAY_KEY_FIELD && ((key_off % 4) || key_off + 4 > stride))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: key_offset must be 4-byte aligned and inside the record");
    if (class_mask < 0 || class_mask > 7)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: class_mask must be a combination of FILLED (1), EMPTY (2) and UNKNOWN (4)");
    if (int rc = check_display_dims(h, nx, ny, nz)) return rc;
    sel.src.stride = stride;
    sel.src.occ_off = (uint32_t)occ_off;
    sel.src.key_off = (uint32_t)key_off;
    sel.class_mask = (uint32_t)class_mask;
    sel.nx = (uint32_t)nx; sel.ny = (uint32_t)ny; sel.nz = (uint32_t)nz;
    sel.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    return SDFGPU_OK;
}

int check_display_sdf(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, DpSelect& sel) {
    if (!sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
    if (int rc = check_display_dims(h, nx, ny, nz)) return rc;
    sel.src.stride = 4;
    sel.nx = (uint32_t)nx; sel.ny = (uint32_t)ny; sel.nz = (uint32_t)nz;
    sel.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    return SDFGPU_OK;
}

// a = min(max(alpha, 0), 1); the extrema into dp_scratch's status words, then one rgba per voxel.  Synchronises `st` (the status
// words are scratch of the handle).
int display_sdf_colors_impl(sdfgpu_handle h, const float* d_sdf, uint64_t n, float alpha, float* d_colors, hipStream_t st) {
    if (int rc = ensure(h, h->dp_scratch, sizeof(DpStatus), "display scratch")) return rc;
    DpStatus* const d_st = static_cast<DpStatus*>(h->dp_scratch.ptr);
    HIP_TRY(h, hipMemsetAsync(d_st, 0, sizeof(DpStatus), st));
    HIP_TRY(h, dp_launch_minmax(d_sdf, n, d_st, st));
    HIP_TRY(h, dp_launch_sdf_colors(d_sdf, n, std::min(std::max(alpha, 0.0f), 1.0f), d_st, d_colors, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return SDFGPU_OK;
}

// ---- resample (sdfgpu_resample.hpp) ------------------------------------------------------------------------------------------------
// Only rs_scratch (and, in the host form, the cell and field staging and the pinned chunks) is used.
int check_resample_args(sdfgpu_handle h, const void* src, size_t cell_bytes, int64_t nx, int64_t ny, int64_t nz, const double* src_cell,
                        const double* origin, const double* dst_inverse_origin, const double* dst_inv_cell, const void* dst, int64_t mx,
                        int64_t my, int64_t mz, const void* fill_cell, ResampleArgs& a) {
    if (!src || !dst || !src_cell || !origin || !dst_inverse_origin || !dst_inv_cell || !fill_cell)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: null pointer");
    if (cell_bytes != 4 && cell_bytes != 8 && cell_bytes != 16)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: cell_bytes must be 4, 8 or 16 (got %zu)", cell_bytes);
    if (src == dst) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: the source and the result must be different buffers");
    const int64_t kMaxCells = INT64_MAX / 16;
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx > kMaxCells / ny || nx * ny > kMaxCells / nz)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: unsupported source grid %lld x %lld x %lld", (long long)nx, (long long)ny, (long long)nz);
    if (mx <= 0 || my <= 0 || mz <= 0 || mx > kMaxCells / my || mx * my > kMaxCells / mz)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: unsupported result grid %lld x %lld x %lld", (long long)mx, (long long)my, (long long)mz);
    a = ResampleArgs{};
    a.nx = nx; a.ny = ny; a.nz = nz; a.mx = mx; a.my = my; a.mz = mz;
    a.n_src = nx * ny * nz; a.n_dst = mx * my * mz;
    for (int i = 0; i < 3; ++i) { a.cell[i] = src_cell[i]; a.inv_cell[i] = dst_inv_cell[i]; }
    for (int i = 0; i < 16; ++i) { a.origin[i] = origin[i]; a.inverse[i] = dst_inverse_origin[i]; }
    memcpy(a.fill, fill_cell, cell_bytes);
    a.cell_bytes = (int)cell_bytes;
    a.winner_bytes = resample_winner_bytes(a.n_src);
    a.plain_atomics = h->opt.rs_plain_atomics;
    return SDFGPU_OK;
}

// a.src -> a.dst (device) on `st`; synchronises `st` only when out_written is asked for
int resample_impl(sdfgpu_handle h, ResampleArgs& a, uint64_t* out_written, hipStream_t st) {
    // the winner words belong to the handle and the call may return with its kernels pending: a call on another stream waits for
    // them on the device first, as the local extrema do (ensure() below may free the scratch: hipFree waits for the device)
    HIP_TRY(h, h->rs_order.create());
    HIP_TRY(h, h->rs_order.wait(st));
    if (int rc = ensure(h, h->rs_scratch, resample_scratch_bytes(a.n_dst, a.winner_bytes), "resample winners")) return rc;
    a.winner = h->rs_scratch.ptr;
    unsigned long long* const counter =
        reinterpret_cast<unsigned long long*>(static_cast<char*>(h->rs_scratch.ptr) + resample_counter_offset(a.n_dst, a.winner_bytes));
    a.written = out_written ? counter : nullptr;
    if (h->opt.rs_timing) {
        for (hipEvent_t& e : h->rs_time_ev) if (!e) HIP_TRY(h, hipEventCreate(&e));
        HIP_TRY(h, hipEventRecord(h->rs_time_ev[0], st));
    }
    const hipError_t le = resample_launch(a, st, h->opt.rs_timing ? h->rs_time_ev[1] : nullptr);
    if (h->opt.rs_timing) h->rs_timed = le == hipSuccess && hipEventRecord(h->rs_time_ev[2], st) == hipSuccess;
    (void)h->rs_order.record(st);                       // (also behind a failed launch: what it did enqueue is ordered)
    HIP_TRY(h, le);
    if (out_written) {
        unsigned long long count = 0;
        HIP_TRY(h, hipMemcpyAsync(&count, counter, sizeof count, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        *out_written = (uint64_t)count;
    }
    return SDFGPU_OK;
}

// ---- local extrema and convex segments (sdfgpu_convex.hpp) ---------------------------------------------------------------------
// The extrema and segment stages use only cx_scratch and cx_field (and, in the host forms, the staging buffers and the pinned
// chunks); the SDF scratch, status block and policy are left as they were.  sdfgpu_convex_segments_cells builds its SDF with the
// ordinary tagged build.
int check_convex_args(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz, double resolution, const double* q_and_qinv) {
    if (!q_and_qinv) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "grid dimensions must be positive (got %lld x %lld x %lld)",
                    (long long)nx, (long long)ny, (long long)nz);
    // Indices, kCxOff and the doubling markers share one uint32 space (sdfgpu_convex.hip): the markers are 2^32 - 1 (= kCxOff),
    // 2^32 - 2 and 2^32 - 3, so every index must stay below 2^32 - 3 and n may be at most 2^32 - 3.
    if ((unsigned __int128)nx * (unsigned __int128)ny * (unsigned __int128)nz >= (unsigned __int128)0xFFFFFFFEu)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT,
                    "grid %lld x %lld x %lld has 2^32 - 2 voxels or more: uint32 indices share their space with the OFF sentinel and "
                    "the doubling markers 2^32 - 1, 2^32 - 2, 2^32 - 3, so at most 2^32 - 3 voxels can be numbered",
                    (long long)nx, (long long)ny, (long long)nz);
    if (!(resolution > 0.0) || !std::isfinite(resolution))
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resolution must be positive and finite (got %g)", resolution);
    return SDFGPU_OK;
}

// d_sdf (device) -> d_ext (device); synchronises `st` once per doubling round
int extrema_impl(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution, const double* q_and_qinv,
                 uint32_t* d_ext, hipStream_t st) {
    const CxPlan plan = cx_plan(nx, ny, nz);
    // cx_extrema returns with its basin / entry / final kernels still pending on `st`, and they read and write cx_scratch: a
    // computation on another stream is ordered behind them, as the builds are ordered by build_order.  (ensure() below may
    // free the scratch: hipFree waits for the device.)
    HIP_TRY(h, h->cx_order.create());
    HIP_TRY(h, h->cx_order.wait(st));
    if (int rc = ensure(h, h->cx_scratch, plan.scratch_bytes, "convex scratch")) return rc;
    CxRot rot;
    for (int i = 0; i < 4; ++i) { rot.q[i] = q_and_qinv[i]; rot.qi[i] = q_and_qinv[4 + i]; }
    int rounds = 0;
    h->cx_stats_off = 0;
    const hipError_t ce = cx_extrema(plan, d_sdf, resolution, rot, d_ext, h->cx_scratch.ptr, st, &rounds);
    (void)h->cx_order.record(st);                       // (also behind a failed launch: what it did enqueue is ordered)
    HIP_TRY(h, ce);
    h->cx_stats_off = plan.off_stats;
    h->cx_rounds = rounds;
    return SDFGPU_OK;
}

// records in stage_in -> SDF in stage_out (float), the virtual-border or the free-and-named-objects form
int convex_sdf(sdfgpu_handle h, size_t stride, size_t occ_off, size_t obj_off, int64_t nx, int64_t ny, int64_t nz, double resolution,
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

}  // namespace

extern "C" {

const char* sdfgpu_version(void) { return "sdfgpu 0.1 (gfx950, HIP)"; }

int sdfgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sdfgpu_create(int device, sdfgpu_handle* out_handle) {
    if (!out_handle) return fail(nullptr, SDFGPU_ERR_INVALID_ARGUMENT, "out_handle is null");
    *out_handle = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, SDFGPU_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n)
        return fail(nullptr, SDFGPU_ERR_NO_DEVICE, "device index %d out of range (0..%d)", device, n - 1);
    HIP_TRY(nullptr, hipSetDevice(device));
    sdfgpu_context* ctx = new (std::nothrow) sdfgpu_context();
    if (!ctx) return fail(nullptr, SDFGPU_ERR_INVALID_ARGUMENT, "out of host memory");
    ctx->device = device;
    {
        const char* rz = getenv("SDFGPU_REDZONE");
        ctx->redzone = rz && rz[0] && rz[0] != '0';
    }
    hipError_t ce = rz_malloc(ctx, "extrema slots", (size_t)kSlots * kSlotWords * 4, (void**)&ctx->d_slots) == SDFGPU_OK ? hipSuccess : hipErrorOutOfMemory;
    if (ce == hipSuccess) ce = hipMemset(ctx->d_slots, 0, (size_t)kSlots * kSlotWords * 4);
    if (ce == hipSuccess) ce = rz_malloc(ctx, "status block", 512, (void**)&ctx->d_small) == SDFGPU_OK ? hipSuccess : hipErrorOutOfMemory;
    if (ce == hipSuccess) ce = hipMemset(ctx->d_small, 0, 512);
    if (ce != hipSuccess) {
        if (ctx->d_slots) (void)rz_free(ctx, ctx->d_slots);
        if (ctx->d_small) (void)rz_free(ctx, ctx->d_small);
        delete ctx;
        return fail(nullptr, SDFGPU_ERR_HIP, "HIP error %d (%s) while allocating the context's status blocks",
                    (int)ce, hipGetErrorString(ce));
    }
    ctx->d_result = ctx->d_small + 64;                       // second half of the same allocation
    if (hipHostMalloc((void**)&ctx->h_flags, 256, hipHostMallocMapped) != hipSuccess) ctx->h_flags = nullptr;
    if (ctx->h_flags && hipHostGetDevicePointer((void**)&ctx->h_flags_dev, ctx->h_flags, 0) != hipSuccess) ctx->h_flags_dev = nullptr;
    if (ctx->h_flags && hipEventCreateWithFlags(&ctx->flags_ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipHostFree(ctx->h_flags);
        ctx->h_flags = nullptr;
    }
    if (ctx->h_flags && ctx->h_flags_dev && hipEventCreateWithFlags(&ctx->far_ev, hipEventDisableTiming) == hipSuccess) {
        memset(ctx->h_flags, 0, 256);
        ctx->h_far = ctx->h_flags + 32;                        // second half of the same pinned allocation
        ctx->h_far_dev = ctx->h_flags_dev + 32;
    } else {
        ctx->far_ev = nullptr;
    }
    *out_handle = ctx;
    return SDFGPU_OK;
}

int sdfgpu_destroy(sdfgpu_handle h) {
    if (!h) return SDFGPU_OK;
    (void)hipSetDevice(h->device);
    for (DeviceBuffer& b : *h) if (b.ptr) (void)rz_free(h, b.ptr);
    if (h->d_small) (void)rz_free(h, h->d_small);
    if (h->d_slots) (void)rz_free(h, h->d_slots);
    if (h->rz_table) (void)hipFree(h->rz_table);
    if (h->batch_pin) (void)hipHostFree(h->batch_pin);
    if (h->h_flags) { (void)hipHostFree(h->h_flags); (void)hipEventDestroy(h->flags_ev); }
    if (h->far_ev) (void)hipEventDestroy(h->far_ev);
    for (StreamOrder* o : {&h->build_order, &h->cx_order, &h->rs_order}) o->destroy();
    for (hipEvent_t e : h->rs_time_ev) if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) { if (h->pin[i]) (void)hipHostFree(h->pin[i]); if (h->pin_ev[i]) (void)hipEventDestroy(h->pin_ev[i]); }
    for (size_t i = 0; i < h->events.size(); ++i)
        if (i % 8 == 0 || h->events[i] != h->events[i - 1]) (void)hipEventDestroy(h->events[i]);
    for (hipEvent_t e : h->event_pool) (void)hipEventDestroy(e);
    delete h->team;                                             // (joins the parked host threads)
    delete h;
    return SDFGPU_OK;
}

const char* sdfgpu_last_error(sdfgpu_handle h) { return h ? h->error.c_str() : g_create_error.c_str(); }

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
        if (h && !cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cells is null");
        if (h) if (int rc = check_cell_layout(h, cell_stride, occupancy_offset)) return rc;
        return build_host_impl(h, Occupancy::of_cells(cells, cell_stride, occupancy_offset, unknown_is_filled), nx, ny, nz,
                               resolution, add_virtual_border, out_sdf, out_max, out_min);
    });
}

int sdfgpu_build_to_device(sdfgpu_handle h, const uint8_t* filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                           int add_virtual_border, float* d_out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (h && !d_out_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_out_sdf is null");
        float* const no_host_field = nullptr;
        return build_host_impl(h, Occupancy::of_mask(filled), nx, ny, nz, resolution, add_virtual_border, no_host_field, out_max, out_min,
                               d_out_sdf);
    });
}

int sdfgpu_build_cells_to_device(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset,
                                 int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 int add_virtual_border, float* d_out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (h && !cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cells is null");
        if (h && !d_out_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_out_sdf is null");
        if (h) if (int rc = check_cell_layout(h, cell_stride, occupancy_offset)) return rc;
        float* const no_host_field = nullptr;
        return build_host_impl(h, Occupancy::of_cells(cells, cell_stride, occupancy_offset, unknown_is_filled), nx, ny, nz, resolution,
                               add_virtual_border, no_host_field, out_max, out_min, d_out_sdf);
    });
}

int sdfgpu_build_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t nx, int64_t ny, int64_t nz,
                        double resolution, int add_virtual_border, float* d_out_sdf, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (h && !d_filled) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_filled is null");
        return build_device_impl(h, Occupancy::of_mask(d_filled), nx, ny, nz, resolution, add_virtual_border, d_out_sdf, (hipStream_t)stream);
    });
}

int sdfgpu_build_cells_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset,
                              int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              int add_virtual_border, float* d_out_sdf, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (h && !d_cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_cells is null");
        return build_device_impl(h, Occupancy::of_cells(d_cells, cell_stride, occupancy_offset, unknown_is_filled), nx, ny, nz,
                                 resolution, add_virtual_border, d_out_sdf, (hipStream_t)stream);
    });
}

int sdfgpu_build_bits_device(sdfgpu_handle h, const uint32_t* d_bits, int64_t nx, int64_t ny, int64_t nz,
                             double resolution, int add_virtual_border, float* d_out_sdf, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (h && !d_bits) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_bits is null");
        return build_device_impl(h, Occupancy::of_bits(d_bits), nx, ny, nz, resolution, add_virtual_border, d_out_sdf, (hipStream_t)stream);
    });
}

int sdfgpu_build_bits(sdfgpu_handle h, const uint32_t* bits, int64_t nx, int64_t ny, int64_t nz, double resolution,
                      int add_virtual_border, float* out_sdf, double* out_max, double* out_min) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (h && !bits) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "bits is null");
        return build_host_impl(h, Occupancy::of_bits(bits), nx, ny, nz, resolution, add_virtual_border, out_sdf, out_max, out_min);
    });
}

int sdfgpu_copy_to_host(sdfgpu_handle h, void* dst, const void* d_src, size_t bytes, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (bytes > 0 && (!dst || !d_src)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        HIP_TRY(h, hipSetDevice(h->device));
        return copy_to_host(h, dst, d_src, bytes, (hipStream_t)stream);
    });
}

int sdfgpu_copy_from_host(sdfgpu_handle h, void* d_dst, const void* src, size_t bytes, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (bytes > 0 && (!d_dst || !src)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        HIP_TRY(h, hipSetDevice(h->device));
        return copy_from_host(h, d_dst, src, bytes, (hipStream_t)stream);
    });
}

int sdfgpu_upload_classified(sdfgpu_handle h, const uint8_t* filled, const void* cells, size_t cell_stride, size_t occupancy_offset,
                             int unknown_is_filled, int64_t n, uint8_t* d_mask, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if ((!filled && !cells) || !d_mask) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (n <= 0) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "voxel count must be positive");
        if (cells) if (int rc = check_cell_layout(h, cell_stride, occupancy_offset)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const Occupancy occ = cells ? Occupancy::of_cells(cells, cell_stride, occupancy_offset, unknown_is_filled) : Occupancy::of_mask(filled);
        return upload_packed(h, occ, n, d_mask, (hipStream_t)stream);
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

int sdfgpu_get_extrema(sdfgpu_handle h, double* out_max, double* out_min) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!h->last.have_result) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no build has been issued on this handle");
    HIP_TRY(h, hipSetDevice(h->device));
    uint32_t v[4];
    // (the build's own event, not its stream: the stream is the caller's and may be gone by now -- ADVICE r4)
    HIP_TRY(h, h->build_order.host_wait());
    HIP_TRY(h, hipMemcpy(v, h->d_result, sizeof v, hipMemcpyDeviceToHost));
    return sdfgpu_extrema_from_dsq(v[kSwMaxFree], v[kSwMaxFilled], h->last.last_resolution, out_max, out_min);
}

int sdfgpu_sweep_zy_tiered_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t nxs, int64_t ny, int64_t nz,
                                  int32_t* d_plane_dsq, uint32_t* d_far, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (h->opt.force_env < 0) {
            if (int rc = launch_envelope_probe(h, 2, ke2, nxs, ny, nz, unit, no_border, kUnguarded, dy, s)) return rc;
        } else if (int rc = launch_decide(h, dy, s)) return rc;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (h->opt.force_env < 0) {
            if (int rc = launch_envelope_probe(h, 3, ke3, nx, nys, nz, resolution, add_virtual_border, kUnguarded, dx, s)) return rc;
        } else if (int rc = launch_decide(h, dx, s)) return rc;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!filled || !out_sdf) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null host pointer");
        if (int rc = check_batch_args(h, batch, nx, ny, nz, resolution, resolutions)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const size_t total = (size_t)(batch * nx * ny * nz);
        h->tag_cached_bytes = 0;                        // (stage_in is about to be overwritten)
        if (int rc = ensure(h, h->stage_in, total, "input staging")) return rc;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        h->tag_cached_bytes = 0;
        if (int rc = ensure(h, h->stage_in, (size_t)(rows + 2) * plane * 4, "input staging")) return rc;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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

int sdfgpu_device_malloc(sdfgpu_handle h, size_t bytes, void** out_ptr) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!out_ptr) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "out_ptr is null");
    *out_ptr = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    return rz_malloc(h, "sdfgpu_device_malloc", h->redzone ? std::max<size_t>(bytes, 4) : std::max<size_t>(bytes, 256), out_ptr);
}

int sdfgpu_device_free(sdfgpu_handle h, void* ptr) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!ptr) return SDFGPU_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->redzone) if (int rc = redzone_check(h, nullptr)) { (void)rz_free(h, ptr); return rc; }      // (last look at this buffer's zones)
    return rz_free(h, ptr);
}

int sdfgpu_query_points(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                        const double* world_to_grid, const double* grid_to_world_rotation, float oob_value,
                        const double* points, int64_t n_points, int enable_edge_gradients, double* out_distance,
                        double* out_gradient, uint8_t* out_flags) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h || !d_out || n <= 0 || n > (1ll << 24)) return SDFGPU_ERR_INVALID_ARGUMENT;
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

int sdfgpu_redzone_check(sdfgpu_handle h, void* stream) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    return redzone_check(h, (hipStream_t)stream);
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
                    (h->last.last_lines_tiered ? 128 : 0) | ((h->last.last_dc_x & 31) << 8);
    return SDFGPU_OK;
}

int sdfgpu_last_dense_certified(sdfgpu_handle h, int* out_certified) {
    if (!h || !out_certified) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!h->last.have_result) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no build has been issued on this handle");
    HIP_TRY(h, hipSetDevice(h->device));
    uint32_t v[8];
    // (the build's own event, not its stream: the stream is the caller's and may be gone by now -- ADVICE r4)
    HIP_TRY(h, h->build_order.host_wait());
    HIP_TRY(h, hipMemcpy(v, h->d_result, sizeof v, hipMemcpyDeviceToHost));
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

int sdfgpu_components_bits_device(sdfgpu_handle h, const uint32_t* d_bits, int64_t nx, int64_t ny, int64_t nz, uint32_t* d_labels,
                                  uint32_t* out_count, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!d_bits || !d_labels || !out_count) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if ((reinterpret_cast<uintptr_t>(d_bits) | reinterpret_cast<uintptr_t>(d_labels)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_bits and d_labels must be 4-byte aligned");
        if (int rc = check_components_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return components_impl(h, d_bits, nx, ny, nz, d_labels, out_count, (hipStream_t)stream);
    });
}

int sdfgpu_components(sdfgpu_handle h, const uint8_t* filled, int64_t nx, int64_t ny, int64_t nz, uint32_t* out_labels, uint32_t* out_count) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!filled || !out_labels || !out_count) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_components_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = components_host(h, Occupancy::of_mask(filled), nx, ny, nz, out_count)) return rc;
        return copy_to_host(h, out_labels, h->stage_out.ptr, (size_t)(nx * ny * nz) * 4);
    });
}

int sdfgpu_components_cells(sdfgpu_handle h, void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                            int64_t nx, int64_t ny, int64_t nz, uint32_t* out_count) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!cells || !out_count) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_component_layout(h, cell_stride, occupancy_offset, component_offset)) return rc;
        if (int rc = check_components_dims(h, nx, ny, nz)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = components_host(h, Occupancy::of_cells(cells, cell_stride, occupancy_offset, 0), nx, ny, nz, out_count)) return rc;
        char* const rec = static_cast<char*>(cells) + component_offset;
        // the drain team writes each label into its record (download offsets are multiples of 4: whole labels)
        return staged_download_hip(h, h->stage_out.ptr, (size_t)(nx * ny * nz) * 4, nullptr, [=](const char* src, size_t goff, size_t len) {
            char* dst = rec + (goff / 4) * cell_stride;
            for (size_t o = 0; o < len; o += 4, dst += cell_stride) memcpy(dst, src + o, 4);
        });
    });
}

int sdfgpu_component_topology_device(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select_bits, int64_t nx, int64_t ny,
                                     int64_t nz, uint32_t max_label, int64_t* out_counts, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!d_labels) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if ((reinterpret_cast<uintptr_t>(d_labels) | reinterpret_cast<uintptr_t>(d_select_bits)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_labels and d_select_bits must be 4-byte aligned");
        if (int rc = check_topology_args(h, nx, ny, nz, max_label, out_counts)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return topology_impl(h, d_labels, d_select_bits, nx, ny, nz, max_label, out_counts, (hipStream_t)stream);
    });
}

int sdfgpu_component_topology(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select_mask, int64_t nx, int64_t ny, int64_t nz,
                              uint32_t max_label, int64_t* out_counts) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!labels) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_topology_args(h, nx, ny, nz, max_label, out_counts)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return topology_host(h, labels, select_mask, nullptr, 0, 0, 0, 7, nx, ny, nz, max_label, out_counts);
    });
}

int sdfgpu_component_topology_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                                    int64_t nx, int64_t ny, int64_t nz, int class_mask, uint32_t max_label, int64_t* out_counts) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_component_layout(h, cell_stride, occupancy_offset, component_offset)) return rc;
        if (class_mask < 1 || class_mask > 7)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "class_mask must be a nonzero combination of FILLED (1), EMPTY (2) and UNKNOWN (4)");
        if (int rc = check_topology_args(h, nx, ny, nz, max_label, out_counts)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return topology_host(h, nullptr, nullptr, cells, cell_stride, occupancy_offset, component_offset, class_mask, nx, ny, nz, max_label,
                             out_counts);
    });
}

int sdfgpu_component_surfaces_device(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select_bits, int64_t nx, int64_t ny,
                                     int64_t nz, uint32_t max_label, int64_t* out_counts, uint32_t* d_indices, int64_t capacity,
                                     int64_t* out_total, uint32_t* d_surface_bits, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!d_labels) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if ((reinterpret_cast<uintptr_t>(d_labels) | reinterpret_cast<uintptr_t>(d_select_bits) | reinterpret_cast<uintptr_t>(d_indices) |
             reinterpret_cast<uintptr_t>(d_surface_bits)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_labels, d_select_bits, d_indices and d_surface_bits must be 4-byte aligned");
        if (int rc = check_surfaces_args(h, nx, ny, nz, max_label, out_counts, d_indices != nullptr, capacity, out_total)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return surfaces_impl(h, d_labels, d_select_bits, nx, ny, nz, max_label, out_counts, d_indices, nullptr, capacity, out_total,
                             d_surface_bits, (hipStream_t)stream);
    });
}

int sdfgpu_component_surfaces(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select_mask, int64_t nx, int64_t ny, int64_t nz,
                              uint32_t max_label, int64_t* out_counts, uint32_t* out_indices, int64_t capacity, int64_t* out_total) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!labels) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_surfaces_args(h, nx, ny, nz, max_label, out_counts, out_indices != nullptr, capacity, out_total)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return surfaces_host(h, labels, select_mask, nullptr, 0, 0, 0, 7, nx, ny, nz, max_label, out_counts, out_indices, capacity, out_total);
    });
}

int sdfgpu_component_surfaces_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                                    int64_t nx, int64_t ny, int64_t nz, int class_mask, uint32_t max_label, int64_t* out_counts,
                                    uint32_t* out_indices, int64_t capacity, int64_t* out_total) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!cells) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_component_layout(h, cell_stride, occupancy_offset, component_offset)) return rc;
        if (class_mask < 1 || class_mask > 7)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "class_mask must be a nonzero combination of FILLED (1), EMPTY (2) and UNKNOWN (4)");
        if (int rc = check_surfaces_args(h, nx, ny, nz, max_label, out_counts, out_indices != nullptr, capacity, out_total)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return surfaces_host(h, nullptr, nullptr, cells, cell_stride, occupancy_offset, component_offset, class_mask, nx, ny, nz, max_label,
                             out_counts, out_indices, capacity, out_total);
    });
}

int sdfgpu_local_extrema_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                const double q_and_qinv[8], uint32_t* d_extremum, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!d_sdf || !d_extremum) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if ((reinterpret_cast<uintptr_t>(d_sdf) | reinterpret_cast<uintptr_t>(d_extremum)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "d_sdf and d_extremum must be 4-byte aligned");
        if (int rc = check_convex_args(h, nx, ny, nz, resolution, q_and_qinv)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return extrema_impl(h, d_sdf, nx, ny, nz, resolution, q_and_qinv, d_extremum, (hipStream_t)stream);
    });
}

int sdfgpu_local_extrema(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                         const double q_and_qinv[8], uint32_t* out_extremum) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!sdf || !out_extremum) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_convex_args(h, nx, ny, nz, resolution, q_and_qinv)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const size_t n = (size_t)(nx * ny * nz);
        if (int rc = ensure(h, h->cx_field, n * 4, "convex field")) return rc;
        if (int rc = ensure(h, h->stage_out, n * 4, "output staging")) return rc;
        if (int rc = copy_from_host(h, h->cx_field.ptr, sdf, n * 4)) return rc;
        if (int rc = extrema_impl(h, (const float*)h->cx_field.ptr, nx, ny, nz, resolution, q_and_qinv, (uint32_t*)h->stage_out.ptr, nullptr))
            return rc;
        return copy_to_host(h, out_extremum, h->stage_out.ptr, n * 4);
    });
}

int sdfgpu_convex_segments_cells(sdfgpu_handle h, void* cells, size_t cell_stride, size_t occupancy_offset, size_t object_id_offset,
                                 size_t segment_offset, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 const double q_and_qinv[8], double connected_threshold, int add_virtual_border, uint32_t* out_count) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!cells || !out_count) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (cell_stride < 12 || (cell_stride % 4) || (occupancy_offset % 4) || (object_id_offset % 4) || (segment_offset % 4) ||
            occupancy_offset + 4 > cell_stride || object_id_offset + 4 > cell_stride || segment_offset + 4 > cell_stride ||
            occupancy_offset == object_id_offset || segment_offset == occupancy_offset || segment_offset == object_id_offset)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT,
                        "cell_stride / occupancy_offset / object_id_offset / segment_offset must be 4-byte aligned, in range and distinct");
        if (int rc = check_convex_args(h, nx, ny, nz, resolution, q_and_qinv)) return rc;
        if (int rc = check_dims(h, nx, ny, nz)) return rc;                     // (the SDF build's own limits)
        HIP_TRY(h, hipSetDevice(h->device));
        const int64_t n = nx * ny * nz;
        const CxPlan plan = cx_plan(nx, ny, nz);
        h->tag_cached_bytes = 0;
        if (int rc = ensure(h, h->stage_in, (size_t)n * cell_stride, "input staging")) return rc;
        if (int rc = ensure(h, h->stage_out, (size_t)n * 4, "output staging")) return rc;
        if (int rc = ensure(h, h->tagmask, (size_t)n, "tagged-object mask")) return rc;
        if (int rc = ensure(h, h->tagids, 4, "object id list")) return rc;
        if (int rc = ensure(h, h->cx_field, (size_t)n * 4, "convex field")) return rc;
        if (int rc = ensure(h, h->cx_scratch, plan.scratch_bytes, "convex scratch")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, cells, (size_t)n * cell_stride)) return rc;
        if (int rc = convex_sdf(h, cell_stride, occupancy_offset, object_id_offset, nx, ny, nz, resolution, add_virtual_border)) return rc;
        uint32_t* d_ext = (uint32_t*)h->cx_field.ptr;                          // (the named-object SDF is consumed by now)
        if (int rc = extrema_impl(h, (const float*)h->stage_out.ptr, nx, ny, nz, resolution, q_and_qinv, d_ext, nullptr)) return rc;
        uint32_t* d_labels = (uint32_t*)h->stage_out.ptr;                      // (the SDF is consumed by the extrema)
        HIP_TRY(h, cx_segments(plan, d_ext, (const char*)h->stage_in.ptr, cell_stride, occupancy_offset, object_id_offset, resolution,
                               connected_threshold, d_labels, h->cx_scratch.ptr, nullptr));
        uint32_t count = 0;
        HIP_TRY(h, hipMemcpyAsync(&count, static_cast<char*>(h->cx_scratch.ptr) + plan.off_stats + offsetof(CxStats, count), 4,
                                  hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(h, hipStreamSynchronize(nullptr));
        char* const rec = static_cast<char*>(cells) + segment_offset;
        if (int rc = staged_download_hip(h, d_labels, (size_t)n * 4, nullptr, [=](const char* src, size_t goff, size_t len) {
                char* dst = rec + (goff / 4) * cell_stride;
                for (size_t o = 0; o < len; o += 4, dst += cell_stride) memcpy(dst, src + o, 4);
            }))
            return rc;
        *out_count = count;
        return SDFGPU_OK;
    });
}

int sdfgpu_convex_last_info(sdfgpu_handle h, int* out_rounds, uint32_t* out_cycles, uint32_t* out_longest_cycle,
                            uint32_t* out_longest_entry) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (h->cx_stats_off == 0 || !h->cx_scratch.ptr) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no local extrema computed on this handle");
    HIP_TRY(h, hipSetDevice(h->device));
    static thread_local CxStats st;                            // (336 KiB: not on the stack)
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(&st, static_cast<char*>(h->cx_scratch.ptr) + h->cx_stats_off, sizeof st, hipMemcpyDeviceToHost));
    if (out_rounds) *out_rounds = h->cx_rounds;
    if (out_cycles) *out_cycles = cx_row_sum(st.cycles);
    if (out_longest_cycle) *out_longest_cycle = st.longest_cycle[0];
    if (out_longest_entry) *out_longest_entry = st.longest_entry[0];
    return SDFGPU_OK;
}

int sdfgpu_project_step_limit(int64_t nx, int64_t ny, int64_t nz, double stepsize_multiplier, int max_steps, int* out_limit) {
    if (!out_limit || nx <= 0 || ny <= 0 || nz <= 0) return SDFGPU_ERR_INVALID_ARGUMENT;
    const int limit = project_step_limit(nx, ny, nz, stepsize_multiplier, max_steps);
    if (limit < 0) return SDFGPU_ERR_INVALID_ARGUMENT;
    *out_limit = limit;
    return SDFGPU_OK;
}

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

int sdfgpu_project_points_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 const double world_to_grid[12], const double grid_to_world[12], double minimum_distance,
                                 double stepsize_multiplier, int max_steps, int mode, const double* d_points, int64_t n_points,
                                 double* d_out_points, uint8_t* d_out_status, int32_t* d_out_steps, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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

int sdfgpu_query_gradients_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                  const double world_to_grid[12], float oob_value, int kind, double window, const double* d_points,
                                  int64_t n_points, double* d_value, double* d_gradient, uint8_t* d_status, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
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

int sdfgpu_resample_cells_device(sdfgpu_handle h, const void* d_src, size_t cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                                 const double src_cell[3], const double origin[16], const double dst_inverse_origin[16],
                                 const double dst_inv_cell[3], void* d_dst, int64_t mx, int64_t my, int64_t mz, const void* fill_cell,
                                 uint64_t* out_cells_written, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        ResampleArgs a;
        if (int rc = check_resample_args(h, d_src, cell_bytes, nx, ny, nz, src_cell, origin, dst_inverse_origin, dst_inv_cell, d_dst, mx, my,
                                         mz, fill_cell, a)) return rc;
        if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "resample: d_src and d_dst must be 4-byte aligned");
        HIP_TRY(h, hipSetDevice(h->device));
        a.src = d_src; a.dst = d_dst;
        return resample_impl(h, a, out_cells_written, (hipStream_t)stream);
    });
}

int sdfgpu_debug_resample_times(sdfgpu_handle h, double* out_winner_ms, double* out_gather_ms) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    if (!out_winner_ms || !out_gather_ms) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
    if (!h->rs_timed) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "no resample timed on this handle (option \"resample_timing\")");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventSynchronize(h->rs_time_ev[2]));
    float a = 0.0f, b = 0.0f;
    HIP_TRY(h, hipEventElapsedTime(&a, h->rs_time_ev[0], h->rs_time_ev[1]));
    HIP_TRY(h, hipEventElapsedTime(&b, h->rs_time_ev[1], h->rs_time_ev[2]));
    *out_winner_ms = (double)a;
    *out_gather_ms = (double)b;
    return SDFGPU_OK;
}

int sdfgpu_resample_cells(sdfgpu_handle h, const void* src, size_t cell_bytes, int64_t nx, int64_t ny, int64_t nz, const double src_cell[3],
                          const double origin[16], const double dst_inverse_origin[16], const double dst_inv_cell[3], void* dst, int64_t mx,
                          int64_t my, int64_t mz, const void* fill_cell, uint64_t* out_cells_written) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        ResampleArgs a;
        if (int rc = check_resample_args(h, src, cell_bytes, nx, ny, nz, src_cell, origin, dst_inverse_origin, dst_inv_cell, dst, mx, my, mz,
                                         fill_cell, a)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        // the null stream throughout: source records through the cell staging, the result through the field staging
        const size_t src_bytes = (size_t)a.n_src * cell_bytes, dst_bytes = (size_t)a.n_dst * cell_bytes;
        h->tag_cached_bytes = 0;                        // (stage_in is about to be overwritten)
        if (int rc = ensure(h, h->stage_in, src_bytes, "input staging")) return rc;
        if (int rc = ensure(h, h->stage_out, dst_bytes, "output staging")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, src, src_bytes)) return rc;
        a.src = h->stage_in.ptr; a.dst = h->stage_out.ptr;
        if (int rc = resample_impl(h, a, out_cells_written, nullptr)) return rc;
        return copy_to_host(h, dst, h->stage_out.ptr, dst_bytes);
    });
}

int sdfgpu_display_select_cells_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset,
                                       int64_t nx, int64_t ny, int64_t nz, int rule, int class_mask, int surface_only,
                                       const uint32_t* draw_keys, int64_t n_draw_keys, int draw_zero, int grouped, uint32_t* d_indices,
                                       uint32_t* d_keys, int64_t capacity, int64_t* out_total, uint32_t* d_group_keys,
                                       uint32_t* d_group_offsets, int64_t group_capacity, int64_t* out_groups, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        DpSelect sel;
        if (int rc = check_display_cells(h, d_cells, cell_stride, occupancy_offset, key_offset, nx, ny, nz, rule, class_mask, sel)) return rc;
        if (reinterpret_cast<uintptr_t>(d_cells) & 3) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: d_cells must be 4-byte aligned");
        DisplayRequest rq;
        rq.rule = rule == SDFGPU_DISPLAY_OCCUPANCY ? kDpRuleOccupancy : kDpRuleKeyField;
        rq.draw_keys = draw_keys; rq.n_draw_keys = n_draw_keys; rq.grouped = grouped != 0;
        rq.indices = d_indices; rq.keys = d_keys; rq.capacity = capacity; rq.out_total = out_total;
        rq.group_keys = d_group_keys; rq.group_offsets = d_group_offsets; rq.group_capacity = group_capacity; rq.out_groups = out_groups;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        sel.src.cells = static_cast<const char*>(d_cells);
        sel.surface_only = surface_only != 0;
        sel.draw_zero = draw_zero != 0;
        return display_select_impl(h, sel, rq, (hipStream_t)stream);
    });
}

int sdfgpu_display_select_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset, int64_t nx,
                                int64_t ny, int64_t nz, int rule, int class_mask, int surface_only, const uint32_t* draw_keys,
                                int64_t n_draw_keys, int draw_zero, int grouped, uint32_t* out_indices, uint32_t* out_keys, int64_t capacity,
                                int64_t* out_total, uint32_t* out_group_keys, uint32_t* out_group_offsets, int64_t group_capacity,
                                int64_t* out_groups) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        DpSelect sel;
        if (int rc = check_display_cells(h, cells, cell_stride, occupancy_offset, key_offset, nx, ny, nz, rule, class_mask, sel)) return rc;
        DisplayRequest rq;
        rq.rule = rule == SDFGPU_DISPLAY_OCCUPANCY ? kDpRuleOccupancy : kDpRuleKeyField;
        rq.draw_keys = draw_keys; rq.n_draw_keys = n_draw_keys; rq.grouped = grouped != 0; rq.to_host = true;
        rq.indices = out_indices; rq.keys = out_keys; rq.capacity = capacity; rq.out_total = out_total;
        rq.group_keys = out_group_keys; rq.group_offsets = out_group_offsets; rq.group_capacity = group_capacity; rq.out_groups = out_groups;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        const size_t bytes = (size_t)sel.n * cell_stride;       // the null stream throughout: records through the cell staging
        h->tag_cached_bytes = 0;                                // (stage_in is about to be overwritten)
        if (int rc = ensure(h, h->stage_in, bytes, "input staging")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, cells, bytes)) return rc;
        sel.src.cells = static_cast<const char*>(h->stage_in.ptr);
        sel.surface_only = surface_only != 0;
        sel.draw_zero = draw_zero != 0;
        return display_select_impl(h, sel, rq, nullptr);
    });
}

int sdfgpu_display_select_sdf_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, uint32_t* d_indices,
                                     int64_t capacity, int64_t* out_total, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        DpSelect sel;
        if (int rc = check_display_sdf(h, d_sdf, nx, ny, nz, sel)) return rc;
        if (reinterpret_cast<uintptr_t>(d_sdf) & 3) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: d_sdf must be 4-byte aligned");
        DisplayRequest rq;
        rq.rule = kDpRuleSdfNonPositive;
        rq.indices = d_indices; rq.capacity = capacity; rq.out_total = out_total;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        sel.src.cells = reinterpret_cast<const char*>(d_sdf);
        return display_select_impl(h, sel, rq, (hipStream_t)stream);
    });
}

int sdfgpu_display_select_sdf(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, uint32_t* out_indices, int64_t capacity,
                              int64_t* out_total) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        DpSelect sel;
        if (int rc = check_display_sdf(h, sdf, nx, ny, nz, sel)) return rc;
        DisplayRequest rq;
        rq.rule = kDpRuleSdfNonPositive;
        rq.to_host = true;
        rq.indices = out_indices; rq.capacity = capacity; rq.out_total = out_total;
        if (int rc = check_display_request(h, rq)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        h->tag_cached_bytes = 0;
        if (int rc = ensure(h, h->stage_in, (size_t)sel.n * 4, "input staging")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, sdf, (size_t)sel.n * 4)) return rc;
        sel.src.cells = static_cast<const char*>(h->stage_in.ptr);
        return display_select_impl(h, sel, rq, nullptr);
    });
}

int sdfgpu_display_expand_device(sdfgpu_handle h, const uint32_t* d_indices, const uint32_t* d_keys, int64_t count, int64_t nx, int64_t ny,
                                 int64_t nz, const double cell_sizes[3], double* d_points, float* d_colors, const float* d_color_table,
                                 int64_t table_entries, const float default_color[4], void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        if (!d_indices || !cell_sizes || (!d_points && !d_colors)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
        if (d_colors && (!default_color || table_entries < 0 || table_entries > (int64_t)0xFFFFFFFFll || (table_entries > 0 && !d_color_table)))
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: colours need a default colour and a table of [0, 2^32) entries");
        if (count < 0 || count > (int64_t)0xFFFFFFFFll)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: count must be in [0, 2^32) (got %lld)", (long long)count);
        if (int rc = check_display_dims(h, nx, ny, nz)) return rc;
        if ((reinterpret_cast<uintptr_t>(d_indices) | reinterpret_cast<uintptr_t>(d_keys) | reinterpret_cast<uintptr_t>(d_points) |
             reinterpret_cast<uintptr_t>(d_colors) | reinterpret_cast<uintptr_t>(d_color_table)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: device pointers must be 4-byte aligned");
        HIP_TRY(h, hipSetDevice(h->device));
        DpExpand a;
        a.idx = d_indices; a.keys = d_keys; a.count = (uint64_t)count;
        a.ny = (uint32_t)ny; a.nz = (uint32_t)nz;
        for (int i = 0; i < 3; ++i) a.cell[i] = cell_sizes[i];
        a.points = reinterpret_cast<uint32_t*>(d_points);
        a.colors = d_colors;
        if (d_colors) {
            a.table = d_color_table; a.table_len = (uint32_t)table_entries;
            for (int i = 0; i < 4; ++i) a.fallback[i] = default_color[i];
        }
        HIP_TRY(h, dp_launch_expand(a, (hipStream_t)stream));
        return SDFGPU_OK;
    });
}

int sdfgpu_display_sdf_colors_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, float alpha, float* d_colors,
                                     void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        DpSelect sel;
        if (!d_colors) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
        if (int rc = check_display_sdf(h, d_sdf, nx, ny, nz, sel)) return rc;
        if (std::isnan(alpha)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: alpha must not be NaN");
        if ((reinterpret_cast<uintptr_t>(d_sdf) | reinterpret_cast<uintptr_t>(d_colors)) & 3)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: d_sdf and d_colors must be 4-byte aligned");
        HIP_TRY(h, hipSetDevice(h->device));
        return display_sdf_colors_impl(h, d_sdf, sel.n, alpha, d_colors, (hipStream_t)stream);
    });
}

int sdfgpu_display_sdf_colors(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, float alpha, float* out_colors) {
    return rz_wrap(h, nullptr, [&]() -> int {
        if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
        DpSelect sel;
        if (!out_colors) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: null pointer");
        if (int rc = check_display_sdf(h, sdf, nx, ny, nz, sel)) return rc;
        if (std::isnan(alpha)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "display: alpha must not be NaN");
        HIP_TRY(h, hipSetDevice(h->device));
        h->tag_cached_bytes = 0;
        if (int rc = ensure(h, h->stage_in, (size_t)sel.n * 4, "input staging")) return rc;
        if (int rc = ensure(h, h->stage_out, (size_t)sel.n * 16, "output staging")) return rc;
        if (int rc = copy_from_host(h, h->stage_in.ptr, sdf, (size_t)sel.n * 4)) return rc;
        if (int rc = display_sdf_colors_impl(h, (const float*)h->stage_in.ptr, sel.n, alpha, (float*)h->stage_out.ptr, nullptr)) return rc;
        return copy_to_host(h, out_colors, h->stage_out.ptr, (size_t)sel.n * 16);
    });
}

}  // extern "C"
