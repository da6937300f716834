// CPU harness around sdf_tools_amd/csrc/sdfgpu_plan.hpp (host-only: no HIP): the test compiles this file with g++ into a shared
// library and asks plan_build what a build would enqueue, for facts and options a GPU test can only reach by building scenes.
#include <cstdint>
#include <cstring>

#include "../sdf_tools_amd/csrc/sdfgpu_plan.hpp"

using namespace sdfgpu;

namespace {
struct Planner {
    BuildOptions opt;
    DensePolicy pol;
    FarHabit far;
};
}  // namespace

extern "C" {

void* plan_new() { return new Planner(); }
void plan_free(void* h) { delete static_cast<Planner*>(h); }

// the options the planner reads, under the names and with the meanings of sdfgpu_set_option; 0 = ok, 1 = not one of them
int plan_set_option(void* h, const char* name, int value) {
    Planner* p = static_cast<Planner*>(h);
    BuildOptions& o = p->opt;
    auto is = [&](const char* n) { return std::strcmp(name, n) == 0; };
    if (is("dense")) o.dense_on = value != 0;
    else if (is("dense_generic")) o.dense_generic_on = value != 0;
    else if (is("dense_retry")) { p->pol.dense_retry = value; p->pol.dense_skip = 0; p->pol.dense_backoff = 0; }
    else if (is("envelope")) o.envelope_on = value != 0;
    else if (is("envelope_mode")) o.force_env = value != 0 ? 1 : -1;
    else if (is("far_predict")) p->far.set_mode(value);
    else if (is("policy_reset")) { p->pol.reset(); p->far.reset(); }
    else if (is("expect_dense")) p->pol.expect_dense = value != 0;
    else if (is("fixup_mode")) p->pol.fix_mode = value != 0;
    else if (is("dense3_mode")) p->pol.dense3_mode = value != 0;
    else if (is("standby_far")) o.standby_far = value != 0;
    else if (is("standby_fold")) o.standby_fold = value != 0;
    else if (is("standby_single")) o.standby_single = value != 0;
    else if (is("fused_zy")) { o.fused_zy = value != 0; o.fused_always = value == 2; }
    else if (is("plane16")) o.plane16_on = value != 0;
    else if (is("i32_handoff")) o.i32_handoff = value != 0;
    else if (is("plane_skip")) o.plane_skip = value != 0;
    else return 1;
    return 0;
}

void plan_far_report(void* h, int far_y, int far_x) { static_cast<Planner*>(h)->far.consume_report(far_y != 0, far_x != 0); }
// what the two policy objects count: 0 FarHabit::seq, 1 DensePolicy::dense_skip (set: 1 only)
int64_t plan_counter(void* h, int which) {
    Planner* p = static_cast<Planner*>(h);
    return which == 0 ? (int64_t)p->far.seq : (int64_t)p->pol.dense_skip;
}
void plan_set_dense_skip(void* h, int builds) { static_cast<Planner*>(h)->pol.dense_skip = builds; }

// facts: nx, ny, nz, vb, occupancy kind (0 mask, 1 cells, 2 bits), occ16, out16, dense_shape, far_shape y, far_shape x,
// z_wave_shape, fused_nz, dense_slot_free, far_slot_free.
// out: [0] the flags below, [1] Bits, [2] Report, [3..8] bytes of yz, plane16, z, bits, unc, planebits.
enum : int64_t {
    kOut16 = 1 << 0, kP16 = 1 << 1, kDense = 1 << 2, kDenseGeneric = 1 << 3, kFix = 1 << 4, kDense3 = 1 << 5, kStaged = 1 << 6,
    kFarOk = 1 << 7, kEnvelope = 1 << 8, kStandby = 1 << 9, kStandbySingle = 1 << 10, kFused = 1 << 11, kSelect = 1 << 12,
    kPredicted = 1 << 13, kHandoff = 1 << 14, kWindowChoice = 1 << 15, kPlaneSkip = 1 << 16, kStandbyFolds = 1 << 17,
    kZSweep = 1 << 18, kFarPair = 1 << 19
};
void plan_run(void* h, const int64_t* facts, int64_t* out) {
    Planner* p = static_cast<Planner*>(h);
    BuildFacts f;
    f.nx = facts[0]; f.ny = facts[1]; f.nz = facts[2]; f.vb = facts[3] != 0;
    f.occ = facts[4] == 1 ? BuildFacts::Occ::cells : facts[4] == 2 ? BuildFacts::Occ::bits : BuildFacts::Occ::mask;
    f.occ16 = facts[5] != 0; f.out16 = facts[6] != 0; f.dense_shape = facts[7] != 0;
    f.far_shape[0] = facts[8] != 0; f.far_shape[1] = facts[9] != 0;
    f.z_wave_shape = facts[10] != 0; f.fused_nz = facts[11] != 0;
    f.dense_slot_free = facts[12] != 0; f.far_slot_free = facts[13] != 0;
    const BuildPlan b = plan_build(p->opt, p->pol, p->far, f);
    out[0] = (b.out16 ? kOut16 : 0) | (b.p16 ? kP16 : 0) | (b.dense ? kDense : 0) | (b.dense_generic ? kDenseGeneric : 0) |
             (b.tier.fix ? kFix : 0) | (b.tier.dense3 ? kDense3 : 0) | (b.tier.staged ? kStaged : 0) | (b.far_ok ? kFarOk : 0) |
             (b.envelope ? kEnvelope : 0) | (b.standby ? kStandby : 0) | (b.standby_single ? kStandbySingle : 0) |
             (b.fused ? kFused : 0) | (b.select ? kSelect : 0) | (b.predicted ? kPredicted : 0) | (b.handoff ? kHandoff : 0) |
             (b.window_choice ? kWindowChoice : 0) | (b.plane_skip ? kPlaneSkip : 0) | (b.standby_folds ? kStandbyFolds : 0) |
             (b.z_sweep() ? kZSweep : 0) | (b.far_pair() ? kFarPair : 0);
    out[1] = (int64_t)b.bits;
    out[2] = (int64_t)b.report;
    out[3] = (int64_t)b.yz_bytes; out[4] = (int64_t)b.plane16_bytes; out[5] = (int64_t)b.z_bytes;
    out[6] = (int64_t)b.bits_bytes; out[7] = (int64_t)b.unc_bytes; out[8] = (int64_t)b.planebits_bytes;
}

}  // extern "C"
