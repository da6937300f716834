// sdfgpu_policy.hpp -- the host-side policy of the dense tier, as one plain C++ object (no HIP in here: the CPU suite compiles
// this header with g++ and drives it through sequences of reports, tests/policy_harness.cpp).
//
// Every decision below is EXACTNESS-NEUTRAL: results never depend on it, only which kernels are enqueued in front of / behind
// which guard.  Which tier does a SWEEP is not decided here at all (that happens on the device inside each build); what the
// handle learns from the status block of an earlier build -- which arrives asynchronously, possibly many builds late -- is only
//   * whether the dense tier is worth enqueueing (pause it after a failure, probe again later, back off while probes fail),
//   * which form of it (KD alone; KD with the fix-up stage KD3 + KF staged behind it; the fix-up stage in KD's place),
//   * whether the general pipeline behind it may be the cheap two-launch stand-by (only behind a TRUSTED dense tier).
// (Round 4: extracted from build_device_impl, where these 40 lines of state machine lived between launches -- VERDICT r3 weak #8,
//  and the sequence ADVICE r3 asked to pin: staged build -> fix-up mode -> failing seed.)
#pragma once
#include <algorithm>
#include <cstdint>

namespace sdfgpu {

// "This handle's scene is a far-field scene on both axes" (round 5).  Learnt from the far flags of the status blocks that come back
// (status words 4 and 5: the y / x sweep was the far-field kernel's); a build in the habit enqueues KE2 -> KE3 directly, without the two
// tier probes and the three guarded marching launches.  Like everything in this header it is exactness-neutral: the far-field pair is
// exact on any scene, so a stale habit costs time on at most kProbeEvery - 1 builds, never a voxel.
struct FarHabit {
    static constexpr int kStreak = 4;                // far-field reports in a row before the probes are dropped
    static constexpr unsigned kProbeEvery = 16;      // ... and every 16th build carries them again
    int mode = 1;                                    // option "far_predict": 0 never, 1 learnt, 2 every build (tests, the fuzz)
    int streak = 0;                                  // consecutive reported builds whose y AND x sweeps were far-field
    uint64_t seq = 0;                                // builds planned so far

    void reset() { streak = 0; }
    void set_mode(int m) { mode = (m >= 0 && m <= 2) ? m : 1; streak = 0; }
    // a report has arrived (any build's: a dense-certified build has both flags down and ends the habit at once)
    void consume_report(bool far_y, bool far_x) { streak = (far_y && far_x) ? std::min(streak + 1, 1 << 20) : 0; }
    // One call per build.  selectable: the build would otherwise choose its sweeps' tiers on the device (probes); forced: a tier is
    // forced by an option (nothing to predict).  Returns whether this build takes the far-field pair without probing.
    bool plan(bool selectable, bool forced) {
        ++seq;
        return selectable && !forced && (mode == 2 || (mode == 1 && streak >= kStreak && (seq % kProbeEvery) != 0u));
    }
};

// What a build was, remembered with its report.
struct ReportedBuild {
    bool dense = false;      // the dense kernels were enqueued
    bool generic = false;    // ... in their generic form (any nz / no fix-up stage behind it)
    bool fix_mode = false;   // ... as the fix-up stage (KD3 or KD with KF behind it, in fix-up mode)
    bool staged = false;     // ... as KD with the fix-up stage staged behind it, guarded on KD's verdict
    bool predicted = false;  // the far-field pair was enqueued on the strength of earlier builds: its far flags say "the launch ran",
                             // not "a probe found the scene far-field" -- they must not extend the habit
};

// What the next build enqueues around the dense kernels.
struct DensePlan {
    bool dense = false;      // enqueue the dense tier at all
    bool fix = false;        // fix-up mode: undecided voxels go to KF
    bool dense3 = false;     // KD3 in KD's place (with KF behind it)
    bool staged = false;     // KD, then KD3 + KF guarded on KD's verdict
    bool fix_mode_build() const { return fix || dense3; }
};

struct DensePolicy {
    // ---- options (sdfgpu_set_option) ----
    int dense3_on = 1;            // KD3 (ball kernel with |offset| <= 3) in KD's place whenever the fix-up kernel runs
    bool dense3_mode = false;     // KD3 + KF with every dense build (tests)
    int dense3_staged = 1;        // a build that does not expect KD to decide the scene carries KD3 + KF behind KD
    int dense_retry = 16;         // after an uncertified dense attempt, probe the dense kernels again after N - 1 builds (0 = always try)
    // ---- learned ----
    bool fix_mode = false;        // launch the fix-up stage with the next dense build
    int fix_clean = 0;            // consecutive fix-mode builds that needed no fix (the mode is left after 8)
    int fix_trust = 0;            // certified fix-up-mode reports in a row (the cheap stand-by needs 4)
    int dense_skip = 0;           // builds left that skip the dense kernels
    int dense_backoff = 0;        // current length of that pause: doubles while the probes keep failing
    bool expect_dense = false;    // the dense tier is trusted to certify the next build's scene
    ReportedBuild prev;           // the build whose report is outstanding / was consumed last

    void reset() {
        expect_dense = false; dense_skip = 0; dense_backoff = 0; fix_mode = false; dense3_mode = false; fix_trust = 0;
    }

    // The status block of the build remembered in `prev` has arrived: uncertified = status word 3 (the dense tier left voxels
    // to the general pipeline), fix_needed = word 6 (KF had work), kd_uncertified = word 8 (a staged build: KD's own verdict).
    void consume_report(bool uncertified, bool fix_needed, bool kd_uncertified) {
        const bool general_ran = !prev.dense || uncertified;
        // The cheap stand-by is only safe behind a dense tier that is trusted to certify the scene: on a noise-like scene at the
        // edge of the fix-up stage's reach (Bernoulli p = 0.02: two seeds of three certify) every failed build would run it over
        // a sparse grid.  A handle whose builds go through the fix-up stage earns it with 4 certified reports in a row and
        // loses it with the first failure.  A STAGED build that KD failed and the fix-up stage certified is such a report
        // like any other.
        const bool via_fix = prev.fix_mode || (prev.staged && kd_uncertified);
        if (prev.dense && via_fix) fix_trust = general_ran ? 0 : std::min(255, fix_trust + 1);
        expect_dense = !general_ran && (!via_fix || fix_trust >= 4);
        // almost dense (the ball kernel left voxels undecided): first the fix-up stage; only if that cannot certify the scene
        // either are the dense kernels paused
        if (prev.dense && !prev.generic) {
            if (!prev.fix_mode) { fix_mode = prev.staged ? kd_uncertified : uncertified; fix_clean = 0; }   // KD alone could not
            else if (uncertified) fix_mode = false;                                 // KF could not certify it either
            else {                                                                  // keep the stage while it is needed: left
                fix_clean = fix_needed ? 0 : fix_clean + 1;                         // after 8 clean builds in a row (a scene at
                if (fix_clean >= 8) { fix_mode = false; fix_clean = 0; }            // the edge of the ball must not flap)
            }
        }
        // dense attempted, not certified, nothing further to escalate to: pause the dense kernels (0.13 ms wasted per attempt
        // at 512^3) for dense_retry - 1 builds, twice as long (+1) after every failed probe
        if (prev.dense && uncertified && dense_retry > 0 && (prev.fix_mode || prev.staged || prev.generic)) {
            dense_backoff = dense_backoff ? std::min(255, 2 * dense_backoff + 1) : dense_retry - 1;
            dense_skip = dense_backoff;
        }
        if (prev.dense && !uncertified) { dense_backoff = 0; dense_skip = 0; }     // certified again: start over
    }

    // One call per build.  dense_eligible: the shape / options allow the dense tier; generic: only in its generic form;
    // d3_shape_ok: the shape takes KD3 (256-lane tiles); vb: add_virtual_border.
    DensePlan plan(bool dense_eligible, bool generic, bool d3_shape_ok, bool vb) {
        DensePlan p;
        bool dense = dense_eligible;
        if (dense && dense_skip > 0) { --dense_skip; dense = false; }
        // A retry after a pause is a PROBE: pause again at once, on the assumption that it fails like the attempts before it,
        // and let its report lift the pause if it did not.  (With the pause re-armed only when the failure report arrived, a
        // caller that enqueues builds without synchronising -- the report is then ~30 builds late -- attempted the dense tier
        // in EVERY build between the end of a pause and that report: Bernoulli p = 0.015 at 512^3 took 1.16 ms per build
        // where p = 0.01 takes 1.00.)
        else if (dense && dense_backoff > 0 && dense_retry > 0) dense_skip = dense_backoff;
        p.dense = dense;
        if (dense && !generic) {
            // fix-up mode: undecided voxels go to KF, which raises `uncertified` only for what it cannot decide either
            // (with a virtual border KF stays out: a voxel it would finish may still be bound by b >= 3)
            p.fix = fix_mode && !vb;
            const bool d3_ok = dense3_on && !vb && d3_shape_ok;
            p.dense3 = d3_ok && (p.fix || dense3_mode);
            // A build that has no reason to expect that KD decides the scene (a fresh context: the reference API is one-shot;
            // or the build after a failure) carries the fix-up stage behind KD in the SAME build, guarded on KD's verdict
            p.staged = d3_ok && !p.dense3 && !expect_dense && dense3_staged;
        }
        return p;
    }
};

}  // namespace sdfgpu
