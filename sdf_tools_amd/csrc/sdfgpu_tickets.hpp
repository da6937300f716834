// Two dependent stages in ONE plain launch, ordered by tickets: claim, arrive, wait.
//
// The stand-by behind a trusted dense tier is a y sweep and an x sweep that needs the WHOLE y sweep.  As two launches the
// kernel boundary is the dependency; k_envelope_standby (sdfgpu_envelope_dc.hpp) runs both from one launch instead.  Its
// workgroups claim tickets from one counter: tickets [0, T2) are the tiles of the first stage, [T2, T2 + T3) those of the
// second (in the kernel a ticket is a run of four consecutive tiles; the protocol does not care).  A workgroup that has
// finished a first-stage tile ARRIVES (release, then + 1 on a second counter); a workgroup that holds a second-stage ticket
// WAITS until that counter reads T2, then acquires.
//
// Why this needs neither a grid barrier nor every workgroup resident: tickets are claimed in increasing order, so a workgroup
// that waits holds a ticket >= T2 -- and then every ticket below T2 has already been claimed, by a workgroup that is running
// (it claimed from inside the kernel) and that never waits before it arrives.  The first stage therefore always completes,
// whatever the grid size, the number of resident workgroups or their placement; tests/ticket_harness.cpp executes that
// argument with fewer workers than workgroups.
//
// The three steps are templates over the memory operations (`Ops`), so that the harness runs THIS code on std::atomic and
// threads, and the kernel runs it on agent-scope atomics and fences:
//   uint32_t fetch_add(uint32_t* p)          relaxed + 1, returns the old value
//   uint32_t load(const uint32_t* p)         relaxed load that is not cached across polls
//   void release() / void acquire()          fences that make the first stage's stores visible to the second stage's loads
//   void pause()                             between two polls
//   uint64_t now()                           a clock for the bound of the wait
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SDFGPU_TICKET_FN __host__ __device__ __forceinline__
#else
#define SDFGPU_TICKET_FN inline
#endif

namespace sdfgpu {

// The next ticket.  Every value comes out once; a value at or beyond the number of tickets means "nothing left".
template <class Ops>
SDFGPU_TICKET_FN uint32_t ticket_claim(Ops& ops, uint32_t* next) { return ops.fetch_add(next); }

// A first-stage tile is complete.  The caller has made sure that all of the tile's stores have been issued AND have left the
// workgroup (on the device: every wave waits for its stores, then the workgroup's barrier, then ONE lane calls this).
template <class Ops>
SDFGPU_TICKET_FN void ticket_arrive(Ops& ops, uint32_t* done) {
    ops.release();
    (void)ops.fetch_add(done);
}

// Wait until all `want` first-stage tiles have arrived; false when `budget` ticks of ops.now() pass first.  The poll is a
// relaxed load: ONE acquire follows the match, by the caller (on the device every wave of the workgroup does it, behind the
// barrier that hands this result round).
template <class Ops>
SDFGPU_TICKET_FN bool ticket_wait(Ops& ops, const uint32_t* done, uint32_t want, uint64_t budget) {
    if (ops.load(done) == want) return true;
    const uint64_t t0 = ops.now();
    for (;;) {
        ops.pause();
        if (ops.load(done) == want) return true;
        if (ops.now() - t0 > budget) return false;
    }
}

}  // namespace sdfgpu
