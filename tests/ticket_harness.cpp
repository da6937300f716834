// ticket_harness.cpp -- the ticket protocol of the single stand-by launch (sdf_tools_amd/csrc/sdfgpu_tickets.hpp: claim, arrive,
// wait) on the CPU.  The kernel (k_envelope_standby) and this harness run the SAME three functions; here the memory operations
// are the host's atomics and a "workgroup" is a function call on a worker thread.
//
//   ticket_harness <seed> <iters>
//
// G logical workgroups run on R worker threads, R = 1, 2, 3 < G and R = G.  A worker starts its next workgroup only when the
// current one has RETURNED -- a machine on which only R workgroups are resident at a time, with no way to pre-empt one that
// waits.  Each workgroup is the kernel's loop: claim a ticket; a ticket below T2 is a y tile (write the tile's plain words, then
// arrive), one from T2 on is an x tile (wait for all T2 arrivals, acquire, read EVERY y tile's words).  Checked per run:
//   * the run completes (a watchdog ends a hang with exit code 4): progress does not depend on residency -- a workgroup that waits
//     holds a ticket >= T2, so every y ticket is already held by a workgroup that is running and never waits;
//   * every ticket ran exactly once;
//   * every x tile started after the last y tile was complete, and read the words every y tile wrote;
//   * no wait ran into its bound.
// Built plain and with -fsanitize=thread (tests/test_tickets_cpu.py): the y tiles' words are plain memory, ordered against the x
// tiles' reads by the protocol alone.  The sanitizer does not model stand-alone fences, so the host's Ops carry the release on the
// arrival's add and the acquire on the poll's load as well; where the DEVICE's fences stand is what tests/test_gpu_standby_single.py
// checks.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "../sdf_tools_amd/csrc/sdfgpu_tickets.hpp"

namespace {

struct HostOps {
    uint32_t fetch_add(uint32_t* p) { return __atomic_fetch_add(p, 1u, __ATOMIC_ACQ_REL); }
    uint32_t load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    void release() { std::atomic_thread_fence(std::memory_order_release); }
    void acquire() { std::atomic_thread_fence(std::memory_order_acquire); }
    void pause() { ++polls; std::this_thread::yield(); }
    uint64_t now() { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    uint64_t polls = 0;
};

struct Run {
    uint32_t t2, t3;
    uint32_t next = 0, done_y = 0, failed = 0;      // the three status words
    std::vector<uint32_t> plane;                    // [t2 * kWords] plain words: the "plane field" a y tile writes
    std::vector<uint32_t> ran;                      // [t2 + t3] how often each ticket ran
    std::vector<uint64_t> stamp;                    // [t2 + t3] y: when the tile was complete, x: when its wait was over
    std::vector<uint64_t> sum;                      // [t3] what each x tile read
    std::atomic<uint64_t> clock{1};                 // (relaxed: it orders nothing for the sanitizer)
    std::atomic<uint64_t> waits{0};
};
constexpr int kWords = 16;
constexpr uint64_t kBudgetUs = 60ull * 1000 * 1000;

// The loop of k_envelope_standby behind its guard, one call per logical workgroup.
void workgroup(Run& r, uint32_t seed, int slow_us) {
    HostOps ops;
    std::minstd_rand rng(seed);
    bool y_seen = false;
    for (;;) {
        const uint32_t ticket = sdfgpu::ticket_claim(ops, &r.next);
        if (ticket >= r.t2 + r.t3) break;
        ++r.ran[ticket];
        if (ticket < r.t2) {
            if (slow_us) std::this_thread::sleep_for(std::chrono::microseconds(rng() % (unsigned)slow_us));
            for (int k = 0; k < kWords; ++k) r.plane[(size_t)ticket * kWords + k] = ticket * 31u + (uint32_t)k + 1u;
            r.stamp[ticket] = r.clock.fetch_add(1, std::memory_order_relaxed);
            sdfgpu::ticket_arrive(ops, &r.done_y);
        } else {
            if (!y_seen) {
                const uint64_t before = ops.polls;
                if (!sdfgpu::ticket_wait(ops, &r.done_y, r.t2, kBudgetUs)) { __atomic_store_n(&r.failed, 1u, __ATOMIC_RELAXED); break; }
                ops.acquire();
                y_seen = true;
                if (ops.polls != before) r.waits.fetch_add(1, std::memory_order_relaxed);
            }
            r.stamp[ticket] = r.clock.fetch_add(1, std::memory_order_relaxed);
            uint64_t s = 0;
            for (size_t i = 0; i < r.plane.size(); ++i) s += r.plane[i];
            r.sum[ticket - r.t2] = s;
        }
    }
}

int run_one(uint32_t G, uint32_t R, uint32_t t2, uint32_t t3, uint32_t seed, int slow_us, uint64_t& waits) {
    Run r;
    r.t2 = t2; r.t3 = t3;
    r.plane.assign((size_t)t2 * kWords, 0u);
    r.ran.assign((size_t)t2 + t3, 0u);
    r.stamp.assign((size_t)t2 + t3, 0u);
    r.sum.assign(t3, 0u);
    std::atomic<uint32_t> dispatch{0};                      // workgroups are started in index order, one per free worker
    std::vector<std::thread> workers;
    for (uint32_t w = 0; w < R; ++w)
        workers.emplace_back([&] {
            for (;;) {
                const uint32_t g = dispatch.fetch_add(1, std::memory_order_relaxed);
                if (g >= G) return;
                workgroup(r, seed * 7919u + g, slow_us);
            }
        });
    for (auto& t : workers) t.join();
    waits = r.waits.load();
    if (r.failed) { fprintf(stderr, "G=%u R=%u t2=%u t3=%u: a wait ran into its bound\n", G, R, t2, t3); return 1; }
    uint64_t want = 0, last_y = 0;
    for (uint32_t t = 0; t < t2; ++t) {
        for (int k = 0; k < kWords; ++k) want += t * 31u + (uint32_t)k + 1u;
        if (r.stamp[t] > last_y) last_y = r.stamp[t];
    }
    for (uint32_t t = 0; t < t2 + t3; ++t)
        if (r.ran[t] != 1u) { fprintf(stderr, "G=%u R=%u t2=%u t3=%u: ticket %u ran %u times\n", G, R, t2, t3, t, r.ran[t]); return 1; }
    for (uint32_t t = 0; t < t3; ++t) {
        if (r.stamp[t2 + t] <= last_y) { fprintf(stderr, "G=%u R=%u t2=%u t3=%u: x tile %u started before the last y tile was complete\n", G, R, t2, t3, t); return 1; }
        if (r.sum[t] != want) { fprintf(stderr, "G=%u R=%u t2=%u t3=%u: x tile %u read %llu, want %llu\n", G, R, t2, t3, t, (unsigned long long)r.sum[t], (unsigned long long)want); return 1; }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: ticket_harness <seed> <iters>\n"); return 2; }
    const uint32_t seed = (uint32_t)atoi(argv[1]);
    const int iters = atoi(argv[2]);
    std::thread([] { std::this_thread::sleep_for(std::chrono::seconds(120)); fprintf(stderr, "ticket_harness: watchdog -- a workgroup waits for ever\n"); _Exit(4); }).detach();
    // {G, t2, t3}: tickets that wrap in both stages, fewer tickets than workgroups, one tile per stage, a stage without tiles
    const uint32_t shapes[][3] = {{32, 160, 104}, {8, 5, 3}, {16, 1, 1}, {4, 40, 7}, {6, 3, 50}, {5, 0, 9}, {5, 9, 0}, {64, 2, 2}};
    uint64_t runs = 0, waited = 0;
    for (int it = 0; it < iters; ++it)
        for (const auto& s : shapes)
            for (uint32_t R : {1u, 2u, 3u, s[0]}) {
                uint64_t w = 0;
                // (every other run with slow y tiles: workers then meet the x tickets while y tiles are still running, and wait)
                if (int rc = run_one(s[0], R, s[1], s[2], seed + (uint32_t)it, (it & 1) ? 200 : 0, w)) return rc;
                ++runs; waited += w;
            }
    printf("ticket protocol OK: %llu runs, %llu workgroups waited for the y stage\n", (unsigned long long)runs, (unsigned long long)waited);
    return 0;
}
