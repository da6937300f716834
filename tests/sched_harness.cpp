// sched_harness.cpp -- the library's host-side schedulers (sdf_tools_amd/csrc/sdfgpu_hostteam.hpp) on the CPU, with the device
// behind fakes: built plain and with -fsanitize=thread by tests/test_host_cpu.py (VERDICT r5 "next round" 5).
//
//   sched_harness team    <seed> <iters>     HostTeam: every index of every job runs exactly once, team sizes 1 .. 33
//   sched_harness upload  <seed> <iters>     staged_upload against a fake DMA engine (its own thread, random latencies), random sizes,
//                                            team 1 .. 32, a slow member, an injected DMA error now and then: bytes must arrive intact
//   sched_harness upload_prefix <seed> <iters>   the same on the PRE-FIX arithmetic (one running total of filled slices): exits 3
//                                            when a chunk went out unfinished (and -fsanitize=thread reports the race itself)
//   sched_harness drain   <seed> <iters>     staged_drain likewise
//   sched_harness ranks   <seed> <iters>     RankTeam: 1 .. 8 ranks, builds of compute / exchange / wait steps with and without host
//                                            barriers, a rank failing at a random step: the run must come back with that rank and
//                                            must not hang (a posted exchange is ended by on_stuck, like ncclCommAbort)
// Exit code 0 = all checks passed.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../sdf_tools_amd/csrc/sdfgpu_hostteam.hpp"

using namespace sdfgpu;

namespace {

void nap(std::mt19937& rng, int max_us) {
    const int us = (int)(rng() % (unsigned)(max_us + 1));
    if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
}

// A DMA engine with two staging buffers and one "event" per buffer, like the pinned chunks + hipEvents of sdfgpu_context.hpp: copies are
// executed by the engine's own thread some time after they were issued.
struct FakeDma {
    struct Op { char* dst; const char* src; size_t len; int buf; };
    std::mutex m;
    std::condition_variable cv;
    std::deque<Op> q;
    uint64_t issued[2] = {0, 0}, completed[2] = {0, 0};
    bool quit = false;
    std::mt19937 rng;
    std::thread th;
    explicit FakeDma(unsigned seed) : rng(seed), th([this] { loop(); }) {}
    ~FakeDma() {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv.notify_all();
        th.join();
    }
    void loop() {
        for (;;) {
            Op op;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return quit || !q.empty(); });
                if (q.empty()) return;
                op = q.front();
                q.pop_front();
            }
            nap(rng, 200);
            memcpy(op.dst, op.src, op.len);
            {
                std::lock_guard<std::mutex> lk(m);
                ++completed[op.buf];
            }
            cv.notify_all();
        }
    }
    void issue(char* dst, const char* src, size_t len, int buf) {
        { std::lock_guard<std::mutex> lk(m); q.push_back({dst, src, len, buf}); ++issued[buf]; }
        cv.notify_all();
    }
    void wait(int buf) {
        std::unique_lock<std::mutex> lk(m);
        const uint64_t want = issued[buf];
        cv.wait(lk, [&] { return completed[buf] >= want; });
    }
    void drain_all() { wait(0); wait(1); }
};

int test_team(unsigned seed, int iters) {
    std::mt19937 rng(seed);
    HostTeam team;
    for (int it = 0; it < iters; ++it) {
        const int n = 1 + (int)(rng() % 33);
        std::vector<std::atomic<int>> hits((size_t)n);
        for (auto& h : hits) h.store(0);
        team.run(n, [&](int w) { hits[(size_t)w].fetch_add(1); });
        for (int w = 0; w < n; ++w)
            if (hits[(size_t)w].load() != 1) { fprintf(stderr, "team: job %d index %d ran %d times\n", it, w, hits[(size_t)w].load()); return 1; }
    }
    printf("team ok: %d jobs, %d workers alive\n", iters, team.workers());
    return 0;
}

template <bool kFixed>
int test_upload(unsigned seed, int iters) {
    std::mt19937 rng(seed);
    HostTeam team;
    FakeDma dma(seed ^ 0x5bd1e995u);
    constexpr size_t kChunk = 64 << 10;
    std::vector<char> pin[2] = {std::vector<char>(kChunk), std::vector<char>(kChunk)};
    int bad_runs = 0, errors_seen = 0;
    for (int it = 0; it < iters; ++it) {
        const size_t bytes = 1 + rng() % (kChunk * 9);
        const int members = 1 + (int)(rng() % 32);
        const int slow = (int)(rng() % (unsigned)members);
        const int64_t fail_at = (rng() % 8 == 0) ? (int64_t)(rng() % ((bytes + kChunk - 1) / kChunk)) : -1;
        std::vector<char> src(bytes), dev(bytes, (char)0x5A);
        for (size_t i = 0; i < bytes; ++i) src[i] = (char)(rng() >> 7);
        std::atomic<unsigned> salt{(unsigned)rng()};
        const int rc = staged_upload<kFixed>(
            team, bytes, kChunk, members,
            [&](int buf, size_t off, size_t goff, size_t len) {
                std::mt19937 local(salt.fetch_add(1) * 2654435761u);
                // one member is slow now and then: its slice of chunk i is still being written while the others are a chunk ahead
                if ((int)((off / 4096) % (unsigned)members) == slow || local() % 5 == 0) nap(local, 300);
                memcpy(pin[buf].data() + off, src.data() + goff, len / 2);
                if (local() % 3 == 0) nap(local, 100);
                memcpy(pin[buf].data() + off + len / 2, src.data() + goff + len / 2, len - len / 2);
            },
            [&](int64_t i, int buf, size_t len) -> int {
                if (i == fail_at) return 7;
                dma.issue(dev.data() + (size_t)i * kChunk, pin[buf].data(), len, buf);
                return 0;
            },
            [&](int buf) -> int { dma.wait(buf); return 0; });
        dma.drain_all();
        if (fail_at >= 0) {
            if (rc != 7) { fprintf(stderr, "upload: injected error at chunk %lld came back as %d\n", (long long)fail_at, rc); return 1; }
            ++errors_seen;
            continue;
        }
        if (rc != 0) { fprintf(stderr, "upload: rc %d\n", rc); return 1; }
        if (memcmp(dev.data(), src.data(), bytes) != 0) {
            ++bad_runs;
            if (kFixed) { fprintf(stderr, "upload: %zu bytes, team %d: data corrupted\n", bytes, members); return 1; }
        }
    }
    printf("upload%s: %d runs, %d injected errors returned, %d corrupted\n", kFixed ? "" : " (pre-fix arithmetic)", iters, errors_seen, bad_runs);
    return (!kFixed && bad_runs > 0) ? 3 : 0;
}

int test_drain(unsigned seed, int iters) {
    std::mt19937 rng(seed);
    HostTeam team;
    FakeDma dma(seed ^ 0x27d4eb2fu);
    constexpr size_t kChunk = 64 << 10;
    std::vector<char> pin[2] = {std::vector<char>(kChunk), std::vector<char>(kChunk)};
    int errors_seen = 0;
    for (int it = 0; it < iters; ++it) {
        const size_t bytes = 1 + rng() % (kChunk * 9);
        const int members = 1 + (int)(rng() % 16);
        const int64_t fail_at = (rng() % 8 == 0) ? (int64_t)(rng() % ((bytes + kChunk - 1) / kChunk)) : -1;
        std::vector<char> dev(bytes), dst(bytes, (char)0x33);
        for (size_t i = 0; i < bytes; ++i) dev[i] = (char)(rng() >> 9);
        std::atomic<unsigned> salt{(unsigned)rng()};
        const int rc = staged_drain(
            team, bytes, kChunk, members,
            [&](int64_t i, int buf, size_t len) -> int {
                if (i == fail_at) return 9;
                dma.issue(pin[buf].data(), dev.data() + (size_t)i * kChunk, len, buf);
                return 0;
            },
            [&](int buf) -> int { dma.wait(buf); return 0; },
            [&](int buf, size_t off, size_t goff, size_t len) {
                std::mt19937 local(salt.fetch_add(1) * 2246822519u);
                if (local() % 4 == 0) nap(local, 300);
                memcpy(dst.data() + goff, pin[buf].data() + off, len);
            });
        dma.drain_all();
        if (fail_at >= 0) {
            if (rc != 9) { fprintf(stderr, "drain: injected error came back as %d\n", rc); return 1; }
            ++errors_seen;
            continue;
        }
        if (rc != 0 || memcmp(dev.data(), dst.data(), bytes) != 0) { fprintf(stderr, "drain: %zu bytes, team %d: rc %d or data corrupted\n", bytes, members, rc); return 1; }
    }
    printf("drain ok: %d runs, %d injected errors returned\n", iters, errors_seen);
    return 0;
}

// An exchange that completes on the "device" only when every rank has posted its part -- or when the communicators are aborted.
struct FakeExchange {
    std::mutex m;
    std::condition_variable cv;
    int posted = 0, G = 1;
    bool aborted = false;
    void reset(int g) { std::lock_guard<std::mutex> lk(m); posted = 0; G = g; aborted = false; }
    void post() { { std::lock_guard<std::mutex> lk(m); ++posted; } cv.notify_all(); }
    void wait_done() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return aborted || posted >= G; }); }
    void abort() { { std::lock_guard<std::mutex> lk(m); aborted = true; } cv.notify_all(); }
};

int test_ranks(unsigned seed, int iters) {
    std::mt19937 rng(seed);
    int aborts = 0, failures = 0, skipped_without_abort = 0;
    for (int G = 1; G <= 8; ++G) {
        RankTeam team;
        FakeExchange ex[2];
        team.stuck_timeout_ms = 20;
        team.on_stuck = [&] { ex[0].abort(); ex[1].abort(); };
        team.start(G);
        for (int it = 0; it < iters; ++it) {
            const bool barriers = rng() % 2 == 0;            // copy mode (ranks share a GPU) vs RCCL mode
            const int fail_rank = (rng() % 3 == 0) ? (int)(rng() % (unsigned)G) : -1;
            const int fail_step = (int)(rng() % 6);
            // (copy mode: the "exchange" is device-to-device copies behind events, which never wait for a peer's post -- only
            //  RCCL-mode operations do)
            ex[0].reset(barriers ? 0 : G);
            ex[1].reset(barriers ? 0 : G);
            team.aborted = false;
            std::vector<std::atomic<int>> progress((size_t)G);
            for (auto& p : progress) p.store(0);
            std::vector<unsigned> salts((size_t)G);
            for (auto& s : salts) s = (unsigned)rng();
            auto body = [&](int step, int q) -> int {
                std::mt19937 local(salts[(size_t)q] + 977u * (unsigned)step);
                nap(local, 150);
                if (q == fail_rank && step == fail_step) return -2;
                progress[(size_t)q].fetch_add(1);
                return 0;
            };
            std::vector<RankStep> steps;
            steps.push_back({[&](int q) { return body(0, q); }, barriers, false, false});
            steps.push_back({[&](int q) { const int rc = body(1, q); if (rc == 0) ex[0].post(); return rc; }, barriers, false, true});
            steps.push_back({[&](int q) { const int rc = body(2, q); if (rc == 0) ex[0].wait_done(); return rc; }, barriers, true, false});     // (a stream wait inside a step)
            steps.push_back({[&](int q) { const int rc = body(3, q); if (rc == 0) ex[1].post(); return rc; }, barriers, false, true});
            steps.push_back({[&](int q) { return body(4, q); }, false, false, false});
            steps.push_back({[&](int q) { const int rc = body(5, q); if (rc == 0) ex[1].wait_done(); return rc; }, false, true, false});
            const int bad = team.run(steps);
            if (fail_rank < 0) {
                if (bad != -1) { fprintf(stderr, "ranks: G %d run %d: no failure injected, run() says rank %d\n", G, it, bad); return 1; }
                for (int q = 0; q < G; ++q) if (progress[(size_t)q].load() != 6) { fprintf(stderr, "ranks: rank %d did %d of 6 steps\n", q, progress[(size_t)q].load()); return 1; }
            } else {
                ++failures;
                if (bad != fail_rank) { fprintf(stderr, "ranks: G %d run %d: rank %d failed at step %d, run() says %d\n", G, it, fail_rank, fail_step, bad); return 1; }
                if (team.rc[(size_t)fail_rank] != -2) { fprintf(stderr, "ranks: the failing rank's code was lost\n"); return 1; }
                if (team.aborted) ++aborts; else ++skipped_without_abort;
            }
        }
        team.stop();
    }
    printf("ranks ok: %d injected failures came back (%d of them needed the abort, %d were settled by the look before the exchange)\n",
           failures, aborts, skipped_without_abort);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    const unsigned seed = argc > 2 ? (unsigned)strtoul(argv[2], nullptr, 10) : 1u;
    const int iters = argc > 3 ? atoi(argv[3]) : 100;
    // nothing here may hang: a watchdog ends the process instead
    std::thread([] { std::this_thread::sleep_for(std::chrono::seconds(300)); fprintf(stderr, "sched_harness: watchdog -- a scheduler hangs\n"); _Exit(4); }).detach();
    if (what == "team") return test_team(seed, iters);
    if (what == "upload") return test_upload<true>(seed, iters);
    if (what == "upload_prefix") return test_upload<false>(seed, iters);
    if (what == "drain") return test_drain(seed, iters);
    if (what == "ranks") return test_ranks(seed, iters);
    fprintf(stderr, "usage: sched_harness team|upload|upload_prefix|drain|ranks <seed> <iters>\n");
    return 2;
}
