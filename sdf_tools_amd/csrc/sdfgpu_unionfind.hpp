// sdfgpu_unionfind.hpp -- what the analysis families share on the device: the lock-free union-find over uint32 words in HBM, the
// root ranking that turns roots into 1..K in scan order, and the layout of the ranking's tables.  Device code: included by
// sdfgpu_components.hip, sdfgpu_convex.hip, sdfgpu_topology.hip and sdfgpu_dsh.hip and by nothing else (sdfgpu_context.hpp pulls in no kernels).
// Every __global__ kernel stays in its unit, under its own name, as a thin kernel around a body defined here.
//
// Union-find invariant, relied on by every find: a word only ever DECREASES, and a word that names a parent names an index BELOW
// its own.  A root is marked in one of two ways (the Root policies below): the word equals its own index (components, convex
// segments: a provisional label is the index of a root <= the voxel), or the word equals a sentinel above every index (topology:
// a fill with 0xFF makes every node a root).  A link stores a smaller root into a larger root's word with an atomic min, and path
// halving stores a grandparent, smaller still.  Every parent chain is therefore strictly decreasing until it meets a root, so every
// find ends, and the root of a set is its minimum index -- the element at which the reference's x -> y -> z scan starts the set.
//
// Memory scope: other workgroups, on other XCDs, link roots while this one walks.  The per-XCD L2s are not coherent with each
// other, so every read of a word is a relaxed agent-scope load (sc1: past this CU's L1 and never a stale line of this XCD's L2 for
// words another XCD's atomic wrote) and every write an agent-scope atomic.  A stale read would still be safe (it returns an older,
// larger ancestor), but nothing here depends on that.  A kernel that runs after the links in stream order (the flatten, k_tp_roots)
// sees them with plain loads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace sdfgpu {

// ---- union-find ---------------------------------------------------------------------------------------------------------------
struct RootIsSelf {                            // a root's word holds its own index
    static __device__ __forceinline__ bool is_root(uint32_t word, uint32_t index) { return word == index; }
};
template <uint32_t kSentinel>
struct RootIsSentinel {                        // a root's word holds kSentinel (above every index)
    static __device__ __forceinline__ bool is_root(uint32_t word, uint32_t) { return word == kSentinel; }
};

__device__ __forceinline__ uint32_t ld_agent(uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t min_agent(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// find with path halving: a hop whose grandparent is no root is shortened with the atomic min (monotone, stays in the set)
template <class Root>
__device__ __forceinline__ uint32_t uf_find(uint32_t* L, uint32_t a) {
    for (;;) {
        const uint32_t p = ld_agent(&L[a]);
        if (Root::is_root(p, a)) return a;
        const uint32_t gp = ld_agent(&L[p]);
        if (Root::is_root(gp, p)) return p;
        (void)min_agent(&L[a], gp);
        a = gp;
    }
}

template <class Root>
__device__ __forceinline__ void uf_union(uint32_t* L, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find<Root>(L, a);
        b = uf_find<Root>(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = min_agent(&L[a], b);     // a was a root: it now hangs under b
        if (Root::is_root(old, a)) return;
        a = old;                                      // a had been linked meanwhile (old < a): join its new root instead
    }
}

// ---- the same over LDS words of one workgroup (k_cc_local, k_dsh_cc_local): a root holds its own index ------------------------
__device__ __forceinline__ uint32_t lds_find(volatile uint32_t* l, uint32_t a) {
    uint32_t p = l[a];
    while (p != a) { a = p; p = l[a]; }
    return a;
}

__device__ __forceinline__ void lds_union(uint32_t* l, uint32_t a, uint32_t b) {
    for (;;) {
        a = lds_find(l, a);
        b = lds_find(l, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&l[a], b);    // a was a root: it now hangs under b; else retry from what a had become
        if (old == a) return;
        a = old;
    }
}

// ---- rank tables --------------------------------------------------------------------------------------------------------------
// Elements are ranked in chunks of kRankChunk, one flatten workgroup each.  rb[w]: root flags of elements 32 w .. 32 w + 31;
// wr[w]: roots in the chunk's words before w; cc[chunk]: roots in the chunk; co[chunk]: roots in the chunks before it.
constexpr int kRankChunk = 8192;               // elements per flatten workgroup: kRankWords flag words
constexpr int kRankWords = kRankChunk / 32;    // = the flatten's workgroup size (one word count per thread in its scan)
constexpr int kRankScanThreads = 1024;         // the one workgroup of the chunk-count scan

struct RankTables {                            // (a flatten kernel fills rb, wr and cc and passes co = nullptr)
    uint32_t *rb, *wr, *cc, *co;
};

inline uint64_t rank_chunks(uint64_t n) { return (n + kRankChunk - 1) / kRankChunk; }
inline size_t rank_tables_bytes(uint64_t chunks) { return (size_t)(2 * chunks * kRankWords + 2 * chunks) * 4; }
// the tables in rank_tables_bytes(chunks) bytes at p (4-byte aligned), in the order rb | wr | cc | co
inline RankTables rank_tables_at(void* p, uint64_t chunks) {
    uint32_t* rb = static_cast<uint32_t*>(p);
    uint32_t* wr = rb + chunks * kRankWords;
    uint32_t* cc = wr + chunks * kRankWords;
    return RankTables{rb, wr, cc, cc + chunks};
}

// ---- flatten: one workgroup of kRankWords threads per chunk ---------------------------------------------------------------------
// After the links (stream order: their atomics are visible).  Writes inside this launch only replace a label by its root, so any
// value a plain load sees is an ancestor of the element.  is_root(v) says whether the self-labelled element v counts as a root.
template <class IsRoot>
__device__ __forceinline__ void rank_flatten(uint32_t* __restrict__ L, uint64_t n, const RankTables& t, IsRoot is_root) {
    __shared__ uint32_t wc[kRankWords];
    const uint64_t base = (uint64_t)blockIdx.x * kRankChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = 0; j < kRankChunk / kRankWords; ++j) {
        const uint64_t v = base + (uint64_t)j * kRankWords + threadIdx.x;
        bool root = false;
        if (v < n) {
            const uint32_t r = L[v];
            if (r == (uint32_t)v) {
                root = is_root(v);
            } else {
                uint32_t q = r, p = L[q];
                while (p != q) { q = p; p = L[q]; }
                if (q != r) L[v] = q;
            }
        }
        const uint64_t m = __ballot(root);
        if (lane == 0) {
            const int w = j * 8 + 2 * wave;
            t.rb[base / 32 + w] = (uint32_t)m;
            t.rb[base / 32 + w + 1] = (uint32_t)(m >> 32);
            wc[w] = __popc((uint32_t)m);
            wc[w + 1] = __popc((uint32_t)(m >> 32));
        }
    }
    __syncthreads();
    const int i = threadIdx.x;
    const uint32_t own = wc[i];
    for (int d = 1; d < kRankWords; d <<= 1) {     // inclusive scan of the word counts
        const uint32_t add = i >= d ? wc[i - d] : 0u;
        __syncthreads();
        wc[i] += add;
        __syncthreads();
    }
    t.wr[base / 32 + i] = wc[i] - own;
    if (i == kRankWords - 1) t.cc[blockIdx.x] = wc[kRankWords - 1];
}

// ---- scan: one workgroup of kRankScanThreads, exclusive scan of the chunk counts; the total goes to *total -----------------------
// Sum is the type the counts are added in; co takes its low 32 bits (a caller with a 64-bit total uses co only when it fits).
template <typename Sum>
__device__ __forceinline__ void rank_scan(const uint32_t* __restrict__ cc, uint32_t* __restrict__ co, uint64_t chunks,
                                          Sum* __restrict__ total) {
    __shared__ Sum s[kRankScanThreads];
    const int t = threadIdx.x;
    const uint64_t per = (chunks + kRankScanThreads - 1) / kRankScanThreads;
    const uint64_t lo = std::min<uint64_t>(chunks, per * t), hi = std::min<uint64_t>(chunks, lo + per);
    Sum sum = 0;
    for (uint64_t i = lo; i < hi; ++i) sum += cc[i];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kRankScanThreads; d <<= 1) {
        const Sum add = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    Sum run = s[t] - sum;
    for (uint64_t i = lo; i < hi; ++i) { const uint32_t c = cc[i]; co[i] = (uint32_t)run; run += c; }
    if (t == kRankScanThreads - 1) *total = s[t];
}

// ---- rank: the 1-based rank of the root at index `root` among all roots, in index order -----------------------------------------
__device__ __forceinline__ uint32_t rank_of(uint32_t root, const uint32_t* __restrict__ rb, const uint32_t* __restrict__ wr,
                                            const uint32_t* __restrict__ co) {
    const uint32_t w = root >> 5;
    return co[w / kRankWords] + wr[w] + (uint32_t)__popc(rb[w] & ((1u << (root & 31)) - 1u)) + 1u;
}

}  // namespace sdfgpu
