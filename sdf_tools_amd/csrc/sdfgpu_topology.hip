// sdfgpu_topology.hip -- the component-topology kernels (sdfgpu_topology.hpp) and their launchers.  Compiled beside sdfgpu.hip
// and linked into the same libsdfgpu.so (sdf_tools_amd/build.py).
// The family's host orchestration and C ABI entry points (sdfgpu_component_topology*) are at the end of this file, over the handle of
// sdfgpu_context.hpp.
//
// The union-find over the node words is sdfgpu_unionfind.hpp's, with its invariant and memory scope: a node word holds kRoot (the
// node is a root) or a node id BELOW its own, so a surface's root is its smallest node id.
#include "sdfgpu_context.hpp"
#include "sdfgpu_topology.hpp"
#include "sdfgpu_unionfind.hpp"
#include "sdfgpu.h"

#include <algorithm>

namespace sdfgpu {

namespace {

constexpr int kVertexThreads = 256;
constexpr int kTableSlots = 1024;              // k_tp_vertex's LDS table of per-label counts (open addressing)
constexpr int kTableProbes = 16;               // (a label that finds no slot goes straight to the global counters)
constexpr uint32_t kOut = 0xFFFFFFFFu;         // label of an out-of-grid voxel (a real label is <= max_label < 2^32 - 1)
constexpr uint32_t kRoot = 0xFFFFFFFFu;        // node word of a root (node ids are < 2^32 - 1)
using NodeRoot = RootIsSentinel<kRoot>;

struct TpArgs {
    const uint32_t* L;                         // labels
    const uint32_t* S;                         // selection bits or nullptr
    int64_t nx, ny, nz;
    uint64_t nv;
    uint32_t max_label;
    unsigned long long* cnt;                   // (max_label + 1) * 5
    TpStatus* st;
    uint32_t* flags;                           // per label: 1 = a selected voxel seen, 2 = an unselected one
    uint8_t* nm;                               // node byte per vertex
    uint32_t* gb;                              // per 8 vertices: node bits of the chunk before them
    uint32_t* cc;                              // per chunk: node bits
    uint32_t* co;                              // per chunk: node bits before it
    uint32_t* P;                               // union-find words, one per node
};

// slot s = 4 dx + 2 dy + dz of vertex (i, j, k) is voxel (i - 1 + dx, j - 1 + dy, k - 1 + dz); bit s of the result: in the grid
__device__ __forceinline__ uint32_t cube_in(const TpArgs& a, int64_t i, int64_t j, int64_t k) {
    const uint32_t xm = (uint32_t)(i > 0) | (uint32_t)(i < a.nx) << 1;          // dx = 0 / 1 in range
    const uint32_t ym = (uint32_t)(j > 0) | (uint32_t)(j < a.ny) << 1;
    const uint32_t zm = (uint32_t)(k > 0) | (uint32_t)(k < a.nz) << 1;
    uint32_t in = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) in |= ((xm >> (s >> 2)) & (ym >> ((s >> 1) & 1)) & (zm >> (s & 1)) & 1u) << s;
    return in;
}

// linear index of slot 0's voxel (i - 1, j - 1, k - 1), modulo 2^64 (only in-grid slots are ever dereferenced)
__device__ __forceinline__ uint64_t cube_base(const TpArgs& a, int64_t i, int64_t j, int64_t k) {
    return ((uint64_t)(i - 1) * (uint64_t)a.ny + (uint64_t)(j - 1)) * (uint64_t)a.nz + (uint64_t)(k - 1);
}

__device__ __forceinline__ uint64_t slot_offset(const TpArgs& a, int s) {
    return (uint64_t)(s >> 2) * (uint64_t)a.ny * (uint64_t)a.nz + (uint64_t)((s >> 1) & 1) * (uint64_t)a.nz + (uint64_t)(s & 1);
}

__device__ __forceinline__ void load_cube(const TpArgs& a, int64_t i, int64_t j, int64_t k, uint32_t lab[8]) {
    const uint32_t in = cube_in(a, i, j, k);
    const uint64_t b = cube_base(a, i, j, k);
#pragma unroll
    for (int s = 0; s < 8; ++s) lab[s] = ((in >> s) & 1u) ? a.L[b + slot_offset(a, s)] : kOut;
}

__device__ __forceinline__ void vertex_of(const TpArgs& a, uint64_t v, int64_t& i, int64_t& j, int64_t& k) {
    const uint64_t vz = (uint64_t)a.nz + 1, vy = (uint64_t)a.ny + 1;
    if ((v >> 32) == 0 && (vz >> 32) == 0 && (vy >> 32) == 0) {               // (32-bit divisions: the common case)
        const uint32_t v32 = (uint32_t)v, t = v32 / (uint32_t)vz, ii = t / (uint32_t)vy;
        k = (int64_t)(v32 - t * (uint32_t)vz);
        i = (int64_t)ii;
        j = (int64_t)(t - ii * (uint32_t)vy);
        return;
    }
    const uint64_t t = v / vz;
    k = (int64_t)(v - t * vz);
    i = (int64_t)(t / vy);
    j = (int64_t)(t - (uint64_t)i * vy);
}

// bit t of the result: slot t holds the label of slot s (out-of-grid slots match nothing)
__device__ __forceinline__ uint32_t same_mask(const uint32_t lab[8], int s) {
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) m |= (uint32_t)(lab[t] == lab[s]) << t;
    return lab[s] == kOut ? 0u : m;
}

// slots of m with a face neighbour (slot ^ 1, ^ 2, ^ 4) outside m
__device__ __forceinline__ uint32_t boundary_slots(uint32_t m) {
    const uint32_t s1 = ((m & 0x55u) << 1) | ((m & 0xAAu) >> 1);
    const uint32_t s2 = ((m & 0x33u) << 2) | ((m & 0xCCu) >> 2);
    const uint32_t s4 = ((m & 0x0Fu) << 4) | ((m & 0xF0u) >> 4);
    return m & ~(s1 & s2 & s4) & 0xFFu;
}

__device__ __forceinline__ bool exposed(uint32_t m, uint32_t face) {
    const uint32_t x = m & face;
    return x != 0 && x != face;
}

// the reference's edge mask: bit 0 z-, 1 z+, 2 y-, 3 y+, 4 x-, 5 x+ (topology_computation.hpp:531-608)
__device__ __forceinline__ uint32_t edge_mask(uint32_t m) {
    return (uint32_t)exposed(m, 0x55u) | (uint32_t)exposed(m, 0xAAu) << 1 | (uint32_t)exposed(m, 0x33u) << 2 |
           (uint32_t)exposed(m, 0xCCu) << 3 | (uint32_t)exposed(m, 0x0Fu) << 4 | (uint32_t)exposed(m, 0xF0u) << 5;
}

__device__ __forceinline__ uint32_t node_base(const TpArgs& a, uint64_t v) {
    const uint64_t g = v >> 3;
    const uint64_t w = reinterpret_cast<const uint64_t*>(a.nm)[g];
    const uint32_t sh = (uint32_t)(v & 7) * 8;
    return a.co[g / (kTpChunk / 8)] + a.gb[g] + (uint32_t)__popcll(w & ((1ull << sh) - 1ull));
}

// ---- k_tp_vertex ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kVertexThreads) void k_tp_vertex(const TpArgs a) {
    __shared__ uint32_t wsum[kVertexThreads / 64];
    __shared__ uint32_t tkey[kTableSlots];                  // label, or kOut for a free slot
    __shared__ uint32_t tval[kTableSlots][4];               // surface vertices, M3, M5, M6 of this workgroup (<= 8 kTpChunk each)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = threadIdx.x; t < kTableSlots; t += kVertexThreads) {
        tkey[t] = kOut;
        tval[t][0] = tval[t][1] = tval[t][2] = tval[t][3] = 0u;
    }
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t run = 0;                                       // node bits of the chunk's earlier rounds
    for (int r = 0; r < kTpChunk / kVertexThreads; ++r) {
        const uint64_t v = (uint64_t)blockIdx.x * kTpChunk + (uint64_t)r * kVertexThreads + threadIdx.x;
        uint32_t lab[8] = {kOut, kOut, kOut, kOut, kOut, kOut, kOut, kOut};
        uint32_t sel = 0, nodes = 0, m3 = 0, m5 = 0, m6 = 0;     // per slot s: bit s
        if (v < a.nv) {
            int64_t i, j, k;
            vertex_of(a, v, i, j, k);
            const uint32_t in = cube_in(a, i, j, k);
            const uint64_t base = cube_base(a, i, j, k);
#pragma unroll
            for (int s = 0; s < 8; ++s) lab[s] = ((in >> s) & 1u) ? a.L[base + slot_offset(a, s)] : kOut;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if (!((in >> s) & 1u)) continue;
                const uint64_t g = base + slot_offset(a, s);
                const uint32_t b = a.S ? (a.S[g >> 5] >> (g & 31)) & 1u : 1u;
                sel |= b << s;
                if (s == 7) {                               // each voxel is slot 7 of exactly one vertex: check it there
                    const uint32_t c = lab[7];
                    if (c > a.max_label) {                  // (max_label < kOut: an in-grid label equal to kOut lands here too)
                        atomicOr(&a.st->err, kTpErrLabel);
                        atomicMax(&a.st->label_over, c);
                    } else if (a.S) {
                        const uint32_t bit = b ? 1u : 2u;
                        if (!(a.flags[c] & bit)) {          // (a stale read only costs an extra atomic)
                            const uint32_t old = atomicOr(&a.flags[c], bit);
                            if ((old | bit) == 3u && old != 3u) {
                                atomicOr(&a.st->err, kTpErrMixed);
                                atomicMax(&a.st->label_mixed, c);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const uint32_t m = same_mask(lab, s);
                if (!m || (m & ((1u << s) - 1u))) continue;     // out of grid, or not the label's first slot
                if (!(boundary_slots(m) & sel)) continue;       // no selected voxel of the label faces another label here
                nodes |= 1u << s;
                const int e = __popc(edge_mask(m));
                m3 |= (uint32_t)(e == 3) << s;
                m5 |= (uint32_t)(e == 5) << s;
                m6 |= (uint32_t)(e == 6) << s;
            }
        }
        a.nm[v] = (uint8_t)nodes;                           // (the whole chunk is written: bytes past nv are 0)

        // per-label counts: lanes with a node at slot s that share its label add once per wave
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const bool has = (nodes >> s) & 1u;
            const uint32_t c = has ? lab[s] : 0u;
            uint64_t act = __ballot(has);
            while (act) {
                const int leader = __ffsll((long long)act) - 1;
                const uint32_t cl = __shfl(c, leader);
                const bool mine = has && c == cl;
                const uint64_t mm = __ballot(mine);
                const uint64_t b3 = __ballot(mine && ((m3 >> s) & 1u));
                const uint64_t b5 = __ballot(mine && ((m5 >> s) & 1u));
                const uint64_t b6 = __ballot(mine && ((m6 >> s) & 1u));
                if (lane == leader && cl <= a.max_label) {
                    const uint32_t add[4] = {(uint32_t)__popcll(mm), (uint32_t)__popcll(b3), (uint32_t)__popcll(b5),
                                             (uint32_t)__popcll(b6)};
                    bool placed = false;
                    for (int p = 0, h = (int)((cl * 2654435761u) >> 22); p < kTableProbes && !placed; ++p, h = (h + 1) & (kTableSlots - 1)) {
                        const uint32_t old = atomicCAS(&tkey[h], kOut, cl);
                        if (old == kOut || old == cl) {
                            for (int q = 0; q < 4; ++q)
                                if (add[q]) atomicAdd(&tval[h][q], add[q]);
                            placed = true;
                        }
                    }
                    if (!placed) {
                        unsigned long long* q = a.cnt + (uint64_t)cl * kTpCounters;
                        for (int e = 0; e < 4; ++e)
                            if (add[e]) atomicAdd(q + e, (unsigned long long)add[e]);
                    }
                }
                act &= ~mm;
            }
        }

        // chunk-relative node offsets: exclusive prefix of the node counts (0..8, four bit planes) over the block
        const uint32_t cnt = (uint32_t)__popc(nodes);
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint64_t plane = __ballot((cnt >> b) & 1u);
            pre += (uint32_t)__popcll(plane & lt) << b;
            tot += (uint32_t)__popcll(plane) << b;
        }
        if (lane == 0) wsum[wave] = tot;
        __syncthreads();
        uint32_t before = run, all = 0;
#pragma unroll
        for (int w = 0; w < kVertexThreads / 64; ++w) {
            before += w < wave ? wsum[w] : 0u;
            all += wsum[w];
        }
        if ((v & 7) == 0) a.gb[v >> 3] = before + pre;
        run += all;
        __syncthreads();                                    // (wsum is rewritten by the next round)
    }
    if (threadIdx.x == 0) a.cc[blockIdx.x] = run;
    for (int t = threadIdx.x; t < kTableSlots; t += kVertexThreads) {   // (the last round's barrier ordered every table update)
        const uint32_t c = tkey[t];
        if (c == kOut) continue;
        unsigned long long* q = a.cnt + (uint64_t)c * kTpCounters;
        for (int e = 0; e < 4; ++e)
            if (tval[t][e]) atomicAdd(q + e, (unsigned long long)tval[t][e]);
    }
}

// ---- k_tp_scan: one workgroup, exclusive scan of the chunk counts; the node total goes to the status -------------------------
// (the scan of sdfgpu_unionfind.hpp with a 64-bit sum: co is only used when the total fits in 32 bits)
__global__ __launch_bounds__(kRankScanThreads) void k_tp_scan(const uint32_t* __restrict__ cc, uint32_t* __restrict__ co,
                                                              uint64_t chunks, TpStatus* __restrict__ st) {
    rank_scan(cc, co, chunks, &st->nodes);
}

// Joins the nodes of vertex v (cube lab, node byte nmv, ids from base) with the nodes of vertex v + step along axis AX
// (slot bit 1 = z, 2 = y, 4 = x) for every node whose edge that way is exposed.
template <int AX>
__device__ __forceinline__ void link_axis(const TpArgs& a, int64_t i, int64_t j, int64_t k, uint64_t v, const uint32_t lab[8],
                                          uint32_t nmv, uint32_t base) {
    const uint32_t face = AX == 1 ? 0xAAu : AX == 2 ? 0xCCu : 0xF0u;     // the slots on the far side of v along the axis
    uint32_t want = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if ((nmv >> s) & 1u) want |= (uint32_t)exposed(same_mask(lab, s), face) << s;
    if (!want) return;
    const int64_t wi = i + (AX == 4), wj = j + (AX == 2), wk = k + (AX == 1);
    if (wi > a.nx || wj > a.ny || wk > a.nz) return;        // (an exposed edge holds an in-grid voxel: never taken)
    const uint64_t w = (uint64_t)((wi * (a.ny + 1) + wj) * (a.nz + 1) + wk);
    uint32_t nl[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (s & AX) {
            const int64_t x = wi - 1 + (s >> 2), y = wj - 1 + ((s >> 1) & 1), z = wk - 1 + (s & 1);
            const bool in = x >= 0 && y >= 0 && z >= 0 && x < a.nx && y < a.ny && z < a.nz;
            nl[s] = in ? a.L[((uint64_t)x * (uint64_t)a.ny + (uint64_t)y) * (uint64_t)a.nz + (uint64_t)z] : kOut;
        } else {
            nl[s] = lab[s | AX];
        }
    }
    const uint32_t nmw = a.nm[w];
    const uint32_t wbase = node_base(a, w);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (!((want >> s) & 1u)) continue;
        const uint32_t c = lab[s];
        int t = -1;
#pragma unroll
        for (int q = 7; q >= 0; --q)
            if (nl[q] == c) t = q;
        // the far vertex's cube shares the exposed edge's 4 voxels, so it holds c; its node exists unless a label is both selected
        // and unselected (refused before this kernel runs) -- checked anyway
        if (t < 0 || !((nmw >> t) & 1u)) continue;
        uf_union<NodeRoot>(a.P, base + (uint32_t)__popc(nmv & ((1u << s) - 1u)), wbase + (uint32_t)__popc(nmw & ((1u << t) - 1u)));
    }
}

// ---- k_tp_link ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tp_link(const TpArgs a) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.nv) return;
    const uint32_t nmv = a.nm[v];
    if (!nmv) return;
    int64_t i, j, k;
    vertex_of(a, v, i, j, k);
    uint32_t lab[8];
    load_cube(a, i, j, k, lab);
    const uint32_t base = node_base(a, v);
    link_axis<1>(a, i, j, k, v, lab, nmv, base);
    link_axis<2>(a, i, j, k, v, lab, nmv, base);
    link_axis<4>(a, i, j, k, v, lab, nmv, base);
}

// ---- k_tp_roots: after k_tp_link (stream order), a node word is kRoot iff the node is its surface's root -------------------------
__global__ __launch_bounds__(256) void k_tp_roots(const TpArgs a) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.nv) return;
    const uint32_t nmv = a.nm[v];
    if (!nmv) return;
    const uint32_t base = node_base(a, v);
    uint32_t roots = 0;
    for (uint32_t m = nmv, r = 0; m; m &= m - 1u, ++r)
        if (a.P[base + r] == kRoot) roots |= m & (0u - m);
    if (!roots) return;
    int64_t i, j, k;
    vertex_of(a, v, i, j, k);
    for (; roots; roots &= roots - 1u) {
        const int s = __ffs(roots) - 1;
        const int64_t x = i - 1 + (s >> 2), y = j - 1 + ((s >> 1) & 1), z = k - 1 + (s & 1);
        const uint32_t c = a.L[((uint64_t)x * (uint64_t)a.ny + (uint64_t)y) * (uint64_t)a.nz + (uint64_t)z];   // (a node's slot is in the grid)
        if (c <= a.max_label) atomicAdd(a.cnt + (uint64_t)c * kTpCounters + 4, 1ull);
    }
}

TpArgs make_args(const TpPlan& p, const uint32_t* d_labels, const uint32_t* d_select, void* d_scratch, uint32_t* d_nodes) {
    char* b = static_cast<char*>(d_scratch);
    TpArgs a;
    a.L = d_labels;
    a.S = d_select;
    a.nx = p.nx; a.ny = p.ny; a.nz = p.nz;
    a.nv = p.nv;
    a.max_label = p.max_label;
    a.cnt = reinterpret_cast<unsigned long long*>(b);
    a.st = reinterpret_cast<TpStatus*>(b + p.off_status);
    a.flags = reinterpret_cast<uint32_t*>(b + p.off_flags);
    a.nm = reinterpret_cast<uint8_t*>(b + p.off_nm);
    a.gb = reinterpret_cast<uint32_t*>(b + p.off_gb);
    a.cc = reinterpret_cast<uint32_t*>(b + p.off_cc);
    a.co = reinterpret_cast<uint32_t*>(b + p.off_co);
    a.P = d_nodes;
    return a;
}

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

}  // namespace

TpPlan tp_plan(int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, bool select) {
    TpPlan p;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.nv = (uint64_t)(nx + 1) * (uint64_t)(ny + 1) * (uint64_t)(nz + 1);
    p.chunks = (p.nv + kTpChunk - 1) / kTpChunk;
    p.max_label = max_label;
    p.select = select;
    const uint64_t labels = (uint64_t)max_label + 1;
    p.off_status = align8(labels * kTpCounters * 8);
    p.off_flags = p.off_status + sizeof(TpStatus);
    p.zero_bytes = align8(p.off_flags + (select ? labels * 4 : 0));
    p.off_nm = p.zero_bytes;
    p.off_gb = p.off_nm + p.chunks * kTpChunk;
    p.off_cc = p.off_gb + p.chunks * (kTpChunk / 8) * 4;
    p.off_co = p.off_cc + p.chunks * 4;
    p.scratch_bytes = p.off_co + p.chunks * 4;
    return p;
}

hipError_t tp_launch_count(const TpPlan& p, const uint32_t* d_labels, const uint32_t* d_select, void* d_scratch, hipStream_t s) {
    const TpArgs a = make_args(p, d_labels, p.select ? d_select : nullptr, d_scratch, nullptr);
    hipError_t e = hipMemsetAsync(d_scratch, 0, p.zero_bytes, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tp_vertex, dim3((unsigned)p.chunks), dim3(kVertexThreads), 0, s, a);
    hipLaunchKernelGGL(k_tp_scan, dim3(1), dim3(kRankScanThreads), 0, s, (const uint32_t*)a.cc, a.co, p.chunks, a.st);
    return hipGetLastError();
}

hipError_t tp_launch_surfaces(const TpPlan& p, const uint32_t* d_labels, void* d_scratch, uint32_t* d_nodes, uint64_t nodes, hipStream_t s) {
    if (nodes == 0) return hipSuccess;
    const TpArgs a = make_args(p, d_labels, nullptr, d_scratch, d_nodes);
    hipError_t e = hipMemsetAsync(d_nodes, 0xFF, (size_t)nodes * 4, s);     // every node starts as a root (kRoot)
    if (e != hipSuccess) return e;
    const uint64_t blocks = (p.nv + 255) / 256;
    hipLaunchKernelGGL(k_tp_link, dim3((unsigned)blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_tp_roots, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

// ---- component topology (sdfgpu_topology.hpp) ----------------------------------------------------------------------------------
// Like the components: only tp_scratch and tp_nodes (and, in the host forms, the label / bit staging and the pinned chunks) are
// used; the SDF builds' scratch, status block and policy are not touched.
int check_topology_args(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, const int64_t* out_counts) {
    if (!out_counts) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = check_dims_u32(h, nx, ny, nz, kLabelsTail)) return rc;
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

// host labels / cell records -> counters
int topology_host(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select, const void* cells, size_t stride, size_t occ_off,
                  size_t comp_off, int class_mask, int64_t nx, int64_t ny, int64_t nz, uint32_t max_label, int64_t* out_counts) {
    bool selected = false;
    if (int rc = stage_labels_selection(h, labels, select, cells, stride, occ_off, comp_off, class_mask, nx * ny * nz, &selected)) return rc;
    return topology_impl(h, (const uint32_t*)h->stage_out.ptr, selected ? (const uint32_t*)h->stage_bits.ptr : nullptr, nx, ny, nz,
                         max_label, out_counts, nullptr);
}

}  // namespace

extern "C" {

int sdfgpu_component_topology_device(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select_bits, int64_t nx, int64_t ny,
                                     int64_t nz, uint32_t max_label, int64_t* out_counts, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
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
        if (!labels) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = check_topology_args(h, nx, ny, nz, max_label, out_counts)) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        return topology_host(h, labels, select_mask, nullptr, 0, 0, 0, 7, nx, ny, nz, max_label, out_counts);
    });
}

int sdfgpu_component_topology_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                                    int64_t nx, int64_t ny, int64_t nz, int class_mask, uint32_t max_label, int64_t* out_counts) {
    return rz_wrap(h, nullptr, [&]() -> int {
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

}  // extern "C"
