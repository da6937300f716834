// sdfgpu_convex.hip -- the local-extrema and convex-segment kernels (sdfgpu_convex.hpp) and their launchers.  Compiled beside
// sdfgpu.hip and linked into the same libsdfgpu.so (sdf_tools_amd/build.py).
// The family's host orchestration and C ABI entry points (sdfgpu_local_extrema*, sdfgpu_convex_segments_cells, sdfgpu_convex_last_info) are at the end of this file, over the handle of
// sdfgpu_context.hpp.
//
// Arithmetic: the rotated gradient and the extremum distance must round exactly as the reference's host code does (separate
// products and sums, eigen_lite order), so nothing in this file may be contracted into an FMA (hipcc contracts by default).
// The host code at the end of this file falls under the pragma too.  It is compiled for baseline x86-64, which has no FMA to
// contract into, so the pragma changes nothing there -- look again before giving the host pass a -march.
#pragma clang fp contract(off)
#define SDFGPU_AUX_TU
#include "sdfgpu_kernels.hpp"
#include "sdfgpu_context.hpp"
#include "sdfgpu_convex.hpp"
#include "sdfgpu_unionfind.hpp"
#include "sdfgpu.h"

#include <algorithm>

namespace sdfgpu {

namespace {

constexpr int kThreads = 256;
// The doubling state of an unresolved node is (p_k(v) << 32) | m_k(v), m_k(v) < n <= 2^32 - 3 (check_convex_args): an index must
// never equal one of the three markers below, or an open state would read as resolved.  A resolved node's low word is
// a marker, its high word the answer: kResTerm -> the terminal (a fixed point, or kCxOff), kResCycle -> the cycle's minimum index;
// k_cx_entry turns the marker of every cycle node into kOnCycle.
constexpr uint32_t kResTerm = 0xFFFFFFFFu;
constexpr uint32_t kResCycle = 0xFFFFFFFEu;
constexpr uint32_t kOnCycle = 0xFFFFFFFDu;

__device__ __forceinline__ uint64_t pack(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }
__device__ __forceinline__ uint32_t hi32(uint64_t s) { return (uint32_t)(s >> 32); }
__device__ __forceinline__ uint32_t lo32(uint64_t s) { return (uint32_t)s; }
__device__ __forceinline__ bool resolved(uint64_t s) { return lo32(s) >= kOnCycle; }

// One lane per voxel.  A launch of 2^32 work-items or more along one axis is refused by the runtime, and n > 2^32 - 256 takes
// 2^24 workgroups of 256, so the workgroups are numbered over a 2-D grid, x fastest: workgroup b = blockIdx.y gridDim.x +
// blockIdx.x holds indices [256 b, 256 b + 256), dispatched in the order of a 1-D grid.
constexpr unsigned kGridX = 1u << 16;
__device__ __forceinline__ uint64_t lane_index() {
    return ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * kThreads + threadIdx.x;
}

// Sum (and maxima) of a per-lane value over the workgroup; the result is valid in thread 0.  Every thread must call these.
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
    for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}
__device__ __forceinline__ void block_reduce(uint32_t count, uint32_t a, uint32_t b, uint32_t& sum, uint32_t& amax, uint32_t& bmax) {
    __shared__ uint32_t part[3][kThreads / 64];
    for (int o = 32; o > 0; o >>= 1) count += (uint32_t)__shfl_xor((int)count, o);
    a = wave_max(a);
    b = wave_max(b);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = count; part[1][wave] = a; part[2][wave] = b; }
    __syncthreads();
    sum = amax = bmax = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kThreads / 64; ++w) { sum += part[0][w]; amax = max(amax, part[1][w]); bmax = max(bmax, part[2][w]); }
}

// eigen_lite.hpp Quaterniond::operator*, term by term (no contraction: see the pragma above)
struct Q4 { double w, x, y, z; };
__device__ __forceinline__ Q4 qmul(const Q4& a, const Q4& o) {
    return Q4{a.w * o.w - a.x * o.x - a.y * o.y - a.z * o.z, a.w * o.x + a.x * o.w + a.y * o.z - a.z * o.y,
              a.w * o.y - a.x * o.z + a.y * o.w + a.z * o.x, a.w * o.z + a.x * o.y - a.y * o.x + a.z * o.w};
}

// ---- k_cx_next ----------------------------------------------------------------------------------------------------------------
// GetGradient(x, y, z, true) (gradient_one with edge gradients, then q * ((0, g) * q^-1)); the step of GetNextFromGradient on the
// sign-corrected gradient.  No axis steps exactly when the reference's GradientIsEffectiveFlat holds or a component is NaN (a NaN
// compares false both ways), and the reference then stops at v: v is a terminal.  A, B: the doubling state S_0 (markers in both).
__global__ __launch_bounds__(kThreads) void k_cx_next(const float* __restrict__ f, int64_t nx, int64_t ny, int64_t nz, uint64_t n,
                                                      const GradScale sc, double step, const CxRot rot, uint32_t* __restrict__ nxt,
                                                      uint64_t* __restrict__ A, uint64_t* __restrict__ B) {
    const uint64_t v = lane_index();
    if (v >= n) return;
    const int64_t z = (int64_t)(v % (uint64_t)nz), r = (int64_t)(v / (uint64_t)nz), y = r % ny, x = r / ny;
    double g[3];
    gradient_one(f, (int64_t)v, x, y, z, nx, ny, nz, sc, 1, g);
    const Q4 q{rot.q[0], rot.q[1], rot.q[2], rot.q[3]}, qi{rot.qi[0], rot.qi[1], rot.qi[2], rot.qi[3]};
    const Q4 w4 = qmul(q, qmul(Q4{0.0, g[0], g[1], g[2]}, qi));
    double w[3] = {w4.x, w4.y, w4.z};
    if (f[v] < 0.0f) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; }    // (gradient * -1.0: the same value, NaN stays NaN)
    int d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = w[k] > step ? 1 : (w[k] < -step ? -1 : 0);
    uint64_t s;
    uint32_t to;
    if (d[0] == 0 && d[1] == 0 && d[2] == 0) {
        to = (uint32_t)v;
        s = pack((uint32_t)v, kResTerm);
    } else {
        const int64_t X = x + d[0], Y = y + d[1], Z = z + d[2];
        if (X < 0 || Y < 0 || Z < 0 || X >= nx || Y >= ny || Z >= nz) {
            to = kCxOff;
            s = pack(kCxOff, kResTerm);
        } else {
            to = (uint32_t)((X * ny + Y) * nz + Z);
            s = pack(to, (uint32_t)v);                  // p_0 = next(v), window {v}
        }
    }
    nxt[v] = to;
    A[v] = s;
    if (resolved(s)) B[v] = s;
}

// ---- k_cx_round ---------------------------------------------------------------------------------------------------------------
// Round k reads S_k from `in` and writes S_{k+1} to `out`.  For an unresolved v with p = p_k(v):
//   p == kCxOff, or S_k(p) resolved                    -> v takes that answer (p is on v's orbit);
//   c = m_k(p) (on v's orbit), d = next(c): d == kCxOff or S_k(d) resolved -> that answer;
//   m_k(d) == c                                        -> v's orbit ends in the cycle whose minimum is c (DESIGN section 15:
//                                                         m_k(next(c)) == c iff c lies on a cycle of length <= 2^k and is its
//                                                         minimum);
//   else S_{k+1}(v) = (p_k(p), min(m_k(v), c)).
// A node that resolves writes its marker into `out` AND `in`: a reader of `in` in this launch then sees either S_k or the marker,
// and both are correct for it (the marker is an answer for every node whose orbit passes v).  After that it writes nothing.
// The nodes left open are counted per workgroup into one of the spread slots of round k.
__global__ __launch_bounds__(kThreads) void k_cx_round(uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                       const uint32_t* __restrict__ nxt, uint64_t n, CxStats* __restrict__ st, int k) {
    const uint64_t v = lane_index();
    bool open = false;
    if (v < n) {
        const uint64_t s = in[v];
        if (!resolved(s)) {
            const uint32_t p = hi32(s);
            uint64_t r = pack(kCxOff, kResTerm);
            bool done = true;
            if (p != kCxOff) {
                const uint64_t sp = in[p];
                if (resolved(sp)) {
                    r = sp;
                } else {
                    const uint32_t c = lo32(sp), d = nxt[c];
                    if (d != kCxOff) {
                        const uint64_t sd = in[d];
                        if (resolved(sd)) r = sd;
                        else if (lo32(sd) == c) r = pack(c, kResCycle);
                        else { done = false; out[v] = pack(hi32(sp), min(lo32(s), c)); }
                    }
                }
            }
            if (done) {
                out[v] = r;
                __hip_atomic_store(&in[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            open = !done;
        }
    }
    uint32_t total, unused0, unused1;
    block_reduce(open ? 1u : 0u, 0u, 0u, total, unused0, unused1);
    if (threadIdx.x == 0 && total) atomicAdd(&st->open[k][(blockIdx.x % kCxSpread) * kCxLine], total);
}

// ---- k_cx_basin: slot[c] = min index of the voxels whose orbit ends in the cycle c ---------------------------------------------
// A basin is usually one cycle for a whole wave (a room's free space drains into a handful): one atomic per wave then.
__global__ __launch_bounds__(kThreads) void k_cx_basin(const uint64_t* __restrict__ A, uint64_t n, uint32_t* __restrict__ slot) {
    const uint64_t v = lane_index();
    uint32_t c = kCxOff;
    if (v < n) {
        const uint64_t s = A[v];
        if (lo32(s) == kResCycle) c = hi32(s);
    }
    const bool mine = c != kCxOff;
    const uint64_t m = __ballot(mine);
    if (!m) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    const uint32_t c0 = __shfl(c, lead);
    // A slot only decreases: a plain load that already shows an index <= v (stale or not) makes the atomic useless.  Workgroups
    // start roughly in index order, so after a basin's first wave nearly every other one skips it.
    if (__all(!mine || c == c0)) {
        if ((int)(threadIdx.x & 63) == lead && slot[c0] > (uint32_t)v) atomicMin(&slot[c0], (uint32_t)v);   // (lowest lane, lowest index)
    } else if (mine && slot[c] > (uint32_t)v) {
        atomicMin(&slot[c], (uint32_t)v);
    }
}

// ---- k_cx_entry: one lane per cycle (its minimum c) ---------------------------------------------------------------------------
// Marks the cycle's nodes (kOnCycle), then walks next from the basin minimum b = slot[c] to the first marked node: the node at
// which the reference's walk from b, the first walk of the basin in scan order, closes its path.  slot[c] = that node.  Each
// lane touches only its own basin's nodes; all walks together are at most n steps.
__global__ __launch_bounds__(kThreads) void k_cx_entry(uint64_t* __restrict__ A, const uint32_t* __restrict__ nxt, uint64_t n,
                                                       uint32_t* __restrict__ slot, CxStats* __restrict__ st) {
    const uint64_t v = lane_index();
    uint32_t len = 0, steps = 0;
    if (v < n) {
        const uint64_t s = A[v];
        if (lo32(s) == kResCycle && hi32(s) == (uint32_t)v) {
            uint32_t u = (uint32_t)v;
            do {
                A[u] = pack((uint32_t)v, kOnCycle);
                u = nxt[u];
                ++len;
            } while (u != (uint32_t)v);
            uint32_t w = slot[v];
            while (lo32(A[w]) != kOnCycle) { w = nxt[w]; ++steps; }
            slot[v] = w;
        }
    }
    uint32_t cycles, longest, entry;
    block_reduce(len ? 1u : 0u, len, steps, cycles, longest, entry);
    if (threadIdx.x == 0 && cycles) {
        atomicAdd(&st->cycles[(blockIdx.x % kCxSpread) * kCxLine], cycles);
        if (longest > st->longest_cycle[0]) atomicMax(&st->longest_cycle[0], longest);
        if (entry > st->longest_entry[0]) atomicMax(&st->longest_entry[0], entry);
    }
}

__global__ __launch_bounds__(kThreads) void k_cx_final(const uint64_t* __restrict__ A, const uint32_t* __restrict__ slot, uint64_t n,
                                                       uint32_t* __restrict__ ext) {
    const uint64_t v = lane_index();
    if (v >= n) return;
    const uint64_t s = A[v];
    ext[v] = lo32(s) == kResTerm ? hi32(s) : slot[hi32(s)];
}

// ---- segments -----------------------------------------------------------------------------------------------------------------
// key = (object id << 32) | extremum, the extremum kCxOff for a cell that takes no part: (occupancy < 0.5f || object id > 0) fails
// (NaN occupancy with object 0 included), or its walk leaves the grid.
__global__ __launch_bounds__(kThreads) void k_cx_key(const uint32_t* __restrict__ ext, const char* __restrict__ cells, uint64_t stride,
                                                     uint64_t occ_off, uint64_t obj_off, uint64_t n, uint64_t* __restrict__ key) {
    const uint64_t v = lane_index();
    if (v >= n) return;
    const char* rec = cells + v * stride;
    const float occ = *reinterpret_cast<const float*>(rec + occ_off);
    const uint32_t obj = *reinterpret_cast<const uint32_t*>(rec + obj_off);
    const uint32_t e = ext[v];
    key[v] = pack(obj, (occ < 0.5f || obj > 0u) ? e : kCxOff);
}

struct SegGeom {
    int64_t ny, nz;
    double res, thr;
};

// the reference's are_connected_fn on two taking-part cells: same object id, (e1 - e2).norm() < threshold with eigen_lite's
// VecNd::norm (0 + dx dx + dy dy + dz dz, correctly rounded sqrt)
__device__ __forceinline__ bool joined(uint64_t ka, uint64_t kb, const SegGeom& g) {
    const uint32_t ea = lo32(ka), eb = lo32(kb);
    if (ea == kCxOff || eb == kCxOff || hi32(ka) != hi32(kb)) return false;
    if (ea == eb) return 0.0 < g.thr;
    const uint64_t pa = ea / (uint64_t)g.nz, pb = eb / (uint64_t)g.nz;
    const double za = g.res * ((double)(ea - pa * (uint64_t)g.nz) + 0.5), zb = g.res * ((double)(eb - pb * (uint64_t)g.nz) + 0.5);
    const uint64_t xa = pa / (uint64_t)g.ny, xb = pb / (uint64_t)g.ny;
    const double ya = g.res * ((double)(pa - xa * (uint64_t)g.ny) + 0.5), yb = g.res * ((double)(pb - xb * (uint64_t)g.ny) + 0.5);
    const double dx = g.res * ((double)xa + 0.5) - g.res * ((double)xb + 0.5), dy = ya - yb, dz = za - zb;
    double s = 0.0;
    s += dx * dx;
    s += dy * dy;
    s += dz * dz;
    return __dsqrt_rn(s) < g.thr;
}

// The union-find over the label words is sdfgpu_unionfind.hpp's (a root's word is its own index): a segment's root is its minimum
// index -- the cell at which the reference's scan starts it.
// L[v] = the first voxel of v's run of joined z neighbours inside v's wave (64 consecutive indices): chains of depth <= 1
__global__ __launch_bounds__(kThreads) void k_cx_uf_init(const uint64_t* __restrict__ key, uint64_t n, const SegGeom g,
                                                         uint32_t* __restrict__ L) {
    const uint64_t v = lane_index();
    const int lane = threadIdx.x & 63;
    bool j = false;
    if (v < n && v % (uint64_t)g.nz != 0) j = joined(key[v], key[v - 1], g);
    const uint64_t m = __ballot(j);
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const uint64_t starts = ~m & upto;                  // lanes <= this one that are not joined to their predecessor
    const int s = starts ? 63 - __clzll((long long)starts) : 0;
    if (v < n) L[v] = (uint32_t)(v - (uint64_t)(lane - s));
}

// The remaining pairs: z across wave boundaries; y and x unless the square through the z predecessors already joins them
__global__ __launch_bounds__(kThreads) void k_cx_uf_link(const uint64_t* __restrict__ key, uint64_t n, const SegGeom g,
                                                         uint32_t* __restrict__ L) {
    const uint64_t v = lane_index();
    if (v >= n) return;
    const uint64_t kv = key[v];
    if (lo32(kv) == kCxOff) return;
    const uint64_t nz = (uint64_t)g.nz, plane = (uint64_t)g.ny * nz;
    const uint64_t z = v % nz, y = (v / nz) % (uint64_t)g.ny;
    const bool zj = z > 0 && joined(kv, key[v - 1], g);
    if (zj && (v & 63) == 0) uf_union<RootIsSelf>(L, (uint32_t)v, (uint32_t)(v - 1));
    if (y > 0) {
        const uint64_t u = v - nz;
        const uint64_t ku = key[u];
        if (joined(kv, ku, g)) {
            const bool square = zj && joined(ku, key[u - 1], g) && joined(key[v - 1], key[u - 1], g);
            if (!square) uf_union<RootIsSelf>(L, (uint32_t)v, (uint32_t)u);
        }
    }
    if (v >= plane) {
        const uint64_t u = v - plane;
        const uint64_t ku = key[u];
        if (joined(kv, ku, g)) {
            const bool square = zj && joined(ku, key[u - 1], g) && joined(key[v - 1], key[u - 1], g);
            if (!square) uf_union<RootIsSelf>(L, (uint32_t)v, (uint32_t)u);
        }
    }
}

// The root ranking of sdfgpu_unionfind.hpp, with root = a taking-part voxel that is its own label; 0 for cells that take no part.
__global__ __launch_bounds__(256) void k_cx_flatten(uint32_t* __restrict__ L, const uint64_t* __restrict__ key, uint64_t n,
                                                    uint32_t* __restrict__ rb, uint32_t* __restrict__ wr, uint32_t* __restrict__ cc) {
    rank_flatten(L, n, RankTables{rb, wr, cc, nullptr}, [key](uint64_t v) { return lo32(key[v]) != kCxOff; });
}

__global__ __launch_bounds__(kRankScanThreads) void k_cx_scan(const uint32_t* __restrict__ cc, uint32_t* __restrict__ co,
                                                              uint64_t chunks, uint32_t* __restrict__ count) {
    rank_scan(cc, co, chunks, count);
}

__global__ __launch_bounds__(256) void k_cx_relabel(uint32_t* __restrict__ L, const uint64_t* __restrict__ key, uint64_t n,
                                                    const uint32_t* __restrict__ rb, const uint32_t* __restrict__ wr,
                                                    const uint32_t* __restrict__ co) {
    const uint64_t v = lane_index();
    if (v >= n) return;
    if (lo32(key[v]) == kCxOff) { L[v] = 0u; return; }
    L[v] = rank_of(L[v], rb, wr, co);
}

__global__ __launch_bounds__(kThreads) void k_cx_combine(float* __restrict__ fr, const float* __restrict__ nm, uint64_t n) {
    const uint64_t v = lane_index();
    if (v >= n) return;
    const float a = fr[v], b = nm[v];
    fr[v] = a >= 0.0f ? a : (b <= -0.0f ? b : 0.0f);
}

dim3 lanes(uint64_t n) {
    const uint64_t b = (n + kThreads - 1) / kThreads;
    return b <= kGridX ? dim3((unsigned)b) : dim3(kGridX, (unsigned)((b + kGridX - 1) / kGridX));
}

}  // namespace

CxPlan cx_plan(int64_t nx, int64_t ny, int64_t nz) {
    CxPlan p;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    p.chunks = rank_chunks(p.n);
    p.off_b = p.n * 8;
    p.off_next = 2 * p.n * 8;
    p.off_stats = (p.off_next + p.n * 4 + 7) & ~(size_t)7;
    p.off_ranks = p.off_stats + ((sizeof(CxStats) + 7) & ~(size_t)7);
    p.scratch_bytes = p.off_ranks + rank_tables_bytes(p.chunks);
    return p;
}

hipError_t cx_extrema(const CxPlan& p, const float* d_sdf, double res, const CxRot& rot, uint32_t* d_ext, void* d_scratch,
                      hipStream_t s, int* rounds) {
    char* base = static_cast<char*>(d_scratch);
    uint64_t* A = reinterpret_cast<uint64_t*>(base);
    uint64_t* B = reinterpret_cast<uint64_t*>(base + p.off_b);
    uint32_t* nxt = reinterpret_cast<uint32_t*>(base + p.off_next);
    CxStats* st = reinterpret_cast<CxStats*>(base + p.off_stats);
    hipError_t e = hipMemsetAsync(st, 0, sizeof(CxStats), s);
    if (e != hipSuccess) return e;
    // the reference's reciprocals and step, with its own double operations (sdf.hpp:447, :464-512; sdf.cpp:131, :150)
    GradScale sc{};
    sc.inv2 = 1.0 / (2.0 * res);
    sc.inv_w1 = 1.0 / ((double)1 * res);
    sc.inv_w2 = 1.0 / ((double)2 * res);
    sc.inv2f = (float)sc.inv2;
    const double step = res * 0.06125;
    const dim3 nb = lanes(p.n);
    hipLaunchKernelGGL(k_cx_next, nb, dim3(kThreads), 0, s, d_sdf, p.nx, p.ny, p.nz, p.n, sc, step, rot, nxt, A, B);
    // doubling: one launch per round; the host reads the round's count of open nodes
    int used = 0;
    for (int k = 0;; ++k) {
        if (k >= kCxMaxRounds) return hipErrorUnknown;           // (unreachable: ceil(log2 n) + 1 rounds resolve every node)
        uint64_t* in = (k & 1) ? B : A;
        uint64_t* out = (k & 1) ? A : B;
        hipLaunchKernelGGL(k_cx_round, nb, dim3(kThreads), 0, s, in, out, (const uint32_t*)nxt, p.n, st, k);
        static thread_local uint32_t row[kCxSpread * kCxLine];
        if ((e = hipMemcpyAsync(row, st->open[k], sizeof row, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if (cx_row_sum(row) == 0) { used = k + 1; break; }
    }
    if (rounds) *rounds = used;
    // every resolved node holds its marker in A and in B: B's words become the per-cycle slots
    uint32_t* slot = reinterpret_cast<uint32_t*>(B);
    if ((e = hipMemsetAsync(slot, 0xFF, p.n * 4, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_cx_basin, nb, dim3(kThreads), 0, s, (const uint64_t*)A, p.n, slot);
    hipLaunchKernelGGL(k_cx_entry, nb, dim3(kThreads), 0, s, A, (const uint32_t*)nxt, p.n, slot, st);
    hipLaunchKernelGGL(k_cx_final, nb, dim3(kThreads), 0, s, (const uint64_t*)A, (const uint32_t*)slot, p.n, d_ext);
    return hipGetLastError();
}

hipError_t cx_segments(const CxPlan& p, const uint32_t* d_ext, const char* d_cells, size_t stride, size_t occ_off, size_t obj_off,
                       double res, double threshold, uint32_t* d_labels, void* d_scratch, hipStream_t s) {
    char* base = static_cast<char*>(d_scratch);
    uint64_t* key = reinterpret_cast<uint64_t*>(base);
    CxStats* st = reinterpret_cast<CxStats*>(base + p.off_stats);
    const RankTables t = rank_tables_at(base + p.off_ranks, p.chunks);
    const dim3 nb = lanes(p.n);
    SegGeom g{p.ny, p.nz, res, threshold};
    hipLaunchKernelGGL(k_cx_key, nb, dim3(kThreads), 0, s, d_ext, d_cells, (uint64_t)stride, (uint64_t)occ_off, (uint64_t)obj_off,
                       p.n, key);
    hipLaunchKernelGGL(k_cx_uf_init, nb, dim3(kThreads), 0, s, (const uint64_t*)key, p.n, g, d_labels);
    hipLaunchKernelGGL(k_cx_uf_link, nb, dim3(kThreads), 0, s, (const uint64_t*)key, p.n, g, d_labels);
    hipLaunchKernelGGL(k_cx_flatten, dim3((unsigned)p.chunks), dim3(256), 0, s, d_labels, (const uint64_t*)key, p.n, t.rb, t.wr, t.cc);
    hipLaunchKernelGGL(k_cx_scan, dim3(1), dim3(kRankScanThreads), 0, s, (const uint32_t*)t.cc, t.co, p.chunks, st->count);
    hipLaunchKernelGGL(k_cx_relabel, nb, dim3(256), 0, s, d_labels, (const uint64_t*)key, p.n, (const uint32_t*)t.rb,
                       (const uint32_t*)t.wr, (const uint32_t*)t.co);
    return hipGetLastError();
}

hipError_t cx_combine(float* free_sdf, const float* named_sdf, uint64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_cx_combine, lanes(n), dim3(kThreads), 0, s, free_sdf, named_sdf, n);
    return hipGetLastError();
}

}  // namespace sdfgpu

// ---- host side: argument checks, orchestration and the C ABI entry points -----------------------------------------------------------
using namespace sdfgpu;

namespace {

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

}  // namespace

extern "C" {

int sdfgpu_local_extrema_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                const double q_and_qinv[8], uint32_t* d_extremum, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
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
        if (int rc = stage_input(h, (size_t)n * cell_stride)) return rc;
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

}  // extern "C"
