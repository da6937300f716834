// sdfgpu_batch.hip -- the batched exact EDT for small grids: B grids of one shape (every axis <= 128) in two launches.
// Contract: include/sdfgpu.h "Batches of same-shape grids"; interface: sdfgpu_batch.hpp; DESIGN.md section 18.
//
//   k_batch_zy        one workgroup per group of P consecutive x-planes of the batch (P > 1 where a plane is tiny).  Loads the
//                     planes' occupancy (bytes, or tagged cell records classified in the loader), packs it to bits in LDS, does
//                     the z pass as a nearest-opposite-bit search on the row's two 64-bit words, the y pass as an exact min-plus
//                     down each column out of LDS, and stores the signed in-plane d^2 as int16.
//   k_batch_x_finish  one workgroup per (grid, tile of 128 y.z columns): the tile's nx planes into LDS, exact min-plus along x
//                     over the grid's OWN planes only, the virtual border as D <- min(D, b^2), float(sqrt(double(D)) * res_b),
//                     and the per-grid maxima of D per class merged into ext[b] with one atomicMax per class and workgroup.
//
// Both min-plus passes walk outwards from the voxel and stop as soon as d^2 >= the best value so far: exact for every scene,
// two or three steps on dense ones, at most the line (<= 128) on empty ones.
#define SDFGPU_AUX_TU
#include "sdfgpu_kernels.hpp"
#include "sdfgpu_batch.hpp"

#include <algorithm>

namespace sdfgpu {

namespace {

constexpr int kBatchBlock = 256;
constexpr int kNone16 = 0x7FFF;        // LDS / scratch magnitude of "no opposite voxel in this row / plane"
// One dimension of a HIP launch takes fewer than 2^32 threads (a larger one is not refused: its size wraps and most workgroups
// never run), so more than kBatchGridX workgroups go over two grid dimensions and a workgroup's number is y * gridDim.x + x.
constexpr int64_t kBatchGridX = (int64_t)1 << 22;

dim3 batch_grid(int64_t workgroups) {
    if (workgroups <= kBatchGridX) return dim3((unsigned)workgroups);
    return dim3((unsigned)kBatchGridX, (unsigned)((workgroups + kBatchGridX - 1) / kBatchGridX));
}

__device__ __forceinline__ int64_t batch_workgroup() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__device__ __forceinline__ int mag16(int v) { return v >= kNone16 ? kInf32 : v; }

template <bool TAGGED>
__global__ __launch_bounds__(kBatchBlock) void k_batch_zy(const BatchArgs a, const int P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int nz = a.nz, ny = a.ny, plane = ny * nz;
    const int64_t planes_total = (int64_t)a.batch * a.nx;
    const int64_t wg = batch_workgroup();
    const int64_t gp0 = wg * P;
    if (gp0 >= planes_total) return;                                          // (the last row of a two-dimensional launch)
    const int np = (int)min((int64_t)P, planes_total - gp0);
    const int nvox = np * plane, rows = np * ny;
    uint32_t* bm = reinterpret_cast<uint32_t*>(smem);                         // [P * ny][4] row bitmaps (nz <= 128)
    uint16_t* g = reinterpret_cast<uint16_t*>(smem + (size_t)P * ny * 16);    // [P * plane] bit 15 = class, bits 0..14 = dz^2

    if (wg == 0)                     // the x pass's per-grid maxima start at 0
        for (int i = t; i < 2 * a.batch; i += kBatchBlock) a.ext[i] = 0u;
    for (int i = t; i < rows * 4; i += kBatchBlock) bm[i] = 0u;
    __syncthreads();

    // load + pack: a wave's ballot holds 64 consecutive voxels; the lane at the start of each 32-bit bitmap word (or of the wave)
    // ORs the piece of the ballot that belongs to that word
    for (int v0 = 0; v0 < nvox; v0 += kBatchBlock) {
        const int v = v0 + t;
        const bool in = v < nvox;
        bool f = false;
        int row = 0, z = 0;
        if (in) {
            row = v / nz; z = v - row * nz;
            const int p = v / plane, r = v - p * plane;
            const int64_t gp = gp0 + p;
            if constexpr (TAGGED) {
                const int64_t b = gp / a.nx, x = gp - b * a.nx;
                const char* c = a.cells + (x * plane + r) * a.stride;
                const float occ = *reinterpret_cast<const float*>(c + a.occ_off);
                const uint32_t obj = *reinterpret_cast<const uint32_t*>(c + a.obj_off);
                f = ((occ > 0.5f) || (a.unknown_is_filled && (occ == 0.5f))) && obj == a.ids[b];
            } else {
                f = a.mask[gp * plane + r] != 0;
            }
        }
        const uint64_t w = __ballot(f);
        if (in && ((z & 31) == 0 || lane == 0)) {
            const int cnt = min(32 - (z & 31), min(nz - z, 64 - lane));
            const uint32_t bits = (uint32_t)(w >> lane) & (cnt >= 32 ? ~0u : ((1u << cnt) - 1u));
            if (bits) atomicOr(&bm[row * 4 + (z >> 5)], bits << (z & 31));
        }
    }
    __syncthreads();

    // z pass: nearest voxel of the other class in the row, by clz / ffs on the row's two words
    const uint64_t vlo = nz >= 64 ? ~0ull : ((1ull << nz) - 1ull);
    const uint64_t vhi = nz <= 64 ? 0ull : (nz >= 128 ? ~0ull : ((1ull << (nz - 64)) - 1ull));
    for (int v = t; v < nvox; v += kBatchBlock) {
        const int row = v / nz, z = v - row * nz;
        const uint64_t lo = (uint64_t)bm[row * 4] | ((uint64_t)bm[row * 4 + 1] << 32);
        const uint64_t hi = (uint64_t)bm[row * 4 + 2] | ((uint64_t)bm[row * 4 + 3] << 32);
        const bool cls = (((z < 64) ? lo : hi) >> (z & 63)) & 1ull;
        const uint64_t olo = (cls ? ~lo : lo) & vlo, ohi = (cls ? ~hi : hi) & vhi;
        int d = kFar;
        if (z < 64) {
            const uint64_t l = olo & ((1ull << z) - 1ull);
            if (l) d = z - (63 - __clzll((long long)l));
            const uint64_t r = (olo >> z) >> 1;
            if (r) d = min(d, (int)__ffsll((unsigned long long)r));
            else if (ohi) d = min(d, 64 + (int)__ffsll((unsigned long long)ohi) - 1 - z);
        } else {
            const int zz = z - 64;
            const uint64_t l = ohi & ((1ull << zz) - 1ull);
            if (l) d = zz - (63 - __clzll((long long)l));
            else if (olo) d = z - (63 - __clzll((long long)olo));
            const uint64_t r = (ohi >> zz) >> 1;
            if (r) d = min(d, (int)__ffsll((unsigned long long)r));
        }
        g[v] = (uint16_t)((cls ? 0x8000 : 0) | (d >= kFar ? kNone16 : d * d));
    }
    __syncthreads();

    // y pass: exact min-plus down the column.  A candidate of the voxel's own class offers its dz^2, one of the other class 0.
    int16_t* dst = a.plane + gp0 * plane;
    for (int v = t; v < nvox; v += kBatchBlock) {
        const int r = v % plane, y = r / nz;
        const int me = g[v];
        int best = mag16(me & kNone16);
        for (int dy = 1; dy < ny && dy * dy < best; ++dy) {
            const int dd = dy * dy;
            if (y - dy >= 0) {
                const int c = g[v - dy * nz];
                best = min(best, (((c ^ me) & 0x8000) ? 0 : mag16(c & kNone16)) + dd);
            }
            if (y + dy < ny) {
                const int c = g[v + dy * nz];
                best = min(best, (((c ^ me) & 0x8000) ? 0 : mag16(c & kNone16)) + dd);
            }
        }
        const int s = min(best, kNone16);             // (finite values are <= 2 * 127^2 = 32258)
        dst[v] = (int16_t)((me & 0x8000) ? -s : s);
    }
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_x_finish(const BatchArgs a, const int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int part[2 * (kBatchBlock / 64)];
    constexpr int TC = kBatchTileCols;
    int16_t* col = reinterpret_cast<int16_t*>(smem);          // [nx][TC]
    const int t = threadIdx.x;
    const int nx = a.nx, ny = a.ny, nz = a.nz, plane = ny * nz;
    const int64_t wg = batch_workgroup();
    if (wg >= (int64_t)a.batch * tiles) return;
    const int b = (int)(wg / tiles), tile = (int)(wg - (int64_t)b * tiles);
    const int c0 = tile * TC, nc = min(TC, plane - c0);
    const int64_t base = (int64_t)b * nx * plane;
    const double res = a.res ? a.res[b] : a.res_uniform;

    for (int i = t; i < nx * TC; i += kBatchBlock) {
        const int x = i / TC, c = i - x * TC;
        if (c < nc) col[i] = a.plane[base + (int64_t)x * plane + c0 + c];
    }
    __syncthreads();

    int mxF = 0, mxQ = 0;
    for (int i = t; i < nx * TC; i += kBatchBlock) {
        const int x = i / TC, c = i - x * TC;
        if (c >= nc) continue;
        const int me = col[i];
        const bool neg = me < 0;
        int best = mag16(abs(me));
        for (int dx = 1; dx < nx && dx * dx < best; ++dx) {
            const int dd = dx * dx;
            if (x - dx >= 0) {
                const int u = col[i - dx * TC];
                best = min(best, (((u < 0) == neg) ? mag16(abs(u)) : 0) + dd);
            }
            if (x + dx < nx) {
                const int u = col[i + dx * TC];
                best = min(best, (((u < 0) == neg) ? mag16(abs(u)) : 0) + dd);
            }
        }
        int D = min(best, kInf32);
        const int cc = c0 + c;
        if (a.vb) {
            // net effect of sdf_generation.hpp:287-419: D = min(D, b^2), b = axis distance to the virtual layer over axes with
            // more than one cell (the single build's arithmetic, sdfgpu_kernels.hpp)
            const int y = cc / nz, z = cc - y * nz;
            int bd = kInf32;
            if (nx > 1) bd = min(bd, min(x + 1, nx - x));
            if (ny > 1) bd = min(bd, min(y + 1, ny - y));
            if (nz > 1) bd = min(bd, min(z + 1, nz - z));
            if (bd < 32768) D = min(D, bd * bd);
        }
        if (neg) mxQ = max(mxQ, D); else mxF = max(mxF, D);
        // sdf_generation.hpp:254-265: sqrt and multiply in double, one narrowing cast
        const float f = (D >= kInf32) ? __builtin_inff() : (float)(sqrt((double)D) * res);
        a.out[base + (int64_t)x * plane + cc] = neg ? -f : f;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mxF = max(mxF, __shfl_xor(mxF, off));
        mxQ = max(mxQ, __shfl_xor(mxQ, off));
    }
    if ((t & 63) == 0) { part[2 * (t >> 6)] = mxF; part[2 * (t >> 6) + 1] = mxQ; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kBatchBlock / 64; ++w) { mxF = max(mxF, part[2 * w]); mxQ = max(mxQ, part[2 * w + 1]); }
        if (mxF) atomicMax(a.ext + 2 * b, (uint32_t)mxF);
        if (mxQ) atomicMax(a.ext + 2 * b + 1, (uint32_t)mxQ);
    }
}

// sdfgpu_gradient_device's per-voxel definition (gradient_one) with grid b's scale; blockIdx.y walks the grids
template <typename OutT>
__global__ __launch_bounds__(kBatchBlock) void k_batch_gradient(const BatchGradArgs a) {
    const int64_t n = a.nx * a.ny * a.nz;
    const int64_t i = (int64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t z = i % a.nz, y = (i / a.nz) % a.ny, x = i / (a.nz * a.ny);
    for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
        GradScale sc;
        if (a.scales) sc = reinterpret_cast<const GradScale*>(a.scales)[b];
        else { sc.inv2 = a.inv2; sc.inv_w1 = a.inv_w1; sc.inv_w2 = a.inv_w2; sc.inv2f = (float)a.inv2; }
        double v[3];
        gradient_one(a.sdf + (int64_t)b * n, i, x, y, z, a.nx, a.ny, a.nz, sc, a.edge, v);
        OutT* o = reinterpret_cast<OutT*>(a.out) + ((int64_t)b * n + i) * 3;
        o[0] = (OutT)v[0];
        o[1] = (OutT)v[1];
        o[2] = (OutT)v[2];
    }
}

}  // namespace

hipError_t batch_launch(const BatchArgs& a, hipStream_t s, int* launches) {
    const int plane = a.ny * a.nz;
    const int64_t planes_total = (int64_t)a.batch * a.nx;
    // several planes per workgroup where a plane is tiny (25 x 20 x 15: 300 voxels a plane), never across more LDS than one
    // 128 x 128 plane takes
    const int P = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(1024 / plane, 8), planes_total));
    const size_t lds_zy = (size_t)P * a.ny * 16 + (size_t)P * plane * 2;
    const dim3 grid_zy = batch_grid((planes_total + P - 1) / P);
    if (a.mask)
        hipLaunchKernelGGL(k_batch_zy<false>, grid_zy, dim3(kBatchBlock), lds_zy, s, a, P);
    else
        hipLaunchKernelGGL(k_batch_zy<true>, grid_zy, dim3(kBatchBlock), lds_zy, s, a, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int tiles = (plane + kBatchTileCols - 1) / kBatchTileCols;
    const size_t lds_x = (size_t)a.nx * kBatchTileCols * 2;
    hipLaunchKernelGGL(k_batch_x_finish, batch_grid((int64_t)a.batch * tiles), dim3(kBatchBlock), lds_x, s, a, tiles);
    if (launches) *launches = 2;
    return hipGetLastError();
}

hipError_t batch_gradient_launch(const BatchGradArgs& a, hipStream_t s) {
    const int64_t n = a.nx * a.ny * a.nz;
    const dim3 grid((unsigned)((n + kBatchBlock - 1) / kBatchBlock), (unsigned)std::min(a.batch, 65535));
    if (a.f64) hipLaunchKernelGGL(k_batch_gradient<double>, grid, dim3(kBatchBlock), 0, s, a);
    else hipLaunchKernelGGL(k_batch_gradient<float>, grid, dim3(kBatchBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfgpu
