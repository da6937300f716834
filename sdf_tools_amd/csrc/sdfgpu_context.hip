// sdfgpu_context.hip -- the handle (sdfgpu_context.hpp): errors, the allocator and its red zones, the shared argument checks, the
// staged host transfers and the host-side bit packers, and the C ABI entry points that are about the handle and not about a build.
// Compiled beside sdfgpu.hip and linked into the same libsdfgpu.so (sdf_tools_amd/build.py).  Its one kernel is the red-zone
// check; sdfgpu_kernels.hpp comes in for its constants only (kSlots, kSlotWords, kInf32).
#define SDFGPU_AUX_TU
#include "sdfgpu_kernels.hpp"
#include "sdfgpu_context.hpp"

#include <sys/mman.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

using namespace sdfgpu;

namespace {

constexpr int64_t kMaxDim = 16384;

thread_local std::string g_create_error = "";

constexpr size_t kRzPad = 4096;
constexpr int kRzByte = 0xC5;

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

}  // namespace

namespace sdfgpu {

int fail(sdfgpu_handle h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->error = buf; else g_create_error = buf;
    return code;
}

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

int ensure(sdfgpu_handle h, DeviceBuffer& b, size_t bytes, const char* name) {
    if (b.bytes >= bytes && b.ptr) return SDFGPU_OK;
    if (b.ptr) { if (int rc = rz_free(h, b.ptr)) return rc; b.ptr = nullptr; b.bytes = 0; }
    // (red zones: the buffer is exactly as large as asked for, so that the first byte behind it is canary)
    const size_t want = h->redzone ? std::max<size_t>(bytes, 4) : std::max<size_t>(bytes, 256);
    if (int rc = rz_malloc(h, name, want, &b.ptr)) return rc;
    b.bytes = want;
    return SDFGPU_OK;
}

int stage_input(sdfgpu_handle h, size_t bytes) {
    h->tag_cached_bytes = 0;
    return ensure(h, h->stage_in, bytes, "input staging");
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

// Grids whose voxels a uint32 numbers (labels, display indices): `tail` says what cannot number a larger one.
int check_dims_u32(sdfgpu_handle h, int64_t nx, int64_t ny, int64_t nz, const char* tail) {
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "grid dimensions must be positive (got %lld x %lld x %lld)",
                    (long long)nx, (long long)ny, (long long)nz);
    if ((unsigned __int128)nx * (unsigned __int128)ny * (unsigned __int128)nz > (unsigned __int128)0xFFFFFFFFu)
        return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "grid %lld x %lld x %lld has more than 2^32 - 1 voxels: %s",
                    (long long)nx, (long long)ny, (long long)nz, tail);
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

int copy_to_host(sdfgpu_handle h, void* dst, const void* d_src, size_t bytes, hipStream_t st) {
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

int copy_from_host(sdfgpu_handle h, void* d_dst, const void* src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return SDFGPU_OK;
    if (bytes < kPinMin) {
        HIP_TRY(h, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return SDFGPU_OK;
    }
    return staged_upload_hip(h, d_dst, bytes, st, 16, [src](char* dst, size_t o, size_t len) { memcpy(dst, static_cast<const char*>(src) + o, len); });
}

// Host cells / mask -> bits (team) -> h->stage_bits, enqueued on `st`; the host buffer has been consumed when this returns.  The
// bits are the caller's input (the host-buffer builds, the analysis calls), or what sdfgpu_upload_classified spreads into a byte mask.
int upload_packed(sdfgpu_handle h, const Occupancy& occ, int64_t n, hipStream_t st) {
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
    return SDFGPU_OK;
}

// the caller's host bit field (ceil(n / 32) words) -> h->stage_bits
int upload_bits(sdfgpu_handle h, const uint32_t* bits, int64_t n, hipStream_t st) {
    const size_t bytes = (((size_t)n + 31) / 32) * 4;
    if (int rc = ensure(h, h->stage_bits, bytes, "bit staging")) return rc;
    return copy_from_host(h, h->stage_bits.ptr, bits, bytes, st);
}

// The cell records of the two tagged entry points in stage_in: uploaded, or (cells == nullptr) those the previous tagged call on
// this handle left on the device.
int stage_tagged_records(sdfgpu_handle h, const void* cells, size_t bytes) {
    if (!cells) {
        if (h->tag_cached_bytes == 0 || h->tag_cached_bytes != bytes)
            return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "cells is null and the handle holds no cell records of this size");
        return SDFGPU_OK;
    }
    if (int rc = stage_input(h, bytes)) return rc;
    if (int rc = copy_from_host(h, h->stage_in.ptr, cells, bytes)) return rc;
    h->tag_cached_bytes = bytes;
    return SDFGPU_OK;
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
            if (int rc = upload_packed(h, occ, n, kNullStream)) return rc;
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

}  // namespace sdfgpu

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
    for (StreamOrder* o : {&h->build_order, &h->cx_order, &h->rs_order, &h->sc_order, &h->mr_order, &h->cs_order}) o->destroy();
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

int sdfgpu_copy_to_host(sdfgpu_handle h, void* dst, const void* d_src, size_t bytes, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (bytes > 0 && (!dst || !d_src)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        HIP_TRY(h, hipSetDevice(h->device));
        return copy_to_host(h, dst, d_src, bytes, (hipStream_t)stream);
    });
}

int sdfgpu_copy_from_host(sdfgpu_handle h, void* d_dst, const void* src, size_t bytes, void* stream) {
    return rz_wrap(h, stream, [&]() -> int {
        if (bytes > 0 && (!d_dst || !src)) return fail(h, SDFGPU_ERR_INVALID_ARGUMENT, "null pointer");
        HIP_TRY(h, hipSetDevice(h->device));
        return copy_from_host(h, d_dst, src, bytes, (hipStream_t)stream);
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

int sdfgpu_redzone_check(sdfgpu_handle h, void* stream) {
    if (!h) return SDFGPU_ERR_INVALID_ARGUMENT;
    return redzone_check(h, (hipStream_t)stream);
}

}  // extern "C"
