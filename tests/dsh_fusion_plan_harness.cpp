// dsh_fusion_plan_harness.cpp -- the host arithmetic of a fused frame of sensor rays (sdf_tools_amd/csrc/sdfgpu_dsh.hpp: dsh_fuse_update,
// dsh_fuse_model_ok, dsh_mark_bytes, dsh_mark_offset) driven on the CPU.  It prints
//   u <prior bits> <m bits> <clamp_min bits> <clamp_max bits> <result bits>      one update, all as hexadecimal float32 bit patterns
//   model <four bit patterns> <0 | 1>                                            what the model check says
//   marks <pool chunks> <cells per chunk> <bytes> <offset of the last cell>      the mark plane's 64-bit sizes
// for tests/test_dsh_fusion_cpu.py to compare with numpy bit for bit, then "dsh fusion plan OK".  The test builds it with
// -ffp-contract=off -fsanitize=address,undefined.
#include "../sdf_tools_amd/csrc/sdfgpu_dsh.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace sdfgpu;

static uint32_t bits_of(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
static float float_of(uint32_t b) { float v; std::memcpy(&v, &b, 4); return v; }

int main() {
    // priors: the special values, the clamps' neighbourhood, and bit patterns from a 64-bit LCG (every exponent, NaNs and denormals among them)
    std::vector<uint32_t> priors = {0x00000000u, 0x80000000u, 0x3F800000u, 0xBF800000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x7FC00001u, 0xFFC12345u, 0x7F800001u,
                                    0x00000001u, 0x807FFFFFu, 0x00800000u, 0x7F7FFFFFu, bits_of(0.5f), bits_of(0.12f), bits_of(0.97f), bits_of(0.7f), bits_of(0.4f),
                                    bits_of(0.001f), bits_of(0.999f), bits_of(0.0009999f), bits_of(0.9990001f), bits_of(0.1199999f), bits_of(0.9700001f)};
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 400; ++k) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        priors.push_back((uint32_t)(state >> 32));
    }
    for (int k = 0; k <= 200; ++k) priors.push_back(bits_of((float)k / 200.0f));
    const float models[][4] = {{0.7f, 0.4f, 0.12f, 0.97f},   {0.001f, 0.001f, 0.001f, 0.001f}, {0.999f, 0.999f, 0.999f, 0.999f}, {0.001f, 0.999f, 0.001f, 0.999f},
                               {0.999f, 0.001f, 0.001f, 0.999f}, {0.5f, 0.5f, 0.3f, 0.3f},     {0.9f, 0.45f, 0.2f, 0.8f},       {0.3f, 0.8f, 0.001f, 0.5f}};
    for (const auto& m : models)
        for (const uint32_t p : priors)
            for (int which = 0; which < 2; ++which) {
                const float meas = m[which], one_minus = 1.0f - meas;
                const float r = dsh_fuse_update(float_of(p), meas, one_minus, m[2], m[3]);
                std::printf("u %08x %08x %08x %08x %08x\n", p, bits_of(meas), bits_of(m[2]), bits_of(m[3]), bits_of(r));
            }
    const uint32_t nan = 0x7FC00000u;
    const uint32_t checks[][4] = {{bits_of(0.7f), bits_of(0.4f), bits_of(0.12f), bits_of(0.97f)},     {bits_of(0.001f), bits_of(0.001f), bits_of(0.001f), bits_of(0.001f)},
                                  {bits_of(0.999f), bits_of(0.999f), bits_of(0.999f), bits_of(0.999f)}, {bits_of(0.4f), bits_of(0.7f), bits_of(0.5f), bits_of(0.5f)},
                                  {bits_of(0.7f), bits_of(0.4f), bits_of(0.97f), bits_of(0.12f)},     {bits_of(0.0009999f), bits_of(0.4f), bits_of(0.12f), bits_of(0.97f)},
                                  {bits_of(0.7f), bits_of(0.9990001f), bits_of(0.12f), bits_of(0.97f)}, {bits_of(0.7f), bits_of(0.4f), 0u, bits_of(0.97f)},
                                  {bits_of(0.7f), bits_of(0.4f), bits_of(0.12f), bits_of(1.0f)},      {nan, bits_of(0.4f), bits_of(0.12f), bits_of(0.97f)},
                                  {bits_of(0.7f), nan, bits_of(0.12f), bits_of(0.97f)},               {bits_of(0.7f), bits_of(0.4f), nan, bits_of(0.97f)},
                                  {bits_of(0.7f), bits_of(0.4f), bits_of(0.12f), nan},                {bits_of(-0.7f), bits_of(0.4f), bits_of(0.12f), bits_of(0.97f)},
                                  {bits_of(0.7f), bits_of(0.4f), bits_of(0.12f), 0x7F800000u}};
    for (const auto& c : checks)
        std::printf("model %08x %08x %08x %08x %d\n", c[0], c[1], c[2], c[3], (int)dsh_fuse_model_ok(float_of(c[0]), float_of(c[1]), float_of(c[2]), float_of(c[3])));
    // the mark plane past 2^32 cells: pools of 2^17 and more chunks of 32768 cells, and small chunks in pools of 2^31
    const uint64_t pools[][2] = {{1, 1}, {64, 4096}, {65536, 32768}, {65541, 32768}, {131072, 32768}, {131073, 32768}, {(uint64_t)1 << 30, 32768}, {((uint64_t)1 << 31) - 1, 45}};
    for (const auto& p : pools)
        std::printf("marks %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p[0], p[1], dsh_mark_bytes(p[0], p[1]), dsh_mark_offset(p[0] - 1, p[1], (uint32_t)(p[1] - 1)));
    std::printf("dsh fusion plan OK\n");
    return 0;
}
