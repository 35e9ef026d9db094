// debug_guard.h - what the operator-level debug entry points (gemm_debug.hip, attn_debug.hip, codec_debug.hip, enc_debug.hip) share: poisoned, guarded device buffers.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "common.h"

namespace {

constexpr size_t IN_GUARD = 4096;                          // trailing guard of every input, elements
constexpr uint16_t BF16_NAN = 0x7FC0, F16_NAN = 0x7E00;

// device bytes [guard | body | guard], all 0xFF until somebody writes
struct GuardedOut {
    DevBuf<uint8_t> buf;
    size_t guard = 0, body = 0;
    void alloc(size_t body_bytes, size_t guard_bytes) {
        guard = round_up(guard_bytes, 256); body = body_bytes;
        buf.alloc(2 * guard + body);
        HIP_CHECK(hipMemset(buf.p, 0xFF, 2 * guard + body));
    }
    uint8_t* p() { return buf.p + guard; }
    void check_guards() {
        std::vector<uint8_t> g(guard);
        for (int side = 0; side < 2; ++side) {
            HIP_CHECK(hipMemcpy(g.data(), side ? buf.p + guard + body : buf.p, guard, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < guard; ++i)
                MIS_REQUIRE(g[i] == 0xFF, MIS_ERR_GENERATION_FAILED, "the kernel wrote %s its output (guard byte %zu)", side ? "behind" : "before", i);
        }
    }
};

// n 16-bit elements followed by IN_GUARD elements of `nan`; src == nullptr leaves the body to a pack kernel (pre-filled with `nan` too)
void alloc16(DevBuf<uint16_t>& d, const uint16_t* src, size_t n, uint16_t nan) {
    std::vector<uint16_t> h(n + IN_GUARD, nan);
    if (src) std::copy(src, src + n, h.begin());
    d.alloc(h.size());
    HIP_CHECK(hipMemcpy(d.p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
}
void alloc_bytes(DevBuf<uint8_t>& d, const void* src, size_t n) {           // codes: 0xFF guard
    std::vector<uint8_t> h(n + IN_GUARD, 0xFF);
    if (src) memcpy(h.data(), src, n);
    d.alloc(h.size());
    HIP_CHECK(hipMemcpy(d.p, h.data(), h.size(), hipMemcpyHostToDevice));
}
// n 32-bit words followed by IN_GUARD words of `guard` (floats: a quiet NaN)
constexpr uint32_t F32_NAN = 0x7FC00000u;
void alloc32(DevBuf<uint32_t>& d, const void* src, size_t n, uint32_t guard) {
    std::vector<uint32_t> h(n + IN_GUARD, guard);
    if (src) memcpy(h.data(), src, n * 4);
    d.alloc(h.size());
    HIP_CHECK(hipMemcpy(d.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
}

}  // namespace
