// lm_debug_util.h - what gemm_debug.hip and glue_debug.hip share: weights packed by the product's load-time kernel, the output of a skinny
// GEMM launch sized and copied back as float.
#pragma once
#include "lm_kernels.h"
#include "debug_guard.h"

namespace {

// W [N][K] (and W2, interleaved in tiles of 16 rows behind it: the gate / up layout) -> packed MFMA-A tiles through launch_pack_weight
void pack_w(DevBuf<uint16_t>& wp, const uint16_t* W, const uint16_t* W2, int N, int K) {
    const int nt = N / 16;
    alloc16(wp, nullptr, (size_t)(W2 ? 2 : 1) * N * K, BF16_NAN);
    DevBuf<uint16_t> src;
    for (int h = 0; h < (W2 ? 2 : 1); ++h) {
        alloc16(src, h ? W2 : W, (size_t)N * K, BF16_NAN);
        launch_pack_weight(src.p, wp.p, N, K, nt, W2 ? 2 : 1, h, 0);
        HIP_CHECK(hipDeviceSynchronize());
    }
}

// copies the result of a skinny launch back as float: EPI_PARTIAL [S][Mpad][ncols], EPI_BF16 [Mpad][ncols], packed epilogues un-packed
// with xpk_index into [Mpad][F] (F = ncols, or ncols / 2 behind the gate * up product)
void fetch_skinny(GuardedOut& o, int epi, int S, int Mpad, int ncols, float* out, int64_t capacity) {
    const int MT = Mpad / 16;
    if (epi == EPI_PARTIAL) {
        const size_t n = (size_t)S * Mpad * ncols;
        MIS_REQUIRE((int64_t)n <= capacity, MIS_ERR_INVALID_INPUT, "output needs %zu floats", n);
        HIP_CHECK(hipMemcpy(out, o.p(), n * 4, hipMemcpyDeviceToHost));
        return;
    }
    std::vector<uint16_t> h(o.body / 2);
    HIP_CHECK(hipMemcpy(h.data(), o.p(), o.body, hipMemcpyDeviceToHost));
    const int F = epi == EPI_SILU_MUL ? ncols / 2 : ncols;
    MIS_REQUIRE((int64_t)Mpad * F <= capacity, MIS_ERR_INVALID_INPUT, "output needs %zu floats", (size_t)Mpad * F);
    if (epi == EPI_BF16) {
        for (size_t i = 0; i < (size_t)Mpad * F; ++i) out[i] = bf16_to_f32(h[i]);
        return;
    }
    const int Fpad = (int)round_up(F, 32);
    for (int m = 0; m < Mpad; ++m)
        for (int k = 0; k < Fpad; ++k) {
            const uint16_t v = h[xpk_index(m, k, MT)];
            if (k < F) out[(size_t)m * F + k] = bf16_to_f32(v);
            else MIS_REQUIRE(v == 0xFFFF, MIS_ERR_GENERATION_FAILED, "packed output: column %d past the %d features was written", k, F);
        }
}

size_t skinny_out_bytes(int epi, int S, int Mpad, int ncols) {
    if (epi == EPI_PARTIAL) return (size_t)S * Mpad * ncols * 4;
    if (epi == EPI_BF16) return (size_t)Mpad * ncols * 2;
    const int F = epi == EPI_SILU_MUL ? ncols / 2 : ncols;
    return round_up(F, 32) * (size_t)Mpad * 2;
}

}  // namespace
