// gemm_debug.hip - test scaffolding (include/mi_speech_debug.h): ONE launch of a GEMM launcher of lm_kernels.hip / lm_qgemm.hip /
// lm_prefill.hip on caller-supplied host data, so that tests/test_gpu_gemm_ops.py can hold the kernels to an operator-level reference.
//
// Every call packs its operands with the product's own load-time kernels (launch_pack_weight / launch_pack_qweight, k_pf_pack_rows),
// launches once and copies the result back as float.  What makes a silent error visible:
//   - the output is allocated as [guard | body | guard] (a guard is at least one tile row, 16 output rows), all of it filled with the
//     byte 0xFF (a NaN in float32 and in bf16) before the launch: an element the kernel never wrote comes back as NaN, and a guard
//     byte that changed fails the call (MIS_ERR_GENERATION_FAILED);
//   - every input the kernel reads is followed by a guard of NaN (16-bit inputs: quiet NaN of their format; codes: 0xFF bytes), so a
//     read past the end lands in the result instead of in a neighbour's memory.
#include <cstring>
#include "common.h"
#include "lm_kernels.h"
#include "debug_guard.h"
#include "lm_debug_util.h"

namespace {

// X [M][K] host bf16 -> packed fragments [K/32][MT][64][8] through k_pf_pack_rows (rows >= M zero), NaN behind
void pack_x(DevBuf<uint16_t>& xpk, const uint16_t* X, int M, int K, int Mpad) {
    std::vector<uint16_t> rows((size_t)Mpad * K, 0);
    std::copy(X, X + (size_t)M * K, rows.begin());
    DevBuf<uint16_t> drows;
    alloc16(drows, rows.data(), rows.size(), BF16_NAN);
    alloc16(xpk, nullptr, (size_t)Mpad * K, BF16_NAN);
    launch_pf_pack_rows(drows.p, xpk.p, Mpad, K, 0);
    HIP_CHECK(hipDeviceSynchronize());
}

void report_launch(int32_t* report) {
    if (!report) return;
    const GemmLaunchInfo& g = g_gemm_last_launch;
    const int32_t r[8] = {g.kernel, g.MT, g.R, g.epi, g.ksb, g.U, g.bits, g.sbt};
    std::copy(r, r + 8, report);
}

}  // namespace

extern "C" mis_status mis_debug_gemm_skinny(int device, const uint16_t* W, const uint16_t* W2, const uint16_t* X, const uint16_t* bias, int M,
                                            int N, int K, int epi, int R, int ksb, int U, int S, float* out, int64_t capacity, int32_t* report) {
    MIS_API_BEGIN
    MIS_REQUIRE(W && X && out && M >= 1 && M <= 64 && N >= 16 && N % 16 == 0 && K >= 32 && K % 32 == 0 && S >= 1, MIS_ERR_INVALID_INPUT,
                "dense GEMM: 1..64 rows, N a multiple of 16, K a multiple of 32");
    MIS_REQUIRE(epi >= EPI_PARTIAL && epi <= EPI_SILU_PACKED, MIS_ERR_INVALID_INPUT, "unknown epilogue %d", epi);
    const int KT = K / 32, NT = (W2 ? 2 : 1) * (N / 16), ncols = NT * 16, Mpad = (int)round_up(M, 16);
    MIS_REQUIRE(S <= KT, MIS_ERR_INVALID_INPUT, "%d K slices for %d k-tiles", S, KT);
    MIS_REQUIRE(epi != EPI_SILU_MUL || W2, MIS_ERR_INVALID_INPUT, "the gate * up epilogue needs the interleaved second matrix");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> wp, xpk, db;
    pack_w(wp, W, W2, N, K);
    pack_x(xpk, X, M, K, Mpad);
    if (bias) alloc16(db, bias, ncols, BF16_NAN);
    GuardedOut o;
    o.alloc(skinny_out_bytes(epi, S, Mpad, ncols), (size_t)16 * ncols * 4);
    g_gemm_last_launch = GemmLaunchInfo{};
    launch_gemm_skinny(epi, R, ksb, wp.p, xpk.p, o.p(), NT, KT, S, ncols, Mpad, 0, bias ? db.p : nullptr, U);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    report_launch(report);
    o.check_guards();
    fetch_skinny(o, epi, S, Mpad, ncols, out, capacity);
    MIS_API_END
}

extern "C" mis_status mis_debug_gemm_skinny_q(int device, int bits, int sb_dtype, const uint32_t* wq, const uint16_t* scales, const uint16_t* biases,
                                              const uint32_t* wq2, const uint16_t* scales2, const uint16_t* biases2, const uint16_t* X,
                                              const uint16_t* bias, int M, int N, int K, int epi, int R, int ksb, int S, float* out,
                                              int64_t capacity, int32_t* report) {
    MIS_API_BEGIN
    MIS_REQUIRE(wq && scales && biases && X && out && M >= 1 && M <= 64 && N >= 16 && N % 16 == 0 && K >= 64 && K % 64 == 0 && S >= 1,
                MIS_ERR_INVALID_INPUT, "quantised GEMM: 1..64 rows, N a multiple of 16, K a multiple of 64");
    MIS_REQUIRE((bits == 8 || bits == 4) && (sb_dtype == MIS_BF16 || sb_dtype == MIS_F16), MIS_ERR_INVALID_INPUT, "8 or 4 bits, bf16 or f16 scales");
    MIS_REQUIRE(epi >= EPI_PARTIAL && epi <= EPI_GELU_PACKED, MIS_ERR_INVALID_INPUT, "unknown epilogue %d", epi);
    const bool two = wq2 != nullptr;
    MIS_REQUIRE(!two || (scales2 && biases2), MIS_ERR_INVALID_INPUT, "second matrix without scales / biases");
    MIS_REQUIRE(epi != EPI_SILU_MUL || two, MIS_ERR_INVALID_INPUT, "the gate * up epilogue needs the interleaved second matrix");
    const int G = K / 64, NT = (two ? 2 : 1) * (N / 16), ncols = NT * 16, Mpad = (int)round_up(M, 16);
    const uint16_t nan = sb_dtype == MIS_F16 ? F16_NAN : BF16_NAN;
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint8_t> qp, dq;
    DevBuf<uint16_t> sb, dsc, dbi, xpk, db;
    const size_t code_bytes = (size_t)N * K * bits / 8;
    alloc_bytes(qp, nullptr, (two ? 2 : 1) * code_bytes);
    alloc16(sb, nullptr, (size_t)NT * G * 32, nan);
    for (int h = 0; h < (two ? 2 : 1); ++h) {
        alloc_bytes(dq, h ? wq2 : wq, code_bytes);
        alloc16(dsc, h ? scales2 : scales, (size_t)N * G, nan);
        alloc16(dbi, h ? biases2 : biases, (size_t)N * G, nan);
        launch_pack_qweight(bits, reinterpret_cast<const uint32_t*>(dq.p), dsc.p, dbi.p, qp.p, sb.p, N, K, two ? 2 : 1, h, 0);
        HIP_CHECK(hipDeviceSynchronize());
    }
    pack_x(xpk, X, M, K, Mpad);
    if (bias) alloc16(db, bias, ncols, BF16_NAN);
    GuardedOut o;
    o.alloc(skinny_out_bytes(epi, S, Mpad, ncols), (size_t)16 * ncols * 4);
    g_gemm_last_launch = GemmLaunchInfo{};
    launch_gemm_skinny_q(bits, epi, R, ksb, qp.p, sb.p, xpk.p, o.p(), NT, G, S, ncols, Mpad, 0, bias ? db.p : nullptr, sb_dtype);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    report_launch(report);
    o.check_guards();
    fetch_skinny(o, epi, S, Mpad, ncols, out, capacity);
    MIS_API_END
}

extern "C" mis_status mis_debug_gemm_pf(int device, const uint16_t* W, const uint16_t* W2, const uint16_t* X, const uint16_t* h, int M, int N, int K,
                                        int epi, float* out, int64_t capacity, int32_t* report) {
    MIS_API_BEGIN
    MIS_REQUIRE(W && X && out && M >= 1 && N >= 16 && N % 16 == 0 && K >= 32 && K % 32 == 0, MIS_ERR_INVALID_INPUT,
                "prefill GEMM: N a multiple of 16, K a multiple of 32");
    MIS_REQUIRE(epi >= PF_F32 && epi <= PF_SILU, MIS_ERR_INVALID_INPUT, "unknown prefill epilogue %d", epi);
    MIS_REQUIRE(epi != PF_RESID || h, MIS_ERR_INVALID_INPUT, "the residual epilogue needs h");
    MIS_REQUIRE(epi != PF_SILU || W2, MIS_ERR_INVALID_INPUT, "the gate * up epilogue needs the interleaved second matrix");
    const int ncols = (W2 ? 2 : 1) * N, ocols = epi == PF_SILU ? ncols / 2 : ncols;
    const size_t n_out = (size_t)M * ocols, esz = epi == PF_F32 ? 4 : 2;
    MIS_REQUIRE((int64_t)n_out <= capacity, MIS_ERR_INVALID_INPUT, "output needs %zu floats", n_out);
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> wp, dx;
    pack_w(wp, W, W2, N, K);
    alloc16(dx, X, (size_t)M * K, BF16_NAN);
    GuardedOut o;
    o.alloc(n_out * esz, (size_t)128 * ocols * esz);             // a whole 128-row block tile of rows >= M would still land in it
    if (epi == PF_RESID) HIP_CHECK(hipMemcpy(o.p(), h, n_out * 2, hipMemcpyHostToDevice));
    g_gemm_last_launch = GemmLaunchInfo{};
    launch_gemm_pf(epi, dx.p, wp.p, o.p(), M, ncols, K, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    report_launch(report);
    o.check_guards();
    if (epi == PF_F32) {
        HIP_CHECK(hipMemcpy(out, o.p(), n_out * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> hb(n_out);
        HIP_CHECK(hipMemcpy(hb.data(), o.p(), n_out * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n_out; ++i) out[i] = bf16_to_f32(hb[i]);
    }
    MIS_API_END
}
