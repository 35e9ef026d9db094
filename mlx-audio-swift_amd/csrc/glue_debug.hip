// glue_debug.hip - test scaffolding (include/mi_speech_debug.h): ONE call of a launcher of the LM glue - launch_embed_rmsnorm,
// launch_reduce_residual_rmsnorm, launch_gemm_skinny_norm, the prefill row kernels of lm_prefill.hip, launch_prefill_feed and the two load-time
// kernels launch_convert_to_bf16 / launch_dequant_affine - on caller-supplied host data, so that tests/test_gpu_glue_ops.py can hold them to
// an operator-level reference (tests/glue_ref.py).
//
// Nothing is computed here: the operands are uploaded as given and what the launch wrote is copied back.  What makes a silent error
// visible (debug_guard.h, as gemm_debug.hip, attn_debug.hip, codec_debug.hip and enc_debug.hip):
//   - every output is allocated as [guard | body | guard], all of it the byte 0xFF (a NaN in bf16 and float32, -1 as an integer) before the
//     launch: an element the kernel never wrote comes back as that, a guard byte that changed fails the call (MIS_ERR_GENERATION_FAILED);
//     buffers that go in and come back (h, the position arrays, the step counter) are uploaded into such a body;
//   - every input is followed by IN_GUARD NaNs (ids: an id outside every vocabulary; lens, prompts: zeros; bytes: 0xFF).
// The entry points refuse what would make a KERNEL read or write outside these buffers; what a launcher checks itself is left to it - its
// status is returned and nothing is launched.
#include <cstring>
#include "common.h"
#include "lm_kernels.h"
#include "debug_guard.h"
#include "lm_debug_util.h"
#include "../../include/mi_speech_debug.h"

namespace {

constexpr int64_t GLUE_MAX_ELEMS = (int64_t)1 << 26;         // per tensor

void glue_sync() {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
}

// a guarded buffer that goes in and comes back
void alloc_inout(GuardedOut& g, const void* src, size_t bytes, size_t guard_bytes) {
    g.alloc(bytes, guard_bytes);
    if (src) HIP_CHECK(hipMemcpy(g.p(), src, bytes, hipMemcpyHostToDevice));
}
void fetch(GuardedOut& g, void* dst) {
    g.check_guards();
    if (dst) HIP_CHECK(hipMemcpy(dst, g.p(), g.body, hipMemcpyDeviceToHost));
}

void report_glue(int32_t* report, bool gemm) {
    if (!report) return;
    const GlueLaunchInfo& g = g_glue_last_launch;
    if (gemm) { const int32_t r[5] = {g.kernel == 3 ? 3 : -1, g.epi, g.LN, g.SG, g.KW}; std::copy(r, r + 5, report); }
    else { const int32_t r[4] = {g.kernel, g.SG, g.CPT, g.threads}; std::copy(r, r + 4, report); }
}

}  // namespace

extern "C" mis_status mis_debug_lm_embed_rmsnorm(int device, const uint16_t* emb, const int32_t* ids, const uint8_t* active, int32_t* pos_cur,
                                                 int32_t* pos_next, const uint16_t* wnorm, int d, int vocab, float eps, int batch, int Mpad,
                                                 uint16_t* h_out, uint16_t* x_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(emb && ids && active && pos_cur && pos_next && wnorm && h_out && x_out, MIS_ERR_INVALID_INPUT, "embed + RMSNorm: every pointer is required");
    MIS_REQUIRE(d >= 1 && vocab >= 1 && batch >= 1 && Mpad >= batch && Mpad % 16 == 0 && Mpad <= 4096, MIS_ERR_INVALID_INPUT,
                "embed + RMSNorm: positive d, vocab; 1 <= batch <= Mpad (a multiple of 16)");
    MIS_REQUIRE((int64_t)vocab * d <= GLUE_MAX_ELEMS && (int64_t)Mpad * round_up(d, 32) <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "embed + RMSNorm: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> de, dw;
    DevBuf<uint32_t> di;
    DevBuf<uint8_t> da;
    alloc16(de, emb, (size_t)vocab * d, BF16_NAN);                 // a read behind the last row of the table is a NaN
    alloc16(dw, wnorm, d, BF16_NAN);
    alloc32(di, ids, batch, 0x7FFFFFFFu);                          // an id read past the batch is outside every vocabulary
    alloc_bytes(da, active, batch);
    GuardedOut pc, pn, h, x;
    alloc_inout(pc, pos_cur, (size_t)batch * 4, 256);
    alloc_inout(pn, pos_next, (size_t)batch * 4, 256);
    h.alloc((size_t)Mpad * d * 2, (size_t)16 * d * 2);
    x.alloc((size_t)Mpad * round_up(d, 32) * 2, (size_t)16 * round_up(d, 32) * 2);
    launch_embed_rmsnorm(de.p, reinterpret_cast<const int32_t*>(di.p), da.p, reinterpret_cast<int*>(pc.p()), reinterpret_cast<int*>(pn.p()), dw.p,
                         reinterpret_cast<bf16_t*>(h.p()), reinterpret_cast<bf16_t*>(x.p()), d, vocab, eps, batch, Mpad, 0);
    glue_sync();
    fetch(pc, pos_cur); fetch(pn, pos_next); fetch(h, h_out); fetch(x, x_out);
    MIS_API_END
}

extern "C" mis_status mis_debug_lm_glue(int device, const float* slabs, int S, int Mpad, int N, uint16_t* h, const uint16_t* wnorm,
                                        const uint16_t* ln_bias, float eps, uint16_t* x_out, int32_t* report) {
    MIS_API_BEGIN
    if (report) { const int32_t none[4] = {-1, 0, 0, 0}; std::copy(none, none + 4, report); }
    MIS_REQUIRE(slabs && h && wnorm && x_out, MIS_ERR_INVALID_INPUT, "glue: slabs, h, wnorm and x_out are required");
    MIS_REQUIRE(S >= 1 && S <= 64 && N >= 1 && Mpad >= 16 && Mpad % 16 == 0 && Mpad <= 4096, MIS_ERR_INVALID_INPUT,
                "glue: 1 .. 64 slabs, positive N, Mpad a multiple of 16");
    MIS_REQUIRE((int64_t)S * Mpad * N <= GLUE_MAX_ELEMS && (int64_t)Mpad * round_up(N, 32) <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "glue: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> ds;
    DevBuf<uint16_t> dw, db;
    alloc32(ds, slabs, (size_t)S * Mpad * N, F32_NAN);
    alloc16(dw, wnorm, N, BF16_NAN);
    if (ln_bias) alloc16(db, ln_bias, N, BF16_NAN);
    GuardedOut gh, x;
    alloc_inout(gh, h, (size_t)Mpad * N * 2, (size_t)16 * N * 2);
    x.alloc((size_t)Mpad * round_up(N, 32) * 2, (size_t)16 * round_up(N, 32) * 2);
    g_glue_last_launch = GlueLaunchInfo{};
    launch_reduce_residual_rmsnorm(reinterpret_cast<const float*>(ds.p), S, Mpad, N, reinterpret_cast<bf16_t*>(gh.p()), dw.p, reinterpret_cast<bf16_t*>(x.p()), eps,
                                   0, ln_bias ? db.p : nullptr);
    glue_sync();
    report_glue(report, false);
    fetch(gh, h); fetch(x, x_out);
    MIS_API_END
}

extern "C" int32_t mis_debug_gemm_skinny_norm_ok(int epi, int R, int KT, int S, int S_in, int Mpad, int nrows, int layer_norm) {
    return gemm_skinny_norm_ok(epi, R, KT, S, S_in, Mpad, nrows, layer_norm != 0) ? 1 : 0;
}

extern "C" mis_status mis_debug_gemm_skinny_norm(int device, const uint16_t* W, const float* slabs, int S_in, const uint16_t* h_in, const uint16_t* wnorm,
                                                 const uint16_t* ln_bias, float eps, int nrows, int epi, int R, int S, const uint16_t* bias, int N_out,
                                                 int K, float* out, int64_t capacity, uint16_t* h_out, uint16_t* h_in_after, int32_t* report) {
    MIS_API_BEGIN
    if (report) { const int32_t none[5] = {-1, 0, 0, 0, 0}; std::copy(none, none + 5, report); }
    MIS_REQUIRE(W && slabs && h_in && wnorm && out && h_out, MIS_ERR_INVALID_INPUT, "norm-prologue GEMM: W, slabs, h_in, wnorm, out and h_out are required");
    MIS_REQUIRE(N_out >= 16 && N_out % 16 == 0 && K >= 32 && K % 32 == 0 && S >= 1 && S <= 64 && S_in >= 1 && S_in <= 64 && R >= 1, MIS_ERR_INVALID_INPUT,
                "norm-prologue GEMM: N_out a multiple of 16, K a multiple of 32, 1 .. 64 slabs in and out");
    MIS_REQUIRE(epi >= EPI_PARTIAL && epi <= EPI_SILU_PACKED && epi != EPI_SILU_MUL, MIS_ERR_INVALID_INPUT, "norm-prologue GEMM: epilogue %d", epi);
    MIS_REQUIRE((int64_t)N_out * K <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "norm-prologue GEMM: tensor too large");
    constexpr int Mpad = 16;
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> wp, dh, dw, dlb, db;
    DevBuf<uint32_t> ds;
    pack_w(wp, W, nullptr, N_out, K);
    alloc32(ds, slabs, (size_t)S_in * Mpad * K, F32_NAN);
    alloc16(dh, h_in, (size_t)Mpad * K, BF16_NAN);
    alloc16(dw, wnorm, K, BF16_NAN);
    if (ln_bias) alloc16(dlb, ln_bias, K, BF16_NAN);
    if (bias) alloc16(db, bias, N_out, BF16_NAN);
    GuardedOut o, ho;
    o.alloc(skinny_out_bytes(epi, S, Mpad, N_out), (size_t)16 * N_out * 4);
    ho.alloc((size_t)Mpad * K * 2, (size_t)16 * K * 2);
    g_glue_last_launch = GlueLaunchInfo{};
    launch_gemm_skinny_norm(epi, R, wp.p, reinterpret_cast<const float*>(ds.p), S_in, dh.p, reinterpret_cast<bf16_t*>(ho.p()), dw.p, ln_bias ? dlb.p : nullptr, eps,
                            nrows, o.p(), N_out / 16, K / 32, S, N_out, Mpad, 0, bias ? db.p : nullptr);
    glue_sync();
    report_glue(report, true);
    o.check_guards();
    fetch_skinny(o, epi, S, Mpad, N_out, out, capacity);
    fetch(ho, h_out);
    if (h_in_after) HIP_CHECK(hipMemcpy(h_in_after, dh.p, (size_t)Mpad * K * 2, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_pf_rows(int device, int mode, const uint16_t* table, const int32_t* prompt, const int32_t* lens, int Lmax, int t0, int Tc,
                                        int batch, int Mpad, int vocab, int src_rows, const uint16_t* wnorm, const float* part, int64_t n, int d, float eps,
                                        uint16_t* h, uint16_t* x, int32_t* pos_tab, uint8_t* act_tab) {
    MIS_API_BEGIN
    MIS_REQUIRE(mode >= 0 && mode <= 4, MIS_ERR_INVALID_INPUT, "prefill rows: mode 0 .. 4");
    HIP_CHECK(hipSetDevice(device));
    if (mode == 3) {                                               // add_resid: h [n] += part [n]
        MIS_REQUIRE(h && part && n >= 1 && n <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "add_resid: h, part and 1 <= n are required");
        DevBuf<uint32_t> dp;
        alloc32(dp, part, (size_t)n, F32_NAN);
        GuardedOut gh;
        alloc_inout(gh, h, (size_t)n * 2, 4096);
        launch_pf_add_resid(reinterpret_cast<bf16_t*>(gh.p()), reinterpret_cast<const float*>(dp.p), (size_t)n, 0);
        glue_sync();
        fetch(gh, h);
        return MIS_OK;
    }
    MIS_REQUIRE(h && x && d >= 1 && Mpad >= 1 && Mpad <= 4096, MIS_ERR_INVALID_INPUT, "prefill rows: h, x, positive d and Mpad are required");
    if (mode == 4) {                                               // pack_rows: h = rows [Mpad][d] -> x = the packed image
        MIS_REQUIRE(Mpad % 16 == 0 && (int64_t)Mpad * round_up(d, 32) <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "pack_rows: Mpad a multiple of 16");
        DevBuf<uint16_t> dr;
        alloc16(dr, h, (size_t)Mpad * d, BF16_NAN);
        GuardedOut gx;
        gx.alloc((size_t)Mpad * round_up(d, 32) * 2, (size_t)16 * round_up(d, 32) * 2);
        launch_pf_pack_rows(dr.p, reinterpret_cast<bf16_t*>(gx.p()), Mpad, d, 0);
        glue_sync();
        fetch(gx, x);
        HIP_CHECK(hipMemcpy(h, dr.p, (size_t)Mpad * d * 2, hipMemcpyDeviceToHost));
        return MIS_OK;
    }
    MIS_REQUIRE(wnorm && Tc >= 1 && (int64_t)Tc * Mpad * d <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "prefill rows: wnorm and Tc >= 1 are required");
    const size_t rows = (size_t)Tc * Mpad;
    DevBuf<uint16_t> dw;
    alloc16(dw, wnorm, d, BF16_NAN);
    GuardedOut gx;
    gx.alloc(rows * d * 2, (size_t)4 * d * 2);
    if (mode == 2) {                                               // rmsnorm: h [rows][d] -> x
        DevBuf<uint16_t> dh;
        alloc16(dh, h, rows * d, BF16_NAN);
        launch_pf_rmsnorm(dh.p, dw.p, reinterpret_cast<bf16_t*>(gx.p()), (int)rows, d, eps, 0);
        glue_sync();
        fetch(gx, x);
        HIP_CHECK(hipMemcpy(h, dh.p, rows * d * 2, hipMemcpyDeviceToHost));
        return MIS_OK;
    }
    // embed (0) / rows (1): the chunk [t0, t0 + Tc) of a left-padded prompt of Lmax positions
    MIS_REQUIRE(table && lens && pos_tab && act_tab && batch >= 1 && batch <= Mpad && Lmax >= 1 && t0 >= 0 && t0 + Tc <= Lmax, MIS_ERR_INVALID_INPUT,
                "prefill rows: table, lens, both tables, 1 <= batch <= Mpad and a chunk inside 0 .. Lmax are required");
    for (int b = 0; b < batch; ++b) MIS_REQUIRE(lens[b] >= 0 && lens[b] <= Lmax, MIS_ERR_INVALID_INPUT, "prefill rows: row %d of %d positions", b, lens[b]);
    DevBuf<uint16_t> dt;
    DevBuf<uint32_t> dp, dl;
    alloc32(dl, lens, batch, 0);
    GuardedOut gh, gp, ga;
    gh.alloc(rows * d * 2, (size_t)4 * d * 2);
    gp.alloc(rows * 4, 256);
    ga.alloc(rows, 256);
    if (mode == 0) {
        MIS_REQUIRE(prompt && vocab >= 1 && (int64_t)vocab * d <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "prefill embed: prompt and vocab >= 1 are required");
        alloc16(dt, table, (size_t)vocab * d, BF16_NAN);
        alloc32(dp, prompt, (size_t)batch * Lmax, 0);
        launch_pf_embed_rmsnorm(dt.p, reinterpret_cast<const int32_t*>(dp.p), reinterpret_cast<const int32_t*>(dl.p), Lmax, t0, Tc, batch, Mpad, vocab, dw.p,
                                reinterpret_cast<bf16_t*>(gh.p()), reinterpret_cast<bf16_t*>(gx.p()), reinterpret_cast<int32_t*>(gp.p()), ga.p(), d, eps, 0);
    } else {
        MIS_REQUIRE(src_rows >= batch && (int64_t)Lmax * src_rows * d <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "prefill rows: src_rows >= batch");
        alloc16(dt, table, (size_t)Lmax * src_rows * d, BF16_NAN);
        launch_pf_rows_rmsnorm(dt.p, src_rows, reinterpret_cast<const int32_t*>(dl.p), Lmax, t0, Tc, batch, Mpad, dw.p, reinterpret_cast<bf16_t*>(gh.p()),
                               reinterpret_cast<bf16_t*>(gx.p()), reinterpret_cast<int32_t*>(gp.p()), ga.p(), d, eps, 0);
    }
    glue_sync();
    fetch(gh, h); fetch(gx, x); fetch(gp, pos_tab); fetch(ga, act_tab);
    MIS_API_END
}

extern "C" mis_status mis_debug_prefill_feed(int device, const int32_t* prompt, const int32_t* lens, int Lmax, int32_t* step_counter, int batch,
                                             int32_t* ids_out, uint8_t* active_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(prompt && lens && step_counter && ids_out && active_out && Lmax >= 1 && batch >= 1 && batch <= 1024, MIS_ERR_INVALID_INPUT,
                "prefill feed: every pointer, Lmax >= 1 and 1 <= batch <= 1024 (one block) are required");
    for (int b = 0; b < batch; ++b) MIS_REQUIRE(lens[b] >= 0 && lens[b] <= Lmax, MIS_ERR_INVALID_INPUT, "prefill feed: row %d of %d positions", b, lens[b]);
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> dp, dl;
    alloc32(dp, prompt, (size_t)batch * Lmax, 0);
    alloc32(dl, lens, batch, 0);
    GuardedOut sc, gi, ga;
    alloc_inout(sc, step_counter, 4, 256);
    gi.alloc((size_t)batch * 4, 256);
    ga.alloc(batch, 256);
    launch_prefill_feed(reinterpret_cast<const int32_t*>(dp.p), reinterpret_cast<const int32_t*>(dl.p), Lmax, reinterpret_cast<int*>(sc.p()),
                        reinterpret_cast<int32_t*>(gi.p()), ga.p(), batch, 0);
    glue_sync();
    fetch(sc, step_counter); fetch(gi, ids_out); fetch(ga, active_out);
    MIS_API_END
}

extern "C" mis_status mis_debug_convert_to_bf16(int device, const void* src, int dtype, int64_t n, uint16_t* dst_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(src && dst_out && n >= 1 && n <= GLUE_MAX_ELEMS && (dtype == MIS_F32 || dtype == MIS_F16 || dtype == MIS_BF16), MIS_ERR_INVALID_INPUT,
                "convert: src, dst_out, n >= 1 and a float dtype are required");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> d32;
    DevBuf<uint16_t> d16;
    if (dtype == MIS_F32) alloc32(d32, src, (size_t)n, F32_NAN);
    else alloc16(d16, static_cast<const uint16_t*>(src), (size_t)n, dtype == MIS_F16 ? F16_NAN : BF16_NAN);
    GuardedOut o;
    o.alloc((size_t)n * 2, 4096);
    launch_convert_to_bf16(dtype == MIS_F32 ? (const void*)d32.p : (const void*)d16.p, dtype, reinterpret_cast<bf16_t*>(o.p()), (size_t)n, 0);
    glue_sync();
    fetch(o, dst_out);
    MIS_API_END
}

extern "C" mis_status mis_debug_dequant_affine(int device, const uint32_t* wq, const void* scales, const void* biases, int sb_dtype, int N, int K, int group,
                                               int bits, uint16_t* dst_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(wq && scales && biases && dst_out && N >= 1 && K >= 1 && (int64_t)N * K <= GLUE_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "dequantise: wq, scales, biases, dst_out and positive N, K are required");
    MIS_REQUIRE(bits >= 1 && bits <= 16 && 32 % bits == 0 && K % (32 / bits) == 0 && group >= 1 && K % group == 0, MIS_ERR_INVALID_INPUT,
                "dequantise: bits a divisor of 32 (<= 16), K whole words and whole groups");
    MIS_REQUIRE(sb_dtype == MIS_F32 || sb_dtype == MIS_F16 || sb_dtype == MIS_BF16, MIS_ERR_INVALID_INPUT, "dequantise: scales as f32, f16 or bf16");
    HIP_CHECK(hipSetDevice(device));
    const size_t G = (size_t)N * (K / group);
    DevBuf<uint32_t> dq, s32, b32;
    DevBuf<uint16_t> s16, b16;
    alloc32(dq, wq, (size_t)N * (K / (32 / bits)), 0xFFFFFFFFu);
    if (sb_dtype == MIS_F32) { alloc32(s32, scales, G, F32_NAN); alloc32(b32, biases, G, F32_NAN); }
    else {
        const uint16_t nan = sb_dtype == MIS_F16 ? F16_NAN : BF16_NAN;
        alloc16(s16, static_cast<const uint16_t*>(scales), G, nan); alloc16(b16, static_cast<const uint16_t*>(biases), G, nan);
    }
    GuardedOut o;
    o.alloc((size_t)N * K * 2, (size_t)K * 2);
    launch_dequant_affine(dq.p, sb_dtype == MIS_F32 ? (const void*)s32.p : (const void*)s16.p, sb_dtype == MIS_F32 ? (const void*)b32.p : (const void*)b16.p,
                          sb_dtype, reinterpret_cast<bf16_t*>(o.p()), N, K, group, bits, 0);
    glue_sync();
    fetch(o, dst_out);
    MIS_API_END
}
