// enc_debug.hip - test scaffolding (include/mi_speech_debug.h): ONE call of a launcher of whisper_kernels.h (launch_gemm_big,
// launch_layernorm, launch_im2col3_*, launch_scatter_kv, launch_attn_prefill, launch_whisper_embed_ln, launch_whisper_suppress) on
// caller-supplied host data, so that tests/test_gpu_enc_ops.py can hold the encoder kernels to an operator-level reference.
//
// Nothing is computed here: the operands are uploaded as given and what the launch wrote is copied back.  What makes a silent error
// visible (debug_guard.h, as gemm_debug.hip, attn_debug.hip and codec_debug.hip):
//   - every output is allocated as [guard | body | guard], all of it the byte 0xFF (a NaN in bf16) before the launch: an element the kernel
//     never wrote comes back as 0xFFFF, a guard byte that changed fails the call (MIS_ERR_GENERATION_FAILED), and so does a changed padding
//     column of a strided output;
//   - every input is followed by IN_GUARD NaNs, and the columns of a strided input that the kernel has no business with are NaN.  Inputs
//     are sized so that every address a CORRECT kernel reads lies inside the allocation - the GEMM's X is (M - 1) ldx + K elements, which
//     is what the clamped staging rows of k_gemm_big2 / 3 reach when rows overlap (ldx < K).
// The entry points refuse what would make a KERNEL read or write out of bounds; what a launcher checks itself is left to it - its status
// is returned and nothing is launched.
#include <cstring>
#include "common.h"
#include "whisper_kernels.h"
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

namespace {

constexpr int64_t ENC_MAX_ELEMS = (int64_t)1 << 28;          // per tensor

void enc_sync() {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
}

// rows x cols payloads -> rows of stride ld (>= cols), the columns behind NaN
void alloc16_rows(DevBuf<uint16_t>& d, const uint16_t* src, size_t rows, size_t cols, size_t ld) {
    std::vector<uint16_t> h(rows * ld, BF16_NAN);
    for (size_t r = 0; r < rows; ++r) std::copy(src + r * cols, src + (r + 1) * cols, h.begin() + r * ld);
    alloc16(d, h.data(), h.size(), BF16_NAN);
}

// rows x ld payloads of a guarded output -> the first `cols` of every row; the columns behind must still hold the fill
void fetch16_rows(GuardedOut& o, size_t rows, size_t ld, size_t cols, uint16_t* out) {
    o.check_guards();
    std::vector<uint16_t> h(o.body / 2);
    HIP_CHECK(hipMemcpy(h.data(), o.p(), o.body, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        std::copy(h.begin() + r * ld, h.begin() + r * ld + cols, out + r * cols);
        for (size_t c = cols; c < ld; ++c)
            MIS_REQUIRE(h[r * ld + c] == 0xFFFF, MIS_ERR_GENERATION_FAILED, "the kernel wrote column %zu of row %zu behind its %zu columns", c, r, cols);
    }
}

}  // namespace

extern "C" mis_status mis_debug_gemm_big(int device, int epi, const uint16_t* X, const uint16_t* W, const uint16_t* bias, const uint16_t* R,
                                         int M, int N, int K, int ldx, int pos_rows, uint16_t* C_out, int32_t* report) {
    MIS_API_BEGIN
    if (report) { const int32_t none[4] = {-1, 0, 0, 0}; std::copy(none, none + 4, report); }
    MIS_REQUIRE(X && W && C_out && M >= 1 && N >= 1 && K >= 1 && ldx >= 1, MIS_ERR_INVALID_INPUT, "big GEMM: X, W, C_out and positive M, N, K, ldx are required");
    MIS_REQUIRE((int64_t)M * N <= ENC_MAX_ELEMS && (int64_t)N * K <= ENC_MAX_ELEMS && (int64_t)(M - 1) * ldx + K <= ENC_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "big GEMM: tensor too large");
    MIS_REQUIRE((epi != BG_RESID && epi != BG_GELU_POS) || R, MIS_ERR_INVALID_INPUT, "big GEMM: the epilogue needs R");
    MIS_REQUIRE(epi != BG_GELU_POS || (pos_rows >= 1 && (int64_t)pos_rows * N <= ENC_MAX_ELEMS), MIS_ERR_INVALID_INPUT, "big GEMM: pos_rows >= 1");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> dX, dW, dB, dR;
    {   // the image the kernels address: row m at m ldx, K columns; with ldx > K the columns between the rows are NaN
        const size_t n = (size_t)(M - 1) * ldx + K;
        std::vector<uint16_t> h(X, X + n);
        if (ldx > K)
            for (int m = 0; m + 1 < M; ++m) std::fill(h.begin() + (size_t)m * ldx + K, h.begin() + (size_t)(m + 1) * ldx, BF16_NAN);
        alloc16(dX, h.data(), n, BF16_NAN);
    }
    alloc16(dW, W, (size_t)N * K, BF16_NAN);
    if (bias) alloc16(dB, bias, N, BF16_NAN);
    if (R && (epi == BG_RESID || epi == BG_GELU_POS)) alloc16(dR, R, (size_t)(epi == BG_RESID ? M : pos_rows) * N, BF16_NAN);
    GuardedOut c;
    c.alloc((size_t)M * N * 2, (size_t)256 * N * 2);               // a guard is one 256-row tile of output
    BigGemmParams p{dX.p, dW.p, bias ? dB.p : nullptr, dR.p, reinterpret_cast<bf16_t*>(c.p()), M, N, K, ldx, pos_rows};
    g_enc_last_launch = EncLaunchInfo{};
    launch_gemm_big(epi, p, 0);
    enc_sync();
    if (report) {
        const EncLaunchInfo& g = g_enc_last_launch;
        const int32_t r[4] = {g.gemm, g.epi, g.WM, g.WN};
        std::copy(r, r + 4, report);
    }
    c.check_guards();
    HIP_CHECK(hipMemcpy(C_out, c.p(), c.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_enc_layernorm(int device, const uint16_t* x, const uint16_t* w, const uint16_t* b, int rows, int d, float eps,
                                              uint16_t* y_out, int32_t* report) {
    MIS_API_BEGIN
    if (report) report[0] = -1;
    MIS_REQUIRE(x && w && b && y_out && rows >= 1 && d >= 1 && (int64_t)rows * d <= ENC_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "LayerNorm: x, w, b, y_out and positive rows, d are required");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> dx, dw, db;
    alloc16(dx, x, (size_t)rows * d, BF16_NAN);
    alloc16(dw, w, d, BF16_NAN);                                   // (k_layernorm8 reads w and b 16 bytes at a time: d % 8 == 0 there)
    alloc16(db, b, d, BF16_NAN);
    GuardedOut y;
    y.alloc((size_t)rows * d * 2, (size_t)4 * d * 2);
    g_enc_last_launch = EncLaunchInfo{};
    launch_layernorm(dx.p, reinterpret_cast<bf16_t*>(y.p()), dw.p, db.p, rows, d, eps, 0);
    enc_sync();
    if (report) report[0] = g_enc_last_launch.ln;
    y.check_guards();
    HIP_CHECK(hipMemcpy(y_out, y.p(), y.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_enc_im2col3(int device, const void* in, int in_is_f32, int B, int Tin, int C, int Tout, int stride, uint16_t* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(in && out && B >= 1 && Tin >= 1 && C >= 1 && Tout >= 1 && stride >= 1 && stride <= 4, MIS_ERR_INVALID_INPUT,
                "im2col: in, out and positive B, Tin, C, Tout, stride 1 .. 4 are required");
    MIS_REQUIRE((int64_t)B * Tin * C <= ENC_MAX_ELEMS && (int64_t)B * Tout * 3 * C <= ENC_MAX_ELEMS && (int64_t)Tout * stride <= ENC_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "im2col: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> d32;
    DevBuf<uint16_t> d16;
    const size_t n = (size_t)B * Tin * C;
    if (in_is_f32) alloc32(d32, in, n, F32_NAN);
    else alloc16(d16, static_cast<const uint16_t*>(in), n, BF16_NAN);
    GuardedOut o;
    o.alloc((size_t)B * Tout * 3 * C * 2, (size_t)4 * 3 * C * 2);
    if (in_is_f32) launch_im2col3_f32(reinterpret_cast<const float*>(d32.p), reinterpret_cast<bf16_t*>(o.p()), B, Tin, C, Tout, stride, 0);
    else launch_im2col3_bf16(d16.p, reinterpret_cast<bf16_t*>(o.p()), B, Tin, C, Tout, stride, 0);
    enc_sync();
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_enc_scatter_kv(int device, const uint16_t* src, int ld, int kcol0, int vcol0, int B, int T, int H, int D, int Spad,
                                               uint16_t* kc_out, uint16_t* vc_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(src && kc_out && vc_out && B >= 1 && T >= 1 && H >= 1 && D >= 1 && ld >= 1, MIS_ERR_INVALID_INPUT,
                "K/V scatter: src, both outputs and positive B, T, H, D, ld are required");
    MIS_REQUIRE(kcol0 >= 0 && vcol0 >= 0 && (int64_t)kcol0 + (int64_t)H * D <= ld && (int64_t)vcol0 + (int64_t)H * D <= ld, MIS_ERR_INVALID_INPUT,
                "K/V scatter: the K and V columns must lie inside a row of ld");
    MIS_REQUIRE(Spad >= 32 * cdiv(T, 32) && (int64_t)B * H * Spad * D <= ENC_MAX_ELEMS && (int64_t)B * T * ld <= ENC_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "K/V scatter: Spad must hold every 32-key tile of T");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> ds;
    {   // columns that are neither K nor V: NaN
        const size_t rows = (size_t)B * T, HD = (size_t)H * D;
        std::vector<uint16_t> h(rows * ld, BF16_NAN);
        for (size_t r = 0; r < rows; ++r) {
            std::copy(src + r * ld + kcol0, src + r * ld + kcol0 + HD, h.begin() + r * ld + kcol0);
            std::copy(src + r * ld + vcol0, src + r * ld + vcol0 + HD, h.begin() + r * ld + vcol0);
        }
        alloc16(ds, h.data(), h.size(), BF16_NAN);
    }
    GuardedOut kc, vc;
    const size_t el = (size_t)B * H * Spad * D;
    kc.alloc(el * 2, (size_t)Spad * D * 2);                          // a guard is one (row, head) slice
    vc.alloc(el * 2, (size_t)Spad * D * 2);
    launch_scatter_kv(ds.p, ld, kcol0, vcol0, reinterpret_cast<bf16_t*>(kc.p()), reinterpret_cast<bf16_t*>(vc.p()), B, T, H, D, Spad, 0);
    enc_sync();
    kc.check_guards(); vc.check_guards();
    HIP_CHECK(hipMemcpy(kc_out, kc.p(), el * 2, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(vc_out, vc.p(), el * 2, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_enc_attn_prefill(int device, const uint16_t* q, int ldq, const uint16_t* kc_img, const uint16_t* vc_img, int B, int T,
                                                 int H, int D, int Spad, int ldo, uint16_t* out, int32_t* report) {
    MIS_API_BEGIN
    if (report) { report[0] = -1; report[1] = 0; }
    MIS_REQUIRE(q && kc_img && vc_img && out && B >= 1 && T >= 1 && H >= 1 && D >= 8 && D % 8 == 0, MIS_ERR_INVALID_INPUT,
                "prefill attention: q, both cache images, out and positive B, T, H, D (a multiple of 8) are required");
    const int64_t HD = (int64_t)H * D;
    MIS_REQUIRE(ldq >= HD && ldq % 8 == 0 && ldo >= HD, MIS_ERR_INVALID_INPUT, "prefill attention: ldq >= H D (16-byte rows), ldo >= H D");
    MIS_REQUIRE(Spad % 32 == 0 && Spad >= 32 * cdiv(T, 32), MIS_ERR_INVALID_INPUT, "prefill attention: Spad a multiple of 32 that holds every tile of T");
    MIS_REQUIRE((int64_t)B * T * ldq <= ENC_MAX_ELEMS && (int64_t)B * T * ldo <= ENC_MAX_ELEMS && (int64_t)B * HD * Spad <= ENC_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "prefill attention: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> dq, dk, dv;
    const size_t rows = (size_t)B * T, el = (size_t)B * HD * Spad;
    alloc16_rows(dq, q, rows, HD, ldq);
    alloc16(dk, kc_img, el, BF16_NAN);
    alloc16(dv, vc_img, el, BF16_NAN);
    GuardedOut o;
    o.alloc(rows * ldo * 2, (size_t)16 * ldo * 2);
    g_enc_last_launch = EncLaunchInfo{};
    launch_attn_prefill(dq.p, ldq, dk.p, dv.p, reinterpret_cast<bf16_t*>(o.p()), ldo, B, T, H, D, Spad, 0);
    enc_sync();
    if (report) { report[0] = g_enc_last_launch.attn; report[1] = g_enc_last_launch.attn_D; }
    fetch16_rows(o, rows, ldo, HD, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_whisper_embed_ln(int device, const uint16_t* emb, const uint16_t* pos_emb, const int32_t* ids, const uint8_t* active,
                                                 int32_t* pos_cur, int32_t* pos_next, const uint16_t* lw, const uint16_t* lb, int d, int vocab,
                                                 int max_pos, int batch, int Mpad, uint16_t* h_out, uint16_t* x_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(emb && pos_emb && ids && active && pos_cur && pos_next && lw && lb && h_out && x_out, MIS_ERR_INVALID_INPUT, "embed + LayerNorm: every pointer is required");
    MIS_REQUIRE(d >= 32 && d % 32 == 0 && vocab >= 1 && max_pos >= 1 && batch >= 1 && Mpad >= batch && Mpad % 16 == 0 && Mpad <= 4096, MIS_ERR_INVALID_INPUT,
                "embed + LayerNorm: d a multiple of 32, 1 <= batch <= Mpad (a multiple of 16)");
    MIS_REQUIRE((int64_t)vocab * d <= ENC_MAX_ELEMS && (int64_t)max_pos * d <= ENC_MAX_ELEMS && (int64_t)Mpad * d <= ENC_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "embed + LayerNorm: tensor too large");
    for (int m = 0; m < batch; ++m) MIS_REQUIRE(pos_next[m] >= 0, MIS_ERR_INVALID_INPUT, "embed + LayerNorm: row %d at position %d", m, pos_next[m]);
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> de, dp, dw, db;
    DevBuf<uint32_t> di;
    DevBuf<uint8_t> da;
    alloc16(de, emb, (size_t)vocab * d, BF16_NAN);
    alloc16(dp, pos_emb, (size_t)max_pos * d, BF16_NAN);
    alloc16(dw, lw, d, BF16_NAN);
    alloc16(db, lb, d, BF16_NAN);
    alloc32(di, ids, batch, 0x7FFFFFFFu);                          // an id read past the batch is out of range (-> row 0)
    alloc_bytes(da, active, batch);
    GuardedOut pc, pn, h, x;
    pc.alloc((size_t)batch * 4, 256); pn.alloc((size_t)batch * 4, 256);
    HIP_CHECK(hipMemcpy(pc.p(), pos_cur, (size_t)batch * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pn.p(), pos_next, (size_t)batch * 4, hipMemcpyHostToDevice));
    h.alloc((size_t)Mpad * d * 2, (size_t)16 * d * 2);
    x.alloc((size_t)Mpad * d * 2, (size_t)16 * d * 2);
    launch_whisper_embed_ln(de.p, dp.p, reinterpret_cast<const int32_t*>(di.p), da.p, reinterpret_cast<int*>(pc.p()), reinterpret_cast<int*>(pn.p()), dw.p, db.p,
                            reinterpret_cast<bf16_t*>(h.p()), reinterpret_cast<bf16_t*>(x.p()), d, vocab, max_pos, batch, Mpad, 0);
    enc_sync();
    pc.check_guards(); pn.check_guards(); h.check_guards(); x.check_guards();
    HIP_CHECK(hipMemcpy(pos_cur, pc.p(), (size_t)batch * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(pos_next, pn.p(), (size_t)batch * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h_out, h.p(), h.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(x_out, x.p(), x.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_whisper_suppress(int device, uint16_t* logits, int Vpad, int vocab, const int32_t* sup, int n_sup, const int32_t* bsup,
                                                 int n_bsup, const int32_t* n_gen, const uint8_t* active, int batch) {
    MIS_API_BEGIN
    MIS_REQUIRE(logits && n_gen && batch >= 1 && vocab >= 1 && Vpad >= vocab && (int64_t)batch * Vpad <= ENC_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "suppress: logits, n_gen, 1 <= vocab <= Vpad are required");
    MIS_REQUIRE(n_sup >= 0 && n_bsup >= 0 && n_sup <= 65536 && n_bsup <= 65536 && (n_sup == 0 || sup) && (n_bsup == 0 || bsup), MIS_ERR_INVALID_INPUT,
                "suppress: lists of 0 .. 65536 ids");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> ds, dbs, dg;
    DevBuf<uint8_t> da;
    alloc32(ds, sup, n_sup, 0xFFFFFFFFu);                          // an id read past a list is -1: ignored
    alloc32(dbs, bsup, n_bsup, 0xFFFFFFFFu);
    alloc32(dg, n_gen, batch, 1);
    if (active) alloc_bytes(da, active, batch);
    GuardedOut l;
    l.alloc((size_t)batch * Vpad * 2, (size_t)Vpad * 2);
    HIP_CHECK(hipMemcpy(l.p(), logits, l.body, hipMemcpyHostToDevice));
    launch_whisper_suppress(reinterpret_cast<bf16_t*>(l.p()), Vpad, vocab, reinterpret_cast<const int32_t*>(ds.p), n_sup, reinterpret_cast<const int32_t*>(dbs.p),
                            n_bsup, reinterpret_cast<const int32_t*>(dg.p), active ? da.p : nullptr, batch, 0);
    enc_sync();
    l.check_guards();
    HIP_CHECK(hipMemcpy(logits, l.p(), l.body, hipMemcpyDeviceToHost));
    MIS_API_END
}
