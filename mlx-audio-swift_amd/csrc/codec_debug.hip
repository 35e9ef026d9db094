// codec_debug.hip - test scaffolding (include/mi_speech_debug.h): ONE call of a codec launcher of codec_kernels.h (launch_gemm with its four
// kernel families, launch_codec_final / _hist / _embed, launch_dw7, launch_vq_nearest) on caller-supplied host data, so that
// tests/test_gpu_codec_ops.py can hold the kernels to an operator-level reference.
//
// Nothing is computed here: the operands are uploaded as given and what the launch wrote is copied back.  What makes a silent error
// visible (debug_guard.h, as gemm_debug.hip and attn_debug.hip):
//   - every output is allocated as [guard | body | guard], all of it filled with the byte 0xFF (a float NaN, the code -1) before the
//     launch: an element the kernel never wrote comes back as NaN, a guard byte that changed fails the call (MIS_ERR_GENERATION_FAILED),
//     and so does a changed padding column of a strided output (columns >= Tout of a row of ldy);
//   - every input is followed by IN_GUARD NaNs (codes: 0xFF bytes); the activations, which kernels address at negative columns, are
//     preceded by as many, and every column of their row stride that holds neither history nor data is NaN: a read past Tin, or below
//     x_lo, lands in the result.
// The entry points refuse what would make a KERNEL read or write out of bounds (operands the mode needs, strides that do not hold the
// rows); what a launcher checks itself is left to it - its status is returned and nothing is launched.
#include <cstring>
#include "common.h"
#include "codec_kernels.h"
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

namespace {

const float* f32p(const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); }

// n floats (or NULL) behind alloc32's NaN guard
const float* up(DevBuf<uint32_t>& d, const float* src, size_t n) {
    if (!src) return nullptr;
    alloc32(d, src, n, F32_NAN);
    return f32p(d);
}

// activations: `rows` rows of `hist` history columns + `cols` data columns (dense on the host) -> [IN_GUARD NaN | lead | rows x ld | IN_GUARD
// NaN] with column 0 of row r at IN_GUARD + lead + r ld (lead = hist rounded up to 4 floats: 16-byte aligned rows when ld % 4 == 0);
// everything that is not history or data is NaN.  Returns the pointer to column 0 of row 0
const float* up_rows(DevBuf<uint32_t>& d, const float* src, size_t rows, int hist, int cols, int ld) {
    const size_t lead = round_up(hist, 4), w = (size_t)hist + cols;
    std::vector<uint32_t> h(2 * IN_GUARD + lead + rows * ld, F32_NAN);
    for (size_t r = 0; r < rows; ++r) memcpy(&h[IN_GUARD + lead + r * ld - hist], src + r * w, w * 4);
    d.alloc(h.size());
    HIP_CHECK(hipMemcpy(d.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    return f32p(d) + IN_GUARD + lead;
}

// rows x ld words of a guarded output -> the first `cols` of every row; the columns behind must still hold the fill
void fetch_rows(GuardedOut& o, size_t rows, int ld, int cols, void* out) {
    o.check_guards();
    std::vector<uint32_t> h(o.body / 4);
    HIP_CHECK(hipMemcpy(h.data(), o.p(), o.body, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        memcpy(static_cast<uint32_t*>(out) + r * cols, &h[r * ld], (size_t)cols * 4);
        for (int c = cols; c < ld && r * ld + c < h.size(); ++c)
            MIS_REQUIRE(h[r * ld + c] == 0xFFFFFFFFu, MIS_ERR_GENERATION_FAILED, "the kernel wrote column %d of row %zu behind its %d columns", c, r, cols);
    }
}

void sync_launch() {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
}

constexpr int64_t MAX_ELEMS = (int64_t)1 << 28;          // per tensor: the kernels index some of them with 32-bit products

}  // namespace

extern "C" mis_status mis_debug_codec_gemm(int device, const mis_debug_codec_gemm_args* a) {
    MIS_API_BEGIN
    MIS_REQUIRE(a && a->AT && a->X && a->Y, MIS_ERR_INVALID_INPUT, "codec GEMM: A^T, X and Y are required");
    if (a->report) { const int32_t none[6] = {-1, 0, 0, 0, 0, 0}; std::copy(none, none + 6, a->report); }
    const int mode = a->mode, B = a->batch, M = a->M, K = a->K, N = a->N, Tin = a->Tin, Tout = a->Tout;
    MIS_REQUIRE(mode >= GEMM_PLAIN && mode <= GEMM_TAPS && B >= 1 && M >= 1 && K >= 1 && N >= 1 && Tin >= 1 && Tout >= 1, MIS_ERR_INVALID_INPUT,
                "codec GEMM: mode 0 .. 5, batch, M, K, N, Tin, Tout >= 1");
    const bool one = mode == GEMM_PLAIN || mode == GEMM_GELU || mode == GEMM_RESID || mode == GEMM_NOISE;
    const int Kx = one ? K : a->Cin, hist = a->x_lo < 0 ? -a->x_lo : 0;
    const int ldx = a->ldx ? a->ldx : Tin, ldy = a->ldy ? a->ldy : Tout;
    MIS_REQUIRE(ldx >= hist + Tin && ldy >= Tout, MIS_ERR_INVALID_INPUT, "codec GEMM: ldx holds history + Tin columns, ldy holds Tout");
    if (one) {
        // the 1x1 kernels write columns [0, N) of Y, read R there, and k_pw_fused reads X up to N without looking at Tin
        MIS_REQUIRE(N <= Tout && N <= Tin, MIS_ERR_INVALID_INPUT, "codec GEMM: a 1x1 mode covers N <= Tin, Tout columns");
        MIS_REQUIRE(mode != GEMM_RESID || a->R, MIS_ERR_INVALID_INPUT, "codec GEMM: the residual mode needs R");
        MIS_REQUIRE(mode != GEMM_NOISE || M <= K, MIS_ERR_INVALID_INPUT, "codec GEMM: the noise mode reads X rows [0, M)");
        // k_snac_gemm<RESID, true> reads alpha unconditionally (the other 1x1 modes have no Snake prologue: launch_gemm ignores the flag)
        MIS_REQUIRE(!a->snake || mode != GEMM_RESID || (a->alpha && a->ralpha), MIS_ERR_INVALID_INPUT,
                    "codec GEMM: Snake in front of the residual mode reads alpha and ralpha");
        MIS_REQUIRE(!a->alpha == !a->ralpha, MIS_ERR_INVALID_INPUT, "codec GEMM: alpha and ralpha come in pairs");
    } else {
        MIS_REQUIRE(Kx >= 1 && K % Kx == 0 && a->pad >= 0, MIS_ERR_INVALID_INPUT, "codec GEMM: K a multiple of Cin, pad >= 0");
        if (mode == GEMM_TAPS) {
            MIS_REQUIRE(a->taps >= 1 && a->dil >= 1 && K == a->taps * Kx && N <= Tout, MIS_ERR_INVALID_INPUT, "codec GEMM: K = taps Cin, dil >= 1, N <= Tout");
            MIS_REQUIRE(!a->alpha == !a->ralpha, MIS_ERR_INVALID_INPUT, "codec GEMM: alpha and ralpha come in pairs");
        } else {
            MIS_REQUIRE(a->s >= 1 && (!a->snake || (a->alpha && a->ralpha)), MIS_ERR_INVALID_INPUT, "codec GEMM: stride >= 1; the transposed conv reads alpha and ralpha");
        }
    }
    MIS_REQUIRE((int64_t)B * Kx * ldx <= MAX_ELEMS && (int64_t)B * M * ldy <= MAX_ELEMS && (int64_t)(mode == GEMM_CONVT ? a->s : 1) * K * M <= MAX_ELEMS,
                MIS_ERR_INVALID_INPUT, "codec GEMM: tensor too large for the debug entry point");
    HIP_CHECK(hipSetDevice(device));

    DevBuf<uint32_t> d_at, d_bias, d_x, d_r, d_scale, d_noise, d_al, d_ral, d_ids;
    CodecPack pack;
    GemmParams p{};
    p.pack = a->use_pack ? &pack : nullptr;
    p.AT = up(d_at, a->AT, (size_t)(mode == GEMM_CONVT ? a->s : 1) * K * M);
    p.bias = up(d_bias, a->bias, M);
    p.X = up_rows(d_x, a->X, (size_t)B * Kx, hist, Tin, ldx);
    if (a->R) p.R = up_rows(d_r, a->R, (size_t)B * M, 0, Tout, ldy);
    p.scale = up(d_scale, a->scale, M);
    p.noise = up(d_noise, a->noise, (size_t)B * N);
    p.noise_rng = a->noise_rng; p.noise_key = a->noise_key; p.row_offset = a->row_offset;
    if (a->row_ids) { alloc32(d_ids, a->row_ids, B, 0); p.row_ids = reinterpret_cast<const int32_t*>(d_ids.p); }
    p.alpha = up(d_al, a->alpha, Kx); p.ralpha = up(d_ral, a->ralpha, Kx);
    p.M = M; p.K = K; p.N = N; p.Tin = Tin; p.Tout = Tout; p.s = a->s; p.pad = a->pad; p.Cin = a->Cin;
    p.ldx = a->ldx; p.ldy = a->ldy; p.x_lo = a->x_lo; p.dup_bias_n0 = a->dup_bias_n0; p.split_k_ok = a->split_k_ok;
    p.taps = a->taps; p.dil = a->dil;
    GuardedOut o;
    o.alloc((size_t)B * M * ldy * 4, (size_t)128 * ldy * 4);     // a whole 128-row block tile of rows >= M would still land in it
    p.Y = reinterpret_cast<float*>(o.p());

    g_codec_last_launch = CodecLaunchInfo{};
    launch_gemm(mode, a->snake != 0, p, B, 0);
    sync_launch();
    if (a->report) {
        const CodecLaunchInfo& g = g_codec_last_launch;
        const int32_t r[6] = {g.kernel, g.ntaps, g.NQ, g.ksplit, g.Tp, g.Cp};
        std::copy(r, r + 6, a->report);
    }
    fetch_rows(o, (size_t)B * M, ldy, Tout, a->Y);
    MIS_API_END
}

extern "C" mis_status mis_debug_codec_final(int device, const float* x, const float* w, float bias, const float* a, const float* ra, int C, int T, int ld,
                                            int x_lo, int k, int batch, int64_t out_stride, float* out) {
    MIS_API_BEGIN
    const int hist = x_lo < 0 ? -x_lo : 0;
    MIS_REQUIRE(x && w && out && !a == !ra && C >= 1 && T >= 1 && batch >= 1 && k >= 1 && ld >= hist + T && x_lo <= 0 && out_stride >= T,
                MIS_ERR_INVALID_INPUT, "codec final: x, w, out; a and ra in pairs; ld holds history + T columns; out_stride >= T");
    MIS_REQUIRE((int64_t)batch * C * ld <= MAX_ELEMS && (int64_t)batch * out_stride <= MAX_ELEMS && k <= 64, MIS_ERR_INVALID_INPUT, "codec final: too large");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> d_x, d_w, d_a, d_ra;
    const float* dx = up_rows(d_x, x, (size_t)batch * C, hist, T, ld);
    const float* dw = up(d_w, w, (size_t)k * C);
    const float* da = up(d_a, a, C);
    const float* dra = up(d_ra, ra, C);
    GuardedOut o;
    o.alloc((size_t)batch * out_stride * 4, (size_t)out_stride * 4);
    launch_codec_final(dx, reinterpret_cast<float*>(o.p()), out_stride, dw, bias, da, dra, C, T, ld, x_lo, k, batch, 0);
    sync_launch();
    fetch_rows(o, batch, (int)out_stride, T, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_codec_hist(int device, const float* st, const float* x_img, int C, int ld, int H, int Tn, int batch, float* st_out,
                                           float* x_out) {
    MIS_API_BEGIN
    MIS_REQUIRE((H == 0 || (st && st_out)) && x_img && x_out && C >= 1 && batch >= 1 && H >= 0 && H <= 4096 && Tn >= 1 && ld >= H + Tn, MIS_ERR_INVALID_INPUT,
                "codec hist: st, the x image and both outputs; ld holds H + Tn columns");
    MIS_REQUIRE((int64_t)batch * C * ld <= MAX_ELEMS, MIS_ERR_INVALID_INPUT, "codec hist: too large");
    HIP_CHECK(hipSetDevice(device));
    const size_t n_st = (size_t)batch * C * H, n_x = (size_t)batch * C * ld;
    GuardedOut s, x;
    s.alloc(n_st * 4, (size_t)(H + 64) * 4);
    x.alloc(n_x * 4, (size_t)ld * 4);
    if (n_st) HIP_CHECK(hipMemcpy(s.p(), st, n_st * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(x.p(), x_img, n_x * 4, hipMemcpyHostToDevice));
    launch_codec_hist(reinterpret_cast<float*>(s.p()), reinterpret_cast<float*>(x.p()) + H, C, ld, H, Tn, batch, 0);
    sync_launch();
    s.check_guards(); x.check_guards();
    if (n_st) HIP_CHECK(hipMemcpy(st_out, s.p(), n_st * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(x_out, x.p(), n_x * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_codec_embed(int device, const int32_t* codes, int64_t n_codes, int64_t cs_b, int64_t cs_q, int64_t cs_t,
                                            const float* tables, int nq, int bins, int C, int ld, int T, int batch, float* h) {
    MIS_API_BEGIN
    MIS_REQUIRE(codes && tables && h && nq >= 1 && bins >= 1 && C >= 1 && T >= 1 && batch >= 1 && ld >= T && cs_b >= 0 && cs_q >= 0 && cs_t >= 0,
                MIS_ERR_INVALID_INPUT, "codec embed: codes, tables, h; non-negative code strides; ld >= T");
    MIS_REQUIRE((batch - 1) * cs_b + (nq - 1) * cs_q + (T - 1) * cs_t < n_codes && n_codes <= MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "codec embed: the strides address codes behind the %lld given", (long long)n_codes);
    MIS_REQUIRE((int64_t)nq * bins * C <= MAX_ELEMS && (int64_t)batch * C * ld <= MAX_ELEMS, MIS_ERR_INVALID_INPUT, "codec embed: too large");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> d_codes, d_tab;
    alloc32(d_codes, codes, (size_t)n_codes, 0xFFFFFFFFu);
    const float* dt = up(d_tab, tables, (size_t)nq * bins * C);
    GuardedOut o;
    o.alloc((size_t)batch * C * ld * 4, (size_t)ld * 4);
    launch_codec_embed(reinterpret_cast<const int32_t*>(d_codes.p), cs_b, cs_q, cs_t, dt, reinterpret_cast<float*>(o.p()), nq, bins, C, ld, T, batch, 0);
    sync_launch();
    fetch_rows(o, (size_t)batch * C, ld, T, h);
    MIS_API_END
}

extern "C" mis_status mis_debug_codec_dw7(int device, const float* X, const float* w7, const float* bias, int batch, int C, int T, int dil, float* Y) {
    MIS_API_BEGIN
    MIS_REQUIRE(X && w7 && bias && Y && batch >= 1 && C >= 1 && T >= 1 && dil >= 1 && dil <= 9 && (int64_t)batch * C * T <= MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "depthwise conv: X, w7, bias, Y; dilation 1 .. 9 (the tile's halo)");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> d_x, d_w, d_b;
    const float* dx = up_rows(d_x, X, (size_t)batch * C, 0, T, T);
    const float* dw = up(d_w, w7, (size_t)C * 7);
    const float* db = up(d_b, bias, C);
    GuardedOut o;
    o.alloc((size_t)batch * C * T * 4, (size_t)T * 4);
    launch_dw7(dx, reinterpret_cast<float*>(o.p()), dw, db, batch, C, T, dil, 0);
    sync_launch();
    fetch_rows(o, (size_t)batch * C, T, T, Y);
    MIS_API_END
}

extern "C" mis_status mis_debug_codec_vq_nearest(int device, const float* ze, const float* cn, const float* cn2, int batch, int CD, int CB, int Tm,
                                                 int32_t* codes_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(ze && cn && cn2 && codes_out && batch >= 1 && CD >= 1 && CB >= 1 && Tm >= 1 && (int64_t)batch * CD * Tm <= MAX_ELEMS &&
                    (int64_t)CB * CD <= MAX_ELEMS, MIS_ERR_INVALID_INPUT, "nearest code: ze, cn, cn2, codes_out");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> d_ze, d_cn, d_cn2;
    const float* dz = up(d_ze, ze, (size_t)batch * CD * Tm);
    const float* dc = up(d_cn, cn, (size_t)CB * CD);
    const float* dc2 = up(d_cn2, cn2, CB);
    GuardedOut o;
    o.alloc((size_t)batch * Tm * 4, 1024);
    launch_vq_nearest(dz, dc, dc2, reinterpret_cast<int32_t*>(o.p()), batch, CD, CB, Tm, 0);
    sync_launch();
    fetch_rows(o, batch, Tm, Tm, codes_out);
    MIS_API_END
}
