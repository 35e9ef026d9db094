// attn_debug.hip - test scaffolding (include/mi_speech_debug.h): ONE call of launch_attn_decode (lm_kernels.hip) on caller-supplied host
// data, so that tests/test_gpu_attn_ops.py can hold k_attn_decode<D, NIT, XS, QP> and k_attn_decode2<NS> to an operator-level reference.
//
// Nothing is computed here: the operands are uploaded as given - the K / V^T caches as raw images of the kernels' tiled layout, so that the
// caller decides what sits past kv_len and the layout is under test from the writer's side (the append) and the reader's (the main loop) -
// and everything the launch can write is copied back.  What makes a silent error visible (debug_guard.h, as gemm_debug.hip):
//   - the output, qp_h_out and both caches are allocated as [guard | body | guard], guards of the byte 0xFF (a NaN in bf16); the output
//     and qp_h_out bodies are filled with it too: an element the kernel never wrote comes back as NaN, a guard byte that changed fails
//     the call (MIS_ERR_GENERATION_FAILED), and a key or value read behind the last cache row is a NaN;
//   - every other input is followed by a guard of NaN (pos and active: zeros - inactive rows at position 0).
// The entry point refuses what would make the KERNEL write or read out of bounds (a position outside the cache, columns the slabs do not
// have): the launcher leaves those to the engines.  What the launcher itself checks is left to it - its status is returned.
#include <cstring>
#include "common.h"
#include "lm_kernels.h"
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

extern "C" mis_status mis_debug_attn_decode(int device, const mis_debug_attn_args* a) {
    MIS_API_BEGIN
    MIS_REQUIRE(a && a->pos && a->active && a->kcache && a->vtcache && a->kcache_out && a->vtcache_out && a->out, MIS_ERR_INVALID_INPUT,
                "attention: pos, active, both cache images and the outputs are required");
    if (a->report) { const int32_t none[6] = {-1, 0, 0, 0, 0, 0}; std::copy(none, none + 6, a->report); }
    const int B = a->batch, Mpad = a->Mpad, H = a->H, Hkv = a->Hkv, D = a->D, Smax = a->Smax;
    MIS_REQUIRE(B >= 1 && Mpad >= B && Mpad % 16 == 0 && Mpad <= 64 && H >= 1 && Hkv >= 1 && H <= 64 && (D == 64 || D == 128) && Smax >= 1 && Smax <= 4096,
                MIS_ERR_INVALID_INPUT, "attention: 1 <= batch <= Mpad <= 64 (a multiple of 16), head_dim 64 or 128, at most 4096 cache positions");
    const int HD = H * D, rows = a->cache_rows ? a->cache_rows : B;
    MIS_REQUIRE(a->cache_rows >= 0 && a->cache_rows <= B && a->S >= 0 && a->S <= 64 && a->qp_S >= 0 && a->qp_S <= 64, MIS_ERR_INVALID_INPUT,
                "attention: cache_rows 0 .. batch, slab counts 0 .. 64");
    MIS_REQUIRE(a->out_ld == 0 || a->out_ld >= HD, MIS_ERR_INVALID_INPUT, "attention: out_ld 0 (packed) or >= H D");
    MIS_REQUIRE(!a->rope_cos == !a->rope_sin && !a->qnorm_w == !a->knorm_w, MIS_ERR_INVALID_INPUT, "attention: cos and sin, q and k norm weights come in pairs");
    if (a->qp_w) {
        MIS_REQUIRE(a->qp_slabs && a->qp_h_in && a->qp_h_out && a->qp_lnw && a->qp_lnb, MIS_ERR_INVALID_INPUT, "attention: incomplete query-projection block");
    } else {
        MIS_REQUIRE(a->qkv_part && a->Nqkv % 4 == 0 && a->Nqkv >= (a->cross ? HD : HD + 2 * Hkv * D), MIS_ERR_INVALID_INPUT,
                    "attention: the slabs need %d columns", a->cross ? HD : HD + 2 * Hkv * D);
    }
    if (a->cross) {
        MIS_REQUIRE(a->cross_len >= 1 && a->cross_len <= Smax, MIS_ERR_INVALID_INPUT, "attention: cross_len 1 .. Smax");
    } else {
        for (int b = 0; b < B; ++b)
            MIS_REQUIRE(!a->active[b] || (a->pos[b] >= 0 && a->pos[b] < Smax), MIS_ERR_INVALID_INPUT, "attention: row %d at position %d of %d", b, a->pos[b], Smax);
    }
    HIP_CHECK(hipSetDevice(device));

    DevBuf<uint32_t> d_qkv, d_pos, d_cos, d_sin, d_slabs;
    DevBuf<uint8_t> d_act;
    DevBuf<uint16_t> d_qn, d_kn, d_wq, d_wsrc, d_qb, d_hin, d_lnw, d_lnb;
    AttnParams p{};
    p.S = a->S; p.Mpad = Mpad; p.Nqkv = a->Nqkv;
    if (a->qkv_part) {
        alloc32(d_qkv, a->qkv_part, (size_t)std::max(a->S, 1) * Mpad * a->Nqkv, F32_NAN);
        p.qkv_part = reinterpret_cast<const float*>(d_qkv.p);
    }
    alloc32(d_pos, a->pos, Mpad, 0);
    p.pos = reinterpret_cast<const int*>(d_pos.p);
    {
        std::vector<uint8_t> h((size_t)Mpad + IN_GUARD, 0);
        memcpy(h.data(), a->active, Mpad);
        d_act.alloc(h.size());
        HIP_CHECK(hipMemcpy(d_act.p, h.data(), h.size(), hipMemcpyHostToDevice));
        p.active = d_act.p;
    }
    if (a->rope_cos) {
        alloc32(d_cos, a->rope_cos, (size_t)Smax * (D / 2), F32_NAN);
        alloc32(d_sin, a->rope_sin, (size_t)Smax * (D / 2), F32_NAN);
        p.rope_cos = reinterpret_cast<const float*>(d_cos.p); p.rope_sin = reinterpret_cast<const float*>(d_sin.p);
    }
    if (a->qnorm_w) {
        alloc16(d_qn, a->qnorm_w, D, BF16_NAN); alloc16(d_kn, a->knorm_w, D, BF16_NAN);
        p.qnorm_w = d_qn.p; p.knorm_w = d_kn.p;
    }
    p.qk_eps = a->qk_eps; p.rope_in_dtype = a->rope_in_dtype; p.cross = a->cross; p.cross_len = a->cross_len; p.out_ld = a->out_ld;
    p.H = H; p.Hkv = Hkv; p.D = D; p.Smax = Smax; p.scale = a->scale;
    p.cache_rows = a->cache_rows; p.append_only = a->append_only; p.first_schedule = a->first_schedule;

    GuardedOut o, hq, kc, vc;
    const size_t ld = a->out_ld ? a->out_ld : HD;
    o.alloc((size_t)Mpad * ld * 2, (size_t)16 * ld * 2);
    p.out = reinterpret_cast<bf16_t*>(o.p());
    const size_t cache_el = (size_t)rows * Hkv * Smax * D;
    kc.alloc(cache_el * 2, (size_t)Smax * D * 2);                 // a guard is one (row, kv head) slice
    vc.alloc(cache_el * 2, (size_t)Smax * D * 2);
    HIP_CHECK(hipMemcpy(kc.p(), a->kcache, cache_el * 2, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(vc.p(), a->vtcache, cache_el * 2, hipMemcpyHostToDevice));
    p.kcache = reinterpret_cast<bf16_t*>(kc.p()); p.vtcache = reinterpret_cast<bf16_t*>(vc.p());
    if (a->qp_w) {
        MIS_REQUIRE(HD % 32 == 0, MIS_ERR_INVALID_INPUT, "attention: H D a multiple of 32");
        alloc16(d_wsrc, a->qp_w, (size_t)HD * HD, BF16_NAN);
        alloc16(d_wq, nullptr, (size_t)HD * HD, BF16_NAN);
        launch_pack_weight(d_wsrc.p, d_wq.p, HD, HD, HD / 16, 1, 0, 0);
        HIP_CHECK(hipDeviceSynchronize());
        p.qp_w = d_wq.p;
        if (a->qp_bias) { alloc16(d_qb, a->qp_bias, HD, BF16_NAN); p.qp_bias = d_qb.p; }
        alloc32(d_slabs, a->qp_slabs, (size_t)std::max(a->qp_S, 1) * Mpad * HD, F32_NAN);
        p.qp_slabs = reinterpret_cast<const float*>(d_slabs.p);
        alloc16(d_hin, a->qp_h_in, (size_t)Mpad * HD, BF16_NAN);
        alloc16(d_lnw, a->qp_lnw, HD, BF16_NAN); alloc16(d_lnb, a->qp_lnb, HD, BF16_NAN);
        p.qp_h_in = d_hin.p; p.qp_lnw = d_lnw.p; p.qp_lnb = d_lnb.p;
        hq.alloc((size_t)B * HD * 2, (size_t)16 * HD * 2);
        p.qp_h_out = reinterpret_cast<bf16_t*>(hq.p());
        p.qp_eps = a->qp_eps; p.qp_S = a->qp_S; p.qp_KT = a->qp_KT;
    }

    g_attn_last_launch = AttnLaunchInfo{};
    launch_attn_decode(p, B, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (a->report) {
        const AttnLaunchInfo& g = g_attn_last_launch;
        const int32_t r[6] = {g.kernel, g.D, g.NIT, g.XS, g.QP, g.NS};
        std::copy(r, r + 6, a->report);
    }
    o.check_guards(); kc.check_guards(); vc.check_guards();
    if (a->qp_w) hq.check_guards();

    std::vector<uint16_t> h((size_t)Mpad * ld);
    HIP_CHECK(hipMemcpy(h.data(), o.p(), o.body, hipMemcpyDeviceToHost));
    for (int m = 0; m < Mpad; ++m)
        for (size_t k = 0; k < ld; ++k) {
            const uint16_t v = h[a->out_ld ? (size_t)m * ld + k : xpk_index(m, (int)k, Mpad >> 4)];
            if (k < (size_t)HD) a->out[(size_t)m * HD + k] = bf16_to_f32(v);
            else MIS_REQUIRE(v == 0xFFFF, MIS_ERR_GENERATION_FAILED, "attention output: column %zu past the %d features was written", k, HD);
        }
    HIP_CHECK(hipMemcpy(a->kcache_out, kc.p(), cache_el * 2, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(a->vtcache_out, vc.p(), cache_el * 2, hipMemcpyDeviceToHost));
    if (a->qp_w) HIP_CHECK(hipMemcpy(a->qp_h_out, hq.p(), (size_t)B * HD * 2, hipMemcpyDeviceToHost));
    MIS_API_END
}
