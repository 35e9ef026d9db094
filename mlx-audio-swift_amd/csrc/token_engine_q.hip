// token_engine_q.hip - the batch-1 token engine (token_engine.hip) on MLX affine-quantised checkpoints: the same persistent launch, with
// the matrix waves streaming the LM's packed CODES (8 or 4 bit, group 64, bf16 scales) instead of bf16 tiles.
//
// Reference being replaced: QuantizedLinear -> quantizedMatmul (SopranoModel.fromPretrained quantises every module with a `.scales`
// companion, Soprano.swift:949-963); arithmetic as csrc/lm_qgemm.hip: per 64-wide group y += scale * sum_k(x_k q_k) + bias * sum_k(x_k)
// in float32.  Here the codes are widened to bf16 (exact) and run through v_mfma_f32_16x16x32_bf16 against the engine's x fragments, one
// float32 accumulator per group (= two k-tiles); sum_k x_k of a group comes from one MFMA pair against an all-ones A tile; the group's
// scale and bias are applied on the four output lanes, then the partials go through `red` / te_combine exactly as the dense kernel's.
// Everything else - vector waves, edges, attention, sampler, relay, rounding points - is the shared program of token_engine_impl.h.
//
// Why: the engine is bound by hand-off latency, not bytes ("Batch-1 token engine"), so streaming 0.53x / 0.28x of the bf16
// bytes costs nothing per position, while a quantised checkpoint on the launch chain pays ~2.3x per token.
//
// Layouts (lm_engine.hip place_qmatrix, lm_qgemm.hip k_pack_qweight): codes [NT][KT][64 lanes][8 codes] - the engine's bf16 tile order
// with codes for values - so tile ids, k ranges and pieces are the dense kernel's; scale / bias pairs [NT][G][2][16] bf16, a lane of
// row group q = lane >> 4 reads the four rows 4q .. 4q + 3 of its C/D fragment as 8 bytes.  Registers per (tile row, k-tile): 2 (8 bit)
// or 1 (4 bit) instead of 4, plus 4 per (tile row, group) for the scale / bias pair: at most the dense kernel's 4 per tile.
//
// Accepted (token_engine_supports): q|k|v, o_proj, gate|up and down all streamed with ONE width B in {8, 4}; the output projection
// streamed with the same B (HQ) or dense (tied embeddings, or a bf16 / dequantised-at-load lm_head).
// Tests: tests/test_gpu_token_engine_quant.py, tests/test_gpu_soprano_quant.py, tests/test_isa_token_engine_q_cpu.py (register budget).
#include "token_engine_impl.h"
#include "lm_qcodes.h"

namespace {
// every matrix wave's K range must cut at scale groups: TE_MW waves x KPW k-tiles, KPW even (two k-tiles per 64-wide group)
template <int KT>
struct TeQSplit {
    static_assert(KT % TE_MW == 0 && (KT / TE_MW) % 2 == 0, "a matrix wave's K range must hold whole scale groups");
    static constexpr int KPW = KT / TE_MW;
};
static_assert(TeQSplit<TeShape::d / 32>::KPW == TeDims<1>::KPW_D && TeQSplit<TeShape::HD / 32>::KPW == TeDims<1>::KPW_HD &&
              TeQSplit<TeShape::ff / 32>::KPW == TeDims<1>::KPW_FF, "the dense kernel's k ranges are the code kernel's");

template <int R, int KPW, int B>
struct TeQTiles {
    typename QTile<B>::type a[R][KPW];     // this lane's 8 codes of tile (row r, k-tile u)
    u32x2_t sb[R][KPW / 2][2];              // scale, bias of rows 4 (lane >> 4) .. + 3, group u / 2 (four bf16 each)
    bf16x8_t wn[KPW];
};
// as te_load: tiles FROM .. TO - 1 of the flattened list f = u R + r; a group's scale / bias pair travels with its first k-tile.
// nt_cap: code tiles of the matrix (the output projection's vocabulary tiles past it are clamped - their ids are >= V and never read)
template <int R, int KPW, int B, bool NORM, int FROM = 0, int TO = R * KPW>
__device__ __forceinline__ void te_qload(TeQTiles<R, KPW, B>& T, const uint8_t* Qp, const bf16_t* SBp, const int KT, const int (&nt)[R],
                                         const int nt_cap, const bf16_t* wnorm, const int mw, const int lane) {
    typedef typename QTile<B>::type CT;
    const int kt0 = mw * KPW, G = KT / 2;
    const unsigned voff = (unsigned)lane * (unsigned)B;                    // 8 codes of B bits
    const unsigned soff = (unsigned)(lane >> 4) * 8u;
#pragma unroll
    for (int u = 0; u < KPW; ++u) {
        const int kk = kt0 + u;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (u * R + r < FROM || u * R + r >= TO) continue;
            int tile = nt[r] < 0 ? 0 : nt[r];
            tile = tile < nt_cap ? tile : nt_cap - 1;
            const uint8_t* base = Qp + ((size_t)tile * KT + kk) * (64 * B);                           // wave-uniform
            T.a[r][u] = __builtin_nontemporal_load(reinterpret_cast<const CT*>(base + voff));
            if ((u & 1) == 0) {
                const uint8_t* sbase = reinterpret_cast<const uint8_t*>(SBp) + ((size_t)tile * G + (kk >> 1)) * 64;
                T.sb[r][u >> 1][0] = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(sbase + soff));
                T.sb[r][u >> 1][1] = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(sbase + 32 + soff));
            }
        }
        if (NORM && u * R >= FROM && u * R < TO) {
            const char* nb = reinterpret_cast<const char*>(wnorm) + (size_t)kk * 64;
            T.wn[u] = *reinterpret_cast<const bf16x8_t*>(nb + (unsigned)(lane >> 4) * 16u);
        }
    }
}
// y = W x on codes: per group g the two k-tiles' MFMAs into a fresh accumulator, then y += scale * acc + bias * sum(x) (float32, group
// order); the partial sums land in `red` as te_mma's do
template <int R, int KPW, int B>
__device__ __forceinline__ void te_qmma(const TeQTiles<R, KPW, B>& T, const bf16x8_t (&xf)[KPW], float* red, const int mw, const int lane) {
    constexpr int RB = R > 5 ? 5 : R, NG = KPW / 2;
    const int g = lane >> 4;
    bf16x8_t ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (short)0x3F80;                    // bf16 1.0
    float sx[NG];                                                          // sum of x over group gi (the same for every row: column 0 of D)
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
        f32x4_t s = {0.f, 0.f, 0.f, 0.f};
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, xf[2 * gi], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, xf[2 * gi + 1], s, 0, 0, 0);
        sx[gi] = s[0];
    }
#pragma unroll
    for (int r0 = 0; r0 < R; r0 += RB) {
        f32x4_t y[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) y[r] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int gi = 0; gi < NG; ++gi)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r0 + r >= R) continue;
                f32x4_t ag = {0.f, 0.f, 0.f, 0.f};
                ag = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dq_codes(T.a[r0 + r][2 * gi]), xf[2 * gi], ag, 0, 0, 0);
                ag = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dq_codes(T.a[r0 + r][2 * gi + 1]), xf[2 * gi + 1], ag, 0, 0, 0);
                const u32x2_t s2 = T.sb[r0 + r][gi][0], b2 = T.sb[r0 + r][gi][1];
                const float sc[4] = {sb_to_f32<0>(s2.x), sb_to_f32<0>(s2.x >> 16), sb_to_f32<0>(s2.y), sb_to_f32<0>(s2.y >> 16)};
                const float bi[4] = {sb_to_f32<0>(b2.x), sb_to_f32<0>(b2.x >> 16), sb_to_f32<0>(b2.y), sb_to_f32<0>(b2.y >> 16)};
#pragma unroll
                for (int e = 0; e < 4; ++e) y[r][e] += sc[e] * ag[e] + bi[e] * sx[gi];
            }
        if ((lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (r0 + r < R) *reinterpret_cast<f32x4_t*>(red + ((size_t)(mw * R + r0 + r) * 16 + 4 * g)) = y[r];
        }
    }
    __builtin_amdgcn_sched_barrier(0);                                     // (as te_mma: the next phase's requests stay behind the MFMAs)
}

// ---------------------------------------------------------------------------- the matrix waves' program on codes: te_matrix_role of
// token_engine.hip phase by phase (same barriers, same pieces, same opaque ids), tile loads and MFMAs of te_qload / te_qmma.  HQ: the
// output projection streamed as codes too; else its dense bf16 tiles (te_load / te_mma).
template <int XCDS, int B, bool HQ>
__device__ __forceinline__ void te_matrix_role_q(const TeParams& p, const TeQParams& q, const TeLds& L, const int w_in, const int mw_in,
                                                 const int lane) {
    using S = TeShape;
    using Dm = TeDims<XCDS>;
    constexpr int W = Dm::W, R_QKV = Dm::R_QKV, R_O = Dm::R_O, P_GU = Dm::P_GU, R_GU = Dm::R_GU, R_HEAD = Dm::R_HEAD;
    constexpr int KPW_D = TeQSplit<S::d / 32>::KPW, KPW_HD = TeQSplit<S::HD / 32>::KPW, KPW_FF = TeQSplit<S::ff / 32>::KPW;
    constexpr int NT_ALL = 1 << 30;                                          // (no clamp: every layer role has whole tiles)
    const int NTV = p.Vpad / 16;
#define TE_OPAQUE_IDS() int wq = w_in, mw = mw_in; asm volatile("" : "+s"(wq), "+s"(mw))
#define TE_ROWS_QKV(NT) int NT[R_QKV]; _Pragma("unroll") for (int r = 0; r < R_QKV; ++r) NT[r] = (wq + r * W) < S::Nqkv / 16 ? wq + r * W : -1
#define TE_ROWS_O(NT) int NT[R_O]; _Pragma("unroll") for (int r = 0; r < R_O; ++r) NT[r] = (wq + r * W) < S::d / 16 ? wq + r * W : -1
#define TE_ROWS_GU(NT) int NT[R_GU]; _Pragma("unroll") for (int r = 0; r < P_GU; ++r) { const int pr = wq + r * W;                       \
        NT[2 * r] = pr < S::ff / 16 ? 2 * pr : -1; NT[2 * r + 1] = pr < S::ff / 16 ? 2 * pr + 1 : -1; }
#define TE_ROWS_HEAD(NT, PASS) int NT[R_HEAD]; _Pragma("unroll") for (int r = 0; r < R_HEAD; ++r)                                      \
        NT[r] = (wq + ((PASS) * R_HEAD + r) * W) < NTV ? wq + ((PASS) * R_HEAD + r) * W : -1
#define TE_CUT(N, a, b) ((N) * (a) / 40), ((N) * (b) / 40)
    constexpr int N_G = R_GU * KPW_D;
    using HeadTiles = std::conditional_t<HQ, TeQTiles<R_HEAD, KPW_D, B>, TeTiles<R_HEAD, KPW_D>>;
    auto head_load = [&](HeadTiles& th, const int (&nt)[R_HEAD], const bf16_t* wnorm, const int mw_, auto norm) {
        if constexpr (HQ) te_qload<R_HEAD, KPW_D, B, decltype(norm)::value>(th, q.head.q, q.head.sb, S::d / 32, nt, q.head_nt, wnorm, mw_, lane);
        else te_load<R_HEAD, KPW_D, decltype(norm)::value>(th, p.head, S::d / 32, nt, wnorm, mw_, lane);
    };
    auto head_mma = [&](const HeadTiles& th, const bf16x8_t (&xf)[KPW_D], const int mw_) {
        if constexpr (HQ) te_qmma<R_HEAD, KPW_D, B>(th, xf, L.red, mw_, lane);
        else te_mma<R_HEAD, KPW_D>(th, xf, L.red, mw_, lane);
    };
    TeQTiles<R_QKV, KPW_D, B> tq;
    {
        TE_OPAQUE_IDS();
        TE_ROWS_QKV(nt);
        te_qload<R_QKV, KPW_D, B, true>(tq, q.qkv.q, q.qkv.sb, S::d / 32, nt, NT_ALL, p.norms, mw, lane);
    }
    for (int t = p.t_start; t < p.n_total; ++t) {
        te_sync();                                                   // token id
        if (*L.s_done) return;
        te_sync();                                                   // embedding row + sum of squares
        const bool do_head = t >= p.head_from && t < p.head_until;
        for (int li = 0; li < p.L; ++li) {
            TeQTiles<R_O, KPW_HD, B> to;
            TeQTiles<R_GU, KPW_D, B> tg;
            TeQTiles<R_O, KPW_FF, B> td;
            const uint8_t* gq_l = q.gu.q + (size_t)li * q.gu.q_layer;
            const bf16_t* gs_l = q.gu.sb + (size_t)li * q.gu.sb_layer;
            const bf16_t* n2_l = p.norms + (size_t)(2 * li + 1) * S::d;
            if (li > 0) {
                te_sync();                                           // (previous layer) edge 4: residual stream gathered
                if (!*L.s_ok) return;
            }
            {   // q|k|v; then o_proj's tiles and the first quarter of gate|up's
                TE_OPAQUE_IDS();
                const float inv = rsqrtf(((L.s_ss[0] + L.s_ss[1]) + (L.s_ss[2] + L.s_ss[3])) / (float)S::d + p.eps);
                bf16x8_t xf[KPW_D];
                te_xfrag_norm<KPW_D>(xf, L.hf, tq.wn, inv, S::d / 32, mw, lane);
                te_qmma<R_QKV, KPW_D, B>(tq, xf, L.red, mw, lane);
                te_sync();                                           // red ready
                TE_ROWS_O(nt);
                te_qload<R_O, KPW_HD, B, false>(to, q.o.q + (size_t)li * q.o.q_layer, q.o.sb + (size_t)li * q.o.sb_layer, S::HD / 32, nt, NT_ALL,
                                                nullptr, mw, lane);
                TE_ROWS_GU(ng);
                te_qload<R_GU, KPW_D, B, true, TE_CUT(N_G, 0, 10)>(tg, gq_l, gs_l, S::d / 32, ng, NT_ALL, n2_l, mw, lane);
                te_sync();                                           // edge 1: q|k|v gathered
                if (!*L.s_ok) return;
                te_qload<R_GU, KPW_D, B, true, TE_CUT(N_G, 10, 16)>(tg, gq_l, gs_l, S::d / 32, ng, NT_ALL, n2_l, mw, lane);
                te_sync();                                           // q/k-norm + RoPE
                te_qload<R_GU, KPW_D, B, true, TE_CUT(N_G, 16, 28)>(tg, gq_l, gs_l, S::d / 32, ng, NT_ALL, n2_l, mw, lane);
                te_sync();                                           // scores
                te_qload<R_GU, KPW_D, B, true, TE_CUT(N_G, 28, 34)>(tg, gq_l, gs_l, S::d / 32, ng, NT_ALL, n2_l, mw, lane);
                te_sync();                                           // softmax
                te_qload<R_GU, KPW_D, B, true, TE_CUT(N_G, 34, 40)>(tg, gq_l, gs_l, S::d / 32, ng, NT_ALL, n2_l, mw, lane);
                te_sync();                                           // attention output ready
            }
            {   // o_proj
                TE_OPAQUE_IDS();
                bf16x8_t xf[KPW_HD];
                te_xfrag_bf16<KPW_HD>(xf, L.xb, S::HD / 32, mw, lane);
                te_qmma<R_O, KPW_HD, B>(to, xf, L.red, mw, lane);
                te_sync();                                           // red ready
            }
            te_sync();                                               // edge 2: residual stream gathered
            if (!*L.s_ok) return;
            {   // gate|up; then down_proj's tiles
                TE_OPAQUE_IDS();
                const float inv = rsqrtf(((L.s_ss[0] + L.s_ss[1]) + (L.s_ss[2] + L.s_ss[3])) / (float)S::d + p.eps);
                bf16x8_t xf[KPW_D];
                te_xfrag_norm<KPW_D>(xf, L.hf, tg.wn, inv, S::d / 32, mw, lane);
                te_qmma<R_GU, KPW_D, B>(tg, xf, L.red, mw, lane);
                te_sync();                                           // red ready
                TE_ROWS_O(nt);
                te_qload<R_O, KPW_FF, B, false>(td, q.down.q + (size_t)li * q.down.q_layer, q.down.sb + (size_t)li * q.down.sb_layer, S::ff / 32, nt,
                                                NT_ALL, nullptr, mw, lane);
                te_sync();                                           // edge 3: activation gathered
                if (!*L.s_ok) return;
            }
            {   // down; then the next layer's q|k|v tiles
                TE_OPAQUE_IDS();
                bf16x8_t xf[KPW_FF];
                te_xfrag_bf16<KPW_FF>(xf, L.xb, S::ff / 32, mw, lane);
                te_qmma<R_O, KPW_FF, B>(td, xf, L.red, mw, lane);
                te_sync();                                           // red ready
                if (li + 1 < p.L) {
                    TE_ROWS_QKV(nt);
                    te_qload<R_QKV, KPW_D, B, true>(tq, q.qkv.q + (size_t)(li + 1) * q.qkv.q_layer, q.qkv.sb + (size_t)(li + 1) * q.qkv.sb_layer,
                                                    S::d / 32, nt, NT_ALL, p.norms + (size_t)(2 * li + 2) * S::d, mw, lane);
                }
            }
        }
        if (!do_head) {
            TE_OPAQUE_IDS();
            TE_ROWS_QKV(nt);
            te_qload<R_QKV, KPW_D, B, true>(tq, q.qkv.q, q.qkv.sb, S::d / 32, nt, NT_ALL, p.norms, mw, lane);
            te_sync();                                               // (last layer) edge 4: residual stream gathered
            if (!*L.s_ok) return;
        } else {
            HeadTiles th;
            int mw_h;
            {
                TE_OPAQUE_IDS();
                mw_h = mw;
                TE_ROWS_HEAD(nth, 0);
                head_load(th, nth, p.norms + (size_t)(2 * p.L) * S::d, mw, std::true_type{});
                te_sync();                                           // (last layer) edge 4: residual stream gathered
                if (!*L.s_ok) return;
            }
            const float inv = rsqrtf(((L.s_ss[0] + L.s_ss[1]) + (L.s_ss[2] + L.s_ss[3])) / (float)S::d + p.eps);
            bf16x8_t xf[KPW_D];
            te_xfrag_norm<KPW_D>(xf, L.hf, th.wn, inv, S::d / 32, mw_h, lane);
            for (int pass = 0; pass * R_HEAD * W < NTV; ++pass) {
                TE_OPAQUE_IDS();
                head_mma(th, xf, mw);
                te_sync();                                           // red ready
                if ((pass + 1) * R_HEAD * W < NTV) {
                    TE_ROWS_HEAD(nt2, pass + 1);
                    head_load(th, nt2, nullptr, mw, std::false_type{});
                } else {
                    TE_ROWS_QKV(nt);
                    te_qload<R_QKV, KPW_D, B, true>(tq, q.qkv.q, q.qkv.sb, S::d / 32, nt, NT_ALL, p.norms, mw, lane);     // layer 0 of the next position
                }
                te_sync();                                           // red consumed
            }
            te_sync();                                               // candidates of the vector waves
            te_sync();                                               // edge 5: candidates (arg-max) / maxima (sampling) gathered
            if (!*L.s_ok) return;
            if (p.sample == 1) {
                te_sync();                                           // edge 6: tile masses gathered
                if (!*L.s_ok) return;
                te_sync(); te_sync();                                // scan of the tile masses: wave totals, the chosen tile
                te_sync();                                           // edge 7: the token
                if (!*L.s_ok) return;
            } else if (p.sample == 2) {
                te_sync();                                           // the waves' id candidates
                te_sync();                                           // edge 6: the id
                if (!*L.s_ok) return;
            }
        }
    }
#undef TE_OPAQUE_IDS
#undef TE_ROWS_QKV
#undef TE_ROWS_O
#undef TE_ROWS_GU
#undef TE_ROWS_HEAD
#undef TE_CUT
}

template <int XCDS, int B, bool HQ>
__global__ void __launch_bounds__(TE_NT) k_token_engine_q(TeParams p, TeQParams q) {
    using S = TeShape;
    using Dm = TeDims<XCDS>;
    static_assert(S::H == TE_VW && S::Hkv == 1 && S::D == 128 && S::d / 4 <= 128 && S::Nqkv / 4 <= TE_VW * 64, "vector-wave mapping of the engine");
    extern __shared__ __attribute__((aligned(16))) unsigned char te_lds_pad[];      // (requested size keeps the launch at one block per CU)
    __shared__ __attribute__((aligned(16))) float hf[S::d];
    __shared__ __attribute__((aligned(16))) bf16_t xb[S::ff > S::HD ? S::ff : S::HD];
    __shared__ __attribute__((aligned(16))) float qkvf[S::Nqkv];
    __shared__ __attribute__((aligned(16))) float qh[S::H * S::D];
    __shared__ __attribute__((aligned(16))) float knew[S::D], vnew[S::D];
    __shared__ __attribute__((aligned(16))) float sc[S::H * TE_CTX];
    __shared__ __attribute__((aligned(16))) bf16_t ph[S::H * TE_CTX], pl[S::H * TE_CTX];
    __shared__ __attribute__((aligned(16))) bf16_t stage[Dm::R_RED * 16];
    __shared__ __attribute__((aligned(16))) float red[TE_MW * Dm::R_RED * 16];
    __shared__ float s_ss[TE_VW];
    __shared__ u64 s_cand[2 * TE_VW];
    __shared__ int s_ok;
    __shared__ int s_tok;
    __shared__ int s_done;
    __shared__ int s_cancel;
    __shared__ u64 earr[TE_HP * Dm::R_HEAD * 16];
    __shared__ uint32_t tsum32[TE_XG];
    __shared__ int win[65];
    __shared__ u64 s_wtot[TE_VW + 2];
    if (p.n_total < 0) te_lds_pad[threadIdx.x] = 0;
    const int b = blockIdx.x;
    if (b >= 256) { if (b == 256 + XCDS) te_relay(p); return; }
    if ((b & 7) >= XCDS) return;
    const int w = (b >> 3) * XCDS + (b & 7);
    const int tid = threadIdx.x, wave = tid >> 6;
    if (tid < TE_VW) s_ss[tid] = 0.f;
    if (tid == 0) { s_ok = 1; s_tok = 0; s_done = 0; s_cancel = 0; win[64] = 0; }
    const TeLds L{hf, xb, qkvf, qh, knew, vnew, sc, ph, pl, stage, red, s_ss, s_cand, &s_ok, &s_tok, &s_done, &s_cancel, earr, tsum32, win, s_wtot};
    te_sync();
    if (wave >= TE_VW) te_matrix_role_q<XCDS, B, HQ>(p, q, L, w, __builtin_amdgcn_readfirstlane(wave - TE_VW), tid & 63);
    else te_vector_role<XCDS>(p, L, w, tid);
}
}   // namespace

const void* token_engine_q_kernel(int xcds, int bits, bool head_q) {
#define TEQ_CASE(X, B)                                                                                                    \
    if (xcds == X && bits == B) return head_q ? (const void*)k_token_engine_q<X, B, true> : (const void*)k_token_engine_q<X, B, false>;
    TEQ_CASE(1, 8) TEQ_CASE(2, 8) TEQ_CASE(4, 8) TEQ_CASE(8, 8)
    TEQ_CASE(1, 4) TEQ_CASE(2, 4) TEQ_CASE(4, 4) TEQ_CASE(8, 4)
#undef TEQ_CASE
    return nullptr;
}
