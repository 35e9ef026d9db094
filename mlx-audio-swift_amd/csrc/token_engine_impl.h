// token_engine_impl.h - the device program of the batch-1 token engine shared by its two translation units: token_engine.hip
// (bf16 weight tiles, k_token_engine) and token_engine_q.hip (MLX-quantised code tiles, k_token_engine_q).  Everything except the
// matrix waves' program and the kernels lives here: shape, parameters, LDS map, the bf16 tile helpers, the vector waves' program and
// the relay.  See token_engine.hip for the design.
#pragma once
#include "common.h"
#include "kernels.h"
#include "sampler_math.h"
#include <type_traits>

namespace {
typedef unsigned long long u64;

// the one shape compiled in: Soprano-80M's LM (SopranoConfig.swift:103-167; layer count and vocabulary stay run-time)
struct TeShape {
    static constexpr int d = 512, ff = 2304, H = 4, Hkv = 1, D = 128, Nqkv = (H + 2 * Hkv) * D, HD = H * D;
};
constexpr int TE_NT = 512;                     // threads per worker: TE_VW vector waves + TE_MW matrix waves
constexpr int TE_VW = 4, TE_MW = 4;
constexpr int TE_CTX = 1024;                   // positions per request (scores and probabilities in LDS); Soprano's default budget is 512 ids
constexpr int TE_HP = 2;                       // output-projection passes at most (vocabulary <= TE_HP x 8 x 16 x workers ids)
constexpr int TE_KPRE = 2, TE_VPRE = 4;        // key tiles per wave / 32-key value steps requested before the layer's first poll (128 positions)
constexpr int TE_XG = 2048;                    // granules per exchange buffer (two bf16 values + the edge's tag each)

struct TeParams {
    const bf16_t *emb, *wqkv, *wo, *wgu, *wdown, *head, *norms, *qknorm;
    const float *rope_cos, *rope_sin;
    int L, V, Vpad;
    float eps;
    const int32_t* prompt;
    int n_prompt, n_total;
    int t_start;                // first position the engine walks (the K/V of the positions before it were imported from the launch chain's prefill)
    int32_t* tok_dev;           // [n_total] device memory, -1 = not chosen yet: the id chosen after position t (one agent-scope store by worker 0)
    int32_t* next_tokens;       // [n_total] HOST-VISIBLE (pinned, coherent) copy, filled WHILE the launch runs by the relay block (te_relay): the
                                // host reads the ids from here for generateStream's .token events (Soprano.swift:877)
    const int* cancel;          // host-visible word or null, read by the relay block only
    int* cancel_dev;            // device word the relay forwards it to: worker 0 reads it once per position, the value travels with edge 5
                                // (every worker sees the SAME value at the same position) and a non-zero value ends the request like the stop id
    unsigned* relay_done;       // device word: worker 0 has left (everything it chose is in tok_dev)
    float* logits_out;          // [n_total][V] or null
    float* hidden_out;          // [n_total][d] or null (final-norm output: what Soprano's decoder consumes)
    bf16_t* kv;                 // the K/V copy [L][2][TE_CTX][Hkv*D] (every worker writes the same bytes, see te_vector_role)
    u64* xbuf;                  // [2][TE_XG]
    unsigned* fail;             // set when a poll ran out (workers not co-resident)
    int xcds, spin;
    // which positions get an output projection and a token: [head_from, head_until) - the laboratory asks for all of them, generate for
    // the last prompt position and every generated one but the last (whose hidden state is still wanted, not its successor)
    int head_from, head_until;
    // token choice: 0 = arg-max of the logits (laboratory form); 2 = arg-max behind the repetition penalty (generate at temperature 0);
    // 1 = "mis-sampler-v1" (oracle/sampler.py) behind the Soprano flavour's repetition penalty (float32, once
    // per occurrence among the last win_cap GENERATED ids, Soprano.swift:833-901), bit for bit what lm_sampler.hip computes
    int sample, win_cap;
    float temperature, penalty;
    u64 seed;
    long long row;              // global row index of the request (RNG key)
    int stop_id;                // a sampled id that ends the request (-1: none)
    int32_t* n_done;            // [2] out: positions processed, ids sampled
    u64* dbg;                   // diagnostics (MIS_TE_STAMPS=<position>): cycle stamps of worker 0 at the phase boundaries of layer 1 of that position
    int dbg_token;
};

__device__ __forceinline__ unsigned te_key(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
// sum over the 16 lanes of a DPP row (lanes 16 r .. 16 r + 15), result in every lane of the row: two quad permutes, half-row mirror, row
// mirror - four VALU-rate instructions.  (__shfl_xor compiles to ds_bpermute_b32, an LDS round trip of ~64 cycles each: the score loop's
// 128 of them per thread were 5-7 us per layer.)
__device__ __forceinline__ float te_row16_sum(float x) {
    int xi = __builtin_bit_cast(int, x);
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, xi, 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]
    xi = __builtin_bit_cast(int, x);
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, xi, 0x4E, 0xF, 0xF, true));      // quad_perm [2,3,0,1]
    xi = __builtin_bit_cast(int, x);
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, xi, 0x141, 0xF, 0xF, true));     // row_half_mirror
    xi = __builtin_bit_cast(int, x);
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, xi, 0x140, 0xF, 0xF, true));     // row_mirror
    return x;
}
__device__ __forceinline__ float te_wave_max_dpp(float x) {
    auto step = [](float v, int tag) {
        const int vi = __builtin_bit_cast(int, v);
        int yi;
        switch (tag) {
            case 0: yi = __builtin_amdgcn_update_dpp(vi, vi, 0xB1, 0xF, 0xF, false); break;
            case 1: yi = __builtin_amdgcn_update_dpp(vi, vi, 0x4E, 0xF, 0xF, false); break;
            case 2: yi = __builtin_amdgcn_update_dpp(vi, vi, 0x141, 0xF, 0xF, false); break;
            default: yi = __builtin_amdgcn_update_dpp(vi, vi, 0x140, 0xF, 0xF, false); break;
        }
        return fmaxf(v, __builtin_bit_cast(float, yi));
    };
    x = step(x, 0); x = step(x, 1); x = step(x, 2); x = step(x, 3);
    const int vi = __builtin_bit_cast(int, x);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 16)),
                r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
// Block barrier that waits for LDS traffic only.  __syncthreads() carries a workgroup-scope fence, i.e. s_waitcnt vmcnt(0): it would make
// the matrix waves wait for every weight tile they have just requested for the NEXT phase.  Global-memory ordering is handled where it is
// needed (the publishers' own s_waitcnt vmcnt(0) before an edge).
__device__ __forceinline__ void te_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- matrix waves.  A worker's slice of y = W x is R tile rows (ids nt[r], -1 = none); each of the TE_MW matrix waves takes a quarter of
// the KT k-tiles of every row and holds them in registers: requested one phase AHEAD (right after the previous phase's MFMAs), so that the
// stream runs under the vector waves' epilogue, the edge and the gather.  Loads are unconditional on clamped addresses.
template <int R, int KPW>
struct TeTiles { bf16x8_t a[R][KPW]; bf16x8_t wn[KPW]; };
// Tiles FROM .. TO - 1 of the flattened list f = u R + r (all of them by default): a phase's tiles are requested in PIECES, one piece behind
// each barrier the matrix waves pass on their way to the phase (te_matrix_role) - a wave that requests 40 tiles at once stays in the issue
// loop for as long as the CU's memory queue is full (~4 us at one XCD's 40 GB/s per CU), and the vector waves wait for it at the next barrier.
template <int R, int KPW, bool NORM, int FROM = 0, int TO = R * KPW>
__device__ __forceinline__ void te_load(TeTiles<R, KPW>& T, const bf16_t* Wp, const int KT, const int (&nt)[R], const bf16_t* wnorm, const int mw,
                                        const int lane) {
    const int kt0 = mw * KT / TE_MW, kt1 = (mw + 1) * KT / TE_MW;
    const int klast = kt1 > kt0 ? kt1 - 1 : kt0;
    const unsigned voff = (unsigned)lane * 16u;                      // the only per-lane part of a tile address (scalar base + 32-bit offset)
#pragma unroll
    for (int u = 0; u < KPW; ++u) {
        int kk = kt0 + u;
        kk = kk > klast ? klast : kk;
        kk = kk >= KT ? KT - 1 : kk;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (u * R + r < FROM || u * R + r >= TO) continue;
            const int tile = nt[r] < 0 ? 0 : nt[r];
            const char* base = reinterpret_cast<const char*>(Wp) + ((size_t)tile * KT + kk) * 1024;        // wave-uniform
            T.a[r][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(base + voff));
        }
        if (NORM && u * R >= FROM && u * R < TO) {                                                         // the norm weights of this wave's k range
            const char* nb = reinterpret_cast<const char*>(wnorm) + (size_t)kk * 64;
            T.wn[u] = *reinterpret_cast<const bf16x8_t*>(nb + (unsigned)(lane >> 4) * 16u);
        }
    }
}
// B fragments (row 0 of the 16-row operand): lanes with (lane & 15) == 0 hold x[32 kk + 8 (lane >> 4) ..+8], everything else is zero
template <int KPW>
__device__ __forceinline__ void te_xfrag_bf16(bf16x8_t (&xf)[KPW], const bf16_t* xb, const int KT, const int mw, const int lane) {
    const int kt0 = mw * KT / TE_MW, kt1 = (mw + 1) * KT / TE_MW;
    const int klast = kt1 > kt0 ? kt1 - 1 : kt0;
    const bool row0 = (lane & 15) == 0;
    const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < KPW; ++u) {
        int kk = kt0 + u;
        const bool live = kk < kt1;
        kk = kk > klast ? klast : kk;
        kk = kk >= KT ? KT - 1 : kk;
        const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(xb + 32 * kk + 8 * (lane >> 4));
        xf[u] = (row0 && live) ? v : zero;
    }
}
// the same from the float32 residual stream through RMSNorm: T(w * T(h * inv))
template <int KPW>
__device__ __forceinline__ void te_xfrag_norm(bf16x8_t (&xf)[KPW], const float* hf, const bf16x8_t (&wn)[KPW], const float inv, const int KT,
                                              const int mw, const int lane) {
    const int kt0 = mw * KT / TE_MW, kt1 = (mw + 1) * KT / TE_MW;
    const int klast = kt1 > kt0 ? kt1 - 1 : kt0;
    const bool row0 = (lane & 15) == 0;
#pragma unroll
    for (int u = 0; u < KPW; ++u) {
        int kk = kt0 + u;
        const bool live = kk < kt1;
        kk = kk > klast ? klast : kk;
        kk = kk >= KT ? KT - 1 : kk;
        const float* hp = hf + 32 * kk + 8 * (lane >> 4);
        const f32x4_t h0 = *reinterpret_cast<const f32x4_t*>(hp), h1 = *reinterpret_cast<const f32x4_t*>(hp + 4);
        bf16x8_t v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float hv = e < 4 ? h0[e] : h1[e - 4];
            v[e] = (short)f32_to_bf16(bf16_to_f32((bf16_t)wn[u][e]) * bf16_round_f32(hv * inv));
        }
        const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
        xf[u] = (row0 && live) ? v : zero;
    }
}
template <int R, int KPW>
__device__ __forceinline__ void te_mma(const TeTiles<R, KPW>& T, const bf16x8_t (&xf)[KPW], float* red, const int mw, const int lane) {
    constexpr int RB = R > 5 ? 5 : R;                                // tile rows per block of accumulators (gate|up: 10 rows = 2 blocks - with all
    const int g = lane >> 4;                                         //  ten live next to 176 registers of tiles the kernel spills)
#pragma unroll
    for (int r0 = 0; r0 < R; r0 += RB) {
        f32x4_t acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < KPW; ++u)
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (r0 + r < R) acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(T.a[r0 + r][u], xf[u], acc[r], 0, 0, 0);
        if ((lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (r0 + r < R) *reinterpret_cast<f32x4_t*>(red + ((size_t)(mw * R + r0 + r) * 16 + 4 * g)) = acc[r];
        }
    }
    // the NEXT phase's tile requests follow in program order: left to the scheduler they are hoisted above these MFMAs, and two phases'
    // tiles (gate|up: 176 registers, down: 72) are live at once - spills into scratch, i.e. more traffic in the same vmcnt queue
    __builtin_amdgcn_sched_barrier(0);
}
// sum of the matrix waves' partials for element (r, i), fixed order
template <int R>
__device__ __forceinline__ float te_combine(const float* red, int r, int i) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < TE_MW; ++m) s += red[(size_t)(m * R + r) * 16 + i];
    return s;
}

// LDS of one worker
struct TeLds {
    float* hf;          // [d] residual stream (bf16 values)
    bf16_t* xb;         // [max(ff, H D)] attention output / activation: the plain GEMV inputs
    float* qkvf;        // [Nqkv]
    float* qh;          // [H][D]
    float *knew, *vnew; // [D]
    float* sc;          // [H][TE_CTX]
    bf16_t *ph, *pl;    // [H][TE_CTX] probabilities of the keys before this position, bf16 hi and lo
    bf16_t* stage;      // [R x 16] one epilogue value per thread before four of them are packed into a granule
    float* red;         // [TE_MW][R][16] partial sums of the matrix waves
    float* s_ss;        // [TE_VW] sum-of-squares partials of the residual stream
    u64* s_cand;        // [2][TE_VW] the waves' best candidates: own slice, then all workers'
    int *s_ok, *s_tok, *s_done, *s_cancel;
    u64* earr;          // [TE_HP][R_HEAD x 16] fixed-point masses of this worker's ids
    uint32_t* tsum32;   // [2 x tiles] the mass of every 16-id tile of the vocabulary, lo / hi words
    int* win;           // [64] + length: the repetition window (generated ids)
    u64* s_wtot;        // [TE_VW + 2] wave totals of the tile scan; the chosen tile and the draw's remainder inside it
};
template <int XCDS>
struct TeDims {
    using S = TeShape;
    static constexpr int W = 32 * XCDS;
    static constexpr int R_QKV = (S::Nqkv / 16 + W - 1) / W, R_O = (S::d / 16 + W - 1) / W, P_GU = (S::ff / 16 + W - 1) / W, R_GU = 2 * P_GU;
    static constexpr int R_HEAD = 8;                                 // tile rows of the output projection per pass
    static constexpr int KPW_D = (S::d / 32 + TE_MW - 1) / TE_MW, KPW_HD = (S::HD / 32 + TE_MW - 1) / TE_MW, KPW_FF = (S::ff / 32 + TE_MW - 1) / TE_MW;
    static constexpr int R_RED = R_GU > R_HEAD ? R_GU : R_HEAD;
};

// ---------------------------------------------------------------------------- the vector waves' program (256 threads)
// An EDGE (all-to-all hand-off of one op's output vector): every value travels in a self-validating 8-byte granule {two bf16 values, the
// edge's 32-bit tag}, written with ONE agent-scope store by its producer and polled with agent-scope loads by every consumer thread
// that needs it (MI355X_MICROARCH.md, hand-off form R2: "granule = one naturally aligned 8-byte {data, tag}") - no counter, no drain of
// the producer's stores, no barrier between publishing and gathering: the consumer's load that finds the tag IS the gather.  Tags count
// edges from 1 (buffers start zeroed); two buffers alternate - a worker can only publish edge e + 2 after it has gathered all of edge
// e + 1, which every worker publishes only after it has gathered edge e.  Polls are bounded: a time-out clears s_ok, and both programs
// leave at the next barrier.  (Round 5's first form - values, store drain, barrier, arrival counter, poll, barrier, gather - cost
// 3.7 + 1.9 us per edge inside the engine, three barriers of it shared with the matrix waves.)
template <int XCDS>
__device__ __forceinline__ void te_vector_role(const TeParams& p, const TeLds& L, const int w, const int tid) {
    using S = TeShape;
    using Dm = TeDims<XCDS>;
    constexpr int W = Dm::W, R_QKV = Dm::R_QKV, R_O = Dm::R_O, P_GU = Dm::P_GU, R_GU = Dm::R_GU, R_HEAD = Dm::R_HEAD;
    constexpr int VT = TE_VW * 64;
    const int wave = tid >> 6, lane = tid & 63;
    const int NTV = p.Vpad / 16;
    unsigned edge = 0;                                               // edges passed so far; the current edge's tag is edge + 1
    // ONE K/V copy for all workers, written by every one of them: the new row is computed redundantly from the same gathered q|k|v by
    // the same instructions, so all writers store identical bytes, and a worker only consumes positions it has itself written at an
    // earlier step.  (Private copies - 32 x 17 x 2 x ctx x 256 B - do not fit the XCD's 4 MB L2: every row came from the Infinity
    // Cache, ~2 us per round trip under the weight stream.)
    bf16_t* kv_mine = p.kv;
    const float scale = rsqrtf((float)S::D);
    float(*qh)[S::D] = reinterpret_cast<float(*)[S::D]>(L.qh);
    float(*sc)[TE_CTX] = reinterpret_cast<float(*)[TE_CTX]>(L.sc);
    auto granule = [&](const u64* buf, int gi, unsigned tag) -> uint32_t {         // poll granule gi until it carries `tag`; its two values
        u64 g = __hip_atomic_load(buf + gi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int it = 0;
        while ((unsigned)(g >> 32) != tag) {
            if (++it > p.spin) { *L.s_ok = 0; break; }
            __builtin_amdgcn_s_sleep(1);
            g = __hip_atomic_load(buf + gi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return (uint32_t)g;
    };
    // the same for the NG granules tid, tid + VT, ... of a vector of n granules: all first polls in flight together (a thread that polls
    // its granules one after the other pays a memory round trip for each: 5 for the activation vector)
    auto granules = [&](const u64* buf, int n, unsigned tag, auto&& NGc, auto&& sink) {
        constexpr int NG = std::remove_reference_t<decltype(NGc)>::value;
        u64 g[NG];
#pragma unroll
        for (int k = 0; k < NG; ++k) { const int gi = tid + k * VT; g[k] = __hip_atomic_load(buf + (gi < n ? gi : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int gi = tid + k * VT;
            if (gi < n) {
                uint32_t v = (uint32_t)g[k];
                if ((unsigned)(g[k] >> 32) != tag) v = granule(buf, gi, tag);
                sink(gi, v);
            }
        }
    };
    // One epilogue value per thread (tid < n_vals, value index tid = 16 r + i); the even thread of each pair sends both (through LDS: the
    // pair sits in one wave, whose own s_waitcnt orders the write before the read).  first_pair = granule index of value 16 r, or -1.
    auto publish2 = [&](u64* buf, int n_vals, float value, int first_pair, unsigned tag) {
        if (tid < n_vals) L.stage[tid] = f32_to_bf16(value);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (tid < n_vals && (tid & 1) == 0 && first_pair >= 0)
            __hip_atomic_store(buf + first_pair + ((tid & 15) >> 1), (u64)*reinterpret_cast<const uint32_t*>(L.stage + tid) | ((u64)tag << 32),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // gather of the residual stream (d values = d / 2 granules, one per thread) + its sum of squares per wave
    auto gather_h = [&](const u64* buf, unsigned tag) {
        float ss = 0.f;
        if (tid < S::d / 2) {
            const uint32_t g2 = granule(buf, tid, tag);
            const float v0 = bf16_to_f32((bf16_t)(g2 & 0xffffu)), v1 = bf16_to_f32((bf16_t)(g2 >> 16));
            L.hf[2 * tid] = v0; L.hf[2 * tid + 1] = v1;
            ss = v0 * v0 + v1 * v1;
        }
        ss = wave_sum_dpp(ss);
        if (lane == 0) L.s_ss[wave] = ss;
    };
    // residual epilogue of o_proj / down_proj: this worker's R_O x 16 outputs, T(h + T(acc))
    auto publish_resid = [&](u64* buf, unsigned tag) {
        float v = 0.f;
        int gr = -1;
        if (tid < R_O * 16) {
            const int r = tid >> 4, i = tid & 15, nt = w + r * W;
            if (nt < S::d / 16) { v = L.hf[nt * 16 + i] + bf16_round_f32(te_combine<R_O>(L.red, r, i)); gr = nt * 8; }
        }
        publish2(buf, R_O * 16, v, gr, tag);
    };
#define TE_STAMP(i) do { if (p.dbg && w == 0 && tid == 0 && t == p.dbg_token && li == 1) p.dbg[i] = __builtin_readcyclecounter(); } while (0)
#define TE_EDGE_BUF() (p.xbuf + (size_t)(edge & 1u) * TE_XG)
    int t_last = p.t_start - 1, n_sampled = 0;
    for (int t = p.t_start; t < p.n_total; ++t) {
        if (tid == 0 && t < p.n_prompt) *L.s_tok = p.prompt[t];
        // (requested here, consumed at edge 5; the relay block keeps the device word equal to the host's)
        uint32_t cancel_word = 0u;
        if (p.cancel && w == 0 && tid == 0) cancel_word = (uint32_t)__hip_atomic_load(p.cancel_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        te_sync();                                                   // token id
        if (*L.s_done) break;
        t_last = t;
        const bool do_head = t >= p.head_from && t < p.head_until;
        {
            const int tok = *L.s_tok;
            float ss = 0.f;
            if (tid < S::d / 2) {
                const uint32_t g2 = *reinterpret_cast<const uint32_t*>(p.emb + (size_t)tok * S::d + 2 * tid);
                const float v0 = bf16_to_f32((bf16_t)(g2 & 0xffffu)), v1 = bf16_to_f32((bf16_t)(g2 >> 16));
                L.hf[2 * tid] = v0; L.hf[2 * tid + 1] = v1;
                ss = v0 * v0 + v1 * v1;
            }
            ss = wave_sum_dpp(ss);
            if (lane == 0) L.s_ss[wave] = ss;
        }
        te_sync();                                                   // embedding row + sum of squares
        const float rope_c = p.rope_cos[(size_t)t * (S::D / 2) + lane], rope_s = p.rope_sin[(size_t)t * (S::D / 2) + lane];     // this position's row
        for (int li = 0; li < p.L; ++li) {
            bf16_t nw_q[2], nw_k[2];
            bf16x8_t kpre[TE_KPRE][S::D / 32], vpre[TE_VPRE][2];
            // ================= q|k|v slice -> edge 1
            TE_STAMP(0);
            te_sync();                                               // red ready
            TE_STAMP(1);
            {
                u64* buf = TE_EDGE_BUF();
                const unsigned tag = ++edge;
                float v = 0.f;
                int gr = -1;
                if (tid < R_QKV * 16) {
                    const int r = tid >> 4, i = tid & 15, nt = w + r * W;
                    if (nt < S::Nqkv / 16) { v = te_combine<R_QKV>(L.red, r, i); gr = nt * 8; }
                }
                publish2(buf, R_QKV * 16, v, gr, tag);
                TE_STAMP(2);
                // everything the attention phase reads from memory that does not depend on this layer's q|k|v, requested BEFORE the poll:
                // the q/k-norm weights, this wave's first TE_KPRE key tiles, the first TE_VPRE 32-key steps of its two value tiles
                nw_q[0] = p.qknorm[(size_t)(2 * li) * S::D + lane]; nw_q[1] = p.qknorm[(size_t)(2 * li) * S::D + lane + 64];
                nw_k[0] = p.qknorm[(size_t)(2 * li + 1) * S::D + lane]; nw_k[1] = p.qknorm[(size_t)(2 * li + 1) * S::D + lane + 64];
                {
                    const int i16 = lane & 15, q4 = lane >> 4, pos = t;
                    const bf16_t* kcl = kv_mine + ((size_t)li * 2 + 0) * TE_CTX * S::D;
                    const bf16_t* vcl = kv_mine + ((size_t)li * 2 + 1) * TE_CTX * S::D;
#pragma unroll
                    for (int k = 0; k < TE_KPRE; ++k) {
                        int row = 16 * (wave + TE_VW * k) + i16;
                        row = row < pos ? row : (pos > 0 ? pos - 1 : 0);
#pragma unroll
                        for (int ds = 0; ds < S::D / 32; ++ds)
                            kpre[k][ds] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(kcl + (size_t)row * S::D + 8 * q4 + 32 * ds));
                    }
#pragma unroll
                    for (int k = 0; k < TE_VPRE; ++k)
#pragma unroll
                        for (int n = 0; n < 2; ++n)   // (past L1: a value line holds 64 positions, the newest written by this CU a step ago)
                            vpre[k][n] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(vcl + (size_t)(16 * (2 * wave + n) + i16) * TE_CTX + 32 * k + 8 * q4));
                }
                granules(buf, S::Nqkv / 2, tag, std::integral_constant<int, (S::Nqkv / 2 + VT - 1) / VT>{}, [&](int gi, uint32_t g2) {
                    L.qkvf[2 * gi] = bf16_to_f32((bf16_t)(g2 & 0xffffu)); L.qkvf[2 * gi + 1] = bf16_to_f32((bf16_t)(g2 >> 16));
                });
                TE_STAMP(3);
            }
            te_sync();                                               // edge 1: q|k|v gathered
            if (!*L.s_ok) { if (tid == 0) __hip_atomic_store(p.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
            TE_STAMP(4);
            // ================= q/k-norm, RoPE, attention (redundant on every worker)
            bf16_t* kc = kv_mine + ((size_t)li * 2 + 0) * TE_CTX * S::D;
            bf16_t* vc = kv_mine + ((size_t)li * 2 + 1) * TE_CTX * S::D;
            const int pos = t, ctx = t + 1;
            {   // wave v: q head v; wave 0 also the key, wave 1 the value.  Lane holds elements lane, lane + 64 (RoPE partners)
                const float c = rope_c, sn = rope_s;
                for (int which = 0; which < 2; ++which) {
                    if (which == 1 && wave != 0) break;
                    const float* src = L.qkvf + (which ? S::HD : wave * S::D);
                    const float x1 = src[lane], x2 = src[lane + 64];
                    const float ss = wave_sum_dpp(x1 * x1 + x2 * x2);
                    const float inv = rsqrtf(ss / (float)S::D + p.eps);
                    const float y1 = bf16_round_f32(bf16_to_f32(which ? nw_k[0] : nw_q[0]) * bf16_round_f32(x1 * inv));
                    const float y2 = bf16_round_f32(bf16_to_f32(which ? nw_k[1] : nw_q[1]) * bf16_round_f32(x2 * inv));
                    const float o1 = bf16_round_f32(y1 * c - y2 * sn), o2 = bf16_round_f32(y1 * sn + y2 * c);
                    if (which) {
                        L.knew[lane] = o1; L.knew[lane + 64] = o2;
                        kc[(size_t)pos * S::D + lane] = f32_to_bf16(o1);
                        kc[(size_t)pos * S::D + lane + 64] = f32_to_bf16(o2);
                    } else {
                        qh[wave][lane] = o1; qh[wave][lane + 64] = o2;
                    }
                }
                if (wave == 1) {                                                 // values: kept TRANSPOSED [d][position] (the P.V MFMA's A operand)
                    const float v1 = L.qkvf[S::HD + S::D + lane], v2 = L.qkvf[S::HD + S::D + lane + 64];
                    L.vnew[lane] = v1; L.vnew[lane + 64] = v2;
                    vc[(size_t)lane * TE_CTX + pos] = f32_to_bf16(v1);
                    vc[(size_t)(lane + 64) * TE_CTX + pos] = f32_to_bf16(v2);
                }
            }
            te_sync();
            TE_STAMP(5);
            {   // scores on the matrix core: D[key][head] = sum_d K[key][d] q[head][d] - A = 16 keys x 32 d straight from the row-major key
                // cache (16 B per lane), B = q^T with the four heads in columns 0..3.  Wave v takes the key tiles v, v + 4, ...; only keys
                // BEFORE this position come from memory (the new key is in LDS: its row is still on its way to the cache).  (The VALU form -
                // 16 lanes per key, DPP reductions - was 4.5 us per layer at 81 keys.)
                const int i16 = lane & 15, q4 = lane >> 4;
                bf16x8_t qf[S::D / 32];
#pragma unroll
                for (int ds = 0; ds < S::D / 32; ++ds) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) qf[ds][e] = i16 < S::H ? (short)f32_to_bf16(qh[i16 < S::H ? i16 : 0][32 * ds + 8 * q4 + e]) : (short)0;
                }
                const int n_kt = (pos + 15) >> 4;
                auto score_tile = [&](int kt, const bf16x8_t (&ka)[S::D / 32]) {
                    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ds = 0; ds < S::D / 32; ++ds) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[ds], qf[ds], acc, 0, 0, 0);
                    if (i16 < S::H) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int j = 16 * kt + 4 * q4 + r;
                            if (j < pos) sc[i16][j] = acc[r] * scale;
                        }
                    }
                };
#pragma unroll
                for (int k = 0; k < TE_KPRE; ++k)
                    if (wave + TE_VW * k < n_kt) score_tile(wave + TE_VW * k, kpre[k]);              // requested ahead of edge 1's poll
                for (int kt = wave + TE_VW * TE_KPRE; kt < n_kt; kt += TE_VW) {                        // longer contexts: the tiles behind them
                    int row = 16 * kt + i16;
                    row = row < pos ? row : pos - 1;
                    const bf16_t* kr = kc + (size_t)row * S::D + 8 * q4;
                    bf16x8_t ka[S::D / 32];
#pragma unroll
                    for (int ds = 0; ds < S::D / 32; ++ds) ka[ds] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(kr + 32 * ds));
                    score_tile(kt, ka);
                }
                {   // the new key: head `wave`
                    const float dsum = wave_sum_dpp(qh[wave][lane] * L.knew[lane] + qh[wave][lane + 64] * L.knew[lane + 64]);
                    if (lane == 0) sc[wave][pos] = dsum * scale;
                }
            }
            te_sync();
            TE_STAMP(6);
            {   // softmax of head `wave`; the probabilities of the keys before this position as bf16 hi + lo (the pair keeps float32 accuracy
                // through the bf16 MFMA), zero up to the next multiple of 32 keys; the new key's probability stays float32 (sc[head][pos])
                float m = -3.0e38f;
                for (int j = lane; j < ctx; j += 64) m = fmaxf(m, sc[wave][j]);
                m = te_wave_max_dpp(m);
                float sum = 0.f;
                for (int j = lane; j < ctx; j += 64) { const float e = expf(sc[wave][j] - m); sc[wave][j] = e; sum += e; }
                sum = wave_sum_dpp(sum);
                const float rinv = 1.0f / sum;
                const int pend = (pos + 31) & ~31;
                for (int j = lane; j < pend || j < ctx; j += 64) {
                    const float pj = j < ctx ? sc[wave][j] * rinv : 0.f;
                    if (j < ctx) sc[wave][j] = pj;
                    if (j < pend) {
                        const float pm = j < pos ? pj : 0.f;
                        const bf16_t hi = f32_to_bf16(pm);
                        L.ph[wave * TE_CTX + j] = hi;
                        L.pl[wave * TE_CTX + j] = f32_to_bf16(pm - bf16_to_f32(hi));
                    }
                }
            }
            te_sync();
            {   // P.V on the matrix core: D[d][head] = sum_key Vt[d][key] P[head][key] - A = 16 d x 32 keys from the transposed value cache,
                // B = P^T (hi, then lo).  Wave v owns the d tiles 2 v, 2 v + 1 over ALL keys (no cross-wave sum); the new key joins in the
                // epilogue from LDS.
                const int i16 = lane & 15, q4 = lane >> 4;
                const int n_k32 = (pos + 31) >> 5;
                f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
                auto pv_step = [&](int kt, const bf16x8_t (&va)[2]) {
                    const bf16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
                    const bf16x8_t bh = i16 < S::H ? *reinterpret_cast<const bf16x8_t*>(L.ph + (i16 < S::H ? i16 : 0) * TE_CTX + 32 * kt + 8 * q4) : z;
                    const bf16x8_t bl = i16 < S::H ? *reinterpret_cast<const bf16x8_t*>(L.pl + (i16 < S::H ? i16 : 0) * TE_CTX + 32 * kt + 8 * q4) : z;
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[n], bh, acc[n], 0, 0, 0);
                        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[n], bl, acc[n], 0, 0, 0);
                    }
                };
#pragma unroll
                for (int k = 0; k < TE_VPRE; ++k)
                    if (k < n_k32) pv_step(k, vpre[k]);                                              // requested ahead of edge 1's poll
                for (int kt = TE_VPRE; kt < n_k32; ++kt) {
                    bf16x8_t va[2];
#pragma unroll
                    for (int n = 0; n < 2; ++n)       // (past L1: a value line holds 64 positions, the newest written by this CU a step ago)
                        va[n] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(vc + (size_t)(16 * (2 * wave + n) + i16) * TE_CTX + 32 * kt + 8 * q4));
                    pv_step(kt, va);
                }
                if (i16 < S::H) {
                    const float pn = sc[i16][pos];
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const int d0 = 16 * (2 * wave + n) + 4 * q4;
                        bf16_t o[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16(acc[n][r] + pn * L.vnew[d0 + r]);
                        *reinterpret_cast<u64*>(L.xb + i16 * S::D + d0) = (u64)o[0] | ((u64)o[1] << 16) | ((u64)o[2] << 32) | ((u64)o[3] << 48);
                    }
                }
            }
            te_sync();                                               // attention output ready
            TE_STAMP(7);
            // ================= o_proj slice, residual -> edge 2
            te_sync();                                               // red ready
            TE_STAMP(8);
            {
                u64* buf = TE_EDGE_BUF();
                const unsigned tag = ++edge;
                publish_resid(buf, tag);
                TE_STAMP(9);
                gather_h(buf, tag);
                TE_STAMP(10);
            }
            te_sync();                                               // edge 2: residual stream gathered
            if (!*L.s_ok) { if (tid == 0) __hip_atomic_store(p.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
            TE_STAMP(11);
            // ================= gate|up pairs -> SwiGLU -> edge 3
            te_sync();                                               // red ready
            TE_STAMP(12);
            {
                u64* buf = TE_EDGE_BUF();
                const unsigned tag = ++edge;
                float v = 0.f;
                int gr = -1;
                if (tid < P_GU * 16) {
                    const int r = tid >> 4, i = tid & 15, pr = w + r * W;
                    if (pr < S::ff / 16) {
                        const float gt = bf16_round_f32(te_combine<R_GU>(L.red, 2 * r, i)), up = bf16_round_f32(te_combine<R_GU>(L.red, 2 * r + 1, i));
                        const float sg = bf16_round_f32(1.0f / (1.0f + expf(-gt)));
                        v = bf16_round_f32(gt * sg) * up;
                        gr = pr * 8;
                    }
                }
                publish2(buf, P_GU * 16, v, gr, tag);
                TE_STAMP(13);
                granules(buf, S::ff / 2, tag, std::integral_constant<int, (S::ff / 2 + VT - 1) / VT>{},
                         [&](int gi, uint32_t g2) { *reinterpret_cast<uint32_t*>(L.xb + 2 * gi) = g2; });
                TE_STAMP(14);
            }
            te_sync();                                               // edge 3: activation gathered
            if (!*L.s_ok) { if (tid == 0) __hip_atomic_store(p.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
            TE_STAMP(15);
            // ================= down_proj slice, residual -> edge 4
            te_sync();                                               // red ready
            TE_STAMP(16);
            {
                u64* buf = TE_EDGE_BUF();
                const unsigned tag = ++edge;
                publish_resid(buf, tag);
                TE_STAMP(17);
                gather_h(buf, tag);
                TE_STAMP(18);
            }
            te_sync();                                               // edge 4: residual stream gathered
            if (!*L.s_ok) { if (tid == 0) __hip_atomic_store(p.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
            TE_STAMP(19);
        }
        // ================= final norm (hidden tap) -> output projection slice -> token -> edges 5 (.. 7)
        if (p.hidden_out && w == 0 && t >= p.head_from && tid < S::d / 4) {
            const float inv = rsqrtf(((L.s_ss[0] + L.s_ss[1]) + (L.s_ss[2] + L.s_ss[3])) / (float)S::d + p.eps);
            const bf16_t* wn = p.norms + (size_t)(2 * p.L) * S::d;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                p.hidden_out[(size_t)(t - p.head_from) * S::d + 4 * tid + e] = bf16_round_f32(bf16_to_f32(wn[4 * tid + e]) * bf16_round_f32(L.hf[4 * tid + e] * inv));
        }
        if (do_head) {
            // arg-max candidate = (16-bit order-preserving key of the bf16 logit) << 16 | (0xffff - id): highest logit, lowest id on ties;
            // sampling candidate = the 32-bit key of the penalised float32 logit (only the maximum travels)
            uint32_t cand = 0;
            float lpen[TE_HP];
            int own_n[TE_HP];
#pragma unroll
            for (int k = 0; k < TE_HP; ++k) { lpen[k] = 0.f; own_n[k] = -1; }
#pragma unroll
            for (int pass = 0; pass < TE_HP; ++pass) {
                if (pass * R_HEAD * W >= NTV) break;
                te_sync();                                           // red ready
                if (tid < R_HEAD * 16) {
                    const int r = tid >> 4, i = tid & 15, nt = w + (pass * R_HEAD + r) * W;
                    if (nt < NTV) {
                        const int n = nt * 16 + i;
                        const float lg = bf16_round_f32(te_combine<R_HEAD>(L.red, r, i));
                        if (n < p.V) {
                            if (p.logits_out) p.logits_out[(size_t)(t - p.head_from) * p.V + n] = lg;
                            if (p.sample) {
                                // Soprano applyRepetitionPenalty (Soprano.swift:888-901): float32, once PER OCCURRENCE in the window
                                float v = lg;
                                if (p.penalty > 0.0f && p.penalty != 1.0f) {
                                    const int wl = L.win[64];
                                    int mult = 0;
                                    for (int j = 0; j < wl; ++j) mult += (L.win[j] == n);
                                    for (int k = 0; k < mult; ++k) v = (v > 0.0f) ? __fdiv_rn(v, p.penalty) : v * p.penalty;
                                }
                                lpen[pass] = v; own_n[pass] = n;
                                const uint32_t c1 = te_key(v);
                                cand = c1 > cand ? c1 : cand;
                            } else {
                                const uint32_t c1 = (te_key(lg) & 0xffff0000u) | (0xffffu - (unsigned)n);
                                cand = c1 > cand ? c1 : cand;
                            }
                        }
                    }
                }
                te_sync();                                           // red consumed
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const uint32_t other = __shfl_xor(cand, o, 64); cand = other > cand ? other : cand; }
            if (lane == 0) L.s_cand[wave] = cand;
            te_sync();                                               // candidates of the vector waves
            uint32_t best_all = 0;
            {   // edge 5: every worker's candidate to every worker
                u64* buf = TE_EDGE_BUF();
                const unsigned tag = ++edge;
                if (tid == 0) {
                    uint32_t best = 0;
#pragma unroll
                    for (int q = 0; q < TE_VW; ++q) best = (uint32_t)L.s_cand[q] > best ? (uint32_t)L.s_cand[q] : best;
                    __hip_atomic_store(buf + w, (u64)best | ((u64)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (p.cancel && w == 0)                          // granule W of this edge: the cancel word as worker 0 read it
                        __hip_atomic_store(buf + W, (u64)cancel_word | ((u64)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                uint32_t c2 = tid < W ? granule(buf, tid, tag) : 0u;
                if (p.cancel) {                                      // polled by an idle thread where there is one (W < 256), else by thread 0 behind its own
                    constexpr int CT = W < VT ? W : 0;
                    if (tid == CT && granule(buf, W, tag) != 0u) *L.s_cancel = 1;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { const uint32_t other = __shfl_xor(c2, o, 64); c2 = other > c2 ? other : c2; }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) L.s_cand[TE_VW + wave] = c2;
            }
            te_sync();                                               // edge 5 gathered
            if (!*L.s_ok) { if (tid == 0) __hip_atomic_store(p.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
#pragma unroll
            for (int q = 0; q < TE_VW; ++q) best_all = (uint32_t)L.s_cand[TE_VW + q] > best_all ? (uint32_t)L.s_cand[TE_VW + q] : best_all;
            int next;
            if (!p.sample) {
                next = (int)(0xffffu - (best_all & 0xffffu));
            } else if (p.sample == 2) {
                // arg-max of the PENALISED float32 logits (temperature 0 in the generate form): the maximum's 32-bit key is known to
                // everybody; the lowest id that holds it travels in a second edge
                uint32_t c3 = 0;
#pragma unroll
                for (int pass = 0; pass < TE_HP; ++pass)
                    if (own_n[pass] >= 0 && te_key(lpen[pass]) == best_all) { const uint32_t c1 = 0x10000u | (0xffffu - (unsigned)own_n[pass]); c3 = c1 > c3 ? c1 : c3; }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { const uint32_t other = __shfl_xor(c3, o, 64); c3 = other > c3 ? other : c3; }
                if (lane == 0) L.s_cand[wave] = c3;
                te_sync();
                u64* buf = TE_EDGE_BUF();
                const unsigned tag = ++edge;
                if (tid == 0) {
                    uint32_t best = 0;
#pragma unroll
                    for (int q = 0; q < TE_VW; ++q) best = (uint32_t)L.s_cand[q] > best ? (uint32_t)L.s_cand[q] : best;
                    __hip_atomic_store(buf + w, (u64)best | ((u64)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                uint32_t c2 = tid < W ? granule(buf, tid, tag) : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { const uint32_t other = __shfl_xor(c2, o, 64); c2 = other > c2 ? other : c2; }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) L.s_cand[TE_VW + wave] = c2;
                te_sync();                                           // edge 6: the id
                if (!*L.s_ok) { if (tid == 0) __hip_atomic_store(p.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
                uint32_t b2 = 0;
#pragma unroll
                for (int q = 0; q < TE_VW; ++q) b2 = (uint32_t)L.s_cand[TE_VW + q] > b2 ? (uint32_t)L.s_cand[TE_VW + q] : b2;
                next = (int)(0xffffu - (b2 & 0xffffu));
            } else {
                // ---- mis-sampler-v1 over the whole vocabulary: x = fdiv(l, T), e = det_exp(min(x - max x, 0)), E = trunc(e 2^40); the draw
                // r = mulhi64(rand64(seed, row, step), sum E) picks the first id, in id order, whose running sum of E exceeds r.  Ids are dealt
                // to the workers in tiles of 16, so the running sum is taken over TILES first (edge 6: every tile's mass to everybody; one block
                // scan), then inside the chosen tile by its owner (edge 7: the token to everybody).
                const float xmax = __fdiv_rn(__uint_as_float((best_all & 0x80000000u) ? (best_all & 0x7fffffffu) : ~best_all), p.temperature);
                u64* buf = TE_EDGE_BUF();
                const unsigned tag = ++edge;
#pragma unroll
                for (int pass = 0; pass < TE_HP; ++pass) {
                    if (pass * R_HEAD * W >= NTV) break;
                    u64 E = 0;
                    if (tid < R_HEAD * 16 && own_n[pass] >= 0) {
                        const float x = __fdiv_rn(lpen[pass], p.temperature);
                        E = (u64)(det_exp_dev(fminf(x - xmax, 0.0f)) * E_SCALE);
                    }
                    if (tid < R_HEAD * 16) L.earr[pass * (R_HEAD * 16) + tid] = E;
                    // tile mass = sum over the 16 lanes of a row: E < 2^41 split into two 21-bit halves, each summed in 32 bits on the DPP network
                    uint32_t a = (uint32_t)(E & 0x1fffffu), bb = (uint32_t)(E >> 21);
#pragma unroll
                    for (int o = 1; o < 16; o <<= 1) { a += __shfl_xor(a, o, 64); bb += __shfl_xor(bb, o, 64); }
                    const u64 tile_mass = (u64)a + ((u64)bb << 21);
                    if (tid < R_HEAD * 16 && (tid & 15) == 0) {
                        const int nt = w + (pass * R_HEAD + (tid >> 4)) * W;
                        if (nt < NTV) {
                            __hip_atomic_store(buf + 2 * nt, (u64)(uint32_t)tile_mass | ((u64)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(buf + 2 * nt + 1, (u64)(uint32_t)(tile_mass >> 32) | ((u64)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                }
                granules(buf, 2 * NTV, tag, std::integral_constant<int, TE_XG / VT>{}, [&](int gi, uint32_t g2) { L.tsum32[gi] = g2; });
                te_sync();                                           // edge 6: tile masses gathered
                if (!*L.s_ok) { if (tid == 0) __hip_atomic_store(p.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
                // scan over the tiles: thread -> tiles 2 tid, 2 tid + 1
                const int t0i = 2 * tid, t1i = 2 * tid + 1;
                const u64 m0 = t0i < NTV ? ((u64)L.tsum32[2 * t0i] | ((u64)L.tsum32[2 * t0i + 1] << 32)) : 0;
                const u64 m1 = t1i < NTV ? ((u64)L.tsum32[2 * t1i] | ((u64)L.tsum32[2 * t1i + 1] << 32)) : 0;
                u64 incl = m0 + m1;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t ulo = __shfl_up((uint32_t)incl, o, 64), uhi = __shfl_up((uint32_t)(incl >> 32), o, 64);
                    if (lane >= o) incl += (u64)ulo | ((u64)uhi << 32);
                }
                if (lane == 63) L.s_wtot[wave] = incl;
                te_sync();
                u64 base = 0, Z = 0;
#pragma unroll
                for (int q = 0; q < TE_VW; ++q) { if (q < wave) base += L.s_wtot[q]; Z += L.s_wtot[q]; }
                const int step = t - (p.n_prompt - 1);
                const u64 rnd = mis_splitmix64(mis_splitmix64(p.seed ^ (0xD1B54A32D192ED03ull * (u64)(p.row + 1))) + (u64)step);
                const u64 r = __umul64hi(rnd, Z);
                const u64 excl = base + incl - (m0 + m1);
                if (r >= excl && r < excl + m0) { L.s_wtot[TE_VW] = (u64)t0i; L.s_wtot[TE_VW + 1] = r - excl; }
                else if (r >= excl + m0 && r < excl + m0 + m1) { L.s_wtot[TE_VW] = (u64)t1i; L.s_wtot[TE_VW + 1] = r - excl - m0; }
                te_sync();
                const int tile = (int)L.s_wtot[TE_VW];
                const u64 rin = L.s_wtot[TE_VW + 1];
                u64* bufc = TE_EDGE_BUF();
                const unsigned tagc = ++edge;
                if (tile % W == w && tid == 0) {                     // the owner: inside the tile in id order
                    const int slot = (tile - w) / W, pass = slot / R_HEAD, rr = slot % R_HEAD;
                    u64 run = 0;
                    int tok = 16 * tile + 15;
                    for (int i = 0; i < 16; ++i) {
                        run += L.earr[pass * (R_HEAD * 16) + rr * 16 + i];
                        if (run > rin) { tok = 16 * tile + i; break; }
                    }
                    __hip_atomic_store(bufc, (u64)(uint32_t)tok | ((u64)tagc << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (tid == 0) L.s_cand[0] = granule(bufc, 0, tagc);
                te_sync();                                           // edge 7: the token
                if (!*L.s_ok) { if (tid == 0) __hip_atomic_store(p.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
                next = (int)(uint32_t)L.s_cand[0];
            }
            n_sampled += 1;
            if (tid == 0) {
                if (t + 1 >= p.n_prompt) *L.s_tok = next;
                if (w == 0) __hip_atomic_store(p.tok_dev + t, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (the relay block takes it to the host)
                if (p.sample && p.win_cap > 0) {                     // the window slides over the generated ids (both sampling forms)
                    int wl = L.win[64];
                    if (wl < p.win_cap) { L.win[wl] = next; L.win[64] = wl + 1; }
                    else { for (int j = 0; j + 1 < wl; ++j) L.win[j] = L.win[j + 1]; L.win[wl - 1] = next; }
                }
                if (next == p.stop_id || *L.s_cancel) *L.s_done = 1;
            }
        }
    }
    if (w == 0 && tid == 0) {
        if (p.n_done) { p.n_done[0] = t_last + 1; p.n_done[1] = n_sampled; }
        __threadfence();                                             // every id above is visible before the relay is told that there are no more
        __hip_atomic_store(p.relay_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The relay: ONE wave on a compute unit no worker uses (block 256 + xcds, i.e. on XCD `xcds`: the blocks with index mod 8 >= xcds have left).  It polls the
// ids worker 0 publishes in device memory and copies them into the host-visible row, and polls the host's cancel word and forwards it
// into device memory - so that no worker ever issues an access that crosses PCIe.  (Round 6, first forms: the id stored to host memory
// by the thread that chose it - a system-scope store retires after a PCIe round trip and vmcnt retires in order, so that wave's next
// loads, and with them every worker's first edge of the position, waited for it; then by a matrix wave behind its tile requests - 512
// extra system-scope stores per position: 17.17 -> 17.56 -> 17.88 ms per request, profiles/r06/c7, c8.)  With 8 XCDs every compute unit
// holds a worker and the relay only runs once they have left: the ids then arrive together at the end - still correct, not streamed.
__device__ __forceinline__ void te_relay(const TeParams& p) {
    if (threadIdx.x != 0) return;
    int k = p.head_from;
    for (long it = 0; it < (1L << 26); ++it) {                       // (bounded: ~1 us per round)
        if (p.cancel && __hip_atomic_load(p.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
            __hip_atomic_store(p.cancel_dev, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (read BEFORE the ids are drained: what worker 0 chose before it raised the flag is then certainly seen below)
        const unsigned fin = __hip_atomic_load(p.relay_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
                             __hip_atomic_load(p.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (k < p.head_until) {
            const int v = __hip_atomic_load(p.tok_dev + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v < 0) break;
            __hip_atomic_store(p.next_tokens + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            ++k;
        }
        if (fin) break;
        __builtin_amdgcn_s_sleep(32);
    }
}


// The code tiles of an MLX-quantised checkpoint (k_token_engine_q, token_engine_q.hip): per layer role the packed codes and scale /
// bias pairs of lm_qgemm.hip (q: bytes, layer stride q_layer; sb: bf16 elements, layer stride sb_layer).  Passed as the kernel's
// second argument; the host side (token_engine.hip) fills it and launches the kernel by address.
struct TeQRole { const uint8_t* q; const bf16_t* sb; size_t q_layer, sb_layer; };
struct TeQParams { TeQRole qkv, o, gu, down, head; int head_nt; };
}   // namespace

// the code-streaming kernel k_token_engine_q<xcds, bits, head_q> (token_engine_q.hip), arguments (TeParams, TeQParams); null if not built
const void* token_engine_q_kernel(int xcds, int bits, bool head_q);
