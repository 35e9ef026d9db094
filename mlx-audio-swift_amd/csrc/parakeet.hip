// parakeet.hip - Parakeet TDT speech-to-text: 16 kHz samples -> NeMo log-mel (per-feature normalisation) -> depthwise-striding Conv2d stem
// (factor 8) -> FastConformer blocks with relative-position attention -> joint.enc over every frame -> greedy TDT decode (embedding, two
// LSTM layers, joint, token and duration arg-max) in ONE launch.  Exact f32 throughout.
//
// Reference being replaced: ParakeetModel (Sources/MLXAudioSTT/Models/Parakeet/ParakeetModel.swift decodeTDTSerial :389-479,
// makeCompiledTDTStep :894-931, ParakeetConformer.swift), NemoDecodingLogic.tdtStep (Nemo/NemoDecodingLogic.swift:41-67), NemoPredictNetwork /
// NemoJointNetwork (Nemo/NemoRNNTLayers.swift), NemoRelPositionMultiHeadAttention (Nemo/NemoAttention.swift).
//
// The front end is audio_front.h's, the stem and the Conformer block are sortformer_kernels.h's (the kernels Sortformer runs, unchanged), with
// the ragged-batch rule of sortformer.hip: every kernel takes the row's own counts, so a row's bits do not depend on its batch.  Two kernels
// are new:
//
//   k_pk_attn   relative-position flash attention for head sizes 65..128 (zero-padded to 128).  64 queries x head x row per block, FOUR
//               waves: wave = qh + 2 dh owns the 32 queries of half qh and the 64 head dimensions of half dh.  Its (q + u) and (q + v)
//               fragments stay in registers (2 x 32), it forms the PARTIAL 32 x 32 content score and the partial 64 x 32 band product over its
//               own 64 dimensions on v_mfma_f32_32x32x2_f32; the two dh waves of a query half exchange the partials through LDS and add
//               them in one fixed order (dh 0 + dh 1), so both hold the same scores and run the same online softmax; each then accumulates
//               O^T for its own 64 output dimensions (2 x 16 accumulators), reading V straight from memory (the MFMA A operand of P V is
//               32 consecutive floats of one key: a coalesced load, no LDS).  LDS: K 32 x 129 + band 96 x 129 + u, v 2 x 128 floats = 67072
//               bytes, two blocks a CU; the band space also carries the staged Q tile, the exchanged partials and the staged output.
//   k_pk_tdt    the whole greedy TDT loop of one row in one block of 1024 threads.  h, c (committed and proposed), the embedding row, the pred
//               projection and the joint vector live in LDS.  A thread owns the four gates of one hidden unit (c and h update without a
//               shuffle) and reads Wx / Wh from copies transposed at finalize ([k][gate][unit]: a wave reads consecutive floats); the
//               joint output is one logit a thread, in passes, from the transposed [joint][logit] copy; the two arg-maxes are fixed-order
//               reductions, ties to the lower index.  The LSTM and the pred projection run once per EMISSION: a blank leaves the state, so
//               the proposal computed behind the last emission stays valid.  The loop bound is static, T_b (max_symbols + 1).
//
// Launches: generate = 2 (front end) + 4 (stem) + 1 (intake) + 15 L + 1 (joint.enc) + 1 (decode) = 9 + 15 L; encode = 7 + 15 L.
#include "common.h"
#define AUDIO_FRONT_NEMO_KERNELS
#include "audio_front.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"
#include "sortformer_kernels.h"

#include <math.h>
#include <string.h>
#include <memory>

#define PK_MAX_BATCH 64
#define PK_MAX_SECONDS 120
#define PK_MAX_DUR 8
#define PK_NT 1024                   // threads of the decode block
#define PK_MAXW 1024                 // pred_hidden, joint_hidden

// ============================================================================ kernel A: attention, head sizes 65..128
// SfAttn as k_sf_attn<.., true> takes it.  LDP: an odd row stride, so the 32 rows a half-wave reads fall into 32 banks.
#define PK_LDP 129
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_pk_attn(SfAttn p) {
    __shared__ float Ks[32][PK_LDP];
    __shared__ float Pb[96 * PK_LDP];                               // the band; between uses: Q tile, exchanged partials, output tile
    __shared__ float Ub[2][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5, qh = wave & 1, dh = wave >> 1;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64, n = min(p.cnt[b], p.Tp), hd = p.hd;
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = tid; i < 64 * hd; i += 256) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0.0f;
        }
        return;
    }
#pragma unroll 4
    for (int i = tid; i < 64 * 128; i += 256) {
        const int r = i >> 7, c = i & 127, tq = q0 + r;
        Pb[r * PK_LDP + c] = (tq < n && c < hd) ? p.qkv[(rowbase + tq) * p.ld + h * hd + c] * p.qscale : 0.0f;
    }
    {
        const int c = tid & 127;
        Ub[tid >> 7][c] = c < hd ? (tid < 128 ? p.u : p.v)[h * hd + c] : 0.0f;
    }
    __syncthreads();
    const int wq = qh * 32, d0 = dh * 64;
    float qf[32];                                                   // the wave's 64 dimensions of query wq + l31; u and v are added at use (LDS), as registers are short
#pragma unroll
    for (int i = 0; i < 32; ++i) qf[i] = Pb[(wq + l31) * PK_LDP + d0 + 2 * i + kh];
    f32x16_t O[2];
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dn][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float* Bd0 = Pb + qh * 2048;                              // band products [64 band rows][32 queries] of dh 0, dh 1
    const float* Bd1 = Pb + (qh + 2) * 2048;
    const float* Sx0 = Pb + 8192 + qh * 1024;                       // content scores [32 keys][32 queries] of dh 0, dh 1
    const float* Sx1 = Pb + 8192 + (qh + 2) * 1024;
    for (int kb = 0; kb < n; kb += 32) {
        __syncthreads();                                            // the previous tile's reads are done (first pass: the Q fragments are taken)
#pragma unroll 4
        for (int i = tid; i < 32 * 128; i += 256) {
            const int r = i >> 7, c = i & 127, key = kb + r;
            Ks[r][c] = (key < n && c < hd) ? p.qkv[(rowbase + key) * p.ld + p.koff + h * hd + c] : 0.0f;
        }
        const int base = q0 - kb - 31 + p.Tcap - 1;                 // table row of band row 0
#pragma unroll 4
        for (int i = tid; i < 96 * 128; i += 256) {
            const int r = i >> 7, c = i & 127, idx = base + r;
            Pb[r * PK_LDP + c] = (idx >= 0 && idx < 2 * p.Tcap - 1 && c < hd) ? p.P[(size_t)idx * p.ldp + h * hd + c] : 0.0f;
        }
        __syncthreads();
        // partial S^T[key][query] and partial band products over the wave's 64 dimensions
        f32x16_t S, G0, G1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = 0.0f; G0[r] = 0.0f; G1[r] = 0.0f; }
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int k = d0 + 2 * i + kh;
            const float qu = qf[i] + Ub[0][k], qv = qf[i] + Ub[1][k];
            S = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31][k], qu, S, 0, 0, 0);
            G0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(wq + l31) * PK_LDP + k], qv, G0, 0, 0, 0);
            G1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(wq + 32 + l31) * PK_LDP + k], qv, G1, 0, 0, 0);
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // keep the operand loads of at most four steps in flight (registers)
        }
        __syncthreads();                                            // every wave has read its band rows: the space becomes the partials'
        {
            float* Bd = Pb + wave * 2048;
            float* Sx = Pb + 8192 + wave * 1024;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int br = f32_tile_row(r, kh);
                Bd[br * 32 + l31] = G0[r];
                Bd[(br + 32) * 32 + l31] = G1[r];
                Sx[br * 32 + l31] = S[r];
            }
        }
        __syncthreads();
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = f32_tile_row(r, kh), at = (l31 - j + 31) * 32 + l31;   // distance i - j, the literal rel-shift's entry
            const float s = (Sx0[j * 32 + l31] + Sx1[j * 32 + l31]) + (Bd0[at] + Bd1[at]);
            S[r] = (kb + j < n) ? s / p.sdk : -INFINITY;
            mx = fmaxf(mx, S[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                       // finite: every tile holds a key < n
        const float alpha = expf(m_run - m_new);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = expf(S[r] - m_new); psum += S[r]; }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int dn = 0; dn < 2; ++dn) {
#pragma unroll
            for (int r = 0; r < 16; ++r) O[dn][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {                          // V^T straight from memory: 32 consecutive floats of key f32_tile_row(r, kh)
                const int key = kb + f32_tile_row(r, kh), d = d0 + dn * 32 + l31;
                const float vv = (key < n && d < hd) ? p.qkv[(rowbase + key) * p.ld + p.voff + h * hd + d] : 0.0f;
                O[dn] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, S[r], O[dn], 0, 0, 0);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    __syncthreads();                                                // the band space is free: the outputs go through it for coalesced stores
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) Pb[(wq + l31) * PK_LDP + d0 + dn * 32 + f32_tile_row(r, kh)] = O[dn][r] / l_tot;
    __syncthreads();
    for (int i = tid; i < 64 * hd; i += 256) {
        const int r = i / hd, c = i - r * hd, t = q0 + r;
        if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + c] = t < n ? Pb[r * PK_LDP + c] : 0.0f;
    }
}

template <class Ctx>
static void pk_attn(Ctx* c, const SfAttn& p, int heads, int hd, int batch) {
    if (hd <= 64) { sf_attn<true>(c, p, heads, hd, batch); return; }
    MIS_LAUNCH(c, k_pk_attn, dim3(cdiv(p.Tp, 64), heads, batch), dim3(256), p);
}

// ============================================================================ kernel B: greedy TDT decode, one block a row
struct PkTdt {
    const float* encp; const int* cnt; int Tp, J, P, V, D;          // joint.enc of every frame [B][Tp][J]; V = vocab + 1 token logits, D durations
    const float *embed, *wxT0, *whT0, *bih0, *bhh0, *wxT1, *whT1, *bih1, *bhh1, *wpT, *bp, *woT, *bo;
    int dur[PK_MAX_DUR], max_symbols, cap;
    int *tokens, *frames, *durs, *count, *flag, *steps;             // [B][cap] x 3, [B] x 3
};

__device__ __forceinline__ float pk_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// one LSTM layer, torch.nn.LSTM's: gates i, f, g, o = (b_ih + b_hh) + W_ih x + W_hh h, k ascending; c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c')
__device__ __forceinline__ void pk_lstm_layer(const float* __restrict__ wxT, const float* __restrict__ whT, const float* __restrict__ bih,
                                              const float* __restrict__ bhh, const float* x, const float* h, const float* c, float* hn, float* cn,
                                              int P) {
    for (int u = threadIdx.x; u < P; u += PK_NT) {
        float g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = bih[q * P + u] + bhh[q * P + u];
        for (int k = 0; k < P; ++k) {
            const float xk = x[k];
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = fmaf(wxT[((size_t)k * 4 + q) * P + u], xk, g[q]);
        }
        for (int k = 0; k < P; ++k) {
            const float hk = h[k];
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = fmaf(whT[((size_t)k * 4 + q) * P + u], hk, g[q]);
        }
        const float cc = pk_sigmoid(g[1]) * c[u] + pk_sigmoid(g[0]) * tanhf(g[2]);
        cn[u] = cc;
        hn[u] = pk_sigmoid(g[3]) * tanhf(cc);
    }
    __syncthreads();
}

__device__ __forceinline__ bool pk_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ void __launch_bounds__(PK_NT) k_pk_tdt(PkTdt p) {
    __shared__ float xs[PK_MAXW], hs[2][PK_MAXW], cs[2][PK_MAXW], hn[2][PK_MAXW], cn[2][PK_MAXW], pp[PK_MAXW], zs[PK_MAXW];
    __shared__ float rv[2][PK_NT / 64];
    __shared__ int ri[2][PK_NT / 64], dec[2], sd[PK_MAX_DUR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, P = p.P, J = p.J, V = p.V, NL = p.V + p.D, blank = p.V - 1;
    const int T = min(p.cnt[b], p.Tp);
    for (int u = tid; u < P; u += PK_NT) { hs[0][u] = 0.0f; hs[1][u] = 0.0f; cs[0][u] = 0.0f; cs[1][u] = 0.0f; }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < PK_MAX_DUR; ++i) sd[i] = p.dur[i];
    }
    // the proposal behind `token` from the committed state: hn, cn and pp = joint.pred(h' of layer 1); a blank feeds zeros, as the reference masks it
    auto predict = [&](int token) {
        for (int u = tid; u < P; u += PK_NT) xs[u] = token == blank ? 0.0f : p.embed[(size_t)token * P + u];
        __syncthreads();
        pk_lstm_layer(p.wxT0, p.whT0, p.bih0, p.bhh0, xs, hs[0], cs[0], hn[0], cn[0], P);
        pk_lstm_layer(p.wxT1, p.whT1, p.bih1, p.bhh1, hn[0], hs[1], cs[1], hn[1], cn[1], P);
        for (int j = tid; j < J; j += PK_NT) {
            float acc = p.bp[j];
            for (int k = 0; k < P; ++k) acc = fmaf(p.wpT[(size_t)k * J + j], hn[1][k], acc);
            pp[j] = acc;
        }
        __syncthreads();
    };
    predict(blank);
    int t = 0, ns = 0, n = 0, steps = 0, flagged = 0;
    const int bound = T * (p.max_symbols + 1);
    int* otok = p.tokens + (size_t)b * p.cap;
    int* ofrm = p.frames + (size_t)b * p.cap;
    int* odur = p.durs + (size_t)b * p.cap;
    for (int it = 0; it < bound && t < T; ++it) {                   // (every branch below is uniform over the block)
        const float* e = p.encp + ((size_t)b * p.Tp + t) * J;
        for (int j = tid; j < J; j += PK_NT) zs[j] = fmaxf(e[j] + pp[j], 0.0f);
        __syncthreads();
        float bv0 = -INFINITY, bv1 = -INFINITY;
        int bi0 = 0x7fffffff, bi1 = 0x7fffffff;
        for (int v = tid; v < NL; v += PK_NT) {
            float acc = p.bo[v];
            for (int j = 0; j < J; ++j) acc = fmaf(p.woT[(size_t)j * NL + v], zs[j], acc);
            if (v < V) { if (pk_better(acc, v, bv0, bi0)) { bv0 = acc; bi0 = v; } }
            else if (pk_better(acc, v - V, bv1, bi1)) { bv1 = acc; bi1 = v - V; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov0 = __shfl_xor(bv0, o, 64), ov1 = __shfl_xor(bv1, o, 64);
            const int oi0 = __shfl_xor(bi0, o, 64), oi1 = __shfl_xor(bi1, o, 64);
            if (pk_better(ov0, oi0, bv0, bi0)) { bv0 = ov0; bi0 = oi0; }
            if (pk_better(ov1, oi1, bv1, bi1)) { bv1 = ov1; bi1 = oi1; }
        }
        if (lane == 0) { rv[0][wave] = bv0; ri[0][wave] = bi0; rv[1][wave] = bv1; ri[1][wave] = bi1; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < PK_NT / 64; ++w) {
                if (pk_better(rv[0][w], ri[0][w], bv0, bi0)) { bv0 = rv[0][w]; bi0 = ri[0][w]; }
                if (pk_better(rv[1][w], ri[1][w], bv1, bi1)) { bv1 = rv[1][w]; bi1 = ri[1][w]; }
            }
            dec[0] = bi0 < V ? bi0 : 0;                             // (no finite logit at all: index 0)
            dec[1] = bi1 < p.D ? bi1 : 0;
        }
        __syncthreads();
        const int tok = dec[0], jump = sd[dec[1]];
        ++steps;
        if (tok != blank) {
            if (n >= p.cap) { flagged = 1; break; }
            if (tid == 0) { otok[n] = tok; ofrm[n] = t; odur[n] = jump; }
            ++n;
            for (int u = tid; u < P; u += PK_NT) { hs[0][u] = hn[0][u]; hs[1][u] = hn[1][u]; cs[0][u] = cn[0][u]; cs[1][u] = cn[1][u]; }
            __syncthreads();
            predict(tok);
        }
        // NemoDecodingLogic.tdtStep
        t += jump;
        ++ns;
        if (jump != 0) ns = 0;
        else if (ns >= p.max_symbols) { t += 1; ns = 0; }
    }
    if (tid == 0) { p.count[b] = n; p.flag[b] = flagged; p.steps[b] = steps; }
}

// the decoder's tensors as a checkpoint holds them (host), and their device form
struct PkDecHost { const float *embed, *wih[2], *whh[2], *bih[2], *bhh[2], *wp, *bp, *wo, *bo; };
struct PkDecDev { DevBuf<float> arena; };

// transposed copies: Wx / Wh [4 P][P] -> [k][gate][unit], joint.pred [J][P] -> [k][j], joint_net [NL][J] -> [j][logit]; plain index arithmetic
static void pk_pack_decoder(const PkDecHost& s, int P, int J, int V, int NL, PkDecDev& dev, PkTdt& p) {
    std::vector<float> blob;
    auto push = [&](const float* src, size_t n) { const size_t o = blob.size(); blob.insert(blob.end(), src, src + n); blob.resize(round_up(blob.size(), 64), 0.0f); return o; };
    auto gatesT = [&](const float* w) {
        std::vector<float> t((size_t)4 * P * P);
        for (int q = 0; q < 4; ++q) for (int u = 0; u < P; ++u) for (int k = 0; k < P; ++k) t[((size_t)k * 4 + q) * P + u] = w[((size_t)q * P + u) * P + k];
        return push(t.data(), t.size());
    };
    auto linT = [&](const float* w, int N, int K) {
        std::vector<float> t((size_t)N * K);
        for (int o = 0; o < N; ++o) for (int k = 0; k < K; ++k) t[(size_t)k * N + o] = w[(size_t)o * K + k];
        return push(t.data(), t.size());
    };
    size_t off[13];
    off[0] = push(s.embed, (size_t)V * P);
    for (int l = 0; l < 2; ++l) { off[1 + 4 * l] = gatesT(s.wih[l]); off[2 + 4 * l] = gatesT(s.whh[l]); off[3 + 4 * l] = push(s.bih[l], 4 * P); off[4 + 4 * l] = push(s.bhh[l], 4 * P); }
    off[9] = linT(s.wp, J, P); off[10] = push(s.bp, J); off[11] = linT(s.wo, NL, J); off[12] = push(s.bo, NL);
    dev.arena.alloc(blob.size());
    HIP_CHECK(hipMemcpy(dev.arena.p, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
    const float* a = dev.arena.p;
    p.embed = a + off[0];
    p.wxT0 = a + off[1]; p.whT0 = a + off[2]; p.bih0 = a + off[3]; p.bhh0 = a + off[4];
    p.wxT1 = a + off[5]; p.whT1 = a + off[6]; p.bih1 = a + off[7]; p.bhh1 = a + off[8];
    p.wpT = a + off[9]; p.bp = a + off[10]; p.woT = a + off[11]; p.bo = a + off[12];
}

static void pk_check_decoder_dims(int P, int J, int vocab, int D, int max_symbols, const int32_t* durations) {
    MIS_REQUIRE(P >= 1 && P <= PK_MAXW, MIS_ERR_INVALID_INPUT, "pred_hidden %d outside 1..%d", P, PK_MAXW);
    MIS_REQUIRE(J >= 1 && J <= PK_MAXW, MIS_ERR_INVALID_INPUT, "joint_hidden %d outside 1..%d", J, PK_MAXW);
    MIS_REQUIRE(vocab >= 1 && vocab <= 65535, MIS_ERR_INVALID_INPUT, "vocab_size %d outside 1..65535", vocab);
    MIS_REQUIRE(D >= 1 && D <= PK_MAX_DUR, MIS_ERR_INVALID_INPUT, "num_durations %d outside 1..%d", D, PK_MAX_DUR);
    MIS_REQUIRE(max_symbols >= 1 && max_symbols <= 64, MIS_ERR_INVALID_INPUT, "max_symbols %d outside 1..64 (without it a blank of duration 0 never ends)", max_symbols);
    for (int i = 0; i < D; ++i) MIS_REQUIRE(durations[i] >= 0 && durations[i] <= 64, MIS_ERR_INVALID_INPUT, "durations[%d] = %d outside 0..64", i, durations[i]);
}

// ============================================================================ host
struct mis_parakeet {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_parakeet_config cfg{};
    int mels = 0, C = 0, d = 0, H = 0, hd = 0, f = 0, L = 0, ck = 0, F1 = 0, F2 = 0, F3 = 0, P = 0, J = 0, V = 0, D = 0, cap = 0;
    HostWeights raw{"Parakeet", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, ptab;
    DevBuf<int> fbr;
    const float *window = nullptr, *twc = nullptr, *tws = nullptr, *fb = nullptr, *c0w = nullptr, *c0b = nullptr, *dw2w = nullptr, *dw2b = nullptr,
                *dw5w = nullptr, *dw5b = nullptr;
    SfLin pw3, pw6, lin, jenc;
    struct Layer {
        const float *ln1w, *ln1b, *lnaw, *lnab, *lncw, *lncb, *ln2w, *ln2b, *lnow, *lnob, *u, *v, *P, *dw, *dwshift;
        SfLin ff1a, ff1b, qkv, o, pw1, pw2, ff2a, ff2b;
    };
    std::vector<Layer> fc;
    PkDecDev dec;
    PkTdt tdt{};
    // workspace (sized at finalize)
    int64_t maxN = 0;
    int Fcap = 0, T1cap = 0, T2cap = 0, Tcap = 0;
    DevBuf<float> pcm, melraw, feats, s0, s1, s2, emb, h, stats, big, qkv, att, encp;
    DevBuf<int> cntN, cntF, cnt1, cnt2, cnt3, outs;                  // outs: tokens, frames, durations [B][cap] each, then count, flag, steps [B] each
    // state of the last call
    int batch = 0, Fp = 0, T1p = 0, T2p = 0, Tp = 0, launches = 0;
    std::vector<int> hN, hF, hT1, hT2, hT3;
    HipEvents<4> ev;
    bool timed = false, timed_done = false, has_emb = false;
};

static inline int pk_half(int t) { return t >= 1 ? (t - 1) / 2 + 1 : 0; }
static inline int pk_frames(int64_t n) { return (int)(1 + n / NEMO_HOP); }

extern "C" mis_status mis_parakeet_create(const mis_parakeet_config* cfg, int device, mis_parakeet** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    const int d = cfg->hidden_size, H = cfg->num_attention_heads;
    MIS_REQUIRE(cfg->sampling_rate == 16000 && cfg->n_fft == NEMO_NFFT && cfg->hop_length == NEMO_HOP && cfg->win_length == NEMO_WIN, MIS_ERR_INVALID_INPUT,
                "sampling_rate / n_fft / hop_length / win_length: only 16000 / 512 / 160 / 400 are implemented");
    MIS_REQUIRE(cfg->preemphasis >= 0.0f && cfg->preemphasis <= 1.0f, MIS_ERR_INVALID_INPUT, "preemphasis outside 0..1");
    MIS_REQUIRE(cfg->num_mel_bins >= 8 && cfg->num_mel_bins <= 256, MIS_ERR_INVALID_INPUT, "num_mel_bins %d outside 8..256", cfg->num_mel_bins);
    MIS_REQUIRE(cfg->subsampling_factor == 8, MIS_ERR_INVALID_INPUT, "subsampling_factor %d: only 8 is implemented", cfg->subsampling_factor);
    MIS_REQUIRE(cfg->subsampling_conv_channels >= 1 && cfg->subsampling_conv_channels <= 1024, MIS_ERR_INVALID_INPUT,
                "subsampling_conv_channels %d outside 1..1024", cfg->subsampling_conv_channels);
    MIS_REQUIRE(d >= 8 && d <= 4096, MIS_ERR_INVALID_INPUT, "hidden_size %d outside 8..4096", d);
    MIS_REQUIRE(H >= 1 && d % H == 0 && d / H <= 128, MIS_ERR_INVALID_INPUT,
                "num_attention_heads %d: head size hidden_size / num_attention_heads must be a whole number up to 128", H);
    MIS_REQUIRE(cfg->intermediate_size >= 1 && cfg->intermediate_size <= 16384, MIS_ERR_INVALID_INPUT, "intermediate_size %d outside 1..16384",
                cfg->intermediate_size);
    MIS_REQUIRE(cfg->num_hidden_layers >= 1 && cfg->num_hidden_layers <= 64, MIS_ERR_INVALID_INPUT, "num_hidden_layers %d outside 1..64", cfg->num_hidden_layers);
    MIS_REQUIRE(cfg->conv_kernel_size >= 3 && cfg->conv_kernel_size <= SF_DW_MAXK && cfg->conv_kernel_size % 2 == 1, MIS_ERR_INVALID_INPUT,
                "conv_kernel_size %d unsupported (odd, 3..%d)", cfg->conv_kernel_size, SF_DW_MAXK);
    MIS_REQUIRE(cfg->pred_rnn_layers == 2, MIS_ERR_INVALID_INPUT, "pred_rnn_layers %d: only 2 is implemented", cfg->pred_rnn_layers);
    pk_check_decoder_dims(cfg->pred_hidden, cfg->joint_hidden, cfg->vocab_size, cfg->num_durations, cfg->max_symbols, cfg->durations);
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= PK_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch %d outside 1..%d", cfg->max_batch, PK_MAX_BATCH);
    MIS_REQUIRE(cfg->max_seconds >= 1 && cfg->max_seconds <= PK_MAX_SECONDS, MIS_ERR_INVALID_INPUT, "max_seconds %d outside 1..%d", cfg->max_seconds,
                PK_MAX_SECONDS);
    MIS_REQUIRE(cfg->max_tokens >= 1 && cfg->max_tokens <= 65536, MIS_ERR_INVALID_INPUT, "max_tokens %d outside 1..65536", cfg->max_tokens);
    hipStream_t stream = mis_open_stream(device);      // first: the handle's events belong to this device
    auto c = std::make_unique<mis_parakeet>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->mels = cfg->num_mel_bins; c->C = cfg->subsampling_conv_channels; c->d = d; c->H = H; c->hd = d / H; c->f = cfg->intermediate_size;
    c->L = cfg->num_hidden_layers; c->ck = cfg->conv_kernel_size;
    c->F1 = pk_half(c->mels); c->F2 = pk_half(c->F1); c->F3 = pk_half(c->F2);
    c->P = cfg->pred_hidden; c->J = cfg->joint_hidden; c->V = cfg->vocab_size + 1; c->D = cfg->num_durations; c->cap = cfg->max_tokens;
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_parakeet_destroy(mis_parakeet* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}

extern "C" mis_status mis_parakeet_set_tensor(mis_parakeet* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 4, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

static const char* const PK_LSTM = "decoder.prediction.dec_rnn.lstm.";

extern "C" mis_status mis_parakeet_finalize(mis_parakeet* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t mels = c->mels, C = c->C, d = c->d, f = c->f, ck = c->ck, F3 = c->F3, H = c->H, hd = c->hd, P = c->P, J = c->J, V = c->V, NL = c->V + c->D;
    const bool ab = c->cfg.attention_bias != 0;
    HostArena a(c->raw);
    std::vector<float>& fh = a.fhost;
    const size_t o_win = a.ftake(NEMO_NFFT, c->window), o_twc = a.ftake(NEMO_NFFT / 2, c->twc), o_tws = a.ftake(NEMO_NFFT / 2, c->tws);
    hann_padded(&fh[o_win], NEMO_WIN, NEMO_NFFT);
    fft512_twiddles(&fh[o_twc], &fh[o_tws]);
    const size_t o_fb = a.ftake((size_t)NEMO_BINS * mels, c->fb);
    std::vector<int> ranges(2 * mels, 0);
    slaney_filterbank(&fh[o_fb], ranges.data(), NEMO_BINS, (int)mels, 16000.0, NEMO_NFFT);
    c->maxN = (int64_t)c->cfg.max_seconds * 16000;
    c->Fcap = pk_frames(c->maxN); c->T1cap = pk_half(c->Fcap); c->T2cap = pk_half(c->T1cap); c->Tcap = pk_half(c->T2cap);
    const int Tc = c->Tcap, NP = 2 * Tc - 1;
    auto lin = [&](const std::string& p, int64_t N, int64_t K, bool bias, SfLin& l) {
        l = SfLin{};
        a.fvec(p + ".weight", {N, K}, N * K, l.w);
        if (bias) a.fvec(p + ".bias", {N}, N, l.b);
    };
    auto norm = [&](const std::string& p, int64_t n, const float*& w, const float*& b) { a.fvec(p + ".weight", {n}, n, w); a.fvec(p + ".bias", {n}, n, b); };
    const std::string SUB = "encoder.subsampling.";
    auto taps9 = [&](const std::string& name, const float*& dst) {    // conv taps [C][3][3][1] -> [9][C]
        const HostTensor& t = c->raw.need(name, {C, 3, 3, 1});
        const size_t off = a.ftake(9 * C, dst);
        for (int64_t ch = 0; ch < C; ++ch) for (int k = 0; k < 9; ++k) fh[off + k * C + ch] = t.v[ch * 9 + k];
    };
    taps9(SUB + "layers_0.weight", c->c0w); a.fvec(SUB + "layers_0.bias", {C}, C, c->c0b);
    taps9(SUB + "layers_2.weight", c->dw2w); a.fvec(SUB + "layers_2.bias", {C}, C, c->dw2b);
    a.fvec(SUB + "layers_3.weight", {C, 1, 1, C}, C * C, c->pw3.w); a.fvec(SUB + "layers_3.bias", {C}, C, c->pw3.b);
    taps9(SUB + "layers_5.weight", c->dw5w); a.fvec(SUB + "layers_5.bias", {C}, C, c->dw5b);
    a.fvec(SUB + "layers_6.weight", {C, 1, 1, C}, C * C, c->pw6.w); a.fvec(SUB + "layers_6.bias", {C}, C, c->pw6.b);
    {   // linear [d][C F3] reads the flattening (c, f); the stem keeps channels last: columns re-ordered to (f, c)
        const size_t ow = a.ftake((size_t)d * C * F3, c->lin.w);
        a.fvec(SUB + "linear.bias", {d}, d, c->lin.b);
        const HostTensor& w = c->raw.need(SUB + "linear.weight", {d, C * F3});
        for (int64_t n = 0; n < d; ++n) for (int64_t ch = 0; ch < C; ++ch) for (int64_t fq = 0; fq < F3; ++fq)
            fh[ow + (n * F3 + fq) * C + ch] = w.v[n * C * F3 + ch * F3 + fq];
    }
    c->fc.assign(c->L, mis_parakeet::Layer{});
    std::vector<SfLin> rk(c->L);
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li) + ".";
        mis_parakeet::Layer& l = c->fc[li];
        norm(q + "norm_feed_forward1", d, l.ln1w, l.ln1b);
        lin(q + "feed_forward1.linear1", f, d, ab, l.ff1a); lin(q + "feed_forward1.linear2", d, f, ab, l.ff1b);
        norm(q + "norm_self_att", d, l.lnaw, l.lnab);
        {   // q, k, v over the same input as one [3 d][d]; an absent bias is zero
            const size_t ow = a.ftake((size_t)3 * d * d, l.qkv.w), ob = a.ftake(3 * d, l.qkv.b);
            const char* names[3] = {"q_proj", "k_proj", "v_proj"};
            for (int i = 0; i < 3; ++i) {
                const HostTensor& w = c->raw.need(q + "self_attn." + names[i] + ".weight", {d, d});
                std::copy(w.v.begin(), w.v.end(), fh.begin() + ow + (size_t)i * d * d);
                if (ab) { const HostTensor& bb = c->raw.need(q + "self_attn." + names[i] + ".bias", {d}); std::copy(bb.v.begin(), bb.v.end(), fh.begin() + ob + (size_t)i * d); }
            }
        }
        lin(q + "self_attn.o_proj", d, d, ab, l.o);
        a.fvec(q + "self_attn.relative_k_proj.weight", {d, d}, d * d, rk[li].w);
        a.fvec(q + "self_attn.bias_u", {H, hd}, d, l.u); a.fvec(q + "self_attn.bias_v", {H, hd}, d, l.v);
        norm(q + "norm_conv", d, l.lncw, l.lncb);
        a.fvec(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, 2 * d * d, l.pw1.w);
        a.fvec(q + "conv.pointwise_conv2.weight", {d, 1, d}, d * d, l.pw2.w);
        if (ab) { a.fvec(q + "conv.pointwise_conv1.bias", {2 * d}, 2 * d, l.pw1.b); a.fvec(q + "conv.pointwise_conv2.bias", {d}, d, l.pw2.b); }
        const HostTensor& dw = c->raw.need(q + "conv.depthwise_conv.weight", {d, ck, 1});
        const HostTensor* dwb = ab ? &c->raw.need(q + "conv.depthwise_conv.bias", {d}) : nullptr;
        const HostTensor& bw = c->raw.need(q + "conv.norm.weight", {d}); const HostTensor& bb = c->raw.need(q + "conv.norm.bias", {d});
        const HostTensor& bm = c->raw.need(q + "conv.norm.running_mean", {d}); const HostTensor& bv = c->raw.need(q + "conv.norm.running_var", {d});
        const size_t o_dw = a.ftake((size_t)ck * d, l.dw), o_sh = a.ftake(d, l.dwshift);
        fold_bn_dwconv(&fh[o_dw], &fh[o_sh], dw.v.data(), dwb ? dwb->v.data() : nullptr, bw.v.data(), bb.v.data(), bm.v.data(), bv.v.data(), d, ck);
        norm(q + "norm_feed_forward2", d, l.ln2w, l.ln2b);
        lin(q + "feed_forward2.linear1", f, d, ab, l.ff2a); lin(q + "feed_forward2.linear2", d, f, ab, l.ff2b);
        norm(q + "norm_out", d, l.lnow, l.lnob);
    }
    lin("joint.enc", J, d, true, c->jenc);
    // the sinusoid table by distance: row dist + Tcap - 1, columns interleaved sin, cos; formed in double, rounded once
    const float* tab = nullptr;
    const size_t o_tab = a.ftake((size_t)NP * d, tab);
    for (int r = 0; r < NP; ++r) {
        const double dist = (double)(r - (Tc - 1));
        for (int64_t k = 0; 2 * k < d; ++k) {
            const double ang = dist * exp(-(double)(2 * k) * log(10000.0) / (double)d);
            fh[o_tab + (size_t)r * d + 2 * k] = (float)sin(ang);
            if (2 * k + 1 < d) fh[o_tab + (size_t)r * d + 2 * k + 1] = (float)cos(ang);
        }
    }
    // the decoder, checked before anything is uploaded
    PkDecHost s{};
    s.embed = c->raw.need("decoder.prediction.embed.weight", {V, P}).v.data();
    for (int l = 0; l < 2; ++l) {
        const std::string n = std::to_string(l);
        s.wih[l] = c->raw.need(PK_LSTM + ("weight_ih_l" + n), {4 * P, P}).v.data(); s.whh[l] = c->raw.need(PK_LSTM + ("weight_hh_l" + n), {4 * P, P}).v.data();
        s.bih[l] = c->raw.need(PK_LSTM + ("bias_ih_l" + n), {4 * P}).v.data(); s.bhh[l] = c->raw.need(PK_LSTM + ("bias_hh_l" + n), {4 * P}).v.data();
    }
    s.wp = c->raw.need("joint.pred.weight", {J, P}).v.data(); s.bp = c->raw.need("joint.pred.bias", {J}).v.data();
    s.wo = c->raw.need("joint.joint_net.weight", {NL, J}).v.data(); s.bo = c->raw.need("joint.joint_net.bias", {NL}).v.data();
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    pk_pack_decoder(s, (int)P, (int)J, (int)V, (int)NL, c->dec, c->tdt);
    c->fbr.alloc(2 * mels);
    HIP_CHECK(hipMemcpy(c->fbr.p, ranges.data(), 2 * mels * sizeof(int), hipMemcpyHostToDevice));
    c->ptab.alloc((size_t)c->L * NP * d);                          // each layer's relative_k_proj of the table: one GEMM, once
    for (int li = 0; li < c->L; ++li) {
        float* dst = c->ptab.p + (size_t)li * NP * d;
        sf_gemm(c, sf_lin(tab, (int)d, rk[li], dst, (int)d, nullptr, NP), 1);
        c->fc[li].P = dst;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->launches = 0;
    const size_t B = c->cfg.max_batch, M = B * Tc;
    c->pcm.alloc(B * c->maxN); c->melraw.alloc(B * c->Fcap * mels); c->feats.alloc(B * c->Fcap * mels);
    c->s0.alloc(B * c->T1cap * c->F1 * C); c->s1.alloc(B * c->T2cap * c->F2 * C); c->s2.alloc(M * F3 * C); c->emb.alloc(M * d);
    c->h.alloc(M * d); c->stats.alloc(M * 2); c->big.alloc(M * std::max<size_t>(f, 2 * d)); c->qkv.alloc(M * 3 * d); c->att.alloc(M * d);
    c->encp.alloc(M * J);
    c->cntN.alloc(B); c->cntF.alloc(B); c->cnt1.alloc(B); c->cnt2.alloc(B); c->cnt3.alloc(B);
    c->outs.alloc(3 * B * c->cap + 3 * B);
    c->tdt.J = (int)J; c->tdt.P = (int)P; c->tdt.V = (int)V; c->tdt.D = c->D; c->tdt.max_symbols = c->cfg.max_symbols; c->tdt.cap = c->cap;
    for (int i = 0; i < PK_MAX_DUR; ++i) c->tdt.dur[i] = i < c->D ? c->cfg.durations[i] : 1;
    c->tdt.tokens = c->outs.p; c->tdt.frames = c->outs.p + B * c->cap; c->tdt.durs = c->outs.p + 2 * B * c->cap;
    c->tdt.count = c->outs.p + 3 * B * c->cap; c->tdt.flag = c->tdt.count + B; c->tdt.steps = c->tdt.flag + B;
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of the engine
extern "C" mis_status mis_parakeet_init_synthetic(mis_parakeet* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    const int64_t C = c->C, d = c->d, f = c->f, ck = c->ck, P = c->P, J = c->J, V = c->V, NL = c->V + c->D;
    const bool ab = c->cfg.attention_bias != 0;
    const std::string SUB = "encoder.subsampling.";
    for (const char* n : {"layers_0", "layers_2", "layers_5"}) { sw.put(SUB + n + ".weight", {C, 3, 3, 1}, sqrt(3.0 / 9.0), 0.0f); sw.put(SUB + n + ".bias", {C}, 0.05, 0.0f); }
    for (const char* n : {"layers_3", "layers_6"}) { sw.put(SUB + n + ".weight", {C, 1, 1, C}, sqrt(3.0 / (double)C), 0.0f); sw.put(SUB + n + ".bias", {C}, 0.05, 0.0f); }
    sw.lin(SUB + "linear", d, C * c->F3, true, 1.0);
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li) + ".";
        for (const char* n : {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"}) sw.norm(q + n, d);
        for (const char* n : {"feed_forward1", "feed_forward2"}) { sw.lin(q + n + ".linear1", f, d, ab, 1.0); sw.lin(q + n + ".linear2", d, f, ab, 0.5); }
        for (const char* n : {"q_proj", "k_proj", "v_proj"}) sw.lin(q + "self_attn." + n, d, d, ab, 1.0);
        sw.lin(q + "self_attn.o_proj", d, d, ab, 0.5);
        sw.lin(q + "self_attn.relative_k_proj", d, d, false, 1.0);
        sw.put(q + "self_attn.bias_u", {c->H, c->hd}, 0.1, 0.0f); sw.put(q + "self_attn.bias_v", {c->H, c->hd}, 0.1, 0.0f);
        sw.put(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, sqrt(3.0 / (double)d), 0.0f);
        sw.put(q + "conv.pointwise_conv2.weight", {d, 1, d}, 0.5 * sqrt(3.0 / (double)d), 0.0f);
        sw.put(q + "conv.depthwise_conv.weight", {d, ck, 1}, sqrt(3.0 / (double)ck), 0.0f);
        if (ab) {
            sw.put(q + "conv.pointwise_conv1.bias", {2 * d}, 0.05, 0.0f); sw.put(q + "conv.pointwise_conv2.bias", {d}, 0.05, 0.0f);
            sw.put(q + "conv.depthwise_conv.bias", {d}, 0.05, 0.0f);
        }
        sw.put(q + "conv.norm.weight", {d}, 0.1, 1.0f); sw.put(q + "conv.norm.bias", {d}, 0.05, 0.0f);
        sw.put(q + "conv.norm.running_mean", {d}, 0.05, 0.0f); sw.put(q + "conv.norm.running_var", {d}, 0.1, 1.0f);
    }
    sw.put("decoder.prediction.embed.weight", {V, P}, 1.0, 0.0f);
    for (int l = 0; l < 2; ++l) {
        const std::string n = std::to_string(l);
        sw.put(PK_LSTM + ("weight_ih_l" + n), {4 * P, P}, sqrt(3.0 / (double)P), 0.0f); sw.put(PK_LSTM + ("weight_hh_l" + n), {4 * P, P}, sqrt(3.0 / (double)P), 0.0f);
        sw.put(PK_LSTM + ("bias_ih_l" + n), {4 * P}, 0.05, 0.0f); sw.put(PK_LSTM + ("bias_hh_l" + n), {4 * P}, 0.05, 0.0f);
    }
    sw.lin("joint.enc", J, d, true, 1.0); sw.lin("joint.pred", J, P, true, 1.0); sw.lin("joint.joint_net", NL, J, true, 4.0);
    MIS_API_END
}

// ============================================================================ the chain
extern "C" int mis_parakeet_launches(const mis_parakeet* c) { return c ? c->launches : 0; }

extern "C" mis_status mis_parakeet_frames(const mis_parakeet* c, const int64_t* lens, int batch, int32_t* F_out, int32_t* T_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    const int64_t cap = (int64_t)c->cfg.max_seconds * 16000;
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] <= cap, MIS_ERR_INVALID_INPUT, "row %d: %lld samples outside 0..%lld (max_seconds %d)", b, (long long)lens[b],
                    (long long)cap, c->cfg.max_seconds);
        const int F = pk_frames(lens[b]);
        if (F_out) F_out[b] = F;
        if (T_out) T_out[b] = pk_half(pk_half(pk_half(F)));
    }
    MIS_API_END
}

// judged first (nothing of the handle is written), then taken: counts uploaded, pcm copied, the front end and the stem launched (6 launches)
static void pk_front_stem(mis_parakeet* c, const float* pcm, const int64_t* lens, int batch, int64_t stride) {
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch %d outside 1..%d (max_batch)", batch, c->cfg.max_batch);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    std::vector<int> N(batch), F(batch), t1(batch), t2(batch), t3(batch);
    int Fp = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the row stride %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->maxN, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the workspace of %d seconds (max_seconds)", b, (long long)n,
                    c->cfg.max_seconds);
        N[b] = (int)n; F[b] = pk_frames(n); t1[b] = pk_half(F[b]); t2[b] = pk_half(t1[b]); t3[b] = pk_half(t2[b]);
        Fp = std::max(Fp, F[b]);
    }
    c->hN = N; c->hF = F; c->hT1 = t1; c->hT2 = t2; c->hT3 = t3;
    c->batch = batch; c->Fp = Fp; c->T1p = pk_half(Fp); c->T2p = pk_half(c->T1p); c->Tp = pk_half(c->T2p);
    c->launches = 0; c->has_emb = false; c->timed_done = false;
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->cntN.p, c->hN.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cntF.p, c->hF.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt1.p, c->hT1.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt2.p, c->hT2.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt3.p, c->hT3.data(), batch * 4, hipMemcpyHostToDevice, s));
    const int64_t ws = std::min<int64_t>(stride, c->maxN);
    HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, ws * 4, pcm, stride * 4, ws * 4, batch, hipMemcpyDefault, s));
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[0], s));
    MIS_LAUNCH(c, k_nemo_log_mel<false>, dim3(Fp, batch), dim3(256), c->pcm.p, ws, c->cntN.p, c->cntF.p, (const float*)nullptr, c->cfg.preemphasis, c->window,
               c->twc, c->tws, c->fb, c->fbr.p, c->melraw.p, Fp, c->mels);
    MIS_LAUNCH(c, k_nemo_norm, dim3(cdiv(c->mels, 64), batch), dim3(256), c->melraw.p, c->cntF.p, c->feats.p, Fp, c->mels, c->cfg.normalize);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[1], s));
    const int B = batch, C = c->C, F1 = c->F1, F2 = c->F2, F3 = c->F3;
    const size_t n0 = (size_t)B * c->T1p * F1 * C;
    MIS_LAUNCH(c, k_sf_conv0, dim3((unsigned)((n0 + 255) / 256)), dim3(256), c->feats.p, c->cntF.p, c->cnt1.p, c->c0w, c->c0b, c->s0.p, c->Fp, c->mels, c->T1p,
               F1, C, n0);
    auto dwpw = [&](const float* in, const int* cin, int Tin, int Fin, const float* dww, const float* dwb, const SfLin& pw, float* out, const int* cout,
                    int Tout, int Fout) {
        SfGemm p{};
        p.X = in; p.ldx = C; p.W = pw.w; p.bias = pw.b; p.Y = out; p.ldy = C; p.cnt = cout; p.Tp = Tout; p.rowmul = Fout; p.K = C; p.N = C;
        p.load = SF_LOAD_DW; p.act = SF_ACT_RELU; p.cnt_in = cin; p.Tin = Tin; p.Fin = Fin; p.Fout = Fout; p.dww = dww; p.dwb = dwb;
        sf_gemm(c, p, B);
    };
    dwpw(c->s0.p, c->cnt1.p, c->T1p, F1, c->dw2w, c->dw2b, c->pw3, c->s1.p, c->cnt2.p, c->T2p, F2);
    dwpw(c->s1.p, c->cnt2.p, c->T2p, F2, c->dw5w, c->dw5b, c->pw6, c->s2.p, c->cnt3.p, c->Tp, F3);
    sf_gemm(c, sf_lin(c->s2.p, F3 * C, c->lin, c->emb.p, c->d, c->cnt3.p, c->Tp), B);
    c->has_emb = true;
}

// c->emb -> the Conformer blocks -> c->h (1 + 15 L launches); stop: -1 all, 1 .. L behind that block
static void pk_encoder(mis_parakeet* c, int stop) {
    const int B = c->batch, Tp = c->Tp, d = c->d, f = c->f, M = B * Tp;
    const int* cnt = c->cnt3.p;
    const size_t nd = (size_t)M * d;
    MIS_LAUNCH(c, k_sf_intake, dim3((unsigned)((nd + 255) / 256)), dim3(256), c->emb.p, c->h.p, cnt, Tp, d, c->cfg.scale_input ? sqrtf((float)d) : 1.0f, nd);
    auto stats = [&](const float* x) { MIS_LAUNCH(c, k_sf_stats, dim3(cdiv(M, 4)), dim3(256), x, c->stats.p, d, 1e-5f, M); };
    auto ln_lin = [&](const float* x, const float* w, const float* b, const SfLin& l, float* y, int N, int act) {
        SfGemm p = sf_lin(x, d, l, y, N, cnt, Tp, act);
        p.load = SF_LOAD_LN; p.stats = c->stats.p; p.lnw = w; p.lnb = b;
        sf_gemm(c, p, B);
    };
    auto res_lin = [&](const float* x, int K, const SfLin& l, float* hres, int N, float ra) {
        SfGemm p = sf_lin(x, K, l, hres, N, cnt, Tp);
        p.R = hres; p.ldr = N; p.ra = ra;
        sf_gemm(c, p, B);
    };
    for (int li = 0; li < c->L; ++li) {                            // 15 launches a block
        const mis_parakeet::Layer& l = c->fc[li];
        stats(c->h.p);
        ln_lin(c->h.p, l.ln1w, l.ln1b, l.ff1a, c->big.p, f, SF_ACT_SILU);
        res_lin(c->big.p, f, l.ff1b, c->h.p, d, 0.5f);
        stats(c->h.p);
        ln_lin(c->h.p, l.lnaw, l.lnab, l.qkv, c->qkv.p, 3 * d, SF_ACT_NONE);
        SfAttn ap{c->qkv.p, 3 * d, d, 2 * d, c->att.p, d, cnt, Tp, c->hd, 1.0f, sqrtf((float)c->hd), l.u, l.v, l.P, d, c->Tcap};
        pk_attn(c, ap, c->H, c->hd, B);
        res_lin(c->att.p, d, l.o, c->h.p, d, 1.0f);
        stats(c->h.p);
        ln_lin(c->h.p, l.lncw, l.lncb, l.pw1, c->big.p, 2 * d, SF_ACT_NONE);
        MIS_LAUNCH(c, k_sf_glu_dwconv, dim3(cdiv(Tp, SF_DW_TT), cdiv(d, 64), B), dim3(256), c->big.p, l.dw, l.dwshift, cnt, c->att.p, Tp, d, c->ck);
        res_lin(c->att.p, d, l.pw2, c->h.p, d, 1.0f);
        stats(c->h.p);
        ln_lin(c->h.p, l.ln2w, l.ln2b, l.ff2a, c->big.p, f, SF_ACT_SILU);
        res_lin(c->big.p, f, l.ff2b, c->h.p, d, 0.5f);
        MIS_LAUNCH(c, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), c->h.p, c->h.p, l.lnow, l.lnob, d, 1e-5f, M, cnt, Tp);
        if (stop == li + 1) return;
    }
}

static void pk_joint_enc(mis_parakeet* c) { sf_gemm(c, sf_lin(c->h.p, c->d, c->jenc, c->encp.p, c->J, c->cnt3.p, c->Tp), c->batch); }

static void pk_sync(mis_parakeet* c) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));                    // the call's one synchronisation
}

extern "C" mis_status mis_parakeet_encode(mis_parakeet* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    pk_front_stem(c, pcm, lens, batch, stride);
    pk_encoder(c, -1);
    HIP_CHECK(hipMemcpyAsync(out, c->h.p, (size_t)batch * c->Tp * c->d * 4, hipMemcpyDeviceToHost, c->stream));
    pk_sync(c);
    MIS_API_END
}

extern "C" mis_status mis_parakeet_generate(mis_parakeet* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int32_t* tokens,
                                            int32_t* frames, int32_t* durations, int32_t* counts, int32_t* flags, int32_t* steps) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && tokens && frames && durations && counts && flags, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    pk_front_stem(c, pcm, lens, batch, stride);
    pk_encoder(c, -1);
    pk_joint_enc(c);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[2], s));
    PkTdt p = c->tdt;
    p.encp = c->encp.p; p.cnt = c->cnt3.p; p.Tp = c->Tp;
    MIS_LAUNCH(c, k_pk_tdt, dim3(batch), dim3(PK_NT), p);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[3], s));
    const size_t n = (size_t)batch * c->cap;
    HIP_CHECK(hipMemcpyAsync(tokens, p.tokens, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(frames, p.frames, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(durations, p.durs, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(counts, p.count, batch * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(flags, p.flag, batch * 4, hipMemcpyDeviceToHost, s));
    if (steps) HIP_CHECK(hipMemcpyAsync(steps, p.steps, batch * 4, hipMemcpyDeviceToHost, s));
    pk_sync(c);
    c->timed_done = c->timed;
    MIS_API_END
}

// tensors of the last encode / generate, f32, zero rows behind a row's own T: stage 0 the stem's embeddings [B, T, hidden], 1 .. L that Conformer
// block, L + 1 joint.enc of the last block [B, T, joint_hidden].  The chain is deterministic: stages >= 1 are recomputed from the embeddings.
extern "C" mis_status mis_parakeet_tap(mis_parakeet* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && dims, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized && c->batch > 0 && c->has_emb, MIS_ERR_NOT_INITIALIZED, "no call to tap: the last call must be encode or generate");
    MIS_REQUIRE(stage >= 0 && stage <= c->L + 1, MIS_ERR_INVALID_INPUT, "stage %d outside 0..%d", stage, c->L + 1);
    HIP_CHECK(hipSetDevice(c->device));
    const int width = stage <= c->L ? c->d : c->J;
    dims[0] = c->batch; dims[1] = c->Tp; dims[2] = width;
    if (!out) return MIS_OK;
    const size_t n = (size_t)c->batch * c->Tp * width;
    MIS_REQUIRE((int64_t)n <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    const int kept = c->launches;
    if (stage >= 1) pk_encoder(c, stage > c->L ? -1 : stage);
    if (stage == c->L + 1) pk_joint_enc(c);
    c->launches = kept;
    const float* src = stage == 0 ? c->emb.p : stage <= c->L ? c->h.p : c->encp.p;
    HIP_CHECK(hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToHost, c->stream));
    pk_sync(c);
    MIS_API_END
}

// ============================================================================ test and bench scaffolding (include/mi_speech_debug.h)
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

// benches: device milliseconds of the next / last mis_parakeet_generate: front end, stem + Conformer blocks + joint.enc, decode
extern "C" mis_status mis_debug_parakeet_timing(mis_parakeet* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    if (!ms) { c->timed = true; return MIS_OK; }
    MIS_REQUIRE(c->timed && c->timed_done, MIS_ERR_NOT_INITIALIZED, "no timed generate: the last call must be mis_parakeet_generate");
    for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    MIS_API_END
}

namespace {
struct PkdCtx { hipStream_t stream = nullptr; int launches = 0; };
constexpr int64_t PKD_MAX_ELEMS = (int64_t)1 << 28;
void pkd_sync(const PkdCtx& c) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
}
const float* pkd_fp(const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); }
}  // namespace

// ONE launch of k_pk_attn on caller-supplied host data; guards as mis_debug_sortformer_attn: the output is [guard | body | guard] of 0xFF
// bytes, every input is followed by NaNs (counts: 0x7FFFFFFF)
extern "C" mis_status mis_debug_parakeet_attn(int device, const float* qkv, int ld, int koff, int voff, const int32_t* cnt, int batch, int Tp, int heads, int hd,
                                              float qscale, float sdk, const float* u, const float* v, const float* P, int ldp, int Tcap, int ldo, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(qkv && cnt && out && u && v && P && batch >= 1 && Tp >= 1 && heads >= 1 && hd >= 65 && hd <= 128 && Tcap >= 1, MIS_ERR_INVALID_INPUT,
                "Parakeet attention: every pointer, positive batch, Tp, heads, Tcap and a head size of 65..128 are required");
    const int64_t width = (int64_t)heads * hd;
    MIS_REQUIRE(koff >= 0 && voff >= 0 && width <= ld && koff + width <= ld && voff + width <= ld && width <= ldo && ldp >= width, MIS_ERR_INVALID_INPUT,
                "Parakeet attention: q, k and v must lie inside a row of ld columns, the output inside ldo, the table inside ldp");
    MIS_REQUIRE((int64_t)batch * Tp * ld <= PKD_MAX_ELEMS && (int64_t)batch * Tp * ldo <= PKD_MAX_ELEMS && (2 * (int64_t)Tcap - 1) * ldp <= PKD_MAX_ELEMS &&
                    batch <= 65535 && heads <= 65535, MIS_ERR_INVALID_INPUT, "Parakeet attention: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    PkdCtx c;
    const size_t rows = (size_t)batch * Tp;
    DevBuf<uint32_t> dq, dcnt, du, dv, dP;
    alloc32(dq, qkv, rows * ld, F32_NAN);
    alloc32(dcnt, cnt, batch, 0x7FFFFFFFu);
    alloc32(du, u, width, F32_NAN); alloc32(dv, v, width, F32_NAN); alloc32(dP, P, (size_t)(2 * Tcap - 1) * ldp, F32_NAN);
    GuardedOut o;
    o.alloc(rows * ldo * 4, (size_t)64 * ldo * 4);
    SfAttn p{pkd_fp(dq), ld, koff, voff, reinterpret_cast<float*>(o.p()), ldo, reinterpret_cast<const int*>(dcnt.p), Tp, hd, qscale, sdk, pkd_fp(du), pkd_fp(dv),
             pkd_fp(dP), ldp, Tcap};
    pk_attn(&c, p, heads, hd, batch);
    pkd_sync(c);
    o.check_guards();
    std::vector<uint32_t> hbuf(o.body / 4);
    HIP_CHECK(hipMemcpy(hbuf.data(), o.p(), o.body, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        memcpy(out + r * width, hbuf.data() + r * ldo, width * 4);
        for (size_t col = width; col < (size_t)ldo; ++col)
            MIS_REQUIRE(hbuf[r * ldo + col] == 0xFFFFFFFFu, MIS_ERR_GENERATION_FAILED, "the kernel wrote column %zu of row %zu behind its %lld columns", col, r, (long long)width);
    }
    MIS_API_END
}

// ONE launch of k_pk_tdt on caller-supplied projected frames encp [batch][Tp][J] (joint.enc applied, bias included) and the decoder's tensors
// as a checkpoint holds them; outputs [batch][cap] x 3 and [batch] x 3.  The token outputs are guarded; entries behind a row's count stay 0xFF.
extern "C" mis_status mis_debug_parakeet_tdt(int device, const float* encp, const int32_t* cnt, int batch, int Tp, int J, int P, int vocab, int D,
                                             const int32_t* durations, int max_symbols, int cap, const float* embed, const float* const* wih,
                                             const float* const* whh, const float* const* bih, const float* const* bhh, const float* wp, const float* bp,
                                             const float* wo, const float* bo, int32_t* tokens, int32_t* frames, int32_t* durs, int32_t* counts, int32_t* flags,
                                             int32_t* steps) {
    MIS_API_BEGIN
    MIS_REQUIRE(encp && cnt && durations && embed && wih && whh && bih && bhh && wp && bp && wo && bo && tokens && frames && durs && counts && flags && steps,
                MIS_ERR_INVALID_INPUT, "Parakeet TDT: null argument");
    MIS_REQUIRE(batch >= 1 && batch <= 65535 && Tp >= 1 && cap >= 1 && (int64_t)batch * Tp * J <= PKD_MAX_ELEMS && (int64_t)batch * cap <= PKD_MAX_ELEMS,
                MIS_ERR_INVALID_INPUT, "Parakeet TDT: positive batch, Tp, cap are required");
    pk_check_decoder_dims(P, J, vocab, D, max_symbols, durations);
    HIP_CHECK(hipSetDevice(device));
    PkdCtx c;
    PkTdt p{};
    PkDecDev dev;
    PkDecHost s{embed, {wih[0], wih[1]}, {whh[0], whh[1]}, {bih[0], bih[1]}, {bhh[0], bhh[1]}, wp, bp, wo, bo};
    const int V = vocab + 1;
    pk_pack_decoder(s, P, J, V, V + D, dev, p);
    DevBuf<uint32_t> de, dc;
    alloc32(de, encp, (size_t)batch * Tp * J, F32_NAN);
    alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    GuardedOut o;
    const size_t n = (size_t)batch * cap;
    o.alloc((3 * n + 3 * batch) * 4, 4096);
    int* ob = reinterpret_cast<int*>(o.p());
    p.encp = pkd_fp(de); p.cnt = reinterpret_cast<const int*>(dc.p); p.Tp = Tp; p.J = J; p.P = P; p.V = V; p.D = D; p.max_symbols = max_symbols; p.cap = cap;
    for (int i = 0; i < PK_MAX_DUR; ++i) p.dur[i] = i < D ? durations[i] : 1;
    p.tokens = ob; p.frames = ob + n; p.durs = ob + 2 * n; p.count = ob + 3 * n; p.flag = p.count + batch; p.steps = p.flag + batch;
    MIS_LAUNCH(&c, k_pk_tdt, dim3(batch), dim3(PK_NT), p);
    pkd_sync(c);
    o.check_guards();
    HIP_CHECK(hipMemcpy(tokens, p.tokens, n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(frames, p.frames, n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(durs, p.durs, n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(counts, p.count, batch * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(flags, p.flag, batch * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(steps, p.steps, batch * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}
