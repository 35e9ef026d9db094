// nemotron_kernels.h - what the offline Nemotron engine (nemotron.hip) and its cache-aware stream session (nemotron_stream.hip) share:
// the operand loads added to k_sf_gemm, the causal stem's first conv, the attention / decode parameter blocks, the decoder packing and the
// model handle.  Every kernel sits in an unnamed namespace: each of the two files gets its own copy, with the bits it always had.
#pragma once
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

#define NM_MAX_BATCH 64
#define NM_MAX_SECONDS 1200
#define NM_MAX_CONTEXTS 8
#define NM_NT 1024                   // threads of the decode block
#define NM_MAXW 1024                 // pred_hidden, joint_hidden
#define NM_DW_TT 16                  // frames of a conv-module block
#define NM_UNLIMITED (1 << 20)       // left chunks of an unlimited left context

// ============================================================================ the operand loads this engine adds to k_sf_gemm
enum { NM_LOAD_DWC = 16, NM_LOAD_LN_SILU, NM_LOAD_PROMPT };
namespace {
// SF_LOAD_DW with pad (2, 1): value = dwb[k] + sum_ij dww[3 i + j][k] X[2 t + i - 2][2 f + j - 2][k], zero outside the row's frames and Fin
template <>
__device__ __forceinline__ float sf_load<NM_LOAD_DWC>(const SfGemm& p, int b, size_t row, int r, int ci) {
    const int t = r / p.Fout, f = r - t * p.Fout, n = min(p.cnt_in[b], p.Tin);
    const float* x = p.X + (size_t)b * p.Tin * p.Fin * p.K;
    float acc = p.dwb[ci];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int ti = 2 * t + a - 2;
        if (ti < 0 || ti >= n) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int fi = 2 * f + j - 2;
            if (fi >= 0 && fi < p.Fin) acc = fmaf(p.dww[(3 * a + j) * p.K + ci], x[((size_t)ti * p.Fin + fi) * p.K + ci], acc);
        }
    }
    return acc;
}
// SiLU(LayerNorm(x)): stats [rows][2] = mean, rstd (k_nm_glu_dwconv_ln's)
template <>
__device__ __forceinline__ float sf_load<NM_LOAD_LN_SILU>(const SfGemm& p, int b, size_t row, int r, int ci) {
    const float v = fmaf((p.X[row * p.ldx + ci] - p.stats[2 * row]) * p.stats[2 * row + 1], p.lnw[ci], p.lnb[ci]);
    return v / (1.0f + expf(-v));
}
// [x, onehot(language of the row)]: Tin = the width of x, cnt_in [B] = the language index
template <>
__device__ __forceinline__ float sf_load<NM_LOAD_PROMPT>(const SfGemm& p, int b, size_t row, int r, int ci) {
    return ci < p.Tin ? p.X[row * p.ldx + ci] : (ci - p.Tin == p.cnt_in[b] ? 1.0f : 0.0f);
}
}  // namespace

template <class Ctx>
static void nm_gemm(Ctx* c, SfGemm p, int B) {
    const dim3 grid(cdiv((int64_t)p.Tp * p.rowmul, 64), cdiv(p.N, 64), B);
    switch (p.load) {
        case NM_LOAD_DWC: MIS_LAUNCH(c, k_sf_gemm<NM_LOAD_DWC>, grid, dim3(256), p); break;
        case NM_LOAD_LN_SILU: MIS_LAUNCH(c, k_sf_gemm<NM_LOAD_LN_SILU>, grid, dim3(256), p); break;
        case NM_LOAD_PROMPT: MIS_LAUNCH(c, k_sf_gemm<NM_LOAD_PROMPT>, grid, dim3(256), p); break;
        default: sf_gemm(c, p, B); break;
    }
}

namespace {
// ============================================================================ kernel A: the causal stem's first conv
// out[b][t][f][c] = ReLU(bias[c] + sum_ij w[3 i + j][c] feats[b][2 t + i - 2][2 f + j - 2]) for t < T1[b]; the features are zero outside
// the row's own F[b] frames and the mel range (pad (2, 1): the frame behind the last one is the right pad)
__global__ void __launch_bounds__(256) k_nm_conv0(const float* __restrict__ feats, const int* __restrict__ F, const int* __restrict__ T1,
                                                  const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out, int Fp,
                                                  int mels, int T1p, int F1, int C, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    size_t r = i / C;
    const int f = (int)(r % F1);
    r /= F1;
    const int t = (int)(r % T1p), b = (int)(r / T1p);
    float v = 0.0f;
    if (t < T1[b]) {
        const int n = min(F[b], Fp);
        const float* x = feats + (size_t)b * Fp * mels;
        float acc = bias[c];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int ti = 2 * t + a - 2;
            if (ti < 0 || ti >= n) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int fi = 2 * f + j - 2;
                if (fi >= 0 && fi < mels) acc = fmaf(w[(3 * a + j) * C + c], x[(size_t)ti * mels + fi], acc);
            }
        }
        v = fmaxf(acc, 0.0f);
    }
    out[i] = v;
}
}  // namespace

// ============================================================================ chunked-limited attention: parameters and the context
struct NmAttn {
    const float* qkv; int ld, koff, voff;                    // q at column h hd, k at koff + h hd, v at voff + h hd
    float* out; int ldo;
    const int* cnt; int Tp, hd;
    float qscale, sdk;                                       // q x qscale at staging; score / sdk
    const float *u, *v;                                      // [H][hd]
    const float* P; int ldp, poff;                           // projected table by distance, rows dlo .. dhi: row = distance + poff
    int C, L, dlo, dhi;                                      // chunk size, left chunks; the distances the rule lets occur
};

// the call's context as the kernel takes it (createChunkedLimitedMask: C = max(right + 1, 1), L = left / C, left < 0: unlimited); C is
// cut to Tcap (one chunk holds the row: `regular` attention is right >= Tcap - 1, left 0)
struct NmCtx { int C, L, dlo, dhi; };
static NmCtx nm_context(int left, int right, int Tcap) {
    NmCtx x;
    x.C = (int)std::min<int64_t>(std::max<int64_t>((int64_t)right + 1, 1), Tcap);
    x.L = left >= 0 ? std::min(left / x.C, NM_UNLIMITED) : NM_UNLIMITED;
    x.dlo = -(x.C - 1);
    x.dhi = (int)std::min<int64_t>((int64_t)x.L * x.C + x.C - 1, Tcap - 1);
    return x;
}

#define NM_LDP 129                   // an odd row stride: the 32 rows a half-wave reads fall into 32 banks

// ============================================================================ greedy RNN-T decode: parameters and the LSTM step
struct NmRnnt {
    const float* encp; const int* cnt; int Tp, J, P, V, layers;     // joint.enc of every frame [B][Tp][J]; V = vocab + 1 logits, blank = V - 1
    const float *embed, *wxT[2], *whT[2], *bih[2], *bhh[2], *wpT, *bp, *woT, *bo;
    int max_symbols, cap;                                           // max_symbols 0: none
    int *tokens, *frames, *count, *flag, *steps;                    // [B][cap] x 2, [B] x 3
};

__device__ __forceinline__ float nm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// one LSTM layer, torch.nn.LSTM's: gates i, f, g, o = (b_ih + b_hh) + W_ih x + W_hh h, k ascending; c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c')
__device__ __forceinline__ void nm_lstm_layer(const float* __restrict__ wxT, const float* __restrict__ whT, const float* __restrict__ bih,
                                              const float* __restrict__ bhh, const float* x, const float* h, const float* c, float* hn, float* cn,
                                              int P) {
    for (int u = threadIdx.x; u < P; u += NM_NT) {
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
        const float cc = nm_sigmoid(g[1]) * c[u] + nm_sigmoid(g[0]) * tanhf(g[2]);
        cn[u] = cc;
        hn[u] = nm_sigmoid(g[3]) * tanhf(cc);
    }
    __syncthreads();
}

__device__ __forceinline__ bool nm_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// the decoder's tensors as a checkpoint holds them (host), and their device form
struct NmDecHost { const float *embed, *wih[2], *whh[2], *bih[2], *bhh[2], *wp, *bp, *wo, *bo; };

// transposed copies: Wx / Wh [4 P][P] -> [k][gate][unit], joint.pred [J][P] -> [k][j], joint_net [V][J] -> [j][logit]; plain index arithmetic
static void nm_pack_decoder(const NmDecHost& s, int layers, int P, int J, int V, DevBuf<float>& arena, NmRnnt& p) {
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
    size_t off[13] = {};
    off[0] = push(s.embed, (size_t)V * P);
    for (int l = 0; l < layers; ++l) { off[1 + 4 * l] = gatesT(s.wih[l]); off[2 + 4 * l] = gatesT(s.whh[l]); off[3 + 4 * l] = push(s.bih[l], 4 * P); off[4 + 4 * l] = push(s.bhh[l], 4 * P); }
    off[9] = linT(s.wp, J, P); off[10] = push(s.bp, J); off[11] = linT(s.wo, V, J); off[12] = push(s.bo, V);
    arena.alloc(blob.size());
    HIP_CHECK(hipMemcpy(arena.p, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
    const float* a = arena.p;
    p.embed = a + off[0];
    for (int l = 0; l < 2; ++l) {                                   // one layer: the second set is never read
        const int m = l < layers ? l : 0;
        p.wxT[l] = a + off[1 + 4 * m]; p.whT[l] = a + off[2 + 4 * m]; p.bih[l] = a + off[3 + 4 * m]; p.bhh[l] = a + off[4 + 4 * m];
    }
    p.wpT = a + off[9]; p.bp = a + off[10]; p.woT = a + off[11]; p.bo = a + off[12];
    p.layers = layers; p.P = P; p.J = J; p.V = V;
}

static void nm_check_decoder_dims(int layers, int P, int J, int vocab, int max_symbols) {
    MIS_REQUIRE(layers == 1 || layers == 2, MIS_ERR_INVALID_INPUT, "pred_rnn_layers %d: 1 or 2", layers);
    MIS_REQUIRE(P >= 1 && P <= NM_MAXW, MIS_ERR_INVALID_INPUT, "pred_hidden %d outside 1..%d", P, NM_MAXW);
    MIS_REQUIRE(J >= 1 && J <= NM_MAXW, MIS_ERR_INVALID_INPUT, "joint_hidden %d outside 1..%d", J, NM_MAXW);
    MIS_REQUIRE(vocab >= 1 && vocab <= 65535, MIS_ERR_INVALID_INPUT, "vocab_size %d outside 1..65535", vocab);
    MIS_REQUIRE(max_symbols >= 0 && max_symbols <= 64, MIS_ERR_INVALID_INPUT, "max_symbols %d outside 0..64 (0: none)", max_symbols);
}

// ============================================================================ the model handle
struct mis_nemotron {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_nemotron_config cfg{};
    int mels = 0, C = 0, d = 0, H = 0, hd = 0, f = 0, L = 0, ck = 0, padl = 0, F1 = 0, F2 = 0, F3 = 0, P = 0, J = 0, V = 0, cap = 0, NP = 0, PH = 0;
    HostWeights raw{"Nemotron", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, ptab, dec;
    DevBuf<int> fbr;
    const float *window = nullptr, *twc = nullptr, *tws = nullptr, *fb = nullptr, *c0w = nullptr, *c0b = nullptr, *dw2w = nullptr, *dw2b = nullptr,
                *dw5w = nullptr, *dw5b = nullptr;
    SfLin pw3, pw6, lin, jenc, pr0, pr2;
    struct Layer {
        const float *ln1w, *ln1b, *lnaw, *lnab, *lncw, *lncb, *ln2w, *ln2b, *lnow, *lnob, *u, *v, *P, *dw, *dwb, *cnw, *cnb;
        SfLin ff1a, ff1b, qkv, o, pw1, pw2, ff2a, ff2b;
    };
    std::vector<Layer> fc;
    // bf16 mode (nemotron_encoder_bf16.h, offline engine only): the block matrices [N][K] and the rounded tables [tab_hi - tab_lo + 1][d];
    // the f32 matrices, ptab, qkv and att do not exist then, big only as the prompt kernel's buffer
    int enc_bf16 = 0;
    struct Layer16 { bf16_t *ff1a, *ff1b, *qkv, *o, *pw1, *pw2, *ff2a, *ff2b, *P; };
    std::vector<Layer16> fc16;
    DevBuf<bf16_t> warena, ptab16, big16, qkv16, att16;
    NmRnnt rnnt{};
    int tab_lo = 0, tab_hi = 0;                                      // the distances the projected tables hold
    // workspace (sized at finalize)
    int64_t maxN = 0;
    int Fcap = 0, T1cap = 0, T2cap = 0, Tcap = 0;
    DevBuf<float> pcm, melraw, feats, s0, s1, s2, emb, h, stats, big, qkv, att, prm, encp;
    DevBuf<int> cntN, cntF, cnt1, cnt2, cnt3, lang, outs;            // outs: tokens, frames [B][cap] each, then count, flag, steps [B] each
    // state of the last call
    int batch = 0, Fp = 0, T1p = 0, T2p = 0, Tp = 0, launches = 0;
    NmCtx ctx{};
    std::vector<int> hN, hF, hT1, hT2, hT3, hlang;
    HipEvents<4> ev;
    bool timed = false, timed_done = false, has_emb = false;
};

static inline int nm_half(int t) { return t / 2 + 1; }              // floor((t + 2 + 1 - 3) / 2) + 1
static inline int nm_frames(int64_t n) { return (int)(1 + n / NEMO_HOP); }
