// parakeet.hip - Parakeet TDT speech-to-text: 16 kHz samples -> NeMo log-mel (per-feature normalisation) -> depthwise-striding Conv2d stem
// (factor 8) -> FastConformer blocks with relative-position attention -> joint.enc over every frame -> greedy TDT decode (embedding, two
// LSTM layers, joint, token and duration arg-max) in ONE launch.  Exact f32 throughout, unless mis_parakeet_set_encoder_dtype(MIS_BF16)
// selects the bf16 form of the Conformer blocks (parakeet_encoder_bf16.h holds its kernels and its precision contract).
//
// Reference being replaced: ParakeetModel (Sources/MLXAudioSTT/Models/Parakeet/ParakeetModel.swift decodeTDTSerial :389-479,
// makeCompiledTDTStep :894-931, ParakeetConformer.swift), NemoDecodingLogic.tdtStep (Nemo/NemoDecodingLogic.swift:41-67), NemoPredictNetwork /
// NemoJointNetwork (Nemo/NemoRNNTLayers.swift), NemoRelPositionMultiHeadAttention (Nemo/NemoAttention.swift).
//
// The front end is audio_front.h's, the stem and the Conformer block are sortformer_kernels.h's (the kernels Sortformer runs, unchanged), with
// the ragged-batch rule of sortformer.hip: every kernel takes the row's own counts, so a row's bits do not depend on its batch.  The encoder
// (k_pk_attn, its members, pk_front_stem, pk_encoder) lives in parakeet_encoder.h, which canary.hip shares.  Two kernels are Parakeet's:
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
#include "parakeet_encoder.h"
#include "parakeet_encoder_bf16.h"

#include <math.h>
#include <string.h>
#include <memory>

#define PK_MAX_DUR 8
#define PK_NT 1024                   // threads of the decode block
#define PK_MAXW 1024                 // pred_hidden, joint_hidden

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
struct mis_parakeet : PkEncoder {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_parakeet_config cfg{};
    int P = 0, J = 0, V = 0, D = 0, cap = 0;
    HostWeights raw{"Parakeet", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    SfLin jenc;
    PkDecDev dec;
    PkTdt tdt{};
    DevBuf<float> encp;
    DevBuf<int> outs;                                                // tokens, frames, durations [B][cap] each, then count, flag, steps [B] each
    HipEvents<4> ev;
    bool timed = false, timed_done = false;
};


extern "C" mis_status mis_parakeet_create(const mis_parakeet_config* cfg, int device, mis_parakeet** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    pk_encoder_check(cfg);
    MIS_REQUIRE(cfg->pred_rnn_layers == 2, MIS_ERR_INVALID_INPUT, "pred_rnn_layers %d: only 2 is implemented", cfg->pred_rnn_layers);
    pk_check_decoder_dims(cfg->pred_hidden, cfg->joint_hidden, cfg->vocab_size, cfg->num_durations, cfg->max_symbols, cfg->durations);
    MIS_REQUIRE(cfg->max_tokens >= 1 && cfg->max_tokens <= 65536, MIS_ERR_INVALID_INPUT, "max_tokens %d outside 1..65536", cfg->max_tokens);
    hipStream_t stream = mis_open_stream(device);      // first: the handle's events belong to this device
    auto c = std::make_unique<mis_parakeet>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    pk_encoder_dims(c.get());
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

extern "C" mis_status mis_parakeet_set_encoder_dtype(mis_parakeet* c, mis_dtype dtype) {
    MIS_API_BEGIN
    pk_set_encoder_dtype(c, dtype);
    MIS_API_END
}

static const char* const PK_LSTM = "decoder.prediction.dec_rnn.lstm.";

extern "C" mis_status mis_parakeet_finalize(mis_parakeet* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t d = c->d, P = c->P, J = c->J, V = c->V, NL = c->V + c->D;
    HostArena a(c->raw);
    pk_encoder_weights(c, a);
    a.fvec("joint.enc.weight", {J, d}, J * d, c->jenc.w); a.fvec("joint.enc.bias", {J}, J, c->jenc.b);
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
    a.upload(c->warena, c->farena);
    pk_pack_decoder(s, (int)P, (int)J, (int)V, (int)NL, c->dec, c->tdt);
    pk_encoder_workspace(c);
    const size_t B = c->cfg.max_batch, M = B * c->Tcap;
    c->encp.alloc(M * J);
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
    const int64_t d = c->d, P = c->P, J = c->J, V = c->V, NL = c->V + c->D;
    pk_encoder_synthetic(c, sw);
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

// ---------------------------------------------------------------------------- the bf16 encoder's kernels (parakeet_encoder_bf16.h)
namespace {
// the ONE checked launch; then, with ms, `repeat` more of the same launch between two events: *ms = milliseconds a launch
template <class F>
void pkd_run(PkdCtx& c, F launch, int repeat, float* ms) {
    launch();
    pkd_sync(c);
    if (!ms) return;
    MIS_REQUIRE(repeat >= 1 && repeat <= 10000, MIS_ERR_INVALID_INPUT, "repeat %d outside 1..10000", repeat);
    HipEvents<2> ev;
    HIP_CHECK(hipEventRecord(ev[0], c.stream));
    for (int r = 0; r < repeat; ++r) launch();
    HIP_CHECK(hipEventRecord(ev[1], c.stream));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipEventElapsedTime(ms, ev[0], ev[1]));
    *ms /= (float)repeat;
}
// rows x width elements of `es` bytes out of a guarded [rows][ld] body; the columns behind width must be untouched
void pkd_rows_out(GuardedOut& o, void* out, size_t rows, size_t width, size_t ld, size_t es) {
    o.check_guards();
    std::vector<uint8_t> hbuf(o.body);
    HIP_CHECK(hipMemcpy(hbuf.data(), o.p(), o.body, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        memcpy(static_cast<uint8_t*>(out) + r * width * es, hbuf.data() + r * ld * es, width * es);
        for (size_t i = width * es; i < ld * es; ++i)
            MIS_REQUIRE(hbuf[r * ld * es + i] == 0xFF, MIS_ERR_GENERATION_FAILED, "the kernel wrote behind the %zu columns of row %zu", width, r);
    }
}
}  // namespace

// ONE launch of k_pk_gemm_bf16.  load PKB_LOAD_BF16 (0): x bf16 [batch Tp][K]; PKB_LOAD_LN (1): x f32 with stats [batch Tp][2], lnw, lnb [K].
// epi 0 none / 1 SiLU: out bf16 [batch Tp][N]; 2: out f32 = R + ra v, R f32 [batch Tp][N].  rule 0: 64 x 64 tile, 1: 32 x 32.
extern "C" mis_status mis_debug_parakeet_gemm_bf16(int device, int load, int epi, int rule, const void* x, const float* stats, const float* lnw, const float* lnb,
                                                   const uint16_t* w, const float* bias, const float* R, float ra, const int32_t* cnt, int batch, int Tp, int K,
                                                   int N, void* out, int repeat, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && w && cnt && out && batch >= 1 && batch <= 65535 && Tp >= 1 && K >= 32 && K % 32 == 0 && N >= 8 && N % 8 == 0, MIS_ERR_INVALID_INPUT,
                "Parakeet bf16 GEMM: pointers, positive batch and Tp, K a multiple of 32 and N a multiple of 8 are required");
    MIS_REQUIRE((load == PKB_LOAD_BF16 || (load == PKB_LOAD_LN && stats && lnw && lnb)) && epi >= PKB_EPI_NONE && epi <= PKB_EPI_RES && (epi != PKB_EPI_RES || R) &&
                    (rule == PKB_TILE64 || rule == PKB_TILE32), MIS_ERR_INVALID_INPUT, "Parakeet bf16 GEMM: unknown load / epilogue / rule, or a missing operand");
    const size_t rows = (size_t)batch * Tp;
    MIS_REQUIRE((int64_t)rows * K <= PKD_MAX_ELEMS && (int64_t)rows * N <= PKD_MAX_ELEMS && (int64_t)N * K <= PKD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Parakeet bf16 GEMM: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    PkdCtx c;
    DevBuf<uint16_t> dxb, dw;
    DevBuf<uint32_t> dxf, dst, dlw, dlb, dbias, dR, dcnt;
    PkbGemm p{};
    if (load == PKB_LOAD_LN) {
        alloc32(dxf, x, rows * K, F32_NAN); alloc32(dst, stats, rows * 2, F32_NAN); alloc32(dlw, lnw, K, F32_NAN); alloc32(dlb, lnb, K, F32_NAN);
        p.Xf = pkd_fp(dxf); p.stats = pkd_fp(dst); p.lnw = pkd_fp(dlw); p.lnb = pkd_fp(dlb);
    } else {
        alloc16(dxb, static_cast<const uint16_t*>(x), rows * K, BF16_NAN);
        p.Xb = dxb.p;
    }
    alloc16(dw, w, (size_t)N * K, BF16_NAN);
    alloc32(dcnt, cnt, batch, 0x7FFFFFFFu);
    if (bias) { alloc32(dbias, bias, N, F32_NAN); p.bias = pkd_fp(dbias); }
    if (epi == PKB_EPI_RES) { alloc32(dR, R, rows * N, F32_NAN); p.R = pkd_fp(dR); p.ldr = N; p.ra = ra; }
    const size_t es = epi == PKB_EPI_RES ? 4 : 2;
    GuardedOut o;
    o.alloc(rows * N * es, (size_t)64 * N * es);
    p.Yf = reinterpret_cast<float*>(o.p()); p.Yb = reinterpret_cast<bf16_t*>(o.p());
    p.ldx = K; p.W = dw.p; p.ldy = N; p.cnt = reinterpret_cast<const int*>(dcnt.p); p.Tp = Tp; p.K = K; p.N = N; p.epi = epi;
    pkd_run(c, [&] { pkb_gemm_launch(&c, p, load, rule, batch); c.launches = 1; }, repeat, ms);
    pkd_rows_out(o, out, rows, N, N, es);
    MIS_API_END
}

// ONE launch of k_pk_attn_bf16: the arguments of mis_debug_parakeet_attn with bf16 qkv and table, head sizes 1..128; out bf16 [batch Tp][heads hd]
extern "C" mis_status mis_debug_parakeet_attn_bf16(int device, const uint16_t* qkv, int ld, int koff, int voff, const int32_t* cnt, int batch, int Tp, int heads,
                                                   int hd, float qscale, float sdk, const float* u, const float* v, const uint16_t* P, int ldp, int Tcap, int ldo,
                                                   uint16_t* out, int repeat, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(qkv && cnt && out && u && v && P && batch >= 1 && Tp >= 1 && heads >= 1 && hd >= 1 && hd <= 128 && Tcap >= 1, MIS_ERR_INVALID_INPUT,
                "Parakeet bf16 attention: every pointer, positive batch, Tp, heads, Tcap and a head size of 1..128 are required");
    const int64_t width = (int64_t)heads * hd;
    MIS_REQUIRE(koff >= 0 && voff >= 0 && width <= ld && koff + width <= ld && voff + width <= ld && width <= ldo && ldp >= width, MIS_ERR_INVALID_INPUT,
                "Parakeet bf16 attention: q, k and v must lie inside a row of ld columns, the output inside ldo, the table inside ldp");
    MIS_REQUIRE((int64_t)batch * Tp * ld <= PKD_MAX_ELEMS && (int64_t)batch * Tp * ldo <= PKD_MAX_ELEMS && (2 * (int64_t)Tcap - 1) * ldp <= PKD_MAX_ELEMS &&
                    batch <= 65535 && heads <= 65535, MIS_ERR_INVALID_INPUT, "Parakeet bf16 attention: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    PkdCtx c;
    const size_t rows = (size_t)batch * Tp;
    DevBuf<uint16_t> dq, dP;
    DevBuf<uint32_t> dcnt, du, dv;
    alloc16(dq, qkv, rows * ld, BF16_NAN); alloc16(dP, P, (size_t)(2 * Tcap - 1) * ldp, BF16_NAN);
    alloc32(dcnt, cnt, batch, 0x7FFFFFFFu);
    alloc32(du, u, width, F32_NAN); alloc32(dv, v, width, F32_NAN);
    GuardedOut o;
    o.alloc(rows * ldo * 2, (size_t)64 * ldo * 2);
    PkbAttn p{dq.p, ld, koff, voff, reinterpret_cast<bf16_t*>(o.p()), ldo, reinterpret_cast<const int*>(dcnt.p), Tp, hd, qscale, sdk, pkd_fp(du), pkd_fp(dv),
              dP.p, ldp, Tcap};
    pkd_run(c, [&] { pkb_attn(&c, p, heads, hd, batch); c.launches = 1; }, repeat, ms);
    pkd_rows_out(o, out, rows, width, ldo, 2);
    MIS_API_END
}

// ONE launch of k_pk_glu_dwconv_bf16: pw bf16 [batch Tp][2 C], taps f32 [k][C], shift f32 [C] -> out bf16 [batch Tp][C]
extern "C" mis_status mis_debug_parakeet_glu_dwconv_bf16(int device, const uint16_t* pw, const float* taps, const float* shift, const int32_t* cnt, int batch, int Tp,
                                                         int C, int k, uint16_t* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(pw && taps && shift && cnt && out && batch >= 1 && batch <= 65535 && Tp >= 1 && C >= 1 && k >= 3 && k <= SF_DW_MAXK && k % 2 == 1,
                MIS_ERR_INVALID_INPUT, "Parakeet bf16 GLU / depthwise: pointers, positive batch, Tp, C and an odd k of 3..%d are required", SF_DW_MAXK);
    const size_t rows = (size_t)batch * Tp;
    MIS_REQUIRE((int64_t)rows * 2 * C <= PKD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Parakeet bf16 GLU / depthwise: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    PkdCtx c;
    DevBuf<uint16_t> dpw;
    DevBuf<uint32_t> dt, dsh, dcnt;
    alloc16(dpw, pw, rows * 2 * C, BF16_NAN);
    alloc32(dt, taps, (size_t)k * C, F32_NAN); alloc32(dsh, shift, C, F32_NAN); alloc32(dcnt, cnt, batch, 0x7FFFFFFFu);
    GuardedOut o;
    o.alloc(rows * C * 2, (size_t)64 * C * 2);
    MIS_LAUNCH(&c, k_pk_glu_dwconv_bf16, dim3(cdiv(Tp, SF_DW_TT), cdiv(C, 64), batch), dim3(256), dpw.p, pkd_fp(dt), pkd_fp(dsh),
               reinterpret_cast<const int*>(dcnt.p), reinterpret_cast<bf16_t*>(o.p()), Tp, C, k);
    pkd_sync(c);
    pkd_rows_out(o, out, rows, C, C, 2);
    MIS_API_END
}
