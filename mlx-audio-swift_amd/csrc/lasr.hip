// lasr.hip - the LASR CTC engine: raw 16 kHz samples -> NeMo-style log-mel -> strided conv stem -> RoPE Conformer -> CTC head -> greedy ids.
//
// Reference being replaced: LasrCTCModel / LasrEncoder / LasrEncoderBlock / LasrEncoderAttention / LasrEncoderConvolutionModule
// (Sources/MLXAudioSTT/Models/LasrCTC/LasrCTCModel.swift:7-406), ParakeetAudio.logMelSpectrogram (ParakeetAudio.swift:6-62) with DSP.swift's
// hanningWindow / stft(.constant) / melFilters(slaney, slaney), Wav2Vec2CTCModel.greedyCTCTokens (Wav2Vec2CTC.swift:520-542).
// Tokenizer and text stay on the host.
//
// Ragged batch.  A row of n samples has F = 1 + n / 160 feature frames, T1 = (F - k_s) / s + 1 and T2 = (T1 - k_s) / s + 1 stem frames.
// The batch is laid out with the longest row's Fp / T1p / T2p frames per row; every kernel takes the row's own count: the normalisation
// statistics run over the row's F frames, the im2col writes zero patches behind T1[b] / T2[b], the depthwise conv reads zeros outside
// 0 .. T2[b], attention masks keys >= T2[b], the LayerNorms that close a block write zero rows behind T2[b], the CTC scan stops there.
// Samples behind lens[b] are never read.
//
// Precision: f32 from the waveform through the normalised features, one rounding to bf16 there; bf16 storage with f32 accumulation
// behind it, one rounding per kernel output; f32 logits; f32 statistics in every LayerNorm; f32 RoPE tables (the reference casts them to
// the activations' dtype); the depthwise conv with the BatchNorm folded into its taps accumulates in f32.
//
//   k_nemo_log_mel     pre-emphasis, 512-point FFT of one frame in LDS, power, slaney mel, log      (audio_front.h: the front end
//   k_nemo_norm        per-row per-bin mean / unbiased variance in two passes over the row's own frames   shared with sortformer.hip)
//   k_lasr_pack        f32 features -> the bf16 rows dense_0 multiplies (K padded to 32, zero rows behind F[b])
//   k_lasr_im2col      k_s-tap strided patches with per-row valid counts
//   k_lasr_gemm        C = X W^T on v_mfma_f32_16x16x32_bf16, 128 x 128 or 64 x 64 tiles; epilogues bias / ReLU / SiLU / a R + b acc / f32
//   k_lasr_ln          LayerNorm with weight and bias, one wave per row, optional zero rows behind the row count
//   k_lasr_rope        rotate-half RoPE over the whole 64-wide head on the q and k columns, in place, before attention
//   k_lasr_attn        non-causal flash attention, 64 queries x head x row per block, K / V tiles staged through LDS, per-row key count
//   k_lasr_glu_dwconv  GLU -> zero-padded depthwise conv (<= 64 taps) -> folded BatchNorm -> activation, a time tile + halo in LDS
//   k_lasr_argmax      per-frame arg-max (lowest index on ties);  k_lasr_collapse  CTC collapse + compaction per row
#include "common.h"
#include "bf16_tile.h"
#define AUDIO_FRONT_NEMO_KERNELS
#include "audio_front.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define LS_HD 64                 // head size
#define LS_MAX_BATCH 64
#define LS_MAX_SECONDS 120
#define LS_DW_TT 64              // depthwise conv: output frames per block
#define LS_DW_MAXK 64

struct LsLayer {
    bf16_t *ln_ff1w, *ln_ff1b, *ff1_w1, *ff1_b1, *ff1_w2, *ff1_b2;
    bf16_t *ln_attw, *ln_attb, *wqkv, *bqkv, *wo, *bo;
    bf16_t *ln_cvw, *ln_cvb, *pw1, *pw1b, *pw2, *pw2b;
    float *dw, *dwshift;         // [k][C] taps with the BatchNorm scale folded in; [C] shift
    bf16_t *ln_ff2w, *ln_ff2b, *ff2_w1, *ff2_b1, *ff2_w2, *ff2_b2;
    bf16_t *ln_outw, *ln_outb;
};

struct mis_lasr {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_lasr_config cfg{};
    int d = 0, f = 0, V = 0, H = 0, Hk = 0, L = 0, mels = 0, Kp = 0, cc = 0, ks = 0, st = 0, ck = 0;
    HostWeights raw{"LASR", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<bf16_t> arena;
    DevBuf<float> farena;
    float *window = nullptr, *tw_cos = nullptr, *tw_sin = nullptr, *fb = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
    int* fb_range = nullptr;
    bf16_t *d0w = nullptr, *d0b = nullptr, *c0w = nullptr, *c0b = nullptr, *c1w = nullptr, *c1b = nullptr, *d1w = nullptr, *d1b = nullptr,
           *onw = nullptr, *onb = nullptr, *headw = nullptr, *headb = nullptr;
    std::vector<LsLayer> layers;
    // workspace (sized at finalize)
    int64_t maxN = 0;
    int Fcap = 0, T1cap = 0, T2cap = 0;
    DevBuf<float> pcm, melraw, feats, logits;
    DevBuf<int> fbr, cntN, cntF, cnt1, cnt2, pred, tokens, ntok;
    DevBuf<bf16_t> x0, h0, col, c0, c1, h, x, qkv, att, ff, enc_out;
    PinnedBuf<int32_t> host_tokens;
    // state of the last call
    int batch = 0, Fp = 0, T1p = 0, T2p = 0, launches = 0;
    std::vector<int> hN, hF, hT1, hT2;
    HipEvents<4> ev;
    bool timed = false;
};

// ---------------------------------------------------------------------------- frame counts
static inline int ls_frames(int64_t n) { return (int)(1 + n / NEMO_HOP); }
static inline int ls_conv_out(int t, int k, int s) { return t >= k ? (t - k) / s + 1 : 0; }

extern "C" mis_status mis_lasr_frames(const mis_lasr* c, const int64_t* lens, int batch, int32_t* F_out, int32_t* T2_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0, MIS_ERR_INVALID_INPUT, "row %d: negative sample count", b);
        const int F = ls_frames(lens[b]);
        if (F_out) F_out[b] = F;
        if (T2_out) T2_out[b] = ls_conv_out(ls_conv_out(F, c->ks, c->st), c->ks, c->st);
    }
    MIS_API_END
}

extern "C" mis_status mis_lasr_create(const mis_lasr_config* cfg, int device, mis_lasr** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    const int d = cfg->hidden_size, H = cfg->num_attention_heads, Hk = cfg->num_key_value_heads;
    MIS_REQUIRE(d > 0 && d % 32 == 0, MIS_ERR_INVALID_INPUT, "hidden_size %d unsupported (a positive multiple of 32)", d);
    MIS_REQUIRE(H > 0 && d % H == 0 && d / H == LS_HD, MIS_ERR_INVALID_INPUT,
                "num_attention_heads %d: head size hidden_size / num_attention_heads must be %d", H, LS_HD);
    MIS_REQUIRE(Hk > 0 && H % Hk == 0, MIS_ERR_INVALID_INPUT, "num_key_value_heads %d must divide num_attention_heads %d", Hk, H);
    MIS_REQUIRE(cfg->intermediate_size > 0 && cfg->intermediate_size % 32 == 0, MIS_ERR_INVALID_INPUT,
                "intermediate_size %d unsupported (a positive multiple of 32)", cfg->intermediate_size);
    MIS_REQUIRE(cfg->subsampling_conv_channels > 0 && cfg->subsampling_conv_channels % 32 == 0, MIS_ERR_INVALID_INPUT,
                "subsampling_conv_channels %d unsupported (a positive multiple of 32)", cfg->subsampling_conv_channels);
    MIS_REQUIRE(cfg->conv_kernel_size >= 2 && cfg->conv_kernel_size <= LS_DW_MAXK, MIS_ERR_INVALID_INPUT,
                "conv_kernel_size %d outside 2..%d", cfg->conv_kernel_size, LS_DW_MAXK);
    MIS_REQUIRE(cfg->subsampling_conv_kernel_size >= 2 && cfg->subsampling_conv_kernel_size <= 8, MIS_ERR_INVALID_INPUT,
                "subsampling_conv_kernel_size %d outside 2..8", cfg->subsampling_conv_kernel_size);
    MIS_REQUIRE(cfg->subsampling_conv_stride >= 1 && cfg->subsampling_conv_stride <= 4, MIS_ERR_INVALID_INPUT,
                "subsampling_conv_stride %d outside 1..4", cfg->subsampling_conv_stride);
    MIS_REQUIRE(cfg->vocab_size >= 1 && cfg->vocab_size <= 65536, MIS_ERR_INVALID_INPUT, "vocab_size %d outside 1..65536", cfg->vocab_size);
    MIS_REQUIRE(cfg->num_mel_bins >= 8 && cfg->num_mel_bins <= 256, MIS_ERR_INVALID_INPUT, "num_mel_bins %d outside 8..256", cfg->num_mel_bins);
    MIS_REQUIRE(cfg->num_hidden_layers >= 1, MIS_ERR_INVALID_INPUT, "num_hidden_layers %d must be positive", cfg->num_hidden_layers);
    MIS_REQUIRE(cfg->rope_type == 0, MIS_ERR_INVALID_INPUT, "rope_type: only \"default\" is implemented");
    MIS_REQUIRE(cfg->rope_theta > 0.0f, MIS_ERR_INVALID_INPUT, "rope_theta must be positive");
    MIS_REQUIRE(cfg->hidden_act == 0 || cfg->hidden_act == 1, MIS_ERR_INVALID_INPUT, "hidden_act must be 0 (silu) or 1 (relu)");
    MIS_REQUIRE(cfg->pad_token_id >= 0, MIS_ERR_INVALID_INPUT, "pad_token_id must not be negative");
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= LS_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch %d outside 1..%d", cfg->max_batch, LS_MAX_BATCH);
    MIS_REQUIRE(cfg->max_seconds >= 1 && cfg->max_seconds <= LS_MAX_SECONDS, MIS_ERR_INVALID_INPUT, "max_seconds %d outside 1..%d", cfg->max_seconds,
                LS_MAX_SECONDS);
    hipStream_t stream = mis_open_stream(device);      // first: the handle's events belong to this device
    auto c = std::make_unique<mis_lasr>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->d = d; c->f = cfg->intermediate_size; c->V = cfg->vocab_size; c->H = H; c->Hk = Hk; c->L = cfg->num_hidden_layers;
    c->mels = cfg->num_mel_bins; c->Kp = (int)round_up(c->mels, 32); c->cc = cfg->subsampling_conv_channels;
    c->ks = cfg->subsampling_conv_kernel_size; c->st = cfg->subsampling_conv_stride; c->ck = cfg->conv_kernel_size;
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_lasr_destroy(mis_lasr* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}

extern "C" mis_status mis_lasr_set_tensor(mis_lasr* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 3, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

extern "C" mis_status mis_lasr_finalize(mis_lasr* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t d = c->d, f = c->f, V = c->V, cc = c->cc, ks = c->ks, ck = c->ck, mels = c->mels, Kp = c->Kp;
    const bool ab = c->cfg.attention_bias != 0, cb = c->cfg.convolution_bias != 0;
    HostArena a(c->raw);
    std::vector<bf16_t>& host = a.host;
    std::vector<float>& fhost = a.fhost;
    const std::string E = "encoder.", S = "encoder.subsampler.";
    // ---- front end tables (f32): window 400 -> 512, FFT twiddles, slaney filters [257][mels] and each filter's bin range
    const size_t o_win = a.ftake(NEMO_NFFT, c->window), o_twc = a.ftake(NEMO_NFFT / 2, c->tw_cos), o_tws = a.ftake(NEMO_NFFT / 2, c->tw_sin);
    hann_padded(&fhost[o_win], NEMO_WIN, NEMO_NFFT);
    fft512_twiddles(&fhost[o_twc], &fhost[o_tws]);
    const size_t o_fb = a.ftake((size_t)NEMO_BINS * mels, c->fb);
    std::vector<int> ranges(2 * mels, 0);
    slaney_filterbank(&fhost[o_fb], ranges.data(), NEMO_BINS, (int)mels, 16000.0, NEMO_NFFT);
    // ---- workspace extents and the rotary tables [T2cap][32] (LasrRotaryEmbedding, :23-42): f32, angle = pos * theta^(-2i/64)
    c->maxN = (int64_t)c->cfg.max_seconds * 16000;
    c->Fcap = ls_frames(c->maxN); c->T1cap = ls_conv_out(c->Fcap, c->ks, c->st); c->T2cap = ls_conv_out(c->T1cap, c->ks, c->st);
    MIS_REQUIRE(c->T2cap >= 1, MIS_ERR_INVALID_INPUT, "max_seconds %d gives no encoder frame", c->cfg.max_seconds);
    const size_t o_rc = a.ftake((size_t)c->T2cap * 32, c->rope_cos), o_rs = a.ftake((size_t)c->T2cap * 32, c->rope_sin);
    for (int i = 0; i < 32; ++i) {
        const float inv = 1.0f / powf(c->cfg.rope_theta, (float)(2 * i) / (float)LS_HD);
        for (int p = 0; p < c->T2cap; ++p) {
            const float ang = (float)p * inv;
            fhost[o_rc + (size_t)p * 32 + i] = (float)cos((double)ang);
            fhost[o_rs + (size_t)p * 32 + i] = (float)sin((double)ang);
        }
    }
    // ---- stem.  dense_0 [d][mels] -> [d][Kp] (zero columns); conv weights [O][k][I] are already the patch order k * I + i
    const HostTensor& w0 = c->raw.need(S + "dense_0.weight", {d, mels});
    const size_t o_d0w = a.btake((size_t)d * Kp, c->d0w);
    for (int64_t n = 0; n < d; ++n) for (int64_t k = 0; k < mels; ++k) host[o_d0w + n * Kp + k] = f32_to_bf16(w0.v[n * mels + k]);
    a.bvec(S + "dense_0.bias", d, c->d0b);
    auto conv3 = [&](const std::string& name, int64_t O, int64_t K, int64_t I, bf16_t*& dst) {
        const HostTensor& t = c->raw.need(name, {O, K, I});
        const size_t off = a.btake((size_t)O * K * I, dst);
        for (size_t i = 0; i < (size_t)O * K * I; ++i) host[off + i] = f32_to_bf16(t.v[i]);
    };
    conv3(S + "conv_0.weight", d, ks, d, c->c0w); a.bvec(S + "conv_0.bias", d, c->c0b);
    conv3(S + "conv_1.weight", cc, ks, d, c->c1w); a.bvec(S + "conv_1.bias", cc, c->c1b);
    a.bmat(S + "dense_1.weight", d, cc, c->d1w); a.bvec(S + "dense_1.bias", d, c->d1b);
    // ---- blocks.  A LayerNorm bias the checkpoint does not carry is zero, the value the reference's LayerNorm is created with (the
    // published checkpoints have weight-only LayerNorms and the reference loads them with noUnusedKeys, :401).  A linear or conv bias
    // the configuration turns off stays nullptr.
    auto ln_bias = [&](const std::string& name, bf16_t*& dst) { if (c->raw.find(name)) a.bvec(name, d, dst); else a.btake(d, dst); };
    const int64_t NQ = (int64_t)(c->H + 2 * c->Hk) * LS_HD;
    c->layers.assign(c->L, LsLayer{});
    for (int li = 0; li < c->L; ++li) {
        const std::string q = E + "layers." + std::to_string(li) + ".";
        LsLayer& l = c->layers[li];
        auto norm = [&](const std::string& n, bf16_t*& w, bf16_t*& b) { a.bvec(q + n + ".weight", d, w); ln_bias(q + n + ".bias", b); };
        auto ffn = [&](const std::string& n, bf16_t*& w1, bf16_t*& b1, bf16_t*& w2, bf16_t*& b2) {
            a.bmat(q + n + ".linear1.weight", f, d, w1); if (ab) a.bvec(q + n + ".linear1.bias", f, b1);
            a.bmat(q + n + ".linear2.weight", d, f, w2); if (ab) a.bvec(q + n + ".linear2.bias", d, b2);
        };
        norm("norm_feed_forward1", l.ln_ff1w, l.ln_ff1b); ffn("feed_forward1", l.ff1_w1, l.ff1_b1, l.ff1_w2, l.ff1_b2);
        norm("norm_self_att", l.ln_attw, l.ln_attb);
        const size_t o_qkv = a.btake((size_t)NQ * d, l.wqkv);
        a.bmat_into(q + "self_attn.q_proj.weight", d, d, o_qkv);
        a.bmat_into(q + "self_attn.k_proj.weight", (int64_t)c->Hk * LS_HD, d, o_qkv + (size_t)d * d);
        a.bmat_into(q + "self_attn.v_proj.weight", (int64_t)c->Hk * LS_HD, d, o_qkv + (size_t)(d + c->Hk * LS_HD) * d);
        if (ab) {
            const size_t o_b = a.btake(NQ, l.bqkv);
            const HostTensor& bq = c->raw.need(q + "self_attn.q_proj.bias", {d});
            const HostTensor& bk = c->raw.need(q + "self_attn.k_proj.bias", {(int64_t)c->Hk * LS_HD});
            const HostTensor& bv = c->raw.need(q + "self_attn.v_proj.bias", {(int64_t)c->Hk * LS_HD});
            for (int64_t i = 0; i < d; ++i) host[o_b + i] = f32_to_bf16(bq.v[i]);
            for (int64_t i = 0; i < c->Hk * LS_HD; ++i) {
                host[o_b + d + i] = f32_to_bf16(bk.v[i]);
                host[o_b + d + c->Hk * LS_HD + i] = f32_to_bf16(bv.v[i]);
            }
        }
        a.bmat(q + "self_attn.o_proj.weight", d, d, l.wo); if (ab) a.bvec(q + "self_attn.o_proj.bias", d, l.bo);
        norm("norm_conv", l.ln_cvw, l.ln_cvb);
        conv3(q + "conv.pointwise_conv1.weight", 2 * d, 1, d, l.pw1); if (cb) a.bvec(q + "conv.pointwise_conv1.bias", 2 * d, l.pw1b);
        conv3(q + "conv.pointwise_conv2.weight", d, 1, d, l.pw2); if (cb) a.bvec(q + "conv.pointwise_conv2.bias", d, l.pw2b);
        // inference BatchNorm folded into the depthwise taps and a shift
        const HostTensor& dw = c->raw.need(q + "conv.depthwise_conv.weight", {d, ck, 1});
        const HostTensor* dwb = cb ? &c->raw.need(q + "conv.depthwise_conv.bias", {d}) : nullptr;
        const HostTensor& bw = c->raw.need(q + "conv.norm.weight", {d}); const HostTensor& bb = c->raw.need(q + "conv.norm.bias", {d});
        const HostTensor& bm = c->raw.need(q + "conv.norm.running_mean", {d}); const HostTensor& bvv = c->raw.need(q + "conv.norm.running_var", {d});
        const size_t o_dw = a.ftake((size_t)ck * d, l.dw), o_sh = a.ftake(d, l.dwshift);
        fold_bn_dwconv(&fhost[o_dw], &fhost[o_sh], dw.v.data(), dwb ? dwb->v.data() : nullptr, bw.v.data(), bb.v.data(), bm.v.data(), bvv.v.data(), d, ck);
        norm("norm_feed_forward2", l.ln_ff2w, l.ln_ff2b); ffn("feed_forward2", l.ff2_w1, l.ff2_b1, l.ff2_w2, l.ff2_b2);
        norm("norm_out", l.ln_outw, l.ln_outb);
    }
    a.bvec(E + "out_norm.weight", d, c->onw); ln_bias(E + "out_norm.bias", c->onb);
    a.bmat("ctc_head.weight", V, d, c->headw); a.bvec("ctc_head.bias", V, c->headb);
    // ---- upload: every pointer bound above now addresses the device arenas
    a.upload(c->arena, c->farena);
    c->fbr.alloc(2 * mels);
    HIP_CHECK(hipMemcpy(c->fbr.p, ranges.data(), 2 * mels * sizeof(int), hipMemcpyHostToDevice));
    c->fb_range = c->fbr.p;
    // ---- the workspace: every buffer a call touches, for max_batch rows of max_seconds
    const size_t B = c->cfg.max_batch, Fc = c->Fcap, T1c = c->T1cap, M = B * c->T2cap;
    c->pcm.alloc(B * c->maxN); c->melraw.alloc(B * Fc * mels); c->feats.alloc(B * Fc * mels); c->logits.alloc(M * V);
    c->cntN.alloc(B); c->cntF.alloc(B); c->cnt1.alloc(B); c->cnt2.alloc(B); c->pred.alloc(M); c->tokens.alloc(M); c->ntok.alloc(B);
    c->x0.alloc(B * Fc * Kp); c->h0.alloc(B * Fc * d); c->col.alloc(B * T1c * ks * d); c->c0.alloc(B * T1c * d); c->c1.alloc(M * cc);
    c->h.alloc(M * d); c->x.alloc(M * d); c->qkv.alloc(M * NQ); c->att.alloc(M * d); c->ff.alloc(M * std::max<size_t>(f, 2 * d));
    c->enc_out.alloc(M * d);
    c->host_tokens.alloc(M + B);
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of LasrCTCModel, amplitudes as the other engines' synthetic models
extern "C" mis_status mis_lasr_init_synthetic(mis_lasr* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    const int64_t d = c->d, f = c->f, cc = c->cc, ks = c->ks, ck = c->ck;
    const bool ab = c->cfg.attention_bias != 0, cb = c->cfg.convolution_bias != 0;
    const std::string S = "encoder.subsampler.";
    sw.lin(S + "dense_0", d, c->mels, true, 1.0);
    sw.put(S + "conv_0.weight", {d, ks, d}, sqrt(3.0 / (double)(ks * d)), 0.0f); sw.put(S + "conv_0.bias", {d}, 0.05, 0.0f);
    sw.put(S + "conv_1.weight", {cc, ks, d}, sqrt(3.0 / (double)(ks * d)), 0.0f); sw.put(S + "conv_1.bias", {cc}, 0.05, 0.0f);
    sw.lin(S + "dense_1", d, cc, true, 1.0);
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li) + ".";
        for (const char* n : {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"}) sw.norm(q + n, d);
        for (const char* n : {"feed_forward1", "feed_forward2"}) {
            sw.lin(q + n + ".linear1", f, d, ab, 1.0); sw.lin(q + n + ".linear2", d, f, ab, 0.5);
        }
        sw.lin(q + "self_attn.q_proj", d, d, ab, 1.0); sw.lin(q + "self_attn.k_proj", (int64_t)c->Hk * LS_HD, d, ab, 1.0);
        sw.lin(q + "self_attn.v_proj", (int64_t)c->Hk * LS_HD, d, ab, 1.0); sw.lin(q + "self_attn.o_proj", d, d, ab, 0.5);
        sw.put(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, sqrt(3.0 / (double)d), 0.0f);
        sw.put(q + "conv.pointwise_conv2.weight", {d, 1, d}, 0.5 * sqrt(3.0 / (double)d), 0.0f);
        sw.put(q + "conv.depthwise_conv.weight", {d, ck, 1}, sqrt(3.0 / (double)ck), 0.0f);
        if (cb) {
            sw.put(q + "conv.pointwise_conv1.bias", {2 * d}, 0.05, 0.0f); sw.put(q + "conv.pointwise_conv2.bias", {d}, 0.05, 0.0f);
            sw.put(q + "conv.depthwise_conv.bias", {d}, 0.05, 0.0f);
        }
        sw.put(q + "conv.norm.weight", {d}, 0.1, 1.0f); sw.put(q + "conv.norm.bias", {d}, 0.05, 0.0f);
        sw.put(q + "conv.norm.running_mean", {d}, 0.05, 0.0f); sw.put(q + "conv.norm.running_var", {d}, 0.1, 1.0f);
    }
    sw.norm("encoder.out_norm", d);
    sw.lin("ctc_head", c->V, d, true, 1.0);
    MIS_API_END
}

// ============================================================================ front end
// k_nemo_log_mel (pre-emphasis 0.97, no scale) and k_nemo_norm of audio_front.h; then
// f32 features [B][Fp][mels] -> bf16 rows [B Fp][Kp] (the single rounding of the front end), zero behind F[b] and in the padding columns
__global__ void __launch_bounds__(256) k_lasr_pack(const float* __restrict__ feats, const int* __restrict__ F, bf16_t* __restrict__ out, int Fp,
                                                   int mels, int Kp, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / Kp;
    const int k = (int)(i - row * Kp), b = (int)(row / Fp), t = (int)(row - (size_t)b * Fp);
    out[i] = (k < mels && t < F[b]) ? f32_to_bf16(feats[row * mels + k]) : (bf16_t)0;
}

// ============================================================================ stem patches
// out[(b Tout + t)][k C + c] = in[(b Tin + t s + k)][c] for t < cnt[b], zero behind it; eight values a thread
__global__ void __launch_bounds__(256) k_lasr_im2col(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, const int* __restrict__ cnt, int Tin,
                                                     int Tout, int C, int ks, int st, size_t total8) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total8) return;
    const int C8 = C >> 3;
    const int c8 = (int)(i % C8);
    size_t r = i / C8;
    const int k = (int)(r % ks);
    r /= ks;
    const int t = (int)(r % Tout), b = (int)(r / Tout);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (t < cnt[b]) v = *reinterpret_cast<const uint4*>(in + ((size_t)b * Tin + (size_t)t * st + k) * C + c8 * 8);
    reinterpret_cast<uint4*>(out)[i] = v;
}

// ============================================================================ GEMM
// C[m][n] = sum_k X[m][k] W[n][k]: 2 x 2 waves, a wave holds TI x TI MFMA tiles (block tile 32 TI squared), BK = 32, the next k-slab in
// registers while this one is multiplied.  One MFMA per 32 k in ascending order whatever TI: both tile sizes give the same bits.
// Epilogues, v = T(acc + bias): LG_BIAS v; LG_RELU T(max(v, 0)); LG_SILU T(v sigmoid(v)); LG_AXPBY T(a R + b v) (R may be C);
// LG_F32 acc + bias unrounded, f32, any N.  cnt != null: rows m with m % Tp >= cnt[m / Tp] are written as zero.
enum { LG_BIAS = 0, LG_RELU = 1, LG_SILU = 2, LG_AXPBY = 3, LG_F32 = 4 };
struct LasrGemm {
    const bf16_t *X, *W, *bias, *R;
    void* C;
    int M, N, K, ldx;
    float a, b;
    const int* cnt;
    int Tp;
};
template <int EPI, int TI>
__global__ void __launch_bounds__(256) k_lasr_gemm(LasrGemm p) {
    constexpr int BT = 32 * TI;
    __shared__ __attribute__((aligned(16))) bf16_t Ws[BT][BF16_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Xs[BT][BF16_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * BT, m0 = blockIdx.y * BT;
    const int wn = wave >> 1, wm = wave & 1;
    f32x4_t acc[TI][TI];
    bf16_tile_contract<TI>(p.W, p.X, p.ldx, p.M, p.N, p.K, n0, m0, Ws, Xs, acc);
    // C/D lane l, register e: n = 4 (l >> 4) + e (A rows), m = l & 15 (B columns)
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const int n = n0 + wn * 16 * TI + i * 16 + (lane >> 4) * 4;
        if (n >= p.N) continue;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[e] = (n + e < p.N) ? bf16_to_f32(p.bias[n + e]) : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < TI; ++j) {
            const int m = m0 + wm * 16 * TI + j * 16 + (lane & 15);
            if (m >= p.M) continue;
            const bool valid = !p.cnt || (m % p.Tp) < p.cnt[m / p.Tp];
            if (EPI == LG_F32) {
                float* o = static_cast<float*>(p.C) + (size_t)m * p.N + n;
#pragma unroll
                for (int e = 0; e < 4; ++e) if (n + e < p.N) o[e] = valid ? acc[i][j][e] + bv[e] : 0.0f;
                continue;
            }
            float rv[4] = {0.f, 0.f, 0.f, 0.f};
            if (EPI == LG_AXPBY) bf16x4_unpack(*reinterpret_cast<const uint2*>(p.R + (size_t)m * p.N + n), rv);
            uint16_t res[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = bf16_round_f32(acc[i][j][e] + bv[e]);
                if (EPI == LG_RELU) v = fmaxf(v, 0.0f);
                if (EPI == LG_SILU) v = v / (1.0f + __expf(-v));
                if (EPI == LG_AXPBY) v = fmaf(p.a, rv[e], p.b * v);
                res[e] = valid ? f32_to_bf16(v) : (uint16_t)0;
            }
            *reinterpret_cast<uint2*>(static_cast<bf16_t*>(p.C) + (size_t)m * p.N + n) = bf16x4_pack(res[0], res[1], res[2], res[3]);      // (N % 4 == 0 for every bf16 output)
        }
    }
}
// tile: 0 the rule below, 2 / 4 that tile whatever the grid (tests); returns the TI that ran
template <int EPI>
static int ls_gemm_epi(mis_lasr* c, const LasrGemm& p, int tile) {
    // the 128 x 128 tile once its grid fills the chip, the 64 x 64 tile (four times the blocks) below that
    const bool big = tile ? tile == 4 : (long)cdiv(p.N, 128) * cdiv(p.M, 128) >= 256;
    if (big) MIS_LAUNCH(c, (k_lasr_gemm<EPI, 4>), dim3(cdiv(p.N, 128), cdiv(p.M, 128)), dim3(256), p);
    else MIS_LAUNCH(c, (k_lasr_gemm<EPI, 2>), dim3(cdiv(p.N, 64), cdiv(p.M, 64)), dim3(256), p);
    return big ? 4 : 2;
}
static int ls_gemm(mis_lasr* c, int epi, const bf16_t* X, int ldx, const bf16_t* W, const bf16_t* bias, void* C, int M, int N, int K,
                   const bf16_t* R = nullptr, float ra = 0.0f, float rb = 0.0f, const int* cnt = nullptr, int Tp = 1, int tile = 0) {
    MIS_REQUIRE(K % 32 == 0 && ldx % 8 == 0 && (epi == LG_F32 || N % 4 == 0) && M >= 1, MIS_ERR_GENERATION_FAILED, "LASR GEMM: unsupported shape");
    const LasrGemm p{X, W, bias, R, C, M, N, K, ldx, ra, rb, cnt, Tp};
    switch (epi) {
        case LG_BIAS: return ls_gemm_epi<LG_BIAS>(c, p, tile);
        case LG_RELU: return ls_gemm_epi<LG_RELU>(c, p, tile);
        case LG_SILU: return ls_gemm_epi<LG_SILU>(c, p, tile);
        case LG_AXPBY: return ls_gemm_epi<LG_AXPBY>(c, p, tile);
        case LG_F32: return ls_gemm_epi<LG_F32>(c, p, tile);
        default: throw MisError(MIS_ERR_GENERATION_FAILED, "unknown LASR GEMM epilogue");
    }
}

// ============================================================================ LayerNorm
// y = T((x - mean) rstd w + b), f32 statistics in two passes, one wave per row; cnt != null: rows behind the row count are zero
__global__ void __launch_bounds__(256) k_lasr_ln(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, const bf16_t* __restrict__ w,
                                                 const bf16_t* __restrict__ bias, int d, float eps, int M, const int* __restrict__ cnt, int Tp) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int d2 = d >> 1;
    const uint32_t* xr = reinterpret_cast<const uint32_t*>(x + (size_t)row * d);
    uint32_t* yr = reinterpret_cast<uint32_t*>(y + (size_t)row * d);
    if (cnt && (row % Tp) >= cnt[row / Tp]) {
        for (int i = lane; i < d2; i += 64) yr[i] = 0u;
        return;
    }
    float s = 0.0f;
    for (int i = lane; i < d2; i += 64) { const uint32_t u = xr[i]; s += __uint_as_float(u << 16) + __uint_as_float(u & 0xffff0000u); }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.0f;
    for (int i = lane; i < d2; i += 64) {
        const uint32_t u = xr[i];
        const float a = __uint_as_float(u << 16) - mean, b = __uint_as_float(u & 0xffff0000u) - mean;
        q += a * a + b * b;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
    const uint32_t* wr = reinterpret_cast<const uint32_t*>(w);
    const uint32_t* br = reinterpret_cast<const uint32_t*>(bias);
    for (int i = lane; i < d2; i += 64) {
        const uint32_t u = xr[i], wu = wr[i], bu = br[i];
        const float a = (__uint_as_float(u << 16) - mean) * rstd * __uint_as_float(wu << 16) + __uint_as_float(bu << 16);
        const float b = (__uint_as_float(u & 0xffff0000u) - mean) * rstd * __uint_as_float(wu & 0xffff0000u) + __uint_as_float(bu & 0xffff0000u);
        yr[i] = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
    }
}

// ============================================================================ attention
// rotate-half RoPE over the whole head (:16-21,110-111): column i < 32 pairs with i + 32; T(x cos + rotate_half(x) sin) in f32 with one
// rounding.  Heads 0 .. nheads - 1 of 64 columns from column 0 (q heads, then k heads) of rows [M][ld], position m % Tp, in place.
__global__ void __launch_bounds__(256) k_lasr_rope(bf16_t* __restrict__ rows, int ld, int nheads, int Tp, const float* __restrict__ cs,
                                                   const float* __restrict__ sn, size_t M) {
    const int lane = threadIdx.x & 63;
    const size_t item = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= M * nheads) return;
    const size_t m = item / nheads;
    const int h = (int)(item - m * nheads), pos = (int)(m % Tp);
    bf16_t* p = rows + m * ld + h * LS_HD + lane;
    const float x = bf16_to_f32(*p), partner = __shfl_xor(x, 32, 64);
    const float c = cs[(size_t)pos * 32 + (lane & 31)], s = sn[(size_t)pos * 32 + (lane & 31)];
    *p = f32_to_bf16(fmaf(x, c, (lane < 32 ? -partner : partner) * s));
}

// Non-causal attention over the row's own n = cnt[b] keys (:121-127).  grid (ceil(Tp / 64), H, B), 4 waves x 16 queries.  A 32-key tile
// of the head's K and V columns of the q|k|v rows goes through LDS once per block (keys >= n are staged as ZERO, whatever the rows hold
// there): K in row order, V transposed, so that both MFMA operands are single 16-byte LDS reads.  S^T = K Q^T with the K rows taken in
// the order (0-3, 8-11, 16-19, 24-27 | 4-7, ...), which leaves lane (query j, group g) with the scores of keys 8 g .. 8 g + 7 - the A
// operand of O += P V as it stands.  Online softmax in f32; P as bf16 hi + lo.  Queries >= n are written as zero.
__global__ void __launch_bounds__(256) k_lasr_attn(const bf16_t* __restrict__ qkv, int ld, int H, int Hkv, const int* __restrict__ cnt, int Tp,
                                                   float scale, bf16_t* __restrict__ out, int ldo) {
    __shared__ __attribute__((aligned(16))) bf16_t ks[32][72];
    __shared__ __attribute__((aligned(16))) bf16_t vt[LS_HD][40];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, hk = h / (H / Hkv), q0 = blockIdx.x * 64, n = min(cnt[b], Tp);
    const size_t rowbase = (size_t)b * Tp;
    if (q0 >= n) {                                                 // (uniform over the block)
        for (int i = tid; i < 64 * LS_HD; i += 256) {
            const int t = q0 + (i >> 6);
            if (t < Tp) out[(rowbase + t) * ldo + h * LS_HD + (i & 63)] = 0;
        }
        return;
    }
    const int j = lane & 15, g4 = lane >> 4, t0 = q0 + wave * 16, tq = t0 + j;
    bf16x8_t qf[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (tq < n) qf[c] = *reinterpret_cast<const bf16x8_t*>(qkv + (rowbase + tq) * ld + h * LS_HD + c * 32 + g4 * 8);
        else qf[c] = (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
    }
    const bf16_t* Kg = qkv + rowbase * ld + (size_t)(H + hk) * LS_HD;
    const bf16_t* Vg = qkv + rowbase * ld + (size_t)(H + Hkv + hk) * LS_HD;
    const int sr = tid >> 3, sc8 = (tid & 7) * 8;                  // staging: key sr of the tile, columns sc8 .. + 8
    const int pr0 = ((j >> 2) << 3) | (j & 3);
    f32x4_t O[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) O[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.0f;
    const int n_tiles = (n + 31) >> 5;
    for (int tile = 0; tile < n_tiles; ++tile) {
        const int kb = tile * 32;
        __syncthreads();                                          // the previous tile's reads are done
        {
            const int key = kb + sr;
            uint4 kv = make_uint4(0, 0, 0, 0), vv = kv;
            if (key < n) {
                kv = *reinterpret_cast<const uint4*>(Kg + (size_t)key * ld + sc8);
                vv = *reinterpret_cast<const uint4*>(Vg + (size_t)key * ld + sc8);
            }
            *reinterpret_cast<uint4*>(&ks[sr][sc8]) = kv;
            const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) { vt[sc8 + 2 * e][sr] = (bf16_t)(w[e] & 0xffffu); vt[sc8 + 2 * e + 1][sr] = (bf16_t)(w[e] >> 16); }
        }
        __syncthreads();
        f32x4_t S0 = (f32x4_t){0.f, 0.f, 0.f, 0.f}, S1 = S0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const bf16x8_t a0 = *reinterpret_cast<const bf16x8_t*>(&ks[pr0][c * 32 + g4 * 8]);
            const bf16x8_t a1 = *reinterpret_cast<const bf16x8_t*>(&ks[pr0 | 4][c * 32 + g4 * 8]);
            S0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, qf[c], S0, 0, 0, 0);
            S1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, qf[c], S1, 0, 0, 0);
        }
        float sc[8], mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = (e < 4 ? S0[e] : S1[e - 4]) * scale;
            v = (kb + g4 * 8 + e < n) ? v : -INFINITY;
            sc[e] = v;
            mx = fmaxf(mx, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                     // finite: every tile holds a key < n
        const float alpha = __expf(m_run - m_new);
        float psum = 0.0f;
        bf16x8_t ph, pl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float pe = __expf(sc[e] - m_new);
            psum += pe;
            const bf16_t hi = f32_to_bf16(pe);
            const bf16_t lo = f32_to_bf16(pe - bf16_to_f32(hi));
            ph[e] = (short)hi;
            pl[e] = (short)lo;
        }
        l_run = l_run * alpha + psum;
        m_run = m_new;
        float ar[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, g4 * 4 + r, 64);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const bf16x8_t vb = *reinterpret_cast<const bf16x8_t*>(&vt[dt * 16 + j][g4 * 8]);
            f32x4_t o = O[dt];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] *= ar[r];
            o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vb, o, 0, 0, 0);
            o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl, vb, o, 0, 0, 0);
            O[dt] = o;
        }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    // O[dt][r]: query 4 g + r, column 16 dt + j; the query's normaliser lives in lane 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float lr = __shfl(l_run, g4 * 4 + r, 64);
        const int tr = t0 + g4 * 4 + r;
        if (tr < Tp) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                out[(rowbase + tr) * ldo + h * LS_HD + dt * 16 + j] = tr < n ? f32_to_bf16(O[dt][r] / lr) : (bf16_t)0;
        }
    }
}

// ============================================================================ conv module
// pw [M][2C] (pointwise_conv1) -> out [M][C]: g = T(a sigmoid(b)) (a the first C columns, b the last, :172-173), zero padding of
// (k - 1) / 2 frames in front and k - 1 - (k - 1) / 2 behind the row's own n = cnt[b] frames (:174), depthwise conv with the BatchNorm
// folded in (taps [k][C], shift [C], f32), activation, one rounding.  A block is 64 output frames x 64 channels of one row: the tile's
// 64 + k - 1 gated frames sit in LDS as f32; a wave is 16 frames, a lane a channel.
template <int ACT>
__global__ void __launch_bounds__(256) k_lasr_glu_dwconv(const bf16_t* __restrict__ pw, const float* __restrict__ taps,
                                                         const float* __restrict__ shift, const int* __restrict__ cnt, bf16_t* __restrict__ out,
                                                         int Tp, int C, int k) {
    __shared__ float g[LS_DW_TT + LS_DW_MAXK - 1][64];
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6, ch = blockIdx.y * 64 + cl, b = blockIdx.z, t0 = blockIdx.x * LS_DW_TT;
    const int n = min(cnt[b], Tp), padl = (k - 1) >> 1;
    const bool live = ch < C;
    const size_t rowbase = (size_t)b * Tp;
    for (int r = tl; r < LS_DW_TT + k - 1; r += 4) {
        const int t = t0 - padl + r;
        float v = 0.0f;
        if (live && t >= 0 && t < n) {
            const bf16_t* row = pw + (rowbase + t) * 2 * C;
            const float a = bf16_to_f32(row[ch]), gate = bf16_to_f32(row[C + ch]);
            v = bf16_round_f32(a / (1.0f + __expf(-gate)));
        }
        g[r][cl] = v;
    }
    __syncthreads();
    if (!live) return;
    float acc[16];
    const float sh = shift[ch];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = sh;
    for (int kk = 0; kk < k; ++kk) {
        const float w = taps[(size_t)kk * C + ch];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = fmaf(w, g[tl * 16 + i + kk][cl], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + tl * 16 + i;
        if (t >= Tp) continue;
        float v = acc[i];
        v = ACT == 1 ? fmaxf(v, 0.0f) : v / (1.0f + __expf(-v));
        out[(rowbase + t) * C + ch] = t < n ? f32_to_bf16(v) : (bf16_t)0;
    }
}

// ============================================================================ CTC tail
// arg-max of a frame's V logits, lowest index on ties (MLX argMax); one wave per frame
__global__ void __launch_bounds__(256) k_lasr_argmax(const float* __restrict__ logits, int V, int M, int* __restrict__ pred) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* x = logits + (size_t)row * V;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int i = lane; i < V; i += 64) {
        const float v = x[i];
        if (v > best || (v == best && i < idx)) { best = v; idx = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) pred[row] = (idx < 0 || idx >= V) ? 0 : idx;    // (a frame of NaNs: no comparison holds)
}
// greedy CTC (Wav2Vec2CTC.swift:520-542): frame t < cnt[b] emits its token when it differs from frame t - 1's (-1 in front of frame 0)
// and is not the blank; the kept tokens are compacted in frame order into tokens[b][0 .. ntok[b]).  One block per row.
__global__ void __launch_bounds__(256) k_lasr_collapse(const int* __restrict__ pred, const int* __restrict__ cnt, int Tp, int blank,
                                                       int* __restrict__ tokens, int* __restrict__ ntok) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = min(cnt[b], Tp);
    const int* p = pred + (size_t)b * Tp;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int t = c0 + tid;
        int tok = 0;
        bool keep = false;
        if (t < n) { tok = p[t]; keep = tok != blank && tok != (t > 0 ? p[t - 1] : -1); }
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(mask);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (keep) tokens[(size_t)b * Tp + off + before] = tok;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) ntok[b] = base;
}

// ============================================================================ the chain
static void ls_check_ready(const mis_lasr* c, int batch) {
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch %d outside 1..%d (max_batch)", batch, c->cfg.max_batch);
}
// frame counts of every row from its feature frames; need_stem: rejects a row the stem cannot take (the front end alone takes any row)
static void ls_set_frames(mis_lasr* c, const std::vector<int>& F, int Fp, bool need_stem) {
    const int B = (int)F.size();
    std::vector<int> t1(B), t2(B);
    int Fmax = 0;
    for (int b = 0; b < B; ++b) {
        MIS_REQUIRE(F[b] >= 0 && F[b] <= Fp, MIS_ERR_INVALID_INPUT, "row %d: %d frames exceed the row stride %d", b, F[b], Fp);
        t1[b] = ls_conv_out(F[b], c->ks, c->st); t2[b] = ls_conv_out(t1[b], c->ks, c->st);
        MIS_REQUIRE(!need_stem || t2[b] >= 1, MIS_ERR_INVALID_INPUT, "row %d: %d feature frames are too short for the conv stem (kernel %d, stride %d)", b, F[b],
                    c->ks, c->st);
        Fmax = std::max(Fmax, F[b]);
    }
    MIS_REQUIRE(Fp <= c->Fcap, MIS_ERR_INVALID_INPUT, "%d feature frames exceed the workspace of %d (max_seconds %d)", Fp, c->Fcap, c->cfg.max_seconds);
    c->hF = F; c->hT1 = t1; c->hT2 = t2;
    c->batch = B; c->Fp = Fp; c->T1p = ls_conv_out(Fp, c->ks, c->st); c->T2p = ls_conv_out(c->T1p, c->ks, c->st);
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->cntF.p, c->hF.data(), B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt1.p, c->hT1.data(), B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt2.p, c->hT2.data(), B * 4, hipMemcpyHostToDevice, s));
}

// pcm f32 [B][stride] (host or device) -> c->feats [B][Fp][mels]
static void ls_front(mis_lasr* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, bool need_stem) {
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    std::vector<int> N(batch), F(batch);
    int Fp = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the row stride %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->maxN, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the workspace of %d seconds (max_seconds)", b, (long long)n,
                    c->cfg.max_seconds);
        N[b] = (int)n; F[b] = ls_frames(n);
        Fp = std::max(Fp, F[b]);
    }
    ls_set_frames(c, F, Fp, need_stem);
    c->hN = N;
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->cntN.p, c->hN.data(), batch * 4, hipMemcpyHostToDevice, s));
    // the rows are packed at the workspace's own stride: only a row's own samples travel
    const int64_t ws = std::min<int64_t>(stride, c->maxN);
    HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, ws * 4, pcm, stride * 4, ws * 4, batch, hipMemcpyDefault, s));
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[0], s));
    MIS_LAUNCH(c, k_nemo_log_mel<false>, dim3(Fp, batch), dim3(256), c->pcm.p, ws, c->cntN.p, c->cntF.p, nullptr, 0.97f, c->window, c->tw_cos,
              c->tw_sin, c->fb, c->fb_range, c->melraw.p, Fp, c->mels);
    MIS_LAUNCH(c, k_nemo_norm, dim3(cdiv(c->mels, 64), batch), dim3(256), c->melraw.p, c->cntF.p, c->feats.p, Fp, c->mels, 1);
}

// c->feats -> stem -> blocks -> out_norm (c->enc_out).  stop: -1 everything, 0 behind the stem, 1 .. L behind that block.
static void ls_encoder(mis_lasr* c, int stop) {
    const int B = c->batch, d = c->d, f = c->f, Fp = c->Fp, T1p = c->T1p, T2p = c->T2p, ks = c->ks, st = c->st, M = B * T2p;
    const int NQ = (c->H + 2 * c->Hk) * LS_HD;
    const int act = c->cfg.hidden_act == 1 ? LG_RELU : LG_SILU;
    const float eps = c->cfg.layer_norm_eps, ffa = c->cfg.feed_forward_residual_weights[0], ffb = c->cfg.feed_forward_residual_weights[1],
                cva = c->cfg.conv_residual_weights[0], cvb = c->cfg.conv_residual_weights[1];
    // ---- stem (:67-72)
    const size_t n0 = (size_t)B * Fp * c->Kp;
    MIS_LAUNCH(c, k_lasr_pack, dim3((unsigned)((n0 + 255) / 256)), dim3(256), c->feats.p, c->cntF.p, c->x0.p, Fp, c->mels, c->Kp, n0);
    ls_gemm(c, LG_RELU, c->x0.p, c->Kp, c->d0w, c->d0b, c->h0.p, B * Fp, d, c->Kp);
    size_t n8 = (size_t)B * T1p * ks * d / 8;
    MIS_LAUNCH(c, k_lasr_im2col, dim3((unsigned)((n8 + 255) / 256)), dim3(256), c->h0.p, c->col.p, c->cnt1.p, Fp, T1p, d, ks, st, n8);
    ls_gemm(c, LG_RELU, c->col.p, ks * d, c->c0w, c->c0b, c->c0.p, B * T1p, d, ks * d);
    n8 = (size_t)B * T2p * ks * d / 8;
    MIS_LAUNCH(c, k_lasr_im2col, dim3((unsigned)((n8 + 255) / 256)), dim3(256), c->c0.p, c->col.p, c->cnt2.p, T1p, T2p, d, ks, st, n8);
    ls_gemm(c, LG_RELU, c->col.p, ks * d, c->c1w, c->c1b, c->c1.p, M, c->cc, ks * d);
    ls_gemm(c, LG_BIAS, c->c1.p, c->cc, c->d1w, c->d1b, c->h.p, M, d, c->cc, nullptr, 0.0f, 0.0f, c->cnt2.p, T2p);
    if (stop == 0) return;
    // ---- blocks (:226-245), 16 launches each
    const float scale = 1.0f / sqrtf((float)LS_HD);
    auto ln = [&](const bf16_t* x, bf16_t* y, const bf16_t* w, const bf16_t* b, const int* cnt) {
        MIS_LAUNCH(c, k_lasr_ln, dim3(cdiv(M, 4)), dim3(256), x, y, w, b, d, eps, M, cnt, T2p);
    };
    for (int li = 0; li < c->L; ++li) {
        const LsLayer& l = c->layers[li];
        ln(c->h.p, c->x.p, l.ln_ff1w, l.ln_ff1b, nullptr);
        ls_gemm(c, act, c->x.p, d, l.ff1_w1, l.ff1_b1, c->ff.p, M, f, d);
        ls_gemm(c, LG_AXPBY, c->ff.p, f, l.ff1_w2, l.ff1_b2, c->h.p, M, d, f, c->h.p, ffa, ffb);
        ln(c->h.p, c->x.p, l.ln_attw, l.ln_attb, nullptr);
        ls_gemm(c, LG_BIAS, c->x.p, d, l.wqkv, l.bqkv, c->qkv.p, M, NQ, d);
        const size_t items = (size_t)M * (c->H + c->Hk);
        MIS_LAUNCH(c, k_lasr_rope, dim3((unsigned)((items + 3) / 4)), dim3(256), c->qkv.p, NQ, c->H + c->Hk, T2p, c->rope_cos, c->rope_sin, (size_t)M);
        MIS_LAUNCH(c, k_lasr_attn, dim3(cdiv(T2p, 64), c->H, B), dim3(256), c->qkv.p, NQ, c->H, c->Hk, c->cnt2.p, T2p, scale, c->att.p, d);
        ls_gemm(c, LG_AXPBY, c->att.p, d, l.wo, l.bo, c->h.p, M, d, d, c->h.p, 1.0f, 1.0f);
        ln(c->h.p, c->x.p, l.ln_cvw, l.ln_cvb, nullptr);
        ls_gemm(c, LG_BIAS, c->x.p, d, l.pw1, l.pw1b, c->ff.p, M, 2 * d, d);
        if (c->cfg.hidden_act == 1)
            MIS_LAUNCH(c, (k_lasr_glu_dwconv<1>), dim3(cdiv(T2p, LS_DW_TT), cdiv(d, 64), B), dim3(256), c->ff.p, l.dw, l.dwshift, c->cnt2.p, c->att.p, T2p, d, c->ck);
        else
            MIS_LAUNCH(c, (k_lasr_glu_dwconv<0>), dim3(cdiv(T2p, LS_DW_TT), cdiv(d, 64), B), dim3(256), c->ff.p, l.dw, l.dwshift, c->cnt2.p, c->att.p, T2p, d, c->ck);
        ls_gemm(c, LG_AXPBY, c->att.p, d, l.pw2, l.pw2b, c->h.p, M, d, d, c->h.p, cva, cvb);
        ln(c->h.p, c->x.p, l.ln_ff2w, l.ln_ff2b, nullptr);
        ls_gemm(c, act, c->x.p, d, l.ff2_w1, l.ff2_b1, c->ff.p, M, f, d);
        ls_gemm(c, LG_AXPBY, c->ff.p, f, l.ff2_w2, l.ff2_b2, c->x.p, M, d, f, c->h.p, ffa, ffb);
        ln(c->x.p, c->h.p, l.ln_outw, l.ln_outb, c->cnt2.p);
        if (stop == li + 1) return;
    }
    ln(c->h.p, c->enc_out.p, c->onw, c->onb, c->cnt2.p);
}

static void ls_head(mis_lasr* c) {
    ls_gemm(c, LG_F32, c->enc_out.p, c->d, c->headw, c->headb, c->logits.p, c->batch * c->T2p, c->V, c->d, nullptr, 0.0f, 0.0f, c->cnt2.p, c->T2p);
}

extern "C" int mis_lasr_launches(const mis_lasr* c) { return c ? c->launches : 0; }

// copies [B][Tp][W] f32 device rows into out [B][Tp][W]
static void ls_copy_out(mis_lasr* c, const float* dev, float* out, size_t n) {
    HIP_CHECK(hipMemcpyAsync(out, dev, n * 4, hipMemcpyDeviceToHost, c->stream));
}

extern "C" mis_status mis_lasr_features(mis_lasr* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* feats_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && feats_out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    ls_check_ready(c, batch);
    c->launches = 0;
    ls_front(c, pcm, lens, batch, stride, false);
    ls_copy_out(c, c->feats.p, feats_out, (size_t)batch * c->Fp * c->mels);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    MIS_API_END
}

extern "C" mis_status mis_lasr_forward_features(mis_lasr* c, const float* feats, const int32_t* frames, int batch, int F, float* logits_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && feats && logits_out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    ls_check_ready(c, batch);
    MIS_REQUIRE(F >= 1, MIS_ERR_INVALID_INPUT, "bad frame count");
    std::vector<int> fr(batch, F);
    if (frames) for (int b = 0; b < batch; ++b) fr[b] = frames[b];
    c->launches = 0;
    ls_set_frames(c, fr, F, true);
    HIP_CHECK(hipMemcpyAsync(c->feats.p, feats, (size_t)batch * F * c->mels * 4, hipMemcpyDefault, c->stream));
    ls_encoder(c, -1);
    ls_head(c);
    ls_copy_out(c, c->logits.p, logits_out, (size_t)batch * c->T2p * c->V);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    MIS_API_END
}

extern "C" mis_status mis_lasr_forward(mis_lasr* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* logits_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && logits_out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    ls_check_ready(c, batch);
    c->launches = 0;
    ls_front(c, pcm, lens, batch, stride, true);
    ls_encoder(c, -1);
    ls_head(c);
    ls_copy_out(c, c->logits.p, logits_out, (size_t)batch * c->T2p * c->V);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    MIS_API_END
}

extern "C" mis_status mis_stt_lasr_generate(mis_lasr* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int32_t* tokens_out,
                                            int64_t tokens_stride, int32_t* n_tokens) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && tokens_out && n_tokens && tokens_stride >= 1, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    ls_check_ready(c, batch);
    c->launches = 0;
    hipStream_t s = c->stream;
    ls_front(c, pcm, lens, batch, stride, true);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[1], s));
    ls_encoder(c, -1);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[2], s));
    ls_head(c);
    const int M = batch * c->T2p;
    MIS_LAUNCH(c, k_lasr_argmax, dim3(cdiv(M, 4)), dim3(256), c->logits.p, c->V, M, c->pred.p);
    MIS_LAUNCH(c, k_lasr_collapse, dim3(batch), dim3(256), c->pred.p, c->cnt2.p, c->T2p, c->cfg.pad_token_id, c->tokens.p, c->ntok.p);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[3], s));
    int32_t* ht = c->host_tokens.p;
    HIP_CHECK(hipMemcpyAsync(ht, c->tokens.p, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ht + M, c->ntok.p, batch * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                            // the call's one synchronisation
    for (int b = 0; b < batch; ++b) {
        const int n = (int)std::min<int64_t>(ht[M + b], tokens_stride);
        n_tokens[b] = n;
        memcpy(tokens_out + (size_t)b * tokens_stride, ht + (size_t)b * c->T2p, (size_t)n * 4);
    }
    MIS_API_END
}

// tensors of the last call, f32 [B][T2p][d], zero rows behind a row's own T2: stage 0 the stem's output, 1 .. L that block's output,
// L + 1 out_norm.  The chain is deterministic and the call's features are still in the workspace: stages 0 .. L are recomputed from
// them (the same bits as the call produced), out_norm is read where the call left it.
extern "C" mis_status mis_lasr_tap(mis_lasr* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && dims, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized && c->batch > 0, MIS_ERR_NOT_INITIALIZED, "no call to tap");
    MIS_REQUIRE(stage >= 0 && stage <= c->L + 1, MIS_ERR_INVALID_INPUT, "stage %d outside 0..%d", stage, c->L + 1);
    HIP_CHECK(hipSetDevice(c->device));
    dims[0] = c->batch; dims[1] = c->T2p; dims[2] = c->d;
    if (!out) return MIS_OK;
    const size_t n = (size_t)c->batch * c->T2p * c->d;
    MIS_REQUIRE((int64_t)n <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    const int kept = c->launches;
    if (stage <= c->L) ls_encoder(c, stage);
    c->launches = kept;
    const bf16_t* src = stage <= c->L ? c->h.p : c->enc_out.p;
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<bf16_t> hostv(n);
    HIP_CHECK(hipMemcpy(hostv.data(), src, n * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = bf16_to_f32(hostv[i]);
    MIS_API_END
}

// benches: device milliseconds of the next / last mis_stt_lasr_generate: front end, encoder, tail
extern "C" mis_status mis_debug_lasr_timing(mis_lasr* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    if (!ms) { c->timed = true; return MIS_OK; }
    MIS_REQUIRE(c->timed && c->batch > 0, MIS_ERR_NOT_INITIALIZED, "no timed generate");
    for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    MIS_API_END
}

// ============================================================================ test scaffolding (include/mi_speech_debug.h)
// ONE call of ls_gemm, or one launch line of ls_encoder / mis_stt_lasr_generate, on caller-supplied host data, so that
// tests/test_gpu_lasr_ops.py can hold the kernels above to an operator-level reference.  Nothing is computed here: the operands are
// uploaded as given and what the launch wrote is copied back.  Guards as gemm_debug.hip, attn_debug.hip, codec_debug.hip and
// enc_debug.hip (debug_guard.h): every output is [guard | body | guard], all of it the byte 0xFF before the launch (an output that
// also goes IN - the rotated rows, the in-place residual - holds the caller's data instead); a changed guard byte or padding column
// fails the call; every input is followed by IN_GUARD NaNs (ints: 0x7FFFFFFF).  The entry points refuse what would make a KERNEL leave
// these buffers; what ls_gemm refuses is returned as its status and nothing is launched.  The launches run on a bare mis_lasr (device
// and the null stream, no weights, no workspace): the launchers need nothing else of it.
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

namespace {

constexpr int64_t LSD_MAX_ELEMS = (int64_t)1 << 28;          // per tensor

void lsd_sync(const mis_lasr& c) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
}
void lsd_open(mis_lasr& c, int device) {
    HIP_CHECK(hipSetDevice(device));
    c.device = device;
}
// counts [n] followed by 0x7FFFFFFF (a row count that masks nothing)
void lsd_counts(DevBuf<uint32_t>& d, const int32_t* cnt, size_t n) { alloc32(d, cnt, n, 0x7FFFFFFFu); }
const int* lsd_int(const DevBuf<uint32_t>& d) { return reinterpret_cast<const int*>(d.p); }
// the body of a guarded output
void lsd_fetch(GuardedOut& o, void* out) {
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
}
// rows of ld with `cols` live columns -> the live columns; the columns behind must still hold the fill
void lsd_fetch16_rows(GuardedOut& o, size_t rows, size_t ld, size_t cols, uint16_t* out) {
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

extern "C" mis_status mis_debug_lasr_gemm(int device, int epi, const uint16_t* X, const uint16_t* W, const uint16_t* bias, const uint16_t* R, float a,
                                          float b, const int32_t* cnt, int Tp, int in_place, int tile, int M, int N, int K, int ldx, void* C_out,
                                          uint16_t* R_after, int32_t* report) {
    MIS_API_BEGIN
    if (report) { report[0] = -1; report[1] = 0; }
    MIS_REQUIRE(X && W && C_out && M >= 1 && N >= 1 && K >= 1 && ldx >= 1, MIS_ERR_INVALID_INPUT, "LASR GEMM: X, W, C_out and positive M, N, K, ldx are required");
    MIS_REQUIRE((int64_t)M * N <= LSD_MAX_ELEMS && (int64_t)N * K <= LSD_MAX_ELEMS && (int64_t)(M - 1) * ldx + K <= LSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "LASR GEMM: tensor too large");
    MIS_REQUIRE(epi != LG_AXPBY || R, MIS_ERR_INVALID_INPUT, "LASR GEMM: the epilogue needs R");
    MIS_REQUIRE(!in_place || epi == LG_AXPBY, MIS_ERR_INVALID_INPUT, "LASR GEMM: in_place is the residual epilogue's");
    MIS_REQUIRE(!cnt || Tp >= 1, MIS_ERR_INVALID_INPUT, "LASR GEMM: row counts need Tp >= 1");
    MIS_REQUIRE(tile == 0 || tile == 2 || tile == 4, MIS_ERR_INVALID_INPUT, "LASR GEMM: tile 0 (the launcher's rule), 2 or 4");
    mis_lasr c;
    lsd_open(c, device);
    DevBuf<uint16_t> dX, dW, dB, dR;
    DevBuf<uint32_t> dcnt;
    {   // the image the kernel addresses: row m at m ldx, K columns; with ldx > K the columns between the rows are NaN
        const size_t n = (size_t)(M - 1) * ldx + K;
        std::vector<uint16_t> h(X, X + n);
        if (ldx > K)
            for (int m = 0; m + 1 < M; ++m) std::fill(h.begin() + (size_t)m * ldx + K, h.begin() + (size_t)(m + 1) * ldx, BF16_NAN);
        alloc16(dX, h.data(), n, BF16_NAN);
    }
    alloc16(dW, W, (size_t)N * K, BF16_NAN);
    if (bias) alloc16(dB, bias, N, BF16_NAN);
    const bool sep = epi == LG_AXPBY && !in_place;
    if (sep) alloc16(dR, R, (size_t)M * N, BF16_NAN);
    if (cnt) lsd_counts(dcnt, cnt, (size_t)cdiv(M, Tp));
    const size_t es = epi == LG_F32 ? 4 : 2;
    GuardedOut o;
    o.alloc((size_t)M * N * es, (size_t)128 * N * es);             // a guard is one 128-row tile of output
    if (in_place) HIP_CHECK(hipMemcpy(o.p(), R, o.body, hipMemcpyHostToDevice));
    const bf16_t* Rp = in_place ? reinterpret_cast<const bf16_t*>(o.p()) : sep ? dR.p : nullptr;
    const int ti = ls_gemm(&c, epi, dX.p, ldx, dW.p, bias ? dB.p : nullptr, o.p(), M, N, K, Rp, a, b, cnt ? lsd_int(dcnt) : nullptr, Tp, tile);
    lsd_sync(c);
    if (report) { report[0] = epi; report[1] = ti; }
    lsd_fetch(o, C_out);
    if (sep && R_after) HIP_CHECK(hipMemcpy(R_after, dR.p, (size_t)M * N * 2, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_lasr_ln(int device, const uint16_t* x, const uint16_t* w, const uint16_t* b, int M, int d, float eps, const int32_t* cnt,
                                        int Tp, uint16_t* y_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && w && b && y_out && M >= 1 && d >= 2 && d % 2 == 0 && (int64_t)M * d <= LSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "LASR LayerNorm: x, w, b, y_out, M >= 1 and an even d (the kernel moves 32-bit pairs) are required");
    MIS_REQUIRE(!cnt || Tp >= 1, MIS_ERR_INVALID_INPUT, "LASR LayerNorm: row counts need Tp >= 1");
    mis_lasr c;
    lsd_open(c, device);
    DevBuf<uint16_t> dx, dw, db;
    DevBuf<uint32_t> dcnt;
    alloc16(dx, x, (size_t)M * d, BF16_NAN);
    alloc16(dw, w, d, BF16_NAN);
    alloc16(db, b, d, BF16_NAN);
    if (cnt) lsd_counts(dcnt, cnt, (size_t)cdiv(M, Tp));
    GuardedOut y;
    y.alloc((size_t)M * d * 2, (size_t)4 * d * 2);
    MIS_LAUNCH(&c, k_lasr_ln, dim3(cdiv(M, 4)), dim3(256), dx.p, reinterpret_cast<bf16_t*>(y.p()), dw.p, db.p, d, eps, M, cnt ? lsd_int(dcnt) : nullptr, Tp);
    lsd_sync(c);
    lsd_fetch(y, y_out);
    MIS_API_END
}

extern "C" mis_status mis_debug_lasr_rope(int device, uint16_t* rows, int M, int ld, int nheads, int Tp, const float* cs, const float* sn) {
    MIS_API_BEGIN
    MIS_REQUIRE(rows && cs && sn && M >= 1 && nheads >= 1 && Tp >= 1 && (int64_t)nheads * LS_HD <= ld, MIS_ERR_INVALID_INPUT,
                "LASR RoPE: rows, both tables, M, Tp >= 1 and 1 <= nheads <= ld / 64 are required");
    MIS_REQUIRE((int64_t)M * ld <= LSD_MAX_ELEMS && (int64_t)Tp * 32 <= LSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "LASR RoPE: tensor too large");
    mis_lasr c;
    lsd_open(c, device);
    DevBuf<uint32_t> dc, ds;
    alloc32(dc, cs, (size_t)Tp * 32, F32_NAN);
    alloc32(ds, sn, (size_t)Tp * 32, F32_NAN);
    GuardedOut r;
    r.alloc((size_t)M * ld * 2, (size_t)4 * ld * 2);
    HIP_CHECK(hipMemcpy(r.p(), rows, r.body, hipMemcpyHostToDevice));
    const size_t items = (size_t)M * nheads;
    MIS_LAUNCH(&c, k_lasr_rope, dim3((unsigned)((items + 3) / 4)), dim3(256), reinterpret_cast<bf16_t*>(r.p()), ld, nheads, Tp,
              reinterpret_cast<const float*>(dc.p), reinterpret_cast<const float*>(ds.p), (size_t)M);
    lsd_sync(c);
    lsd_fetch(r, rows);
    MIS_API_END
}

extern "C" mis_status mis_debug_lasr_attn(int device, const uint16_t* qkv, int ld, int H, int Hkv, const int32_t* cnt, int B, int Tp, float scale, int ldo,
                                          uint16_t* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(qkv && cnt && out && B >= 1 && Tp >= 1 && H >= 1 && Hkv >= 1 && H % Hkv == 0, MIS_ERR_INVALID_INPUT,
                "LASR attention: qkv, cnt, out, B, Tp >= 1 and Hkv dividing H are required");
    MIS_REQUIRE(ld % 8 == 0 && (int64_t)(H + 2 * Hkv) * LS_HD <= ld && (int64_t)H * LS_HD <= ldo, MIS_ERR_INVALID_INPUT,
                "LASR attention: ld >= (H + 2 Hkv) 64 in 16-byte rows, ldo >= H 64");
    MIS_REQUIRE((int64_t)B * Tp * ld <= LSD_MAX_ELEMS && (int64_t)B * Tp * ldo <= LSD_MAX_ELEMS && B <= 65535 && H <= 65535, MIS_ERR_INVALID_INPUT,
                "LASR attention: tensor too large");
    mis_lasr c;
    lsd_open(c, device);
    const size_t rows = (size_t)B * Tp;
    DevBuf<uint16_t> dq;
    DevBuf<uint32_t> dcnt;
    alloc16(dq, qkv, rows * ld, BF16_NAN);
    lsd_counts(dcnt, cnt, B);
    GuardedOut o;
    o.alloc(rows * ldo * 2, (size_t)64 * ldo * 2);
    MIS_LAUNCH(&c, k_lasr_attn, dim3(cdiv(Tp, 64), H, B), dim3(256), dq.p, ld, H, Hkv, lsd_int(dcnt), Tp, scale, reinterpret_cast<bf16_t*>(o.p()), ldo);
    lsd_sync(c);
    lsd_fetch16_rows(o, rows, ldo, (size_t)H * LS_HD, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_lasr_glu_dwconv(int device, int act, const uint16_t* pw, const float* taps, const float* shift, const int32_t* cnt, int B,
                                                int Tp, int C, int k, uint16_t* out, int32_t* report) {
    MIS_API_BEGIN
    if (report) report[0] = -1;
    MIS_REQUIRE(pw && taps && shift && cnt && out && B >= 1 && Tp >= 1 && C >= 1 && (act == 0 || act == 1), MIS_ERR_INVALID_INPUT,
                "LASR GLU + depthwise conv: every pointer, B, Tp, C >= 1 and act 0 / 1 are required");
    MIS_REQUIRE(k >= 1 && k <= LS_DW_MAXK, MIS_ERR_INVALID_INPUT, "LASR GLU + depthwise conv: k %d outside 1..%d (the LDS tile)", k, LS_DW_MAXK);
    MIS_REQUIRE((int64_t)B * Tp * 2 * C <= LSD_MAX_ELEMS && B <= 65535 && cdiv(C, 64) <= 65535, MIS_ERR_INVALID_INPUT, "LASR GLU + depthwise conv: tensor too large");
    mis_lasr c;
    lsd_open(c, device);
    const size_t rows = (size_t)B * Tp;
    DevBuf<uint16_t> dp;
    DevBuf<uint32_t> dt, ds, dcnt;
    alloc16(dp, pw, rows * 2 * C, BF16_NAN);
    alloc32(dt, taps, (size_t)k * C, F32_NAN);
    alloc32(ds, shift, C, F32_NAN);
    lsd_counts(dcnt, cnt, B);
    GuardedOut o;
    o.alloc(rows * C * 2, (size_t)LS_DW_TT * C * 2);
    const float *tp = reinterpret_cast<const float*>(dt.p), *sp = reinterpret_cast<const float*>(ds.p);
    bf16_t* op = reinterpret_cast<bf16_t*>(o.p());
    if (act == 1) MIS_LAUNCH(&c, (k_lasr_glu_dwconv<1>), dim3(cdiv(Tp, LS_DW_TT), cdiv(C, 64), B), dim3(256), dp.p, tp, sp, lsd_int(dcnt), op, Tp, C, k);
    else MIS_LAUNCH(&c, (k_lasr_glu_dwconv<0>), dim3(cdiv(Tp, LS_DW_TT), cdiv(C, 64), B), dim3(256), dp.p, tp, sp, lsd_int(dcnt), op, Tp, C, k);
    lsd_sync(c);
    if (report) report[0] = act;
    lsd_fetch(o, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_lasr_im2col(int device, const uint16_t* in, const int32_t* cnt, int B, int Tin, int Tout, int C, int ks, int st,
                                            uint16_t* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(in && cnt && out && B >= 1 && Tin >= 1 && Tout >= 1 && C >= 8 && C % 8 == 0 && ks >= 1 && st >= 1, MIS_ERR_INVALID_INPUT,
                "LASR im2col: in, cnt, out, positive B, Tin, Tout, ks, st and C a multiple of 8 are required");
    MIS_REQUIRE((int64_t)B * Tin * C <= LSD_MAX_ELEMS && (int64_t)B * Tout * ks * C <= LSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "LASR im2col: tensor too large");
    for (int b = 0; b < B; ++b) {
        const int64_t n = std::min(cnt[b], Tout);
        MIS_REQUIRE(n <= 0 || (n - 1) * st + ks <= Tin, MIS_ERR_INVALID_INPUT, "LASR im2col: row %d: frame %lld reads behind the row's %d input frames", b,
                    (long long)(n - 1), Tin);
    }
    mis_lasr c;
    lsd_open(c, device);
    DevBuf<uint16_t> di;
    DevBuf<uint32_t> dcnt;
    alloc16(di, in, (size_t)B * Tin * C, BF16_NAN);
    lsd_counts(dcnt, cnt, B);
    GuardedOut o;
    const size_t n = (size_t)B * Tout * ks * C, n8 = n / 8;
    o.alloc(n * 2, (size_t)4 * ks * C * 2);
    MIS_LAUNCH(&c, k_lasr_im2col, dim3((unsigned)((n8 + 255) / 256)), dim3(256), di.p, reinterpret_cast<bf16_t*>(o.p()), lsd_int(dcnt), Tin, Tout, C, ks, st, n8);
    lsd_sync(c);
    lsd_fetch(o, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_lasr_pack(int device, const float* feats, const int32_t* F, int B, int Fp, int mels, int Kp, uint16_t* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(feats && F && out && B >= 1 && Fp >= 1 && mels >= 1 && Kp >= mels, MIS_ERR_INVALID_INPUT,
                "LASR pack: feats, F, out, positive B, Fp and 1 <= mels <= Kp are required");
    MIS_REQUIRE((int64_t)B * Fp * Kp <= LSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "LASR pack: tensor too large");
    mis_lasr c;
    lsd_open(c, device);
    DevBuf<uint32_t> df, dcnt;
    alloc32(df, feats, (size_t)B * Fp * mels, F32_NAN);
    lsd_counts(dcnt, F, B);
    GuardedOut o;
    const size_t n = (size_t)B * Fp * Kp;
    o.alloc(n * 2, (size_t)4 * Kp * 2);
    MIS_LAUNCH(&c, k_lasr_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), reinterpret_cast<const float*>(df.p), lsd_int(dcnt), reinterpret_cast<bf16_t*>(o.p()), Fp,
              mels, Kp, n);
    lsd_sync(c);
    lsd_fetch(o, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_lasr_argmax(int device, const float* logits, int M, int V, int32_t* pred) {
    MIS_API_BEGIN
    MIS_REQUIRE(logits && pred && M >= 1 && V >= 1 && (int64_t)M * V <= LSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "LASR arg-max: logits, pred and positive M, V are required");
    mis_lasr c;
    lsd_open(c, device);
    DevBuf<uint32_t> dl;
    alloc32(dl, logits, (size_t)M * V, F32_NAN);
    GuardedOut o;
    o.alloc((size_t)M * 4, 256);
    MIS_LAUNCH(&c, k_lasr_argmax, dim3(cdiv(M, 4)), dim3(256), reinterpret_cast<const float*>(dl.p), V, M, reinterpret_cast<int*>(o.p()));
    lsd_sync(c);
    lsd_fetch(o, pred);
    MIS_API_END
}

extern "C" mis_status mis_debug_lasr_collapse(int device, const int32_t* pred, const int32_t* cnt, int B, int Tp, int blank, int32_t* tokens, int32_t* ntok) {
    MIS_API_BEGIN
    MIS_REQUIRE(pred && cnt && tokens && ntok && B >= 1 && Tp >= 1 && (int64_t)B * Tp <= LSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "LASR CTC collapse: pred, cnt, tokens, ntok and positive B, Tp are required");
    mis_lasr c;
    lsd_open(c, device);
    DevBuf<uint32_t> dp, dcnt;
    alloc32(dp, pred, (size_t)B * Tp, 0x7FFFFFFFu);
    lsd_counts(dcnt, cnt, B);
    GuardedOut t, n;
    t.alloc((size_t)B * Tp * 4, (size_t)Tp * 4);
    n.alloc((size_t)B * 4, 256);
    MIS_LAUNCH(&c, k_lasr_collapse, dim3(B), dim3(256), lsd_int(dp), lsd_int(dcnt), Tp, blank, reinterpret_cast<int*>(t.p()), reinterpret_cast<int*>(n.p()));
    lsd_sync(c);
    lsd_fetch(t, tokens);
    lsd_fetch(n, ntok);
    MIS_API_END
}
