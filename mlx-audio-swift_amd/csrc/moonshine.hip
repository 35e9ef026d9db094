// moonshine.hip - the Moonshine STT engine: raw 16 kHz samples -> strided conv stem -> encoder -> cached decoder -> greedy ids.
//
// Reference being replaced: MoonshineModel / MoonshineEncoder / MoonshineDecoder / MoonshineAttention
// (Sources/MLXAudioSTT/Models/Moonshine/MoonshineModel.swift:112-411).  Tokenizer and text stay on the host (:7-69).
//
// Ragged batch.  A row of n samples has T1 = (n - 127) / 64 + 1 conv1 frames, T2 = (T1 - 7) / 3 + 1, T3 = (T2 - 3) / 2 + 1 (no padding in
// any conv, :309-312).  The batch is laid out with T1pad = 6 * ceil(max T1 / 6), T2pad = T1pad / 3, T3pad = T2pad / 2 frames per row, so
// that frame t2 of row b of conv2 is the CONTIGUOUS span of 7 d values starting at element 3 d (b T2pad + t2) of the GroupNorm output
// (and likewise conv3 on conv2's output): both dense convs are one launch_gemm_big each with ldx = stride * C_in < K = k * C_in, no patch
// matrix.  Frames past a row's own extent are written as zeros by the GroupNorm kernel, the statistics run over the row's own T1 d
// values, and every attention masks keys >= T3[b]: samples past lens[b] never reach a value that is kept.
//
// Precision: f32 from the waveform through GroupNorm (conv1 + tanh, statistics, affine), one rounding to bf16 there; bf16 storage with
// f32 accumulation from conv2 on, rounding at every primitive boundary as in the Whisper engine.  Logits stay f32.
//
// Head sizes 36 / 52 (hidden / heads): every head is zero-padded to 64 at load (rows of q/k/v, columns of o_proj), which leaves scores
// and outputs unchanged; the scale stays head_dim^-0.5 of the real size and RoPE touches the first rotary_dim columns only (:142-147).
//
//   k_ms_conv1_tanh    [T1,127] x [127,d] on overlapping sample windows held in LDS (f32)
//   k_ms_gn_partial    whole-row GroupNorm statistics, two passes over fixed 32768-element chunks (a row's result does not depend on the batch)
//   k_ms_gn_apply      affine + the single rounding to bf16, zeros past T1[b]
//   k_ms_rope_rows     partial interleaved RoPE on the q and k columns of the encoder's q|k|v rows
//   k_ms_attn_enc      non-causal attention over the row's own T3 keys, one wave per query
//   k_ms_gemv          decode-step GEMM for <= 64 rows: LayerNorm in the prologue, bias / residual / SiLU gate in the epilogue
//   k_ms_attn_self     RoPE + cache append + causal attention of the new token;  k_ms_attn_cross  over the cached encoder K/V
//   k_ms_argmax_embed  greedy choice, EOS rule, token bookkeeping and the next token's embedding in one launch
#include "common.h"
#include "host_weights.h"
#include "lm_kernels.h"
#include "whisper_kernels.h"

#include <math.h>
#include <string.h>
#include <memory>

#define MS_DP 64                 // padded head size
#define MS_MAX_SAMPLES 480000    // per-row cap: 30 s at 16 kHz
#define MS_MAX_KEYS 1280         // >= T3 of the cap (1248)
#define MS_MAX_POS 2048          // decoder positions (start token + max_tokens)
#define MS_MAX_BATCH 64
#define MS_GN_CHUNK 32768
static const float MS_EPS = 1e-5f;

struct MsEncLayer { bf16_t *ln1, *ln2, *wqkv, *bqkv, *wo, *fc1, *b1, *fc2, *b2; };
struct MsDecLayer { bf16_t *ln1, *ln2, *ln3, *sqkv, *sbqkv, *so, *cq, *cbq, *ckv, *cbkv, *co, *fc1, *b1, *fc2, *b2; };

struct mis_moonshine {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_moonshine_config cfg{};
    int d = 0, f = 0, V = 0, He = 0, Hke = 0, Hd = 0, Hkd = 0, hde = 0, hdd = 0, rote = 0, rotd = 0;
    HostWeights raw{"Moonshine"};
    bool finalized = false;
    DevBuf<bf16_t> arena;
    DevBuf<float> farena;
    float *conv1wT = nullptr, *gn_w = nullptr, *gn_b = nullptr, *cos_e = nullptr, *sin_e = nullptr, *cos_d = nullptr, *sin_d = nullptr;
    bf16_t *conv2w = nullptr, *conv2b = nullptr, *conv3w = nullptr, *conv3b = nullptr, *enc_ln = nullptr, *zeros = nullptr, *emb = nullptr,
           *proj = nullptr, *dec_norm = nullptr;
    std::vector<MsEncLayer> enc;
    std::vector<MsDecLayer> dec;
    // state of the last encode
    int batch = 0, T1pad = 0, T2pad = 0, T3pad = 0, T3max = 0, Smax = 0, pos = 0;
    std::vector<int> hT1, hT3;
    DevBuf<float> pcm, c1, gn_part0, gn_part1, gn_stats, logits;
    DevBuf<int> T1, T3;
    DevBuf<bf16_t> gn, c2, h, x, qkv, att, ff, enc_out, cross, self_k, self_v;
    DevBuf<bf16_t> dh, dqkv, dq, datt, dact;
    DevBuf<int32_t> ids, n_gen, tokens_out, done_count;
    DevBuf<uint8_t> active;
};

// ---------------------------------------------------------------------------- frame counts
static inline int ms_t1(int64_t n) { return n >= 127 ? (int)((n - 127) / 64 + 1) : 0; }
static inline int ms_t2(int t1) { return t1 >= 7 ? (t1 - 7) / 3 + 1 : 0; }
static inline int ms_t3(int t2) { return t2 >= 3 ? (t2 - 3) / 2 + 1 : 0; }

// rotaryDim (MoonshineModel.swift:142-144)
static int ms_rotary_dim(int head_dim, float factor) {
    int r = (int)((float)head_dim * factor);
    r -= r % 2;
    return std::max(2, r);
}

extern "C" mis_status mis_moonshine_frames(const mis_moonshine*, const int64_t* lens, int batch, int32_t* frames_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(lens && frames_out && batch >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    for (int b = 0; b < batch; ++b) frames_out[b] = ms_t3(ms_t2(ms_t1(lens[b])));
    MIS_API_END
}

extern "C" mis_status mis_moonshine_create(const mis_moonshine_config* cfg, int device, mis_moonshine** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    const int d = cfg->hidden_size;
    MIS_REQUIRE(d > 0 && d % 32 == 0 && d <= 512, MIS_ERR_INVALID_INPUT, "hidden_size %d unsupported (a multiple of 32, at most 512)", d);
    MIS_REQUIRE(cfg->intermediate_size > 0 && cfg->intermediate_size % 32 == 0, MIS_ERR_INVALID_INPUT, "intermediate_size must be a multiple of 32");
    MIS_REQUIRE(cfg->vocab_size > 0 && cfg->encoder_num_hidden_layers > 0 && cfg->decoder_num_hidden_layers > 0, MIS_ERR_INVALID_INPUT, "bad dims");
    const int He = cfg->encoder_num_attention_heads, Hd = cfg->decoder_num_attention_heads;
    const int Hke = cfg->encoder_num_key_value_heads, Hkd = cfg->decoder_num_key_value_heads;
    MIS_REQUIRE(He > 0 && Hd > 0 && d % He == 0 && d % Hd == 0, MIS_ERR_INVALID_INPUT, "bad head counts");
    MIS_REQUIRE(Hke > 0 && Hkd > 0 && He % Hke == 0 && Hd % Hkd == 0, MIS_ERR_INVALID_INPUT, "bad key/value head counts");
    MIS_REQUIRE(d / He <= MS_DP && d / Hd <= MS_DP && d / He >= 2 && d / Hd >= 2, MIS_ERR_INVALID_INPUT, "head_dim above %d unsupported", MS_DP);
    MIS_REQUIRE(cfg->encoder_hidden_act == 0, MIS_ERR_INVALID_INPUT, "encoder_hidden_act: only gelu is implemented");
    MIS_REQUIRE(cfg->partial_rotary_factor > 0.0f && cfg->partial_rotary_factor <= 1.0f && cfg->rope_theta > 0.0f, MIS_ERR_INVALID_INPUT, "bad rotary parameters");
    MIS_REQUIRE(cfg->decoder_start_token_id >= 0 && cfg->decoder_start_token_id < cfg->vocab_size, MIS_ERR_INVALID_INPUT, "decoder_start_token_id outside the vocabulary");
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_moonshine>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->d = d; c->f = cfg->intermediate_size; c->V = cfg->vocab_size;
    c->He = He; c->Hke = Hke; c->Hd = Hd; c->Hkd = Hkd; c->hde = d / He; c->hdd = d / Hd;
    c->rote = ms_rotary_dim(c->hde, cfg->partial_rotary_factor);
    c->rotd = ms_rotary_dim(c->hdd, cfg->partial_rotary_factor);
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_moonshine_destroy(mis_moonshine* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}

// checkpoint key -> the name the engine indexes by (MoonshineModel.sanitize, :443-459: "model." stripped); "" = ignored
static std::string ms_canonical_name(const mis_moonshine* c, const std::string& raw) {
    std::string name = raw;
    if (name.rfind("model.", 0) == 0) name = name.substr(6);
    if (name.rfind("proj_out.", 0) == 0 && c->cfg.tie_word_embeddings) return "";
    return name;
}

extern "C" mis_status mis_moonshine_set_tensor(mis_moonshine* c, const char* name_, const void* data, mis_dtype dtype, const int64_t* shape,
                                               int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name_, data, shape, ndim, 3, c && c->finalized, dtype);
    const std::string name = ms_canonical_name(c, name_);
    if (name.empty()) return MIS_OK;
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

extern "C" mis_status mis_moonshine_finalize(mis_moonshine* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t d = c->d, f = c->f, V = c->V;
    const bool ab = c->cfg.attention_bias != 0;
    HostArena a(c->raw);
    std::vector<bf16_t>& host = a.host;                 // the packers below write through these
    std::vector<float>& fhost = a.fhost;
    // projection rows [H hd][d] -> [H 64][d] at dst row0 (head h, column j -> row h 64 + j; the padding rows stay zero)
    auto pad_rows = [&](const std::string& name, int H, int hd, size_t off, int64_t row0) {
        const HostTensor& t = c->raw.need(name, {(int64_t)H * hd, d});
        for (int h = 0; h < H; ++h) for (int j = 0; j < hd; ++j) for (int64_t k = 0; k < d; ++k)
            host[off + (size_t)(row0 + h * MS_DP + j) * d + k] = f32_to_bf16(t.v[(size_t)(h * hd + j) * d + k]);
    };
    auto pad_bias = [&](const std::string& name, int H, int hd, size_t off, int64_t row0) {
        const HostTensor& t = c->raw.need(name, {(int64_t)H * hd});
        for (int h = 0; h < H; ++h) for (int j = 0; j < hd; ++j) host[off + row0 + h * MS_DP + j] = f32_to_bf16(t.v[h * hd + j]);
    };
    // o_proj [d][H hd] -> [d][H 64]
    auto pad_cols = [&](const std::string& name, int H, int hd, bf16_t*& dst) {
        const HostTensor& t = c->raw.need(name, {d, (int64_t)H * hd});
        size_t off = a.btake((size_t)d * H * MS_DP, dst);
        for (int64_t n = 0; n < d; ++n) for (int h = 0; h < H; ++h) for (int j = 0; j < hd; ++j)
            host[off + (size_t)n * H * MS_DP + h * MS_DP + j] = f32_to_bf16(t.v[(size_t)n * H * hd + h * hd + j]);
    };
    // conv weight [out][in][k] (published layout) -> [out][k in] (the order of a contiguous span of k frames)
    auto conv_w = [&](const std::string& name, int64_t O, int64_t I, int64_t K, bf16_t*& dst) {
        const HostTensor& t = c->raw.need(name, {O, I, K});
        size_t off = a.btake((size_t)O * I * K, dst);
        for (int64_t o = 0; o < O; ++o) for (int64_t k = 0; k < K; ++k) for (int64_t i = 0; i < I; ++i)
            host[off + ((size_t)o * K + k) * I + i] = f32_to_bf16(t.v[((size_t)o * I + i) * K + k]);
    };
    const std::string E = "encoder", D = "decoder";
    // ---- stem (f32 through GroupNorm)
    const HostTensor& w1 = c->raw.need(E + ".conv1.weight", {d, 1, 127});
    const size_t o_c1 = a.ftake((size_t)127 * d, c->conv1wT);
    for (int64_t ch = 0; ch < d; ++ch) for (int k = 0; k < 127; ++k) fhost[o_c1 + (size_t)k * d + ch] = w1.v[(size_t)ch * 127 + k];
    const size_t o_gw = a.ftake(d, c->gn_w), o_gb = a.ftake(d, c->gn_b);
    { const HostTensor& gw = c->raw.need(E + ".groupnorm.weight", {d}); const HostTensor& gb = c->raw.need(E + ".groupnorm.bias", {d});
      for (int64_t i = 0; i < d; ++i) { fhost[o_gw + i] = gw.v[i]; fhost[o_gb + i] = gb.v[i]; } }
    // rotary tables [MS_MAX_POS][rot / 2] (MoonshineRotaryEmbedding, :88-110)
    auto rope_tab = [&](int rot, float*& cos_t, float*& sin_t) {
        const size_t oc = a.ftake((size_t)MS_MAX_POS * (rot / 2), cos_t), os = a.ftake((size_t)MS_MAX_POS * (rot / 2), sin_t);
        for (int i = 0; i < rot / 2; ++i) {
            const float inv = 1.0f / powf(c->cfg.rope_theta, (float)(2 * i) / (float)rot);
            for (int p = 0; p < MS_MAX_POS; ++p) {
                const float a = (float)p * inv;
                fhost[oc + (size_t)p * (rot / 2) + i] = (float)cos((double)a);
                fhost[os + (size_t)p * (rot / 2) + i] = (float)sin((double)a);
            }
        }
    };
    rope_tab(c->rote, c->cos_e, c->sin_e);
    rope_tab(c->rotd, c->cos_d, c->sin_d);
    a.btake(std::max<int64_t>(d, 64), c->zeros);
    conv_w(E + ".conv2.weight", 2 * d, d, 7, c->conv2w); a.bvec(E + ".conv2.bias", 2 * d, c->conv2b);
    conv_w(E + ".conv3.weight", d, 2 * d, 3, c->conv3w); a.bvec(E + ".conv3.bias", d, c->conv3b);
    // fused q | k | v rows and their bias.  The bias buffer is taken whether or not the checkpoint has one (the arena's layout does
    // not depend on attention_bias); without one it stays zero and unbound: the pointer is nullptr
    auto qkv = [&](const std::string& p, const char* const* names, const int* heads, int n, int hd, bf16_t*& w, bf16_t*& b) {
        int64_t rows = 0;
        for (int i = 0; i < n; ++i) rows += (int64_t)heads[i] * MS_DP;
        const size_t ow = a.btake((size_t)rows * d, w), ob = ab ? a.btake(rows, b) : a.btake(rows);
        int64_t row0 = 0;
        for (int i = 0; i < n; row0 += (int64_t)heads[i++] * MS_DP) pad_rows(p + names[i] + ".weight", heads[i], hd, ow, row0);
        row0 = 0;
        for (int i = 0; ab && i < n; row0 += (int64_t)heads[i++] * MS_DP) pad_bias(p + names[i] + ".bias", heads[i], hd, ob, row0);
    };
    static const char* const QKV[3] = {".q_proj", ".k_proj", ".v_proj"};
    // ---- encoder layers
    c->enc.assign(c->cfg.encoder_num_hidden_layers, MsEncLayer{});
    for (size_t li = 0; li < c->enc.size(); ++li) {
        const std::string q = E + ".layers." + std::to_string(li);
        MsEncLayer& l = c->enc[li];
        a.bvec(q + ".input_layernorm.weight", d, l.ln1); a.bvec(q + ".post_attention_layernorm.weight", d, l.ln2);
        const int he[3] = {c->He, c->Hke, c->Hke};
        qkv(q + ".self_attn", QKV, he, 3, c->hde, l.wqkv, l.bqkv);
        pad_cols(q + ".self_attn.o_proj.weight", c->He, c->hde, l.wo);
        a.bmat(q + ".mlp.fc1.weight", f, d, l.fc1); a.bvec(q + ".mlp.fc1.bias", f, l.b1);
        a.bmat(q + ".mlp.fc2.weight", d, f, l.fc2); a.bvec(q + ".mlp.fc2.bias", d, l.b2);
    }
    a.bvec(E + ".layer_norm.weight", d, c->enc_ln);
    // ---- decoder; a tied proj is the embedding's offset bound a second time
    const size_t o_emb = a.bmat(D + ".embed_tokens.weight", V, d, c->emb);
    if (c->cfg.tie_word_embeddings) a.bind(c->proj, o_emb); else a.bmat("proj_out.weight", V, d, c->proj);
    c->dec.assign(c->cfg.decoder_num_hidden_layers, MsDecLayer{});
    for (size_t li = 0; li < c->dec.size(); ++li) {
        const std::string q = D + ".layers." + std::to_string(li);
        MsDecLayer& l = c->dec[li];
        a.bvec(q + ".input_layernorm.weight", d, l.ln1); a.bvec(q + ".post_attention_layernorm.weight", d, l.ln2);
        a.bvec(q + ".final_layernorm.weight", d, l.ln3);
        const int hd3[3] = {c->Hd, c->Hkd, c->Hkd};
        qkv(q + ".self_attn", QKV, hd3, 3, c->hdd, l.sqkv, l.sbqkv);
        pad_cols(q + ".self_attn.o_proj.weight", c->Hd, c->hdd, l.so);
        qkv(q + ".encoder_attn", QKV, hd3, 1, c->hdd, l.cq, l.cbq);
        qkv(q + ".encoder_attn", QKV + 1, hd3 + 1, 2, c->hdd, l.ckv, l.cbkv);
        pad_cols(q + ".encoder_attn.o_proj.weight", c->Hd, c->hdd, l.co);
        a.bmat(q + ".mlp.fc1.weight", 2 * f, d, l.fc1); a.bvec(q + ".mlp.fc1.bias", 2 * f, l.b1);
        a.bmat(q + ".mlp.fc2.weight", d, f, l.fc2); a.bvec(q + ".mlp.fc2.bias", d, l.b2);
    }
    a.bvec(D + ".norm.weight", d, c->dec_norm);
    // ---- upload: every pointer bound above now addresses the device arenas
    a.upload(c->arena, c->farena);
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every published key, amplitudes as the other engines' synthetic models
extern "C" mis_status mis_moonshine_init_synthetic(mis_moonshine* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    const int64_t d = c->d, f = c->f;
    auto attn = [&](const std::string& p, int H, int Hk, int hd) {
        const bool ab = c->cfg.attention_bias != 0;
        sw.lin(p + ".q_proj", (int64_t)H * hd, d, ab, 1.0); sw.lin(p + ".k_proj", (int64_t)Hk * hd, d, ab, 1.0);
        sw.lin(p + ".v_proj", (int64_t)Hk * hd, d, ab, 1.0); sw.lin(p + ".o_proj", d, (int64_t)H * hd, false, 0.5);
    };
    sw.put("encoder.conv1.weight", {d, 1, 127}, sqrt(3.0 / 127.0) * 4.0, 0.0f);
    sw.put("encoder.groupnorm.weight", {d}, 0.1, 1.0f); sw.put("encoder.groupnorm.bias", {d}, 0.05, 0.0f);
    sw.put("encoder.conv2.weight", {2 * d, d, 7}, sqrt(3.0 / (7.0 * d)), 0.0f); sw.put("encoder.conv2.bias", {2 * d}, 0.05, 0.0f);
    sw.put("encoder.conv3.weight", {d, 2 * d, 3}, sqrt(3.0 / (6.0 * d)), 0.0f); sw.put("encoder.conv3.bias", {d}, 0.05, 0.0f);
    for (int li = 0; li < c->cfg.encoder_num_hidden_layers; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li);
        attn(q + ".self_attn", c->He, c->Hke, c->hde);
        sw.put(q + ".input_layernorm.weight", {d}, 0.1, 1.0f); sw.put(q + ".post_attention_layernorm.weight", {d}, 0.1, 1.0f);
        sw.lin(q + ".mlp.fc1", f, d, true, 1.0); sw.lin(q + ".mlp.fc2", d, f, true, 0.5);
    }
    sw.put("encoder.layer_norm.weight", {d}, 0.1, 1.0f);
    sw.put("decoder.embed_tokens.weight", {(int64_t)c->V, d}, 0.5, 0.0f);
    for (int li = 0; li < c->cfg.decoder_num_hidden_layers; ++li) {
        const std::string q = "decoder.layers." + std::to_string(li);
        attn(q + ".self_attn", c->Hd, c->Hkd, c->hdd); attn(q + ".encoder_attn", c->Hd, c->Hkd, c->hdd);
        sw.put(q + ".input_layernorm.weight", {d}, 0.1, 1.0f); sw.put(q + ".post_attention_layernorm.weight", {d}, 0.1, 1.0f);
        sw.put(q + ".final_layernorm.weight", {d}, 0.1, 1.0f);
        sw.lin(q + ".mlp.fc1", 2 * f, d, true, 1.0); sw.lin(q + ".mlp.fc2", d, f, true, 0.5);
    }
    sw.put("decoder.norm.weight", {d}, 0.1, 1.0f);
    if (!c->cfg.tie_word_embeddings) sw.put("proj_out.weight", {(int64_t)c->V, d}, 0.5, 0.0f);
    MIS_API_END
}

// ============================================================================ stem kernels
// tanh(conv1d(1 -> d, k 127, stride 64, no bias)) (:309,321): a block is 16 frames of one row - their 16 * 64 + 63 samples sit in LDS
// once, a thread is a channel and reads its 127 taps once (weights transposed to [127][d]: coalesced) for all 16 frames.
__global__ void __launch_bounds__(256) k_ms_conv1_tanh(const float* __restrict__ pcm, int64_t stride, const int* __restrict__ T1,
                                                       const float* __restrict__ wT, float* __restrict__ out, int T1pad, int d) {
    __shared__ float xs[16 * 64 + 64];
    const int b = blockIdx.y, t0 = blockIdx.x * 16, n1 = T1[b];
    const int64_t extent = n1 > 0 ? (int64_t)(n1 - 1) * 64 + 127 : 0;         // samples the row's own frames read (<= lens[b])
    for (int i = threadIdx.x; i < 16 * 64 + 63; i += 256) {
        const int64_t s = (int64_t)t0 * 64 + i;
        xs[i] = s < extent ? pcm[(int64_t)b * stride + s] : 0.0f;
    }
    __syncthreads();
    for (int ch = threadIdx.x; ch < d; ch += 256) {
        float acc[16];
#pragma unroll
        for (int fidx = 0; fidx < 16; ++fidx) acc[fidx] = 0.0f;
        for (int k = 0; k < 127; ++k) {
            const float w = wT[(size_t)k * d + ch];
#pragma unroll
            for (int fidx = 0; fidx < 16; ++fidx) acc[fidx] = fmaf(w, xs[fidx * 64 + k], acc[fidx]);
        }
#pragma unroll
        for (int fidx = 0; fidx < 16; ++fidx) {
            const int t = t0 + fidx;
            if (t < T1pad) out[((size_t)b * T1pad + t) * d + ch] = t < n1 ? tanhf(acc[fidx]) : 0.0f;
        }
    }
}

static void ms_launch_conv1(const float* pcm, int64_t stride, const int* T1, const float* wT, float* out, int T1pad, int d, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_ms_conv1_tanh, dim3(cdiv(T1pad, 16), B), dim3(256), 0, s, pcm, stride, T1, wT, out, T1pad, d);
}

// GroupNorm(1 group) statistics over the row's own T1[b] * d values (:310,322; pytorchCompatible: biased variance).  Chunks of a fixed
// 32768 elements, so that a row's sums are formed in the same order whatever the batch it travels in; PASS 1 reads the mean as the
// ordered sum of the PASS 0 partials (chunks past the row's extent hold 0).
template <int PASS>
__global__ void __launch_bounds__(256) k_ms_gn_partial(const float* __restrict__ x, const int* __restrict__ T1, int T1pad, int d,
                                                       const float* __restrict__ sums, float* __restrict__ out, int nch) {
    __shared__ float red[4];
    const int b = blockIdx.y, ch = blockIdx.x;
    const size_t n = (size_t)T1[b] * d, lo = (size_t)ch * MS_GN_CHUNK, hi = lo + MS_GN_CHUNK < n ? lo + MS_GN_CHUNK : n;
    float mean = 0.0f;
    if (PASS == 1) {
        float s = 0.0f;
        for (int i = 0; i < nch; ++i) s += sums[b * nch + i];
        mean = s / (float)n;
    }
    const float* xr = x + (size_t)b * T1pad * d;
    float acc = 0.0f;
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) { const float v = xr[i] - mean; acc += PASS == 1 ? v * v : v; }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[b * nch + ch] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void k_ms_gn_final(const float* __restrict__ sums, const float* __restrict__ sq, const int* __restrict__ T1, int d, int nch,
                              float* __restrict__ stats, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float s = 0.0f, q = 0.0f;
    for (int i = 0; i < nch; ++i) { s += sums[b * nch + i]; q += sq[b * nch + i]; }
    const float n = (float)((size_t)T1[b] * d);
    stats[2 * b] = s / n;
    stats[2 * b + 1] = 1.0f / sqrtf(q / n + 1e-5f);
}
// y = T((x - mean) rstd gamma + beta) for t < T1[b], 0 behind it and in the tail the dense convs read past the last row
__global__ void __launch_bounds__(256) k_ms_gn_apply(const float* __restrict__ x, const int* __restrict__ T1, const float* __restrict__ stats,
                                                     const float* __restrict__ gw, const float* __restrict__ gb, bf16_t* __restrict__ y,
                                                     int T1pad, int d, int B, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / d;
    const int ch = (int)(i - row * d);
    const size_t b = row / T1pad;
    const int t = (int)(row - b * T1pad);
    bf16_t v = 0;
    if (b < (size_t)B && t < T1[b]) v = f32_to_bf16((x[i] - stats[2 * b]) * stats[2 * b + 1] * gw[ch] + gb[ch]);
    y[i] = v;
}

// the four GroupNorm launches: chunks of the longest row, PASS 0 / 1 partials [B][nch], the per-row statistics, the affine
static int ms_gn_chunks(int T1max, int d) { return cdiv((int64_t)T1max * d, MS_GN_CHUNK); }
static void ms_launch_gn_partial(int pass, const float* x, const int* T1, int T1pad, int d, const float* sums, float* out, int nch, int B, hipStream_t s) {
    if (pass == 0) hipLaunchKernelGGL((k_ms_gn_partial<0>), dim3(nch, B), dim3(256), 0, s, x, T1, T1pad, d, nullptr, out, nch);
    else hipLaunchKernelGGL((k_ms_gn_partial<1>), dim3(nch, B), dim3(256), 0, s, x, T1, T1pad, d, sums, out, nch);
}
static void ms_launch_gn_final(const float* sums, const float* sq, const int* T1, int d, int nch, float* stats, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_ms_gn_final, dim3(1), dim3(64), 0, s, sums, sq, T1, d, nch, stats, B);
}
// y holds B T1pad d elements and the tail of 8 d the dense convs read past the last row
static size_t ms_gn_tail(int d) { return (size_t)8 * d; }
static void ms_launch_gn_apply(const float* x, const int* T1, const float* stats, const float* gw, const float* gb, bf16_t* y, int T1pad, int d, int B,
                               hipStream_t s) {
    const size_t total = (size_t)B * T1pad * d + ms_gn_tail(d);
    hipLaunchKernelGGL(k_ms_gn_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, T1, stats, gw, gb, y, T1pad, d, B, total);
}

// ============================================================================ attention
// partial interleaved RoPE (:80-110,165-178): pairs (2i, 2i + 1) of the first `rot` columns of a head, T(x cos + rotate_half(x) sin)
__device__ __forceinline__ float ms_rope(float x, int lane, int rot, const float* __restrict__ cs, const float* __restrict__ sn, int pos) {
    const float partner = __shfl_xor(x, 1, 64);
    if (lane >= rot) return x;
    const float c = cs[(size_t)pos * (rot >> 1) + (lane >> 1)], s = sn[(size_t)pos * (rot >> 1) + (lane >> 1)];
    return bf16_round_f32(x * c + ((lane & 1) ? partner : -partner) * s);
}
// rows [M][ld]: heads 0 .. nheads - 1 of 64 columns from column 0 (q heads, then k heads) are rotated in place at position m % Tpad
__global__ void __launch_bounds__(256) k_ms_rope_rows(bf16_t* __restrict__ rows, int ld, int nheads, int Tpad, int rot,
                                                      const float* __restrict__ cs, const float* __restrict__ sn, size_t M) {
    const int lane = threadIdx.x & 63;
    const size_t item = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= M * nheads) return;
    const size_t m = item / nheads;
    const int h = (int)(item - m * nheads);
    bf16_t* p = rows + m * ld + h * MS_DP + lane;
    const float r = ms_rope(bf16_to_f32(*p), lane, rot, cs, sn, (int)(m % Tpad));
    if (lane < rot) *p = f32_to_bf16(r);
}

static void ms_launch_rope_rows(bf16_t* rows, int ld, int nheads, int Tpad, int rot, const float* cs, const float* sn, size_t M, hipStream_t s) {
    const size_t items = M * nheads;
    hipLaunchKernelGGL(k_ms_rope_rows, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, rows, ld, nheads, Tpad, rot, cs, sn, M);
}

// one query against n keys: q (f32, in LDS, 64 wide), K / V rows of 64 bf16 with row strides ldk / ldv.  A lane is a key in the score
// pass (the query is broadcast from LDS) and a column in the value pass; scores, softmax and the value sum in f32.  Returns the lane's
// output column.  `cur_*`: one more key held in registers behind the n cached ones (the decoder's new token), cur_s = its score.
__device__ __forceinline__ float ms_attend(const float* __restrict__ qs, float* __restrict__ sc, const bf16_t* __restrict__ K, size_t ldk,
                                           const bf16_t* __restrict__ Vv, size_t ldv, int n, float scale, int lane, bool has_cur, float cur_s,
                                           float cur_v) {
    float mx = has_cur ? cur_s : -INFINITY;
    for (int j = lane; j < n; j += 64) {
        const uint4* kr = reinterpret_cast<const uint4*>(K + (size_t)j * ldk);
        float dot = 0.0f;
#pragma unroll
        for (int c8 = 0; c8 < MS_DP / 8; ++c8) {
            const uint4 u = kr[c8];
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dot = fmaf(bf16_to_f32((bf16_t)(w[e] & 0xffffu)), qs[c8 * 8 + 2 * e], dot);
                dot = fmaf(bf16_to_f32((bf16_t)(w[e] >> 16)), qs[c8 * 8 + 2 * e + 1], dot);
            }
        }
        const float s = dot * scale;
        sc[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.0f;
    for (int j = lane; j < n; j += 64) { const float e = __expf(sc[j] - mx); sc[j] = e; sum += e; }
    sum = wave_sum(sum);
    __syncthreads();                                              // the wave's own probabilities, written by other lanes
    float acc = 0.0f;
    for (int j = 0; j < n; ++j) acc = fmaf(sc[j], bf16_to_f32(Vv[(size_t)j * ldv + lane]), acc);
    if (has_cur) { const float e = __expf(cur_s - mx); sum += e; acc = fmaf(e, cur_v, acc); }
    return acc / sum;
}

// encoder self-attention, non-causal over the row's own T3[b] keys (:181-194).  grid (ceil(Tpad / 4), H, B): a wave is one query.
__global__ void __launch_bounds__(256) k_ms_attn_enc(const bf16_t* __restrict__ qkv, int ld, int H, int Hkv, const int* __restrict__ T3,
                                                     int Tpad, float scale, bf16_t* __restrict__ out, int ldo) {
    __shared__ float sc[4][MS_MAX_KEYS];
    __shared__ float qs[4][MS_DP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y, hk = h / (H / Hkv);
    const int n = min(T3[b], MS_MAX_KEYS);
    const int t = min(blockIdx.x * 4 + wave, Tpad - 1);           // (a clamped wave repeats the last row's work: uniform barriers)
    const size_t row = (size_t)b * Tpad + t;
    qs[wave][lane] = bf16_to_f32(qkv[row * ld + h * MS_DP + lane]);
    __syncthreads();
    const bf16_t* K = qkv + (size_t)b * Tpad * ld + (size_t)(H + hk) * MS_DP;
    const bf16_t* Vv = qkv + (size_t)b * Tpad * ld + (size_t)(H + Hkv + hk) * MS_DP;
    const float o = ms_attend(qs[wave], sc[wave], K, ld, Vv, ld, n, scale, lane, false, 0.0f, 0.0f);
    if ((int)(blockIdx.x * 4 + wave) < Tpad) out[row * ldo + h * MS_DP + lane] = f32_to_bf16(t < n ? o : 0.0f);
}

// decoder self-attention of the token at position `pos` (causal, :155-194): RoPE on q and k, the new K / V rows appended to the caches
// [B][Hkv][Smax][64] by the first head of each group, attention over positions 0 .. pos.  grid (H, B), one wave.
__global__ void __launch_bounds__(64) k_ms_attn_self(const bf16_t* __restrict__ qkv, int H, int Hkv, bf16_t* __restrict__ kc,
                                                     bf16_t* __restrict__ vc, int Smax, int pos, int rot, const float* __restrict__ cs,
                                                     const float* __restrict__ sn, float scale, bf16_t* __restrict__ out) {
    __shared__ float sc[MS_MAX_POS];
    __shared__ float qs[MS_DP];
    const int lane = threadIdx.x, h = blockIdx.x, b = blockIdx.y, group = H / Hkv, hk = h / group;
    const size_t N = (size_t)(H + 2 * Hkv) * MS_DP;
    const float q = ms_rope(bf16_to_f32(qkv[b * N + h * MS_DP + lane]), lane, rot, cs, sn, pos);
    const float k = ms_rope(bf16_to_f32(qkv[b * N + (size_t)(H + hk) * MS_DP + lane]), lane, rot, cs, sn, pos);
    const float v = bf16_to_f32(qkv[b * N + (size_t)(H + Hkv + hk) * MS_DP + lane]);
    const size_t base = ((size_t)b * Hkv + hk) * Smax * MS_DP;
    if (h % group == 0) { kc[base + (size_t)pos * MS_DP + lane] = f32_to_bf16(k); vc[base + (size_t)pos * MS_DP + lane] = f32_to_bf16(v); }
    qs[lane] = q;
    const float cur_s = wave_sum(q * k) * scale;
    __syncthreads();
    const float o = ms_attend(qs, sc, kc + base, MS_DP, vc + base, MS_DP, pos, scale, lane, true, cur_s, v);
    out[(size_t)b * H * MS_DP + h * MS_DP + lane] = f32_to_bf16(o);
}

// decoder cross-attention over the row's cached encoder K / V (no RoPE, :165): kv rows [B Tpad][2 Hkv 64] (K heads, then V heads)
__global__ void __launch_bounds__(64) k_ms_attn_cross(const bf16_t* __restrict__ q, int H, int Hkv, const bf16_t* __restrict__ kv,
                                                      const int* __restrict__ T3, int Tpad, float scale, bf16_t* __restrict__ out) {
    __shared__ float sc[MS_MAX_KEYS];
    __shared__ float qs[MS_DP];
    const int lane = threadIdx.x, h = blockIdx.x, b = blockIdx.y, hk = h / (H / Hkv);
    const size_t ld = (size_t)2 * Hkv * MS_DP;
    qs[lane] = bf16_to_f32(q[(size_t)b * H * MS_DP + h * MS_DP + lane]);
    __syncthreads();
    const bf16_t* K = kv + (size_t)b * Tpad * ld + (size_t)hk * MS_DP;
    const bf16_t* Vv = kv + (size_t)b * Tpad * ld + (size_t)(Hkv + hk) * MS_DP;
    const float o = ms_attend(qs, sc, K, ld, Vv, ld, min(T3[b], MS_MAX_KEYS), scale, lane, false, 0.0f, 0.0f);
    out[(size_t)b * H * MS_DP + h * MS_DP + lane] = f32_to_bf16(o);
}

static void ms_launch_attn_enc(const bf16_t* qkv, int ld, int H, int Hkv, const int* T3, int Tpad, float scale, bf16_t* out, int ldo, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_ms_attn_enc, dim3(cdiv(Tpad, 4), H, B), dim3(256), 0, s, qkv, ld, H, Hkv, T3, Tpad, scale, out, ldo);
}
static void ms_launch_attn_self(const bf16_t* qkv, int H, int Hkv, bf16_t* kc, bf16_t* vc, int Smax, int pos, int rot, const float* cs, const float* sn,
                                float scale, bf16_t* out, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_ms_attn_self, dim3(H, B), dim3(64), 0, s, qkv, H, Hkv, kc, vc, Smax, pos, rot, cs, sn, scale, out);
}
static void ms_launch_attn_cross(const bf16_t* q, int H, int Hkv, const bf16_t* kv, const int* T3, int Tpad, float scale, bf16_t* out, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_ms_attn_cross, dim3(H, B), dim3(64), 0, s, q, H, Hkv, kv, T3, Tpad, scale, out);
}

// ============================================================================ decode-step GEMM
// out[b][n] = sum_k X[b][k] W[n][k] for B <= 64 rows: a wave is one output column (GATE: the pair n, n + F), lanes split K in pieces of
// four, eight rows at a time in registers.  LN: X = T(LayerNorm(h) w) (weight only, eps 1e-5, :247,286-288) rebuilt per block into LDS
// (K <= 512) - no separate LayerNorm launch.  Epilogues: MS_BF16 T(acc + bias); MS_RESID h = T(T(acc + bias) + h) in place (a column's
// rows are read and written by the same lane only); MS_GATE T(T(silu(g)) a) with a = T(rows n), g = T(rows n + F) (:223-227);
// MS_F32 the raw f32 sums (logits).
enum { MS_BF16 = 0, MS_RESID = 1, MS_GATE = 2, MS_F32 = 3 };
template <bool LN, int EPI>
__global__ void __launch_bounds__(256) k_ms_gemv(const bf16_t* __restrict__ X, int K, const bf16_t* __restrict__ lnw, const bf16_t* __restrict__ W,
                                                 const bf16_t* __restrict__ bias, void* __restrict__ out, int N, int B, int F) {
    extern __shared__ __attribute__((aligned(16))) bf16_t xn[];          // LN: [B][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (LN) {
        for (int r = wave; r < B; r += 4) {
            float s = 0.0f;
            for (int i = lane; i < K; i += 64) s += bf16_to_f32(X[(size_t)r * K + i]);
            const float mean = wave_sum(s) / (float)K;
            float q = 0.0f;
            for (int i = lane; i < K; i += 64) { const float t = bf16_to_f32(X[(size_t)r * K + i]) - mean; q += t * t; }
            const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)K + 1e-5f);
            for (int i = lane; i < K; i += 64)
                xn[(size_t)r * K + i] = f32_to_bf16((bf16_to_f32(X[(size_t)r * K + i]) - mean) * rstd * bf16_to_f32(lnw[i]));
        }
        __syncthreads();
    }
    const int n = blockIdx.x * 4 + wave;
    const int ncols = EPI == MS_GATE ? F : N;
    if (n >= ncols) return;
    const bf16_t* xsrc = LN ? xn : X;
    const int K4 = K >> 2;
    for (int r0 = 0; r0 < B; r0 += 8) {
        float acc[8], accg[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { acc[r] = 0.0f; accg[r] = 0.0f; }
        for (int k4 = lane; k4 < K4; k4 += 64) {
            const uint2 wu = *reinterpret_cast<const uint2*>(W + (size_t)n * K + k4 * 4);
            const float w0 = bf16_to_f32((bf16_t)(wu.x & 0xffffu)), w1 = bf16_to_f32((bf16_t)(wu.x >> 16)),
                        w2 = bf16_to_f32((bf16_t)(wu.y & 0xffffu)), w3 = bf16_to_f32((bf16_t)(wu.y >> 16));
            float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
            if (EPI == MS_GATE) {
                const uint2 gu = *reinterpret_cast<const uint2*>(W + (size_t)(n + F) * K + k4 * 4);
                g0 = bf16_to_f32((bf16_t)(gu.x & 0xffffu)); g1 = bf16_to_f32((bf16_t)(gu.x >> 16));
                g2 = bf16_to_f32((bf16_t)(gu.y & 0xffffu)); g3 = bf16_to_f32((bf16_t)(gu.y >> 16));
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = min(r0 + r, B - 1);
                const uint2 xu = *reinterpret_cast<const uint2*>(xsrc + (size_t)row * K + k4 * 4);
                const float x0 = bf16_to_f32((bf16_t)(xu.x & 0xffffu)), x1 = bf16_to_f32((bf16_t)(xu.x >> 16)),
                            x2 = bf16_to_f32((bf16_t)(xu.y & 0xffffu)), x3 = bf16_to_f32((bf16_t)(xu.y >> 16));
                acc[r] = fmaf(x3, w3, fmaf(x2, w2, fmaf(x1, w1, fmaf(x0, w0, acc[r]))));
                if (EPI == MS_GATE) accg[r] = fmaf(x3, g3, fmaf(x2, g2, fmaf(x1, g1, fmaf(x0, g0, accg[r]))));
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float a = wave_sum(acc[r]);
            const float g = EPI == MS_GATE ? wave_sum(accg[r]) : 0.0f;
            const int row = r0 + r;
            if (lane != 0 || row >= B) continue;
            if (EPI == MS_F32) { static_cast<float*>(out)[(size_t)row * N + n] = a; continue; }
            float v = bf16_round_f32(a + (bias ? bf16_to_f32(bias[n]) : 0.0f));
            bf16_t* o = static_cast<bf16_t*>(out);
            if (EPI == MS_RESID) v = bf16_round_f32(v + bf16_to_f32(o[(size_t)row * N + n]));
            if (EPI == MS_GATE) {
                const float gg = bf16_round_f32(g + (bias ? bf16_to_f32(bias[n + F]) : 0.0f));
                const float sg = bf16_round_f32(gg / (1.0f + __expf(-gg)));
                o[(size_t)row * F + n] = f32_to_bf16(sg * v);
                continue;
            }
            o[(size_t)row * N + n] = f32_to_bf16(v);
        }
    }
}
// returns the instantiation that ran: 4 LN + EPI
template <bool LN, int EPI>
static int ms_gemv(const bf16_t* X, int K, const bf16_t* lnw, const bf16_t* W, const bf16_t* bias, void* out, int N, int B, int F, hipStream_t s) {
    MIS_REQUIRE(K % 4 == 0 && B >= 1 && B <= MS_MAX_BATCH && (!LN || K <= 512), MIS_ERR_INVALID_INPUT, "decode GEMM: unsupported shape");
    const int ncols = EPI == MS_GATE ? F : N;
    hipLaunchKernelGGL((k_ms_gemv<LN, EPI>), dim3(cdiv(ncols, 4)), dim3(256), LN ? (size_t)B * K * 2 : 0, s, X, K, lnw, W, bias, out, N, B, F);
    return (LN ? 4 : 0) + EPI;
}

// h[b] = E[ids[b]] (:345)
__global__ void __launch_bounds__(256) k_ms_embed(const bf16_t* __restrict__ emb, const int32_t* __restrict__ ids, bf16_t* __restrict__ h,
                                                  int d, int vocab) {
    int id = ids[blockIdx.x];
    if (id < 0 || id >= vocab) id = 0;
    for (int i = threadIdx.x; i < d; i += 256) h[(size_t)blockIdx.x * d + i] = emb[(size_t)id * d + i];
}
// greedy step of generate (:388-398): arg-max (lowest id on ties); EOS ends the row and is not kept; otherwise the id is appended and
// becomes the next input, whose embedding is written here.  One block per row.
__global__ void __launch_bounds__(256) k_ms_argmax_embed(const float* __restrict__ logits, int V, int eos, uint8_t* __restrict__ active,
                                                         int32_t* __restrict__ n_gen, int32_t* __restrict__ tokens_out, int stride,
                                                         int32_t* __restrict__ done_count, const bf16_t* __restrict__ emb,
                                                         bf16_t* __restrict__ h, int d) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    __shared__ int chosen;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int i = threadIdx.x; i < V; i += 256) {
        const float v = logits[(size_t)b * V + i];
        if (v > best || (v == best && i < idx)) { best = v; idx = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
        if (idx < 0 || idx >= V) idx = 0;                             // (a row of NaNs: no comparison holds)
        if (active[b]) {
            if (idx == eos) { active[b] = 0; atomicAdd(done_count, 1); }
            else {
                const int g = n_gen[b];
                if (g < stride) tokens_out[(size_t)b * stride + g] = idx;
                n_gen[b] = g + 1;
            }
        }
        chosen = idx;
    }
    __syncthreads();
    const int id = chosen;
    for (int i = threadIdx.x; i < d; i += 256) h[(size_t)b * d + i] = emb[(size_t)id * d + i];
}

static void ms_launch_embed(const bf16_t* emb, const int32_t* ids, bf16_t* h, int d, int vocab, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_ms_embed, dim3(B), dim3(256), 0, s, emb, ids, h, d, vocab);
}
static void ms_launch_argmax_embed(const float* logits, int V, int eos, uint8_t* active, int32_t* n_gen, int32_t* tokens_out, int stride, int32_t* done_count,
                                   const bf16_t* emb, bf16_t* h, int d, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_ms_argmax_embed, dim3(B), dim3(256), 0, s, logits, V, eos, active, n_gen, tokens_out, stride, done_count, emb, h, d);
}

// ============================================================================ encoder pass
static void ms_check_lens(const mis_moonshine* c, const int64_t* lens, int batch, int64_t stride, std::vector<int64_t>* hl) {
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= MS_MAX_BATCH, MIS_ERR_INVALID_INPUT, "batch per GPU must be 1..%d", MS_MAX_BATCH);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    hl->assign(batch, stride);
    if (lens) memcpy(hl->data(), lens, batch * sizeof(int64_t));
    for (int b = 0; b < batch; ++b) {
        const int64_t n = (*hl)[b];
        MIS_REQUIRE(n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the row stride %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(ms_t3(ms_t2(ms_t1(n))) >= 1, MIS_ERR_INVALID_INPUT, "row %d: %lld samples give no encoder frame (at least 895 are needed)", b, (long long)n);
        MIS_REQUIRE(n <= MS_MAX_SAMPLES, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the per-row cap of %d (30 s at 16 kHz)", b, (long long)n,
                    MS_MAX_SAMPLES);
    }
}

static void ms_decoder_reset(mis_moonshine* c, int max_positions) {
    const int Smax = std::max(max_positions, 1);
    MIS_REQUIRE(Smax <= MS_MAX_POS, MIS_ERR_INVALID_INPUT, "at most %d decoder positions", MS_MAX_POS);
    const size_t n = (size_t)c->dec.size() * c->batch * c->Hkd * Smax * MS_DP;
    c->Smax = Smax; c->pos = 0;
    c->self_k.alloc(n); c->self_v.alloc(n);
    HIP_CHECK(hipMemsetAsync(c->self_k.p, 0, n * 2, c->stream));
    HIP_CHECK(hipMemsetAsync(c->self_v.p, 0, n * 2, c->stream));
    const int B = c->batch;
    c->dh.alloc((size_t)B * c->d); c->dqkv.alloc((size_t)B * (c->Hd + 2 * c->Hkd) * MS_DP); c->dq.alloc((size_t)B * c->Hd * MS_DP);
    c->datt.alloc((size_t)B * c->Hd * MS_DP); c->dact.alloc((size_t)B * c->f); c->logits.alloc((size_t)B * c->V);
    c->ids.alloc(B); c->n_gen.alloc(B); c->active.alloc(B); c->done_count.alloc(1);
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// pcm_dev f32 [B][stride]; stop_stage < 0: the whole encoder and the cross K / V of every decoder layer; 0..3: stop behind conv1 + tanh,
// GroupNorm, conv2, conv3 (the debug tap)
static void ms_encode_device(mis_moonshine* c, const float* pcm_dev, const std::vector<int64_t>& hl, int batch, int64_t stride, int stop_stage) {
    hipStream_t s = c->stream;
    const int d = c->d, f = c->f, B = batch;
    c->hT1.resize(B); c->hT3.resize(B);
    int T1max = 0, T3max = 0;
    for (int b = 0; b < B; ++b) {
        c->hT1[b] = ms_t1(hl[b]); c->hT3[b] = ms_t3(ms_t2(c->hT1[b]));
        T1max = std::max(T1max, c->hT1[b]); T3max = std::max(T3max, c->hT3[b]);
    }
    const int T1pad = (int)round_up(T1max, 6), T2pad = T1pad / 3, T3pad = T2pad / 2;
    MIS_REQUIRE(T3max <= MS_MAX_KEYS && T3pad >= T3max, MIS_ERR_GENERATION_FAILED, "frame layout");
    c->batch = B; c->T1pad = T1pad; c->T2pad = T2pad; c->T3pad = T3pad; c->T3max = T3max;
    c->T1.alloc(B); c->T3.alloc(B);
    HIP_CHECK(hipMemcpyAsync(c->T1.p, c->hT1.data(), B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->T3.p, c->hT3.data(), B * 4, hipMemcpyHostToDevice, s));
    // ---- stem
    const size_t n1 = (size_t)B * T1pad * d, tail = ms_gn_tail(d);
    c->c1.alloc(n1);
    ms_launch_conv1(pcm_dev, stride, c->T1.p, c->conv1wT, c->c1.p, T1pad, d, B, s);
    if (stop_stage == 0) { HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(s)); return; }
    const int nch = ms_gn_chunks(T1max, d);
    c->gn_part0.alloc((size_t)B * nch); c->gn_part1.alloc((size_t)B * nch); c->gn_stats.alloc(2 * B);
    ms_launch_gn_partial(0, c->c1.p, c->T1.p, T1pad, d, nullptr, c->gn_part0.p, nch, B, s);
    ms_launch_gn_partial(1, c->c1.p, c->T1.p, T1pad, d, c->gn_part0.p, c->gn_part1.p, nch, B, s);
    ms_launch_gn_final(c->gn_part0.p, c->gn_part1.p, c->T1.p, d, nch, c->gn_stats.p, B, s);
    c->gn.alloc(n1 + tail);
    ms_launch_gn_apply(c->c1.p, c->T1.p, c->gn_stats.p, c->gn_w, c->gn_b, c->gn.p, T1pad, d, B, s);
    if (stop_stage == 1) { HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(s)); return; }
    // gelu(conv2), gelu(conv3) (:311-312,323-324): frame t of row b is the span of k C_in values at stride C_in * (b Tpad + t)
    const int M2 = B * T2pad, M = B * T3pad;
    const size_t n2 = (size_t)M2 * 2 * d;
    c->c2.alloc(n2 + tail);
    HIP_CHECK(hipMemsetAsync(c->c2.p + n2, 0, tail * 2, s));
    BigGemmParams g{c->gn.p, c->conv2w, c->conv2b, nullptr, c->c2.p, M2, 2 * d, 7 * d, 3 * d, 0};
    launch_gemm_big(BG_GELU, g, s);
    if (stop_stage == 2) { HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(s)); return; }
    c->h.alloc((size_t)M * d);
    g = BigGemmParams{c->c2.p, c->conv3w, c->conv3b, nullptr, c->h.p, M, d, 6 * d, 4 * d, 0};
    launch_gemm_big(BG_GELU, g, s);
    if (stop_stage == 3) { HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(s)); return; }
    // ---- encoder layers (:230-256)
    const int NQ = (c->He + 2 * c->Hke) * MS_DP, NA = c->He * MS_DP;
    c->x.alloc((size_t)M * d); c->qkv.alloc((size_t)M * NQ); c->att.alloc((size_t)M * NA); c->ff.alloc((size_t)M * f);
    c->enc_out.alloc((size_t)M * d);
    const float scale_e = 1.0f / sqrtf((float)c->hde);
    for (const MsEncLayer& L : c->enc) {
        launch_layernorm(c->h.p, c->x.p, L.ln1, c->zeros, M, d, MS_EPS, s);
        g = BigGemmParams{c->x.p, L.wqkv, L.bqkv, nullptr, c->qkv.p, M, NQ, d, d, 0};
        launch_gemm_big(BG_NONE, g, s);
        ms_launch_rope_rows(c->qkv.p, NQ, c->He + c->Hke, T3pad, c->rote, c->cos_e, c->sin_e, (size_t)M, s);
        ms_launch_attn_enc(c->qkv.p, NQ, c->He, c->Hke, c->T3.p, T3pad, scale_e, c->att.p, NA, B, s);
        g = BigGemmParams{c->att.p, L.wo, nullptr, c->h.p, c->h.p, M, d, NA, NA, 0};
        launch_gemm_big(BG_RESID, g, s);
        launch_layernorm(c->h.p, c->x.p, L.ln2, c->zeros, M, d, MS_EPS, s);
        g = BigGemmParams{c->x.p, L.fc1, L.b1, nullptr, c->ff.p, M, f, d, d, 0};
        launch_gemm_big(BG_GELU, g, s);
        g = BigGemmParams{c->ff.p, L.fc2, L.b2, c->h.p, c->h.p, M, d, f, f, 0};
        launch_gemm_big(BG_RESID, g, s);
    }
    launch_layernorm(c->h.p, c->enc_out.p, c->enc_ln, c->zeros, M, d, MS_EPS, s);
    // cross-attention K / V of every decoder layer, once per request (:162-163 with encoderHiddenStates)
    const int NKV = 2 * c->Hkd * MS_DP;
    c->cross.alloc((size_t)c->dec.size() * M * NKV);
    for (size_t li = 0; li < c->dec.size(); ++li) {
        g = BigGemmParams{c->enc_out.p, c->dec[li].ckv, c->dec[li].cbkv, nullptr, c->cross.p + li * (size_t)M * NKV, M, NKV, d, d, 0};
        launch_gemm_big(BG_NONE, g, s);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    ms_decoder_reset(c, std::min(c->cfg.max_position_embeddings, MS_MAX_POS));
}

static void ms_upload_pcm(mis_moonshine* c, const float* pcm, int batch, int64_t stride) {
    c->pcm.alloc((size_t)batch * stride);
    HIP_CHECK(hipMemcpy(c->pcm.p, pcm, (size_t)batch * stride * 4, hipMemcpyDefault));
}

extern "C" mis_status mis_moonshine_encode(mis_moonshine* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* enc_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<int64_t> hl;
    ms_check_lens(c, lens, batch, stride, &hl);
    ms_upload_pcm(c, pcm, batch, stride);
    ms_encode_device(c, c->pcm.p, hl, batch, stride, -1);
    if (enc_out) {                                            // [B][T3max][d], zeros behind a row's own T3
        const size_t n = (size_t)batch * c->T3pad * c->d;
        DevBuf<float> o;
        o.alloc(n);
        launch_bf16_to_f32(c->enc_out.p, o.p, n, c->stream);
        std::vector<float> hostv(n);
        HIP_CHECK(hipMemcpyAsync(hostv.data(), o.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        memset(enc_out, 0, (size_t)batch * c->T3max * c->d * 4);
        for (int b = 0; b < batch; ++b)
            memcpy(enc_out + (size_t)b * c->T3max * c->d, hostv.data() + (size_t)b * c->T3pad * c->d, (size_t)c->hT3[b] * c->d * 4);
    }
    MIS_API_END
}

// tests: stem stage outputs, out f32 [batch, dims[0], dims[1]] (frames as laid out by the engine: the row's own frames first, zeros or
// padding-frame values behind them); out == NULL: dims only
extern "C" mis_status mis_debug_moonshine_stem_tap(mis_moonshine* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int stage,
                                                   float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && dims && stage >= 0 && stage <= 3, MIS_ERR_INVALID_INPUT, "bad argument");
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<int64_t> hl;
    ms_check_lens(c, lens, batch, stride, &hl);
    ms_upload_pcm(c, pcm, batch, stride);
    ms_encode_device(c, c->pcm.p, hl, batch, stride, stage);
    const int64_t T = stage <= 1 ? c->T1pad : stage == 2 ? c->T2pad : c->T3pad, C = stage == 2 ? 2 * c->d : c->d;
    dims[0] = T; dims[1] = C;
    if (out) {
        const size_t n = (size_t)batch * T * C;
        MIS_REQUIRE((int64_t)n <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
        if (stage == 0) HIP_CHECK(hipMemcpy(out, c->c1.p, n * 4, hipMemcpyDeviceToHost));
        else {
            DevBuf<float> o;
            o.alloc(n);
            const bf16_t* src = stage == 1 ? c->gn.p : stage == 2 ? c->c2.p : c->h.p;
            launch_bf16_to_f32(src, o.p, n, c->stream);
            HIP_CHECK(hipStreamSynchronize(c->stream));
            HIP_CHECK(hipMemcpy(out, o.p, n * 4, hipMemcpyDeviceToHost));
        }
    }
    c->batch = 0;                                             // no encoder output behind a tap: encode before decoding
    MIS_API_END
}

// ============================================================================ decoder step
// 8 launches per layer: [LN1 + q|k|v] [RoPE + append + self-attention] [o_proj + residual] [LN2 + cross q] [cross-attention]
// [o_proj + residual] [LN3 + fc1 + SiLU gate] [fc2 + residual]   (:258-297); a single chain on one stream
static int ms_launches_per_step(const mis_moonshine* c) { return 8 * (int)c->dec.size() + 2; }
static void ms_enqueue_layers(mis_moonshine* c, int pos) {
    hipStream_t s = c->stream;
    const int d = c->d, f = c->f, B = c->batch, H = c->Hd, Hk = c->Hkd, NQ = (H + 2 * Hk) * MS_DP, NA = H * MS_DP, NKV = 2 * Hk * MS_DP;
    const float scale = 1.0f / sqrtf((float)c->hdd);
    const size_t M = (size_t)B * c->T3pad, ls = (size_t)B * Hk * c->Smax * MS_DP;
    for (size_t li = 0; li < c->dec.size(); ++li) {
        const MsDecLayer& L = c->dec[li];
        ms_gemv<true, MS_BF16>(c->dh.p, d, L.ln1, L.sqkv, L.sbqkv, c->dqkv.p, NQ, B, 0, s);
        ms_launch_attn_self(c->dqkv.p, H, Hk, c->self_k.p + li * ls, c->self_v.p + li * ls, c->Smax, pos, c->rotd, c->cos_d, c->sin_d, scale, c->datt.p, B, s);
        ms_gemv<false, MS_RESID>(c->datt.p, NA, nullptr, L.so, nullptr, c->dh.p, d, B, 0, s);
        ms_gemv<true, MS_BF16>(c->dh.p, d, L.ln2, L.cq, L.cbq, c->dq.p, NA, B, 0, s);
        ms_launch_attn_cross(c->dq.p, H, Hk, c->cross.p + li * M * NKV, c->T3.p, c->T3pad, scale, c->datt.p, B, s);
        ms_gemv<false, MS_RESID>(c->datt.p, NA, nullptr, L.co, nullptr, c->dh.p, d, B, 0, s);
        ms_gemv<true, MS_GATE>(c->dh.p, d, L.ln3, L.fc1, L.b1, c->dact.p, 2 * f, B, f, s);
        ms_gemv<false, MS_RESID>(c->dact.p, f, nullptr, L.fc2, L.b2, c->dh.p, d, B, 0, s);
    }
    // logitsForHidden(norm(x)) (:349,427-432): the final LayerNorm in the prologue of the vocabulary projection
    ms_gemv<true, MS_F32>(c->dh.p, d, c->dec_norm, c->proj, nullptr, c->logits.p, c->V, B, 0, s);
}

extern "C" int mis_moonshine_launches_per_step(const mis_moonshine* c) { return c && c->finalized ? ms_launches_per_step(c) : 0; }

extern "C" mis_status mis_moonshine_decoder_reset(mis_moonshine* c, int max_positions) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && c->batch > 0, MIS_ERR_NOT_INITIALIZED, "encode first");
    HIP_CHECK(hipSetDevice(c->device));
    ms_decoder_reset(c, max_positions > 0 ? max_positions : std::min(c->cfg.max_position_embeddings, MS_MAX_POS));
    MIS_API_END
}

extern "C" mis_status mis_moonshine_decoder_forward(mis_moonshine* c, const int32_t* tokens, float* logits_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && tokens, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->batch > 0, MIS_ERR_NOT_INITIALIZED, "encode first");
    MIS_REQUIRE(c->pos < c->Smax, MIS_ERR_INVALID_INPUT, "decoder position %d beyond the %d the caches were reset for", c->pos, c->Smax);
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->ids.p, tokens, c->batch * 4, hipMemcpyDefault, s));
    ms_launch_embed(c->emb, c->ids.p, c->dh.p, c->d, c->V, c->batch, s);
    ms_enqueue_layers(c, c->pos);
    c->pos += 1;
    if (logits_out) HIP_CHECK(hipMemcpyAsync(logits_out, c->logits.p, (size_t)c->batch * c->V * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    MIS_API_END
}

// MoonshineModel.generate (:374-411) for a ragged batch: start token, arg-max per step, EOS ends a row and is not kept, at most
// max_tokens ids per row.  The reference recomputes the decoder over all tokens each step; the caches make that the same arithmetic.
extern "C" mis_status mis_stt_moonshine_generate(mis_moonshine* c, const float* pcm, const int64_t* lens, int batch, int64_t stride,
                                                 const mis_stt_params* sp, int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && sp && tokens_out && tokens_stride && n_tokens, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(!(sp->temperature > 0.0f), MIS_ERR_INVALID_INPUT, "Moonshine: temperature > 0 (categorical sampling) is not implemented; use temperature 0");
    const int max_tokens = sp->max_tokens > 0 ? sp->max_tokens : 200;
    MIS_REQUIRE(max_tokens + 1 <= MS_MAX_POS, MIS_ERR_INVALID_INPUT, "max_tokens above %d", MS_MAX_POS - 1);
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<int64_t> hl;
    ms_check_lens(c, lens, batch, stride, &hl);
    ms_upload_pcm(c, pcm, batch, stride);
    ms_encode_device(c, c->pcm.p, hl, batch, stride, -1);
    ms_decoder_reset(c, max_tokens);
    hipStream_t s = c->stream;
    c->tokens_out.alloc((size_t)batch * max_tokens);
    c->tokens_out.zero(s); c->n_gen.zero(s); c->done_count.zero(s);
    HIP_CHECK(hipMemsetAsync(c->active.p, 1, batch, s));
    std::vector<int32_t> start(batch, c->cfg.decoder_start_token_id);
    HIP_CHECK(hipMemcpyAsync(c->ids.p, start.data(), batch * 4, hipMemcpyHostToDevice, s));
    ms_launch_embed(c->emb, c->ids.p, c->dh.p, c->d, c->V, batch, s);
    PinnedBuf<int32_t> done(1);
    *done.p = 0;
    for (int step = 0; step < max_tokens; ++step) {
        ms_enqueue_layers(c, step);
        ms_launch_argmax_embed(c->logits.p, c->V, c->cfg.eos_token_id, c->active.p, c->n_gen.p, c->tokens_out.p, max_tokens, c->done_count.p, c->emb,
                               c->dh.p, c->d, batch, s);
        if ((step & 7) == 7 || step + 1 == max_tokens) {          // the EOS check the loop needs, every 8 steps
            HIP_CHECK(hipMemcpyAsync(done.p, c->done_count.p, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            if (*done.p >= batch) break;
        }
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    PinnedBuf<int32_t> th((size_t)batch * max_tokens + 1);
    HIP_CHECK(hipMemcpy(th.p, c->tokens_out.p, (size_t)batch * max_tokens * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(n_tokens, c->n_gen.p, batch * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b) n_tokens[b] = std::min(n_tokens[b], max_tokens);
    *tokens_out = th.release();
    *tokens_stride = max_tokens;
    MIS_API_END
}

// ============================================================================ test scaffolding (include/mi_speech_debug.h)
// ONE launch of a private kernel above (GroupNorm: its chain of four), through the launcher the engine calls, on caller-supplied host
// data, so that tests/test_gpu_moonshine_ops.py can hold the kernels to an operator-level reference.  Nothing is computed here: the
// operands are uploaded as given and what the launch wrote is copied back.  Guards as the other operator entry points (debug_guard.h):
// every output is [guard | body | guard], all of it the byte 0xFF before the launch (an output that also goes IN - the rotated rows, the
// caches, the in-place residual, the token bookkeeping - holds the caller's data instead); a changed guard byte or padding column fails
// the call; every input is followed by IN_GUARD NaNs (ints: 0x7FFFFFFF).  The entry points refuse what the kernels' contract excludes
// (MIS_ERR_INVALID_INPUT, nothing launched).  The launches run on the null stream.
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

namespace {

constexpr int64_t MSD_MAX_ELEMS = (int64_t)1 << 28;          // per tensor

void msd_sync() {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
}
const int* msd_int(const DevBuf<uint32_t>& d) { return reinterpret_cast<const int*>(d.p); }
const float* msd_f32(const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); }
void msd_fetch(GuardedOut& o, void* out) {
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
}
// an output that also goes in
void msd_inout(GuardedOut& o, const void* src, size_t bytes, size_t guard_bytes) {
    o.alloc(bytes, guard_bytes);
    HIP_CHECK(hipMemcpy(o.p(), src, bytes, hipMemcpyHostToDevice));
}
// rows of ld with `cols` live columns -> the live columns; the columns behind must still hold the fill
void msd_fetch16_rows(GuardedOut& o, size_t rows, size_t ld, size_t cols, uint16_t* out) {
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

extern "C" mis_status mis_debug_moonshine_conv1(int device, const float* pcm, int64_t stride, const int32_t* T1, int B, int T1pad, int d, const float* wT,
                                                float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(pcm && T1 && wT && out && B >= 1 && B <= 65535 && T1pad >= 1 && d >= 1 && stride >= 1, MIS_ERR_INVALID_INPUT,
                "Moonshine conv1: every pointer and positive B, T1pad, d, stride are required");
    MIS_REQUIRE((int64_t)B * stride <= MSD_MAX_ELEMS && (int64_t)B * T1pad * d <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Moonshine conv1: tensor too large");
    for (int b = 0; b < B; ++b)
        MIS_REQUIRE(T1[b] >= 0 && T1[b] <= T1pad && (T1[b] == 0 || (int64_t)(T1[b] - 1) * 64 + 127 <= stride), MIS_ERR_INVALID_INPUT,
                    "Moonshine conv1: row %d: %d frames outside 0..T1pad or reading behind the row's %lld samples", b, T1[b], (long long)stride);
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> dp, dw, dT;
    alloc32(dp, pcm, (size_t)B * stride, F32_NAN);
    alloc32(dw, wT, (size_t)127 * d, F32_NAN);
    alloc32(dT, T1, B, 0x7FFFFFFFu);
    GuardedOut o;
    o.alloc((size_t)B * T1pad * d * 4, (size_t)16 * d * 4);
    ms_launch_conv1(msd_f32(dp), stride, msd_int(dT), msd_f32(dw), reinterpret_cast<float*>(o.p()), T1pad, d, B, nullptr);
    msd_sync();
    msd_fetch(o, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_moonshine_groupnorm(int device, const float* x, const int32_t* T1, int B, int T1pad, int d, const float* gw, const float* gb,
                                                    int stage, float* part0, float* part1, float* stats, uint16_t* y, int32_t* nch_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && T1 && gw && gb && nch_out && B >= 1 && B <= MS_MAX_BATCH && T1pad >= 1 && d >= 1 && stage >= 0 && stage <= 2, MIS_ERR_INVALID_INPUT,
                "Moonshine GroupNorm: x, T1, gw, gb, nch_out, 1 <= B <= 64, positive T1pad, d and stage 0..2 are required");
    MIS_REQUIRE(part0 && (stage < 1 || part1) && (stage < 2 || (stats && y)), MIS_ERR_INVALID_INPUT, "Moonshine GroupNorm: the stage's outputs are required");
    MIS_REQUIRE((int64_t)B * T1pad * d + 8 * (int64_t)d <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Moonshine GroupNorm: tensor too large");
    int T1max = 0;
    for (int b = 0; b < B; ++b) {
        MIS_REQUIRE(T1[b] >= 1 && T1[b] <= T1pad, MIS_ERR_INVALID_INPUT, "Moonshine GroupNorm: row %d: %d frames outside 1..T1pad", b, T1[b]);
        T1max = std::max(T1max, T1[b]);
    }
    HIP_CHECK(hipSetDevice(device));
    const size_t n1 = (size_t)B * T1pad * d;
    const int nch = ms_gn_chunks(T1max, d);
    *nch_out = nch;
    DevBuf<uint32_t> dx, dT, dgw, dgb;
    {   // frames behind a row's own count: NaN
        std::vector<float> h(x, x + n1);
        for (int b = 0; b < B; ++b)
            for (size_t i = ((size_t)b * T1pad + T1[b]) * d; i < (size_t)(b + 1) * T1pad * d; ++i) memcpy(&h[i], &F32_NAN, 4);
        alloc32(dx, h.data(), n1, F32_NAN);
    }
    alloc32(dT, T1, B, 0x7FFFFFFFu);
    alloc32(dgw, gw, d, F32_NAN);
    alloc32(dgb, gb, d, F32_NAN);
    GuardedOut p0, p1, st, o;
    p0.alloc((size_t)B * nch * 4, 256);                            // only what the stage launches into
    if (stage >= 1) p1.alloc((size_t)B * nch * 4, 256);
    if (stage >= 2) { st.alloc((size_t)2 * B * 4, 256); o.alloc((n1 + ms_gn_tail(d)) * 2, (size_t)4 * d * 2); }
    float *f0 = reinterpret_cast<float*>(p0.p()), *f1 = reinterpret_cast<float*>(p1.p());
    ms_launch_gn_partial(0, msd_f32(dx), msd_int(dT), T1pad, d, nullptr, f0, nch, B, nullptr);
    if (stage >= 1) ms_launch_gn_partial(1, msd_f32(dx), msd_int(dT), T1pad, d, f0, f1, nch, B, nullptr);
    if (stage >= 2) {
        float* fs = reinterpret_cast<float*>(st.p());
        ms_launch_gn_final(f0, f1, msd_int(dT), d, nch, fs, B, nullptr);
        ms_launch_gn_apply(msd_f32(dx), msd_int(dT), fs, msd_f32(dgw), msd_f32(dgb), reinterpret_cast<bf16_t*>(o.p()), T1pad, d, B, nullptr);
    }
    msd_sync();
    msd_fetch(p0, part0);
    if (stage >= 1) msd_fetch(p1, part1);
    if (stage >= 2) { msd_fetch(st, stats); msd_fetch(o, y); }
    MIS_API_END
}

extern "C" mis_status mis_debug_moonshine_rope(int device, uint16_t* rows, int M, int ld, int nheads, int Tpad, int rot, const float* cs, const float* sn) {
    MIS_API_BEGIN
    MIS_REQUIRE(rows && cs && sn && M >= 1 && nheads >= 1 && Tpad >= 1 && (int64_t)nheads * MS_DP <= ld, MIS_ERR_INVALID_INPUT,
                "Moonshine RoPE: rows, both tables, M, Tpad >= 1 and 1 <= nheads <= ld / 64 are required");
    MIS_REQUIRE(rot >= 2 && rot <= MS_DP && rot % 2 == 0, MIS_ERR_INVALID_INPUT, "Moonshine RoPE: rot %d is not an even number in 2..64", rot);
    MIS_REQUIRE((int64_t)M * ld <= MSD_MAX_ELEMS && (int64_t)Tpad * (rot / 2) <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Moonshine RoPE: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> dc, ds;
    alloc32(dc, cs, (size_t)Tpad * (rot / 2), F32_NAN);
    alloc32(ds, sn, (size_t)Tpad * (rot / 2), F32_NAN);
    GuardedOut r;
    msd_inout(r, rows, (size_t)M * ld * 2, (size_t)4 * ld * 2);
    ms_launch_rope_rows(reinterpret_cast<bf16_t*>(r.p()), ld, nheads, Tpad, rot, msd_f32(dc), msd_f32(ds), (size_t)M, nullptr);
    msd_sync();
    msd_fetch(r, rows);
    MIS_API_END
}

extern "C" mis_status mis_debug_moonshine_attn(int device, int kind, const uint16_t* q, const uint16_t* kv, int ld, int H, int Hkv, const int32_t* T3, int B,
                                               int Tpad, float scale, int ldo, uint16_t* kc, uint16_t* vc, int Smax, int pos, int rot, const float* cs,
                                               const float* sn, uint16_t* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(kind >= 0 && kind <= 2 && q && out && B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && Hkv >= 1, MIS_ERR_INVALID_INPUT,
                "Moonshine attention: kind 0..2, q, out and positive B, H, Hkv are required");
    MIS_REQUIRE(H % Hkv == 0, MIS_ERR_INVALID_INPUT, "Moonshine attention: %d kv heads do not divide %d heads", Hkv, H);
    const size_t NA = (size_t)H * MS_DP, NQ = (size_t)(H + 2 * Hkv) * MS_DP, NKV = (size_t)2 * Hkv * MS_DP;
    if (kind != 1) {
        MIS_REQUIRE(T3 && Tpad >= 1 && (int64_t)B * Tpad * std::max<int64_t>(ld, NKV) <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                    "Moonshine attention: T3 and Tpad >= 1 are required (or the tensor is too large)");
        for (int b = 0; b < B; ++b)
            MIS_REQUIRE(T3[b] >= (kind == 2 ? 1 : 0) && T3[b] <= MS_MAX_KEYS && T3[b] <= Tpad, MIS_ERR_INVALID_INPUT,
                        "Moonshine attention: row %d: %d keys outside %d..min(Tpad, %d)", b, T3[b], kind == 2 ? 1 : 0, MS_MAX_KEYS);
    }
    if (kind == 0)
        MIS_REQUIRE(ld % 8 == 0 && (int64_t)NQ <= ld && (int64_t)NA <= ldo && (int64_t)B * Tpad * ldo <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                    "Moonshine encoder attention: ld >= (H + 2 Hkv) 64 in 16-byte rows, ldo >= H 64");
    if (kind == 2) MIS_REQUIRE(kv, MIS_ERR_INVALID_INPUT, "Moonshine cross-attention: kv is required");
    if (kind == 1) {
        MIS_REQUIRE(kc && vc && cs && sn && Smax >= 1 && Smax <= MS_MAX_POS && pos >= 0 && pos < Smax, MIS_ERR_INVALID_INPUT,
                    "Moonshine self-attention: both caches and tables, 1 <= Smax <= %d and 0 <= pos < Smax are required", MS_MAX_POS);
        MIS_REQUIRE(rot >= 2 && rot <= MS_DP && rot % 2 == 0, MIS_ERR_INVALID_INPUT, "Moonshine self-attention: rot %d is not an even number in 2..64", rot);
        MIS_REQUIRE((int64_t)B * Hkv * Smax * MS_DP <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Moonshine self-attention: tensor too large");
    }
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> dq, dkv;
    DevBuf<uint32_t> dT, dc, ds;
    GuardedOut o;
    bf16_t* op = nullptr;
    if (kind == 0) {
        const size_t rows = (size_t)B * Tpad;
        alloc16(dq, q, rows * ld, BF16_NAN);
        alloc32(dT, T3, B, 0x7FFFFFFFu);
        o.alloc(rows * ldo * 2, (size_t)4 * ldo * 2);
        op = reinterpret_cast<bf16_t*>(o.p());
        ms_launch_attn_enc(dq.p, ld, H, Hkv, msd_int(dT), Tpad, scale, op, ldo, B, nullptr);
        msd_sync();
        msd_fetch16_rows(o, rows, ldo, NA, out);
    } else if (kind == 2) {
        alloc16(dq, q, (size_t)B * NA, BF16_NAN);
        alloc16(dkv, kv, (size_t)B * Tpad * NKV, BF16_NAN);
        alloc32(dT, T3, B, 0x7FFFFFFFu);
        o.alloc((size_t)B * NA * 2, NA * 2);
        op = reinterpret_cast<bf16_t*>(o.p());
        ms_launch_attn_cross(dq.p, H, Hkv, dkv.p, msd_int(dT), Tpad, scale, op, B, nullptr);
        msd_sync();
        msd_fetch(o, out);
    } else {
        const size_t nc = (size_t)B * Hkv * Smax * MS_DP;
        alloc16(dq, q, (size_t)B * NQ, BF16_NAN);
        alloc32(dc, cs, (size_t)Smax * (rot / 2), F32_NAN);
        alloc32(ds, sn, (size_t)Smax * (rot / 2), F32_NAN);
        GuardedOut gk, gv;
        msd_inout(gk, kc, nc * 2, (size_t)Smax * MS_DP * 2);
        msd_inout(gv, vc, nc * 2, (size_t)Smax * MS_DP * 2);
        o.alloc((size_t)B * NA * 2, NA * 2);
        op = reinterpret_cast<bf16_t*>(o.p());
        ms_launch_attn_self(dq.p, H, Hkv, reinterpret_cast<bf16_t*>(gk.p()), reinterpret_cast<bf16_t*>(gv.p()), Smax, pos, rot, msd_f32(dc), msd_f32(ds), scale,
                            op, B, nullptr);
        msd_sync();
        msd_fetch(o, out);
        msd_fetch(gk, kc);
        msd_fetch(gv, vc);
    }
    MIS_API_END
}

extern "C" mis_status mis_debug_moonshine_gemv(int device, int ln, int epi, const uint16_t* X, const uint16_t* lnw, const uint16_t* W, const uint16_t* bias,
                                               int B, int K, int N, int F, void* out, int32_t* report) {
    MIS_API_BEGIN
    if (report) { report[0] = -1; report[1] = -1; }
    MIS_REQUIRE(X && W && out && B >= 1 && K >= 1 && N >= 1 && (ln == 0 || ln == 1) && (!ln || lnw), MIS_ERR_INVALID_INPUT,
                "Moonshine decode GEMM: X, W, out, positive B, K, N and ln 0 / 1 (with lnw) are required");
    MIS_REQUIRE(K % 4 == 0 && B <= MS_MAX_BATCH && (!ln || K <= 512), MIS_ERR_INVALID_INPUT,
                "Moonshine decode GEMM: K %% 4, B <= %d and K <= 512 under LayerNorm are the kernel's contract", MS_MAX_BATCH);
    const int inst = 4 * ln + epi;
    MIS_REQUIRE(inst == 4 + MS_BF16 || inst == MS_RESID || inst == 4 + MS_GATE || inst == 4 + MS_F32, MIS_ERR_INVALID_INPUT,
                "Moonshine decode GEMM: (ln %d, epi %d) is not one of the decoder's four instantiations", ln, epi);
    MIS_REQUIRE(epi != MS_GATE || (F >= 1 && N == 2 * F), MIS_ERR_INVALID_INPUT, "Moonshine decode GEMM: the gate epilogue needs N == 2 F");
    MIS_REQUIRE((int64_t)N * K <= MSD_MAX_ELEMS && (int64_t)B * N <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Moonshine decode GEMM: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> dX, dl, dW, db;
    alloc16(dX, X, (size_t)B * K, BF16_NAN);
    if (ln) alloc16(dl, lnw, K, BF16_NAN);
    alloc16(dW, W, (size_t)N * K, BF16_NAN);
    if (bias) alloc16(db, bias, N, BF16_NAN);
    const size_t cols = epi == MS_GATE ? F : N, es = epi == MS_F32 ? 4 : 2;
    GuardedOut o;
    if (epi == MS_RESID) msd_inout(o, out, (size_t)B * cols * es, (size_t)8 * cols * es);          // a guard is one eight-row register group
    else o.alloc((size_t)B * cols * es, (size_t)8 * cols * es);
    const bf16_t *lp = ln ? dl.p : nullptr, *bp = bias ? db.p : nullptr;
    int ran = -1;
    if (inst == 4 + MS_BF16) ran = ms_gemv<true, MS_BF16>(dX.p, K, lp, dW.p, bp, o.p(), N, B, F, nullptr);
    else if (inst == MS_RESID) ran = ms_gemv<false, MS_RESID>(dX.p, K, lp, dW.p, bp, o.p(), N, B, F, nullptr);
    else if (inst == 4 + MS_GATE) ran = ms_gemv<true, MS_GATE>(dX.p, K, lp, dW.p, bp, o.p(), N, B, F, nullptr);
    else ran = ms_gemv<true, MS_F32>(dX.p, K, lp, dW.p, bp, o.p(), N, B, F, nullptr);
    msd_sync();
    if (report) { report[0] = ran / 4; report[1] = ran % 4; }
    msd_fetch(o, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_moonshine_embed(int device, const uint16_t* emb, const int32_t* ids, int B, int d, int vocab, uint16_t* h) {
    MIS_API_BEGIN
    MIS_REQUIRE(emb && ids && h && B >= 1 && d >= 1 && vocab >= 1 && (int64_t)vocab * d <= MSD_MAX_ELEMS && (int64_t)B * d <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Moonshine embed: emb, ids, h and positive B, d, vocab are required");
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint16_t> de;
    DevBuf<uint32_t> di;
    alloc16(de, emb, (size_t)vocab * d, BF16_NAN);
    alloc32(di, ids, B, 0x7FFFFFFFu);
    GuardedOut o;
    o.alloc((size_t)B * d * 2, (size_t)d * 2);
    ms_launch_embed(de.p, msd_int(di), reinterpret_cast<bf16_t*>(o.p()), d, vocab, B, nullptr);
    msd_sync();
    msd_fetch(o, h);
    MIS_API_END
}

extern "C" mis_status mis_debug_moonshine_argmax_embed(int device, const float* logits, int B, int V, int eos, uint8_t* active, int32_t* n_gen, int32_t* tokens,
                                                       int stride, int32_t* done_count, const uint16_t* emb, int d, uint16_t* h) {
    MIS_API_BEGIN
    MIS_REQUIRE(logits && active && n_gen && tokens && done_count && emb && h && B >= 1 && V >= 1 && stride >= 1 && d >= 1, MIS_ERR_INVALID_INPUT,
                "Moonshine arg-max + embed: every pointer and positive B, V, stride, d are required");
    MIS_REQUIRE((int64_t)B * V <= MSD_MAX_ELEMS && (int64_t)V * d <= MSD_MAX_ELEMS && (int64_t)B * stride <= MSD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Moonshine arg-max + embed: tensor too large");
    for (int b = 0; b < B; ++b) MIS_REQUIRE(n_gen[b] >= 0, MIS_ERR_INVALID_INPUT, "Moonshine arg-max + embed: row %d: negative token count", b);
    HIP_CHECK(hipSetDevice(device));
    DevBuf<uint32_t> dl;
    DevBuf<uint16_t> de;
    alloc32(dl, logits, (size_t)B * V, F32_NAN);
    alloc16(de, emb, (size_t)V * d, BF16_NAN);
    GuardedOut ga, gn, gt, gd, o;
    msd_inout(ga, active, B, 256);
    msd_inout(gn, n_gen, (size_t)B * 4, 256);
    msd_inout(gt, tokens, (size_t)B * stride * 4, (size_t)stride * 4);
    msd_inout(gd, done_count, 4, 256);
    o.alloc((size_t)B * d * 2, (size_t)d * 2);
    ms_launch_argmax_embed(msd_f32(dl), V, eos, ga.p(), reinterpret_cast<int32_t*>(gn.p()), reinterpret_cast<int32_t*>(gt.p()), stride,
                           reinterpret_cast<int32_t*>(gd.p()), de.p, reinterpret_cast<bf16_t*>(o.p()), d, B, nullptr);
    msd_sync();
    msd_fetch(ga, active);
    msd_fetch(gn, n_gen);
    msd_fetch(gt, tokens);
    msd_fetch(gd, done_count);
    msd_fetch(o, h);
    MIS_API_END
}
