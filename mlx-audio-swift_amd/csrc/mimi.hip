// mimi.hip - Mimi codec (Kyutai, 12.5 Hz codes <-> 24 kHz mono), float32: decoder (whole sequence and per-frame streaming) and the
// handle around the shared tokenizer encoder of q3_reference.hip.
//
// Reference being replaced: Mimi.decode (Sources/MLXAudioCodecs/Mimi/Mimi.swift:178-186) = SplitResidualVectorQuantizer.decode
// (Quantization.swift:49-52,113-120,161-166,203-210) -> ConvTrUpsample1d (Conv.swift:349-362: depthwise transposed conv k = 2s,
// stride s, no bias, causal right trim) -> decoder ProjectedTransformer (Transformer.swift:110-314: pre-LayerNorm, fused in_proj,
// interleaved RoPE, causal SDPA, layer scale, GELU MLP) -> SeanetDecoder (Seanet.swift:259-356: conv k7, per ratio ELU + causal
// transposed conv k = 2r + SeanetResnetBlock(ELU, conv k3 -> dim/2, ELU, conv k1, identity skip), ELU, conv k3 -> 1, no clip);
// MimiStreamingDecoder.decodeFrames (:207-232) = decodeStep (:196-204) once per frame.  Mimi.encode (:168-176) runs the encoder
// program of q3_reference.hip (keys without the Qwen3-TTS "encoder_model." prefix) one row at a time.
//
// The decoder follows q3_codec.hip: activations NCT ([B][C][T], time contiguous), every contraction on launch_gemm (split-bf16 where the
// shape pays, exact-f32 MFMA otherwise), the transformer on k_q3_norm_ct / k_q3_attn with the q / k rows of every head permuted
// evens-then-odds (interleaved RoPE == rotate-half RoPE on the permuted rows).  ELU is a staging pass (k_mimi_elu) in front of the conv
// that consumes it: the operand prologues of the shared GEMMs stay exactly as they are.
// Streaming: work buffers carry MIMI_HP columns of head room in front of every row; launch_codec_hist carries drop the last (k-1)*d
// inputs of every causal conv and the last input column of every transposed conv there (StreamableConvTranspose1d.step subtracts the
// bias from its carried tail, Conv.swift:316, so the overlap-add is exact and nothing is added twice).  The transformer keeps K/V in a
// per-layer ring; a step's queries see keys [max(0, s*f - context), p] (the cache trim of Transformer.swift:155-166 under MLX's
// bottom-right causal mask), RoPE at the absolute position.  Every output column runs the same instruction sequence in both modes, so
// the stream is bitwise equal to whole decode while the window holds every key (frames 0 .. context/s).
#include "common.h"
#include "host_weights.h"
#include "kernels.h"
#include "codec_kernels.h"
#include "q3_kernels.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <string>

#define MIMI_HP 64          // head-room columns in front of every streaming work-buffer row (>= the longest carried history)
#define MIMI_CHUNK 32       // frames per internal streaming sub-step (work buffers and the K/V ring are sized for it)

struct mis_mimi {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_mimi_config cfg{};
    int up_s = 2;                        // upsample stride = encoder frame rate / frame rate
    HostWeights raw{"Mimi"};
    bool finalized = false;
    DevBuf<float> arena;
    typedef F32Lin Lin;
    size_t rvq_tables = 0, up_w = 0, zeros = 0;
    struct TL { size_t n1w, n1b, n2w, n2b, ls1, ls2; Lin qkv, o, f1, f2; };
    std::vector<TL> tl;
    Lin init;
    struct Res { Lin c1, c2; int dil; };
    struct Dl { Lin ct; std::vector<Res> res; int r, cin, cout; };
    std::vector<Dl> dl;
    size_t fin_w = 0;
    float fin_b = 0.0f;
    int fin_c = 0;
    DevBuf<float> buf[4];
    CodecPack pack;
    DevBuf<int32_t> codes_dev;
    DevBuf<float> wav;                   // pcm of a call (kept: a stream step allocates nothing)
    struct Stream {
        bool open = false;
        int batch = 0, pos = 0, ring = 0;
        size_t hist_n = 0;
        DevBuf<float> hist;              // carried conv inputs, layers in call order: [layer][B][C][H]
        DevBuf<float> kv;                // [layers][B][2 D][ring]: K rows (unrotated), then V rows
    } st;
    mis_q3ref* enc = nullptr;            // tokenizer encoder (q3_reference.hip), built when the checkpoint has one
};

// ---------------------------------------------------------------------------- kernels
// ConvTrUpsample1d (depthwise, k = 2s, no bias, causal trim): y[c][s m + p] = x[c][m] w[c][p] + x[c][m-1] w[c][p+s]; column -1 of x is
// the carried input when streaming (x_lo = -HP), zero otherwise.  w [C][2s]
__global__ void k_mimi_upsample(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ w, int C, int Tin, int ldx,
                                int ldy, int s, int x_lo) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (n >= Tin * s) return;
    const int m = n / s, p = n - m * s;
    const float* xr = x + ((size_t)b * C + c) * ldx;
    const float prev = m - 1 >= x_lo ? xr[m - 1] : 0.0f;
    const float acc = xr[m] * w[c * 2 * s + p];
    y[((size_t)b * C + c) * ldy + n] = fmaf(prev, w[c * 2 * s + p + s], acc);
}

// ELU (alpha 1, Seanet.swift): y[c][t] = x > 0 ? x : exp(x) - 1 over columns [0, T) of [B][C][ld] rows
__global__ void k_mimi_elu(const float* __restrict__ x, float* __restrict__ y, int C, int T, int ld) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const size_t o = ((size_t)b * C + c) * ld + t;
    const float v = x[o];
    y[o] = v > 0.0f ? v : expf(v) - 1.0f;
}

// K and V rows of the fused q|k|v output (columns [0, Tn)) -> ring columns (pos0 + t) % ring
__global__ void k_mimi_kv_ring(const float* __restrict__ qkv, int64_t q_bs, int q_ld, int row0, float* __restrict__ kv, int64_t kv_bs,
                               int ring, int pos0, int Tn) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
    if (t >= Tn) return;
    kv[(size_t)b * kv_bs + (size_t)r * ring + (pos0 + t) % ring] = qkv[(size_t)b * q_bs + (size_t)(row0 + r) * q_ld + t];
}

// ---------------------------------------------------------------------------- handle and weights
extern "C" void mis_mimi_202407(int num_codebooks, mis_mimi_config* o) {
    if (!o) return;
    *o = mis_mimi_config{};
    o->channels = 1; o->sample_rate = 24000; o->frame_rate = 12.5f;
    o->dimension = 512; o->n_filters = 64; o->n_residual_layers = 1; o->n_ratios = 4;
    o->ratios[0] = 8; o->ratios[1] = 6; o->ratios[2] = 5; o->ratios[3] = 4;
    o->kernel_size = 7; o->residual_kernel_size = 3; o->last_kernel_size = 3; o->dilation_base = 2; o->compress = 2;
    o->num_layers = 8; o->num_heads = 8; o->dim_feedforward = 2048; o->context = 250;
    o->max_period = 10000.0f; o->norm_eps = 1e-5f;
    o->num_quantizers = num_codebooks; o->bins = 2048; o->quantizer_dim = 256;
}

static int mimi_hop(const mis_mimi_config& c) {
    int h = 1;
    for (int i = 0; i < c.n_ratios; ++i) h *= c.ratios[i];
    return h;
}

extern "C" mis_status mis_mimi_create(const mis_mimi_config* cfg, int device, mis_mimi** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    const mis_mimi_config& c = *cfg;
    MIS_REQUIRE(c.channels == 1 && c.n_ratios >= 1 && c.n_ratios <= 8 && c.n_filters >= 1 && c.dimension >= 1 && c.n_residual_layers >= 1 &&
                    c.compress >= 1 && c.dilation_base >= 1 && c.sample_rate > 0 && c.frame_rate > 0.0f,
                MIS_ERR_INVALID_INPUT, "bad Mimi SEANet configuration");
    MIS_REQUIRE(c.num_heads >= 1 && c.dimension % c.num_heads == 0, MIS_ERR_INVALID_INPUT, "bad Mimi transformer configuration");
    const int hd = c.dimension / c.num_heads;
    MIS_REQUIRE(hd == 16 || hd == 32 || hd == 64, MIS_ERR_INVALID_INPUT, "Mimi head_dim must be 16, 32 or 64");
    MIS_REQUIRE(c.num_quantizers >= 2 && c.bins >= 1 && c.quantizer_dim >= 1 && c.num_layers >= 0 && c.dim_feedforward >= 1 && c.context >= 1,
                MIS_ERR_INVALID_INPUT, "bad Mimi quantizer / transformer configuration");
    MIS_REQUIRE(c.kernel_size >= 1 && c.kernel_size <= 8 && c.last_kernel_size >= 1 && c.last_kernel_size <= 8 && c.residual_kernel_size >= 1 &&
                    c.residual_kernel_size <= 8, MIS_ERR_INVALID_INPUT, "Mimi kernel sizes above 8 are unsupported");
    int64_t dil = 1;
    for (int i = 1; i < c.n_residual_layers; ++i) dil *= c.dilation_base;
    MIS_REQUIRE((c.residual_kernel_size - 1) * dil <= MIMI_HP, MIS_ERR_INVALID_INPUT, "Mimi residual dilation too large");
    const double enc_fps = (double)c.sample_rate / (double)mimi_hop(c);
    const int s = (int)(enc_fps / (double)c.frame_rate);                                   // Mimi.swift:125-126
    MIS_REQUIRE(s >= 1 && s <= 8, MIS_ERR_INVALID_INPUT, "Mimi up/downsample stride %d unsupported", s);
    MIS_REQUIRE(((int64_t)(c.n_filters) << c.n_ratios) >= 1, MIS_ERR_INVALID_INPUT, "bad Mimi filters");
    hipStream_t stream = mis_open_stream(device);
    mis_mimi* m = new mis_mimi();
    m->device = device; m->cfg = c; m->up_s = s; m->stream = stream;
    *out = m;
    MIS_API_END
}

extern "C" void mis_mimi_destroy(mis_mimi* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->enc) q3ref_destroy(m->enc);
    hipStream_t s = m->stream;
    delete m;
    if (s) (void)hipStreamDestroy(s);
}

extern "C" int64_t mis_mimi_num_samples(const mis_mimi* m, int n_frames) {
    if (!m || n_frames < 0) return 0;
    return (int64_t)n_frames * m->up_s * mimi_hop(m->cfg);
}

extern "C" mis_status mis_mimi_set_tensor(mis_mimi* m, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    MIS_REQUIRE(m && name && data && shape, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(!m->finalized && ndim >= 1 && ndim <= 3, MIS_ERR_INVALID_INPUT, "bad tensor %s", name);
    m->raw.put_staged(m->device, name, data, dtype, shape, ndim);
    MIS_API_END
}

static bool mimi_is_encoder_key(const std::string& k) {
    return !k.compare(0, 8, "encoder.") || !k.compare(0, 20, "encoder_transformer.") || !k.compare(0, 11, "downsample.") ||
           !k.compare(0, 10, "quantizer.");
}

extern "C" mis_status mis_mimi_finalize(mis_mimi* m) {
    MIS_API_BEGIN
    MIS_REQUIRE(m && !m->finalized, MIS_ERR_INVALID_INPUT, "null or already finalized Mimi handle");
    HIP_CHECK(hipSetDevice(m->device));
    const mis_mimi_config& cf = m->cfg;
    const int64_t D = cf.dimension, H = cf.num_heads, hd = D / H, I = cf.dim_feedforward, nq = cf.num_quantizers, bins = cf.bins,
                  qd = cf.quantizer_dim, s = m->up_s;
    F32Arena arena;
    auto linear = [&](const std::vector<float>& w, int64_t out_f, int64_t in_f) { return arena.packed(lin_t(w, out_f, in_f), out_f, in_f, nullptr); };
    auto conv = [&](const std::string& p, int64_t co, int64_t k, int64_t ci) { return arena.conv(m->raw, p, co, k, ci); };
    auto convT = [&](const std::string& p, int64_t co, int64_t r, int64_t ci) {                     // [co][2r][ci], causal: phase ph takes taps ph + r j
        return arena.packed(convt_phases_t(m->raw.need(p + ".weight", {co, 2 * r, ci}).v, co, 2 * r, ci, r, 0, false), co, 2 * ci,
                            &m->raw.need(p + ".bias", {co}).v);
    };
    m->zeros = arena.zeros((size_t)std::max<int64_t>(D, (int64_t)cf.n_filters << cf.n_ratios));
    {   // folded RVQ tables [nq][bins][D] = output_proj . (embedding_sum / max(cluster_usage, 1e-5))  (Quantization.swift:22-32)
        std::vector<float> tables((size_t)nq * bins * D);
        for (int64_t q = 0; q < nq; ++q) {
            const std::string grp = q == 0 ? "rvq_first" : "rvq_rest";
            const std::string p = "quantizer." + grp + ".vq.layers." + std::to_string(q == 0 ? 0 : q - 1) + ".codebook";
            const auto& es = m->raw.need(p + ".embedding_sum", {bins, qd}).v;
            const auto& cu = m->raw.need(p + ".cluster_usage", {bins}).v;
            const auto& pw = m->raw.need("quantizer." + grp + ".output_proj.weight", {D, 1, qd}).v;
            std::vector<float> e((size_t)bins * qd);
            for (int64_t v = 0; v < bins; ++v) {
                const float den = std::max(cu[v], 1e-5f);
                for (int64_t k = 0; k < qd; ++k) e[v * qd + k] = es[v * qd + k] / den;
            }
            fold_tables_into(&tables[(size_t)q * bins * D], pw.data(), e.data(), nullptr, D, qd, bins);
        }
        m->rvq_tables = arena.push(tables);
    }
    m->up_w = arena.push(m->raw.need("upsample.convtr.convtr.convtr.weight", {D, 2 * s, 1}).v);                   // [C][2s][1] == [C][2s]
    m->tl.clear();
    for (int li = 0; li < cf.num_layers; ++li) {
        const std::string p = "decoder_transformer.transformer.layers." + std::to_string(li);
        mis_mimi::TL L{};
        L.n1w = arena.push(m->raw.need(p + ".norm1.weight", {D}).v); L.n1b = arena.push(m->raw.need(p + ".norm1.bias", {D}).v);
        L.n2w = arena.push(m->raw.need(p + ".norm2.weight", {D}).v); L.n2b = arena.push(m->raw.need(p + ".norm2.bias", {D}).v);
        L.ls1 = arena.push(m->raw.need(p + ".layer_scale_1.scale", {D}).v); L.ls2 = arena.push(m->raw.need(p + ".layer_scale_2.scale", {D}).v);
        {   // q / k rows of every head evens-then-odds (as q3_reference.hip): interleaved RoPE pairs become rotate-half pairs
            const auto& w = m->raw.need(p + ".self_attn.in_proj.weight", {3 * D, D}).v;
            std::vector<float> pw(w.size());
            for (int part = 0; part < 3; ++part)
                for (int64_t h = 0; h < H; ++h)
                    for (int64_t i = 0; i < hd; ++i) {
                        const int64_t src = part < 2 ? (i < hd / 2 ? 2 * i : 2 * (i - hd / 2) + 1) : i;
                        memcpy(&pw[((size_t)part * D + (size_t)h * hd + i) * D], &w[((size_t)part * D + (size_t)h * hd + src) * D], (size_t)D * 4);
                    }
            L.qkv = linear(pw, 3 * D, D);
        }
        L.o = linear(m->raw.need(p + ".self_attn.out_proj.weight", {D, D}).v, D, D);
        L.f1 = linear(m->raw.need(p + ".gating.linear1.weight", {I, D}).v, I, D);
        L.f2 = linear(m->raw.need(p + ".gating.linear2.weight", {D, I}).v, D, I);
        m->tl.push_back(L);
    }
    int64_t mult = (int64_t)1 << cf.n_ratios;
    m->init = conv("decoder.init_conv1d.conv.conv", mult * cf.n_filters, cf.kernel_size, D);
    m->dl.clear();
    for (int li = 0; li < cf.n_ratios; ++li) {
        const int64_t r = cf.ratios[li], cin = mult * cf.n_filters, cout = cin / 2, hid = cout / cf.compress;
        const std::string p = "decoder.layers." + std::to_string(li);
        mis_mimi::Dl L;
        L.r = (int)r; L.cin = (int)cin; L.cout = (int)cout;
        L.ct = convT(p + ".upsample.convtr.convtr", cout, r, cin);
        int dil = 1;
        for (int ri = 0; ri < cf.n_residual_layers; ++ri) {
            const std::string q = p + ".residuals." + std::to_string(ri);
            mis_mimi::Res R;
            R.c1 = conv(q + ".block.0.conv.conv", hid, cf.residual_kernel_size, cout);
            R.c2 = conv(q + ".block.1.conv.conv", cout, 1, hid);
            R.dil = dil;
            L.res.push_back(R);
            dil *= cf.dilation_base;
        }
        m->dl.push_back(L);
        mult /= 2;
    }
    m->fin_c = cf.n_filters;
    {
        const auto& w = m->raw.need("decoder.final_conv1d.conv.conv.weight", {1, cf.last_kernel_size, cf.n_filters}).v;   // [1][k][C] == [k][C]
        m->fin_w = arena.push(w);
        m->fin_b = m->raw.need("decoder.final_conv1d.conv.conv.bias", {1}).v[0];
    }
    // the encoder: present when the checkpoint carries it
    if (m->raw.count("encoder.init_conv1d.conv.conv.weight")) {
        mis_qwen3tts_reference_config rc{};
        rc.enc_audio_channels = 1; rc.enc_num_filters = cf.n_filters; rc.enc_kernel_size = cf.kernel_size;
        rc.enc_last_kernel_size = cf.last_kernel_size; rc.enc_residual_kernel_size = cf.residual_kernel_size;
        rc.enc_num_residual_layers = cf.n_residual_layers; rc.enc_dilation_growth_rate = cf.dilation_base; rc.enc_compress = cf.compress;
        rc.enc_n_ratios = cf.n_ratios;
        for (int i = 0; i < cf.n_ratios; ++i) rc.enc_upsampling_ratios[i] = cf.ratios[i];
        rc.enc_use_causal_conv = 1; rc.enc_use_conv_shortcut = 0;                                // trueSkip (Seanet.swift:140-150)
        rc.enc_hidden_size = cf.dimension; rc.enc_num_layers = cf.num_layers; rc.enc_num_heads = cf.num_heads;
        rc.enc_intermediate_size = cf.dim_feedforward;
        rc.enc_codebook_dim = cf.quantizer_dim; rc.enc_codebook_size = cf.bins; rc.enc_num_quantizers = cf.num_quantizers;
        rc.enc_valid_num_quantizers = cf.num_quantizers; rc.enc_sampling_rate = cf.sample_rate;
        rc.enc_rope_theta = cf.max_period; rc.enc_frame_rate = cf.frame_rate; rc.enc_norm_eps = cf.norm_eps;
        mis_q3ref* e = q3ref_create(&rc, m->device, m->stream, "");
        try {
            for (auto& kv : m->raw) {
                if (!mimi_is_encoder_key(kv.first)) continue;
                const auto& sh = kv.second.shape;
                q3ref_set_tensor(e, kv.first.c_str(), kv.second.v.data(), MIS_F32, sh.data(), (int)sh.size());
            }
            q3ref_finalize(e);
        } catch (...) { q3ref_destroy(e); throw; }
        m->enc = e;
    }
    arena.upload(m->arena);
    m->raw.clear();
    m->finalized = true;
    MIS_API_END
}

// ---------------------------------------------------------------------------- decode
// history floats one row carries through a stream (in call order of mimi_run)
static size_t mimi_hist_floats(const mis_mimi* m) {
    const mis_mimi_config& cf = m->cfg;
    size_t n = (size_t)cf.dimension;                                             // upsample: one input column
    n += (size_t)cf.dimension * (cf.kernel_size - 1);                            // init conv
    for (auto& L : m->dl) {
        n += (size_t)L.cin;                                                      // transposed conv: one input column
        for (auto& R : L.res) n += (size_t)L.cout * (cf.residual_kernel_size - 1) * R.dil;
    }
    n += (size_t)m->fin_c * (cf.last_kernel_size - 1);
    return n;
}

// floats per batch row of one work buffer for T frames (row stride LD(columns))
static size_t mimi_buf_elems(const mis_mimi* m, int T, int HP) {
    const mis_mimi_config& cf = m->cfg;
    auto LD = [&](int64_t Tc) { return (size_t)(HP ? HP + round_up(Tc, 4) : Tc); };
    const int64_t Tt = (int64_t)T * m->up_s;
    size_t need = (size_t)cf.dimension * LD(T);
    need = std::max(need, (size_t)std::max<int64_t>({3 * (int64_t)cf.dimension, cf.dim_feedforward, m->init.M}) * LD(Tt));
    int64_t Tc = Tt;
    for (auto& L : m->dl) { need = std::max(need, (size_t)L.cin * LD(Tc)); Tc *= L.r; need = std::max(need, (size_t)L.cout * LD(Tc)); }
    return need;
}

// codes element (b, q, t) at codes_dev[b*cs_b + q*cs_q + t*cs_t].  st == nullptr: whole sequence of T frames; else the next T frames of
// the open stream.  stop_after (whole sequence only): 0 full; 1 RVQ latent; 2 upsampled; 3 transformer; 4 init conv; 5 + i layer i.
static const float* mimi_run(mis_mimi* m, const int32_t* codes_dev, int64_t cs_b, int64_t cs_q, int64_t cs_t, int n_q, int batch, int T,
                             float* wav_dev, int64_t wav_stride, int stop_after, int* outC, int64_t* outT, mis_mimi::Stream* st) {
    CodecPackScope pack_scope(&m->pack);
    const mis_mimi_config& cf = m->cfg;
    hipStream_t s = m->stream;
    const float* W = m->arena.p;
    const int D = cf.dimension, H = cf.num_heads, hd = D / H, us = m->up_s;
    const int HP = st ? MIMI_HP : 0;
    auto LD = [&](int64_t Tc) { return (int)(HP ? HP + round_up(Tc, 4) : Tc); };
    if (!st) {
        const size_t need = mimi_buf_elems(m, T, 0);
        for (int i = 0; i < 4; ++i) m->buf[i].alloc((size_t)batch * need);
    }
    float *a = m->buf[0].p + HP, *b = m->buf[1].p + HP, *t1 = m->buf[2].p + HP, *t2 = m->buf[3].p + HP;   // column 0 of row 0
    auto gemm = [&](const mis_mimi::Lin& L, const float* X, float* Y, int N, int Tin, int Tout, const float* R = nullptr, const float* scale = nullptr) {
        GemmParams g{};
        g.AT = W + L.w; g.bias = L.b == F32Lin::npos ? nullptr : W + L.b; g.X = X; g.Y = Y; g.R = R; g.scale = scale;
        g.M = L.M; g.K = L.K; g.N = N; g.Tin = Tin; g.Tout = Tout;
        g.ldx = LD(Tin); g.ldy = LD(Tout); g.x_lo = -HP;
        return g;
    };
    size_t hist_cur = 0;
    auto hist = [&](float* x, int C, int Tn, int Hc) {
        if (!st || Hc == 0) return;
        MIS_REQUIRE(Hc <= MIMI_HP && hist_cur + (size_t)batch * C * Hc <= st->hist_n, MIS_ERR_GENERATION_FAILED, "streaming history overflow");
        launch_codec_hist(st->hist.p + hist_cur, x, C, LD(Tn), Hc, Tn, batch, s);
        hist_cur += (size_t)batch * C * Hc;
    };
    auto elu = [&](const float* x, float* y, int C, int Tc) {
        hipLaunchKernelGGL(k_mimi_elu, dim3(cdiv(Tc, 256), C, batch), dim3(256), 0, s, x, y, C, Tc, LD(Tc));
    };
    const float* Z = W + m->zeros;
    launch_codec_embed(codes_dev, cs_b, cs_q, cs_t, W + m->rvq_tables, a, n_q, cf.bins, D, LD(T), T, batch, s);
    if (stop_after == 1) { *outC = D; *outT = T; return a; }
    // ConvTrUpsample1d
    const int Tt = T * us;
    hist(a, D, T, 1);
    hipLaunchKernelGGL(k_mimi_upsample, dim3(cdiv(Tt, 256), D, batch), dim3(256), 0, s, a, b, W + m->up_w, D, T, LD(T), LD(Tt), us, -HP);
    float* x = b; float* y = a;
    if (stop_after == 2) { *outC = D; *outT = Tt; return x; }
    // decoder transformer on Tt columns at positions pos0 ..
    const int ldT = LD(Tt), pos0 = st ? st->pos * us : 0;
    int li = 0;
    for (auto& L : m->tl) {
        launch_q3_norm_ct(x, t1, W + L.n1w, W + L.n1b, batch, D, Tt, ldT, cf.norm_eps, 0, s);
        launch_gemm(GEMM_PLAIN, false, gemm(L.qkv, t1, t2, Tt, Tt, Tt), batch, s);
        Q3AttnArgs aa{};
        aa.q = t2; aa.q_bs = (int64_t)3 * D * ldT; aa.q_ld = ldT;
        aa.out = t1; aa.o_bs = (int64_t)D * ldT; aa.o_ld = ldT;
        aa.H = H; aa.Hkv = H; aa.Tq = Tt; aa.pos0 = pos0; aa.theta = cf.max_period; aa.scale = 1.0f / sqrtf((float)hd);
        if (st) {
            const int64_t kv_bs = (int64_t)2 * D * st->ring;
            float* cache = st->kv.p + (size_t)li * batch * kv_bs;
            hipLaunchKernelGGL(k_mimi_kv_ring, dim3(cdiv(Tt, 64), 2 * D, batch), dim3(64), 0, s, t2, aa.q_bs, ldT, D, cache, kv_bs, st->ring, pos0, Tt);
            aa.k = cache; aa.v = cache + (size_t)D * st->ring; aa.kv_bs = kv_bs; aa.kv_ld = st->ring;
            aa.window = cf.context; aa.win_group = us; aa.ring = st->ring;
        } else {
            aa.k = t2 + (size_t)D * ldT; aa.v = t2 + (size_t)2 * D * ldT; aa.kv_bs = aa.q_bs; aa.kv_ld = ldT;
        }
        launch_q3_attn(aa, hd, batch, s);
        launch_gemm(GEMM_RESID, false, gemm(L.o, t1, y, Tt, Tt, Tt, x, W + L.ls1), batch, s);
        std::swap(x, y);
        launch_q3_norm_ct(x, t1, W + L.n2w, W + L.n2b, batch, D, Tt, ldT, cf.norm_eps, 0, s);
        launch_gemm(GEMM_GELU, false, gemm(L.f1, t1, t2, Tt, Tt, Tt), batch, s);
        launch_gemm(GEMM_RESID, false, gemm(L.f2, t2, y, Tt, Tt, Tt, x, W + L.ls2), batch, s);
        std::swap(x, y);
        ++li;
    }
    if (stop_after == 3) { *outC = D; *outT = Tt; return x; }
    // SeanetDecoder
    int Tc = Tt;
    {
        const int k = cf.kernel_size;
        hist(x, D, Tc, k - 1);
        GemmParams g = gemm(m->init, x, y, Tc, Tc, Tc);
        g.Cin = D; g.taps = k; g.dil = 1; g.pad = k - 1;
        launch_gemm(GEMM_TAPS, false, g, batch, s);
        std::swap(x, y);
    }
    if (stop_after == 4) { *outC = m->init.M; *outT = Tc; return x; }
    int bi = 0;
    for (auto& L : m->dl) {
        elu(x, t1, L.cin, Tc);
        hist(t1, L.cin, Tc, 1);                                          // tap p + r of output frame n reads input column n - 1
        GemmParams g = gemm(L.ct, t1, y, Tc, Tc, Tc * L.r, nullptr, nullptr);
        g.alpha = Z; g.ralpha = Z;                                       // the transposed conv always runs the operand prologue: identity
        g.s = L.r; g.pad = 0; g.Cin = L.cin;
        launch_gemm(GEMM_CONVT, true, g, batch, s);
        Tc *= L.r;
        std::swap(x, y);
        for (auto& R : L.res) {
            const int k = cf.residual_kernel_size;
            elu(x, t1, L.cout, Tc);
            hist(t1, L.cout, Tc, (k - 1) * R.dil);
            GemmParams g1 = gemm(R.c1, t1, t2, Tc, Tc, Tc);
            g1.Cin = L.cout; g1.taps = k; g1.dil = R.dil; g1.pad = (k - 1) * R.dil;
            launch_gemm(GEMM_TAPS, false, g1, batch, s);
            elu(t2, t2, R.c1.M, Tc);
            launch_gemm(GEMM_RESID, false, gemm(R.c2, t2, y, Tc, Tc, Tc, x), batch, s);
            std::swap(x, y);
        }
        if (stop_after == 5 + bi) { *outC = L.cout; *outT = Tc; return x; }
        ++bi;
    }
    MIS_REQUIRE((int64_t)Tc == mis_mimi_num_samples(m, T), MIS_ERR_GENERATION_FAILED, "internal length mismatch");
    hist(x, m->fin_c, Tc, cf.last_kernel_size - 1);
    launch_codec_final(x, wav_dev, wav_stride, W + m->fin_w, m->fin_b, nullptr, nullptr, m->fin_c, Tc, LD(Tc), -HP, cf.last_kernel_size, batch, s);   // ELU
    HIP_CHECK(hipGetLastError());
    if (st) {
        MIS_REQUIRE(hist_cur == st->hist_n, MIS_ERR_GENERATION_FAILED, "streaming history bookkeeping mismatch");
        st->pos += T;
    }
    *outC = 1; *outT = Tc;
    return wav_dev;
}

static void mimi_check_codes(const mis_mimi* m, const int32_t* codes, int batch, int n_q, int T, const void* out) {
    MIS_REQUIRE(m && codes && out && batch >= 1 && T >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(m->finalized, MIS_ERR_NOT_INITIALIZED, "Mimi handle not finalized");
    MIS_REQUIRE(n_q >= 2 && n_q <= m->cfg.num_quantizers, MIS_ERR_INVALID_INPUT, "n_q %d outside [2, %d]", n_q, m->cfg.num_quantizers);
}

extern "C" mis_status mis_mimi_decode(mis_mimi* m, const int32_t* codes, int batch, int n_q, int T, float* pcm_out) {
    MIS_API_BEGIN
    mimi_check_codes(m, codes, batch, n_q, T, pcm_out);
    HIP_CHECK(hipSetDevice(m->device));
    const int64_t n = mis_mimi_num_samples(m, T);
    m->codes_dev.alloc((size_t)batch * n_q * T);
    HIP_CHECK(hipMemcpyAsync(m->codes_dev.p, codes, (size_t)batch * n_q * T * 4, hipMemcpyDefault, m->stream));
    DevBuf<float>& wav = m->wav;
    wav.alloc((size_t)batch * n);
    int C; int64_t Tt;
    mimi_run(m, m->codes_dev.p, (int64_t)n_q * T, T, 1, n_q, batch, T, wav.p, n, 0, &C, &Tt, nullptr);
    HIP_CHECK(hipMemcpyAsync(pcm_out, wav.p, (size_t)batch * n * 4, hipMemcpyDefault, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    MIS_API_END
}

extern "C" mis_status mis_debug_mimi_decoder_tap(mis_mimi* m, const int32_t* codes, int batch, int n_q, int T, int stage, float* out,
                                                 int64_t capacity, int32_t* channels, int64_t* length) {
    MIS_API_BEGIN
    mimi_check_codes(m, codes, batch, n_q, T, out);
    MIS_REQUIRE(channels && length && stage >= 0 && stage <= 4 + m->cfg.n_ratios, MIS_ERR_INVALID_INPUT, "bad tap stage %d", stage);
    HIP_CHECK(hipSetDevice(m->device));
    const int64_t n = mis_mimi_num_samples(m, T);
    m->codes_dev.alloc((size_t)batch * n_q * T);
    HIP_CHECK(hipMemcpyAsync(m->codes_dev.p, codes, (size_t)batch * n_q * T * 4, hipMemcpyDefault, m->stream));
    DevBuf<float> wav;
    wav.alloc((size_t)batch * n);
    int C = 0; int64_t Tt = 0;
    const int stop = stage == 4 + m->cfg.n_ratios ? 0 : stage + 1;
    const float* res = mimi_run(m, m->codes_dev.p, (int64_t)n_q * T, T, 1, n_q, batch, T, wav.p, n, stop, &C, &Tt, nullptr);
    MIS_REQUIRE((int64_t)batch * C * Tt <= capacity, MIS_ERR_INVALID_INPUT, "tap buffer too small (%lld floats needed)", (long long)((int64_t)batch * C * Tt));
    HIP_CHECK(hipMemcpyAsync(out, res, (size_t)batch * C * Tt * 4, hipMemcpyDefault, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    *channels = C; *length = Tt;
    MIS_API_END
}

// ---- streaming (MimiStreamingDecoder.reset / decodeFrames)
extern "C" mis_status mis_mimi_decode_stream_begin(mis_mimi* m, int batch) {
    MIS_API_BEGIN
    MIS_REQUIRE(m && batch >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(m->finalized, MIS_ERR_NOT_INITIALIZED, "Mimi handle not finalized");
    HIP_CHECK(hipSetDevice(m->device));
    const mis_mimi_config& cf = m->cfg;
    auto& st = m->st;
    st.open = false;
    st.batch = batch; st.pos = 0;
    st.ring = round_up(cf.context + m->up_s * MIMI_CHUNK, 4);         // >= every key a sub-step's queries see plus the keys it appends
    st.hist_n = (size_t)batch * mimi_hist_floats(m);
    st.hist.alloc(st.hist_n);
    st.kv.alloc(std::max<size_t>((size_t)cf.num_layers * batch * 2 * cf.dimension * st.ring, 4));
    HIP_CHECK(hipMemsetAsync(st.hist.p, 0, st.hist_n * 4, m->stream));   // no history = the causal zero padding (Conv.swift:237-241)
    const size_t need = mimi_buf_elems(m, MIMI_CHUNK, MIMI_HP);
    for (int i = 0; i < 4; ++i) m->buf[i].alloc((size_t)batch * need + 2 * MIMI_HP);
    HIP_CHECK(hipStreamSynchronize(m->stream));
    st.open = true;
    MIS_API_END
}

extern "C" mis_status mis_mimi_decode_stream_step(mis_mimi* m, const int32_t* codes, int n_q, int n_frames, float* pcm_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(m, MIS_ERR_INVALID_INPUT, "null handle");
    MIS_REQUIRE(m->st.open, MIS_ERR_NOT_INITIALIZED, "no Mimi stream is open (mis_mimi_decode_stream_begin)");
    const int batch = m->st.batch;
    mimi_check_codes(m, codes, batch, n_q, n_frames, pcm_out);
    HIP_CHECK(hipSetDevice(m->device));
    const int64_t spf = mis_mimi_num_samples(m, 1), n = (int64_t)n_frames * spf;
    m->codes_dev.alloc((size_t)batch * n_q * n_frames);
    HIP_CHECK(hipMemcpyAsync(m->codes_dev.p, codes, (size_t)batch * n_q * n_frames * 4, hipMemcpyDefault, m->stream));
    DevBuf<float>& wav = m->wav;
    wav.alloc((size_t)batch * n);
    // a step of several frames equals the frames one call at a time; the sub-steps keep the work buffers and the ring bounded
    for (int f0 = 0; f0 < n_frames; f0 += MIMI_CHUNK) {
        const int Tn = std::min(MIMI_CHUNK, n_frames - f0);
        int C; int64_t Tt;
        mimi_run(m, m->codes_dev.p + f0, (int64_t)n_q * n_frames, n_frames, 1, n_q, batch, Tn, wav.p + f0 * spf, n, 0, &C, &Tt, &m->st);
    }
    HIP_CHECK(hipMemcpyAsync(pcm_out, wav.p, (size_t)batch * n * 4, hipMemcpyDefault, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    MIS_API_END
}

// hooks for marvis.hip (kernels.h): the open session's next frames from device codes, enqueued on the handle's stream, no synchronisation
hipStream_t mimi_internal_stream(mis_mimi* m) { return m->stream; }
int mimi_internal_device(const mis_mimi* m) { return m->device; }
int mimi_internal_num_quantizers(const mis_mimi* m) { return m->cfg.num_quantizers; }
bool mimi_internal_stream_open(const mis_mimi* m) { return m->st.open; }
void mimi_internal_stream_step_device(mis_mimi* m, const int32_t* codes_dev, int64_t cs_b, int64_t cs_q, int64_t cs_t, int n_q, int n_frames,
                                      float* wav_dev, int64_t wav_stride) {
    MIS_REQUIRE(m && m->st.open, MIS_ERR_NOT_INITIALIZED, "no Mimi stream is open (mis_mimi_decode_stream_begin)");
    mimi_check_codes(m, codes_dev, m->st.batch, n_q, n_frames, wav_dev);
    HIP_CHECK(hipSetDevice(m->device));
    const int64_t spf = mis_mimi_num_samples(m, 1);
    for (int f0 = 0; f0 < n_frames; f0 += MIMI_CHUNK) {
        const int Tn = std::min(MIMI_CHUNK, n_frames - f0);
        int C; int64_t Tt;
        mimi_run(m, codes_dev + (int64_t)f0 * cs_t, cs_b, cs_q, cs_t, n_q, m->st.batch, Tn, wav_dev + f0 * spf, wav_stride, 0, &C, &Tt, &m->st);
    }
}

extern "C" mis_status mis_mimi_decode_stream_end(mis_mimi* m) {
    MIS_API_BEGIN
    MIS_REQUIRE(m, MIS_ERR_INVALID_INPUT, "null handle");
    MIS_REQUIRE(m->st.open, MIS_ERR_NOT_INITIALIZED, "no Mimi stream is open");
    m->st.open = false;
    MIS_API_END
}

// ---- encode (Mimi.encode :168-176)
extern "C" int64_t mis_mimi_encode_num_frames(const mis_mimi* m, int64_t n_samples) {
    if (!m || n_samples < 1) return 0;
    int64_t T = n_samples;                                                   // every strided conv completes its last stride (Conv.swift:206-226)
    for (int i = m->cfg.n_ratios - 1; i >= 0; --i) T = (T + m->cfg.ratios[i] - 1) / m->cfg.ratios[i];
    return (T + m->up_s - 1) / m->up_s;
}

extern "C" mis_status mis_mimi_encode(mis_mimi* m, const float* audio, int batch, int64_t n_samples, int n_q, int32_t* codes_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(m && audio && codes_out && batch >= 1 && n_samples >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(m->finalized, MIS_ERR_NOT_INITIALIZED, "Mimi handle not finalized");
    MIS_REQUIRE(m->enc, MIS_ERR_AUDIO_ENCODE, "this Mimi checkpoint has no encoder tensors");
    MIS_REQUIRE(n_q >= 1 && n_q <= m->cfg.num_quantizers, MIS_ERR_INVALID_INPUT, "n_q %d outside [1, %d]", n_q, m->cfg.num_quantizers);
    HIP_CHECK(hipSetDevice(m->device));
    const int64_t T = mis_mimi_encode_num_frames(m, n_samples);
    for (int b = 0; b < batch; ++b) {                                        // one row at a time
        std::vector<int32_t> codes;
        int nq = 0; int64_t Tr = 0;
        q3ref_encode(m->enc, audio + (size_t)b * n_samples, n_samples, -1, nullptr, 0, nullptr, &Tr, &codes, &nq);
        MIS_REQUIRE(Tr == T && nq >= n_q, MIS_ERR_GENERATION_FAILED, "encoder frame count mismatch (%lld vs %lld)", (long long)Tr, (long long)T);
        // codes [nq][T]: the first n_q rows (the residual of later layers never reaches earlier ones)
        HIP_CHECK(hipMemcpy(codes_out + (size_t)b * n_q * T, codes.data(), (size_t)n_q * T * 4, hipMemcpyDefault));
    }
    MIS_API_END
}
