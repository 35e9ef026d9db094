// smartturn.hip - Smart Turn endpoint detection: waveform window -> log-mel -> Whisper-style encoder -> attention pool -> classifier.
//
// Reference being replaced: SmartTurnModel / SmartTurnWhisperEncoder (Sources/MLXAudioVAD/Models/SmartTurn/SmartTurn.swift:29-272),
// smartTurnPrepareAudioSamples / smartTurnLogMelSpectrogram (SmartTurnFeatures.swift:10-81), SmartTurnConfig.swift.
//
// One call serves 1..64 rows.  Every row is its own window of W = max_audio_seconds * sampling_rate samples (the row's tail, or the row
// left-padded with zeros), F = W / hop_length frames, T = F / 2 encoder positions: the batch is dense, nothing is masked.
//
//   k_st_stat_partial  mean / variance of the padded window over fixed 8192-sample chunks summed in a fixed order: a row's statistics
//                      do not depend on the batch it travels in (the reference sums sequentially on the host, :35-42)
//   k_st_prepare       the window itself: tail or left padding, (x - mean) / max(std, 1e-7)
//   mel_spectrogram_device (mel.hip)  symmetric Hann, Slaney scale and norm, last frame dropped, per-row clamp
//   k_st_patches       k = 3 patches of the f32 features, rounded to bf16, columns zero-padded to a multiple of 32
//   whisper_encoder_enqueue (whisper_kernels.hip)  the encoder, the chain the Whisper engine runs: bf16 storage, f32 accumulation, one
//                      rounding per primitive
//   k_st_pool_scores   s_t = w2 . tanh(W0 h_t + b0) + b2 in f32, 8 positions per block (T / 8 blocks per row.  Chosen from the
//                      arithmetic: at the published shape a row's scores are 400 x 384 x 256 = 39 M multiply-adds, which one
//                      256-thread block would walk alone; one block per row was not measured.  Measured: scores + head together
//                      0.079 ms at 1 row, 0.214 ms at 64, profiles/smartturn/bench.jsonl)
//   k_st_pool_head     softmax over the row's T scores, pooled = sum_t a_t h_t, Linear -> LayerNorm -> GELU -> Linear -> GELU -> Linear,
//                      sigmoid and the decision; one block per row, f32 throughout
//
// The chain from the patches to the head is linear and is captured once per batch size into a hipGraph (MIS_NO_GRAPH: plain launches).
// As measured the replay is level with plain launches (0.484 vs 0.481 ms on the device at 1 row, 0.865 vs 0.875 ms per call).
// Prepare and mel stay in front of it: the mel front end allocates and synchronises.
#include "common.h"
#include "host_weights.h"
#include "step_loop.h"
#include "kernels.h"
#include "lm_kernels.h"
#include "whisper_kernels.h"

#include <math.h>
#include <string.h>
#include <memory>

#define ST_MAX_BATCH 64
#define ST_CHUNK 8192            // samples per statistics chunk
#define ST_POOL_HID 256          // pool_attention_0 / classifier_0 width (SmartTurn.swift:168-172)
#define ST_CLS_MID 64
#define ST_TS 8                  // positions per k_st_pool_scores block
#define ST_LN_EPS 1e-5f       // MLXNN.LayerNorm default

struct mis_smartturn {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_smartturn_config cfg{};
    int W = 0, F = 0, T = 0, d = 0, H = 0, D = 0, ffn = 0, nmel = 0, K1 = 0, Spad = 0, nch = 0;
    mis_mel_config mel{};
    HostWeights raw{"Smart Turn", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<bf16_t> arena;
    DevBuf<float> farena;
    WhisperEncWeights enc;
    float *p0wT = nullptr, *p0b = nullptr, *p2w = nullptr, *p2b = nullptr, *c0wT = nullptr, *c0b = nullptr, *c1w = nullptr, *c1b = nullptr,
          *c4wT = nullptr, *c4b = nullptr, *c6w = nullptr, *c6b = nullptr;
    // work buffers for `cap` rows; the graphs hold their addresses and die with them
    int cap = 0, last_batch = 0, last_launches = 0;
    DevBuf<float> pcm_in, prep, part0, part1, feat, feat_in, scores, pooled, logit, prob, thr;
    DevBuf<int64_t> lens;
    DevBuf<int32_t> pred;
    DevBuf<bf16_t> col1, h1, col2, h, x, qkv, att, ff, kc, vc, enc_out;
    std::map<int, StepGraph> graphs;
    HipEvents<4> ev;
    float ms_prepare = 0.0f, ms_encoder = 0.0f, ms_head = 0.0f;
};

extern "C" mis_status mis_smartturn_create(const mis_smartturn_config* cfg, int device, mis_smartturn** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    // the configuration is judged before the device is touched
    MIS_REQUIRE(cfg->sampling_rate > 0 && cfg->max_audio_seconds > 0 && cfg->hop_length > 0, MIS_ERR_INVALID_INPUT, "bad processor sizes");
    MIS_REQUIRE(cfg->n_fft >= 16 && cfg->n_fft <= 2048 && cfg->n_fft % 2 == 0, MIS_ERR_INVALID_INPUT, "n_fft %d unsupported (even, 16..2048)", cfg->n_fft);
    MIS_REQUIRE(cfg->num_mel_bins >= 1 && cfg->num_mel_bins <= 256, MIS_ERR_INVALID_INPUT, "num_mel_bins %d unsupported (1..256)", cfg->num_mel_bins);
    const int64_t W = (int64_t)cfg->max_audio_seconds * cfg->sampling_rate;
    MIS_REQUIRE(W <= 16000 * 60 && W >= cfg->n_fft, MIS_ERR_INVALID_INPUT, "window of %lld samples unsupported", (long long)W);
    const int F = (int)(W / cfg->hop_length), T = F / 2;
    MIS_REQUIRE(F >= 2 && F % 2 == 0, MIS_ERR_INVALID_INPUT, "the window gives %d frames: an even count is needed (conv2 has stride 2)", F);
    MIS_REQUIRE(T <= cfg->max_source_positions, MIS_ERR_INVALID_INPUT, "the window gives %d positions, max_source_positions is %d", T,
                cfg->max_source_positions);
    MIS_REQUIRE(T <= 4096, MIS_ERR_INVALID_INPUT, "%d positions unsupported (at most 4096)", T);
    const int d = cfg->d_model, H = cfg->encoder_attention_heads;
    MIS_REQUIRE(d > 0 && d % 32 == 0 && d <= 1280, MIS_ERR_INVALID_INPUT, "d_model %d unsupported (a multiple of 32, at most 1280)", d);
    MIS_REQUIRE(cfg->encoder_ffn_dim > 0 && cfg->encoder_ffn_dim % 32 == 0, MIS_ERR_INVALID_INPUT, "encoder_ffn_dim must be a multiple of 32");
    MIS_REQUIRE(H > 0 && d % H == 0 && (d / H == 64 || d / H == 128), MIS_ERR_INVALID_INPUT, "head size %d unsupported (64 or 128)", H > 0 ? d / H : 0);
    MIS_REQUIRE(cfg->encoder_layers >= 1 && cfg->encoder_layers <= 64, MIS_ERR_INVALID_INPUT, "bad encoder_layers");
    MIS_REQUIRE(cfg->threshold >= 0.0f && cfg->threshold <= 1.0f, MIS_ERR_INVALID_INPUT, "threshold outside [0, 1]");
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_smartturn>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->W = (int)W; c->F = F; c->T = T; c->d = d; c->H = H; c->D = d / H; c->ffn = cfg->encoder_ffn_dim; c->nmel = cfg->num_mel_bins;
    c->K1 = (int)round_up((size_t)3 * c->nmel, 32); c->Spad = (int)round_up(T, 32); c->nch = cdiv(W, ST_CHUNK);
    c->mel.sample_rate = cfg->sampling_rate; c->mel.n_fft = cfg->n_fft; c->mel.hop_length = cfg->hop_length; c->mel.n_mels = c->nmel;
    c->mel.window = 1; c->mel.mel_scale = 1; c->mel.slaney_norm = 1; c->mel.drop_last_frame = 1;      // SmartTurnFeatures.swift:56-72
    MIS_REQUIRE(mis_mel_num_frames(&c->mel, W) == F, MIS_ERR_INVALID_INPUT, "frame count of the front end differs from W / hop_length");
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_smartturn_destroy(mis_smartturn* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->graphs.clear();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// names are the ones SmartTurnModel.sanitize leaves (SmartTurn.swift:274-324); host pointers
extern "C" mis_status mis_smartturn_set_tensor(mis_smartturn* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape,
                                               int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 3, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

extern "C" mis_status mis_smartturn_finalize(mis_smartturn* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t d = c->d, f = c->ffn, nm = c->nmel, K1 = c->K1, T = c->T;
    HostArena a(c->raw);
    std::vector<bf16_t>& host = a.host;                 // the packers below write through these
    std::vector<float>& fhost = a.fhost;                // the f32 head
    // Linear.weight [N][K] -> [K][N]: a thread is an output unit, neighbouring threads read neighbouring floats
    auto fmatT = [&](const std::string& name, int64_t N, int64_t K, float*& dst) {
        const HostTensor& t = c->raw.need(name, {N, K});
        size_t off = a.ftake((size_t)N * K, dst);
        for (int64_t n = 0; n < N; ++n) for (int64_t k = 0; k < K; ++k) fhost[off + (size_t)k * N + n] = t.v[(size_t)n * K + k];
    };
    const std::string E = "encoder";
    WhisperEncWeights& w = c->enc;
    // conv weights [out][k][in] (MLX layout after sanitize): the column order of the k = 3 patches; conv1's rows padded to K1 columns
    {
        const HostTensor& t = c->raw.need(E + ".conv1.weight", {d, 3, nm});
        const size_t o = a.btake((size_t)d * K1, w.conv1w);
        for (int64_t n = 0; n < d; ++n) for (int64_t k = 0; k < 3 * nm; ++k) host[o + (size_t)n * K1 + k] = f32_to_bf16(t.v[(size_t)n * 3 * nm + k]);
    }
    a.bvec(E + ".conv1.bias", d, w.conv1b);
    {
        const HostTensor& t = c->raw.need(E + ".conv2.weight", {d, 3, d});
        const size_t o = a.btake((size_t)d * 3 * d, w.conv2w);
        for (size_t i = 0; i < (size_t)d * 3 * d; ++i) host[o + i] = f32_to_bf16(t.v[i]);
    }
    a.bvec(E + ".conv2.bias", d, w.conv2b);
    {   // rows 0 .. T - 1 of the table (:141-142)
        const HostTensor& t = c->raw.need(E + ".embed_positions.weight", {(int64_t)c->cfg.max_source_positions, d});
        const size_t o = a.btake((size_t)T * d, w.pos);
        for (size_t i = 0; i < (size_t)T * d; ++i) host[o + i] = f32_to_bf16(t.v[i]);
    }
    w.layers.assign(c->cfg.encoder_layers, WhisperEncLayer{});
    for (size_t li = 0; li < w.layers.size(); ++li) {
        const std::string q = E + ".layers." + std::to_string(li);
        WhisperEncLayer& l = w.layers[li];
        a.bvec(q + ".self_attn_layer_norm.weight", d, l.ln1w); a.bvec(q + ".self_attn_layer_norm.bias", d, l.ln1b);
        const size_t ow = a.btake((size_t)3 * d * d, l.wqkv);
        a.bmat_into(q + ".self_attn.q_proj.weight", d, d, ow);
        a.bmat_into(q + ".self_attn.k_proj.weight", d, d, ow + (size_t)d * d);
        a.bmat_into(q + ".self_attn.v_proj.weight", d, d, ow + (size_t)2 * d * d);
        const size_t ob = a.btake(3 * d, l.bqkv);
        {
            const HostTensor& qb = c->raw.need(q + ".self_attn.q_proj.bias", {d});
            const HostTensor& vb = c->raw.need(q + ".self_attn.v_proj.bias", {d});
            for (int64_t i = 0; i < d; ++i) { host[ob + i] = f32_to_bf16(qb.v[i]); host[ob + 2 * d + i] = f32_to_bf16(vb.v[i]); }
            if (c->cfg.k_proj_bias) {
                const HostTensor& kb = c->raw.need(q + ".self_attn.k_proj.bias", {d});
                for (int64_t i = 0; i < d; ++i) host[ob + d + i] = f32_to_bf16(kb.v[i]);
            }
        }
        a.bmat(q + ".self_attn.out_proj.weight", d, d, l.wo); a.bvec(q + ".self_attn.out_proj.bias", d, l.bo);
        a.bvec(q + ".final_layer_norm.weight", d, l.ln2w); a.bvec(q + ".final_layer_norm.bias", d, l.ln2b);
        a.bmat(q + ".fc1.weight", f, d, l.fc1); a.bvec(q + ".fc1.bias", f, l.b1);
        a.bmat(q + ".fc2.weight", d, f, l.fc2); a.bvec(q + ".fc2.bias", d, l.b2);
    }
    a.bvec(E + ".layer_norm.weight", d, w.lnw); a.bvec(E + ".layer_norm.bias", d, w.lnb);
    // ---- the head, f32 as stored
    fmatT("pool_attention_0.weight", ST_POOL_HID, d, c->p0wT); a.fvec("pool_attention_0.bias", {ST_POOL_HID}, ST_POOL_HID, c->p0b);
    a.fvec("pool_attention_2.weight", {1, ST_POOL_HID}, ST_POOL_HID, c->p2w); a.fvec("pool_attention_2.bias", {1}, 1, c->p2b);
    fmatT("classifier_0.weight", ST_POOL_HID, d, c->c0wT); a.fvec("classifier_0.bias", {ST_POOL_HID}, ST_POOL_HID, c->c0b);
    a.fvec("classifier_1.weight", {ST_POOL_HID}, ST_POOL_HID, c->c1w); a.fvec("classifier_1.bias", {ST_POOL_HID}, ST_POOL_HID, c->c1b);
    fmatT("classifier_4.weight", ST_CLS_MID, ST_POOL_HID, c->c4wT); a.fvec("classifier_4.bias", {ST_CLS_MID}, ST_CLS_MID, c->c4b);
    a.fvec("classifier_6.weight", {1, ST_CLS_MID}, ST_CLS_MID, c->c6w); a.fvec("classifier_6.bias", {1}, 1, c->c6b);
    // ---- upload (no call reads the handle before finalized is set: a rejected finalize can be repeated)
    a.upload(c->arena, c->farena);
    w.d = c->d; w.H = c->H; w.D = c->D; w.ffn = c->ffn; w.K1 = c->K1; w.Spad = c->Spad;
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of a sanitized checkpoint; the head's gains keep logits of order 1
extern "C" mis_status mis_smartturn_init_synthetic(mis_smartturn* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    const int64_t d = c->d, f = c->ffn, nm = c->nmel;
    sw.put("encoder.conv1.weight", {d, 3, nm}, sqrt(3.0 / (3.0 * nm)), 0.0f); sw.put("encoder.conv1.bias", {d}, 0.05, 0.0f);
    sw.put("encoder.conv2.weight", {d, 3, d}, sqrt(3.0 / (3.0 * d)), 0.0f); sw.put("encoder.conv2.bias", {d}, 0.05, 0.0f);
    sw.put("encoder.embed_positions.weight", {(int64_t)c->cfg.max_source_positions, d}, 0.1, 0.0f);
    for (int li = 0; li < c->cfg.encoder_layers; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li);
        sw.norm(q + ".self_attn_layer_norm", d); sw.norm(q + ".final_layer_norm", d);
        sw.lin(q + ".self_attn.q_proj", d, d, true, 1.0); sw.lin(q + ".self_attn.k_proj", d, d, c->cfg.k_proj_bias != 0, 1.0);
        sw.lin(q + ".self_attn.v_proj", d, d, true, 1.0); sw.lin(q + ".self_attn.out_proj", d, d, true, 0.5);
        sw.lin(q + ".fc1", f, d, true, 1.0); sw.lin(q + ".fc2", d, f, true, 0.5);
    }
    sw.norm("encoder.layer_norm", d);
    sw.lin("pool_attention_0", ST_POOL_HID, d, true, 1.0); sw.lin("pool_attention_2", 1, ST_POOL_HID, true, 2.0);
    sw.lin("classifier_0", ST_POOL_HID, d, true, 1.0); sw.norm("classifier_1", ST_POOL_HID);
    sw.lin("classifier_4", ST_CLS_MID, ST_POOL_HID, true, 2.0); sw.lin("classifier_6", 1, ST_CLS_MID, true, 2.0);
    MIS_API_END
}

// ============================================================================ prepare
// the padded window of row b: sample i (0 <= i < W) is pcm[b][len - n + (i - (W - n))] for i >= W - n, n = min(len, W), else 0
// (SmartTurnFeatures.swift:27-33: the tail of a long row, zeros in front of a short one)
__device__ __forceinline__ float st_window_sample(const float* __restrict__ row, int64_t len, int W, int i) {
    const int64_t n = len < (int64_t)W ? len : (int64_t)W;
    const int64_t lead = (int64_t)W - n;
    return (int64_t)i >= lead ? row[len - n + ((int64_t)i - lead)] : 0.0f;
}
// PASS 0: chunk sums; PASS 1: chunk sums of (x - mean)^2 with the mean taken as the ordered sum of the PASS 0 partials (:36-40)
template <int PASS>
__global__ void __launch_bounds__(256) k_st_stat_partial(const float* __restrict__ pcm, int64_t stride, const int64_t* __restrict__ lens, int W,
                                                         const float* __restrict__ sums, float* __restrict__ out, int nch) {
    __shared__ float red[4];
    const int b = blockIdx.y, ch = blockIdx.x;
    const int lo = ch * ST_CHUNK, hi = min(lo + ST_CHUNK, W);
    float mean = 0.0f;
    if (PASS == 1) {
        float s = 0.0f;
        for (int i = 0; i < nch; ++i) s += sums[b * nch + i];
        mean = s / (float)W;
    }
    const float* row = pcm + (int64_t)b * stride;
    const int64_t len = lens[b];
    float acc = 0.0f;
    for (int i = lo + threadIdx.x; i < hi; i += 256) { const float v = st_window_sample(row, len, W, i) - mean; acc += PASS == 1 ? v * v : v; }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[b * nch + ch] = (red[0] + red[1]) + (red[2] + red[3]);
}
// out[b][i] = (x - mean) / max(sqrt(var), 1e-7) (:41-42), or the window as it is
__global__ void __launch_bounds__(256) k_st_prepare(const float* __restrict__ pcm, int64_t stride, const int64_t* __restrict__ lens, int W,
                                                    const float* __restrict__ sums, const float* __restrict__ sq, int nch, int normalize,
                                                    float* __restrict__ out) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= W) return;
    float v = st_window_sample(pcm + (int64_t)b * stride, lens[b], W, i);
    if (normalize) {
        float s = 0.0f, q = 0.0f;
        for (int k = 0; k < nch; ++k) { s += sums[b * nch + k]; q += sq[b * nch + k]; }
        const float mean = s / (float)W;
        const float sd = fmaxf(sqrtf(q / (float)W), 1e-7f);
        v = (v - mean) / sd;
    }
    out[(size_t)b * W + i] = v;
}

// ============================================================================ stem hand-off
// out[(b F + t)][k C + c] = T(in[b][t + k - 1][c]) (zero outside the row and in the columns 3 C .. K1 - 1): Conv1d k 3 pad 1 patches
__global__ void __launch_bounds__(256) k_st_patches(const float* __restrict__ in, bf16_t* __restrict__ out, int Fr, int C, int K1, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int col = (int)(i % K1);
    const size_t r = i / K1;
    const int t = (int)(r % Fr);
    const size_t b = r / Fr;
    float v = 0.0f;
    if (col < 3 * C) {
        const int k = col / C, ch = col - k * C, ti = t + k - 1;
        if (ti >= 0 && ti < Fr) v = in[(b * Fr + ti) * C + ch];
    }
    out[i] = f32_to_bf16(v);
}
// features [B][C][F] (the layout SmartTurnModel.callAsFunction takes) -> [B][F][C]
__global__ void __launch_bounds__(256) k_st_features_to_nlc(const float* __restrict__ in, float* __restrict__ out, int Fr, int C, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % C);
    const size_t r = i / C;
    const int t = (int)(r % Fr);
    const size_t b = r / Fr;
    out[i] = in[(b * C + ch) * Fr + t];
}

// ============================================================================ pool + classifier head (f32)
__device__ __forceinline__ float st_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }     // MLX gelu: exact erf
// sum over the block's 256 threads in a fixed order; every thread gets the total.  `red` holds 4 floats.
__device__ __forceinline__ float st_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                                   // (the previous use of red is over)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float st_block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// s[b][t] = w2 . tanh(W0 h_t + b0) + b2 (SmartTurn.swift:187).  grid (ceil(T / 8), B); a thread is one of the 256 hidden units and keeps
// 8 positions in registers; the 8 rows of h sit in LDS as f32 and are read as broadcasts.
__global__ void __launch_bounds__(ST_POOL_HID) k_st_pool_scores(const bf16_t* __restrict__ h, int T, int d, const float* __restrict__ w0T,
                                                                const float* __restrict__ b0, const float* __restrict__ w2,
                                                                const float* __restrict__ b2, float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float hs[];        // [ST_TS][d]
    __shared__ float red[4];
    const int b = blockIdx.y, t0 = blockIdx.x * ST_TS, j = threadIdx.x;
    for (int i = j; i < ST_TS * d; i += ST_POOL_HID) {
        const int r = i / d, t = t0 + r;
        hs[i] = t < T ? bf16_to_f32(h[((size_t)b * T + t) * d + (i - r * d)]) : 0.0f;
    }
    __syncthreads();
    float acc[ST_TS];
#pragma unroll
    for (int r = 0; r < ST_TS; ++r) acc[r] = 0.0f;
#pragma unroll 4
    for (int k = 0; k < d; ++k) {
        const float w = w0T[(size_t)k * ST_POOL_HID + j];
#pragma unroll
        for (int r = 0; r < ST_TS; ++r) acc[r] = fmaf(w, hs[r * d + k], acc[r]);
    }
    const float bj = b0[j], wj = w2[j], bb = b2[0];
#pragma unroll
    for (int r = 0; r < ST_TS; ++r) {
        const float s = st_block_sum(wj * tanhf(acc[r] + bj), red);
        if (j == 0 && t0 + r < T) scores[(size_t)b * T + t0 + r] = s + bb;
    }
}

// the rest of the head (:188-201), one block of 256 threads per row:
//   a = softmax_t(s), pooled = sum_t a_t h_t, x = GELU(LayerNorm(W_c0 pooled + b)), y = GELU(W_c4 x + b), logit = w_c6 . y + b,
//   probability = sigmoid(logit), prediction = probability > threshold (:261-262)
struct StHeadParams {
    const bf16_t* h; const float* scores; int T, d;
    const float *c0wT, *c0b, *n1w, *n1b, *c4wT, *c4b, *c6w, *c6b, *thr;
    float *pooled, *logit, *prob; int32_t* pred;
};
__global__ void __launch_bounds__(ST_POOL_HID) k_st_pool_head(StHeadParams p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];        // a[T] | pooled[d] | partial sums [4][d]
    __shared__ float red[4];
    __shared__ float xs[ST_POOL_HID];
    __shared__ float ys[ST_CLS_MID];
    float* a = sm;
    float* pl = sm + p.T;
    float* part = pl + p.d;
    const int b = blockIdx.x, j = threadIdx.x, T = p.T, d = p.d;
    float mx = -INFINITY;
    for (int t = j; t < T; t += ST_POOL_HID) { const float s = p.scores[(size_t)b * T + t]; a[t] = s; mx = fmaxf(mx, s); }
    mx = st_block_max(mx, red);
    float sum = 0.0f;
    for (int t = j; t < T; t += ST_POOL_HID) { const float e = expf(a[t] - mx); a[t] = e; sum += e; }
    sum = st_block_sum(sum, red);
    for (int t = j; t < T; t += ST_POOL_HID) a[t] = a[t] / sum;
    __syncthreads();
    // pooled: a wave takes every fourth position, a lane two neighbouring channels of a 128-channel slice; the four partial sums meet
    // in LDS in a fixed order
    const int w = j >> 6, lane = j & 63;
    for (int c0 = 0; c0 < d; c0 += 128) {
        const int ch = c0 + lane * 2;
        if (ch >= d) continue;                                         // (d is even: ch + 1 < d)
        const bf16_t* hp = p.h + (size_t)b * T * d + ch;
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll 8
        for (int t = w; t < T; t += 4) {
            const uint32_t u = *reinterpret_cast<const uint32_t*>(hp + (size_t)t * d);
            a0 = fmaf(a[t], bf16_to_f32((bf16_t)(u & 0xffffu)), a0);
            a1 = fmaf(a[t], bf16_to_f32((bf16_t)(u >> 16)), a1);
        }
        part[w * d + ch] = a0; part[w * d + ch + 1] = a1;
    }
    __syncthreads();
    for (int ch = j; ch < d; ch += ST_POOL_HID) {
        const float v = (part[ch] + part[d + ch]) + (part[2 * d + ch] + part[3 * d + ch]);
        pl[ch] = v;
        p.pooled[(size_t)b * d + ch] = v;
    }
    __syncthreads();
    float x = p.c0b[j];
#pragma unroll 8
    for (int k = 0; k < d; ++k) x = fmaf(p.c0wT[(size_t)k * ST_POOL_HID + j], pl[k], x);
    const float mean = st_block_sum(x, red) / (float)ST_POOL_HID;
    const float dv = x - mean;
    const float var = st_block_sum(dv * dv, red) / (float)ST_POOL_HID;
    xs[j] = st_gelu(dv / sqrtf(var + ST_LN_EPS) * p.n1w[j] + p.n1b[j]);
    __syncthreads();
    if (j < ST_CLS_MID) {
        float y = p.c4b[j];
        for (int k = 0; k < ST_POOL_HID; ++k) y = fmaf(p.c4wT[k * ST_CLS_MID + j], xs[k], y);
        ys[j] = st_gelu(y);
    }
    __syncthreads();
    if (j < 64) {
        const float lg = wave_sum(p.c6w[j] * ys[j]) + p.c6b[0];
        if (j == 0) {
            const float pr = 1.0f / (1.0f + expf(-lg));
            p.logit[b] = lg; p.prob[b] = pr; p.pred[b] = pr > p.thr[0] ? 1 : 0;
        }
    }
}

// ============================================================================ host
static void st_reserve(mis_smartturn* c, int batch) {
    if (batch <= c->cap) return;
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->graphs.clear();                                                // they hold the old addresses
    const size_t B = batch, M1 = B * c->F, M = B * c->T, d = c->d;
    c->prep.alloc(B * c->W); c->part0.alloc(B * c->nch); c->part1.alloc(B * c->nch); c->feat.alloc(M1 * c->nmel);
    c->lens.alloc(ST_MAX_BATCH); c->thr.alloc(1);
    c->col1.alloc(M1 * c->K1); c->h1.alloc(M1 * d); c->col2.alloc(M * 3 * d); c->h.alloc(M * d); c->x.alloc(M * d); c->qkv.alloc(M * 3 * d);
    c->att.alloc(M * d); c->ff.alloc(M * c->ffn); c->enc_out.alloc(M * d);
    const size_t kvn = B * c->H * c->Spad * c->D;
    c->kc.alloc(kvn); c->vc.alloc(kvn);
    HIP_CHECK(hipMemsetAsync(c->kc.p, 0, kvn * 2, c->stream));
    HIP_CHECK(hipMemsetAsync(c->vc.p, 0, kvn * 2, c->stream));
    c->scores.alloc(M); c->pooled.alloc(B * d); c->logit.alloc(B); c->prob.alloc(B); c->pred.alloc(B);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->cap = batch;
}

static int st_chain_launches(const mis_smartturn* c) { return 4 + 8 * (int)c->enc.layers.size() + 1 + 2; }

// features f32 [B][F][nmel] in c->feat -> logits; `mark`: an event recorded between the encoder and the head (plain launches only)
static void st_enqueue_chain(mis_smartturn* c, int B, hipEvent_t mark) {
    hipStream_t s = c->stream;
    const int d = c->d, T = c->T, Fr = c->F;
    const size_t n1 = (size_t)B * Fr * c->K1;
    hipLaunchKernelGGL(k_st_patches, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, c->feat.p, c->col1.p, Fr, c->nmel, c->K1, n1);
    // the encoder (:86-97, 137-142)
    const WhisperEncWork k{c->col1.p, c->h1.p, c->col2.p, c->h.p, c->x.p, c->qkv.p, c->att.p, c->ff.p, c->kc.p, c->vc.p};
    whisper_encoder_enqueue(c->enc, k, B, Fr, T, c->enc_out.p, s);
    if (mark) HIP_CHECK(hipEventRecord(mark, s));
    hipLaunchKernelGGL(k_st_pool_scores, dim3(cdiv(T, ST_TS), B), dim3(ST_POOL_HID), (size_t)ST_TS * d * 4, s, c->enc_out.p, T, d, c->p0wT, c->p0b,
                       c->p2w, c->p2b, c->scores.p);
    StHeadParams hp{c->enc_out.p, c->scores.p, T, d, c->c0wT, c->c0b, c->c1w, c->c1b, c->c4wT, c->c4b, c->c6w, c->c6b, c->thr.p,
                    c->pooled.p, c->logit.p, c->prob.p, c->pred.p};
    hipLaunchKernelGGL(k_st_pool_head, dim3(B), dim3(ST_POOL_HID), (size_t)(T + 5 * d) * 4, s, hp);
}

// runs the chain on c->feat: a replay of the batch size's graph, or plain launches under MIS_NO_GRAPH.  A batch size met for the first
// time runs the chain once with plain launches (launch-time attributes of the GEMM kernels are set outside a capture, and a bad launch
// is reported by name), then captures it.
static void st_run_chain(mis_smartturn* c, int B, float threshold) {
    hipStream_t s = c->stream;
    const float thr = threshold < 0.0f ? c->cfg.threshold : threshold;
    HIP_CHECK(hipMemcpyAsync(c->thr.p, &thr, 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));                               // (thr is a stack variable)
    const bool use_graph = getenv("MIS_NO_GRAPH") == nullptr;
    HIP_CHECK(hipEventRecord(c->ev[1], s));
    if (!use_graph) {
        st_enqueue_chain(c, B, c->ev[2]);
        HIP_CHECK(hipGetLastError());
        c->last_launches = st_chain_launches(c);
    } else {
        StepGraph& g = c->graphs[B];
        if (!g) {
            st_enqueue_chain(c, B, nullptr);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));
            g.capture(s, [&]() { st_enqueue_chain(c, B, nullptr); });
            HIP_CHECK(hipEventRecord(c->ev[1], s));
        }
        g.launch(s);
        c->last_launches = g.nodes();
    }
    HIP_CHECK(hipEventRecord(c->ev[3], s));
    HIP_CHECK(hipStreamSynchronize(s));
    c->last_batch = B;
    if (use_graph) { HIP_CHECK(hipEventElapsedTime(&c->ms_encoder, c->ev[1], c->ev[3])); c->ms_head = -1.0f; }
    else { HIP_CHECK(hipEventElapsedTime(&c->ms_encoder, c->ev[1], c->ev[2])); HIP_CHECK(hipEventElapsedTime(&c->ms_head, c->ev[2], c->ev[3])); }
}

static void st_copy_out(mis_smartturn* c, int B, float* probability, float* logit, int32_t* prediction) {
    if (probability) HIP_CHECK(hipMemcpy(probability, c->prob.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (logit) HIP_CHECK(hipMemcpy(logit, c->logit.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (prediction) HIP_CHECK(hipMemcpy(prediction, c->pred.p, (size_t)B * 4, hipMemcpyDeviceToHost));
}

extern "C" int mis_smartturn_launches(const mis_smartturn* c) { return c ? c->last_launches : 0; }

extern "C" mis_status mis_smartturn_predict(mis_smartturn* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float threshold,
                                            float* probability, float* logit, int32_t* prediction) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "Smart Turn model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= ST_MAX_BATCH, MIS_ERR_INVALID_INPUT, "batch must be 1..%d", ST_MAX_BATCH);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    MIS_REQUIRE(threshold <= 1.0f, MIS_ERR_INVALID_INPUT, "threshold must be a number, at most 1 (negative: the configuration's)");
    std::vector<int64_t> hl(batch, stride);
    if (lens) memcpy(hl.data(), lens, batch * sizeof(int64_t));
    for (int b = 0; b < batch; ++b)
        MIS_REQUIRE(hl[b] >= 1 && hl[b] <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples (1 .. the row stride %lld are served)", b,
                    (long long)hl[b], (long long)stride);
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    st_reserve(c, batch);
    c->pcm_in.alloc((size_t)batch * stride);
    HIP_CHECK(hipMemcpyAsync(c->pcm_in.p, pcm, (size_t)batch * stride * 4, hipMemcpyDefault, s));
    HIP_CHECK(hipMemcpyAsync(c->lens.p, hl.data(), (size_t)batch * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipEventRecord(c->ev[0], s));
    if (c->cfg.normalize_audio) {
        hipLaunchKernelGGL((k_st_stat_partial<0>), dim3(c->nch, batch), dim3(256), 0, s, c->pcm_in.p, stride, c->lens.p, c->W, nullptr, c->part0.p, c->nch);
        hipLaunchKernelGGL((k_st_stat_partial<1>), dim3(c->nch, batch), dim3(256), 0, s, c->pcm_in.p, stride, c->lens.p, c->W, c->part0.p, c->part1.p, c->nch);
    }
    hipLaunchKernelGGL(k_st_prepare, dim3(cdiv(c->W, 256), batch), dim3(256), 0, s, c->pcm_in.p, stride, c->lens.p, c->W, c->part0.p, c->part1.p, c->nch,
                       c->cfg.normalize_audio ? 1 : 0, c->prep.p);
    HIP_CHECK(hipGetLastError());
    mel_spectrogram_device(c->device, c->mel, c->prep.p, batch, c->W, c->feat.p, s);
    st_run_chain(c, batch, threshold);
    HIP_CHECK(hipEventElapsedTime(&c->ms_prepare, c->ev[0], c->ev[1]));
    st_copy_out(c, batch, probability, logit, prediction);
    MIS_API_END
}

extern "C" mis_status mis_smartturn_forward_features(mis_smartturn* c, const float* features, int batch, float* probability, float* logit) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && features, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "Smart Turn model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= ST_MAX_BATCH, MIS_ERR_INVALID_INPUT, "batch must be 1..%d", ST_MAX_BATCH);
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    st_reserve(c, batch);
    const size_t n = (size_t)batch * c->F * c->nmel;
    c->feat_in.alloc(n);                                              // (in front of the graph: no captured node holds it)
    HIP_CHECK(hipMemcpyAsync(c->feat_in.p, features, n * 4, hipMemcpyDefault, s));
    hipLaunchKernelGGL(k_st_features_to_nlc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c->feat_in.p, c->feat.p, c->F, c->nmel, n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    st_run_chain(c, batch, -1.0f);
    c->ms_prepare = 0.0f;
    st_copy_out(c, batch, probability, logit, nullptr);
    MIS_API_END
}

// tests: tensors of the last call.  stage 0 prepared samples [B, W], 1 features [B, F, n_mels], 2 encoder output [B, T, d], 3 pooled [B, d]
// (stage 0 is that of the last predict); out f32, `capacity` floats
extern "C" mis_status mis_debug_smartturn_tap(mis_smartturn* c, int stage, float* out, int64_t capacity) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && out && stage >= 0 && stage <= 3, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(c->last_batch > 0, MIS_ERR_INVALID_INPUT, "no call to tap");
    HIP_CHECK(hipSetDevice(c->device));
    const size_t B = c->last_batch;
    const size_t n = stage == 0 ? B * c->W : stage == 1 ? B * c->F * c->nmel : stage == 2 ? B * c->T * c->d : B * c->d;
    MIS_REQUIRE((int64_t)n <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    if (stage == 2) {
        DevBuf<float> o;
        o.alloc(n);
        launch_bf16_to_f32(c->enc_out.p, o.p, n, c->stream);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        HIP_CHECK(hipMemcpy(out, o.p, n * 4, hipMemcpyDeviceToHost));
    } else {
        const float* src = stage == 0 ? c->prep.p : stage == 1 ? c->feat.p : c->pooled.p;
        HIP_CHECK(hipMemcpy(out, src, n * 4, hipMemcpyDeviceToHost));
    }
    MIS_API_END
}

// measurements: device milliseconds of the last call - ms[0] prepare + mel, ms[1] encoder, ms[2] head.  Inside a graph replay the
// encoder and the head are one interval: ms[1] holds it and ms[2] is -1.
extern "C" mis_status mis_debug_smartturn_timing(const mis_smartturn* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && ms, MIS_ERR_INVALID_INPUT, "null argument");
    ms[0] = c->ms_prepare; ms[1] = c->ms_encoder; ms[2] = c->ms_head;
    MIS_API_END
}
