/*
 * mi_speech.h - C ABI of libmi_speech.so: MI355X-native (gfx950) kernels for the
 * TTS generate()/generateStream() + neural-codec hot path of Blaizzy/mlx-audio-swift.
 *
 * The reference has NO FFI: its boundary is Swift protocol conformance
 *   SpeechGenerationModel   Sources/MLXAudioTTS/Generation.swift:8-39
 *   AudioCodecModel         Sources/MLXAudioCodecs/AudioCodecModel.swift:4-27
 * implemented per model by classes whose arithmetic is MLX (un-vendored mlx-swift 0.31.4).
 * This header is what a thin Swift class conforming to those protocols binds instead of MLX
 * (see INTEGRATION.md for the Swift shim); every entry point cites the reference symbol it
 * replaces.  Plain C types only: pointers + sizes, no torch / MLX types.
 *
 * Pointer convention: every data pointer may be HOST or DEVICE memory of the handle's GPU
 * (copies use hipMemcpyDefault; unified addressing tells them apart).  Inputs are borrowed for
 * the duration of the call.  Library-allocated outputs are pinned host memory released with
 * mis_free().  No entry point aborts: failures return a status and set mis_last_error().
 * Threading: one in-flight call per handle; distinct handles are independent.
 */
#ifndef MI_SPEECH_H
#define MI_SPEECH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIS_ABI_VERSION 1

/* <-> AudioGenerationError, Sources/MLXAudioCore/Generation/GenerationTypes.swift:66-87 */
typedef enum {
    MIS_OK = 0,
    MIS_ERR_NOT_INITIALIZED = 1,   /* .modelNotInitialized */
    MIS_ERR_GENERATION_FAILED = 2, /* .generationFailed    */
    MIS_ERR_INVALID_INPUT = 3,     /* .invalidInput        */
    MIS_ERR_AUDIO_DECODE = 4,      /* .audioDecodingFailed */
    MIS_ERR_AUDIO_ENCODE = 5,      /* .audioEncodingFailed */
    MIS_ERR_CANCELLED = 6,         /* Task cancellation, LlamaTTS.swift:715,911 */
    MIS_ERR_DEVICE = 7             /* HIP runtime failure / no GPU */
} mis_status;

typedef enum { MIS_F32 = 0, MIS_F16 = 1, MIS_BF16 = 2, MIS_I32 = 3 } mis_dtype;

const char* mis_last_error(void);          /* thread-local message of the last failing call */
int         mis_abi_version(void);
void        mis_free(void* p);             /* releases library-allocated (pinned host) outputs */
int         mis_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Orpheus <-> SNAC token framing (integer-exact).
 * ---------------------------------------------------------------------------------------- */

/* llamaDecodeAudioFromCodes, LlamaTTS.swift:41-64: split 7-token frames into the three SNAC
 * levels.  codes7: [batch, 7*groups] values in [0, 7*4096); l0 [batch,groups], l1 [batch,2*groups],
 * l2 [batch,4*groups], values in [0,4096).  Runs on the GPU `device`. */
mis_status mis_orpheus_deinterleave(int device, const int32_t* codes7, int batch, int groups,
                                    int32_t* l0, int32_t* l1, int32_t* l2);

/* LlamaTTSModel.parseOutput, LlamaTTS.swift:383-434, per row (App. D.2 of SURVEY.md): crop after
 * the last start-of-speech (128257), drop end-of-speech (128258), trim to a multiple of 7, subtract
 * 128266.  ids: [batch, stride] with lens[batch] valid entries per row; codes_out: [batch, stride];
 * n_codes_out: [batch]. */
mis_status mis_speech_parse_output(int device, const int32_t* ids, const int32_t* lens, int batch, int stride, int32_t* codes_out,
                                   int32_t* n_codes_out, int start_of_speech, int end_of_speech, int audio_token_offset,
                                   int start_of_ai);     /* explicit ids (VyvoTTS); start_of_ai < 0: no fallback */
mis_status mis_orpheus_parse_output(int device, const int32_t* ids, const int32_t* lens, int batch,
                                    int stride, int32_t* codes_out, int32_t* n_codes_out);

/* ------------------------------------------------------------------------------------------
 * SNAC codec (decode path).   Replaces class SNAC, Sources/MLXAudioCodecs/SNAC/SNACDecoder.swift.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_snac mis_snac;

/* SNACConfig, SNAC/Config.swift:10-37 (decode-relevant fields) */
typedef struct {
    int32_t sampling_rate;
    int32_t latent_dim;        /* = encoder_dim * 2^len(encoder_rates), SNACDecoder.swift:50 */
    int32_t decoder_dim;
    int32_t n_decoder_rates;   /* <= 8 */
    int32_t decoder_rates[8];
    int32_t codebook_size;
    int32_t codebook_dim;
    int32_t n_codebooks;       /* <= 8 */
    int32_t vq_strides[8];
    int32_t noise;             /* bool */
    int32_t depthwise;         /* bool; only 1 is supported (24 kHz model) */
    int32_t attn_window_size;  /* 0 = none (24 kHz model); 32: LocalMHA of the 32 / 44 kHz models (SNAC/Attention.swift; <= 64) */
} mis_snac_config;

/* SNAC.fromModelDirectory, SNACDecoder.swift:156-189: config.json + model.safetensors */
mis_status mis_snac_load(const char* model_dir, int device, mis_snac** out);
/* programmatic construction (tests / hosts that already hold the arrays) */
mis_status mis_snac_create(const mis_snac_config* cfg, int device, mis_snac** out);
/* one tensor in the reference's key layout, e.g.
 * "decoder.model.layers.1.weight_v"; dtype F32/F16/BF16; shape as stored. */
mis_status mis_snac_set_tensor(mis_snac*, const char* name, const void* data, mis_dtype dtype,
                               const int64_t* shape, int ndim);
/* update(parameters:verify:.all), SNACDecoder.swift:185: every decoder/quantizer key must be
 * present; folds weight-norm (Layers.swift:35-42,102-103,166) and builds device tables. */
mis_status mis_snac_finalize(mis_snac*);
void       mis_snac_destroy(mis_snac*);
/* number of samples decode() produces for t_coarse entries of codes[0] */
int64_t    mis_snac_num_samples(const mis_snac*, int t_coarse);
/* length of NoiseBlock i's input (i < n_decoder_rates) for t_coarse */
int64_t    mis_snac_noise_len(const mis_snac*, int block, int t_coarse);

/* NoiseBlock policy when a decode is given noise == NULL: null_noise_is_zero = 0 (default, the
 * reference's behaviour: x + N(0,1)[B,1,T] * conv(x), Layers.swift:270-278) draws the noise on the
 * device from the documented counter generator keyed by (seed, block, global row, t);
 * null_noise_is_zero = 1 adds nothing (deterministic decode). */
mis_status mis_snac_set_noise(mis_snac*, int null_noise_is_zero, uint64_t seed);

/* SNAC.decode / decodeAudio, SNACDecoder.swift:127-131,201-203 (fromCodes VQ.swift:165-191 +
 * Decoder Layers.swift:364-421).  codes[i]: int32 [batch, t_coarse * vq_strides[0]/vq_strides[i]];
 * noise: NULL (see mis_snac_set_noise) or n_decoder_rates pointers to f32 [batch, noise_len(i)]
 * standing in for MLXRandom.normal (Layers.swift:274); pcm_out: f32 [batch, num_samples]. */
mis_status mis_snac_decode(mis_snac*, const int32_t* const* codes, int batch, int t_coarse,
                           const float* const* noise, float* pcm_out);
/* debug/parity taps: copy an intermediate ("zq","stem_dw","stem_pw","block0".."blockN") of the
 * LAST decode into out (f32 [batch, C, T]); returns its C and T. */
/* encode path (SNAC.encode, SNACDecoder.swift:86-125: preprocess right-pad -> Encoder (Layers.swift:319-360) -> residual VQ with
 * nearest normalised code, VQ.swift:47-163).  Available when the checkpoint's "encoder.*" tensors were loaded (depthwise
 * configs without LocalMHA, i.e. snac_24khz).  padded_length = n rounded up to hop * lcm(vq_strides). */
int64_t    mis_snac_padded_length(const mis_snac*, int64_t n_samples);
/* audio f32 [batch, n_samples]; codes_out[i] int32 [batch, padded / hop / vq_strides[i]]; z_out (nullable) f32
 * [batch, latent_dim, padded / hop] = encoder output before quantisation */
mis_status mis_snac_encode(mis_snac*, const float* audio, int batch, int64_t n_samples, int32_t* const* codes_out, float* z_out);
mis_status mis_snac_debug_tap(mis_snac*, const char* name, float* out, int64_t capacity,
                              int32_t* channels, int64_t* length);

/* ------------------------------------------------------------------------------------------
 * Orpheus / Llama token LM + TTS generate.  Replaces LlamaTTSModel, LlamaTTS.swift:354-977.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_tts mis_tts;

/* LlamaTTSConfiguration, LlamaTTSConfig.swift:15-61 */
typedef struct {
    int32_t hidden_size, num_hidden_layers, intermediate_size;
    int32_t num_attention_heads, num_key_value_heads, head_dim;
    int32_t vocab_size;
    float   rms_norm_eps;
    float   rope_theta;
    /* llama3 rope scaling, LlamaTTS.swift:111-186 (defaults 32 / 1 / 4 / 8192) */
    float   rope_factor, rope_low_freq_factor, rope_high_freq_factor, rope_original_max_pos;
    int32_t tie_word_embeddings;
    int32_t sample_rate;
    /* Qwen3-style variants (Soprano Soprano.swift:24-97, VyvoTTS Qwen3.swift:204-205): per-head RMSNorm of q and k
     * before RoPE (weights model.layers.N.self_attn.{q,k}_norm.weight [head_dim]) and plain RoPE(base) without the
     * llama3 rescale.  Both 0 for Orpheus (LlamaTTS.swift always builds Llama3ScaledRoPE, :161-186). */
    int32_t qk_norm;
    int32_t rope_plain;
    /* Qwen3-TTS talker / code predictor write the rotation as array ops in the model dtype (cos/sin cast to bf16,
     * T(T(x*cos) + T(rotate_half(x)*sin)), Qwen3TTSTalker.swift:15-24,92-95) instead of MLXFast.RoPE */
    int32_t rope_ops_in_dtype;
    /* speech token ids of the generate loop (0 = Orpheus: 128257 / 128258 / 128266, LlamaTTS.swift:20-30).  VyvoTTS
     * (Qwen3.swift:19-29): start_of_speech 151670, end_of_speech 151671, audio_token_offset 151679, start_of_ai 151674
     * (parse fallback, :332-358; 0 = none) */
    int32_t start_of_speech_id, end_of_speech_id, audio_token_offset, start_of_ai_id;
    /* SNAC decode granularity of generate(): 0 = the whole utterance in one decode (LlamaTTS.swift:759).  VyvoTTS decodes
     * INDEPENDENT chunks of 50 code groups and concatenates the samples (decodeAudioFromCodes, Qwen3.swift:47-83; nothing is
     * carried across a chunk boundary, so the waveform differs from a single decode near every boundary) */
    int32_t codec_chunk_groups;
} mis_lm_config;

/* GenerateParameters as used by LlamaTTS.swift:573-581,691-696 (mlx-swift-lm) */
typedef struct {
    int32_t  max_tokens;           /* default 1200 */
    float    temperature;          /* 0 => greedy argmax */
    float    top_p;                /* outside (0,1) => no nucleus cut */
    float    repetition_penalty;   /* <= 0 or 1 => off */
    int32_t  repetition_context;   /* default 20 */
    uint64_t seed;                 /* mis-sampler-v1 RNG key (see csrc/lm_sampler.hip) */
    int32_t  frame_constrained;    /* 0 normal. 1 (synthetic-weight benches): step i may only emit
                                      128266 + (i%7)*4096 + [0,4096); EOS can then never be sampled; the
                                      sampler only visits that range (k_samp_narrow).  2: the same
                                      constraint through the FULL-vocabulary sampler (every id visited,
                                      masked ones get zero mass) - the code path of an unconstrained
                                      checkpoint, with tokens that still form valid frames */
    int64_t  row_offset;           /* global index of row 0 (RNG keyed by global row => sharding-invariant) */
    int32_t  sampler_flavor;       /* 0 mlx-lm processor/sampler (Orpheus).  1 Soprano streamGenerate (Soprano.swift:801-901):
                                      penalty window = generated tokens only, applied per occurrence in float32; the reference's
                                      TopPSampler thresholds UNNORMALISED exp(logit) sums (:1003-1036) and so only ever drops
                                      tokens of vanishing mass - this flavour keeps them (top_p is ignored) */
    int32_t  reserved;
} mis_gen_params;

/* AudioGeneration events, GenerationTypes.swift:50-61 */
typedef enum { MIS_EVENT_TOKEN = 0, MIS_EVENT_INFO = 1, MIS_EVENT_AUDIO = 2 } mis_event_kind;
/* AudioGenerationInfo, GenerationTypes.swift:14-45 */
typedef struct {
    int32_t prompt_token_count, generation_token_count;
    double  prefill_time, generate_time, tokens_per_second, peak_memory_gb;
} mis_gen_info;
/* payload: TOKEN -> const int32_t* (n=1); INFO -> const mis_gen_info* (n=1); AUDIO -> const float* (n samples) */
typedef void (*mis_event_cb)(void* user, int row, mis_event_kind kind, const void* payload, int64_t n);

/* LlamaTTSModel.fromModelDirectory, LlamaTTS.swift:942-977: config.json + *.safetensors of the LM;
 * codec is borrowed (post_load_hook loads SNAC separately, :595-602). */
mis_status mis_tts_load(const char* model_dir, mis_snac* codec, int device, mis_tts** out);
mis_status mis_tts_create(const mis_lm_config* cfg, mis_snac* codec /* may be NULL */, int device, mis_tts** out);
/* HF/MLX key layout: model.embed_tokens.weight, model.layers.N.*, model.norm.weight, [lm_head.weight] */
mis_status mis_tts_set_tensor(mis_tts*, const char* name, const void* data, mis_dtype dtype,
                              const int64_t* shape, int ndim);
/* fills every weight on the device with the documented generator "mis-synth-v1"
 * (oracle/synth.py has the same formula); benches only - there are no checkpoints offline. */
/* Linear / Embedding in MLX's affine-quantised form (mlx quantize [3P]): wq uint32 [N, K*bits/32] (element i of a row =
 * (word[i / (32/bits)] >> (bits * (i % (32/bits)))) & mask), scales / biases [N, K/group_size] of dtype sb_dtype;
 * w = scale * q + bias.  The reference keeps QuantizedLinear (LlamaTTS.swift:958-968, Qwen3TTS.swift:1157-1170) and never
 * materialises the weight: quantizedMatmul applies scale and bias to float32 group sums.  So does the engine for a role
 * (q|k|v, o_proj, gate|up, down_proj, lm_head) whose matrices ALL arrive with 8 or 4 bits, group size 64 and bf16 scales: the
 * codes are streamed as stored (0.53x / 0.28x of the bf16 bytes) and dequantised in registers (csrc/lm_qgemm.hip).  Any other
 * combination (2 bit, other groups, f16 / f32 scales, per-layer overrides inside a role, MIS_QUANT_NATIVE=0) is dequantised once at
 * load into the bf16 layout, which rounds s*q+b to bf16 per weight - a stated deviation for those cases only.  The embedding
 * (QuantizedEmbedding: a gather of dequantised rows in the model dtype) is always dequantised at load. */
mis_status mis_tts_set_tensor_quantized(mis_tts*, const char* name, const uint32_t* wq, const void* scales, const void* biases,
                                        mis_dtype sb_dtype, int64_t N, int64_t K, int group_size, int bits);
/* after finalize: bits of the quantised form a role is streamed in (0 = dense bf16); role 0 q|k|v, 1 o_proj, 2 gate|up, 3 down, 4 lm_head */
int        mis_tts_native_quant_bits(const mis_tts*, int role);
/* benches: every Linear as a synthetic MLX-quantised matrix (bits 8 or 4, group 64, bf16 scales) - no checkpoints offline */
mis_status mis_tts_init_synthetic_quantized(mis_tts*, uint64_t seed, int bits);
mis_status mis_tts_init_synthetic(mis_tts*, uint64_t seed);
mis_status mis_tts_finalize(mis_tts*);     /* verify all keys present; pack weights for MFMA streaming */
void       mis_tts_destroy(mis_tts*);

/* LM-only taps (parity tests, teacher forcing).  reset: new batch, empty KV caches (makeCache,
 * LlamaTTS.swift:604-608).  forward: ONE token per active row through the model
 * (LlamaTTSModel.callAsFunction :557-567 with L=1 and cache), logits_out f32 [batch, vocab]
 * (bf16 values, widened) or NULL. */
mis_status mis_lm_reset(mis_tts*, int batch, int max_context);
/* the prefill call of the reference loop, `model(inputIds, cache:)` (LlamaTTS.swift:711): ragged prompts (flat ids + lens) through
 * the model with empty caches as ONE [positions x rows] pass of MFMA GEMMs (csrc/lm_prefill.hip) - position by position only for
 * natively quantised roles or MIS_PREFILL_SEQ=1.  logits_out f32 [batch, vocab] (nullable): the next-token logits of every row;
 * hidden_out f32 [batch, hidden] (nullable): model.norm(h) of every row's last prompt token (Soprano's first decoder input,
 * Soprano.swift:824-825).  The caches then hold the prompts; mis_lm_forward continues behind them.  mis_tts_generate* prefill the
 * same way. */
mis_status mis_lm_prefill(mis_tts*, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch, int max_context,
                          float* logits_out, float* hidden_out);
mis_status mis_lm_forward(mis_tts*, const int32_t* ids, const uint8_t* active, float* logits_out);
/* same, also returning model.norm(h) of the fed token: hidden_out f32 [batch, hidden_size] (Soprano decodes these,
 * Soprano.swift:254-275); either output may be NULL */
mis_status mis_lm_forward_hidden(mis_tts*, const int32_t* ids, const uint8_t* active, float* logits_out, float* hidden_out);
/* processor + sampler of the generate loop (LlamaTTS.swift:717-721) on caller-provided logits:
 * logits f32 [batch, vocab]; window [batch, ctx] (ids, right-aligned valid part = window_len[b]);
 * lo/hi: optional allowed id range (hi<=0 => vocab); tokens_out [batch].  mis-sampler-v1.
 * Wide ranges run in ONE launch whose 8 blocks per row wait for each other (bounded spins); if a row's blocks were not all resident
 * (another stream holding CUs) the time-out is detected after the launch and the call falls back to the multi-launch path on fresh
 * inputs - the tokens are the same.  Inside mis_*_generate* (a captured graph) the same condition is reported as
 * MIS_ERR_GENERATION_FAILED after the decode loop; MIS_SAMPLER_WIDE=1 selects the multi-launch path for such deployments. */
mis_status mis_sample_logits(int device, const float* logits, int batch, int vocab,
                             const int32_t* window, const int32_t* window_len, int ctx,
                             const mis_gen_params* params, int step, int lo, int hi,
                             int32_t* tokens_out);

/* generate(text:voice:...) LlamaTTS.swift:658-765 for a BATCH of already-tokenised prompts
 * (tokenisation stays on the host side: prepareInputIds :446-553 / swift-transformers).
 * prompt_ids: concatenated rows; prompt_lens[batch].  snac_noise: NULL (N(0,1) drawn on the device,
 * keyed by params->seed and the global row) or explicit noise as in mis_snac_decode (then every row
 * must produce the same number of frames).  Outputs (library-allocated, mis_free):
 * *pcm_out f32 [batch, *pcm_stride] with pcm_lens[batch] valid samples per row;
 * *tokens_out (optional, may be NULL) int32 [batch, *tokens_stride] generated ids (EOS included
 * when sampled, as in the .token stream :862-866), n_tokens[batch]. */
mis_status mis_tts_generate(mis_tts*, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch,
                            const mis_gen_params* params, const float* const* snac_noise,
                            float** pcm_out, int64_t* pcm_stride, int64_t* pcm_lens,
                            int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens);
/* Same, leaving PCM resident in HBM: pcm_dev f32 [batch, pcm_stride] caller-allocated DEVICE memory
 * (pcm_stride >= num_samples for max_tokens/7 groups).  What bench.py times. */
mis_status mis_tts_generate_device(mis_tts*, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch,
                                   const mis_gen_params* params, const float* const* snac_noise,
                                   float* pcm_dev, int64_t pcm_stride, int64_t* pcm_lens, int32_t* n_tokens);
/* generateStream(...) LlamaTTS.swift:777-913: .token per step and row, then per row .info and ONE
 * final .audio (Orpheus does not stream audio chunks, :893-904).  cancel_flag polled per step. */
mis_status mis_tts_generate_stream(mis_tts*, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch,
                                   const mis_gen_params* params, const float* const* snac_noise,
                                   mis_event_cb on_event, void* user, const volatile int* cancel_flag);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: utterance-batch data parallelism behind the boundary (the reference is single-device and has
 * no counterpart).  Rows are independent units; every GPU holds a full replica of the weights (the host loads one mis_tts per
 * device, exactly as it loads one); a batch is cut into contiguous row blocks (mis_shard_rows); the sampler / codec-noise RNG is
 * keyed by the GLOBAL row index (row_offset), so every row's tokens and samples are independent of the number of shards; the only
 * exchange is ONE all-gather of the decoded PCM (+ lengths) at the end.
 * ---------------------------------------------------------------------------------------- */
/* contiguous block [*lo, *hi) of `rank` among `world` shards; block sizes differ by at most one row */
void mis_shard_rows(int n_rows, int rank, int world, int* lo, int* hi);

/* (1) SINGLE PROCESS, N devices (a Swift host): a group of replicas - one finalized mis_tts (with its own codec) per device;
 * devices may repeat (logical shards of one GPU).  The group borrows the handles. */
typedef struct mis_group mis_group;
typedef struct { int32_t n_shards; double generate_ms, slowest_shard_ms, gather_ms; } mis_group_timing;
mis_status mis_tts_group_create(mis_tts* const* replicas, int n, mis_group** out);
void       mis_tts_group_destroy(mis_group*);
int        mis_tts_group_size(const mis_group*);
/* mis_tts_generate over the group: one worker thread + stream per replica, each generating its block with row_offset advanced by
 * the block start; outputs as mis_tts_generate (rows in batch order, one pinned host buffer) - identical, bit for bit, to the
 * single-handle call. */
mis_status mis_tts_group_generate(mis_group*, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch,
                                  const mis_gen_params* params, float** pcm_out, int64_t* pcm_stride, int64_t* pcm_lens,
                                  int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens);
/* PCM left in HBM and all-gathered: pcm_dev[i] = replica i's DEVICE buffer [batch, pcm_stride] on its own GPU; on return every
 * buffer holds every row (each replica writes its block into every peer's buffer over xGMI: direct peer copies). */
mis_status mis_tts_group_generate_device(mis_group*, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch,
                                         const mis_gen_params* params, float* const* pcm_dev, int64_t pcm_stride,
                                         int64_t* pcm_lens, int32_t* n_tokens);
mis_status mis_tts_group_last_timing(mis_group*, mis_group_timing* out);

/* (2) ONE PROCESS PER GPU (any launcher; what bench.py --gpus N runs): an RCCL communicator behind the ABI.  Rank 0 obtains a
 * 128-byte id (ncclUniqueId), the host distributes it to the other ranks by whatever means it has, every rank creates its
 * communicator, generates its block with mis_tts_generate_device(row_offset = block start) and calls the all-gather:
 * pcm_local_dev [rows_local, stride] -> pcm_all_dev [world * rows_local, stride] (device), lens (host) likewise; RCCL
 * ncclAllGather over xGMI on the communicator's stream; *gather_ms (nullable) = device time of the exchange. */
typedef struct mis_comm mis_comm;
#define MIS_COMM_ID_BYTES 128
mis_status mis_comm_unique_id(void* id_out /* MIS_COMM_ID_BYTES */);
mis_status mis_comm_create(int device, int rank, int world, const void* unique_id, mis_comm** out);
void       mis_comm_destroy(mis_comm*);
mis_status mis_comm_all_gather_pcm(mis_comm*, const float* pcm_local_dev, const int64_t* lens_local, int rows_local,
                                   int64_t stride, float* pcm_all_dev, int64_t* lens_all, double* gather_ms);

/* per-phase device timings of the last generate (ms): [0]=prefill [1]=decode loop [2]=parse+codec,
 * plus average duration (ms) and launch count of the dominant GEMM kernel measured with HIP events
 * on the library's own stream when profiling is enabled with mis_tts_set_profiling(ctx, 1). */
typedef struct {
    double prefill_ms, decode_ms, codec_ms;
    double step_ms_avg;            /* decode_ms / steps */
    int32_t steps;
    double gemm_probe_ms;          /* avg duration of ONE lm_head GEMM launch (HIP events), 0 if off */
    double gemm_probe_bytes;       /* algorithmic bytes of that launch */
    double hbm_bytes_per_step;     /* algorithmic bytes per decode step: weights + KV read */
} mis_tts_timing;
mis_status mis_tts_set_profiling(mis_tts*, int enabled);
mis_status mis_tts_last_timing(mis_tts*, mis_tts_timing* out);
/* time `iters` launches of one kernel of the decode step in isolation (HIP events on the library stream), rotating over the
 * layers so the Infinity Cache cannot serve the operands: which = 0 qkv, 1 o_proj, 2 gate_up, 3 down, 4 lm_head (weight-streaming
 * GEMMs), 5 decode attention at context 368 (the C3 mean; bytes = K/V rows read), 6 the slab-reduce + residual + RMSNorm kernel.
 * avg_ms and the algorithmic bytes of one launch are returned.  Used by bench.py for the roofline object. */
mis_status mis_tts_time_gemm(mis_tts*, int which, int batch, int iters, double* avg_ms, double* bytes);

/* ------------------------------------------------------------------------------------------
 * Soprano TTS.  Replaces SopranoModel / SopranoDecoder (Sources/MLXAudioTTS/Models/Soprano/Soprano.swift:201-690,
 * SopranoDecoder.swift:225-284, Vocos backbone Sources/MLXAudioCodecs/Vocos/VocosBackbone.swift:109-204).
 * Text splitting / cleaning / tokenisation stay on the host (TextUtils.swift).
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_soprano mis_soprano;
/* SopranoConfiguration, SopranoConfig.swift:103-167 */
typedef struct {
    mis_lm_config lm;              /* qk_norm / rope_plain are forced on (SopranoAttention) */
    int32_t decoder_num_layers, decoder_dim, decoder_intermediate_dim;
    int32_t hop_length, n_fft, upscale, input_kernel, dw_kernel, token_size;
    int32_t stop_token_id;         /* "[STOP]" (Soprano.swift:855) */
} mis_soprano_config;
mis_status mis_soprano_create(const mis_soprano_config*, int device, mis_soprano** out);
/* checkpoint keys as stored; SopranoModel.sanitize (Soprano.swift:314-361) is applied: "decoder.*" -> float32 decoder
 * weights, everything else -> the token LM (model.* / lm_head.weight) */
mis_status mis_soprano_set_tensor(mis_soprano*, const char* name, const void* data, mis_dtype dtype,
                                  const int64_t* shape, int ndim);
/* A Linear in MLX's affine-quantised form (SopranoModel.fromPretrained quantises every module with a `.scales` companion,
 * Soprano.swift:949-963), with the format and validation of mis_tts_set_tensor_quantized; `name` is the .weight key, sanitised as
 * above.  LM keys go to the token LM, which streams a role's codes or dequantises them at load as mis_tts_set_tensor_quantized says.
 * Decoder keys (decoder.decoder.convnext.N.pwconv1 / pwconv2, decoder.head.out) are dequantised once at load to float32 (s*q+b in
 * float32) into the decoder's layouts: a stated deviation - the reference runs quantizedMatmul on float32 activations, this differs
 * from it in summation order only. */
mis_status mis_soprano_set_tensor_quantized(mis_soprano*, const char* name, const uint32_t* wq, const void* scales, const void* biases,
                                            mis_dtype sb_dtype, int64_t N, int64_t K, int group_size, int bits);
mis_status mis_soprano_finalize(mis_soprano*);
void       mis_soprano_destroy(mis_soprano*);
mis_tts*   mis_soprano_lm(mis_soprano*);                 /* borrowed handle of the token LM (taps, synthetic init) */
int64_t    mis_soprano_num_samples(const mis_soprano*, int n_hidden);   /* (upscale*(n-1)) * hop_length */
/* SopranoDecoder.callAsFunction: hidden f32 [batch, L, hidden_size] -> audio f32 [batch, num_samples(L)] */
mis_status mis_soprano_decode(mis_soprano*, const float* hidden, int batch, int L, float* audio_out);
/* generate for a batch of tokenised sentences: outputs as mis_tts_generate (pcm rows padded to the longest).  One row runs on the batch-1
 * token engine wherever mis_soprano_lm_path below says so - bf16 checkpoints and 8 / 4-bit quantised ones of the engine's widths alike. */
mis_status mis_soprano_generate(mis_soprano*, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch,
                                const mis_gen_params* params, float** pcm_out, int64_t* pcm_stride, int64_t* pcm_lens,
                                int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens);
/* Which program ran the LM loop of the handle's LAST generate / generateStream call: 0 = the launch chain, chosen by rule; 1 = the batch-1
 * token engine (one persistent launch; chosen by rule: a ONE-row request - over all shards of a group call - on a checkpoint of
 * Soprano-80M's widths that is bf16 or MLX-quantised with q|k|v, o_proj, gate|up and down_proj all streamed as codes of ONE width,
 * 8 or 4 bit (mis_tts_native_quant_bits; the output projection dense or of the same width), device of 8 XCDs x 32 compute units not
 * shared with another replica, prompt + max_tokens <= 1024, repetition context <= 64; MIS_TOKEN_ENGINE=0 disables it); 2 = the launch
 * chain AFTER the engine's workers could not be made
 * co-resident (another stream held compute units; also written to stderr).  The two programs round at the same points but sum in other
 * orders: ids can differ on near-ties, so the choice never depends on stream vs non-stream, only on the request (and, reported, on 2). */
int32_t    mis_soprano_lm_path(const mis_soprano*);
/* generateStream (Soprano.swift:693-800) for a batch of tokenised sentences: MIS_EVENT_TOKEN per sampled id while the loop runs
 * (the [STOP] token is not announced, :855-857), then per row MIS_EVENT_INFO (SopranoGenerationInfo :771-779: prompt count and
 * prefill time 0, generation count = hidden states decoded) and ONE MIS_EVENT_AUDIO (:781).  cancel_flag polled every 8 steps
 * (token engine: every ~20 us, honoured at the launch's next position) (continuation.onTermination -> task.cancel(), :798)
 * -> MIS_ERR_CANCELLED.  At one row the events are fired while ONE persistent launch runs (csrc/token_engine.hip): the ids arrive in
 * host-visible memory, the calling thread polls them. */
mis_status mis_soprano_generate_stream(mis_soprano*, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch,
                                       const mis_gen_params* params, mis_event_cb on_event, void* user,
                                       const volatile int* cancel_flag);

/* ------------------------------------------------------------------------------------------
 * Qwen3-TTS.  Replaces Qwen3TTSModel.generate / generateStream -> generateVoiceDesign
 * (Sources/MLXAudioTTS/Models/Qwen3TTS/Qwen3TTS.swift:60-133,306-569), the talker and code predictor LMs
 * (Qwen3TTSTalker.swift, Qwen3TTSCodePredictor.swift), sampleToken (:1003-1118) and the speech-tokenizer decoder
 * (Qwen3TTSSpeechTokenizer.swift:888-1006).  Tokenisation and the ChatML prompt text stay on the host.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_qwen3tts mis_qwen3tts;
typedef struct {
    mis_lm_config talker;          /* Qwen3TTSTalkerConfig (:200-305): vocab_size = codec vocabulary (3072) */
    mis_lm_config predictor;       /* Qwen3TTSTalkerCodePredictorConfig (:6-67): vocab_size 2048 */
    int32_t num_code_groups;       /* 16 */
    int32_t text_hidden_size, text_vocab_size;
    int32_t codec_eos_token_id;    /* 2150 */
    int32_t tts_pad_token_id;      /* 151671 */
    /* Qwen3TTSTokenizerDecoderConfig (:307-385) */
    int32_t dec_latent_dim, dec_codebook_dim, dec_codebook_size, dec_decoder_dim, dec_hidden_size, dec_intermediate_size;
    int32_t dec_head_dim, dec_num_heads, dec_num_layers, dec_num_kv_heads, dec_num_quantizers, dec_num_semantic_quantizers;
    float   dec_rms_norm_eps, dec_rope_theta;
    int32_t n_upsample_rates;    int32_t upsample_rates[8];      /* [8,5,4,3] */
    int32_t n_upsampling_ratios; int32_t upsampling_ratios[8];   /* [2,2] */
    int32_t sample_rate;           /* 24000 */
} mis_qwen3tts_config;
/* sampleToken parameters (VoiceDesignGenerationSettings, Qwen3TTS.swift:651-664; defaults 0.9 / 1.0 / - / 1.05 / 0) */
typedef struct {
    int32_t  max_frames;           /* maxTokens (4096); per-row caps via row_max_frames = min(maxTokens, max(75, 6 * text tokens)) (:383) */
    float    temperature, top_p;
    int32_t  top_k;                /* 0 = off */
    float    repetition_penalty, min_p;
    uint64_t seed;
    int64_t  row_offset;
} mis_qwen3tts_params;
mis_status mis_qwen3tts_create(const mis_qwen3tts_config*, int device, mis_qwen3tts** out);
/* keys after the reference's sanitize steps: talker tensors with or without the "talker." prefix
 * (model.*, codec_head.weight, text_projection.*, code_predictor.*), speech-tokenizer decoder tensors as "decoder.*"
 * with the module-tree names Qwen3TTSSpeechTokenizer.sanitize produces */
mis_status mis_qwen3tts_set_tensor(mis_qwen3tts*, const char* name, const void* data, mis_dtype dtype,
                                   const int64_t* shape, int ndim);
/* the same keys in MLX's affine-quantised form (the published Qwen3-TTS checkpoints are 8 bit, Qwen3TTS.swift:1157-1170): the
 * Linear layers of the talker and the code predictor are streamed as codes (see mis_tts_set_tensor_quantized); embeddings,
 * text projection, predictor tables / heads are dequantised at load (gathered or folded tensors) */
mis_status mis_qwen3tts_set_tensor_quantized(mis_qwen3tts*, const char* name, const uint32_t* wq, const void* scales,
                                             const void* biases, mis_dtype sb_dtype, int64_t N, int64_t K, int group_size, int bits);
mis_status mis_qwen3tts_finalize(mis_qwen3tts*);
void       mis_qwen3tts_destroy(mis_qwen3tts*);
mis_tts*   mis_qwen3tts_talker(mis_qwen3tts*);            /* borrowed handle (parity taps) */
int        mis_qwen3tts_samples_per_frame(const mis_qwen3tts*);   /* 1920 */
int        mis_qwen3tts_num_code_groups(const mis_qwen3tts*);     /* 16: ints per frame of codes_out */
/* Prompts as prepareGenerationInputs builds them (:883-1000): prefill position p of row b is
 * text_projection(text_embedding[text_ids[b,p]]) (text id >= 0) plus codec_embedding[codec_ids[b,p]] (codec id >= 0);
 * trailing_ids = the text ids added to the generated frames' embeddings (then tts_pad).  int32 [batch, P] / [batch, Tt].
 * *codes_out (mis_free) int32 [batch, *codes_stride, num_code_groups]; n_frames[batch]. */
mis_status mis_qwen3tts_generate_codes(mis_qwen3tts*, const int32_t* text_ids, const int32_t* codec_ids,
                                       const int32_t* prefill_lens, int P, const int32_t* trailing_ids,
                                       const int32_t* trailing_lens, int Tt, int batch, const mis_qwen3tts_params* params,
                                       const int32_t* row_max_frames, int32_t** codes_out, int64_t* codes_stride,
                                       int32_t* n_frames);
mis_status mis_qwen3tts_decode(mis_qwen3tts*, const int32_t* codes, int batch, int T, float* wav_out);
mis_status mis_qwen3tts_decoder_tap(mis_qwen3tts*, const int32_t* codes, int batch, int T, int stage, float* out,
                                    int64_t capacity, int32_t* channels, int64_t* length);
/* streamingStep / resetStreamingState (Qwen3TTSSpeechTokenizer.swift:948-1006) as a session on the handle: carried conv
 * inputs (CausalConv1d.step :199-227, k7 conv steps :655-667,:710-722), transposed-conv overlap (:553-576) and the decoder
 * transformer's K/V cache live on the device between steps; a step computes only the new frames.
 * begin: batch rows, at most max_frames frames in the session, at most max_chunk_frames per step.
 * step:  codes int32 [batch, num_quantizers, n_frames] (host or device) = the NEXT n_frames frames of every row ->
 *        wav_out f32 [batch, n_frames * samples_per_frame] (host or device).
 * set_stream_exact(1): chunked decode bitwise equal to mis_qwen3tts_decode of the whole sequence.  Default 0 = the
 * reference's arithmetic: its overlap-add sums two biased transposed-conv outputs, so the first `stride` samples of each
 * decoder block after a chunk boundary carry that block's bias twice. */
mis_status mis_qwen3tts_set_stream_exact(mis_qwen3tts*, int exact);
mis_status mis_qwen3tts_decode_stream_begin(mis_qwen3tts*, int batch, int max_frames, int max_chunk_frames);
mis_status mis_qwen3tts_decode_stream_step(mis_qwen3tts*, const int32_t* codes, int n_frames, float* wav_out);
mis_status mis_qwen3tts_decode_stream_end(mis_qwen3tts*);
/* generateVoiceDesign for a batch of prepared prompts (Qwen3TTS.swift:306-569).  *pcm_out (mis_free) f32 [batch, *pcm_stride].
 * on_event == NULL or chunk_frames <= 0: all frames, then one whole-sequence decode (one MIS_EVENT_AUDIO per row if on_event).
 * on_event != NULL and chunk_frames > 0 = generateStream (chunk_frames = streamingInterval * 12.5, :394-395): every
 * chunk_frames frames a streaming step of the whole batch runs on a second stream WHILE the frame loop continues; each
 * row's new samples arrive as MIS_EVENT_AUDIO as soon as they are on the host (:492-505), the frames after the last full
 * chunk when the loop ends (:537-546).  A row's pcm is the concatenation of its chunks (see set_stream_exact). */
mis_status mis_qwen3tts_generate(mis_qwen3tts*, const int32_t* text_ids, const int32_t* codec_ids, const int32_t* prefill_lens,
                                 int P, const int32_t* trailing_ids, const int32_t* trailing_lens, int Tt, int batch,
                                 const mis_qwen3tts_params* params, const int32_t* row_max_frames, float** pcm_out,
                                 int64_t* pcm_stride, int64_t* pcm_lens, int32_t** codes_out, int64_t* codes_stride,
                                 int32_t* n_frames, int chunk_frames, mis_event_cb on_event, void* user,
                                 const volatile int* cancel_flag);
/* In-context voice cloning.  Replaces the reference-audio front end - extractSpeakerEmbedding (Qwen3TTS.swift:839-881:
 * computeMelSpectrogram(24 kHz, nFft 1024, hop 256, 128 mels) -> Qwen3TTSSpeakerEncoder, Qwen3TTSSpeakerEncoder.swift:20-307) and
 * Qwen3TTSSpeechTokenizerEncoder.encode (Qwen3TTSSpeechTokenizer.swift:792-881: Mimi SEANet encoder, causal transformer, edge-padded
 * downsampling conv, split residual VQ) - and the ReferenceAudioContext the model keeps (:268-300): codecEmbedIcl (:249-266) rows
 * and the speaker vector become extra prompt rows of the handle that prefill positions address by codec id. */
typedef struct {
    /* Qwen3TTSSpeakerEncoderConfig (Qwen3TTSConfig.swift:69-117); spk_n_blocks = entries of enc_channels, 0 = no speaker encoder */
    int32_t spk_mel_dim, spk_enc_dim, spk_n_blocks;
    int32_t spk_channels[8], spk_kernel_sizes[8], spk_dilations[8];
    int32_t spk_attention_channels, spk_res2net_scale, spk_se_channels, spk_sample_rate;
    /* Qwen3TTSTokenizerEncoderConfig (Qwen3TTSConfig.swift:388-497); enc_num_filters == 0 = the tokenizer has no encoder */
    int32_t enc_audio_channels, enc_num_filters, enc_kernel_size, enc_last_kernel_size, enc_residual_kernel_size;
    int32_t enc_num_residual_layers, enc_dilation_growth_rate, enc_compress;
    int32_t enc_n_ratios, enc_upsampling_ratios[8];      /* as configured ([8,6,5,4]); the encoder applies them reversed */
    int32_t enc_use_causal_conv, enc_use_conv_shortcut;
    int32_t enc_hidden_size, enc_num_layers, enc_num_heads, enc_intermediate_size;
    int32_t enc_codebook_dim, enc_codebook_size, enc_num_quantizers, enc_valid_num_quantizers, enc_sampling_rate;
    float   enc_rope_theta, enc_frame_rate, enc_norm_eps;
} mis_qwen3tts_reference_config;
/* before the first set_tensor of these keys: "speaker_encoder.*" (names as Qwen3TTSSpeakerEncoder.sanitize leaves them behind the
 * prefix, conv weights [out, k, in]) and "encoder_model.*" (Qwen3TTSSpeechTokenizer.sanitize :1093-1440) are then routed to the
 * front end by mis_qwen3tts_set_tensor and checked by mis_qwen3tts_finalize */
mis_status mis_qwen3tts_enable_reference(mis_qwen3tts*, const mis_qwen3tts_reference_config*);
/* audio f32 [n_samples] mono at spk_sample_rate (host or device) -> out f32 [spk_enc_dim] */
mis_status mis_qwen3tts_speaker_embedding(mis_qwen3tts*, const float* audio, int64_t n_samples, float* out);
/* audio f32 [n_samples] mono at enc_sampling_rate -> *codes_out (mis_free) int32 [*n_q][*n_frames], n_q = min(valid, num_quantizers) */
mis_status mis_qwen3tts_encode_audio(mis_qwen3tts*, const float* audio, int64_t n_samples, int32_t** codes_out, int32_t* n_q,
                                     int32_t* n_frames);
/* parity taps, out f32 [channels, length] (capacity floats).  kind 0 = speaker encoder: stage i < spk_n_blocks - 1 = output of
 * blocks[i], then mfa, then asp ([2C, 1]); kind 1 = tokenizer encoder: 0 SEANet, 1 transformer, 2 downsampled latent */
mis_status mis_qwen3tts_reference_tap(mis_qwen3tts*, int kind, const float* audio, int64_t n_samples, int stage, float* out,
                                      int64_t capacity, int32_t* channels, int64_t* length);
/* A reference context on the handle: codes int32 [n_q, T] (n_q <= num_code_groups) and optionally the speaker vector
 * (f32 [hidden_size of the talker], rounded to the talker's bf16 on entry).  Its prompt rows follow the codec vocabulary: a prefill
 * position whose codec id is vocab_size + *speaker_row reads the speaker vector, vocab_size + *first_frame_row + t reads
 * codec_embedding[code 0 of frame t] + sum_i code_predictor.codec_embedding[i][code i+1 of frame t] (one bf16 rounding per add,
 * codecEmbedIcl :249-266).  A non-streaming generate prepends the reference codes of a row whose prompt uses such frame rows to the
 * generated ones before decoding and cuts the proportional head (ref frames / total frames) off the waveform (:550-563).
 * *speaker_row = -1 without a speaker vector.  Contexts live until clear_references / destroy; at most 64. */
mis_status mis_qwen3tts_add_reference(mis_qwen3tts*, const int32_t* codes, int n_q, int T, const float* speaker_embedding,
                                      int speaker_dim, int32_t* speaker_row, int32_t* first_frame_row);
mis_status mis_qwen3tts_clear_references(mis_qwen3tts*);
/* stand-alone sampleToken (parity tests): logits f32 [batch, vocab], seen u8 [batch, vocab] or NULL */
mis_status mis_qwen3tts_sample_logits(int device, const float* logits, int batch, int vocab, const uint8_t* seen,
                                      const mis_qwen3tts_params* params, int suppress_lo, int suppress_hi, int eos_id, int step,
                                      int32_t* tokens_out);

/* ------------------------------------------------------------------------------------------
 * Descript DAC decoder.  Replaces DescriptDAC.decodeFromCodes / decode (Sources/MLXAudioCodecs/Descript/DescriptDAC.swift:
 * 103-160,235-242), DescriptResidualVectorQuantize.fromCodes (DescriptQuantization.swift:150-163) and, when the checkpoint
 * carries the encoder tensors ("encoder.*", "*.in_proj.*"), DescriptDAC.encode / encodeAudio (:40-95,216-233,340-345).
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_dac mis_dac;
typedef struct {                   /* DescriptDACConfig.swift:3-34; latent_dim resolved (encoder_dim * 2^len(encoder_rates)) */
    int32_t latent_dim, decoder_dim;
    int32_t n_decoder_rates; int32_t decoder_rates[8];
    int32_t n_codebooks, codebook_size, codebook_dim;
    int32_t sample_rate;
} mis_dac_config;
mis_status mis_dac_create(const mis_dac_config*, int device, mis_dac** out);
/* checkpoint keys as stored; DescriptDAC.sanitize (:274-286) is applied */
mis_status mis_dac_set_tensor(mis_dac*, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim);
mis_status mis_dac_finalize(mis_dac*);
void       mis_dac_destroy(mis_dac*);
int64_t    mis_dac_num_samples(const mis_dac*, int n_frames);    /* 250 frames @ [8,5,4,2] -> 80 043 (output_padding 1 per block) */
mis_status mis_dac_decode_codes(mis_dac*, const int32_t* codes, int batch, int T, float* wav_out);
/* encode / encodeAudio (DescriptDAC.swift:216-233,340-345; needs the checkpoint's encoder.* and in_proj tensors, else
 * MIS_ERR_AUDIO_ENCODE): audio f32 [batch, n_samples] is right-padded to the hop length (prod of the encoder strides) ->
 * codes int32 [batch, nq, padded / hop] with nq = n_quantizers (0 = all; the reference's nQuantizers); z_out (nullable) f32 [batch, latent, T] = the encoder output before the RVQ.
 * Codebook lookup = nearest L2-normalised code, first index on ties (DescriptQuantization.swift:76-94). */
int64_t    mis_dac_padded_length(const mis_dac*, int64_t n_samples);
mis_status mis_dac_encode(mis_dac*, const float* audio, int batch, int64_t n_samples, int n_quantizers, int32_t* codes_out, float* z_out);
mis_status mis_dac_debug_tap(mis_dac*, const int32_t* codes, int batch, int T, int block, float* out, int64_t capacity,
                             int32_t* channels, int64_t* length);

/* ------------------------------------------------------------------------------------------
 * EnCodec decoder and encoder.  Replaces Encodec.decodeFrame / EncodecDecoder (Sources/MLXAudioCodecs/Encodec/Encodec.swift:94-170,295-302)
 * incl. the 2-layer LSTM (EncodecLayers.swift:15-80) and EncodecResidualVectorQuantizer.decode (EncodecQuantization.swift:117-133).
 * norm_type "weight_norm" models (no GroupNorm), mono, causal.  Chunked decode = decode_frame per chunk + the host
 * linearOverlapAdd of the reference (Encodec.swift:304-355; mirrored in the Python host layer).
 * Encode: Encodec.encodeFrame (Encodec.swift:212-238) = loudness normalisation (config.normalize), EncodecEncoder (:17-89) and
 * EncodecResidualVectorQuantizer.encode (EncodecQuantization.swift:22-32,100-114); the chunk walk of Encodec.encode (:248-291) is host
 * work (mirrored in the Python host layer), which folds all chunks of all batch rows into the rows of one encode_frame call.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_encodec mis_encodec;
typedef struct {                   /* EncodecConfig.swift:64-89 */
    int32_t audio_channels, num_filters, kernel_size, num_residual_layers, dilation_growth_rate;
    int32_t codebook_size, codebook_dim, hidden_size, num_lstm_layers, residual_kernel_size;
    int32_t use_causal_conv, pad_reflect, last_kernel_size, compress, use_conv_shortcut;
    float   trim_right_ratio;
    int32_t n_upsampling_ratios; int32_t upsampling_ratios[8];
    int32_t n_quantizers;          /* EncodecQuantization.swift:60-64 */
    int32_t sampling_rate;
    int32_t group_norm;            /* 1: norm_type "time_group_norm" (the 48 kHz model): GroupNorm(1 group) after every conv, in the
                                      transposed-conv layer before the trim (EncodecLayers.swift:128-131,203-212,244-262); 0: plain convs */
    int32_t normalize;             /* 1: encode divides every row by its loudness and returns it as the row's scale (Encodec.swift:227-233) */
} mis_encodec_config;
mis_status mis_encodec_create(const mis_encodec_config*, int device, mis_encodec** out);
/* module-tree keys: quantizer.layers.N.codebook.embed, decoder.layers.N.conv.{weight [out,k,in],bias},
 * decoder.layers.1.lstm.N.{Wx,Wh,bias}, decoder.layers.N.{block.1,block.3,shortcut}.conv.*, with group_norm also
 * <conv prefix>.norm.{weight,bias} [out].  Optional, all or none: the same key forms under encoder.layers.N (EncodecEncoder numbering:
 * 0 conv, then per reversed ratio [resnet x num_residual_layers, ELU, strided conv], LSTM block, ELU, last conv).  A checkpoint
 * without them finalizes and decodes; encoding with it returns MIS_ERR_AUDIO_ENCODE */
mis_status mis_encodec_set_tensor(mis_encodec*, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim);
mis_status mis_encodec_finalize(mis_encodec*);
void       mis_encodec_destroy(mis_encodec*);
int        mis_encodec_hop_length(const mis_encodec*);
/* wav_out f32 [batch, audio_channels, T * hop] (audio_channels 1 or 2) */
mis_status mis_encodec_decode_frame(mis_encodec*, const int32_t* codes, int batch, int n_q, int T, const float* scales, float* wav_out);
/* stage 1 conv0, 2 LSTM block, 3 + i upsampling block i: out f32 [batch, C, T'] */
mis_status mis_encodec_debug_tap(mis_encodec*, const int32_t* codes, int batch, int n_q, int T, int stage, float* out, int64_t capacity,
                                 int32_t* channels, int64_t* length);
int        mis_encodec_has_encoder(const mis_encodec*);          /* 1: finalized with the encoder.layers.* tensors */
int64_t    mis_encodec_encode_num_frames(const mis_encodec*, int64_t L);   /* frames of L samples: a ceil per strided conv */
/* encodeFrame of rows = chunks x batch independent rows: audio f32 [rows][channels][L], mask u8 [rows][L] or NULL (all ones; read by
 * normalize models only) -> codes_out i32 [rows][n_q][F], F = encode_num_frames(L); scales_out f32 [rows] or NULL (written by
 * normalize models only).  Host or device pointers.  A row's codes and scale do not depend on the other rows of the call */
mis_status mis_encodec_encode_frame(mis_encodec*, const float* audio, const uint8_t* mask, int rows, int64_t L, int n_q, int32_t* codes_out,
                                    float* scales_out);

/* ------------------------------------------------------------------------------------------
 * Mimi codec (Kyutai, 12.5 Hz codes, 24 kHz mono).  Replaces Mimi.decode / encode (Sources/MLXAudioCodecs/Mimi/Mimi.swift:168-186),
 * MimiStreamingDecoder.decodeFrames (:207-232, decodeStep :196-204) and the modules behind them: SplitResidualVectorQuantizer
 * (Quantization.swift), ConvTrUpsample1d / StreamableConv1d / StreamableConvTranspose1d (Conv.swift), the decoder transformer
 * (Transformer.swift) and SeanetDecoder / SeanetEncoder (Seanet.swift).  Float32 throughout.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_mimi mis_mimi;
typedef struct {                   /* MimiConfig of mimi_202407 (Mimi.swift:47-99); mis_mimi_202407 fills the defaults */
    int32_t channels, sample_rate; float frame_rate;
    /* SeanetConfig: dimension, filters, residual layers, ratios (decoder order), kernel sizes, dilation base, compress */
    int32_t dimension, n_filters, n_residual_layers, n_ratios, ratios[8];
    int32_t kernel_size, residual_kernel_size, last_kernel_size, dilation_base, compress;
    /* TransformerConfig: layers, heads, feed-forward width, streaming attention context, RoPE max period, LayerNorm eps */
    int32_t num_layers, num_heads, dim_feedforward, context;
    float   max_period, norm_eps;
    /* SplitResidualVectorQuantizer: codebooks (one semantic + nq - 1 acoustic), bins, codebook dimension */
    int32_t num_quantizers, bins, quantizer_dim;
} mis_mimi_config;
void       mis_mimi_202407(int num_codebooks, mis_mimi_config* out);
mis_status mis_mimi_create(const mis_mimi_config*, int device, mis_mimi** out);
/* post-sanitize names and layouts (Mimi.sanitize :337-415): conv [out, k, in], convtr [out, k, in / groups], Linear [out, in],
 * quantizer "*.output_proj.weight" / "*.input_proj.weight" [out, 1, in].  Missing keys fail at finalize.  The encoder is built when
 * "encoder.*" / "encoder_transformer.*" / "downsample.*" / the input projections are present; the codebooks serve both directions. */
mis_status mis_mimi_set_tensor(mis_mimi*, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim);
mis_status mis_mimi_finalize(mis_mimi*);
void       mis_mimi_destroy(mis_mimi*);
int64_t    mis_mimi_num_samples(const mis_mimi*, int n_frames);            /* n_frames * 1920 for mimi_202407 */
/* Mimi.decode: codes int32 [batch, n_q, T] (host or device), 2 <= n_q <= num_quantizers (else MIS_ERR_INVALID_INPUT) ->
 * pcm f32 [batch, num_samples(T)].  Plain causal attention over the whole sequence. */
mis_status mis_mimi_decode(mis_mimi*, const int32_t* codes, int batch, int n_q, int T, float* pcm_out);
/* Mimi.encode: audio f32 [batch, n_samples] -> codes int32 [batch, n_q, encode_num_frames(n_samples)], 1 <= n_q <= num_quantizers;
 * MIS_ERR_AUDIO_ENCODE without encoder tensors */
int64_t    mis_mimi_encode_num_frames(const mis_mimi*, int64_t n_samples);
mis_status mis_mimi_encode(mis_mimi*, const float* audio, int batch, int64_t n_samples, int n_q, int32_t* codes_out);
/* MimiStreamingDecoder: begin opens (or resets) a session of `batch` independent rows; each step decodes the next n_frames frames of
 * every row, codes int32 [batch, n_q, n_frames] -> pcm f32 [batch, n_frames * num_samples(1)], the result of n_frames decodeStep
 * calls.  The attention of the step sees the last `context` keys before the frame (Transformer.swift:155-166); the stream has no
 * length limit.  step without begin: MIS_ERR_NOT_INITIALIZED. */
mis_status mis_mimi_decode_stream_begin(mis_mimi*, int batch);
mis_status mis_mimi_decode_stream_step(mis_mimi*, const int32_t* codes, int n_q, int n_frames, float* pcm_out);
mis_status mis_mimi_decode_stream_end(mis_mimi*);

/* ------------------------------------------------------------------------------------------
 * Marvis TTS (CSM): backbone LM + depth decoder over Mimi codes.  Replaces CSMModel.generateFrame
 * (Sources/MLXAudioTTS/Models/Marvis/CSMModel.swift:467-526), CSMLlamaModel (CSMLlamaModel.swift) and the generate loop of
 * MarvisTTSModel.swift:402-477.  Rows of a batch are independent utterances (the reference runs batch 1).
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_marvis mis_marvis;
typedef struct {
    mis_lm_config backbone;        /* CSMLlamaConfiguration of the backbone; vocab_size / qk_norm / rope_* flags are set by the engine */
    mis_lm_config decoder;         /* ... of the depth decoder */
    int32_t text_vocab_size, audio_vocab_size, audio_num_codebooks;   /* K = audio_num_codebooks <= 32, audio_vocab_size <= 4096 */
} mis_marvis_config;
typedef struct {
    int32_t  max_frames;           /* 0 = 750 (60 s at 12.5 Hz, MarvisTTSModel.swift:402); at most 750 */
    int32_t  codebooks;            /* Cb = min(K, qualityLevel) (:17-22); 0 = K; outside 1..K: MIS_ERR_INVALID_INPUT */
    float    temperature;          /* 0 => arg-max; the reference samples with TopPSampler(temperature 0.9, topP 0.8) (:429) */
    float    top_p;
    uint64_t seed;                 /* mis-sampler-v1 keyed by (seed, row_offset + row, frame * K + codebook) */
    int64_t  row_offset;
} mis_marvis_params;
mis_status mis_marvis_create(const mis_marvis_config*, int device, mis_marvis** out);
/* post-sanitize names (MarvisTTSModel.sanitize :225-262): model.backbone.layers.N.*, model.backbone.norm.weight, model.decoder.*,
 * model.text_embeddings.weight [text_vocab, D], model.audio_embeddings.weight [audio_vocab * K, D], model.projection.weight [Dd, D],
 * model.codebook0_head.weight [audio_vocab, D], model.audio_head [K - 1, Dd, audio_vocab].  q_proj / k_proj rows are de-interleaved per
 * head when set (the engine rotates halves; CSM rotates pairs). */
mis_status mis_marvis_set_tensor(mis_marvis*, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim);
/* a module of an MLX-quantised checkpoint (`name` = its .weight key): Linear layers of both LMs and codebook0_head stream as 8 / 4-bit
 * codes where the GEMMs take the format (group 64, bf16 / f16 scales; otherwise dequantised at load); the embeddings and projection are
 * dequantised at load */
mis_status mis_marvis_set_tensor_quantized(mis_marvis*, const char* name, const uint32_t* wq, const void* scales, const void* biases,
                                           mis_dtype sb_dtype, int64_t N, int64_t K, int group_size, int bits);
mis_status mis_marvis_init_synthetic(mis_marvis*, uint64_t seed);
mis_status mis_marvis_init_synthetic_quantized(mis_marvis*, uint64_t seed, int bits);
mis_status mis_marvis_finalize(mis_marvis*);
void       mis_marvis_destroy(mis_marvis*);
mis_tts*   mis_marvis_backbone(mis_marvis*);          /* borrowed: the two LM handles (introspection, e.g. mis_tts_native_quant_bits) */
mis_tts*   mis_marvis_decoder(mis_marvis*);
int        mis_marvis_launches_per_frame(const mis_marvis*);   /* nodes of the last call's captured frame graph (MIS_NO_GRAPH: the expected count) */
/* Frames only.  tokens int32 [batch, P, K + 1] / mask u8 [batch, P, K + 1]: a text position has its id in the last column and mask
 * there only, an audio position K codes and mask on those (:70-134); prompt_lens[batch] < 2048 - 750.  row_max_frames (may be NULL):
 * per-row frame caps.  A frame whose Cb codes are all 0 ends its row and is not kept (:444-447).  Outputs: *codes_out (mis_free) int32
 * [batch, *codes_stride, Cb]; n_frames[batch].  Bad lengths, Cb, or ids outside their tables: MIS_ERR_INVALID_INPUT before any launch. */
mis_status mis_marvis_generate_codes(mis_marvis*, const int32_t* tokens, const uint8_t* mask, const int32_t* prompt_lens, int P, int batch,
                                     const mis_marvis_params* params, const int32_t* row_max_frames, int32_t** codes_out,
                                     int64_t* codes_stride, int32_t* n_frames);
/* Frames + audio through a borrowed Mimi (same device; its decode-stream session must be closed; 2 <= Cb <= its quantizers).  *pcm_out
 * (mis_free) f32 [batch, *pcm_stride], pcm_lens[batch] = n_frames * mis_mimi_num_samples(1).  A row's audio is the STREAMING decode of its
 * frames in both forms, so they return identical samples.  on_event == NULL or chunk_frames <= 0: all frames, then the audio (one
 * MIS_EVENT_AUDIO per row if on_event).  on_event and chunk_frames > 0 (streamingInterval * 12.5 frames, :403,464-470): Mimi's stream
 * step of the whole batch runs on Mimi's stream while the frame loop continues; MIS_EVENT_TOKEN (payload: the frame's Cb codes) per
 * frame, MIS_EVENT_AUDIO per row and chunk, MIS_EVENT_INFO per row when the loop ends, then the remainder.  cancel_flag is polled every
 * 8 frames -> MIS_ERR_CANCELLED.  codes_out / codes_stride / n_frames may be NULL. */
mis_status mis_marvis_generate(mis_marvis*, mis_mimi* mimi, const int32_t* tokens, const uint8_t* mask, const int32_t* prompt_lens, int P,
                               int batch, const mis_marvis_params* params, const int32_t* row_max_frames, float** pcm_out,
                               int64_t* pcm_stride, int64_t* pcm_lens, int32_t** codes_out, int64_t* codes_stride, int32_t* n_frames,
                               int chunk_frames, mis_event_cb on_event, void* user, const volatile int* cancel_flag);

/* ------------------------------------------------------------------------------------------
 * Log-mel / STFT front end.  Replaces WhisperAudio.logMelSpectrogram / encoderFeatures
 * (Sources/MLXAudioSTT/Models/Whisper/WhisperAudio.swift:38-87) and computeMelSpectrogram
 * (Sources/MLXAudioCore/DSP.swift:230-273): reflect pad, window, rfft, |.|^2, mel filterbank
 * (melFilters DSP.swift:76-168), log10, clamp to (max - 8), (x + 4) / 4.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t sample_rate, n_fft /* even, <= 2048 */, hop_length, n_mels /* <= 256 */;
    int32_t window;           /* 0 periodic Hann (WhisperAudio.swift:42-43), 1 symmetric Hann (DSP.swift:15-22) */
    int32_t mel_scale;        /* 0 HTK (DSP default), 1 Slaney (Whisper) */
    int32_t slaney_norm;      /* 1 = area normalisation (DSP.swift:155-162) */
    int32_t drop_last_frame;  /* 1 = Whisper (WhisperAudio.swift:65-67) */
} mis_mel_config;
int64_t    mis_mel_num_frames(const mis_mel_config*, int64_t n_samples);
/* pcm f32 [batch, n_samples] -> out f32 [batch, n_frames, n_mels]; every row is normalised by its own max */
mis_status mis_mel_spectrogram(int device, const mis_mel_config*, const float* pcm, int batch, int64_t n_samples,
                               float* out, int64_t* n_frames_out);
/* WhisperAudio.encoderFeatures: rows of `stride` samples with lens[b] valid (NULL = stride) are zero-padded /
 * trimmed to 480000 samples; out f32 [batch, 3000, n_mels], n_mels in {80, 128}. */
mis_status mis_whisper_encoder_features(int device, const float* pcm, const int64_t* lens, int batch, int64_t stride,
                                        int n_mels, float* out);

/* Streaming front end: IncrementalMelSpectrogram (Sources/MLXAudioSTT/Streaming/IncrementalMelSpectrogram.swift:17-215).
 * One handle per audio session; overlap-save framing and the running log-maximum are carried between calls.
 * out f32 [capacity_frames, n_mels]; *n_frames = frames produced by this call (0 while a frame is incomplete). */
typedef struct mis_mel_stream mis_mel_stream;
mis_status mis_mel_stream_create(int device, int sample_rate, int n_fft, int hop_length, int n_mels, mis_mel_stream** out);
mis_status mis_mel_stream_process(mis_mel_stream*, const float* samples, int64_t n, float* out, int64_t capacity_frames,
                                  int64_t* n_frames);
mis_status mis_mel_stream_flush(mis_mel_stream*, float* out, int64_t capacity_frames, int64_t* n_frames);
mis_status mis_mel_stream_reset(mis_mel_stream*);
int64_t    mis_mel_stream_total_frames(const mis_mel_stream*);
void       mis_mel_stream_destroy(mis_mel_stream*);

/* ------------------------------------------------------------------------------------------
 * Whisper STT.  Replaces WhisperModel / WhisperEncoder / WhisperDecoder
 * (Sources/MLXAudioSTT/Models/Whisper/WhisperModel.swift:36-309, WhisperLayers.swift:110-328).
 * bf16 compute (fp16 checkpoints are converted at load).  Tokenisation / prompt construction /
 * text decoding stay on the host (WhisperTokenizer.swift), as in the reference.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_whisper mis_whisper;
/* WhisperConfig, WhisperConfig.swift:3-22 */
typedef struct {
    int32_t vocab_size, num_mel_bins, d_model;
    int32_t encoder_layers, encoder_attention_heads, encoder_ffn_dim, max_source_positions;
    int32_t decoder_layers, decoder_attention_heads, decoder_ffn_dim, max_target_positions;
} mis_whisper_config;
/* generation knobs of transcribeChunk (WhisperModel.swift:213-236) + WhisperGenerationConfig suppress lists */
typedef struct {
    int32_t max_tokens;            /* STTGenerateParameters.maxTokens */
    float   temperature;           /* <= 0: greedy argmax (:284-287) */
    uint64_t seed;
    int32_t eot_id;                /* tokenizer.endOfTextId: ends a row, not emitted */
    int32_t timestamp_begin;       /* suppressFromIndex(:300-309): ids >= this are never sampled (0 = off) */
    const int32_t* suppress;       /* suppress_tokens, every step */
    int32_t n_suppress;
    const int32_t* begin_suppress; /* begin_suppress_tokens, first step only (default [eot]) */
    int32_t n_begin_suppress;
    int64_t row_offset;            /* global index of row 0 (sharding): the sampler's RNG is keyed by the global row */
} mis_stt_params;
mis_status mis_whisper_create(const mis_whisper_config*, int device, mis_whisper** out);
/* HF transformers key layout (model.encoder.* / model.decoder.*; conv weights [out, in, k]; proj_out ignored: tied) or the
 * mlx-whisper layout (encoder.blocks.N.attn.query.*, conv weights [out, k, in], encoder positional embedding synthesised):
 * WhisperModel.sanitize, WhisperModel.swift:321-478 */
mis_status mis_whisper_set_tensor(mis_whisper*, const char* name, const void* data, mis_dtype dtype,
                                  const int64_t* shape, int ndim);
/* the same keys in MLX's affine-quantised form (mlx-community whisper conversions; WhisperModel.fromDirectory quantises every Linear and
 * decoder.embed_tokens, WhisperModel.swift:499-510): `name` is the `.weight` key (either layout), wq uint32 [N, K*bits/32], scales /
 * biases [N, K/group_size] of dtype sb_dtype - the format and validation of mis_tts_set_tensor_quantized.  The reference keeps
 * QuantizedLinear and never materialises the weight: quantizedMatmul applies scale and bias to float32 group sums.  So does the engine
 * for the decoder matrices every step re-reads (self q|k|v, self out, cross q, cross out, fc1, fc2 and the tied vocab projection) when
 * they arrive with 8 or 4 bits, group size 64 and bf16 or f16 scales (f16 read as stored): the codes are streamed (csrc/lm_qgemm.hip);
 * a layer's q|k|v only if its three projections share bits and scale dtype.  The encoder matrices and the cross-attention K/V
 * projections (run once per 30 s window at 1500 rows) are dequantised once at load into the bf16 layouts; so is the token-embedding
 * gather (QuantizedEmbedding: dequantised rows).  Any other combination (2 bit, other group sizes, f32 scales, MIS_QUANT_NATIVE=0) is
 * dequantised at load into the bf16 layout, which rounds s*q+b to bf16 per weight - a stated deviation for those cases only.
 * proj_out.{weight,scales,biases} are ignored (tied). */
mis_status mis_whisper_set_tensor_quantized(mis_whisper*, const char* name, const uint32_t* wq, const void* scales, const void* biases,
                                            mis_dtype sb_dtype, int64_t N, int64_t K, int group_size, int bits);
/* after finalize: bits a decoder matrix is streamed in (0 = dense bf16).  role 0 self q|k|v, 1 self out, 2 cross q, 3 cross out,
 * 4 fc1, 5 fc2 of decoder layer `layer`; role 6 the tied vocab projection (layer ignored) */
int        mis_whisper_native_quant_bits(const mis_whisper*, int layer, int role);
mis_status mis_whisper_init_synthetic(mis_whisper*, uint64_t seed);
/* benches: every Linear and the token embedding as a synthetic MLX-quantised matrix (bits 8 or 4, group 64, sb_dtype MIS_BF16 or
 * MIS_F16) through the path of mis_whisper_set_tensor_quantized - no checkpoints offline */
mis_status mis_whisper_init_synthetic_quantized(mis_whisper*, uint64_t seed, int bits, mis_dtype sb_dtype);
mis_status mis_whisper_finalize(mis_whisper*);
void       mis_whisper_destroy(mis_whisper*);
/* WhisperEncoder (+ the cross-attention K/V of every decoder layer): features f32 [batch, 3000, n_mels];
 * enc_out f32 [batch, 1500, d_model] or NULL.  Resets the decoder state. */
mis_status mis_whisper_encode(mis_whisper*, const float* features, int batch, float* enc_out);
mis_status mis_whisper_decoder_reset(mis_whisper*);
/* one decoder token per active row through the KV caches (WhisperDecoder.callAsFunction with Tnew = 1);
 * logits_out f32 [batch, vocab] (tied projection) or NULL */
mis_status mis_whisper_decoder_forward(mis_whisper*, const int32_t* tokens, const uint8_t* active, float* logits_out);
/* transcribeChunk for a batch of <= 30 s windows: pcm f32 [batch, stride] (lens[b] valid samples, NULL = stride),
 * prompt_ids = buildPromptTokens(...) shared by all rows.  *tokens_out (mis_free) int32 [batch, *tokens_stride],
 * n_tokens[batch] generated ids per row (EOT excluded). */
mis_status mis_stt_whisper_generate(mis_whisper*, const float* pcm, const int64_t* lens, int batch, int64_t stride,
                                    const int32_t* prompt_ids, int n_prompt, const mis_stt_params*,
                                    int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens);
/* generateStream (WhisperModel.swift:92-160): same work, announcing every sampled id as MIS_EVENT_TOKEN (row, id) while the loop
 * runs (every 4 steps; EOT is never announced) - the host turns ids into the reference's text deltas (decode-and-diff,
 * onTokenDelta :186-250) - then one MIS_EVENT_INFO per row (prompt_token_count, generation_token_count of the final .result).
 * cancel_flag polled at the same cadence -> MIS_ERR_CANCELLED.  tokens_out / tokens_stride / n_tokens may be NULL. */
mis_status mis_stt_whisper_generate_stream(mis_whisper*, const float* pcm, const int64_t* lens, int batch, int64_t stride,
                                           const int32_t* prompt_ids, int n_prompt, const mis_stt_params*,
                                           mis_event_cb on_event, void* user, const volatile int* cancel_flag,
                                           int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens);

/* ------------------------------------------------------------------------------------------
 * Moonshine STT (Sources/MLXAudioSTT/Models/Moonshine/MoonshineModel.swift:112-411, MoonshineConfig.swift:3-125): raw 16 kHz samples ->
 * strided conv stem -> encoder -> decoder with cached self / cross K/V -> greedy ids.  No mel front end: the work follows the audio
 * length, and a batch is RAGGED - every row has its own frame count T3 = ((T1 - 7) / 3 + 1 - 3) / 2 + 1, T1 = (n - 127) / 64 + 1;
 * samples past lens[b] never influence a result.  Rows shorter than 895 samples (T3 < 1) or longer than 480000 (30 s) and batches above
 * 64 rows are MIS_ERR_INVALID_INPUT.  f32 through GroupNorm, bf16 storage / f32 accumulation behind it (f32 checkpoints are rounded to
 * bf16 once, at finalize); logits f32.  hidden_size <= 512 (a multiple of 32), head_dim <= 64 (heads are zero-padded to 64 at load).
 * Tokenizer and text stay on the host (MoonshineTokenizer, :7-69).
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_moonshine mis_moonshine;
/* MoonshineConfig.swift:3-25; *_hidden_act: 0 gelu, 1 silu (the decoder MLP is the SiLU gate whatever decoder_hidden_act says, :223-227;
 * encoder_hidden_act 1 is not implemented) */
typedef struct {
    int32_t vocab_size, hidden_size, intermediate_size;
    int32_t encoder_num_hidden_layers, decoder_num_hidden_layers, encoder_num_attention_heads, decoder_num_attention_heads;
    int32_t encoder_num_key_value_heads, decoder_num_key_value_heads, encoder_hidden_act, decoder_hidden_act;
    int32_t max_position_embeddings, attention_bias;
    float   partial_rotary_factor, rope_theta;
    int32_t bos_token_id, eos_token_id, decoder_start_token_id, tie_word_embeddings;
} mis_moonshine_config;
mis_status mis_moonshine_create(const mis_moonshine_config*, int device, mis_moonshine** out);
/* published key layout ("model.encoder.conv1.weight" [d, 1, 127], conv weights [out, in, k], "proj_out.weight" ignored when tied);
 * host pointers; MoonshineModel.sanitize, :443-459 */
mis_status mis_moonshine_set_tensor(mis_moonshine*, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim);
mis_status mis_moonshine_init_synthetic(mis_moonshine*, uint64_t seed);
mis_status mis_moonshine_finalize(mis_moonshine*);
void       mis_moonshine_destroy(mis_moonshine*);
/* lens[batch] samples -> frames_out[batch] encoder frames T3 (0: too short).  Host arithmetic; the handle may be NULL. */
mis_status mis_moonshine_frames(const mis_moonshine*, const int64_t* lens, int batch, int32_t* frames_out);
/* MoonshineEncoder (+ the cross-attention K/V of every decoder layer): pcm f32 [batch, stride], lens[batch] valid samples (NULL =
 * stride); enc_out f32 [batch, max T3, hidden] (zeros behind a row's own T3) or NULL.  Resets the decoder state. */
mis_status mis_moonshine_encode(mis_moonshine*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* enc_out);
/* empties the self-attention caches; max_positions: decoder positions to provide for (<= 2048; 0 = max_position_embeddings) */
mis_status mis_moonshine_decoder_reset(mis_moonshine*, int max_positions);
/* one teacher-forced decoder token per row through the caches (MoonshineDecoder with one new position); logits_out f32 [batch, vocab] or NULL */
mis_status mis_moonshine_decoder_forward(mis_moonshine*, const int32_t* tokens, float* logits_out);
/* kernel launches of one decoder step of the generate loop (8 per layer + vocabulary projection + arg-max) */
int        mis_moonshine_launches_per_step(const mis_moonshine*);
/* MoonshineModel.generate (:374-411) for a ragged batch: decoder_start_token_id, arg-max per step, eos_token_id ends a row and is not
 * kept, at most max_tokens ids (<= 0: 200; <= 2047).  Only max_tokens and temperature of mis_stt_params are read; temperature > 0 is
 * MIS_ERR_INVALID_INPUT (sampling is not mirrored).  *tokens_out (mis_free) int32 [batch, *tokens_stride], n_tokens[batch]. */
mis_status mis_stt_moonshine_generate(mis_moonshine*, const float* pcm, const int64_t* lens, int batch, int64_t stride,
                                      const mis_stt_params*, int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens);

/* ------------------------------------------------------------------------------------------
 * Smart Turn endpoint detection (Sources/MLXAudioVAD/Models/SmartTurn/SmartTurn.swift:29-272, SmartTurnFeatures.swift:10-81,
 * SmartTurnConfig.swift): has the speaker finished?  Every row is cut or left-padded with zeros to W = max_audio_seconds * sampling_rate
 * samples, normalised to zero mean and unit deviation over the whole window (padding included), turned into F = W / hop_length log-mel
 * frames (symmetric Hann, Slaney filters, last frame dropped) and run through a Whisper-style encoder of T = F / 2 positions, an
 * attention pool and a small classifier.  Encoder in bf16 storage / f32 accumulation (an f32 checkpoint is rounded once, at finalize);
 * prepare, features, pool and classifier in f32.  1..64 rows per call.  No step mixes rows, and every reduction runs in a fixed order,
 * so a row's result is the same bit for bit in every batch whose encoder GEMMs run the same kernel; the GEMM launcher picks its
 * 256 x 256 tile once a product has 200 or more such tiles (at the published shape: from about 22 rows), and across that switch the
 * f32 summation order may differ, i.e. results agree to bf16 rounding only.
 * Rejected with MIS_ERR_INVALID_INPUT before any launch: T > max_source_positions, odd F, head size other than 64 / 128, d_model or
 * encoder_ffn_dim not a multiple of 32, n_fft / num_mel_bins outside what mis_mel_config takes; at a call, batch outside 1..64,
 * lens[b] outside 1..stride, a null pointer, a handle that is not finalized.  A rejected call leaves the handle usable.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_smartturn mis_smartturn;
/* SmartTurnEncoderConfig + SmartTurnProcessorConfig (SmartTurnConfig.swift:3-104); n_mels of the processor = num_mel_bins */
typedef struct {
    int32_t num_mel_bins, max_source_positions, d_model, encoder_attention_heads, encoder_layers, encoder_ffn_dim, k_proj_bias;
    int32_t sampling_rate, max_audio_seconds, n_fft, hop_length, normalize_audio;
    float   threshold;
} mis_smartturn_config;
mis_status mis_smartturn_create(const mis_smartturn_config*, int device, mis_smartturn** out);
/* names as SmartTurnModel.sanitize leaves them (:274-324): encoder.conv{1,2}.weight [out, k, in], encoder.embed_positions.weight,
 * encoder.layers.N.{self_attn_layer_norm,self_attn.{q,k,v,out}_proj,fc1,fc2,final_layer_norm}.*, encoder.layer_norm.*,
 * pool_attention_{0,2}.*, classifier_{0,1,4,6}.*; host pointers.  finalize names a missing weight and checks every shape. */
mis_status mis_smartturn_set_tensor(mis_smartturn*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_smartturn_init_synthetic(mis_smartturn*, uint64_t seed);
mis_status mis_smartturn_finalize(mis_smartturn*);
void       mis_smartturn_destroy(mis_smartturn*);
/* kernel nodes of the last call's encoder + head chain: the node count of the replayed graph, or the launches made under MIS_NO_GRAPH */
int        mis_smartturn_launches(const mis_smartturn*);
/* pcm f32 [batch, stride], lens[batch] (NULL = stride); threshold < 0 = the config's.  Outputs caller-allocated [batch]; any may be NULL. */
mis_status mis_smartturn_predict(mis_smartturn*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float threshold,
                                 float* probability, float* logit, int32_t* prediction);
/* already-prepared features f32 [batch, n_mels, F] (HF layout, SmartTurnModel.callAsFunction) */
mis_status mis_smartturn_forward_features(mis_smartturn*, const float* features, int batch, float* probability, float* logit);

/* ------------------------------------------------------------------------------------------
 * Spoken language identification: ECAPA-TDNN over VoxLingua107 (Sources/MLXAudioLID/Models/EcapaTdnn/EcapaTdnnLID.swift:13-195,
 * EcapaTdnnLayers.swift:52-78, EcapaMelSpectrogram.swift:15-55, MLXAudioCodecs/EcapaTdnn/EcapaTdnnBackbone.swift:16-282 with zero padding
 * and global context): which language is spoken?  16 kHz mono rows of differing lengths, 1..max_batch a call.  Row b of n_b samples has
 * T_b = n_b / 160 + 1 frames: periodic Hamming window of 400, 200 zeros on each side, power spectrum, HTK filters without
 * normalisation, 10 log10 max(., 1e-10) floored at the row's own maximum - 80, minus the per-mel mean over the row's own frames; then
 * the backbone (BatchNorm after every ReLU, running statistics), attentive statistics pooling over the valid frames, and the
 * BatchNorm / LeakyReLU classifier with log-softmax.  f32 weights and activations, contractions in exact f32 on the matrix cores.
 * A row's result does not depend on the batch it travels in, on the longest row, or on what lies behind lens[b]: bit for bit.
 * The workspace is sized once, at finalize, from max_batch and max_samples; a call allocates nothing.
 * Rejected with MIS_ERR_INVALID_INPUT before any launch: kernel sizes other than 1 / 3 / 5, channels not a multiple of res2net_scale,
 * sizes outside the ranges mis_ecapa_lid_create names, a tensor missing or misshapen at finalize; at a call, batch outside
 * 1..max_batch, an empty row (the reference would return NaN), a row longer than stride or max_samples, a null pointer, a handle that
 * is not finalized.  A rejected call leaves the handle usable.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_ecapa_lid mis_ecapa_lid;
/* EcapaTdnnConfig (EcapaTdnnConfig.swift:8-89) + the sizes of the workspace */
typedef struct {
    int32_t n_mels, channels, kernel_sizes[5], dilations[5], attention_channels, res2net_scale, se_channels, embedding_dim,
            classifier_hidden_dim, num_classes;
    int32_t max_batch, max_samples;      /* 1..64 rows a call; samples per row (at most 120 s) */
} mis_ecapa_lid_config;
mis_status mis_ecapa_lid_create(const mis_ecapa_lid_config*, int device, mis_ecapa_lid** out);
/* names as EcapaTdnn.sanitize leaves them (EcapaTdnnLID.swift:99-131): embedding_model.{block0,mfa,asp.tdnn}.{conv,norm}.*,
 * embedding_model.blockN.{tdnn1,tdnn2,res2net_block.blocks.M}.{conv,norm}.*, embedding_model.blockN.se_block.conv{1,2}.*,
 * embedding_model.{asp.conv,asp_bn,fc}.*, classifier.{norm,DNN.block_0.linear.w,DNN.block_0.norm,out.w}.*; conv weights [out, k, in],
 * BatchNorm as weight / bias / running_mean / running_var; host pointers.  finalize names a missing weight and checks every shape. */
mis_status mis_ecapa_lid_set_tensor(mis_ecapa_lid*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_ecapa_lid_init_synthetic(mis_ecapa_lid*, uint64_t seed);
mis_status mis_ecapa_lid_finalize(mis_ecapa_lid*);
void       mis_ecapa_lid_destroy(mis_ecapa_lid*);
/* kernel launches of the last call */
int        mis_ecapa_lid_launches(const mis_ecapa_lid*);
/* pcm f32 [batch, stride], lens[batch] (NULL = stride).  top_k is clamped to 0..num_classes: k.  Outputs caller-allocated, any may be
 * NULL: log_probs [batch, num_classes], embedding [batch, embedding_dim], top_idx / top_prob [batch, k], sorted on the device by
 * descending probability, ties to the lower index. */
mis_status mis_ecapa_lid_predict(mis_ecapa_lid*, const float* pcm, const int64_t* lens, int batch, int64_t stride, int top_k,
                                 float* log_probs, float* embedding, int32_t* top_idx, float* top_prob);
/* already-computed mel dB f32 [batch, T, n_mels] with frames[batch] valid frames each (NULL = T): EcapaTdnn.callAsFunction, the
 * sentence-mean step included */
mis_status mis_ecapa_lid_forward_features(mis_ecapa_lid*, const float* mel, const int32_t* frames, int batch, int T, int top_k,
                                          float* log_probs, float* embedding, int32_t* top_idx, float* top_prob);
/* tensors of the last call, f32, zeros behind a row's own frames.  stage 0 mel dB [B, Ts, n_mels] (Ts: frames of the longest row),
 * 1 normalised features, 2 block0 [B, Ts, C], 3-5 the SE-Res2Net blocks, 6 mfa [B, Ts, 3 C], 7 pooled [B, 1, 6 C], 8 embedding,
 * 9 log-probabilities.  dims[3] receives B, Ts, width; out NULL for the dims alone, else room for `capacity` floats. */
mis_status mis_ecapa_lid_tap(mis_ecapa_lid*, int stage, float* out, int64_t capacity, int64_t* dims);

/* ------------------------------------------------------------------------------------------
 * LASR CTC speech-to-text (Sources/MLXAudioSTT/Models/LasrCTC/LasrCTCModel.swift:7-406, LasrCTCConfig.swift:3-193; front end
 * ParakeetAudio.swift:6-62 with DSP.swift hanningWindow / stft(.constant) / melFilters(slaney, slaney); greedy CTC
 * Wav2Vec2CTC.swift:520-542): 16 kHz mono rows of differing lengths, 1..max_batch a call.  Row b of n_b samples has F_b = 1 + n_b / 160
 * feature frames (pre-emphasis 0.97, symmetric Hann window of 400 in 512, 256 zeros on each side, power spectrum, slaney filters,
 * log(. + 2^-24), per-bin mean / unbiased variance over the row's own frames), T1_b = (F_b - k_s) / s + 1 and T2_b = (T1_b - k_s) / s + 1
 * frames behind the two stem convs; then the macaron Conformer blocks (full non-causal attention with rotate-half RoPE over the row's
 * own T2_b keys, GLU -> depthwise conv -> inference BatchNorm), out_norm, the CTC head and greedy CTC collapse on the device.
 * f32 through the normalised features, bf16 storage with f32 accumulation behind them, f32 logits; the RoPE tables stay f32.
 * A row's result does not depend on the batch it travels in, on the longest row, or on what lies behind lens[b]: bit for bit.
 * The workspace is sized once, at finalize, from max_batch and max_seconds; a call allocates nothing.
 * Limits, MIS_ERR_INVALID_INPUT at create with a message naming the field: head size hidden_size / num_attention_heads = 64;
 * hidden_size, intermediate_size, subsampling_conv_channels multiples of 32; num_key_value_heads divides num_attention_heads;
 * conv_kernel_size 2..64; subsampling_conv_kernel_size 2..8; subsampling_conv_stride 1..4; vocab_size <= 65536 (any value: a vocabulary
 * that is no multiple of 4 is padded inside the engine); num_mel_bins 8..256 (dense_0's K is zero-padded to a multiple of 32 at load);
 * rope_type 0 ("default") only; max_batch 1..64; max_seconds 1..120.  At finalize: a tensor missing or misshapen.  At a call, before
 * any launch: batch outside 1..max_batch, a row longer than stride or max_seconds, a row too short for the stem (F_b < k_s or
 * T1_b < k_s), a null pointer.  A rejected call leaves the handle usable.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_lasr mis_lasr;
/* LasrCTCConfig + LasrEncoderConfig; hidden_act 0 silu, 1 relu; rope_type 0 "default"; max_batch / max_seconds size the workspace */
typedef struct {
    int32_t vocab_size, hidden_size, num_hidden_layers, num_attention_heads, num_key_value_heads, intermediate_size, hidden_act,
            conv_kernel_size, convolution_bias, num_mel_bins, subsampling_conv_channels, subsampling_conv_kernel_size,
            subsampling_conv_stride, attention_bias, rope_type, pad_token_id, max_batch, max_seconds;
    float layer_norm_eps, rope_theta, conv_residual_weights[2], feed_forward_residual_weights[2];
} mis_lasr_config;
mis_status mis_lasr_create(const mis_lasr_config*, int device, mis_lasr** out);
/* names as LasrCTCModel.sanitize leaves them (:352-367): encoder.subsampler.{dense_0,conv_0,conv_1,dense_1}.*,
 * encoder.layers.N.{feed_forward1,feed_forward2}.{linear1,linear2}.*, .self_attn.{q,k,v,o}_proj.*, .conv.{pointwise_conv1,depthwise_conv,
 * pointwise_conv2}.*, .conv.norm.{weight,bias,running_mean,running_var}, .norm_{feed_forward1,self_att,conv,feed_forward2,out}.*,
 * encoder.out_norm.*, ctc_head.*; conv weights [out, k, in]; host pointers.  finalize names a missing weight and checks every shape;
 * only a LayerNorm's bias may be absent (zero, as the reference creates it: the published checkpoints carry none). */
mis_status mis_lasr_set_tensor(mis_lasr*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_lasr_init_synthetic(mis_lasr*, uint64_t seed);
mis_status mis_lasr_finalize(mis_lasr*);
void       mis_lasr_destroy(mis_lasr*);
/* kernel launches of the last call */
int        mis_lasr_launches(const mis_lasr*);
/* F_b and T2_b of rows of lens[b] samples (either output may be NULL; T2 0: too short for the stem) */
mis_status mis_lasr_frames(const mis_lasr*, const int64_t* lens, int batch, int32_t* F_out, int32_t* T2_out);
/* pcm f32 [batch, stride], lens[batch] (NULL = stride) -> normalised features f32 [batch, Fmax, num_mel_bins], Fmax the longest row's
 * frames, zeros behind a row's own F_b */
mis_status mis_lasr_features(mis_lasr*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* feats_out);
/* LasrCTCModel.callAsFunction on given features f32 [batch, F, num_mel_bins], frames[batch] valid frames each (NULL = F) ->
 * logits f32 [batch, T2 of F, vocab_size], zeros behind a row's own T2_b */
mis_status mis_lasr_forward_features(mis_lasr*, const float* feats, const int32_t* frames, int batch, int F, float* logits_out);
/* front end + callAsFunction: logits f32 [batch, T2 of the longest row, vocab_size] */
mis_status mis_lasr_forward(mis_lasr*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* logits_out);
/* generate for a ragged batch: arg-max per frame (lowest index on ties), a token is kept when it differs from the previous frame's and
 * is not pad_token_id.  tokens_out int32 [batch, tokens_stride] and n_tokens[batch] are the caller's; a row's ids behind tokens_stride
 * are dropped (T2 of the longest row always suffices).  One synchronisation per call. */
mis_status mis_stt_lasr_generate(mis_lasr*, const float* pcm, const int64_t* lens, int batch, int64_t stride, int32_t* tokens_out,
                                 int64_t tokens_stride, int32_t* n_tokens);
/* tensors of the last call, f32 [B, T2max, hidden_size], zero rows behind a row's own T2_b: stage 0 the stem's output, 1..L that
 * block's output, L + 1 out_norm.  dims[3] receives B, T2max, hidden_size; out NULL for the dims alone, else room for `capacity` floats. */
mis_status mis_lasr_tap(mis_lasr*, int stage, float* out, int64_t capacity, int64_t* dims);

/* ------------------------------------------------------------------------------------------
 * FSMN voice activity detection (Sources/MLXAudioVAD/Models/FSMNVAD/FSMNVAD.swift): mono rows of differing lengths at the model's
 * sample rate, 1..max_batch a call, of ANY length.  Row b of n_b samples has T_b = 1 + (n_b - win) / hop fbank frames (0 below one
 * window; win / hop = sample_rate x frame_length / frame_shift / 1000) and R_b = (T_b + (lfr_m - 1) / 2 + lfr_n - 1) / lfr_n LFR rows.
 * Front end: x 32768, minus the frame mean, pre-emphasis 0.97 with the frame's first sample kept, symmetric Hamming, 512-point power
 * spectrum, HTK triangles from 20 Hz to Nyquist (unnormalised, none on the Nyquist bin), log max(., 1e-8); per frame also
 * decibel = 10 log10(sum x^2 + 1e-6) of the raw samples.  LFR row o, slot i = fbank frame clamp(o lfr_n + i - (lfr_m - 1) / 2, 0, T - 1);
 * (x + shift) scale when cmvn.shift / cmvn.scale of input_dim values are loaded.  Encoder: in_linear1, ReLU(in_linear2), fsmn_layers x
 * {linear, p + depthwise causal conv of lorder taps, ReLU(affine)}, out_linear1, softmax(out_linear2).  All of it exact f32.
 * The encoder is causal with a reach of fsmn_layers (lorder - 1) rows: a call walks the LFR rows in chunks of chunk_frames, recomputing
 * that halo, inside one workspace sized at finalize for max_batch rows of chunk_frames (+ halo) - a call allocates nothing and
 * synchronises once.  A row's result does not depend on the batch it travels in, on what lies behind lens[b], or on chunk_frames:
 * bit for bit.  The serial post-processing that turns the two per-frame floats into segments is host work (vad.py).
 * Rejected with MIS_ERR_INVALID_INPUT at create: lstride != 1, lfr_n > lfr_m, input_dim != n_mels x lfr_m, a window outside 257..512
 * samples, output_dim > 256, sizes outside the ranges the messages name; at finalize a tensor missing or misshapen; at a call batch
 * outside 1..max_batch, a row longer than stride, too little room in an output, a null pointer, a handle that is not finalized.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_fsmn_vad mis_fsmn_vad;
/* FSMNVADEncoderConfig + the front-end fields of FSMNVADConfig + sil_pdf_ids (the first n_sil entries) + the sizes of the workspace */
typedef struct {
    int32_t input_dim, input_affine_dim, fsmn_layers, linear_dim, proj_dim, lorder, rorder, lstride, rstride, output_affine_dim, output_dim;
    int32_t sample_rate, n_mels, frame_length, frame_shift, lfr_m, lfr_n;
    int32_t n_sil, sil_pdf_ids[16];
    int32_t max_batch, chunk_frames;     /* 1..64 rows a call; LFR rows a chunk */
} mis_fsmn_vad_config;
mis_status mis_fsmn_vad_create(const mis_fsmn_vad_config*, int device, mis_fsmn_vad** out);
/* names with the "encoder." prefix stripped: in_linear{1,2}.{weight,bias}, fsmn.N.linear.weight, fsmn.N.fsmn_block.conv_left.weight
 * [proj, lorder, 1], fsmn.N.affine.{weight,bias}, out_linear{1,2}.{weight,bias}; optional cmvn.shift / cmvn.scale (ignored unless both
 * hold input_dim values, as the reference ignores them); host pointers.  finalize names a missing weight and checks every shape. */
mis_status mis_fsmn_vad_set_tensor(mis_fsmn_vad*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_fsmn_vad_init_synthetic(mis_fsmn_vad*, uint64_t seed);
mis_status mis_fsmn_vad_finalize(mis_fsmn_vad*);
void       mis_fsmn_vad_destroy(mis_fsmn_vad*);
/* kernel launches of the last call: 5 + 2 fsmn_layers per chunk from pcm (13 at the published depth), one less from features */
int        mis_fsmn_vad_launches(const mis_fsmn_vad*);
/* T_b and R_b of rows of lens[b] samples (either output may be NULL) */
mis_status mis_fsmn_vad_frames(const mis_fsmn_vad*, const int64_t* lens, int batch, int32_t* frames_out, int32_t* rows_out);
/* pcm f32 [batch, stride], lens[batch] (NULL = stride) -> LFR + CMVN features f32 [batch, rows, input_dim]; rows >= the longest row's
 * R_b, zeros behind a row's own.  A batch of rows below one window launches nothing and writes nothing. */
mis_status mis_fsmn_vad_features(mis_fsmn_vad*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* features_out,
                                 int rows);
/* FSMNVAD.callAsFunction on given features f32 [batch, rows, input_dim], counts[batch] valid rows each (NULL = rows) -> scores f32
 * [batch, rows, output_dim], zeros behind a row's own */
mis_status mis_fsmn_vad_forward_features(mis_fsmn_vad*, const float* features, const int32_t* counts, int batch, int rows, float* scores_out);
/* front end + encoder: scores f32 [batch, rows, output_dim] */
mis_status mis_fsmn_vad_forward(mis_fsmn_vad*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* scores_out, int rows);
/* what the post-processing reads: silence f32 [batch, rows] = the sum of the scores over sil_pdf_ids in their order, decibel f32
 * [batch, frames]; rows >= the longest R_b, frames >= the longest T_b */
mis_status mis_fsmn_vad_detect_raw(mis_fsmn_vad*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* silence_out,
                                   int rows, float* decibel_out, int frames);
/* tensors of the last chunk of the last call, f32, zeros behind a row's own rows.  stage 0 fbank [B, F, n_mels], 1 decibel [B, F, 1],
 * 2 features [B, R, input_dim], 3 in_linear1, 4 in_linear2, 5 + 2 i layer i's projection, 6 + 2 i its output, 5 + 2 L out_linear1,
 * 6 + 2 L scores, 7 + 2 L the silence sum [B, R, 1].  dims[3] receives B, rows, width; out NULL for the dims alone. */
mis_status mis_fsmn_vad_tap(mis_fsmn_vad*, int stage, float* out, int64_t capacity, int64_t* dims);

/* ------------------------------------------------------------------------------------------
 * SenseVoice speech-to-text (Sources/MLXAudioSTT/Models/SenseVoice/SenseVoiceModel.swift, SenseVoiceAudio.swift; DSP.swift melFilters /
 * hammingWindow / hanningWindow): a non-autoregressive CTC recogniser that also returns the language, emotion and audio event of a
 * clip.  Mono rows of differing lengths at the model's sample rate, 1..max_batch a call.  Row b of n_b samples has F_b = 1 + (n_b - win)
 * / hop fbank frames (0 below one window) and T_b = 4 + ceil(F_b / lfr_n) sequence rows; a row without frames is its four query rows.
 * Front end: x 32768 iff the row's own max |x| <= 1, minus the frame mean, pre-emphasis 0.97 (first sample x0 - 0.97 x0), symmetric
 * Hamming (Hann when window_hann), 512-point power spectrum over 257 bins, unnormalised HTK triangles from 20 Hz, log max(., 1e-10).
 * Sequence row 0 embed[lid], rows 1, 2 embed[1], embed[2], row 3 embed[textnorm], row r >= 4 the fbank frames
 * clamp((r - 4) lfr_n + i - (lfr_m - 1) / 2, 0, F_b - 1), i < lfr_m, then (x + shift) scale when cmvn.shift / cmvn.scale are loaded; all of
 * it x sqrt(output_size) + the sinusoid of position r + 1.  Encoder: L = 1 + max(num_blocks - 1, 0) + tp_blocks SAN-M layers
 * {LayerNorm, linear_q_k_v, attention over the row's own T_b keys, linear_out + v + depthwise_conv(v) [+ residual, not in layer 0],
 * LayerNorm, w_2(relu(w_1)), + residual}, after_norm behind the first stack, tp_norm at the end; head ctc_lo.  All of it exact f32.
 * The workspace is sized once, at finalize, from max_batch, max_seconds and head_rows; a call allocates nothing and generate
 * synchronises once.  A row's result does not depend on the batch it travels in or on what lies behind lens[b]: bit for bit.
 * Rejected with MIS_ERR_INVALID_INPUT at create: a head size above 128, kernel_size above 32, n_mels above 128, input_size !=
 * n_mels x lfr_m, a window outside 257..512 samples (the next power of two must be 512), sizes outside the ranges the messages name;
 * at finalize a tensor missing or misshapen; at a call batch outside 1..max_batch, a row longer than stride or than max_seconds (rows are
 * never truncated), query ids outside 0..15, a null pointer, a handle that is not finalized.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_sensevoice mis_sensevoice;
/* SenseVoiceConfig + SenseVoiceEncoderConfig + SenseVoiceFrontendConfig; window_hann: the window's name contains "hann"; max_batch /
 * max_seconds size the workspace, head_rows the logits scratch of forward (frames a chunk) */
typedef struct {
    int32_t vocab_size, input_size, output_size, attention_heads, linear_units, num_blocks, tp_blocks, kernel_size, sanm_shift, normalize_before;
    int32_t sample_rate, n_mels, frame_length, frame_shift, lfr_m, lfr_n, window_hann;
    int32_t max_batch, max_seconds, head_rows;
} mis_sensevoice_config;
mis_status mis_sensevoice_create(const mis_sensevoice_config*, int device, mis_sensevoice** out);
/* names as SenseVoiceModel.sanitize leaves them: embed.weight [16, input_size]; encoder.{encoders0.0, encoders.N, tp_encoders.N}.
 * {self_attn.linear_q_k_v, self_attn.linear_out, feed_forward.w_1, feed_forward.w_2, norm1, norm2}.{weight,bias} and
 * .self_attn.fsmn_block.weight [output_size, kernel_size, 1] (the torch layout [output_size, 1, kernel_size] holds the same values in the
 * same order and is taken as well); encoder.after_norm / encoder.tp_norm.{weight,bias}; ctc_lo.{weight,bias}; optional cmvn.shift /
 * cmvn.scale of input_size values; host pointers.  finalize names a missing weight and checks every shape. */
mis_status mis_sensevoice_set_tensor(mis_sensevoice*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_sensevoice_init_synthetic(mis_sensevoice*, uint64_t seed);
mis_status mis_sensevoice_finalize(mis_sensevoice*);
void       mis_sensevoice_destroy(mis_sensevoice*);
/* kernel launches of the last call: generate 7 + 5 L (peak, fbank, intake, five a layer - LayerNorm + linear_q_k_v; attention; linear_out
 * + memory block + residual; LayerNorm + w_1 + ReLU; w_2 + residual - after_norm, tp_norm, head + arg-max, decode); forward 5 + 5 L + 2 per
 * chunk of head_rows; forward_features 3 + 5 L + 2 per chunk; features 3 */
int        mis_sensevoice_launches(const mis_sensevoice*);
/* F_b and T_b of rows of lens[b] samples (either output may be NULL) */
mis_status mis_sensevoice_frames(const mis_sensevoice*, const int64_t* lens, int batch, int32_t* frames_out, int32_t* rows_out);
/* pcm f32 [batch, stride], lens[batch] (NULL = stride) -> the LFR + CMVN features extractFeatures returns, f32 [batch, rows, input_size];
 * rows >= max(1, the longest row's T_b - 4), zeros behind a row's own */
mis_status mis_sensevoice_features(mis_sensevoice*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* features_out, int rows);
/* callAsFunction on given features f32 [batch, rows, input_size], counts[batch] valid rows each (NULL = rows); lid / textnorm: rows of
 * the embedding (language 0 auto, 3 zh, 4 en, 7 yue, 11 ja, 12 ko, 13 nospeech; 14 with ITN, 15 without) -> log-probabilities f32
 * [batch, 4 + rows, vocab_size], zeros behind a row's own.  Walks the (row, frame) space in chunks of head_rows frames. */
mis_status mis_sensevoice_forward_features(mis_sensevoice*, const float* features, const int32_t* counts, int batch, int rows, int lid, int textnorm,
                                           float* logp_out);
/* front end + callAsFunction: log-probabilities f32 [batch, Tmax, vocab_size], Tmax the longest row's T_b */
mis_status mis_sensevoice_forward(mis_sensevoice*, const float* pcm, const int64_t* lens, int batch, int64_t stride, int lid, int textnorm,
                                  float* logp_out);
/* generate for a ragged batch.  The head's epilogue reduces every 64-column tile to (max, lowest index attaining it) per frame - no
 * logit reaches memory - and one kernel combines the tiles in tile order (ties to the lower index), reads frames 0, 1, 2 as the
 * language, emotion and event ids (rich_out int32 [batch, 3]) and collapses frames 4.. : a token is kept when it differs from the
 * previous frame's and is not blank 0.  tokens_out int32 [batch, tokens_stride] and n_tokens[batch] are the caller's; a row's ids behind
 * tokens_stride are dropped (Tmax - 4 always suffices).  One synchronisation per call. */
mis_status mis_stt_sensevoice_generate(mis_sensevoice*, const float* pcm, const int64_t* lens, int batch, int64_t stride, int lid, int textnorm,
                                       int32_t* tokens_out, int64_t tokens_stride, int32_t* n_tokens, int32_t* rich_out);
/* tensors of the last call, f32, zeros behind a row's own rows.  stage 0 fbank [B, Fmax, n_mels] (a call from pcm), 1 the intake
 * [B, Tmax, input_size], 2 + i the stages of the encoder in the order they run, [B, Tmax, output_size]: the layers of the first stack,
 * after_norm, the tp layers, tp_norm (stages 2 .. 3 + L).  dims[3] receives B, rows, width; out NULL for the dims alone. */
mis_status mis_sensevoice_tap(mis_sensevoice*, int stage, float* out, int64_t capacity, int64_t* dims);

/* ------------------------------------------------------------------------------------------
 * Silero voice activity detection (Sources/MLXAudioVAD/Models/SileroVAD/SileroVAD.swift): mono rows of differing lengths at 16 kHz or
 * 8 kHz (two branches with their own weights), 1..max_batch a call, of ANY length -> one speech probability per chunk of chunk_size
 * samples (32 ms).  Row b of n_b samples has ceil(n_b / chunk_size) chunks; chunk j's window is samples [j chunk - context, (j + 1) chunk)
 * of the row, zeros before sample 0 and behind sample n_b, then `pad` samples reflected on the right (padded[n + i] = w[n - 2 - i], NOT
 * torch's reflect).  Per window: stft_conv (1 -> 2 cutoff, kernel filter_length, stride hop_length) + magnitude, conv1..conv4 (k3; strides
 * 1, 2, 2, 1; zero-padded inside the chunk) + ReLU, LSTM 128 -> 128 (gates i, f, g, o) carrying (h, c) from the previous chunk,
 * sigmoid(final_conv(relu(h))) averaged over the chunk's LSTM steps (one at the published branches).  All of it exact f32.
 * The chunks of a call are walked in passes of max_chunks inside one workspace sized at finalize, with the state carried on the device -
 * a call allocates nothing and synchronises once.  A row's probabilities and final state do not depend on the batch it travels in, on
 * what lies behind lens[b], on max_chunks, or on whether it came through predict or chunk by chunk through forward: bit for bit.
 * The thresholding into timestamps and segments is host work (vad.py).
 * Rejected with MIS_ERR_INVALID_INPUT at create: a window (context + chunk) no longer than pad, a padded window shorter than the filter,
 * sizes outside the ranges the messages name; at set_tensor an unknown name, a second tensor of a name, a wrong shape; at finalize a
 * missing tensor; at a call a sample rate other than 16000 / 8000, batch outside 1..max_batch, a row longer than stride, too little
 * room in an output, a null pointer, a handle that is not finalized.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_silero_vad mis_silero_vad;
/* SileroVADBranchConfig */
typedef struct {
    int32_t sample_rate, filter_length, hop_length, pad, cutoff, context_size, chunk_size;
} mis_silero_vad_branch_config;
typedef struct {
    mis_silero_vad_branch_config branch16k, branch8k;   /* served at sample_rate 16000 / 8000 */
    int32_t max_batch, max_chunks;                      /* 1..64 rows a call; chunks a pass (1..65536) */
} mis_silero_vad_config;
mis_status mis_silero_vad_create(const mis_silero_vad_config*, int device, mis_silero_vad** out);
/* names as SileroVAD.sanitize leaves them: branch16k. / branch8k. + stft_conv.weight [2 cutoff, filter_length, 1], conv1.weight
 * [128, 3, cutoff], conv2.weight [64, 3, 128], conv3.weight [64, 3, 64], conv4.weight [128, 3, 64], convN.bias, lstm.Wx / lstm.Wh
 * [512, 128], lstm.bias [512], final_conv.weight [1, 1, 128], final_conv.bias [1]; host pointers.  Every name is set exactly once and
 * its shape is checked at the call; finalize names a missing one. */
mis_status mis_silero_vad_set_tensor(mis_silero_vad*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_silero_vad_init_synthetic(mis_silero_vad*, uint64_t seed);
mis_status mis_silero_vad_finalize(mis_silero_vad*);
void       mis_silero_vad_destroy(mis_silero_vad*);
/* kernel launches of the last call: 7 a pass (STFT + magnitude, conv1..conv4, Wx, the recurrence) */
int        mis_silero_vad_launches(const mis_silero_vad*);
/* chunks of rows of lens[b] samples at that sample rate */
mis_status mis_silero_vad_chunks(const mis_silero_vad*, const int64_t* lens, int batch, int sample_rate, int32_t* chunks_out);
/* predictProba of a ragged batch: pcm f32 [batch, stride], lens[batch] (NULL = stride) -> probs f32 [batch, cols], cols >= the longest
 * row's chunks, zeros behind a row's own.  state f32 [2, batch, 128] (h, c): state_in NULL = zeros, state_out NULL = not returned.  A
 * batch of empty rows launches nothing and passes the state through. */
mis_status mis_silero_vad_predict(mis_silero_vad*, const float* pcm, const int64_t* lens, int batch, int64_t stride, int sample_rate,
                                  float* probs_out, int cols, const float* state_in, float* state_out);
/* SileroVAD.callAsFunction, one chunk: windows f32 [batch, context_size + chunk_size] -> probs f32 [batch] and the new state */
mis_status mis_silero_vad_forward(mis_silero_vad*, const float* windows, int batch, int sample_rate, const float* state_in, float* probs_out,
                                  float* state_out);
/* tensors of the last pass of the last call, f32, zeros behind a row's own chunks.  stage 0 magnitude [B, P F, cutoff], 1 conv1
 * [B, P F, 128], 2 conv2 [B, P F2, 64], 3 conv3 [B, P F3, 64], 4 conv4 [B, P F3, 128], 5 the gate pre-activations Wx x + bias
 * [B, P S, 512], 6 the probabilities [B, P, 1]; P the pass's chunks.  dims[3] receives B, rows, width; out NULL for the dims alone. */
mis_status mis_silero_vad_tap(mis_silero_vad*, int stage, float* out, int64_t capacity, int64_t* dims);

/* ------------------------------------------------------------------------------------------
 * MossFormer2-SE speech enhancement (csrc/mossformer2.hip; MLXAudioSTS/Models/MossFormer2SE): noisy waveform -> enhanced waveform.
 * Row b of n_b samples has T_b = n_b < win_len ? 0 : 1 + (n_b - win_len) / win_inc frames and (T_b - 1) win_inc + min(win_len, fft_len)
 * output samples (0 without a frame).  Front end: x 32768, per frame minus its mean, pre-emphasis (first sample x0 - c x0), symmetric
 * Hamming / Hann window, FFT of nextpow2(win_len) points, power, Hz triangles from 20 Hz to Nyquist (the Nyquist bin included,
 * unnormalised), log max(., 1e-10); features = [fbank | delta | delta-delta], the 5-tap filter with edge padding.  Mask network:
 * GlobalLayerNorm over the row, conv1d_encoder, scaled sinusoidal positions, num_blocks x (FLASH layer, GatedFSMNBlock), two LayerNorms
 * + skip, PReLU, conv1d_out (speaker 0: the first out_channels outputs, all the reference returns), tanh(output) x sigmoid(output_gate),
 * conv1_decoder, ReLU.  Synthesis: windowed frames of the x 32768 waveform, fft_len-point transform (any even length), x mask,
 * inverse transform, x window, overlap-add, / max(sum w^2, 1e-8), / 32768.  All of it exact f32.  One workspace is sized at finalize
 * for max_batch rows of max_samples: a call allocates nothing and synchronises once; a row's result does not depend on the batch it
 * travels in or on what lies behind lens[b], bit for bit.
 * Rejected with MIS_ERR_INVALID_INPUT at create: win_len outside 33..2048, win_inc > win_len, an odd fft_len, out_channels_final !=
 * fft_len / 2 + 1, in_channels != 3 num_mels, out_channels no multiple of 16, sizes outside the ranges the messages name; at finalize
 * a tensor missing or misshapen; at a call batch outside 1..max_batch, a row longer than stride or max_samples, too little room in an
 * output, a null pointer, a handle that is not finalized.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_mossformer2 mis_mossformer2;
/* the fields of MossFormer2SEConfig the engine reads + the sizes of the workspace */
typedef struct {
    int32_t sample_rate, win_len, win_inc, fft_len, num_mels, win_hann, in_channels, out_channels, out_channels_final, num_blocks;
    int32_t max_batch;                   /* 1..64 rows a call */
    float   preemphasis;
    int64_t max_samples;                 /* the longest row a call may carry */
} mis_mossformer2_config;
mis_status mis_mossformer2_create(const mis_mossformer2_config*, int device, mis_mossformer2** out);
/* names below "model.mossformer." of a sanitized checkpoint (norm.weight, conv1d_encoder.weight, pos_enc.inv_freq,
 * mdl.intra_mdl.mossformerM.layers.N.to_hidden.linear.weight, ...); conv weights [out, 1, in], depthwise taps [C, 17, 1] and [C, 39, 1, 1],
 * scalars as [1]; host pointers; f32 / f16 / bf16, widened to f32.  finalize names a missing weight and checks every shape. */
mis_status mis_mossformer2_set_tensor(mis_mossformer2*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_mossformer2_init_synthetic(mis_mossformer2*, uint64_t seed);
mis_status mis_mossformer2_finalize(mis_mossformer2*);
void       mis_mossformer2_destroy(mis_mossformer2*);
/* kernel launches of the last call: enhance 11 + 18 num_blocks, mask 8 + 18 num_blocks, mask_features 6 + 18 num_blocks, features 2,
 * synthesize 3; 0 when no row had a frame */
int        mis_mossformer2_launches(const mis_mossformer2*);
/* T_b and the output length of rows of lens[b] samples (either output may be NULL) */
mis_status mis_mossformer2_frames(const mis_mossformer2*, const int64_t* lens, int batch, int32_t* frames_out, int64_t* out_lens);
/* pcm f32 [batch, stride], lens[batch] (NULL = stride) -> features f32 [batch, rows, 3 num_mels]; rows >= the longest row's T_b, zeros
 * behind a row's own.  A batch of rows below one window launches nothing and writes nothing. */
mis_status mis_mossformer2_features(mis_mossformer2*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* features_out,
                                    int rows);
/* the mask network on given features f32 [batch, rows, in_channels], counts[batch] valid rows each (NULL = rows) -> mask f32
 * [batch, rows, out_channels_final], zeros behind a row's own */
mis_status mis_mossformer2_mask_features(mis_mossformer2*, const float* features, const int32_t* counts, int batch, int rows, float* mask_out);
/* front end + mask network: mask f32 [batch, rows, out_channels_final] */
mis_status mis_mossformer2_mask(mis_mossformer2*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* mask_out, int rows);
/* MossFormer2SEModel.enhance for a ragged batch: out f32 [batch, out_stride], out_lens[batch] (may be NULL); zeros behind a row's own */
mis_status mis_mossformer2_enhance(mis_mossformer2*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* out,
                                   int64_t out_stride, int64_t* out_lens);
/* the synthesis alone with a given mask f32 [batch, rows, out_channels_final], rows = the longest row's T_b */
mis_status mis_mossformer2_synthesize(mis_mossformer2*, const float* pcm, const int64_t* lens, int batch, int64_t stride, const float* mask,
                                      int rows, float* out, int64_t out_stride, int64_t* out_lens);
/* tensors of the last call, f32 [B, rows, width], zeros behind a row's own rows.  With L = num_blocks: stage 0 fbank, 1 features,
 * 2 GlobalLayerNorm, 3 encoder + positions, 4 + 2 i FLASH layer i, 5 + 2 i GatedFSMNBlock i; from base = 4 + 2 L: + 0 LayerNorms + skip +
 * PReLU, + 1 conv1d_out (speaker 0), + 2 tanh(output) | sigmoid(output_gate), + 3 mask, + 4 spectrum [re | im], + 5 windowed
 * synthesis frames, + 6 waveform [B, samples, 1]; base + 7 + k, k = 0..12: the last block's inner stages (csrc/mossformer2.hip lists
 * them).  dims[3] receives B, rows, width; out NULL for the dims alone. */
mis_status mis_mossformer2_tap(mis_mossformer2*, int stage, float* out, int64_t capacity, int64_t* dims);

/* ------------------------------------------------------------------------------------------
 * DeepFilterNet V2 / V3 speech enhancement, offline (csrc/deepfilternet.hip; MLXAudioSTS/Models/DeepFilterNet): noisy waveform ->
 * enhanced waveform of the same length.  Row b of n_b samples is padded with hop_size zeros in front and fft_size zeros behind (in the
 * operand load) and has T_b = 1 + (hop_size + n_b) / hop_size frames.  Analysis: Vorbis window, fft_size-point transform, x wnorm =
 * 2 hop / fft^2.  Features: ERB energies (erb_fb [freq_bins, nb_erb] as a contraction when the checkpoint has it, else band means over
 * erb_widths), 10 log10(. + 1e-10), and the two exponential normalisations as the recurrence s_t = a s_(t-1) + (1 - a) x_t (band mean:
 * state linspace(-60, -90), / 40; complex unit norm of the first nb_df bins: state linspace(1e-3, 1e-4), / sqrt(max(s, 1e-12))).
 * Network: the look-ahead shift, causal convs (time kernel 1..5, frequency kernel 1 or 3, grouped / depthwise in the operand load of
 * their pointwise conv, BatchNorm folded at finalize), three squeezed GRUs (grouped linear_in, every GRU layer the checkpoint has, one
 * launch a layer for all frames of all rows; linear_out where present), ERB decoder -> mask [T, nb_erb], DF decoder -> coefficients
 * [T, nb_df, df_order, 2], lsnr.  Synthesis: bins >= nb_df: spec x (mask @ erb_inv_fb); bins < nb_df: the deep filter of the unmasked
 * spec; / wnorm, inverse transform, window, overlap-add / max(sum w^2, 1e-8), the first fft_size - hop_size samples dropped, n_b
 * samples kept, clip to [-1, 1].  All of it exact f32.  One workspace is sized at finalize for max_batch rows of max_samples: a call
 * allocates nothing and synchronises once; a row's result does not depend on the batch it travels in or on what lies behind lens[b],
 * bit for bit.  Not served: DeepFilterNet (V1), enc_concat.  Hop-by-hop streaming: mis_deepfilternet_stream_* below.
 * Rejected with MIS_ERR_INVALID_INPUT at create: sizes outside the ranges the messages name, a hidden size other than 32 / 64 / 128 /
 * 256 (the recurrence kernel's instantiations), erb_widths that do not sum to freq_bins; at finalize a tensor missing or misshapen, a
 * kernel size outside the served ones; at a call batch outside 1..max_batch, a row longer than stride or max_samples, too little room
 * in an output, a null pointer, a handle that is not finalized.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_deepfilternet mis_deepfilternet;
/* the fields of DeepFilterNetConfig the engine reads + the sizes of the workspace.  emb_num_layers .. df_pathway_kernel_size_t only
 * shape init_synthetic's weights: a checkpoint's layer counts, groups and kernel sizes are taken from its tensors. */
typedef struct {
    int32_t sample_rate, fft_size, hop_size, nb_erb, nb_df, df_order, df_lookahead, conv_lookahead, conv_ch, emb_hidden_dim, df_hidden_dim;
    int32_t lsnr_max, lsnr_min;
    int32_t emb_num_layers, df_num_layers, linear_groups, enc_linear_groups, conv_kernel[2], convt_kernel[2], conv_kernel_inp[2],
            df_pathway_kernel_size_t;
    int32_t gru_kr;                      /* columns of Wh a thread keeps in registers at hidden size 256: 64, 96, 128; 0 = the default */
    int32_t max_batch;                   /* 1..64 rows a call */
    float   norm_alpha;                  /* computeNormAlpha(hop_size, sample_rate) */
    int32_t erb_widths[128];             /* the first nb_erb: bins of every band, summing to fft_size / 2 + 1 */
    int64_t max_samples;                 /* the longest row a call may carry */
} mis_deepfilternet_config;
mis_status mis_deepfilternet_create(const mis_deepfilternet_config*, int device, mis_deepfilternet** out);
/* names as the reference reads them (mask.erb_inv_fb, erb_fb, enc.erb_conv0.1.weight, enc.emb_gru.gru.weight_hh_l0,
 * df_dec.df_out.0.weight, ...) in the torch layouts: Conv2d [out, in / groups, kT, kF], ConvTranspose2d [in, out / groups, kT, kF],
 * grouped linears [groups, in / groups, out / groups], GRU [3 H, in] with gates r | z | n; host pointers; f32 / f16 / bf16, widened
 * to f32.  finalize names a missing weight and checks every shape. */
mis_status mis_deepfilternet_set_tensor(mis_deepfilternet*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_deepfilternet_init_synthetic(mis_deepfilternet*, uint64_t seed);
mis_status mis_deepfilternet_finalize(mis_deepfilternet*);
void       mis_deepfilternet_destroy(mis_deepfilternet*);
/* kernel launches of the last call: 26 + [erb_fb] + [df_skip] + [enc linear_out] + [erb_dec linear_out] + 2 L_enc + L_erb + L_df +
 * (emb_hidden_dim == df_hidden_dim ? max(L_erb, L_df) : L_erb + L_df), L_. the GRU layers of the three chains */
int        mis_deepfilternet_launches(const mis_deepfilternet*);
/* T_b and the output length (= lens[b]) of rows of lens[b] samples (either output may be NULL) */
mis_status mis_deepfilternet_frames(const mis_deepfilternet*, const int64_t* lens, int batch, int32_t* frames_out, int64_t* out_lens);
/* DeepFilterNetModel.enhance for a ragged batch: pcm f32 [batch, stride], lens[batch] (NULL = stride) -> out f32 [batch, out_stride]
 * (out_stride >= the longest row, at least 1), out_lens[batch] (may be NULL), lsnr f32 [batch, lsnr_rows] per frame (may be NULL;
 * lsnr_rows >= the longest row's T_b); zeros behind a row's own */
mis_status mis_deepfilternet_enhance(mis_deepfilternet*, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* out,
                                     int64_t out_stride, int64_t* out_lens, float* lsnr_out, int lsnr_rows);
/* tensors of the last call, f32 [B, rows, width], zeros behind a row's own rows; width = frequency x channel, channel fastest.
 * stage 0 spec [re F | im F], 1 ERB feature [nb_erb], 2 complex feature [nb_df, 2], 3..6 e0..e3, 7 c0, 8 c1, 9 emb in front of the
 * encoder GRU, 10 emb behind it (after linear_out), 11 lsnr, 12 the ERB decoder's squeezed GRU (after linear_out), 13 relu(conv3p) +
 * that, 14 convt3, 15 relu(conv2p) + 14, 16 convt2, 17 relu(conv1p) + 16, 18 convt1, 19 relu(conv0p) + 18, 20 mask [nb_erb], 21 the DF
 * decoder's GRU output (+ df_skip), 22 c0p [nb_df, 2 df_order], 23 coefficients [nb_df, df_order, 2], 24 enhanced spec / wnorm
 * [re F | im F], 25 waveform [B, samples, 1], 26 ERB energies in dB (with erb_fb only); 32 + 16 chain + 0 linear_in, + 1 + l GRU layer
 * l, chain 0 enc.emb_gru, 1 erb_dec.emb_gru, 2 df_dec.df_gru.  dims[3] receives B, rows, width; out NULL for the dims alone. */
mis_status mis_deepfilternet_tap(mis_deepfilternet*, int stage, float* out, int64_t capacity, int64_t* dims);

/* DeepFilterNet hop by hop (csrc/deepfilternet_stream.hip; DeepFilterNetStreamer.processChunk / flush / reset of the reference):
 * 1..max_batch streams on one finalized model, with a workspace of their own (mis_deepfilternet_enhance and feeds may interleave; the
 * model outlives its streams).  Semantics, the engine's own:
 *   Framing.  A stream is a sequence of whole hops.  After h hops the frames 0..h-1 exist; frame k is hops k-1, k, with zeros for hop
 *   -1: offline frame k of the same samples.  With L = conv_lookahead, target frame t is computed once frame t + L exists.
 *   Emission.  Target t emits its hop_size finished overlap-add samples (padded samples [t hop, (t + 1) hop): the first target's are the
 *   fft_size - hop_size samples the offline call drops) through the offline expression: partial sums in frame order, / max(sum w^2,
 *   1e-8), clip to [-1, 1].  The reference's processChunk neither divides nor clips; for the Vorbis window at fft = 2 hop the divisor is
 *   sin^2 + cos^2 = 1 up to rounding, and its enhanceStreaming clips the concatenation.
 *   State, on the device per stream: the last fft - hop input samples; both normalisation states (nb_erb + nb_df floats, from the
 *   linspace expressions above at hop 0); kT - 1 input frames of every conv with a time kernel above 1; h of every GRU layer; the
 *   unmasked spec frames t - (df_order - df_lookahead - 1) .. t + L (the deep filter's reach and the frames waiting for their
 *   look-ahead); the last synthesis frame (the overlap-add tail).  The hop counter is kept by the host.
 *   Yardstick.  After H hops in any chunking a stream has returned (H - L) hop samples (0 when negative) and H - L lsnr values.  With
 *   x the samples fed, returned sample hop + s equals mis_deepfilternet_enhance(x)[s], and lsnr value t the offline lsnr of frame t,
 *   bit for bit: every output element is the same fixed-order sum, zero history equals zero padding, and a sum continued from a
 *   carried partial has the order of the offline sum.  A stream's result does not depend on its slot, on what the other streams bring
 *   or on what lies behind its hops in pcm; a stream that brings 0 hops is untouched.
 * A feed allocates nothing and synchronises once.  Feeds whose longest stream has at most 4 targets run the recurrence in its
 * short-chunk form (every column of Wh streamed from the transposed copy, no register slice to fill), longer ones in the offline form:
 * the same accumulation order, the same bits.
 * Rejected with MIS_ERR_INVALID_INPUT at create: a model that is not finalized, streams outside 1..max_batch, max_hops outside 1..256,
 * fft_size != 2 hop_size (the offline frame grid and the streamer's analysis memory coincide at this ratio only), df_lookahead >
 * conv_lookahead (the deep filter would read frames that have not arrived); at a feed a null pointer, hops outside 0..max_hops, too
 * little room in pcm, out or lsnr. */
typedef struct mis_deepfilternet_stream mis_deepfilternet_stream;
mis_status mis_deepfilternet_stream_create(mis_deepfilternet*, int streams, int max_hops, mis_deepfilternet_stream** out);
void       mis_deepfilternet_stream_destroy(mis_deepfilternet_stream*);
/* stream 0..streams-1, or -1 for all: zero history, hop counter 0 */
mis_status mis_deepfilternet_stream_reset(mis_deepfilternet_stream*, int stream);
/* pcm f32 [streams, stride], stream b brings hops[b] whole hops (0..max_hops) -> out f32 [streams, out_stride], out_lens[streams] (hop_size
 * samples for every target that became ready), lsnr f32 [streams, lsnr_rows] and lsnr_counts[streams] (both NULL, or both given) */
mis_status mis_deepfilternet_stream_feed(mis_deepfilternet_stream*, const float* pcm, const int32_t* hops, int64_t stride, float* out,
                                         int64_t out_stride, int64_t* out_lens, float* lsnr_out, int lsnr_rows, int32_t* lsnr_counts);
/* kernel launches of the last feed: the offline count + 1 (the history roll); launches without a row are skipped (no targets yet: the
 * front end and the roll only); 0 when no stream brought a hop */
int        mis_deepfilternet_stream_launches(const mis_deepfilternet_stream*);
/* hops a stream has been fed since create or its last reset (-1: bad argument) */
int64_t    mis_deepfilternet_stream_hops_seen(const mis_deepfilternet_stream*, int stream);

/* ------------------------------------------------------------------------------------------
 * Sortformer speaker diarization (csrc/sortformer.hip; Sources/MLXAudioVAD/Models/Sortformer/Sortformer.swift, SortformerConfig.swift,
 * SortformerFeatures.swift): "who spoke when" for up to num_speakers speakers.  16 kHz mono rows of differing lengths, 1..max_batch a
 * call.  Row b of n_b samples has F_b = 1 + n_b / 160 feature frames (per-call options: peak normalisation x / (max|x| + 1e-3);
 * pre-emphasis, symmetric Hann window of 400 in 512, 256 zeros on each side, power spectrum, slaney filters, log(. + 2^-24);
 * normalize: per-bin mean / unbiased variance over the row's own frames, (x - mean) / (std + 1e-5); pad_to: zero frames appended after
 * the normalisation up to a multiple of it, which count as frames of the row), then T_b = the three-fold floor((L - 1) / 2) + 1 of F_b
 * diarization frames behind the depthwise-striding Conv2d stem, the FastConformer blocks (Transformer-XL relative-position attention
 * with bias_u / bias_v and a per-layer relative_k_proj over the row's own T_b keys; GLU -> depthwise conv -> inference BatchNorm ->
 * SiLU), encoder_proj + embed_positions, the post-LN BART layers (keys limited to the row's own count) and the speaker sigmoids.
 * All of it exact f32.  A row's result does not depend on the batch it travels in, on the longest row, or on what lies behind
 * lens[b]: bit for bit.  The workspace is sized once, at finalize, from max_batch and max_seconds; a call allocates nothing and
 * synchronises once.  The streaming state (speaker cache, FIFO, compression) is host work (sortformer.py) over pre_encode and
 * encode_embeddings.
 * Limits, MIS_ERR_INVALID_INPUT at create with a message naming the field: sampling_rate / n_fft / hop_length / win_length 16000 / 512 /
 * 160 / 400; num_mel_bins 8..256; subsampling_factor / subsampling_conv_kernel_size / subsampling_conv_stride 8 / 3 / 2;
 * subsampling_conv_channels 1..1024; hidden_size and d_model 8..4096; both head sizes whole numbers up to 64; num_key_value_heads =
 * num_attention_heads; intermediate_size, encoder_ffn_dim 1..16384; both depths 1..64; conv_kernel_size odd, 3..31; fc_d_model /
 * tf_d_model of the modules equal to hidden_size / d_model; num_speakers 1..64; max_batch 1..64; max_seconds 1..120.  At finalize: a
 * tensor missing or misshapen.  At a call, before any launch: batch outside 1..max_batch, a row longer than stride or max_seconds,
 * more frames than the workspace or max_source_positions hold, a count outside 1..the row stride, pad_to not 0 or a divisor of 16, a
 * null pointer.  A rejected call leaves the handle usable.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_sortformer mis_sortformer;
/* FCEncoderConfig, TFEncoderConfig, ModulesConfig (fc_d_model, tf_d_model_modules = its tf_d_model, num_speakers) and ProcessorConfig
 * fields the engine reads; max_batch / max_seconds size the workspace */
typedef struct {
    int32_t hidden_size, num_hidden_layers, num_attention_heads, num_key_value_heads, intermediate_size, num_mel_bins, conv_kernel_size,
            subsampling_factor, subsampling_conv_channels, subsampling_conv_kernel_size, subsampling_conv_stride, attention_bias, scale_input;
    int32_t tf_d_model, encoder_layers, encoder_attention_heads, encoder_ffn_dim, max_source_positions, k_proj_bias;
    int32_t num_speakers, fc_d_model, tf_d_model_modules;
    int32_t sampling_rate, hop_length, n_fft, win_length;
    int32_t max_batch, max_seconds;
    float   layer_norm_eps, preemphasis;
} mis_sortformer_config;
mis_status mis_sortformer_create(const mis_sortformer_config*, int device, mis_sortformer** out);
/* names as SortformerModel.sanitize leaves them: fc_encoder.subsampling.{layers_0,layers_2,layers_3,layers_5,layers_6,linear}.*,
 * fc_encoder.layers.N.{feed_forward1,feed_forward2}.{linear1,linear2}.*, .self_attn.{q,k,v,o}_proj.*, .self_attn.relative_k_proj.weight,
 * .self_attn.{bias_u,bias_v}, .conv.{pointwise_conv1,depthwise_conv,pointwise_conv2}.*, .conv.norm.{weight,bias,running_mean,running_var},
 * .norm_{feed_forward1,self_att,conv,feed_forward2,out}.*, tf_encoder.embed_positions.weight, tf_encoder.layers.N.self_attn.{q,k,v,out}_proj.*,
 * .{self_attn_layer_norm,final_layer_norm}.*, .{fc1,fc2}.*, sortformer_modules.{encoder_proj,first_hidden_to_hidden,single_hidden_to_spks,
 * hidden_to_spks}.*; Conv2d weights [out, 3, 3, in / groups], Conv1d weights [out, k, in / groups]; host pointers.  finalize names a
 * missing weight and checks every shape (hidden_to_spks too, which nothing reads, as in the reference). */
mis_status mis_sortformer_set_tensor(mis_sortformer*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_sortformer_init_synthetic(mis_sortformer*, uint64_t seed);
mis_status mis_sortformer_finalize(mis_sortformer*);
void       mis_sortformer_destroy(mis_sortformer*);
/* kernel launches of the last call, with L_fc = num_hidden_layers and L_tf = encoder_layers: forward 11 + 15 L_fc + 7 L_tf,
 * forward_features 8 + 15 L_fc + 7 L_tf, encode_embeddings 4 + 15 L_fc + 7 L_tf, pre_encode 4, features 3 */
int        mis_sortformer_launches(const mis_sortformer*);
/* F_b (pad_to applied) and T_b of rows of lens[b] samples (either output may be NULL); pad_to and a row beyond max_seconds are
 * rejected as by the calls below */
mis_status mis_sortformer_frames(const mis_sortformer*, const int64_t* lens, int batch, int pad_to, int32_t* F_out, int32_t* T_out);
/* pcm f32 [batch, stride], lens[batch] (NULL = stride) -> features f32 [batch, Fmax, num_mel_bins], Fmax the longest row's frames,
 * zeros behind a row's own F_b */
mis_status mis_sortformer_features(mis_sortformer*, const float* pcm, const int64_t* lens, int batch, int64_t stride, int peak_normalize,
                                   int normalize, int pad_to, float* feats_out);
/* SortformerModel.callAsFunction on given features f32 [batch, F, num_mel_bins], frames[batch] valid frames each (NULL = F) ->
 * probabilities f32 [batch, T of F, num_speakers], zeros behind a row's own T_b */
mis_status mis_sortformer_forward_features(mis_sortformer*, const float* feats, const int32_t* frames, int batch, int F, float* probs_out);
/* front end + callAsFunction: probabilities f32 [batch, T of the longest row, num_speakers].  One synchronisation per call. */
mis_status mis_sortformer_forward(mis_sortformer*, const float* pcm, const int64_t* lens, int batch, int64_t stride, int peak_normalize,
                                  int normalize, int pad_to, float* probs_out);
/* fcEncoder.preEncode: features as above -> the stem's embeddings f32 [batch, T of F, hidden_size] (not scaled by sqrt(hidden_size)) */
mis_status mis_sortformer_pre_encode(mis_sortformer*, const float* feats, const int32_t* frames, int batch, int F, float* emb_out);
/* fcEncoder.encode onward, what streamingStep runs on [spkcache, fifo, left, chunk, right]: embeddings f32 [batch, T, hidden_size],
 * counts[batch] valid frames each (NULL = T) -> probabilities f32 [batch, T, num_speakers] */
mis_status mis_sortformer_encode_embeddings(mis_sortformer*, const float* emb, const int32_t* counts, int batch, int T, float* probs_out);
/* tensors of the last call - forward, forward_features, pre_encode or encode_embeddings; after features alone, which leaves no
 * embeddings, the tap is rejected with MIS_ERR_NOT_INITIALIZED - f32, zero rows behind a row's own T_b.  With L = num_hidden_layers, Lt = encoder_layers: stage 0 the stem's
 * embeddings [B, T, hidden_size], 1..L that Conformer block, L + 1 encoder_proj + positions [B, T, d_model], L + 2 .. L + 1 + Lt that BART
 * layer, L + 2 + Lt the probabilities [B, T, num_speakers].  dims[3] receives B, T, width; out NULL for the dims alone. */
mis_status mis_sortformer_tap(mis_sortformer*, int stage, float* out, int64_t capacity, int64_t* dims);

/* ------------------------------------------------------------------------------------------
 * Device groups for the other families ("Whisper (30 s chunks), Soprano (sentence prompts) and Qwen3-TTS rows shard the
 * same way").  replicas[n]: one finalized handle per GPU holding the same weights.  The rows of the call are split into n contiguous
 * blocks (mis_shard_rows), every replica runs its block on its own worker thread through the single-device entry point - with
 * row_offset advanced by the block start, so a row's tokens / samples do not depend on n - and the results are gathered on the host
 * in global row order.  No collective is on the critical path; outputs and ownership are those of the single-device calls.
 * Callbacks are serialised (one at a time, any worker thread) and carry GLOBAL row indices.  Errors: the first failing shard's
 * status, message prefixed "shard r:". */
mis_status mis_whisper_group_generate(mis_whisper* const* replicas, int n, const float* pcm, const int64_t* lens, int batch, int64_t stride,
                                      const int32_t* prompt_ids, int n_prompt, const mis_stt_params*,
                                      int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens);
mis_status mis_soprano_group_generate(mis_soprano* const* replicas, int n, const int32_t* prompt_ids, const int32_t* prompt_lens, int batch,
                                      const mis_gen_params* params, float** pcm_out, int64_t* pcm_stride, int64_t* pcm_lens,
                                      int32_t** tokens_out, int64_t* tokens_stride, int32_t* n_tokens);
/* arguments as mis_qwen3tts_generate; with on_event and chunk_frames > 0 every replica streams its rows' chunks as they are decoded
 * (generateStream): per-rank chunk emission, nothing is exchanged between GPUs.  In-context prompts address reference rows by codec id:
 * register the same reference contexts, in the same order, on every replica (mis_qwen3tts_add_reference). */
mis_status mis_qwen3tts_group_generate(mis_qwen3tts* const* replicas, int n, const int32_t* text_ids, const int32_t* codec_ids,
                                       const int32_t* prefill_lens, int P, const int32_t* trailing_ids, const int32_t* trailing_lens, int Tt,
                                       int batch, const mis_qwen3tts_params* params, const int32_t* row_max_frames, float** pcm_out,
                                       int64_t* pcm_stride, int64_t* pcm_lens, int32_t** codes_out, int64_t* codes_stride,
                                       int32_t* n_frames, int chunk_frames, mis_event_cb on_event, void* user,
                                       const volatile int* cancel_flag);

/* ------------------------------------------------------------------------------------------
 * BigVGAN vocoder (csrc/bigvgan.hip; Sources/MLXAudioCodecs/BigVGAN): mel [batch, num_mels, frames] -> waveform, hop = the product of
 * upsample_rates samples a frame.  conv_pre (7 taps); per stage a weight-normalised transposed conv (kernel 2 x stride, pad stride / 2)
 * and the mean of num_kernels AMP blocks (resblock 1: x + convs2(act(convs1(act(x)))) per dilation; 2: x + convs(act(x))); then
 * activation_post, conv_post (7 taps -> 1 channel) and tanh or clip(-1, 1).  Every act is the anti-aliased Activation1d: 2 x Kaiser-sinc
 * up-sampling with edge padding (12 taps, cutoff 0.25, half width 0.3), Snake / SnakeBeta, 2 x low-pass down-sampling with edge padding.
 * All of it exact f32, weight norm folded at finalize in double.  1..max_batch ragged rows a call, each of 1..max_frames frames, inside
 * one workspace sized at finalize: a call allocates nothing and synchronises once.  A row's waveform does not depend on the batch it
 * travels in or on what lies behind its own frames: bit for bit.
 * Rejected with MIS_ERR_INVALID_INPUT at create: upsample_kernel_sizes[i] != 2 upsample_rates[i], an odd or out-of-range rate, an even
 * resblock kernel or one above 11 taps, a dilation above 5, sizes outside the ranges the messages name; at finalize a tensor missing or
 * misshapen; at a call batch outside 1..max_batch, a stride above max_frames, a frame count outside 1..stride, a null pointer, a handle
 * that is not finalized.
 * ---------------------------------------------------------------------------------------- */
typedef struct mis_bigvgan mis_bigvgan;
/* BigVGANConfig's eleven fields (lists with their counts) + the sizes of the workspace */
typedef struct {
    int32_t num_mels;
    int32_t n_upsamples, upsample_rates[8];
    int32_t n_upsample_kernel_sizes, upsample_kernel_sizes[8];
    int32_t upsample_initial_channel;
    int32_t resblock;                                       /* 1 or 2 */
    int32_t n_resblock_kernels, resblock_kernel_sizes[8];
    int32_t n_resblock_dilations[8], resblock_dilation_sizes[8][8];
    int32_t activation;                                     /* 0 snake, 1 snakebeta */
    int32_t snake_logscale, use_bias_at_final, use_tanh_at_final;
    int32_t max_batch, max_frames;                          /* 1..64 rows a call; mel frames a row */
} mis_bigvgan_config;
mis_status mis_bigvgan_create(const mis_bigvgan_config*, int device, mis_bigvgan** out);
/* the reference's keys and MLX layouts: conv_pre.{weight_g [out, 1, 1], weight_v [out, k, in], bias}, ups.N.0.{weight_g [1, 1, in],
 * weight_v [out, k, in], bias}, resblocks.N.{convs1,convs2}.M.* (resblock 1) or resblocks.N.convs.M.* (2),
 * resblocks.N.activations.M.act.{alpha, beta} [channels], activation_post.act.*, conv_post.* (no bias without use_bias_at_final); beta
 * only for snakebeta; host pointers.  finalize names a missing or misshapen tensor. */
mis_status mis_bigvgan_set_tensor(mis_bigvgan*, const char* name, const void* data, mis_dtype, const int64_t* shape, int ndim);
mis_status mis_bigvgan_init_synthetic(mis_bigvgan*, uint64_t seed);
mis_status mis_bigvgan_finalize(mis_bigvgan*);
void       mis_bigvgan_destroy(mis_bigvgan*);
int        mis_bigvgan_hop(const mis_bigvgan*);           /* samples a mel frame: the product of the rates */
/* kernel launches of the last call: 3 + sum over stages of (2 + sum over AMP blocks of 4 (resblock 1) or 2 (resblock 2) per dilation) */
int        mis_bigvgan_launches(const mis_bigvgan*);
/* mel f32 [batch, num_mels, stride] and frames[batch] (1..stride each; NULL = stride), host -> wav f32 [batch, stride x hop], host;
 * zeros behind a row's own frames[b] x hop samples */
mis_status mis_bigvgan_decode(mis_bigvgan*, const float* mel, const int32_t* frames, int batch, int64_t stride, float* wav_out);
/* tensors of the last call, f32 [B, C, stride x up-sampling so far], zeros behind a row's own samples.  stage 0 conv_pre; with
 * n = num_kernels, 1 + i (n + 2) stage i's transposed conv, + 1 + j its AMP block j, + n + 1 the stage mean; 1 + stages x (n + 2)
 * activation_post.  dims[3] receives B, C, length; out NULL for the dims alone. */
mis_status mis_bigvgan_tap(mis_bigvgan*, int stage, float* out, int64_t capacity, int64_t* dims);

/* Diagnostics and test scaffolding (launch floor, split-factor model, CU spinner, failure counters) are NOT part of the product
 * surface: include/mi_speech_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* MI_SPEECH_H */
