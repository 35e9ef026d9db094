// marvis.hip - Marvis TTS (CSM): backbone LM + depth decoder, one hipGraph replay per 12.5 Hz frame, audio through a borrowed Mimi.
//
// Reference being replaced: CSMModel.generateFrame (Sources/MLXAudioTTS/Models/Marvis/CSMModel.swift:467-526), _embedTokens (:534-557),
// CSMLlamaModel / CSMLlama3ScaledRoPE (CSMLlamaModel.swift:69-170,279-304), the generate loop of MarvisTTSModel.swift:402-477 and its
// loader (:144-263).  The reference syncs with the host once per frame (`frame.sum().item`, :445) and runs batch 1; here a frame of a
// whole batch is one graph: codebook0_head -> sampler -> projection -> depth decoder (2 + Cb - 2 positions of the small LM, one head and
// one sampler launch per codebook) -> frame-end kernel -> the backbone's next position, and the host polls a done counter every 8 frames.
// Both LMs run on the weight-streaming step chain of lm_engine.hip (rope_ops_in_dtype, llama3 rescale on).
//
// Launches per frame (L_b / L_d layers, 7 launches per layer + 1 embed): 1 head + 1 sampler + 1 projection +
// Cb x (7 L_d + 1) decoder chains + (Cb - 1) x 2 head/sampler + 1 frame end + 1 counter + (7 L_b + 1) backbone:
// 1 108 at the published depth (16 / 4 layers) and 32 codebooks, 364 at 8.  mis_marvis_launches_per_frame reports the node count of
// the captured graph (hipGraphGetNodes), which the tests compare with this formula; without a graph (MIS_NO_GRAPH) it is the formula.
//
// Deviations, in summation order / streams only:
//  * the frame input is the masked sum of up to K rows of audio_embeddings (+ the text row) accumulated in FLOAT32 in codebook order and
//    rounded ONCE to bf16 (k_mv_frame_end, k_mv_prompt_rows); MLX's reduction order for sum(axis: 2) on bf16 is third-party and unknown.
//  * NOT built as asked: the frame input is written as row-major bf16 rows (in_emb / pf_rows) and enters the chain through its
//    embed + RMSNorm kernel by an iota id table, as the Qwen3-TTS frame does - not straight into the packed MFMA-B layout.  The cost is
//    the iota table and one extra d-wide round trip per row and frame; the values are the same.
//  * interleaved RoPE (pairs 2i, 2i+1) runs as the engine's half rotation on q / k whose head channels were de-interleaved when the
//    tensor was set (rows of q_proj / k_proj permuted per head, codes / scales / biases alike): q'.k' is the same dot product with its
//    terms in another order.  cos / sin come from marvis_rope_tables (CSM's formula), not from the engine's own.
//  * sampling is mis-sampler-v1 (oracle/sampler.py) keyed by (seed, global row, frame * K + codebook); MLX's categorical stream cannot
//    be reproduced outside MLX.
//  * depth-decoder inputs: audio_embeddings @ projection^T is folded into a [K * audio_vocab][Dd] table at finalize (one gather per
//    codebook instead of a GEMM launch); only projection(lastH) runs per frame.  A QUANTISED projection is dequantised at load and takes
//    the same folded path (its one launch per frame streams bf16 tiles); the embeddings are dequantised at load (gathered tensors).
#include "common.h"
#include "kernels.h"
#include "lm_kernels.h"
#include "quant_intake.h"
#include "sampler_math.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <deque>
#include <functional>
#include <memory>
#include <set>

typedef unsigned long long u64;

struct mis_marvis {
    int device = 0;
    mis_marvis_config cfg{};
    mis_tts* bb = nullptr;                   // backbone
    mis_tts* dec = nullptr;                  // depth decoder
    hipStream_t s = nullptr;
    bool finalized = false;
    int K = 0, Va = 0, VaPad = 0, Vt = 0, d = 0, dd = 0;
    std::set<std::string> loaded;
    int heads_loaded = 0;
    DevBuf<uint8_t> raw;
    DevBuf<bf16_t> stage;
    DevBuf<bf16_t> text_emb, audio_emb, audio_emb_proj, proj_w, heads;     // heads: [K-1] packed [VaPad/16][dd/32][64][8]
    // per-call state
    DevBuf<bf16_t> in_emb, hid_proj, xpk, pf_rows;
    DevBuf<int32_t> iota, ptok, plen, cur_codes, codes, sampled, n_frames, frame, done, row_max, forced;
    DevBuf<uint8_t> pmask;
    DevBuf<float> logits_dbg;
    int last_launches = 0;
};

// ---------------------------------------------------------------------------- CSM RoPE tables
// CSMLlama3ScaledRoPE.ropeInit / applyScaling (CSMLlamaModel.swift:69-104), float32 arithmetic; cos / sin of the float32 angle
void marvis_rope_tables(int D, float base, float factor, float lowf, float highf, float old, int n_pos, float* cs, float* sn) {
    const int half = D / 2;
    std::vector<float> theta(half);
    for (int i = 0; i < half; ++i) {
        const float expo = (float)(2 * i) / (float)D;
        const float freqs = (float)pow((double)base, (double)expo);    // the correctly rounded float32 power (libm powf implementations differ by an ulp)
        const float f = 1.0f / freqs;                                   // invFreqs
        const float wl = (2.0f * (float)M_PI) / f;
        const float low = old / lowf, high = old / highf;
        float smooth = (old / wl - lowf) / (highf - lowf);
        smooth = fminf(fmaxf(smooth, 0.0f), 1.0f);
        const float scaled = f / factor;
        volatile float a = (1.0f - smooth) * scaled, b = smooth * f;    // two roundings, no contraction
        const float blended = a + b;
        theta[i] = wl < high ? f : (wl > low ? scaled : blended);
    }
    for (int p = 0; p < n_pos; ++p)
        for (int i = 0; i < half; ++i) {
            const float ang = (float)p * theta[i];
            cs[(size_t)p * half + i] = (float)cos((double)ang);
            sn[(size_t)p * half + i] = (float)sin((double)ang);
        }
}
extern "C" mis_status mis_debug_marvis_rope_tables(int head_dim, float theta, float factor, float low_freq_factor, float high_freq_factor,
                                                   float old_context_len, int n_pos, float* cos_out, float* sin_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(head_dim >= 2 && head_dim % 2 == 0 && n_pos >= 1 && cos_out && sin_out, MIS_ERR_INVALID_INPUT, "bad argument");
    marvis_rope_tables(head_dim, theta, factor, low_freq_factor, high_freq_factor, old_context_len, n_pos, cos_out, sin_out);
    MIS_API_END
}

// ---------------------------------------------------------------------------- kernels
__global__ void k_mv_iota(int32_t* p, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}
__global__ void k_mv_bump(int* p) { if (threadIdx.x == 0 && blockIdx.x == 0) *p = *p + 1; }

// rows base .. base + n_valid - 1 of `table` ([*][Kd] bf16) -> packed MFMA-B fragments of a [16 MT][Kd] activation
__global__ void k_mv_gather_pack(const bf16_t* __restrict__ table, int Kd, int base, int n_valid, bf16_t* __restrict__ xpk, int MT) {
    const int m = blockIdx.x;
    for (int k = threadIdx.x; k < Kd; k += blockDim.x)
        xpk[xpk_index(m, k, MT)] = m < n_valid ? table[(size_t)(base + m) * Kd + k] : (bf16_t)0;
}
// [Kd][N] -> [N][Kd] (audio_head[i] is used as x @ W: stored transposed relative to a Linear)
__global__ void k_mv_transpose(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int Kd, int N) {
    const int n = blockIdx.x;
    for (int k = threadIdx.x; k < Kd; k += blockDim.x) dst[(size_t)n * Kd + k] = src[(size_t)k * N + n];
}

// masked sum of one token frame (K codes + text id, K + 1 mask bytes) in float32, codebook order then text, one rounding
__device__ __forceinline__ void mv_frame_sum(const int32_t* __restrict__ tok, const uint8_t* __restrict__ msk, int K, int Va,
                                             const bf16_t* __restrict__ audio_emb, const bf16_t* __restrict__ text_emb, int d,
                                             bf16_t* __restrict__ out, int* cs /* LDS [33] row index or -1 */) {
    if (threadIdx.x <= K) {
        const int i = threadIdx.x;
        cs[i] = tok && msk[i] ? (i < K ? i * Va + tok[i] : tok[i]) : -1;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        float e = 0.0f;
        for (int i = 0; i < K; ++i)
            if (cs[i] >= 0) e += bf16_to_f32(audio_emb[(size_t)cs[i] * d + k]);
        if (cs[K] >= 0) e += bf16_to_f32(text_emb[(size_t)cs[K] * d + k]);
        out[k] = f32_to_bf16(e);
    }
}
// the whole right-aligned prompt matrix for the batched prefill: rows[(j * Mpad + b)] = input of row b at its position j - (Lmax - len[b])
__global__ void __launch_bounds__(256) k_mv_prompt_rows(const int32_t* __restrict__ ptok, const uint8_t* __restrict__ pmask,
                                                        const int32_t* __restrict__ plen, int P, int Lmax, int K, int Va,
                                                        const bf16_t* __restrict__ audio_emb, const bf16_t* __restrict__ text_emb,
                                                        bf16_t* __restrict__ rows, int d, int batch, int Mpad) {
    __shared__ int cs[33];
    const int b = blockIdx.x, j = blockIdx.y;
    const int idx = b < batch ? j - (Lmax - plen[b]) : -1;
    const size_t o = idx >= 0 ? ((size_t)b * P + idx) * (K + 1) : 0;
    mv_frame_sum(idx >= 0 ? ptok + o : nullptr, pmask + o, K, Va, audio_emb, text_emb, d, rows + ((size_t)j * Mpad + b) * d, cs);
}
// the same, one position j per launch (quantised mixes / odd widths: the position-by-position prefill); sets the rows' active flags
__global__ void __launch_bounds__(256) k_mv_prompt_feed(const int32_t* __restrict__ ptok, const uint8_t* __restrict__ pmask,
                                                        const int32_t* __restrict__ plen, int P, int Lmax, int j, int K, int Va,
                                                        const bf16_t* __restrict__ audio_emb, const bf16_t* __restrict__ text_emb,
                                                        bf16_t* __restrict__ in_emb, uint8_t* __restrict__ active, int d, int batch) {
    __shared__ int cs[33];
    const int b = blockIdx.x;
    const int idx = b < batch ? j - (Lmax - plen[b]) : -1;
    if (threadIdx.x == 0) active[b] = idx >= 0 ? 1 : 0;
    const size_t o = idx >= 0 ? ((size_t)b * P + idx) * (K + 1) : 0;
    mv_frame_sum(idx >= 0 ? ptok + o : nullptr, pmask + o, K, Va, audio_emb, text_emb, d, in_emb + (size_t)b * d, cs);
}

// packed x (final-norm output of the step chain) is the projection GEMM's operand as it is; nothing to unpack.

struct MvSampleArgs {
    const bf16_t* logits;        // [Mpad][Vpad]
    int Vpad, V;
    float temperature, top_p;
    uint64_t seed;
    int64_t row_offset;
    const int* frame;            // device frame counter; RNG step = frame * K + slot
    int slot, K, Cb;
    int32_t* cur_codes;          // [K][Mpad]: codes the frame continues from (the forced ones under teacher forcing)
    int Mpad;
    const uint8_t* active;
    const int32_t* forced;       // [B][F][Cb] or null
    int F;
    int32_t* sampled;            // [B][F][Cb] what the sampler chose (debug entry) or null
    float* logits_out;           // [B][F][Cb][V] (debug entry) or null
};
#define MV_NT 256
#define MV_PER 16
__device__ __forceinline__ u64 mv_wave_scan(u64 v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// inclusive scan of one u64 per thread over the 256 threads; sh: [4]
__device__ __forceinline__ u64 mv_block_scan(u64 v, u64* sh, u64* total) {
    const int tid = threadIdx.x, w = tid >> 6;
    const u64 incl = mv_wave_scan(v);
    if ((tid & 63) == 63) sh[w] = incl;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < MV_NT / 64; ++i) { const u64 t = sh[i]; base += i < w ? t : 0; tot += t; }
    __syncthreads();
    if (total) *total = tot;
    return incl + base;
}
// mis-sampler-v1 (oracle/sampler.py::sample) on one small vocabulary (V <= 4096) per row: one 256-thread block, 16 CONSECUTIVE ids per
// thread, everything in registers / LDS.  E, Z, thr, k*, Z_K and r are exact integers, so the token equals the numpy oracle's bit for bit.
__global__ void __launch_bounds__(MV_NT) k_mv_sample(MvSampleArgs a) {
    __shared__ u64 hist[256];
    __shared__ u64 sh[MV_NT / 64];
    __shared__ float redf[MV_NT / 64];
    __shared__ int redi[MV_NT / 64];
    __shared__ unsigned s_bin, s_bin2;
    __shared__ u64 s_below;
    __shared__ int s_token;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!a.active[b]) return;
    const int f = *a.frame;
    const bf16_t* lg = a.logits + (size_t)b * a.Vpad;
    const int i_base = tid * MV_PER;
    float l[MV_PER];
#pragma unroll
    for (int e = 0; e < MV_PER; ++e) l[e] = i_base + e < a.V ? bf16_to_f32(lg[i_base + e]) : -INFINITY;   // padded columns can never be sampled
    if (a.logits_out && f < a.F) {
        float* lo = a.logits_out + (((size_t)b * a.F + f) * a.Cb + a.slot) * a.V;
#pragma unroll
        for (int e = 0; e < MV_PER; ++e) if (i_base + e < a.V) lo[i_base + e] = l[e];
    }
    if (tid == 0) { s_token = 0; s_bin = 255; s_bin2 = 255; s_below = 0; }
    hist[tid] = 0;
    // ---- max (first index on ties)
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < MV_PER; ++e)
        if (i_base + e < a.V && l[e] > best) { best = l[e]; bi = i_base + e; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if ((tid & 63) == 0) { redf[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    best = redf[0]; bi = redi[0];
#pragma unroll
    for (int w = 1; w < MV_NT / 64; ++w)
        if (redf[w] > best || (redf[w] == best && redi[w] < bi)) { best = redf[w]; bi = redi[w]; }
    if (a.temperature == 0.0f) {
        if (tid == 0 && bi != 0x7fffffff) s_token = bi;
    } else {
        const float xmax = __fdiv_rn(best, a.temperature);              // fdiv is monotone: max x = fdiv(max l, T)
        u64 E[MV_PER];
        unsigned key[MV_PER];
#pragma unroll
        for (int e = 0; e < MV_PER; ++e) {
            const float x = __fdiv_rn(l[e], a.temperature);
            const float y = fminf(x - xmax, 0.0f);
            const float ee = i_base + e < a.V ? det_exp_dev(y) : 0.0f;
            E[e] = (u64)(ee * E_SCALE);
            key[e] = __float_as_uint(ee) >> 16;
        }
        unsigned kstar = 0;
        if (a.top_p > 0.0f && a.top_p < 1.0f) {
#pragma unroll
            for (int e = 0; e < MV_PER; ++e) if (E[e]) atomicAdd(&hist[key[e] >> 8], E[e]);
            __syncthreads();
            u64 Z = 0;
            u64 mine = hist[tid];
            u64 incl = mv_block_scan(mine, sh, &Z);
            const u64 thr = (u64)((double)(1.0f - a.top_p) * (double)Z);
            if (incl > thr && incl - mine <= thr) { s_bin = (unsigned)tid; s_below = incl - mine; }      // unique crossing
            __syncthreads();
            const unsigned bin1 = s_bin;
            const u64 below1 = s_below;
            hist[tid] = 0;
            __syncthreads();
#pragma unroll
            for (int e = 0; e < MV_PER; ++e) if (E[e] && (key[e] >> 8) == bin1) atomicAdd(&hist[key[e] & 255], E[e]);
            __syncthreads();
            mine = hist[tid];
            incl = mv_block_scan(mine, sh, nullptr) + below1;
            if (incl > thr && incl - mine <= thr) s_bin2 = (unsigned)tid;
            __syncthreads();
            kstar = (bin1 << 8) | s_bin2;
        }
        u64 Ek[MV_PER], mine = 0;
#pragma unroll
        for (int e = 0; e < MV_PER; ++e) { Ek[e] = key[e] >= kstar ? E[e] : 0; mine += Ek[e]; }
        u64 Zk = 0;
        const u64 incl = mv_block_scan(mine, sh, &Zk);
        const u64 excl = incl - mine;
        const u64 row = (u64)(a.row_offset + b);
        const u64 step = (u64)f * (u64)a.K + (u64)a.slot;
        const u64 sa = a.seed ^ (0xD1B54A32D192ED03ull * (row + 1));
        const u64 rnd = mis_splitmix64(mis_splitmix64(sa) + step);
        const u64 r = __umul64hi(rnd, Zk);
        if (mine > 0 && r >= excl && r < incl) {
            u64 run = excl;
            int pick = -1;
#pragma unroll
            for (int e = 0; e < MV_PER; ++e) {
                run += Ek[e];
                if (pick < 0 && Ek[e] && run > r) pick = i_base + e;
            }
            s_token = pick;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int token = s_token;
        int go_on = token;
        if (a.sampled && f < a.F) a.sampled[((size_t)b * a.F + f) * a.Cb + a.slot] = token;
        if (a.forced && f < a.F) go_on = a.forced[((size_t)b * a.F + f) * a.Cb + a.slot];
        a.cur_codes[(size_t)a.slot * a.Mpad + b] = go_on;
    }
}
static void launch_mv_sample(const MvSampleArgs& a, int batch, hipStream_t s) {
    MIS_REQUIRE(a.V <= MV_NT * MV_PER, MIS_ERR_INVALID_INPUT, "audio vocabulary %d exceeds the in-register sampler (%d)", a.V, MV_NT * MV_PER);
    hipLaunchKernelGGL(k_mv_sample, dim3(batch), dim3(MV_NT), 0, s, a);
}

struct MvEndArgs {
    const int32_t* cur_codes;    // [K][Mpad]
    int Mpad, Cb, K, Va, d;
    const bf16_t* audio_emb;     // [K * Va][d]
    bf16_t* in_emb;              // [Mpad][d] next backbone input
    int32_t* codes;              // [B][max_frames][Cb]
    int32_t* n_frames;           // [B]
    const int32_t* row_max;      // [B]
    int max_frames;
    uint8_t* active_a; uint8_t* active_b;
    int32_t* dec_pos_next;       // [Mpad] the depth decoder starts every frame with a fresh cache
    int32_t* done_count;
};
// end of a frame (MarvisTTSModel.swift:444-460): an all-zero frame ends the row and is not kept; otherwise the Cb codes are stored and
// the next position is the frame with a zero text column, mask on the Cb codes: sum of Cb embedding rows, float32, one rounding
__global__ void __launch_bounds__(256) k_mv_frame_end(MvEndArgs a) {
    __shared__ int cs[32];
    const int b = blockIdx.x;
    if (threadIdx.x == 0) a.dec_pos_next[b] = 0;
    if (!a.active_a[b]) return;
    const int f = a.n_frames[b];
    int c = 0;
    if (threadIdx.x < a.Cb) c = a.cur_codes[(size_t)threadIdx.x * a.Mpad + b];
    const int any = __syncthreads_or(c != 0);
    if (!any) {
        if (threadIdx.x == 0) { a.active_a[b] = 0; a.active_b[b] = 0; atomicAdd(a.done_count, 1); }
        return;
    }
    if (threadIdx.x < a.Cb) {
        a.codes[((size_t)b * a.max_frames + f) * a.Cb + threadIdx.x] = c;
        cs[threadIdx.x] = threadIdx.x * a.Va + min(max(c, 0), a.Va - 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < a.d; k += blockDim.x) {
        float e = 0.0f;
        for (int i = 0; i < a.Cb; ++i) e += bf16_to_f32(a.audio_emb[(size_t)cs[i] * a.d + k]);
        a.in_emb[(size_t)b * a.d + k] = f32_to_bf16(e);
    }
    if (threadIdx.x == 0) {
        a.n_frames[b] = f + 1;
        if (f + 1 >= a.row_max[b]) { a.active_a[b] = 0; a.active_b[b] = 0; atomicAdd(a.done_count, 1); }
    }
}

// ---------------------------------------------------------------------------- model handle
static void upload_bf16(mis_marvis* c, const void* data, mis_dtype dtype, size_t n, bf16_t* dst) {
    const size_t esz = dtype == MIS_F32 ? 4 : 2;
    c->raw.alloc(n * esz);
    HIP_CHECK(hipMemcpyAsync(c->raw.p, data, n * esz, hipMemcpyDefault, c->s));
    launch_convert_to_bf16(c->raw.p, dtype, dst, n, c->s);
    HIP_CHECK(hipStreamSynchronize(c->s));
}

extern "C" void mis_marvis_destroy(mis_marvis* c);
extern "C" mis_status mis_marvis_create(const mis_marvis_config* cfg, int device, mis_marvis** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(cfg->audio_num_codebooks >= 1 && cfg->audio_num_codebooks <= 32, MIS_ERR_INVALID_INPUT, "audio_num_codebooks must be 1..32");
    MIS_REQUIRE(cfg->audio_vocab_size >= 2 && cfg->audio_vocab_size <= MV_NT * MV_PER, MIS_ERR_INVALID_INPUT,
                "audio vocabulary must fit the in-register sampler (<= %d)", MV_NT * MV_PER);
    MIS_REQUIRE(cfg->text_vocab_size >= 1, MIS_ERR_INVALID_INPUT, "bad text vocabulary");
    mis_marvis* c = new mis_marvis();
    c->device = device; c->cfg = *cfg;
    mis_lm_config bc = cfg->backbone, dc = cfg->decoder;
    // both LMs take embeddings and return norm(h): their own embedding table is unused, the backbone's output projection is
    // codebook0_head, the decoder's are the audio_head slices.  CSM's rotation: array ops in the model dtype, llama3 rescale on.
    bc.vocab_size = dc.vocab_size = cfg->audio_vocab_size;
    bc.qk_norm = dc.qk_norm = 0; bc.rope_plain = dc.rope_plain = 0; bc.rope_ops_in_dtype = dc.rope_ops_in_dtype = 1;
    bc.tie_word_embeddings = dc.tie_word_embeddings = 0;
    mis_status st = mis_tts_create(&bc, nullptr, device, &c->bb);
    if (st == MIS_OK) st = mis_tts_create(&dc, nullptr, device, &c->dec);
    if (st != MIS_OK) { mis_marvis_destroy(c); return st; }
    c->cfg.backbone = bc; c->cfg.decoder = dc;
    tts_internal_set_rope_csm(c->bb, true);
    tts_internal_set_rope_csm(c->dec, true);
    c->s = tts_stream(c->bb);
    tts_internal_use_stream(c->dec, c->s);
    c->K = cfg->audio_num_codebooks; c->Va = cfg->audio_vocab_size; c->VaPad = (int)round_up(c->Va, 16); c->Vt = cfg->text_vocab_size;
    c->d = bc.hidden_size; c->dd = dc.hidden_size;
    HIP_CHECK(hipSetDevice(device));
    c->text_emb.alloc((size_t)c->Vt * c->d);
    c->audio_emb.alloc((size_t)c->K * c->Va * c->d);
    c->proj_w.alloc((size_t)c->dd * c->d);
    if (c->K > 1) c->heads.alloc((size_t)(c->K - 1) * c->VaPad * c->dd);
    {   // the LMs' own embedding slots (and the decoder's lm_head) are unused: satisfy their loaders
        std::vector<bf16_t> z((size_t)c->Va * std::max(c->d, c->dd), (bf16_t)0);
        int64_t shb[2] = {c->Va, c->d}, shd[2] = {c->Va, c->dd};
        st = mis_tts_set_tensor(c->bb, "model.embed_tokens.weight", z.data(), MIS_BF16, shb, 2);
        if (st == MIS_OK) st = mis_tts_set_tensor(c->dec, "model.embed_tokens.weight", z.data(), MIS_BF16, shd, 2);
        if (st == MIS_OK) st = mis_tts_set_tensor(c->dec, "lm_head.weight", z.data(), MIS_BF16, shd, 2);
        if (st != MIS_OK) { mis_marvis_destroy(c); return st; }
    }
    *out = c;
    MIS_API_END
}

extern "C" void mis_marvis_destroy(mis_marvis* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->s) (void)hipStreamSynchronize(c->s);
    if (c->dec) mis_tts_destroy(c->dec);            // borrows the backbone's stream (or still owns its own if create failed early)
    if (c->bb) mis_tts_destroy(c->bb);
    delete c;
}

// "model.backbone.layers.3.self_attn.q_proj.weight" -> (lm, "model.layers.3.self_attn.q_proj.weight"); false: not an LM tensor
static bool mv_lm_key(mis_marvis* c, const std::string& name, mis_tts** lm, std::string* inner) {
    for (int w = 0; w < 2; ++w) {
        const std::string pre = w == 0 ? "model.backbone." : "model.decoder.";
        if (name.rfind(pre, 0) == 0) { *lm = w == 0 ? c->bb : c->dec; *inner = "model." + name.substr(pre.size()); return true; }
    }
    return false;
}
// rows of a q_proj / k_proj matrix de-interleaved per head: row h*D + i <- row h*D + 2i, row h*D + D/2 + i <- row h*D + 2i + 1
static bool mv_is_qk(const std::string& inner) {
    return inner.find(".self_attn.q_proj.weight") != std::string::npos || inner.find(".self_attn.k_proj.weight") != std::string::npos;
}
static void mv_permute_rows(const void* src, size_t row_bytes, int64_t N, int D, std::vector<uint8_t>& dst) {
    std::vector<uint8_t> host((size_t)N * row_bytes);
    HIP_CHECK(hipMemcpy(host.data(), src, host.size(), hipMemcpyDefault));
    dst.resize(host.size());
    for (int64_t r = 0; r < N; ++r) {
        const int64_t h = r / D, i = r % D;
        const int64_t from = h * D + (i < D / 2 ? 2 * i : 2 * (i - D / 2) + 1);
        memcpy(dst.data() + (size_t)r * row_bytes, host.data() + (size_t)from * row_bytes, row_bytes);
    }
}
static int mv_head_dim(const mis_lm_config& l) { return l.head_dim > 0 ? l.head_dim : l.hidden_size / l.num_attention_heads; }

extern "C" mis_status mis_marvis_set_tensor(mis_marvis* c, const char* name_, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && name_ && data && shape && ndim >= 1, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(!c->finalized, MIS_ERR_INVALID_INPUT, "set_tensor after finalize");
    MIS_REQUIRE(dtype == MIS_F32 || dtype == MIS_F16 || dtype == MIS_BF16, MIS_ERR_INVALID_INPUT, "unsupported dtype");
    const std::string name = name_;
    HIP_CHECK(hipSetDevice(c->device));
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { MIS_REQUIRE(shape[i] > 0, MIS_ERR_INVALID_INPUT, "bad shape"); n *= (size_t)shape[i]; }
    auto want2 = [&](int64_t a, int64_t b) {
        MIS_REQUIRE(ndim == 2 && shape[0] == a && shape[1] == b, MIS_ERR_INVALID_INPUT, "%s has the wrong shape", name.c_str());
    };
    mis_tts* lm = nullptr;
    std::string inner;
    if (name.find("rotary_emb.inv_freq") != std::string::npos) return MIS_OK;      // CSMLlamaModel.sanitize (:306-310)
    if (mv_lm_key(c, name, &lm, &inner)) {
        MIS_REQUIRE(inner != "model.embed_tokens.weight" && inner != "lm_head.weight", MIS_ERR_INVALID_INPUT, "unexpected tensor %s", name.c_str());
        mis_status st;
        if (ndim == 2 && mv_is_qk(inner)) {
            const int D = mv_head_dim(lm == c->bb ? c->cfg.backbone : c->cfg.decoder);
            MIS_REQUIRE(shape[0] % D == 0, MIS_ERR_INVALID_INPUT, "%s: rows are not whole heads", name.c_str());
            std::vector<uint8_t> perm;
            mv_permute_rows(data, (size_t)shape[1] * (dtype == MIS_F32 ? 4 : 2), shape[0], D, perm);
            st = mis_tts_set_tensor(lm, inner.c_str(), perm.data(), dtype, shape, ndim);
        } else st = mis_tts_set_tensor(lm, inner.c_str(), data, dtype, shape, ndim);
        if (st != MIS_OK) return st;
    } else if (name == "model.text_embeddings.weight") {
        want2(c->Vt, c->d); upload_bf16(c, data, dtype, n, c->text_emb.p);
    } else if (name == "model.audio_embeddings.weight") {
        want2((int64_t)c->K * c->Va, c->d); upload_bf16(c, data, dtype, n, c->audio_emb.p);
    } else if (name == "model.projection.weight") {
        want2(c->dd, c->d);
        c->stage.alloc(n);
        upload_bf16(c, data, dtype, n, c->stage.p);
        launch_pack_weight(c->stage.p, c->proj_w.p, c->dd, c->d, c->dd / 16, 1, 0, c->s);
        HIP_CHECK(hipStreamSynchronize(c->s));
    } else if (name == "model.codebook0_head.weight") {
        want2(c->Va, c->d);
        mis_status st = mis_tts_set_tensor(c->bb, "lm_head.weight", data, dtype, shape, ndim);
        if (st != MIS_OK) return st;
    } else if (name == "model.audio_head") {
        MIS_REQUIRE(c->K > 1 && ndim == 3 && shape[0] == c->K - 1 && shape[1] == c->dd && shape[2] == c->Va, MIS_ERR_INVALID_INPUT,
                    "model.audio_head must be [%d, %d, %d]", c->K - 1, c->dd, c->Va);
        // each slice [Dd][Va] transposed to a Linear's [Va][Dd] and packed once; rows Va .. VaPad - 1 stay zero and the sampler never reads them
        c->stage.alloc(n);
        upload_bf16(c, data, dtype, n, c->stage.p);
        DevBuf<bf16_t> tr;
        tr.alloc((size_t)c->Va * c->dd);
        HIP_CHECK(hipMemsetAsync(c->heads.p, 0, c->heads.bytes(), c->s));
        for (int i = 0; i + 1 < c->K; ++i) {
            hipLaunchKernelGGL(k_mv_transpose, dim3(c->Va), dim3(256), 0, c->s, c->stage.p + (size_t)i * c->dd * c->Va, tr.p, c->dd, c->Va);
            launch_pack_weight(tr.p, c->heads.p + (size_t)i * c->VaPad * c->dd, c->Va, c->dd, c->VaPad / 16, 1, 0, c->s);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->s));
    } else {
        throw MisError(MIS_ERR_INVALID_INPUT, "unexpected tensor " + name);
    }
    c->loaded.insert(name);
    MIS_API_END
}

// A tensor of a quantised checkpoint (mlx quantize: uint32 words + scales + biases; MarvisTTSModel.swift:195-203 quantises every module
// with a `.scales` key, the two Embeddings included).  The Linear layers of the two LMs and codebook0_head keep their quantised form and
// are streamed as codes where lm_qgemm.hip takes the format (mis_tts_set_tensor_quantized); the embeddings (gathered tensors) and
// projection (folded into the decoder's input table, see the header) are dequantised here to bf16 rows.
extern "C" mis_status mis_marvis_set_tensor_quantized(mis_marvis* c, const char* name_, const uint32_t* wq, const void* scales, const void* biases,
                                                      mis_dtype sb_dtype, int64_t N, int64_t K, int group_size, int bits) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && name_ && wq && scales && biases, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(!c->finalized, MIS_ERR_INVALID_INPUT, "set_tensor after finalize");
    quant_check_args(name_, sb_dtype, N, K, group_size, bits);
    const std::string name = name_;
    HIP_CHECK(hipSetDevice(c->device));
    mis_tts* lm = nullptr;
    std::string inner;
    const bool head0 = name == "model.codebook0_head.weight";
    if (head0 || mv_lm_key(c, name, &lm, &inner)) {
        if (head0) { lm = c->bb; inner = "lm_head.weight"; }
        mis_status st;
        if (mv_is_qk(inner)) {
            const int D = mv_head_dim(lm == c->bb ? c->cfg.backbone : c->cfg.decoder);
            MIS_REQUIRE(N % D == 0, MIS_ERR_INVALID_INPUT, "%s: rows are not whole heads", name.c_str());
            const size_t esz = sb_dtype == MIS_F32 ? 4 : 2;
            std::vector<uint8_t> pw, ps, pb;
            mv_permute_rows(wq, (size_t)K * bits / 32 * 4, N, D, pw);
            mv_permute_rows(scales, (size_t)(K / group_size) * esz, N, D, ps);
            mv_permute_rows(biases, (size_t)(K / group_size) * esz, N, D, pb);
            st = mis_tts_set_tensor_quantized(lm, inner.c_str(), (const uint32_t*)pw.data(), ps.data(), pb.data(), sb_dtype, N, K, group_size, bits);
        } else st = mis_tts_set_tensor_quantized(lm, inner.c_str(), wq, scales, biases, sb_dtype, N, K, group_size, bits);
        if (st != MIS_OK) return st;
        c->loaded.insert(name);
        return MIS_OK;
    }
    QuantStaged q;
    DevBuf<bf16_t> rows;
    q.stage(wq, scales, biases, sb_dtype, N, K, group_size, bits, c->s);
    rows.alloc((size_t)N * K);
    q.dequantise(rows.p, c->s);
    HIP_CHECK(hipStreamSynchronize(c->s));
    const int64_t shape[2] = {N, K};
    return mis_marvis_set_tensor(c, name_, rows.p, MIS_BF16, shape, 2);
    MIS_API_END
}

// benches: every tensor synthetic (there are no checkpoints offline).  The LMs' matrices are taken as ALREADY de-interleaved.
static mis_status mv_init_synthetic(mis_marvis* c, uint64_t seed, int bits) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized && (bits == 0 || bits == 4 || bits == 8), MIS_ERR_INVALID_INPUT, "bad argument");
    HIP_CHECK(hipSetDevice(c->device));
    mis_status st = bits ? mis_tts_init_synthetic_quantized(c->bb, seed, bits) : mis_tts_init_synthetic(c->bb, seed);
    if (st == MIS_OK) st = bits ? mis_tts_init_synthetic_quantized(c->dec, seed + 1, bits) : mis_tts_init_synthetic(c->dec, seed + 1);
    if (st != MIS_OK) return st;
    const uint64_t base = seed * 100000ull + 70000ull;
    launch_synth_fill_bf16(c->text_emb.p, (size_t)c->Vt * c->d, base + 1, (float)(0.5 * sqrt(3.0)), 0, c->s);
    launch_synth_fill_bf16(c->audio_emb.p, (size_t)c->K * c->Va * c->d, base + 2, (float)(0.5 * sqrt(3.0) / sqrt((double)c->K)), 0, c->s);
    c->stage.alloc((size_t)std::max((size_t)c->dd * c->d, (size_t)c->Va * c->dd));
    launch_synth_fill_bf16(c->stage.p, (size_t)c->dd * c->d, base + 3, (float)sqrt(3.0 / c->d), 0, c->s);
    launch_pack_weight(c->stage.p, c->proj_w.p, c->dd, c->d, c->dd / 16, 1, 0, c->s);
    HIP_CHECK(hipStreamSynchronize(c->s));
    if (c->K > 1) HIP_CHECK(hipMemsetAsync(c->heads.p, 0, c->heads.bytes(), c->s));
    for (int i = 0; i + 1 < c->K; ++i) {
        launch_synth_fill_bf16(c->stage.p, (size_t)c->Va * c->dd, base + 10 + i, (float)(sqrt(3.0 / c->dd) * 2.0), 0, c->s);
        launch_pack_weight(c->stage.p, c->heads.p + (size_t)i * c->VaPad * c->dd, c->Va, c->dd, c->VaPad / 16, 1, 0, c->s);
        HIP_CHECK(hipStreamSynchronize(c->s));
    }
    HIP_CHECK(hipGetLastError());
    for (const char* n : {"model.text_embeddings.weight", "model.audio_embeddings.weight", "model.projection.weight", "model.codebook0_head.weight",
                          "model.audio_head"})
        c->loaded.insert(n);
    MIS_API_END
}
extern "C" mis_status mis_marvis_init_synthetic(mis_marvis* c, uint64_t seed) { return mv_init_synthetic(c, seed, 0); }
extern "C" mis_status mis_marvis_init_synthetic_quantized(mis_marvis* c, uint64_t seed, int bits) {
    if (bits != 4 && bits != 8) return mis_fail(MIS_ERR_INVALID_INPUT, "bits must be 4 or 8");
    return mv_init_synthetic(c, seed, bits);
}

extern "C" mis_status mis_marvis_finalize(mis_marvis* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<std::string> want = {"model.text_embeddings.weight", "model.audio_embeddings.weight", "model.projection.weight",
                                     "model.codebook0_head.weight"};
    if (c->K > 1) want.push_back("model.audio_head");
    for (auto& w : want) MIS_REQUIRE(c->loaded.count(w), MIS_ERR_NOT_INITIALIZED, "Marvis weight missing: %s", w.c_str());
    mis_status st = mis_tts_finalize(c->bb);
    if (st == MIS_OK) st = mis_tts_finalize(c->dec);
    if (st != MIS_OK) return st;
    {   // audio_embeddings @ projection^T -> [K * Va][Dd], 64 rows a launch: per row the arithmetic of projecting after the gather
        // (same GEMM arrangement as the per-frame projection of lastH, so the bf16 results agree for equal inputs)
        const int rows = c->K * c->Va;
        c->audio_emb_proj.alloc((size_t)round_up(rows, 64) * c->dd);
        c->xpk.alloc((size_t)64 * c->d);
        for (int r0 = 0; r0 < rows; r0 += 64) {
            const int nv = std::min(64, rows - r0);
            hipLaunchKernelGGL(k_mv_gather_pack, dim3(64), dim3(256), 0, c->s, c->audio_emb.p, c->d, r0, nv, c->xpk.p, 4);
            launch_gemm_skinny(EPI_BF16, 2, 4, c->proj_w.p, c->xpk.p, c->audio_emb_proj.p + (size_t)r0 * c->dd, c->dd / 16, c->d / 32, 1, c->dd, 64, c->s);
        }
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(c->s));
    c->raw.release(); c->stage.release();
    c->finalized = true;
    MIS_API_END
}
extern "C" mis_tts* mis_marvis_backbone(mis_marvis* c) { return c ? c->bb : nullptr; }
extern "C" mis_tts* mis_marvis_decoder(mis_marvis* c) { return c ? c->dec : nullptr; }
extern "C" int mis_marvis_launches_per_frame(const mis_marvis* c) { return c ? c->last_launches : 0; }

// ---------------------------------------------------------------------------- frame loop
#define MV_MAX_SEQ 2048
#define MV_MAX_AUDIO_FRAMES 750            // Int(60000 / 80.0), MarvisTTSModel.swift:402

struct MvDebug {                                        // teacher forcing (mis_debug_marvis_forced_logits)
    const int32_t* forced = nullptr;                    // host [batch][F][Cb]
    int F = 0;
    std::vector<float>* logits = nullptr;               // [batch][F][Cb][Va]
    std::vector<int32_t>* sampled = nullptr;            // [batch][F][Cb]
};

static void mv_check_params(const mis_marvis* c, const mis_marvis_params* gp, int* Cb_out, int* max_frames_out) {
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "Marvis model not finalized");
    const int Cb = gp->codebooks == 0 ? c->K : gp->codebooks;
    MIS_REQUIRE(Cb >= 1 && Cb <= c->K, MIS_ERR_INVALID_INPUT, "codebooks %d outside 1..%d", Cb, c->K);
    const int mf = gp->max_frames == 0 ? MV_MAX_AUDIO_FRAMES : gp->max_frames;
    MIS_REQUIRE(mf >= 1 && mf <= MV_MAX_AUDIO_FRAMES, MIS_ERR_INVALID_INPUT, "max_frames %d outside 1..%d", mf, MV_MAX_AUDIO_FRAMES);
    MIS_REQUIRE(gp->temperature >= 0.0f, MIS_ERR_INVALID_INPUT, "negative temperature");
    *Cb_out = Cb; *max_frames_out = mf;
}

static void mv_generate_codes(mis_marvis* c, const int32_t* tokens, const uint8_t* mask, const int32_t* prompt_lens, int P, int batch,
                              const mis_marvis_params* gp, const int32_t* row_max_frames, std::vector<int32_t>& codes_host,
                              std::vector<int32_t>& n_frames_host, int* stride_out, const volatile int* cancel, FrameStreamHook* hook = nullptr,
                              MvDebug* dbg = nullptr) {
    int Cb = 0, max_frames = 0;
    mv_check_params(c, gp, &Cb, &max_frames);
    MIS_REQUIRE(batch >= 1 && batch <= 64 && P >= 1, MIS_ERR_INVALID_INPUT, "bad batch / prompt sizes");
    const int K = c->K, Va = c->Va, d = c->d, dd = c->dd, W = K + 1;
    // ---- everything is checked before anything is launched
    int Lmax = 0;
    for (int b = 0; b < batch; ++b) {
        const int n = prompt_lens[b];
        MIS_REQUIRE(n >= 1 && n <= P, MIS_ERR_INVALID_INPUT, "row %d: bad prompt length", b);
        MIS_REQUIRE(n < MV_MAX_SEQ - MV_MAX_AUDIO_FRAMES, MIS_ERR_INVALID_INPUT,
                    "row %d: inputs too long, must be below max_seq_len - max_audio_frames: %d", b, MV_MAX_SEQ - MV_MAX_AUDIO_FRAMES);
        Lmax = std::max(Lmax, n);
        for (int p = 0; p < n; ++p) {
            const int32_t* t = tokens + ((size_t)b * P + p) * W;
            const uint8_t* m = mask + ((size_t)b * P + p) * W;
            for (int i = 0; i < K; ++i) MIS_REQUIRE(!m[i] || (t[i] >= 0 && t[i] < Va), MIS_ERR_INVALID_INPUT, "row %d position %d: audio code outside its table", b, p);
            MIS_REQUIRE(!m[K] || (t[K] >= 0 && t[K] < c->Vt), MIS_ERR_INVALID_INPUT, "row %d position %d: text id outside its table", b, p);
        }
    }
    if (dbg) {
        MIS_REQUIRE(dbg->forced && dbg->F >= 1 && dbg->F <= max_frames, MIS_ERR_INVALID_INPUT, "bad forced frames");
        for (size_t i = 0; i < (size_t)batch * dbg->F * Cb; ++i)
            MIS_REQUIRE(dbg->forced[i] >= 0 && dbg->forced[i] < Va, MIS_ERR_INVALID_INPUT, "forced code outside its table");
    }
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->s;
    tts_internal_reset(c->bb, batch, Lmax + max_frames + 1);
    tts_internal_reset(c->dec, batch, 64);
    TtsView tv = tts_internal_view(c->bb), pv = tts_internal_view(c->dec);
    const int Mpad = tv.Mpad;
    c->in_emb.alloc((size_t)Mpad * d); c->hid_proj.alloc((size_t)Mpad * dd);
    c->iota.alloc(Mpad); c->ptok.alloc((size_t)batch * P * W); c->pmask.alloc((size_t)batch * P * W + W); c->plen.alloc(batch);
    c->cur_codes.alloc((size_t)K * Mpad); c->codes.alloc((size_t)batch * max_frames * Cb); c->n_frames.alloc(Mpad); c->frame.alloc(1);
    c->done.alloc(1); c->row_max.alloc(batch);
    c->in_emb.zero(s); c->cur_codes.zero(s); c->codes.zero(s); c->n_frames.zero(s); c->frame.zero(s); c->done.zero(s); c->pmask.zero(s);
    hipLaunchKernelGGL(k_mv_iota, dim3(1), dim3(64), 0, s, c->iota.p, Mpad);
    std::vector<int32_t> rmax(batch);
    for (int b = 0; b < batch; ++b) rmax[b] = row_max_frames ? std::max(1, std::min(row_max_frames[b], max_frames)) : max_frames;
    HIP_CHECK(hipMemcpyAsync(c->ptok.p, tokens, (size_t)batch * P * W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->pmask.p, mask, (size_t)batch * P * W, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->plen.p, prompt_lens, batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->row_max.p, rmax.data(), batch * 4, hipMemcpyHostToDevice, s));
    if (dbg) {
        const size_t nf = (size_t)batch * dbg->F * Cb;
        c->forced.alloc(nf); c->sampled.alloc(nf); c->logits_dbg.alloc(nf * Va);
        HIP_CHECK(hipMemcpyAsync(c->forced.p, dbg->forced, nf * 4, hipMemcpyHostToDevice, s));
        c->sampled.zero(s); c->logits_dbg.zero(s);
    }
    const bool use_graph = getenv("MIS_NO_GRAPH") == nullptr;
    {
        StepGraph g_frame;
        // ---- prefill: the right-aligned prompt matrix, all positions at once where lm_prefill.hip applies, else one position a launch chain
        if (tts_internal_prefill_rows_ok(c->bb, Lmax)) {
            c->pf_rows.alloc((size_t)Lmax * Mpad * d);
            hipLaunchKernelGGL(k_mv_prompt_rows, dim3(Mpad, Lmax), dim3(256), 0, s, c->ptok.p, c->pmask.p, c->plen.p, P, Lmax, K, Va, c->audio_emb.p,
                               c->text_emb.p, c->pf_rows.p, d, batch, Mpad);
            tts_internal_prefill_rows(c->bb, c->pf_rows.p, prompt_lens, Lmax);
        } else {
            for (int j = 0; j < Lmax; ++j) {
                hipLaunchKernelGGL(k_mv_prompt_feed, dim3(Mpad), dim3(256), 0, s, c->ptok.p, c->pmask.p, c->plen.p, P, Lmax, j, K, Va, c->audio_emb.p,
                                   c->text_emb.p, c->in_emb.p, tv.active, d, batch);
                tts_internal_enqueue_layers(c->bb, c->in_emb.p, Mpad, c->iota.p);
            }
        }
        {
            std::vector<uint8_t> ones(Mpad, 0);
            for (int b = 0; b < batch; ++b) ones[b] = 1;
            HIP_CHECK(hipMemcpyAsync(tv.active, ones.data(), Mpad, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(pv.active, ones.data(), Mpad, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s));                       // `ones` leaves scope
        }
        // ---- one frame
        MvSampleArgs sa{};
        sa.temperature = gp->temperature; sa.top_p = gp->top_p; sa.seed = gp->seed; sa.row_offset = gp->row_offset; sa.frame = c->frame.p;
        sa.K = K; sa.Cb = Cb; sa.cur_codes = c->cur_codes.p; sa.Mpad = Mpad; sa.active = tv.active; sa.V = Va;
        if (dbg) { sa.forced = c->forced.p; sa.F = dbg->F; sa.sampled = c->sampled.p; sa.logits_out = c->logits_dbg.p; }
        const int chain_b = 7 * tv.L + 1, chain_d = 7 * pv.L + 1;
        c->last_launches = 1 + 1 + 1 + (Cb > 1 ? Cb * chain_d + (Cb - 1) * 2 : 0) + 1 + 1 + chain_b;
        auto frame_body = [&]() {
            // codebook 0 from the backbone's last position (the previous frame's / the prefill's final norm is in the packed x)
            tts_internal_enqueue_head(c->bb, nullptr);
            MvSampleArgs t = sa;
            t.logits = tv.logits; t.Vpad = tv.Vpad; t.slot = 0;
            launch_mv_sample(t, batch, s);
            if (Cb > 1) {
                // depth decoder, fresh cache: positions 0, 1 = projection(lastH), projection(emb_0(c0)); then one embedding per codebook
                launch_gemm_skinny(EPI_BF16, 2, 4, c->proj_w.p, tv.x, c->hid_proj.p, dd / 16, d / 32, 1, dd, Mpad, s);
                tts_internal_enqueue_layers(c->dec, c->hid_proj.p, Mpad, c->iota.p);
                for (int i = 1; i < Cb; ++i) {
                    tts_internal_enqueue_layers(c->dec, c->audio_emb_proj.p + (size_t)(i - 1) * Va * dd, Va, c->cur_codes.p + (size_t)(i - 1) * Mpad);
                    tts_internal_enqueue_head(c->dec, c->heads.p + (size_t)(i - 1) * c->VaPad * dd);
                    MvSampleArgs p = sa;
                    p.logits = pv.logits; p.Vpad = pv.Vpad; p.slot = i;
                    launch_mv_sample(p, batch, s);
                }
            }
            MvEndArgs ea{};
            ea.cur_codes = c->cur_codes.p; ea.Mpad = Mpad; ea.Cb = Cb; ea.K = K; ea.Va = Va; ea.d = d; ea.audio_emb = c->audio_emb.p;
            ea.in_emb = c->in_emb.p; ea.codes = c->codes.p; ea.n_frames = c->n_frames.p; ea.row_max = c->row_max.p; ea.max_frames = max_frames;
            ea.active_a = tv.active; ea.active_b = pv.active; ea.dec_pos_next = pv.pos_next; ea.done_count = c->done.p;
            hipLaunchKernelGGL(k_mv_frame_end, dim3(Mpad), dim3(256), 0, s, ea);
            hipLaunchKernelGGL(k_mv_bump, dim3(1), dim3(64), 0, s, c->frame.p);
            tts_internal_enqueue_layers(c->bb, c->in_emb.p, Mpad, c->iota.p);       // the next frame's backbone position
        };
        if (use_graph) {
            g_frame.capture(s, frame_body);
            c->last_launches = g_frame.nodes();                        // what the graph really holds (the formula above is the expectation)
        }
        PinnedBuf<int32_t> done_pin(1);
        *done_pin.p = 0;
        run_frame_loop(dbg ? dbg->F : max_frames, batch, cancel, hook,
                       [&]() { if (use_graph) g_frame.launch(s); else frame_body(); },
                       [&]() { HIP_CHECK(hipMemcpyAsync(done_pin.p, c->done.p, 4, hipMemcpyDeviceToHost, s)); },
                       [&]() { HIP_CHECK(hipStreamSynchronize(s)); return (int)*done_pin.p; },
                       [&]() { HIP_CHECK(hipGetLastError()); },
                       [&]() {
                           n_frames_host.resize(batch);
                           HIP_CHECK(hipMemcpyAsync(n_frames_host.data(), c->n_frames.p, batch * 4, hipMemcpyDeviceToHost, s));
                           HIP_CHECK(hipStreamSynchronize(s));
                           return *std::max_element(n_frames_host.begin(), n_frames_host.end());
                       });
    }
    codes_host.resize((size_t)batch * max_frames * Cb);
    n_frames_host.resize(batch);
    HIP_CHECK(hipMemcpyAsync(codes_host.data(), c->codes.p, codes_host.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(n_frames_host.data(), c->n_frames.p, batch * 4, hipMemcpyDeviceToHost, s));
    if (dbg) {
        const size_t nf = (size_t)batch * dbg->F * Cb;
        dbg->logits->resize(nf * Va); dbg->sampled->resize(nf);
        HIP_CHECK(hipMemcpyAsync(dbg->logits->data(), c->logits_dbg.p, nf * Va * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(dbg->sampled->data(), c->sampled.p, nf * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    *stride_out = max_frames;
}

extern "C" mis_status mis_marvis_generate_codes(mis_marvis* c, const int32_t* tokens, const uint8_t* mask, const int32_t* prompt_lens, int P,
                                                int batch, const mis_marvis_params* params, const int32_t* row_max_frames,
                                                int32_t** codes_out, int64_t* codes_stride, int32_t* n_frames) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && tokens && mask && prompt_lens && params && codes_out && codes_stride && n_frames, MIS_ERR_INVALID_INPUT, "null argument");
    std::vector<int32_t> codes, nf;
    int stride = 0;
    mv_generate_codes(c, tokens, mask, prompt_lens, P, batch, params, row_max_frames, codes, nf, &stride, nullptr);
    PinnedBuf<int32_t> host(codes.size() + 1);
    memcpy(host.p, codes.data(), codes.size() * 4);
    *codes_out = host.release(); *codes_stride = stride;
    for (int b = 0; b < batch; ++b) n_frames[b] = nf[b];
    MIS_API_END
}

// the frame loop teacher-forced: samples as usual, continues from forced[b][f][i]; logits_out f32 [batch][F][Cb][audio_vocab] (rows past a
// row's end stay 0), sampled_out int32 [batch][F][Cb] (may be NULL), n_frames[batch] under the end rule applied to the forced codes
extern "C" mis_status mis_debug_marvis_forced_logits(mis_marvis* c, const int32_t* tokens, const uint8_t* mask, const int32_t* prompt_lens, int P,
                                                     int batch, const mis_marvis_params* params, const int32_t* forced, int F, float* logits_out,
                                                     int32_t* sampled_out, int32_t* n_frames) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && tokens && mask && prompt_lens && params && forced && logits_out && n_frames, MIS_ERR_INVALID_INPUT, "null argument");
    std::vector<int32_t> codes, nf, sampled;
    std::vector<float> logits;
    MvDebug dbg;
    dbg.forced = forced; dbg.F = F; dbg.logits = &logits; dbg.sampled = &sampled;
    int stride = 0;
    mv_generate_codes(c, tokens, mask, prompt_lens, P, batch, params, nullptr, codes, nf, &stride, nullptr, nullptr, &dbg);
    memcpy(logits_out, logits.data(), logits.size() * 4);
    if (sampled_out) memcpy(sampled_out, sampled.data(), sampled.size() * 4);
    for (int b = 0; b < batch; ++b) n_frames[b] = nf[b];
    MIS_API_END
}

// stand-alone sampler for parity tests: logits f32 [batch, vocab] (bf16-rounded on upload) -> tokens[batch], RNG step = frame * K + slot
extern "C" mis_status mis_debug_marvis_sample_logits(int device, const float* logits, int batch, int vocab, float temperature, float top_p,
                                                     uint64_t seed, int64_t row_offset, int frame, int slot, int K, int32_t* tokens_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(logits && tokens_out && batch >= 1 && vocab >= 1 && vocab <= MV_NT * MV_PER && K >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    HIP_CHECK(hipSetDevice(device));
    const int Vpad = (int)round_up(vocab, 16), Mpad = (int)round_up(batch, 16);
    std::vector<bf16_t> lb((size_t)Mpad * Vpad, f32_to_bf16(1e30f));        // padding columns hold a LARGE value: they must never be read
    for (int b = 0; b < batch; ++b) for (int i = 0; i < vocab; ++i) lb[(size_t)b * Vpad + i] = f32_to_bf16(logits[(size_t)b * vocab + i]);
    DevBuf<bf16_t> dl; DevBuf<uint8_t> act; DevBuf<int32_t> cur, fr;
    dl.alloc(lb.size()); act.alloc(Mpad); cur.alloc((size_t)K * Mpad); fr.alloc(1);
    HIP_CHECK(hipMemcpy(dl.p, lb.data(), lb.size() * 2, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(act.p, 1, Mpad));
    HIP_CHECK(hipMemset(cur.p, 0, (size_t)K * Mpad * 4));
    HIP_CHECK(hipMemcpy(fr.p, &frame, 4, hipMemcpyHostToDevice));
    MvSampleArgs a{};
    a.logits = dl.p; a.Vpad = Vpad; a.V = vocab; a.temperature = temperature; a.top_p = top_p; a.seed = seed; a.row_offset = row_offset;
    a.frame = fr.p; a.slot = slot; a.K = K; a.Cb = K; a.cur_codes = cur.p; a.Mpad = Mpad; a.active = act.p;
    MIS_REQUIRE(slot >= 0 && slot < K, MIS_ERR_INVALID_INPUT, "slot outside 0..K-1");
    launch_mv_sample(a, batch, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(tokens_out, cur.p + (size_t)slot * Mpad, batch * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// ---------------------------------------------------------------------------- generate (frames + audio through a borrowed Mimi)
// The audio of a row is ALWAYS the streaming decode of its frames (MimiStreamingDecoder.decodeFrames, MarvisTTSModel.swift:501-510; the
// reference never uses the batched decode here), so both forms return identical samples:
//  * on_event == NULL or chunk_frames <= 0: all frames, then one stream session over every row's frames (one MIS_EVENT_AUDIO per row if on_event);
//  * on_event != NULL and chunk_frames > 0: whenever another chunk_frames frames exist, Mimi's stream step of the whole batch runs on
//    Mimi's stream WHILE the frame loop continues on the LM stream; each row's new samples are delivered as MIS_EVENT_AUDIO as soon as
//    they are on the host, MIS_EVENT_TOKEN (the frame's Cb codes) per frame at every poll, one MIS_EVENT_INFO per row when the loop ends,
//    then the frames after the last full chunk.  cancel_flag is honoured at the poll.
extern "C" mis_status mis_marvis_generate(mis_marvis* c, mis_mimi* mimi, const int32_t* tokens, const uint8_t* mask, const int32_t* prompt_lens,
                                          int P, int batch, const mis_marvis_params* params, const int32_t* row_max_frames, float** pcm_out,
                                          int64_t* pcm_stride, int64_t* pcm_lens, int32_t** codes_out, int64_t* codes_stride, int32_t* n_frames,
                                          int chunk_frames, mis_event_cb on_event, void* user, const volatile int* cancel_flag) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && mimi && tokens && mask && prompt_lens && params && pcm_out && pcm_stride && pcm_lens, MIS_ERR_INVALID_INPUT, "null argument");
    int Cb = 0, max_frames = 0;
    mv_check_params(c, params, &Cb, &max_frames);
    MIS_REQUIRE(mimi_internal_device(mimi) == c->device, MIS_ERR_INVALID_INPUT, "the Mimi handle lives on another device");
    MIS_REQUIRE(Cb >= 2 && Cb <= mimi_internal_num_quantizers(mimi), MIS_ERR_INVALID_INPUT, "codebooks %d outside what Mimi's stream step takes [2, %d]", Cb,
                mimi_internal_num_quantizers(mimi));
    MIS_REQUIRE(!mimi_internal_stream_open(mimi), MIS_ERR_INVALID_INPUT,
                "generate needs the Mimi handle's decode-stream session, but the host has one open (mis_mimi_decode_stream_end first)");
    const int64_t up = mis_mimi_num_samples(mimi, 1);
    const bool streaming = on_event && chunk_frames > 0;
    hipStream_t s_mimi = mimi_internal_stream(mimi);
    std::vector<int32_t> codes, nf;
    int stride = 0;

    struct Session {                                     // Mimi's decode-stream session while THIS call holds it
        mis_mimi* m = nullptr;
        ~Session() { if (m) (void)mis_mimi_decode_stream_end(m); }
    } session;
    std::unique_ptr<ChunkedAudio> pipe;
    DevBuf<float> wav_dev;
    FrameStreamHook hook;
    const auto t_start = std::chrono::steady_clock::now();
    try {
        HIP_CHECK(hipSetDevice(c->device));
        if (streaming) {
            MIS_REQUIRE(mis_mimi_decode_stream_begin(mimi, batch) == MIS_OK, MIS_ERR_GENERATION_FAILED, "Mimi stream: %s", mis_last_error());
            session.m = mimi;
            pipe = std::make_unique<ChunkedAudio>(batch, Cb, max_frames, chunk_frames, up, c->s, s_mimi, &c->codes, &c->n_frames, on_event, user, Cb);
            pipe->t_start = t_start; pipe->prompt_lens = prompt_lens;
            // the loop's code store is [B][max_frames][Cb]: no transposition, the quantizer kernel takes the strides
            pipe->decode = [&](int f0, int fn, float* wav, int64_t row_stride) {
                mimi_internal_stream_step_device(mimi, c->codes.p + (size_t)f0 * Cb, (int64_t)max_frames * Cb, 1, Cb, Cb, fn, wav, row_stride);
            };
            hook = pipe->hook(chunk_frames);
        }
        mv_generate_codes(c, tokens, mask, prompt_lens, P, batch, params, row_max_frames, codes, nf, &stride, cancel_flag, streaming ? &hook : nullptr);
        if (streaming) pipe->emit_ready(true);
    } catch (...) {
        (void)hipStreamSynchronize(s_mimi);
        throw;
    }
    int64_t longest = 0;
    int longest_f = 0;
    for (int b = 0; b < batch; ++b) { pcm_lens[b] = (int64_t)nf[b] * up; longest = std::max(longest, pcm_lens[b]); longest_f = std::max(longest_f, nf[b]); }
    PinnedBuf<float> host_pin((size_t)std::max<int64_t>(longest, 1) * batch);
    float* host = host_pin.p;
    memset(host, 0, (size_t)std::max<int64_t>(longest, 1) * batch * 4);
    try {
        if (streaming) {
            pipe->gather(host, longest, nf);
        } else if (longest_f > 0) {
            // one session over the frames of every row (rows right-padded with zero codes: every layer is causal, a row's samples do not
            // depend on what follows them), in sub-steps that bound the staging buffer
            MIS_REQUIRE(mis_mimi_decode_stream_begin(mimi, batch) == MIS_OK, MIS_ERR_GENERATION_FAILED, "Mimi stream: %s", mis_last_error());
            session.m = mimi;
            const int sub = 64;
            wav_dev.alloc((size_t)batch * std::min(sub, longest_f) * up);
            HIP_CHECK(hipStreamSynchronize(c->s));
            for (int f0 = 0; f0 < longest_f; f0 += sub) {
                const int fn = std::min(sub, longest_f - f0);
                mimi_internal_stream_step_device(mimi, c->codes.p + (size_t)f0 * Cb, (int64_t)max_frames * Cb, 1, Cb, Cb, fn, wav_dev.p, (int64_t)fn * up);
                for (int b = 0; b < batch; ++b) {
                    const int valid = std::min(std::max(nf[b] - f0, 0), fn);
                    if (valid > 0)
                        HIP_CHECK(hipMemcpyAsync(host + (size_t)b * longest + (size_t)f0 * up, wav_dev.p + (size_t)b * fn * up, (size_t)valid * up * 4,
                                                 hipMemcpyDeviceToHost, s_mimi));
                }
                HIP_CHECK(hipStreamSynchronize(s_mimi));
                if (cancel_flag && *cancel_flag) throw MisError(MIS_ERR_CANCELLED, "generation cancelled");
            }
            if (on_event)
                for (int b = 0; b < batch; ++b)
                    if (nf[b] > 0) on_event(user, b, MIS_EVENT_AUDIO, host + (size_t)b * longest, pcm_lens[b]);
        }
    } catch (...) {
        (void)hipStreamSynchronize(s_mimi);
        throw;
    }
    if (codes_out) {
        PinnedBuf<int32_t> ch(codes.size() + 1);
        memcpy(ch.p, codes.data(), codes.size() * 4);
        *codes_out = ch.release();
        if (codes_stride) *codes_stride = stride;
    }
    *pcm_out = host_pin.release(); *pcm_stride = longest;
    if (n_frames) for (int b = 0; b < batch; ++b) n_frames[b] = nf[b];
    MIS_API_END
}
