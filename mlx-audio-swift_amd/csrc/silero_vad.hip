// silero_vad.hip - Silero voice activity detection: waveform -> one speech probability per chunk (32 ms), the LSTM state carried.
//
// Reference being replaced: SileroVAD (Sources/MLXAudioVAD/Models/SileroVAD/SileroVAD.swift): reflectPadRight (:50-57), SileroVADBranch
// (:59-132: stft_conv + magnitude, conv1..conv4 + ReLU, LSTM, final_conv + sigmoid + mean), predictProba's windowing (:192-241) and
// callAsFunction (:153-160).  Two branches (16 kHz / 8 kHz) with their own weights; the thresholding of the probabilities
// (probsToTimestamps, SpeechSegmenter.swift) stays on the host (vad.py): it reads one float a chunk.
//
// One call serves 1..max_batch ragged rows.  Row b has nc_b = ceil(n_b / chunk) chunks; chunk j's window is samples
// [j chunk - context, (j + 1) chunk) of the row, zeros before sample 0 and behind sample n_b, then `pad` reflected samples on the right
// (padded[n + i] = w[n - 2 - i]).  A window gives F STFT frames, F -> F -> F2 -> F3 -> F3 frames through the four convs and S = F3 LSTM
// steps (4 -> 4 -> 2 -> 1 -> 1 at the published branches).  Everything before the recurrence is independent per chunk, so the M dimension
// of every contraction is all (row, chunk, frame) triples of a pass; only the 128-wide recurrence is serial.
//
// A pass covers chunks [c0, c0 + P) of every row, P <= max_chunks (the workspace, sized at finalize); a row with more chunks is walked in
// several passes with (h, c) carried on the device.  A pass is 7 launches:
//
//   k_sv_gemm<MAG>   the STFT as a contraction, K = filter.  Operand load: the window gather (zero pre-context, zero tail, reflect pad)
//                    from the pass's samples.  A wave holds two 32-column accumulators: re bins b0..b0+31 and the SAME im bins, so re
//                    and im of a bin meet in one lane and the epilogue writes sqrt(re re + im im) [.., cutoff].
//   k_sv_gemm<ACT>   conv1..conv4 (K = 3 Cin, k = tap Cin + ci as MLX stores [out, k, in]; the tap shift, the stride and the zero padding
//                    INSIDE the chunk are the operand load: a tap never reads another chunk's frames) + bias + ReLU, and the LSTM's
//                    input projection Wx x + bias (one tap), each its own launch.
//   k_sv_lstm        the recurrence: one block of 512 threads per row, ONE launch for all chunks of the pass.  Thread t keeps row t of Wh
//                    (128 floats, contiguous in memory) in registers for every step; h lives in LDS and is read as broadcasts, c in the
//                    registers of threads 0..127.  A step: gate t = (Wx x + b)[t] + sum_k Wh[t][k] h[k], k ascending; barrier; threads
//                    0..127 apply the nonlinearities (i, f, g, o) and write h; barrier; wave 0 adds sigmoid(final_conv(relu(h))) to the
//                    chunk's mean.  The block waits on nothing but its own barriers, and every barrier sits in block-uniform control
//                    flow: the loop bound is the row's host-validated chunk count.
//
// exact f32 on v_mfma_f32_32x32x2_f32 (f32_tile.h), every edge guarded (K = 387, N = 258 are multiples of nothing).  Every output element
// is one fixed-order sum that depends on its own window alone, so a row's probabilities and state are the same bit for bit whatever the
// batch, the junk behind lens[b], the split into passes, or the path (predict, or chunk by chunk through forward).  No allocation and one
// synchronisation per call.
#include "common.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define SV_MAX_BATCH 64
#define SV_H 128                  // LSTM hidden size = conv4's width (hard-coded in the reference)
#define SV_G 512                  // the four gates
#define SV_TIMED_PASSES 64

enum { SV_EPI_RELU = 0, SV_EPI_PLAIN = 1 };

// a pass: chunks [c0, c0 + P) of every row; nc[b] chunks and lens[b] samples a row
struct SvGeom { const int32_t* nc; const int32_t* lens; int c0, P, B; };

__device__ __forceinline__ int sv_count(const SvGeom& g, int b) {
    const int c = g.nc[b] - g.c0;
    return c < 0 ? 0 : (c > g.P ? g.P : c);
}

struct SvGemm {
    // MAG: the pass's samples [B][pcm_ld], element 0 is sample s_lo of the row
    const float* pcm; int64_t pcm_ld; int s_lo, n, chunk, ctx_off, hop;
    // ACT: [B][P][Fin][Cin], K / Cin taps at stride `stride`, `padl` zeros on the left
    const float* X; int Fin, Cin, stride, padl;
    const float* W; const float* bias;                      // [N rows][K] as the checkpoint stores them; bias may be null
    float* Y; int Fo, K, N, epi;                            // [B][P][Fo][N] (MAG: N = cutoff, W has 2 cutoff rows)
    SvGeom g;
};

// sample p of the padded window of chunk c0 + j of row b
__device__ __forceinline__ float sv_window_sample(const SvGemm& p, int b, int j, int q) {
    if (q >= p.n) q = p.n - 2 - (q - p.n);                   // reflectPadRight: n - 2, n - 3, ...
    const int s = (p.g.c0 + j) * p.chunk - p.ctx_off + q;
    return (s >= 0 && s < p.g.lens[b]) ? p.pcm[(size_t)b * p.pcm_ld + (s - p.s_lo)] : 0.0f;
}

// 2 x 2 waves, 64 rows x 64 columns.  MAG: a wave's two accumulators are re / im of the same 32 bins, the block covers 64 bins.
template <bool MAG>
__global__ void __launch_bounds__(256) k_sv_gemm(SvGemm p) {
    constexpr int CT = MAG ? 2 : 1, TT = 64, TC = 64 * CT;
    __shared__ float As[TT][F32_KC + 1];
    __shared__ float Bs[TC][F32_KC + 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kh = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.x * TT, c0 = blockIdx.y * 64, per_row = p.g.P * p.Fo, M = p.g.B * per_row;
    const int wt = (wave & 1) * 32, wcg = wave >> 1;
    f32x16_t acc[CT] = {};
    for (int k0 = 0; k0 < p.K; k0 += F32_KC) {
#pragma unroll
        for (int n = 0; n < TT * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, k = k0 + (i & 31), m = m0 + r;
            float v = 0.0f;
            if (m < M && k < p.K) {
                const int b = m / per_row, rem = m - b * per_row, j = rem / p.Fo, f = rem - j * p.Fo;
                if (j < sv_count(p.g, b)) {
                    if constexpr (MAG) v = sv_window_sample(p, b, j, f * p.hop + k);
                    else {
                        const int t = k / p.Cin, ci = k - t * p.Cin, fi = f * p.stride + t - p.padl;
                        if (fi >= 0 && fi < p.Fin) v = p.X[(((size_t)b * p.g.P + j) * p.Fin + fi) * p.Cin + ci];
                    }
                }
            }
            As[r][i & 31] = v;
        }
#pragma unroll
        for (int n = 0; n < TC * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, k = k0 + (i & 31);
            int col, wrow;                                   // MAG: Bs row = (wave column, re / im, bin): re at W row bin, im at cutoff + bin
            if constexpr (MAG) { col = c0 + (r >> 6) * 32 + (r & 31); wrow = ((r >> 5) & 1) ? p.N + col : col; }
            else { col = c0 + r; wrow = col; }
            Bs[r][i & 31] = (col < p.N && k < p.K) ? p.W[(size_t)wrow * p.K + k] : 0.0f;
        }
        __syncthreads();
        f32_tile_mfma(As, Bs, wt + l31, wcg * 32 * CT + l31, kh, acc);
        __syncthreads();
    }
    // C/D: column = lane & 31, row = f32_tile_row(r, lane >> 5)
    const int co = c0 + wcg * 32 + l31;
    if (co >= p.N) return;
    const float add = (!MAG && p.bias) ? p.bias[co] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wt + f32_tile_row(r, kh);
        if (m >= M) continue;
        const int b = m / per_row, j = (m - b * per_row) / p.Fo;
        float v;
        if constexpr (MAG) {
            const float re = acc[0][r], im = acc[CT - 1][r];
            v = __fsqrt_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)));
        } else {
            v = acc[0][r] + add;
            if (p.epi == SV_EPI_RELU) v = fmaxf(v, 0.0f);
        }
        p.Y[(size_t)m * p.N + co] = j < sv_count(p.g, b) ? v : 0.0f;
    }
}

struct SvLstm {
    const float* gates;                                     // [B][P][S][512]: Wx x + bias
    const float* Wh;                                        // [512][128]: thread t's slice is row t
    const float* wf; float bf;                              // final_conv [128], its bias
    float* state;                                           // [2][B][128]: h, c; read at the start, written at the end
    float* probs;                                           // [B][P]
    SvGeom g; int S; float inv_S;
};

__device__ __forceinline__ float sv_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ void __launch_bounds__(SV_G) k_sv_lstm(SvLstm p) {
    __shared__ __attribute__((aligned(16))) float hs[SV_H];
    __shared__ float gs[SV_G];
    const int b = blockIdx.x, t = threadIdx.x, cnt = sv_count(p.g, b);
    float w[SV_H];
    {
        const float4* src = reinterpret_cast<const float4*>(p.Wh + (size_t)t * SV_H);
#pragma unroll
        for (int q = 0; q < SV_H / 4; ++q) { const float4 v = src[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    }
    float c = 0.0f, wf0 = 0.0f, wf1 = 0.0f;
    float* hst = p.state + (size_t)b * SV_H;
    float* cst = p.state + ((size_t)p.g.B + b) * SV_H;
    if (t < SV_H) { hs[t] = hst[t]; c = cst[t]; }
    if (t < 64) { wf0 = p.wf[t]; wf1 = p.wf[t + 64]; }
    __syncthreads();
    const float* gin = p.gates + (size_t)b * p.g.P * p.S * SV_G + t;
    for (int j = 0; j < cnt; ++j) {
        float mean = 0.0f;
        for (int s = 0; s < p.S; ++s) {
            float a = 0.0f;
            const float4* h4 = reinterpret_cast<const float4*>(hs);
#pragma unroll
            for (int q = 0; q < SV_H / 4; ++q) {
                const float4 h = h4[q];
                a = fmaf(w[4 * q], h.x, a); a = fmaf(w[4 * q + 1], h.y, a); a = fmaf(w[4 * q + 2], h.z, a); a = fmaf(w[4 * q + 3], h.w, a);
            }
            gs[t] = gin[(size_t)(j * p.S + s) * SV_G] + a;
            __syncthreads();
            if (t < SV_H) {
                const float gi = sv_sigmoid(gs[t]), gf = sv_sigmoid(gs[SV_H + t]), gg = tanhf(gs[2 * SV_H + t]), go = sv_sigmoid(gs[3 * SV_H + t]);
                c = __fadd_rn(__fmul_rn(gf, c), __fmul_rn(gi, gg));
                hs[t] = __fmul_rn(go, tanhf(c));
            }
            __syncthreads();
            if (t < 64) {                                             // wave 0: hs stays as it is until the next step's first barrier
                const float z = wave_sum(fmaf(wf1, fmaxf(hs[t + 64], 0.0f), __fmul_rn(wf0, fmaxf(hs[t], 0.0f))));
                mean += sv_sigmoid(z + p.bf);
            }
        }
        if (t == 0) p.probs[(size_t)b * p.g.P + j] = mean * p.inv_S;
    }
    for (int j = cnt + t; j < p.g.P; j += SV_G) p.probs[(size_t)b * p.g.P + j] = 0.0f;
    if (t < SV_H) { hst[t] = hs[t]; cst[t] = c; }
}

// ============================================================================ host
struct SvConv { const float *w = nullptr, *b = nullptr; int cin = 0, cout = 0, k = 0, stride = 1; };

struct SvBranch {
    mis_silero_vad_branch_config cfg{};
    int n = 0, F = 0, F2 = 0, F3 = 0, S = 0, C = 0;
    const float* stft = nullptr;
    SvConv conv[4], wx;
    const float *Wh = nullptr, *wf = nullptr;
    float bf = 0.0f;
};

struct mis_silero_vad {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_silero_vad_config cfg{};
    SvBranch br[2];                                         // 16 kHz, 8 kHz
    HostWeights raw{"Silero VAD", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, work;
    DevBuf<int32_t> counts;                                 // nc[64] | lens[64]
    std::vector<int32_t> h_counts;
    float *pcm = nullptr, *mag = nullptr, *a[4] = {}, *gates = nullptr, *probs = nullptr, *state = nullptr;
    size_t pcm_cap = 0;
    SvGeom last{};
    const SvBranch* last_br = nullptr;
    int last_launches = 0;
    HipEvents<3 * SV_TIMED_PASSES> ev;
    float ms_front = 0.0f, ms_rec = 0.0f;
};

static const char* const SV_PREFIX[2] = {"branch16k.", "branch8k."};

static void sv_check_branch(const mis_silero_vad_branch_config& c, const char* name) {
    MIS_REQUIRE(c.filter_length >= 2 && c.filter_length <= 4096 && c.hop_length >= 1 && c.hop_length <= c.filter_length, MIS_ERR_INVALID_INPUT,
                "%s: filter_length %d / hop_length %d unsupported (2..4096, 1..filter_length)", name, c.filter_length, c.hop_length);
    MIS_REQUIRE(c.cutoff >= 1 && c.cutoff <= 2048, MIS_ERR_INVALID_INPUT, "%s: cutoff %d unsupported (1..2048)", name, c.cutoff);
    MIS_REQUIRE(c.chunk_size >= 1 && c.chunk_size <= 65536 && c.context_size >= 0 && c.context_size <= 65536, MIS_ERR_INVALID_INPUT,
                "%s: chunk_size %d / context_size %d unsupported (1..65536, 0..65536)", name, c.chunk_size, c.context_size);
    const int n = c.context_size + c.chunk_size;
    MIS_REQUIRE(c.pad >= 0 && n > c.pad, MIS_ERR_INVALID_INPUT, "%s: Reflect padding of %d requires more than %d samples (got %d)", name, c.pad,
                c.pad, n);
    MIS_REQUIRE(n + c.pad >= c.filter_length, MIS_ERR_INVALID_INPUT, "%s: a padded window of %d samples is shorter than the filter (%d)", name,
                n + c.pad, c.filter_length);
    MIS_REQUIRE((n + c.pad - c.filter_length) / c.hop_length + 1 <= 64, MIS_ERR_INVALID_INPUT, "%s: more than 64 frames a chunk", name);
}

static void sv_derive(SvBranch& b) {
    const auto& c = b.cfg;
    b.n = c.context_size + c.chunk_size; b.C = c.cutoff;
    b.F = (b.n + c.pad - c.filter_length) / c.hop_length + 1;
    b.F2 = (b.F - 1) / 2 + 1; b.F3 = (b.F2 - 1) / 2 + 1; b.S = b.F3;
}

extern "C" mis_status mis_silero_vad_create(const mis_silero_vad_config* cfg, int device, mis_silero_vad** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    // the configuration is judged before the device is touched
    sv_check_branch(cfg->branch16k, "branch_16k");
    sv_check_branch(cfg->branch8k, "branch_8k");
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= SV_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch must be 1..%d", SV_MAX_BATCH);
    MIS_REQUIRE(cfg->max_chunks >= 1 && cfg->max_chunks <= (1 << 16), MIS_ERR_INVALID_INPUT, "max_chunks must be 1..%d", 1 << 16);
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_silero_vad>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->br[0].cfg = cfg->branch16k; c->br[1].cfg = cfg->branch8k;
    sv_derive(c->br[0]); sv_derive(c->br[1]);
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_silero_vad_destroy(mis_silero_vad* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// name -> shape of every tensor of one branch, as SileroVAD.sanitize leaves the names
static std::vector<std::pair<std::string, std::vector<int64_t>>> sv_expected(const SvBranch& b, const char* prefix) {
    const std::string p = prefix;
    const int64_t C = b.C, Fl = b.cfg.filter_length;
    return {{p + "stft_conv.weight", {2 * C, Fl, 1}},
            {p + "conv1.weight", {128, 3, C}}, {p + "conv1.bias", {128}}, {p + "conv2.weight", {64, 3, 128}}, {p + "conv2.bias", {64}},
            {p + "conv3.weight", {64, 3, 64}}, {p + "conv3.bias", {64}}, {p + "conv4.weight", {128, 3, 64}}, {p + "conv4.bias", {128}},
            {p + "lstm.Wx", {SV_G, SV_H}}, {p + "lstm.Wh", {SV_G, SV_H}}, {p + "lstm.bias", {SV_G}},
            {p + "final_conv.weight", {1, 1, SV_H}}, {p + "final_conv.bias", {1}}};
}

// every name is set exactly once, with its shape checked here; host pointers
extern "C" mis_status mis_silero_vad_set_tensor(mis_silero_vad* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 3, c && c->finalized, dtype);
    const std::vector<int64_t> got(shape, shape + ndim);
    bool known = false;
    for (int i = 0; i < 2 && !known; ++i)
        for (const auto& e : sv_expected(c->br[i], SV_PREFIX[i]))
            if (e.first == name) {
                MIS_REQUIRE(e.second == got, MIS_ERR_INVALID_INPUT, "Silero VAD weight %s has the wrong shape", name);
                known = true;
                break;
            }
    MIS_REQUIRE(known, MIS_ERR_INVALID_INPUT, "Silero VAD: unexpected tensor %s", name);
    MIS_REQUIRE(!c->raw.count(name), MIS_ERR_INVALID_INPUT, "Silero VAD: tensor %s set twice", name);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of a sanitized checkpoint
extern "C" mis_status mis_silero_vad_init_synthetic(mis_silero_vad* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    c->raw.clear();
    SynthWeights sw{c->raw, seed * 100000ull};
    for (int i = 0; i < 2; ++i)
        for (const auto& e : sv_expected(c->br[i], SV_PREFIX[i])) {
            int64_t fan = 1;
            for (size_t d = 1; d < e.second.size(); ++d) fan *= e.second[d];
            const bool bias = e.second.size() == 1;
            sw.put(e.first, e.second, bias ? 0.05 : sqrt(3.0 / (double)fan), 0.0f);
        }
    MIS_API_END
}

extern "C" mis_status mis_silero_vad_finalize(mis_silero_vad* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    HostArena a(c->raw);
    size_t pcm_chunk = 0;
    for (int i = 0; i < 2; ++i) {
        SvBranch& b = c->br[i];
        const std::string p = SV_PREFIX[i];
        const int64_t C = b.C, Fl = b.cfg.filter_length;
        a.fvec(p + "stft_conv.weight", {2 * C, Fl, 1}, 2 * C * Fl, b.stft);
        const int64_t cin[4] = {C, 128, 64, 64}, cout[4] = {128, 64, 64, 128};
        for (int k = 0; k < 4; ++k) {
            const std::string q = p + "conv" + std::to_string(k + 1);
            b.conv[k].cin = (int)cin[k]; b.conv[k].cout = (int)cout[k]; b.conv[k].k = 3; b.conv[k].stride = (k == 1 || k == 2) ? 2 : 1;
            a.fvec(q + ".weight", {cout[k], 3, cin[k]}, cout[k] * 3 * cin[k], b.conv[k].w);
            a.fvec(q + ".bias", {cout[k]}, cout[k], b.conv[k].b);
        }
        b.wx.cin = SV_H; b.wx.cout = SV_G; b.wx.k = 1; b.wx.stride = 1;
        a.fvec(p + "lstm.Wx", {SV_G, SV_H}, SV_G * SV_H, b.wx.w);
        a.fvec(p + "lstm.bias", {SV_G}, SV_G, b.wx.b);
        a.fvec(p + "lstm.Wh", {SV_G, SV_H}, SV_G * SV_H, b.Wh);       // row t = thread t's slice, contiguous; arena offsets are 256-byte multiples
        a.fvec(p + "final_conv.weight", {1, 1, SV_H}, SV_H, b.wf);
        b.bf = c->raw.need(p + "final_conv.bias", {1}).v[0];
        pcm_chunk = std::max(pcm_chunk, (size_t)b.cfg.chunk_size);
    }
    // ---- the workspace, sized once (no call reads the handle before finalized is set: a rejected finalize can be repeated)
    const size_t B = c->cfg.max_batch, rows = B * (size_t)c->cfg.max_chunks;
    const size_t ctx = (size_t)std::max(c->br[0].cfg.context_size, c->br[1].cfg.context_size);
    c->pcm_cap = B * ((size_t)c->cfg.max_chunks * pcm_chunk + ctx);
    size_t mag = 0, a1 = 0, a2 = 0, a34 = 0, g = 0;                   // floats a chunk, the larger branch of each
    for (const SvBranch& b : c->br) {
        mag = std::max(mag, (size_t)b.F * b.C); a1 = std::max(a1, (size_t)b.F * 128); a2 = std::max(a2, (size_t)b.F2 * 64);
        a34 = std::max(a34, (size_t)b.F3 * 128); g = std::max(g, (size_t)b.S * SV_G);
    }
    const size_t sizes[9] = {c->pcm_cap, rows * mag, rows * a1, rows * a2, rows * a34, rows * a34, rows * g, rows, 2 * SV_MAX_BATCH * SV_H};
    size_t total = 0;
    for (size_t n : sizes) total += round_up(n, 64);
    MIS_REQUIRE(total * 4 <= ((size_t)24 << 30), MIS_ERR_INVALID_INPUT, "max_batch x max_chunks needs a workspace of %zu MiB (at most 24 GiB)",
                total * 4 >> 20);
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    c->work.alloc(total);
    c->counts.alloc(2 * SV_MAX_BATCH);
    c->h_counts.assign(2 * SV_MAX_BATCH, 0);
    float* w = c->work.p;
    float** dst[9] = {&c->pcm, &c->mag, &c->a[0], &c->a[1], &c->a[2], &c->a[3], &c->gates, &c->probs, &c->state};
    for (int i = 0; i < 9; ++i) { *dst[i] = w; w += round_up(sizes[i], 64); }
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// kernel launches of the last call: 7 a pass (STFT, conv1..conv4, Wx, recurrence)
extern "C" int mis_silero_vad_launches(const mis_silero_vad* c) { return c ? c->last_launches : 0; }

static const SvBranch& sv_branch(const mis_silero_vad* c, int sample_rate) {
    MIS_REQUIRE(sample_rate == 16000 || sample_rate == 8000, MIS_ERR_INVALID_INPUT, "Silero VAD supports 8000 Hz and 16000 Hz audio (got %d)",
                sample_rate);
    return c->br[sample_rate == 16000 ? 0 : 1];
}

// chunks of rows of lens[b] samples
extern "C" mis_status mis_silero_vad_chunks(const mis_silero_vad* c, const int64_t* lens, int batch, int sample_rate, int32_t* chunks_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && chunks_out && batch >= 0, MIS_ERR_INVALID_INPUT, "bad argument");
    const SvBranch& br = sv_branch(c, sample_rate);
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] < ((int64_t)1 << 30), MIS_ERR_INVALID_INPUT, "row %d: bad length", b);
        chunks_out[b] = (int32_t)((lens[b] + br.cfg.chunk_size - 1) / br.cfg.chunk_size);
    }
    MIS_API_END
}

static SvGemm sv_conv_gemm(const SvConv& l, const float* X, int Fin, float* Y, int Fo, int epi) {
    SvGemm g{};
    g.X = X; g.Fin = Fin; g.Cin = l.cin; g.stride = l.stride; g.padl = l.k / 2;
    g.W = l.w; g.bias = l.b; g.Y = Y; g.Fo = Fo; g.K = l.k * l.cin; g.N = l.cout; g.epi = epi;
    return g;
}

// The one driver: pcm f32 [B][stride] (host), h_counts set.  ctx_off = context (predict: window j starts context before chunk j) or 0
// (forward: the row IS the window).  Walks the chunks in passes, copies each pass's probabilities into probs_out [B][cols] and
// synchronises once, at the end.
static void sv_run(mis_silero_vad* c, const SvBranch& br, const float* pcm, int64_t stride, int B, int maxc, int ctx_off, const float* state_in,
                   float* probs_out, int cols, float* state_out) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->last_launches = 0; c->ms_front = c->ms_rec = 0.0f;
    const size_t st_bytes = (size_t)2 * B * SV_H * 4;
    if (maxc == 0) {                                                  // nothing to compute: the state passes through
        if (state_out) { if (state_in) memcpy(state_out, state_in, st_bytes); else memset(state_out, 0, st_bytes); }
        c->last.B = 0;
        return;
    }
    HIP_CHECK(hipMemcpyAsync(c->counts.p, c->h_counts.data(), 2 * SV_MAX_BATCH * 4, hipMemcpyHostToDevice, s));
    if (state_in) HIP_CHECK(hipMemcpyAsync(c->state, state_in, st_bytes, hipMemcpyHostToDevice, s));
    else HIP_CHECK(hipMemsetAsync(c->state, 0, st_bytes, s));
    const int chunk = br.cfg.chunk_size, Pmax = c->cfg.max_chunks;
    int launches = 0, passes = 0;
    SvGeom geo{c->counts.p, c->counts.p + SV_MAX_BATCH, 0, 0, B};
    for (int c0 = 0; c0 < maxc; c0 += Pmax, ++passes) {
        const int P = std::min(Pmax, maxc - c0);
        geo.c0 = c0; geo.P = P;
        const bool timed = passes < SV_TIMED_PASSES;
        if (timed) HIP_CHECK(hipEventRecord(c->ev[3 * passes], s));
        const int64_t s_lo = std::max<int64_t>(0, (int64_t)c0 * chunk - ctx_off), s_hi = std::min<int64_t>(stride, (int64_t)(c0 + P) * chunk - ctx_off + br.n - chunk);
        const int64_t ns = s_hi - s_lo;
        MIS_REQUIRE(ns >= 1 && (size_t)B * (size_t)ns <= c->pcm_cap, MIS_ERR_GENERATION_FAILED, "pass samples outside the workspace");
        HIP_CHECK(hipMemcpy2DAsync(c->pcm, (size_t)ns * 4, pcm + s_lo, (size_t)stride * 4, (size_t)ns * 4, B, hipMemcpyHostToDevice, s));
        const int BP = B * P;
        {
            SvGemm g{};
            g.pcm = c->pcm; g.pcm_ld = ns; g.s_lo = (int)s_lo; g.n = br.n; g.chunk = chunk; g.ctx_off = ctx_off; g.hop = br.cfg.hop_length;
            g.W = br.stft; g.Y = c->mag; g.Fo = br.F; g.K = br.cfg.filter_length; g.N = br.C; g.g = geo;
            hipLaunchKernelGGL((k_sv_gemm<true>), dim3(cdiv((int64_t)BP * br.F, 64), cdiv(br.C, 64)), dim3(256), 0, s, g);
        }
        const int Fin[4] = {br.F, br.F, br.F2, br.F3}, Fo[4] = {br.F, br.F2, br.F3, br.F3};
        const float* x = c->mag;
        for (int k = 0; k < 4; ++k) {
            SvGemm g = sv_conv_gemm(br.conv[k], x, Fin[k], c->a[k], Fo[k], SV_EPI_RELU);
            g.g = geo;
            hipLaunchKernelGGL((k_sv_gemm<false>), dim3(cdiv((int64_t)BP * Fo[k], 64), cdiv(g.N, 64)), dim3(256), 0, s, g);
            x = c->a[k];
        }
        {
            SvGemm g = sv_conv_gemm(br.wx, x, br.S, c->gates, br.S, SV_EPI_PLAIN);
            g.g = geo;
            hipLaunchKernelGGL((k_sv_gemm<false>), dim3(cdiv((int64_t)BP * br.S, 64), cdiv(g.N, 64)), dim3(256), 0, s, g);
        }
        if (timed) HIP_CHECK(hipEventRecord(c->ev[3 * passes + 1], s));
        SvLstm l{c->gates, br.Wh, br.wf, br.bf, c->state, c->probs, geo, br.S, 1.0f / (float)br.S};
        hipLaunchKernelGGL(k_sv_lstm, dim3(B), dim3(SV_G), 0, s, l);
        launches += 7;
        if (timed) HIP_CHECK(hipEventRecord(c->ev[3 * passes + 2], s));
        if (probs_out)
            HIP_CHECK(hipMemcpy2DAsync(probs_out + c0, (size_t)cols * 4, c->probs, (size_t)P * 4, (size_t)P * 4, B, hipMemcpyDeviceToHost, s));
    }
    if (state_out) HIP_CHECK(hipMemcpyAsync(state_out, c->state, st_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                               // the one synchronisation of a call
    for (int i = 0; i < std::min(passes, SV_TIMED_PASSES); ++i) {
        float f = 0.0f, r = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&f, c->ev[3 * i], c->ev[3 * i + 1]));
        HIP_CHECK(hipEventElapsedTime(&r, c->ev[3 * i + 1], c->ev[3 * i + 2]));
        c->ms_front += f; c->ms_rec += r;
    }
    c->last = geo; c->last_br = &br; c->last_launches = launches;
}

static void sv_check_call(const mis_silero_vad* c, int batch) {
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "Silero VAD model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
}

// predictProba for a ragged batch: pcm f32 [batch, stride], lens[batch] (NULL = stride) -> probs f32 [batch, cols], cols >= the longest
// row's chunks, zeros behind a row's own.  state f32 [2, batch, 128]: NULL in = zeros, NULL out = not returned.
extern "C" mis_status mis_silero_vad_predict(mis_silero_vad* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int sample_rate,
                                             float* probs_out, int cols, const float* state_in, float* state_out) {
    MIS_API_BEGIN
    sv_check_call(c, batch);
    MIS_REQUIRE(pcm && stride >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    const SvBranch& br = sv_branch(c, sample_rate);
    int maxc = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride && n < ((int64_t)1 << 30), MIS_ERR_INVALID_INPUT, "row %d: %lld samples, the row stride is %lld", b,
                    (long long)n, (long long)stride);
        c->h_counts[b] = (int32_t)((n + br.cfg.chunk_size - 1) / br.cfg.chunk_size);
        c->h_counts[SV_MAX_BATCH + b] = (int32_t)n;
        maxc = std::max(maxc, c->h_counts[b]);
    }
    MIS_REQUIRE(maxc == 0 || (probs_out && cols >= maxc), MIS_ERR_INVALID_INPUT, "probs: room for %d chunks, %d are needed", cols, maxc);
    sv_run(c, br, pcm, stride, batch, maxc, br.cfg.context_size, state_in, probs_out, cols, state_out);
    MIS_API_END
}

// callAsFunction, one chunk: windows f32 [batch, context + chunk] -> probs f32 [batch]
extern "C" mis_status mis_silero_vad_forward(mis_silero_vad* c, const float* windows, int batch, int sample_rate, const float* state_in,
                                             float* probs_out, float* state_out) {
    MIS_API_BEGIN
    sv_check_call(c, batch);
    MIS_REQUIRE(windows && probs_out, MIS_ERR_INVALID_INPUT, "null argument");
    const SvBranch& br = sv_branch(c, sample_rate);
    for (int b = 0; b < batch; ++b) { c->h_counts[b] = 1; c->h_counts[SV_MAX_BATCH + b] = br.n; }
    sv_run(c, br, windows, br.n, batch, 1, 0, state_in, probs_out, 1, state_out);
    MIS_API_END
}

// tensors of the last pass of the last call, f32, zeros behind a row's own chunks.  stage 0 magnitude [B, P F, cutoff], 1 conv1
// [B, P F, 128], 2 conv2 [B, P F2, 64], 3 conv3 [B, P F3, 64], 4 conv4 [B, P F3, 128], 5 gate pre-activations Wx x + b [B, P S, 512],
// 6 probabilities [B, P, 1].
extern "C" mis_status mis_silero_vad_tap(mis_silero_vad* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && stage >= 0 && stage <= 6, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(c->last.B > 0 && c->last_br, MIS_ERR_INVALID_INPUT, "no call to tap");
    HIP_CHECK(hipSetDevice(c->device));
    const SvBranch& br = *c->last_br;
    const size_t B = c->last.B, P = c->last.P;
    const float* src[7] = {c->mag, c->a[0], c->a[1], c->a[2], c->a[3], c->gates, c->probs};
    const size_t fr[7] = {(size_t)br.F, (size_t)br.F, (size_t)br.F2, (size_t)br.F3, (size_t)br.F3, (size_t)br.S, 1};
    const size_t wd[7] = {(size_t)br.C, 128, 64, 64, 128, SV_G, 1};
    const size_t n = P * fr[stage], width = wd[stage];
    if (dims) { dims[0] = (int64_t)B; dims[1] = (int64_t)n; dims[2] = (int64_t)width; }
    if (!out) return MIS_OK;
    MIS_REQUIRE((int64_t)(B * n * width) <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    HIP_CHECK(hipMemcpy(out, src[stage], B * n * width * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// measurements: device milliseconds of the last call summed over its first 64 passes, ms[2] = front end (copy in + six contractions),
// recurrence
extern "C" mis_status mis_debug_silero_vad_timing(const mis_silero_vad* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && ms, MIS_ERR_INVALID_INPUT, "null argument");
    ms[0] = c->ms_front; ms[1] = c->ms_rec;
    MIS_API_END
}
