// fsmn_vad.hip - FSMN voice activity detection: waveform -> Kaldi-style fbank + per-frame decibel -> LFR stacking + CMVN -> FSMN encoder
// -> softmax scores and the per-frame sum over the silence pdf ids.
//
// Reference being replaced: FSMNVAD (Sources/MLXAudioVAD/Models/FSMNVAD/FSMNVAD.swift): computeKaldiFbank / kaldiMelFilterbank (:821-955),
// applyLFR (:866-898), the CMVN of extractFeatures (:736-738), FSMNVADEncoder (:160-237) and computeDecibel (:373-392).  The serial
// post-processing (:239-701) stays on the host (vad.py): it reads two floats a frame.
//
// One call serves 1..max_batch ragged rows of any length.  Row b has n_b samples, T_b = 1 + (n_b - win) / hop fbank frames (0 below one
// window) and R_b = (T_b + (lfr_m - 1) / 2 + lfr_n - 1) / lfr_n LFR rows.  The encoder is causal with a reach of fsmn_layers (lorder - 1)
// rows, so the C side walks the LFR rows in chunks of chunk_frames, recomputing that many rows of left halo (and the fbank frames they
// stack), and every chunk uses the one workspace sized at finalize.  A chunk computes rows [g0, r1) of every row of the batch into
// f32 [B][nr][C] buffers, nr = r1 - g0; a kernel derives a row's own count from R_b and the chunk, loads zeros outside it and writes
// zeros behind it.  Every output element is one fixed-order sum that depends on the row alone, so a row's result is the same bit for
// bit whatever batch, padding or chunking it travels in.
//
//   k_fvad_fbank   one frame per block: x 32768, minus the frame mean, pre-emphasis 0.97 with the first sample kept (:838-843), symmetric
//                  Hamming, 512-point radix-2 FFT in LDS, power, the sparse HTK triangles (each filter over its own bins, the Nyquist
//                  bin never read), log max(., 1e-8); and the frame's 10 log10(sum x^2 + 1e-6) over the raw samples (block_sum_256)
//   k_fvad_lfr     the stacked, CMVN-ed features as a tensor (features / tap only: the forward pass gathers them in in_linear1's load)
//   k_fvad_gemm    the one contraction, exact f32 on v_mfma_f32_32x32x2_f32, every dimension guarded.  Loads: activations, the LFR + CMVN
//                  gather from the fbank, or the memory block p + depthwise_causal_conv(p) formed from a time tile + lorder - 1 rows of
//                  halo in LDS.  Epilogues: bias / none, ReLU, or (256-column tile) bias + softmax + the silence sum. (On f32_tile.h.)
//
// A chunk is 5 + 2 fsmn_layers launches (13 at the published depth): fbank, in_linear1 (LFR load), in_linear2, per layer linear and
// affine (memory-block load), out_linear1, out_linear2 + softmax.  No allocation and one synchronisation per call.
#include "common.h"
#include "audio_front.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define FV_MAX_BATCH 64
#define FV_NFFT 512
#define FV_BINS 256               // bins 0..255 carry filters; the reference's loop never reaches the Nyquist bin (:943)
#define FV_LMAX 64                // lorder
#define FV_MAX_SIL 16
#define FV_TIMED_CHUNKS 128

enum { FV_LOAD_ACT = 0, FV_LOAD_LFR = 1, FV_LOAD_MEM = 2 };
enum { FV_EPI_PLAIN = 0, FV_EPI_RELU = 1, FV_EPI_SOFTMAX = 2 };

// a chunk: LFR rows [g0, r1) of every row (nr of them), fbank frames [fa, fa + nf)
struct FvGeom { const int32_t* T; const int32_t* R; int g0, r1, nr, fa, nf; };

__device__ __forceinline__ int fv_count(const FvGeom& g, int b) {
    const int c = min(g.R[b], g.r1) - g.g0;
    return c < 0 ? 0 : (c > g.nr ? g.nr : c);
}

struct FvLfr { const float* fbank; const float* shift; const float* scale; int nm, m, n, lp; };

// LFR row g0 + l, column ci of row b: slot i = ci / nm of fbank frame clamp((g0 + l) n + i - lp, 0, T_b - 1) (:876-886), then
// (x + shift) scale, each rounded on its own
__device__ __forceinline__ float fv_lfr_value(const FvLfr& q, const FvGeom& g, int b, int l, int ci) {
    const int i = ci / q.nm, f = ci - i * q.nm;
    int src = (g.g0 + l) * q.n + i - q.lp;
    src = min(max(src, 0), g.T[b] - 1) - g.fa;
    src = min(max(src, 0), g.nf - 1);
    float v = q.fbank[((size_t)b * g.nf + src) * q.nm + f];
    if (q.shift) v = __fmul_rn(__fadd_rn(v, q.shift[ci]), q.scale[ci]);
    return v;
}

struct FvFront {
    const float* pcm; int64_t pcm_stride;                   // the chunk's samples: [B][pcm_stride], sample 0 is frame fa's first
    const float *win, *twc, *tws, *fb; const int32_t* fbr;  // window [wlen], twiddles [256], filters [256][nm], bin range per filter
    float *fbank, *dec;                                      // [B][nf][nm], [B][nf]
    FvGeom g; int wlen, hop, nm; float log_floor;
};

__global__ void __launch_bounds__(256) k_fvad_fbank(FvFront p) {
    __shared__ float re[FV_NFFT], im[FV_NFFT], red[4];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* o = p.fbank + ((size_t)b * p.g.nf + f) * p.nm;
    if (p.g.fa + f >= p.g.T[b]) {
        if (tid < p.nm) o[tid] = 0.0f;
        if (tid == 0) p.dec[(size_t)b * p.g.nf + f] = 0.0f;
        return;
    }
    const float* x = p.pcm + (size_t)b * p.pcm_stride + (size_t)f * p.hop;
    const float v0 = tid < p.wlen ? x[tid] : 0.0f, v1 = tid + 256 < p.wlen ? x[tid + 256] : 0.0f;
    const float s0 = v0 * 32768.0f, s1 = v1 * 32768.0f;
    const float energy = block_sum_256(fmaf(v1, v1, v0 * v0), red);
    const float mean = block_sum_256(s0 + s1, red) / (float)p.wlen;
    im[tid] = s0 - mean; im[tid + 256] = s1 - mean;
    __syncthreads();
    for (int j = tid; j < FV_NFFT; j += 256) {
        float y = 0.0f;
        if (j < p.wlen) {
            y = j == 0 ? im[0] : __fsub_rn(im[j], __fmul_rn(0.97f, im[j - 1]));
            y = __fmul_rn(y, p.win[j]);
        }
        re[__brev((unsigned)j) >> 23] = y;
    }
    __syncthreads();
    im[tid] = 0.0f; im[tid + 256] = 0.0f;
    __syncthreads();
    for (int half = 1; half < FV_NFFT; half <<= 1) {
        const int k = tid & (half - 1), i0 = ((tid - k) << 1) + k, i1 = i0 + half, ti = k * (FV_NFFT / 2 / half);
        const float c = p.twc[ti], s = p.tws[ti];
        const float xr = re[i1], xi = im[i1];
        const float pr = xr * c - xi * s, pi = xr * s + xi * c;
        const float ar = re[i0], ai = im[i0];
        re[i0] = ar + pr; im[i0] = ai + pi; re[i1] = ar - pr; im[i1] = ai - pi;
        __syncthreads();
    }
    { const float a = re[tid], c = im[tid]; re[tid] = a * a + c * c; }          // bins 0..255
    __syncthreads();
    if (tid < p.nm) {
        float acc = 0.0f;
        for (int i = p.fbr[2 * tid]; i < p.fbr[2 * tid + 1]; ++i) acc = fmaf(re[i], p.fb[(size_t)i * p.nm + tid], acc);
        o[tid] = acc > 1e-8f ? logf(acc) : p.log_floor;
    }
    if (tid == 0) p.dec[(size_t)b * p.g.nf + f] = (float)(10.0 * log10((double)(energy + 1e-6f)));
}

// feat[b][l][ci] for l < nr: the row's LFR rows of the chunk, zeros behind them
__global__ void __launch_bounds__(256) k_fvad_lfr(FvLfr q, FvGeom g, float* __restrict__ feat, int D, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ci = (int)(i % D);
    const size_t r = i / D;
    const int l = (int)(r % g.nr), b = (int)(r / g.nr);
    feat[i] = l < fv_count(g, b) ? fv_lfr_value(q, g, b, l, ci) : 0.0f;
}

struct FvGemm {
    const float* X; int ldx;                                // ACT / MEM: [B][nr][ldx]
    FvLfr lfr;                                              // LFR
    const float* dw; int lorder;                            // MEM: depthwise taps [Cin][lorder]
    const float* W; const float* bias;                      // [Cout][Cin]; bias may be null
    float* Y; int ldy;
    float* sil; const int32_t* sil_ids; int n_sil;          // SOFTMAX: [B][nr], the ids summed in their order
    FvGeom g; int Cin, Cout, epi, load;
};

// WT x (4 / WT) waves, CT 32-column accumulators a wave: <2, 1> is a 64 x 64 tile, <1, 2> a 32 x 256 tile that holds a whole score row
template <int WT, int CT>
__global__ void __launch_bounds__(256) k_fvad_gemm(FvGemm p) {
    constexpr int WCW = 4 / WT, TT = 32 * WT, TC = 32 * WCW * CT;
    constexpr bool WIDE = CT > 1;
    __shared__ float As[TT][F32_KC + 1];
    __shared__ float Bs[TC][F32_KC + 1];
    __shared__ float Hs[WIDE ? 1 : TT + FV_LMAX - 1][F32_KC + 1];
    __shared__ float Ws[WIDE ? 1 : F32_KC][FV_LMAX + 1];
    const int b = blockIdx.z, t0 = blockIdx.x * TT, c0 = blockIdx.y * TC, nr = p.g.nr;
    const int cnt = fv_count(p.g, b), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t row0 = (size_t)b * nr;
    if (t0 >= cnt) {                                                  // nothing of the row here: zeros
        f32_tile_zero<TT, TC>(p.Y, p.ldy, row0, t0, c0, nr, p.Cout);
        if (p.epi == FV_EPI_SOFTMAX && tid < TT && t0 + tid < nr) p.sil[row0 + t0 + tid] = 0.0f;
        return;
    }
    f32x16_t acc[CT] = {};
    const int wt = (wave % WT) * 32, wc = (wave / WT) * CT * 32, kh = lane >> 5, l31 = lane & 31;
    for (int ci0 = 0; ci0 < p.Cin; ci0 += F32_KC) {
        if constexpr (!WIDE) {
            if (p.load == FV_LOAD_MEM) {
                const int L = p.lorder, nh = TT + L - 1;
                for (int i = tid; i < nh * F32_KC; i += 256) {
                    const int h = i >> 5, ci = ci0 + (i & 31), t = t0 - (L - 1) + h;
                    Hs[h][i & 31] = (ci < p.Cin && t >= 0 && t < cnt) ? p.X[(row0 + t) * p.ldx + ci] : 0.0f;
                }
                for (int i = tid; i < F32_KC * L; i += 256) {
                    const int c = i / L, j = i - c * L;
                    Ws[c][j] = ci0 + c < p.Cin ? p.dw[(size_t)(ci0 + c) * L + j] : 0.0f;
                }
                __syncthreads();
#pragma unroll
                for (int n = 0; n < TT * F32_KC / 256; ++n) {          // x[t] + sum_j w[j] x[t + j - (L - 1)], taps ascending
                    const int i = tid + n * 256, r = i >> 5, cc = i & 31;
                    float a = 0.0f;
                    for (int j = 0; j < L; ++j) a = fmaf(Ws[cc][j], Hs[r + j][cc], a);
                    As[r][cc] = Hs[r + L - 1][cc] + a;
                }
            }
        }
        if (WIDE || p.load != FV_LOAD_MEM) {
#pragma unroll
            for (int n = 0; n < TT * F32_KC / 256; ++n) {
                const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), t = t0 + r;
                float v = 0.0f;
                if (ci < p.Cin && t < cnt) v = p.load == FV_LOAD_LFR ? fv_lfr_value(p.lfr, p.g, b, t, ci) : p.X[(row0 + t) * p.ldx + ci];
                As[r][i & 31] = v;
            }
        }
#pragma unroll
        for (int n = 0; n < TC * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), co = c0 + r;
            Bs[r][i & 31] = (co < p.Cout && ci < p.Cin) ? p.W[(size_t)co * p.Cin + ci] : 0.0f;
        }
        __syncthreads();
        f32_tile_mfma(As, Bs, wt + l31, wc + l31, kh, acc);
        __syncthreads();
    }
    // C/D: column (output channel) = lane & 31, row (frame) = f32_tile_row(r, lane >> 5)
    if constexpr (WIDE) {
        if (p.epi == FV_EPI_SOFTMAX) {                                // (one block column: c0 = 0, Cout <= TC)
            float* Ls = &Bs[0][0];                                    // logits [TT][TC + 1]
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const int co = wc + ct * 32 + l31;
                const float add = (co < p.Cout && p.bias) ? p.bias[co] : 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) Ls[f32_tile_row(r, kh) * (TC + 1) + co] = acc[ct][r] + add;
            }
            __syncthreads();
            for (int rr = wave; rr < TT; rr += 4) {                   // a wave per frame; the 64 partial maxima / sums meet in a fixed order
                const int t = t0 + rr;
                if (t >= nr) break;
                const float* lg = Ls + rr * (TC + 1);
                float mx = -INFINITY;
                for (int co = lane; co < p.Cout; co += 64) mx = fmaxf(mx, lg[co]);
                mx = wave_max(mx);
                float s = 0.0f;
                for (int co = lane; co < p.Cout; co += 64) s += expf(lg[co] - mx);
                s = wave_sum(s);
                const bool live = t < cnt;
                for (int co = lane; co < p.Cout; co += 64) p.Y[(row0 + t) * p.ldy + co] = live ? expf(lg[co] - mx) / s : 0.0f;
                if (lane == 0) {
                    float q = 0.0f;
                    for (int k = 0; k < p.n_sil; ++k) q += expf(lg[p.sil_ids[k]] - mx) / s;
                    p.sil[row0 + t] = live ? q : 0.0f;
                }
            }
            return;
        }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int co = c0 + wc + ct * 32 + l31;
        if (co >= p.Cout) continue;
        const float add = p.bias ? p.bias[co] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = t0 + wt + f32_tile_row(r, kh);
            if (t >= nr) continue;
            float v = acc[ct][r] + add;
            if (p.epi == FV_EPI_RELU) v = fmaxf(v, 0.0f);
            p.Y[(row0 + t) * p.ldy + co] = t < cnt ? v : 0.0f;
        }
    }
}

// ============================================================================ host
struct FvLin { const float *w, *b; int cin, cout; };
struct FvLayer { FvLin linear, affine; const float* dw; };

struct mis_fsmn_vad {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_fsmn_vad_config cfg{};
    int D = 0, A = 0, Ld = 0, P = 0, L = 0, NL = 0, Ao = 0, O = 0, nm = 0, wlen = 0, hop = 0, m = 0, n = 0, lp = 0, halo = 0;
    int Rc = 0, Fc = 0;                                     // LFR rows / fbank frames a chunk can hold
    int64_t Sc = 0;                                         // samples a chunk can hold
    HostWeights raw{"FSMN VAD", MIS_ERR_INVALID_INPUT};
    bool finalized = false, has_cmvn = false;
    DevBuf<float> farena, work, pcm;
    DevBuf<int32_t> counts, iarena;                         // T[64] | R[64]; filter bin ranges | silence ids
    std::vector<int32_t> h_T, h_R;
    const float *win = nullptr, *twc = nullptr, *tws = nullptr, *fb = nullptr, *shift = nullptr, *scale = nullptr;
    const int32_t *fbr = nullptr, *sil_ids = nullptr;
    FvLin in1{}, in2{}, out1{}, out2{};
    std::vector<FvLayer> layers;
    float *fbank = nullptr, *dec = nullptr, *feat = nullptr, *a1 = nullptr, *h0 = nullptr, *ao = nullptr, *scores = nullptr, *sil = nullptr;
    std::vector<float*> pbuf, hbuf;
    FvGeom last{};                                          // the last chunk of the last call (tap)
    int last_batch = 0, last_launches = 0;
    bool last_front = false;
    HipEvents<3 * FV_TIMED_CHUNKS> ev;
    float ms_front = 0.0f, ms_model = 0.0f;
};

static int fv_frames_of(const mis_fsmn_vad* c, int64_t n) { return n < c->wlen ? 0 : (int)(1 + (n - c->wlen) / c->hop); }
static int fv_rows_of(const mis_fsmn_vad* c, int T) { return T <= 0 ? 0 : (T + c->lp + c->n - 1) / c->n; }

extern "C" mis_status mis_fsmn_vad_create(const mis_fsmn_vad_config* cfg, int device, mis_fsmn_vad** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    // the configuration is judged before the device is touched
    MIS_REQUIRE(cfg->lstride == 1, MIS_ERR_INVALID_INPUT, "lstride %d unsupported: the reference's memory block keeps its length only at lstride 1",
                cfg->lstride);
    MIS_REQUIRE(cfg->fsmn_layers >= 0 && cfg->fsmn_layers <= 64, MIS_ERR_INVALID_INPUT, "fsmn_layers %d unsupported (0..64)", cfg->fsmn_layers);
    MIS_REQUIRE(cfg->lorder >= 1 && cfg->lorder <= FV_LMAX, MIS_ERR_INVALID_INPUT, "lorder %d unsupported (1..%d)", cfg->lorder, FV_LMAX);
    for (int v : {cfg->input_dim, cfg->input_affine_dim, cfg->linear_dim, cfg->proj_dim, cfg->output_affine_dim})
        MIS_REQUIRE(v >= 1 && v <= 4096, MIS_ERR_INVALID_INPUT, "layer width %d unsupported (1..4096)", v);
    MIS_REQUIRE(cfg->output_dim >= 1 && cfg->output_dim <= 256, MIS_ERR_INVALID_INPUT, "output_dim %d unsupported (1..256: one softmax tile)",
                cfg->output_dim);
    MIS_REQUIRE(cfg->n_mels >= 1 && cfg->n_mels <= 256, MIS_ERR_INVALID_INPUT, "n_mels %d unsupported (1..256)", cfg->n_mels);
    MIS_REQUIRE(cfg->lfr_m >= 1 && cfg->lfr_m <= 64 && cfg->lfr_n >= 1 && cfg->lfr_n <= cfg->lfr_m, MIS_ERR_INVALID_INPUT,
                "lfr_m %d / lfr_n %d unsupported (1 <= lfr_n <= lfr_m <= 64)", cfg->lfr_m, cfg->lfr_n);
    MIS_REQUIRE(cfg->input_dim == cfg->n_mels * cfg->lfr_m, MIS_ERR_INVALID_INPUT, "input_dim %d is not n_mels x lfr_m = %d", cfg->input_dim,
                cfg->n_mels * cfg->lfr_m);
    MIS_REQUIRE(cfg->sample_rate >= 1000 && cfg->sample_rate <= 192000 && cfg->frame_length >= 1 && cfg->frame_shift >= 1, MIS_ERR_INVALID_INPUT,
                "sample_rate / frame_length / frame_shift unsupported");
    const int64_t wlen = (int64_t)cfg->sample_rate * cfg->frame_length / 1000, hop = (int64_t)cfg->sample_rate * cfg->frame_shift / 1000;
    MIS_REQUIRE(wlen > FV_NFFT / 2 && wlen <= FV_NFFT, MIS_ERR_INVALID_INPUT, "a window of %lld samples is unsupported (257..512: a 512-point FFT)",
                (long long)wlen);
    MIS_REQUIRE(hop >= 1 && hop <= 4096, MIS_ERR_INVALID_INPUT, "a frame shift of %lld samples is unsupported (1..4096)", (long long)hop);
    MIS_REQUIRE(cfg->n_sil >= 0 && cfg->n_sil <= FV_MAX_SIL, MIS_ERR_INVALID_INPUT, "%d silence pdf ids (0..%d)", cfg->n_sil, FV_MAX_SIL);
    for (int i = 0; i < cfg->n_sil; ++i)
        MIS_REQUIRE(cfg->sil_pdf_ids[i] >= 0 && cfg->sil_pdf_ids[i] < cfg->output_dim, MIS_ERR_INVALID_INPUT, "sil_pdf_ids[%d] = %d outside the scores",
                    i, cfg->sil_pdf_ids[i]);
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= FV_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch must be 1..%d", FV_MAX_BATCH);
    MIS_REQUIRE(cfg->chunk_frames >= 1 && cfg->chunk_frames <= (1 << 20), MIS_ERR_INVALID_INPUT, "chunk_frames must be 1..%d", 1 << 20);
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_fsmn_vad>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->D = cfg->input_dim; c->A = cfg->input_affine_dim; c->Ld = cfg->linear_dim; c->P = cfg->proj_dim; c->L = cfg->lorder; c->NL = cfg->fsmn_layers;
    c->Ao = cfg->output_affine_dim; c->O = cfg->output_dim; c->nm = cfg->n_mels; c->wlen = (int)wlen; c->hop = (int)hop;
    c->m = cfg->lfr_m; c->n = cfg->lfr_n; c->lp = (cfg->lfr_m - 1) / 2; c->halo = cfg->fsmn_layers * (cfg->lorder - 1);
    c->Rc = cfg->chunk_frames + c->halo; c->Fc = c->Rc * c->n + c->m; c->Sc = (int64_t)c->Fc * c->hop + c->wlen;
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_fsmn_vad_destroy(mis_fsmn_vad* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// names as fsmn_vad_sanitize leaves them: in_linear{1,2}.{weight,bias}, fsmn.N.linear.weight, fsmn.N.fsmn_block.conv_left.weight
// [proj, lorder, 1], fsmn.N.affine.{weight,bias}, out_linear{1,2}.{weight,bias}; optional cmvn.shift / cmvn.scale; host pointers
extern "C" mis_status mis_fsmn_vad_set_tensor(mis_fsmn_vad* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 3, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

static float fv_kaldi_mel(float f) { return 1127.0f * logf(1.0f + f / 700.0f); }

extern "C" mis_status mis_fsmn_vad_finalize(mis_fsmn_vad* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t D = c->D, A = c->A, Ld = c->Ld, P = c->P, L = c->L, Ao = c->Ao, O = c->O, nm = c->nm;
    HostArena a(c->raw);
    std::vector<float>& fh = a.fhost;
    auto lin = [&](const std::string& p, int64_t cout, int64_t cin, bool bias, FvLin& l) {
        l = FvLin{nullptr, nullptr, (int)cin, (int)cout};
        a.fvec(p + ".weight", {cout, cin}, cout * cin, l.w);
        if (bias) a.fvec(p + ".bias", {cout}, cout, l.b);
    };
    lin("in_linear1", A, D, true, c->in1); lin("in_linear2", Ld, A, true, c->in2);
    c->layers.assign(c->NL, FvLayer{});
    for (int i = 0; i < c->NL; ++i) {
        const std::string q = "fsmn." + std::to_string(i);
        lin(q + ".linear", P, Ld, false, c->layers[i].linear);
        a.fvec(q + ".fsmn_block.conv_left.weight", {P, L, 1}, P * L, c->layers[i].dw);
        lin(q + ".affine", Ld, P, true, c->layers[i].affine);
    }
    lin("out_linear1", Ao, Ld, true, c->out1); lin("out_linear2", O, Ao, true, c->out2);
    // CMVN: applied only when both tensors have the feature width (FSMNVAD.swift:736)
    const HostTensor *sh = c->raw.find("cmvn.shift"), *sc = c->raw.find("cmvn.scale");
    const bool cmvn = sh && sc && (int64_t)sh->v.size() == D && (int64_t)sc->v.size() == D;
    c->shift = c->scale = nullptr;
    if (cmvn) {
        const size_t o_shift = a.ftake(D, c->shift), o_scale = a.ftake(D, c->scale);
        for (int64_t i = 0; i < D; ++i) { fh[o_shift + i] = sh->v[i]; fh[o_scale + i] = sc->v[i]; }
    }
    // front end: symmetric Hamming window, twiddles, and the filters in the reference's own f32 arithmetic (:923-955), [bin][mel]
    const size_t o_win = a.ftake(c->wlen, c->win), o_twc = a.ftake(FV_NFFT / 2, c->twc), o_tws = a.ftake(FV_NFFT / 2, c->tws),
                 o_fb = a.ftake((size_t)FV_BINS * nm, c->fb);
    const double PI = 3.14159265358979323846;
    for (int i = 0; i < c->wlen; ++i) fh[o_win + i] = (float)(0.54 - 0.46 * cos(2.0 * PI * i / (double)(c->wlen - 1)));
    fft512_twiddles(&fh[o_twc], &fh[o_tws]);
    std::vector<int32_t> ih((size_t)round_up(2 * nm, 64) + 64, 0);
    {
        const float nyquist = 0.5f * (float)c->cfg.sample_rate, width = (float)c->cfg.sample_rate / (float)FV_NFFT;
        const float mel_low = fv_kaldi_mel(20.0f), mel_high = fv_kaldi_mel(0.0f + nyquist), delta = (mel_high - mel_low) / (float)(nm + 1);
        for (int j = 0; j < nm; ++j) {
            const float left = mel_low + (float)j * delta, center = mel_low + (float)(j + 1) * delta, right = mel_low + (float)(j + 2) * delta;
            for (int i = 0; i < FV_BINS; ++i) {
                const float mel = fv_kaldi_mel(width * (float)i);
                const float up = (mel - left) / (center - left), down = (right - mel) / (right - center);
                fh[o_fb + (size_t)i * nm + j] = std::max(0.0f, std::min(up, down));
            }
        }
        filter_bin_ranges(&fh[o_fb], FV_BINS, (int)nm, ih.data());
    }
    const size_t o_sil = round_up(2 * nm, 64);
    for (int i = 0; i < c->cfg.n_sil; ++i) ih[o_sil + i] = c->cfg.sil_pdf_ids[i];
    // ---- the workspace, sized once (no call reads the handle before finalized is set: a rejected finalize can be repeated)
    const size_t B = c->cfg.max_batch, rows = B * (size_t)c->Rc, frames = B * (size_t)c->Fc;
    const size_t per_row = D + A + Ld + (size_t)c->NL * (P + Ld) + Ao + O + 1;
    const size_t total = frames * (nm + 1) + rows * per_row + 64 * 32;
    MIS_REQUIRE((total + B * (size_t)c->Sc) * 4 <= ((size_t)24 << 30), MIS_ERR_INVALID_INPUT,
                "max_batch x chunk_frames needs a workspace of %zu MiB (at most 24 GiB)", (total + B * (size_t)c->Sc) * 4 >> 20);
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    c->iarena.alloc(ih.size());
    HIP_CHECK(hipMemcpy(c->iarena.p, ih.data(), ih.size() * 4, hipMemcpyHostToDevice));
    c->work.alloc(total);
    c->pcm.alloc(B * (size_t)c->Sc);
    c->counts.alloc(2 * FV_MAX_BATCH);
    c->h_T.assign(FV_MAX_BATCH, 0); c->h_R.assign(FV_MAX_BATCH, 0);
    float* w = c->work.p;
    auto take = [&](size_t n) { float* p = w; w += round_up(n, 64); return p; };
    c->fbank = take(frames * nm); c->dec = take(frames); c->feat = take(rows * D); c->a1 = take(rows * A); c->h0 = take(rows * Ld);
    c->pbuf.clear(); c->hbuf.clear();
    for (int i = 0; i < c->NL; ++i) { c->pbuf.push_back(take(rows * P)); c->hbuf.push_back(take(rows * Ld)); }
    c->ao = take(rows * Ao); c->scores = take(rows * O); c->sil = take(rows);
    c->has_cmvn = cmvn;
    c->fbr = c->iarena.p; c->sil_ids = c->iarena.p + o_sil;
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of a sanitized checkpoint and a CMVN
extern "C" mis_status mis_fsmn_vad_init_synthetic(mis_fsmn_vad* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    sw.lin("in_linear1", c->A, c->D, true, 1.0);
    sw.lin("in_linear2", c->Ld, c->A, true, 1.0);
    for (int i = 0; i < c->NL; ++i) {
        const std::string q = "fsmn." + std::to_string(i);
        sw.lin(q + ".linear", c->P, c->Ld, false, 1.0);
        sw.put(q + ".fsmn_block.conv_left.weight", {c->P, c->L, 1}, sqrt(3.0 / (double)c->L), 0.0f);
        sw.lin(q + ".affine", c->Ld, c->P, true, 1.0);
    }
    sw.lin("out_linear1", c->Ao, c->Ld, true, 1.0);
    sw.lin("out_linear2", c->O, c->Ao, true, 2.0);
    sw.put("cmvn.shift", {c->D}, 1.0, -8.0f);
    sw.put("cmvn.scale", {c->D}, 0.05, 0.2f);
    MIS_API_END
}

extern "C" int mis_fsmn_vad_launches(const mis_fsmn_vad* c) { return c ? c->last_launches : 0; }

extern "C" mis_status mis_fsmn_vad_frames(const mis_fsmn_vad* c, const int64_t* lens, int batch, int32_t* frames, int32_t* rows) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 0, MIS_ERR_INVALID_INPUT, "bad argument");
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] < ((int64_t)1 << 40), MIS_ERR_INVALID_INPUT, "row %d: bad length", b);
        const int64_t T = lens[b] < c->wlen ? 0 : 1 + (lens[b] - c->wlen) / c->hop;
        MIS_REQUIRE(T < (1 << 30), MIS_ERR_INVALID_INPUT, "row %d: too many frames", b);
        if (frames) frames[b] = (int32_t)T;
        if (rows) rows[b] = fv_rows_of(c, (int)T);
    }
    MIS_API_END
}

static void fv_launch_gemm(mis_fsmn_vad* c, FvGemm g, const FvGeom& geo, int B) {
    g.g = geo;
    if (g.epi == FV_EPI_SOFTMAX) hipLaunchKernelGGL((k_fvad_gemm<1, 2>), dim3(cdiv(geo.nr, 32), 1, B), dim3(256), 0, c->stream, g);
    else hipLaunchKernelGGL((k_fvad_gemm<2, 1>), dim3(cdiv(geo.nr, 64), cdiv(g.Cout, 64), B), dim3(256), 0, c->stream, g);
}
static FvGemm fv_lin_gemm(const FvLin& l, const float* X, float* Y, int epi) {
    FvGemm g{};
    g.X = X; g.ldx = l.cin; g.W = l.w; g.bias = l.b; g.Y = Y; g.ldy = l.cout; g.Cin = l.cin; g.Cout = l.cout; g.epi = epi; g.load = FV_LOAD_ACT;
    return g;
}
static FvLfr fv_lfr(const mis_fsmn_vad* c) { return FvLfr{c->fbank, c->shift, c->scale, c->nm, c->m, c->n, c->lp}; }

// the encoder over one chunk: from the fbank (from_fbank) or from c->feat.  Returns the launches made.
static int fv_enqueue_encoder(mis_fsmn_vad* c, const FvGeom& geo, int B, bool from_fbank) {
    FvGemm g = fv_lin_gemm(c->in1, c->feat, c->a1, FV_EPI_PLAIN);
    if (from_fbank) { g.load = FV_LOAD_LFR; g.lfr = fv_lfr(c); }
    fv_launch_gemm(c, g, geo, B);
    fv_launch_gemm(c, fv_lin_gemm(c->in2, c->a1, c->h0, FV_EPI_RELU), geo, B);
    const float* h = c->h0;
    for (int i = 0; i < c->NL; ++i) {
        fv_launch_gemm(c, fv_lin_gemm(c->layers[i].linear, h, c->pbuf[i], FV_EPI_PLAIN), geo, B);
        FvGemm ga = fv_lin_gemm(c->layers[i].affine, c->pbuf[i], c->hbuf[i], FV_EPI_RELU);
        ga.load = FV_LOAD_MEM; ga.dw = c->layers[i].dw; ga.lorder = c->L;
        fv_launch_gemm(c, ga, geo, B);
        h = c->hbuf[i];
    }
    fv_launch_gemm(c, fv_lin_gemm(c->out1, h, c->ao, FV_EPI_PLAIN), geo, B);
    FvGemm gs = fv_lin_gemm(c->out2, c->ao, c->scores, FV_EPI_SOFTMAX);
    gs.sil = c->sil; gs.sil_ids = c->sil_ids; gs.n_sil = c->cfg.n_sil;
    fv_launch_gemm(c, gs, geo, B);
    return 4 + 2 * c->NL;
}

enum { FV_WANT_FEATURES = 0, FV_WANT_SCORES = 1, FV_WANT_RAW = 2 };

// The one driver.  Source: pcm [B][stride] (h_T / h_R set from the lens) or features [B][Rs][D] (h_R set).  Walks the LFR rows in chunks,
// copies each chunk's results into the caller's arrays ([B][Rs][.] / [B][Ts]) and synchronises once, at the end.
static void fv_run(mis_fsmn_vad* c, int want, const float* pcm, int64_t stride, const float* feats, int B, int Tmax, int Rs, int Ts,
                   float* out_a, float* out_dec) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int Rmax = 0;
    for (int b = 0; b < B; ++b) Rmax = std::max(Rmax, c->h_R[b]);
    c->last_launches = 0; c->ms_front = c->ms_model = 0.0f;
    if (Rmax == 0) { c->last_batch = 0; return; }
    HIP_CHECK(hipMemcpyAsync(c->counts.p, c->h_T.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->counts.p + FV_MAX_BATCH, c->h_R.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    const int chunk = c->cfg.chunk_frames, halo = want == FV_WANT_FEATURES ? 0 : c->halo;
    int launches = 0, chunks = 0;
    FvGeom geo{c->counts.p, c->counts.p + FV_MAX_BATCH, 0, 0, 0, 0, 0};
    for (int r0 = 0; r0 < Rmax; r0 += chunk, ++chunks) {
        const int r1 = std::min(Rmax, r0 + chunk), g0 = std::max(0, r0 - halo), nr = r1 - g0;
        geo.g0 = g0; geo.r1 = r1; geo.nr = nr;
        const bool timed = chunks < FV_TIMED_CHUNKS;
        if (timed) HIP_CHECK(hipEventRecord(c->ev[3 * chunks], s));
        if (pcm) {
            const int64_t fa = std::max<int64_t>(0, (int64_t)g0 * c->n - c->lp), fb = std::min<int64_t>(Tmax, (int64_t)(r1 - 1) * c->n + c->m - c->lp);
            MIS_REQUIRE(fb > fa && fb - fa <= c->Fc && nr <= c->Rc, MIS_ERR_GENERATION_FAILED, "chunk geometry outside the workspace");
            geo.fa = (int)fa; geo.nf = (int)(fb - fa);
            const int64_t s0 = fa * c->hop, ns = (int64_t)(geo.nf - 1) * c->hop + c->wlen;
            MIS_REQUIRE(ns <= c->Sc && s0 + ns <= stride, MIS_ERR_GENERATION_FAILED, "chunk samples outside the workspace");
            HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, (size_t)ns * 4, pcm + s0, (size_t)stride * 4, (size_t)ns * 4, B, hipMemcpyHostToDevice, s));
            FvFront fp{c->pcm.p, ns, c->win, c->twc, c->tws, c->fb, c->fbr, c->fbank, c->dec, geo, c->wlen, c->hop, c->nm, (float)log((double)1e-8f)};
            hipLaunchKernelGGL(k_fvad_fbank, dim3(geo.nf, B), dim3(256), 0, s, fp);
            ++launches;
            if (want == FV_WANT_RAW && out_dec)
                HIP_CHECK(hipMemcpy2DAsync(out_dec + fa, (size_t)Ts * 4, c->dec, (size_t)geo.nf * 4, (size_t)geo.nf * 4, B, hipMemcpyDeviceToHost, s));
        } else {
            geo.fa = 0; geo.nf = 0;
            MIS_REQUIRE(nr <= c->Rc, MIS_ERR_GENERATION_FAILED, "chunk geometry outside the workspace");
            HIP_CHECK(hipMemcpy2DAsync(c->feat, (size_t)nr * c->D * 4, feats + (size_t)g0 * c->D, (size_t)Rs * c->D * 4, (size_t)nr * c->D * 4, B,
                                       hipMemcpyHostToDevice, s));
        }
        if (timed) HIP_CHECK(hipEventRecord(c->ev[3 * chunks + 1], s));
        const size_t keep = (size_t)(r1 - r0), skip = (size_t)(r0 - g0);
        if (want == FV_WANT_FEATURES) {
            const size_t total = (size_t)B * nr * c->D;
            hipLaunchKernelGGL(k_fvad_lfr, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, fv_lfr(c), geo, c->feat, c->D, total);
            ++launches;
            HIP_CHECK(hipMemcpy2DAsync(out_a + (size_t)r0 * c->D, (size_t)Rs * c->D * 4, c->feat, (size_t)nr * c->D * 4, keep * c->D * 4, B,
                                       hipMemcpyDeviceToHost, s));
        } else {
            launches += fv_enqueue_encoder(c, geo, B, pcm != nullptr);
            if (want == FV_WANT_SCORES)
                HIP_CHECK(hipMemcpy2DAsync(out_a + (size_t)r0 * c->O, (size_t)Rs * c->O * 4, c->scores + skip * c->O, (size_t)nr * c->O * 4,
                                           keep * c->O * 4, B, hipMemcpyDeviceToHost, s));
            else
                HIP_CHECK(hipMemcpy2DAsync(out_a + r0, (size_t)Rs * 4, c->sil + skip, (size_t)nr * 4, keep * 4, B, hipMemcpyDeviceToHost, s));
        }
        if (timed) HIP_CHECK(hipEventRecord(c->ev[3 * chunks + 2], s));
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                               // the one synchronisation of a call
    for (int i = 0; i < std::min(chunks, FV_TIMED_CHUNKS); ++i) {
        float a = 0.0f, b = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&a, c->ev[3 * i], c->ev[3 * i + 1]));
        HIP_CHECK(hipEventElapsedTime(&b, c->ev[3 * i + 1], c->ev[3 * i + 2]));
        c->ms_front += a; c->ms_model += b;
    }
    c->last = geo; c->last_batch = B; c->last_launches = launches; c->last_front = pcm != nullptr;
}

// lens -> h_T / h_R; returns the longest row's frames
static int fv_take_lens(mis_fsmn_vad* c, const float* pcm, const int64_t* lens, int batch, int64_t stride) {
    MIS_REQUIRE(c && pcm, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "FSMN VAD model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    int Tmax = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples, the row stride is %lld", b, (long long)n, (long long)stride);
        const int64_t T = n < c->wlen ? 0 : 1 + (n - c->wlen) / c->hop;
        MIS_REQUIRE(T < (1 << 30), MIS_ERR_INVALID_INPUT, "row %d: too many frames", b);
        c->h_T[b] = (int32_t)T; c->h_R[b] = fv_rows_of(c, (int)T);
        Tmax = std::max(Tmax, (int)T);
    }
    return Tmax;
}

// pcm f32 [batch, stride] -> features [batch, rows, input_dim], rows >= the longest row's LFR rows; zeros behind a row's own
extern "C" mis_status mis_fsmn_vad_features(mis_fsmn_vad* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* features,
                                            int rows) {
    MIS_API_BEGIN
    const int Tmax = fv_take_lens(c, pcm, lens, batch, stride);
    MIS_REQUIRE(features && rows >= fv_rows_of(c, Tmax), MIS_ERR_INVALID_INPUT, "features: room for %d rows, %d are needed", rows, fv_rows_of(c, Tmax));
    fv_run(c, FV_WANT_FEATURES, pcm, stride, nullptr, batch, Tmax, rows, 0, features, nullptr);
    MIS_API_END
}

extern "C" mis_status mis_fsmn_vad_forward(mis_fsmn_vad* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* scores,
                                           int rows) {
    MIS_API_BEGIN
    const int Tmax = fv_take_lens(c, pcm, lens, batch, stride);
    MIS_REQUIRE(scores && rows >= fv_rows_of(c, Tmax), MIS_ERR_INVALID_INPUT, "scores: room for %d rows, %d are needed", rows, fv_rows_of(c, Tmax));
    fv_run(c, FV_WANT_SCORES, pcm, stride, nullptr, batch, Tmax, rows, 0, scores, nullptr);
    MIS_API_END
}

extern "C" mis_status mis_fsmn_vad_detect_raw(mis_fsmn_vad* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* silence,
                                              int rows, float* decibel, int frames) {
    MIS_API_BEGIN
    const int Tmax = fv_take_lens(c, pcm, lens, batch, stride);
    MIS_REQUIRE(silence && decibel && rows >= fv_rows_of(c, Tmax) && frames >= Tmax, MIS_ERR_INVALID_INPUT,
                "detect_raw: room for %d rows / %d frames, %d / %d are needed", rows, frames, fv_rows_of(c, Tmax), Tmax);
    fv_run(c, FV_WANT_RAW, pcm, stride, nullptr, batch, Tmax, rows, frames, silence, decibel);
    MIS_API_END
}

// features f32 [batch, rows, input_dim] with counts[batch] valid rows each (NULL = rows) -> scores [batch, rows, output_dim]
extern "C" mis_status mis_fsmn_vad_forward_features(mis_fsmn_vad* c, const float* features, const int32_t* counts, int batch, int rows,
                                                    float* scores) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && features && scores, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "FSMN VAD model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(rows >= 1 && rows < (1 << 30), MIS_ERR_INVALID_INPUT, "bad row count");
    for (int b = 0; b < batch; ++b) {
        const int r = counts ? counts[b] : rows;
        MIS_REQUIRE(r >= 0 && r <= rows, MIS_ERR_INVALID_INPUT, "row %d: %d feature rows (0 .. %d are served)", b, r, rows);
        c->h_T[b] = 0; c->h_R[b] = r;
    }
    fv_run(c, FV_WANT_SCORES, nullptr, 0, features, batch, 0, rows, 0, scores, nullptr);
    MIS_API_END
}

// tensors of the last chunk of the last call, f32, a row's own rows first and zeros behind them.  stage 0 fbank [B, F, n_mels], 1 decibel
// [B, F, 1], 2 LFR + CMVN features [B, R, input_dim] (formed here from the fbank after a pcm call), 3 in_linear1, 4 in_linear2, 5 + 2 i
// layer i's projection, 6 + 2 i its output, 5 + 2 L out_linear1, 6 + 2 L scores, 7 + 2 L the silence sum [B, R, 1].
extern "C" mis_status mis_fsmn_vad_tap(mis_fsmn_vad* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && stage >= 0 && stage <= 7 + 2 * c->NL, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(c->last_batch > 0, MIS_ERR_INVALID_INPUT, "no call to tap");
    MIS_REQUIRE(stage >= 2 || c->last_front, MIS_ERR_INVALID_INPUT, "the last call had no front end");
    HIP_CHECK(hipSetDevice(c->device));
    const int NL = c->NL;
    const size_t B = c->last_batch, n = stage <= 1 ? c->last.nf : c->last.nr;
    const float* src; size_t width;
    if (stage == 0) { src = c->fbank; width = c->nm; }
    else if (stage == 1) { src = c->dec; width = 1; }
    else if (stage == 2) { src = c->feat; width = c->D; }
    else if (stage == 3) { src = c->a1; width = c->A; }
    else if (stage == 4) { src = c->h0; width = c->Ld; }
    else if (stage < 5 + 2 * NL) { const int i = (stage - 5) / 2; const bool pr = ((stage - 5) & 1) == 0; src = pr ? c->pbuf[i] : c->hbuf[i]; width = pr ? c->P : c->Ld; }
    else if (stage == 5 + 2 * NL) { src = c->ao; width = c->Ao; }
    else if (stage == 6 + 2 * NL) { src = c->scores; width = c->O; }
    else { src = c->sil; width = 1; }
    if (dims) { dims[0] = (int64_t)B; dims[1] = (int64_t)n; dims[2] = (int64_t)width; }
    if (!out) return MIS_OK;
    MIS_REQUIRE((int64_t)(B * n * width) <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    if (stage == 2 && c->last_front) {
        const size_t total = B * n * width;
        hipLaunchKernelGGL(k_fvad_lfr, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, fv_lfr(c), c->last, c->feat, c->D, total);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    HIP_CHECK(hipMemcpy(out, src, B * n * width * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// measurements: device milliseconds of the last call summed over its first 128 chunks, ms[2] = front end (copy in + fbank), encoder
extern "C" mis_status mis_debug_fsmn_vad_timing(const mis_fsmn_vad* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && ms, MIS_ERR_INVALID_INPUT, "null argument");
    ms[0] = c->ms_front; ms[1] = c->ms_model;
    MIS_API_END
}
