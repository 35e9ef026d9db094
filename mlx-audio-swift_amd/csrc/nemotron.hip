// nemotron.hip - Nemotron ASR (cache-aware FastConformer + RNN-T), offline: 16 kHz samples -> NeMo log-mel -> CAUSAL depthwise-striding
// Conv2d stem (factor 8, pad (2, 1) on both axes) -> FastConformer blocks with CHUNKED-LIMITED relative-position attention and a conv
// module normalised by a LayerNorm over channels -> prompt conditioning -> joint.enc over every frame -> greedy RNN-T decode (embedding,
// one or two LSTM layers, joint, arg-max) in ONE launch.  Exact f32 throughout; mis_nemotron_set_encoder_dtype(MIS_BF16) before finalize
// selects the bf16 form of the Conformer blocks (nemotron_encoder_bf16.h holds its kernels and its precision contract).
//
// Reference being replaced: NemotronASRModel.decode / applyPrompt (Sources/MLXAudioSTT/Models/NemotronASR/NemotronASRModel.swift :184-275),
// NemotronASRAttentionMask, NemotronASRConvolution, NemotronASRCausalDwStridingSubsampling (NemotronASRConformer.swift),
// NemoDecodingLogic.rnntStep (Nemo/NemoDecodingLogic.swift:23-39), NemoRelPositionMultiHeadAttention (Nemo/NemoAttention.swift).
//
// The front end is audio_front.h's; the contraction, the frame statistics, LayerNorm and the intake are sortformer_kernels.h's, unchanged:
// the three operand loads this engine adds to the contraction are explicit specialisations of sf_load made in nemotron_kernels.h (shared
// with the stream session, nemotron_stream.hip, together with the stem's first conv, the parameter blocks and the handle), so that header and the
// code objects of the other engines keep their bits.  Every kernel takes the row's own counts (a row's bits do not depend on its batch).
// New kernels (resources off -Rpass-analysis=kernel-resource-usage, gfx950):
//
//   k_nm_attn   k_pk_attn's wave split (64 queries x head x row per block, four waves: wave = qh + 2 dh owns 32 queries and 64 head
//               dimensions; partial scores exchanged through LDS and added in one fixed order) under the chunked-limited rule: query q
//               sees key k iff 0 <= q / C - k / C <= L.  (a) the block walks only the 32-key tiles that intersect
//               [(q0 / C - L) C, (q_last / C + 1) C) and [0, n): tiles outside are never loaded; (b) inside a tile the rule is two
//               compares per (query, key) against the lane's own [lo, hi), made once; an excluded key has weight exactly 0, as the
//               reference's additive -1e9 gives in f32 (a query always sees its own chunk); a query that sees nothing of a tile keeps
//               m = -inf, and the rescale guards that case; (c) only the distances -(C - 1) .. L C + C - 1 occur: the projected
//               table holds those rows alone (row = distance + poff) and band rows outside them are staged as zeros, never read.
//               LDS 67072 bytes (two blocks a CU), 234 VGPRs, 0 AGPRs, scratch 0, 2 waves a SIMD.
//               (k_nm_glu_dwconv_ln: LDS 11776, 45 VGPRs, scratch 0; k_nm_rnnt: LDS 45188, 69 VGPRs, scratch 0; the DWC / LN_SILU /
//               PROMPT instantiations of k_sf_gemm: 239 / 85 / 62 VGPRs + 16 AGPRs, scratch 0.)
//   k_nm_glu_dwconv_ln   GLU -> depthwise conv with (padLeft, k - 1 - padLeft) zero frames -> the frame's LayerNorm statistics over ALL
//               channels, one launch.  A block owns 16 frames of one row across every channel, 64 channels at a time (tile + halo of
//               gated frames in LDS; a wave is 4 frames, a lane a channel); the sums run lane-strided over the channels and meet in
//               wave_sum's fixed order, two passes (the second re-reads the thread's own outputs), as wave_mean_rstd does.  LayerNorm's
//               affine and SiLU are pointwise_conv2's operand load (NM_LOAD_LN_SILU): the block stays at 15 launches.
//   k_nm_conv0 / NM_LOAD_DWC   the stem's first conv and the depthwise operand load with pad (2, 1): taps at 2 t + i - 2, 2 f + j - 2.
//   k_nm_rnnt   the whole greedy RNN-T loop of one row in one block of 1024 threads, k_pk_tdt's layout (a thread owns the four gates of a
//               unit, transposed Wx / Wh, one logit a thread, fixed-order arg-max with ties to the lower index), no duration head,
//               rnntStep's advance.  The LSTM and joint.pred run once per EMISSION.  Static bound T max_symbols + T (no max_symbols:
//               T + cap + 1); stops with a flag at the output capacity.
//   NM_LOAD_PROMPT   linear0([x, onehot(p)]) without the concatenation: the operand load yields x for k < d and (k - d == p_b) behind it.
//
// Launches: generate = 2 (front end) + 4 (stem) + 1 (intake) + 15 L + 2 (prompt kernel, if the model has one) + 1 (joint.enc) + 1 (decode).
#include "nemotron_kernels.h"
#include "nemotron_encoder_bf16.h"
#include "nemotron_stream_bf16.h"                                  // the short-pass contraction: a rule of mis_debug_nemotron_gemm_bf16


// ============================================================================ kernel B: chunked-limited attention, head sizes 65..128
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_nm_attn(NmAttn p) {
    __shared__ float Ks[32][NM_LDP];
    __shared__ float Pb[96 * NM_LDP];                               // the band; between uses: Q tile, exchanged partials, output tile
    __shared__ float Ub[2][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5, qh = wave & 1, dh = wave >> 1;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64, n = min(p.cnt[b], p.Tp), hd = p.hd;
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = tid; i < 64 * hd; i += 256) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0.0f;
        }
        return;
    }
#pragma unroll 4
    for (int i = tid; i < 64 * 128; i += 256) {
        const int r = i >> 7, c = i & 127, tq = q0 + r;
        Pb[r * NM_LDP + c] = (tq < n && c < hd) ? p.qkv[(rowbase + tq) * p.ld + h * hd + c] * p.qscale : 0.0f;
    }
    {
        const int c = tid & 127;
        Ub[tid >> 7][c] = c < hd ? (tid < 128 ? p.u : p.v)[h * hd + c] : 0.0f;
    }
    __syncthreads();
    const int wq = qh * 32, d0 = dh * 64;
    float qf[32];                                                   // the wave's 64 dimensions of query wq + l31; u and v are added at use (LDS)
#pragma unroll
    for (int i = 0; i < 32; ++i) qf[i] = Pb[(wq + l31) * NM_LDP + d0 + 2 * i + kh];
    f32x16_t O[2];
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dn][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float* Bd0 = Pb + qh * 2048;                              // band products [64 band rows][32 queries] of dh 0, dh 1
    const float* Bd1 = Pb + (qh + 2) * 2048;
    const float* Sx0 = Pb + 8192 + qh * 1024;                       // content scores [32 keys][32 queries] of dh 0, dh 1
    const float* Sx1 = Pb + 8192 + (qh + 2) * 1024;
    // the rule: the lane's query sees the keys [vlo, vhi); the block walks the tiles that the first and the last live query of it see
    const int qc = (q0 + wq + l31) / p.C, vlo = max(qc - p.L, 0) * p.C, vhi = (qc + 1) * p.C;
    const int wlo = (max(q0 / p.C - p.L, 0) * p.C) & ~31, whi = min(n, (min(q0 + 63, n - 1) / p.C + 1) * p.C);
    for (int kb = wlo; kb < whi; kb += 32) {
        __syncthreads();                                            // the previous tile's reads are done (first pass: the Q fragments are taken)
#pragma unroll 4
        for (int i = tid; i < 32 * 128; i += 256) {
            const int r = i >> 7, c = i & 127, key = kb + r;
            Ks[r][c] = (key < n && c < hd) ? p.qkv[(rowbase + key) * p.ld + p.koff + h * hd + c] : 0.0f;
        }
        const int base = q0 - kb - 31;                              // distance of band row 0
#pragma unroll 4
        for (int i = tid; i < 96 * 128; i += 256) {
            const int r = i >> 7, c = i & 127, dist = base + r;
            Pb[r * NM_LDP + c] = (dist >= p.dlo && dist <= p.dhi && c < hd) ? p.P[(size_t)(dist + p.poff) * p.ldp + h * hd + c] : 0.0f;
        }
        __syncthreads();
        // partial S^T[key][query] and partial band products over the wave's 64 dimensions
        f32x16_t S, G0, G1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = 0.0f; G0[r] = 0.0f; G1[r] = 0.0f; }
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int k = d0 + 2 * i + kh;
            const float qu = qf[i] + Ub[0][k], qv = qf[i] + Ub[1][k];
            S = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31][k], qu, S, 0, 0, 0);
            G0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(wq + l31) * NM_LDP + k], qv, G0, 0, 0, 0);
            G1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(wq + 32 + l31) * NM_LDP + k], qv, G1, 0, 0, 0);
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // keep the operand loads of at most four steps in flight (registers)
        }
        __syncthreads();                                            // every wave has read its band rows: the space becomes the partials'
        {
            float* Bd = Pb + wave * 2048;
            float* Sx = Pb + 8192 + wave * 1024;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int br = f32_tile_row(r, kh);
                Bd[br * 32 + l31] = G0[r];
                Bd[(br + 32) * 32 + l31] = G1[r];
                Sx[br * 32 + l31] = S[r];
            }
        }
        __syncthreads();
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = f32_tile_row(r, kh), at = (l31 - j + 31) * 32 + l31, key = kb + j;   // distance i - j, the literal rel-shift's entry
            const float s = (Sx0[j * 32 + l31] + Sx1[j * 32 + l31]) + (Bd0[at] + Bd1[at]);
            S[r] = (key < n && key >= vlo && key < vhi) ? s / p.sdk : -INFINITY;
            mx = fmaxf(mx, S[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.0f : m_new;      // the query has seen no key yet: every weight below is exp(-inf) = 0
        const float alpha = expf(m_run - m_use);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = expf(S[r] - m_use); psum += S[r]; }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int dn = 0; dn < 2; ++dn) {
#pragma unroll
            for (int r = 0; r < 16; ++r) O[dn][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {                          // V^T straight from memory: 32 consecutive floats of key f32_tile_row(r, kh)
                const int key = kb + f32_tile_row(r, kh), d = d0 + dn * 32 + l31;
                const float vv = (key < n && d < hd) ? p.qkv[(rowbase + key) * p.ld + p.voff + h * hd + d] : 0.0f;
                O[dn] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, S[r], O[dn], 0, 0, 0);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);         // > 0 for a live query: it sees itself
    __syncthreads();                                                // the band space is free: the outputs go through it for coalesced stores
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) Pb[(wq + l31) * NM_LDP + d0 + dn * 32 + f32_tile_row(r, kh)] = O[dn][r] / l_tot;
    __syncthreads();
    for (int i = tid; i < 64 * hd; i += 256) {
        const int r = i / hd, c = i - r * hd, t = q0 + r;
        if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + c] = t < n ? Pb[r * NM_LDP + c] : 0.0f;
    }
}

template <class Ctx>
static void nm_attn(Ctx* c, const NmAttn& p, int heads, int batch) {
    MIS_LAUNCH(c, k_nm_attn, dim3(cdiv(p.Tp, 64), heads, batch), dim3(256), p);
}

// ============================================================================ kernel C: GLU + depthwise conv + LayerNorm statistics
// pw [M][2 C] (pointwise_conv1) -> out [M][C] and stats [M][2] = mean, rstd over the C channels of a frame: g = a sigmoid(b), padl zero
// frames before the row and zeros from its count on, taps [k][C], bias [C] or null.  Frames behind the count: zeros, stats 0, 0.
__global__ void __launch_bounds__(256) k_nm_glu_dwconv_ln(const float* __restrict__ pw, const float* __restrict__ taps, const float* __restrict__ bias,
                                                          const int* __restrict__ cnt, float* out, float* __restrict__ stats, int Tp, int C, int k,
                                                          int padl, float eps) {
    __shared__ float g[NM_DW_TT + SF_DW_MAXK - 1][64];
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6, b = blockIdx.y, t0 = blockIdx.x * NM_DW_TT, tw = t0 + tl * 4;
    const int n = min(cnt[b], Tp);
    const size_t rowbase = (size_t)b * Tp;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int ch = c0 + cl;
        const bool live = ch < C;
        __syncthreads();                                            // the previous 64 channels are read
        for (int r = tl; r < NM_DW_TT + k - 1; r += 4) {
            const int t = t0 - padl + r;
            float v = 0.0f;
            if (live && t >= 0 && t < n) {
                const float* row = pw + (rowbase + t) * 2 * C;
                v = row[ch] * (1.0f / (1.0f + expf(-row[C + ch])));
            }
            g[r][cl] = v;
        }
        __syncthreads();
        if (!live) continue;                                        // (the barriers above are reached: the loop bound is uniform)
        float acc[4];
        const float bv = bias ? bias[ch] : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = bv;
        for (int kk = 0; kk < k; ++kk) {
            const float w = taps[(size_t)kk * C + ch];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(w, g[tl * 4 + i + kk][cl], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = tw + i;
            if (t >= Tp) continue;
            const float v = t < n ? acc[i] : 0.0f;
            out[(rowbase + t) * C + ch] = v;
            s[i] += v;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                   // the wave's four frames: the lanes hold the channels cl, cl + 64, ..
        const int t = tw + i;
        const float mean = wave_sum(s[i]) / (float)C;
        float q = 0.0f;
        if (t < n)
            for (int ch = cl; ch < C; ch += 64) { const float v = out[(rowbase + t) * C + ch] - mean; q = fmaf(v, v, q); }   // the thread's own stores
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
        if (cl == 0 && t < Tp) { stats[2 * (rowbase + t)] = t < n ? mean : 0.0f; stats[2 * (rowbase + t) + 1] = t < n ? rstd : 0.0f; }
    }
}

template <class Ctx>
static void nm_glu_dwconv_ln(Ctx* c, const float* pw, const float* taps, const float* bias, const int* cnt, float* out, float* stats, int Tp, int C,
                             int k, int padl, int batch) {
    MIS_LAUNCH(c, k_nm_glu_dwconv_ln, dim3(cdiv(Tp, NM_DW_TT), batch), dim3(256), pw, taps, bias, cnt, out, stats, Tp, C, k, padl, 1e-5f);
}

// ============================================================================ kernel D: greedy RNN-T decode, one block a row
__global__ void __launch_bounds__(NM_NT) k_nm_rnnt(NmRnnt p) {
    __shared__ float xs[NM_MAXW], hs[2][NM_MAXW], cs[2][NM_MAXW], hn[2][NM_MAXW], cn[2][NM_MAXW], pp[NM_MAXW], zs[NM_MAXW];
    __shared__ float rv[NM_NT / 64];
    __shared__ int ri[NM_NT / 64], dec;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, P = p.P, J = p.J, V = p.V, blank = p.V - 1, top = p.layers - 1;
    const int T = min(p.cnt[b], p.Tp);
    for (int u = tid; u < P; u += NM_NT) { hs[0][u] = 0.0f; hs[1][u] = 0.0f; cs[0][u] = 0.0f; cs[1][u] = 0.0f; }
    // the proposal behind `token` from the committed state: hn, cn and pp = joint.pred(h' of the top layer); a blank feeds zeros (blank_as_pad)
    auto predict = [&](int token) {
        for (int u = tid; u < P; u += NM_NT) xs[u] = token == blank ? 0.0f : p.embed[(size_t)token * P + u];
        __syncthreads();
        nm_lstm_layer(p.wxT[0], p.whT[0], p.bih[0], p.bhh[0], xs, hs[0], cs[0], hn[0], cn[0], P);
        if (top == 1) nm_lstm_layer(p.wxT[1], p.whT[1], p.bih[1], p.bhh[1], hn[0], hs[1], cs[1], hn[1], cn[1], P);
        for (int j = tid; j < J; j += NM_NT) {
            float acc = p.bp[j];
            for (int k = 0; k < P; ++k) acc = fmaf(p.wpT[(size_t)k * J + j], hn[top][k], acc);
            pp[j] = acc;
        }
        __syncthreads();
    };
    predict(blank);
    int t = 0, ns = 0, n = 0, steps = 0, flagged = 0;
    const int bound = p.max_symbols > 0 ? T * p.max_symbols + T : T + p.cap + 1;   // a step emits or advances
    int* otok = p.tokens + (size_t)b * p.cap;
    int* ofrm = p.frames + (size_t)b * p.cap;
    for (int it = 0; it < bound && t < T; ++it) {                   // (every branch below is uniform over the block)
        const float* e = p.encp + ((size_t)b * p.Tp + t) * J;
        for (int j = tid; j < J; j += NM_NT) zs[j] = fmaxf(e[j] + pp[j], 0.0f);
        __syncthreads();
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = tid; v < V; v += NM_NT) {
            float acc = p.bo[v];
            for (int j = 0; j < J; ++j) acc = fmaf(p.woT[(size_t)j * V + v], zs[j], acc);
            if (nm_better(acc, v, bv, bi)) { bv = acc; bi = v; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (nm_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < NM_NT / 64; ++w)
                if (nm_better(rv[w], ri[w], bv, bi)) { bv = rv[w]; bi = ri[w]; }
            dec = bi < V ? bi : 0;                                  // (no finite logit at all: index 0)
        }
        __syncthreads();
        const int tok = dec;
        ++steps;
        // NemoDecodingLogic.rnntStep
        if (tok == blank) { t += 1; ns = 0; continue; }
        if (n >= p.cap) { flagged = 1; break; }
        if (tid == 0) { otok[n] = tok; ofrm[n] = t; }
        ++n;
        for (int u = tid; u < P; u += NM_NT) { hs[0][u] = hn[0][u]; hs[1][u] = hn[1][u]; cs[0][u] = cn[0][u]; cs[1][u] = cn[1][u]; }
        __syncthreads();
        predict(tok);
        ++ns;
        if (p.max_symbols > 0 && ns >= p.max_symbols) { t += 1; ns = 0; }
    }
    if (tid == 0) { p.count[b] = n; p.flag[b] = flagged; p.steps[b] = steps; }
}

// ============================================================================ host
extern "C" mis_status mis_nemotron_create(const mis_nemotron_config* cfg, int device, mis_nemotron** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    const int d = cfg->hidden_size, H = cfg->num_attention_heads, ck = cfg->conv_kernel_size;
    MIS_REQUIRE(cfg->sampling_rate == 16000 && cfg->n_fft == NEMO_NFFT && cfg->hop_length == NEMO_HOP && cfg->win_length == NEMO_WIN, MIS_ERR_INVALID_INPUT,
                "sampling_rate / n_fft / hop_length / win_length: only 16000 / 512 / 160 / 400 are implemented");
    MIS_REQUIRE(cfg->preemphasis >= 0.0f && cfg->preemphasis <= 1.0f, MIS_ERR_INVALID_INPUT, "preemphasis outside 0..1");
    MIS_REQUIRE(cfg->num_mel_bins >= 8 && cfg->num_mel_bins <= 256, MIS_ERR_INVALID_INPUT, "num_mel_bins %d outside 8..256", cfg->num_mel_bins);
    MIS_REQUIRE(cfg->subsampling_factor == 8, MIS_ERR_INVALID_INPUT, "subsampling_factor %d: only 8 is implemented", cfg->subsampling_factor);
    MIS_REQUIRE(cfg->subsampling_conv_channels >= 1 && cfg->subsampling_conv_channels <= 1024, MIS_ERR_INVALID_INPUT,
                "subsampling_conv_channels %d outside 1..1024", cfg->subsampling_conv_channels);
    MIS_REQUIRE(d >= 8 && d <= 4096, MIS_ERR_INVALID_INPUT, "hidden_size %d outside 8..4096", d);
    MIS_REQUIRE(H >= 1 && d % H == 0 && d / H >= 65 && d / H <= 128, MIS_ERR_INVALID_INPUT,
                "num_attention_heads %d: head size hidden_size / num_attention_heads must be a whole number of 65..128", H);
    MIS_REQUIRE(cfg->intermediate_size >= 1 && cfg->intermediate_size <= 16384, MIS_ERR_INVALID_INPUT, "intermediate_size %d outside 1..16384",
                cfg->intermediate_size);
    MIS_REQUIRE(cfg->num_hidden_layers >= 1 && cfg->num_hidden_layers <= 64, MIS_ERR_INVALID_INPUT, "num_hidden_layers %d outside 1..64", cfg->num_hidden_layers);
    MIS_REQUIRE(ck >= 2 && ck <= SF_DW_MAXK, MIS_ERR_INVALID_INPUT, "conv_kernel_size %d outside 2..%d", ck, SF_DW_MAXK);
    MIS_REQUIRE(cfg->conv_pad_left >= 0 && cfg->conv_pad_right >= 0 && cfg->conv_pad_left + cfg->conv_pad_right == ck - 1, MIS_ERR_INVALID_INPUT,
                "conv_context_size (%d, %d): the pads must be >= 0 and add up to conv_kernel_size - 1", cfg->conv_pad_left, cfg->conv_pad_right);
    MIS_REQUIRE(cfg->num_contexts >= 1 && cfg->num_contexts <= NM_MAX_CONTEXTS, MIS_ERR_INVALID_INPUT, "att_context_size: %d pairs outside 1..%d",
                cfg->num_contexts, NM_MAX_CONTEXTS);
    for (int i = 0; i < cfg->num_contexts; ++i)
        MIS_REQUIRE(cfg->att_context[i][1] >= 0, MIS_ERR_INVALID_INPUT, "att_context_size[%d]: right context %d below 0", i, cfg->att_context[i][1]);
    MIS_REQUIRE((cfg->prompt_hidden == 0 && cfg->num_prompts == 0) || (cfg->prompt_hidden >= 1 && cfg->prompt_hidden <= 16384 && cfg->num_prompts >= 1 &&
                 cfg->num_prompts <= 4096), MIS_ERR_INVALID_INPUT, "prompt_hidden %d / num_prompts %d outside 1..16384 / 1..4096 (0 / 0: no prompt kernel)",
                cfg->prompt_hidden, cfg->num_prompts);
    nm_check_decoder_dims(cfg->pred_rnn_layers, cfg->pred_hidden, cfg->joint_hidden, cfg->vocab_size, cfg->max_symbols);
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= NM_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch %d outside 1..%d", cfg->max_batch, NM_MAX_BATCH);
    MIS_REQUIRE(cfg->max_seconds >= 1 && cfg->max_seconds <= NM_MAX_SECONDS, MIS_ERR_INVALID_INPUT, "max_seconds %d outside 1..%d", cfg->max_seconds,
                NM_MAX_SECONDS);
    MIS_REQUIRE(cfg->max_tokens >= 1 && cfg->max_tokens <= 65536, MIS_ERR_INVALID_INPUT, "max_tokens %d outside 1..65536", cfg->max_tokens);
    hipStream_t stream = mis_open_stream(device);      // first: the handle's events belong to this device
    auto c = std::make_unique<mis_nemotron>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->mels = cfg->num_mel_bins; c->C = cfg->subsampling_conv_channels; c->d = d; c->H = H; c->hd = d / H; c->f = cfg->intermediate_size;
    c->L = cfg->num_hidden_layers; c->ck = ck; c->padl = cfg->conv_pad_left;
    c->F1 = nm_half(c->mels); c->F2 = nm_half(c->F1); c->F3 = nm_half(c->F2);
    c->P = cfg->pred_hidden; c->J = cfg->joint_hidden; c->V = cfg->vocab_size + 1; c->cap = cfg->max_tokens;
    c->NP = cfg->num_prompts; c->PH = cfg->prompt_hidden;
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_nemotron_destroy(mis_nemotron* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}

extern "C" mis_status mis_nemotron_set_encoder_dtype(mis_nemotron* c, mis_dtype dtype) {
    MIS_API_BEGIN
    pk_set_encoder_dtype(c, dtype);
    MIS_API_END
}

extern "C" mis_status mis_nemotron_set_tensor(mis_nemotron* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 4, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

static const char* const NM_LSTM = "decoder.prediction.dec_rnn.lstm.";

extern "C" mis_status mis_nemotron_finalize(mis_nemotron* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t mels = c->mels, C = c->C, d = c->d, f = c->f, ck = c->ck, F3 = c->F3, H = c->H, hd = c->hd, P = c->P, J = c->J, V = c->V, NP = c->NP, PH = c->PH;
    const bool ab = c->cfg.attention_bias != 0;
    // bf16 mode: the eight block matrices go to wm and relative_k_proj and the sinusoid table to wt, for nm_bf16_tables alone
    const bool b16 = c->enc_bf16 != 0;
    HostArena a(c->raw), wm(c->raw), wt(c->raw);
    HostArena &am = b16 ? wm : a, &at = b16 ? wt : a;
    std::vector<float>& fh = a.fhost;
    const size_t o_win = a.ftake(NEMO_NFFT, c->window), o_twc = a.ftake(NEMO_NFFT / 2, c->twc), o_tws = a.ftake(NEMO_NFFT / 2, c->tws);
    hann_padded(&fh[o_win], NEMO_WIN, NEMO_NFFT);
    fft512_twiddles(&fh[o_twc], &fh[o_tws]);
    const size_t o_fb = a.ftake((size_t)NEMO_BINS * mels, c->fb);
    std::vector<int> ranges(2 * mels, 0);
    slaney_filterbank(&fh[o_fb], ranges.data(), NEMO_BINS, (int)mels, 16000.0, NEMO_NFFT);
    c->maxN = (int64_t)c->cfg.max_seconds * 16000;
    c->Fcap = nm_frames(c->maxN); c->T1cap = nm_half(c->Fcap); c->T2cap = nm_half(c->T1cap); c->Tcap = nm_half(c->T2cap);
    const int Tc = c->Tcap;
    // the distances any listed context lets occur: -(C - 1) .. L C + C - 1, independent of T unless a left context is unlimited
    c->tab_lo = 0; c->tab_hi = 0;
    for (int i = 0; i < c->cfg.num_contexts; ++i) {
        const NmCtx x = nm_context(c->cfg.att_context[i][0], c->cfg.att_context[i][1], Tc);
        c->tab_lo = std::min(c->tab_lo, x.dlo); c->tab_hi = std::max(c->tab_hi, x.dhi);
    }
    const int NR = c->tab_hi - c->tab_lo + 1;
    auto lin = [&](const std::string& p, int64_t N, int64_t K, bool bias, SfLin& l) {
        l = SfLin{};
        a.fvec(p + ".weight", {N, K}, N * K, l.w);
        if (bias) a.fvec(p + ".bias", {N}, N, l.b);
    };
    auto mat = [&](const std::string& p, int64_t N, int64_t K, bool bias, SfLin& l) {      // a block matrix; its bias stays with the f32 tensors
        l = SfLin{};
        am.fvec(p + ".weight", {N, K}, N * K, l.w);
        if (bias) a.fvec(p + ".bias", {N}, N, l.b);
    };
    auto norm = [&](const std::string& p, int64_t n, const float*& w, const float*& b) { a.fvec(p + ".weight", {n}, n, w); a.fvec(p + ".bias", {n}, n, b); };
    const std::string SUB = "encoder.subsampling.";
    auto taps9 = [&](const std::string& name, const float*& dst) {    // conv taps [C][3][3][1] -> [9][C]
        const HostTensor& t = c->raw.need(name, {C, 3, 3, 1});
        const size_t off = a.ftake(9 * C, dst);
        for (int64_t ch = 0; ch < C; ++ch) for (int k = 0; k < 9; ++k) fh[off + k * C + ch] = t.v[ch * 9 + k];
    };
    taps9(SUB + "layers_0.weight", c->c0w); a.fvec(SUB + "layers_0.bias", {C}, C, c->c0b);
    taps9(SUB + "layers_2.weight", c->dw2w); a.fvec(SUB + "layers_2.bias", {C}, C, c->dw2b);
    a.fvec(SUB + "layers_3.weight", {C, 1, 1, C}, C * C, c->pw3.w); a.fvec(SUB + "layers_3.bias", {C}, C, c->pw3.b);
    taps9(SUB + "layers_5.weight", c->dw5w); a.fvec(SUB + "layers_5.bias", {C}, C, c->dw5b);
    a.fvec(SUB + "layers_6.weight", {C, 1, 1, C}, C * C, c->pw6.w); a.fvec(SUB + "layers_6.bias", {C}, C, c->pw6.b);
    {   // linear [d][C F3] reads the flattening (c, f); the stem keeps channels last: columns re-ordered to (f, c)
        const size_t ow = a.ftake((size_t)d * C * F3, c->lin.w);
        a.fvec(SUB + "linear.bias", {d}, d, c->lin.b);
        const HostTensor& w = c->raw.need(SUB + "linear.weight", {d, C * F3});
        for (int64_t n = 0; n < d; ++n) for (int64_t ch = 0; ch < C; ++ch) for (int64_t fq = 0; fq < F3; ++fq)
            fh[ow + (n * F3 + fq) * C + ch] = w.v[n * C * F3 + ch * F3 + fq];
    }
    c->fc.assign(c->L, mis_nemotron::Layer{});
    std::vector<SfLin> rk(c->L);
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li) + ".";
        mis_nemotron::Layer& l = c->fc[li];
        norm(q + "norm_feed_forward1", d, l.ln1w, l.ln1b);
        mat(q + "feed_forward1.linear1", f, d, ab, l.ff1a); mat(q + "feed_forward1.linear2", d, f, ab, l.ff1b);
        norm(q + "norm_self_att", d, l.lnaw, l.lnab);
        {   // q, k, v over the same input as one [3 d][d]; an absent bias is zero
            const size_t ow = am.ftake((size_t)3 * d * d, l.qkv.w), ob = a.ftake(3 * d, l.qkv.b);
            const char* names[3] = {"q_proj", "k_proj", "v_proj"};
            for (int i = 0; i < 3; ++i) {
                const HostTensor& w = c->raw.need(q + "self_attn." + names[i] + ".weight", {d, d});
                std::copy(w.v.begin(), w.v.end(), am.fhost.begin() + ow + (size_t)i * d * d);
                if (ab) { const HostTensor& bb = c->raw.need(q + "self_attn." + names[i] + ".bias", {d}); std::copy(bb.v.begin(), bb.v.end(), fh.begin() + ob + (size_t)i * d); }
            }
        }
        mat(q + "self_attn.o_proj", d, d, ab, l.o);
        at.fvec(q + "self_attn.relative_k_proj.weight", {d, d}, d * d, rk[li].w);
        a.fvec(q + "self_attn.bias_u", {H, hd}, d, l.u); a.fvec(q + "self_attn.bias_v", {H, hd}, d, l.v);
        norm(q + "norm_conv", d, l.lncw, l.lncb);
        am.fvec(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, 2 * d * d, l.pw1.w);
        am.fvec(q + "conv.pointwise_conv2.weight", {d, 1, d}, d * d, l.pw2.w);
        if (ab) {
            a.fvec(q + "conv.pointwise_conv1.bias", {2 * d}, 2 * d, l.pw1.b); a.fvec(q + "conv.pointwise_conv2.bias", {d}, d, l.pw2.b);
            a.fvec(q + "conv.depthwise_conv.bias", {d}, d, l.dwb);
        }
        {   // depthwise taps [d][k][1] -> [k][d]
            const HostTensor& dw = c->raw.need(q + "conv.depthwise_conv.weight", {d, ck, 1});
            const size_t o_dw = a.ftake((size_t)ck * d, l.dw);
            for (int64_t ch = 0; ch < d; ++ch) for (int64_t k = 0; k < ck; ++k) fh[o_dw + k * d + ch] = dw.v[ch * ck + k];
        }
        norm(q + "conv.norm", d, l.cnw, l.cnb);
        norm(q + "norm_feed_forward2", d, l.ln2w, l.ln2b);
        mat(q + "feed_forward2.linear1", f, d, ab, l.ff2a); mat(q + "feed_forward2.linear2", d, f, ab, l.ff2b);
        norm(q + "norm_out", d, l.lnow, l.lnob);
    }
    if (PH) { lin("prompt_kernel.linear0", PH, d + NP, true, c->pr0); lin("prompt_kernel.linear2", d, PH, true, c->pr2); }
    lin("joint.enc", J, d, true, c->jenc);
    // the sinusoid table by distance, the rows tab_lo .. tab_hi alone: columns interleaved sin, cos; formed in double, rounded once
    const float* tab = nullptr;
    const size_t o_tab = at.ftake((size_t)NR * d, tab);
    for (int r = 0; r < NR; ++r) {
        const double dist = (double)(r + c->tab_lo);
        for (int64_t k = 0; 2 * k < d; ++k) {
            const double ang = dist * exp(-(double)(2 * k) * log(10000.0) / (double)d);
            at.fhost[o_tab + (size_t)r * d + 2 * k] = (float)sin(ang);
            if (2 * k + 1 < d) at.fhost[o_tab + (size_t)r * d + 2 * k + 1] = (float)cos(ang);
        }
    }
    // the decoder, checked before anything is uploaded
    NmDecHost s{};
    s.embed = c->raw.need("decoder.prediction.embed.weight", {V, P}).v.data();
    for (int l = 0; l < c->cfg.pred_rnn_layers; ++l) {
        const std::string n = std::to_string(l);
        s.wih[l] = c->raw.need(NM_LSTM + ("weight_ih_l" + n), {4 * P, P}).v.data(); s.whh[l] = c->raw.need(NM_LSTM + ("weight_hh_l" + n), {4 * P, P}).v.data();
        s.bih[l] = c->raw.need(NM_LSTM + ("bias_ih_l" + n), {4 * P}).v.data(); s.bhh[l] = c->raw.need(NM_LSTM + ("bias_hh_l" + n), {4 * P}).v.data();
    }
    s.wp = c->raw.need("joint.pred.weight", {J, P}).v.data(); s.bp = c->raw.need("joint.pred.bias", {J}).v.data();
    s.wo = c->raw.need("joint.joint_net.weight", {V, J}).v.data(); s.bo = c->raw.need("joint.joint_net.bias", {V}).v.data();
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    nm_pack_decoder(s, c->cfg.pred_rnn_layers, (int)P, (int)J, (int)V, c->dec, c->rnnt);
    c->fbr.alloc(2 * mels);
    HIP_CHECK(hipMemcpy(c->fbr.p, ranges.data(), 2 * mels * sizeof(int), hipMemcpyHostToDevice));
    if (b16) nm_bf16_tables(c, wm, wt, tab, rk);
    else {
        c->ptab.alloc((size_t)c->L * NR * d);                      // each layer's relative_k_proj of the short table: one GEMM, once
        for (int li = 0; li < c->L; ++li) {
            float* dst = c->ptab.p + (size_t)li * NR * d;
            sf_gemm(c, sf_lin(tab, (int)d, rk[li], dst, (int)d, nullptr, NR), 1);
            c->fc[li].P = dst;
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    c->launches = 0;
    const size_t B = c->cfg.max_batch, M = B * Tc;
    c->pcm.alloc(B * c->maxN); c->melraw.alloc(B * c->Fcap * mels); c->feats.alloc(B * c->Fcap * mels);
    c->s0.alloc(B * c->T1cap * c->F1 * C); c->s1.alloc(B * c->T2cap * c->F2 * C); c->s2.alloc(M * F3 * C); c->emb.alloc(M * d);
    c->h.alloc(M * d); c->stats.alloc(M * 2);
    if (b16) {                                                      // big stays as the prompt kernel's f32 buffer alone
        c->big16.alloc(M * std::max<size_t>(f, 2 * d)); c->qkv16.alloc(M * 3 * d); c->att16.alloc(M * d);
        if (PH) c->big.alloc(M * PH);
    } else {
        c->big.alloc(M * std::max<size_t>(std::max<size_t>(f, 2 * d), PH)); c->qkv.alloc(M * 3 * d); c->att.alloc(M * d);
    }
    if (PH) c->prm.alloc(M * d);
    c->encp.alloc(M * J);
    c->cntN.alloc(B); c->cntF.alloc(B); c->cnt1.alloc(B); c->cnt2.alloc(B); c->cnt3.alloc(B); c->lang.alloc(B);
    c->outs.alloc(2 * B * c->cap + 3 * B);
    c->rnnt.max_symbols = c->cfg.max_symbols; c->rnnt.cap = c->cap;
    c->rnnt.tokens = c->outs.p; c->rnnt.frames = c->outs.p + B * c->cap;
    c->rnnt.count = c->outs.p + 2 * B * c->cap; c->rnnt.flag = c->rnnt.count + B; c->rnnt.steps = c->rnnt.flag + B;
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of the engine
extern "C" mis_status mis_nemotron_init_synthetic(mis_nemotron* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    const int64_t C = c->C, d = c->d, f = c->f, ck = c->ck, P = c->P, J = c->J, V = c->V;
    const bool ab = c->cfg.attention_bias != 0;
    const std::string SUB = "encoder.subsampling.";
    for (const char* n : {"layers_0", "layers_2", "layers_5"}) { sw.put(SUB + n + ".weight", {C, 3, 3, 1}, sqrt(3.0 / 9.0), 0.0f); sw.put(SUB + n + ".bias", {C}, 0.05, 0.0f); }
    for (const char* n : {"layers_3", "layers_6"}) { sw.put(SUB + n + ".weight", {C, 1, 1, C}, sqrt(3.0 / (double)C), 0.0f); sw.put(SUB + n + ".bias", {C}, 0.05, 0.0f); }
    sw.lin(SUB + "linear", d, C * c->F3, true, 1.0);
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li) + ".";
        for (const char* n : {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out", "conv.norm"}) sw.norm(q + n, d);
        for (const char* n : {"feed_forward1", "feed_forward2"}) { sw.lin(q + n + ".linear1", f, d, ab, 1.0); sw.lin(q + n + ".linear2", d, f, ab, 0.5); }
        for (const char* n : {"q_proj", "k_proj", "v_proj"}) sw.lin(q + "self_attn." + n, d, d, ab, 1.0);
        sw.lin(q + "self_attn.o_proj", d, d, ab, 0.5);
        sw.lin(q + "self_attn.relative_k_proj", d, d, false, 1.0);
        sw.put(q + "self_attn.bias_u", {c->H, c->hd}, 0.1, 0.0f); sw.put(q + "self_attn.bias_v", {c->H, c->hd}, 0.1, 0.0f);
        sw.put(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, sqrt(3.0 / (double)d), 0.0f);
        sw.put(q + "conv.pointwise_conv2.weight", {d, 1, d}, 0.5 * sqrt(3.0 / (double)d), 0.0f);
        sw.put(q + "conv.depthwise_conv.weight", {d, ck, 1}, sqrt(3.0 / (double)ck), 0.0f);
        if (ab) {
            sw.put(q + "conv.pointwise_conv1.bias", {2 * d}, 0.05, 0.0f); sw.put(q + "conv.pointwise_conv2.bias", {d}, 0.05, 0.0f);
            sw.put(q + "conv.depthwise_conv.bias", {d}, 0.05, 0.0f);
        }
    }
    if (c->PH) { sw.lin("prompt_kernel.linear0", c->PH, d + c->NP, true, 1.0); sw.lin("prompt_kernel.linear2", d, c->PH, true, 1.0); }
    sw.put("decoder.prediction.embed.weight", {V, P}, 1.0, 0.0f);
    for (int l = 0; l < c->cfg.pred_rnn_layers; ++l) {
        const std::string n = std::to_string(l);
        sw.put(NM_LSTM + ("weight_ih_l" + n), {4 * P, P}, sqrt(3.0 / (double)P), 0.0f); sw.put(NM_LSTM + ("weight_hh_l" + n), {4 * P, P}, sqrt(3.0 / (double)P), 0.0f);
        sw.put(NM_LSTM + ("bias_ih_l" + n), {4 * P}, 0.05, 0.0f); sw.put(NM_LSTM + ("bias_hh_l" + n), {4 * P}, 0.05, 0.0f);
    }
    sw.lin("joint.enc", J, d, true, 1.0); sw.lin("joint.pred", J, P, true, 1.0); sw.lin("joint.joint_net", V, J, true, 4.0);
    MIS_API_END
}

// ============================================================================ the chain
extern "C" int mis_nemotron_launches(const mis_nemotron* c) { return c ? c->launches : 0; }

extern "C" mis_status mis_nemotron_frames(const mis_nemotron* c, const int64_t* lens, int batch, int32_t* F_out, int32_t* T_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    const int64_t cap = (int64_t)c->cfg.max_seconds * 16000;
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] <= cap, MIS_ERR_INVALID_INPUT, "row %d: %lld samples outside 0..%lld (max_seconds %d)", b, (long long)lens[b],
                    (long long)cap, c->cfg.max_seconds);
        const int F = nm_frames(lens[b]);
        if (F_out) F_out[b] = F;
        if (T_out) T_out[b] = nm_half(nm_half(nm_half(F)));
    }
    MIS_API_END
}

// judged first (nothing of the handle is written), then taken: counts uploaded, pcm copied, the front end and the stem launched (6 launches)
static void nm_front_stem(mis_nemotron* c, const float* pcm, const int64_t* lens, const int32_t* langs, int batch, int64_t stride, int left, int right) {
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch %d outside 1..%d (max_batch)", batch, c->cfg.max_batch);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    MIS_REQUIRE(right >= 0, MIS_ERR_INVALID_INPUT, "att_context_size (%d, %d): right context below 0", left, right);
    const NmCtx ctx = nm_context(left, right, c->Tcap);
    MIS_REQUIRE(ctx.dlo >= c->tab_lo && ctx.dhi <= c->tab_hi, MIS_ERR_INVALID_INPUT,
                "att_context_size (%d, %d) needs the distances %d..%d: the model's listed contexts cover %d..%d", left, right, ctx.dlo, ctx.dhi, c->tab_lo,
                c->tab_hi);
    std::vector<int> N(batch), F(batch), t1(batch), t2(batch), t3(batch), lg(batch, 0);
    int Fp = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the row stride %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->maxN, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the workspace of %d seconds (max_seconds)", b, (long long)n,
                    c->cfg.max_seconds);
        if (c->PH && langs) {
            MIS_REQUIRE(langs[b] >= 0 && langs[b] < c->NP, MIS_ERR_INVALID_INPUT, "row %d: prompt index %d outside 0..%d", b, langs[b], c->NP - 1);
            lg[b] = langs[b];
        }
        N[b] = (int)n; F[b] = nm_frames(n); t1[b] = nm_half(F[b]); t2[b] = nm_half(t1[b]); t3[b] = nm_half(t2[b]);
        Fp = std::max(Fp, F[b]);
    }
    c->hN = N; c->hF = F; c->hT1 = t1; c->hT2 = t2; c->hT3 = t3; c->hlang = lg; c->ctx = ctx;
    c->batch = batch; c->Fp = Fp; c->T1p = nm_half(Fp); c->T2p = nm_half(c->T1p); c->Tp = nm_half(c->T2p);
    c->launches = 0; c->has_emb = false; c->timed_done = false;
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->cntN.p, c->hN.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cntF.p, c->hF.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt1.p, c->hT1.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt2.p, c->hT2.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt3.p, c->hT3.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->lang.p, c->hlang.data(), batch * 4, hipMemcpyHostToDevice, s));
    const int64_t ws = std::min<int64_t>(stride, c->maxN);
    HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, ws * 4, pcm, stride * 4, ws * 4, batch, hipMemcpyDefault, s));
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[0], s));
    MIS_LAUNCH(c, k_nemo_log_mel<false>, dim3(Fp, batch), dim3(256), c->pcm.p, ws, c->cntN.p, c->cntF.p, (const float*)nullptr, c->cfg.preemphasis, c->window,
               c->twc, c->tws, c->fb, c->fbr.p, c->melraw.p, Fp, c->mels);
    MIS_LAUNCH(c, k_nemo_norm, dim3(cdiv(c->mels, 64), batch), dim3(256), c->melraw.p, c->cntF.p, c->feats.p, Fp, c->mels, c->cfg.normalize);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[1], s));
    const int B = batch, C = c->C, F1 = c->F1, F2 = c->F2, F3 = c->F3;
    const size_t n0 = (size_t)B * c->T1p * F1 * C;
    MIS_LAUNCH(c, k_nm_conv0, dim3((unsigned)((n0 + 255) / 256)), dim3(256), c->feats.p, c->cntF.p, c->cnt1.p, c->c0w, c->c0b, c->s0.p, c->Fp, c->mels, c->T1p,
               F1, C, n0);
    auto dwpw = [&](const float* in, const int* cin, int Tin, int Fin, const float* dww, const float* dwb, const SfLin& pw, float* out, const int* cout,
                    int Tout, int Fout) {
        SfGemm p{};
        p.X = in; p.ldx = C; p.W = pw.w; p.bias = pw.b; p.Y = out; p.ldy = C; p.cnt = cout; p.Tp = Tout; p.rowmul = Fout; p.K = C; p.N = C;
        p.load = NM_LOAD_DWC; p.act = SF_ACT_RELU; p.cnt_in = cin; p.Tin = Tin; p.Fin = Fin; p.Fout = Fout; p.dww = dww; p.dwb = dwb;
        nm_gemm(c, p, B);
    };
    dwpw(c->s0.p, c->cnt1.p, c->T1p, F1, c->dw2w, c->dw2b, c->pw3, c->s1.p, c->cnt2.p, c->T2p, F2);
    dwpw(c->s1.p, c->cnt2.p, c->T2p, F2, c->dw5w, c->dw5b, c->pw6, c->s2.p, c->cnt3.p, c->Tp, F3);
    sf_gemm(c, sf_lin(c->s2.p, F3 * C, c->lin, c->emb.p, c->d, c->cnt3.p, c->Tp), B);
    c->has_emb = true;
}

// c->emb -> the Conformer blocks -> c->h (1 + 15 L launches); stop: -1 all, 1 .. L behind that block
static void nm_encoder(mis_nemotron* c, int stop) {
    if (c->enc_bf16) { nm_encoder_bf16(c, stop); return; }
    const int B = c->batch, Tp = c->Tp, d = c->d, f = c->f, M = B * Tp;
    const int* cnt = c->cnt3.p;
    const size_t nd = (size_t)M * d;
    MIS_LAUNCH(c, k_sf_intake, dim3((unsigned)((nd + 255) / 256)), dim3(256), c->emb.p, c->h.p, cnt, Tp, d, c->cfg.scale_input ? sqrtf((float)d) : 1.0f, nd);
    auto stats = [&](const float* x) { MIS_LAUNCH(c, k_sf_stats, dim3(cdiv(M, 4)), dim3(256), x, c->stats.p, d, 1e-5f, M); };
    auto ln_lin = [&](const float* x, const float* w, const float* b, const SfLin& l, float* y, int N, int act) {
        SfGemm p = sf_lin(x, d, l, y, N, cnt, Tp, act);
        p.load = SF_LOAD_LN; p.stats = c->stats.p; p.lnw = w; p.lnb = b;
        sf_gemm(c, p, B);
    };
    auto res_lin = [&](const float* x, int K, const SfLin& l, float* hres, int N, float ra) {
        SfGemm p = sf_lin(x, K, l, hres, N, cnt, Tp);
        p.R = hres; p.ldr = N; p.ra = ra;
        sf_gemm(c, p, B);
    };
    for (int li = 0; li < c->L; ++li) {                            // 15 launches a block
        const mis_nemotron::Layer& l = c->fc[li];
        stats(c->h.p);
        ln_lin(c->h.p, l.ln1w, l.ln1b, l.ff1a, c->big.p, f, SF_ACT_SILU);
        res_lin(c->big.p, f, l.ff1b, c->h.p, d, 0.5f);
        stats(c->h.p);
        ln_lin(c->h.p, l.lnaw, l.lnab, l.qkv, c->qkv.p, 3 * d, SF_ACT_NONE);
        NmAttn ap{c->qkv.p, 3 * d, d, 2 * d, c->att.p, d, cnt, Tp, c->hd, 1.0f, sqrtf((float)c->hd), l.u, l.v, l.P, d, -c->tab_lo,
                  c->ctx.C, c->ctx.L, c->ctx.dlo, c->ctx.dhi};
        nm_attn(c, ap, c->H, B);
        res_lin(c->att.p, d, l.o, c->h.p, d, 1.0f);
        stats(c->h.p);
        ln_lin(c->h.p, l.lncw, l.lncb, l.pw1, c->big.p, 2 * d, SF_ACT_NONE);
        nm_glu_dwconv_ln(c, c->big.p, l.dw, l.dwb, cnt, c->att.p, c->stats.p, Tp, d, c->ck, c->padl, B);
        {   // pointwise_conv2 over SiLU(LayerNorm(.)) formed in its operand load, + the residual
            SfGemm p = sf_lin(c->att.p, d, l.pw2, c->h.p, d, cnt, Tp);
            p.load = NM_LOAD_LN_SILU; p.stats = c->stats.p; p.lnw = l.cnw; p.lnb = l.cnb; p.R = c->h.p; p.ldr = d; p.ra = 1.0f;
            nm_gemm(c, p, B);
        }
        stats(c->h.p);
        ln_lin(c->h.p, l.ln2w, l.ln2b, l.ff2a, c->big.p, f, SF_ACT_SILU);
        res_lin(c->big.p, f, l.ff2b, c->h.p, d, 0.5f);
        MIS_LAUNCH(c, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), c->h.p, c->h.p, l.lnow, l.lnob, d, 1e-5f, M, cnt, Tp);
        if (stop == li + 1) return;
    }
}

// the prompt kernel, linear2(ReLU(linear0([h, onehot(language)]))): two launches; without one the frames pass as they are
static const float* nm_prompt(mis_nemotron* c) {
    if (!c->PH) return c->h.p;
    SfGemm p = sf_lin(c->h.p, c->d + c->NP, c->pr0, c->big.p, c->PH, c->cnt3.p, c->Tp, SF_ACT_RELU);
    p.ldx = c->d; p.load = NM_LOAD_PROMPT; p.Tin = c->d; p.cnt_in = c->lang.p;
    nm_gemm(c, p, c->batch);
    sf_gemm(c, sf_lin(c->big.p, c->PH, c->pr2, c->prm.p, c->d, c->cnt3.p, c->Tp), c->batch);
    return c->prm.p;
}

static void nm_joint_enc(mis_nemotron* c, const float* x) { sf_gemm(c, sf_lin(x, c->d, c->jenc, c->encp.p, c->J, c->cnt3.p, c->Tp), c->batch); }

static void nm_sync(mis_nemotron* c) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));                    // the call's one synchronisation
}

extern "C" mis_status mis_nemotron_encode(mis_nemotron* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int left, int right, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    nm_front_stem(c, pcm, lens, nullptr, batch, stride, left, right);
    nm_encoder(c, -1);
    HIP_CHECK(hipMemcpyAsync(out, c->h.p, (size_t)batch * c->Tp * c->d * 4, hipMemcpyDeviceToHost, c->stream));
    nm_sync(c);
    MIS_API_END
}

extern "C" mis_status mis_nemotron_generate(mis_nemotron* c, const float* pcm, const int64_t* lens, const int32_t* langs, int batch, int64_t stride, int left,
                                            int right, int32_t* tokens, int32_t* frames, int32_t* counts, int32_t* flags, int32_t* steps) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && tokens && frames && counts && flags, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    nm_front_stem(c, pcm, lens, langs, batch, stride, left, right);
    nm_encoder(c, -1);
    nm_joint_enc(c, nm_prompt(c));
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[2], s));
    NmRnnt p = c->rnnt;
    p.encp = c->encp.p; p.cnt = c->cnt3.p; p.Tp = c->Tp;
    MIS_LAUNCH(c, k_nm_rnnt, dim3(batch), dim3(NM_NT), p);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[3], s));
    const size_t n = (size_t)batch * c->cap;
    HIP_CHECK(hipMemcpyAsync(tokens, p.tokens, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(frames, p.frames, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(counts, p.count, batch * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(flags, p.flag, batch * 4, hipMemcpyDeviceToHost, s));
    if (steps) HIP_CHECK(hipMemcpyAsync(steps, p.steps, batch * 4, hipMemcpyDeviceToHost, s));
    nm_sync(c);
    c->timed_done = c->timed;
    MIS_API_END
}

// tensors of the last encode / generate, f32, zero rows behind a row's own T: stage 0 the stem's embeddings [B, T, hidden], 1 .. L that Conformer
// block, L + 1 the prompt kernel's output (without one: block L again), L + 2 joint.enc of it [B, T, joint_hidden].  The chain is
// deterministic: stages >= 1 are recomputed from the embeddings with the call's context and languages.
extern "C" mis_status mis_nemotron_tap(mis_nemotron* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && dims, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized && c->batch > 0 && c->has_emb, MIS_ERR_NOT_INITIALIZED, "no call to tap: the last call must be encode or generate");
    MIS_REQUIRE(stage >= 0 && stage <= c->L + 2, MIS_ERR_INVALID_INPUT, "stage %d outside 0..%d", stage, c->L + 2);
    HIP_CHECK(hipSetDevice(c->device));
    const int width = stage <= c->L + 1 ? c->d : c->J;
    dims[0] = c->batch; dims[1] = c->Tp; dims[2] = width;
    if (!out) return MIS_OK;
    const size_t n = (size_t)c->batch * c->Tp * width;
    MIS_REQUIRE((int64_t)n <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    const int kept = c->launches;
    const float* src = c->emb.p;
    if (stage >= 1) { nm_encoder(c, stage > c->L ? -1 : stage); src = c->h.p; }
    if (stage >= c->L + 1) src = nm_prompt(c);
    if (stage == c->L + 2) { nm_joint_enc(c, src); src = c->encp.p; }
    c->launches = kept;
    HIP_CHECK(hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToHost, c->stream));
    nm_sync(c);
    MIS_API_END
}

// ============================================================================ test and bench scaffolding (include/mi_speech_debug.h)
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

// benches: device milliseconds of the next / last mis_nemotron_generate: front end, stem + Conformer blocks + prompt + joint.enc, decode
extern "C" mis_status mis_debug_nemotron_timing(mis_nemotron* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    if (!ms) { c->timed = true; return MIS_OK; }
    MIS_REQUIRE(c->timed && c->timed_done, MIS_ERR_NOT_INITIALIZED, "no timed generate: the last call must be mis_nemotron_generate");
    for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    MIS_API_END
}

namespace {
struct NmdCtx { hipStream_t stream = nullptr; int launches = 0; };
constexpr int64_t NMD_MAX_ELEMS = (int64_t)1 << 28;
void nmd_sync(const NmdCtx& c) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
}
const float* nmd_fp(const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); }
const int* nmd_ip(const DevBuf<uint32_t>& d) { return reinterpret_cast<const int*>(d.p); }
}  // namespace

// ONE launch of k_nm_attn on caller-supplied host data; guards as mis_debug_parakeet_attn.  P [prow][ldp] holds the distances -poff ..
// prow - 1 - poff and must cover those of the context (left, right) under Tcap.  repeat > 1 (benches): the launch is timed over
// `repeat` further launches and ms_out receives the mean device milliseconds; the output is that of the first.
extern "C" mis_status mis_debug_nemotron_attn(int device, const float* qkv, int ld, int koff, int voff, const int32_t* cnt, int batch, int Tp, int heads, int hd,
                                              float qscale, float sdk, const float* u, const float* v, const float* P, int ldp, int prow, int poff, int left,
                                              int right, int Tcap, int ldo, float* out, int repeat, float* ms_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(qkv && cnt && out && u && v && P && batch >= 1 && Tp >= 1 && heads >= 1 && hd >= 65 && hd <= 128 && Tcap >= 1 && right >= 0 && prow >= 1,
                MIS_ERR_INVALID_INPUT, "Nemotron attention: every pointer, positive batch, Tp, heads, Tcap, prow, right >= 0 and a head size of 65..128 are required");
    const int64_t width = (int64_t)heads * hd;
    MIS_REQUIRE(koff >= 0 && voff >= 0 && width <= ld && koff + width <= ld && voff + width <= ld && width <= ldo && ldp >= width, MIS_ERR_INVALID_INPUT,
                "Nemotron attention: q, k and v must lie inside a row of ld columns, the output inside ldo, the table inside ldp");
    MIS_REQUIRE((int64_t)batch * Tp * ld <= NMD_MAX_ELEMS && (int64_t)batch * Tp * ldo <= NMD_MAX_ELEMS && (int64_t)prow * ldp <= NMD_MAX_ELEMS &&
                    batch <= 65535 && heads <= 65535 && Tp <= Tcap, MIS_ERR_INVALID_INPUT, "Nemotron attention: tensor too large (Tp <= Tcap)");
    const NmCtx x = nm_context(left, right, Tcap);
    MIS_REQUIRE(x.dlo + poff >= 0 && x.dhi + poff < prow, MIS_ERR_INVALID_INPUT, "Nemotron attention: the table rows %d..%d do not cover the distances %d..%d",
                -poff, prow - 1 - poff, x.dlo, x.dhi);
    HIP_CHECK(hipSetDevice(device));
    NmdCtx c;
    const size_t rows = (size_t)batch * Tp;
    DevBuf<uint32_t> dq, dcnt, du, dv, dP;
    alloc32(dq, qkv, rows * ld, F32_NAN);
    alloc32(dcnt, cnt, batch, 0x7FFFFFFFu);
    alloc32(du, u, width, F32_NAN); alloc32(dv, v, width, F32_NAN); alloc32(dP, P, (size_t)prow * ldp, F32_NAN);
    GuardedOut o;
    o.alloc(rows * ldo * 4, (size_t)64 * ldo * 4);
    NmAttn p{nmd_fp(dq), ld, koff, voff, reinterpret_cast<float*>(o.p()), ldo, nmd_ip(dcnt), Tp, hd, qscale, sdk, nmd_fp(du), nmd_fp(dv),
             nmd_fp(dP), ldp, poff, x.C, x.L, x.dlo, x.dhi};
    nm_attn(&c, p, heads, batch);
    nmd_sync(c);
    o.check_guards();
    std::vector<uint32_t> hbuf(o.body / 4);
    HIP_CHECK(hipMemcpy(hbuf.data(), o.p(), o.body, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        memcpy(out + r * width, hbuf.data() + r * ldo, width * 4);
        for (size_t col = width; col < (size_t)ldo; ++col)
            MIS_REQUIRE(hbuf[r * ldo + col] == 0xFFFFFFFFu, MIS_ERR_GENERATION_FAILED, "the kernel wrote column %zu of row %zu behind its %lld columns", col, r, (long long)width);
    }
    if (repeat > 1 && ms_out) {
        HipEvents<2> ev;
        HIP_CHECK(hipEventRecord(ev[0], c.stream));
        for (int i = 0; i < repeat; ++i) nm_attn(&c, p, heads, batch);
        HIP_CHECK(hipEventRecord(ev[1], c.stream));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipEventElapsedTime(ms_out, ev[0], ev[1]));
        *ms_out /= (float)repeat;
    }
    MIS_API_END
}

// ONE launch of k_nm_glu_dwconv_ln: pw [batch Tp][2 C], taps [k][C], bias [C] or NULL -> out [batch Tp][C], stats [batch Tp][2]
extern "C" mis_status mis_debug_nemotron_dwconv_ln(int device, const float* pw, const float* taps, const float* bias, const int32_t* cnt, int batch, int Tp, int C,
                                                   int k, int padl, float* out, float* stats) {
    MIS_API_BEGIN
    MIS_REQUIRE(pw && taps && cnt && out && stats && batch >= 1 && batch <= 65535 && Tp >= 1 && C >= 1 && k >= 1 && k <= SF_DW_MAXK && padl >= 0 && padl < k &&
                    (int64_t)batch * Tp * 2 * C <= NMD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Nemotron conv module: every pointer, positive batch, Tp, C, 1 <= k <= %d and 0 <= padl < k are required", SF_DW_MAXK);
    HIP_CHECK(hipSetDevice(device));
    NmdCtx c;
    const size_t rows = (size_t)batch * Tp;
    DevBuf<uint32_t> dpw, dt, db, dc;
    alloc32(dpw, pw, rows * 2 * C, F32_NAN); alloc32(dt, taps, (size_t)k * C, F32_NAN); alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    if (bias) alloc32(db, bias, C, F32_NAN);
    GuardedOut o, st;
    o.alloc(rows * C * 4, 4096); st.alloc(rows * 2 * 4, 4096);
    nm_glu_dwconv_ln(&c, nmd_fp(dpw), nmd_fp(dt), bias ? nmd_fp(db) : nullptr, nmd_ip(dc), reinterpret_cast<float*>(o.p()), reinterpret_cast<float*>(st.p()), Tp, C,
                     k, padl, batch);
    nmd_sync(c);
    o.check_guards(); st.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(stats, st.p(), st.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

// ONE launch of the causal stem: stage 0 k_nm_conv0 on x [batch][Tin][Fin] (w9 [9][C], b9 [C]); stage 1 the depthwise operand load +
// pointwise conv + ReLU on x [batch][Tin][Fin][C] (w9, b9 the depthwise taps, pw [C][C], pwb [C]).  cnt_in [batch] -> out [batch][Tin / 2 + 1]
// [Fin / 2 + 1][C], frames behind cnt_in / 2 + 1 zero.
extern "C" mis_status mis_debug_nemotron_stem(int device, int stage, const float* x, const int32_t* cnt_in, int batch, int Tin, int Fin, int C, const float* w9,
                                              const float* b9, const float* pw, const float* pwb, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && cnt_in && w9 && b9 && out && (stage == 0 || (stage == 1 && pw && pwb)) && batch >= 1 && batch <= 65535 && Tin >= 1 && Fin >= 1 && C >= 1 &&
                    (int64_t)batch * Tin * Fin * C <= NMD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Nemotron stem: every pointer of the stage (0, 1), positive sizes are required");
    HIP_CHECK(hipSetDevice(device));
    NmdCtx c;
    const int Tout = nm_half(Tin), Fout = nm_half(Fin);
    std::vector<int32_t> hout(batch);
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(cnt_in[b] >= 0 && cnt_in[b] <= Tin, MIS_ERR_INVALID_INPUT, "Nemotron stem: count %d outside 0..%d", cnt_in[b], Tin);
        hout[b] = nm_half(cnt_in[b]);
    }
    DevBuf<uint32_t> dx, dci, dco, dw, db, dpw, dpb;
    alloc32(dx, x, (size_t)batch * Tin * Fin * (stage ? C : 1), F32_NAN); alloc32(dci, cnt_in, batch, 0x7FFFFFFFu); alloc32(dco, hout.data(), batch, 0x7FFFFFFFu);
    alloc32(dw, w9, (size_t)9 * C, F32_NAN); alloc32(db, b9, C, F32_NAN);
    GuardedOut o;
    const size_t total = (size_t)batch * Tout * Fout * C;
    o.alloc(total * 4, 4096);
    if (stage == 0) {
        MIS_LAUNCH(&c, k_nm_conv0, dim3((unsigned)((total + 255) / 256)), dim3(256), nmd_fp(dx), nmd_ip(dci), nmd_ip(dco), nmd_fp(dw), nmd_fp(db),
                   reinterpret_cast<float*>(o.p()), Tin, Fin, Tout, Fout, C, total);
    } else {
        alloc32(dpw, pw, (size_t)C * C, F32_NAN); alloc32(dpb, pwb, C, F32_NAN);
        SfGemm p{};
        p.X = nmd_fp(dx); p.ldx = C; p.W = nmd_fp(dpw); p.bias = nmd_fp(dpb); p.Y = reinterpret_cast<float*>(o.p()); p.ldy = C; p.cnt = nmd_ip(dco); p.Tp = Tout;
        p.rowmul = Fout; p.K = C; p.N = C; p.load = NM_LOAD_DWC; p.act = SF_ACT_RELU; p.cnt_in = nmd_ip(dci); p.Tin = Tin; p.Fin = Fin; p.Fout = Fout;
        p.dww = nmd_fp(dw); p.dwb = nmd_fp(db);
        nm_gemm(&c, p, batch);
    }
    nmd_sync(c);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

// ONE launch of k_nm_rnnt on caller-supplied projected frames encp [batch][Tp][J] (joint.enc applied, bias included) and the decoder's tensors
// as a checkpoint holds them; outputs [batch][cap] x 2 and [batch] x 3.  The token outputs are guarded; entries behind a row's count stay 0xFF.
extern "C" mis_status mis_debug_nemotron_rnnt(int device, const float* encp, const int32_t* cnt, int batch, int Tp, int J, int P, int vocab, int layers,
                                              int max_symbols, int cap, const float* embed, const float* const* wih, const float* const* whh,
                                              const float* const* bih, const float* const* bhh, const float* wp, const float* bp, const float* wo, const float* bo,
                                              int32_t* tokens, int32_t* frames, int32_t* counts, int32_t* flags, int32_t* steps) {
    MIS_API_BEGIN
    MIS_REQUIRE(encp && cnt && embed && wih && whh && bih && bhh && wp && bp && wo && bo && tokens && frames && counts && flags && steps, MIS_ERR_INVALID_INPUT,
                "Nemotron RNN-T: null argument");
    MIS_REQUIRE(batch >= 1 && batch <= 65535 && Tp >= 1 && cap >= 1 && (int64_t)batch * Tp * J <= NMD_MAX_ELEMS && (int64_t)batch * cap <= NMD_MAX_ELEMS,
                MIS_ERR_INVALID_INPUT, "Nemotron RNN-T: positive batch, Tp, cap are required");
    nm_check_decoder_dims(layers, P, J, vocab, max_symbols);
    HIP_CHECK(hipSetDevice(device));
    NmdCtx c;
    NmRnnt p{};
    DevBuf<float> arena;
    NmDecHost s{embed, {wih[0], layers > 1 ? wih[1] : nullptr}, {whh[0], layers > 1 ? whh[1] : nullptr}, {bih[0], layers > 1 ? bih[1] : nullptr},
                {bhh[0], layers > 1 ? bhh[1] : nullptr}, wp, bp, wo, bo};
    nm_pack_decoder(s, layers, P, J, vocab + 1, arena, p);
    DevBuf<uint32_t> de, dc;
    alloc32(de, encp, (size_t)batch * Tp * J, F32_NAN);
    alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    GuardedOut o;
    const size_t n = (size_t)batch * cap;
    o.alloc((2 * n + 3 * batch) * 4, 4096);
    int* ob = reinterpret_cast<int*>(o.p());
    p.encp = nmd_fp(de); p.cnt = nmd_ip(dc); p.Tp = Tp; p.max_symbols = max_symbols; p.cap = cap;
    p.tokens = ob; p.frames = ob + n; p.count = ob + 2 * n; p.flag = p.count + batch; p.steps = p.flag + batch;
    MIS_LAUNCH(&c, k_nm_rnnt, dim3(batch), dim3(NM_NT), p);
    nmd_sync(c);
    o.check_guards();
    HIP_CHECK(hipMemcpy(tokens, p.tokens, n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(frames, p.frames, n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(counts, p.count, batch * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(flags, p.flag, batch * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(steps, p.steps, batch * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// ---------------------------------------------------------------------------- the bf16 encoder's kernels (nemotron_encoder_bf16.h)
namespace {
// the ONE checked launch; then, with ms, `repeat` more of the same launch between two events: *ms = milliseconds a launch
template <class F>
void nmd_run(NmdCtx& c, F launch, int repeat, float* ms) {
    launch();
    nmd_sync(c);
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
void nmd_rows_out(GuardedOut& o, void* out, size_t rows, size_t width, size_t ld, size_t es) {
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

// ONE launch of k_nm_attn_bf16: the arguments of mis_debug_nemotron_attn with bf16 qkv and table, head sizes 1..128; out bf16 [batch Tp][heads hd]
extern "C" mis_status mis_debug_nemotron_attn_bf16(int device, const uint16_t* qkv, int ld, int koff, int voff, const int32_t* cnt, int batch, int Tp, int heads,
                                                   int hd, float qscale, float sdk, const float* u, const float* v, const uint16_t* P, int ldp, int prow, int poff,
                                                   int left, int right, int Tcap, int ldo, uint16_t* out, int repeat, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(qkv && cnt && out && u && v && P && batch >= 1 && Tp >= 1 && heads >= 1 && hd >= 1 && hd <= 128 && Tcap >= 1 && right >= 0 && prow >= 1,
                MIS_ERR_INVALID_INPUT, "Nemotron bf16 attention: every pointer, positive batch, Tp, heads, Tcap, prow, right >= 0 and a head size of 1..128 are required");
    const int64_t width = (int64_t)heads * hd;
    MIS_REQUIRE(koff >= 0 && voff >= 0 && width <= ld && koff + width <= ld && voff + width <= ld && width <= ldo && ldp >= width, MIS_ERR_INVALID_INPUT,
                "Nemotron bf16 attention: q, k and v must lie inside a row of ld columns, the output inside ldo, the table inside ldp");
    MIS_REQUIRE((int64_t)batch * Tp * ld <= NMD_MAX_ELEMS && (int64_t)batch * Tp * ldo <= NMD_MAX_ELEMS && (int64_t)prow * ldp <= NMD_MAX_ELEMS &&
                    batch <= 65535 && heads <= 65535 && Tp <= Tcap, MIS_ERR_INVALID_INPUT, "Nemotron bf16 attention: tensor too large (Tp <= Tcap)");
    const NmCtx x = nm_context(left, right, Tcap);
    MIS_REQUIRE(x.dlo + poff >= 0 && x.dhi + poff < prow, MIS_ERR_INVALID_INPUT, "Nemotron bf16 attention: the table rows %d..%d do not cover the distances %d..%d",
                -poff, prow - 1 - poff, x.dlo, x.dhi);
    HIP_CHECK(hipSetDevice(device));
    NmdCtx c;
    const size_t rows = (size_t)batch * Tp;
    DevBuf<uint16_t> dq, dP;
    DevBuf<uint32_t> dcnt, du, dv;
    alloc16(dq, qkv, rows * ld, BF16_NAN); alloc16(dP, P, (size_t)prow * ldp, BF16_NAN);
    alloc32(dcnt, cnt, batch, 0x7FFFFFFFu);
    alloc32(du, u, width, F32_NAN); alloc32(dv, v, width, F32_NAN);
    GuardedOut o;
    o.alloc(rows * ldo * 2, (size_t)64 * ldo * 2);
    NmbAttn p{dq.p, ld, koff, voff, reinterpret_cast<bf16_t*>(o.p()), ldo, nmd_ip(dcnt), Tp, hd, qscale, sdk, nmd_fp(du), nmd_fp(dv), dP.p, ldp, poff,
              x.C, x.L, x.dlo, x.dhi};
    nmd_run(c, [&] { nmb_attn(&c, p, heads, hd, batch); c.launches = 1; }, repeat, ms);
    nmd_rows_out(o, out, rows, width, ldo, 2);
    MIS_API_END
}

// ONE launch of k_nm_glu_dwconv_ln_bf16: pw bf16 [batch Tp][2 C], taps f32 [k][C], bias f32 [C] or NULL -> out bf16 [batch Tp][C], stats f32 [batch Tp][2]
extern "C" mis_status mis_debug_nemotron_dwconv_ln_bf16(int device, const uint16_t* pw, const float* taps, const float* bias, const int32_t* cnt, int batch, int Tp,
                                                        int C, int k, int padl, uint16_t* out, float* stats) {
    MIS_API_BEGIN
    MIS_REQUIRE(pw && taps && cnt && out && stats && batch >= 1 && batch <= 65535 && Tp >= 1 && C >= 1 && k >= 1 && k <= SF_DW_MAXK && padl >= 0 && padl < k &&
                    (int64_t)batch * Tp * 2 * C <= NMD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Nemotron bf16 conv module: every pointer, positive batch, Tp, C, 1 <= k <= %d and 0 <= padl < k are required", SF_DW_MAXK);
    HIP_CHECK(hipSetDevice(device));
    NmdCtx c;
    const size_t rows = (size_t)batch * Tp;
    DevBuf<uint16_t> dpw;
    DevBuf<uint32_t> dt, db, dc;
    alloc16(dpw, pw, rows * 2 * C, BF16_NAN);
    alloc32(dt, taps, (size_t)k * C, F32_NAN); alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    if (bias) alloc32(db, bias, C, F32_NAN);
    GuardedOut o, st;
    o.alloc(rows * C * 2, 4096); st.alloc(rows * 2 * 4, 4096);
    nmb_glu_dwconv_ln(&c, dpw.p, nmd_fp(dt), bias ? nmd_fp(db) : nullptr, nmd_ip(dc), reinterpret_cast<bf16_t*>(o.p()), reinterpret_cast<float*>(st.p()), Tp, C, k,
                      padl, batch);
    nmd_sync(c);
    o.check_guards(); st.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(stats, st.p(), st.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

// ONE launch of k_pk_gemm_bf16 as mis_debug_parakeet_gemm_bf16, with load 2 (PKB_LOAD_LN_SILU): x bf16 [batch Tp][K] read as
// SiLU((x - mean) rstd lnw + lnb), stats [batch Tp][2], lnw, lnb [K].  rule 2 / 3 / 4: k_nm_gemm_bf16_rows (nemotron_stream_bf16.h) at 64 /
// 32 / 16 columns a block, batch <= 64; it leaves the rows behind cnt[b] unwritten (0xFF bytes in out)
extern "C" mis_status mis_debug_nemotron_gemm_bf16(int device, int load, int epi, int rule, const void* x, const float* stats, const float* lnw, const float* lnb,
                                                   const uint16_t* w, const float* bias, const float* R, float ra, const int32_t* cnt, int batch, int Tp, int K,
                                                   int N, void* out, int repeat, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && w && cnt && out && batch >= 1 && batch <= 65535 && Tp >= 1 && K >= 32 && K % 32 == 0 && N >= 8 && N % 8 == 0, MIS_ERR_INVALID_INPUT,
                "Nemotron bf16 GEMM: pointers, positive batch and Tp, K a multiple of 32 and N a multiple of 8 are required");
    MIS_REQUIRE((load == PKB_LOAD_BF16 || ((load == PKB_LOAD_LN || load == PKB_LOAD_LN_SILU) && stats && lnw && lnb)) && epi >= PKB_EPI_NONE &&
                    epi <= PKB_EPI_RES && (epi != PKB_EPI_RES || R) && rule >= PKB_TILE64 && rule <= NMR_ROWS16 &&
                    (rule < NMR_ROWS64 || batch <= NMR_MAXB), MIS_ERR_INVALID_INPUT,
                "Nemotron bf16 GEMM: unknown load / epilogue / rule (the short-pass rules take at most %d batch entries), or a missing operand", NMR_MAXB);
    int live = 0;
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(cnt[b] >= 0, MIS_ERR_INVALID_INPUT, "Nemotron bf16 GEMM: negative count of row %d", b);
        live += std::min(cnt[b], Tp);
    }
    const size_t rows = (size_t)batch * Tp;
    MIS_REQUIRE((int64_t)rows * K <= NMD_MAX_ELEMS && (int64_t)rows * N <= NMD_MAX_ELEMS && (int64_t)N * K <= NMD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Nemotron bf16 GEMM: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    NmdCtx c;
    DevBuf<uint16_t> dxb, dw;
    DevBuf<uint32_t> dxf, dst, dlw, dlb, dbias, dR, dcnt;
    PkbGemm p{};
    if (load == PKB_LOAD_LN) { alloc32(dxf, x, rows * K, F32_NAN); p.Xf = nmd_fp(dxf); }
    else { alloc16(dxb, static_cast<const uint16_t*>(x), rows * K, BF16_NAN); p.Xb = dxb.p; }
    if (load != PKB_LOAD_BF16) {
        alloc32(dst, stats, rows * 2, F32_NAN); alloc32(dlw, lnw, K, F32_NAN); alloc32(dlb, lnb, K, F32_NAN);
        p.stats = nmd_fp(dst); p.lnw = nmd_fp(dlw); p.lnb = nmd_fp(dlb);
    }
    alloc16(dw, w, (size_t)N * K, BF16_NAN);
    alloc32(dcnt, cnt, batch, 0x7FFFFFFFu);
    if (bias) { alloc32(dbias, bias, N, F32_NAN); p.bias = nmd_fp(dbias); }
    if (epi == PKB_EPI_RES) { alloc32(dR, R, rows * N, F32_NAN); p.R = nmd_fp(dR); p.ldr = N; p.ra = ra; }
    const size_t es = epi == PKB_EPI_RES ? 4 : 2;
    GuardedOut o;
    o.alloc(rows * N * es, (size_t)64 * N * es);
    p.Yf = reinterpret_cast<float*>(o.p()); p.Yb = reinterpret_cast<bf16_t*>(o.p());
    p.ldx = K; p.W = dw.p; p.ldy = N; p.cnt = nmd_ip(dcnt); p.Tp = Tp; p.K = K; p.N = N; p.epi = epi;
    nmd_run(c, [&] { nmr_gemm_launch(&c, p, load, rule, batch, live); c.launches = 1; }, repeat, ms);
    nmd_rows_out(o, out, rows, N, N, es);
    MIS_API_END
}
