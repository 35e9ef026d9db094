// whisper_kernels.h - launchers of the Whisper encoder kernels (whisper_kernels.hip)
#pragma once
#include "common.h"

enum { BG_NONE = 0, BG_GELU = 1, BG_RESID = 2, BG_GELU_POS = 3 };
struct BigGemmParams {
    const bf16_t* X;     // [M][ldx] row-major, first K columns used
    const bf16_t* W;     // [N][K] row-major (Linear.weight layout)
    const bf16_t* bias;  // [N] or null
    const bf16_t* R;     // BG_RESID: [M][N]; BG_GELU_POS: positional table [pos_rows][N] indexed by m % pos_rows
    bf16_t* C;           // [M][N]
    int M, N, K, ldx, pos_rows;
};
void launch_gemm_big(int epi, const BigGemmParams& p, hipStream_t s);
// what launch_gemm_big / launch_layernorm / launch_attn_prefill launched last on this thread (host bookkeeping only, as
// g_codec_last_launch of codec_kernels.h): the mis_debug_* entry points of enc_debug.hip report it
struct EncLaunchInfo {
    int gemm = -1, epi = 0, WM = 0, WN = 0;   // 0 k_gemm_big, 1 k_gemm_big2, 2 k_gemm_big3; the wave grid (m x n)
    int ln = -1;                              // 0 k_layernorm, 1 k_layernorm8
    int attn = -1, attn_D = 0;                // 0 k_attn_prefill, 1 k_attn_prefill2
};
extern thread_local EncLaunchInfo g_enc_last_launch;
void launch_layernorm(const bf16_t* x, bf16_t* y, const bf16_t* w, const bf16_t* b, int rows, int d, float eps, hipStream_t s);
void launch_im2col3_f32(const float* in, bf16_t* out, int B, int Tin, int C, int Tout, int stride, hipStream_t s);
void launch_im2col3_bf16(const bf16_t* in, bf16_t* out, int B, int Tin, int C, int Tout, int stride, hipStream_t s);
void launch_scatter_kv(const bf16_t* src, int ld, int kcol0, int vcol0, bf16_t* kc, bf16_t* vc, int B, int T, int H, int D,
                       int Spad, hipStream_t s);
// Cache contract of launch_attn_prefill: kc / vc hold ceil(T / 32) tiles per (row, head) within Spad keys; keys T .. tile end of the
// last tile must be ZERO in both images, as launch_scatter_kv leaves them - the kernels mask the scores there (p = 0) but still multiply
// p by the stored values, so a NaN or Inf there reaches the output.  Tiles behind the last one are never read.  ldq must be a multiple of 8.
void launch_attn_prefill(const bf16_t* q, int ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, int ldo, int B, int T,
                         int H, int D, int Spad, hipStream_t s);
void launch_whisper_embed_ln(const bf16_t* emb, const bf16_t* pos_emb, const int32_t* ids, const uint8_t* active, int* pos_cur,
                             int* pos_next, const bf16_t* lw, const bf16_t* lb, bf16_t* h, bf16_t* x, int d, int vocab,
                             int max_pos, int batch, int Mpad, hipStream_t s);
void launch_whisper_suppress(bf16_t* logits, int Vpad, int vocab, const int32_t* sup, int n_sup, const int32_t* bsup, int n_bsup,
                             const int32_t* n_gen, const uint8_t* active, int batch, hipStream_t s);

// The Whisper encoder (WhisperEncoder, WhisperLayers.swift:110-160; Smart Turn's encoder is the same stack): weights as bf16 device
// pointers, work buffers owned by the caller and sized for B rows.
struct WhisperEncLayer { bf16_t *ln1w, *ln1b, *wqkv, *bqkv, *wo, *bo, *ln2w, *ln2b, *fc1, *b1, *fc2, *b2; };
struct WhisperEncWeights {
    bf16_t *conv1w = nullptr, *conv1b = nullptr, *conv2w = nullptr, *conv2b = nullptr, *pos = nullptr, *lnw = nullptr, *lnb = nullptr;
    std::vector<WhisperEncLayer> layers;
    int d = 0, H = 0, D = 0, ffn = 0, K1 = 0, Spad = 0;   // K1: columns of a conv1 patch row; Spad: key rows per head of kc / vc
};
struct WhisperEncWork { bf16_t *col1, *h1, *col2, *h, *x, *qkv, *att, *ff, *kc, *vc; };
// col1 (k = 3 patches of B x frames feature rows, K1 columns) -> enc_out [B T][d], T = frames / 2.  Launches only - 4 + 8 per layer + 1 -
// on s: no allocation, no synchronisation, so the chain can be captured into a graph.
void whisper_encoder_enqueue(const WhisperEncWeights& w, const WhisperEncWork& k, int B, int frames, int T, bf16_t* enc_out, hipStream_t s);
