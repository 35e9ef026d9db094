/* mi_speech_debug.h - diagnostics and test scaffolding exported by libmi_speech.so next to the product ABI (include/mi_speech.h).
 *
 * Nothing here replaces a reference interface and no host application needs it: these entry points exist for DESIGN.md's
 * measurements (launch floor, split-factor model) and for tests that have to provoke conditions a healthy run never meets
 * (compute units held by another stream, counted sampler time-outs).  Kept out of mi_speech.h so that the drop-in surface is
 * exactly what a Swift shim binds. */
#ifndef MI_SPEECH_DEBUG_H
#define MI_SPEECH_DEBUG_H
#include "mi_speech.h"
#ifdef __cplusplus
extern "C" {
#endif

/* diagnostics: microseconds per dependent kernel boundary in a replayed hipGraph of n trivial kernels
 * (mode 0: 1 block x 64 threads, 1: 32 x 1024, 2: 1024 x 256).  DESIGN.md quotes it as the launch floor. */
mis_status mis_debug_launch_floor(int device, int n_kernels, int mode, int reps, double* us_per_kernel);
/* diagnostics: the inter-block split-K factor the engines pick for a weight-streaming GEMM with `items` n-tile groups, `k_tiles`
 * 32-wide k-tiles and `waves_per_item` waves per work item ("Split-K factor from a cost model"); no GPU needed
 * (falls back to 256 CUs when no device is visible). */
int32_t mis_debug_choose_split(int32_t items, int32_t k_tiles, int32_t waves_per_item, int32_t s_max);
/* tests: occupy compute units from ANOTHER stream - `blocks` workgroups of `threads` threads, each reserving 128 KB of the CU's 160 KB of LDS (one per CU, and
 * nothing that needs more than 32 KB of LDS fits beside it), that spin (s_sleep) for `seconds` - so that launches on the library's streams find fewer CUs than the device has (the
 * condition under which the one-launch sampler's row barriers time out and the engines recover on the multi-launch path).  Every
 * spinner announces itself on entry; the call returns MIS_OK only once all `blocks` of them are RESIDENT (handshake through a
 * host-visible counter), or MIS_ERR_DEVICE if that does not happen within two seconds - the spinner is then released and the caller
 * should treat the condition as not reproducible on this device (tests skip).  mis_debug_occupy_wait() releases the spinners early
 * (if they are still running), waits for them and frees the stream. */
mis_status mis_debug_occupy_cus(int device, int blocks, int threads, double seconds);
mis_status mis_debug_occupy_wait(void);
int32_t mis_debug_device_cus(int device);            /* compute units of a device (0 when it does not exist) */
/* diagnostics / tests: launches of the one-launch sampler that reported a timed-out row barrier in this process so far */
int32_t mis_debug_sampler_failures(void);
/* tests: device bytes a finalized Whisper handle holds for its weights (the bf16 arena plus the code / scale tables of the natively
 * streamed quantised decoder matrices) */
int64_t mis_debug_whisper_weight_bytes(const mis_whisper* c);
/* tests: stage outputs of the Mimi decoder (whole sequence), out f32 [batch, C, T'].  stage 0 RVQ latent, 1 upsampled, 2 transformer,
 * 3 init conv, 4 + i decoder layer i (ELU, transposed conv, residual blocks), 4 + n_ratios final (pcm, C = 1) */
mis_status mis_debug_mimi_decoder_tap(mis_mimi* m, const int32_t* codes, int batch, int n_q, int T, int stage, float* out, int64_t capacity,
                                      int32_t* channels, int64_t* length);
/* tests (tests/test_gpu_encodec_encode.py): the EnCodec encode chain.  stage >= 0: `in` is audio f32 [rows][channels][L] (+ mask u8
 * [rows][L] or NULL); out f32 [rows][C][T'] is that stage's output: 0 normalised input, 1 conv0, 2 + i down block i (resnets, ELU, strided
 * conv), 2 + n_ratios LSTM block, 3 + n_ratios embeddings.  stage -1: ONE launch of the residual-VQ search on caller-supplied embeddings
 * `in` f32 [rows][D][L] (L frames): codes_out i32 [rows][n_q][L] and out f32 [n_q + 1][rows][D][L], the residual before every quantizer
 * and after the last.  Inputs are followed by NaN (mask: 0xFF); the RVQ outputs lie between guard bands, a changed guard byte fails the
 * call with MIS_ERR_GENERATION_FAILED */
mis_status mis_debug_encodec_encode_tap(mis_encodec* c, const float* in, const uint8_t* mask, int rows, int64_t L, int n_q, int stage, float* out,
                                        int64_t capacity, int32_t* codes_out, int32_t* channels, int64_t* length);

/* csrc/gemm_debug.hip, tests (tests/test_gpu_gemm_ops.py): ONE launch of a GEMM launcher on caller-supplied host data.  16-bit operands are
 * passed as raw payloads (uint16).  Operands are packed by the product's load-time kernels; W2 (optional, same shape as W) is packed with
 * tile stride 2 at offset 1 behind W at offset 0 - the gate / up interleave, twice the output columns.  The output is poisoned (NaN) before
 * the launch and lies between poisoned guard bands: an element never written comes back as NaN, a changed guard word fails the call with
 * MIS_ERR_GENERATION_FAILED; every input is followed by NaN (codes: 0xFF), so an over-read shows in the result.  An arrangement the
 * launcher does not build returns the launcher's status and launches nothing.  report (may be NULL) int32[8]: the instantiation that ran -
 * kernel (0 k_gemm_skinny, 1 k_gemm_skinny_q, 2 k_gemm_skinny_q1, 3 k_gemm_pf), MT, R, epilogue, KSB, U, bits (16 = bf16 weights), scale
 * format (0 bf16, 1 f16).
 *   gemm_skinny: W bf16 [N][K], X bf16 [M][K] (M <= 64; packed as Mpad = 16 ceil(M / 16) rows, rows >= M zero), bias bf16 [output columns]
 *     or NULL, epi / R / ksb / U / S the arguments of launch_gemm_skinny (S > K / 32: MIS_ERR_INVALID_INPUT).  out f32: epilogue 0 (partial)
 *     the raw slabs [S][Mpad][cols]; 1 (bf16) [Mpad][cols]; 2 (silu(gate) * up) [Mpad][cols / 2], 3 / 4 (gelu / silu, packed) [Mpad][cols] un-packed.
 *   gemm_skinny_q: the same on MLX affine-quantised operands (group size 64): wq uint32 [N][K bits / 32], scales / biases 16-bit [N][K / 64]
 *     of sb_dtype (MIS_BF16 / MIS_F16); the launcher picks the one-shot or the streaming kernel as in the product (MIS_QGEMM_V2).
 *   gemm_pf: X bf16 [M][K] row-major, epi 0 f32 [M][cols], 1 h = T(h + T(x W^T)) on the given h bf16 [M][cols], 2 silu(gate) * up [M][cols / 2]. */
mis_status mis_debug_gemm_skinny(int device, const uint16_t* W, const uint16_t* W2, const uint16_t* X, const uint16_t* bias, int M, int N, int K,
                                 int epi, int R, int ksb, int U, int S, float* out, int64_t capacity, int32_t* report);
mis_status mis_debug_gemm_skinny_q(int device, int bits, int sb_dtype, const uint32_t* wq, const uint16_t* scales, const uint16_t* biases,
                                   const uint32_t* wq2, const uint16_t* scales2, const uint16_t* biases2, const uint16_t* X, const uint16_t* bias,
                                   int M, int N, int K, int epi, int R, int ksb, int S, float* out, int64_t capacity, int32_t* report);
mis_status mis_debug_gemm_pf(int device, const uint16_t* W, const uint16_t* W2, const uint16_t* X, const uint16_t* h, int M, int N, int K, int epi,
                             float* out, int64_t capacity, int32_t* report);

/* csrc/attn_debug.hip, tests (tests/test_gpu_attn_ops.py): ONE call of launch_attn_decode (csrc/lm_kernels.hip: k_attn_decode<D, NIT, XS, QP>
 * or k_attn_decode2<NS>) on caller-supplied host data.  The fields carry the names and meanings of AttnParams (csrc/lm_kernels.h); 16-bit
 * operands are raw payloads (uint16), NULL where AttnParams allows null.  The K and V^T caches are passed as raw IMAGES in the kernels'
 * tiled layout (K [rows][Hkv][Smax/32][2][D/32][64][8], V^T [rows][Hkv][Smax/32][D/16][64][8], rows = cache_rows or batch) and uploaded
 * unchanged - the caller decides what sits past kv_len; kcache_out / vtcache_out receive the images after the launch.  qp_w (QP launches
 * only) is the row-major W_q bf16 [H D][H D], packed by launch_pack_weight; qp_KT is passed to the launcher as given.
 * The attention output, qp_h_out and both caches lie between guard bands of the byte 0xFF (a NaN in bf16), and the output and qp_h_out
 * bodies are pre-filled with it: an element never written comes back as NaN, a changed guard byte fails the call with
 * MIS_ERR_GENERATION_FAILED, and a key read behind row rows - 1 of a cache is a NaN.  Every other input is followed by NaN (pos and
 * active, which have no NaN: zeros, i.e. inactive rows at position 0), both RoPE tables included.  A shape the launcher rejects returns
 * the launcher's status and launches nothing.
 *   out f32 [Mpad][H D]: the output, un-packed with xpk_index when out_ld == 0, else the first H D columns of each row of out_ld (>= H D;
 *     the columns behind must stay untouched); rows the kernel did not write (inactive, >= batch, append_only) are NaN.
 *   qp_h_out uint16 [batch][H D] (QP launches; 0xFFFF where never written).
 *   report (may be NULL) int32[6]: kernel (0 k_attn_decode, 1 k_attn_decode2; -1 nothing launched), D, NIT, XS, QP, NS. */
typedef struct mis_debug_attn_args {
    int32_t batch, Mpad, S, Nqkv, H, Hkv, D, Smax;
    int32_t cache_rows, append_only, first_schedule, cross, cross_len, out_ld, rope_in_dtype;
    int32_t qp_S, qp_KT;
    float scale, qk_eps, qp_eps;
    const float* qkv_part;                       /* [S][Mpad][Nqkv] (NULL with qp_w) */
    const int32_t* pos;                          /* [Mpad] */
    const uint8_t* active;                       /* [Mpad] */
    const float *rope_cos, *rope_sin;            /* [Smax][D/2] or NULL */
    const uint16_t *qnorm_w, *knorm_w;           /* bf16 [D] or NULL */
    const uint16_t* qp_w;                        /* bf16 [H D][H D] row-major or NULL */
    const uint16_t* qp_bias;                     /* bf16 [H D] or NULL */
    const float* qp_slabs;                       /* [qp_S][Mpad][H D] */
    const uint16_t *qp_h_in, *qp_lnw, *qp_lnb;   /* bf16 [Mpad][H D], [H D], [H D] */
    const uint16_t *kcache, *vtcache;            /* images, rows x Hkv x Smax x D elements each */
    uint16_t *kcache_out, *vtcache_out;
    float* out;
    uint16_t* qp_h_out;
    int32_t* report;
} mis_debug_attn_args;
mis_status mis_debug_attn_decode(int device, const mis_debug_attn_args* args);

/* csrc/codec_debug.hip, tests (tests/test_gpu_codec_ops.py): ONE call of a codec launcher (csrc/codec_kernels.h) on caller-supplied host
 * data; nothing is computed in the entry points.  Guards as for the GEMM and attention entry points above: every output lies between
 * guard bands and is pre-filled with the byte 0xFF (a float NaN; code -1): an element never written comes back as that, a changed guard
 * byte - or a changed padding column of a strided output - fails the call with MIS_ERR_GENERATION_FAILED.  Every input is followed (the
 * activations: also preceded) by NaN, and the padding columns of a strided input are NaN, so an over-read shows in the result; codes are
 * followed by 0xFF bytes.  The entry points refuse (MIS_ERR_INVALID_INPUT) what would make a KERNEL read or write out of bounds; what a
 * launcher checks itself is left to it: its status is returned and nothing is launched.
 *
 * codec_gemm: launch_gemm(mode, snake, GemmParams, batch).  The fields carry the names and meanings of GemmParams; ldx / ldy 0 = dense.
 *   mode 0 PLAIN, 1 RESID, 2 NOISE, 3 CONVT, 4 GELU, 5 TAPS.  use_pack 0: pack = NULL and no CodecPackScope (the exact-f32 kernels);
 *   1: a fresh CodecPack owned by the call (the split-bf16 path where the launcher's shape rule and the MIS_BF3_* / MIS_CODEC_EXACT_F32
 *   environment, read per launch, allow it).
 *   X  [batch][Kx][hist + Tin] dense, hist = max(-x_lo, 0) history columns in front of column 0 (Kx = K; CONVT / TAPS: Cin); uploaded with
 *      row stride ldx (>= hist + Tin), column 0 of every row 16-byte aligned when ldx is a multiple of 4, all other columns NaN.
 *   R  [batch][M][Tout] dense or NULL, uploaded with row stride ldy (padding NaN).  noise [batch][N] or NULL; row_ids [batch] or NULL.
 *   AT [K][M] (CONVT: [s][K][M]); bias, scale [M] or NULL; alpha, ralpha [Kx] or NULL.
 *   Y  [batch][M][Tout] dense: the first Tout columns of every row of ldy.
 *   report (may be NULL) int32[6]: kernel (0 k_snac_gemm, 1 k_conv_taps, 2 k_pw_fused, 3 k_bf3_gemm; -1 nothing launched), ntaps, NQ,
 *   ksplit, Tp, Cp (the last four: split-bf16 launches only).
 * codec_final: launch_codec_final.  x [batch][C][hist + T] dense (hist = max(-x_lo, 0)), uploaded with row stride ld; w [k][C]; a, ra [C] or
 *   both NULL (ELU); out [batch][T]: the first T columns of every row of out_stride.
 * codec_hist: launch_codec_hist.  st [batch][C][H] and the image x_img [batch][C][ld] (H columns of head room, then Tn new columns, then
 *   padding: the launcher gets x_img + H) go in and come back (st_out, x_out) as the launch left them.
 * codec_embed: launch_codec_embed.  codes int32 [n_codes] addressed through cs_b / cs_q / cs_t (>= 0); tables [nq][bins][C]; h [batch][C][T]:
 *   the first T columns of every row of ld.
 * codec_dw7: launch_dw7.  X, Y [batch][C][T]; w7 [C][7]; bias [C]; dil 1 .. 9 (the kernel's halo).
 * codec_vq_nearest: launch_vq_nearest.  ze [batch][CD][Tm]; cn [CB][CD]; cn2 [CB]; codes_out int32 [batch][Tm]. */
typedef struct mis_debug_codec_gemm_args {
    int32_t mode, snake, batch, use_pack;
    int32_t M, K, N, Tin, Tout, s, pad, Cin, ldx, ldy, x_lo, dup_bias_n0, split_k_ok, taps, dil, noise_rng;
    uint64_t noise_key;
    int64_t row_offset;
    const float *AT, *bias, *X, *R, *scale, *noise, *alpha, *ralpha;
    const int32_t* row_ids;
    float* Y;
    int32_t* report;
} mis_debug_codec_gemm_args;
mis_status mis_debug_codec_gemm(int device, const mis_debug_codec_gemm_args* args);
mis_status mis_debug_codec_final(int device, const float* x, const float* w, float bias, const float* a, const float* ra, int C, int T, int ld,
                                 int x_lo, int k, int batch, int64_t out_stride, float* out);
mis_status mis_debug_codec_hist(int device, const float* st, const float* x_img, int C, int ld, int H, int Tn, int batch, float* st_out,
                                float* x_out);
mis_status mis_debug_codec_embed(int device, const int32_t* codes, int64_t n_codes, int64_t cs_b, int64_t cs_q, int64_t cs_t,
                                 const float* tables, int nq, int bins, int C, int ld, int T, int batch, float* h);
mis_status mis_debug_codec_dw7(int device, const float* X, const float* w7, const float* bias, int batch, int C, int T, int dil, float* Y);
mis_status mis_debug_codec_vq_nearest(int device, const float* ze, const float* cn, const float* cn2, int batch, int CD, int CB, int Tm,
                                      int32_t* codes_out);

/* csrc/enc_debug.hip, tests (tests/test_gpu_enc_ops.py): ONE call of a launcher of csrc/whisper_kernels.h - the Whisper / Smart Turn encoder
 * chain, Moonshine's encoder GEMMs, the decoders' cross-K/V projection - on caller-supplied host data; nothing is computed in the entry
 * points.  16-bit operands and results are raw bf16 payloads (uint16).  Guards as above: every output lies between guard bands and is
 * pre-filled with the byte 0xFF, so an element never written comes back as 0xFFFF, and a changed guard byte - or a changed padding column
 * of a strided output - fails the call with MIS_ERR_GENERATION_FAILED; every input is followed by NaN and the columns of a strided input
 * that the launch has no business with are NaN.  The entry points refuse (MIS_ERR_INVALID_INPUT) what would make a KERNEL read or write
 * outside these buffers; what a launcher checks itself is left to it: its status is returned and nothing is launched.
 *   gemm_big: launch_gemm_big(epi, BigGemmParams).  X is the IMAGE the kernels address, (M - 1) ldx + K elements with row m at m ldx - rows
 *     overlap when ldx < K (Moonshine's conv2 / conv3), and with ldx > K the columns between two rows are replaced by NaN; exactly that many
 *     elements are uploaded, which is also what the clamped staging rows of k_gemm_big2 / 3 reach.  W [N][K]; bias [N] or NULL; R [M][N]
 *     (epi 2, BG_RESID) or [pos_rows][N] (epi 3, BG_GELU_POS); C_out [M][N].  report (may be NULL) int32[4]: kernel (0 k_gemm_big,
 *     1 k_gemm_big2, 2 k_gemm_big3; -1 nothing launched), epilogue, wave grid WM, WN.  MIS_GEMM_BIG3 is read per launch.
 *   enc_layernorm: launch_layernorm.  x, y_out [rows][d]; w, b [d].  report int32[1]: 0 k_layernorm, 1 k_layernorm8.
 *   enc_im2col3: launch_im2col3_f32 / _bf16.  in [B][Tin][C] float (in_is_f32) or bf16; out [B Tout][3 C].
 *   enc_scatter_kv: launch_scatter_kv.  src [B T][ld], of which only the K columns kcol0 .. + H D and the V columns vcol0 .. + H D are
 *     uploaded (the others: NaN); kc_out / vc_out: the WHOLE images [B][H][Spad D], 0xFFFF where nothing was written.
 *   enc_attn_prefill: launch_attn_prefill.  q [B T][H D] dense, uploaded with row stride ldq (a multiple of 8); kc_img / vc_img [B][H][Spad D]
 *     uploaded unchanged, as mis_debug_attn_decode does - the caller decides what sits behind T; out [B T][H D]: the first H D columns of
 *     every row of ldo.  report int32[2]: kernel (0 k_attn_prefill, 1 k_attn_prefill2), D.  MIS_ATTN_PREFILL_V1 is read per launch.
 *   whisper_embed_ln: launch_whisper_embed_ln.  emb [vocab][d], pos_emb [max_pos][d], ids, active, pos_cur, pos_next [batch] (the two position
 *     arrays go in and come back; pos_next >= 0), lw, lb [d]; h_out [Mpad][d], x_out the packed image of Mpad d elements (xpk layout; d a
 *     multiple of 32, Mpad of 16).
 *   whisper_suppress: launch_whisper_suppress.  logits [batch][Vpad] go in and come back; sup [n_sup], bsup [n_bsup], n_gen [batch], active
 *     [batch] or NULL. */
mis_status mis_debug_gemm_big(int device, int epi, const uint16_t* X, const uint16_t* W, const uint16_t* bias, const uint16_t* R, int M, int N, int K,
                              int ldx, int pos_rows, uint16_t* C_out, int32_t* report);
mis_status mis_debug_enc_layernorm(int device, const uint16_t* x, const uint16_t* w, const uint16_t* b, int rows, int d, float eps, uint16_t* y_out,
                                   int32_t* report);
mis_status mis_debug_enc_im2col3(int device, const void* in, int in_is_f32, int B, int Tin, int C, int Tout, int stride, uint16_t* out);
mis_status mis_debug_enc_scatter_kv(int device, const uint16_t* src, int ld, int kcol0, int vcol0, int B, int T, int H, int D, int Spad,
                                    uint16_t* kc_out, uint16_t* vc_out);
mis_status mis_debug_enc_attn_prefill(int device, const uint16_t* q, int ldq, const uint16_t* kc_img, const uint16_t* vc_img, int B, int T, int H, int D,
                                      int Spad, int ldo, uint16_t* out, int32_t* report);
mis_status mis_debug_whisper_embed_ln(int device, const uint16_t* emb, const uint16_t* pos_emb, const int32_t* ids, const uint8_t* active,
                                      int32_t* pos_cur, int32_t* pos_next, const uint16_t* lw, const uint16_t* lb, int d, int vocab, int max_pos,
                                      int batch, int Mpad, uint16_t* h_out, uint16_t* x_out);
mis_status mis_debug_whisper_suppress(int device, uint16_t* logits, int Vpad, int vocab, const int32_t* sup, int n_sup, const int32_t* bsup, int n_bsup,
                                      const int32_t* n_gen, const uint8_t* active, int batch);

/* csrc/glue_debug.hip, tests (tests/test_gpu_glue_ops.py): ONE call of a launcher of the LM glue (csrc/lm_kernels.h) on caller-supplied host
 * data; nothing is computed in the entry points.  16-bit operands and results are raw bf16 payloads (uint16).  Guards as above: every output
 * lies between guard bands and is pre-filled with the byte 0xFF (0xFFFF in bf16, -1 as an integer), a changed guard byte fails the call with
 * MIS_ERR_GENERATION_FAILED; every input is followed by NaN (ids: 0x7FFFFFFF; prompts and lens: zeros; bytes: 0xFF).  The entry points
 * refuse (MIS_ERR_INVALID_INPUT) only what would make a KERNEL read or write outside these buffers; what a launcher refuses is returned as
 * its status and nothing is launched.
 *   lm_embed_rmsnorm: launch_embed_rmsnorm.  emb [vocab][d], ids, active, pos_cur, pos_next [batch] (the two position arrays go in and come
 *     back), wnorm [d]; h_out [Mpad][d]; x_out the packed image (xpk layout) of Mpad round_up(d, 32) elements.
 *     TOKEN IDS: an id outside 0 .. vocab - 1 is not part of any model's contract - every host entry point that takes ids (mis_tts_generate,
 *     mis_lm_prefill, mis_lm_forward, the token engine) rejects it with MIS_ERR_INVALID_INPUT before a launch, so neither kernel meets one
 *     in the product.  What the kernels do with one is therefore only a memory-safety rule, pinned as it is: k_embed_rmsnorm reads
 *     embedding row 0 (as it does for the rows batch .. Mpad - 1), k_pf_embed_rmsnorm writes a zero row.
 *   lm_glue: launch_reduce_residual_rmsnorm.  slabs f32 [S][Mpad][N]; h [Mpad][N] goes in and comes back; wnorm [N]; ln_bias [N] or NULL
 *     (RMSNorm); x_out the packed image of Mpad round_up(N, 32) elements - the columns N .. of the last k-tile are never written (0xFFFF).
 *     report (may be NULL) int32[4]: kernel (0 k_reduce_residual_rmsnorm, 1 k_glue4, 2 k_glue_cpt; -1 nothing launched), SG, CPT, threads per block.
 *   gemm_skinny_norm: launch_gemm_skinny_norm at Mpad = 16.  W bf16 [N_out][K] row-major, packed by launch_pack_weight; slabs f32
 *     [S_in][16][K]; h_in [16][K]; wnorm, ln_bias (NULL: RMSNorm) [K]; bias [N_out] or NULL.  out f32 as mis_debug_gemm_skinny returns it
 *     (packed epilogues un-packed into [16][N_out]); h_out [16][K] is a buffer of its own, pre-filled: rows >= nrows stay 0xFFFF;
 *     h_in_after (may be NULL) [16][K]: h_in as the launch left it.  report int32[5]: kernel (3 k_gemm_skinny_norm; -1 nothing launched),
 *     epilogue, LN, SG, KW.  gemm_skinny_norm_ok: the launcher's capability check (1 / 0).
 *   pf_rows: mode 0 launch_pf_embed_rmsnorm (table = emb [vocab][d], prompt [batch][Lmax] left padded, lens [batch]), 1 launch_pf_rows_rmsnorm
 *     (table = rows [Lmax][src_rows][d]), 2 launch_pf_rmsnorm (h [Tc Mpad][d] -> x), 3 launch_pf_add_resid (h [n] += part [n]),
 *     4 launch_pf_pack_rows (h [Mpad][d] -> x the packed image of Mpad round_up(d, 32) elements).  Modes 0 / 1 write h, x [Tc Mpad][d] and
 *     pos_tab (int32), act_tab (uint8) [Tc Mpad] for the chunk t0 .. t0 + Tc - 1 (inside 0 .. Lmax; 0 <= lens <= Lmax).  h, x, pos_tab and
 *     act_tab come back whole; arguments a mode does not use may be NULL / 0.
 *   prefill_feed: launch_prefill_feed.  step_counter int32[1] goes in and comes back; ids_out int32 [batch], active_out uint8 [batch].
 *   convert_to_bf16: launch_convert_to_bf16, src of dtype (mis_dtype) MIS_F32 / MIS_F16 / MIS_BF16, n elements.
 *   dequant_affine: launch_dequant_affine.  wq uint32 [N][K bits / 32]; scales, biases [N][K / group] of sb_dtype MIS_F32 / MIS_F16 / MIS_BF16;
 *     dst_out bf16 [N][K]. */
mis_status mis_debug_lm_embed_rmsnorm(int device, const uint16_t* emb, const int32_t* ids, const uint8_t* active, int32_t* pos_cur, int32_t* pos_next,
                                      const uint16_t* wnorm, int d, int vocab, float eps, int batch, int Mpad, uint16_t* h_out, uint16_t* x_out);
mis_status mis_debug_lm_glue(int device, const float* slabs, int S, int Mpad, int N, uint16_t* h, const uint16_t* wnorm, const uint16_t* ln_bias,
                             float eps, uint16_t* x_out, int32_t* report);
int32_t mis_debug_gemm_skinny_norm_ok(int epi, int R, int KT, int S, int S_in, int Mpad, int nrows, int layer_norm);
mis_status mis_debug_gemm_skinny_norm(int device, const uint16_t* W, const float* slabs, int S_in, const uint16_t* h_in, const uint16_t* wnorm,
                                      const uint16_t* ln_bias, float eps, int nrows, int epi, int R, int S, const uint16_t* bias, int N_out, int K,
                                      float* out, int64_t capacity, uint16_t* h_out, uint16_t* h_in_after, int32_t* report);
mis_status mis_debug_pf_rows(int device, int mode, const uint16_t* table, const int32_t* prompt, const int32_t* lens, int Lmax, int t0, int Tc, int batch,
                             int Mpad, int vocab, int src_rows, const uint16_t* wnorm, const float* part, int64_t n, int d, float eps, uint16_t* h,
                             uint16_t* x, int32_t* pos_tab, uint8_t* act_tab);
mis_status mis_debug_prefill_feed(int device, const int32_t* prompt, const int32_t* lens, int Lmax, int32_t* step_counter, int batch, int32_t* ids_out,
                                  uint8_t* active_out);
mis_status mis_debug_convert_to_bf16(int device, const void* src, int dtype, int64_t n, uint16_t* dst_out);
mis_status mis_debug_dequant_affine(int device, const uint32_t* wq, const void* scales, const void* biases, int sb_dtype, int N, int K, int group, int bits,
                                    uint16_t* dst_out);

/* csrc/lasr.hip, tests (tests/test_gpu_lasr_ops.py): ONE call of ls_gemm, or one launch line of the LASR chain (k_lasr_ln, k_lasr_rope,
 * k_lasr_attn, k_lasr_glu_dwconv, k_lasr_im2col, k_lasr_pack, k_lasr_argmax, k_lasr_collapse - the kernels are private to csrc/lasr.hip, so
 * the entry points live at its end), on caller-supplied host data; nothing is computed in the entry points.  16-bit operands and results
 * are raw bf16 payloads (uint16).  Guards as above: every output lies between guard bands and is pre-filled with the byte 0xFF (0xFFFF in
 * bf16, -1 as an integer), a changed guard byte - or a changed padding column of a strided output - fails the call with
 * MIS_ERR_GENERATION_FAILED; every input is followed by NaN (ints and row counts: 0x7FFFFFFF).  The entry points refuse
 * (MIS_ERR_INVALID_INPUT) only what would make a KERNEL read or write outside these buffers; a shape ls_gemm refuses is returned as its
 * status (MIS_ERR_GENERATION_FAILED) and nothing is launched.  Row counts: cnt[r] frames of every Tp rows are live, NULL = all.
 *   lasr_gemm: ls_gemm.  epi 0 LG_BIAS, 1 LG_RELU, 2 LG_SILU, 3 LG_AXPBY, 4 LG_F32.  X is the IMAGE the kernel addresses, (M - 1) ldx + K
 *     elements with row m at m ldx; with ldx > K the columns between two rows are replaced by NaN.  W [N][K]; bias [N] or NULL; R [M][N]
 *     (LG_AXPBY) or NULL; cnt [ceil(M / Tp)] or NULL.  in_place (LG_AXPBY): the output buffer is loaded with R and passed as the residual too,
 *     as the chain's FF1 / attention / conv calls do; else R is a buffer of its own (the FF2 call) and R_after (may be NULL) [M][N] receives
 *     it as the launch left it.  tile 0: the launcher's rule, 2 / 4: the 64- / 128-tile whatever the grid.  C_out bf16 [M][N], LG_F32: float
 *     [M][N].  report (may be NULL) int32[2]: epilogue (-1: nothing launched), TI (2 / 4).
 *   lasr_ln: x, y_out [M][d] (d even), w, b [d]; cnt [ceil(M / Tp)] or NULL.
 *   lasr_rope: rows [M][ld] go in and come back whole; heads 0 .. nheads - 1 of 64 columns are rotated with row m % Tp of cs / sn [Tp][32].
 *   lasr_attn: qkv [B Tp][ld] uploaded as given (q heads | k heads | v heads from column 0; the caller decides what sits behind cnt[b] and
 *     in the padding columns; ld a multiple of 8); out [B Tp][H 64]: the first H 64 columns of every row of ldo.
 *   lasr_glu_dwconv: act 0 SiLU, 1 ReLU.  pw [B Tp][2 C], taps [k][C], shift [C], cnt [B], 1 <= k <= 64; out [B Tp][C].  report int32[1]: act.
 *   lasr_im2col: in [B][Tin][C] (C a multiple of 8), cnt [B]; out [B Tout][ks C].  A live frame must read inside its own row:
 *     (min(cnt[b], Tout) - 1) st + ks <= Tin.
 *   lasr_pack: feats float [B][Fp][mels], F [B]; out [B Fp][Kp], Kp >= mels.
 *   lasr_argmax: logits float [M][V]; pred int32 [M].
 *   lasr_collapse: pred [B][Tp], cnt [B]; tokens int32 [B][Tp] comes back whole (-1: never written), ntok [B]. */
mis_status mis_debug_lasr_gemm(int device, int epi, const uint16_t* X, const uint16_t* W, const uint16_t* bias, const uint16_t* R, float a, float b,
                               const int32_t* cnt, int Tp, int in_place, int tile, int M, int N, int K, int ldx, void* C_out, uint16_t* R_after,
                               int32_t* report);
mis_status mis_debug_lasr_ln(int device, const uint16_t* x, const uint16_t* w, const uint16_t* b, int M, int d, float eps, const int32_t* cnt, int Tp,
                             uint16_t* y_out);
mis_status mis_debug_lasr_rope(int device, uint16_t* rows, int M, int ld, int nheads, int Tp, const float* cs, const float* sn);
mis_status mis_debug_lasr_attn(int device, const uint16_t* qkv, int ld, int H, int Hkv, const int32_t* cnt, int B, int Tp, float scale, int ldo,
                               uint16_t* out);
mis_status mis_debug_lasr_glu_dwconv(int device, int act, const uint16_t* pw, const float* taps, const float* shift, const int32_t* cnt, int B, int Tp,
                                     int C, int k, uint16_t* out, int32_t* report);
mis_status mis_debug_lasr_im2col(int device, const uint16_t* in, const int32_t* cnt, int B, int Tin, int Tout, int C, int ks, int st, uint16_t* out);
mis_status mis_debug_lasr_pack(int device, const float* feats, const int32_t* F, int B, int Fp, int mels, int Kp, uint16_t* out);
mis_status mis_debug_lasr_argmax(int device, const float* logits, int M, int V, int32_t* pred);
mis_status mis_debug_lasr_collapse(int device, const int32_t* pred, const int32_t* cnt, int B, int Tp, int blank, int32_t* tokens, int32_t* ntok);

/* csrc/sortformer.hip, tests (tests/test_gpu_sortformer_ops.py): ONE call of sf_gemm / sf_attn - the launchers the chain itself calls -, or
 * one launch line of the Sortformer chain (k_sf_conv0, k_sf_stats, k_sf_ln, k_sf_intake, k_sf_glu_dwconv, k_sf_peak - private to
 * csrc/sortformer.hip, so the entry points live at its end), on caller-supplied host data; nothing is computed in the entry points.  Every
 * tensor is float32; outputs come back as the launch left them, so a word nobody wrote is still 0xFFFFFFFF.  Guards as above: every output
 * lies between guard bands and is pre-filled with the byte 0xFF, a changed guard byte - or a changed padding column of a strided output -
 * fails the call with MIS_ERR_GENERATION_FAILED; every input is followed by NaN (row counts: 0x7FFFFFFF) and uploaded UNCHANGED: the
 * caller decides what sits in padding columns, behind a row's count and in unused table rows.  The entry points refuse
 * (MIS_ERR_INVALID_INPUT, nothing launched) only what would make a KERNEL read or write outside these buffers.
 *   sortformer_gemm: the fields of SfGemm plus batch.  load 0 plain, 1 LayerNorm, 2 ReLU, 3 depthwise 3 x 3 stride 2; act 0 none, 1 SiLU,
 *     2 ReLU, 3 sigmoid.  rows = batch Tp rowmul.  X is the IMAGE the kernel addresses: (rows - 1) ldx + K elements (load 3:
 *     [batch][Tin][Fin][K] channels last, ldx unused).  W [N][K]; bias [N] or NULL; cnt [batch] or NULL (every row live); stats [rows][2],
 *     lnw, lnb [K] (load 1); pos [Tp][N] or NULL; cnt_in [batch], dww [9][K], dwb [K] (load 3).  R NULL: no residual.  in_place: R dense
 *     [rows][N] is loaded into the output buffer, which is passed as the residual too (the Conformer calls); else R is the image
 *     (rows - 1) ldr + N of a buffer of its own (the BART calls) and R_after (may be NULL) receives it as the launch left it.  Y_out
 *     [rows][N]: the first N columns of every row of ldy.  report (may be NULL) int32[1]: load (-1: nothing launched).
 *   sortformer_attn: the fields of SfAttn plus heads and batch; rel 0 / 1 picks k_sf_attn<ND, false / true>.  qkv [batch Tp][ld]: q of head
 *     h at column h hd, k at koff + h hd, v at voff + h hd.  u, v [heads hd], P [2 Tcap - 1][ldp] (rel).  hd 1 .. 64.  out [batch Tp][heads hd]:
 *     the first columns of every row of ldo.  report int32[2]: ND (1 iff hd <= 32), REL; -1: nothing launched.
 *   sortformer_conv0: feats [batch][Fp][mels], F, T1 [batch], w [9][C], bias [C]; out [batch][T1p][F1][C].
 *   sortformer_stats: x [M][d]; stats_out [M][2] = mean, 1 / sqrt(var + eps).
 *   sortformer_ln: x, y_out [M][d], w, b [d], cnt [ceil(M / Tp)]; in_place: x is loaded into the output buffer and normalised there.
 *   sortformer_intake: x, y_out [batch Tp][d], cnt [batch]: y = x g.
 *   sortformer_glu_dwconv: pw [batch Tp][2 C], taps [k][C], shift [C], cnt [batch], 1 <= k <= 31; out [batch Tp][C].
 *   sortformer_peak: pcm [batch][stride], N [batch] (each <= stride); scale_out [batch]. */
mis_status mis_debug_sortformer_gemm(int device, int load, int act, const float* X, int ldx, const float* W, const float* bias, const int32_t* cnt, int batch,
                                     int Tp, int rowmul, int K, int N, int ldy, const float* stats, const float* lnw, const float* lnb, const float* R,
                                     int ldr, float ra, int in_place, const float* pos, const int32_t* cnt_in, int Tin, int Fin, int Fout, const float* dww,
                                     const float* dwb, float* Y_out, float* R_after, int32_t* report);
mis_status mis_debug_sortformer_attn(int device, int rel, const float* qkv, int ld, int koff, int voff, const int32_t* cnt, int batch, int Tp, int heads,
                                     int hd, float qscale, float sdk, const float* u, const float* v, const float* P, int ldp, int Tcap, int ldo, float* out,
                                     int32_t* report);
mis_status mis_debug_sortformer_conv0(int device, const float* feats, const int32_t* F, const int32_t* T1, const float* w, const float* bias, int batch,
                                      int Fp, int mels, int T1p, int F1, int C, float* out);
mis_status mis_debug_sortformer_stats(int device, const float* x, int M, int d, float eps, float* stats_out);
mis_status mis_debug_sortformer_ln(int device, const float* x, const float* w, const float* b, int M, int d, float eps, const int32_t* cnt, int Tp,
                                   int in_place, float* y_out);
mis_status mis_debug_sortformer_intake(int device, const float* x, const int32_t* cnt, int batch, int Tp, int d, float g, float* y_out);
mis_status mis_debug_sortformer_glu_dwconv(int device, const float* pw, const float* taps, const float* shift, const int32_t* cnt, int batch, int Tp, int C,
                                           int k, float* out);
mis_status mis_debug_sortformer_peak(int device, const float* pcm, int64_t stride, const int32_t* N, int batch, int on, float* scale_out);

/* csrc/token_engine.hip (round 5): a whole batch-1 request in ONE persistent launch on the compute units of `xcds` (1, 2, 4 or 8) XCDs,
 * streaming the handle's own packed weights; compiled for Soprano-80M's LM widths (other shapes: MIS_ERR_INVALID_INPUT).  The product
 * reaches it through mis_soprano_generate at batch 1; this entry point is for tests and measurements.
 *   sampling == NULL (laboratory form): `n_prompt` prompt positions, then `n_new` arg-max steps; next_tokens[t] = arg-max id after position
 *     t for EVERY t < n_prompt + n_new, logits_out [n_prompt + n_new][vocab], hidden_out [n_prompt + n_new][hidden] (final-norm output).
 *   sampling != NULL (generate form, the semantics of the Soprano loop, Soprano.swift:801-885): a token after the last prompt position and
 *     after every generated one until `stop_id` or n_new ids - arg-max when sampling->temperature == 0, else "mis-sampler-v1" behind the
 *     Soprano repetition penalty (repetition_penalty over the last repetition_context generated ids, seed, row_offset); next_tokens[t] is
 *     set for t >= n_prompt - 1 (the prompt but its last position runs through the launch chain's batched prefill, whose K/V the engine
 *     imports - as in the product); logits_out row k = the logits the k-th token was drawn from; hidden_out row k = position n_prompt - 1 + k.
 * counts (may be NULL): [0] positions processed, [1] ids chosen.  logits_out / hidden_out may be NULL; ms_out = device time of the launch.
 * Host pointers. */
mis_status mis_debug_token_engine(mis_tts* lm, const int32_t* prompt, int n_prompt, int n_new, int xcds, const mis_gen_params* sampling,
                                  int stop_id, int32_t* next_tokens, float* logits_out, float* hidden_out, int32_t* counts, double* ms_out);

/* csrc/marvis.hip, tests.  forced_logits: the Marvis frame loop TEACHER-FORCED for F frames - the loop samples as usual but continues
 * from forced int32 [batch, F, Cb] (Cb = params->codebooks, or all) - returning logits_out f32 [batch, F, Cb, audio_vocab] of every
 * (frame, codebook) (frames past a row's end stay 0), sampled_out int32 [batch, F, Cb] (may be NULL: what the sampler chose) and
 * n_frames[batch] under the end rule applied to the forced codes (an all-zero frame ends the row and is not counted).
 * sample_logits: the loop's sampler (mis-sampler-v1, RNG step = frame * K + slot) on given logits f32 [batch, vocab] (rounded to bf16).
 * rope_tables: cos / sin f32 [n_pos, head_dim / 2] of CSMLlama3ScaledRoPE (host arithmetic only: no GPU needed). */
mis_status mis_debug_marvis_forced_logits(mis_marvis* c, const int32_t* tokens, const uint8_t* mask, const int32_t* prompt_lens, int P,
                                          int batch, const mis_marvis_params* params, const int32_t* forced, int F, float* logits_out,
                                          int32_t* sampled_out, int32_t* n_frames);
mis_status mis_debug_marvis_sample_logits(int device, const float* logits, int batch, int vocab, float temperature, float top_p,
                                          uint64_t seed, int64_t row_offset, int frame, int slot, int K, int32_t* tokens_out);
mis_status mis_debug_marvis_rope_tables(int head_dim, float theta, float factor, float low_freq_factor, float high_freq_factor,
                                        float old_context_len, int n_pos, float* cos_out, float* sin_out);

/* csrc/moonshine.hip, tests: stage outputs of the Moonshine stem for a ragged batch (arguments of mis_moonshine_encode).  stage 0 conv1 + tanh
 * (f32), 1 GroupNorm, 2 gelu(conv2), 3 gelu(conv3).  dims[0] frames per row as the engine lays the batch out, dims[1] channels; out f32
 * [batch, dims[0], dims[1]] (a row's own frames first) or NULL for the dims alone.  Leaves the handle without encoder output. */
mis_status mis_debug_moonshine_stem_tap(mis_moonshine* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int stage,
                                        float* out, int64_t capacity, int64_t* dims);
/* csrc/moonshine.hip, tests (tests/test_gpu_moonshine_ops.py): ONE launch of a private kernel of the Moonshine engine (GroupNorm: its chain of
 * four), through the launcher the engine itself calls, on caller-supplied host data; nothing is computed in the entry points.  16-bit operands
 * and results are raw bf16 payloads (uint16).  Guards as above: every output lies between guard bands and is pre-filled with the byte 0xFF, a
 * changed guard byte - or a changed padding column of a strided output - fails the call with MIS_ERR_GENERATION_FAILED; every input is followed
 * by NaN (ints: 0x7FFFFFFF).  What the kernels' contract excludes is refused with MIS_ERR_INVALID_INPUT and nothing is launched: K % 4, B > 64,
 * LayerNorm with K > 512, more than 1280 keys (MS_MAX_KEYS) or keys behind Tpad, pos >= Smax, Smax > 2048 (MS_MAX_POS), H % Hkv, a
 * cross-attention row without a key, a GroupNorm row without a frame, a conv1 frame that reads behind the row's stride.
 *   conv1: k_ms_conv1_tanh.  pcm float [B][stride], T1 [B] (0 .. T1pad), wT float [127][d]; out float [B][T1pad][d].
 *   groupnorm: k_ms_gn_partial<0>, <1>, k_ms_gn_final, k_ms_gn_apply as ms_encode_device chains them.  x float [B][T1pad][d] (the frames behind
 *     T1[b] are replaced by NaN), gw, gb float [d].  stage 0 stops behind pass 0, 1 behind pass 1, 2 runs the chain.  part0, part1 float
 *     [B][*nch_out] (room for ceil(T1pad d / 32768) chunks a row), stats float [2 B] (mean, rstd), y [B T1pad d + 8 d].
 *   rope: k_ms_rope_rows.  rows [M][ld] go in and come back whole; heads 0 .. nheads - 1 of 64 columns: the first rot columns are rotated
 *     with row m % Tpad of cs / sn float [Tpad][rot / 2].
 *   attn: kind 0 k_ms_attn_enc: q = qkv [B Tpad][ld] (q heads | k heads | v heads, ld a multiple of 8), out [B Tpad][H 64]: the first H 64
 *     columns of every row of ldo.  kind 1 k_ms_attn_self: q = qkv [B][(H + 2 Hkv) 64] of the new token, kc / vc [B][Hkv][Smax][64] go in
 *     and come back whole, cs / sn float [Smax][rot / 2]; out [B][H 64].  kind 2 k_ms_attn_cross: q [B][H 64], kv [B Tpad][2 Hkv 64] (K heads,
 *     then V heads); out [B][H 64].  T3 [B] (kinds 0, 2); arguments a kind does not use may be NULL / 0.
 *   gemv: k_ms_gemv<ln, epi>, epi 0 MS_BF16, 1 MS_RESID, 2 MS_GATE, 3 MS_F32; only the decoder's four instantiations (1, 0), (0, 1), (1, 2),
 *     (1, 3).  X [B][K], lnw [K], W [N][K] (MS_GATE: N = 2 F), bias [N] or NULL; out bf16 [B][N] (MS_RESID: goes in as h and comes back;
 *     MS_GATE: [B][F]; MS_F32: float).  report (may be NULL) int32[2]: (ln, epi) of the instantiation that ran, -1 when nothing was launched.
 *   embed: k_ms_embed.  emb [vocab][d], ids [B]; h [B][d].
 *   argmax_embed: k_ms_argmax_embed.  logits float [B][V]; active uint8 [B], n_gen [B], tokens [B][stride] and done_count [1] go in and come
 *     back; emb [V][d]; h [B][d]. */
mis_status mis_debug_moonshine_conv1(int device, const float* pcm, int64_t stride, const int32_t* T1, int B, int T1pad, int d, const float* wT,
                                     float* out);
mis_status mis_debug_moonshine_groupnorm(int device, const float* x, const int32_t* T1, int B, int T1pad, int d, const float* gw, const float* gb,
                                         int stage, float* part0, float* part1, float* stats, uint16_t* y, int32_t* nch_out);
mis_status mis_debug_moonshine_rope(int device, uint16_t* rows, int M, int ld, int nheads, int Tpad, int rot, const float* cs, const float* sn);
mis_status mis_debug_moonshine_attn(int device, int kind, const uint16_t* q, const uint16_t* kv, int ld, int H, int Hkv, const int32_t* T3, int B,
                                    int Tpad, float scale, int ldo, uint16_t* kc, uint16_t* vc, int Smax, int pos, int rot, const float* cs,
                                    const float* sn, uint16_t* out);
mis_status mis_debug_moonshine_gemv(int device, int ln, int epi, const uint16_t* X, const uint16_t* lnw, const uint16_t* W, const uint16_t* bias, int B,
                                    int K, int N, int F, void* out, int32_t* report);
mis_status mis_debug_moonshine_embed(int device, const uint16_t* emb, const int32_t* ids, int B, int d, int vocab, uint16_t* h);
mis_status mis_debug_moonshine_argmax_embed(int device, const float* logits, int B, int V, int eos, uint8_t* active, int32_t* n_gen, int32_t* tokens,
                                            int stride, int32_t* done_count, const uint16_t* emb, int d, uint16_t* h);

/* csrc/smartturn.hip, tests: tensors of the handle's last call, out f32 with room for `capacity` floats.  stage 0 prepared samples
 * [B, W] (of the last predict), 1 features [B, F, n_mels], 2 encoder output [B, T, d], 3 pooled [B, d]. */
mis_status mis_debug_smartturn_tap(mis_smartturn* c, int stage, float* out, int64_t capacity);
/* measurements: device milliseconds of the last call, ms[3] = prepare + mel, encoder, head.  Inside a graph replay encoder and head
 * are one interval: ms[1] holds it and ms[2] is -1. */
mis_status mis_debug_smartturn_timing(const mis_smartturn* c, float* ms);

/* csrc/ecapa_lid.hip, measurements: device milliseconds of the last call, ms[2] = front end (0 after forward_features), model */
mis_status mis_debug_ecapa_lid_timing(const mis_ecapa_lid* c, float* ms);

/* csrc/lasr.hip, measurements: ms NULL switches the timestamps of mis_stt_lasr_generate on; else device milliseconds of the last
 * generate, ms[3] = front end, encoder, tail */
mis_status mis_debug_lasr_timing(mis_lasr* c, float* ms);

/* csrc/fsmn_vad.hip, measurements: device milliseconds of the last call summed over its first 128 chunks, ms[2] = front end (copy in +
 * fbank), encoder (+ copy out) */
mis_status mis_debug_fsmn_vad_timing(const mis_fsmn_vad* c, float* ms);

/* csrc/sensevoice.hip, measurements: device milliseconds of the last generate / forward, ms[3] = front end (copy in + peak + fbank +
 * intake; 0 for forward_features), encoder, head (generate: the fused head + arg-max and the decode; forward: the head GEMM +
 * log-softmax summed over its first 64 chunks, copies excluded) */
mis_status mis_debug_sensevoice_timing(const mis_sensevoice* c, float* ms);
/* csrc/sensevoice.hip, tests (tests/test_gpu_sensevoice.py): ONE launch each on host data; inputs are followed by NaN (counts: 0x7FFFFFFF)
 * and every poisoned output lies between guard bands, as for the other operator entry points.
 *   sensevoice_attn: k_sv_attn<1 | 2 | 4> (hd <= 32 | 64 | 128).  qkv [batch Tp][ld]: q of head h at column h hd, k at koff + h hd, v at
 *     voff + h hd; cnt [batch] keys (= queries) of each row; q is multiplied by `scale` at the load.  out [batch Tp][ldo].
 *   sensevoice_head_argmax: k_sv_gemm<SV_ARGMAX> on X [batch Tp][K], W [N][K], bias [N] or NULL, cnt [batch] -> pmax_out / pidx_out
 *     [batch Tp][ceil(N / 64)]: per frame and 64-column tile the maximum and the lowest column attaining it (frames behind cnt stay
 *     0xFFFFFFFF).  A second launch, k_sv_decode, then combines what the first wrote: pred_out [batch Tp], tokens_out [batch Tp],
 *     ntok_out [batch], rich_out [batch 3] as mis_stt_sensevoice_generate forms them. */
mis_status mis_debug_sensevoice_attn(int device, const float* qkv, int ld, int koff, int voff, const int32_t* cnt, int batch, int Tp, int heads,
                                     int hd, float scale, int ldo, float* out);
mis_status mis_debug_sensevoice_head_argmax(int device, const float* X, const float* W, const float* bias, const int32_t* cnt, int batch, int Tp,
                                            int K, int N, float* pmax_out, int32_t* pidx_out, int32_t* pred_out, int32_t* tokens_out,
                                            int32_t* ntok_out, int32_t* rich_out);

/* csrc/silero_vad.hip, measurements: device milliseconds of the last call summed over its first 64 passes, ms[2] = front end (copy in +
 * the six contractions), recurrence */
mis_status mis_debug_silero_vad_timing(const mis_silero_vad* c, float* ms);

/* csrc/mossformer2.hip, measurements: device milliseconds of the last call, ms[3] = front end (copy in + fbank + deltas), mask network,
 * synthesis (+ copy out) */
mis_status mis_debug_mossformer2_timing(const mis_mossformer2* c, float* ms);

/* csrc/deepfilternet.hip, measurements: device milliseconds of the last call, ms[4] = front end (copy in + STFT + features), network
 * without the recurrences, the recurrence launches, synthesis (+ copy out) */
mis_status mis_debug_deepfilternet_timing(const mis_deepfilternet* c, float* ms);
/* csrc/deepfilternet_stream.hip, measurements: device milliseconds of the last feed, ms[2] = the whole feed (copies included), its
 * recurrence launches */
mis_status mis_debug_deepfilternet_stream_timing(const mis_deepfilternet_stream* s, float* ms);
/* feeds of at most `frames` targets run the short-chunk recurrence (0: never; negative: the default, 4) */
mis_status mis_debug_deepfilternet_stream_gru_step_frames(mis_deepfilternet_stream* s, int frames);

/* csrc/sortformer.hip, measurements: ms NULL switches the timestamps of mis_sortformer_forward on; else device milliseconds of the
 * last call, which must have been mis_sortformer_forward (MIS_ERR_NOT_INITIALIZED otherwise): ms[4] = front end, stem, Conformer blocks,
 * projection + BART layers + head */
mis_status mis_debug_sortformer_timing(mis_sortformer* c, float* ms);

/* csrc/bigvgan.hip, measurements: device milliseconds of the last decode's kernels (behind the copy in, before the copy out), ms[1] */
mis_status mis_debug_bigvgan_timing(const mis_bigvgan* c, float* ms);
/* csrc/bigvgan.hip, tests (tests/test_gpu_bigvgan.py): ONE launch of the anti-aliased activation k_bv_aa_act on host data.  x f32
 * [batch][channels][stride], counts[batch] columns of each row (1..stride), alpha / beta [channels] as the activation uses them (after
 * any exp(); 1 / (beta + 1e-9) is folded here as finalize folds it) -> out f32 [batch][channels][stride], zeros behind a row's own
 * columns.  Inputs are followed by NaN and the poisoned output lies between guard bands, as for the other operator entry points. */
mis_status mis_debug_bigvgan_aa_act(int device, const float* x, const int32_t* counts, int batch, int channels, int64_t stride,
                                    const float* alpha, const float* beta, float* out);

#ifdef __cplusplus
}
#endif
#endif /* MI_SPEECH_DEBUG_H */
