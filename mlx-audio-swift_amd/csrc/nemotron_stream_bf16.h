// nemotron_stream_bf16.h - the bf16 form of the stream session's Conformer blocks (nemotron_stream.hip's nms_pass in bf16 mode): include it
// behind nemotron_kernels.h.  Opt-in per session (mis_nemotron_stream_create_dtype with MIS_BF16) on a model finalized in bf16 mode; it runs
// on the bf16 matrices and ptab16 tables that model already holds.  The yardstick is the f32 session's, moved to bf16: a stream's block
// taps are those of the OFFLINE bf16 engine (nemotron_encoder_bf16.h) on the whole audio, bit for bit, for any split into feeds, any slot
// and any neighbours.  The precision contract is nemotron_encoder_bf16.h's, unchanged.  What makes the bits equal:
//   contraction  an output element is ONE f32 accumulator fed the k-slabs of 32 in ascending order through v_mfma_f32_16x16x32_bf16, with
//                k_pk_gemm_bf16's operand-load and epilogue expressions: the bits k_pk_gemm_bf16 gives it at either tile rule.  So the
//                dispatch may depend on the shape of the pass.
//   attention    k_nm_attn_bf16's wave (16 queries over all head dimensions, the same absolute 32-aligned key tiles walked upwards under
//                the same two compares); K and V come from a bf16 ring addressed by absolute frame % R.
//   conv         the k - 1 frames in front of a pass are the stream's carried bf16 pointwise_conv1 ROWS (a | gate, the same bytes as f32
//                gated frames would take): the gate is recomputed by the offline expression from the offline bits.  Zeros at frame 0 gate
//                to 0 = offline's causal pad.
//
// Kernels (resources off -Rpass-analysis=kernel-resource-usage for gfx950 with the flags the Makefile gives nemotron_stream.o, packed f32
// arithmetic off, hipcc of ROCm 7.2.0 = AMD clang 22.0.0git; without that flag the same compiler allots up to 8 VGPRs more or 2 fewer.
// None uses scratch under either):
//   k_nm_gemm_bf16_rows<LOAD, NW>   the short-pass contraction.  A pass's rows lie as [streams][Tq] with cnt[b] live ones each; a block's
//                16-row tile is the NEXT 16 LIVE ROWS OF THE WHOLE PASS across streams (64 streams of one frame: 4 tiles, not 64), found
//                from an inclusive prefix sum over the <= 64 counts that wave 0 forms with shuffles.  NW waves a block, wave w owns the 16
//                columns n0 + 16 w ..: W is the MFMA A operand, 16 bytes a lane straight into registers, four k-slabs (128 k) a step with
//                the next step in flight, every weight byte read once a block; the 16 staged rows go through LDS once per step (row
//                stride 136 elements) and are shared by the waves.  No K split and no reduction between waves.  Rows behind cnt[b] are
//                NOT written: nothing reads them (every consumer of big / qkv / att - this kernel, k_pk_gemm_bf16, the ring put, the
//                attention, the conv module, the taps - guards its rows by cnt[b]; h behind cnt[b] is zero from k_nm_intake_stream on).
//                NW 4 / 2 / 1 (64 / 32 / 16 columns): LDS 4688 bytes; VGPRs LN 76 / 88 / 104, bf16 56 / 64 / 76, LN + SiLU 76 / 92 / 110;
//                4 AGPRs; scratch 0.
//   k_nm_attn_stream_bf16<NS, QW>   QW waves = 16 QW queries x head x stream a block.  A pass has 1..3 C + 2 queries a stream: a session
//                whose pass capacity is <= 16 frames (every one-chunk-a-pass session up to right = 13) launches ONE wave a block - a second
//                wave would own no live query and only lengthen the staging barriers - and larger capacities launch 32 queries a block,
//                which halves the K / V / band staging a query.  The choice depends on the session's capacity alone; the bits do not
//                depend on it (a wave's online softmax sees only the partition of its keys into absolute tiles).  Ring rows in front of
//                the block's first visible key are staged as zeros (they may hold anything), as are band rows outside [dlo, dhi].
//                QW 1, NS 1 / 2 / 3 / 4: LDS 12224 / 19904 / 27584 / 35264 bytes, 81 / 104 / 120 / 152 VGPRs; QW 2: LDS 16768 / 25472 /
//                34176 / 42880 bytes, 86 / 104 / 120 / 152 VGPRs; both 16 / 20 / 24 / 32 AGPRs, scratch 0.
//   k_nm_glu_dwconv_ln_stream_bf16   k_nm_glu_dwconv_ln_bf16 at padl = k - 1 with hin [S][k - 1][2 C] where offline pads zeros; block 0 of a
//                stream writes hout = the last k - 1 rows of [hin ++ the pass's] (double-buffered by parity: a stream without frames
//                copies its history through).  LDS 11776 bytes, 69 VGPRs, scratch 0.
//   k_nm_ring_put_bf16   K | V of the pass's frames -> the ring rows (pos + i) % R, 16 bytes a thread.
#pragma once

#include "nemotron_encoder_bf16.h"

namespace {

enum { NMR_ROWS64 = 2, NMR_ROWS32, NMR_ROWS16 };                    // the short-pass rules behind PKB_TILE64 / PKB_TILE32: columns a block
constexpr int NMR_KS = 128, NMR_LDX = NMR_KS + 8, NMR_MAXB = 64;    // k a step; the staged row's stride (272 bytes); streams a pass

// ============================================================================ the short-pass contraction
// PkbGemm as k_pk_gemm_bf16 takes it, B <= 64 batch entries; grid (ceil(live rows / 16), ceil(N / 16 NW))
template <int LOAD, int NW>
__global__ void __launch_bounds__(64 * NW) k_nm_gemm_bf16_rows(PkbGemm p, int B) {
    constexpr int NT = 64 * NW, CH = 256 / NT;                      // chunks of 8 k a thread stages a step
    __shared__ __attribute__((aligned(16))) bf16_t Xs[16][NMR_LDX];
    __shared__ int pre[NMR_MAXB + 1], rowat[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int g0 = blockIdx.x * 16, n0 = blockIdx.y * 16 * NW;
    if (wave == 0) {                                                // pre[b + 1] = live rows of the entries 0 .. b
        int c = lane < B ? max(min(p.cnt[lane], p.Tp), 0) : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(c, o, 64);
            if (lane >= o) c += v;
        }
        pre[lane + 1] = c;
        if (lane == 0) pre[0] = 0;
    }
    __syncthreads();
    if (tid < 16) {                                                 // live row g0 + tid of the pass: entry b, frame g - pre[b]
        const int g = g0 + tid;
        int row = -1;
        if (g < pre[B]) {
            int b = 0;
            while (pre[b + 1] <= g) ++b;
            row = b * p.Tp + (g - pre[b]);
        }
        rowat[tid] = row;
    }
    __syncthreads();
    // staging: 16 rows x 128 k = 256 chunks of 16 B a step, chunk i = tid + NT j: row i >> 4, k offset 8 (i & 15)
    int xrow[CH];
    float mean[CH], rstd[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        xrow[j] = rowat[(tid + NT * j) >> 4];
        mean[j] = 0.0f; rstd[j] = 0.0f;
        if (LOAD != PKB_LOAD_BF16 && xrow[j] >= 0) { mean[j] = p.stats[2 * (size_t)xrow[j]]; rstd[j] = p.stats[2 * (size_t)xrow[j] + 1]; }
    }
    const int nrow = n0 + 16 * wave + l15;
    const bool wlive = nrow < p.N;
    const bf16_t* wsrc = p.W + (size_t)(wlive ? nrow : 0) * p.K + 8 * kq;
    bf16x8_t wreg[4];
    uint4 xreg[CH];
    auto load = [&](int k0) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            wreg[s] = (wlive && k0 + 32 * s < p.K) ? *reinterpret_cast<const bf16x8_t*>(wsrc + k0 + 32 * s) : (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int k = k0 + 8 * ((tid + NT * j) & 15);
            xreg[j] = make_uint4(0, 0, 0, 0);
            if (xrow[j] < 0 || k >= p.K) continue;
            const size_t at = (size_t)xrow[j] * p.ldx + k;
            // the three loads of k_pk_gemm_bf16, expression for expression: the staged operand has its bits
            if constexpr (LOAD == PKB_LOAD_LN_SILU) {
                const uint4 q = *reinterpret_cast<const uint4*>(p.Xb + at);
                const float4* w = reinterpret_cast<const float4*>(p.lnw + k);
                const float4* bb = reinterpret_cast<const float4*>(p.lnb + k);
                const float4 w0 = w[0], w1 = w[1], b0 = bb[0], b1 = bb[1];
                const float mu = mean[j], rs = rstd[j];
                float lo[4], hi[4];
                bf16x4_unpack(make_uint2(q.x, q.y), lo);
                bf16x4_unpack(make_uint2(q.z, q.w), hi);
                auto act = [&](float x, float wv, float bv) { const float v = fmaf((x - mu) * rs, wv, bv); return v / (1.0f + expf(-v)); };
                xreg[j].x = pkb_pack2(act(lo[0], w0.x, b0.x), act(lo[1], w0.y, b0.y));
                xreg[j].y = pkb_pack2(act(lo[2], w0.z, b0.z), act(lo[3], w0.w, b0.w));
                xreg[j].z = pkb_pack2(act(hi[0], w1.x, b1.x), act(hi[1], w1.y, b1.y));
                xreg[j].w = pkb_pack2(act(hi[2], w1.z, b1.z), act(hi[3], w1.w, b1.w));
            } else if (LOAD == PKB_LOAD_LN) {
                const float4* x = reinterpret_cast<const float4*>(p.Xf + at);
                const float4* w = reinterpret_cast<const float4*>(p.lnw + k);
                const float4* bb = reinterpret_cast<const float4*>(p.lnb + k);
                const float4 x0 = x[0], x1 = x[1], w0 = w[0], w1 = w[1], b0 = bb[0], b1 = bb[1];
                const float mu = mean[j], rs = rstd[j];
                xreg[j].x = pkb_pack2(fmaf((x0.x - mu) * rs, w0.x, b0.x), fmaf((x0.y - mu) * rs, w0.y, b0.y));
                xreg[j].y = pkb_pack2(fmaf((x0.z - mu) * rs, w0.z, b0.z), fmaf((x0.w - mu) * rs, w0.w, b0.w));
                xreg[j].z = pkb_pack2(fmaf((x1.x - mu) * rs, w1.x, b1.x), fmaf((x1.y - mu) * rs, w1.y, b1.y));
                xreg[j].w = pkb_pack2(fmaf((x1.z - mu) * rs, w1.z, b1.z), fmaf((x1.w - mu) * rs, w1.w, b1.w));
            } else {
                xreg[j] = *reinterpret_cast<const uint4*>(p.Xb + at);
            }
        }
    };
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    load(0);
    for (int k0 = 0; k0 < p.K; k0 += NMR_KS) {
        __syncthreads();                                            // the previous step's fragments are read
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int i = tid + NT * j;
            *reinterpret_cast<uint4*>(&Xs[i >> 4][8 * (i & 15)]) = xreg[j];
        }
        __syncthreads();
        const bf16x8_t w0 = wreg[0], w1 = wreg[1], w2 = wreg[2], w3 = wreg[3];
        if (k0 + NMR_KS < p.K) load(k0 + NMR_KS);
        const bf16_t* xf = &Xs[l15][8 * kq];                        // the slabs in ascending order, one MFMA a slab
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, *reinterpret_cast<const bf16x8_t*>(xf), acc, 0, 0, 0);
        if (k0 + 32 < p.K) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, *reinterpret_cast<const bf16x8_t*>(xf + 32), acc, 0, 0, 0);
        if (k0 + 64 < p.K) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, *reinterpret_cast<const bf16x8_t*>(xf + 64), acc, 0, 0, 0);
        if (k0 + 96 < p.K) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w3, *reinterpret_cast<const bf16x8_t*>(xf + 96), acc, 0, 0, 0);
    }
    // C/D: lane l, element e = column n + 4 (l >> 4) + e of tile row l & 15; k_pk_gemm_bf16's epilogue on the live rows
    const int m = rowat[l15], n = n0 + 16 * wave + 4 * kq;
    if (m < 0 || n >= p.N) return;
    const float4 add = p.bias ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    float v[4] = {acc[0] + add.x, acc[1] + add.y, acc[2] + add.z, acc[3] + add.w};
    if (p.epi == PKB_EPI_SILU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f + expf(-v[e]));
    } else if (p.epi == PKB_EPI_RES) {
        const float4 r = *reinterpret_cast<const float4*>(p.R + (size_t)m * p.ldr + n);
        v[0] = fmaf(p.ra, v[0], r.x); v[1] = fmaf(p.ra, v[1], r.y); v[2] = fmaf(p.ra, v[2], r.z); v[3] = fmaf(p.ra, v[3], r.w);
    }
    if (p.epi == PKB_EPI_RES) *reinterpret_cast<float4*>(p.Yf + (size_t)m * p.ldy + n) = make_float4(v[0], v[1], v[2], v[3]);
    else *reinterpret_cast<uint2*>(p.Yb + (size_t)m * p.ldy + n) = make_uint2(pkb_pack2(v[0], v[1]), pkb_pack2(v[2], v[3]));
}

template <int NW, class Ctx>
static void nmr_gemm_launch_w(Ctx* c, const PkbGemm& p, int load, int B, int live) {
    const dim3 grid(std::max(cdiv(live, 16), 1), cdiv(p.N, 16 * NW)), block(64 * NW);
    if (load == PKB_LOAD_LN) MIS_LAUNCH(c, (k_nm_gemm_bf16_rows<PKB_LOAD_LN, NW>), grid, block, p, B);
    else if (load == PKB_LOAD_LN_SILU) MIS_LAUNCH(c, (k_nm_gemm_bf16_rows<PKB_LOAD_LN_SILU, NW>), grid, block, p, B);
    else MIS_LAUNCH(c, (k_nm_gemm_bf16_rows<PKB_LOAD_BF16, NW>), grid, block, p, B);
}

// rule NMR_ROWS64 / 32 / 16 on the `live` = sum of min(cnt[b], Tp) rows of B <= 64 entries; PKB_TILE64 / 32: k_pk_gemm_bf16
template <class Ctx>
static void nmr_gemm_launch(Ctx* c, const PkbGemm& p, int load, int rule, int B, int live) {
    if (rule == NMR_ROWS64) nmr_gemm_launch_w<4>(c, p, load, B, live);
    else if (rule == NMR_ROWS32) nmr_gemm_launch_w<2>(c, p, load, B, live);
    else if (rule == NMR_ROWS16) nmr_gemm_launch_w<1>(c, p, load, B, live);
    else nmb_gemm_launch(c, p, load, rule, B);
}

// ============================================================================ K | V into the ring
// qkv bf16 [S][Tp][3 d]: the columns d .. 3 d of frame i -> the ring row (pos[b] + i) % R of the stream, [k (d) | v (d)]; d % 8 == 0
__global__ void __launch_bounds__(256) k_nm_ring_put_bf16(const bf16_t* __restrict__ qkv, const int* __restrict__ cnt, const int* __restrict__ pos,
                                                          bf16_t* __restrict__ ring, size_t sstride, int R, int Tp, int d) {
    const int i = blockIdx.x, b = blockIdx.y;
    if (i >= min(cnt[b], Tp)) return;
    const uint4* src = reinterpret_cast<const uint4*>(qkv + ((size_t)b * Tp + i) * 3 * d + d);
    uint4* dst = reinterpret_cast<uint4*>(ring + b * sstride + (size_t)((pos[b] + i) % R) * 2 * d);
    for (int c = threadIdx.x; c < d / 4; c += 256) dst[c] = src[c];
}

// ============================================================================ chunked-limited attention over the bf16 ring
struct NmbAttnS {
    const bf16_t* q; int ldq;                                // the pass's rows [S][Tp][ldq], q at column h hd
    const bf16_t* ring; size_t sstride; int R, ldk, voff;    // ring row (key % R): k at h hd, v at voff + h hd; sstride in elements
    bf16_t* out; int ldo;
    const int *cnt, *pos; int Tp, hd;                        // the stream's pass frames and the absolute index of the first
    float qscale, sdk;
    const float *u, *v;
    const bf16_t* P; int ldp, poff;
    int C, L, dlo, dhi;
};

template <int NS, int QW>
__global__ void __launch_bounds__(64 * QW) k_nm_attn_stream_bf16(NmbAttnS p) {
    constexpr int HP = 32 * NS, LDK = HP + 8, CH = HP / 8, NT = 64 * QW, QB = 16 * QW, BR = QB + 32;
    __shared__ __attribute__((aligned(16))) bf16_t Ks[32][LDK];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HP][BF16_LD];    // [dimension][key]
    __shared__ __attribute__((aligned(16))) bf16_t Pb[BR][LDK];        // band row r = distance pos + q0 - kb - 31 + r
    __shared__ float Gp[QW][48][17];                                   // a wave's band products [band row][query]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * QB, n = min(p.cnt[b], p.Tp), hd = p.hd;
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = tid; i < QB * hd; i += NT) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0;
        }
        return;
    }
    const int pos = p.pos[b], kend = pos + n;                       // the ring holds the keys < kend
    const bf16_t* ring = p.ring + b * p.sstride;
    const bool vec = ((hd | p.ldk | p.voff | p.ldp) & 7) == 0;
    const int tq = q0 + wave * 16 + l15;
    bf16x8_t qu[NS], qv[NS];                                        // B fragments: query l15, dimensions 32 s + 8 g .. + 7
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = s * 32 + g * 8 + e;
            const bool in = c < hd;
            const float q = (in && tq < n) ? bf16_to_f32(p.q[(rowbase + tq) * p.ldq + h * hd + c]) * p.qscale : 0.0f;
            qu[s][e] = (short)f32_to_bf16(in ? q + p.u[h * hd + c] : 0.0f);
            qv[s][e] = (short)f32_to_bf16(in ? q + p.v[h * hd + c] : 0.0f);
        }
    f32x4_t O[2 * NS];                                              // O^T: dimension 16 t + 4 g + e of query l15
#pragma unroll
    for (int t = 0; t < 2 * NS; ++t) O[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.0f;
    const int kr0 = 8 * (l15 >> 2) + (l15 & 3);                     // A row l15 of key tile t reads key kr0 + 4 t: D rows 4 g + e are keys 8 g + 4 t + e
    // the rule in absolute frames: the lane's query sees the keys [vlo, vhi); the block walks the absolute 32-aligned tiles that the first
    // and the last live query of it see; keys in front of blo belong to no query of the block and are staged as zeros
    const int qc = (pos + tq) / p.C, vlo = max(qc - p.L, 0) * p.C, vhi = (qc + 1) * p.C;
    const int blo = max((pos + q0) / p.C - p.L, 0) * p.C, wlo = blo & ~31, whi = min(kend, ((pos + min(q0 + QB - 1, n - 1)) / p.C + 1) * p.C);
    for (int kb = wlo; kb < whi; kb += 32) {
        __syncthreads();                                            // the previous tile's reads are done
        for (int i = tid; i < 32 * CH; i += NT) {
            const int r = i / CH, cc = (i % CH) * 8, key = kb + r;
            *reinterpret_cast<uint4*>(&Ks[r][cc]) =
                (key >= blo && key < kend) ? pkb_chunk(ring + (size_t)(key % p.R) * p.ldk + h * hd, cc, hd, vec) : make_uint4(0, 0, 0, 0);
        }
        for (int i = tid; i < 32 * CH; i += NT) {                   // V transposed: consecutive threads, consecutive keys
            const int r = i & 31, cc = (i >> 5) * 8, key = kb + r;
            const uint4 q = (key >= blo && key < kend) ? pkb_chunk(ring + (size_t)(key % p.R) * p.ldk + p.voff + h * hd, cc, hd, vec) : make_uint4(0, 0, 0, 0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[cc + e][r] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
        }
        const int base = pos + q0 - kb - 31;                        // distance of band row 0
        for (int i = tid; i < BR * CH; i += NT) {
            const int r = i / CH, cc = (i % CH) * 8, dist = base + r;
            *reinterpret_cast<uint4*>(&Pb[r][cc]) = (r < QB + 31 && dist >= p.dlo && dist <= p.dhi)
                                                        ? pkb_chunk(p.P + (size_t)(dist + p.poff) * p.ldp + h * hd, cc, hd, vec) : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        f32x4_t S0 = {0.f, 0.f, 0.f, 0.f}, S1 = S0, G0 = S0, G1 = S0, G2 = S0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int col = s * 32 + g * 8;
            S0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&Ks[kr0][col]), qu[s], S0, 0, 0, 0);
            S1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&Ks[kr0 + 4][col]), qu[s], S1, 0, 0, 0);
            const bf16_t* band = &Pb[wave * 16 + l15][col];
            G0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(band), qv[s], G0, 0, 0, 0);
            G1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(band + 16 * LDK), qv[s], G1, 0, 0, 0);
            G2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(band + 32 * LDK), qv[s], G2, 0, 0, 0);
        }
        // the wave's patch: band row 16 t + 4 g + e of query l15; then the shifted diagonal, band row l15 - key + 31
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Gp[wave][4 * g + e][l15] = G0[e];
            Gp[wave][16 + 4 * g + e][l15] = G1[e];
            Gp[wave][32 + 4 * g + e][l15] = G2[e];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float sc[8], mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = 8 * g + e, key = kb + kk;                // keys 8 g .. 8 g + 7 of the tile
            const float s = (e < 4 ? S0[e & 3] : S1[e & 3]) + Gp[wave][l15 - kk + 31][l15];
            sc[e] = (key < kend && key >= vlo && key < vhi) ? s / p.sdk : -INFINITY;
            mx = fmaxf(mx, sc[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.0f : m_new;      // the query has seen no key yet: every weight below is exp(-inf) = 0
        const float alpha = expf(m_run - m_use);
        float psum = 0.0f;
        bf16x8_t pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float pe = expf(sc[e] - m_use);
            psum += pe;                                             // the row sum takes the unrounded probability
            pf[e] = (short)f32_to_bf16(pe);
        }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int t = 0; t < 2 * NS; ++t) {
#pragma unroll
            for (int e = 0; e < 4; ++e) O[t][e] *= alpha;
            O[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&Vt[t * 16 + l15][g * 8]), pf, O[t], 0, 0, 0);
        }
    }
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);                // > 0 for a live query: it sees itself
    l_tot += __shfl_xor(l_tot, 32, 64);
    if (tq >= p.Tp) return;
    bf16_t* orow = p.out + (rowbase + tq) * p.ldo + h * hd;
    const bool vst = ((hd | p.ldo) & 3) == 0;
#pragma unroll
    for (int t = 0; t < 2 * NS; ++t) {
        const int dcol = t * 16 + 4 * g;
        if (dcol >= hd) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tq < n ? O[t][e] / l_tot : 0.0f;
        if (vst) *reinterpret_cast<uint2*>(orow + dcol) = make_uint2(pkb_pack2(v[0], v[1]), pkb_pack2(v[2], v[3]));
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (dcol + e < hd) orow[dcol + e] = f32_to_bf16(v[e]);
        }
    }
}

template <int QW, class Ctx>
static void nmb_attn_stream_w(Ctx* c, const NmbAttnS& p, int heads, int hd, int streams) {
    const dim3 grid(cdiv(p.Tp, 16 * QW), heads, streams), block(64 * QW);
    if (hd <= 32) MIS_LAUNCH(c, (k_nm_attn_stream_bf16<1, QW>), grid, block, p);
    else if (hd <= 64) MIS_LAUNCH(c, (k_nm_attn_stream_bf16<2, QW>), grid, block, p);
    else if (hd <= 96) MIS_LAUNCH(c, (k_nm_attn_stream_bf16<3, QW>), grid, block, p);
    else MIS_LAUNCH(c, (k_nm_attn_stream_bf16<4, QW>), grid, block, p);
}

// 16 queries a block while a stream's pass holds no more than that, 32 above (the header's reasoning)
template <class Ctx>
static void nmb_attn_stream(Ctx* c, const NmbAttnS& p, int heads, int hd, int streams) {
    if (p.Tp <= 16) nmb_attn_stream_w<1>(c, p, heads, hd, streams);
    else nmb_attn_stream_w<2>(c, p, heads, hd, streams);
}

// ============================================================================ conv module, carried
// k_nm_glu_dwconv_ln_bf16 at padl = k - 1 with hin [S][k - 1][2 C] (the stream's last pointwise_conv1 rows, oldest first) where offline pads
// zeros; block 0 of a stream writes hout = the last k - 1 rows of [hin ++ the pass's].  sstride: elements between two streams' histories.
__global__ void __launch_bounds__(256) k_nm_glu_dwconv_ln_stream_bf16(const bf16_t* __restrict__ pw, const float* __restrict__ taps,
                                                                      const float* __restrict__ bias, const int* __restrict__ cnt,
                                                                      bf16_t* __restrict__ out, float* __restrict__ stats,
                                                                      const bf16_t* __restrict__ hin, bf16_t* __restrict__ hout, size_t sstride, int Tp,
                                                                      int C, int k, float eps) {
    __shared__ __attribute__((aligned(16))) float g[NM_DW_TT + SF_DW_MAXK - 1][64];
    const int tid = threadIdx.x, cl = tid & 63, tl = tid >> 6, b = blockIdx.y, t0 = blockIdx.x * NM_DW_TT, tw = t0 + tl * 4, padl = k - 1;
    const int n = min(cnt[b], Tp);
    const size_t rowbase = (size_t)b * Tp;
    const bf16_t* hi_ = hin + b * sstride;
    const bool vec = (C & 7) == 0;
    if (blockIdx.x == 0) {                                          // the next history: frame n - padl + r, two elements a thread (2 C is even)
        const uint32_t* hsrc = reinterpret_cast<const uint32_t*>(hi_);
        uint32_t* hdst = reinterpret_cast<uint32_t*>(hout + b * sstride);
        for (int i = tid; i < padl * C; i += 256) {
            const int r = i / C, c = i - r * C, t = n - padl + r;
            hdst[i] = t < 0 ? hsrc[(size_t)(padl + t) * C + c] : reinterpret_cast<const uint32_t*>(pw + (rowbase + t) * 2 * C)[c];
        }
    }
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, q[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mean[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int pass = 0; pass < 2; ++pass) {                          // 0: the sums; 1: the same values again, their squared distances, the stores
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int ch = c0 + cl;
            __syncthreads();                                        // the previous 64 channels are read
            for (int i = tid; i < (NM_DW_TT + k - 1) * 8; i += 256) {   // a thread: 8 channels of a frame, a and its gate in one chunk each
                const int r = i >> 3, cc = (i & 7) * 8, t = t0 - padl + r;
                float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (t < n && c0 + cc < C) {                         // t < 0: the carried rows (t >= -padl)
                    const bf16_t* row = t >= 0 ? pw + (rowbase + t) * 2 * C : hi_ + (size_t)(padl + t) * 2 * C;
                    const uint4 xa = pkb_chunk(row, c0 + cc, C, vec), xg = pkb_chunk(row + C, c0 + cc, C, vec);
                    float al[4], ah[4], gl[4], gh[4];
                    bf16x4_unpack(make_uint2(xa.x, xa.y), al);
                    bf16x4_unpack(make_uint2(xa.z, xa.w), ah);
                    bf16x4_unpack(make_uint2(xg.x, xg.y), gl);
                    bf16x4_unpack(make_uint2(xg.z, xg.w), gh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a[e] = al[e] * (1.0f / (1.0f + expf(-gl[e])));
                        a[4 + e] = ah[e] * (1.0f / (1.0f + expf(-gh[e])));
                    }
                }
                *reinterpret_cast<float4*>(&g[r][cc]) = make_float4(a[0], a[1], a[2], a[3]);
                *reinterpret_cast<float4*>(&g[r][cc + 4]) = make_float4(a[4], a[5], a[6], a[7]);
            }
            __syncthreads();
            if (ch >= C) continue;                                  // (the barriers above are reached: the loop bound is uniform)
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
                const float v = t < n ? acc[i] : 0.0f;
                if (pass == 0) { s[i] += v; continue; }
                const float dv = v - mean[i];
                if (t < n) q[i] = fmaf(dv, dv, q[i]);
                if (t < Tp) out[(rowbase + t) * C + ch] = t < n ? f32_to_bf16(v) : (bf16_t)0;
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mean[i] = wave_sum(s[i]) / (float)C;   // the wave's four frames: the lanes hold the channels cl, cl + 64, ..
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = tw + i;
        const float rstd = 1.0f / sqrtf(wave_sum(q[i]) / (float)C + eps);
        if (cl == 0 && t < Tp) { stats[2 * (rowbase + t)] = t < n ? mean[i] : 0.0f; stats[2 * (rowbase + t) + 1] = t < n ? rstd : 0.0f; }
    }
}

template <class Ctx>
static void nmb_glu_dwconv_ln_stream(Ctx* c, const bf16_t* pw, const float* taps, const float* bias, const int* cnt, bf16_t* out, float* stats,
                                     const bf16_t* hin, bf16_t* hout, size_t sstride, int Tp, int C, int k, int streams) {
    MIS_LAUNCH(c, k_nm_glu_dwconv_ln_stream_bf16, dim3(cdiv(Tp, NM_DW_TT), streams), dim3(256), pw, taps, bias, cnt, out, stats, hin, hout, sstride, Tp, C,
               k, 1e-5f);
}

}  // namespace
