// codec_stream.hip - the kernels the code-driven decoders share around their contractions (declared in codec_kernels.h): the RVQ
// gather-sum that opens a decode, the streaming carry in front of every causal conv, and the activation + conv (C -> 1) that ends the
// Mimi and Qwen3-TTS decoders.  The bitwise "any chunking equals the whole decode" guarantee of both streams rests on the carry and on
// the final conv running the same instruction sequence for every output column.
#include "common.h"
#include "codec_kernels.h"

// codes -> h [B][C][ld]: sum over the quantizers, q ascending, of the folded tables [nq][bins][C]; a code is clamped to [0, bins)
__global__ void k_codec_embed(const int32_t* __restrict__ codes, int64_t cs_b, int64_t cs_q, int64_t cs_t, const float* __restrict__ tables,
                              float* __restrict__ h, int nq, int bins, int C, int ld) {
    const int t = blockIdx.x, b = blockIdx.y;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float acc = 0.0f;
        for (int q = 0; q < nq; ++q) {
            int code = codes[(size_t)b * cs_b + (size_t)q * cs_q + (size_t)t * cs_t];
            code = min(max(code, 0), bins - 1);
            acc += tables[((size_t)q * bins + code) * C + c];
        }
        h[((size_t)b * C + c) * ld + t] = acc;
    }
}
void launch_codec_embed(const int32_t* codes, int64_t cs_b, int64_t cs_q, int64_t cs_t, const float* tables, float* h, int nq, int bins, int C,
                        int ld, int T, int batch, hipStream_t s) {
    hipLaunchKernelGGL(k_codec_embed, dim3(T, batch), dim3(256), 0, s, codes, cs_b, cs_q, cs_t, tables, h, nq, bins, C, ld);
}

// One block per row: columns [-H, 0) of x <- st, then st <- the last H columns of [st | new]
__global__ void __launch_bounds__(64) k_codec_hist(float* __restrict__ st, float* __restrict__ x, int C, int ld, int H, int Tn) {
    const int c = blockIdx.x, b = blockIdx.y, i = threadIdx.x;
    float* sr = st + ((size_t)b * C + c) * H;
    float* xr = x + ((size_t)b * C + c) * ld;
    float old = 0.0f, nw = 0.0f;
    if (i < H) {
        old = sr[i];
        const int src = Tn - H + i;
        nw = src >= 0 ? xr[src] : sr[i + Tn];
    }
    __syncthreads();
    if (i < H) { xr[i - H] = old; sr[i] = nw; }
}
void launch_codec_hist(float* st, float* x, int C, int ld, int H, int Tn, int batch, hipStream_t s) {
    MIS_REQUIRE(H >= 0 && H <= 64, MIS_ERR_GENERATION_FAILED, "streaming history of %d columns does not fit one block", H);
    hipLaunchKernelGGL(k_codec_hist, dim3(C, batch), dim3(64), 0, s, st, x, C, ld, H, Tn);
}

// 256 output columns per block; 16 channels at a time are staged through LDS with the activation applied ONCE per element (the
// per-thread version evaluated sin() k times per element and ran at 0.6 TB/s); accumulation channel-major, tap-minor
#define CODEC_F_TILE 256
#define CODEC_F_CH 16
enum { ACT_SNAKE_BETA_CLIP = 0, ACT_ELU = 1 };
__device__ __forceinline__ float snake_beta(float v, int c, const float* __restrict__ a, const float* __restrict__ ra) {
    return fmaf(ra[c], mis_sin_sq(a[c] * v), v);
}
// ACT_SNAKE_BETA_CLIP: x + ra sin^2(a x) on the operand, output clipped to [-1, 1] (AP = a, ra); ACT_ELU: ELU (alpha 1), no clip (AP empty).
// The activation's own arguments are a pack and the ELU is written out in the staging branch, so each instantiation keeps the argument
// list and the instruction sequence of the kernel it replaced (expf runs only on the lanes with v <= 0)
template <int ACT, typename... AP>
__global__ void __launch_bounds__(256) k_codec_final(const float* __restrict__ x, float* __restrict__ out, int64_t out_stride,
                                                     const float* __restrict__ w /*[k][C]*/, float bias, AP... ap, int C, int T, int ld, int x_lo,
                                                     int k) {
    __shared__ float sx[CODEC_F_CH][CODEC_F_TILE + 8];
    const int b = blockIdx.y, t0 = blockIdx.x * CODEC_F_TILE, tid = threadIdx.x;
    const int halo = k - 1;                                              // k <= 8
    float acc = bias;
    for (int c0 = 0; c0 < C; c0 += CODEC_F_CH) {
        __syncthreads();
        for (int i = tid; i < CODEC_F_CH * (CODEC_F_TILE + halo); i += 256) {
            const int cc = i / (CODEC_F_TILE + halo), j = i - cc * (CODEC_F_TILE + halo);
            const int c = c0 + cc, t = t0 - halo + j;
            float v = 0.0f;
            if (c < C && t >= x_lo && t < T) {
                v = x[((int64_t)b * C + c) * ld + t];
                if constexpr (ACT == ACT_ELU) v = v > 0.0f ? v : expf(v) - 1.0f;
                else v = snake_beta(v, c, ap...);
            }
            sx[cc][j] = v;
        }
        __syncthreads();
        const int cmax = min(CODEC_F_CH, C - c0);
        for (int cc = 0; cc < cmax; ++cc)
            for (int j = 0; j < k; ++j) acc += w[j * C + c0 + cc] * sx[cc][tid + j];
    }
    const int t = t0 + tid;
    if (t < T) out[(size_t)b * out_stride + t] = ACT == ACT_ELU ? acc : fminf(fmaxf(acc, -1.0f), 1.0f);
}
void launch_codec_final(const float* x, float* out, int64_t out_stride, const float* w, float bias, const float* a, const float* ra, int C, int T,
                        int ld, int x_lo, int k, int batch, hipStream_t s) {
    MIS_REQUIRE(k >= 1 && k <= 8, MIS_ERR_GENERATION_FAILED, "final conv of %d taps does not fit the tile's halo", k);
    const dim3 grid(cdiv(T, CODEC_F_TILE), batch);
    if (a) hipLaunchKernelGGL((k_codec_final<ACT_SNAKE_BETA_CLIP, const float*, const float*>), grid, dim3(256), 0, s, x, out, out_stride, w, bias, a, ra, C, T, ld, x_lo, k);
    else hipLaunchKernelGGL((k_codec_final<ACT_ELU>), grid, dim3(256), 0, s, x, out, out_stride, w, bias, C, T, ld, x_lo, k);
}
