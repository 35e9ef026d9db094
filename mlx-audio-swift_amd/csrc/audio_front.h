// audio_front.h - what the filter-bank front ends share.  Host tables of the 512-point FFT front ends (lasr.hip, sortformer.hip,
// fsmn_vad.hip, sensevoice.hip) and of mossformer2.hip: the twiddles and each filter's range of non-zero bins.  And the whole NeMo log-mel front end of
// lasr.hip and sortformer.hip, which is ONE front end: the Hann window of 400 in 512, the slaney filters, the log-mel kernel and the
// per-feature normalisation (below, behind AUDIO_FRONT_NEMO_KERNELS).  The engines promise results that are bit for bit independent of
// the batch, and their kernels read these tables, so they are formed in one place; tests/test_gpu_front_bits.py holds the engines'
// outputs to recorded hashes, and Sortformer's features to LASR's.
//
// A shared device piece is held to what these engines promise a caller: a row's bits in any batch (the recorded hashes), and the
// time, measured against the parent (f32_tile.h is shared on those terms; DESIGN.md has what was measured).  The FFT kernels of
// fsmn_vad.hip and mossformer2.hip keep their own copy of the butterfly loop and of the filter dot: ten lines each, and the kernels
// differ around them.  A further fbank engine starts from these tables and from block_sum_256 / block_max_256 in common.h; a further
// NeMo model (Parakeet) starts from the front end below.
#pragma once
#include <math.h>
#include <algorithm>
#include <stddef.h>
#include <vector>

// c[k] = cos(2 pi k / 512), s[k] = -sin(2 pi k / 512), k < 256, formed in double and rounded once
static inline void fft512_twiddles(float* c, float* s) {
    for (int k = 0; k < 256; ++k) {
        c[k] = (float)cos(2.0 * 3.14159265358979323846 * (double)k / 512);
        s[k] = (float)-sin(2.0 * 3.14159265358979323846 * (double)k / 512);
    }
}

// c[k] = cos(2 pi k / 2048), s[k] = -sin(2 pi k / 2048), k < 1024, formed in double and rounded once (mossformer2.hip).  A shorter
// power-of-two transform of n points reads every (2048 / n)-th entry: the same angles, the same values.
static inline void fft2048_twiddles(float* c, float* s) {
    for (int k = 0; k < 1024; ++k) {
        c[k] = (float)cos(2.0 * 3.14159265358979323846 * (double)k / 2048);
        s[k] = (float)-sin(2.0 * 3.14159265358979323846 * (double)k / 2048);
    }
}

// ranges[2 m], ranges[2 m + 1] = [first, last) non-zero bin of filter m in the finished fb [bins][nm]; 0, 0 for an all-zero filter
static inline void filter_bin_ranges(const float* fb, int bins, int nm, int* ranges) {
    for (int m = 0; m < nm; ++m) {
        int first = bins, last = 0;
        for (int i = 0; i < bins; ++i)
            if (fb[(size_t)i * nm + m] != 0.0f) { first = std::min(first, i); last = std::max(last, i + 1); }
        ranges[2 * m] = first < last ? first : 0; ranges[2 * m + 1] = first < last ? last : 0;
    }
}

// ---------------------------------------------------------------------------- the NeMo log-mel front end (16 kHz)
#define NEMO_NFFT 512
#define NEMO_HOP 160
#define NEMO_WIN 400
#define NEMO_BINS 257

// dst [nfft]: the symmetric Hann window of `win` points centred in nfft, zeros around it; f32 as the reference forms it
static inline void hann_padded(float* dst, int win, int nfft) {
    for (int n = 0; n < nfft; ++n) dst[n] = 0.0f;
    for (int n = 0; n < win; ++n) dst[(nfft - win) / 2 + n] = 0.5f * (1.0f - (float)cos(2.0 * M_PI * (double)n / (double)(win - 1)));
}

// slaney mel scale (DSP.swift melFilters, melScale .slaney)
static inline double slaney_hz_to_mel(double f) { return f < 1000.0 ? f / (200.0 / 3.0) : 15.0 + log(f / 1000.0) / (log(6.4) / 27.0); }
static inline double slaney_mel_to_hz(double m) { return m < 15.0 ? (200.0 / 3.0) * m : 1000.0 * exp((log(6.4) / 27.0) * (m - 15.0)); }

// fb [bins][mels]: slaney-normalised triangles between 0 and sample_rate / 2 over the bins of an nfft-point transform, formed in double
// and rounded once; ranges [2 mels] as filter_bin_ranges
static inline void slaney_filterbank(float* fb, int* ranges, int bins, int mels, double sample_rate, int nfft) {
    const double mmax = slaney_hz_to_mel(sample_rate / 2.0);
    std::vector<double> fp(mels + 2);
    for (int i = 0; i < mels + 2; ++i) fp[i] = slaney_mel_to_hz((double)i * mmax / (double)(mels + 1));
    for (int j = 0; j < mels; ++j) {
        const double lo = fp[j], ce = fp[j + 1], hi = fp[j + 2], enorm = 2.0 / (hi - lo);
        for (int i = 0; i < bins; ++i) {
            const double fr = (double)i * sample_rate / nfft;
            double w = 0.0;
            if (fr >= lo && fr < ce) w = (fr - lo) / (ce - lo);
            else if (fr >= ce && fr <= hi) w = (hi - fr) / (hi - ce);
            fb[(size_t)i * mels + j] = (float)(w * enorm);
        }
    }
    filter_bin_ranges(fb, bins, mels, ranges);
}

#ifdef AUDIO_FRONT_NEMO_KERNELS     // lasr.hip and sortformer.hip: each gets its own (static) copy of the one pair of kernels
// One frame of one row: samples t 160 - 256 .. + 511 of the zero-centred, pre-emphasised waveform (y[0] = x[0], y[i] = x[i] - c x[i - 1]),
// window, 512-point radix-2 FFT in LDS, |.|^2, slaney filters over each filter's own bins, log(. + 2^-24); zeros behind F[b].  SCALED:
// every sample is first multiplied by the row's scale[b] (Sortformer's peak normalisation); without it no scale is read or multiplied.
// Samples behind N[b] are never read.
template <bool SCALED>
static __global__ void __launch_bounds__(256) k_nemo_log_mel(const float* __restrict__ pcm, int64_t stride, const int* __restrict__ N,
                                                             const int* __restrict__ F, const float* __restrict__ scale, float preemph,
                                                             const float* __restrict__ window, const float* __restrict__ twc,
                                                             const float* __restrict__ tws, const float* __restrict__ fb,
                                                             const int* __restrict__ fbr, float* __restrict__ out, int Fp, int mels) {
    __shared__ float re[NEMO_NFFT], im[NEMO_NFFT];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* o = out + ((size_t)b * Fp + t) * mels;
    if (t >= F[b]) { if (tid < mels) o[tid] = 0.0f; return; }
    const int n = N[b];
    const float g = SCALED ? scale[b] : 1.0f;
    const float* x = pcm + (size_t)b * stride;
    for (int j = tid; j < NEMO_NFFT; j += 256) {
        const float w = window[j];
        const int64_t s = (int64_t)t * NEMO_HOP - NEMO_NFFT / 2 + j;
        float v = 0.0f;
        if (w != 0.0f && s >= 0 && s < n) {
            const float cur = SCALED ? __fmul_rn(g, x[s]) : x[s];
            v = s == 0 ? cur : __fsub_rn(cur, __fmul_rn(preemph, SCALED ? __fmul_rn(g, x[s - 1]) : x[s - 1]));
        }
        const int r = (int)(__brev((unsigned)j) >> 23);
        re[r] = __fmul_rn(v, w); im[r] = 0.0f;
    }
    __syncthreads();
    for (int half = 1; half < NEMO_NFFT; half <<= 1) {
        const int k = tid & (half - 1), i0 = ((tid - k) << 1) + k, i1 = i0 + half, ti = k * (NEMO_NFFT / 2 / half);
        const float c = twc[ti], s = tws[ti];
        const float xr = re[i1], xi = im[i1];
        const float pr = xr * c - xi * s, pi = xr * s + xi * c;
        const float ar = re[i0], ai = im[i0];
        re[i0] = ar + pr; im[i0] = ai + pi; re[i1] = ar - pr; im[i1] = ai - pi;
        __syncthreads();
    }
    for (int j = tid; j < NEMO_BINS; j += 256) { const float a = re[j], c = im[j]; re[j] = a * a + c * c; }
    __syncthreads();
    if (tid < mels) {
        float acc = 0.0f;
        for (int i = fbr[2 * tid]; i < fbr[2 * tid + 1]; ++i) acc = fmaf(re[i], fb[(size_t)i * mels + tid], acc);
        o[tid] = logf(acc + 5.9604644775390625e-08f);
    }
}

// per_feature normalisation (ParakeetAudio.swift:47-53): per mel bin, mean and unbiased variance (divisor max(F - 1, 1)) over the row's
// own F[b] computed frames in two passes, (x - mean) / (sqrt(var) + 1e-5), or the copy (normalize 0); zeros behind F[b].  A thread owns
// one bin and every fourth frame; the four partial sums are added in a fixed order, so a row's statistics depend on nothing but the row.
static __global__ void __launch_bounds__(256) k_nemo_norm(const float* __restrict__ raw, const int* __restrict__ F, float* __restrict__ out, int Fp,
                                                          int mels, int normalize) {
    __shared__ float part[4][64];
    const int b = blockIdx.y, ml = threadIdx.x & 63, fl = threadIdx.x >> 6, m = blockIdx.x * 64 + ml, n = F[b];
    const bool live = m < mels;
    const float* x = raw + (size_t)b * Fp * mels + (live ? m : 0);
    float mean = 0.0f, den = 1.0f;
    if (normalize) {
        float s = 0.0f;
        for (int t = fl; t < n; t += 4) s += x[(size_t)t * mels];
        part[fl][ml] = s;
        __syncthreads();
        mean = ((part[0][ml] + part[1][ml]) + (part[2][ml] + part[3][ml])) / (float)n;
        __syncthreads();
        float q = 0.0f;
        for (int t = fl; t < n; t += 4) { const float v = x[(size_t)t * mels] - mean; q = fmaf(v, v, q); }
        part[fl][ml] = q;
        __syncthreads();
        const float var = ((part[0][ml] + part[1][ml]) + (part[2][ml] + part[3][ml])) / (float)max(n - 1, 1);
        den = sqrtf(var) + 1e-5f;
    }
    if (!live) return;
    float* y = out + (size_t)b * Fp * mels + m;
    for (int t = fl; t < Fp; t += 4) y[(size_t)t * mels] = t < n ? (normalize ? (x[(size_t)t * mels] - mean) / den : x[(size_t)t * mels]) : 0.0f;
}
#endif
