// audio_front.h - host tables of the 512-point FFT filter-bank front ends (lasr.hip, fsmn_vad.hip): the twiddles and each filter's
// range of non-zero bins.  Both engines promise results that are bit for bit independent of the batch, and both kernels read these
// tables, so they are formed in one place; tests/test_gpu_front_bits.py holds the engines' outputs to recorded hashes.
//
// A shared device piece is held to what these engines promise a caller: a row's bits in any batch (the recorded hashes), and the
// time, measured against the parent (f32_tile.h is shared on those terms; DESIGN.md has what was measured).  The FFT kernels keep
// their own copy of the butterfly loop and of the filter dot: ten lines each, and the kernels differ around them.  A further fbank
// engine starts from these tables and from block_sum_256 / block_max_256 in common.h.
#pragma once
#include <math.h>
#include <algorithm>
#include <stddef.h>

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
