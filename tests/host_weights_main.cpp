// Stand-alone check of csrc/host_weights.h (test_host_weights_cpu.py builds it with the address and undefined-behaviour sanitizers and
// runs it): the weight stash, the bf16 / f32 arena and its bindings, the BatchNorm fold, the exact-f32 codec arena and its re-layouts, the
// synthetic tensors; the host tables of the NeMo front end (csrc/audio_front.h).  Host code only: no HIP call is made, no device is opened.
#include "../mlx-audio-swift_amd/csrc/host_weights.h"
#include "../mlx-audio-swift_amd/csrc/audio_front.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// what() and code of the MisError that f throws; code -1: nothing thrown
template <typename F>
static std::string thrown(F f, int* code) {
    *code = -1;
    try { f(); } catch (const MisError& e) { *code = (int)e.code; return e.what(); }
    return "";
}

static void need_messages(const char* label, mis_status missing) {
    HostWeights w(label, missing);
    const float v[6] = {1, 2, 3, 4, 5, 6};
    const int64_t sh[2] = {2, 3};
    w.put("a.weight", v, MIS_F32, sh, 2);
    const HostTensor& t = w.need("a.weight", {2, 3});
    CHECK(t.shape == (std::vector<int64_t>{2, 3}) && t.v.size() == 6 && t.v[5] == 6.0f);
    CHECK(&w.need("a.weight") == &t && w.find("a.weight") == &t && w.find("b") == nullptr && w.count("a.weight") == 1 && w.count("b") == 0);
    int code;
    std::string m = thrown([&] { w.need("b.bias", {3}); }, &code);
    CHECK(code == (int)missing && m == std::string(label) + " weight missing: b.bias");
    m = thrown([&] { w.need("b.bias"); }, &code);
    CHECK(code == (int)missing && m == std::string(label) + " weight missing: b.bias");
    for (auto wrong : {std::vector<int64_t>{3, 2}, std::vector<int64_t>{6}, std::vector<int64_t>{2, 3, 1}}) {
        m = thrown([&] {
            if (wrong.size() == 1) w.need("a.weight", {wrong[0]});
            else if (wrong.size() == 2) w.need("a.weight", {wrong[0], wrong[1]});
            else w.need("a.weight", {wrong[0], wrong[1], wrong[2]});
        }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == std::string(label) + " weight a.weight has the wrong shape");
    }
    size_t n = 0;
    for (auto& kv : w) { CHECK(kv.first == "a.weight"); ++n; }
    CHECK(n == 1);
    w.clear();
    CHECK(w.find("a.weight") == nullptr && w.begin() == w.end());
}

int main() {
    HostWeights w("DAC");
    int code;
    std::string m;
    {   // f32 as stored; f16: zero, -zero, the smallest and the largest subnormal, +-inf, full mantissas; bf16
        const float f[3] = {1.00390625f, -0.0f, 3.0e38f};
        const int64_t s3[1] = {3};
        w.put("f32", f, MIS_F32, s3, 1);
        for (int i = 0; i < 3; ++i) CHECK(bits(w.need("f32", {3}).v[i]) == bits(f[i]));
        const uint16_t h[10] = {0x0000, 0x8000, 0x0001, 0x03ff, 0x7c00, 0xfc00, 0x3fff, 0x7bff, 0xc248, 0x0400};
        const uint32_t want[10] = {0x00000000u, 0x80000000u, 0x33800000u /* 2^-24 */, 0x387fc000u /* 1023 x 2^-24 */, 0x7f800000u, 0xff800000u,
                                   0x3fffe000u /* 1.9990234375 */, 0x477fe000u /* 65504 */, 0xc0490000u /* -3.140625 */, 0x38800000u /* 2^-14 */};
        const int64_t s10[2] = {2, 5};
        w.put("f16", h, MIS_F16, s10, 2);
        const HostTensor& t = w.need("f16", {2, 5});
        for (int i = 0; i < 10; ++i) CHECK(bits(t.v[i]) == want[i]);
        CHECK(t.v[2] == 5.9604644775390625e-08f && t.v[3] == 6.097555160522461e-05f && t.v[6] == 1.9990234375f && t.v[7] == 65504.0f);
        CHECK(isinf(t.v[4]) && t.v[4] > 0 && isinf(t.v[5]) && t.v[5] < 0);
        const uint16_t b[4] = {0x3f80, 0xc049, 0x0001, 0x7f80};
        const uint32_t bwant[4] = {0x3f800000u, 0xc0490000u, 0x00010000u, 0x7f800000u};
        const int64_t s4[3] = {1, 4, 1};
        w.put("bf16", b, MIS_BF16, s4, 3);
        for (int i = 0; i < 4; ++i) CHECK(bits(w.need("bf16", {1, 4, 1}).v[i]) == bwant[i]);
        CHECK(w.need("bf16").v[1] == -3.140625f);
        m = thrown([&] { w.put("bad", b, MIS_I32, s4, 3); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == "unsupported dtype" && !w.find("bad"));
    }
    {   // a shape entry <= 0
        const float f[2] = {1, 2};
        const int64_t zero[2] = {2, 0}, neg[1] = {-1};
        m = thrown([&] { w.put("z", f, MIS_F32, zero, 2); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == "bad shape");
        m = thrown([&] { w.put("z", f, MIS_F32, neg, 1); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == "bad shape" && !w.find("z"));
        m = thrown([&] { HostWeights::count(zero, 2); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT);
        const int64_t ok[3] = {2, 3, 4};
        CHECK(HostWeights::count(ok, 3) == 24);
    }
    {   // the second put of a name replaces the first, shape included
        const float a[2] = {1, 2}, b[3] = {7, 8, 9};
        const int64_t s2[1] = {2}, s3[2] = {3, 1};
        w.put("r", a, MIS_F32, s2, 1);
        w.put("r", b, MIS_F32, s3, 2);
        CHECK(w.need("r", {3, 1}).v == (std::vector<float>{7, 8, 9}));
        thrown([&] { w.need("r", {2}); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT);
        w.put("r", HostTensor{{4.0f}, {1}});
        CHECK(w.need("r", {1}).v[0] == 4.0f);
    }
    need_messages("Smart Turn", MIS_ERR_INVALID_INPUT);
    need_messages("DAC", MIS_ERR_NOT_INITIALIZED);
    {   // arena: offsets rounded up to 64 elements, zero fill, one round-to-nearest-even per element
        // 1 + 2^-8: tie, even below; 1 + 3 x 2^-8: tie, even above; one ulp above and below the first tie; a negative tie
        const float f[5] = {from_bits(0x3f808000u), from_bits(0x3f818000u), from_bits(0x3f808001u), from_bits(0x3f807fffu), from_bits(0xbf818000u)};
        const uint16_t want[5] = {0x3f80, 0x3f82, 0x3f81, 0x3f80, 0xbf82};
        const int64_t s5[1] = {5}, s23[2] = {2, 3};
        const float g[6] = {0.5f, -2.0f, 3.0f, 65536.0f, 1e-3f, -0.0f};
        w.put("v", f, MIS_F32, s5, 1);
        w.put("m", g, MIS_F32, s23, 2);
        HostArena a(w);
        CHECK(a.btake(1) == 0 && a.host.size() == 64);
        CHECK(a.btake(65) == 64 && a.host.size() == 192);
        CHECK(a.btake(64) == 192 && a.host.size() == 256);
        const size_t ov = a.bvec("v", 5);
        CHECK(ov == 256 && a.host.size() == 320);
        for (int i = 0; i < 5; ++i) CHECK(a.host[ov + i] == want[i]);
        const size_t om = a.bmat("m", 2, 3);
        CHECK(om == 320 && a.host.size() == 384);
        for (int i = 0; i < 6; ++i) CHECK(a.host[om + i] == f32_to_bf16(g[i]));
        CHECK(a.host[om + 1] == 0xc000 && a.host[om + 4] == 0x3a83 && a.host[om + 5] == 0x8000);
        a.bmat_into("m", 2, 3, 10);
        CHECK(a.host[10] == 0x3f00 && a.host[15] == 0x8000);
        for (size_t i = 0; i < a.host.size(); ++i)
            if (!(i >= 10 && i < 16) && !(i >= ov && i < ov + 5) && !(i >= om && i < om + 6)) CHECK(a.host[i] == 0);
        CHECK(a.ftake(3) == 0 && a.fhost.size() == 64 && a.ftake(128) == 64 && a.fhost.size() == 192);
        const size_t of = a.fvec("m", {2, 3}, 4);
        CHECK(of == 192 && a.fhost.size() == 256);
        for (size_t i = 0; i < a.fhost.size(); ++i) CHECK(bits(a.fhost[i]) == (i >= of && i < of + 4 ? bits(g[i - of]) : 0u));
        m = thrown([&] { a.bvec("v", 4); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == "DAC weight v has the wrong shape" && a.host.size() == 384);
        m = thrown([&] { a.fvec("nope", {1}, 1); }, &code);
        CHECK(code == (int)MIS_ERR_NOT_INITIALIZED && m == "DAC weight missing: nope");
    }
    {   // bindings: resolve() writes base + offset into every bound pointer, each arena from its own base; the takes are the plain ones
        HostArena a(w);
        struct { bf16_t *v = nullptr, *m = nullptr, *pad = nullptr, *tied = nullptr, *absent = nullptr; float* f = nullptr; const float *cf = nullptr, *cabs = nullptr; } dst;
        float* local = nullptr;
        CHECK(a.btake(1, dst.pad) == 0 && a.bvec("v", 5, dst.v) == 64 && a.btake(3) == 128 && a.bmat("m", 2, 3, dst.m) == 192 && a.host.size() == 256);
        a.bind(dst.tied, 64);                                      // one offset, two destinations
        CHECK(a.ftake(65, dst.f) == 0 && a.fvec("m", {2, 3}, 4, dst.cf) == 128 && a.ftake(2, local) == 192 && a.fhost.size() == 256);
        CHECK(a.host[64] == 0x3f80 && a.host[192] == f32_to_bf16(0.5f) && bits(a.fhost[129]) == bits(-2.0f));
        for (size_t i = 0; i < a.host.size(); ++i) if (!(i >= 64 && i < 69) && !(i >= 192 && i < 198)) CHECK(a.host[i] == 0);
        for (size_t i = 0; i < a.fhost.size(); ++i) if (!(i >= 128 && i < 132)) CHECK(bits(a.fhost[i]) == 0u);
        CHECK(!dst.v && !dst.f && !local);                          // nothing is written before resolve
        std::vector<bf16_t> A(256);
        std::vector<float> F(256);
        a.resolve(A.data(), F.data());
        CHECK(dst.pad == A.data() && dst.v == A.data() + 64 && dst.tied == A.data() + 64 && dst.m == A.data() + 192);
        CHECK(dst.f == F.data() && dst.cf == F.data() + 128 && local == F.data() + 192);
        CHECK(dst.absent == nullptr && dst.cabs == nullptr);
        std::vector<bf16_t> A2(256);
        a.resolve(A2.data(), F.data() + 7);                         // the two bases are independent
        CHECK(dst.v == A2.data() + 64 && dst.cf == F.data() + 7 + 128 && local == F.data() + 7 + 192 && dst.absent == nullptr);
        static_assert(!std::is_copy_constructible<HostArena>::value && !std::is_copy_assignable<HostArena>::value, "HostArena holds addresses");
    }
    for (bool with_bias : {false, true}) {   // fold_bn_dwconv against its formula: f32, eps 1e-5
        const int64_t d = 5, k = 3;
        std::vector<float> dw(d * k), db(d), bw(d), bb(d), mu(d), var(d), taps(k * d + 1, 7.0f), shift(d + 1, 7.0f);
        for (int64_t i = 0; i < d * k; ++i) dw[i] = mis_synth_value(21, i, 1.0f);
        for (int64_t i = 0; i < d; ++i) {
            db[i] = mis_synth_value(22, i, 0.1f); bw[i] = 1.0f + mis_synth_value(23, i, 0.1f); bb[i] = mis_synth_value(24, i, 0.1f);
            mu[i] = mis_synth_value(25, i, 0.1f); var[i] = 1.0f + mis_synth_value(26, i, 0.3f);
        }
        fold_bn_dwconv(taps.data(), shift.data(), dw.data(), with_bias ? db.data() : nullptr, bw.data(), bb.data(), mu.data(), var.data(), d, k);
        for (int64_t ch = 0; ch < d; ++ch) {
            const float scale = bw[ch] / sqrtf(var[ch] + 1e-5f);
            for (int64_t j = 0; j < k; ++j) CHECK(bits(taps[j * d + ch]) == bits(dw[ch * k + j] * scale));
            CHECK(bits(shift[ch]) == bits(((with_bias ? db[ch] : 0.0f) - mu[ch]) * scale + bb[ch]));
        }
        CHECK(taps[k * d] == 7.0f && shift[d] == 7.0f);
    }
    {   // the NeMo front end's tables against their formulas, in double: Hann 400 in 512, slaney filters for 80 and 128 mels
        std::vector<float> win(513, 7.0f);
        hann_padded(win.data(), 400, 512);
        for (int n = 0; n < 512; ++n) {
            const int i = n - 56;
            const float want = (i >= 0 && i < 400) ? 0.5f * (1.0f - (float)cos(2.0 * 3.14159265358979323846 * (double)i / 399.0)) : 0.0f;
            CHECK(bits(win[n]) == bits(want));
        }
        CHECK(win[512] == 7.0f && win[56] == 0.0f && win[455] == 0.0f && win[57] > 0.0f && win[256] > 0.9999f);
        for (int mels : {80, 128}) {
            const int bins = 257;
            std::vector<float> fb((size_t)bins * mels + 1, 7.0f);
            std::vector<int> ranges(2 * mels + 1, -5), want_ranges(2 * mels, -5);
            slaney_filterbank(fb.data(), ranges.data(), bins, mels, 16000.0, 512);
            auto h2m = [](double f) { return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + 27.0 * log(f / 1000.0) / log(6.4); };
            auto m2h = [](double m) { return m < 15.0 ? 200.0 * m / 3.0 : 1000.0 * exp(log(6.4) * (m - 15.0) / 27.0); };
            double worst = 0.0;
            for (int j = 0; j < mels; ++j) {
                const double lo = m2h(j * h2m(8000.0) / (mels + 1)), ce = m2h((j + 1) * h2m(8000.0) / (mels + 1)), hi = m2h((j + 2) * h2m(8000.0) / (mels + 1));
                double area = 0.0;
                for (int i = 0; i < bins; ++i) {
                    const double fr = i * 31.25, tri = std::max(0.0, std::min((fr - lo) / (ce - lo), (hi - fr) / (hi - ce))), want = tri * 2.0 / (hi - lo);
                    const double got = fb[(size_t)i * mels + j];
                    worst = std::max(worst, fabs(got - want) / std::max(want, 1e-30) * (want > 1e-12 ? 1.0 : 0.0));
                    CHECK(fabs(got - want) <= 1e-6 * want + 1e-12);           // one rounding to f32 (2^-24) and a few ulps of double
                    CHECK((got != 0.0) == (fr > lo && fr < hi));
                    area += got * 31.25;
                }
                // slaney normalisation: unit area up to the sampling of the triangle at 31.25 Hz (exact for an integrand linear between
                // the bins; the kinks at lo, ce and hi cost at most three trapezoid corners)
                CHECK(fabs(area - 1.0) < 3.0 * 31.25 / (hi - lo) + 1e-5);
            }
            CHECK(worst < 1e-6 && fb[(size_t)bins * mels] == 7.0f && ranges[2 * mels] == -5);
            filter_bin_ranges(fb.data(), bins, mels, want_ranges.data());
            for (int i = 0; i < 2 * mels; ++i) CHECK(ranges[i] == want_ranges[i]);
            for (int j = 0; j < mels; ++j) CHECK(ranges[2 * j] >= 1 && ranges[2 * j] < ranges[2 * j + 1] && ranges[2 * j + 1] <= bins);
        }
    }
    {   // F32Arena::push: offsets count floats, zero padding to a multiple of 4 after every push
        F32Arena a;
        const size_t len[5] = {1, 4, 5, 0, 7}, want[5] = {0, 4, 8, 16, 16};
        for (int i = 0; i < 5; ++i) CHECK(a.push(std::vector<float>(len[i], -1.5f)) == want[i]);
        CHECK(a.host.size() == 24);
        const bool data[24] = {1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0};
        for (int i = 0; i < 24; ++i) CHECK(bits(a.host[i]) == (data[i] ? bits(-1.5f) : 0u));
        CHECK(a.zeros(6) == 24 && a.host.size() == 32);
        for (int i = 24; i < 32; ++i) CHECK(bits(a.host[i]) == 0u);
    }
    {   // re-layouts against the index formulas of the engines, written out; distinct integers, no two equal dimensions
        auto iota = [](size_t n) { std::vector<float> v(n); for (size_t i = 0; i < n; ++i) v[i] = (float)(i + 1); return v; };
        {
            const int64_t out = 3, in = 5;
            const std::vector<float> w = iota(out * in), at = lin_t(w, out, in);
            CHECK(at.size() == (size_t)(out * in));
            for (int64_t o = 0; o < out; ++o) for (int64_t i = 0; i < in; ++i) CHECK(at[i * out + o] == w[o * in + i]);
        }
        for (int64_t k : {4, 1}) {
            const int64_t co = 3, ci = 5;
            const std::vector<float> w = iota(co * k * ci), at = conv_taps_t(w, co, k, ci);
            CHECK(at.size() == (size_t)(co * k * ci));
            for (int64_t o = 0; o < co; ++o) for (int64_t j = 0; j < k; ++j) for (int64_t c = 0; c < ci; ++c)
                CHECK(at[(j * ci + c) * co + o] == w[(o * k + j) * ci + c]);
        }
        struct { int64_t k, s, pad; } cases[] = {{4, 2, 0}, {4, 2, 1}, {6, 2, 0}, {6, 2, 1}, {2, 2, 0}, {6, 3, 2}};
        for (auto cs : cases)
            for (bool in_major : {false, true}) {
                const int64_t co = 3, ci = 5, k = cs.k, s = cs.s, pad = cs.pad, nt = k / s;
                const std::vector<float> w = iota(co * k * ci), at = convt_phases_t(w, co, k, ci, s, pad, in_major);
                CHECK(at.size() == (size_t)(s * nt * ci * co));
                for (int64_t ph = 0; ph < s; ++ph) for (int64_t j = 0; j < nt; ++j) for (int64_t c = 0; c < ci; ++c) for (int64_t o = 0; o < co; ++o) {
                    const int64_t tap = ((ph + pad) % s) + s * j;
                    CHECK(at[((ph * nt + j) * ci + c) * co + o] == (in_major ? w[(c * k + tap) * co + o] : w[(o * k + tap) * ci + c]));
                }
            }
    }
    {   // fold_tables_into: f32 accumulator, d ascending, bias after the sum; the codebook is used as given
        const int64_t C = 3, cd = 7, bins = 5;
        std::vector<float> proj(C * cd), cb(bins * cd), bias(C);
        for (size_t i = 0; i < proj.size(); ++i) proj[i] = mis_synth_value(11, i, 1.0f);
        for (size_t i = 0; i < cb.size(); ++i) cb[i] = mis_synth_value(12, i, 3.0f) / 3.0f;       // pre-scaled by the caller, in its own arithmetic
        for (size_t i = 0; i < bias.size(); ++i) bias[i] = mis_synth_value(13, i, 0.1f);
        const std::vector<float> cb0 = cb;
        bool inexact = false;
        for (const float* b : {(const float*)nullptr, (const float*)bias.data()}) {
            std::vector<float> got(bins * C + 1, 7.0f);
            fold_tables_into(got.data(), proj.data(), cb.data(), b, C, cd, bins);
            for (int64_t v = 0; v < bins; ++v) for (int64_t c = 0; c < C; ++c) {
                float acc = 0.0f;
                double exact = 0.0;
                for (int64_t d = 0; d < cd; ++d) { acc += proj[c * cd + d] * cb[v * cd + d]; exact += (double)proj[c * cd + d] * (double)cb[v * cd + d]; }
                inexact = inexact || (double)acc != exact;
                CHECK(bits(got[v * C + c]) == bits(b ? acc + b[c] : acc));
            }
            CHECK(got[bins * C] == 7.0f);
        }
        CHECK(inexact && cb == cb0);
    }
    {   // arena.lin / arena.conv read prefix.weight / prefix.bias through need(): its shape message, npos without a bias
        HostWeights s("Mimi");
        const float wv[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, bv[2] = {0.5f, -0.5f};
        const int64_t s26[2] = {2, 6}, s223[3] = {2, 2, 3}, s2[1] = {2};
        s.put("l.weight", wv, MIS_F32, s26, 2);
        s.put("l.bias", bv, MIS_F32, s2, 1);
        s.put("c.weight", wv, MIS_F32, s223, 3);
        s.put("c.bias", bv, MIS_F32, s2, 1);
        s.put("n.weight", wv, MIS_F32, s26, 2);
        F32Arena a;
        const F32Lin L = a.lin(s, "l", 2, 6, true);
        CHECK(L.w == 0 && L.b == 12 && L.M == 2 && L.K == 6 && a.host.size() == 16);
        for (int o = 0; o < 2; ++o) for (int i = 0; i < 6; ++i) CHECK(a.host[L.w + i * 2 + o] == wv[o * 6 + i]);
        CHECK(a.host[L.b] == 0.5f && a.host[L.b + 1] == -0.5f);
        const F32Lin N = a.lin(s, "n", 2, 6, false);
        CHECK(N.w == 16 && N.b == F32Lin::npos && N.b == (size_t)-1 && a.host.size() == 28);
        const F32Lin Cv = a.conv(s, "c", 2, 2, 3);
        CHECK(Cv.w == 28 && Cv.b == 40 && Cv.M == 2 && Cv.K == 6 && a.host.size() == 44);
        for (int o = 0; o < 2; ++o) for (int j = 0; j < 2; ++j) for (int c2 = 0; c2 < 3; ++c2) CHECK(a.host[Cv.w + (j * 3 + c2) * 2 + o] == wv[(o * 2 + j) * 3 + c2]);
        CHECK(F32Lin().b == F32Lin::npos);
        m = thrown([&] { a.lin(s, "l", 6, 2, true); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == "Mimi weight l.weight has the wrong shape");
        m = thrown([&] { a.conv(s, "c", 2, 3, 2); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == "Mimi weight c.weight has the wrong shape");
        // a bias of the input's length, not the output's, is refused by lin and by conv themselves
        const float b6[6] = {1, 2, 3, 4, 5, 6}, b3[3] = {1, 2, 3};
        const int64_t s6[1] = {6}, s3[1] = {3};
        s.put("lb.weight", wv, MIS_F32, s26, 2);
        s.put("lb.bias", b6, MIS_F32, s6, 1);
        s.put("cb.weight", wv, MIS_F32, s223, 3);
        s.put("cb.bias", b3, MIS_F32, s3, 1);
        m = thrown([&] { a.lin(s, "lb", 2, 6, true); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == "Mimi weight lb.bias has the wrong shape");
        m = thrown([&] { a.conv(s, "cb", 2, 2, 3); }, &code);
        CHECK(code == (int)MIS_ERR_INVALID_INPUT && m == "Mimi weight cb.bias has the wrong shape");
        CHECK(a.lin(s, "lb", 2, 6, false).b == F32Lin::npos);
        m = thrown([&] { a.lin(s, "n", 2, 6, true); }, &code);
        CHECK(code == (int)MIS_ERR_NOT_INITIALIZED && m == "Mimi weight missing: n.bias");
    }
    {   // synthetic tensors: put k takes key seed + k
        HostWeights s("Moonshine");
        SynthWeights sw{s, 7 * 100000ull};
        sw.lin("p", 2, 3, true, 0.5);
        sw.norm("n", 2);
        CHECK(sw.key == 700004ull);
        const float amp = (float)(0.5 * sqrt(3.0 / 3.0));
        for (int i = 0; i < 6; ++i) CHECK(s.need("p.weight", {2, 3}).v[i] == 0.0f + mis_synth_value(700001ull, i, amp));
        for (int i = 0; i < 2; ++i) {
            CHECK(s.need("p.bias", {2}).v[i] == 0.0f + mis_synth_value(700002ull, i, 0.05f));
            CHECK(s.need("n.weight", {2}).v[i] == 1.0f + mis_synth_value(700003ull, i, 0.1f));
            CHECK(s.need("n.bias", {2}).v[i] == 0.0f + mis_synth_value(700004ull, i, 0.05f));
        }
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("host_weights ok\n");
    return 0;
}
