// host_weights.h - a model's checkpoint tensors between set_tensor and finalize, widened to f32 on the host (HostWeights), and the
// weight arenas that finalize assembles from them and uploads once: bf16 + f32 for the LM-shaped and the small audio models (HostArena:
// one pass, every take bound to the pointer that will address it; fold_bn_dwconv), exact f32 with the codec re-layouts for the codec
// engines (F32Arena, lin_t / conv_taps_t / convt_phases_t / fold_tables_into).  set_tensor_check is the preamble of every set_tensor.
#pragma once
#include "common.h"

#include <math.h>
#include <string.h>

struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
};

class HostWeights {
public:
    // label: the model's name in the messages; missing: the status of a weight that was never set
    explicit HostWeights(const char* label, mis_status missing = MIS_ERR_NOT_INITIALIZED) : label_(label), missing_(missing) {}

    // the element count of a shape; an entry <= 0 is rejected
    static size_t count(const int64_t* shape, int ndim) {
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) { MIS_REQUIRE(shape[i] > 0, MIS_ERR_INVALID_INPUT, "bad shape"); n *= (size_t)shape[i]; }
        return n;
    }
    // host bytes of dtype f32 / f16 / bf16, widened to f32; a tensor of the same name is replaced
    void put(const std::string& name, const void* host, mis_dtype dtype, const int64_t* shape, int ndim) {
        HostTensor t;
        const size_t n = count(shape, ndim);
        t.shape.assign(shape, shape + ndim);
        t.v.resize(n);
        const uint16_t* s = static_cast<const uint16_t*>(host);
        if (dtype == MIS_F32) memcpy(t.v.data(), host, n * 4);
        else if (dtype == MIS_BF16) for (size_t i = 0; i < n; ++i) t.v[i] = bf16_to_f32(s[i]);
        else if (dtype == MIS_F16) for (size_t i = 0; i < n; ++i) t.v[i] = f16_to_f32_host(s[i]);
        else throw MisError(MIS_ERR_INVALID_INPUT, "unsupported dtype");
        put(name, std::move(t));
    }
    void put(const std::string& name, HostTensor&& t) { map_[name] = std::move(t); }
    // set_tensor's staging copy: the caller's pointer may be a device one (of `device`)
    void put_staged(int device, const std::string& name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
        std::vector<uint8_t> host(count(shape, ndim) * (dtype == MIS_F32 ? 4 : 2));
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipMemcpy(host.data(), data, host.size(), hipMemcpyDefault));
        put(name, host.data(), dtype, shape, ndim);
    }

    const HostTensor& need(const std::string& name) const {
        auto it = map_.find(name);
        MIS_REQUIRE(it != map_.end(), missing_, "%s weight missing: %s", label_, name.c_str());
        return it->second;
    }
    const HostTensor& need(const std::string& name, std::initializer_list<int64_t> shape) const {
        const HostTensor& t = need(name);
        MIS_REQUIRE(t.shape == std::vector<int64_t>(shape), MIS_ERR_INVALID_INPUT, "%s weight %s has the wrong shape", label_, name.c_str());
        return t;
    }
    // nullptr: not set
    const HostTensor* find(const std::string& name) const {
        auto it = map_.find(name);
        return it == map_.end() ? nullptr : &it->second;
    }
    size_t count(const std::string& name) const { return map_.count(name); }
    void clear() { map_.clear(); }
    std::map<std::string, HostTensor>::const_iterator begin() const { return map_.begin(); }
    std::map<std::string, HostTensor>::const_iterator end() const { return map_.end(); }

private:
    const char* label_;
    mis_status missing_;
    std::map<std::string, HostTensor> map_;
};

// what every engine's set_tensor asks before it stores a tensor: arguments, not finalized yet, a dtype put() can widen
static inline void set_tensor_check(const void* handle, const char* name, const void* data, const int64_t* shape, int ndim, int max_ndim, bool finalized,
                                    mis_dtype dtype) {
    MIS_REQUIRE(handle && name && data && shape && ndim >= 1 && ndim <= max_ndim, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(!finalized, MIS_ERR_INVALID_INPUT, "set_tensor after finalize");
    MIS_REQUIRE(dtype == MIS_F32 || dtype == MIS_F16 || dtype == MIS_BF16, MIS_ERR_INVALID_INPUT, "unsupported dtype");
}

// mis-synth-v1 tensors (oracle/synth.py) for init_synthetic: every put takes the next key, value i is plus + synth(key, i, amp)
struct SynthWeights {
    HostWeights& w;
    uint64_t key;
    void put(const std::string& name, std::vector<int64_t> shape, double amp, float plus) {
        HostTensor t;
        size_t n = 1;
        for (auto v : shape) n *= (size_t)v;
        t.shape = shape; t.v.resize(n);
        ++key;
        for (size_t i = 0; i < n; ++i) t.v[i] = plus + mis_synth_value(key, i, (float)amp);
        w.put(name, std::move(t));
    }
    void lin(const std::string& p, int64_t o, int64_t i, bool bias, double gain) {
        put(p + ".weight", {o, i}, gain * sqrt(3.0 / (double)i), 0.0f);
        if (bias) put(p + ".bias", {o}, 0.05, 0.0f);
    }
    void norm(const std::string& p, int64_t n) { put(p + ".weight", {n}, 0.1, 1.0f); put(p + ".bias", {n}, 0.05, 0.0f); }
};

// The bf16 arena and the f32 arena of a model, assembled on the host in ONE pass: an f32 checkpoint is rounded to bf16 once, here.
// Offsets count elements and are multiples of 64; what nobody writes stays zero.  A model's own packers write through `host` / `fhost`.
//
// Every take can name the pointer that will address it on the device (bf16_t*&, float*& or const float*&): the arena keeps (address
// of the pointer, offset) and resolve() - which upload() calls once the device buffers exist - writes base + offset into each.  THE
// RULE: a destination stays at its address until upload() returns.  Size the vectors of layer structs before the loop that binds into
// them; members of the handle and locals of finalize are fine.  An offset may be bound more than once (tied weights); a pointer nobody
// binds keeps its value (nullptr: an absent bias).
struct HostArena {
    const HostWeights& w;
    std::vector<bf16_t> host;
    std::vector<float> fhost;
    explicit HostArena(const HostWeights& weights) : w(weights) {}
    HostArena(const HostArena&) = delete;
    HostArena& operator=(const HostArena&) = delete;

    // offsets a model's own packers filled
    void bind(bf16_t*& dst, size_t off) { binds_.push_back({&dst, off, BF16}); }
    void bind(float*& dst, size_t off) { binds_.push_back({&dst, off, F32}); }
    void bind(const float*& dst, size_t off) { binds_.push_back({&dst, off, CF32}); }

    size_t btake(size_t n) { size_t off = host.size(); host.resize(off + round_up(n, 64), 0); return off; }
    size_t ftake(size_t n) { size_t off = fhost.size(); fhost.resize(off + round_up(n, 64), 0.0f); return off; }
    void bmat_into(const std::string& name, int64_t N, int64_t K, size_t off) {
        const HostTensor& t = w.need(name, {N, K});
        for (size_t i = 0; i < (size_t)N * K; ++i) host[off + i] = f32_to_bf16(t.v[i]);
    }
    size_t bmat(const std::string& name, int64_t N, int64_t K) { size_t off = btake((size_t)N * K); bmat_into(name, N, K, off); return off; }
    size_t bvec(const std::string& name, int64_t n) {
        const HostTensor& t = w.need(name, {n});
        size_t off = btake(n);
        for (int64_t i = 0; i < n; ++i) host[off + i] = f32_to_bf16(t.v[i]);
        return off;
    }
    // the first n values of a tensor of the given shape, as stored
    size_t fvec(const std::string& name, std::initializer_list<int64_t> shape, int64_t n) {
        const HostTensor& t = w.need(name, shape);
        size_t off = ftake(n);
        for (int64_t i = 0; i < n; ++i) fhost[off + i] = t.v[i];
        return off;
    }
    // the same takes, bound to their destination
    size_t btake(size_t n, bf16_t*& dst) { return bound(dst, btake(n)); }
    size_t bmat(const std::string& name, int64_t N, int64_t K, bf16_t*& dst) { return bound(dst, bmat(name, N, K)); }
    size_t bvec(const std::string& name, int64_t n, bf16_t*& dst) { return bound(dst, bvec(name, n)); }
    template <class F> size_t ftake(size_t n, F*& dst) { return bound(dst, ftake(n)); }
    template <class F> size_t fvec(const std::string& name, std::initializer_list<int64_t> shape, int64_t n, F*& dst) { return bound(dst, fvec(name, shape, n)); }

    // host only: every bound pointer = its arena's base + its offset
    void resolve(bf16_t* A, float* F) const {
        for (const Bind& b : binds_) {
            if (b.kind == BF16) *static_cast<bf16_t**>(b.dst) = A + b.off;
            else if (b.kind == F32) *static_cast<float**>(b.dst) = F + b.off;
            else *static_cast<const float**>(b.dst) = F + b.off;
        }
    }
    void upload(DevBuf<bf16_t>& arena, DevBuf<float>& farena) const {
        arena.alloc(host.size());
        farena.alloc(fhost.size());
        HIP_CHECK(hipMemcpy(arena.p, host.data(), host.size() * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(farena.p, fhost.data(), fhost.size() * 4, hipMemcpyHostToDevice));
        resolve(arena.p, farena.p);
    }

private:
    enum Kind { BF16, F32, CF32 };
    struct Bind { void* dst; size_t off; Kind kind; };
    std::vector<Bind> binds_;
    template <class T> size_t bound(T*& dst, size_t off) { bind(dst, off); return off; }
};

// Inference BatchNorm (eps 1e-5, the MLXNN default) folded into depthwise taps dw [d][k] (+ bias [d], or null) in f32:
// taps_out [k][d] = dw scale, shift_out [d] = (bias - mean) scale + bn_b, scale = bn_w / sqrt(var + eps).  Both Conformer engines.
static inline void fold_bn_dwconv(float* taps_out, float* shift_out, const float* dw, const float* dw_bias, const float* bn_w, const float* bn_b,
                                  const float* mean, const float* var, int64_t d, int64_t k) {
    for (int64_t ch = 0; ch < d; ++ch) {
        const float scale = bn_w[ch] / sqrtf(var[ch] + 1e-5f);
        for (int64_t j = 0; j < k; ++j) taps_out[j * d + ch] = dw[ch * k + j] * scale;
        shift_out[ch] = ((dw_bias ? dw_bias[ch] : 0.0f) - mean[ch]) * scale + bn_b[ch];
    }
}

// ---------------------------------------------------------------------------- exact-f32 codec arenas
// Re-layouts of checkpoint weights into the A^T operands of launch_gemm (codec_kernels.h); plain index arithmetic, no rounding.
// Linear [out][in] -> A^T [in][out]
static inline std::vector<float> lin_t(const std::vector<float>& w, int64_t out, int64_t in) {
    std::vector<float> at((size_t)in * out);
    for (int64_t o = 0; o < out; ++o) for (int64_t i = 0; i < in; ++i) at[i * out + o] = w[o * in + i];
    return at;
}
// dense conv [co][k][ci] -> A^T [(j ci + c)][co]
static inline std::vector<float> conv_taps_t(const std::vector<float>& w, int64_t co, int64_t k, int64_t ci) {
    std::vector<float> at((size_t)k * ci * co);
    for (int64_t o = 0; o < co; ++o) for (int64_t j = 0; j < k; ++j) for (int64_t c = 0; c < ci; ++c) at[(j * ci + c) * co + o] = w[(o * k + j) * ci + c];
    return at;
}
// transposed conv (k taps, stride s, k / s taps per output phase) [co][k][ci], or [ci][k][co] when in_major -> [s][(j ci + c)][co]:
// output phase ph (o = s n + ph) takes tap ((ph + pad) % s) + s j from x[n + (ph + pad) / s - j]
static inline std::vector<float> convt_phases_t(const std::vector<float>& w, int64_t co, int64_t k, int64_t ci, int64_t s, int64_t pad, bool in_major) {
    const int64_t nt = k / s;
    std::vector<float> at((size_t)s * nt * ci * co);
    for (int64_t ph = 0; ph < s; ++ph) for (int64_t j = 0; j < nt; ++j) {
        const int64_t tap = (ph + pad) % s + s * j;
        for (int64_t c = 0; c < ci; ++c) for (int64_t o = 0; o < co; ++o)
            at[((ph * nt + j) * ci + c) * co + o] = in_major ? w[(c * k + tap) * co + o] : w[(o * k + tap) * ci + c];
    }
    return at;
}
// folded quantiser table dst[code][c] = sum_d proj[c][d] codebook[code][d] (+ bias[c]): f32 accumulator, d ascending, bias after the
// sum.  The codebook is taken as given: a caller that normalises it does so first, in its own arithmetic.
static inline void fold_tables_into(float* dst, const float* proj, const float* codebook, const float* bias, int64_t C, int64_t cd, int64_t bins) {
    for (int64_t v = 0; v < bins; ++v)
        for (int64_t c = 0; c < C; ++c) {
            float acc = 0.0f;
            for (int64_t d = 0; d < cd; ++d) acc += proj[c * cd + d] * codebook[v * cd + d];
            dst[v * C + c] = bias ? acc + bias[c] : acc;
        }
}

// one contraction's operands in an F32Arena: A^T at w ([K][M]), bias at b (npos: none); offsets count floats
struct F32Lin {
    static constexpr size_t npos = (size_t)-1;
    size_t w = 0, b = npos;
    int M = 0, K = 0;
};

// The f32 arena of a codec engine, assembled on the host in push order.  Offsets count floats and are multiples of 4 (they feed 16-byte
// loads): every push pads the arena with zeros to the next multiple.
struct F32Arena {
    std::vector<float> host;

    size_t push(const std::vector<float>& v) {
        const size_t o = host.size();
        host.insert(host.end(), v.begin(), v.end());
        host.resize(round_up(host.size(), 4), 0.0f);
        return o;
    }
    size_t zeros(size_t n) { return push(std::vector<float>(n, 0.0f)); }
    // a re-laid-out A^T [K][M] and its bias (nullptr: none)
    F32Lin packed(const std::vector<float>& at, int64_t M, int64_t K, const std::vector<float>* bias) {
        F32Lin L;
        L.M = (int)M; L.K = (int)K;
        L.w = push(at);
        if (bias) L.b = push(*bias);
        return L;
    }
    // prefix.weight [out][in] (+ prefix.bias [out])
    F32Lin lin(const HostWeights& s, const std::string& prefix, int64_t out, int64_t in, bool bias) {
        const std::vector<float> at = lin_t(s.need(prefix + ".weight", {out, in}).v, out, in);
        return packed(at, out, in, bias ? &s.need(prefix + ".bias", {out}).v : nullptr);
    }
    // prefix.weight [co][k][ci], prefix.bias [co]
    F32Lin conv(const HostWeights& s, const std::string& prefix, int64_t co, int64_t k, int64_t ci) {
        const std::vector<float> at = conv_taps_t(s.need(prefix + ".weight", {co, k, ci}).v, co, k, ci);
        return packed(at, co, k * ci, &s.need(prefix + ".bias", {co}).v);
    }
    void upload(DevBuf<float>& arena) const {
        arena.alloc(host.size());
        HIP_CHECK(hipMemcpy(arena.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    }
};
