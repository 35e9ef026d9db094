// host_weights.h - a model's checkpoint tensors between set_tensor and finalize, widened to f32 on the host (HostWeights), and the
// bf16 / f32 weight arenas that finalize assembles from them and uploads once (HostArena).
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

// The bf16 arena and the f32 arena of a model, assembled on the host: an f32 checkpoint is rounded to bf16 once, here.  Offsets count
// elements and are multiples of 64; what nobody writes stays zero.  A model's own packers write through `host` / `fhost`.
struct HostArena {
    const HostWeights& w;
    std::vector<bf16_t> host;
    std::vector<float> fhost;
    explicit HostArena(const HostWeights& weights) : w(weights) {}

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
    void upload(DevBuf<bf16_t>& arena, DevBuf<float>& farena) const {
        arena.alloc(host.size());
        farena.alloc(fhost.size());
        HIP_CHECK(hipMemcpy(arena.p, host.data(), host.size() * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(farena.p, fhost.data(), fhost.size() * 4, hipMemcpyHostToDevice));
    }
};
