// lm_tensor_roles.h - what a checkpoint key of a Llama-shaped LM is: host code only, no HIP call (tests/lm_tensor_roles_main.cpp builds
// it stand-alone).  lm_tensor_role names a key once - kind, layer, expected shape and, for a matrix, where its tiles go in the packed
// role (q|k|v share one, gate / up interleave in one) - and lm_required_tensors lists what a configuration must be given, with the
// mis-synth-v1 keys and amplitudes (oracle/llama.py make_synthetic_weights).  lm_engine.hip places, checks and synthesises from these.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <vector>

struct LmDims { int d, L, ff, H, Hkv, D, V; bool tie_word_embeddings, qk_norm; };

enum LmKind {
    LM_IGNORED,        // rotary_emb.inv_freq (sanitize, LlamaTTS.swift:584-586); lm_head.weight of a tied model (:588-590)
    LM_EMBEDDING, LM_HEAD, LM_Q, LM_K, LM_V, LM_O, LM_GATE, LM_UP, LM_DOWN,
    LM_FINAL_NORM, LM_INPUT_NORM, LM_POST_NORM, LM_Q_NORM, LM_K_NORM,
    LM_UNKNOWN
};
enum LmPack { LM_PACK_NONE = -1, LM_PACK_QKV = 0, LM_PACK_O = 1, LM_PACK_GU = 2, LM_PACK_DOWN = 3, LM_PACK_HEAD = 4 };   // = mis_tts_native_quant_bits roles
enum LmNameError { LM_NAME_OK, LM_NAME_UNEXPECTED, LM_NAME_BAD, LM_NAME_LAYER_RANGE };   // "unexpected tensor", "bad tensor name", "layer index out of range in"

struct LmTensorRole {
    LmKind kind = LM_UNKNOWN;
    LmNameError error = LM_NAME_OK;          // why kind is LM_UNKNOWN
    int layer = 0;
    int64_t N = 0, K = 0;                    // expected shape: [N, K], a vector [N] (K = 0)
    LmPack pack = LM_PACK_NONE;              // matrices of the decode step: the packed role,
    int64_t total_rows = 0;                  //   its rows (per layer),
    int tile_stride = 1, tile_offset = 0;    //   and this matrix's n-tile t at tile t * tile_stride + tile_offset of it
    bool is_matrix() const { return kind >= LM_EMBEDDING && kind <= LM_DOWN; }
    bool is_vector() const { return kind >= LM_FINAL_NORM && kind <= LM_K_NORM; }
};

static inline LmTensorRole lm_tensor_role(const LmDims& m, const std::string& name) {
    LmTensorRole r;
    const int64_t HD = (int64_t)m.H * m.D, KD = (int64_t)m.Hkv * m.D;
    auto matrix = [&](LmKind kind, int64_t N, int64_t K, LmPack pack, int64_t total, int stride, int offset) {
        r.kind = kind; r.N = N; r.K = K; r.pack = pack; r.total_rows = total; r.tile_stride = stride; r.tile_offset = offset;
        return r;
    };
    auto vector_of = [&](LmKind kind, int64_t n) { r.kind = kind; r.N = n; return r; };
    auto unknown = [&](LmNameError e) { r.kind = LM_UNKNOWN; r.error = e; return r; };
    if (name.find("rotary_emb.inv_freq") != std::string::npos) { r.kind = LM_IGNORED; return r; }
    if (name == "lm_head.weight") {
        if (m.tie_word_embeddings) { r.kind = LM_IGNORED; return r; }
        return matrix(LM_HEAD, m.V, m.d, LM_PACK_HEAD, m.V, 1, 0);
    }
    if (name == "model.embed_tokens.weight") return matrix(LM_EMBEDDING, m.V, m.d, LM_PACK_NONE, 0, 1, 0);
    if (name == "model.norm.weight") return vector_of(LM_FINAL_NORM, m.d);
    const std::string pre = "model.layers.";
    if (name.rfind(pre, 0) != 0) return unknown(LM_NAME_UNEXPECTED);
    const size_t dot = name.find('.', pre.size());
    if (dot == std::string::npos) return unknown(LM_NAME_BAD);
    r.layer = atoi(name.substr(pre.size(), dot - pre.size()).c_str());      // atoi: "x" reads as layer 0, as it always has
    if (r.layer < 0 || r.layer >= m.L) return unknown(LM_NAME_LAYER_RANGE);
    const std::string rest = name.substr(dot + 1);
    if (rest == "self_attn.q_proj.weight") return matrix(LM_Q, HD, m.d, LM_PACK_QKV, HD + 2 * KD, 1, 0);
    if (rest == "self_attn.k_proj.weight") return matrix(LM_K, KD, m.d, LM_PACK_QKV, HD + 2 * KD, 1, (int)(HD / 16));
    if (rest == "self_attn.v_proj.weight") return matrix(LM_V, KD, m.d, LM_PACK_QKV, HD + 2 * KD, 1, (int)((HD + KD) / 16));
    if (rest == "self_attn.o_proj.weight") return matrix(LM_O, m.d, HD, LM_PACK_O, m.d, 1, 0);
    if (rest == "mlp.gate_proj.weight") return matrix(LM_GATE, m.ff, m.d, LM_PACK_GU, 2 * (int64_t)m.ff, 2, 0);
    if (rest == "mlp.up_proj.weight") return matrix(LM_UP, m.ff, m.d, LM_PACK_GU, 2 * (int64_t)m.ff, 2, 1);
    if (rest == "mlp.down_proj.weight") return matrix(LM_DOWN, m.d, m.ff, LM_PACK_DOWN, m.d, 1, 0);
    if (rest == "input_layernorm.weight") return vector_of(LM_INPUT_NORM, m.d);
    if (rest == "post_attention_layernorm.weight") return vector_of(LM_POST_NORM, m.d);
    if (m.qk_norm && rest == "self_attn.q_norm.weight") return vector_of(LM_Q_NORM, m.D);
    if (m.qk_norm && rest == "self_attn.k_norm.weight") return vector_of(LM_K_NORM, m.D);
    return unknown(LM_NAME_UNEXPECTED);
}

// one tensor a configuration requires; key / amp / plus_one: its mis-synth-v1 fill (seed * 100000 + key; plus_one: 1 + U(+-amp))
struct LmRequiredTensor { std::string name; uint64_t key; double amp; int plus_one; };

static inline std::vector<LmRequiredTensor> lm_required_tensors(const LmDims& m) {
    const double d = m.d, HD = (double)m.H * m.D, ff = m.ff;
    std::vector<LmRequiredTensor> out = {{"model.embed_tokens.weight", 1, 0.5 * sqrt(3.0), 0}, {"model.norm.weight", 2, 0.1, 1}};
    if (!m.tie_word_embeddings) out.push_back({"lm_head.weight", 3, sqrt(3.0 / d) * 2.0, 0});
    for (int li = 0; li < m.L; ++li) {
        const std::string p = "model.layers." + std::to_string(li);
        const uint64_t k = 100 + (uint64_t)li * 16;
        out.push_back({p + ".input_layernorm.weight", k + 0, 0.1, 1});
        out.push_back({p + ".post_attention_layernorm.weight", k + 1, 0.1, 1});
        out.push_back({p + ".self_attn.q_proj.weight", k + 2, sqrt(3.0 / d) * 1.5, 0});
        out.push_back({p + ".self_attn.k_proj.weight", k + 3, sqrt(3.0 / d) * 1.5, 0});
        out.push_back({p + ".self_attn.v_proj.weight", k + 4, sqrt(3.0 / d), 0});
        out.push_back({p + ".self_attn.o_proj.weight", k + 5, sqrt(3.0 / HD) * 0.5, 0});
        out.push_back({p + ".mlp.gate_proj.weight", k + 6, sqrt(3.0 / d), 0});
        out.push_back({p + ".mlp.up_proj.weight", k + 7, sqrt(3.0 / d), 0});
        out.push_back({p + ".mlp.down_proj.weight", k + 8, sqrt(3.0 / ff) * 0.5, 0});
        if (m.qk_norm) {
            out.push_back({p + ".self_attn.q_norm.weight", k + 9, 0.1, 1});
            out.push_back({p + ".self_attn.k_norm.weight", k + 10, 0.1, 1});
        }
    }
    return out;
}
