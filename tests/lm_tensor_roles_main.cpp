// Stand-alone check of csrc/lm_tensor_roles.h (test_lm_tensor_roles_cpu.py builds it with the address and undefined-behaviour sanitizers
// and runs it): lm_tensor_role - kind, layer, expected shape and packed-role placement of every checkpoint key - and lm_required_tensors -
// what a configuration must be given, with its synthetic keys and amplitudes - against constants written out below.  The constants were
// derived by hand from the code these two functions replaced (the per-name branches of place_matrix / place_qmatrix / norm_slot, the
// `want` list of mis_tts_finalize and the two synthetic initialisers of lm_engine.hip).  Host code only: no HIP call, no device.
#include "../mlx-audio-swift_amd/csrc/lm_tensor_roles.h"

#include <stdio.h>
#include <algorithm>
#include <set>

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Want { const char* name; LmKind kind; int layer; int64_t N, K; LmPack pack; int64_t total; int stride, offset; };

static void expect_roles(const LmDims& m, const std::vector<Want>& want) {
    for (const Want& w : want) {
        const LmTensorRole r = lm_tensor_role(m, w.name);
        const bool ok = r.kind == w.kind && r.error == LM_NAME_OK && r.layer == w.layer && r.N == w.N && r.K == w.K && r.pack == w.pack &&
                        r.total_rows == w.total && r.tile_stride == w.stride && r.tile_offset == w.offset;
        if (!ok) {
            printf("FAILED %s: kind %d layer %d [%lld, %lld] pack %d total %lld stride %d offset %d\n", w.name, (int)r.kind, r.layer, (long long)r.N,
                   (long long)r.K, (int)r.pack, (long long)r.total_rows, r.tile_stride, r.tile_offset);
            ++failures;
        }
        CHECK(r.is_matrix() == (w.K != 0) && r.is_vector() == (w.K == 0));
    }
}

struct Req { const char* name; uint64_t key; double amp; int plus_one; };

// the enumeration against the list written out: the same names (as a set, and no name twice), each with its key, amplitude (as the float
// the fill kernels are given) and plus_one flag; every name maps to a role
static void expect_required(const LmDims& m, const std::vector<Req>& want) {
    const std::vector<LmRequiredTensor> got = lm_required_tensors(m);
    std::set<std::string> gs, ws;
    for (const LmRequiredTensor& t : got) gs.insert(t.name);
    for (const Req& w : want) ws.insert(w.name);
    CHECK(gs == ws && gs.size() == got.size() && ws.size() == want.size());
    for (const Req& w : want) {
        auto it = std::find_if(got.begin(), got.end(), [&](const LmRequiredTensor& t) { return t.name == w.name; });
        if (it == got.end()) { printf("FAILED: %s is not enumerated\n", w.name); ++failures; continue; }
        if (it->key != w.key || (float)it->amp != (float)w.amp || it->plus_one != w.plus_one) {
            printf("FAILED %s: key %llu amp %.17g plus_one %d\n", w.name, (unsigned long long)it->key, it->amp, it->plus_one);
            ++failures;
        }
        const LmTensorRole r = lm_tensor_role(m, w.name);
        CHECK(r.is_matrix() || r.is_vector());
    }
}

static void expect_unknown(const LmDims& m, const char* name, LmNameError e) {
    const LmTensorRole r = lm_tensor_role(m, name);
    if (r.kind != LM_UNKNOWN || r.error != e) { printf("FAILED %s: kind %d error %d, wanted unknown with error %d\n", name, (int)r.kind, (int)r.error, (int)e); ++failures; }
    CHECK(!r.is_matrix() && !r.is_vector());
}

int main() {
    const int NONE = 0;     // K of a vector
    // ---- set A: hidden 256, 2 layers, ffn 512, 2 query heads / 1 kv head x 128, vocabulary 640, untied.  H*D = 256, Hkv*D = 128, q|k|v rows 512
    const LmDims A = {256, 2, 512, 2, 1, 128, 640, false, false};
    expect_roles(A, {
        {"model.embed_tokens.weight", LM_EMBEDDING, 0, 640, 256, LM_PACK_NONE, 0, 1, 0},
        {"lm_head.weight", LM_HEAD, 0, 640, 256, LM_PACK_HEAD, 640, 1, 0},
        {"model.norm.weight", LM_FINAL_NORM, 0, 256, NONE, LM_PACK_NONE, 0, 1, 0},
        {"model.layers.0.input_layernorm.weight", LM_INPUT_NORM, 0, 256, NONE, LM_PACK_NONE, 0, 1, 0},
        {"model.layers.1.post_attention_layernorm.weight", LM_POST_NORM, 1, 256, NONE, LM_PACK_NONE, 0, 1, 0},
        {"model.layers.0.self_attn.q_proj.weight", LM_Q, 0, 256, 256, LM_PACK_QKV, 512, 1, 0},
        {"model.layers.1.self_attn.q_proj.weight", LM_Q, 1, 256, 256, LM_PACK_QKV, 512, 1, 0},
        {"model.layers.1.self_attn.k_proj.weight", LM_K, 1, 128, 256, LM_PACK_QKV, 512, 1, 16},      // behind q: 256 / 16 tiles
        {"model.layers.1.self_attn.v_proj.weight", LM_V, 1, 128, 256, LM_PACK_QKV, 512, 1, 24},      // behind q and k: (256 + 128) / 16
        {"model.layers.0.self_attn.o_proj.weight", LM_O, 0, 256, 256, LM_PACK_O, 256, 1, 0},
        {"model.layers.0.mlp.gate_proj.weight", LM_GATE, 0, 512, 256, LM_PACK_GU, 1024, 2, 0},       // gate / up tiles interleave
        {"model.layers.1.mlp.up_proj.weight", LM_UP, 1, 512, 256, LM_PACK_GU, 1024, 2, 1},
        {"model.layers.1.mlp.down_proj.weight", LM_DOWN, 1, 256, 512, LM_PACK_DOWN, 256, 1, 0},
        {"model.layers.x.mlp.up_proj.weight", LM_UP, 0, 512, 256, LM_PACK_GU, 1024, 2, 1},           // atoi("x") = 0: layer 0, as before
    });
    const double e = 0.8660254037844386, h = 0.21650635094610965, qk = 0.16237976320958225, w = 0.10825317547305482,
                 o = 0.05412658773652741, dn = 0.038273277230987154;   // 0.5 sqrt 3; sqrt(3/256) x 2, x 1.5, x 1, x 0.5; sqrt(3/512) x 0.5
    expect_required(A, {
        {"model.embed_tokens.weight", 1, e, 0}, {"model.norm.weight", 2, 0.1, 1}, {"lm_head.weight", 3, h, 0},
        {"model.layers.0.input_layernorm.weight", 100, 0.1, 1}, {"model.layers.0.post_attention_layernorm.weight", 101, 0.1, 1},
        {"model.layers.0.self_attn.q_proj.weight", 102, qk, 0}, {"model.layers.0.self_attn.k_proj.weight", 103, qk, 0},
        {"model.layers.0.self_attn.v_proj.weight", 104, w, 0}, {"model.layers.0.self_attn.o_proj.weight", 105, o, 0},
        {"model.layers.0.mlp.gate_proj.weight", 106, w, 0}, {"model.layers.0.mlp.up_proj.weight", 107, w, 0},
        {"model.layers.0.mlp.down_proj.weight", 108, dn, 0},
        {"model.layers.1.input_layernorm.weight", 116, 0.1, 1}, {"model.layers.1.post_attention_layernorm.weight", 117, 0.1, 1},
        {"model.layers.1.self_attn.q_proj.weight", 118, qk, 0}, {"model.layers.1.self_attn.k_proj.weight", 119, qk, 0},
        {"model.layers.1.self_attn.v_proj.weight", 120, w, 0}, {"model.layers.1.self_attn.o_proj.weight", 121, o, 0},
        {"model.layers.1.mlp.gate_proj.weight", 122, w, 0}, {"model.layers.1.mlp.up_proj.weight", 123, w, 0},
        {"model.layers.1.mlp.down_proj.weight", 124, dn, 0},
    });
    CHECK(lm_tensor_role(A, "model.layers.0.self_attn.rotary_emb.inv_freq").kind == LM_IGNORED);
    CHECK(lm_tensor_role(A, "rotary_emb.inv_freq").kind == LM_IGNORED);
    expect_unknown(A, "model.layers.0.self_attn.q_norm.weight", LM_NAME_UNEXPECTED);                  // qk_norm off
    expect_unknown(A, "model.layers.1.self_attn.k_norm.weight", LM_NAME_UNEXPECTED);
    expect_unknown(A, "model.layers.2.mlp.up_proj.weight", LM_NAME_LAYER_RANGE);                      // index = L
    expect_unknown(A, "model.layers.-1.mlp.up_proj.weight", LM_NAME_LAYER_RANGE);
    expect_unknown(A, "model.layers.1", LM_NAME_BAD);                                                  // no key behind the index
    expect_unknown(A, "model.layer.0.mlp.up_proj.weight", LM_NAME_UNEXPECTED);
    expect_unknown(A, "foo", LM_NAME_UNEXPECTED);
    expect_unknown(A, "model.layers.0.mlp.up_proj.bias", LM_NAME_UNEXPECTED);

    // ---- set B: tied, qk_norm, head_dim 64, vocabulary 100 (hidden 256, 2 layers, ffn 512, 4 / 2 heads): H*D = 256, Hkv*D = 128
    const LmDims B = {256, 2, 512, 4, 2, 64, 100, true, true};
    expect_roles(B, {
        {"model.embed_tokens.weight", LM_EMBEDDING, 0, 100, 256, LM_PACK_NONE, 0, 1, 0},
        {"model.norm.weight", LM_FINAL_NORM, 0, 256, NONE, LM_PACK_NONE, 0, 1, 0},
        {"model.layers.1.input_layernorm.weight", LM_INPUT_NORM, 1, 256, NONE, LM_PACK_NONE, 0, 1, 0},
        {"model.layers.0.post_attention_layernorm.weight", LM_POST_NORM, 0, 256, NONE, LM_PACK_NONE, 0, 1, 0},
        {"model.layers.0.self_attn.q_norm.weight", LM_Q_NORM, 0, 64, NONE, LM_PACK_NONE, 0, 1, 0},
        {"model.layers.1.self_attn.k_norm.weight", LM_K_NORM, 1, 64, NONE, LM_PACK_NONE, 0, 1, 0},
        {"model.layers.0.self_attn.q_proj.weight", LM_Q, 0, 256, 256, LM_PACK_QKV, 512, 1, 0},
        {"model.layers.0.self_attn.k_proj.weight", LM_K, 0, 128, 256, LM_PACK_QKV, 512, 1, 16},
        {"model.layers.0.self_attn.v_proj.weight", LM_V, 0, 128, 256, LM_PACK_QKV, 512, 1, 24},
        {"model.layers.1.self_attn.o_proj.weight", LM_O, 1, 256, 256, LM_PACK_O, 256, 1, 0},
        {"model.layers.1.mlp.gate_proj.weight", LM_GATE, 1, 512, 256, LM_PACK_GU, 1024, 2, 0},
        {"model.layers.0.mlp.up_proj.weight", LM_UP, 0, 512, 256, LM_PACK_GU, 1024, 2, 1},
        {"model.layers.0.mlp.down_proj.weight", LM_DOWN, 0, 256, 512, LM_PACK_DOWN, 256, 1, 0},
    });
    expect_required(B, {
        {"model.embed_tokens.weight", 1, e, 0}, {"model.norm.weight", 2, 0.1, 1},
        {"model.layers.0.input_layernorm.weight", 100, 0.1, 1}, {"model.layers.0.post_attention_layernorm.weight", 101, 0.1, 1},
        {"model.layers.0.self_attn.q_proj.weight", 102, qk, 0}, {"model.layers.0.self_attn.k_proj.weight", 103, qk, 0},
        {"model.layers.0.self_attn.v_proj.weight", 104, w, 0}, {"model.layers.0.self_attn.o_proj.weight", 105, o, 0},
        {"model.layers.0.mlp.gate_proj.weight", 106, w, 0}, {"model.layers.0.mlp.up_proj.weight", 107, w, 0},
        {"model.layers.0.mlp.down_proj.weight", 108, dn, 0},
        {"model.layers.0.self_attn.q_norm.weight", 109, 0.1, 1}, {"model.layers.0.self_attn.k_norm.weight", 110, 0.1, 1},
        {"model.layers.1.input_layernorm.weight", 116, 0.1, 1}, {"model.layers.1.post_attention_layernorm.weight", 117, 0.1, 1},
        {"model.layers.1.self_attn.q_proj.weight", 118, qk, 0}, {"model.layers.1.self_attn.k_proj.weight", 119, qk, 0},
        {"model.layers.1.self_attn.v_proj.weight", 120, w, 0}, {"model.layers.1.self_attn.o_proj.weight", 121, o, 0},
        {"model.layers.1.mlp.gate_proj.weight", 122, w, 0}, {"model.layers.1.mlp.up_proj.weight", 123, w, 0},
        {"model.layers.1.mlp.down_proj.weight", 124, dn, 0},
        {"model.layers.1.self_attn.q_norm.weight", 125, 0.1, 1}, {"model.layers.1.self_attn.k_norm.weight", 126, 0.1, 1},
    });
    CHECK(lm_tensor_role(B, "lm_head.weight").kind == LM_IGNORED);                                     // tied
    CHECK(lm_tensor_role(B, "model.layers.1.self_attn.rotary_emb.inv_freq").kind == LM_IGNORED);
    expect_unknown(B, "model.layers.2.self_attn.q_norm.weight", LM_NAME_LAYER_RANGE);

    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("lm_tensor_roles ok\n");
    return 0;
}
