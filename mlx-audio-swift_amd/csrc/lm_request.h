// lm_request.h - the two pure pieces of the Orpheus / VyvoTTS / Soprano generate call (lm_engine.hip): the host-built request state
// (left-padded prompt matrix, all_ids, repetition windows) and the plan of the codec sub-batches behind the token loop.  Host code
// only: no kernel, no device call (tests/lm_request_main.cpp runs both under the sanitizers without a device).
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------- the request
struct LmRequest {
    int Lmax = 0;                       // longest prompt
    int all_stride = 0;                 // Lmax + max_tokens
    int ctx = 0;                        // max(repetition_context, 0)
    std::vector<int32_t> pm;            // [batch][Lmax] prompts, left-padded with 0
    std::vector<int32_t> all;           // [batch][all_stride] prompts, left-aligned (the generated tokens follow on the device)
    std::vector<int32_t> win, wl;       // [batch][max(ctx, 1)] repetition windows, right-aligned, and their fill
    std::vector<int32_t> alen;          // [batch] tokens in `all`
};

// tokens of all prompts together; a row without a prompt is an error
static size_t lm_prompt_tokens(const std::vector<int32_t>& lens) {
    size_t total = 0;
    for (size_t b = 0; b < lens.size(); ++b) {
        MIS_REQUIRE(lens[b] >= 1, MIS_ERR_INVALID_INPUT, "empty prompt in row %d", (int)b);
        total += lens[b];
    }
    return total;
}

// flat_ids: the prompts one behind the other, lm_prompt_tokens(lens) ids
static LmRequest build_lm_request(const std::vector<int32_t>& lens, const std::vector<int32_t>& flat_ids, int vocab, int max_tokens,
                                  int repetition_context, int sampler_flavor) {
    const int batch = (int)lens.size();
    MIS_REQUIRE(flat_ids.size() == lm_prompt_tokens(lens), MIS_ERR_INVALID_INPUT, "prompt ids do not match the prompt lengths");
    for (auto t : flat_ids) MIS_REQUIRE(t >= 0 && t < vocab, MIS_ERR_INVALID_INPUT, "prompt token %d outside the vocabulary", t);
    LmRequest r;
    for (int b = 0; b < batch; ++b) r.Lmax = std::max(r.Lmax, lens[b]);
    r.ctx = std::max(repetition_context, 0);
    r.all_stride = r.Lmax + max_tokens;
    const int Lmax = r.Lmax, ctx = r.ctx;
    r.pm.assign((size_t)batch * Lmax, 0);
    r.all.assign((size_t)batch * r.all_stride, 0);
    r.win.assign((size_t)batch * std::max(ctx, 1), 0);
    r.wl.assign(batch, 0);
    r.alen.resize(batch);
    size_t off = 0;
    for (int b = 0; b < batch; ++b) {
        for (int j = 0; j < lens[b]; ++j) {
            r.pm[(size_t)b * Lmax + (Lmax - lens[b]) + j] = flat_ids[off + j];
            r.all[(size_t)b * r.all_stride + j] = flat_ids[off + j];
        }
        int w = std::min(ctx, lens[b]);                 // processor.prompt(promptTokens), LlamaTTS.swift:695-696
        if (sampler_flavor == 1) w = 0;                 // Soprano penalises generated tokens only (Soprano.swift:833-848)
        for (int j = 0; j < w; ++j) r.win[(size_t)b * ctx + (ctx - w) + j] = flat_ids[off + lens[b] - w + j];
        r.wl[b] = w;
        r.alen[b] = lens[b];
        off += lens[b];
    }
    return r;
}

// ---------------------------------------------------------------------------- the codec sub-batches
// One SNAC decode: `rows` (in this order) with `gc` groups each, their codes read at code_off of the row's code list, their samples
// written at group_off groups of the row's PCM.
struct SnacDecodeStep {
    int ci = 0;                         // chunk index (0 on the whole-utterance path)
    int gc = 0;                         // groups per row
    std::vector<int32_t> rows;
    int64_t code_off = 0;               // ci * chunk * 7
    int64_t group_off = 0;              // ci * chunk
    bool chunked = false;               // a step of the chunked path
    bool all_rows = false;              // the fast path: every row of the batch, no gather, no row map, PCM written in place
};

// ncodes[b]: codes of row b (ncodes[b] / 7 whole groups).  Rows decode together only when nothing has to be padded - padding a short
// row would change its tail samples.
//   chunk_groups > 0 and the longest row has more groups: VyvoTTS decodeAudioFromCodes (Qwen3.swift:47-83) - rows longer than
//     `chunk` groups are decoded as INDEPENDENT chunks of `chunk` groups (the last one shorter) whose samples are concatenated,
//     shorter rows are a single chunk; per chunk index the rows are grouped by their chunk length, shortest first.
//   otherwise: rows grouped by equal ncodes (NOT by equal ncodes / 7), fewest codes first; rows without a whole group are skipped;
//     when every row has the same count, the one step is the fast path.
static std::vector<SnacDecodeStep> snac_decode_plan(const std::vector<int32_t>& ncodes, int chunk_groups) {
    const int batch = (int)ncodes.size(), chunk = chunk_groups;
    std::vector<SnacDecodeStep> plan;
    int gmax = 0;
    for (int b = 0; b < batch; ++b) gmax = std::max(gmax, ncodes[b] / 7);
    if (chunk > 0 && gmax > chunk) {
        const int n_ch = (gmax + chunk - 1) / chunk;
        for (int ci = 0; ci < n_ch; ++ci) {
            std::vector<std::pair<int, int>> part;                      // (chunk length in groups, row)
            for (int b = 0; b < batch; ++b) {
                int g = ncodes[b] / 7;
                if (g > ci * chunk) part.push_back({std::min(chunk, g - ci * chunk), b});
            }
            std::stable_sort(part.begin(), part.end());
            for (size_t j0 = 0, j1; j0 < part.size(); j0 = j1) {
                for (j1 = j0; j1 < part.size() && part[j1].first == part[j0].first;) ++j1;
                SnacDecodeStep st;
                st.ci = ci; st.gc = part[j0].first; st.chunked = true;
                st.code_off = (int64_t)ci * chunk * 7; st.group_off = (int64_t)ci * chunk;
                for (size_t j = j0; j < j1; ++j) st.rows.push_back(part[j].second);
                plan.push_back(std::move(st));
            }
        }
        return plan;
    }
    std::vector<int32_t> order(batch);
    for (int b = 0; b < batch; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b2) { return ncodes[a] < ncodes[b2]; });
    const bool all_equal = batch > 0 && ncodes[order.front()] == ncodes[order.back()];
    for (size_t i0 = 0, i1; i0 < order.size(); i0 = i1) {
        for (i1 = i0; i1 < order.size() && ncodes[order[i1]] == ncodes[order[i0]];) ++i1;
        if (ncodes[order[i0]] / 7 == 0) continue;
        SnacDecodeStep st;
        st.gc = ncodes[order[i0]] / 7; st.all_rows = all_equal;
        st.rows.assign(order.begin() + i0, order.begin() + i1);
        plan.push_back(std::move(st));
    }
    return plan;
}
