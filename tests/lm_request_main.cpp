// Stand-alone check of csrc/lm_request.h (test_lm_request_cpu.py builds it with the address and undefined-behaviour sanitizers and runs
// it): build_lm_request - the host-built state of a generate call - on a ragged batch against arrays written out below, and
// snac_decode_plan - order and grouping of the codec sub-batches - against plans written out below.  Host code only: no HIP call is
// made, no device is opened.
#include "../mlx-audio-swift_amd/csrc/lm_request.h"

#include <stdio.h>
#include <string>

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

typedef std::vector<int32_t> V;

// "<kind> ci: gc [rows] +code_off/group_off; " per step; kind: fast (all rows in place), chunk (chunked path), rows (gathered)
static std::string plan_text(const V& ncodes, int chunk_groups) {
    std::string t;
    for (const SnacDecodeStep& st : snac_decode_plan(ncodes, chunk_groups)) {
        CHECK(!(st.all_rows && st.chunked));
        t += st.all_rows ? "fast " : st.chunked ? "chunk " : "rows ";
        t += std::to_string(st.ci) + ": " + std::to_string(st.gc) + " [";
        for (size_t k = 0; k < st.rows.size(); ++k) t += (k ? "," : "") + std::to_string(st.rows[k]);
        t += "] +" + std::to_string(st.code_off) + "/" + std::to_string(st.group_off) + "; ";
    }
    return t;
}
#define EXPECT_PLAN(ncodes, chunk, want)                                                            \
    do {                                                                                            \
        const std::string got = plan_text(ncodes, chunk);                                           \
        if (got != std::string(want)) {                                                             \
            printf("FAILED line %d: plan\n  got  %s\n  want %s\n", __LINE__, got.c_str(), want);    \
            ++failures;                                                                             \
        }                                                                                           \
    } while (0)

// the error a call ends with: "" or "<code>: <text>"
template <class F>
static std::string error_of(F&& f) {
    try { f(); } catch (const MisError& e) { return std::to_string((int)e.code) + ": " + e.what(); }
    return "";
}

int main() {
    // ---- snac_decode_plan
    EXPECT_PLAN((V{21, 21, 21}), 0, "fast 0: 3 [0,1,2] +0/0; ");
    EXPECT_PLAN((V{14, 28}), 0, "rows 0: 2 [0] +0/0; rows 0: 4 [1] +0/0; ");
    EXPECT_PLAN((V{28, 14, 28, 0}), 0, "rows 0: 2 [1] +0/0; rows 0: 4 [0,2] +0/0; ");          // rows without a group are skipped
    EXPECT_PLAN((V{15, 14}), 0, "rows 0: 2 [1] +0/0; rows 0: 2 [0] +0/0; ");                   // grouped by codes, not by groups
    EXPECT_PLAN((V{49, 49}), 3, "chunk 0: 3 [0,1] +0/0; chunk 1: 3 [0,1] +21/3; chunk 2: 1 [0,1] +42/6; ");
    EXPECT_PLAN((V{14, 35}), 3, "chunk 0: 2 [0] +0/0; chunk 0: 3 [1] +0/0; chunk 1: 2 [1] +21/3; ");
    EXPECT_PLAN((V{14, 21}), 3, "rows 0: 2 [0] +0/0; rows 0: 3 [1] +0/0; ");                   // longest row = chunk: not chunked
    EXPECT_PLAN((V{21, 21}), 3, "fast 0: 3 [0,1] +0/0; ");
    EXPECT_PLAN((V{28}), 0, "fast 0: 4 [0] +0/0; ");
    EXPECT_PLAN((V{28}), 3, "chunk 0: 3 [0] +0/0; chunk 1: 1 [0] +21/3; ");
    EXPECT_PLAN((V{14, 14, 6}), 0, "rows 0: 2 [0,1] +0/0; ");                                  // not all rows: gathered
    EXPECT_PLAN((V{35, 14, 28, 35, 3}), 2, "chunk 0: 2 [0,1,2,3] +0/0; chunk 1: 2 [0,2,3] +14/2; chunk 2: 1 [0,3] +28/4; ");
    EXPECT_PLAN((V{42, 7, 28}), 4, "chunk 0: 1 [1] +0/0; chunk 0: 4 [0,2] +0/0; chunk 1: 2 [0] +28/4; ");
    EXPECT_PLAN((V{0, 6}), 0, "");
    EXPECT_PLAN((V{5, 5}), 3, "");
    EXPECT_PLAN((V{}), 0, "");

    // ---- build_lm_request: rows of 3, 1 and 5 tokens, two tokens to come
    const V lens{3, 1, 5}, flat{10, 11, 12, 20, 30, 31, 32, 33, 34};
    CHECK(lm_prompt_tokens(lens) == 9);
    const V pm{0, 0, 10, 11, 12, 0, 0, 0, 0, 20, 30, 31, 32, 33, 34};
    const V all{10, 11, 12, 0, 0, 0, 0, 20, 0, 0, 0, 0, 0, 0, 30, 31, 32, 33, 34, 0, 0};
    struct Case { int ctx, flavor, want_ctx; V win, wl; };
    const Case cases[] = {
        {0, 0, 0, {0, 0, 0}, {0, 0, 0}},                                           // no window: one unused slot per row
        {2, 0, 2, {11, 12, 0, 20, 33, 34}, {2, 1, 2}},                             // the last min(ctx, len) tokens, right-aligned
        {4, 0, 4, {0, 10, 11, 12, 0, 0, 0, 20, 31, 32, 33, 34}, {3, 1, 4}},
        {0, 1, 0, {0, 0, 0}, {0, 0, 0}},                                           // flavour 1: the prompt is never in the window
        {2, 1, 2, {0, 0, 0, 0, 0, 0}, {0, 0, 0}},
        {4, 1, 4, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0}},
        {-3, 0, 0, {0, 0, 0}, {0, 0, 0}},                                          // a negative context is none
    };
    for (const Case& k : cases) {
        const LmRequest r = build_lm_request(lens, flat, 100, 2, k.ctx, k.flavor);
        CHECK(r.Lmax == 5 && r.all_stride == 7 && r.ctx == k.want_ctx);
        CHECK(r.pm == pm && r.all == all && r.alen == lens);
        CHECK(r.win == k.win && r.wl == k.wl);
    }
    {   // one row, prompt longer than the window
        const LmRequest r = build_lm_request(V{4}, V{1, 2, 3, 4}, 5, 3, 2, 0);
        CHECK(r.Lmax == 4 && r.all_stride == 7 && r.pm == (V{1, 2, 3, 4}) && r.all == (V{1, 2, 3, 4, 0, 0, 0}));
        CHECK(r.win == (V{3, 4}) && r.wl == (V{2}) && r.alen == (V{4}));
    }
    // ---- the two errors, texts and codes as the engine reports them
    const std::string invalid = std::to_string((int)MIS_ERR_INVALID_INPUT);
    CHECK(error_of([&]() { build_lm_request(V{3, 0, 5}, V{1, 2, 3, 4, 5, 6, 7, 8}, 100, 2, 2, 0); }) == invalid + ": empty prompt in row 1");
    CHECK(error_of([&]() { lm_prompt_tokens(V{2, -1}); }) == invalid + ": empty prompt in row 1");
    V bad = flat;
    bad[4] = 100;
    CHECK(error_of([&]() { build_lm_request(lens, bad, 100, 2, 2, 0); }) == invalid + ": prompt token 100 outside the vocabulary");
    bad[4] = -1;
    CHECK(error_of([&]() { build_lm_request(lens, bad, 100, 2, 2, 0); }) == invalid + ": prompt token -1 outside the vocabulary");
    CHECK(error_of([&]() { build_lm_request(lens, flat, 100, 2, 2, 0); }) == "");
    CHECK(error_of([&]() { build_lm_request(lens, V{1, 2}, 100, 2, 2, 0); }) != "");          // ids that do not match the lengths: no read past them

    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("lm_request ok\n");
    return 0;
}
