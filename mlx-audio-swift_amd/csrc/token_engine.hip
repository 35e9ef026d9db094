// token_engine.hip - a batch-1 decode engine for small LMs: ONE persistent launch runs every position of a request (the generate loop
// with its sampler included) on the compute units of a few XCDs.
//
// Why (BASELINE configs[1], Soprano-80M at batch 1): the launch chain spends ~125 graph nodes x 4.7 us on a
// token whose weights (160 MB) stream in 25 us - 0.03 of HBM.  At one row every op's output is a vector of 1-5 KB, so the per-op cost
// is the hand-off between compute units - a kernel boundary in the chain.  Measured before this was written
// (tools/token_engine_lab/probe.hip, profiles/r05/c2_xcd_stream_exchange_probe.json): an all-to-all edge (publish a slice, arrive on a
// counter, poll, gather the vector) among the 32 CUs of one XCD costs 1.65 us at 1 KB / 2.29 us at 4.6 KB, among 64 / 128 / 256 CUs
// 2.4 / 3.2 / 6.2 us; one XCD streams 1.28 TB/s out of the Infinity Cache (2.6 / 4.9 / 7.1 TB/s for 2 / 4 / 8).  Per token (69 edges,
// 160 MB): ~131 us of stream + ~126 us of edges on ONE XCD against 24 + 441 on eight - the chip-wide form is the launch chain's price
// again, few XCDs are 2-4x under it.  With the edge form this file ended up with (tagged granules, below) four XCDs are the optimum:
// 0.26 ms per position against the chain's 0.60 ("Batch-1 token engine": every version with its measurement).
//
// Structure.  Grid = one 512-thread block per CU; the blocks whose index mod 8 is below `xcds` are the W = 32 x xcds workers (observed
// placement: block b runs on XCD b mod 8 - used for speed only; every hand-off below is placement-independent), the others exit.
// Every worker holds the whole residual stream in LDS and owns a slice of the OUTPUT rows of every matrix:
//   per layer   RMSNorm (local) -> q|k|v slice                       -> edge 1 (Nqkv values)
//               q/k-norm, RoPE, attention - computed REDUNDANTLY by every worker over ONE shared K/V copy that all of them write with the
//               same bytes (no coherence protocol, no edge; ~50 KB of cache reads per layer at one row) -> o_proj slice, residual -> edge 2 (d)
//               RMSNorm (local) -> gate|up pairs, SwiGLU             -> edge 3 (ff)
//               down_proj slice, residual                            -> edge 4 (d)
//   per token   final norm (hidden tap) -> output-projection slice -> the token: arg-max (edge 5), arg-max behind the repetition penalty
//               (edges 5-6) or mis-sampler-v1 (edges 5-7: maximum, tile masses, token) -> next position's embedding
// Two programs share a block (te_matrix_role, te_vector_role): waves 4-7 hold the weight tiles - a GEMV slice runs on
// v_mfma_f32_16x16x32_bf16 with the engine's pre-packed tiles [N/16][K/32][64][8] as the A operand and the input vector as row 0 of B
// (15/16 of the matrix core idles: at one row the tile stream is the cost, not the math), each wave a quarter of the K range, tiles
// requested a phase ahead in pieces; waves 0-3 do the gathers, norms, attention (QK^T and P.V on the matrix core too), epilogues and
// edges.  An edge = self-validating 8-byte granules {two bf16 values, the edge's tag}: one agent-scope store by the producer, polled by
// the consumers (MI355X_MICROARCH.md, hand-off form R2).
// Rounding points are the oracle's (oracle/llama.py = MLX's bf16 graph): every primitive output rounded to bf16, float32 accumulation.
//
// In the product: mis_soprano_generate at batch 1 (csrc/soprano.hip; prompt through the launch chain's batched prefill, its K/V
// imported; falls back to the launch chain when the workers cannot be co-resident).  Compiled for Soprano-80M's widths (TeShape).
// MLX-quantised checkpoints (8 / 4 bit codes on every layer role) run the same program with code tiles in the matrix waves:
// k_token_engine_q, token_engine_q.hip.  The device program both share is token_engine_impl.h.
// Tests: tests/test_gpu_token_engine.py (oracle and launch-chain logits, sampler bit-exact on its own logits, hidden rows, stop id,
// long contexts, 1 / 2 / 4 / 8 XCDs), tests/test_gpu_soprano.py, tests/test_isa_cpu.py (register budget).
#include "token_engine_impl.h"
#include "step_loop.h"
#include <string.h>
#include <chrono>
#include <mutex>
#include <thread>

namespace {
// ---------------------------------------------------------------------------- the matrix waves' program.  Every te_sync() here has its
// partner at the same place of te_vector_role (the two programs are listed phase by phase in the same order); between barriers these
// waves only touch their weight tiles, the GEMV inputs in LDS and `red`.  Where the tiles of a phase are requested: as late as the
// registers demand (gate|up's 176 registers can only be filled once q|k|v's and before down's), and in PIECES sized to the vector waves'
// work behind each barrier - a wave stays in the issue loop while the CU's memory queue is full (one XCD streams 40 GB/s per CU: 24 KB
// per piece = 0.6 us), and everybody waits for it at the next barrier.
template <int XCDS>
__device__ __forceinline__ void te_matrix_role(const TeParams& p, const TeLds& L, const int w_in, const int mw_in, const int lane) {
    using S = TeShape;
    using Dm = TeDims<XCDS>;
    constexpr int W = Dm::W, R_QKV = Dm::R_QKV, R_O = Dm::R_O, P_GU = Dm::P_GU, R_GU = Dm::R_GU, R_HEAD = Dm::R_HEAD;
    constexpr int KPW_D = Dm::KPW_D, KPW_HD = Dm::KPW_HD, KPW_FF = Dm::KPW_FF;
    const int NTV = p.Vpad / 16;
    // This worker's tile rows, recomputed from an OPAQUE copy of the (scalar) worker and wave index wherever tiles are requested: every
    // tile address is loop-invariant, and hoisted out of the layer loop the ~100 of them (64-bit each) exhaust the scalar registers,
    // after which the compiler builds them in vector registers and the tile buffers spill.  A few SALU instructions per request instead.
#define TE_OPAQUE_IDS() int wq = w_in, mw = mw_in; asm volatile("" : "+s"(wq), "+s"(mw))
#define TE_ROWS_QKV(NT) int NT[R_QKV]; _Pragma("unroll") for (int r = 0; r < R_QKV; ++r) NT[r] = (wq + r * W) < S::Nqkv / 16 ? wq + r * W : -1
#define TE_ROWS_O(NT) int NT[R_O]; _Pragma("unroll") for (int r = 0; r < R_O; ++r) NT[r] = (wq + r * W) < S::d / 16 ? wq + r * W : -1
#define TE_ROWS_GU(NT) int NT[R_GU]; _Pragma("unroll") for (int r = 0; r < P_GU; ++r) { const int pr = wq + r * W;                       \
        NT[2 * r] = pr < S::ff / 16 ? 2 * pr : -1; NT[2 * r + 1] = pr < S::ff / 16 ? 2 * pr + 1 : -1; }
#define TE_ROWS_HEAD(NT, PASS) int NT[R_HEAD]; _Pragma("unroll") for (int r = 0; r < R_HEAD; ++r)                                      \
        NT[r] = (wq + ((PASS) * R_HEAD + r) * W) < NTV ? wq + ((PASS) * R_HEAD + r) * W : -1
    // tiles [N a / 40, N b / 40) of a phase's N
#define TE_CUT(N, a, b) ((N) * (a) / 40), ((N) * (b) / 40)
    constexpr int N_G = R_GU * KPW_D;
    TeTiles<R_QKV, KPW_D> tq;
    {
        TE_OPAQUE_IDS();
        TE_ROWS_QKV(nt);
        te_load<R_QKV, KPW_D, true>(tq, p.wqkv, S::d / 32, nt, p.norms, mw, lane);
    }
    for (int t = p.t_start; t < p.n_total; ++t) {
        te_sync();                                                   // token id
        if (*L.s_done) return;
        te_sync();                                                   // embedding row + sum of squares
        const bool do_head = t >= p.head_from && t < p.head_until;
        // (the layer loop is rotated by the last barrier of edge 4: the output projection's first tiles are requested AFTER the loop and
        // still ahead of the last layer's edge 4 - loaded inside the loop's last iteration they would be live across the whole loop, 144
        // registers that the gate|up tiles need)
        for (int li = 0; li < p.L; ++li) {
            TeTiles<R_O, KPW_HD> to;
            TeTiles<R_GU, KPW_D> tg;
            TeTiles<R_O, KPW_FF> td;
            const bf16_t* wg_l = p.wgu + (size_t)li * 2 * S::ff * S::d;
            const bf16_t* n2_l = p.norms + (size_t)(2 * li + 1) * S::d;
            if (li > 0) {
                te_sync();                                           // (previous layer) edge 4: residual stream gathered
                if (!*L.s_ok) return;
            }
            {   // q|k|v; then o_proj's tiles and the first quarter of gate|up's (the vector waves publish, wait for the slowest worker and gather)
                TE_OPAQUE_IDS();
                const float inv = rsqrtf(((L.s_ss[0] + L.s_ss[1]) + (L.s_ss[2] + L.s_ss[3])) / (float)S::d + p.eps);
                bf16x8_t xf[KPW_D];
                te_xfrag_norm<KPW_D>(xf, L.hf, tq.wn, inv, S::d / 32, mw, lane);
                te_mma<R_QKV, KPW_D>(tq, xf, L.red, mw, lane);
                te_sync();                                           // red ready
                TE_ROWS_O(nt);
                te_load<R_O, KPW_HD, false>(to, p.wo + (size_t)li * S::d * S::HD, S::HD / 32, nt, nullptr, mw, lane);
                TE_ROWS_GU(ng);
                te_load<R_GU, KPW_D, true, TE_CUT(N_G, 0, 10)>(tg, wg_l, S::d / 32, ng, n2_l, mw, lane);
                te_sync();                                           // edge 1: q|k|v gathered
                if (!*L.s_ok) return;
                te_load<R_GU, KPW_D, true, TE_CUT(N_G, 10, 16)>(tg, wg_l, S::d / 32, ng, n2_l, mw, lane);
                te_sync();                                           // q/k-norm + RoPE
                te_load<R_GU, KPW_D, true, TE_CUT(N_G, 16, 28)>(tg, wg_l, S::d / 32, ng, n2_l, mw, lane);
                te_sync();                                           // scores
                te_load<R_GU, KPW_D, true, TE_CUT(N_G, 28, 34)>(tg, wg_l, S::d / 32, ng, n2_l, mw, lane);
                te_sync();                                           // softmax
                te_load<R_GU, KPW_D, true, TE_CUT(N_G, 34, 40)>(tg, wg_l, S::d / 32, ng, n2_l, mw, lane);
                te_sync();                                           // attention output ready
            }
            {   // o_proj (gate|up's 176 registers of tiles are live: nothing more can be requested before its MFMAs)
                TE_OPAQUE_IDS();
                bf16x8_t xf[KPW_HD];
                te_xfrag_bf16<KPW_HD>(xf, L.xb, S::HD / 32, mw, lane);
                te_mma<R_O, KPW_HD>(to, xf, L.red, mw, lane);
                te_sync();                                           // red ready
            }
            te_sync();                                               // edge 2: residual stream gathered
            if (!*L.s_ok) return;
            {   // gate|up; then down_proj's tiles
                TE_OPAQUE_IDS();
                const float inv = rsqrtf(((L.s_ss[0] + L.s_ss[1]) + (L.s_ss[2] + L.s_ss[3])) / (float)S::d + p.eps);
                bf16x8_t xf[KPW_D];
                te_xfrag_norm<KPW_D>(xf, L.hf, tg.wn, inv, S::d / 32, mw, lane);
                te_mma<R_GU, KPW_D>(tg, xf, L.red, mw, lane);
                te_sync();                                           // red ready
                TE_ROWS_O(nt);
                te_load<R_O, KPW_FF, false>(td, p.wdown + (size_t)li * S::d * S::ff, S::ff / 32, nt, nullptr, mw, lane);
                te_sync();                                           // edge 3: activation gathered
                if (!*L.s_ok) return;
            }
            {   // down; then the next layer's q|k|v tiles
                TE_OPAQUE_IDS();
                bf16x8_t xf[KPW_FF];
                te_xfrag_bf16<KPW_FF>(xf, L.xb, S::ff / 32, mw, lane);
                te_mma<R_O, KPW_FF>(td, xf, L.red, mw, lane);
                te_sync();                                           // red ready
                if (li + 1 < p.L) {
                    TE_ROWS_QKV(nt);
                    te_load<R_QKV, KPW_D, true>(tq, p.wqkv + (size_t)(li + 1) * S::Nqkv * S::d, S::d / 32, nt, p.norms + (size_t)(2 * li + 2) * S::d, mw, lane);
                }
            }
        }
        if (!do_head) {   // a prompt position: straight to the next position's first tiles
            TE_OPAQUE_IDS();
            TE_ROWS_QKV(nt);
            te_load<R_QKV, KPW_D, true>(tq, p.wqkv, S::d / 32, nt, p.norms, mw, lane);
            te_sync();                                               // (last layer) edge 4: residual stream gathered
            if (!*L.s_ok) return;
        } else {   // output projection, passes of R_HEAD tile rows; the first pass's tiles behind the last layer's down_proj
            TeTiles<R_HEAD, KPW_D> th;
            int mw_h;
            {
                TE_OPAQUE_IDS();
                mw_h = mw;
                TE_ROWS_HEAD(nth, 0);
                te_load<R_HEAD, KPW_D, true>(th, p.head, S::d / 32, nth, p.norms + (size_t)(2 * p.L) * S::d, mw, lane);
                te_sync();                                           // (last layer) edge 4: residual stream gathered
                if (!*L.s_ok) return;
            }
            const float inv = rsqrtf(((L.s_ss[0] + L.s_ss[1]) + (L.s_ss[2] + L.s_ss[3])) / (float)S::d + p.eps);
            bf16x8_t xf[KPW_D];
            te_xfrag_norm<KPW_D>(xf, L.hf, th.wn, inv, S::d / 32, mw_h, lane);
            for (int pass = 0; pass * R_HEAD * W < NTV; ++pass) {
                TE_OPAQUE_IDS();
                te_mma<R_HEAD, KPW_D>(th, xf, L.red, mw, lane);
                te_sync();                                           // red ready
                if ((pass + 1) * R_HEAD * W < NTV) {
                    TE_ROWS_HEAD(nt2, pass + 1);
                    te_load<R_HEAD, KPW_D, false>(th, p.head, S::d / 32, nt2, nullptr, mw, lane);
                } else {
                    TE_ROWS_QKV(nt);
                    te_load<R_QKV, KPW_D, true>(tq, p.wqkv, S::d / 32, nt, p.norms, mw, lane);              // layer 0 of the next position
                }
                te_sync();                                           // red consumed
            }
            te_sync();                                               // candidates of the vector waves
            te_sync();                                               // edge 5: candidates (arg-max) / maxima (sampling) gathered
            if (!*L.s_ok) return;
            if (p.sample == 1) {
                te_sync();                                           // edge 6: tile masses gathered
                if (!*L.s_ok) return;
                te_sync(); te_sync();                                // scan of the tile masses: wave totals, the chosen tile
                te_sync();                                           // edge 7: the token
                if (!*L.s_ok) return;
            } else if (p.sample == 2) {
                te_sync();                                           // the waves' id candidates
                te_sync();                                           // edge 6: the id
                if (!*L.s_ok) return;
            }
        }
    }
}

template <int XCDS>
__global__ void __launch_bounds__(TE_NT) k_token_engine(TeParams p) {
    using S = TeShape;
    using Dm = TeDims<XCDS>;
    static_assert(S::H == TE_VW && S::Hkv == 1 && S::D == 128 && S::d / 4 <= 128 && S::Nqkv / 4 <= TE_VW * 64, "vector-wave mapping of the engine");
    extern __shared__ __attribute__((aligned(16))) unsigned char te_lds_pad[];      // (requested size keeps the launch at one block per CU)
    __shared__ __attribute__((aligned(16))) float hf[S::d];
    __shared__ __attribute__((aligned(16))) bf16_t xb[S::ff > S::HD ? S::ff : S::HD];
    __shared__ __attribute__((aligned(16))) float qkvf[S::Nqkv];
    __shared__ __attribute__((aligned(16))) float qh[S::H * S::D];
    __shared__ __attribute__((aligned(16))) float knew[S::D], vnew[S::D];
    __shared__ __attribute__((aligned(16))) float sc[S::H * TE_CTX];
    __shared__ __attribute__((aligned(16))) bf16_t ph[S::H * TE_CTX], pl[S::H * TE_CTX];
    __shared__ __attribute__((aligned(16))) bf16_t stage[Dm::R_RED * 16];
    __shared__ __attribute__((aligned(16))) float red[TE_MW * Dm::R_RED * 16];
    __shared__ float s_ss[TE_VW];
    __shared__ u64 s_cand[2 * TE_VW];
    __shared__ int s_ok;
    __shared__ int s_tok;
    __shared__ int s_done;
    __shared__ int s_cancel;
    __shared__ u64 earr[TE_HP * Dm::R_HEAD * 16];
    __shared__ uint32_t tsum32[TE_XG];
    __shared__ int win[65];
    __shared__ u64 s_wtot[TE_VW + 2];
    if (p.n_total < 0) te_lds_pad[threadIdx.x] = 0;
    const int b = blockIdx.x;
    if (b >= 256) { if (b == 256 + XCDS) te_relay(p); return; }     // (block 256 + xcds lands on XCD `xcds`, whose compute units the workers do not use)
    if ((b & 7) >= XCDS) return;
    const int w = (b >> 3) * XCDS + (b & 7);
    const int tid = threadIdx.x, wave = tid >> 6;
    if (tid < TE_VW) s_ss[tid] = 0.f;
    if (tid == 0) { s_ok = 1; s_tok = 0; s_done = 0; s_cancel = 0; win[64] = 0; }
    const TeLds L{hf, xb, qkvf, qh, knew, vnew, sc, ph, pl, stage, red, s_ss, s_cand, &s_ok, &s_tok, &s_done, &s_cancel, earr, tsum32, win, s_wtot};
    te_sync();
    // (the wave index as a SCALAR: every tile address is then scalar base + one shared lane offset.  With a vector wave index the
    // compiler keeps a 64-bit address pair per tile live across the layer loop - ~200 registers of addresses, everything spills)
    if (wave >= TE_VW) te_matrix_role<XCDS>(p, L, w, __builtin_amdgcn_readfirstlane(wave - TE_VW), tid & 63);     // waves 4..7: weight tiles and MFMAs
    else te_vector_role<XCDS>(p, L, w, tid);                                         // waves 0..3: everything else
}
// K/V of the positions the launch chain's prefill has processed, from its tiled caches (kernels.h, TtsKvView) into the engine's copy:
// keys row-major [position][D], values transposed [D][position]
__global__ void k_te_import_kv(const bf16_t* __restrict__ kc_all, const bf16_t* __restrict__ vt_all, size_t layer_stride, bf16_t* __restrict__ kv,
                               int n_pos) {
    constexpr int D = TeShape::D;
    const int li = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_pos * D) return;
    const int pos = idx / D, d = idx % D;
    const bf16_t* kc = kc_all + (size_t)li * layer_stride;
    const bf16_t* vt = vt_all + (size_t)li * layer_stride;
    const int ptile = pos >> 5, pr = pos & 31, prow = ((pr >> 3) << 2) | (pr & 3), phalf = (pr >> 2) & 1;
    const bf16_t kval = kc[((((size_t)ptile * 2 + phalf) * (D / 32) + (d >> 5)) * 64 + (((d & 31) >> 3) << 4) + prow) * 8 + (d & 7)];
    const bf16_t vval = vt[(((size_t)ptile * (D / 16) + (d >> 4)) * 64 + ((pr >> 3) << 4) + (d & 15)) * 8 + (pr & 7)];
    kv[((size_t)li * 2 + 0) * TE_CTX * D + (size_t)pos * D + d] = kval;
    kv[((size_t)li * 2 + 1) * TE_CTX * D + (size_t)d * TE_CTX + pos] = vval;
}
}   // namespace

// ---------------------------------------------------------------------------- host side
// Buffers a handle keeps between requests (every request allocated and cleared a ~9 MB K/V copy).  The token row and the
// cancel word are pinned, coherent host memory: the launch writes / reads them with system-scope accesses while the host polls.
struct TokenEngineScratch {
    DevBuf<int32_t> prompt, done, tokd;
    DevBuf<bf16_t> kv;
    DevBuf<u64> x;
    DevBuf<unsigned> sync;
    int32_t* tokens_host = nullptr;    // [TE_CTX + 1]: ids, then the cancel word
    int kv_layers = 0;
    ~TokenEngineScratch() { if (tokens_host) (void)hipHostFree(tokens_host); }
};
TokenEngineScratch* token_engine_scratch_create() { return new TokenEngineScratch(); }
void token_engine_scratch_destroy(TokenEngineScratch* s) { delete s; }

namespace {
// 8 XCDs x 32 compute units (SPX mode of an MI355X): the worker set is "blocks with index mod 8 below xcds" of a 256-block grid, one block
// per compute unit.  Other partition modes / parts keep the launch chain.
bool te_device_ok(int device) {
    static std::mutex mu;
    static std::map<int, bool> ok;
    std::lock_guard<std::mutex> lk(mu);
    auto it = ok.find(device);
    if (it != ok.end()) return it->second;
    hipDeviceProp_t prop{};
    const bool good = hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount == 256;
    ok[device] = good;
    return good;
}
}   // namespace

// Which kernel a handle's weights take: 0 = k_token_engine (bf16 tiles); 8 / 4 = k_token_engine_q (token_engine_q.hip) - the four layer
// roles all streamed as codes of that width, the output projection dense or streamed with the same width; -1 = neither (a role left dense
// by a per-layer override, mixed widths: the launch chain).
static int te_quant_bits(const TtsWeightsView& v) {
    if (!v.quantised) return 0;
    const int b = v.q_qkv.bits;
    if ((b != 8 && b != 4) || v.q_o.bits != b || v.q_gu.bits != b || v.q_down.bits != b) return -1;
    if (v.q_head.bits != 0 && v.q_head.bits != b) return -1;
    return b;
}

bool token_engine_supports(mis_tts* lm) {
    if (!lm) return false;
    const TtsWeightsView v = tts_internal_weights(lm);
    using S = TeShape;
    return v.finalized && v.d == S::d && v.ff == S::ff && v.H == S::H && v.Hkv == S::Hkv && v.D == S::D && v.qk_norm && v.rope_plain &&
           te_quant_bits(v) >= 0 && v.V <= 65536 && v.Vpad / 16 <= 2 * TE_VW * 64 && te_device_ok(v.device);
}

// One request.  generate == false (laboratory): arg-max after EVERY position, no stop; logits / hidden rows are indexed by position.
// generate == true: the product's semantics (tts_generate_hidden): a token after the last prompt position and after every generated one
// until `stop_id` or max_new ids; hidden row k = final-norm output of position n_prompt - 1 + k (row 0 = the last prompt token,
// Soprano.swift:824-825); logits row k = the logits the k-th token was drawn from.
void token_engine_run(mis_tts* lm, const TokenEngineRequest& rq, TokenEngineResult& out) {
    MIS_REQUIRE(lm && rq.prompt && rq.n_prompt >= 1 && rq.max_new >= 0, MIS_ERR_INVALID_INPUT, "bad argument");
    const int xcds = rq.xcds;
    MIS_REQUIRE(xcds == 1 || xcds == 2 || xcds == 4 || xcds == 8, MIS_ERR_INVALID_INPUT, "the engine is compiled for 1, 2, 4 or 8 XCDs");
    MIS_REQUIRE(token_engine_supports(lm), MIS_ERR_INVALID_INPUT,
                "the token engine is compiled for Soprano-80M's widths (d 512, ffn 2304, 4 / 1 heads x 128, q/k norm, plain RoPE, vocabulary <= 8192; "
                "bf16, or every layer role streamed as 8- or 4-bit codes of one width) "
                "on a device of 8 XCDs x 32 compute units");
    const TtsWeightsView v = tts_internal_weights(lm);
    using S = TeShape;
    const int n_total = rq.n_prompt + rq.max_new;
    MIS_REQUIRE(n_total <= TE_CTX, MIS_ERR_INVALID_INPUT, "at most %d positions", TE_CTX);
    MIS_REQUIRE(!rq.sample || (rq.temperature > 0.0f && rq.win_cap >= 0 && rq.win_cap <= 64), MIS_ERR_INVALID_INPUT, "sampling needs temperature > 0 and a window of at most 64 ids");
    MIS_REQUIRE(v.Vpad / 16 <= TE_HP * 8 * 32 * xcds, MIS_ERR_INVALID_INPUT, "vocabulary too large for the engine's output-projection passes");
    MIS_REQUIRE(rq.generate || (!rq.on_token && !rq.cancel), MIS_ERR_INVALID_INPUT, "token callback / cancel flag: generate form only");
    HIP_CHECK(hipSetDevice(v.device));
    const int grid = 256 + xcds + 1;                                     // 256 worker slots + the relay block (te_relay) as the last one: blocks go to
                                                                         // XCD (index mod 8), and XCD `xcds` is the first the workers leave free
    const float* rc = nullptr; const float* rs = nullptr;
    hipStream_t s = v.stream;
    out.n_announced = 0;
    std::vector<int32_t> hp(rq.n_prompt);
    HIP_CHECK(hipMemcpy(hp.data(), rq.prompt, (size_t)rq.n_prompt * 4, hipMemcpyDefault));
    for (int t : hp) MIS_REQUIRE(t >= 0 && t < v.V, MIS_ERR_INVALID_INPUT, "prompt token %d outside the vocabulary", t);
    // The prompt, all but its last position, through the launch chain's batched prefill (one [positions x 1] pass: ~1 ms where the engine
    // walks 0.24 ms per position); its K/V are imported below and the engine starts at the last prompt position.
    const int t_start = (rq.generate && rq.prefill_by_chain && rq.n_prompt >= 2) ? rq.n_prompt - 1 : 0;
    TtsKvView kvv{};
    if (t_start > 0) {
        kvv = tts_internal_prefill_kv(lm, hp.data(), t_start, n_total);
        MIS_REQUIRE(kvv.D == S::D && kvv.Hkv == S::Hkv, MIS_ERR_GENERATION_FAILED, "token engine: unexpected cache geometry");
        rc = kvv.rope_cos; rs = kvv.rope_sin;
    } else {
        tts_internal_rope_tables(lm, n_total, &rc, &rs);                 // (builds the tables for this context length)
    }
    const int head_from = rq.generate ? rq.n_prompt - 1 : 0;
    const int head_until = rq.generate ? n_total - 1 : n_total;
    const int n_rows = n_total - head_from;                              // hidden rows at most; logits rows: head_until - head_from
    TokenEngineScratch local;
    TokenEngineScratch& sc = rq.scratch ? *rq.scratch : local;
    DevBuf<float> d_logits, d_hidden;
    sc.prompt.alloc(TE_CTX); sc.done.alloc(2); sc.tokd.alloc(TE_CTX); sc.x.alloc(2 * TE_XG); sc.sync.alloc(64);
    if (!sc.tokens_host)
        HIP_CHECK(hipHostMalloc((void**)&sc.tokens_host, (TE_CTX + 1) * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
    const size_t kv_pos = (size_t)S::Hkv * S::D;
    // The transposed value rows are read in 32-key steps: positions this request has not written yet (x probability 0) must be finite.
    // Cleared when allocated; what earlier requests of the handle left there are finite K/V values, and 0 x finite = 0 exactly.
    if (sc.kv_layers != v.L) {
        sc.kv.alloc((size_t)v.L * 2 * TE_CTX * kv_pos); sc.kv_layers = v.L;
        HIP_CHECK(hipMemsetAsync(sc.kv.p, 0, sc.kv.bytes(), s));
    }
    if (rq.want_logits) d_logits.alloc((size_t)std::max(head_until - head_from, 1) * v.V);
    float* hidden_dev = rq.hidden_dev;
    if (rq.want_hidden && !hidden_dev) { d_hidden.alloc((size_t)n_rows * S::d); hidden_dev = d_hidden.p; }
    volatile int32_t* tok_host = sc.tokens_host;
    volatile int32_t* cancel_host = sc.tokens_host + TE_CTX;
    for (int t = 0; t < n_total; ++t) tok_host[t] = -1;                   // (an id is >= 0: -1 = not chosen yet)
    *cancel_host = 0;
    HIP_CHECK(hipMemcpyAsync(sc.prompt.p, hp.data(), (size_t)rq.n_prompt * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(sc.sync.p, 0, 64 * sizeof(unsigned), s));
    HIP_CHECK(hipMemsetAsync(sc.x.p, 0, 2 * TE_XG * sizeof(u64), s));
    HIP_CHECK(hipMemsetAsync(sc.done.p, 0, 8, s));
    HIP_CHECK(hipMemsetAsync(sc.tokd.p, 0xFF, (size_t)TE_CTX * 4, s));                 // -1: not chosen yet
    if (t_start > 0)
        hipLaunchKernelGGL(k_te_import_kv, dim3((unsigned)((t_start * S::D + 255) / 256), (unsigned)v.L), dim3(256), 0, s, kvv.kcache, kvv.vtcache,
                           kvv.layer_stride, sc.kv.p, t_start);
    TeParams p{};
    p.emb = v.emb; p.wqkv = v.wqkv; p.wo = v.wo; p.wgu = v.wgu; p.wdown = v.wdown; p.head = v.head; p.norms = v.norms; p.qknorm = v.qknorm;
    p.rope_cos = rc; p.rope_sin = rs; p.L = v.L; p.V = v.V; p.Vpad = v.Vpad; p.eps = v.eps;
    p.prompt = sc.prompt.p; p.n_prompt = rq.n_prompt; p.n_total = n_total; p.t_start = t_start; p.next_tokens = sc.tokens_host;
    p.tok_dev = sc.tokd.p; p.cancel_dev = reinterpret_cast<int*>(sc.sync.p + 40); p.relay_done = sc.sync.p + 41;
    p.cancel = rq.cancel ? sc.tokens_host + TE_CTX : nullptr;
    p.logits_out = rq.want_logits ? d_logits.p : nullptr; p.hidden_out = hidden_dev;
    p.kv = sc.kv.p; p.xbuf = sc.x.p; p.fail = sc.sync.p + 32; p.xcds = xcds;
    p.spin = rq.spin > 0 ? rq.spin : 1 << 20;
    if (const char* e = getenv("MIS_TE_SPIN")) p.spin = std::max(atoi(e), 0);      // (tests: 0 = the first poll that misses times out)
    p.head_from = head_from; p.head_until = head_until;
    p.sample = rq.sample ? 1 : (rq.generate ? 2 : 0); p.win_cap = rq.win_cap; p.temperature = rq.temperature; p.penalty = rq.penalty; p.seed = rq.seed; p.row = rq.row;
    p.stop_id = rq.generate ? rq.stop_id : -1; p.n_done = sc.done.p;
    DevBuf<u64> d_dbg;
    const char* stamp_env = getenv("MIS_TE_STAMPS");
    if (stamp_env) {
        d_dbg.alloc(32);
        HIP_CHECK(hipMemsetAsync(d_dbg.p, 0, 32 * 8, s));
        p.dbg = d_dbg.p; p.dbg_token = atoi(stamp_env);
    }
    const size_t pad = 48 * 1024;                                        // with the static arrays: more than half a CU's LDS -> one block per CU
    // MLX-quantised checkpoints: the code-streaming kernel (token_engine_q.hip), launched by address with the role pointers beside p
    const int qbits = te_quant_bits(v);
    TeQParams qp{};
    const void* qkernel = nullptr;
    if (qbits > 0) {
        auto role = [](const TtsQRoleView& r) { return TeQRole{r.q, r.sb, r.q_layer, r.sb_layer}; };
        qp.qkv = role(v.q_qkv); qp.o = role(v.q_o); qp.gu = role(v.q_gu); qp.down = role(v.q_down); qp.head = role(v.q_head);
        qp.head_nt = v.q_head_nt;
        qkernel = token_engine_q_kernel(xcds, qbits, v.q_head.bits != 0);
        MIS_REQUIRE(qkernel, MIS_ERR_INVALID_INPUT, "token engine: no code-streaming kernel for %d XCDs / %d bits", xcds, qbits);
        MIS_REQUIRE(v.q_head.bits != 0 || v.head, MIS_ERR_INVALID_INPUT, "token engine: no output projection");
    }
    // (the attribute is per device and per function: set on every request - a table keyed by XCD count alone left a second device without it)
    if (qkernel) HIP_CHECK(hipFuncSetAttribute(qkernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad));
    else if (xcds == 1) HIP_CHECK(hipFuncSetAttribute((const void*)k_token_engine<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad));
    else if (xcds == 2) HIP_CHECK(hipFuncSetAttribute((const void*)k_token_engine<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad));
    else if (xcds == 4) HIP_CHECK(hipFuncSetAttribute((const void*)k_token_engine<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad));
    else HIP_CHECK(hipFuncSetAttribute((const void*)k_token_engine<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad));
    HipEvents<2> ev;
    HIP_CHECK(hipEventRecord(ev[0], s));
    if (qkernel) {
        void* args[] = {&p, &qp};
        HIP_CHECK(hipLaunchKernel(qkernel, dim3(grid), dim3(TE_NT), args, pad, s));
    } else if (xcds == 1) hipLaunchKernelGGL(k_token_engine<1>, dim3(grid), dim3(TE_NT), pad, s, p);
    else if (xcds == 2) hipLaunchKernelGGL(k_token_engine<2>, dim3(grid), dim3(TE_NT), pad, s, p);
    else if (xcds == 4) hipLaunchKernelGGL(k_token_engine<4>, dim3(grid), dim3(TE_NT), pad, s, p);
    else hipLaunchKernelGGL(k_token_engine<8>, dim3(grid), dim3(TE_NT), pad, s, p);
    HIP_CHECK(hipEventRecord(ev[1], s));
    HIP_CHECK(hipGetLastError());
    // ---- while the launch runs: the ids it has chosen so far, in order, to the caller; the caller's cancel flag to the launch
    bool cancelled = false;
    int seen = 0;                                                        // chosen ids read so far (index head_from + seen)
    auto drain = [&]() {
        while (head_from + seen < head_until) {
            const int32_t id = tok_host[head_from + seen];
            if (id < 0) break;
            if (rq.on_token) { rq.on_token(seen, id); out.n_announced = seen + 1; }
            seen += 1;
            if (id == p.stop_id) break;
        }
    };
    if (rq.on_token || rq.cancel) {
        for (;;) {
            const hipError_t q = hipEventQuery(ev[1]);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) HIP_CHECK(q);
            drain();
            if (rq.cancel && *rq.cancel && !cancelled) { cancelled = true; *cancel_host = 1; }
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
    HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    unsigned failed = 0;
    HIP_CHECK(hipMemcpy(&failed, sc.sync.p + 32, 4, hipMemcpyDeviceToHost));
    MIS_REQUIRE(!failed, MIS_ERR_GENERATION_FAILED, "token engine: an edge timed out (its workers were not co-resident)");
    if (cancelled || (rq.cancel && *rq.cancel)) throw MisError(MIS_ERR_CANCELLED, "generation cancelled");
    drain();
    int32_t done[2] = {0, 0};
    HIP_CHECK(hipMemcpy(done, sc.done.p, 8, hipMemcpyDeviceToHost));
    out.n_positions = done[0]; out.n_sampled = done[1]; out.ms = ms; out.head_from = head_from;
    out.next_tokens.assign(n_total, 0);
    HIP_CHECK(hipMemcpy(out.next_tokens.data(), sc.tokd.p, (size_t)n_total * 4, hipMemcpyDeviceToHost));
    for (int t = 0; t < n_total; ++t) {
        MIS_REQUIRE(out.next_tokens[t] == tok_host[t], MIS_ERR_GENERATION_FAILED, "token engine: the host-visible id row differs from the device's at position %d", t);
        if (out.next_tokens[t] < 0) out.next_tokens[t] = 0;
    }
    if (rq.want_logits) {
        out.logits.assign((size_t)std::max(head_until - head_from, 1) * v.V, 0.f);
        HIP_CHECK(hipMemcpy(out.logits.data(), d_logits.p, out.logits.size() * 4, hipMemcpyDeviceToHost));
    }
    if (rq.want_hidden && !rq.hidden_dev) {
        out.hidden.assign((size_t)n_rows * S::d, 0.f);
        HIP_CHECK(hipMemcpy(out.hidden.data(), d_hidden.p, out.hidden.size() * 4, hipMemcpyDeviceToHost));
    }
    if (stamp_env) {
        u64 st[32];
        HIP_CHECK(hipMemcpy(st, d_dbg.p, sizeof(st), hipMemcpyDeviceToHost));
        static const char* names[20] = {"layer start", "qkv: red ready", "published", "q|k|v polled in", "barrier", "q/k-norm + RoPE", "scores",
                                        "softmax + P.V", "o: red ready", "published", "h polled in", "barrier", "gate|up: red ready", "published",
                                        "act polled in", "barrier", "down: red ready", "published", "h polled in", "barrier"};
        fprintf(stderr, "token engine, %d XCD(s), position %d, layer 1, worker 0 (shader cycles since layer start, delta):\n", xcds, p.dbg_token);
        for (int i = 0; i < 20; ++i)
            fprintf(stderr, "  %2d %-20s %8llu %6lld\n", i, names[i], (unsigned long long)(st[i] - st[0]), i ? (long long)(st[i] - st[i - 1]) : 0ll);
    }
}

// include/mi_speech_debug.h
extern "C" mis_status mis_debug_token_engine(mis_tts* lm, const int32_t* prompt, int n_prompt, int n_new, int xcds, const mis_gen_params* sampling,
                                             int stop_id, int32_t* next_tokens, float* logits_out, float* hidden_out, int32_t* counts,
                                             double* ms_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(next_tokens, MIS_ERR_INVALID_INPUT, "null argument");
    TokenEngineRequest rq{};
    rq.prompt = prompt; rq.n_prompt = n_prompt; rq.max_new = n_new; rq.xcds = xcds;
    rq.generate = sampling != nullptr;
    rq.prefill_by_chain = rq.generate;                                   // the generate form as the product runs it (mis_soprano_generate)
    if (sampling) {
        rq.sample = sampling->temperature > 0.0f;
        rq.temperature = sampling->temperature; rq.penalty = sampling->repetition_penalty; rq.win_cap = std::max(sampling->repetition_context, 0);
        rq.seed = sampling->seed; rq.row = sampling->row_offset; rq.stop_id = stop_id;
    }
    rq.want_logits = logits_out != nullptr; rq.want_hidden = hidden_out != nullptr;
    TokenEngineResult r;
    token_engine_run(lm, rq, r);
    const int n_total = n_prompt + n_new;
    memcpy(next_tokens, r.next_tokens.data(), (size_t)n_total * 4);
    if (logits_out) memcpy(logits_out, r.logits.data(), r.logits.size() * 4);
    if (hidden_out) memcpy(hidden_out, r.hidden.data(), r.hidden.size() * 4);
    if (counts) { counts[0] = r.n_positions; counts[1] = r.n_sampled; }
    if (ms_out) *ms_out = r.ms;
    MIS_API_END
}
