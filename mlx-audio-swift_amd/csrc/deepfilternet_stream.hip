// deepfilternet_stream.hip - DeepFilterNet V2 / V3 hop by hop (DeepFilterNetStreamer.processChunk / flush / reset of the reference's
// DeepFilterNetStreaming.swift): 1..max_batch streams on one finalized model, each feed a ragged set of whole hops, the state carried on
// the device.  The kernels are the offline engine's in their stream form (deepfilternet_kernels.h, S = true): what a stream returns is
// bit for bit what mis_deepfilternet_enhance returns for the same samples (include/mi_speech.h states the yardstick).
//
// Workspace: every buffer of the model's launch list once more, a stream's block being HIST rows of history and max_hops rows of the
// feed.  Buffers up to the features are indexed by frame (hop h brings frame h), everything behind the look-ahead shift by target
// (target t runs once frame t + conv_lookahead exists).  A feed of hops[b] hops to a stream that has seen h_b:
//   n_b = hops[b] new frames h_b .., m_b = the targets max(0, h_b - L) .. h_b + n_b - 1 - L, off_b = max(0, L - h_b) the feature row
//   of target row 0.
// Carried, all as the last rows of a block rolled in front of it by k_dfn_roll at the end of a feed: fft - hop input samples; spec
// frames (L + df_order - 1 - df_lookahead rows: the deep filter's reach and the frames waiting for their look-ahead); the two features
// (kT - 1 rows); the input of every other conv with a time kernel (kT - 1 rows); h of every GRU layer (the layer's last output row);
// the last windowed synthesis frame (its second half is the overlap-add tail at fft = 2 hop).  The normalisation states have a buffer
// of their own, the hop counter is the host's.
//
//   k_dfn_ola_stream   hop samples a target: the tail of frame t - 1 + the head of frame t through the offline expression
//   k_dfn_roll         one thread a column of a carried buffer: rows [cnt - hist, cnt) -> [-hist, 0), ascending, in place
//
// Launches of a feed: the offline count (the same list) + 1 (the roll); a feed in which no stream brings a hop launches nothing.
#include "deepfilternet_kernels.h"

#define DFS_MAX_HOPS 256

struct DfRoll { float* p; int rw, nr, lead, hist, which; };                   // which: 0 counts frames (n), 1 targets (m)

__global__ void __launch_bounds__(256) k_dfn_roll(const DfRoll* __restrict__ e, const int32_t* __restrict__ n, const int32_t* __restrict__ m) {
    const DfRoll q = e[blockIdx.y];
    const int col = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z, cnt = q.which ? m[b] : n[b];
    if (col >= q.rw || cnt == 0) return;                                  // a stream that brought nothing keeps its history as it is
    float* base = q.p + ((size_t)b * q.nr + q.lead - q.hist) * q.rw + col;
    for (int i = 0; i < q.hist; ++i) {                                    // the source of row i lies cnt rows above it: never a row already written
        const float v = base[(size_t)(i + cnt) * q.rw];
        base[(size_t)i * q.rw] = v;
    }
}

__global__ void __launch_bounds__(256) k_dfn_ola_stream(const float* __restrict__ fr, const float* __restrict__ win, float* __restrict__ out,
                                                        const int32_t* __restrict__ m, const int32_t* __restrict__ t0, int nr, int hist, int W,
                                                        int hop, int64_t out_stride) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (s >= (int64_t)m[b] * hop) return;
    const int j = (int)(s / hop), t = t0[b] + j;                          // target t emits padded samples [t hop, (t + 1) hop)
    const int64_t q = (int64_t)t * hop + (s - (int64_t)j * hop), lo = q - W + 1;
    const int fa = lo <= 0 ? 0 : (int)((lo + hop - 1) / hop);
    out[(size_t)b * out_stride + s] = df_ola_at(fr + (size_t)b * nr * W, hist - t0[b], win, q, fa, t, W, hop);
}

struct mis_deepfilternet_stream {
    mis_deepfilternet* m = nullptr;
    int S = 0, maxh = 0, HIST = 0, nr = 0, L = 0, thr = 0;
    std::vector<DfOp> ops;
    std::vector<float*> buf;                                                  // the model's buffers, this workspace
    std::vector<DfRoll> rolls;
    int max_rw = 0;
    DevBuf<float> work, pcm, out, state;
    DevBuf<int32_t> tab;                                                      // n | m | t0 | off | seen, DF_MAX_BATCH each
    DevBuf<DfRoll> d_rolls;
    std::vector<int32_t> h_tab;
    std::vector<int64_t> seen;
    int last_launches = 0;
    HipEvents<2 + 2 * DF_MAX_REC> ev;
    float ms[2] = {0.0f, 0.0f};
};

// the feed size up to which the short-chunk recurrence runs.  Measured at hidden size 256 (profiles/deepfilternet_stream/bench.jsonl,
// microseconds a launch, short-chunk / offline form, 1 stream): 12.4 / 19.9 at 1 frame, 19.3 / 24.6 at 2, 32.8 / 34.0 at 4, 59.9 / 52.9 at
// 8, 113.8 / 90.4 at 16; 64 streams cross at the same place
#define DFS_GRU_STEP_FRAMES 4

extern "C" mis_status mis_deepfilternet_stream_create(mis_deepfilternet* c, int streams, int max_hops, mis_deepfilternet_stream** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && out, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "DeepFilterNet model not finalized");
    MIS_REQUIRE(streams >= 1 && streams <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "streams must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(max_hops >= 1 && max_hops <= DFS_MAX_HOPS, MIS_ERR_INVALID_INPUT, "max_hops must be 1..%d", DFS_MAX_HOPS);
    MIS_REQUIRE(c->N == 2 * c->hop, MIS_ERR_INVALID_INPUT, "streaming needs fft_size == 2 hop_size (fft_size %d, hop_size %d): the offline "
                "frame grid and the streamer's analysis memory coincide at this ratio only", c->N, c->hop);
    MIS_REQUIRE(c->cfg.df_lookahead <= c->cfg.conv_lookahead, MIS_ERR_INVALID_INPUT, "streaming needs df_lookahead <= conv_lookahead "
                "(df_lookahead %d, conv_lookahead %d): the deep filter would read frames that have not arrived", c->cfg.df_lookahead,
                c->cfg.conv_lookahead);
    HIP_CHECK(hipSetDevice(c->device));
    auto s = std::make_unique<mis_deepfilternet_stream>();
    s->m = c; s->S = streams; s->maxh = max_hops; s->L = c->cfg.conv_lookahead; s->thr = DFS_GRU_STEP_FRAMES;
    const int nb = (int)c->bufs.size() - 1;                                   // the last is the offline waveform
    // ---- history a buffer carries
    std::vector<int> hist(nb, 0), which(nb, 1);
    const int pad_left = c->cfg.df_order - 1 - c->cfg.df_lookahead;
    hist[c->b_spec] = s->L + pad_left;
    which[c->b_spec] = 0; which[c->b_ferb] = 0; which[c->b_fspec] = 0;
    for (const DfOp& op : c->ops) {
        if (op.kind == 0 && op.g.kT > 1 && op.in >= 0) hist[op.in] = std::max(hist[op.in], op.g.kT - 1);
        if (op.kind == 2) for (int i = 0; i < op.chains; ++i) hist[op.rout[i]] = std::max(hist[op.rout[i]], 1);
    }
    hist[c->b_fr] = std::max(hist[c->b_fr], 1);
    s->HIST = 1;
    for (int h : hist) s->HIST = std::max(s->HIST, h);
    s->nr = s->HIST + max_hops;
    // ---- the workspace
    size_t total = 0;
    std::vector<size_t> off(nb);
    for (int i = 0; i < nb; ++i) { off[i] = total; total += round_up((size_t)streams * s->nr * c->bufs[i].F * c->bufs[i].C, 64); }
    s->work.alloc(total);
    s->pcm.alloc((size_t)streams * (1 + max_hops) * c->hop);
    s->out.alloc((size_t)streams * max_hops * c->hop);
    s->state.alloc((size_t)streams * (c->E + c->D));
    s->tab.alloc(5 * DF_MAX_BATCH);
    s->h_tab.assign(5 * DF_MAX_BATCH, 0);
    s->seen.assign(streams, 0);
    s->buf.resize(nb);
    for (int i = 0; i < nb; ++i) s->buf[i] = s->work.p + off[i];
    for (int i = 0; i < nb; ++i)
        if (hist[i] > 0) {
            const int rw = c->bufs[i].F * c->bufs[i].C;
            s->rolls.push_back({s->buf[i], rw, s->nr, s->HIST, hist[i], which[i]});
            s->max_rw = std::max(s->max_rw, rw);
        }
    s->rolls.push_back({s->pcm.p, c->hop, 1 + max_hops, 1, 1, 0});
    s->max_rw = std::max(s->max_rw, c->hop);
    s->d_rolls.alloc(s->rolls.size());
    HIP_CHECK(hipMemcpy(s->d_rolls.p, s->rolls.data(), s->rolls.size() * sizeof(DfRoll), hipMemcpyHostToDevice));
    // ---- the model's launch list, bound to this workspace
    const int32_t *tn = s->tab.p, *tm = tn + DF_MAX_BATCH, *t0 = tm + DF_MAX_BATCH, *toff = t0 + DF_MAX_BATCH, *tseen = toff + DF_MAX_BATCH;
    s->ops = c->ops;
    for (DfOp& op : s->ops) {
        if (op.kind == 0) {
            DfGemm& g = op.g;
            g.cnt = op.phase == DF_PH_FRONT ? tn : tm; g.lens = nullptr; g.nr = s->nr; g.hist = s->HIST; g.t0 = t0; g.off = toff;
            g.pcm = s->pcm.p + c->hop; g.pcm_stride = (int64_t)(1 + max_hops) * c->hop;
            g.Y = s->buf[op.out];
            if (op.in >= 0) g.X = s->buf[op.in];
            if (op.res >= 0) g.R = s->buf[op.res];
        } else if (op.kind == 1) {
            DfNorm& n = op.n;
            n.spec = s->buf[op.in]; n.erb = op.res >= 0 ? s->buf[op.res] : nullptr;
            n.feat_erb = s->buf[c->b_ferb]; n.feat_spec = s->buf[c->b_fspec]; n.cnt = tn; n.nr = s->nr; n.hist = s->HIST;
            n.state = s->state.p; n.seen = tseen;
        } else if (op.kind == 2) {
            op.r.cnt = tm; op.r.nr = s->nr; op.r.hist = s->HIST;
            for (int i = 0; i < op.chains; ++i) { op.r.ch[i].gx = s->buf[op.rgx[i]]; op.r.ch[i].out = s->buf[op.rout[i]]; }
        } else if (op.kind == 3) {
            DfEnh& e = op.e;
            e.spec = s->buf[c->b_spec]; e.mask = s->buf[op.in]; e.coef = s->buf[op.res]; e.enh = s->buf[c->b_enh]; e.cnt = tm;
            e.nr = s->nr; e.hist = s->HIST; e.la = s->L; e.t0 = t0; e.off = toff;
        }
    }
    s->work.zero(c->stream); s->pcm.zero(c->stream); s->state.zero(c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    *out = s.release();
    MIS_API_END
}

extern "C" void mis_deepfilternet_stream_destroy(mis_deepfilternet_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->m->device);
    (void)hipStreamSynchronize(s->m->stream);
    delete s;
}

// back to the state after create: zero histories, hop counter 0 (the normalisation starts from its linspace again)
extern "C" mis_status mis_deepfilternet_stream_reset(mis_deepfilternet_stream* s, int stream) {
    MIS_API_BEGIN
    MIS_REQUIRE(s, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(stream >= -1 && stream < s->S, MIS_ERR_INVALID_INPUT, "stream must be -1 (all) or 0..%d", s->S - 1);
    HIP_CHECK(hipSetDevice(s->m->device));
    hipStream_t q = s->m->stream;
    for (int b = 0; b < s->S; ++b) {
        if (stream >= 0 && b != stream) continue;
        for (const DfRoll& r : s->rolls)
            HIP_CHECK(hipMemsetAsync(r.p + ((size_t)b * r.nr + r.lead - r.hist) * r.rw, 0, (size_t)r.hist * r.rw * 4, q));
        s->seen[b] = 0;
    }
    HIP_CHECK(hipStreamSynchronize(q));
    MIS_API_END
}

extern "C" int mis_deepfilternet_stream_launches(const mis_deepfilternet_stream* s) { return s ? s->last_launches : 0; }

extern "C" int64_t mis_deepfilternet_stream_hops_seen(const mis_deepfilternet_stream* s, int stream) {
    return s && stream >= 0 && stream < s->S ? s->seen[stream] : -1;
}

template <int H, int KR>
static void dfs_launch_gru(hipStream_t q, const DfOp& op, int B) {
    hipLaunchKernelGGL((k_dfn_gru<H, KR, true>), dim3(B, op.chains), dim3(3 * H), 0, q, op.r);
}

// pcm f32 [streams, stride]: stream b brings hops[b] whole hops (0..max_hops) -> out f32 [streams, out_stride], out_lens[b] samples
// (hop_size a target that became ready), lsnr f32 [streams, lsnr_rows] and lsnr_counts[b] (both may be NULL)
extern "C" mis_status mis_deepfilternet_stream_feed(mis_deepfilternet_stream* s, const float* pcm, const int32_t* hops, int64_t stride, float* out,
                                                    int64_t out_stride, int64_t* out_lens, float* lsnr, int lsnr_rows, int32_t* lsnr_counts) {
    MIS_API_BEGIN
    MIS_REQUIRE(s && pcm && hops && out && out_lens, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(!lsnr == !lsnr_counts, MIS_ERR_INVALID_INPUT, "null argument: lsnr and lsnr_counts go together");
    mis_deepfilternet* c = s->m;
    const int B = s->S, hop = c->hop, L = s->L;
    int32_t *tn = s->h_tab.data(), *tm = tn + DF_MAX_BATCH, *t0 = tm + DF_MAX_BATCH, *toff = t0 + DF_MAX_BATCH, *tseen = toff + DF_MAX_BATCH;
    int maxn = 0, maxm = 0;
    for (int b = 0; b < B; ++b) {
        MIS_REQUIRE(hops[b] >= 0 && hops[b] <= s->maxh, MIS_ERR_INVALID_INPUT, "stream %d: %d hops, a feed takes 0..%d (max_hops)", b, hops[b], s->maxh);
        MIS_REQUIRE(s->seen[b] + hops[b] < ((int64_t)1 << 30), MIS_ERR_INVALID_INPUT, "stream %d: the hop counter is full, reset the stream", b);
        maxn = std::max(maxn, hops[b]);
    }
    MIS_REQUIRE(stride >= std::max<int64_t>((int64_t)maxn * hop, 1), MIS_ERR_INVALID_INPUT, "pcm: %lld samples a stream, %lld are needed",
                (long long)stride, (long long)maxn * hop);
    for (int b = 0; b < B; ++b) {
        const int64_t h = s->seen[b];
        tn[b] = hops[b]; t0[b] = (int32_t)std::max<int64_t>(0, h - L); toff[b] = (int32_t)std::max<int64_t>(0, L - h);
        tm[b] = (int32_t)std::max<int64_t>(0, h + hops[b] - L - t0[b]); tseen[b] = (int32_t)h;
        maxm = std::max(maxm, tm[b]);
    }
    MIS_REQUIRE(out_stride >= std::max<int64_t>((int64_t)maxm * hop, 1), MIS_ERR_INVALID_INPUT, "out: room for %lld samples a stream, %lld are needed",
                (long long)out_stride, (long long)maxm * hop);
    MIS_REQUIRE(!lsnr || lsnr_rows >= std::max(maxm, 1), MIS_ERR_INVALID_INPUT, "lsnr: room for %d frames, %d are needed", lsnr_rows, maxm);
    for (int b = 0; b < B; ++b) { out_lens[b] = (int64_t)tm[b] * hop; if (lsnr_counts) lsnr_counts[b] = tm[b]; }
    s->last_launches = 0; s->ms[0] = s->ms[1] = 0.0f;
    if (maxn == 0) return MIS_OK;
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t q = c->stream;
    HIP_CHECK(hipMemcpyAsync(s->tab.p, s->h_tab.data(), s->h_tab.size() * 4, hipMemcpyHostToDevice, q));
    HIP_CHECK(hipEventRecord(s->ev[0], q));
    const int64_t ps = (int64_t)(1 + s->maxh) * hop, os = (int64_t)s->maxh * hop;
    HIP_CHECK(hipMemcpy2DAsync(s->pcm.p + hop, (size_t)ps * 4, pcm, (size_t)stride * 4, (size_t)maxn * hop * 4, B, hipMemcpyHostToDevice, q));
    int launches = 0, nrec = 0;
    const int32_t *dn = s->tab.p, *dm = dn + DF_MAX_BATCH, *dt0 = dm + DF_MAX_BATCH;
    for (DfOp& op : s->ops) {
        const int rows = op.phase == DF_PH_FRONT ? maxn : maxm;           // the launch's longest stream; a launch without rows is skipped
        if (rows == 0) continue;
        if (op.kind == 0) {
            hipLaunchKernelGGL(k_dfn_gemm<true>, dim3(cdiv((int64_t)rows * op.g.Fo, 64), cdiv(op.g.N, 64), B), dim3(256), 0, q, op.g);
        } else if (op.kind == 1) {
            hipLaunchKernelGGL(k_dfn_norm<true>, dim3(B), dim3(256), 0, q, op.n);
        } else if (op.kind == 2) {
            const bool step = rows <= s->thr;
            HIP_CHECK(hipEventRecord(s->ev[2 + 2 * nrec], q));
            if (op.H == 32) { if (step) dfs_launch_gru<32, 0>(q, op, B); else dfs_launch_gru<32, 32>(q, op, B); }
            else if (op.H == 64) { if (step) dfs_launch_gru<64, 0>(q, op, B); else dfs_launch_gru<64, 64>(q, op, B); }
            else if (op.H == 128) { if (step) dfs_launch_gru<128, 0>(q, op, B); else dfs_launch_gru<128, 128>(q, op, B); }
            else if (step) dfs_launch_gru<256, 0>(q, op, B);
            else if (c->KR == 64) dfs_launch_gru<256, 64>(q, op, B);
            else if (c->KR == 96) dfs_launch_gru<256, 96>(q, op, B);
            else dfs_launch_gru<256, 128>(q, op, B);
            HIP_CHECK(hipEventRecord(s->ev[3 + 2 * nrec], q));
            ++nrec;
        } else if (op.kind == 3) {
            op.e.nrc = rows; op.e.total = (size_t)B * rows * c->F;
            hipLaunchKernelGGL(k_dfn_enh<true>, dim3((unsigned)((op.e.total + 255) / 256)), dim3(256), 0, q, op.e);
        } else {
            hipLaunchKernelGGL(k_dfn_ola_stream, dim3(cdiv((int64_t)rows * hop, 256), B), dim3(256), 0, q, s->buf[c->b_fr], c->win, s->out.p, dm, dt0,
                               s->nr, s->HIST, c->N, hop, os);
        }
        ++launches;
    }
    hipLaunchKernelGGL(k_dfn_roll, dim3(cdiv(s->max_rw, 256), (unsigned)s->rolls.size(), B), dim3(256), 0, q, s->d_rolls.p, dn, dm);
    ++launches;
    if (maxm > 0) {
        HIP_CHECK(hipMemcpy2DAsync(out, (size_t)out_stride * 4, s->out.p, (size_t)os * 4, (size_t)maxm * hop * 4, B, hipMemcpyDeviceToHost, q));
        if (lsnr) HIP_CHECK(hipMemcpy2DAsync(lsnr, (size_t)lsnr_rows * 4, s->buf[c->b_lsnr] + s->HIST, (size_t)s->nr * 4, (size_t)maxm * 4, B,
                                             hipMemcpyDeviceToHost, q));
    }
    HIP_CHECK(hipEventRecord(s->ev[1], q));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(q));                               // the one synchronisation of a feed
    for (int b = 0; b < B; ++b) s->seen[b] += hops[b];
    float rec = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&s->ms[0], s->ev[0], s->ev[1]));
    for (int i = 0; i < nrec; ++i) { float m = 0.0f; HIP_CHECK(hipEventElapsedTime(&m, s->ev[2 + 2 * i], s->ev[3 + 2 * i])); rec += m; }
    s->ms[1] = rec;
    s->last_launches = launches;
    MIS_API_END
}

// measurements: device milliseconds of the last feed, ms[2] = the whole feed (copies included), its recurrence launches
extern "C" mis_status mis_debug_deepfilternet_stream_timing(const mis_deepfilternet_stream* s, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(s && ms, MIS_ERR_INVALID_INPUT, "null argument");
    ms[0] = s->ms[0]; ms[1] = s->ms[1];
    MIS_API_END
}

// measurements and tests: feeds of at most `frames` targets run the short-chunk recurrence (0: never, negative: the default)
extern "C" mis_status mis_debug_deepfilternet_stream_gru_step_frames(mis_deepfilternet_stream* s, int frames) {
    MIS_API_BEGIN
    MIS_REQUIRE(s, MIS_ERR_INVALID_INPUT, "null argument");
    s->thr = frames < 0 ? DFS_GRU_STEP_FRAMES : frames;
    MIS_API_END
}
