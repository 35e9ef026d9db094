// step_loop.h - the host side of the decode loops, written once: event and captured-graph owners, the frame loop of the
// frame-synchronous TTS engines (Marvis, Qwen3-TTS) and the chunked audio pipeline of their generate / generateStream.  Host code only.
#pragma once
#include "common.h"
#include <string.h>
#include <chrono>
#include <deque>
#include <functional>
#include <memory>

// ---------------------------------------------------------------------------- N events, destroyed on every exit path
template <int N>
struct HipEvents {
    hipEvent_t e[N] = {};
    explicit HipEvents(unsigned flags = hipEventDefault) {
        try { for (auto& x : e) HIP_CHECK(hipEventCreateWithFlags(&x, flags)); } catch (...) { destroy(); throw; }
    }
    HipEvents(const HipEvents&) = delete;
    HipEvents& operator=(const HipEvents&) = delete;
    ~HipEvents() { destroy(); }
    hipEvent_t operator[](int i) const { return e[i]; }
private:
    void destroy() { for (auto& x : e) if (x) { (void)hipEventDestroy(x); x = nullptr; } }
};

// ---------------------------------------------------------------------------- one captured step, instantiated
struct StepGraph {
    StepGraph() = default;
    StepGraph(const StepGraph&) = delete;
    StepGraph& operator=(const StepGraph&) = delete;
    ~StepGraph() { reset(); }
    // body() enqueues the step on s.  A throwing body ends the capture and drops the dead graph; the hipGraph_t is destroyed on every
    // path, a failed instantiate included.
    template <class Body>
    void capture(hipStream_t s, Body&& body) {
        reset();
        hipGraph_t g = nullptr;
        HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try { body(); } catch (...) { (void)hipStreamEndCapture(s, &g); if (g) (void)hipGraphDestroy(g); throw; }
        HIP_CHECK(hipStreamEndCapture(s, &g));
        size_t n = 0;
        hipError_t err = hipGraphGetNodes(g, nullptr, &n);
        if (err == hipSuccess) err = hipGraphInstantiate(&exec_, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (err != hipSuccess) { exec_ = nullptr; throw MisError(MIS_ERR_DEVICE, std::string("instantiating the captured graph failed: ") + hipGetErrorString(err)); }
        nodes_ = (int)n;
    }
    void launch(hipStream_t s) const { HIP_CHECK(hipGraphLaunch(exec_, s)); }
    void reset() { if (exec_) (void)hipGraphExecDestroy(exec_); exec_ = nullptr; nodes_ = 0; }
    int nodes() const { return nodes_; }                    // what the captured graph really holds
    explicit operator bool() const { return exec_ != nullptr; }
private:
    hipGraphExec_t exec_ = nullptr;
    int nodes_ = 0;
};

// ---------------------------------------------------------------------------- the frame loop
// generateStream: the frame loop tells the caller whenever another `chunk_frames` frames of every row are final on the loop's
// stream, and lets it look for finished work after every host synchronisation.
struct FrameStreamHook {
    int chunk_frames = 0;
    std::function<void(int f0, int fn)> on_boundary;    // frames [f0, f0 + fn) were just enqueued on the loop's stream
    std::function<void(int f)> pre_sync;                // f frames enqueued; the loop is about to synchronise with the host
    std::function<void(int f)> poll;                    // ... and has
    std::function<void()> loop_done;                    // every row has ended (before the frames after the last full chunk go out)
};

// Up to max_frames frames, 8 between two reads of the done count (with a hook: clipped to the next chunk boundary); ends when every
// row is done - looked at before the cancel flag, so a finished batch is never reported cancelled.  The device comes in as callables:
//   frame()      enqueue one frame                      copy_done()  enqueue the copy of the done count
//   sync_done()  synchronise; the count just copied     loop_ended() after the loop (the launch-error check)
//   longest()    only with a hook: the longest row's frame count, read back
template <class Frame, class CopyDone, class SyncDone, class LoopEnded, class Longest>
static void run_frame_loop(int max_frames, int batch, const volatile int* cancel, FrameStreamHook* hook, Frame&& frame, CopyDone&& copy_done,
                           SyncDone&& sync_done, LoopEnded&& loop_ended, Longest&& longest) {
    int f = 0, last_boundary = 0;
    const int poll = 8;
    while (f < max_frames) {
        int chunk = std::min(poll, max_frames - f);
        if (hook) chunk = std::min(chunk, last_boundary + hook->chunk_frames - f);
        for (int i = 0; i < chunk; ++i) frame();
        f += chunk;
        if (hook && f - last_boundary == hook->chunk_frames) { hook->on_boundary(last_boundary, f - last_boundary); last_boundary = f; }
        copy_done();
        if (hook) hook->pre_sync(f);
        const int done = sync_done();
        if (hook) hook->poll(f);
        if (done >= batch) break;
        if (cancel && *cancel) throw MisError(MIS_ERR_CANCELLED, "generation cancelled");
    }
    loop_ended();
    if (hook) {   // the frames after the last full chunk: rows still running there have <= f - last_boundary of them
        const int n = longest();
        hook->loop_done();
        if (n > last_boundary) hook->on_boundary(last_boundary, n - last_boundary);
    }
}

// ---------------------------------------------------------------------------- the chunked audio pipeline above the frame loop
// Whenever another chunk of frames is final, the codec's stream step of the whole batch runs on the codec's stream WHILE the frame loop
// continues on the loop's; each row's new samples are delivered as MIS_EVENT_AUDIO as soon as they are on the host, the frames' codes
// as MIS_EVENT_TOKEN at every poll, one MIS_EVENT_INFO per row when the loop ends.  The engine supplies `decode` (and opens and closes
// the codec session); the loop's code store is [batch][max_frames][width], the frame counts [batch].
struct ChunkedAudio {
    struct Chunk { int f0, fn; PinnedBuf<float> wav; PinnedBuf<int32_t> nf; HipEvents<1> done{hipEventDisableTiming}; bool emitted = false; };
    int batch, width, max_frames;
    int64_t up;                                          // samples per frame
    hipStream_t s_lm, s_codec;
    const DevBuf<int32_t>*codes, *n_frames;              // (allocated by the frame loop: read when used)
    mis_event_cb on_event;
    void* user;
    int token_width;                                     // leading codes of a frame that one MIS_EVENT_TOKEN carries
    const int32_t* prompt_lens = nullptr;                // mis_gen_info.prompt_token_count per row (NULL: 0)
    std::function<void(int f0, int fn, float* wav, int64_t row_stride)> decode;     // frames [f0, f0 + fn) -> wav on s_codec
    std::function<void(int b, int nf, int f)> row_polled;                           // after row b's tokens of a poll (nf of f frames exist)
    std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    std::deque<std::unique_ptr<Chunk>> chunks;
    DevBuf<float> wav_dev;
    HipEvents<1> ev_lm{hipEventDisableTiming};
    PinnedBuf<int32_t> tok_codes, tok_nf;
    int tok_f = 0, tok_pending_f = 0;

    ChunkedAudio(int batch, int width, int max_frames, int chunk_frames, int64_t up, hipStream_t s_lm, hipStream_t s_codec,
                 const DevBuf<int32_t>* codes, const DevBuf<int32_t>* n_frames, mis_event_cb on_event, void* user, int token_width)
        : batch(batch), width(width), max_frames(max_frames), up(up), s_lm(s_lm), s_codec(s_codec), codes(codes), n_frames(n_frames),
          on_event(on_event), user(user), token_width(token_width) {
        wav_dev.alloc((size_t)batch * std::min(chunk_frames, max_frames) * up);
        tok_codes.alloc((size_t)batch * 8 * width);
        tok_nf.alloc(batch);
    }
    void on_boundary(int f0, int fn) {
        auto ch = std::make_unique<Chunk>();
        ch->f0 = f0; ch->fn = fn;
        ch->wav.alloc((size_t)batch * fn * up);
        ch->nf.alloc(batch);
        HIP_CHECK(hipEventRecord(ev_lm[0], s_lm));                   // frames < f0 + fn are final once this fires
        HIP_CHECK(hipStreamWaitEvent(s_codec, ev_lm[0], 0));
        decode(f0, fn, wav_dev.p, (int64_t)fn * up);
        HIP_CHECK(hipMemcpyAsync(ch->wav.p, wav_dev.p, (size_t)batch * fn * up * 4, hipMemcpyDeviceToHost, s_codec));
        // rows that ended inside / before this chunk keep their count; running rows have >= f0 + fn (clipped at emission)
        HIP_CHECK(hipMemcpyAsync(ch->nf.p, n_frames->p, (size_t)batch * 4, hipMemcpyDeviceToHost, s_codec));
        HIP_CHECK(hipEventRecord(ch->done[0], s_codec));
        chunks.push_back(std::move(ch));
    }
    void pre_sync(int f) {                                           // the codes of the frames since the last poll: at most 8
        MIS_REQUIRE(f - tok_f <= 8, MIS_ERR_GENERATION_FAILED, "token window");
        if (f > tok_f)
            HIP_CHECK(hipMemcpy2DAsync(tok_codes.p, (size_t)8 * width * 4, codes->p + (size_t)tok_f * width, (size_t)max_frames * width * 4,
                                       (size_t)(f - tok_f) * width * 4, batch, hipMemcpyDeviceToHost, s_lm));
        HIP_CHECK(hipMemcpyAsync(tok_nf.p, n_frames->p, (size_t)batch * 4, hipMemcpyDeviceToHost, s_lm));
        tok_pending_f = f;
    }
    void poll() {
        for (int b = 0; b < batch; ++b) {
            for (int i = tok_f; i < std::min(tok_nf.p[b], tok_pending_f); ++i)
                on_event(user, b, MIS_EVENT_TOKEN, &tok_codes.p[((size_t)b * 8 + (i - tok_f)) * width], token_width);
            if (row_polled) row_polled(b, tok_nf.p[b], tok_pending_f);
        }
        tok_f = tok_pending_f;
        emit_ready(false);
    }
    void loop_done() {
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        for (int b = 0; b < batch; ++b) {
            mis_gen_info info{};
            info.prompt_token_count = prompt_lens ? prompt_lens[b] : 0;
            info.generation_token_count = tok_nf.p[b];
            info.generate_time = secs;
            info.tokens_per_second = secs > 0 ? tok_nf.p[b] / secs : 0;
            info.peak_memory_gb = (double)(total_b - free_b) / 1e9;
            on_event(user, b, MIS_EVENT_INFO, &info, 1);
        }
    }
    void emit_ready(bool wait) {
        for (auto& ch : chunks) {
            if (ch->emitted) continue;
            if (wait) HIP_CHECK(hipEventSynchronize(ch->done[0]));
            else if (hipEventQuery(ch->done[0]) != hipSuccess) { (void)hipGetLastError(); break; }     // chunks finish in order
            for (int b = 0; b < batch; ++b) {
                const int valid = std::min(std::max(ch->nf.p[b] - ch->f0, 0), ch->fn);
                if (valid > 0) on_event(user, b, MIS_EVENT_AUDIO, ch->wav.p + (size_t)b * ch->fn * up, (int64_t)valid * up);
            }
            ch->emitted = true;
        }
    }
    // every row's pcm is the concatenation of its chunks: host f32 [batch][stride], nf the rows' final frame counts
    void gather(float* host, int64_t stride, const std::vector<int32_t>& nf) const {
        for (auto& ch : chunks)
            for (int b = 0; b < batch; ++b) {
                const int valid = std::min(std::max(nf[b] - ch->f0, 0), ch->fn);
                if (valid > 0) memcpy(host + (size_t)b * stride + (size_t)ch->f0 * up, ch->wav.p + (size_t)b * ch->fn * up, (size_t)valid * up * 4);
            }
    }
    FrameStreamHook hook(int chunk_frames) {
        FrameStreamHook h;
        h.chunk_frames = chunk_frames;
        h.on_boundary = [this](int f0, int fn) { on_boundary(f0, fn); };
        h.pre_sync = [this](int f) { pre_sync(f); };
        h.poll = [this](int) { poll(); };
        h.loop_done = [this]() { loop_done(); };
        return h;
    }
};
