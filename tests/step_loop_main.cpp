// Stand-alone check of run_frame_loop in csrc/step_loop.h (test_step_loop_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it): the frame loop of Marvis and Qwen3-TTS driven by recording fakes, its full call trace compared with traces
// written out below.  Host code only: no HIP call is made, no device is opened.
#include "../mlx-audio-swift_amd/csrc/step_loop.h"

#include <stdio.h>
#include <string>

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// One run of the loop.  The trace holds every call in order; consecutive frame launches are written "launch xN".
struct Run {
    int batch = 2;
    int done_at = -1;            // the read behind this many frames reports every row done (-1: never)
    int cancel_at = -1;          // the synchronisation behind this many frames raises the cancel flag
    int throw_at_launch = -1;    // the frame body throws on this call (1-based)
    int longest_row = 0;
    volatile int cancel = 0;
    int launches = 0, run_len = 0;
    std::string trace;

    void flush() { if (run_len) { trace += "launch x" + std::to_string(run_len) + "; "; run_len = 0; } }
    void say(const std::string& what) { flush(); trace += what + "; "; }
    static std::string call(const char* name, int a) { return std::string(name) + "(" + std::to_string(a) + ")"; }
    static std::string call(const char* name, int a, int b) { return std::string(name) + "(" + std::to_string(a) + "," + std::to_string(b) + ")"; }

    // what the loop ended with: "ok", "cancelled" (MisError MIS_ERR_CANCELLED) or "threw" (the frame body's exception)
    std::string go(int max_frames, int chunk_frames) {
        FrameStreamHook hook;
        hook.chunk_frames = chunk_frames;
        hook.on_boundary = [&](int f0, int fn) { say(call("boundary", f0, fn)); };
        hook.pre_sync = [&](int f) { say(call("pre_sync", f)); };
        hook.poll = [&](int f) { say(call("poll", f)); };
        hook.loop_done = [&]() { say("loop_done"); };
        std::string end = "ok";
        try {
            run_frame_loop(max_frames, batch, &cancel, chunk_frames > 0 ? &hook : nullptr,
                           [&]() { if (++launches == throw_at_launch) { say("throw"); throw std::runtime_error("frame body"); } ++run_len; },
                           [&]() { say("copy_done"); },
                           [&]() { say("sync"); if (launches == cancel_at) cancel = 1; return launches == done_at ? batch : 0; },
                           [&]() { say("loop_ended"); },
                           [&]() { say("longest"); return longest_row; });
        } catch (const MisError& e) {
            CHECK(e.code == MIS_ERR_CANCELLED && std::string(e.what()) == "generation cancelled");
            end = "cancelled";
        } catch (const std::runtime_error&) { end = "threw"; }
        flush();
        return end;
    }
};

#define EXPECT_TRACE(run, want)                                                                     \
    do {                                                                                            \
        if ((run).trace != std::string(want)) {                                                     \
            printf("FAILED line %d: trace\n  got  %s\n  want %s\n", __LINE__, (run).trace.c_str(), want); \
            ++failures;                                                                             \
        }                                                                                           \
    } while (0)

int main() {
    {   // 1. no hook, 20 frames, rows never done: launch groups 8, 8, 4; synchronisations at f = 8, 16, 20; no hook call
        Run r;
        CHECK(r.go(20, 0) == "ok");
        EXPECT_TRACE(r, "launch x8; copy_done; sync; launch x8; copy_done; sync; launch x4; copy_done; sync; loop_ended; ");
        CHECK(r.launches == 20);
    }
    {   // 2. chunk_frames 12, 20 frames, never done, longest row 20: the chunk is clipped to the boundary, the tail is the last 8 frames
        Run r;
        r.longest_row = 20;
        CHECK(r.go(20, 12) == "ok");
        EXPECT_TRACE(r, "launch x8; copy_done; pre_sync(8); sync; poll(8); "
                        "launch x4; boundary(0,12); copy_done; pre_sync(12); sync; poll(12); "
                        "launch x8; copy_done; pre_sync(20); sync; poll(20); "
                        "loop_ended; longest; loop_done; boundary(12,8); ");
    }
    {   // 3. chunk_frames 3, 20 frames, every row done at the read behind f = 6, longest row 5: no tail boundary
        Run r;
        r.done_at = 6; r.longest_row = 5;
        CHECK(r.go(20, 3) == "ok");
        EXPECT_TRACE(r, "launch x3; boundary(0,3); copy_done; pre_sync(3); sync; poll(3); "
                        "launch x3; boundary(3,3); copy_done; pre_sync(6); sync; poll(6); "
                        "loop_ended; longest; loop_done; ");
    }
    {   // 4. cancel raised during the first synchronisation, rows not done: thrown after poll, neither loop_done nor a tail boundary
        Run r;
        r.cancel_at = 8; r.longest_row = 8;
        CHECK(r.go(20, 12) == "cancelled");
        EXPECT_TRACE(r, "launch x8; copy_done; pre_sync(8); sync; poll(8); ");
        Run plain;                                   // the same without a hook
        plain.cancel_at = 8;
        CHECK(plain.go(20, 0) == "cancelled");
        EXPECT_TRACE(plain, "launch x8; copy_done; sync; ");
    }
    {   // 5. cancel raised in the same read that reports every row done: done wins, the loop ends normally
        Run r;
        r.cancel_at = 8; r.done_at = 8; r.longest_row = 8;
        CHECK(r.go(20, 12) == "ok");
        EXPECT_TRACE(r, "launch x8; copy_done; pre_sync(8); sync; poll(8); loop_ended; longest; loop_done; boundary(0,8); ");
        CHECK(r.cancel == 1);
    }
    {   // 6. max_frames 1, chunk_frames 4, longest 1: one launch, the only boundary is the tail
        Run r;
        r.longest_row = 1;
        CHECK(r.go(1, 4) == "ok");
        EXPECT_TRACE(r, "launch x1; copy_done; pre_sync(1); sync; poll(1); loop_ended; longest; loop_done; boundary(0,1); ");
    }
    {   // 7. a frame body that throws on its third call: the exception propagates, nothing is called after it
        Run r;
        r.throw_at_launch = 3; r.longest_row = 2;
        CHECK(r.go(20, 12) == "threw");
        EXPECT_TRACE(r, "launch x2; throw; ");
    }
    {   // 8. chunk_frames equal to the poll interval, 16 frames, longest row 16: every boundary inside the loop, no tail
        Run r;
        r.longest_row = 16;
        CHECK(r.go(16, 8) == "ok");
        EXPECT_TRACE(r, "launch x8; boundary(0,8); copy_done; pre_sync(8); sync; poll(8); "
                        "launch x8; boundary(8,8); copy_done; pre_sync(16); sync; poll(16); "
                        "loop_ended; longest; loop_done; ");
    }
    {   // 9. a cancel flag that is NULL is never read; a row count of one ends on its own done count
        FrameStreamHook* none = nullptr;
        int launches = 0, syncs = 0;
        run_frame_loop(40, 1, nullptr, none, [&]() { ++launches; }, []() {}, [&]() { return ++syncs == 2 ? 1 : 0; }, []() {}, []() { return 0; });
        CHECK(launches == 16 && syncs == 2);
    }
    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("step_loop ok\n");
    return 0;
}
