"""The host side of the Nemotron stream session without a device: the session's own frame bookkeeping (mis_nemotron_stream_plan, the pure
function every feed runs per stream and pass; mas.StreamFrames binds it) against a literal transliteration of streamEncodeChunks +
frozenMelFrames (NemotronASRStreaming.swift, NemotronASRStreamSession.swift), the chunk_ms mapping, the sentence split, and the assembly
of deltas by transcribe_streaming."""
import numpy as np
import pytest

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.nemotron import NemotronASR
import nemotron_ref as N


class Literal:
    """one mel chunk an iteration, as the reference walks them; sub.shape[1] is the stem's three-fold floor(n / 2) + 1"""

    def __init__(self, cf):
        self.cf, self.consumed, self.emitted, self.cache, self.frames = cf, 0, 0, 0, []

    def frozen(self, count, total):
        if count < 256:
            return 0
        return min(total, (count - 256) // 160 + 1)

    def advance(self, count, final):
        if count == 0:
            return
        total = 1 + count // 160
        limit, chunk_mel = total if final else self.frozen(count, total), self.cf * 8
        while self.consumed < limit:
            end = min(self.consumed + chunk_mel, limit)
            if not final and end - self.consumed < chunk_mel:
                break
            win_len = self.cache + end - self.consumed
            is_final = final and end >= limit
            base = (self.consumed - self.cache) // 8
            lo = self.emitted - base
            hi = N.frames(win_len) if is_final else end // 8 - base
            self.consumed, self.cache = end, min(win_len, 16)
            self.emitted = base + max(lo, hi)
            self.frames += list(range(base + lo, base + hi))


@pytest.mark.parametrize("max_chunks", [1, 3])
@pytest.mark.parametrize("cf", [1, 2, 14])
def test_frame_bookkeeping_equals_the_reference_loop(cf, max_chunks):
    chunk = cf * 8 * 160
    patterns = ([1280], [1, 640, 3], [0, 159, 161, 1], [chunk + 1, 0, 7], [3 * chunk + 1281])
    for n in range(0, 3 * chunk + 1, 3 if cf == 1 else 131):         # both steps are coprime to 160 and 1280: every residue of hop and 8 hop shows up
        for pat in patterns:
            lit, mine, got, seen, i = Literal(cf), mas.StreamFrames(cf, max_chunks), [], 0, 0
            while seen < n:
                seen = min(n, seen + pat[i % len(pat)])
                i += 1
                lit.advance(seen, False)
                for first, count in mine.advance(seen, False):
                    got += list(range(first, first + count))
                assert got == lit.frames, (n, pat, seen)
            lit.advance(n, True)
            for first, count in mine.advance(n, True):
                got += list(range(first, first + count))
            want = list(range(N.frames(1 + n // 160))) if n else []
            assert got == lit.frames == want, (n, pat)                   # every offline frame once, in order


def test_chunk_ms_follows_the_latency_ladder():
    ladder = {80: (56, 0), 160: (56, 1), 320: (56, 3), 560: (56, 6), 1120: (56, 13), 1: (56, 0), None: (56, 13)}
    assert {ms: mas.chunk_context(ms, (56, 13)) for ms in ladder} == ladder


def test_segments_follow_the_sentence_rule():
    T = mas.ParakeetToken
    toks = [T(1, " a", 0.0, 0.08), T(2, ".", 0.08, 0.08), T(3, "5", 0.16, 0.08), T(4, ".", 0.24, 0.08), T(5, " b", 0.4, 0.08), T(6, "?", 0.48, 0.08),
            T(7, " c", 0.8, 0.08)]
    assert mas.nemo_tokens_to_sentences(toks) == [dict(text=" a.5.", start=0.0, end=0.24 + 0.08), dict(text=" b?", start=0.4, end=0.48 + 0.08),
                                                  dict(text=" c", start=0.8, end=0.8 + 0.08)]
    assert mas.nemo_tokens_to_sentences([]) == []


def test_transcribe_streaming_assembles_the_deltas():
    class Fake:
        def __init__(self):
            self.text, self.tokens, self.fed, self.closed = "", [], [], False

        def step(self, samples):
            self.fed.append(len(samples))
            piece = " ab" if len(self.fed) % 2 else ""
            self.text += piece
            return mas.Delta(piece, [])

        def finish(self):
            self.text += " end "
            return mas.Delta(" end ", [])

        def close(self):
            self.closed = True

    fake, seen = Fake(), []
    model = NemotronASR.__new__(NemotronASR)
    model.config = mas.NemotronConfig()
    model.make_stream_session = lambda language=None: fake              # the device session's place
    out = model.transcribe_streaming(np.zeros(16000, np.float32), chunk_ms=480, on_delta=seen.append)
    assert fake.fed == [7680, 7680, 640] and seen == [" ab", " ab", " end "] and out.text == "ab ab end" and fake.closed
