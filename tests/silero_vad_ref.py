"""CPU restatement of the reference Silero VAD (Sources/MLXAudioVAD/Models/SileroVAD/SileroVAD.swift) and of segmentSpeech
(SpeechSegmenter.swift), written from the Swift - the parity reference of csrc/silero_vad.hip and of the host ports in vad.py.  The
network in torch, float32 or float64, one row at a time, every stage its own function; probsToTimestamps and the segmenter as literal
transliterations.  test_silero_vad_cpu.py holds it to independent realisations (torch.nn.Conv1d, torch.nn.LSTM, literal index lists)."""
import math

import numpy as np
import torch

import mlx_audio_swift_amd as mas

F32 = np.float32
# name -> (the branch served at 16 kHz or None for the published one, the sample rate the tests call it at)
SMALL = dict(sample_rate=16000, filter_length=64, hop_length=32, pad=16, cutoff=33, context_size=16, chunk_size=224)   # F 7 -> 4 -> 2, S = 2
CASES = {"16k": (None, 16000), "8k": (None, 8000), "S": (SMALL, 16000)}
# chosen on the CPU (test_silero_vad_cpu.py::test_decision_rows): with make_weights(case_config("16k"), DECISION_SEED) the float64
# reference's probabilities cross 0.5 and 0.35 both ways on the decision rows and at most 2 % of the chunks lie within the margin
DECISION_SEED = 3


def case_config(name, max_batch=8, max_chunks=1024):
    small, _ = CASES[name]
    kw = {} if small is None else {"branch16k": mas.SileroVADBranchConfig(**small)}
    return mas.SileroVADConfig(max_batch=max_batch, max_chunks=max_chunks, **kw)


def case_rate(name):
    return CASES[name][1]


def geometry(b):
    """(n, F, F2, F3 = S) of a branch."""
    n = b.context_size + b.chunk_size
    F = (n + b.pad - b.filter_length) // b.hop_length + 1
    F2 = (F - 1) // 2 + 1
    return n, F, F2, (F2 - 1) // 2 + 1


def _noise(g, n, amp):
    return (amp * torch.randn(n, generator=g, dtype=torch.float64)).to(torch.float32).numpy()


def case_rows(chunk, seed=5):
    """The ragged batch of the tap test: 1, chunk - 1, chunk, chunk + 1 and 5 chunk + 17 samples."""
    g = torch.Generator().manual_seed(seed)
    return [_noise(g, n, 0.1) for n in (1, chunk - 1, chunk, chunk + 1, 5 * chunk + 17)]


def burst_row(g, seconds, bursts, rate=16000, amp=0.1, floor=1e-3):
    """A noise floor with noise of amplitude amp in every (start_s, end_s) of bursts, each burst fading in and out over 80 ms."""
    x = _noise(g, int(seconds * rate), floor)
    for a, b in bursts:
        i, j = int(a * rate), min(int(b * rate), len(x))
        env = np.minimum(1.0, np.minimum(np.arange(j - i), np.arange(j - i)[::-1]) / (0.08 * rate)).astype(F32)
        x[i:j] += _noise(g, j - i, amp) * env
    return x


def decision_rows(seed=9):
    """Eight rows of 2-4 s at 16 kHz, bursts of noise between stretches of the floor."""
    g = torch.Generator().manual_seed(seed)
    spec = [(3.0, [(0.3, 1.0), (2.0, 2.6)]), (2.0, []), (2.5, [(1.0, 2.5)]), (4.0, [(0.5, 1.2), (1.5, 2.0), (3.2, 3.9)]),
            (2.2, [(0.0, 0.6)]), (3.5, [(0.8, 2.9)]), (2.8, [(0.2, 0.45), (1.6, 2.5)]), (3.3, [(1.0, 1.4), (2.6, 3.3)])]
    return [burst_row(g, s, b, amp=0.05 + 0.02 * i) for i, (s, b) in enumerate(spec)]


def make_weights(cfg, seed, decisive=True):
    """Random weights under the sanitized names, float32, both branches.  decisive: the STFT filters are real Hann-windowed cos / -sin
    (so the magnitude is a spectrum), and each branch's final_conv is set from a probe row (floor, then noise of amplitude 0.1) run
    through the float64 reference: its weight is k (relu(h) averaged over the burst chunks - the same over the floor chunks) and its bias
    puts the logit at -3 on the floor mean and +3 on the burst mean."""
    g = torch.Generator().manual_seed(seed)
    W = {}
    for name, shape in mas.silero_vad_expected_shapes(cfg).items():
        u = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
        if len(shape) == 1:
            W[name] = (0.1 * u).to(torch.float32)
        else:
            W[name] = (u * math.sqrt(3.0 / int(np.prod(shape[1:])))).to(torch.float32)
    if not decisive:
        return W
    for prefix, b in (("branch16k.", cfg.branch16k), ("branch8k.", cfg.branch8k)):
        n = torch.arange(b.filter_length, dtype=torch.float64)
        win = 0.5 - 0.5 * torch.cos(2 * math.pi * n / b.filter_length)
        ang = 2 * math.pi * torch.arange(b.cutoff, dtype=torch.float64)[:, None] * n[None] / b.filter_length
        W[prefix + "stft_conv.weight"] = torch.cat([win * torch.cos(ang), -win * torch.sin(ang)])[:, :, None].to(torch.float32)
        W[prefix + "lstm.Wx"] = (2.0 * W[prefix + "lstm.Wx"].double()).to(torch.float32)
        ref = SileroRef(b, branch_weights(W, prefix), torch.float64)
        rate = b.sample_rate
        probe = burst_row(g, 2.0, [(1.0, 2.0)], rate)
        hs = torch.relu(ref.hidden(probe))                            # [chunks, S, 128]
        per = hs.shape[0] // 2
        h_sil, h_burst = hs[per // 4: per - 2].mean((0, 1)), hs[per + 4:].mean((0, 1))
        d = h_burst - h_sil
        k = 6.0 / float(d @ d)
        W[prefix + "final_conv.weight"] = (k * d)[None, None, :].to(torch.float32)
        W[prefix + "final_conv.bias"] = torch.tensor([-3.0 - k * float(d @ h_sil)], dtype=torch.float32)
    return W


def branch_weights(W, prefix):
    return {k[len(prefix):]: v for k, v in W.items() if k.startswith(prefix)}


def case_ref(name, W, dtype):
    cfg = case_config(name)
    rate = case_rate(name)
    return SileroRef(cfg.branch(rate), branch_weights(W, "branch16k." if rate == 16000 else "branch8k."), dtype)


# ---------------------------------------------------------------------------------------------------- the network
def reflect_pad_right(x, pad):
    """reflectPadRight (:50-57): indices n - 2, n - 3, ..., n - pad - 1 of the last axis are appended."""
    if pad <= 0:
        return x
    n = x.shape[-1]
    assert n > pad
    return torch.cat([x, x[..., list(range(n - 2, n - pad - 2, -1))]], dim=-1)


def conv1d(x, w, b, stride, pad):
    """MLX Conv1d: x [N, T, Cin], w [Cout, k, Cin], zero padding `pad` on both sides -> [N, To, Cout]; taps ascending."""
    N, T, _ = x.shape
    k = w.shape[1]
    xp = torch.zeros(N, T + 2 * pad, x.shape[2], dtype=x.dtype)
    xp[:, pad: pad + T] = x
    To = (T + 2 * pad - k) // stride + 1
    out = torch.zeros(N, To, w.shape[0], dtype=x.dtype)
    for t in range(k):
        out = out + xp[:, t: t + (To - 1) * stride + 1: stride] @ w[:, t, :].t()
    return out if b is None else out + b


class SileroRef:
    """One branch (SileroVADBranch, :59-132).  Stages as the engine taps them: 0 magnitude, 1..4 conv1..conv4, 5 the gate
    pre-activations Wx x + bias, 6 the probabilities."""

    def __init__(self, b, W, dtype=torch.float32):
        self.b, self.dtype = b, dtype
        self.W = {k: v.to(dtype) for k, v in W.items()}
        self.n, self.F, self.F2, self.S = geometry(b)

    def windows(self, row):
        """predictProba's windowing (:210-222): right zero pad to a multiple of chunk, `context` zeros in front -> [chunks, n]."""
        b = self.b
        a = torch.as_tensor(np.asarray(row, F32)).to(self.dtype)
        if a.numel() == 0:
            return torch.zeros(0, self.n, dtype=self.dtype)
        a = torch.cat([torch.zeros(b.context_size, dtype=self.dtype), a, torch.zeros((-a.numel()) % b.chunk_size, dtype=self.dtype)])
        return torch.stack([a[p - b.context_size: p + b.chunk_size] for p in range(b.context_size, a.numel(), b.chunk_size)])

    def step(self, stage, x):
        """Stage `stage` (0..5) from the stage before it (0: from windows [N, n])."""
        W = self.W
        x = x.to(self.dtype)
        if stage == 0:
            y = conv1d(reflect_pad_right(x, self.b.pad)[:, :, None], W["stft_conv.weight"], None, self.b.hop_length, 0)
            re, im = y[..., : self.b.cutoff], y[..., self.b.cutoff:]
            return torch.sqrt(re * re + im * im)
        if stage <= 4:
            return torch.relu(conv1d(x, W[f"conv{stage}.weight"], W[f"conv{stage}.bias"], 2 if stage in (2, 3) else 1, 1))
        return x @ W["lstm.Wx"].t() + W["lstm.bias"]

    def gates(self, windows):
        x = windows
        for s in range(6):
            x = self.step(s, x)
        return x

    def recur(self, gates, state=None, want_hidden=False):
        """The LSTM (gates i, f, g, o) over [chunks, S, 512] pre-activations, then sigmoid(final_conv(relu(h))) averaged over a chunk's S
        steps -> (probs [chunks], state [2, 128]) or the hidden states [chunks, S, 128]."""
        W = self.W
        gates = gates.to(self.dtype)
        h = torch.zeros(128, dtype=self.dtype) if state is None else torch.as_tensor(state[0]).to(self.dtype)
        c = torch.zeros(128, dtype=self.dtype) if state is None else torch.as_tensor(state[1]).to(self.dtype)
        wf, bf = W["final_conv.weight"].reshape(128), W["final_conv.bias"][0]
        probs, hidden = [], []
        for j in range(gates.shape[0]):
            acc = torch.zeros((), dtype=self.dtype)
            for s in range(gates.shape[1]):
                z = gates[j, s] + W["lstm.Wh"] @ h
                i, f, g, o = torch.sigmoid(z[:128]), torch.sigmoid(z[128:256]), torch.tanh(z[256:384]), torch.sigmoid(z[384:])
                c = f * c + i * g
                h = o * torch.tanh(c)
                hidden.append(h)
                acc = acc + torch.sigmoid(torch.relu(h) @ wf + bf)
            probs.append(acc / gates.shape[1])
        if want_hidden:
            return torch.stack(hidden).reshape(gates.shape[0], gates.shape[1], 128) if hidden else torch.zeros(0, gates.shape[1], 128)
        return (torch.stack(probs) if probs else torch.zeros(0, dtype=self.dtype)), torch.stack([h, c])

    def hidden(self, row):
        return self.recur(self.gates(self.windows(row)), want_hidden=True)

    def predict(self, row, state=None):
        """predictProba of one row -> (probs [chunks], state [2, 128])."""
        w = self.windows(row)
        if w.shape[0] == 0:
            return torch.zeros(0, dtype=self.dtype), (torch.zeros(2, 128, dtype=self.dtype) if state is None else torch.as_tensor(state))
        return self.recur(self.gates(w), state)


# ---------------------------------------------------------------------------------------------------- transliterations
def swift_probs_to_timestamps(probs, audioLen, sampleRate, threshold, minSpeechDurationMs, minSilenceDurationMs, speechPadMs):
    """probsToTimestamps (SileroVAD.swift:265-329), line by line; Float is numpy.float32."""
    probs = [F32(p) for p in np.asarray(probs, F32).ravel()]
    threshold = F32(threshold)
    chunkSize = 512 if sampleRate == 16000 else 256
    minSpeechSamples = F32(sampleRate) * F32(minSpeechDurationMs) / F32(1000)
    minSilenceSamples = F32(sampleRate) * F32(minSilenceDurationMs) / F32(1000)
    speechPadSamples = int(F32(sampleRate) * F32(speechPadMs) / F32(1000))
    negThreshold = max(threshold - F32(0.15), F32(0.01))
    speeches = []
    triggered = False
    currentStart = 0
    tempEnd = 0
    for idx, p in enumerate(probs):
        chunkStart = idx * chunkSize
        if p >= threshold and not triggered:
            triggered = True
            currentStart = chunkStart
            tempEnd = 0
            continue
        if triggered and p >= threshold:
            tempEnd = 0
            continue
        if triggered and p < negThreshold:
            if tempEnd == 0:
                tempEnd = chunkStart
            if F32(chunkStart - tempEnd) >= minSilenceSamples:
                if F32(tempEnd - currentStart) >= minSpeechSamples:
                    speeches.append([currentStart, tempEnd])
                triggered = False
                tempEnd = 0
    if triggered:
        end = min(audioLen, len(probs) * chunkSize)
        if F32(end - currentStart) >= minSpeechSamples:
            speeches.append([currentStart, end])
    padded = []
    for s in speeches:
        start = max(0, s[0] - speechPadSamples)
        end = min(audioLen, s[1] + speechPadSamples)
        if padded and start <= padded[-1][1]:
            padded[-1][1] = max(padded[-1][1], end)
        else:
            padded.append([start, end])
    return [(a, b) for a, b in padded]


def swift_segment_runs(probs32, actualLen, sampleRate, config):
    """detectSpeechRuns behind predictProba + mergeRuns (SpeechSegmenter.swift:47-155), line by line -> [(start, end)] after merging,
    [] when no speech is found."""
    BLOCKS = 8
    probs32 = [F32(p) for p in np.asarray(probs32, F32).ravel()]
    chunkSamples = 512 if sampleRate == 16000 else 256
    blockSamples = chunkSamples * BLOCKS
    blockDurS = F32(blockSamples) / F32(sampleRate)
    n = (len(probs32) // BLOCKS) * BLOCKS
    if n == 0:
        return []
    probs256 = []
    for i in range(n // BLOCKS):
        product = F32(1)
        for k in range(BLOCKS):
            product = F32(product * F32(F32(1.0) - probs32[i * BLOCKS + k]))
        probs256.append(F32(F32(1.0) - product))
    speechPadBlocks = max(0, int(F32(config.speech_pad_ms) / F32(1000) / blockDurS))
    minSpeechBlocks = max(1, int(math.ceil(float(F32(config.min_speech_ms) / F32(1000) / blockDurS))))
    minSilenceBlocks = max(1, int(math.ceil(float(F32(config.min_silence_ms) / F32(1000) / blockDurS))))
    runs = []
    inSpeech = False
    segStart = 0
    lastSpeech = -1
    silentRun = 0
    for idx, p in enumerate(probs256):
        if p >= F32(config.threshold):
            if not inSpeech:
                segStart = max(0, idx - speechPadBlocks)
                inSpeech = True
            lastSpeech = idx
            silentRun = 0
        elif inSpeech:
            silentRun += 1
            if silentRun >= minSilenceBlocks:
                segEnd = min(lastSpeech + 1 + speechPadBlocks, len(probs256))
                if segEnd - segStart >= minSpeechBlocks:
                    s = segStart * blockSamples
                    e = min(segEnd * blockSamples, actualLen)
                    if s < e:
                        runs.append((s, e))
                inSpeech = False
                silentRun = 0
                lastSpeech = -1
    if inSpeech:
        endIdx = min(len(probs256), lastSpeech + 1 + speechPadBlocks)
        if endIdx - segStart >= minSpeechBlocks:
            s = segStart * blockSamples
            e = min(endIdx * blockSamples, actualLen)
            if s < e:
                runs.append((s, e))
    if not runs:
        return runs
    maxChunkSamples = max(1, int(F32(config.max_chunk_s) * F32(sampleRate)))
    maxGapSamples = int(F32(config.merge_gap_s) * F32(sampleRate))

    def splitLong(start, end):
        if end - start <= maxChunkSamples:
            return [(start, end)]
        parts = []
        cur = start
        while cur < end:
            nxt = min(cur + maxChunkSamples, end)
            parts.append((cur, nxt))
            cur = nxt
        return parts

    merged = splitLong(*runs[0])
    for r in runs[1:]:
        prev = merged[-1]
        gap = r[0] - prev[1]
        newDur = r[1] - prev[0]
        if gap <= maxGapSamples and newDur <= maxChunkSamples:
            merged[-1] = (prev[0], r[1])
        else:
            merged.extend(splitLong(*r))
    return merged


def swift_segment_speech(audio, probs32, sampleRate, config):
    """segmentSpeech (:162-183) on given probabilities -> [(start, end, offset_s)]; the whole buffer when no speech is found."""
    runs = swift_segment_runs(probs32, len(audio), sampleRate, config)
    if not runs:
        return [(0, len(audio), 0.0)]
    return [(s, e, float(F32(s) / F32(sampleRate))) for s, e in runs]


class FakeVad:
    """A vad_model for segment_speech on the CPU: predict_proba returns the probabilities it was given."""

    def __init__(self, probs):
        self.probs = np.asarray(probs, F32)

    def predict_proba(self, audio, sample_rate=16000):
        return self.probs


def exempt_chunks(p64, p32, thresholds=(0.5, 0.35)):
    """The chunks whose decision the float32 reference's own error can flip: within 4 max|p32 - p64| + 1e-6 of a threshold."""
    p64 = np.asarray(p64, np.float64)
    margin = 4.0 * float(np.abs(np.asarray(p32, np.float64) - p64).max(initial=0.0)) + 1e-6
    out = np.zeros(len(p64), bool)
    for t in thresholds:
        out |= np.abs(p64 - float(F32(t))) < margin
    return out
