"""CPU restatement of the reference voice activity detector (Sources/MLXAudioVAD/Models/FSMNVAD/FSMNVAD.swift), written from the Swift -
the parity reference of csrc/fsmn_vad.hip and of the post-processing port in vad.py.  The front end and the encoder in torch, float32
or float64, one row at a time; the post-processing as a literal transliteration of FSMNVADPostprocess (:239-701), the copies of the
audio buffer included.  test_fsmn_vad_cpu.py holds it to independent realisations (numpy / scipy, torch.nn)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import mlx_audio_swift_amd as mas

SAMPLE_RATE, WIN, HOP, NFFT = 16000, 400, 160, 512

# name -> input_dim, input_affine, linear, proj, lorder, layers, output_affine, output_dim
CASES = {
    "S": (400, 24, 40, 16, 3, 2, 20, 7),               # small, no width a multiple of a tile
    "P": (400, 140, 250, 128, 20, 4, 140, 248),        # the published defaults
}
# chosen on the CPU (test_fsmn_vad_cpu.py::test_decision_rows): with make_weights(case_config("P"), DECISION_SEED) the float64
# reference's silence probability crosses 0.2 both ways on the decision rows and the rows give two segments / none / an open one
DECISION_SEED = 7


def case_config(name, max_batch=8, chunk_frames=3000):
    d, a, l, p, lo, n, ao, o = CASES[name]
    enc = mas.FSMNVADEncoderConfig(input_dim=d, input_affine_dim=a, fsmn_layers=n, linear_dim=l, proj_dim=p, lorder=lo,
                                   output_affine_dim=ao, output_dim=o)
    return mas.FSMNVADConfig(encoder=enc, max_batch=max_batch, chunk_frames=chunk_frames)


def _noise(g, n, amp):
    return (amp * torch.randn(n, generator=g, dtype=torch.float64)).to(torch.float32).numpy()


def burst_row(g, seconds, bursts, amp=0.1):
    """Zeros with noise of amplitude amp in every (start_s, end_s) of bursts."""
    x = np.zeros(int(seconds * SAMPLE_RATE), np.float32)
    for a, b in bursts:
        i, j = int(a * SAMPLE_RATE), min(int(b * SAMPLE_RATE), len(x))
        x[i:j] = _noise(g, j - i, amp)
    return x


def case_rows(seed=5):
    """The ragged batch of the tap test: below one window, exactly one, two frames, 16 000 and 17 777 samples, a ~3 s burst row,
    silence, and a row at int16 amplitude."""
    g = torch.Generator().manual_seed(seed)
    rows = [_noise(g, n, 0.1) for n in (399, 400, 560, 16000, 17777)]
    rows.append(burst_row(g, 3.01, [(0.4, 1.1), (2.0, 2.7)]))
    rows.append(np.zeros(8000, np.float32))
    rows.append(_noise(g, 4000, 3000.0).round())
    return rows


def decision_rows(seed=9):
    """Eight rows of 2-4 s, bursts of noise between gaps of silence."""
    g = torch.Generator().manual_seed(seed)
    spec = [(3.0, [(0.3, 1.0), (2.0, 2.6)]),        # two segments
            (2.0, []),                              # none
            (2.5, [(1.0, 2.5)]),                    # still open at the last frame
            (4.0, [(0.5, 1.2), (1.5, 2.0), (3.2, 3.9)]),
            (2.2, [(0.0, 0.6)]),
            (3.5, [(0.8, 2.9)]),
            (2.8, [(0.2, 0.45), (1.6, 2.5)]),
            (3.3, [(1.0, 1.4), (2.6, 3.3)])]
    return [burst_row(g, s, b, 0.05 + 0.02 * i) for i, (s, b) in enumerate(spec)]


def make_cmvn(cfg, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    d = cfg.encoder.input_dim
    shift = (-8.0 + 2.0 * (torch.rand(d, generator=g, dtype=torch.float64) * 2 - 1)).to(torch.float32).numpy()
    scale = (0.15 + 0.05 * (torch.rand(d, generator=g, dtype=torch.float64) * 2 - 1)).to(torch.float32).numpy()
    return shift, scale


def make_weights(cfg, seed, decisive=True):
    """Random weights under the sanitized names, float32.  Random weights alone give a near-uniform softmax, a constant "speech".  The
    recipe that makes column 0 a silence detector: run the float64 reference (with make_cmvn(cfg, seed)) on a probe row - 1 s of
    silence, then 1 s of noise of amplitude 0.1 from the seed - take out_linear1's output h_sil at row 50 and h_burst at row 150 and
    the log-sum-exp of the other columns' logits there, and set out_linear2's row 0 to k (h_sil - h_burst) and its bias so that column
    0's logit is 3 above that log-sum-exp at the silence row and 3 below it at the burst row."""
    g = torch.Generator().manual_seed(seed)
    W = {}
    for name, shape in mas.fsmn_vad_expected_shapes(cfg).items():
        u = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
        if name.endswith("bias"):
            W[name] = (0.1 * u).to(torch.float32)
        else:
            fan_in = int(np.prod(shape[1:]))
            W[name] = (u * math.sqrt(3.0 / fan_in)).to(torch.float32)
    if not decisive:
        return W
    probe = np.concatenate([np.zeros(SAMPLE_RATE, np.float32), _noise(g, SAMPLE_RATE, 0.1)])
    ref = FsmnVadRef(cfg, W, make_cmvn(cfg, seed), torch.float64)
    st = ref.stages(ref.features(probe))
    n = cfg.encoder.fsmn_layers
    h, logits = st[5 + 2 * n], st["logits"]
    h_sil, h_burst = h[50], h[150]
    lse_sil, lse_burst = torch.logsumexp(logits[50, 1:], 0), torch.logsumexp(logits[150, 1:], 0)
    d = h_sil - h_burst
    k = ((lse_sil + 3.0) - (lse_burst - 3.0)) / (d @ d)
    W["out_linear2.weight"][0] = (k * d).to(torch.float32)
    W["out_linear2.bias"][0] = float(lse_sil + 3.0 - k * (d @ h_sil))
    return W


# ---------------------------------------------------------------------------------------------------- front end
def frames_of(n):
    return 0 if n < WIN else 1 + (n - WIN) // HOP


def rows_of(T, m=5, n=1):
    return 0 if T <= 0 else (T + (m - 1) // 2 + n - 1) // n


def mel_filters(n_mels, dtype):
    """kaldiMelFilterbank (:923-955) -> [257, n_mels]; the loop stops at bin 255, so the Nyquist row stays zero.  float32: in the Swift's
    own Float arithmetic; float64: the same formulas in double."""
    t = np.float32 if dtype == torch.float32 else np.float64

    def mel(f):
        return t(1127.0) * np.log(t(1.0) + t(f) / t(700.0))

    nyq = t(0.5) * t(SAMPLE_RATE)
    width = t(SAMPLE_RATE) / t(NFFT)
    lo, hi = mel(t(20.0)), mel(t(0.0) + nyq)
    delta = (hi - lo) / t(n_mels + 1)
    fb = np.zeros((NFFT // 2 + 1, n_mels), t)
    for b in range(n_mels):
        left, center, right = lo + t(b) * delta, lo + t(b + 1) * delta, lo + t(b + 2) * delta
        for i in range(NFFT // 2):
            m = mel(width * t(i))
            fb[i, b] = max(t(0), min((m - left) / (center - left), (right - m) / (right - center)))
    return torch.from_numpy(fb)


def hamming(dtype):
    n = torch.arange(WIN, dtype=torch.float64)
    return (0.54 - 0.46 * torch.cos(2.0 * math.pi * n / (WIN - 1))).to(dtype)


_FB = {}


def fbank(wave, n_mels=80, dtype=torch.float32):
    """computeKaldiFbank (:821-864) on waveform x 32768 -> [T, n_mels]"""
    x = torch.as_tensor(np.asarray(wave, np.float32)).to(dtype) * 32768.0
    if x.numel() < WIN:
        return torch.zeros((0, n_mels), dtype=dtype)
    fr = x.unfold(0, WIN, HOP)
    fr = fr - fr.mean(dim=1, keepdim=True)
    fr = torch.cat([fr[:, :1], fr[:, 1:] - 0.97 * fr[:, :-1]], dim=1) * hamming(dtype)
    spec = torch.fft.rfft(F.pad(fr, (0, NFFT - WIN)), dim=1)
    power = spec.real ** 2 + spec.imag ** 2
    key = (n_mels, dtype)
    if key not in _FB:
        _FB[key] = mel_filters(n_mels, dtype)
    return torch.log(torch.clamp(power @ _FB[key], min=1e-8))


def decibel(wave, dtype=torch.float32):
    """computeDecibel (:373-392) -> [T]"""
    x = torch.as_tensor(np.asarray(wave, np.float32)).to(dtype)
    if x.numel() < WIN:
        return torch.zeros(0, dtype=dtype)
    return 10.0 * torch.log10((x.unfold(0, WIN, HOP) ** 2).sum(dim=1) + 1e-6)


def lfr(fb, m=5, n=1):
    """applyLFR (:866-898)"""
    T, d = fb.shape
    if T == 0:
        return fb.new_zeros((0, d * m))
    lp = (m - 1) // 2
    R = (T + lp + n - 1) // n
    idx = (torch.arange(R)[:, None] * n + torch.arange(m)[None, :] - lp).clamp(0, T - 1)
    return fb[idx].reshape(R, m * d)


def lfr_cmvn_numpy(fb, cmvn, m=5, n=1):
    """LFR + CMVN in numpy float32 on a given float32 fbank: the bit-exact statement of what the device stores"""
    fb = np.asarray(fb, np.float32)
    T, d = fb.shape
    lp = (m - 1) // 2
    R = rows_of(T, m, n)
    idx = np.clip(np.arange(R)[:, None] * n + np.arange(m)[None, :] - lp, 0, T - 1)
    out = fb[idx].reshape(R, m * d)
    if cmvn is not None and len(cmvn[0]) == m * d and len(cmvn[1]) == m * d:
        out = (out + np.asarray(cmvn[0], np.float32)) * np.asarray(cmvn[1], np.float32)
    return out


# ---------------------------------------------------------------------------------------------------- model
class FsmnVadRef:
    """features(wave) and stages(features) -> {3: in_linear1, 4: in_linear2, 5 + 2 i: layer i's projection, 6 + 2 i: its output,
    5 + 2 L: out_linear1, "logits", 6 + 2 L: scores, 7 + 2 L: the silence sum}, one row [R, C]."""

    def __init__(self, cfg, W, cmvn=None, dtype=torch.float32):
        self.cfg, self.dtype = cfg, dtype
        self.W = {k: torch.as_tensor(v).to(dtype) for k, v in W.items()}
        d = cfg.encoder.input_dim
        ok = cmvn is not None and len(cmvn[0]) == d and len(cmvn[1]) == d
        self.cmvn = (torch.as_tensor(cmvn[0]).to(dtype), torch.as_tensor(cmvn[1]).to(dtype)) if ok else None

    def cmvn_apply(self, x):
        return x if self.cmvn is None else (x + self.cmvn[0]) * self.cmvn[1]

    def features(self, wave):
        c = self.cfg
        return self.cmvn_apply(lfr(fbank(wave, c.n_mels, self.dtype), c.lfr_m, c.lfr_n))

    def lin(self, x, p, bias=True):
        return F.linear(x, self.W[p + ".weight"], self.W[p + ".bias"] if bias else None)

    def memory(self, p, i):
        w = self.W[f"fsmn.{i}.fsmn_block.conv_left.weight"][:, :, 0]                  # [proj, lorder]
        L = w.shape[1]
        pad = torch.cat([p.new_zeros((L - 1, p.shape[1])), p], dim=0)
        conv = sum(pad[j: j + p.shape[0]] * w[:, j] for j in range(L))
        return p + conv

    def stages(self, feat, start=None):
        """start: (stage, tensor) runs from that stage's output on (the device's own previous stage)"""
        e = self.cfg.encoder
        n = e.fsmn_layers
        out = {}
        x = torch.as_tensor(feat).to(self.dtype)
        out[3] = self.lin(x, "in_linear1")
        out[4] = torch.relu(self.lin(out[3], "in_linear2"))
        h = out[4]
        for i in range(n):
            out[5 + 2 * i] = self.lin(h, f"fsmn.{i}.linear", bias=False)
            h = torch.relu(self.lin(self.memory(out[5 + 2 * i], i), f"fsmn.{i}.affine"))
            out[6 + 2 * i] = h
        out[5 + 2 * n] = self.lin(h, "out_linear1")
        out["logits"] = self.lin(out[5 + 2 * n], "out_linear2")
        out[6 + 2 * n] = torch.softmax(out["logits"], dim=-1)
        out[7 + 2 * n] = self.silence(out[6 + 2 * n])
        return out

    def step(self, stage, prev):
        """The output of `stage` from the previous stage's output (a tensor of the device): what one launch computes"""
        e = self.cfg.encoder
        n = e.fsmn_layers
        x = torch.as_tensor(prev).to(self.dtype)
        if stage == 3:
            return self.lin(x, "in_linear1")
        if stage == 4:
            return torch.relu(self.lin(x, "in_linear2"))
        if stage < 5 + 2 * n:
            i = (stage - 5) // 2
            if (stage - 5) % 2 == 0:
                return self.lin(x, f"fsmn.{i}.linear", bias=False)
            return torch.relu(self.lin(self.memory(x, i), f"fsmn.{i}.affine"))
        if stage == 5 + 2 * n:
            return self.lin(x, "out_linear1")
        sc = torch.softmax(self.lin(x, "out_linear2"), dim=-1)
        return sc if stage == 6 + 2 * n else self.silence(sc)

    def silence(self, scores):
        ids = [i for i in self.cfg.sil_pdf_ids if 0 <= i < scores.shape[1]]
        s = scores.new_zeros(scores.shape[0])
        for i in ids:
            s = s + scores[:, i]
        return s

    def scores(self, wave):
        return self.stages(self.features(wave))[6 + 2 * self.cfg.encoder.fsmn_layers]


def speech_flags(sil, dec, thr):
    """frameState's comparison for every frame on its own (no noise average: it does not enter the flag) in float32"""
    s = np.clip(np.asarray(sil, np.float32), np.float32(1e-7), np.float32(1.0) - np.float32(1e-7))
    n = min(len(s), len(dec))
    with np.errstate(divide="ignore"):
        flag = np.exp(np.log(np.float32(1.0) - s)) >= np.exp(np.log(s)) + np.float32(thr)
    return flag[:n] & (np.asarray(dec, np.float32)[:n] >= -100.0)


# ---------------------------------------------------------------------------------------------------- post-processing, literally
class _SpeechBuffer:
    def __init__(self):
        self.startMs, self.endMs, self.containSegStartPoint, self.containSegEndPoint = 0, 0, False, False


class _WindowDetector:
    def __init__(self, windowSizeMs, silToSpeechTime, speechToSilTime, frameSizeMs):
        self.winSizeFrame = windowSizeMs // frameSizeMs
        self.silToSpeechFrameCountThreshold = silToSpeechTime // frameSizeMs
        self.speechToSilFrameCountThreshold = speechToSilTime // frameSizeMs
        self.reset()

    def reset(self):
        self.curWinPos, self.winSum = 0, 0
        self.winState = [0] * max(self.winSizeFrame, 1)
        self.previousFrameState = "silence"

    def detectOneFrame(self, frameState):
        current = 1 if frameState == "speech" else 0
        self.winSum -= self.winState[self.curWinPos]
        self.winSum += current
        self.winState[self.curWinPos] = current
        self.curWinPos = (self.curWinPos + 1) % len(self.winState)
        if self.previousFrameState == "silence" and self.winSum >= self.silToSpeechFrameCountThreshold:
            self.previousFrameState = "speech"
            return "silenceToSpeech"
        if self.previousFrameState == "speech" and self.winSum <= self.speechToSilFrameCountThreshold:
            self.previousFrameState = "silence"
            return "speechToSilence"
        if self.previousFrameState == "silence":
            return "silenceToSilence"
        if self.previousFrameState == "speech":
            return "speechToSpeech"
        return "invalid"


class SwiftPostprocess:
    """FSMNVADPostprocess (:349-701), statement by statement; Float arithmetic as numpy.float32.  forward(scores [R, O], waveform)."""

    def __init__(self, config):
        f32 = np.float32
        self.config = config
        self.windowDetector = _WindowDetector(config.window_size_ms, config.sil_to_speech_time_thres, config.speech_to_sil_time_thres,
                                              config.frame_in_ms)
        self.dataBufStartFrame, self.frameCount, self.latestConfirmedSpeechFrame, self.latestConfirmedSilenceFrame = 0, 0, 0, -1
        self.continuousSilenceFrameCount, self.vadStateMachine, self.confirmedStartFrame, self.confirmedEndFrame = 0, "notDetected", -1, -1
        self.numberEndTimeDetected, self.silFrame = 0, 0
        self.silPdfIds = list(config.sil_pdf_ids)
        self.noiseAverageDecibel = f32(-100.0)
        self.outputDataBuf, self.outputDataBufOffset = [], 0
        self.maxEndSilFrameCountThreshold = config.max_end_silence_time - config.speech_to_sil_time_thres
        self.speechNoiseThreshold = f32(config.speech_noise_thres)
        self.scores, self.decibel, self.dataBuf, self.dataBufAll = [], [], [], []
        self.lastDropFrames = 0

    @property
    def frameShiftSamples(self):
        return self.config.frame_in_ms * self.config.sample_rate // 1000

    def computeDecibel(self, waveform):
        frameSampleLength = self.config.frame_length * self.config.sample_rate // 1000
        shift = self.frameShiftSamples
        if len(self.dataBufAll) == 0:
            self.dataBufAll = np.array(waveform, np.float32)
            self.dataBuf = np.array(waveform, np.float32)
        else:
            self.dataBufAll = np.concatenate([self.dataBufAll, waveform])
        if len(waveform) < frameSampleLength:
            return
        start = 0
        while start + frameSampleLength <= len(waveform):
            energy = np.float32(0)
            for sample in waveform[start: start + frameSampleLength]:
                energy = np.float32(energy + sample * sample)
            self.decibel.append(np.float32(10.0) * np.log10(np.float32(energy + np.float32(1e-6))))
            start += shift

    def latency(self):
        return self.windowDetector.winSizeFrame + self.config.window_size_ms // self.config.frame_in_ms

    def popDataBufTillFrame(self, frameIndex):
        while self.dataBufStartFrame < frameIndex:
            if len(self.dataBuf) >= self.frameShiftSamples:
                self.dataBufStartFrame += 1
                start = max(0, (self.dataBufStartFrame - self.lastDropFrames) * self.frameShiftSamples)
                self.dataBuf = np.array(self.dataBufAll[start:]) if start < len(self.dataBufAll) else []
            else:
                break

    def popDataToOutputBuffer(self, startFrame, frameCount, firstFrameIsStartPoint, lastFrameIsEndPoint):
        self.popDataBufTillFrame(startFrame)
        if not self.outputDataBuf or firstFrameIsStartPoint:
            buffer = _SpeechBuffer()
            buffer.startMs = startFrame * self.config.frame_in_ms
            buffer.endMs = buffer.startMs
            self.outputDataBuf.append(buffer)
        current = self.outputDataBuf[-1]
        self.dataBufStartFrame += frameCount
        current.endMs = (startFrame + frameCount) * self.config.frame_in_ms
        if firstFrameIsStartPoint:
            current.containSegStartPoint = True
        if lastFrameIsEndPoint:
            current.containSegEndPoint = True

    def onSilenceDetected(self, validFrame):
        self.latestConfirmedSilenceFrame = validFrame
        if self.vadStateMachine == "notDetected":
            self.popDataBufTillFrame(validFrame)

    def onVoiceDetected(self, validFrame):
        self.latestConfirmedSpeechFrame = validFrame
        self.popDataToOutputBuffer(validFrame, 1, False, False)

    def onVoiceStart(self, startFrame, fakeResult=False):
        if self.confirmedStartFrame == -1:
            self.confirmedStartFrame = startFrame
        if not fakeResult and self.vadStateMachine == "notDetected":
            self.popDataToOutputBuffer(self.confirmedStartFrame, 1, True, False)

    def onVoiceEnd(self, endFrame, fakeResult, isLastFrame):
        if self.latestConfirmedSpeechFrame + 1 < endFrame:
            for frame in range(self.latestConfirmedSpeechFrame + 1, endFrame):
                self.onVoiceDetected(frame)
        if self.confirmedEndFrame == -1:
            self.confirmedEndFrame = endFrame
        if not fakeResult:
            self.silFrame = 0
            self.popDataToOutputBuffer(self.confirmedEndFrame, 1, False, True)
        self.numberEndTimeDetected += 1

    def maybeOnVoiceEndIfLastFrame(self, isFinalFrame, currentFrameIndex):
        if isFinalFrame:
            self.onVoiceEnd(currentFrameIndex, False, True)
            self.vadStateMachine = "endPointDetected"

    def resetDetection(self):
        self.continuousSilenceFrameCount, self.latestConfirmedSpeechFrame, self.latestConfirmedSilenceFrame = 0, 0, -1
        self.confirmedStartFrame, self.confirmedEndFrame, self.vadStateMachine = -1, -1, "notDetected"
        self.windowDetector.reset()
        self.silFrame = 0
        if self.outputDataBuf and self.outputDataBuf[-1].containSegEndPoint:
            dropFrames = self.outputDataBuf[-1].endMs // self.config.frame_in_ms
            realDropFrames = dropFrames - self.lastDropFrames
            self.lastDropFrames = dropFrames
            sampleDrop = realDropFrames * self.frameShiftSamples
            self.dataBufAll = np.array(self.dataBufAll[sampleDrop:]) if sampleDrop < len(self.dataBufAll) else []
            self.decibel = list(self.decibel[realDropFrames:]) if realDropFrames < len(self.decibel) else []
            self.scores = list(self.scores[realDropFrames:]) if realDropFrames < len(self.scores) else []

    def frameState(self, index):
        f32 = np.float32
        if index < 0 or index >= len(self.decibel) or index >= len(self.scores):
            return "silence"
        currentDecibel = self.decibel[index]
        currentSNR = f32(currentDecibel - self.noiseAverageDecibel)
        if currentDecibel < f32(-100.0):
            return "silence"
        sumScore, noiseProb = f32(0), np.log(f32(1e-7))
        if self.silPdfIds:
            if len(self.silPdfIds) > 1:
                for i in self.silPdfIds:
                    if i < len(self.scores[index]):
                        sumScore = f32(sumScore + self.scores[index][i])
            elif self.silPdfIds[0] < len(self.scores[index]):
                sumScore = f32(self.scores[index][self.silPdfIds[0]])
            sumScore = max(min(sumScore, f32(1.0) - f32(1e-7)), f32(1e-7))
            noiseProb = np.log(sumScore)
            sumScore = f32(1.0) - sumScore
        with np.errstate(divide="ignore"):
            speechProb = np.log(f32(sumScore))
        if np.exp(speechProb) >= np.exp(noiseProb) + self.speechNoiseThreshold:
            if currentSNR >= f32(-100.0) and currentDecibel >= f32(-100.0):
                return "speech"
            return "silence"
        if self.noiseAverageDecibel < f32(-99.9):
            self.noiseAverageDecibel = currentDecibel
        else:
            self.noiseAverageDecibel = (currentDecibel + self.noiseAverageDecibel * f32(100 - 1)) / f32(100)
        return "silence"

    def detectOneFrame(self, currentFrameState, currentFrameIndex, isFinalFrame):
        stateChange = self.windowDetector.detectOneFrame("speech" if currentFrameState == "speech" else "silence")
        frameShiftMs = self.config.frame_in_ms
        c = self.config

        def inSegment():
            if currentFrameIndex - self.confirmedStartFrame + 1 > 60000 // frameShiftMs:
                self.onVoiceEnd(currentFrameIndex, False, False)
                self.vadStateMachine = "endPointDetected"
            elif not isFinalFrame:
                self.onVoiceDetected(currentFrameIndex)
            else:
                self.maybeOnVoiceEndIfLastFrame(isFinalFrame, currentFrameIndex)

        if stateChange == "silenceToSpeech":
            self.continuousSilenceFrameCount = 0
            if self.vadStateMachine == "notDetected":
                startFrame = max(self.dataBufStartFrame, currentFrameIndex - self.latency())
                self.onVoiceStart(startFrame)
                self.vadStateMachine = "inSpeech"
                if startFrame + 1 <= currentFrameIndex:
                    for frame in range(startFrame + 1, currentFrameIndex + 1):
                        self.onVoiceDetected(frame)
            elif self.vadStateMachine == "inSpeech":
                if self.latestConfirmedSpeechFrame + 1 < currentFrameIndex:
                    for frame in range(self.latestConfirmedSpeechFrame + 1, currentFrameIndex):
                        self.onVoiceDetected(frame)
                inSegment()
        elif stateChange == "speechToSilence":
            self.continuousSilenceFrameCount = 0
            if self.vadStateMachine == "inSpeech":
                inSegment()
        elif stateChange == "speechToSpeech":
            self.continuousSilenceFrameCount = 0
            if self.vadStateMachine == "inSpeech":
                inSegment()
        elif stateChange == "silenceToSilence":
            self.continuousSilenceFrameCount += 1
            if self.vadStateMachine == "notDetected":
                if isFinalFrame and self.numberEndTimeDetected == 0:
                    if self.latestConfirmedSilenceFrame + 1 < currentFrameIndex:
                        for frame in range(self.latestConfirmedSilenceFrame + 1, currentFrameIndex):
                            self.onSilenceDetected(frame)
                    self.onVoiceStart(0, fakeResult=True)
                    self.onVoiceEnd(0, True, False)
                    self.vadStateMachine = "endPointDetected"
                elif currentFrameIndex >= self.latency():
                    self.onSilenceDetected(currentFrameIndex - self.latency())
            elif self.vadStateMachine == "inSpeech":
                if self.continuousSilenceFrameCount * frameShiftMs >= self.maxEndSilFrameCountThreshold:
                    lookbackFrame = self.maxEndSilFrameCountThreshold // frameShiftMs
                    lookbackFrame -= c.window_size_ms // frameShiftMs // 2
                    lookbackFrame -= 1
                    lookbackFrame = max(0, lookbackFrame)
                    self.onVoiceEnd(currentFrameIndex - lookbackFrame, False, False)
                    self.vadStateMachine = "endPointDetected"
                elif currentFrameIndex - self.confirmedStartFrame + 1 > 60000 // frameShiftMs:
                    self.onVoiceEnd(currentFrameIndex, False, False)
                    self.vadStateMachine = "endPointDetected"
                elif self.continuousSilenceFrameCount <= c.window_size_ms // frameShiftMs // 2 and not isFinalFrame:
                    self.onVoiceDetected(currentFrameIndex)
                else:
                    self.maybeOnVoiceEndIfLastFrame(isFinalFrame, currentFrameIndex)
        if self.vadStateMachine == "endPointDetected":
            self.resetDetection()

    def detectLastFrames(self):
        if self.vadStateMachine == "endPointDetected":
            return
        blockSize = len(self.scores)
        for i in range(blockSize - 1, -1, -1):
            frameIndex = self.frameCount - 1 - i
            state = self.frameState(frameIndex - self.lastDropFrames)
            self.detectOneFrame(state, frameIndex, i == 0)

    def forward(self, scores, waveform, decibel=None):
        """decibel: given frame energies take the place of computeDecibel's (the device's own array); the buffers are still kept"""
        waveform = np.asarray(waveform, np.float32)
        if decibel is None:
            self.computeDecibel(waveform)
        else:
            self.dataBufAll, self.dataBuf = np.array(waveform), np.array(waveform)
            self.decibel = [np.float32(v) for v in decibel]
        rows = [np.asarray(r, np.float32) for r in scores]
        self.frameCount += len(rows)
        self.scores.extend(rows)
        self.detectLastFrames()
        segments = []
        for segment in self.outputDataBuf[self.outputDataBufOffset:]:
            self.outputDataBufOffset += 1
            segments.append([segment.startMs, segment.endMs])
        return segments


def swift_segments(cfg, silence, decibel, n_samples):
    """The transliteration on two per-frame arrays: the silence sum stands as the one column sil_pdf_ids = [0] reads"""
    import copy
    c = copy.copy(cfg)
    c.sil_pdf_ids = [0] if cfg.sil_pdf_ids else []
    return SwiftPostprocess(c).forward(np.asarray(silence, np.float32)[:, None], np.zeros(n_samples, np.float32), decibel)
