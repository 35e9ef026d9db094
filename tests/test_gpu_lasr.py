"""-m gpu: the LASR CTC engine (csrc/lasr.hip) through the C ABI against tests/lasr_ref.py, which test_lasr_cpu.py holds to
transformers' LasrForCTC and to a scipy front end.

Gate (the idiom of test_gpu_smartturn.py): relative rms distance of the device to the reference with bf16 rounding points <= 2 x the
distance of the reference's own float64-accumulation realisation to it, + 2e-3.  The stages are held one after the other, each on the
device's own previous stage (features -> stem -> block i -> logits); the distance to the reference WITHOUT rounding is recorded, not
gated.  A row is always compared with the reference of that row alone: the batch-1 rule.  MIS_LASR_PARITY_LOG=<file> keeps every
observed value (profiles/lasr/parity_observed.jsonl)."""
import functools
import json
import os

import numpy as np
import pytest

import lasr_ref as R
import mlx_audio_swift_amd as mas
from gpu_util import observe, record, rms

pytestmark = pytest.mark.gpu

FLOOR_FACTOR, SLACK = 2.0, 2e-3


def _log(row):
    path = os.environ.get("MIS_LASR_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _observe(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    _log(dict(test=name, kind=kind, value=float(value), tol=float(tol)))
    return observe(kind, value, tol)


def _record(name, **kw):
    _log(dict(test=name, **{k: (float(v) if isinstance(v, (int, float, np.floating, np.integer)) else v) for k, v in kw.items()}))
    record(name, **kw)


def _relrms(a, b):
    b = np.asarray(b, np.float64)
    return rms(a, b) / max(float(np.sqrt(np.mean(b ** 2))), 1e-30)


@functools.lru_cache(maxsize=None)
def _weights(name, seed=R.DECISION_SEED, blank_bias=0.0):
    return R.make_weights(R.case_config(name), seed, blank_bias)


@functools.lru_cache(maxsize=None)
def _model(name, seed=R.DECISION_SEED, blank_bias=0.0, max_batch=8, max_seconds=12):
    cfg = R.case_config(name)
    return cfg, mas.LasrCTCModel.from_weights(mas.LasrCTCConfig.from_dict(cfg, max_batch=max_batch, max_seconds=max_seconds),
                                              _weights(name, seed, blank_bias))


def _audio(lens, seed=3):
    rng = np.random.default_rng(seed)
    return [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]


def _lens_for_t2(model, want):
    """The smallest sample count (a multiple of the hop) whose row has `want` encoder frames (mis_lasr_frames)."""
    n = np.arange(0, 4000) * 160
    _, T2 = model.frames(n)
    assert all((T2 == t).any() for t in want)
    return [int(n[np.argmax(T2 == t)]) for t in want]


def _chain_gates(cfg, W, model, audios, tag, per_row=True):
    """Calls forward on the batch, then holds every row's stem, blocks and logits against the references resumed from the device's own
    previous stage.  per_row: one gate per row and stage; else one gate per stage over the valid frames of all rows (the per-row values
    are still recorded).  Returns (ok, logits, T2)."""
    L = cfg["encoder_config"]["num_hidden_layers"]
    feats = model.features(audios)
    logits = model.forward(audios)
    taps = [model.tap(s) for s in range(L + 2)]
    F, T2 = model.frames([len(a) for a in audios])
    rb, r64, rx = R.Ref(cfg, W, round=True, acc=np.float32), R.Ref(cfg, W, round=True, acc=np.float64), R.Ref(cfg, W)
    ok, pool = True, {}

    def hold(stage, b, dev, a, c):
        nonlocal ok
        if per_row:
            ok &= _observe(f"{tag}_row{b}_{stage}", _relrms(dev, a), FLOOR_FACTOR * _relrms(c, a) + SLACK)
        else:
            _record(f"{tag}_row{b}_{stage}", value=_relrms(dev, a), floor=_relrms(c, a))
            pool.setdefault(stage, []).append((np.ravel(dev), np.ravel(a), np.ravel(c)))

    for b in range(len(audios)):
        t = int(T2[b])
        for tp in taps:
            assert not tp[b, t:].any(), "rows behind T2[b] must be exactly zero"
        assert not logits[b, t:].any()
        f = feats[b, : F[b]]
        prev = None
        for s in range(L + 1):
            if s == 0:
                a, c, x = (r.forward(f)["stem"] for r in (rb, r64, rx))
            else:
                a, c, x = (r.forward(None, start=(s - 1, prev))["blocks"][0] for r in (rb, r64, rx))
            dev = taps[s][b, :t]
            hold(f"stage{s}", b, dev, a, c)
            _record(f"{tag}_row{b}_stage{s}_unrounded", value=_relrms(dev, x))
            prev = dev
        a, c = (r.forward(None, start=(L, prev)) for r in (rb, r64))
        hold("out_norm", b, taps[L + 1][b, :t], a["out_norm"], c["out_norm"])
        hold("logits", b, logits[b, :t], a["logits"], c["logits"])
    for stage, parts in pool.items():
        dev, a, c = (np.concatenate(v) for v in zip(*parts))
        ok &= _observe(f"{tag}_{stage}", _relrms(dev, a), FLOOR_FACTOR * _relrms(c, a) + SLACK)
    return ok, logits, T2


# 1 ------------------------------------------------------------------------------------------------ features
def test_features_ragged():
    """Shape A, rows of 400 .. 48 000 samples in one batch, against the float64 front end over the valid frames; bounds as
    test_gpu_mel.py sets them: 4 x the distance of the reference's own float32 realisation."""
    cfg, m = _model("A")
    audios = _audio([400, 1599, 1600, 16000, 48000])
    got = m.features(audios)
    ok = True
    for b, a in enumerate(audios):
        want, f32 = R.front_end(a, 40), R.front_end(a, 40, np.float32)
        F = len(want)
        assert not got[b, F:].any()
        d, own = np.abs(got[b, :F] - want), np.abs(f32 - want)
        ok &= _observe(f"features_row{b}_max", d.max(), 4 * own.max())
        ok &= _observe(f"features_row{b}_rms", np.sqrt(np.mean(d ** 2)), 4 * np.sqrt(np.mean(own ** 2)))
    assert ok


# 2 ------------------------------------------------------------------------------------------------ stem and block taps
@pytest.mark.parametrize("name", ["A", "B"])
def test_stem_and_block_taps(name):
    """Ragged rows of 1.0 to 2.5 s in a batch of 5; one gate per stage over the valid frames of the five rows.  The pooling is on
    purpose: in shape B a single bf16 rounding that falls the other way moves a whole row's block output by 3.6e-3 - the reference's
    own float32- and float64-accumulation realisations differ by exactly that on some rows (0, 0, 6.2e-4, 1.2e-3, 3.6e-3, 3.7e-3 over
    six rows) and by nothing on others, so a floor measured on one row says little about the next.  Observed on an MI355X per row
    (recorded, not gated): shape B block 2.9e-5, 1.2e-3, 3.6e-3 with per-row floors of 2.9e-5, 3.8e-3, 0."""
    cfg, m = _model(name)
    ok, _, _ = _chain_gates(cfg, _weights(name), m, _audio([16000, 21111, 27040, 33333, 40000]), f"taps_{name}", per_row=False)
    assert ok


# 3 ------------------------------------------------------------------------------------------------ attention edges
def test_attention_edges():
    cfg, m = _model("A")
    lens = _lens_for_t2(m, [1, 31, 32, 33, 64, 65, 200])
    ok, _, T2 = _chain_gates(cfg, _weights("A"), m, _audio(lens, 7), "attn_edges")
    assert list(T2) == [1, 31, 32, 33, 64, 65, 200] and ok


# 4 ------------------------------------------------------------------------------------------------ depthwise edges
@pytest.mark.parametrize("name", ["A", "B"])
def test_depthwise_edges(name):
    cfg, m = _model(name)
    lens = _lens_for_t2(m, [1, 2, 15, 16, 17, 40])
    ok, _, T2 = _chain_gates(cfg, _weights(name), m, _audio(lens, 9), f"dw_edges_{name}")
    assert list(T2) == [1, 2, 15, 16, 17, 40] and ok


# 5 ------------------------------------------------------------------------------------------------ padding is inert
def test_padding_is_inert():
    cfg, m = _model("A")
    audios = _audio([9000, 16000, 12345, 30000], 11)
    runs = [(m.features(audios, junk=j), m.forward(audios, junk=j), m.generate_tokens(audios, junk=j)) for j in (0.0, np.nan, 1e30)]
    for f, l, t in runs[1:]:
        assert np.array_equal(f, runs[0][0]) and np.array_equal(l, runs[0][1]) and t == runs[0][2]
    _, T2 = m.frames([len(a) for a in audios])
    r64 = R.Ref(cfg, _weights("A"), round=True, acc=np.float64)
    rb = R.Ref(cfg, _weights("A"), round=True, acc=np.float32)
    ok = True
    for b, a in enumerate(audios):
        assert m.generate_tokens([a]) == [runs[0][2][b]]
        alone = m.forward([a])[0]
        f = m.features([a])[0]
        ref, floor = rb.forward(f)["logits"], r64.forward(f)["logits"]
        ok &= _observe(f"alone_row{b}_logits", _relrms(alone, ref), FLOOR_FACTOR * _relrms(floor, ref) + SLACK)
        _record(f"alone_row{b}_bits", equal=bool(np.array_equal(alone, runs[0][1][b, : T2[b]])))
    assert ok


# 6 ------------------------------------------------------------------------------------------------ decisions
@pytest.mark.parametrize("name", ["A", "B"])
def test_decisions(name):
    cfg, m = _model(name)
    W, blank = _weights(name), cfg["pad_token_id"]
    audios = _audio([16000, 17777, 20000, 23456, 26000, 29999, 32000, 35000], R.DECISION_SEED)
    feats, logits, toks = m.features(audios), m.forward(audios), m.generate_tokens(audios)
    F, T2 = m.frames([len(a) for a in audios])
    rb = R.Ref(cfg, W, round=True, acc=np.float32)
    exempt = frames = 0
    for b in range(len(audios)):
        ref = rb.forward(feats[b, : F[b]])["logits"]
        dev = logits[b, : T2[b]]
        err = rms(dev, ref)
        top2 = np.sort(ref, axis=-1)[:, -2:]
        sure = (top2[:, 1] - top2[:, 0]) >= 4 * err
        exempt += int((~sure).sum())
        frames += len(sure)
        assert np.array_equal(dev.argmax(-1)[sure], ref.argmax(-1)[sure])
        if sure.all():
            assert toks[b] == R.greedy_ctc(ref, blank)
        assert toks[b] == R.greedy_ctc(dev, blank)                 # the device's collapse of the device's own arg-max
        assert blank not in toks[b] and len(toks[b]) <= T2[b]
    _record(f"decisions_{name}", exempt=exempt, frames=frames)
    assert exempt <= 0.01 * frames
    # zero audio with a head bias favouring the blank: no token at all
    _, mb = _model(name, R.DECISION_SEED, 100.0)
    assert mb.generate_tokens([np.zeros(16000, np.float32), audios[1]]) == [[], []]


# 7 ------------------------------------------------------------------------------------------------ published widths
def test_published_widths():
    cfg, m = _model("P", R.DECISION_SEED, 0.0, 2, 10)
    W = _weights("P")
    audios = _audio([160000, 160000], 21)
    feats, logits = m.features(audios), m.forward(audios)
    L = cfg["encoder_config"]["num_hidden_layers"]
    enc = m.tap(L + 1)
    m.generate_tokens(audios)
    assert m.launches == 13 + 16 * L                               # 3 front end + 6 stem + 16 a block + 4 tail
    rb, r64 = R.Ref(cfg, W, round=True, acc=np.float32), R.Ref(cfg, W, round=True, acc=np.float64)
    a, c = rb.forward(feats[0]), r64.forward(feats[0])
    ok = _observe("published_out_norm", _relrms(enc[0], a["out_norm"]), FLOOR_FACTOR * _relrms(c["out_norm"], a["out_norm"]) + SLACK)
    ok &= _observe("published_logits", _relrms(logits[0], a["logits"]), FLOOR_FACTOR * _relrms(c["logits"], a["logits"]) + SLACK)
    assert ok


# 8 ------------------------------------------------------------------------------------------------ forward_features
def test_forward_features_matches_forward_bit_for_bit():
    cfg, m = _model("B")
    audios = _audio([16000, 30000, 22222], 13)
    feats, logits = m.features(audios), m.forward(audios)
    F, _ = m.frames([len(a) for a in audios])
    assert np.array_equal(m(feats, frames=F), logits)


# 9 ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_the_handle_usable():
    cfg, m = _model("A")
    ok_audio = _audio([16000], 1)
    want = m.generate_tokens(ok_audio)

    def fails(fn, text):
        with pytest.raises(mas.AudioGenerationError) as e:
            fn()
        assert text in str(e.value), str(e.value)
        assert m.generate_tokens(ok_audio) == want

    fails(lambda: m.forward([np.zeros(1000, np.float32)]), "too short for the conv stem")
    fails(lambda: m.forward([]), "non-empty")
    z = np.zeros((1, 16000), np.float32)
    lens = np.full(65, 16000, np.int64)
    out = np.zeros(4, np.float32)
    from mlx_audio_swift_amd import _lib
    from mlx_audio_swift_amd.generation import check
    fails(lambda: check(_lib.lib().mis_lasr_forward(m._h, z.ctypes.data, lens.ctypes.data, 0, 16000, out.ctypes.data)), "batch 0 outside")
    fails(lambda: check(_lib.lib().mis_lasr_forward(m._h, z.ctypes.data, lens.ctypes.data, 65, 16000, out.ctypes.data)), "batch 65 outside")
    fails(lambda: m.forward([np.zeros(13 * 16000, np.float32)]), "exceed the workspace of 12 seconds")

    def bad_config(text, **enc):
        c = R.case_config("A")
        c["encoder_config"].update(enc)
        fails(lambda: mas.LasrCTCModel(mas.LasrCTCConfig.from_dict(c)), text)

    bad_config("head size", num_attention_heads=4)                 # 128 / 4 = 32
    bad_config("rope_type", rope_type="linear")
    W = dict(_weights("A"))
    del W["encoder.layers.1.conv.pointwise_conv2.weight"]
    fails(lambda: mas.LasrCTCModel.from_weights(mas.LasrCTCConfig.from_dict(cfg), W),
          "LASR weight missing: encoder.layers.1.conv.pointwise_conv2.weight")


# 10 ----------------------------------------------------------------------------------------------- loader
def test_loader(tmp_path):
    import torch
    from safetensors.torch import save_file
    cfg, m = _model("A")
    W = _weights("A")
    sd = {}
    for k, v in W.items():
        t = torch.from_numpy(v)
        if "conv" in k and k.endswith(".weight") and t.ndim == 3:
            t = t.permute(0, 2, 1)                                  # PyTorch's [out, in, k]
        if k == "ctc_head.weight":
            t = t[:, :, None]
        sd[k] = t.contiguous()
    sd["encoder.rotary_emb.inv_freq"] = torch.ones(32)
    for i in range(cfg["encoder_config"]["num_hidden_layers"]):
        sd[f"encoder.layers.{i}.conv.norm.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    save_file(sd, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    pieces = ["<pad>"] + [f"▁w{i}" for i in range(1, cfg["vocab_size"])]
    (tmp_path / "tokenizer.json").write_text(json.dumps({"model": {"type": "Unigram", "vocab": [[p, 0.0] for p in pieces]},
                                                         "added_tokens": [{"id": 0, "content": "<pad>", "special": True}]}))
    loaded = mas.LasrCTCModel.from_model_directory(str(tmp_path), max_batch=2, max_seconds=4)
    audio = _audio([40000], 17)[0]
    toks = m.generate_tokens([audio])[0]
    out = loaded.generate(audio)
    assert toks and out.token_ids == [toks] and out.text == " ".join(f"w{t}" for t in toks)
    assert out.segments == [{"text": out.text, "start": 0.0, "end": 0.0}] and out.generation_tokens == len(toks)
    events = list(loaded.generate_stream(audio))
    assert [e[0] for e in events] == ["token", "result"] and events[0][1] == out.text
    (tmp_path / "extra.safetensors").write_bytes((tmp_path / "model.safetensors").read_bytes())
    save_file({"encoder.bogus.weight": torch.ones(2)}, str(tmp_path / "zz.safetensors"))
    with pytest.raises(mas.AudioGenerationError, match="unused keys"):
        mas.LasrCTCModel.from_model_directory(str(tmp_path))
    with pytest.raises(mas.AudioGenerationError, match="No safetensors files found"):
        os.makedirs(tmp_path / "empty")
        (tmp_path / "empty" / "config.json").write_text(json.dumps(cfg))
        mas.LasrCTCModel.from_model_directory(str(tmp_path / "empty"))
