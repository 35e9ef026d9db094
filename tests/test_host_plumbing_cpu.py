"""CPU: the host plumbing the model wrappers share (mlx-audio-swift_amd/_handle.py): pack_rows and read_safetensors_dir."""
import numpy as np
import pytest

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd._handle import pack_rows, read_safetensors_dir


def _rows():
    return [np.arange(5, dtype=np.float32), np.zeros(0, np.float32), np.arange(3, dtype=np.float32) + 10.0]


def test_pack_rows_pads_ragged_rows_with_zeros():
    pcm, lens = pack_rows(_rows())
    assert pcm.shape == (3, 5) and pcm.dtype == np.float32 and pcm.flags["C_CONTIGUOUS"]
    assert lens.dtype == np.int64 and lens.tolist() == [5, 0, 3]
    assert pcm[0].tolist() == [0, 1, 2, 3, 4] and pcm[1].tolist() == [0] * 5 and pcm[2].tolist() == [10, 11, 12, 0, 0]


def test_pack_rows_fills_the_padding_with_junk():
    pcm, lens = pack_rows(_rows(), junk=7.5)
    assert pcm.dtype == np.float32 and pcm.flags["C_CONTIGUOUS"] and lens.tolist() == [5, 0, 3]
    assert pcm[0].tolist() == [0, 1, 2, 3, 4] and pcm[1].tolist() == [7.5] * 5 and pcm[2].tolist() == [10, 11, 12, 7.5, 7.5]


def test_pack_rows_of_empty_rows_keeps_a_stride_of_one():
    pcm, lens = pack_rows([np.zeros(0, np.float32)] * 2)
    assert pcm.shape == (2, 1) and lens.tolist() == [0, 0] and not pcm.any()


def test_pack_rows_converts_to_float32():
    pcm, _ = pack_rows([np.arange(3, dtype=np.float64), [1, 2]])
    assert pcm.dtype == np.float32 and pcm[1].tolist() == [1, 2, 0]


def test_the_wrappers_keep_their_own_checks_and_shapes():
    """LASR rejects a row that is not one-dimensional with its own message; Moonshine flattens and returns the stride as well."""
    with pytest.raises(mas.AudioGenerationError, match="LASR: a non-empty list of one-dimensional waveforms is expected"):
        mas.LasrCTCModel._pack([np.zeros((2, 3), np.float32)])
    with pytest.raises(mas.AudioGenerationError, match="LASR: a non-empty list"):
        mas.LasrCTCModel._pack([])
    pcm, lens, stride = mas.MoonshineModel._pack([np.ones((2, 3), np.float32), np.ones(2, np.float32)], junk=-1.0)
    assert stride == 6 and pcm.shape == (2, 6) and lens.tolist() == [6, 2] and pcm[1].tolist() == [1, 1, -1, -1, -1, -1]
    pcm, lens, stride = mas.SmartTurnModel._pack([np.ones(4, np.float32)])
    assert stride == 4 and pcm.shape == (1, 4) and lens.tolist() == [4]


def _save(path, tensors):
    torch = pytest.importorskip("torch")
    st = pytest.importorskip("safetensors.torch")
    st.save_file({k: torch.tensor(v, dtype=torch.float32) for k, v in tensors.items()}, str(path))


def test_read_safetensors_dir_reads_in_name_order_and_later_files_win(tmp_path):
    _save(tmp_path / "b.safetensors", {"x": [2.0], "only_b": [5.0]})
    _save(tmp_path / "a.safetensors", {"x": [1.0], "only_a": [4.0]})
    (tmp_path / "notes.txt").write_text("not a checkpoint")
    seen = []
    w = read_safetensors_dir(str(tmp_path), missing_code=(1, "none"), on_keys=lambda fn, keys: seen.append((fn, sorted(keys))))
    assert sorted(w) == ["only_a", "only_b", "x"] and w["x"].tolist() == [2.0] and w["only_a"].tolist() == [4.0]
    assert seen == [("a.safetensors", ["only_a", "x"]), ("b.safetensors", ["only_b", "x"])]


@pytest.mark.parametrize("code", [1, 2])
def test_read_safetensors_dir_without_files_raises_the_callers_code(tmp_path, code):
    """Moonshine and Smart Turn raise modelNotInitialized (1), LASR 2, each with its own text."""
    with pytest.raises(mas.AudioGenerationError) as e:
        read_safetensors_dir(str(tmp_path), missing_code=(code, f"No safetensors files found in {tmp_path}"))
    assert e.value.status == code and f"No safetensors files found in {tmp_path}" in str(e.value)


def test_read_safetensors_dir_without_files_raises_the_callers_exception(tmp_path):
    """The language-identification loader raises its own error type."""
    with pytest.raises(mas.LIDError) as e:
        read_safetensors_dir(str(tmp_path), missing_code=mas.LIDError("weightsNotFound", "No .safetensors files found in model directory"))
    assert e.value.lid_case == "weightsNotFound" and "No .safetensors files found in model directory" in str(e.value)


def test_the_loaders_report_a_directory_without_weights_as_before(tmp_path):
    (tmp_path / "config.json").write_text("{}")
    with pytest.raises(mas.AudioGenerationError, match="No safetensors files found in") as e:
        mas.smart_turn_read_directory(str(tmp_path))
    assert e.value.status == 1
    (tmp_path / "config.json").write_text('{"id2label": {"0": "en: English"}}')
    with pytest.raises(mas.LIDError, match="No .safetensors files found in model directory") as e:
        mas.ecapa_lid_read_directory(str(tmp_path))
    assert e.value.lid_case == "weightsNotFound"


def test_on_keys_fires_before_any_tensor_is_read(tmp_path, monkeypatch):
    """A loader rejects a quantised checkpoint from the key list alone: no tensor of that file has been read by then."""
    safetensors = pytest.importorskip("safetensors")
    _save(tmp_path / "model.safetensors", {"w.weight": [1.0], "w.scales": [1.0]})
    reads = []
    real_open = safetensors.safe_open

    class Spy:
        def __init__(self, *a, **k):
            self._f = real_open(*a, **k)

        def __enter__(self):
            self._h = self._f.__enter__()
            return self

        def __exit__(self, *a):
            return self._f.__exit__(*a)

        def keys(self):
            return self._h.keys()

        def get_tensor(self, k):
            reads.append(k)
            return self._h.get_tensor(k)

    monkeypatch.setattr(safetensors, "safe_open", Spy)

    def no_quant(fn, keys):
        assert reads == []
        if any(k.endswith(".scales") for k in keys):
            raise mas.AudioGenerationError(3, f"{fn}: quantised")

    with pytest.raises(mas.AudioGenerationError, match="model.safetensors: quantised"):
        read_safetensors_dir(str(tmp_path), missing_code=(1, "none"), on_keys=no_quant)
    assert reads == []
    (tmp_path / "config.json").write_text("{}")
    with pytest.raises(mas.AudioGenerationError, match="MLX-quantised Smart Turn checkpoints are not supported") as e:
        mas.smart_turn_read_directory(str(tmp_path))
    assert e.value.status == 3 and reads == []
