"""Host plumbing the model wrappers share: the handle of a C engine (set_tensor / finalize / close), the packing of a ragged list of
waveforms, and the reading of a directory of *.safetensors.  No arithmetic happens here."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .generation import AudioGenerationError, check

_NP_DTYPES = {np.dtype(np.float32): _lib.MIS_F32, np.dtype(np.float16): _lib.MIS_F16}


def _tensor_args(arr):
    """numpy / torch tensor -> (keepalive, data pointer, mis dtype, shape)."""
    try:
        import torch
        if isinstance(arr, torch.Tensor):
            t = arr.detach().contiguous()
            if t.dtype == torch.bfloat16:
                return t, t.data_ptr(), _lib.MIS_BF16, tuple(t.shape)
            if t.dtype == torch.float16:
                return t, t.data_ptr(), _lib.MIS_F16, tuple(t.shape)
            t = t.to(torch.float32).contiguous()
            return t, t.data_ptr(), _lib.MIS_F32, tuple(t.shape)
    except ImportError:
        pass
    a = np.ascontiguousarray(arr)
    if a.dtype not in _NP_DTYPES:
        a = a.astype(np.float32)
    return a, a.ctypes.data, _NP_DTYPES[a.dtype], a.shape


class NativeHandle:
    """Owns `_h`, a handle of the C family `_prefix`: <prefix>_create / _set_tensor / _set_tensor_quantized / _finalize / _destroy.
    A subclass sets `_prefix` ("mis_lasr", ...) and calls `_create` from its __init__."""
    _prefix = ""
    _h = None

    def _fn(self, suffix: str):
        return getattr(_lib.lib(), f"{self._prefix}_{suffix}")

    def _create(self, cfg_c, *args):
        """<prefix>_create(&cfg_c, *args, &handle)."""
        h = C.c_void_p()
        check(self._fn("create")(C.byref(cfg_c), *args, C.byref(h)))
        self._h = h

    def set_tensor(self, name: str, arr):
        keep, ptr, dt, shape = _tensor_args(arr)
        sh = (C.c_int64 * len(shape))(*shape)
        check(self._fn("set_tensor")(self._h, name.encode(), ptr, dt, sh, len(shape)))

    def set_quantized_tensor(self, name: str, wq, scales, biases, group_size: int = 64, bits: int = 4):
        """A Linear / Embedding in MLX's affine-quantised form (`name` = its .weight key): wq uint32 [N, K*bits/32], scales / biases
        [N, K/group_size] (bf16 / f16 / f32).  Only the engines that export <prefix>_set_tensor_quantized take it."""
        wq = np.ascontiguousarray(wq, dtype=np.uint32)
        ks, ps, ds, ss = _tensor_args(scales)
        kb, pb, db, sb = _tensor_args(biases)
        if ds != db or tuple(ss) != tuple(sb) or len(ss) != 2:
            raise AudioGenerationError(3, "scales and biases must be 2-D and share dtype and shape")
        N, K = int(ss[0]), int(ss[1]) * group_size
        check(self._fn("set_tensor_quantized")(self._h, name.encode(), wq.ctypes.data, ps, pb, ds, N, K, group_size, bits))

    def finalize(self):
        check(self._fn("finalize")(self._h))

    def close(self):
        """Release the handle now (otherwise at garbage collection); a second call does nothing."""
        h, self._h = self._h, None
        if h:
            self._fn("destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:                                                # interpreter shutdown
            pass


def pack_rows(rows, junk=None):
    """Ragged list of 1-D float32 arrays -> (pcm f32 [B, stride] C-contiguous, lens int64 [B]); stride = the longest row, at least 1.
    The padding behind a row is zero, or `junk` (tests: an engine must never read it)."""
    stride = max(1, max(len(r) for r in rows))
    pcm = np.zeros((len(rows), stride), np.float32) if junk is None else np.full((len(rows), stride), junk, np.float32)
    lens = np.zeros(len(rows), np.int64)
    for i, r in enumerate(rows):
        pcm[i, : len(r)] = r
        lens[i] = len(r)
    return pcm, lens


def read_safetensors_dir(model_dir: str, *, missing_code, on_keys=None) -> dict:
    """Every *.safetensors of a directory in name order, later files winning -> name -> torch tensor.  Without such a file:
    `missing_code` is raised if it is an exception, else AudioGenerationError(*missing_code) ((code, message)).  on_keys(file name,
    keys) is called for each file before any of its tensors is read (a loader rejects a quantised checkpoint there)."""
    files = sorted(fn for fn in os.listdir(model_dir) if fn.endswith(".safetensors"))
    if not files:
        raise missing_code if isinstance(missing_code, Exception) else AudioGenerationError(*missing_code)
    from safetensors import safe_open
    weights = {}
    for fn in files:
        with safe_open(os.path.join(model_dir, fn), framework="pt") as sf:
            keys = list(sf.keys())
            if on_keys is not None:
                on_keys(fn, keys)
            for k in keys:
                weights[k] = sf.get_tensor(k)
    return weights
