"""Kaldi fbank -> LFR -> CMVN, the front end FunASR's ``WavFrontend`` puts before Paraformer, SenseVoice, FSMN-VAD and CAM++ (the
reference runs a CoreML replica of it: Documentation/ASR/SenseVoice.md:27,107-114), for a batch of utterances in one launch of
fluidaudio_amd/csrc/fbank.hip.  include/fluidaudio_hip.h, section "Kaldi fbank", states the arithmetic.

Host arrays in, host arrays out (the host-pointer entry, one synchronisation).  Plans on device-resident audio are served by the C ABI
and the C++ mirror (``fluidaudio::FbankPlan``); this module has no device-tensor form yet.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args as A
from . import _lib as L

WINDOWS = {"hamming": L.FBANK_WINDOW_HAMMING, "povey": L.FBANK_WINDOW_POVEY}
TAILS = {"replicate": L.FBANK_TAIL_REPLICATE, "valid": L.FBANK_TAIL_VALID}


def fbank_config(window=None, filterbank=None, **fields) -> L.FbankConfig:
    """fa_fbank_default_config (WavFrontend: 80 mels, Hamming, LFR 7 / 6, replicated tail) with `fields` set over it; `window_type`
    and `tail_mode` also take their names.  `window` [win] / `filterbank` [n_mels, n_fft/2 + 1] replace the built-in tables: the
    record keeps the arrays alive."""
    cfg = L.FbankConfig()
    L.lib().fa_fbank_default_config(C.byref(cfg))
    for name, value in fields.items():
        if not hasattr(cfg, name):
            raise A.invalid("fbank_config", f"no field {name}")
        setattr(cfg, name, {"window_type": WINDOWS, "tail_mode": TAILS}.get(name, {}).get(value, value))
    cfg._tables = []
    for name, table, size in (("window", window, cfg.win), ("filterbank", filterbank, cfg.n_mels * (cfg.n_fft // 2 + 1))):
        if table is not None:
            table = np.ascontiguousarray(table, np.float32).reshape(-1)
            if table.size != size:
                raise A.invalid("fbank_config", f"{name} holds {table.size} values, not {size}")
            cfg._tables.append(table)
            setattr(cfg, name, table.ctypes.data)
    return cfg


def fbank_num_frames(cfg: L.FbankConfig, n_samples: int) -> int:
    return int(L.lib().fa_fbank_num_frames(C.byref(cfg), int(n_samples)))


def fbank_num_rows(cfg: L.FbankConfig, frames: int) -> int:
    return int(L.lib().fa_fbank_num_rows(C.byref(cfg), int(frames)))


def fbank_window(cfg: L.FbankConfig) -> np.ndarray:
    out = np.zeros(cfg.win, np.float32)
    st = L.lib().fa_fbank_window(C.byref(cfg), out.ctypes.data)
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_fbank_window")
    return out


def fbank_filterbank(cfg: L.FbankConfig) -> np.ndarray:
    out = np.zeros((cfg.n_mels, cfg.n_fft // 2 + 1), np.float32)
    st = L.lib().fa_fbank_filterbank(C.byref(cfg), out.ctypes.data)
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_fbank_filterbank")
    return out


def fbank_batch(waves, offsets=None, cfg: L.FbankConfig | None = None, shift=None, scale=None, row_stride: int = 0, ctx: L.Context | None = None):
    """Features of a batch: `waves` a list of float arrays in [-1, 1) (or one flat array with its batch + 1 `offsets`); `shift` / `scale`
    the CMVN vectors [lfr_m * n_mels] or None.  Returns (features float32 [B, row_stride, lfr_m * n_mels] with the rows behind an
    utterance's own zero, rows int32 [B]); row_stride 0 takes the longest utterance's row count."""
    cfg = cfg or fbank_config()
    ctx = ctx or L.default_context()
    pcm, offsets = A.ragged(waves, offsets, np.float32, "fbank_batch", "offsets: one-dimensional, batch + 1 entries")
    batch = offsets.size - 1
    if batch < 1:
        raise A.invalid("fbank_batch", "empty batch")
    width = cfg.lfr_m * cfg.n_mels
    vectors = []
    for name, v in (("shift", shift), ("scale", scale)):
        v = None if v is None else np.ascontiguousarray(v, np.float32).reshape(-1)
        if v is not None and v.size != width:
            raise A.invalid("fbank_batch", f"{name} holds {v.size} values, not {width}")
        vectors.append(v)
    if row_stride <= 0:
        row_stride = max(1, max(fbank_num_rows(cfg, fbank_num_frames(cfg, n)) for n in np.diff(offsets)))
    out = np.zeros((batch, row_stride, width), np.float32)
    rows = np.zeros(batch, np.int32)
    ctx.check(L.lib().fa_fbank_batch(ctx.handle, C.byref(cfg), A.ptr(pcm), A.ptr(offsets), batch, A.ptr(vectors[0]), A.ptr(vectors[1]), row_stride,
                                     A.ptr(out), A.ptr(rows)), "fa_fbank_batch")
    return out, rows


class WavFrontend:
    """FunASR's ``WavFrontend`` for a batch: a configuration and the model's CMVN vectors (``AddShift`` / ``Rescale`` of am.mvn), called
    with the utterances."""

    def __init__(self, shift=None, scale=None, cfg: L.FbankConfig | None = None, ctx: L.Context | None = None):
        self.cfg, self.shift, self.scale, self.ctx = cfg or fbank_config(), shift, scale, ctx

    def __call__(self, waves, offsets=None, row_stride: int = 0):
        return fbank_batch(waves, offsets, self.cfg, self.shift, self.scale, row_stride, self.ctx)
