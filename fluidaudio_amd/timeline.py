"""The diarizer timeline (csrc/timeline.hip, csrc/timeline_host.hip): DiarizerTimeline.rebuild (reference: Sources/FluidAudio/Diarizer/DiarizerTimeline.swift:945-1003,
1169-1336), batched over recordings.  The offline Sortformer diarizer (sortformer.py) ends in it, the streaming Sortformer and LS-EEND
diarizers call it as well, and der.py scores its records.

Predictions given as torch CUDA tensors are read on the device; only counts and records come back."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _args as A, _lib as L

SEGMENT_DTYPE = np.dtype(L.DiarizerSegmentRecord)


def _swift_round(x) -> int:
    """Int(round(x)) on a Float: half away from zero."""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


@dataclass
class DiarizerTimelineConfig:   # DiarizerTimelineConfig (:9-164)
    num_speakers: int = 1
    frame_duration_seconds: float = 0.08
    onset_threshold: float = 0.5
    offset_threshold: float = 0.5
    onset_pad_frames: int = 0
    offset_pad_frames: int = 0
    min_frames_on: int = 0
    min_frames_off: int = 0
    activity_type: str = "sigmoids"

    @classmethod
    def default(cls, num_speakers: int, frame_duration_seconds: float):
        return cls(num_speakers=num_speakers, frame_duration_seconds=frame_duration_seconds)

    @classmethod
    def sortformer_default(cls):
        return cls.default(4, 0.08)

    @classmethod
    def from_seconds(cls, num_speakers: int = 1, frame_duration_seconds: float = 0.08, onset_threshold: float = 0.5,
                     offset_threshold: float = 0.5, onset_pad_seconds: float = 0.0, offset_pad_seconds: float = 0.0,
                     min_duration_on: float = 0.0, min_duration_off: float = 0.0):
        """The seconds initialiser (:139-163): Int(round(x / frameDuration)) in fp32."""
        f = np.float32
        fd = f(frame_duration_seconds)
        return cls(num_speakers, frame_duration_seconds, onset_threshold, offset_threshold, _swift_round(f(f(onset_pad_seconds) / fd)),
                   _swift_round(f(f(offset_pad_seconds) / fd)), _swift_round(f(f(min_duration_on) / fd)), _swift_round(f(f(min_duration_off) / fd)))

    def c_config(self) -> L.TimelineConfig:
        c = L.TimelineConfig()
        L.lib().fa_timeline_default_config(C.byref(c))
        c.onset_threshold, c.offset_threshold = float(self.onset_threshold), float(self.offset_threshold)
        c.onset_pad_frames, c.offset_pad_frames = int(self.onset_pad_frames), int(self.offset_pad_frames)
        c.min_frames_on, c.min_frames_off = int(self.min_frames_on), int(self.min_frames_off)
        c.frame_duration, c.speakers = float(self.frame_duration_seconds), int(self.num_speakers)
        c.activity_type = {"sigmoids": 0, "logits": 1}[self.activity_type]
        return c


@dataclass
class DiarizerSegment:   # DiarizerSegment (:492-560)
    speaker_index: int
    start_frame: int
    end_frame: int
    is_finalized: bool
    frame_duration_seconds: float
    activity: float = 0.0

    @classmethod
    def from_times(cls, speaker_index: int, start_time: float, end_time: float, frame_duration_seconds: float, finalized: bool = True):
        f = np.float32
        fd = f(frame_duration_seconds)
        return cls(speaker_index, _swift_round(f(f(start_time) / fd)), _swift_round(f(f(end_time) / fd)), finalized, frame_duration_seconds)

    @property
    def length(self) -> int:
        return self.end_frame - self.start_frame

    @property
    def start_time(self) -> np.float32:
        return np.float32(np.float32(self.start_frame) * np.float32(self.frame_duration_seconds))

    @property
    def end_time(self) -> np.float32:
        return np.float32(np.float32(self.end_frame) * np.float32(self.frame_duration_seconds))

    @property
    def duration(self) -> np.float32:
        return np.float32(np.float32(self.end_frame - self.start_frame) * np.float32(self.frame_duration_seconds))

    @property
    def speaker_label(self) -> str:
        return f"Speaker {self.speaker_index}"


def _lengths(n_mel_frames) -> np.ndarray:
    return np.ascontiguousarray(np.atleast_1d(n_mel_frames), np.int64)


def timeline_segments(finalized, finalized_frames=None, tentative=None, tentative_frames=None, config: DiarizerTimelineConfig | None = None,
                      is_complete: bool = True, ctx: L.Context | None = None, capacity: int | None = None):
    """DiarizerTimeline.rebuild for a batch: finalized [sum finalized_frames, S] (torch CUDA tensor: read on the device; anything else:
    host entry), tentative likewise or None.  Returns (records: structured array of SEGMENT_DTYPE, recording_counts int64 [B]).
    capacity None: count, then fill; a number: one call that raises FluidAudioHipError(OUTPUT_TOO_SMALL) when it does not hold them."""
    config = config or DiarizerTimelineConfig.sortformer_default()
    ctx = ctx or L.default_context()
    s = config.num_speakers
    on_device = hasattr(finalized, "data_ptr") and finalized.is_cuda

    def placed(x):
        if x is None:
            return None, 0, None
        if on_device:
            import torch
            x = A.device_tensor(x, ctx, torch.float32)
            return x, x.numel() // s, x.data_ptr()
        x = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "data_ptr") else x, np.float32)
        return x, x.size // s, x.ctypes.data

    fin, nfin, pfin = placed(finalized)
    tent, ntent, ptent = placed(tentative)
    ff = _lengths(nfin if finalized_frames is None else finalized_frames)
    tf = None if tentative is None else _lengths(ntent if tentative_frames is None else tentative_frames)
    assert int(ff.sum()) == nfin and (tf is None or (tf.size == ff.size and int(tf.sum()) == ntent)), "frame counts do not match the predictions"
    cfg = config.c_config()
    f = L.lib().fa_timeline_segments_dev if on_device else L.lib().fa_timeline_segments
    name = "fa_timeline_segments_dev" if on_device else "fa_timeline_segments"
    cnt, per = C.c_int64(), np.zeros(ff.size, np.int64)

    def call(out, cap):
        with ctx.torch_ordered(on_device):
            return f(ctx.handle, C.byref(cfg), pfin, ff.ctypes.data, ptent, A.ptr(tf), ff.size, int(bool(is_complete)), A.ptr(out), cap, C.byref(cnt), per.ctypes.data)

    if capacity is None:
        ctx.check(call(None, 0), name)
        capacity = cnt.value
    out = np.zeros(max(int(capacity), 1), SEGMENT_DTYPE)
    ctx.check(call(out, int(capacity)), name)
    return out[:cnt.value], per


class DiarizerTimeline:
    """The part of DiarizerTimeline the device entry covers: rebuild from complete prediction matrices."""

    def __init__(self, config: DiarizerTimelineConfig | None = None, ctx: L.Context | None = None):
        self.config = config or DiarizerTimelineConfig.sortformer_default()
        self.ctx = ctx
        self.segments: list = []

    def rebuild(self, finalized_predictions, tentative_predictions=None, is_complete: bool = True) -> list:
        recs, _ = timeline_segments(finalized_predictions, None, tentative_predictions, None, self.config, is_complete, self.ctx)
        self.segments = _segments(recs, self.config.frame_duration_seconds)
        return self.segments


def _segments(recs, frame_duration) -> list:
    return [DiarizerSegment(int(r["speaker"]), int(r["start_frame"]), int(r["end_frame"]), bool(r["finalized"] & 1), frame_duration,
                            float(r["activity"])) for r in recs]
