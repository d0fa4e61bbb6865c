"""Offline Sortformer around its network (csrc/sortformer.hip, csrc/sortformer_host.hip): the window geometry, model inputs and
stitching of OfflineSortformerDiarizer.processComplete (reference: Sources/FluidAudio/Diarizer/Sortformer/Offline/
OfflineSortformerDiarizer.swift:98-119, 279-375; SortformerSpeakerStitcher.swift:27-77), batched over recordings.  The segments come from
the diarizer timeline (timeline.py).

Everything between the mel and the segment records stays on the device; only counts and records come back.  The network is the
caller's: any callable (d_windows [W, n_mels, windowMel], d_mel_length [W]) -> CUDA tensor [W, windowOut, speakers]."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _args as A, _lib as L
from .timeline import SEGMENT_DTYPE, DiarizerSegment, DiarizerTimeline, DiarizerTimelineConfig, _lengths, _segments, timeline_segments  # noqa: F401

WINDOW_DTYPE = np.dtype(L.SortformerWindow)


@dataclass
class OfflineSortformerConfig:   # OfflineSortformerConfig (:14-58)
    window_output_frames: int = 384
    subsampling_factor: int = 8
    num_speakers: int = 4
    mel_features: int = 128
    overlap_output_frames: int = 100
    sample_rate: int = 16000
    mel_stride: int = 160

    @property
    def window_mel_frames(self) -> int:
        return self.window_output_frames * self.subsampling_factor

    @property
    def frame_duration_seconds(self) -> np.float32:
        f = np.float32
        return f(f(f(self.subsampling_factor) * f(self.mel_stride)) / f(self.sample_rate))

    def c_config(self) -> L.SortformerOfflineConfig:
        return L.SortformerOfflineConfig(int(self.window_output_frames), int(self.subsampling_factor), int(self.num_speakers),
                                         int(self.mel_features), int(self.overlap_output_frames))


def offline_windows(n_mel_frames, config: OfflineSortformerConfig | None = None) -> dict:
    """The windows of :303-363 for a batch of mel lengths (host arithmetic): dict(windows = structured array of WINDOW_DTYPE,
    total_out int64 [B], window_range int64 [B + 1])."""
    cfg = (config or OfflineSortformerConfig()).c_config()
    n = _lengths(n_mel_frames)
    total, rng, cnt = np.zeros(n.size, np.int64), np.zeros(n.size + 1, np.int64), C.c_int64()
    f = L.lib().fa_sortformer_offline_windows
    st = f(C.byref(cfg), n.ctypes.data, n.size, None, 0, C.byref(cnt), total.ctypes.data, rng.ctypes.data)
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_sortformer_offline_windows")
    wins = np.zeros(cnt.value, WINDOW_DTYPE)
    st = f(C.byref(cfg), n.ctypes.data, n.size, wins.ctypes.data, wins.size, C.byref(cnt), None, None)
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_sortformer_offline_windows")
    return dict(windows=wins, total_out=total, window_range=rng)


def pack_windows(d_mel, n_mel_frames, layout: str = "mel_major", config: OfflineSortformerConfig | None = None, ctx: L.Context | None = None):
    """The model's inputs for every window of the batch.  d_mel: torch CUDA float32, [B, n_mels, T] (mel_major) or [B, T, n_mels]
    (frame_major), as a mel plan writes it; n_mel_frames [B].  Returns (d_windows [W, n_mels, windowMel], d_mel_length int32 [W])."""
    import torch
    config = config or OfflineSortformerConfig()
    ctx = ctx or L.default_context()
    d_mel = A.device_tensor(d_mel, ctx, torch.float32)
    if d_mel.dim() == 2:
        d_mel = d_mel.unsqueeze(0)
    n = _lengths(n_mel_frames)
    assert d_mel.dim() == 3 and d_mel.shape[0] == n.size, "mel must be [B, n_mels, T] or [B, T, n_mels]"
    mel_major = layout == "mel_major"
    assert d_mel.shape[1 if mel_major else 2] == config.mel_features, "mel feature count differs from the config's"
    frame_stride = int(d_mel.shape[2 if mel_major else 1])
    assert n.size == 0 or int(n.max()) <= frame_stride, "a recording is longer than the mel buffer"
    w = int(offline_windows(n, config)["window_range"][-1])
    d_out, d_len = A.beside(d_mel, (w, config.mel_features, config.window_mel_frames), "float32", torch_empty=True), A.beside(d_mel, w, "int32", torch_empty=True)
    cfg = config.c_config()
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_sortformer_pack_windows_dev(ctx.handle, C.byref(cfg), d_mel.data_ptr(),
                                                         L.MEL_LAYOUT_MEL_MAJOR if mel_major else L.MEL_LAYOUT_FRAME_MAJOR,
                                                         int(d_mel.shape[1] * d_mel.shape[2]), frame_stride, n.ctypes.data, n.size, w,
                                                         d_out.data_ptr(), d_len.data_ptr()), "fa_sortformer_pack_windows_dev")
    return d_out, d_len


def stitch(d_preds, n_mel_frames, config: OfflineSortformerConfig | None = None, ctx: L.Context | None = None):
    """The windows' predictions [W, windowOut, S] (torch CUDA) -> (d_global [sum total_out, S], d_mapping int32 [W, S]); recording b's
    timeline is rows total_out[:b].sum() onward."""
    import torch
    config = config or OfflineSortformerConfig()
    ctx = ctx or L.default_context()
    d_preds = A.device_tensor(d_preds, ctx, torch.float32)
    n = _lengths(n_mel_frames)
    geo = offline_windows(n, config)
    w, s = int(geo["window_range"][-1]), config.num_speakers
    assert tuple(d_preds.shape) == (w, config.window_output_frames, s), f"predictions must be [{w}, {config.window_output_frames}, {s}]"
    d_global, d_map = A.beside(d_preds, (int(geo["total_out"].sum()), s), "float32", torch_empty=True), A.beside(d_preds, (w, s), "int32", torch_empty=True)
    cfg = config.c_config()
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_sortformer_stitch_dev(ctx.handle, C.byref(cfg), d_preds.data_ptr(), n.ctypes.data, n.size, w, d_global.data_ptr(),
                                                   d_map.data_ptr()), "fa_sortformer_stitch_dev")
    return d_global, d_map


def stitcher_alignment(global_, window, frames: int, num_speakers: int) -> list:
    """SortformerSpeakerStitcher.alignment (:27-77) on host arrays: mapping[windowSpeaker] == globalSpeaker."""
    g = np.ascontiguousarray(global_, np.float32).reshape(-1)
    w = np.ascontiguousarray(window, np.float32).reshape(-1)
    if not (frames > 0 and num_speakers > 0 and g.size >= frames * num_speakers and w.size >= frames * num_speakers):
        return list(range(num_speakers))
    out = np.zeros(num_speakers, np.int32)
    st = L.lib().fa_sortformer_stitcher_alignment(g.ctypes.data, w.ctypes.data, int(frames), int(num_speakers), out.ctypes.data)
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_sortformer_stitcher_alignment")
    return out.tolist()


class OfflineSortformerDiarizer:
    """OfflineSortformerDiarizer.processComplete for one recording or a batch: mel -> pack -> model -> stitch -> segments."""

    def __init__(self, ctx: L.Context | None = None, config: OfflineSortformerConfig | None = None,
                 timeline_config: DiarizerTimelineConfig | None = None):
        from .mel import AudioMelSpectrogram
        self.ctx = ctx or L.default_context()
        self.config = config or OfflineSortformerConfig()
        self.timeline_config = timeline_config or DiarizerTimelineConfig.default(self.config.num_speakers, float(self.config.frame_duration_seconds))
        self.mel = AudioMelSpectrogram(ctx=self.ctx)
        self.last: dict = {}

    def process_complete(self, audio_or_batch, model) -> list:
        """audio_or_batch: one 1-D array of 16 kHz samples or a list of them (ragged); model: see the module docstring.  Returns, per
        recording, its [DiarizerSegment] (for a single array: that list itself).  self.last keeps the device tensors of the call
        (mel, n_mel_frames, windows, mel_length, preds, global, mapping) and the raw records."""
        import torch
        single = not isinstance(audio_or_batch, (list, tuple))
        audios = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in ([audio_or_batch] if single else audio_or_batch)]
        offs = np.concatenate([[0], np.cumsum([a.size for a in audios])]).astype(np.int64)
        results = [[] for _ in audios]
        if offs[-1] == 0:
            return results[0] if single else results
        dev = torch.device("cuda", self.ctx.device)
        plan = self.mel.plan(offs, layout="mel_major", padding_mode="center")
        try:
            d_pcm = torch.from_numpy(np.concatenate(audios)).to(dev)
            d_mel = torch.empty(plan.out_shape(), dtype=torch.float32, device=dev)
            plan.execute(d_pcm, d_mel)
            n_mel = np.array([max(int(L.lib().fa_mel_num_frames(C.byref(plan.cfg), a.size)), 0) if a.size else 0 for a in audios], np.int64)
            n_mel = np.minimum(n_mel, plan.frame_stride)
        finally:
            self.ctx.synchronize()
            plan.close()
        d_win, d_len = pack_windows(d_mel, n_mel, "mel_major", self.config, self.ctx)
        d_preds = model(d_win, d_len)
        d_global, d_map = stitch(d_preds, n_mel, self.config, self.ctx)
        total_out = offline_windows(n_mel, self.config)["total_out"]
        recs, _ = timeline_segments(d_global, total_out, None, None, self.timeline_config, True, self.ctx)
        self.last = dict(mel=d_mel, n_mel_frames=n_mel, windows=d_win, mel_length=d_len, preds=d_preds, global_=d_global, mapping=d_map,
                         total_out=total_out, records=recs)
        fd = self.timeline_config.frame_duration_seconds
        for b in range(len(audios)):
            results[b] = _segments(recs[recs["recording"] == b], fd)
        return results[0] if single else results
