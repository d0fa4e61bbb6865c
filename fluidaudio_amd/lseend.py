"""The LS-EEND front end (Diarizer/LS-EEND/LSEENDPreprocessor.swift:249-279,185-202,158-180; LSEENDInference.swift:87-123): log10-mel,
cumulative mean normalisation, the overlapping [mel_frames, n_mels] windows the network reads with each window's decoder mask and
warm-up count, and the copy that strips the warm-up rows from the network's output — batched over recordings or streams, three launches
of fluidaudio_amd/csrc/lseend.hip per call.  include/fluidaudio_hip.h, section "LS-EEND front end", states the arithmetic and where it
differs from the reference (the mean is a fp64 sum divided by the count, not the fp32 recurrence).

Host arrays in, host arrays out (the host-pointer entries, one synchronisation each).  The device-pointer entries are served by the C ABI
and the C++ mirror (``fluidaudio::LseendStream``); this module has no device-tensor form yet.  The network and the resampler stay the
caller's.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _args as A
from . import _lib as L


class LseendFeatures(NamedTuple):
    """One call's output, the items (recordings or streams) one behind another; plans[i] says which rows are item i's."""
    windows: np.ndarray     # float32 [W, mel_frames, n_mels]
    masks: np.ndarray       # float32 [W, chunk_size]
    warmups: np.ndarray     # int32 [W]
    out_rows: np.ndarray    # int64 [W]: first row of the window's kept rows in the dense probabilities
    raw: np.ndarray         # float32 [F, n_mels]: the log10-mel rows before the normalisation
    plans: list             # LseendItemPlan per item


def lseend_config(**fields) -> L.LseendConfig:
    """fa_lseend_default_config (EEND's 8 kHz front end: win 200, hop 80, 23 mels, context 7, subsampling 10, conv delay 9) with
    `fields` set over it."""
    cfg = L.LseendConfig()
    L.lib().fa_lseend_default_config(C.byref(cfg))
    for name, value in fields.items():
        if not hasattr(cfg, name):
            raise A.invalid("lseend_config", f"no field {name}")
        setattr(cfg, name, value)
    return cfg


def lseend_mel_frames(cfg: L.LseendConfig) -> int:
    return int(L.lib().fa_lseend_mel_frames(C.byref(cfg)))


def _check(status: int, where: str):
    if status != L.SUCCESS:
        raise L.FluidAudioHipError(status, where)


def lseend_plan_file(lengths, cfg: L.LseendConfig | None = None):
    """What the offline call does to recordings of these sample counts, without a device: (plans, warmups int32 [W], masks float32
    [W, chunk_size])."""
    cfg = cfg or lseend_config()
    offsets = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)
    batch = offsets.size - 1
    if batch < 1:
        raise A.invalid("lseend_plan_file", "empty batch")
    plans = (L.LseendItemPlan * batch)()
    _check(L.lib().fa_lseend_plan_file(C.byref(cfg), A.ptr(offsets), batch, plans, None, None, 0), "fa_lseend_plan_file")
    W = int(plans[-1].window0 + plans[-1].windows)
    warmups, masks = np.zeros(W, np.int32), np.zeros((W, cfg.chunk_size), np.float32)
    _check(L.lib().fa_lseend_plan_file(C.byref(cfg), A.ptr(offsets), batch, plans, A.ptr(warmups), A.ptr(masks), W), "fa_lseend_plan_file")
    return list(plans), warmups, masks


def lseend_plan_push(state: L.LseendStreamInfo, samples: int, flush: bool = False, cfg: L.LseendConfig | None = None):
    """One push on one stream, without a device: advances `state` (a zero LseendStreamInfo is a fresh stream) and returns (plan, warmups,
    masks) of the windows the push emits."""
    cfg = cfg or lseend_config()
    probe, plan = L.LseendStreamInfo.from_buffer_copy(state), L.LseendItemPlan()
    _check(L.lib().fa_lseend_plan_push(C.byref(cfg), C.byref(probe), int(samples), int(flush), C.byref(plan), None, None, 0), "fa_lseend_plan_push")
    W = int(plan.windows)
    warmups, masks = np.zeros(W, np.int32), np.zeros((W, cfg.chunk_size), np.float32)
    _check(L.lib().fa_lseend_plan_push(C.byref(cfg), C.byref(state), int(samples), int(flush), C.byref(plan), A.ptr(warmups), A.ptr(masks), W), "fa_lseend_plan_push")
    return plan, warmups, masks


def _outputs(cfg, W: int, F: int):
    mf = lseend_mel_frames(cfg)
    return (np.zeros((W, mf, cfg.n_mels), np.float32), np.zeros((W, cfg.chunk_size), np.float32), np.zeros(W, np.int32), np.zeros(W, np.int64),
            np.zeros((F, cfg.n_mels), np.float32))


def lseend_features(waves, offsets=None, cfg: L.LseendConfig | None = None, ctx: L.Context | None = None) -> LseendFeatures:
    """Every window of every recording in one call: `waves` a list of float arrays at the model's rate (or one flat array with its batch + 1
    `offsets`), each pushed whole and flushed as processComplete does."""
    cfg = cfg or lseend_config()
    ctx = ctx or L.default_context()
    pcm, offsets = A.ragged(waves, offsets, np.float32, "lseend_features", "offsets: one-dimensional, batch + 1 entries")
    plans, _, _ = lseend_plan_file(np.diff(offsets), cfg)
    W, F = int(plans[-1].window0 + plans[-1].windows), int(plans[-1].frame0 + plans[-1].frames)
    windows, masks, warmups, out_rows, raw = _outputs(cfg, W, F)
    ctx.check(L.lib().fa_lseend_features(ctx.handle, C.byref(cfg), A.ptr(pcm), A.ptr(offsets), offsets.size - 1, A.ptr(windows), A.ptr(masks), A.ptr(warmups),
                                         A.ptr(out_rows), A.ptr(raw)), "fa_lseend_features")
    return LseendFeatures(windows, masks, warmups, out_rows, raw, plans)


def lseend_gather_probs(probs, warmups, out_rows, speakers: int, total_rows: int, ctx: L.Context | None = None) -> np.ndarray:
    """predict's copy for all windows of a call: `probs` float32 [W, chunk_size, >= speakers] as the network left it (any window and row
    strides, last axis dense), `warmups` / `out_rows` from the call that made the windows -> dense float32 [total_rows, speakers]."""
    ctx = ctx or L.default_context()
    probs = np.asarray(probs)
    if probs.dtype != np.float32 or probs.ndim != 3 or probs.shape[2] < speakers or (probs.size and probs.strides[2] != 4) or any(s % 4 or s < 0 for s in probs.strides[:2]):
        raise A.invalid("lseend_gather_probs", "probs: float32 [windows, chunk_size, >= speakers] with a dense last axis")
    W, chunk = probs.shape[:2]
    warmups, out_rows = np.ascontiguousarray(warmups, np.int32), np.ascontiguousarray(out_rows, np.int64)
    if warmups.shape != (W,) or out_rows.shape != (W,):
        raise A.invalid("lseend_gather_probs", "warmups / out_rows: one entry per window")
    out = np.zeros((total_rows, speakers), np.float32)
    if W == 0:
        return out
    row_stride = probs.strides[1] // 4 if chunk > 1 else probs.shape[2]
    window_stride = probs.strides[0] // 4 if W > 1 else (chunk - 1) * row_stride + speakers
    # the entry takes the span the strides cover, from the first element to the last one of the view
    span = (W - 1) * window_stride + (chunk - 1) * row_stride + speakers
    flat = np.ascontiguousarray(np.lib.stride_tricks.as_strided(probs, (span,), (4,)))
    ctx.check(L.lib().fa_lseend_gather_probs(ctx.handle, A.ptr(flat), W, chunk, speakers, window_stride, row_stride, A.ptr(warmups), A.ptr(out_rows), A.ptr(out),
                                             total_rows), "fa_lseend_gather_probs")
    return out


class LseendStream:
    """`streams` LS-EEND feature streams whose unread audio, unread normalised rows and running sums stay on the device: push() is
    enqueueAudio / drainRightContextWithSilence followed by every emitNextChunk that succeeds, for all streams at once; snapshot() and
    rollback() are takeSnapshot / rollback without the network's own state."""

    def __init__(self, streams: int = 1, max_push_samples: int = 80000, cfg: L.LseendConfig | None = None, ctx: L.Context | None = None):
        self.cfg, self.ctx, self.streams = cfg or lseend_config(), ctx or L.default_context(), int(streams)
        self._h = C.c_void_p()
        self.ctx.check(L.lib().fa_lseend_stream_create(self.ctx.handle, C.byref(self.cfg), self.streams, int(max_push_samples), C.byref(self._h)), "fa_lseend_stream_create")
        # the most one push can emit and compute, from the plan of a fresh stream given the largest push and a flush
        probe = L.LseendStreamInfo()
        plan, _, _ = lseend_plan_push(probe, int(max_push_samples), True, self.cfg)
        self._max_windows = (int(plan.windows) + 2) * self.streams
        self._max_frames = (int(plan.frames) + 2 * self.cfg.subsampling * self.cfg.chunk_size) * self.streams

    def close(self):
        if self._h:
            L.lib().fa_lseend_stream_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def reset(self, stream: int = -1):
        self.ctx.check(L.lib().fa_lseend_stream_reset(self.ctx.handle, self._h, int(stream)), "fa_lseend_stream_reset")

    def push(self, waves, flush=False) -> LseendFeatures:
        """`waves`: one float array per stream (empty for a stream with nothing new); `flush`: one flag for all streams or one per stream."""
        if len(waves) != self.streams:
            raise A.invalid("LseendStream.push", f"{len(waves)} arrays for {self.streams} streams")
        pcm, offsets = A.ragged(waves, None, np.float32)
        flags = np.ascontiguousarray(np.broadcast_to(np.asarray(flush, np.int32), (self.streams,)))
        windows, masks, warmups, out_rows, raw = _outputs(self.cfg, self._max_windows, self._max_frames)
        plans = (L.LseendItemPlan * self.streams)()
        self.ctx.check(L.lib().fa_lseend_stream_push(self.ctx.handle, self._h, A.ptr(pcm), A.ptr(offsets), A.ptr(flags), self._max_windows, A.ptr(windows), A.ptr(masks),
                                                     A.ptr(warmups), A.ptr(out_rows), A.ptr(raw), self._max_frames, plans), "fa_lseend_stream_push")
        W, F = int(plans[-1].window0 + plans[-1].windows), int(plans[-1].frame0 + plans[-1].frames)
        return LseendFeatures(windows[:W], masks[:W], warmups[:W], out_rows[:W], raw[:F], list(plans))

    def snapshot(self, stream: int = 0):
        """(info, audio tail, mel tail [rows, n_mels], per-mel float64 sums) of one stream, host data"""
        info = L.LseendStreamInfo()
        self.ctx.check(L.lib().fa_lseend_stream_get(self.ctx.handle, self._h, int(stream), C.byref(info), None, None, None), "fa_lseend_stream_get")
        audio, mel, sums = np.zeros(info.unread_audio, np.float32), np.zeros((info.unread_mel_rows, self.cfg.n_mels), np.float32), np.zeros(self.cfg.n_mels, np.float64)
        self.ctx.check(L.lib().fa_lseend_stream_get(self.ctx.handle, self._h, int(stream), C.byref(info), A.ptr(audio), A.ptr(mel), A.ptr(sums)), "fa_lseend_stream_get")
        return info, audio, mel, sums

    def rollback(self, snapshot, stream: int = 0):
        info, audio, mel, sums = snapshot
        audio, mel, sums = np.ascontiguousarray(audio, np.float32), np.ascontiguousarray(mel, np.float32), np.ascontiguousarray(sums, np.float64)
        if audio.size != info.unread_audio or mel.size != info.unread_mel_rows * self.cfg.n_mels or sums.size != self.cfg.n_mels:
            raise A.invalid("LseendStream.rollback", "the arrays do not have the sizes the info names")
        self.ctx.check(L.lib().fa_lseend_stream_set(self.ctx.handle, self._h, int(stream), C.byref(info), A.ptr(audio), A.ptr(mel), A.ptr(sums)), "fa_lseend_stream_set")
