"""Planning the windows of a long recording for Parakeet-TDT on the device (csrc/tdt_plan.hip), batched over recordings: what the
reference's ChunkProcessor decides from the audio before any network runs (Sources/FluidAudio/ASR/Parakeet/SlidingWindow/TDT/
ChunkProcessor.swift) — speechEndSamples :112-128, the chunk starts :163-396 (regular, or pulled towards a nearby silence or an energy
valley), the window loop of process :501-636 with lastChunkWarmupSamples :85-102, the preprocessor's 240 000-sample rows, and the
speech-energy gate of the seam-gap repair (:1245-1276, :1518-1534).  Integers, fp32 and fp64 results are the reference's bit for bit.
OUT OF SCOPE: the networks, the arbitration between the decodes, finding the seam gaps from the tokens, the re-decoding and
collapseSeamWordDuplicates."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _args as A, _lib as L

TDT_WINDOW_DTYPE, TDT_SPAN_DTYPE = np.dtype(L.TdtWindowRecord), np.dtype(L.TdtSpanRecord)
FIVE = ("audio_frames", "t0", "is_last", "global_offset", "emit_after")   # the walk's per-window operands, in the order the entries take them


def window_config(melChunkContext: bool = True, silenceAligned: bool = False, warmupPrefixFrames: int = 0, endAligned: bool = True,
                  overlapSeconds: float = 2.0, sampleRate: int = 16000, frameSamples: int = 1280, melHop: int = 160,
                  maxModelSamples: int = 240000) -> L.TdtWindowConfig:
    """The default path is window_config(); v3 no-mel and arbitration path A: (False, True); path B: (False, True, 7); path C: (False,)."""
    cfg = L.TdtWindowConfig()
    L.lib().fa_tdt_window_default_config(C.byref(cfg))
    cfg.sample_rate, cfg.frame_samples, cfg.mel_hop, cfg.max_model_samples, cfg.overlap_seconds = sampleRate, frameSamples, melHop, maxModelSamples, overlapSeconds
    cfg.mel_chunk_context, cfg.silence_aligned, cfg.warmup_prefix_frames, cfg.end_aligned = int(melChunkContext), int(silenceAligned), int(warmupPrefixFrames), int(endAligned)
    return cfg


def window_layout(config: L.TdtWindowConfig | None = None):
    """chunkLayout: (chunkSamples, strideSamples, melContextSamples, warmupPrefixSamples)."""
    out = [C.c_int64() for _ in range(4)]
    st = L.lib().fa_tdt_window_layout(A.cfg_ref(config), *[C.byref(x) for x in out])
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_tdt_window_layout", "the geometry is refused")
    return tuple(x.value for x in out)


def window_count_bound(samples: int, config: L.TdtWindowConfig | None = None) -> int:
    return int(L.lib().fa_tdt_window_count_bound(A.cfg_ref(config), int(samples)))


@dataclasses.dataclass
class PlannedWindows:
    windows: np.ndarray          # TDT_WINDOW_DTYPE, by recording and in a recording's order
    window_range: np.ndarray     # int64[B + 1]: what merge_windows takes
    speech_end: np.ndarray       # int64[B]
    statuses: np.ndarray         # int32[B]: INVALID_ARGUMENT for a recording with a non-finite energy (it has no windows)
    audio_frames: object         # the five per-window operands of the greedy walk: int32 numpy arrays, or torch tensors on the device
    t0: object
    is_last: object
    global_offset: object
    emit_after: object


def _windows_arg(windows, where):
    w = np.ascontiguousarray(windows, TDT_WINDOW_DTYPE)
    if w.ndim != 1:
        raise A.invalid(where, "windows is a one-dimensional array of TDT_WINDOW_DTYPE")
    return w


def _host_audio(audio, audio_offsets, where, windows=None):
    """The audio of a host entry, with the windows where the entry takes some: what the shared bodies below are handed."""
    audio, offsets = A.ragged(audio, audio_offsets, np.float32, where, "audio_offsets holds batch + 1 offsets")
    w = None if windows is None else _windows_arg(windows, where)
    if audio.ndim != 1 or offsets[-1] > audio.size:
        raise A.invalid(where, "audio is one-dimensional and covers audio_offsets")
    return audio, offsets, w


def _dev_audio(audio, audio_offsets, where, windows=None):
    if not A.is_dev(audio, "float32", 1):
        raise A.invalid(where, "audio is a contiguous one-dimensional float32 tensor on the device")
    _, offsets = A.ragged(audio, audio_offsets, np.float32, where, "audio_offsets holds batch + 1 offsets")
    w = None if windows is None else _windows_arg(windows, where)
    if offsets[-1] > audio.numel():
        raise A.invalid(where, "audio_offsets end beyond the samples")
    return audio, offsets, w


def _run_plan(where, ctx, audio, offsets, config, capacity, ordered) -> PlannedWindows:
    """The body of plan_windows and plan_windows_dev: the five operands are numpy arrays beside host audio, torch tensors beside a device tensor."""
    B = offsets.size - 1
    cap = int(sum(max(0, window_count_bound(int(n), config)) for n in np.diff(offsets))) if capacity is None else int(capacity)
    windows, window_range = np.zeros(cap, TDT_WINDOW_DTYPE), np.zeros(B + 1, np.int64)
    five = [A.beside(audio, cap, "int32") for _ in FIVE]
    speech_end, statuses = np.zeros(B, np.int64), np.zeros(B, np.int32)
    if B:
        ctx = A.context_beside(ctx, audio)
        with ctx.torch_ordered(ordered):
            ctx.check(getattr(L.lib(), where)(ctx.handle, A.cfg_ref(config), A.ptr(audio), offsets.ctypes.data, B, windows.ctypes.data if cap else None, cap,
                                              window_range.ctypes.data, *[A.ptr(x) if cap else None for x in five], speech_end.ctypes.data, statuses.ctypes.data), where)
    n = int(window_range[-1])
    return PlannedWindows(windows[:n], window_range, speech_end, statuses, *[x[:n] for x in five])


def plan_windows(audio, audio_offsets=None, config: L.TdtWindowConfig | None = None, capacity: int | None = None, ctx: L.Context | None = None) -> PlannedWindows:
    """fa_tdt_plan_windows on host arrays: audio a list of B float32 arrays of 16 kHz samples — or one array with audio_offsets
    int64[B + 1].  capacity defaults to the sum of the recordings' bounds."""
    where = "fa_tdt_plan_windows"
    audio, offsets, _ = _host_audio(audio, audio_offsets, where)
    return _run_plan(where, ctx, audio, offsets, config, capacity, False)


def plan_windows_dev(audio, audio_offsets, config: L.TdtWindowConfig | None = None, capacity: int | None = None, ctx: L.Context | None = None,
                     ordered: bool = True) -> PlannedWindows:
    """fa_tdt_plan_windows_dev: audio is a contiguous one-dimensional float32 torch tensor on the context's device.  The five operands of
    the walk come back as int32 torch tensors on that device, laid out as decode_tables / decode_logits read them."""
    where = "fa_tdt_plan_windows_dev"
    audio, offsets, _ = _dev_audio(audio, audio_offsets, where)
    return _run_plan(where, ctx, audio, offsets, config, capacity, ordered)


def _run_pack(where, ctx, audio, offsets, w, config, ordered):
    """The body of pack_windows and pack_windows_dev; rows and lengths come back beside the audio, as _run_plan's operands do."""
    row = config.max_model_samples if config is not None else 240000
    rows, lengths = A.beside(audio, (w.size, max(row, 0)), "float32", torch_empty=True), A.beside(audio, w.size, "int32", torch_empty=True)
    if w.size:
        ctx = A.context_beside(ctx, audio)
        with ctx.torch_ordered(ordered):
            ctx.check(getattr(L.lib(), where)(ctx.handle, A.cfg_ref(config), A.ptr(audio), offsets.ctypes.data, offsets.size - 1, w.ctypes.data, w.size, A.ptr(rows),
                                              w.size, A.ptr(lengths)), where)
    return rows, lengths


def pack_windows(audio, windows, audio_offsets=None, config: L.TdtWindowConfig | None = None, ctx: L.Context | None = None):
    """fa_tdt_pack_windows on host arrays.  Returns (rows [windows, max_model_samples] float32, lengths int32[windows])."""
    where = "fa_tdt_pack_windows"
    return _run_pack(where, ctx, *_host_audio(audio, audio_offsets, where, windows), config, False)


def pack_windows_dev(audio, audio_offsets, windows, config: L.TdtWindowConfig | None = None, ctx: L.Context | None = None, ordered: bool = True):
    """fa_tdt_pack_windows_dev: rows and lengths come back as torch tensors on the audio's device, in stream order — the entry does not
    synchronise.  They are what MelPlan / fa_mel_execute_dev take."""
    where = "fa_tdt_pack_windows_dev"
    return _run_pack(where, ctx, *_dev_audio(audio, audio_offsets, where, windows), config, ordered)


def _run_gate(where, ctx, config, audio, offsets, spans, override):
    B = offsets.size - 1
    s = np.ascontiguousarray(np.zeros(0, TDT_SPAN_DTYPE) if spans is None else spans, TDT_SPAN_DTYPE)
    over = None if override is None else np.ascontiguousarray(override, np.float32)
    if s.ndim != 1 or (over is not None and over.shape != (B,)):
        raise A.invalid(where, "spans is a one-dimensional array of TDT_SPAN_DTYPE, override_thresholds holds one value per recording")
    thresholds, statuses = np.zeros(B, np.float32), np.zeros(B, np.int32)
    frames, seconds = np.zeros(s.size, np.int64), np.zeros(s.size, np.float64)
    if B:
        ctx.check(getattr(L.lib(), where)(ctx.handle, A.cfg_ref(config), A.ptr(audio), offsets.ctypes.data, B, A.ptr(over), thresholds.ctypes.data,
                                          s.ctypes.data if s.size else None, s.size, frames.ctypes.data, seconds.ctypes.data, statuses.ctypes.data), where)
    elif s.size:
        raise A.invalid(where, "a span names a recording outside the batch")
    return thresholds, frames, seconds, statuses


def speech_gate(audio, spans=None, audio_offsets=None, override_thresholds=None, config: L.TdtWindowConfig | None = None, ctx: L.Context | None = None):
    """fa_tdt_speech_gate on host arrays: (thresholds float32[B], span_frames int64[n], span_seconds float64[n], statuses int32[B]);
    spans: records of TDT_SPAN_DTYPE (recording, from_sample, to_sample)."""
    where = "fa_tdt_speech_gate"
    audio, offsets, _ = _host_audio(audio, audio_offsets, where)
    return _run_gate(where, ctx or L.default_context(), config, audio, offsets, spans, override_thresholds)


def speech_gate_dev(audio, audio_offsets, spans=None, override_thresholds=None, config: L.TdtWindowConfig | None = None, ctx: L.Context | None = None, ordered: bool = True):
    """fa_tdt_speech_gate_dev: audio is a contiguous one-dimensional float32 torch tensor on the context's device."""
    where = "fa_tdt_speech_gate_dev"
    audio, offsets, _ = _dev_audio(audio, audio_offsets, where)
    ctx = ctx or L.default_context(audio.device.index)
    with ctx.torch_ordered(ordered):
        return _run_gate(where, ctx, config, audio, offsets, spans, override_thresholds)


class TdtWindowPlanner:
    """A ChunkProcessor-shaped view of one recording: chunkLayout, chunkStartDecisions, speechEndSamples, the windows, the rows and the
    gate, each answered by the batched entries with a batch of one."""

    def __init__(self, audioSamples, config: L.TdtWindowConfig | None = None, ctx: L.Context | None = None):
        self.samples = np.ascontiguousarray(audioSamples, np.float32).reshape(-1)
        self.config, self.ctx = config, ctx
        self._plan = None

    def chunkLayout(self):
        return window_layout(self.config)

    def plan(self) -> PlannedWindows:
        if self._plan is None:
            self._plan = plan_windows([self.samples], config=self.config, ctx=self.ctx)
            if self._plan.statuses[0] != L.SUCCESS:
                raise L.FluidAudioHipError(int(self._plan.statuses[0]), "fa_tdt_plan_windows", "the recording holds a non-finite energy")
        return self._plan

    def chunkStartDecisions(self):
        """(start, useWarmupPrefix) of every window that is decoded."""
        return [(int(w["chunk_start"]), bool(w["use_warmup_prefix"])) for w in self.plan().windows]

    def speechEndSamples(self) -> int:
        return int(self.plan().speech_end[0])

    def packWindows(self):
        return pack_windows([self.samples], self.plan().windows, config=self.config, ctx=self.ctx)

    def adaptiveSpeechRmsThreshold(self) -> float:
        return float(speech_gate([self.samples], config=self.config, ctx=self.ctx)[0][0])

    def speechLikeSeconds(self, startSample: int, endSample: int, threshold: float | None = None) -> float:
        spans = np.array([(0, 0, startSample, endSample)], TDT_SPAN_DTYPE)
        over = None if threshold is None else np.array([threshold], np.float32)
        return float(speech_gate([self.samples], spans, override_thresholds=over, config=self.config, ctx=self.ctx)[2][0])
