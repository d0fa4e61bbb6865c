"""The host arithmetic round the Silero VAD network on the device (csrc/vad.hip), batched over recordings: segmentSpeech(from:totalSamples:
config:) with detectSpeechSampleRanges (reference: Sources/FluidAudio/VAD/VadManager+SpeechSegmentation.swift:22-51, 71-234), the model's
input rows of processAudioSamples / processChunk (VadManager.swift:162-206, 352-376), the audio of segmentSpeechAudio (:55-67) and
streamingStateMachine (VadManager+Streaming.swift:31-107).  Integers, fp32 comparisons and fp64 divisions: the outputs are the reference's
bit for bit.  OUT OF SCOPE: the Silero network and its LSTM state (the caller runs the model on the packed rows and hands the
probabilities back) and isSilentAudio.  FSMN-VAD (VAD/Fsmn/) is fsmn_vad.py."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _args as A, _lib as L

CHUNK_SIZE, CONTEXT_LENGTH, SAMPLE_RATE = 4096, 64, 16000          # VadManager.chunkSize, VadState.contextLength, VadManager.sampleRate
MODEL_INPUT_SIZE = CONTEXT_LENGTH + CHUNK_SIZE
SPEECH_START, SPEECH_END = 0, 1                                    # VadStreamEvent.Kind
VAD_SEGMENT_DTYPE, VAD_STREAM_STATE_DTYPE, VAD_STREAM_EVENT_DTYPE = np.dtype(L.VadSegmentRecord), np.dtype(L.VadStreamStateRecord), np.dtype(L.VadStreamEventRecord)
_DIRECT_CAPACITY = 1 << 16     # records a call's output is sized for without counting first (one per frame is the bound)


def vad_config(minSpeechDuration: float = 0.15, minSilenceDuration: float = 0.75, maxSpeechDuration: float = 14.0, speechPadding: float = 0.1,
               silenceThresholdForSplit: float = 0.3, negativeThreshold: float | None = None, negativeThresholdOffset: float = 0.15,
               minSilenceAtMaxSpeech: float = 0.098, useMaxPossibleSilenceAtMaxSpeech: bool = True, defaultThreshold: float = 0.85) -> L.VadSegmentationConfig:
    """VadSegmentationConfig (VadTypes.swift:24-81) with VadConfig.defaultThreshold beside it; its preconditions are the entries' refusals."""
    cfg = L.VadSegmentationConfig()
    L.lib().fa_vad_default_config(C.byref(cfg))
    cfg.default_threshold = defaultThreshold
    cfg.min_speech_duration, cfg.min_silence_duration, cfg.max_speech_duration, cfg.speech_padding = minSpeechDuration, minSilenceDuration, maxSpeechDuration, speechPadding
    cfg.silence_threshold_for_split = silenceThresholdForSplit
    cfg.has_negative_threshold, cfg.negative_threshold = int(negativeThreshold is not None), negativeThreshold or 0.0
    cfg.negative_threshold_offset, cfg.min_silence_at_max_speech = negativeThresholdOffset, minSilenceAtMaxSpeech
    cfg.use_max_possible_silence_at_max_speech = int(useMaxPossibleSilenceAtMaxSpeech)
    return cfg


def chunk_count(samples: int) -> int:
    return int(L.lib().fa_vad_chunk_count(int(samples)))


_RANGE = "a range holds batch + 1 offsets"
_COVERS = "audio is one-dimensional and covers audio_offsets"
_DEV_AUDIO = "audio is a contiguous one-dimensional float32 tensor on the device"
_BEYOND = "audio_offsets end beyond the samples"


def _run_segments(f, where, ctx, cfg, probs_ptr, frame_range, total_samples, capacity):
    B = frame_range.size - 1
    counts, count = np.zeros(B, np.int64), C.c_int64(0)
    args = (ctx.handle, A.cfg_ref(cfg), probs_ptr, frame_range.ctypes.data, total_samples.ctypes.data, B)
    if capacity is None:
        capacity = int(np.diff(frame_range).clip(min=0).sum())         # a recording yields at most one segment per frame
        if capacity > _DIRECT_CAPACITY:                                # count first: the output of a long batch is far below the bound
            ctx.check(f(*args, None, 0, C.byref(count), None), where)
            capacity = count.value
    segs = np.zeros(int(capacity), VAD_SEGMENT_DTYPE)
    ctx.check(f(*args, segs.ctypes.data, int(capacity), C.byref(count), counts.ctypes.data), where)
    return segs[:count.value], counts


def segment_speech_batch(probs, total_samples, frame_range=None, config: L.VadSegmentationConfig | None = None, capacity: int | None = None,
                         ctx: L.Context | None = None):
    """fa_vad_segments on host arrays: probs a list of B float32 arrays (the model's probability per 4096-sample chunk) — or one array
    with frame_range int64[B + 1]; total_samples int64[B].  Returns (segments, recording_counts): segments a structured array of
    VAD_SEGMENT_DTYPE, by recording and time."""
    where = "fa_vad_segments"
    probs, frame_range = A.ragged(probs, frame_range, np.float32, where, _RANGE)
    total_samples = np.ascontiguousarray(total_samples, np.int64)
    if probs.ndim != 1 or total_samples.shape != (frame_range.size - 1,) or frame_range[-1] > probs.size:
        raise A.invalid(where, "probs is one-dimensional, covers frame_range, and total_samples holds one entry per recording")
    if frame_range.size == 1:
        return np.zeros(0, VAD_SEGMENT_DTYPE), np.zeros(0, np.int64)
    return _run_segments(L.lib().fa_vad_segments, where, ctx or L.default_context(), config, probs.ctypes.data, frame_range, total_samples, capacity)


def segment_speech_batch_dev(probs, frame_range, total_samples, config: L.VadSegmentationConfig | None = None, capacity: int | None = None,
                             ctx: L.Context | None = None, ordered: bool = True):
    """fa_vad_segments_dev: probs is a contiguous one-dimensional float32 torch tensor on the context's device, as the network left it."""
    where = "fa_vad_segments_dev"
    if not A.is_dev(probs, "float32", 1):
        raise A.invalid(where, "probs is a contiguous one-dimensional float32 tensor on the device")
    (_, frame_range), total_samples = A.ragged(probs, frame_range, np.float32, where, _RANGE), np.ascontiguousarray(total_samples, np.int64)
    if total_samples.shape != (frame_range.size - 1,) or frame_range[-1] > probs.numel():
        raise A.invalid(where, "frame_range ends beyond probs, or total_samples does not hold one entry per recording")
    if frame_range.size == 1:
        return np.zeros(0, VAD_SEGMENT_DTYPE), np.zeros(0, np.int64)
    ctx = ctx or L.default_context(probs.device.index)
    with ctx.torch_ordered(ordered):
        return _run_segments(L.lib().fa_vad_segments_dev, where, ctx, config, probs.data_ptr(), frame_range, total_samples, capacity)


def _host_audio(audio, audio_offsets, where, segments=None):
    """The audio of a host entry, with the segments where the entry takes some: what the shared bodies below are handed."""
    audio, audio_offsets = A.ragged(audio, audio_offsets, np.float32, where, _RANGE)
    segs = None if segments is None else _segments_arg(segments, where)
    if audio.ndim != 1 or audio_offsets[-1] > audio.size:
        raise A.invalid(where, _COVERS)
    return audio, audio_offsets, segs


def _dev_audio(audio, audio_offsets, where, segments=None):
    if not A.is_dev(audio, "float32", 1):
        raise A.invalid(where, _DEV_AUDIO)
    _, audio_offsets = A.ragged(audio, audio_offsets, np.float32, where, _RANGE)
    segs = None if segments is None else _segments_arg(segments, where)
    if audio_offsets[-1] > audio.numel():
        raise A.invalid(where, _BEYOND)
    return audio, audio_offsets, segs


def _run_pack(where, ctx, audio, audio_offsets, ordered):
    """The body of pack_chunks and pack_chunks_dev: the rows are a numpy array beside host audio, a torch tensor beside a device tensor."""
    B = audio_offsets.size - 1
    chunk_range = np.zeros(B + 1, np.int64)
    n_rows = int(sum(chunk_count(n) for n in np.diff(audio_offsets)))
    rows = A.beside(audio, (max(n_rows, 0), MODEL_INPUT_SIZE), "float32", torch_empty=True)
    if B == 0:
        return rows, chunk_range
    ctx = A.context_beside(ctx, audio)
    with ctx.torch_ordered(ordered):
        ctx.check(getattr(L.lib(), where)(ctx.handle, A.ptr(audio), audio_offsets.ctypes.data, B, A.ptr(rows), rows.shape[0], chunk_range.ctypes.data), where)
    return rows, chunk_range


def pack_chunks(audio, audio_offsets=None, ctx: L.Context | None = None):
    """fa_vad_pack_chunks on host arrays: audio a list of B float32 arrays of 16 kHz samples — or one array with audio_offsets
    int64[B + 1].  Returns (rows [sum chunks, 4160] float32, chunk_range int64[B + 1])."""
    where = "fa_vad_pack_chunks"
    audio, audio_offsets, _ = _host_audio(audio, audio_offsets, where)
    return _run_pack(where, ctx, audio, audio_offsets, False)


def pack_chunks_dev(audio, audio_offsets, ctx: L.Context | None = None, ordered: bool = True):
    """fa_vad_pack_chunks_dev: audio is a contiguous one-dimensional float32 torch tensor on the context's device; the rows come back as a
    torch tensor on that device, in stream order — the entry does not synchronise."""
    where = "fa_vad_pack_chunks_dev"
    audio, audio_offsets, _ = _dev_audio(audio, audio_offsets, where)
    return _run_pack(where, ctx, audio, audio_offsets, ordered)


def _segments_arg(segments, where):
    segs = np.ascontiguousarray(segments, VAD_SEGMENT_DTYPE)
    if segs.ndim != 1:
        raise A.invalid(where, "segments is a one-dimensional array of VAD_SEGMENT_DTYPE")
    return segs


def segment_bounds(start_time: float, end_time: float, samples: int):
    """The sample bounds segmentSpeechAudio cuts with (:61-64): Int(time * 16000.0), clamped.  Not start_sample / end_sample."""
    to_int = lambda x: int(x)   # noqa: E731  Int(_:) truncates; it traps where int() raises
    lo = max(0, min(to_int(start_time * float(SAMPLE_RATE)), samples))
    return lo, max(lo, min(to_int(end_time * float(SAMPLE_RATE)), samples))


def _gather_size(segs, audio_offsets):
    return sum(b - a for a, b in (segment_bounds(float(s["start_time"]), float(s["end_time"]), int(audio_offsets[s["recording"] + 1] - audio_offsets[s["recording"]]))
                                  for s in segs if 0 <= s["recording"] < audio_offsets.size - 1 and math.isfinite(s["start_time"]) and math.isfinite(s["end_time"])))


def _run_gather(where, ctx, audio, audio_offsets, segs, ordered):
    """The body of gather_segments and gather_segments_dev; the samples come back beside the audio, as _run_pack's rows do."""
    out_range = np.zeros(segs.size + 1, np.int64)
    out = A.beside(audio, _gather_size(segs, audio_offsets), "float32", torch_empty=True)
    if segs.size == 0:
        return out, out_range
    ctx = A.context_beside(ctx, audio)
    with ctx.torch_ordered(ordered):
        ctx.check(getattr(L.lib(), where)(ctx.handle, A.ptr(audio), audio_offsets.ctypes.data, audio_offsets.size - 1, segs.ctypes.data, segs.size, A.ptr(out),
                                          out.shape[0], out_range.ctypes.data), where)
    return out, out_range


def gather_segments(audio, segments, audio_offsets=None, ctx: L.Context | None = None):
    """fa_vad_gather_segments on host arrays: the speech audio of every segment (segmentSpeechAudio).  Returns (samples, out_range
    int64[n + 1]): segment i is samples[out_range[i]:out_range[i + 1]]."""
    where = "fa_vad_gather_segments"
    return _run_gather(where, ctx, *_host_audio(audio, audio_offsets, where, segments), False)


def gather_segments_dev(audio, audio_offsets, segments, ctx: L.Context | None = None, ordered: bool = True):
    """fa_vad_gather_segments_dev: audio as for pack_chunks_dev; the samples come back as a torch tensor on that device."""
    where = "fa_vad_gather_segments_dev"
    return _run_gather(where, ctx, *_dev_audio(audio, audio_offsets, where, segments), ordered)


def initial_stream_states(streams: int) -> np.ndarray:
    """VadStreamState.initial() for every stream (without the model's state, which stays the caller's)."""
    return np.zeros(int(streams), VAD_STREAM_STATE_DTYPE)


def _run_stream(f, where, ctx, cfg, probs_ptr, counts, samples_ptr, S, K, states, return_seconds, time_resolution):
    events, count = np.zeros(int(counts.sum()), VAD_STREAM_EVENT_DTYPE), C.c_int64(0)       # at most one event per chunk
    ctx.check(f(ctx.handle, A.cfg_ref(cfg), probs_ptr, counts.ctypes.data, samples_ptr, S, K, states.ctypes.data, int(bool(return_seconds)),
                int(time_resolution), events.ctypes.data, events.size, C.byref(count)), where)
    return events[:count.value]


def stream_advance(probs, states, chunk_counts=None, chunk_samples=None, config: L.VadSegmentationConfig | None = None, return_seconds: bool = False,
                   time_resolution: int = 1, ctx: L.Context | None = None):
    """fa_vad_stream_advance on host arrays: probs [S, K] float32, states the S records of VAD_STREAM_STATE_DTYPE (updated in place),
    chunk_counts int32[S] (default: K for all), chunk_samples [S, K] int32 (default: 4096).  Returns the events, by stream and chunk."""
    where = "fa_vad_stream_advance"
    probs = np.ascontiguousarray(probs, np.float32)
    if probs.ndim != 2 or states.dtype != VAD_STREAM_STATE_DTYPE or states.shape != (probs.shape[0],) or not states.flags.c_contiguous:
        raise A.invalid(where, "probs is [S, K] and states holds S contiguous records of VAD_STREAM_STATE_DTYPE")
    S, K = probs.shape
    counts = np.full(S, K, np.int32) if chunk_counts is None else np.ascontiguousarray(chunk_counts, np.int32)
    samples = None if chunk_samples is None else np.ascontiguousarray(chunk_samples, np.int32)
    if counts.shape != (S,) or (samples is not None and samples.shape != (S, K)):
        raise A.invalid(where, "chunk_counts is [S] and chunk_samples [S, K]")
    if S == 0:
        return np.zeros(0, VAD_STREAM_EVENT_DTYPE)
    return _run_stream(L.lib().fa_vad_stream_advance, where, ctx or L.default_context(), config, probs.ctypes.data, counts, A.ptr(samples), S, K, states,
                       return_seconds, time_resolution)


def stream_advance_dev(probs, states, chunk_counts=None, chunk_samples=None, config: L.VadSegmentationConfig | None = None, return_seconds: bool = False,
                       time_resolution: int = 1, ctx: L.Context | None = None, ordered: bool = True):
    """fa_vad_stream_advance_dev: probs [S, K] float32 and chunk_samples [S, K] int32 (optional) are contiguous torch tensors on the
    context's device; states and chunk_counts are host arrays."""
    where = "fa_vad_stream_advance_dev"
    if not A.is_dev(probs, "float32", 2) or (chunk_samples is not None and not (A.is_dev(chunk_samples, "int32") and chunk_samples.shape == probs.shape)):
        raise A.invalid(where, "probs is a contiguous [S, K] float32 tensor on the device, chunk_samples an int32 one of the same shape")
    S, K = probs.shape
    if states.dtype != VAD_STREAM_STATE_DTYPE or states.shape != (S,) or not states.flags.c_contiguous:
        raise A.invalid(where, "states holds S contiguous records of VAD_STREAM_STATE_DTYPE")
    counts = np.full(S, K, np.int32) if chunk_counts is None else np.ascontiguousarray(chunk_counts, np.int32)
    if counts.shape != (S,):
        raise A.invalid(where, "chunk_counts is [S]")
    if S == 0:
        return np.zeros(0, VAD_STREAM_EVENT_DTYPE)
    ctx = ctx or L.default_context(probs.device.index)
    with ctx.torch_ordered(ordered):
        return _run_stream(L.lib().fa_vad_stream_advance_dev, where, ctx, config, probs.data_ptr(), counts, A.ptr(chunk_samples), S, K, states, return_seconds,
                           time_resolution)
