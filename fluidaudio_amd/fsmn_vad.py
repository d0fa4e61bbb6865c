"""The host arithmetic round the two networks of FSMN-VAD on the device (csrc/fsmn_vad.hip), batched over recordings: the chunk schedule
of concatenateChunks with lfrFrameCount (reference: Sources/FluidAudio/VAD/Fsmn/FsmnVadManager.swift:91-117), the rows of chunkSilence
(:119-155: the scaled waveform, the zero-padded bucket of features, column 0 of the scores onto the frame grid) and decide (:159-201).
Integers and one fp32 comparison per frame: the segments are the reference's, its two quirks included.  OUT OF SCOPE: the preprocessor
and the scorer (the caller runs them on the packed rows), detect(audioURL:)'s file reading and resampling, isSilentAudio."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args as A, _lib as L

HOP_SAMPLES, FBANK_WINDOW_SAMPLES, LFR_PAD_FRAMES, FEATURE_DIM = 160, 400, 2, 400                 # FsmnVadManager.swift:26, 31-33
BUCKETS = (512, 1024, 2048, 3072)
END_SILENCE, MAX_LENGTH, END_OF_AUDIO = 0, 1, 2                                                   # fa_fsmn_vad_segment.reason
FSMN_VAD_CHUNK_DTYPE, FSMN_VAD_SEGMENT_DTYPE = np.dtype(L.FsmnVadChunkRecord), np.dtype(L.FsmnVadSegmentRecord)
_DIRECT_CAPACITY = 1 << 16     # records a call's output is sized for without counting first (one per frame is the bound)
_RANGE = "a range holds batch + 1 offsets"


def fsmn_vad_config(silenceThreshold: float = 0.2, windowFrames: int = 20, silToSpeech: int = 15, speechToSil: int = 15, maxEndSilenceFrames: int = 80,
                    lookbackFrames: int = 20, lookaheadFrames: int = 10, maxSegmentFrames: int = 6000, frameMs: int = 10) -> L.FsmnVadConfig:
    """The decision constants of FsmnVadManager (:37-45), which the reference keeps private; the bounds are the entries' refusals."""
    return L.FsmnVadConfig(silenceThreshold, windowFrames, silToSpeech, speechToSil, maxEndSilenceFrames, lookbackFrames, lookaheadFrames, maxSegmentFrames, frameMs)


def fsmn_vad_frame_count(samples: int) -> int:
    """lfrFrameCount (:113-117)."""
    return int(L.lib().fa_fsmn_vad_frame_count(int(samples)))


def fsmn_vad_plan_chunks(total_samples):
    """fa_fsmn_vad_plan_chunks: total_samples int64[B].  Returns (chunks of FSMN_VAD_CHUNK_DTYPE, chunk_range int64[B + 1], frame_range
    int64[B + 1]).  No context and no device."""
    where = "fa_fsmn_vad_plan_chunks"
    total = np.ascontiguousarray(total_samples, np.int64)
    if total.ndim != 1:
        raise A.invalid(where, "total_samples is one-dimensional")
    B = total.size
    chunk_range, frame_range, count = np.zeros(B + 1, np.int64), np.zeros(B + 1, np.int64), C.c_int64(0)
    f = L.lib().fa_fsmn_vad_plan_chunks
    st = f(total.ctypes.data, B, None, 0, C.byref(count), chunk_range.ctypes.data, frame_range.ctypes.data)
    chunks = np.zeros(count.value, FSMN_VAD_CHUNK_DTYPE)
    if st == L.SUCCESS:
        st = f(total.ctypes.data, B, chunks.ctypes.data, chunks.size, C.byref(count), chunk_range.ctypes.data, frame_range.ctypes.data)
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, where)
    return chunks, chunk_range, frame_range


def _chunks_arg(chunks, where):
    chunks = np.ascontiguousarray(chunks, FSMN_VAD_CHUNK_DTYPE)
    if chunks.ndim != 1:
        raise A.invalid(where, "chunks is a one-dimensional array of FSMN_VAD_CHUNK_DTYPE")
    return chunks


def _run_pack(where, ctx, audio, audio_offsets, chunks, row_stride, ordered):
    if row_stride is None:
        row_stride = int((chunks["end_sample"] - chunks["start_sample"]).max(initial=0))
    rows = A.beside(audio, (chunks.size, int(row_stride)), "float32", torch_empty=True)
    if chunks.size == 0:
        return rows
    ctx = A.context_beside(ctx, audio)
    with ctx.torch_ordered(ordered):
        ctx.check(getattr(L.lib(), where)(ctx.handle, A.ptr(audio), audio_offsets.ctypes.data, audio_offsets.size - 1, chunks.ctypes.data, chunks.size, A.ptr(rows), int(row_stride),
                                          chunks.size), where)
    return rows


def fsmn_vad_pack_waveforms(audio, chunks, audio_offsets=None, row_stride: int | None = None, ctx: L.Context | None = None):
    """fa_fsmn_vad_pack_waveforms on host arrays: audio a list of B float32 arrays of 16 kHz samples — or one array with audio_offsets
    int64[B + 1].  Returns rows [n, row_stride] float32 (row_stride: the longest chunk by default): the chunk times 32768, zero tails."""
    where = "fa_fsmn_vad_pack_waveforms"
    audio, audio_offsets = A.ragged(audio, audio_offsets, np.float32, where, _RANGE)
    if audio.ndim != 1 or audio_offsets[-1] > audio.size:
        raise A.invalid(where, "audio is one-dimensional and covers audio_offsets")
    return _run_pack(where, ctx, audio, audio_offsets, _chunks_arg(chunks, where), row_stride, False)


def fsmn_vad_pack_waveforms_dev(audio, audio_offsets, chunks, row_stride: int | None = None, ctx: L.Context | None = None, ordered: bool = True):
    """fa_fsmn_vad_pack_waveforms_dev: audio is a contiguous one-dimensional float32 torch tensor on the context's device; the rows come
    back as a torch tensor on that device, in stream order — the entry does not synchronise."""
    where = "fa_fsmn_vad_pack_waveforms_dev"
    if not A.is_dev(audio, "float32", 1):
        raise A.invalid(where, "audio is a contiguous one-dimensional float32 tensor on the device")
    _, audio_offsets = A.ragged(audio, audio_offsets, np.float32, where, _RANGE)
    if audio_offsets[-1] > audio.numel():
        raise A.invalid(where, "audio_offsets end beyond the samples")
    return _run_pack(where, ctx, audio, audio_offsets, _chunks_arg(chunks, where), row_stride, ordered)


def _dtype_of(t, where):
    import torch
    if t.dtype == torch.float32:
        return L.DTYPE_F32
    if t.dtype == torch.float16:
        return L.DTYPE_F16
    raise A.invalid(where, "the tensor is float32 or float16")


def fsmn_vad_pack_feats_dev(feats, chunks, bucket: int, ctx: L.Context | None = None, ordered: bool = True):
    """fa_fsmn_vad_pack_feats_dev: feats [n, feat_stride, 400], a contiguous float32 or float16 torch tensor on the device -> the scorer's
    input [n, bucket, 400] float32: a chunk's first `frames` rows, zeros behind them."""
    import torch
    where = "fa_fsmn_vad_pack_feats_dev"
    chunks = _chunks_arg(chunks, where)
    if not (isinstance(feats, torch.Tensor) and feats.is_cuda and feats.is_contiguous() and feats.dim() == 3 and feats.shape[0] == chunks.size and feats.shape[2] == FEATURE_DIM):
        raise A.invalid(where, "feats is a contiguous [n, feat_stride, 400] tensor on the device, one matrix per chunk")
    dtype = _dtype_of(feats, where)
    out = torch.empty((chunks.size, int(bucket), FEATURE_DIM), dtype=torch.float32, device=feats.device)
    ctx = A.context_beside(ctx, feats)
    with ctx.torch_ordered(ordered):
        ctx.check(L.lib().fa_fsmn_vad_pack_feats_dev(ctx.handle, A.ptr(feats), dtype, int(feats.shape[1]), chunks.ctypes.data, chunks.size, int(bucket), A.ptr(out)), where)
    return out


def fsmn_vad_gather_silence_dev(scores, chunks, frame_range, ctx: L.Context | None = None, ordered: bool = True):
    """fa_fsmn_vad_gather_silence_dev: scores [n, bucket, vocab], a contiguous float32 or float16 torch tensor on the device -> the
    silence probabilities float32[frame_range[-1]] of all recordings on their frame grids, ready for fsmn_vad_segments_dev."""
    import torch
    where = "fa_fsmn_vad_gather_silence_dev"
    chunks, frame_range = _chunks_arg(chunks, where), np.ascontiguousarray(frame_range, np.int64)
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.is_contiguous() and scores.dim() == 3 and scores.shape[0] == chunks.size):
        raise A.invalid(where, "scores is a contiguous [n, bucket, vocab] tensor on the device, one matrix per chunk")
    if frame_range.ndim != 1 or frame_range.size < 1:
        raise A.invalid(where, _RANGE)
    dtype = _dtype_of(scores, where)
    silence = torch.empty(max(int(frame_range[-1]), 0), dtype=torch.float32, device=scores.device)
    ctx = A.context_beside(ctx, scores)
    with ctx.torch_ordered(ordered):
        ctx.check(L.lib().fa_fsmn_vad_gather_silence_dev(ctx.handle, A.ptr(scores), dtype, int(scores.shape[1]), int(scores.shape[2]), chunks.ctypes.data, chunks.size,
                                                         frame_range.ctypes.data, frame_range.size - 1, A.ptr(silence), silence.numel()), where)
    return silence


def _run_segments(f, where, ctx, cfg, probs_ptr, frame_range, capacity):
    B = frame_range.size - 1
    counts, count = np.zeros(B, np.int64), C.c_int64(0)
    args = (ctx.handle, A.cfg_ref(cfg), probs_ptr, frame_range.ctypes.data, B)
    if capacity is None:
        capacity = int(np.diff(frame_range).clip(min=0).sum())         # a recording closes at most one segment per frame
        if capacity > _DIRECT_CAPACITY:                                # count first: the output of a long batch is far below the bound
            ctx.check(f(*args, None, 0, C.byref(count), None), where)
            capacity = count.value
    segs = np.zeros(int(capacity), FSMN_VAD_SEGMENT_DTYPE)
    ctx.check(f(*args, segs.ctypes.data, int(capacity), C.byref(count), counts.ctypes.data), where)
    return segs[:count.value], counts


def fsmn_vad_segments(probs, frame_range=None, config: L.FsmnVadConfig | None = None, capacity: int | None = None, ctx: L.Context | None = None):
    """fa_fsmn_vad_segments on host arrays: probs a list of B float32 arrays (the silence probability per 10 ms frame) — or one array with
    frame_range int64[B + 1].  Returns (segments, recording_counts): segments a structured array of FSMN_VAD_SEGMENT_DTYPE, by recording
    and time."""
    where = "fa_fsmn_vad_segments"
    probs, frame_range = A.ragged(probs, frame_range, np.float32, where, _RANGE)
    if probs.ndim != 1 or frame_range[-1] > probs.size:
        raise A.invalid(where, "probs is one-dimensional and covers frame_range")
    if frame_range.size == 1:
        return np.zeros(0, FSMN_VAD_SEGMENT_DTYPE), np.zeros(0, np.int64)
    return _run_segments(L.lib().fa_fsmn_vad_segments, where, ctx or L.default_context(), config, probs.ctypes.data, frame_range, capacity)


def fsmn_vad_segments_dev(probs, frame_range, config: L.FsmnVadConfig | None = None, capacity: int | None = None, ctx: L.Context | None = None, ordered: bool = True):
    """fa_fsmn_vad_segments_dev: probs is a contiguous one-dimensional float32 torch tensor on the context's device, as
    fsmn_vad_gather_silence_dev left it."""
    where = "fa_fsmn_vad_segments_dev"
    if not A.is_dev(probs, "float32", 1):
        raise A.invalid(where, "probs is a contiguous one-dimensional float32 tensor on the device")
    _, frame_range = A.ragged(probs, frame_range, np.float32, where, _RANGE)
    if frame_range[-1] > probs.numel():
        raise A.invalid(where, "frame_range ends beyond probs")
    if frame_range.size == 1:
        return np.zeros(0, FSMN_VAD_SEGMENT_DTYPE), np.zeros(0, np.int64)
    ctx = ctx or L.default_context(probs.device.index)
    with ctx.torch_ordered(ordered):
        return _run_segments(L.lib().fa_fsmn_vad_segments_dev, where, ctx, config, probs.data_ptr(), frame_range, capacity)
