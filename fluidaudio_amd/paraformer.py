"""Paraformer's host loop on the device (csrc/paraformer.hip), batched over utterances: ParaformerCif.integrateAndFireWithFireFrames with
the decoder's input packing (reference: Sources/FluidAudio/ASR/Paraformer/ParaformerCif.swift:19-50, ParaformerManager.swift:416-448)
and the token spans of decodeWithTimestamps (ParaformerManager.swift:134-358).  The fp32 chains and the fp64 time arithmetic run on the
device in the reference's order; the text side — the keep table standing for the charList filter, the BPE merge of the emission
(:228-256) and decode (:450-463) — is formed here.  OUT OF SCOPE: the networks (preprocessor, encoder, CifAlphas, decoder), the
AudioConverter and loading the vocabulary."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _args as A, _lib as L

PARAFORMER_SPAN_DTYPE = np.dtype(L.ParaformerSpan)
CifResult = namedtuple("CifResult", "ac token_counts fire_counts fire_frames enc_packed")
TimestampedSegment = namedtuple("TimestampedSegment", "startTime endTime text")   # ParaformerManager.swift:12-22
WORD_BOUNDARY = "▁"                                                           # ASRConstants.sentencePieceWordBoundary


class ParaformerConfig:
    """ParaformerConfig.swift:8-39"""
    featureDim, encoderDim = 560, 512
    encoderBuckets = (128, 256, 512, 1024, 1800)
    decoderEncFrames, decoderMaxTokens = 512, 128
    blankId, sosId, eosId = 0, 1, 2
    cifThreshold, cifTailThreshold = 1.0, 0.45
    sampleRate = 16000
    waveformScale = 32768.0

    @classmethod
    def pickEncoderBucket(cls, frames: int) -> int:
        return next((b for b in cls.encoderBuckets if b >= frames), cls.encoderBuckets[-1])


def default_config() -> L.ParaformerCifConfig:
    cfg = L.ParaformerCifConfig()
    L.lib().fa_paraformer_cif_default_config(C.byref(cfg))
    return cfg


def _valid(valid_frames, batch, where):
    if valid_frames is None:
        return None
    v = np.ascontiguousarray(valid_frames, np.int32)
    if v.shape != (batch,):
        raise A.invalid(where, "valid_frames holds one entry per utterance")
    return v


def _rows_on_device(t, dtype_names, ndim):
    """A torch tensor of one of the dtypes and of that rank on a CUDA device whose rows are contiguous: any row and matrix stride."""
    return any(A.is_dev(t, name, ndim, contiguous=False) for name in dtype_names) and (t.shape[-1] <= 1 or t.stride(-1) == 1)


def _run_cif(where, ctx, cfg, enc, dtype, dim, matrix_stride, row_stride, alphas, alpha_stride, valid, pack_enc, ordered) -> CifResult:
    """The body of cif_batch and cif_batch_dev: enc and alphas are numpy arrays or device tensors, addressed by the strides; ac and
    enc_packed come back beside them."""
    B, T = enc.shape[:2]
    ac = A.beside(enc, (B, cfg.max_tokens, max(dim, 0)), "float32", torch_empty=True)
    packed = A.beside(enc, (B, cfg.enc_frames, max(dim, 0)), "float32", torch_empty=True) if pack_enc else None
    counts, fires, frames = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, T + 1), -1, np.int32)
    if B:
        ctx = A.context_beside(ctx, enc)
        with ctx.torch_ordered(ordered):
            ctx.check(getattr(L.lib(), where)(ctx.handle, C.byref(cfg), A.ptr(enc), dtype, B, T, dim, row_stride, matrix_stride, A.ptr(alphas), alpha_stride, A.ptr(valid),
                                              A.ptr(ac), A.ptr(packed), counts.ctypes.data, fires.ctypes.data, frames.ctypes.data), where)
    return CifResult(ac, counts, fires, frames, packed)


def cif_batch(enc, alphas, valid_frames=None, dim: int | None = None, config: L.ParaformerCifConfig | None = None, pack_enc: bool = False,
              ctx: L.Context | None = None) -> CifResult:
    """fa_paraformer_cif on host arrays.  enc [B, T, S] float32 or float16, of whose rows the first `dim` (default S) elements are read;
    alphas [B, >= T] float32; valid_frames int32[B] (default: T for all).  Returns CifResult: ac [B, max_tokens, dim], token_counts
    (the decoder's tn), fire_counts (unclamped), fire_frames [B, T + 1] (-1 behind the fires) and, with pack_enc, the decoder's enc
    [B, enc_frames, dim]."""
    where = "fa_paraformer_cif"
    enc = np.ascontiguousarray(enc)
    if enc.ndim != 3 or enc.dtype not in (np.float32, np.float16):
        raise A.invalid(where, "enc is [B, T, S] float32 or float16")
    alphas = np.ascontiguousarray(alphas, np.float32)
    B, T, S = enc.shape
    if alphas.ndim != 2 or alphas.shape[0] != B or alphas.shape[1] < T:
        raise A.invalid(where, "alphas is [B, >= T]")
    cfg = config or default_config()
    return _run_cif(where, ctx, cfg, enc, L.DTYPE_F16 if enc.dtype == np.float16 else L.DTYPE_F32, S if dim is None else int(dim), T * S, S, alphas, alphas.shape[1],
                    _valid(valid_frames, B, where), pack_enc, False)


def cif_batch_dev(enc, alphas, valid_frames=None, dim: int | None = None, config: L.ParaformerCifConfig | None = None, pack_enc: bool = False,
                  ctx: L.Context | None = None, ordered: bool = True) -> CifResult:
    """fa_paraformer_cif_dev: enc [B, T, S] (float32 or float16, rows contiguous: any row and matrix stride) and alphas [B, A] (float32,
    rows contiguous) are torch tensors on the context's device, as the encoder and the CifAlphas model left them; ac and enc_packed come
    back as torch tensors on that device, the counts and the fire frames as numpy arrays."""
    where = "fa_paraformer_cif_dev"
    if not _rows_on_device(enc, ("float32", "float16"), 3):
        raise A.invalid(where, "enc is a [B, T, S] float32 or float16 tensor on the device with contiguous rows")
    if not _rows_on_device(alphas, ("float32",), 2):
        raise A.invalid(where, "alphas is a [B, A] float32 tensor on the device with contiguous rows")
    B, T, S = enc.shape
    if alphas.shape[0] != B or alphas.shape[1] < T:
        raise A.invalid(where, "alphas is [B, >= T]")
    cfg = config or default_config()
    dtype = L.DTYPE_F16 if A.is_dev(enc, "float16", contiguous=False) else L.DTYPE_F32
    return _run_cif(where, ctx, cfg, enc, dtype, S if dim is None else int(dim), *A.dense_strides(enc, max(S, 1)), alphas, *A.dense_strides(alphas),
                    _valid(valid_frames, B, where), pack_enc, ordered)


def keep_table(vocabulary: dict, size: int | None = None) -> np.ndarray:
    """The charList filter of decodeWithTimestamps (:146-156) as a table over the ids: 0 for blank, <s>, </s>, ids without a vocabulary
    entry and empty strings."""
    size = (max(vocabulary) + 1 if vocabulary else 0) if size is None else size
    keep = np.zeros(size, np.uint8)
    for i, tok in vocabulary.items():
        if 0 <= i < size and i not in (ParaformerConfig.blankId, ParaformerConfig.sosId, ParaformerConfig.eosId) and tok:
            keep[i] = 1
    return keep


def _stamp_host_args(valid_frames, token_counts, keep, audio_offsets, B, where):
    valid = _valid(valid_frames, B, where)
    token_counts = np.ascontiguousarray(token_counts, np.int32)
    keep = np.ascontiguousarray(keep, np.uint8)
    audio_offsets = np.ascontiguousarray(audio_offsets, np.int64)
    if token_counts.shape != (B,) or keep.ndim != 1 or audio_offsets.shape != (B + 1,):
        raise A.invalid(where, "token_counts [B], keep [vocab] and audio_offsets [B + 1] are required")
    return valid, token_counts, keep, audio_offsets


def _run_stamps(f, where, ctx, cfg, alphas_ptr, alpha_stride, B, T, valid, ids_ptr, token_counts, keep, audio_ptr, audio_offsets, capacity):
    utt = np.zeros(B, np.int64)
    cap = int(token_counts.sum()) if capacity is None else int(capacity)   # an utterance yields at most one span per token
    spans = np.zeros(cap, PARAFORMER_SPAN_DTYPE)
    count = C.c_int64(0)
    ctx.check(f(ctx.handle, C.byref(cfg), alphas_ptr, alpha_stride, B, T, A.ptr(valid), ids_ptr, token_counts.ctypes.data, keep.ctypes.data, keep.size, audio_ptr,
                audio_offsets.ctypes.data, spans.ctypes.data, cap, C.byref(count), utt.ctypes.data), where)
    return spans[:count.value], utt


def timestamps_batch(alphas, valid_frames, token_ids, token_counts, keep, audio, audio_offsets=None, config: L.ParaformerCifConfig | None = None,
                     capacity: int | None = None, ctx: L.Context | None = None):
    """fa_paraformer_timestamps on host arrays: alphas [B, >= T] float32 (T = alphas.shape[1] unless valid_frames says less), token_ids
    [B, max_tokens] int32 (the argmax of the decoder's logits), token_counts int32[B], keep uint8[vocab] (keep_table), audio a list of B
    float32 arrays of 16 kHz samples — or one array with audio_offsets int64[B + 1].  Returns (spans, utterance_counts): spans a
    structured array of PARAFORMER_SPAN_DTYPE, by utterance and token."""
    where = "fa_paraformer_timestamps"
    alphas = np.ascontiguousarray(alphas, np.float32)
    token_ids = np.ascontiguousarray(token_ids, np.int32)
    cfg = config or default_config()
    if alphas.ndim != 2 or token_ids.ndim != 2 or token_ids.shape != (alphas.shape[0], cfg.max_tokens):
        raise A.invalid(where, "alphas is [B, T] and token_ids [B, max_tokens]")
    B, T = alphas.shape
    audio, audio_offsets = A.ragged(audio, audio_offsets, np.float32)      # the offsets' shape is _stamp_host_args' to refuse
    valid, token_counts, keep, audio_offsets = _stamp_host_args(valid_frames, token_counts, keep, audio_offsets, B, where)
    if audio.ndim != 1 or (B > 0 and audio_offsets[-1] > audio.size):
        raise A.invalid(where, "audio_offsets end beyond the samples")
    if B == 0:
        return np.zeros(0, PARAFORMER_SPAN_DTYPE), np.zeros(0, np.int64)
    ctx = ctx or L.default_context()
    return _run_stamps(L.lib().fa_paraformer_timestamps, where, ctx, cfg, alphas.ctypes.data, alphas.shape[1], B, T, valid, token_ids.ctypes.data, token_counts, keep,
                       audio.ctypes.data, audio_offsets, capacity)


def timestamps_batch_dev(alphas, valid_frames, token_ids, token_counts, keep, audio, audio_offsets, config: L.ParaformerCifConfig | None = None,
                         capacity: int | None = None, ctx: L.Context | None = None, ordered: bool = True):
    """fa_paraformer_timestamps_dev: alphas [B, A] float32, token_ids [B, max_tokens] int32 (contiguous) and audio (one-dimensional
    float32, the utterances one after the other) are torch tensors on the context's device; the rest are host arrays."""
    where = "fa_paraformer_timestamps_dev"
    cfg = config or default_config()
    if not _rows_on_device(alphas, ("float32",), 2):
        raise A.invalid(where, "alphas is a [B, A] float32 tensor on the device with contiguous rows")
    B, T = alphas.shape
    if not (A.is_dev(token_ids, "int32", 2) and tuple(token_ids.shape) == (B, cfg.max_tokens)):
        raise A.invalid(where, "token_ids is a contiguous [B, max_tokens] int32 tensor on the device")
    if not A.is_dev(audio, "float32", 1):
        raise A.invalid(where, "audio is a contiguous one-dimensional float32 tensor on the device")
    valid, token_counts, keep, audio_offsets = _stamp_host_args(valid_frames, token_counts, keep, audio_offsets, B, where)
    if B > 0 and audio_offsets[-1] > audio.numel():
        raise A.invalid(where, "audio_offsets end beyond the samples")
    if B == 0:
        return np.zeros(0, PARAFORMER_SPAN_DTYPE), np.zeros(0, np.int64)
    ctx = ctx or L.default_context(alphas.device.index)
    with ctx.torch_ordered(ordered):
        return _run_stamps(L.lib().fa_paraformer_timestamps_dev, where, ctx, cfg, alphas.data_ptr(), *A.dense_strides(alphas), B, T, valid, token_ids.data_ptr(),
                           token_counts, keep, audio.data_ptr(), audio_offsets, capacity)


def segments_from_spans(vocabulary: dict, token_ids, spans) -> list:
    """The emission of decodeWithTimestamps (:228-256) for ONE utterance: token_ids is its row of ids, spans its records (token_index,
    start, end) in order.  BPE continuations (`cu@@` + `t`) are merged, the word boundary is stripped, empty texts are dropped."""
    raw = [(vocabulary[int(token_ids[int(s["token_index"])])], float(s["start"]), float(s["end"])) for s in spans]
    out, i = [], 0
    while i < len(raw):
        text, start, end = raw[i]
        while text.endswith("@@"):
            text = text[:-2]
            i += 1
            if i < len(raw):
                piece = raw[i][0]
                text += piece[1:] if piece.startswith(WORD_BOUNDARY) else piece
                end = raw[i][2]
        if text.startswith(WORD_BOUNDARY):
            text = text[1:]
        if text:
            out.append(TimestampedSegment(start if start >= 0 else 0.0, end, text))
        i += 1
    return out


def decode_tokens(token_ids, vocabulary: dict) -> str:
    """ParaformerManager.decode (:450-463) behind the argmax: the pieces of the ids that are not blank, <s> or </s> joined, the word
    boundary as a blank, blanks and tabs trimmed."""
    drop = (ParaformerConfig.blankId, ParaformerConfig.sosId, ParaformerConfig.eosId)
    pieces = [vocabulary[int(t)] for t in token_ids if int(t) not in drop and int(t) in vocabulary]
    return "".join(pieces).replace(WORD_BOUNDARY, " ").strip(" \t")
