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

from . import _lib as L

PARAFORMER_SPAN_DTYPE = np.dtype([("utterance", np.int32), ("token_index", np.int32), ("start", np.float64), ("end", np.float64)])
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


def _invalid(where: str, detail: str):
    return L.FluidAudioHipError(L.INVALID_ARGUMENT, where, detail)


def default_config() -> L.ParaformerCifConfig:
    cfg = L.ParaformerCifConfig()
    L.lib().fa_paraformer_cif_default_config(C.byref(cfg))
    return cfg


def _valid(valid_frames, batch, where):
    if valid_frames is None:
        return None
    v = np.ascontiguousarray(valid_frames, np.int32)
    if v.shape != (batch,):
        raise _invalid(where, "valid_frames holds one entry per utterance")
    return v


def _ptr(a):
    return None if a is None else a.ctypes.data


def cif_batch(enc, alphas, valid_frames=None, dim: int | None = None, config: L.ParaformerCifConfig | None = None, pack_enc: bool = False,
              ctx: L.Context | None = None) -> CifResult:
    """fa_paraformer_cif on host arrays.  enc [B, T, S] float32 or float16, of whose rows the first `dim` (default S) elements are read;
    alphas [B, >= T] float32; valid_frames int32[B] (default: T for all).  Returns CifResult: ac [B, max_tokens, dim], token_counts
    (the decoder's tn), fire_counts (unclamped), fire_frames [B, T + 1] (-1 behind the fires) and, with pack_enc, the decoder's enc
    [B, enc_frames, dim]."""
    where = "fa_paraformer_cif"
    enc = np.ascontiguousarray(enc)
    if enc.ndim != 3 or enc.dtype not in (np.float32, np.float16):
        raise _invalid(where, "enc is [B, T, S] float32 or float16")
    alphas = np.ascontiguousarray(alphas, np.float32)
    B, T, S = enc.shape
    dim = S if dim is None else int(dim)
    if alphas.ndim != 2 or alphas.shape[0] != B or alphas.shape[1] < T:
        raise _invalid(where, "alphas is [B, >= T]")
    cfg = config or default_config()
    valid = _valid(valid_frames, B, where)
    ac = np.zeros((B, cfg.max_tokens, max(dim, 0)), np.float32)
    packed = np.zeros((B, cfg.enc_frames, max(dim, 0)), np.float32) if pack_enc else None
    counts, fires, frames = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, T + 1), -1, np.int32)
    if B == 0:
        return CifResult(ac, counts, fires, frames, packed)
    ctx = ctx or L.default_context()
    ctx.check(L.lib().fa_paraformer_cif(ctx.handle, C.byref(cfg), enc.ctypes.data, L.DTYPE_F16 if enc.dtype == np.float16 else L.DTYPE_F32, B, T, dim, S, T * S,
                                        alphas.ctypes.data, alphas.shape[1], _ptr(valid), ac.ctypes.data, _ptr(packed), counts.ctypes.data, fires.ctypes.data,
                                        frames.ctypes.data), where)
    return CifResult(ac, counts, fires, frames, packed)


def cif_batch_dev(enc, alphas, valid_frames=None, dim: int | None = None, config: L.ParaformerCifConfig | None = None, pack_enc: bool = False,
                  ctx: L.Context | None = None, ordered: bool = True) -> CifResult:
    """fa_paraformer_cif_dev: enc [B, T, S] (float32 or float16, rows contiguous: any row and matrix stride) and alphas [B, A] (float32,
    rows contiguous) are torch tensors on the context's device, as the encoder and the CifAlphas model left them; ac and enc_packed come
    back as torch tensors on that device, the counts and the fire frames as numpy arrays."""
    import torch
    where = "fa_paraformer_cif_dev"
    if not (isinstance(enc, torch.Tensor) and enc.is_cuda and enc.dim() == 3 and enc.dtype in (torch.float32, torch.float16) and (enc.shape[2] <= 1 or enc.stride(2) == 1)):
        raise _invalid(where, "enc is a [B, T, S] float32 or float16 tensor on the device with contiguous rows")
    if not (isinstance(alphas, torch.Tensor) and alphas.is_cuda and alphas.dim() == 2 and alphas.dtype == torch.float32 and (alphas.shape[1] <= 1 or alphas.stride(1) == 1)):
        raise _invalid(where, "alphas is a [B, A] float32 tensor on the device with contiguous rows")
    B, T, S = enc.shape
    dim = S if dim is None else int(dim)
    if alphas.shape[0] != B or alphas.shape[1] < T:
        raise _invalid(where, "alphas is [B, >= T]")
    cfg = config or default_config()
    valid = _valid(valid_frames, B, where)
    ac = torch.empty((B, cfg.max_tokens, max(dim, 0)), dtype=torch.float32, device=enc.device)
    packed = torch.empty((B, cfg.enc_frames, max(dim, 0)), dtype=torch.float32, device=enc.device) if pack_enc else None
    counts, fires, frames = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, T + 1), -1, np.int32)
    if B == 0:
        return CifResult(ac, counts, fires, frames, packed)
    ctx = ctx or L.default_context(enc.device.index)
    row_stride = enc.stride(1) if T > 1 else max(S, 1)
    matrix_stride = enc.stride(0) if B > 1 else T * row_stride
    alpha_stride = alphas.stride(0) if B > 1 else alphas.shape[1]
    with ctx.torch_ordered(ordered):
        ctx.check(L.lib().fa_paraformer_cif_dev(ctx.handle, C.byref(cfg), enc.data_ptr(), L.DTYPE_F16 if enc.dtype == torch.float16 else L.DTYPE_F32, B, T, dim,
                                                row_stride, matrix_stride, alphas.data_ptr(), alpha_stride, _ptr(valid), ac.data_ptr(),
                                                None if packed is None else packed.data_ptr(), counts.ctypes.data, fires.ctypes.data, frames.ctypes.data), where)
    return CifResult(ac, counts, fires, frames, packed)


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
        raise _invalid(where, "token_counts [B], keep [vocab] and audio_offsets [B + 1] are required")
    return valid, token_counts, keep, audio_offsets


def _run_stamps(f, where, ctx, cfg, alphas_ptr, alpha_stride, B, T, valid, ids_ptr, token_counts, keep, audio_ptr, audio_offsets, capacity):
    utt = np.zeros(B, np.int64)
    cap = int(token_counts.sum()) if capacity is None else int(capacity)   # an utterance yields at most one span per token
    spans = np.zeros(cap, PARAFORMER_SPAN_DTYPE)
    count = C.c_int64(0)
    ctx.check(f(ctx.handle, C.byref(cfg), alphas_ptr, alpha_stride, B, T, _ptr(valid), ids_ptr, token_counts.ctypes.data, keep.ctypes.data, keep.size, audio_ptr,
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
        raise _invalid(where, "alphas is [B, T] and token_ids [B, max_tokens]")
    B, T = alphas.shape
    if audio_offsets is None:
        audio = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in audio]
        audio_offsets = np.concatenate([[0], np.cumsum([x.size for x in audio])]).astype(np.int64)
        audio = np.concatenate(audio) if audio else np.zeros(0, np.float32)
    audio = np.ascontiguousarray(audio, np.float32)
    valid, token_counts, keep, audio_offsets = _stamp_host_args(valid_frames, token_counts, keep, audio_offsets, B, where)
    if audio.ndim != 1 or (B > 0 and audio_offsets[-1] > audio.size):
        raise _invalid(where, "audio_offsets end beyond the samples")
    if B == 0:
        return np.zeros(0, PARAFORMER_SPAN_DTYPE), np.zeros(0, np.int64)
    ctx = ctx or L.default_context()
    return _run_stamps(L.lib().fa_paraformer_timestamps, where, ctx, cfg, alphas.ctypes.data, alphas.shape[1], B, T, valid, token_ids.ctypes.data, token_counts, keep,
                       audio.ctypes.data, audio_offsets, capacity)


def timestamps_batch_dev(alphas, valid_frames, token_ids, token_counts, keep, audio, audio_offsets, config: L.ParaformerCifConfig | None = None,
                         capacity: int | None = None, ctx: L.Context | None = None, ordered: bool = True):
    """fa_paraformer_timestamps_dev: alphas [B, A] float32, token_ids [B, max_tokens] int32 (contiguous) and audio (one-dimensional
    float32, the utterances one after the other) are torch tensors on the context's device; the rest are host arrays."""
    import torch
    where = "fa_paraformer_timestamps_dev"
    cfg = config or default_config()
    ok = lambda t, dt, nd: isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.dim() == nd   # noqa: E731
    if not (ok(alphas, torch.float32, 2) and (alphas.shape[1] <= 1 or alphas.stride(1) == 1)):
        raise _invalid(where, "alphas is a [B, A] float32 tensor on the device with contiguous rows")
    B, T = alphas.shape
    if not (ok(token_ids, torch.int32, 2) and token_ids.is_contiguous() and tuple(token_ids.shape) == (B, cfg.max_tokens)):
        raise _invalid(where, "token_ids is a contiguous [B, max_tokens] int32 tensor on the device")
    if not (ok(audio, torch.float32, 1) and audio.is_contiguous()):
        raise _invalid(where, "audio is a contiguous one-dimensional float32 tensor on the device")
    valid, token_counts, keep, audio_offsets = _stamp_host_args(valid_frames, token_counts, keep, audio_offsets, B, where)
    if B > 0 and audio_offsets[-1] > audio.numel():
        raise _invalid(where, "audio_offsets end beyond the samples")
    if B == 0:
        return np.zeros(0, PARAFORMER_SPAN_DTYPE), np.zeros(0, np.int64)
    ctx = ctx or L.default_context(alphas.device.index)
    with ctx.torch_ordered(ordered):
        return _run_stamps(L.lib().fa_paraformer_timestamps_dev, where, ctx, cfg, alphas.data_ptr(), alphas.stride(0) if B > 1 else alphas.shape[1], B, T, valid,
                           token_ids.data_ptr(), token_counts, keep, audio.data_ptr(), audio_offsets, capacity)


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
