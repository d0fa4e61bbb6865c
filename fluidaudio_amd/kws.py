"""CTC word spotting for custom vocabularies on the device (csrc/kws.hip, kws_host.hip): CtcDPAlgorithm.ctcWordSpotMultiple /
ctcWordSpotConstrained (reference: Sources/FluidAudio/ASR/Parakeet/SlidingWindow/CustomVocabulary/WordSpotting/CtcDPAlgorithm.swift:250-392)
and the per-term loop of CtcKeywordSpotter.spotKeywordsFromLogProbs (CtcKeywordSpotter.swift:191-254), batched over utterances.

The log-probabilities are a torch device tensor — e.g. straight from ctc_log_probs_dev, without leaving the device — or a numpy array;
keywords are lists of token ids (WILDCARD matches any frame at no cost).  Scores and frames are the reference's bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args as A, _lib as L

WILDCARD = -1
MAX_TOKENS = 127
DEFAULT_BLANK_ID = 1024            # ContextBiasingConstants.defaultBlankId
KWS_DETECTION_DTYPE, KWS_WINDOW_DTYPE = np.dtype(L.KwsDetection), np.dtype(L.KwsWindow)


def adjusted_threshold(min_score, token_count: int) -> float:
    """The threshold of one term (CtcKeywordSpotter.swift:217-222): min_score - max(0, tokens - 3) * 1.0 in fp32, or -15 for None."""
    return float(L.lib().fa_kws_adjusted_threshold(0 if min_score is None else 1, 0.0 if min_score is None else float(min_score), int(token_count)))


def _pack_keywords(keywords):
    off = np.zeros(len(keywords) + 1, np.int64)
    if len(keywords):
        off[1:] = np.cumsum([len(k) for k in keywords])
    flat = [int(t) for k in keywords for t in k]
    return np.asarray(flat if flat else [0], np.int32), off


class _Matrix:
    """The addressing of a [B, T, W] batch of log-probs: a torch device tensor (last dimension contiguous) or a host array."""

    def __init__(self, log_probs, vocab):
        self.device = hasattr(log_probs, "data_ptr")
        if self.device:
            x = log_probs if log_probs.dim() == 3 else log_probs[None]
            import torch
            assert x.dtype == torch.float32 and x.is_cuda and (x.shape[2] <= 1 or x.stride(2) == 1), "log_probs: float32 device tensor, last dimension contiguous"
            self.keep, self.ptr = x, A.ptr(x)
            self.B, self.T, W = (int(v) for v in x.shape)
            self.matrix_stride, self.row_stride = A.dense_strides(x)
        else:
            x = np.ascontiguousarray(log_probs, np.float32)
            x = x if x.ndim == 3 else x[None]
            assert x.ndim == 3, "log_probs must be [T, V] or [B, T, V]"
            self.keep, self.ptr = x, C.c_void_p(x.ctypes.data if x.size else None)
            self.B, self.T, W = x.shape
            self.row_stride, self.matrix_stride = W, self.T * W
        self.V = W if vocab is None else int(vocab)


def spot_keywords_batch(log_probs, keywords, min_score=None, blank_id: int = DEFAULT_BLANK_ID, merge_overlap: bool = True, valid_frames=None,
                        vocab: int | None = None, thresholds=None, capacity: int | None = None, ctx: L.Context | None = None, order: bool = True):
    """Every utterance of log_probs [B, T, V] against every keyword -> (detections, utterance_counts): a structured array of
    KWS_DETECTION_DTYPE ordered by utterance, then keyword, then as the reference's array holds them, and int64[B] counts.
    min_score is the caller's base threshold, adjusted per term as spotKeywordsFromLogProbs does (None: -15); `thresholds` gives
    ctcWordSpotMultiple's minScore per keyword directly instead.  Device tensors are read on ctx.stream, ordered against torch's current
    stream unless order=False."""
    ctx = ctx or L.default_context()
    m = _Matrix(log_probs, vocab)
    tok, off = _pack_keywords(keywords)
    K = len(keywords)
    if thresholds is None:
        mins = None if min_score is None else np.asarray([adjusted_threshold(min_score, len(k)) for k in keywords] or [0.0], np.float32)
    else:
        mins = np.ascontiguousarray(thresholds, np.float32)
        assert mins.size == K
    vf = None if valid_frames is None else np.ascontiguousarray(valid_frames, np.int32)
    counts = np.zeros(max(m.B, 1), np.int64)
    n = C.c_int64()
    f = L.lib().fa_ctc_kws_spot_batch_dev if m.device else L.lib().fa_ctc_kws_spot_batch
    cap = max(1024, 2 * m.B * K) if capacity is None else int(capacity)

    def call(dets):
        return f(ctx.handle, m.ptr, m.B, m.T, m.V, m.row_stride, m.matrix_stride, A.ptr(vf), tok.ctypes.data, off.ctypes.data, K,
                 A.ptr(mins), int(blank_id), 1 if merge_overlap else 0, dets.ctypes.data, dets.size, C.byref(n), counts.ctypes.data)
    with ctx.torch_ordered(order and m.device):
        dets = np.zeros(max(cap, 1), KWS_DETECTION_DTYPE)
        st = call(dets[:cap])
        if st == L.OUTPUT_TOO_SMALL and capacity is None:   # the count is known now
            dets = np.zeros(n.value, KWS_DETECTION_DTYPE)
            st = call(dets)
        ctx.check(st, f.__name__)
    return dets[:min(n.value, dets.size)].copy(), counts[:m.B]


def score_windows(log_probs, keywords, windows, blank_id: int = DEFAULT_BLANK_ID, valid_frames=None, vocab: int | None = None,
                  ctx: L.Context | None = None, order: bool = True):
    """ctcWordSpotConstrained for each (utterance, keyword, start_frame, end_frame) of `windows` -> structured array of KWS_DETECTION_DTYPE,
    one record per window."""
    ctx = ctx or L.default_context()
    m = _Matrix(log_probs, vocab)
    tok, off = _pack_keywords(keywords)
    win = np.zeros(len(windows), KWS_WINDOW_DTYPE)
    for i, w in enumerate(windows):
        win[i] = tuple(int(v) for v in w)
    vf = None if valid_frames is None else np.ascontiguousarray(valid_frames, np.int32)
    out = np.zeros(max(len(windows), 1), KWS_DETECTION_DTYPE)
    f = L.lib().fa_ctc_kws_score_windows_dev if m.device else L.lib().fa_ctc_kws_score_windows
    with ctx.torch_ordered(order and m.device):
        ctx.check(f(ctx.handle, m.ptr, m.B, m.T, m.V, m.row_stride, m.matrix_stride, A.ptr(vf),
                    tok.ctypes.data, off.ctypes.data, len(keywords), win.ctypes.data, len(windows), int(blank_id), out.ctypes.data), f.__name__)
    return out[:len(windows)].copy()
