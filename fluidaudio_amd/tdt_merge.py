"""TDT long-form chunk merging (csrc/tdt_merge.hip): the fold of ChunkProcessor.mergeChunks over a recording's overlapping windows and
enforceMonotonicTimestamps (reference: Sources/FluidAudio/ASR/Parakeet/SlidingWindow/TDT/ChunkProcessor.swift:843-855, 952-1219;
SequenceMatcher.swift:127-225), batched over recordings in one device call.  The merged streams are the reference's bit for bit.

The vocabulary stays the caller's: ``splice_safe_table`` and ``case_canon_table`` turn the reference's spliceSafeTokenIds set and
caseVariantCanonicalIds map into the tables the C ABI takes.  OUT OF SCOPE: collapseSeamWordDuplicates (Unicode strings),
repairSeamGaps (needs the networks), the planning of chunk starts and the streaming removeDuplicateTokenSequence."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib as L

MERGE_EMPTY, MERGE_CONCAT, MERGE_CONTIGUOUS, MERGE_LCS, MERGE_MIDPOINT = range(5)
MERGE_TAIL_VERBATIM, MERGE_TAIL_ADOPT_RIGHT, MERGE_TAIL_KEEP_LEFT = range(3)
MERGE_NO_SEAM = -1
_BASE = ("empty", "concat", "contiguous", "lcs", "midpoint")
_TAIL = ("", "+adopt-right", "+keep-left")

# tokens / timestamps / durations / confidences: flat arrays (numpy, or torch tensors on the device for merge_windows_dev); recording r
# owns [out_range[r], out_range[r] + counts[r]); statuses and counts per recording; routes per window (MERGE_NO_SEAM for a first window)
MergedWindows = namedtuple("MergedWindows", "tokens timestamps durations confidences out_range counts statuses routes")


def merge_route_name(code: int) -> str:
    return "none" if code < 0 else _BASE[code & 15] + _TAIL[code >> 4]


def _invalid(detail: str):
    return L.FluidAudioHipError(L.INVALID_ARGUMENT, "merge_windows", detail)


def splice_safe_table(safe_ids, vocab: int):
    """uint8[vocab] of a spliceSafeTokenIds set; None (nil: the legacy splices) stays None."""
    if safe_ids is None:
        return None
    t = np.zeros(int(vocab), np.uint8)
    ids = np.fromiter((i for i in safe_ids if 0 <= i < vocab), np.int64)
    t[ids] = 1
    return t


def case_canon_table(canon, vocab: int):
    """int32[vocab] of a caseVariantCanonicalIds map, -1 where it has no entry; None (nil) stays None."""
    if canon is None:
        return None
    t = np.full(int(vocab), -1, np.int32)
    for i, v in canon.items():
        if 0 <= i < vocab:
            t[i] = v
    return t


def merge_capacity(counts, window_range) -> np.ndarray:
    """Per recording, |w0| + 2 * sum of the other windows' token counts: always enough (a merge emits a right token at most twice)."""
    counts, window_range = np.asarray(counts, np.int64), np.asarray(window_range, np.int64)
    total = np.concatenate([[0], np.cumsum(counts)])
    lo, hi = window_range[:-1], window_range[1:]
    first = np.zeros(lo.size, np.int64)
    first[hi > lo] = counts[lo[hi > lo]]
    return 2 * (total[hi] - total[lo]) - first


def _tables(splice_safe, case_canon, vocab):
    def table(t, dtype):
        if t is None:
            return None
        t = np.ascontiguousarray(t, dtype)
        if t.ndim != 1:
            raise _invalid("a table is one-dimensional")
        return t
    s, c = table(splice_safe, np.uint8), table(case_canon, np.int32)
    sizes = {t.size for t in (s, c) if t is not None}
    if vocab is None:
        if len(sizes) > 1:
            raise _invalid("the tables disagree about the vocabulary's size")
        vocab = sizes.pop() if sizes else 0
    elif any(z < vocab for z in sizes):
        raise _invalid("a table is shorter than the vocabulary")
    return s, c, int(vocab)


def _config(frame_seconds, overlap_seconds):
    cfg = L.TdtMergeConfig()
    L.lib().fa_tdt_merge_default_config(C.byref(cfg))
    if frame_seconds is not None:
        cfg.frame_seconds = float(frame_seconds)
    if overlap_seconds is not None:
        cfg.overlap_seconds = float(overlap_seconds)
    return cfg


def _ranges(window_range, n_windows, capacities, counts):
    window_range = np.ascontiguousarray(window_range, np.int64)
    if window_range.ndim != 1 or window_range.size < 1 or (np.diff(window_range) < 0).any() or window_range[0] < 0 or window_range[-1] > n_windows:
        raise _invalid("window_range holds n_recordings + 1 ascending entries inside the windows")
    if capacities is None:
        capacities = merge_capacity(counts, window_range)
    capacities = np.asarray(capacities, np.int64)
    if capacities.shape != (window_range.size - 1,) or (capacities < 0).any():
        raise _invalid("one non-negative capacity per recording")
    out_range = np.zeros(window_range.size, np.int64)
    np.cumsum(capacities, out=out_range[1:])
    return window_range, out_range


def _ptr(a):
    return None if a is None else a.ctypes.data


def merge_windows(tokens, timestamps, durations, confidences, counts, window_range, splice_safe=None, case_canon=None, vocab=None,
                  frame_seconds=None, overlap_seconds=None, capacities=None, ctx: L.Context | None = None) -> MergedWindows:
    """fa_tdt_merge_windows on host arrays: the four window arrays [windows, max_out] and counts [windows] as the greedy walk writes them
    (global timestamps), window_range [n_recordings + 1].  capacities: tokens per output slice (default: merge_capacity)."""
    tok, tim, dur = (np.ascontiguousarray(a, np.int32) for a in (tokens, timestamps, durations))
    conf, cnt = np.ascontiguousarray(confidences, np.float32), np.ascontiguousarray(counts, np.int32)
    if tok.ndim != 2 or tim.shape != tok.shape or dur.shape != tok.shape or conf.shape != tok.shape or cnt.shape != (tok.shape[0],):
        raise _invalid("the window arrays are [windows, max_out] and the counts [windows]")
    windows, max_out = tok.shape
    s, c, vocab = _tables(splice_safe, case_canon, vocab)
    window_range, out_range = _ranges(window_range, windows, capacities, np.clip(cnt, 0, max_out))
    n, total = window_range.size - 1, int(out_range[-1])
    o_tok, o_time, o_dur, o_conf = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(total, np.float32)
    o_cnt, o_st, routes = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(windows, MERGE_NO_SEAM, np.int32)
    if n == 0:
        return MergedWindows(o_tok, o_time, o_dur, o_conf, out_range, o_cnt, o_st, routes)
    cfg = _config(frame_seconds, overlap_seconds)
    ctx = ctx or L.default_context()
    ctx.check(L.lib().fa_tdt_merge_windows(ctx.handle, C.byref(cfg), _ptr(tok), _ptr(tim), _ptr(dur), _ptr(conf), _ptr(cnt), max_out, _ptr(window_range), n,
                                           _ptr(s), _ptr(c), vocab, _ptr(o_tok), _ptr(o_time), _ptr(o_dur), _ptr(o_conf), _ptr(out_range), _ptr(o_cnt),
                                           _ptr(o_st), _ptr(routes)), "fa_tdt_merge_windows")
    return MergedWindows(o_tok, o_time, o_dur, o_conf, out_range, o_cnt, o_st, routes)


def merge_windows_dev(d_tokens, d_timestamps, d_durations, d_confidences, d_counts, window_range, splice_safe=None, case_canon=None, vocab=None,
                      frame_seconds=None, overlap_seconds=None, capacities=None, ctx: L.Context | None = None, ordered: bool = True) -> MergedWindows:
    """fa_tdt_merge_windows_dev on the torch tensors the greedy walk left on the device (tdt_decode_tables / tdt_decode_logits' o_tok,
    o_time, o_dur [windows, max_out] int32, o_conf float32, o_cnt [windows] int32).  The merged streams stay on the device (flat torch
    tensors); ranges, counts, statuses and routes are host arrays.  Without `capacities` every slice gets the bound that holds for any
    counts, max_out * (2 * windows - 1) tokens: pass merge_capacity of the counts where they are known."""
    import torch
    for t, dt in ((d_tokens, torch.int32), (d_timestamps, torch.int32), (d_durations, torch.int32), (d_confidences, torch.float32), (d_counts, torch.int32)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise _invalid("the window arrays must be contiguous int32 / float32 tensors on the device")
    if d_tokens.dim() != 2 or any(t.shape != d_tokens.shape for t in (d_timestamps, d_durations, d_confidences)) or d_counts.shape != (d_tokens.shape[0],):
        raise _invalid("the window arrays are [windows, max_out] and the counts [windows]")
    windows, max_out = d_tokens.shape
    s, c, vocab = _tables(splice_safe, case_canon, vocab)
    window_range, out_range = _ranges(window_range, windows, capacities, np.full(windows, max_out, np.int64))
    n, total = window_range.size - 1, int(out_range[-1])
    dev = d_tokens.device
    o_tok, o_time, o_dur = (torch.zeros(total, dtype=torch.int32, device=dev) for _ in range(3))
    o_conf = torch.zeros(total, dtype=torch.float32, device=dev)
    o_cnt, o_st, routes = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(windows, MERGE_NO_SEAM, np.int32)
    if n == 0:
        return MergedWindows(o_tok, o_time, o_dur, o_conf, out_range, o_cnt, o_st, routes)
    cfg = _config(frame_seconds, overlap_seconds)
    ctx = ctx or L.default_context(dev.index)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with ctx.torch_ordered(ordered):
        ctx.check(L.lib().fa_tdt_merge_windows_dev(ctx.handle, C.byref(cfg), p(d_tokens), p(d_timestamps), p(d_durations), p(d_confidences), p(d_counts), max_out,
                                                   _ptr(window_range), n, _ptr(s), _ptr(c), vocab, p(o_tok), p(o_time), p(o_dur), p(o_conf), _ptr(out_range),
                                                   _ptr(o_cnt), _ptr(o_st), _ptr(routes)), "fa_tdt_merge_windows_dev")
    return MergedWindows(o_tok, o_time, o_dur, o_conf, out_range, o_cnt, o_st, routes)
