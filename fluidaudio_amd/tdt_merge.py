"""TDT long-form chunk merging (csrc/tdt_merge.hip): the fold of ChunkProcessor.mergeChunks over a recording's overlapping windows and
enforceMonotonicTimestamps (reference: Sources/FluidAudio/ASR/Parakeet/SlidingWindow/TDT/ChunkProcessor.swift:843-855, 952-1219;
SequenceMatcher.swift:127-225), batched over recordings in one device call.  The merged streams are the reference's bit for bit.

The vocabulary stays the caller's: ``splice_safe_table`` and ``case_canon_table`` turn the reference's spliceSafeTokenIds set and
caseVariantCanonicalIds map into the tables the C ABI takes.  OUT OF SCOPE: collapseSeamWordDuplicates (Unicode strings),
repairSeamGaps (needs the networks), the planning of chunk starts and the streaming removeDuplicateTokenSequence."""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from . import _args as A, _lib as L

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


_invalid = functools.partial(A.invalid, "merge_windows")


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


def _run_merge(where, ctx, arrays, count_bound, window_range, splice_safe, case_canon, vocab, frame_seconds, overlap_seconds, capacities, ordered) -> MergedWindows:
    """The body of merge_windows and merge_windows_dev: `arrays` are the four window arrays and the counts, checked, as numpy arrays or as
    device tensors; the merged streams come back beside them.  count_bound: per window, the most tokens it can hold."""
    windows, max_out = arrays[0].shape
    s, c, vocab = _tables(splice_safe, case_canon, vocab)
    window_range, out_range = _ranges(window_range, windows, capacities, count_bound)
    n, total = window_range.size - 1, int(out_range[-1])
    merged = [A.beside(arrays[0], total, dtype) for dtype in ("int32", "int32", "int32", "float32")]
    o_cnt, o_st, routes = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(windows, MERGE_NO_SEAM, np.int32)
    if n:
        cfg = _config(frame_seconds, overlap_seconds)
        ctx = A.context_beside(ctx, arrays[0])
        with ctx.torch_ordered(ordered):
            ctx.check(getattr(L.lib(), where)(ctx.handle, C.byref(cfg), *[A.ptr(a) for a in arrays], max_out, A.ptr(window_range), n, A.ptr(s), A.ptr(c), vocab,
                                              *[A.ptr(a) for a in merged], A.ptr(out_range), A.ptr(o_cnt), A.ptr(o_st), A.ptr(routes)), where)
    return MergedWindows(*merged, out_range, o_cnt, o_st, routes)


def merge_windows(tokens, timestamps, durations, confidences, counts, window_range, splice_safe=None, case_canon=None, vocab=None,
                  frame_seconds=None, overlap_seconds=None, capacities=None, ctx: L.Context | None = None) -> MergedWindows:
    """fa_tdt_merge_windows on host arrays: the four window arrays [windows, max_out] and counts [windows] as the greedy walk writes them
    (global timestamps), window_range [n_recordings + 1].  capacities: tokens per output slice (default: merge_capacity)."""
    tok, tim, dur = (np.ascontiguousarray(a, np.int32) for a in (tokens, timestamps, durations))
    conf, cnt = np.ascontiguousarray(confidences, np.float32), np.ascontiguousarray(counts, np.int32)
    if tok.ndim != 2 or tim.shape != tok.shape or dur.shape != tok.shape or conf.shape != tok.shape or cnt.shape != (tok.shape[0],):
        raise _invalid("the window arrays are [windows, max_out] and the counts [windows]")
    return _run_merge("fa_tdt_merge_windows", ctx, (tok, tim, dur, conf, cnt), np.clip(cnt, 0, tok.shape[1]), window_range, splice_safe, case_canon, vocab,
                      frame_seconds, overlap_seconds, capacities, False)


def merge_windows_dev(d_tokens, d_timestamps, d_durations, d_confidences, d_counts, window_range, splice_safe=None, case_canon=None, vocab=None,
                      frame_seconds=None, overlap_seconds=None, capacities=None, ctx: L.Context | None = None, ordered: bool = True) -> MergedWindows:
    """fa_tdt_merge_windows_dev on the torch tensors the greedy walk left on the device (tdt_decode_tables / tdt_decode_logits' o_tok,
    o_time, o_dur [windows, max_out] int32, o_conf float32, o_cnt [windows] int32).  The merged streams stay on the device (flat torch
    tensors); ranges, counts, statuses and routes are host arrays.  Without `capacities` every slice gets the bound that holds for any
    counts, max_out * (2 * windows - 1) tokens: pass merge_capacity of the counts where they are known."""
    for t, dt in ((d_tokens, "int32"), (d_timestamps, "int32"), (d_durations, "int32"), (d_confidences, "float32"), (d_counts, "int32")):
        if not A.is_dev(t, dt):
            raise _invalid("the window arrays must be contiguous int32 / float32 tensors on the device")
    if d_tokens.dim() != 2 or any(t.shape != d_tokens.shape for t in (d_timestamps, d_durations, d_confidences)) or d_counts.shape != (d_tokens.shape[0],):
        raise _invalid("the window arrays are [windows, max_out] and the counts [windows]")
    windows, max_out = d_tokens.shape
    return _run_merge("fa_tdt_merge_windows_dev", ctx, (d_tokens, d_timestamps, d_durations, d_confidences, d_counts), np.full(windows, max_out, np.int64), window_range,
                      splice_safe, case_canon, vocab, frame_seconds, overlap_seconds, capacities, ordered)
