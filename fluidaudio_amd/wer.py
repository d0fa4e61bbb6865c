"""Word and character error rates (csrc/wer.hip, csrc/wer_host.hip): WERCalculator.editDistance with its insertion / deletion / substitution breakdown
(reference: Sources/FluidAudioCLI/Utils/WERCalculator.swift:178-239), StringUtils.levenshteinDistance (Sources/FluidAudio/Shared/
StringUtils.swift:12-40) and the metrics the ASR benchmarks print from them (WERCalculator.swift:7-56), batched over (hypothesis,
reference) pairs: one device call for a whole corpus, words and characters together.

Words and characters are numbered here, by first appearance; the device compares integers; the rates are formed here with the
reference's expressions.  OUT OF SCOPE: TextNormalizer (English tables and string logic), the split at whitespace, grapheme
segmentation and Swift's canonical-equivalence `==` — the caller passes NORMALISED text: words separated by single blanks, and strings
whose characters are compared code point by code point."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from . import _args as A, _lib as L

EDIT_COUNTS_DTYPE = np.dtype(L.EditCounts)
WERMetrics = namedtuple("WERMetrics", "wer insertions deletions substitutions totalWords")                                  # :10
WERAndCER = namedtuple("WERAndCER", "wer cer insertions deletions substitutions totalWords totalCharacters")                # :28-31
# the corpus sums as the benchmarks aggregate them (FluidAudioCLI/Commands/ASR/Parakeet/Unified/UnifiedBenchmark.swift:169-187):
# Double(sum of errors) / Double(sum of reference words), 0 for a corpus without reference words
CorpusErrorRate = namedtuple("CorpusErrorRate", "word_errors ref_words wer char_errors ref_chars cer")


_invalid = functools.partial(A.invalid, "edit_distance_batch")


def _ids(seq) -> np.ndarray:
    """One side of a pair as int32; every int32 value is a symbol."""
    a = np.asarray(seq)
    if a.size == 0:
        return np.zeros(0, np.int32)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise _invalid("a sequence must be a one-dimensional array of integers")
    if a.dtype != np.int32 and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise _invalid("a symbol does not fit int32")
    return a.astype(np.int32, copy=False)


def _pack(seqs):
    return A.ragged(seqs, None, np.int32)


def _run_edit(where, ctx, hyp, hyp_range, ref, ref_range, ordered) -> np.ndarray:
    """The body of edit_distance_batch and edit_distance_batch_dev: the symbols are numpy arrays or device tensors, the ranges host arrays."""
    n = hyp_range.size - 1
    out = np.zeros(n, EDIT_COUNTS_DTYPE)
    if n:
        ctx = A.context_beside(ctx, hyp)
        with ctx.torch_ordered(ordered):
            ctx.check(getattr(L.lib(), where)(ctx.handle, A.ptr(hyp), hyp_range.ctypes.data, A.ptr(ref), ref_range.ctypes.data, n, out.ctypes.data), where)
    return out


def edit_distance_batch(pairs, ctx: L.Context | None = None) -> np.ndarray:
    """WERCalculator.editDistance(hyp, ref) for every (hyp ids, ref ids) pair, in one device call (fa_edit_distance_batch).  Returns a
    structured array of EDIT_COUNTS_DTYPE in input order.  The argument contract is answered here, before any context is looked for."""
    sides = []
    for p in pairs:
        if len(p) != 2:
            raise _invalid("a pair is (hypothesis, reference)")
        sides.append((_ids(p[0]), _ids(p[1])))
    return _run_edit("fa_edit_distance_batch", ctx, *_pack([h for h, _ in sides]), *_pack([r for _, r in sides]), False)


def edit_distance_batch_dev(hyp, hyp_range, ref, ref_range, ctx: L.Context | None = None, ordered: bool = True) -> np.ndarray:
    """The same on symbols that are already on the device (fa_edit_distance_batch_dev): hyp and ref are contiguous int32 torch tensors on
    the context's device — e.g. the ids a decoder left there —, pair k's symbols are hyp[hyp_range[k]:hyp_range[k + 1]] and
    ref[ref_range[k]:ref_range[k + 1]]; the ranges are host integers."""
    hyp_range, ref_range = np.ascontiguousarray(hyp_range, np.int64), np.ascontiguousarray(ref_range, np.int64)
    if hyp_range.ndim != 1 or hyp_range.shape != ref_range.shape or hyp_range.size < 1:
        raise _invalid("the ranges hold n_pairs + 1 entries each")
    for t, rng in ((hyp, hyp_range), (ref, ref_range)):
        if not A.is_dev(t, "int32", 1):
            raise _invalid("the symbols must be contiguous one-dimensional int32 tensors on the device")
        if (np.diff(rng) < 0).any() or rng[0] < 0 or rng[-1] > t.numel():
            raise _invalid("a range does not ascend inside its tensor")
    return _run_edit("fa_edit_distance_batch_dev", ctx, hyp, hyp_range, ref, ref_range, ordered)


def _number(seqs):
    """Each sequence of hashable symbols as int32 ids, numbered by first appearance over the whole call."""
    idx = {}
    return [np.fromiter((idx.setdefault(x, len(idx)) for x in s), np.int32, len(s)) for s in seqs]


def levenshtein_distance(a, b, ctx: L.Context | None = None) -> int:
    """StringUtils.levenshteinDistance(a, b) (:12-40) for two sequences of equatable (here: hashable) elements, or two strings compared
    character by character."""
    x, y = _number([list(a), list(b)])
    return int(edit_distance_batch([(x, y)], ctx)["total"][0])


def _rate(errors: int, count: int) -> float:
    return 0.0 if count == 0 else float(errors) / float(count)   # :19, :40, :45


def wer_metrics_batch(pairs, ctx: L.Context | None = None):
    """calculateWERMetrics (:7-22) behind the normalizer and the split, for every (hypothesis words, reference words) pair of word lists.
    Returns ([WERMetrics], CorpusErrorRate); the character fields of the corpus sums are 0."""
    pairs = [(list(h), list(r)) for h, r in pairs]
    ids = _number([s for p in pairs for s in p])
    counts = edit_distance_batch(list(zip(ids[0::2], ids[1::2])), ctx)
    out = [WERMetrics(_rate(int(c["total"]), int(c["ref_len"])), int(c["insertions"]), int(c["deletions"]), int(c["substitutions"]), int(c["ref_len"]))
           for c in counts]
    errors, words = int(counts["total"].astype(np.int64).sum()), int(counts["ref_len"].astype(np.int64).sum())
    return out, CorpusErrorRate(errors, words, _rate(errors, words), 0, 0, 0.0)


def wer_and_cer_batch(pairs, ctx: L.Context | None = None):
    """calculateWERAndCER (:25-56) behind the normalizer, for every (hypothesis, reference) pair of NORMALISED strings: the words are
    what single blanks separate, the characters are the code points of the string without its blanks.  The word and the character
    sequences of the whole call go to the device together.  Returns ([WERAndCER], CorpusErrorRate)."""
    pairs = [(str(h), str(r)) for h, r in pairs]
    n = len(pairs)
    words = _number([[w for w in s.split(" ") if w] for p in pairs for s in p])
    chars = [np.frombuffer(s.replace(" ", "").encode("utf-32-le"), np.uint32).astype(np.int32) for p in pairs for s in p]
    counts = edit_distance_batch(list(zip(words[0::2], words[1::2])) + list(zip(chars[0::2], chars[1::2])), ctx)
    w, c = counts[:n], counts[n:]
    out = [WERAndCER(_rate(int(w[k]["total"]), int(w[k]["ref_len"])), _rate(int(c[k]["total"]), int(c[k]["ref_len"])), int(w[k]["insertions"]),
                     int(w[k]["deletions"]), int(w[k]["substitutions"]), int(w[k]["ref_len"]), int(c[k]["ref_len"])) for k in range(n)]
    we, wn = int(w["total"].astype(np.int64).sum()), int(w["ref_len"].astype(np.int64).sum())
    ce, cn = int(c["total"].astype(np.int64).sum()), int(c["ref_len"].astype(np.int64).sum())
    return out, CorpusErrorRate(we, wn, _rate(we, wn), ce, cn, _rate(ce, cn))
