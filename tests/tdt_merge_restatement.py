"""A plain restatement of the TDT long-form seam merge, with a route log per seam: ChunkProcessor.mergeChunks and what it calls
(Sources/FluidAudio/ASR/Parakeet/SlidingWindow/TDT/ChunkProcessor.swift:952-1219), SequenceMatcher.findLongestCommonSubsequence and
findContiguousMatches (Sources/FluidAudio/ASR/Parakeet/TokenDeduplication/SequenceMatcher.swift:127-225) and
enforceMonotonicTimestamps (ChunkProcessor.swift:843-855).  Lists, full tables, no shortcut: what csrc/tdt_merge_core.h is compared
with.  Python's float is the reference's Double and nothing here is fused.

A token is (id, timestamp, duration, confidence).  The pinned cases below are the reference's literal mergeTokenWindowsForTesting cases
(ChunkProcessorTests.swift:520-786, 837-880, ChunkProcessorSeamResidualTests.swift:104-250): inputs, the safe sets and case-twin
tables of their vocabularies, and the expected token lists."""
from __future__ import annotations

import numpy as np

FRAME = float(1280) / float(16000)     # ASRConstants.secondsPerEncoderFrame
OVERLAP = 2.0                          # ChunkProcessor.overlapSeconds

# a seam's route: base strategy | tail handling << 4 (include/fluidaudio_hip.h: FA_TDT_MERGE_*)
EMPTY, CONCAT, CONTIGUOUS, LCS, MIDPOINT = 0, 1, 2, 3, 4
TAIL_VERBATIM, TAIL_ADOPT_RIGHT, TAIL_KEEP_LEFT = 0, 1, 2
NO_SEAM = -1
SUCCESS, OUTPUT_TOO_SMALL = 0, 3


def route(base, tail=TAIL_VERBATIM):
    return base | (tail << 4)


def ids_match(a, b, canon):                                             # tokenIdsMatch :1068-1074
    if a == b:
        return True
    if canon is None or a not in canon or b not in canon:
        return False
    return canon[a] == canon[b]


def contiguous_matches(left, right, match):                             # SequenceMatcher.swift:188-225
    best = []
    for i in range(len(left)):
        for j in range(len(right)):
            if match(left[i], right[j]):
                cur, k, l = [], i, j
                while k < len(left) and l < len(right) and match(left[k], right[l]):
                    cur.append((k, l))
                    k += 1
                    l += 1
                if len(cur) > len(best):
                    best = cur
    return best


def lcs_matches(left, right, match):                                    # SequenceMatcher.swift:127-172
    m, n = len(left), len(right)
    dp = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            dp[i][j] = dp[i - 1][j - 1] + 1 if match(left[i - 1], right[j - 1]) else max(dp[i - 1][j], dp[i][j - 1])
    out, i, j = [], m, n
    while i > 0 and j > 0:
        if match(left[i - 1], right[j - 1]):
            out.append((i - 1, j - 1))
            i -= 1
            j -= 1
        elif dp[i - 1][j] > dp[i][j - 1]:
            i -= 1
        else:
            j -= 1
    return out[::-1]


class Log:
    """What one seam did: its route and the longest the result ever was while it was built (what the output slice has to hold)."""
    def __init__(self):
        self.route, self.peak = NO_SEAM, 0


def merge_by_midpoint(left, right, left_end, right_start, frame, safe, log):          # :1186-1219
    cutoff = (left_end + right_start) / 2
    le = next((i for i, t in enumerate(left) if float(t[1]) * frame >= cutoff), len(left))
    rs = next((i for i, t in enumerate(right) if float(t[1]) * frame >= cutoff), len(right))
    if safe is not None:
        if le > 0:
            while le < len(left) and left[le][0] not in safe:
                le += 1
        scan = rs
        while scan < len(right) and right[scan][0] not in safe:
            scan += 1
        if scan < len(right):
            rs = scan
    log.route = route(MIDPOINT)
    out = left[:le] + right[rs:]
    log.peak = len(out)
    return out


def merge_using_matches(pairs, o_left, o_right, left, right, safe, log, base):        # :1076-1153
    li = [o_left[a][0] for a, _ in pairs]
    ri = [o_right[b][0] for _, b in pairs]
    result = list(left[:li[0]])
    for k in range(len(pairs)):
        result.append(left[li[k]])
        if k == len(pairs) - 1:
            continue
        gap_l = left[li[k] + 1:li[k + 1]] if li[k + 1] > li[k] + 1 else []
        gap_r = right[ri[k] + 1:ri[k + 1]] if ri[k + 1] > ri[k] + 1 else []
        result += gap_r if len(gap_r) > len(gap_l) else gap_l
    peak, tail_route = len(result), TAIL_VERBATIM
    if ri[-1] + 1 < len(right):
        tail = right[ri[-1] + 1:]
        if safe is not None and tail[0][0] not in safe:
            word_start = next((i for i in range(ri[-1], -1, -1) if right[i][0] in safe), None)          # wordInitialIndex
            cursor = None if word_start is None else next((c for c in range(len(result) - 1, -1, -1) if result[c][0] in safe), None)   # popSeamWord
            if cursor is not None:
                tail_route = TAIL_ADOPT_RIGHT
                result = result[:cursor] + right[word_start:]
            else:
                tail_route = TAIL_KEEP_LEFT
                c = li[-1] + 1
                while c < len(left) and left[c][0] not in safe:
                    result.append(left[c])
                    c += 1
                resume = next((i for i, t in enumerate(tail) if t[0] in safe), None)
                result += tail if resume is None else tail[resume:]
        else:
            result += tail
    log.route, log.peak = route(base, tail_route), max(peak, len(result))
    return result


def merge_chunks(left, right, safe=None, canon=None, overlap=OVERLAP, frame=FRAME, log=None):          # :952-1051
    log = log if log is not None else Log()
    left, right = list(left), list(right)
    if not left or not right:
        log.route, log.peak = route(EMPTY), len(left) + len(right)
        return right if not left else left
    half = overlap / 2
    start = lambda t: float(t[1]) * frame            # noqa: E731
    left_end = start(left[-1]) + frame
    right_start = start(right[0])
    if left_end <= right_start:
        log.route, log.peak = route(CONCAT), len(left) + len(right)
        return left + right
    o_left = [(i, t, start(t)) for i, t in enumerate(left) if start(t) + frame > right_start - overlap]
    o_right = [(i, t, start(t)) for i, t in enumerate(right) if start(t) < left_end + overlap]
    if len(o_left) < 2 or len(o_right) < 2:
        return merge_by_midpoint(left, right, left_end, right_start, frame, safe, log)
    minimum = max(len(o_left) // 2, 1)
    match = lambda l, r: ids_match(l[1][0], r[1][0], canon) and abs(l[2] - r[2]) < half   # noqa: E731
    pairs = contiguous_matches(o_left, o_right, match)
    if len(pairs) >= minimum:
        return merge_using_matches(pairs, o_left, o_right, left, right, safe, log, CONTIGUOUS)
    pairs = lcs_matches(o_left, o_right, match)
    if not pairs:
        return merge_by_midpoint(left, right, left_end, right_start, frame, safe, log)
    return merge_using_matches(pairs, o_left, o_right, left, right, safe, log, LCS)


def enforce_monotonic(tokens):                                          # :843-855
    out, last = [], None
    for t in tokens:
        if last is not None and t[1] < last:
            t = (t[0], last, t[2], t[3])
        else:
            last = t[1]
        out.append(t)
    return out


def fold(windows, safe=None, canon=None, overlap=OVERLAP, frame=FRAME, capacity=None):
    """One recording: merged = w[0]; merged = mergeChunks(merged, w[k]) ...; the clamp.  Returns (tokens, status, routes): a route per
    window, NO_SEAM for the first.  With a capacity, a seam whose result is ever longer than it ends the recording: OUTPUT_TOO_SMALL,
    no tokens, NO_SEAM for that seam and the ones behind it."""
    routes = [NO_SEAM] * len(windows)
    if not windows:
        return [], SUCCESS, routes
    merged = list(windows[0])
    if capacity is not None and len(merged) > capacity:
        return [], OUTPUT_TOO_SMALL, routes
    for k in range(1, len(windows)):
        log = Log()
        merged = merge_chunks(merged, windows[k], safe, canon, overlap, frame, log)
        if capacity is not None and log.peak > capacity:
            return [], OUTPUT_TOO_SMALL, routes
        routes[k] = log.route
    return enforce_monotonic(merged), SUCCESS, routes


def safe_capacity(windows):
    """|w0| + 2 sum |wk|: a merge emits a right token at most twice (a right-side gap adopted, then the seam word spliced again from its start)."""
    return sum(len(w) for w in windows) * 2 - (len(windows[0]) if windows else 0)


def tables(safe, canon, vocab):
    """The caller's tables of the C ABI: uint8[vocab] (None: nil) and int32[vocab] with -1 for no entry (None: nil)."""
    s = None
    if safe is not None:
        s = np.zeros(vocab, np.uint8)
        for i in safe:
            if 0 <= i < vocab:
                s[i] = 1
    c = None
    if canon is not None:
        c = np.full(vocab, -1, np.int32)
        for i, v in canon.items():
            if 0 <= i < vocab:
                c[i] = v
    return s, c


# ---------------------------------------------------------------- the reference's 17 literal cases
def _t(*rows):
    return [(int(a), int(b), int(d), float(np.float32(c))) for a, b, c, d in rows]


SPLICE_SAFE = {10, 20, 24, 27, 30, 40, 60}             # spliceTestVocabulary's word-initial pieces (ChunkProcessorTests.swift:616-634, 805)
CASE_SAFE = {10, 11, 20, 21, 30, 40, 50}               # caseTestVocabulary (:811-823): every piece starts a word
CASE_CANON = {10: 10, 11: 10, 20: 20, 21: 20}          # :834
RESIDUAL_SAFE = {1, 300, 320, 330, 424, 511, 601, 690, 640, 724, 727, 730}   # ChunkProcessorSeamResidualTests.swift:35-79

_HELLO_GRE = _t((10, 120, 0.98, 1), (24, 130, 0.97, 1), (25, 131, 0.96, 1), (26, 132, 0.95, 1))
_WOR_LD = _t((10, 120, 0.98, 1), (20, 130, 0.97, 1), (21, 131, 0.96, 1))
_MID_L = _t((10, 120, 0.98, 1), (20, 133, 0.97, 1), (21, 135, 0.96, 1))
_MID_R = _t((60, 134, 0.90, 1), (50, 136, 0.91, 1), (30, 138, 0.97, 1))
_CASE_L = _t((10, 128, 0.98, 1), (30, 130, 0.97, 1), (20, 132, 0.96, 1), (40, 134, 0.95, 1))
_CASE_R = _t((10, 128, 0.98, 1), (30, 130, 0.97, 1), (21, 132, 0.96, 1), (40, 134, 0.95, 1))

# (name, left, right, safe ids or None, case table or None, expected ids)
PINNED = [
    ("gap_same_length_keeps_older",
     _t((100, 120, 0.98, 1), (200, 130, 0.97, 1), (901, 131, 0.30, 1), (300, 132, 0.97, 1)),
     _t((200, 130, 0.97, 1), (902, 131, 0.95, 1), (300, 132, 0.97, 1), (400, 133, 0.98, 1)), None, None, [100, 200, 901, 300, 400]),
    ("leading_gap_same_length",
     _t((100, 120, 0.98, 1), (110, 130, 0.98, 1), (901, 131, 0.30, 1), (300, 132, 0.97, 1)),
     _t((902, 131, 0.95, 1), (300, 132, 0.97, 1), (400, 133, 0.98, 1)), None, None, [100, 110, 901, 300, 400]),
    ("leading_gap_lower_confidence",
     _t((100, 120, 0.98, 1), (901, 131, 0.94, 1), (902, 132, 0.91, 1), (903, 133, 0.92, 1), (300, 134, 0.97, 1)),
     _t((801, 131, 0.49, 1), (802, 132, 0.65, 1), (803, 133, 0.94, 1), (300, 134, 0.97, 1), (400, 135, 0.98, 1)), None, None,
     [100, 901, 902, 903, 300, 400]),
    ("leading_gap_contested_prefix",
     _t((100, 120, 0.98, 1), (901, 130, 0.84, 3), (300, 133, 0.97, 1)),
     _t((902, 131, 0.75, 1), (300, 133, 0.97, 1), (400, 134, 0.98, 1)), None, None, [100, 901, 300, 400]),
    ("tail_adopts_right_segmentation", _HELLO_GRE,
     _t((27, 130, 0.97, 1), (25, 131, 0.96, 1), (28, 132, 0.95, 1), (30, 134, 0.97, 1)), SPLICE_SAFE, None, [10, 27, 25, 28, 30]),
    ("tail_keeps_left_word", _HELLO_GRE,
     _t((25, 131, 0.96, 1), (28, 132, 0.95, 1), (30, 134, 0.97, 1)), SPLICE_SAFE, None, [10, 24, 25, 26, 30]),
    ("tail_legacy_without_vocabulary", _WOR_LD,
     _t((20, 130, 0.97, 1), (22, 131, 0.95, 1), (30, 133, 0.97, 1), (40, 134, 0.98, 1)), None, None, [10, 20, 22, 30, 40]),
    ("tail_word_initial_verbatim", _WOR_LD,
     _t((21, 131, 0.97, 1), (30, 133, 0.97, 1), (40, 134, 0.98, 1)), SPLICE_SAFE, None, [10, 20, 21, 30, 40]),
    ("midpoint_does_not_cut_words", _MID_L, _MID_R, SPLICE_SAFE, None, [10, 20, 21, 30]),
    ("midpoint_legacy_without_vocabulary", _MID_L, _MID_R, None, None, [10, 20, 50, 30]),
    ("case_fold_keeps_left_casing", _CASE_L, _CASE_R, CASE_SAFE, CASE_CANON, [10, 30, 20, 40]),
    ("case_without_fold_keeps_capital", _CASE_L, _CASE_R, CASE_SAFE, None, [10, 30, 21, 40]),
    ("long_seam_word_past_pop_cap",
     _t((1, 90, 0.98, 1), *[(300 + i, 91 + i, 0.97, 1) for i in range(12)], (312, 103, 0.96, 1)),
     _t((320, 99, 0.95, 1), (312, 103, 0.96, 1), (313, 104, 0.95, 1), (330, 105, 0.97, 1)), RESIDUAL_SAFE, None, [1, 320, 312, 313, 330]),
    ("right_window_ends_mid_word",
     _t((1, 120, 0.98, 1), (424, 130, 0.97, 1), (425, 131, 0.96, 1)),
     _t((425, 131, 0.96, 1), (426, 132, 0.95, 1), (427, 133, 0.95, 1)), RESIDUAL_SAFE, None, [1, 424, 425, 426, 427]),
    ("midpoint_without_safe_token_in_right",
     _t((1, 120, 0.98, 1), (511, 140, 0.97, 1)),
     _t((549, 140, 0.90, 1), (550, 141, 0.91, 1), (551, 142, 0.91, 1), (552, 143, 0.91, 1)), RESIDUAL_SAFE, None, [1, 511, 550, 551, 552]),
    ("punctuation_adjacent_seam",
     _t((1, 120, 0.98, 1), (601, 130, 0.97, 1), (602, 131, 0.96, 1)),
     _t((602, 131, 0.96, 1), (690, 132, 0.97, 1), (640, 134, 0.98, 1)), RESIDUAL_SAFE, None, [1, 601, 602, 690, 640]),
    ("short_seam_word_disagreeing_segmentation",
     _t((1, 120, 0.98, 1), (724, 130, 0.97, 1), (725, 131, 0.96, 1), (726, 132, 0.95, 1)),
     _t((727, 130, 0.97, 1), (725, 131, 0.96, 1), (728, 132, 0.95, 1), (730, 134, 0.97, 1)), RESIDUAL_SAFE, None, [1, 727, 725, 728, 730]),
]
PINNED_VOCAB = 1024


# ---------------------------------------------------------------- generated recordings
def fuzz_recording(rng, frames, overlap_frames, vocab, noise, n_windows, density=0.35, disjoint=False, headless=False):
    """A recording as its windows' token lists: one true stream, seen through windows of `frames` frames that overlap by
    `overlap_frames`; each window drops, substitutes, inserts and shifts by one frame with probability `noise` each.  disjoint: the
    windows alternate between two halves of the vocabulary (nothing matches).  headless: a window's first pieces are continuation
    pieces more often (right begins mid-word)."""
    stride = frames - overlap_frames
    total = stride * (n_windows - 1) + frames
    truth = [(int(rng.integers(0, vocab)), t) for t in range(total) if rng.random() < density]
    windows = []
    for k in range(n_windows):
        lo, hi = k * stride, k * stride + frames
        toks = []
        for tok, t in truth:
            if not lo <= t < hi:
                continue
            u = rng.random(4)
            if u[0] < noise:
                continue
            if u[1] < noise:
                tok = int(rng.integers(0, vocab))
            if u[2] < noise:
                toks.append((int(rng.integers(0, vocab)), t, 1, float(np.float32(rng.random()))))
            if u[3] < noise:
                t = min(hi - 1, max(lo, t + (1 if rng.random() < 0.5 else -1)))
            toks.append((tok, t, int(rng.integers(0, 5)), float(np.float32(rng.random()))))
        if disjoint:
            half = max(vocab // 2, 1)
            toks = [((a % half) + (half if k % 2 else 0), b, c, d) for a, b, c, d in toks]
        if headless and toks:
            n_head = int(rng.integers(2, 12))
            toks = [((a - a % 3) % vocab if i < n_head else a, b, c, d) for i, (a, b, c, d) in enumerate(toks)]
        windows.append(toks)
    return windows


def fuzz_tables(vocab):
    """Ids divisible by 3 are continuation pieces; ids 4k + 1 and 4k + 2 are case twins, canonical 4k + 1."""
    safe = {i for i in range(vocab) if i % 3 != 0}
    canon = {}
    for k in range(vocab // 4):
        canon[4 * k + 1] = canon[4 * k + 2] = 4 * k + 1
    return safe, canon


def fuzz_batch(seed=20240613, n=300):
    """About n recordings: (windows, safe, canon, vocab, overlap seconds) each, over windows of 60 or 187 frames, overlaps of 10, 25 or
    40 frames, vocabularies of 6, 40 or 400 ids and noise of 0, 5 or 30 %, with strata for the rare routes."""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n):
        frames = (60, 187)[r % 2]
        ov = (10, 25, 40)[(r // 2) % 3]
        vocab = (6, 40, 400)[(r // 6) % 3]
        noise = (0.0, 0.05, 0.30)[(r // 18) % 3]
        kind = r % 5
        safe, canon = fuzz_tables(vocab)
        mode = (r // 5) % 3                                    # both tables, safe only, neither
        s, c = (safe, canon) if mode == 0 else ((safe, None) if mode == 1 else (None, None))
        density = 0.05 if kind == 4 else 0.35                  # sparse: windows that only touch (concatenated)
        wins = fuzz_recording(rng, frames, ov, vocab, noise, int(rng.integers(2, 7)), density, disjoint=(kind == 3), headless=(kind == 2))
        if kind == 2 or kind == 3:
            s = safe
        out.append((wins, s, c, vocab, ov * FRAME))
    return out


def as_arrays(tokens):
    """(ids, timestamps, durations, confidences) of a token list, in the ABI's types."""
    return (np.array([t[0] for t in tokens], np.int32), np.array([t[1] for t in tokens], np.int32), np.array([t[2] for t in tokens], np.int32),
            np.array([t[3] for t in tokens], np.float32))
