"""The batches the seam-merge tests share (tests/test_tdt_merge_cpu.py, test_tdt_merge_emul.py, test_gpu_tdt_merge.py): recordings as
lists of windows of (id, timestamp, duration, confidence) tokens, the tables of one call, and how a batch is laid out for the C ABI.
What each batch is for is said at its function; tests/test_tdt_merge_cpu.py asserts, on the restatement alone, that the batches reach
the routes they are meant to reach."""
from collections import namedtuple

import numpy as np

import tdt_merge_restatement as R

# recs: [windows]; safe / canon: a set / dict or None; caps: tokens per output slice, None = the safe bound; counts: {(rec, window):
# count the window reports}, where it is not the number of tokens it holds
Batch = namedtuple("Batch", "name recs safe canon vocab overlap caps counts max_out", defaults=(None, None, None))
LDS_SIDE = 128          # csrc/tdt_merge_core.h: kLdsSide
SMALL_LDS_SIDE = 4      # what the tests lower it to (FA_TDT_MERGE_LDS_SIDE)


def tok(i, ts, dur=1, conf=None):
    return (int(i), int(ts), int(dur), float(np.float32(0.5 + (ts % 7) / 16.0 if conf is None else conf)))


def seq(ids, ts0, step=1):
    return [tok(i, ts0 + k * step) for k, i in enumerate(ids)]


def pinned_batches():
    """The reference's 17 cases as two-window recordings, in two calls: the cases without a safe set (nil), and the others with every
    case's ids moved to a range of their own (case i: + 1024 i), so that one safe table and one case table serve them all; a case
    without a case table has no entries there, which matches like nil.  Returns [(batch, expected ids per recording)]."""
    nil, tabled, want_nil, want_tabled, safe, canon = [], [], [], [], set(), {}
    for i, (_, left, right, s, c, want) in enumerate(R.PINNED):
        if s is None:
            assert c is None
            nil.append([left, right])
            want_nil.append(want)
            continue
        off = 1024 * (len(tabled) + 1)
        move = lambda w: [(t[0] + off,) + t[1:] for t in w]   # noqa: E731
        tabled.append([move(left), move(right)])
        want_tabled.append([x + off for x in want])
        safe |= {x + off for x in s}
        canon.update({k + off: v + off for k, v in (c or {}).items()})
    vocab = 1024 * (len(tabled) + 2)
    return [(Batch("pinned-nil", nil, None, None, R.PINNED_VOCAB, R.OVERLAP), want_nil), (Batch("pinned-tables", tabled, safe, canon, vocab, R.OVERLAP), want_tabled)]


def boundary_batch(n=2048):
    """Where the fp64 expressions round: for every a, a left token at a against a right window at a + 1 (a * frame + frame <= (a + 1) *
    frame fails for 720 of the first 4096 a, and a fused multiply-add flips each of them); left tokens 25, 26 and 27 frames below the
    right start (26 is the filter's edge: the side's length decides minimumPairs, hence contiguous or LCS); right tokens 25, 26 and 27
    above the left end (the second right token decides between the matcher and the midpoint); matches 12 and 13 frames apart."""
    recs = []
    for a in range(n):
        s, e = a + 30, a + 3
        recs.append([[tok(1, a)], [tok(2, a + 1)]])
        recs.append([[tok(11, s - 27), tok(12, s - 26), tok(13, s - 25), tok(4, s), tok(5, s + 1)], [tok(4, s), tok(9, s + 1), tok(6, s + 2)]])
        recs.append([[tok(11, s - 27), tok(12, s - 26), tok(13, s - 25), tok(7, s - 1), tok(4, s), tok(5, s + 1)], [tok(4, s), tok(5, s + 1), tok(6, s + 2)]])
        for d in (25, 26, 27):
            recs.append([[tok(1, e - 1), tok(2, e)], [tok(2, e), tok(3, e + d)]])
        for d in (12, 13):
            recs.append([[tok(1, a), tok(2, a + 13)], [tok(1, a + d), tok(3, a + 14)]])
    return Batch("boundaries", recs, None, None, 16, R.OVERLAP)


def side_batch():
    """Overlap sides of 1, 2, 63, 64, 65 and 130 tokens (one strip of the wavefront, its edges, two strips and a rest; 130 is beyond
    the LDS limit), in both orders, and of SMALL_LDS_SIDE + 1 for the lowered limit: every token of both windows lies in the overlap.
    Per shape one pair that shares most of its tokens (runs) and one over three ids (a dense LCS table with many ties)."""
    rng = np.random.default_rng(7)
    sizes = [1, 2, 63, 64, 65, 130, SMALL_LDS_SIDE + 1]
    shapes = [(a, b) for a in sizes for b in (2, a)] + [(2, a) for a in sizes] + [(1, 5), (5, 1), (130, 65), (65, 130)]
    recs = []
    for nl, nr in shapes:
        base = rng.integers(0, 50, max(nl, nr) + 3)
        ts_l, ts_r = np.sort(rng.integers(100, 110, nl)), np.sort(rng.integers(100, 110, nr))
        left = [tok(base[k], ts_l[k]) for k in range(nl)]
        right = [tok(base[k + 1] if rng.random() > 0.1 else 77, ts_r[k]) for k in range(nr)]
        recs.append([left, right])
        recs.append([[tok(rng.integers(0, 3), ts_l[k]) for k in range(nl)], [tok(rng.integers(0, 3), ts_r[k]) for k in range(nr)]])
    return Batch("sides", recs, {i for i in range(100) if i % 3}, None, 100, R.OVERLAP)


def edge_batch():
    """Strategy edges: two equal longest runs (the first in row-major order wins: the other would keep five tokens); a run of exactly
    minimumPairs and of one less; an LCS whose walk back meets dp[i-1][j] == dp[i][j-1]; an LCS without a match (midpoint)."""
    A, B, C, D, E, F, X, Y = range(1, 9)
    recs = [
        [seq([A, B, X, A, B], 100), seq([A, B], 102)],
        [seq([A, B, C, X, Y, X], 100), seq([A, B, C, D], 101)],                # six left tokens: minimumPairs 3, run 3
        [seq([A, B, Y, X, Y, X], 100), seq([A, B, C, D], 101)],                # run 2: LCS
        [seq([A, B, C, D], 100), seq([B, A, D, C], 100)],                      # ties in the walk back
        [seq([A, B, A, B, A, B], 100), seq([B, X, A, Y, B, X], 100)],
        [seq([A, B, C], 100), seq([D, E, F], 100)],                            # nothing matches
    ]
    return Batch("edges", recs, None, None, 16, R.OVERLAP)


def splice_batches():
    """The tail routes with a safe set (ids 1-9 are continuation pieces, 10 and above start a word), then the same recordings with an
    all-zero table (the empty set), with nil, and the case twins (20 / 21) with and without their table."""
    c1, c2, c3, c4 = 1, 2, 3, 4
    S, T, U, V = 10, 11, 12, 13
    recs = [
        [seq([S, T, c1, c2], 100), seq([U, c1, c3, V], 101)],                  # right's word adopted
        [seq([S, T, c1, c2], 100), seq([c1, c3, V], 102)],                     # right begins mid-word: left keeps its word
        [seq([S, T, c1], 100), seq([c1, c3, c4], 102)],                        # the tail has no safe piece: verbatim
        [seq([c4, c1], 100), seq([S, c1, c3], 100)],                           # popSeamWord finds nothing
        [seq([S, T, c1, c2, c3], 100), seq([c1, U, V], 102)],                  # the tail starts a word: untouched
        [seq([S, 20, T], 100), seq([S, 21, T, U], 100)],                       # case twins
        [seq([S, T, c1, c2, c3, c4, U], 100), seq([c1, c2], 102)],             # right ends at the anchor: left's rest is dropped
    ]
    safe, canon = set(range(10, 32)), {20: 20, 21: 20}
    return [Batch("splice-safe-canon", recs, safe, canon, 32, R.OVERLAP), Batch("splice-safe", recs, safe, None, 32, R.OVERLAP),
            Batch("splice-empty-set", recs, set(), None, 32, R.OVERLAP), Batch("splice-nil", recs, None, None, 32, R.OVERLAP),
            Batch("splice-no-vocabulary", recs, set(), {}, 0, R.OVERLAP)]


MAX_OUT_FOLD = 40


def fold_batch():
    """Folds in which a seam works on what the seams before it left: windows of 60 frames every 20 frames (three windows over every
    frame), with noise, so that the merged stream's timestamps step back before the clamp; windows without tokens first, in the middle
    and throughout; recordings of one window and of none; a window that reports more tokens than max_out."""
    rng = np.random.default_rng(11)
    safe, _ = R.fuzz_tables(40)
    recs = [R.fuzz_recording(rng, 60, 40, 40, noise, 8, density=0.3) for noise in (0.0, 0.05, 0.3, 0.3, 0.3, 0.3)]
    w = R.fuzz_recording(rng, 60, 40, 40, 0.05, 5, density=0.3)
    recs += [[[]] + w, w[:2] + [[]] + w[2:], [[], [], []], [w[0]], [], [[]], w[:1] + [[], []] + w[1:]]
    full = [tok(rng.integers(0, 40), 200 + k // 2) for k in range(MAX_OUT_FOLD)]
    recs.append([w[0], full, seq(rng.integers(0, 40, 6), 215)])
    recs = [[x[:MAX_OUT_FOLD] for x in rec] for rec in recs]
    counts = {(len(recs) - 1, 1): MAX_OUT_FOLD + 5}
    return Batch("folds", recs, safe, None, 40, 40 * R.FRAME, None, counts, MAX_OUT_FOLD)


def tight_batch():
    """Three copies of one recording; the middle one's slice is one token short of what its fold needs at its longest."""
    rng = np.random.default_rng(5)
    rec = R.fuzz_recording(rng, 60, 25, 40, 0.3, 5, density=0.4)
    safe, canon = R.fuzz_tables(40)
    need = fold_peak(rec, safe, canon, R.OVERLAP)
    return Batch("tight", [rec, rec, rec], safe, canon, 40, R.OVERLAP, [need, need - 1, need])


def fold_peak(windows, safe, canon, overlap):
    """The longest the merged stream ever is while the recording is folded."""
    merged, peak = list(windows[0]), len(windows[0])
    for w in windows[1:]:
        log = R.Log()
        merged = R.merge_chunks(merged, w, safe, canon, overlap, R.FRAME, log)
        peak = max(peak, log.peak)
    return peak


def fuzz_batches():
    """R.fuzz_batch's recordings, one call per (tables, vocabulary, overlap)."""
    groups = {}
    for wins, s, c, vocab, ov in R.fuzz_batch():
        key = (s is not None, c is not None, vocab, ov)
        groups.setdefault(key, (s, c, []))[2].append(wins)
    return [Batch(f"fuzz-{k}", recs, s, c, key[2], key[3]) for k, (key, (s, c, recs)) in enumerate(sorted(groups.items(), key=lambda kv: str(kv[0])))]


def all_batches():
    return [b for b, _ in pinned_batches()] + [boundary_batch(), side_batch(), edge_batch()] + splice_batches() + [fold_batch(), tight_batch()] + fuzz_batches()


_expected = {}


def expected(batch):
    """[(tokens, status, routes)] of the restatement, computed once per batch."""
    if batch.name not in _expected:
        caps = batch.caps or [None] * len(batch.recs)
        _expected[batch.name] = [R.fold(rec, batch.safe, batch.canon, batch.overlap, R.FRAME, cap) for rec, cap in zip(batch.recs, caps)]
    return _expected[batch.name]


Packed = namedtuple("Packed", "tok time dur conf counts window_range caps safe canon max_out")


def pack(batch):
    """The batch as the C ABI takes it: [windows, max_out] arrays (cells behind a window's tokens hold a poison), counts, window_range,
    capacities and the two tables."""
    wins = [w for rec in batch.recs for w in rec]
    max_out = batch.max_out or max([len(w) for w in wins] + [1])
    tok_, time_, dur_ = (np.full((len(wins), max_out), -7, np.int32) for _ in range(3))
    conf_ = np.full((len(wins), max_out), -7.0, np.float32)
    counts = np.zeros(len(wins), np.int32)
    at = 0
    for r, rec in enumerate(batch.recs):
        for k, w in enumerate(rec):
            a = R.as_arrays(w)
            tok_[at, :len(w)], time_[at, :len(w)], dur_[at, :len(w)], conf_[at, :len(w)] = a
            counts[at] = (batch.counts or {}).get((r, k), len(w))
            at += 1
    window_range = np.concatenate([[0], np.cumsum([len(rec) for rec in batch.recs])]).astype(np.int64)
    caps = np.asarray(batch.caps if batch.caps else [R.safe_capacity(rec) for rec in batch.recs], np.int64)
    safe, canon = R.tables(batch.safe, batch.canon, batch.vocab)
    return Packed(tok_, time_, dur_, conf_, counts, window_range, caps, safe, canon, max_out)


def flatten(results):
    """The restatement's answers in the shape of the device's: per recording (ids, timestamps, durations, confidences), statuses, routes."""
    streams = [R.as_arrays(toks) for toks, _, _ in results]
    statuses = np.array([st for _, st, _ in results], np.int32)
    routes = np.array([x for _, _, rt in results for x in rt], np.int32)
    return streams, statuses, routes
