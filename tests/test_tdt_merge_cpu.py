"""The restatement of the TDT seam merge (tests/tdt_merge_restatement.py) on the CPU: it reproduces the reference's 17 literal
mergeTokenWindowsForTesting cases, the documented capacity bound holds, and the shared batches (tests/tdt_merge_cases.py) reach the
routes and edges they are built for — asserted here, on the restatement's log, before any device is asked.  No GPU, no library."""
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_merge_cases as K  # noqa: E402
import tdt_merge_restatement as R  # noqa: E402


def test_the_17_pinned_cases():
    assert len(R.PINNED) == 17
    for name, left, right, safe, canon, want in R.PINNED:
        got = R.merge_chunks(left, right, safe, canon)
        assert [t[0] for t in got] == want, name
        # the merged tokens are the windows' own records
        assert all(t in left or t in right for t in got), name
    # and as the two calls the device tests make of them
    for batch, want in K.pinned_batches():
        assert [[t[0] for t in toks] for toks, _, _ in K.expected(batch)] == want


def seams(batch):
    for rec in batch.recs:
        merged = []
        for k, w in enumerate(rec):
            if k == 0:
                merged = list(w)
                continue
            log, before = R.Log(), len(merged)
            merged = R.merge_chunks(merged, w, batch.safe, batch.canon, batch.overlap, R.FRAME, log)
            yield before, len(w), log


def test_capacity_bound_over_the_fuzz_batch():
    """|merge| <= |left| + 2 |right| at every moment of a seam, hence |w0| + 2 sum |wk| for a recording."""
    routes, tails, n = Counter(), Counter(), 0
    for batch in K.fuzz_batches():
        for left, right, log in seams(batch):
            assert log.peak <= left + 2 * right
            routes[log.route & 15] += 1
            tails[log.route >> 4] += 1
            n += 1
        for rec, (toks, status, _) in zip(batch.recs, K.expected(batch)):
            assert status == R.SUCCESS and len(toks) <= R.safe_capacity(rec)
    assert n > 800
    # the condition of the device's fuzz test: every strategy and both splice repairs at least 20 times
    for base in (R.CONCAT, R.CONTIGUOUS, R.LCS, R.MIDPOINT):
        assert routes[base] >= 20, (base, routes)
    assert tails[R.TAIL_ADOPT_RIGHT] >= 20 and tails[R.TAIL_KEEP_LEFT] >= 20, tails


def test_boundaries_reach_both_sides_of_every_edge():
    b = K.boundary_batch()
    routes = [rt[1] for _, _, rt in K.expected(b)]
    per = 8
    assert len(routes) == 2048 * per
    col = lambda k: Counter(routes[k::per])   # noqa: E731
    # a * frame + frame <= (a + 1) * frame: concatenated, or (one token a side) the midpoint
    assert set(col(0)) == {R.CONCAT, R.MIDPOINT} and col(0)[R.MIDPOINT] > 100 and col(0)[R.CONCAT] > 100
    # the left filter's edge at 26 frames: three or four tokens (contiguous / LCS), five or six
    assert set(col(1)) == {R.CONTIGUOUS, R.LCS} and min(col(1).values()) > 100
    assert set(col(2)) == {R.CONTIGUOUS, R.LCS} or set(col(2)) == {R.CONTIGUOUS}
    # the right filter: 25 frames above the left end are inside, 27 outside, 26 is the edge
    assert set(col(3)) == {R.CONTIGUOUS} and set(col(5)) == {R.MIDPOINT} and set(col(4)) == {R.CONTIGUOUS, R.MIDPOINT}
    # 12 frames apart match, 13 do not
    assert set(col(6)) == {R.CONTIGUOUS} and set(col(7)) == {R.MIDPOINT}


def test_edges_and_splices_take_their_routes():
    e = [rt[1] for _, _, rt in K.expected(K.edge_batch())]
    assert e == [R.CONTIGUOUS, R.CONTIGUOUS, R.LCS, R.LCS, R.LCS, R.MIDPOINT]
    assert [t[0] for t in K.expected(K.edge_batch())[0][0]] == [1, 2]            # the first of the two equal runs
    with_canon, safe_only, empty_set, nil, no_vocab = ([rt[1] for _, _, rt in K.expected(b)] for b in K.splice_batches())
    A, L = R.TAIL_ADOPT_RIGHT, R.TAIL_KEEP_LEFT
    assert [x >> 4 for x in safe_only[:5]] == [A, L, L, L, R.TAIL_VERBATIM]
    assert all(x >> 4 == R.TAIL_VERBATIM for x in nil)
    assert any(x >> 4 == L for x in empty_set) and empty_set == no_vocab
    toks = lambda b, r: [t[0] for t in K.expected(b)[r][0]]   # noqa: E731
    sb = K.splice_batches()
    assert toks(sb[0], 5) != toks(sb[1], 5)                                      # the case table changes the twins' seam
    assert toks(sb[2], 1) != toks(sb[3], 1)                                      # the empty set is not nil
    assert toks(sb[1], 3) == [4, 1, 3]                                           # popSeamWord found nothing: nothing popped


def test_folds_depend_on_earlier_seams_and_step_back():
    b = K.fold_batch()
    stepped = 0
    for rec in b.recs:
        merged = []
        for k, w in enumerate(rec):
            merged = list(w) if k == 0 else R.merge_chunks(merged, w, b.safe, b.canon, b.overlap)
        stepped += any(x[1] > y[1] for x, y in zip(merged, merged[1:]))
    assert stepped >= 2
    res = K.expected(b)
    assert all(st == R.SUCCESS for _, st, _ in res)
    assert res[8] == ([], R.SUCCESS, [R.NO_SEAM, R.EMPTY, R.EMPTY]) and res[10] == ([], R.SUCCESS, [])
    t = K.expected(K.tight_batch())
    assert [st for _, st, _ in t] == [R.SUCCESS, R.OUTPUT_TOO_SMALL, R.SUCCESS] and t[0] == t[2] and t[1][0] == []


def test_sides_cover_the_strip_edges():
    b = K.side_batch()
    big = 0
    for left, right, log in seams(b):
        big += max(left, right) > K.LDS_SIDE
    assert big >= 6
    routes = Counter(rt[1] & 15 for _, _, rt in K.expected(b))
    assert routes[R.CONTIGUOUS] >= 10 and routes[R.LCS] >= 10 and routes[R.MIDPOINT] >= 2
