"""fa_der_score_batch on the device against the Python restatement of DiarizationDER.compute (tests/der_restatement.py): the frame
count, the four counts, the index mapping, the overlap table and the label mapping as integers, the DERResult doubles by their bits.
No tolerances.  The same file is run on the poisoned-workspace library (make POISON=1).

Shapes: der_overlap gives a workgroup 256 words (16 384 frames) and der_accumulate 32 words, der_raster shares a range among 8 lanes;
the long recording below has 260 words, every other one stays small so that the restatement's frame loops take a second or two."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import der_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
S = R.Segment
CASE1, CASE2, CASE4 = R.CASE1, R.CASE2, R.CASE4
STEP32 = float(np.float32(0.08))
_want = {}


def want(key, ref, hyp, step, collar):
    """The restatement's answer, computed once per (case, step, collar) and shared."""
    k = (key, step, collar)
    if k not in _want:
        _want[k] = R.compute(ref, hyp, step, collar)
    return _want[k]


def bits(x):
    return struct.pack("<d", x)


def same(got, w):
    assert got.frames == w.frames
    assert (got.miss_frames, got.false_alarm_frames, got.confusion_frames, got.ref_frames) == w.counts
    assert got.ref_labels == w.ref_labels and got.hyp_labels == w.hyp_labels
    assert got.index_mapping == w.index_mapping and got.mapping == w.mapping
    assert got.overlap.tolist() == w.overlap
    for a, b in ((got.der, w.der), (got.confusion, w.confusion), (got.false_alarm, w.false_alarm), (got.miss, w.miss), (got.total_ref_speech, w.total_ref_speech)):
        assert bits(a) == bits(b), (a, b)


def device(fa, ctx, cases, step, collar):
    """cases: [(key, ref, hyp)] -> one batched call, every recording compared."""
    D = fa.DERSpeakerSegment
    pairs = [([D(s.speaker, s.start, s.end) for s in ref], [D(s.speaker, s.start, s.end) for s in hyp]) for _, ref, hyp in cases]
    got = fa.compute_der_batch(pairs, step, collar, ctx)
    assert len(got) == len(cases)
    for g, (key, ref, hyp) in zip(got, cases):
        same(g, want(key, ref, hyp, step, collar))
    return got


def random_side(rng, labels, n, dur, prefix):
    """n segments over `labels` speakers in [-1, dur): every label appears, about half of the times lie on the 5 ms grid (frame midpoints
    at step 0.01: the ceil's tie), lengths overlap within and across labels, one in ten is degenerate (end <= start)."""
    out = []
    for i in range(n):
        lab = i if i < labels else int(rng.integers(labels))
        a = float(rng.uniform(-1.0, dur))
        b = a + float(rng.exponential(dur / 12.0))
        if rng.random() < 0.5:
            a, b = round(a / 0.005) * 0.005, round(b / 0.005) * 0.005
        if rng.random() < 0.1:
            b = a - float(rng.integers(0, 2))
        out.append(S(f"{prefix}{lab}", a, min(b, dur)))
    return out


def test_hand_cases(fa, gpu_ctx):
    cases = [("c1", *CASE1), ("c2", *CASE2), ("c3a", [S("A", 0.0, 1.0)], []), ("c3b", [], [S("x", 0.0, 1.0)]), ("c4", *CASE4)]
    got = device(fa, gpu_ctx, cases, 0.01, 0.0)
    assert (got[0].confusion_frames, got[0].ref_frames, got[0].frames) == (200, 2000, 2001) and got[0].mapping == {"x": "A", "y": "B"}
    assert (got[1].false_alarm_frames, got[1].ref_frames, got[1].index_mapping) == (100, 200, [0, 1, -1])
    assert (got[4].miss_frames, got[4].false_alarm_frames, got[4].ref_frames, got[4].overlap.tolist()) == (65, 14, 114, [[49]])
    got = device(fa, gpu_ctx, cases[:2], 0.01, 0.5)
    assert (got[0].confusion_frames, got[0].ref_frames) == (175, 1900)
    got = device(fa, gpu_ctx, cases[2:4], 0.08, 0.0)
    assert (got[0].miss_frames, got[0].ref_frames, got[0].frames, got[0].der) == (12, 12, 14, 1.0)
    assert (got[1].false_alarm_frames, got[1].ref_frames, got[1].der) == (12, 0, 0.0)
    one = fa.compute_der([fa.DERSpeakerSegment(s.speaker, s.start, s.end) for s in CASE1[0]], [fa.DERSpeakerSegment(s.speaker, s.start, s.end) for s in CASE1[1]],
                         ctx=gpu_ctx)
    same(one, want("c1", *CASE1, 0.01, 0.0))


@pytest.mark.parametrize("frames", [1, 63, 64, 65, 129, 193])
def test_word_edges(fa, gpu_ctx, frames):
    """Step 1: a segment [s, e) of whole seconds is exactly the frames [s, e).  Ranges that start or end on a multiple of 64, lie inside
    one word or span three; the last segment pins maxEnd = frames - 1.  Collar 140 excludes [b - 70, b + 70): three words, clipped at
    both ends; collar 3 a range inside one word or across an edge."""
    last = frames - 1
    spans = [(0, 64), (64, 128), (63, 65), (3, 17), (60, 193), (1, 129), (128, 192), (-5, 1), (0, 1), (62, 64), (64, 65), (127, 129)]
    ref = [S(f"r{i % 3}", float(a), float(b)) for i, (a, b) in enumerate(spans) if b <= last and i % 2 == 0]
    hyp = [S(f"h{i % 4}", float(a), float(b)) for i, (a, b) in enumerate(spans) if b <= last and i % 3 != 1]
    ref.append(S("r0", float(last) - 2.0, float(last)))
    hyp.append(S("h0", -3.0, float(last)))
    for collar in (0.0, 3.0, 140.0):
        got = device(fa, gpu_ctx, [(f"edge{frames}", ref, hyp)], 1.0, collar)
        assert got[0].frames == frames


def test_more_than_one_workgroup(fa, gpu_ctx):
    rng = np.random.default_rng(11)
    dur = 166.0   # 16 601 frames = 260 words: two tiles of der_overlap, nine of der_accumulate, the last ones partial
    ref, hyp = random_side(rng, 4, 60, dur, "r"), random_side(rng, 5, 70, dur, "h")
    ref.append(S("r0", 100.0, dur))
    hyp.append(S("h1", -0.5, 164.0))   # one range across both tiles: 257 words
    for collar in (0.0, 0.25):
        got = device(fa, gpu_ctx, [("long", ref, hyp)], 0.01, collar)
        assert got[0].frames == 16601 and got[0].ref_frames > 0 and got[0].confusion_frames > 0


def random_batch():
    rng = np.random.default_rng(5)
    return [("b0", random_side(rng, 3, 40, 20.0, "r"), random_side(rng, 7, 60, 20.0, "h")),      # H > R
            ("b1", random_side(rng, 8, 90, 35.0, "r"), random_side(rng, 2, 30, 33.0, "h")),      # R > H
            ("b2", [], []),                                                                       # nothing on either side, in the middle
            ("b3", random_side(rng, 64, 200, 9.0, "r"), random_side(rng, 64, 220, 9.5, "h")),    # the label limit on both sides
            ("b4", random_side(rng, 1, 12, 12.0, "r"), random_side(rng, 5, 25, 50.0, "h"))]


@pytest.mark.parametrize("step", [0.01, STEP32])
@pytest.mark.parametrize("collar", [0.0, 0.25])
def test_random_batch(fa, gpu_ctx, step, collar):
    got = device(fa, gpu_ctx, random_batch(), step, collar)
    assert got[2].frames == 0 and got[2].der == 0.0 and got[2].mapping == {}
    assert len(got[3].ref_labels) == 64 and len(got[3].hyp_labels) == 64 and sum(m >= 0 for m in got[3].index_mapping) >= 1
    assert len(got[0].hyp_labels) > len(got[0].ref_labels) and len(got[1].ref_labels) > len(got[1].hyp_labels)


def test_hungarian_ties(fa, gpu_ctx):
    """Many equal overlaps: the mapping has to be the reference solver's, not merely an optimal one."""
    ref4 = [S(f"R{k}", 10.0 * k, 10.0 * k + 10.0) for k in range(4)]
    all4 = [S(f"h{k}", 0.0, 40.0) for k in range(4)]                                            # a 4 x 4 of equal blocks
    pairs = [S(f"p{k}", 20.0 * (k % 2), 20.0 * (k % 2) + 20.0) for k in range(4)]             # each hyp covers two refs equally
    dup = [S("x", 0.0, 12.0), S("x2", 0.0, 12.0), S("y", 12.0, 20.0), S("y2", 12.0, 20.0), S("x3", 0.0, 12.0)]   # duplicated hyp speakers
    rev = [S(f"h{k}", 30.0 - 10.0 * k, 40.0 - 10.0 * k) for k in range(4)] + [S("h4", 0.0, 10.0), S("h5", 0.0, 40.0)]
    cases = [("t_all", ref4, all4), ("t_pairs", ref4, pairs), ("t_dup", CASE1[0], dup), ("t_rev", ref4, rev), ("t_self", ref4, ref4),
             ("t_wide", all4, ref4)]
    got = device(fa, gpu_ctx, cases, 0.01, 0.0)
    assert got[0].overlap.tolist() == [[1000] * 4] * 4 and got[0].index_mapping == [0, 1, 2, 3]
    assert got[2].overlap.tolist() == [[1000, 200], [1000, 200], [0, 800], [0, 800], [1000, 200]]
    assert sorted(m for m in got[2].index_mapping if m >= 0) == [0, 1]
    assert got[4].der == 0.0


def test_reused_context_with_smaller_inputs(fa, gpu_ctx):
    """The call zeroes its own planes and tables: after a large call, a small one on the same context (its buffers come back from the
    context's cache, filled with the large call's bits — or with 0xFF on the poisoned build) answers as a fresh context does."""
    rng = np.random.default_rng(3)
    big = [("big", random_side(rng, 6, 80, 60.0, "r"), random_side(rng, 6, 80, 60.0, "h"))]
    small = [("small", random_side(rng, 3, 10, 6.0, "r"), random_side(rng, 2, 10, 6.0, "h")), ("c4", *CASE4)]
    ctx = fa.Context(0)
    fresh = fa.Context(0)
    try:
        device(fa, ctx, big, 0.01, 0.25)
        a = device(fa, ctx, small, 0.01, 0.25)
        b = device(fa, fresh, small, 0.01, 0.25)
        c = device(fa, ctx, small, 0.01, 0.25)
        for x, y, z in zip(a, b, c):
            assert x.index_mapping == y.index_mapping == z.index_mapping and x.overlap.tolist() == y.overlap.tolist() == z.overlap.tolist()
            assert (x.miss_frames, x.false_alarm_frames, x.confusion_frames, x.ref_frames) == (y.miss_frames, y.false_alarm_frames, y.confusion_frames, y.ref_frames)
    finally:
        ctx.close()
        fresh.close()


def test_output_ranges_and_statuses(fa, gpu_ctx):
    """The mapping range is the caller's: what it holds beyond hyp_labels is -1, a range that is too small or an overlap buffer that is
    too small is OUTPUT_TOO_SMALL, and the overlap table may be left out."""
    import ctypes as C
    L = fa._lib
    f = fa.lib().fa_der_score_batch
    w = want("c1", *CASE1, 0.01, 0.0)
    seg = lambda lab, s: L.DerSegment(lab, 0, s.start, s.end)  # noqa: E731
    ref = (L.DerSegment * 2)(seg(0, CASE1[0][0]), seg(1, CASE1[0][1]))
    hyp = (L.DerSegment * 2)(seg(0, CASE1[1][0]), seg(1, CASE1[1][1]))
    rng = (C.c_int64 * 2)(0, 2)
    cfg = L.DerConfig(0.01, 0.0)
    counts = (L.DerCounts * 1)()
    mapping = (C.c_int32 * 6)(*([9] * 6))
    overlap = (C.c_int64 * 4)()
    h = gpu_ctx.handle
    assert f(h, C.byref(cfg), ref, rng, hyp, rng, 1, counts, mapping, (C.c_int64 * 2)(1, 5), None, 0) == L.SUCCESS
    assert list(mapping) == [9, 0, 1, -1, -1, 9]
    assert (counts[0].frames, counts[0].miss, counts[0].false_alarm, counts[0].confusion, counts[0].ref, counts[0].ref_labels, counts[0].hyp_labels) == \
        (w.frames, *w.counts, 2, 2)
    assert f(h, C.byref(cfg), ref, rng, hyp, rng, 1, counts, mapping, (C.c_int64 * 2)(0, 1), None, 0) == L.OUTPUT_TOO_SMALL
    assert f(h, C.byref(cfg), ref, rng, hyp, rng, 1, counts, mapping, rng, overlap, 3) == L.OUTPUT_TOO_SMALL
    assert f(h, C.byref(cfg), ref, rng, hyp, rng, 1, counts, mapping, rng, overlap, 4) == L.SUCCESS and list(overlap) == [1000, 200, 0, 800]
    assert f(h, C.byref(cfg), ref, rng, hyp, rng, 0, None, None, None, None, 0) == L.SUCCESS
    far = (L.DerSegment * 1)(L.DerSegment(0, 0, 0.0, 1e9))
    assert f(h, C.byref(cfg), far, (C.c_int64 * 2)(0, 1), hyp, rng, 1, counts, mapping, rng, None, 0) == L.INDEX_OVERFLOW
