"""The restatement of DiarizationDER.compute (tests/der_restatement.py) against answers worked out by hand, and the host-only parts of
the wrappers (fluidaudio_amd/der.py): label numbering, the two adapters and the argument contract, which is answered before any device
work and therefore needs no GPU.

The hand answers.  A frame t is active for [start, end) when ceil(start / step - 0.5) <= t < ceil(end / step - 0.5).
1. step 0.01: maxEnd 20 -> 2001 frames.  A = [0, 1000), B = [1000, 2000), x = [0, 1200), y = [1200, 2000).  O[x] = [1000, 200],
   O[y] = [0, 800]; x->A, y->B keeps 1800 frames, the swap 200.  Only frames [1000, 1200) err: one ref, one hyp, wrong label -> 200
   confusions of 2000 reference frames.  Collar 0.5: boundaries 0, 10, 10, 20 drop [0, 25), [975, 1025), [1975, 2001): 1900 reference
   frames stay, and of [1000, 1200) the part [1025, 1200) = 175.
2. step 0.01: maxEnd 2 (z's end counts) -> 201 frames.  A = [0, 100), B = [50, 150), x = y = [0, 150): all four overlaps are 100, the
   cost matrix is zero on the real cells, and the solver's lowest-column preference gives x->A, y->B; z (H = 3 through it) draws the
   padding column.  [0, 50): ref 1, hyp 2, fa 1; [50, 100): 2, 2, both correct; [100, 150): ref 1 (B), hyp 2, y correct, fa 1.
3. step 0.08: ceil(1 / 0.08) + 1 = 14 frames; ceil(12.5 - 0.5) = 12 active frames, all missed (or, mirrored, all false alarms).
4. step 0.01: maxEnd 1.28 -> 129 frames.  A = [ceil(14.0), ceil(63.5)) | [ceil(29.5), ceil(127.5)) = [14, 128): 114 frames;
   x = [0, ceil(63.0)) = [0, 63).  Overlap [14, 63) = 49, false alarm [0, 14), miss [63, 128) = 65."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import der_restatement as R  # noqa: E402

S = R.Segment
CASE1, CASE2, CASE4 = R.CASE1, R.CASE2, R.CASE4


def test_case_1_confusion_and_collar():
    r = R.compute(*CASE1, 0.01, 0.0)
    assert r.frames == 2001 and r.overlap == [[1000, 200], [0, 800]] and r.mapping == {"x": "A", "y": "B"}
    assert r.counts == (0, 0, 200, 2000)
    assert r.der == (0.0 + 0.0 + 200 * 0.01) / (2000 * 0.01) and abs(r.der - 0.1) < 1e-15
    assert (r.miss, r.false_alarm, r.confusion, r.total_ref_speech) == (0.0, 0.0, 200 * 0.01, 2000 * 0.01)
    c = R.compute(*CASE1, 0.01, 0.5)
    assert c.counts == (0, 0, 175, 1900) and c.overlap == r.overlap and c.mapping == r.mapping


def test_case_2_degenerate_label_and_tied_overlaps():
    r = R.compute(*CASE2, 0.01, 0.0)
    assert r.frames == 201 and r.hyp_labels == ["x", "y", "z"] and r.ref_labels == ["A", "B"]
    assert r.overlap == [[100, 100], [100, 100], [0, 0]]
    assert r.index_mapping == [0, 1, -1] and r.mapping == {"x": "A", "y": "B"}
    assert r.counts == (0, 100, 0, 200)


def test_case_3_one_side_empty():
    r = R.compute([S("A", 0.0, 1.0)], [], 0.08, 0.0)
    assert r.frames == 14 and r.counts == (12, 0, 0, 12) and r.der == 1.0 and r.mapping == {}
    m = R.compute([], [S("x", 0.0, 1.0)], 0.08, 0.0)
    assert m.frames == 14 and m.counts == (0, 12, 0, 0) and m.der == 0.0 and m.index_mapping == [-1]
    e = R.compute([], [], 0.01, 0.0)
    assert e.frames == 0 and e.counts == (0, 0, 0, 0) and e.der == 0.0


def test_case_4_overlapping_segments_of_one_label_and_a_negative_start():
    r = R.compute(*CASE4, 0.01, 0.0)
    assert r.frames == 129 and r.overlap == [[49]] and r.counts == (65, 14, 0, 114) and r.mapping == {"x": "A"}


def test_hungarian_prefers_the_lowest_column_among_equals():
    assert R.hungarian([0] * 9, 3) == [0, 1, 2]
    assert R.hungarian([5, 1, 1, 5], 2) == [1, 0]
    assert R.hungarian([], 0) == []


def test_labels_are_numbered_by_first_appearance(fa):
    from fluidaudio_amd import der
    segs = [fa.DERSpeakerSegment("b", 1.0, 2.0), fa.DERSpeakerSegment("a", 0.0, 1.0), fa.DERSpeakerSegment("b", 3.0, 2.0), fa.DERSpeakerSegment("c", 5.0, 5.0)]
    labels, arr = der.index_labels(segs)
    assert labels == ["b", "a", "c"] and arr["label"].tolist() == [0, 1, 0, 2]
    assert arr["start"].tolist() == [1.0, 0.0, 3.0, 5.0] and arr["end"].tolist() == [2.0, 1.0, 2.0, 5.0]
    assert arr.dtype.itemsize == 24 and der.DER_COUNTS_DTYPE.itemsize == 48
    import ctypes as C
    assert C.sizeof(fa._lib.DerSegment) == 24 and C.sizeof(fa._lib.DerCounts) == 48 and C.sizeof(fa._lib.DerConfig) == 16
    assert der.index_labels([])[0] == [] and der.index_labels([])[1].size == 0


def test_adapters(fa):
    timed = [fa.TimedSpeakerSegment("spk1", 0.1, 12.34), fa.TimedSpeakerSegment("spk0", 3.3, 4.7)]
    got = fa.segments_from_timed(timed)
    f = np.float32
    assert got == [fa.DERSpeakerSegment("spk1", float(f(0.1)), float(f(12.34))), fa.DERSpeakerSegment("spk0", float(f(3.3)), float(f(4.7)))]
    assert got[0].start != 0.1   # widened from Float, not the decimal
    from fluidaudio_amd.sortformer import SEGMENT_DTYPE
    recs = np.zeros(2, SEGMENT_DTYPE)
    recs[0] = (0, 2, 7, 1234567, 0.5, 3)
    recs[1] = (0, 0, 3, 11, 0.5, 3)
    fd = f(0.08)
    want = [fa.DERSpeakerSegment("Speaker 2", float(f(f(7) * fd)), float(f(f(1234567) * fd))), fa.DERSpeakerSegment("Speaker 0", float(f(f(3) * fd)), float(f(f(11) * fd)))]
    assert fa.segments_from_timeline(recs, 0.08) == want
    segs = [fa.DiarizerSegment(2, 7, 1234567, True, 0.08), fa.DiarizerSegment(0, 3, 11, True, 0.08)]
    assert fa.segments_from_timeline(segs, 0.08) == want
    assert want[0].end == float(segs[0].end_time) and want[0].end != 1234567 * 0.08


def test_argument_contract_needs_no_device(fa):
    D = fa.DERSpeakerSegment
    ok = [D("A", 0.0, 1.0)]
    bad = [
        dict(ref=[D("A", float("nan"), 1.0)], hyp=ok),
        dict(ref=ok, hyp=[D("x", 0.0, float("inf"))]),
        dict(ref=ok, hyp=[D("x", float("-inf"), 1.0)]),
        dict(ref=ok, hyp=ok, frame_step=0.0),
        dict(ref=ok, hyp=ok, frame_step=-0.01),
        dict(ref=ok, hyp=ok, frame_step=float("nan")),
        dict(ref=ok, hyp=ok, frame_step=float("inf")),
        dict(ref=ok, hyp=ok, collar=-0.25),
        dict(ref=ok, hyp=[D(f"s{i}", 0.0, 1.0) for i in range(65)]),
        dict(ref=[D(f"s{i}", 2.0, 1.0) for i in range(65)], hyp=ok),
    ]
    for kw in bad:
        with pytest.raises(fa.FluidAudioHipError) as e:
            fa.compute_der(**kw)
        assert e.value.status == fa.INVALID_ARGUMENT, kw
    assert fa.compute_der_batch([]) == []


def test_abi_decides_argument_errors_before_device_work(fa):
    """fa_der_score_batch itself, without a context: a status, never a crash, and nothing is written."""
    import ctypes as C
    L = fa._lib
    f = fa.lib().fa_der_score_batch
    cfg = L.DerConfig()
    fa.lib().fa_der_default_config(C.byref(cfg))
    assert (cfg.frame_step, cfg.collar) == (0.01, 0.0)
    fa.lib().fa_der_default_config(None)
    seg = (L.DerSegment * 1)(L.DerSegment(0, 0, 0.0, 1.0))
    rng = (C.c_int64 * 2)(0, 1)
    counts = (L.DerCounts * 1)()
    mapping = (C.c_int32 * 1)(7)
    call = lambda c, s=seg: f(None, C.byref(c), s, rng, s, rng, 1, counts, mapping, rng, None, 0)  # noqa: E731
    assert call(cfg) == L.INVALID_ARGUMENT            # no context
    assert call(L.DerConfig(0.0, 0.0)) == L.INVALID_ARGUMENT
    assert call(L.DerConfig(0.01, -1.0)) == L.INVALID_ARGUMENT
    assert call(cfg, (L.DerSegment * 1)(L.DerSegment(64, 0, 0.0, 1.0))) == L.INVALID_ARGUMENT
    assert call(cfg, (L.DerSegment * 1)(L.DerSegment(0, 0, float("nan"), 1.0))) == L.INVALID_ARGUMENT
    assert f(None, None, None, None, None, None, 0, None, None, None, None, 0) == L.INVALID_ARGUMENT
    assert mapping[0] == 7 and counts[0].frames == 0
