"""The argument pass and the plan of the DER scorer (csrc/der_geom.h: label counts, frame counts, the word offsets of the bit planes
and overlap tables, the raster's items and workgroups, and every refusal of a call) walked on the CPU by tests/cpu/der_geom.cpp against
tests/der_restatement.py and the conditions restated here.  The program is stand-alone, reads its cases from stdin and is built with
the address and undefined-behaviour sanitizers.  No GPU."""
import math
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import der_restatement as R  # noqa: E402
from der_restatement import Segment  # noqa: E402

OK, INVALID_ARGUMENT, INDEX_OVERFLOW, OUTPUT_TOO_SMALL = 0, 1, 2, 3
RASTER_LANES, THREADS = 8, 256


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("der_geom") / "der_geom")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "der_geom.cpp"), "-o", exe], check=True)
    return exe


def number(segs):
    """Labels by first appearance, as fluidaudio_amd.der.index_labels numbers them."""
    idx = {}
    return [(idx.setdefault(s.speaker, len(idx)), s.start, s.end) for s in segs]


def fmt(x):
    return x.hex() if math.isfinite(x) else str(x)


def call(geom, recordings, frame_step=0.01, collar=0.0, mapping_room=None, have_mapping=True, overlap_capacity=None, ranges=None, B=None):
    """recordings: [(ref, hyp)] with sides as [(label, start, end)].  mapping_room: per recording (default: its hypothesis labels).  Returns
    (status, text) or (0, head, [per-recording tuples])."""
    refs = [s for r, _ in recordings for s in r]
    hyps = [s for _, h in recordings for s in h]
    ref_range, hyp_range, map_range = [0], [0], [0]
    for i, (r, h) in enumerate(recordings):
        ref_range.append(ref_range[-1] + len(r))
        hyp_range.append(hyp_range[-1] + len(h))
        room = mapping_room[i] if mapping_room is not None else max((s[0] + 1 for s in h), default=0)
        map_range.append(map_range[-1] + room)
    if ranges is not None:
        ref_range, hyp_range, map_range = ranges
    nb = len(recordings) if B is None else B
    ref_range, hyp_range, map_range = (r[:max(nb, 0) + 1] for r in (ref_range, hyp_range, map_range))
    words = ["call", fmt(frame_step), fmt(collar), nb, len(refs), len(hyps), int(have_mapping), int(overlap_capacity is not None), overlap_capacity or 0]
    words += ref_range + hyp_range + map_range
    for s in refs + hyps:
        words += [s[0], fmt(float(s[1])), fmt(float(s[2]))]
    r = subprocess.run([geom], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    parts = [p.strip() for p in r.stdout.strip().split("|")]
    status = int(parts[0])
    if status != OK:
        return status, parts[1]
    per = [int(x) for x in parts[2].split()]
    return status, tuple(int(x) for x in parts[1].split()), [tuple(per[i:i + 10]) for i in range(0, len(per), 10)]


def one_segment(frames):
    """A recording whose only segment makes `frames` frames: Int(ceil(end / 0.01)) + 1."""
    end = 0.0 if frames == 1 else (frames - 1.5) * 0.01
    rec = ([Segment("A", 0.0, end)], [])
    assert R.compute(*rec).frames == frames
    return rec


CASES = [R.CASE1, R.CASE2, R.CASE4] + [one_segment(n) for n in (1, 63, 64, 65, 129, 193)]


def restated_plan(cases, collar):
    per, plane_off, ov_off, max_words = [], 0, 0, 0
    ref_at = hyp_at = 0
    for ref, hyp in cases:
        want = R.compute(ref, hyp, 0.01, collar)
        nR, nH = len(want.ref_labels), len(want.hyp_labels)
        words = -(-want.frames // 64)
        per.append((want.frames, nR, nH, words, plane_off, ov_off, ref_at, ref_at + len(ref), hyp_at, hyp_at + len(hyp)))
        plane_off += words * (nR + nH + 1)
        ov_off += nR * nH
        max_words = max(max_words, words)
        ref_at += len(ref)
        hyp_at += len(hyp)
    items = ref_at + hyp_at + (2 * ref_at if collar > 0 else 0)
    return (plane_off, ov_off, max_words, items, -(-items * RASTER_LANES // THREADS), OK), per


@pytest.mark.parametrize("collar", [0.0, 0.25])
def test_the_plan_is_the_restated_geometry(geom, collar):
    for cases in ([c] for c in CASES):                                           # every recording on its own ...
        status, head, per = call(geom, [(number(r), number(h)) for r, h in cases], collar=collar, overlap_capacity=10**6)
        assert (status, (head, per)) == (OK, restated_plan(cases, collar))
    status, head, per = call(geom, [(number(r), number(h)) for r, h in CASES], collar=collar, overlap_capacity=10**6)   # ... and all in one call
    assert (status, (head, per)) == (OK, restated_plan(CASES, collar))
    assert [p[0] for p in per[3:]] == [1, 63, 64, 65, 129, 193] and [p[3] for p in per[3:]] == [1, 1, 1, 2, 3, 4]
    assert head[3] == (3 if collar > 0 else 1) * sum(len(r) for r, _ in CASES) + sum(len(h) for _, h in CASES)


def test_a_recording_without_labels_contributes_nothing(geom):
    a, b = (number(R.CASE1[0]), number(R.CASE1[1])), (number(R.CASE2[0]), number(R.CASE2[1]))
    _, head_with, per_with = call(geom, [a, ([], []), b])
    _, head_without, per_without = call(geom, [a, b])
    assert head_with == head_without
    assert per_with[1][:4] == (0, 0, 0, 0) and per_with[1][4:6] == per_with[2][4:6]      # no frames, no words; the offsets do not move
    assert [p[:6] for p in (per_with[0], per_with[2])] == [p[:6] for p in per_without]
    assert call(geom, [([], [])])[1] == (0, 0, 0, 0, 0, OK)                               # plane_words == 0: the entry answers zeros


def test_the_uploads_start_at_the_first_segment_used(geom):
    rec = (number(R.CASE2[0]), number(R.CASE2[1]))
    base = call(geom, [rec])
    ranges = ([0, 2], [0, 3], [0, 3])
    assert call(geom, [rec], ranges=ranges) == base
    pad = ([(0, 0.0, 1.0)] * 3, [(0, 0.0, 1.0)] * 2)                                      # segments ahead of the ranges: not part of the call
    shifted = call(geom, [(pad[0] + rec[0], pad[1] + rec[1])], ranges=([3, 5], [2, 5], [7, 10]))
    assert shifted == base


def test_verdicts(geom):
    seg = [(0, 0.0, 1.0)]
    assert call(geom, [([(63, 0.0, 1.0)], seg)], mapping_room=[1])[0] == OK               # 64 labels a side
    assert call(geom, [(seg, [(63, 0.0, 1.0)])])[0] == OK
    for bad in (([(64, 0.0, 1.0)], seg), (seg, [(64, 0.0, 1.0)]), ([(-1, 0.0, 1.0)], seg)):
        status, text = call(geom, [bad], mapping_room=[64])
        assert status == INVALID_ARGUMENT and "a side holds at most 64 labels" in text
    for t in (float("inf"), float("-inf"), float("nan")):
        for bad in ([(0, t, 1.0)], [(0, 0.0, t)]):
            assert call(geom, [(bad, seg)]) == (INVALID_ARGUMENT, "der: recording 0 has a segment with a non-finite time")
            assert call(geom, [(seg, seg), (seg, bad)]) == (INVALID_ARGUMENT, "der: recording 1 has a segment with a non-finite time")
    for ranges in (([0, 1, 0], [0, 1, 2], [0, 1, 2]), ([0, 1, 2], [1, 0, 2], [0, 1, 2]), ([-1, 1, 2], [0, 1, 2], [0, 1, 2])):
        status, text = call(geom, [(seg, seg), (seg, seg)], ranges=ranges)
        assert status == INVALID_ARGUMENT and text.startswith("der: the segment ranges of recording")
    assert call(geom, [(seg, seg)], ranges=([0, 1], [0, 1], [1, 0])) == (INVALID_ARGUMENT, "der: the mapping range of recording 0 does not ascend")
    for step in (0.0, -0.01, float("inf"), float("nan")):
        assert call(geom, [(seg, seg)], frame_step=step)[0] == INVALID_ARGUMENT
    for collar in (-0.1, float("inf"), float("nan")):
        assert call(geom, [(seg, seg)], collar=collar)[0] == INVALID_ARGUMENT
    assert call(geom, [(seg, seg)], B=-1)[0] == INVALID_ARGUMENT
    assert call(geom, [], B=0) == (OK, (0, 0, 0, 0, 0, OK), [])
    assert call(geom, [([(0, 0.0, 3e7)], seg)]) == (INDEX_OVERFLOW, "der: recording 0 has 2^31 frames or more")
    assert call(geom, [([(0, 0.0, 2.1e7)], seg)])[0] == OK                                # 2.1e9 + 1 frames still fit
    two = [(0, 0.0, 1.0), (1, 0.0, 1.0)]
    assert call(geom, [(seg, two)], mapping_room=[1]) == (OUTPUT_TOO_SMALL, "der: recording 0 has 2 hypothesis labels, its mapping range holds 1")
    assert call(geom, [(seg, two)], have_mapping=False) == (INVALID_ARGUMENT, "der: mapping is required")
    assert call(geom, [(two, two), (seg, two)], overlap_capacity=5) == (OUTPUT_TOO_SMALL, "der: the overlap tables take 6 entries, the output holds 5")
    assert call(geom, [(two, two), (seg, two)], overlap_capacity=6)[0] == OK
    assert call(geom, [(two, two), (seg, two)])[0] == OK                                  # no overlap output: no capacity asked


def test_a_call_with_two_faults_reports_the_first_in_the_order_of_the_pass(geom):
    """The order der_score has always checked in: the config; the sizes; then recording by recording its ranges and, segment by segment with
    the reference side first, a non-finite time before a label out of range, then its frame count; then recording by recording its
    mapping range, the room in it, the mapping array; last the overlap capacity."""
    seg, two = [(0, 0.0, 1.0)], [(0, 0.0, 1.0), (1, 0.0, 1.0)]
    nan = float("nan")
    assert call(geom, [(seg, seg)], frame_step=0.0, B=-1)[1].startswith("der: frame_step must be positive")      # config before sizes
    assert call(geom, [(seg, [(64, 0.0, 1.0)])], B=-1) == (INVALID_ARGUMENT, "der: bad arguments")                 # sizes before segments
    status, text = call(geom, [(seg, [(64, 0.0, 1.0)]), (seg, seg)], ranges=([0, 1, 0], [0, 1, 2], [0, 64, 65]))   # recording 0 before recording 1
    assert status == INVALID_ARGUMENT and text.startswith("der: recording 0 has label 64")
    assert call(geom, [([(64, nan, 1.0)], seg)])[1] == "der: recording 0 has a segment with a non-finite time"     # time before label
    assert call(geom, [([(64, 0.0, 1.0)], [(0, nan, 1.0)])], mapping_room=[1])[1].startswith("der: recording 0 has label 64")   # reference side first
    assert call(geom, [([(0, 0.0, 1.0), (0, nan, 1.0)], [(64, 0.0, 1.0)])])[1] == "der: recording 0 has a segment with a non-finite time"
    assert call(geom, [(seg, seg), ([(0, 0.0, 3e7)], two)], mapping_room=[0, 2])[0] == INDEX_OVERFLOW              # every recording's geometry before any mapping range
    assert call(geom, [(seg, two)], mapping_room=[1], have_mapping=False)[0] == OUTPUT_TOO_SMALL                   # the room before the missing array
    assert call(geom, [(seg, seg), (seg, two)], mapping_room=[1, 1], overlap_capacity=0)[1].startswith("der: recording 1 has 2 hypothesis labels")   # mapping before overlap
