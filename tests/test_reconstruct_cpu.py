"""Speaker segments without a GPU: the numpy restatement (tests/reconstruct_restatement.py) against the reference's own test cases
(Tests/FluidAudioTests/Diarizer/Offline/ZeroVoteReembedderTests.swift), hand cases of the merge / sanitize rules, and the two pure
host entries of the library (fa_offline_chunk_assignments, fa_segments_finalize) against the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reconstruct_restatement as R  # noqa: E402

CENTROIDS3 = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]


# ---- ZeroVoteReembedderTests.swift:16-134 (detectRuns)
@pytest.mark.parametrize("counts, sums, expect", [
    ([1] * 8, [[0.9, 0], [0.8, 0]] + [[0, 0]] * 5 + [[0.7, 0]], [(2, 7)]),                        # :16-33
    ([1, 1, 2, 2, 2, 2, 2, 1], [[0.9, 0], [0.8, 0]] + [[0, 0]] * 5 + [[0.7, 0]], []),             # :35-53 overlap frames
    ([0, 1, 1, 1, 1, 1, 0, 0], [[0, 0]] * 8, [(1, 6)]),                                           # :55-68 non-speech gaps
    ([1] * 5, [[0.9, 0], [0, 0], [0, 0], [0, 0], [0.9, 0]], []),                                  # :70-83 too short
    ([1] * 14, [[0.9, 0]] + [[0, 0]] * 4 + [[0, 0.8]] * 2 + [[0, 0]] * 7, [(1, 5), (7, 14)]),     # :85-101
    ([1] * 6, [[0.9, 0]] + [[0, 0]] * 5, [(1, 6)]),                                               # :103-115 to the end
])
def test_detect_runs_reference_cases(counts, sums, expect):
    assert R.detect_runs(counts, sums, 0.1, 0.4) == expect


def test_detect_runs_empty_and_bad_frame_duration():   # :117-134
    assert R.detect_runs([], [], 0.1, 0.4) == []
    assert R.detect_runs([1] * 5, [[0]] * 5, 0.0, 0.4) == []


def test_zero_vote_assignment_reference_cases():   # :138-180
    assert R.zero_vote_assignment([0.70, 0.71, 0.0], CENTROIDS3) == 1
    assert R.zero_vote_assignment([1, 1, 0], CENTROIDS3) == 0
    assert R.zero_vote_assignment([np.nan, 0.5, 0.5], CENTROIDS3) is None
    assert R.zero_vote_assignment([np.inf, 0, 0], CENTROIDS3) is None
    assert R.zero_vote_assignment([], CENTROIDS3) is None
    assert R.zero_vote_assignment([1, 0, 0], []) is None
    assert R.zero_vote_assignment([1, 0], CENTROIDS3) is None


def zero_vote_scenario():
    """:202-235: one chunk of 30 frames (0.1 s), speaker 0 -> cluster 0 on both flanks, speaker 1 active in frames 10-19 with -2."""
    w = np.array([[[0, 1] if 10 <= f < 20 else [1, 0] for f in range(30)]], np.float32)
    cfg = R.config(min_segment_duration=0.1, min_gap_duration=0.05, min_duration_on=0.0, min_duration_off=0.0, zero_vote_min_duration=0.4)
    return w, np.array([[0, -2]]), [[1, 0, 0], [0, 1, 0]], cfg


def shape(segs):
    return [(s[0], float(s[1]), float(s[2])) for s in segs]


def test_reembedded_run_becomes_its_own_segment():   # :237-259
    w, hard, cen, cfg = zero_vote_scenario()
    spans = []

    def emb(a, b):
        spans.append((a, b))
        return [0.1, 0.9, 0.0]
    segs = R.build_segments(w, hard, cen, [0.0], 0.1, cfg, emb, zero_vote=True)
    assert len(spans) == 1 and abs(spans[0][0] - 1.0) < 1e-6 and abs(spans[0][1] - 2.0) < 1e-6
    assert [s[0] for s in segs] == ["S1", "S2", "S1"]
    assert abs(float(segs[1][1]) - 1.0) < 1e-3 and abs(float(segs[1][2]) - 2.0) < 1e-3


def test_disabled_pass_never_embeds_and_failing_embedder_equals_it():   # :261-301
    w, hard, cen, cfg = zero_vote_scenario()
    calls = []
    off = R.build_segments(w, hard, cen, [0.0], 0.1, cfg, lambda a, b: calls.append(1) or [0.1, 0.9, 0.0], zero_vote=False)
    assert calls == []
    failing = R.build_segments(w, hard, cen, [0.0], 0.1, cfg, lambda a, b: None, zero_vote=True)
    assert shape(failing) == shape(off)
    assert [s[0] for s in off] == ["S1"]   # the zero-vote frames tie-break to cluster 0


# ---- hand cases of merge / sanitize / excludeOverlaps
def seg(spk, a, b, q=1.0):
    return (spk, np.float32(a), np.float32(b), np.float32(q))


def test_overlap_trimming_scales_quality():
    out = R.finalize([seg("S1", 0, 4, 0.8), seg("S2", 3, 6, 0.9)], R.config())
    assert shape(out) == [("S1", 0.0, 4.0), ("S2", 4.0, 6.0)]
    assert out[1][3] == np.float32(np.float32(0.9) * np.float32(np.float32(2) / np.float32(3)))


def test_gap_merge_at_exactly_the_threshold():
    cfg = R.config(min_gap_duration=0.25, min_segment_duration=0.0)   # 0.25 and the Float gap 1.25 - 1.0 are exact
    assert shape(R.finalize([seg("S1", 0, 1), seg("S1", 1.25, 2)], cfg)) == [("S1", 0.0, 2.0)]
    assert shape(R.finalize([seg("S1", 0, 1), seg("S1", 1.3125, 2)], cfg)) == [("S1", 0.0, 1.0), ("S1", 1.3125, 2.0)]


def test_min_duration_drops():
    out = R.finalize([seg("S1", 0, 0.5), seg("S2", 1, 3), seg("S1", 3.5, 3.9)], R.config())
    assert shape(out) == [("S2", 1.0, 3.0)]
    out = R.finalize([seg("S1", 0, 2), seg("S2", 1.5, 2.8)], R.config())   # trimmed to 2.0-2.8 < 1.0 s: dropped by excludeOverlaps
    assert shape(out) == [("S1", 0.0, 2.0)]


def test_segment_open_at_the_end_uses_last_frame_plus_fd():
    fd = 0.1
    w = np.zeros((1, 30, 1), np.float32)
    w[0, 5:, 0] = 1
    segs, st = R.build_segments(w, [[0]], [[1.0]], [0.0], fd, R.config(min_segment_duration=0.0), return_state=True)
    assert st["T"] == 30
    assert st["raw"][0][2] == np.float32(29 * fd + fd) and st["raw"][0][1] == np.float32(5 * fd)
    w[0, 20:, 0] = 0
    _, st = R.build_segments(w, [[0]], [[1.0]], [0.0], fd, R.config(min_segment_duration=0.0), return_state=True)
    assert st["raw"][0][2] == np.float32(20 * fd)


def test_raw_order_rule_decides_equal_start_merges():
    """Two clusters open at frame 0 and both close at frame 10; cluster 1 also speaks again right after.  The raw order (closing frame,
    cluster) puts S1's segment first, so after the stable start sort S2's two pieces are adjacent and merge."""
    fd = 0.1
    w = np.zeros((1, 40, 2), np.float32)
    w[0, 0:10, :] = 1
    w[0, 12:40, 1] = 1
    segs, st = R.build_segments(w, [[0, 1]], [[1.0], [1.0]], [0.0], fd, R.config(exclusive=False, min_segment_duration=0.0,
                                                                                   min_gap_duration=0.3), return_state=True)
    assert [s[0] for s in st["raw"]] == ["S1", "S2", "S2"]
    assert shape(segs) == [("S1", 0.0, float(np.float32(10 * fd))), ("S2", 0.0, float(np.float32(39 * fd + fd)))]


# ---- the pure host entries of the library
def test_chunk_assignments_match_restatement(fa):
    rng = np.random.default_rng(3)
    for trial in range(20):
        C, S, K = int(rng.integers(1, 30)), int(rng.integers(1, 5)), int(rng.integers(0, 9))
        n = int(rng.integers(0, 200))
        ci = rng.integers(-2, C + 2, n)
        si = rng.integers(-1, S + 1, n)
        lab = rng.integers(-3, K + 2, n)           # duplicates of (chunk, speaker): the later embedding wins
        got = fa.chunk_assignments(ci, si, lab, K, C, S)
        assert np.array_equal(got, R.chunk_assignments(ci, si, lab, K, C, S)), trial


def random_raw(rng, n, grid):
    segs = []
    for _ in range(n):
        a = float(rng.integers(0, 200)) * grid
        b = a + float(rng.integers(0, 60)) * grid
        segs.append((f"S{int(rng.integers(1, 4))}", np.float32(a), np.float32(b), np.float32(rng.uniform(-0.2, 1.2))))
    return segs


def test_finalize_matches_restatement(fa):
    rng = np.random.default_rng(11)
    for trial in range(60):
        grid = [0.05, 0.1, 10 / 589][trial % 3]    # equal starts (ties of the stable sorts), gaps at and around the threshold
        raw = random_raw(rng, int(rng.integers(0, 80)), grid)
        kw = dict(min_gap_duration=float(rng.choice([0.0, 0.1, 0.15])), min_segment_duration=float(rng.choice([0.0, 0.2, 1.0])),
                  min_duration_on=float(rng.choice([0.0, 0.3])), min_duration_off=float(rng.choice([0.0, 0.2])), exclusive=bool(trial % 2))
        want = R.finalize(raw, R.config(**kw))
        got = fa.finalize_segments([fa.TimedSpeakerSegment(s[0], float(s[1]), float(s[2]), float(s[3])) for s in raw], fa.ReconstructionConfig(**kw))
        assert [(g.speaker_id, np.float32(g.start_time_seconds), np.float32(g.end_time_seconds), np.float32(g.quality_score)) for g in got] == \
            [(w[0], w[1], w[2], w[3]) for w in want], trial


def test_host_entries_reject_bad_arguments(fa):
    import ctypes as C
    L = fa._lib
    cnt = C.c_int64()
    cfg = fa.ReconstructionConfig().c_config()
    assert L.lib().fa_segments_finalize(None, None, 0, None, 0, C.byref(cnt)) == L.INVALID_ARGUMENT
    assert L.lib().fa_segments_finalize(C.byref(cfg), None, 3, None, 0, C.byref(cnt)) == L.INVALID_ARGUMENT
    assert L.lib().fa_segments_finalize(C.byref(cfg), None, 0, None, 0, C.byref(cnt)) == L.SUCCESS and cnt.value == 0
    assert L.lib().fa_offline_chunk_assignments(2, None, None, None, 1, 1, 1, None) == L.INVALID_ARGUMENT
    c = L.ReconstructConfig()
    L.lib().fa_reconstruct_default_config(C.byref(c))
    assert (c.window_duration, c.frame_duration, c.min_segment_duration, c.min_gap_duration, c.exclusive, c.zero_vote_enabled,
            c.zero_vote_min_duration) == (10.0, 0.0, 1.0, 0.1, 1, 0, 0.4)


# ---- which entry an input reaches: a CPU tensor's pointer is host memory and must never be handed to a _dev entry
class _SpyLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


class _StubCtx:
    handle, device = None, 0

    def check(self, st, where):
        assert st == 0, where

    def torch_ordered(self, enabled=True):
        import contextlib
        return contextlib.nullcontext()


def test_cpu_tensors_take_the_host_entries(fa, monkeypatch):
    import torch
    spy = _SpyLib()
    monkeypatch.setattr(fa.reconstruct.L, "lib", lambda: spy)
    x = torch.zeros((2, 5, 7))
    seg = fa.powerset_decode(x, ctx=_StubCtx())
    assert spy.calls == ["fa_powerset_decode"] and isinstance(seg.speaker_weights, np.ndarray)
    spy.calls.clear()
    rec = fa.OfflineReconstruction(ctx=_StubCtx())
    assert rec.build_segments(fa.SegmentationOutput(torch.ones((2, 5, 3))), np.zeros((2, 3)), np.zeros((1, 2))) == []
    assert "fa_offline_reconstruct" in spy.calls and "fa_offline_reconstruct_dev" not in spy.calls


def test_chunk_assignments_refuses_mismatched_lengths(fa):
    with pytest.raises(ValueError):
        fa.chunk_assignments([0, 1], [0], [0, 0], 2, 2, 3)
