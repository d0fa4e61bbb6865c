"""What pins tests/sortformer_restatement.py without a GPU: the reference's own known-answer cases (Tests/FluidAudioTests/Diarizer/
Sortformer/OfflineSortformerTests.swift:11-98, Diarizer/DiarizerTimelineMergeTests.swift:53-161, Diarizer/Sortformer/
SortformerTimelineTests.swift:139-197, 221-259, 428-443), hand-derived window geometry, and the library's host-only entries against it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sortformer_restatement as R  # noqa: E402

F = np.float32


# ---------------------------------------------------------------- stitcher (OfflineSortformerTests.swift:11-85)

def stitcher_cases():
    ns = 4
    g = np.zeros((4, ns), np.float32)
    for f in range(4):
        g[f, f % ns] = 1
    yield "identity", g, g.copy(), 4
    perm = [2, 0, 3, 1]
    g, w = np.zeros((8, ns), np.float32), np.zeros((8, ns), np.float32)
    for f in range(8):
        g[f, f % ns] = 1
        w[f, perm[f % ns]] = 1
    yield "permutation", g, w, 8
    g, w = np.full((3, ns), 0.1, np.float32), np.full((3, ns), 0.1, np.float32)
    g[:, 1] = 0.9
    w[:, 3] = 0.9
    yield "soft", g, w, 3
    yield "zero", np.zeros((0, ns), np.float32), np.zeros((0, ns), np.float32), 0
    g, w = np.zeros((5, ns), np.float32), np.zeros((5, ns), np.float32)
    for f in range(5):
        g[f, f % ns] = f + 1
        w[f, (f + 2) % ns] = f + 1
    yield "bijection", g, w, 5


def check_stitcher(align):
    for name, g, w, frames in stitcher_cases():
        m = align(g, w, frames, 4)
        if name in ("identity", "zero"):
            assert m == [0, 1, 2, 3], name
        elif name == "permutation":
            for f in range(frames):
                for col in range(4):
                    if w[f, col] > 0:
                        assert m[col] == f % 4
            assert m == [1, 3, 0, 2]                      # the inverse of perm[g] = w = [2, 0, 3, 1]
        elif name == "soft":
            assert m[3] == 1
        else:
            assert set(m) == set(range(4))


def test_stitcher_reference_cases():
    check_stitcher(R.alignment)


def test_stitcher_host_entry_matches(fa):
    check_stitcher(fa.stitcher_alignment)
    rng = np.random.default_rng(0)
    for s in (1, 2, 3, 4):
        for _ in range(20):
            n = int(rng.integers(1, 40))
            g = rng.random((n, s)).astype(np.float32) * (rng.random((n, s)) < 0.7)
            w = rng.random((n, s)).astype(np.float32)
            if rng.random() < 0.3:
                w[:, -1] = w[:, 0]                        # an exact tie between two columns
            if rng.random() < 0.2:
                w[rng.integers(n), rng.integers(s)] = [np.nan, np.inf, -np.inf][int(rng.integers(3))]
            assert fa.stitcher_alignment(g, w, n, s) == R.alignment(g, w, n, s)
    assert fa.lib().fa_sortformer_stitcher_alignment(None, None, 3, 5, np.zeros(5, np.int32).ctypes.data) == fa.INVALID_ARGUMENT


def test_permutation_enumeration_order():
    p = R.permutations(4)
    assert len(p) == 24 and len({tuple(x) for x in p}) == 24
    assert p[:7] == [[0, 1, 2, 3], [0, 1, 3, 2], [0, 2, 1, 3], [0, 2, 3, 1], [0, 3, 2, 1], [0, 3, 1, 2], [1, 0, 2, 3]]
    assert p != sorted(p)                                 # the swap recursion, not lexicographic
    assert R.permutations(3) == [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 1, 0], [2, 0, 1]]


def test_ties_go_to_the_first_enumerated_and_nan_never_wins():
    z = np.zeros((6, 4), np.float32)
    assert R.alignment(z, z, 6, 4) == [0, 1, 2, 3]        # all scores 0: the first enumerated (identity)
    g = np.ones((2, 4), np.float32)
    assert R.alignment(g, np.full((2, 4), np.nan, np.float32), 2, 4) == [0, 1, 2, 3]   # every score NaN: identity stays
    w = np.ones((2, 4), np.float32)
    w[0, 2] = np.nan                                      # correlations [g][2] are NaN: every bijection uses column 2 once
    assert R.alignment(g, w, 2, 4) == [0, 1, 2, 3]


# ---------------------------------------------------------------- config and geometry

def test_offline_config_defaults(fa):   # OfflineSortformerTests.swift:89-98
    for cfg in (R.OfflineConfig(), fa.OfflineSortformerConfig()):
        assert getattr(cfg, "window_output_frames") == 384
        assert getattr(cfg, "subsampling", getattr(cfg, "subsampling_factor", None)) == 8
        assert cfg.window_mel_frames == 3072
        assert getattr(cfg, "speakers", getattr(cfg, "num_speakers", None)) == 4
        assert abs(float(cfg.frame_duration_seconds) - 0.08) <= 1e-6
        assert cfg.overlap_output_frames == 100
    c = fa._lib.SortformerOfflineConfig()
    fa.lib().fa_sortformer_offline_default_config(C.byref(c))
    assert (c.window_output_frames, c.subsampling, c.speakers, c.n_mels, c.overlap_output_frames) == (384, 8, 4, 128, 100)
    t = fa._lib.TimelineConfig()
    fa.lib().fa_timeline_default_config(C.byref(t))
    assert (t.onset_threshold, t.offset_threshold, t.onset_pad_frames, t.offset_pad_frames, t.min_frames_on, t.min_frames_off, t.speakers,
            t.activity_type) == (0.5, 0.5, 0, 0, 0, 0, 4, 0)
    assert F(t.frame_duration) == F(0.08)


def W(mel_start, valid_mel, g_start, valid_out):
    return dict(mel_start=mel_start, valid_mel=valid_mel, g_start=g_start, valid_out=valid_out)


def test_window_geometry_by_hand():
    """Default config: windowMel 3 072, hopMel (384 - 100) * 8 = 2 272."""
    cfg = R.OfflineConfig()
    assert R.offline_windows(cfg, 0) == ([], 0)
    assert R.offline_windows(cfg, 1) == ([W(0, 1, 0, 1)], 1)
    assert R.offline_windows(cfg, 2272) == ([W(0, 2272, 0, 284)], 284)                       # shorter than a window: one, and the break
    assert R.offline_windows(cfg, 2273) == ([W(0, 2273, 0, 285)], 285)
    # exactly one window: it is full, so the loop goes on and finds 800 more valid frames inside it
    assert R.offline_windows(cfg, 3072) == ([W(0, 3072, 0, 384), W(2272, 800, 284, 100)], 384)
    assert R.offline_windows(cfg, 3073) == ([W(0, 3072, 0, 384), W(2272, 801, 284, 101)], 385)
    wins, total = R.offline_windows(cfg, 2880001)                                           # 8 h at 100 mel frames per second, centre padded
    assert total == 360001 and len(wins) == 1268                                            # ceil((2 880 001 - 3 072) / 2 272) + 1
    assert wins[-1] == W(1267 * 2272, 2880001 - 1267 * 2272, 1267 * 284, (2880001 - 1267 * 2272 + 7) // 8)
    assert all(w["valid_mel"] == 3072 and w["mel_start"] == i * 2272 for i, w in enumerate(wins[:-1]))
    # the clamp overlapOut = max(0, min(overlap, window - 1)): windowMel 8, hopMel 2; the window at 14 holds 6 < 8 frames and is the last
    assert [w["mel_start"] for w in R.offline_windows(R.OfflineConfig(4, 2, 4, 8, 99), 20)[0]] == [0, 2, 4, 6, 8, 10, 12, 14]
    assert [w["mel_start"] for w in R.offline_windows(R.OfflineConfig(4, 2, 4, 8, -5), 20)[0]] == [0, 8, 16]


def test_windows_entry_matches_the_restatement(fa):
    rng = np.random.default_rng(1)
    cases = [(R.OfflineConfig(), [0, 1, 2272, 2273, 3072, 3073, 5344, 5345, 100000, 2880001])]
    for _ in range(30):
        win = int(rng.integers(1, 40))
        cfg = R.OfflineConfig(win, int(rng.integers(1, 9)), 4, 16, int(rng.integers(-3, win + 5)))
        cases.append((cfg, [int(v) for v in rng.integers(0, 50 * win * cfg.subsampling, 6)]))
    for cfg, lengths in cases:
        got = fa.offline_windows(lengths, fa.OfflineSortformerConfig(cfg.window_output_frames, cfg.subsampling, cfg.speakers, cfg.n_mels,
                                                                     cfg.overlap_output_frames))
        rows, totals, rng_ = [], [], [0]
        for b, n in enumerate(lengths):
            wins, total = R.offline_windows(cfg, n)
            rows += [(b, w["valid_mel"], w["valid_out"], int(i == 0), w["mel_start"], w["g_start"]) for i, w in enumerate(wins)]
            totals.append(total)
            rng_.append(len(rows))
        assert got["windows"].tolist() == rows
        assert got["total_out"].tolist() == totals and got["window_range"].tolist() == rng_


def test_windows_entry_statuses(fa):
    f = fa.lib().fa_sortformer_offline_windows
    cfg = fa.OfflineSortformerConfig().c_config()
    n = np.array([3072], np.int64)
    cnt = C.c_int64()
    assert f(None, n.ctypes.data, 1, None, 0, C.byref(cnt), None, None) == fa.INVALID_ARGUMENT
    assert f(C.byref(cfg), n.ctypes.data, 1, None, 0, None, None, None) == fa.INVALID_ARGUMENT
    assert f(C.byref(cfg), n.ctypes.data, 1, None, 0, C.byref(cnt), None, None) == fa.SUCCESS and cnt.value == 2
    one = np.zeros(1, fa.sortformer.WINDOW_DTYPE)
    assert f(C.byref(cfg), n.ctypes.data, 1, one.ctypes.data, 1, C.byref(cnt), None, None) == 3 and cnt.value == 2   # OUTPUT_TOO_SMALL
    bad = np.array([-1], np.int64)
    assert f(C.byref(cfg), bad.ctypes.data, 1, None, 0, C.byref(cnt), None, None) == fa.INVALID_ARGUMENT
    cfg.subsampling = 0
    assert f(C.byref(cfg), n.ctypes.data, 1, None, 0, C.byref(cnt), None, None) == fa.INVALID_ARGUMENT


def test_overlap_region_is_the_previous_windows_values():
    """The claim behind the device's parallel path: with 2 * overlap <= window the window-by-window timeline equals the one whose
    alignments read the previous window's own values."""
    rng = np.random.default_rng(3)
    for cfg, n in ((R.OfflineConfig(), 7 * 2272 + 900), (R.OfflineConfig(), 3 * 2272 + 800), (R.OfflineConfig(24, 2, 4, 8, 12), 24 * 2 * 4 + 5),
                   (R.OfflineConfig(24, 2, 3, 8, 5), 24 * 2 * 6)):
        wins, _ = R.offline_windows(cfg, n)
        preds = rng.random((len(wins), cfg.window_output_frames, cfg.speakers)).astype(np.float32)
        preds[rng.random(preds.shape) < 0.2] = 0
        a, ma = R.stitch(cfg, n, preds)
        b, mb = R.stitch_from_previous(cfg, n, preds)
        assert np.array_equal(ma, mb) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert len({tuple(m) for m in ma.tolist()}) > 1     # the alignments are not all the identity


# ---------------------------------------------------------------- timeline

MERGE = R.TimelineConfig(num_speakers=1, frame_duration_seconds=0.1, onset_pad_frames=2, offset_pad_frames=2, min_frames_on=4, min_frames_off=3)


def run_finalized(pred, config=MERGE):
    t = R.Timeline(config)
    t.add_chunk(pred)
    t.finalize()
    return t.speakers[0].finalized_segments if 0 in t.speakers else []


def preds(n, *runs):
    p = np.zeros(n, np.float32)
    for lo, hi in runs:
        p[lo:hi + 1] = 0.9
    return p


def test_merge_short_segment_after_small_gap_keeps_prior():   # DiarizerTimelineMergeTests.swift:53-67
    s = run_finalized(preds(30, (5, 14), (19, 20)))
    assert [(x.start_frame, x.end_frame) for x in s] == [(3, 17)]


def test_merge_small_gap_merges_two_long_segments():          # :70-84
    s = run_finalized(preds(40, (5, 14), (19, 28)))
    assert [(x.start_frame, x.end_frame) for x in s] == [(3, 31)]


def test_merge_trailing_tentative_short_tail():               # :89-104
    _, tent = R.Timeline(MERGE).add_chunk((), preds(22, (5, 14), (19, 21)))
    assert [(x.start_frame, x.end_frame) for x in tent] == [(3, 17)] and abs(float(tent[0].activity) - 0.9) <= 1e-5


def test_merge_segment_in_buffer_zone_survives_next_chunk():  # :111-144
    t = R.Timeline(MERGE)
    t.add_chunk(preds(22, (5, 14)))
    t.add_chunk(np.zeros(22, np.float32))
    t.finalize()
    assert [(x.start_frame, x.end_frame) for x in t.speakers[0].finalized_segments] == [(3, 17)]


def test_merge_trailing_tentative_long_tail():                # :148-161
    _, tent = R.Timeline(MERGE).add_chunk((), preds(29, (5, 14), (19, 28)))
    assert [(x.start_frame, x.end_frame) for x in tent] == [(3, 31)] and abs(float(tent[0].activity) - 0.9) <= 1e-5


def test_confidence_excludes_padding_frames():                # SortformerTimelineTests.swift:139-167
    s = run_finalized([0.0, 0.8, 0.6, 0.0], R.TimelineConfig(1, 0.08, 0.5, 0.5, 1, 2, 0, 0))
    assert (s[0].start_frame, s[0].end_frame) == (0, 5) and abs(float(s[0].activity) - 0.7) <= 1e-6


def test_confidence_excludes_bridged_gap_frames():            # :169-197
    s = run_finalized([0.9, 0.0, 0.7, 0.7, 0.0], R.TimelineConfig(1, 0.08, 0.5, 0.5, 0, 0, 0, 1))
    assert (s[0].start_frame, s[0].end_frame) == (0, 4) and abs(float(s[0].activity) - (0.9 + 0.7 + 0.7) / 3.0) <= 1e-6


def test_rebuild():                                           # :428-443 (boundedSpeaker0Predictions :265-271)
    p = np.zeros((16, 4), np.float32)
    p[:8, 0] = 0.9
    fin, tent = R.Timeline(R.TimelineConfig.sortformer_default()).rebuild(p, (), True)
    assert [(x.speaker_index, x.start_frame, x.end_frame, x.finalized) for x in fin] == [(0, 0, 8, True)] and tent == []


def test_segment_time_conversion(fa):                         # :221-227, 249-259
    for seg in (R.Segment(0, 10, 20, True, 0.08), fa.DiarizerSegment(0, 10, 20, True, 0.08)):
        assert abs(float(seg.start_time) - 0.8) <= 1e-5 and abs(float(seg.end_time) - 1.6) <= 1e-5 and abs(float(seg.duration) - 0.8) <= 1e-5
        assert seg.length == 10
    for seg in (R.Segment.from_times(1, 0.8, 1.6, 0.08), fa.DiarizerSegment.from_times(1, 0.8, 1.6, 0.08)):
        assert (seg.start_frame, seg.end_frame, seg.speaker_index) == (10, 20, 1)
    a = R.TimelineConfig.from_seconds(1, 0.08, 0.5, 0.5, 0.12, 0.2, 0.04, 0.36)       # 1.5, 2.5, 0.5, 4.5 frames in fp32: half away from zero
    b = fa.DiarizerTimelineConfig.from_seconds(1, 0.08, 0.5, 0.5, 0.12, 0.2, 0.04, 0.36)
    want = tuple(R.swift_round(F(F(x) / F(0.08))) for x in (0.12, 0.2, 0.04, 0.36))
    assert (a.onset_pad_frames, a.offset_pad_frames, a.min_frames_on, a.min_frames_off) == want
    assert (b.onset_pad_frames, b.offset_pad_frames, b.min_frames_on, b.min_frames_off) == want
    assert R.swift_round(2.5) == 3 and R.swift_round(-2.5) == -3 and R.swift_round(0.49999997) == 0


def test_rebuild_equals_one_chunk_then_finalize():
    """rebuild(isComplete: true) and addChunk + finalize walk the same code: the same lists."""
    rng = np.random.default_rng(5)
    cfg = R.TimelineConfig(3, 0.08, 0.6, 0.4, 1, 2, 3, 2)
    p = np.clip(np.cumsum(rng.normal(0, 0.15, (400, 3)), axis=0) % 1.0, 0, 1).astype(np.float32)
    a, b = R.Timeline(cfg), R.Timeline(cfg)
    a.rebuild(p[:300], p[300:], True)
    b.add_chunk(p[:300], p[300:])
    b.finalize()
    assert a.records() == b.records() and len(a.records()) > 3


def test_timeline_entry_statuses_need_no_gpu(fa):
    f = fa.lib().fa_timeline_segments_dev
    cnt = C.c_int64(7)
    cfg = fa.DiarizerTimelineConfig.sortformer_default().c_config()
    assert f(None, C.byref(cfg), None, None, None, None, 0, 1, None, 0, C.byref(cnt), None) == fa.INVALID_ARGUMENT
    with pytest.raises(KeyError):
        fa.DiarizerTimelineConfig(activity_type="softmax").c_config()
