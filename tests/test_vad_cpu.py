"""The restatement of the reference's VAD routines (tests/vad_restatement.py) against the reference's own XCTest cases
(Tests/FluidAudioTests/VAD/VadSegmentationTests.swift, VadStreamingTests.swift, built with makeVadResults' recipe), against sample
ranges worked out by hand from the Swift lines, and on the rules the device kernels lean on: the first of equal maxima, the flushes of
one frame, the bound on a recording's raw speeches and the trip of a sample index through fp64 seconds.  No GPU."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vad_restatement as R  # noqa: E402

CHUNK_SECONDS = R.CHUNK / float(R.RATE)


def segments(pattern, cfg=None):
    probs, total = R.make_vad_results(pattern)
    return R.segment_speech(probs, total, cfg)


def durations(segs):
    return [e - s for _, _, s, e in segs]


def ranges(segs):
    return [(a, b) for a, b, _, _ in segs]


# ---- VadSegmentationTests.swift, assertion by assertion
def test_silence_produces_no_segments():
    assert segments([(False, 2.0)]) == []


def test_continuous_speech_produces_segment():
    segs = segments([(True, 5.0)])
    assert len(segs) == 1 and sum(durations(segs)) > 5.0 * 0.9


def test_single_segment_amid_silence():
    segs = segments([(False, 1.0), (True, 3.0), (False, 1.0)], R.Config(minSpeechDuration=0.15))
    assert len(segs) == 1 and 2.7 < durations(segs)[0] < 3.4


def test_multiple_segments_separated_by_silence():
    cfg = R.Config(minSpeechDuration=0.15, minSilenceDuration=0.75)
    assert len(segments([(False, 1.0), (True, 2.0), (False, 1.0), (True, 2.0), (False, 1.0)], cfg)) == 2


def test_merging_within_min_silence():
    segs = segments([(True, 1.0), (False, 0.5), (True, 1.0)], R.Config(minSpeechDuration=0.15, minSilenceDuration=0.75))
    assert len(segs) == 1 and 2.4 < durations(segs)[0] < 2.6


def test_no_merging_beyond_min_silence():
    segs = segments([(True, 1.0), (False, 1.0), (True, 1.0)], R.Config(minSpeechDuration=0.15, minSilenceDuration=0.75))
    assert len(segs) == 2 and all(0.9 < d < 1.3 for d in durations(segs))


def test_min_speech_duration_filter():
    segs = segments([(True, 0.2), (False, 1.0), (True, 0.8), (False, 1.0), (True, 0.1)], R.Config(minSpeechDuration=0.5, minSilenceDuration=0.75))
    assert len(segs) == 1 and 0.7 < durations(segs)[0] < 1.1


def test_split_long_continuous_speech():
    segs = segments([(True, 30.0)], R.Config(minSpeechDuration=0.15, maxSpeechDuration=15.0))
    assert len(segs) >= 2 and all(d < 15.1 for d in durations(segs))


def test_max_speech_duration_enforcement():
    segs = segments([(True, 25.0)], R.Config(minSpeechDuration=0.15, maxSpeechDuration=10.0))
    assert len(segs) >= 3 and all(d < 10.1 for d in durations(segs))


def test_exactly_max_duration_segment():
    probs, total = R.make_vad_results([(True, 5.0)])
    exact = CHUNK_SECONDS * len(probs)
    segs = R.segment_speech(probs, total, R.Config(minSpeechDuration=0.15, maxSpeechDuration=exact))
    assert len(segs) == 1 and abs(durations(segs)[0] - exact) <= CHUNK_SECONDS


def test_alternating_speech_silence():
    assert len(segments([(True, 0.3), (False, 0.3)] * 5, R.Config(minSpeechDuration=0.1, minSilenceDuration=0.2))) >= 1


def test_custom_segmentation_config():
    cfg = R.Config(minSpeechDuration=1.0, minSilenceDuration=2.0, maxSpeechDuration=8.0, speechPadding=0.2, silenceThresholdForSplit=0.5)
    segs = segments([(True, 20.0)], cfg)
    assert len(segs) >= 3 and all(d < 8.1 for d in durations(segs))


def test_real_world_pattern():
    segs = segments([(True, 5.0), (False, 85.0), (True, 30.0)], R.Config(minSpeechDuration=0.15, minSilenceDuration=0.75, maxSpeechDuration=15.0))
    assert 3 <= len(segs) <= 4 and all(d < 15.1 for d in durations(segs))


def test_empty_input():
    assert R.segment_speech([], 0) == []


def test_very_short_speech_filtered():
    assert segments([(True, 0.05)], R.Config(minSpeechDuration=0.15)) == []


# ---- exact sample ranges, from the Swift lines
def test_exact_sample_ranges():
    assert ranges(segments([(True, 1), (False, .5), (True, 1)])) == [(0, 40960)]
    # [(true, 1), (false, 1), (true, 1)] is 4 + 4 + 4 chunks of 4096 samples, 49152 in all; defaults: minSilence = Int(0.75 * 16000) = 12000,
    # pad = Int(0.1 * 16000) = 1600, negative threshold 0.85 - 0.15.  Frame 0 (0.95) triggers at 0.  Frame 4 (0.05, start 16384) opens the
    # silence: tempEnd = 16384.  Frames 5, 6 are 4096 and 8192 samples in, below 12000; frame 7 (start 28672) is 12288 >= 12000 in: the
    # speech (0, 16384) is flushed.  Frame 8 (start 32768) triggers again and the tail flush gives (32768, 49152).  Padding: the first
    # start stays max(0, 0 - 1600) = 0; the gap 32768 - 16384 = 16384 is not below 2 * 1600, so 16384 + 1600 = 17984 and
    # 32768 - 1600 = 31168; the last end is min(49152, 49152 + 1600) = 49152.
    assert ranges(segments([(True, 1), (False, 1), (True, 1)])) == [(0, 17984), (31168, 49152)]
    assert ranges(segments([(False, 1), (True, 3), (False, 1)])) == [(14784, 67136)]
    assert ranges(segments([(True, 30)], R.Config(maxSpeechDuration=15))) == [(0, 235072), (235968, 472640), (473536, 479232)]
    for s, e, st, et in segments([(True, 30)], R.Config(maxSpeechDuration=15)):
        assert (st, et) == (s / 16000.0, e / 16000.0)


def test_the_first_of_equal_maxima_is_the_split():
    """Two silences of two frames each, both with a minimum above silenceThresholdForSplit: the cut takes the longest one, and of the two
    equal ones the first (Sequence.max(by:) replaces its result only by a strictly greater element)."""
    cfg = R.Config(maxSpeechDuration=3.0, minSilenceDuration=2.0, speechPadding=0.0, silenceThresholdForSplit=0.1, minSilenceAtMaxSpeech=0.098)
    H, L = 0.95, 0.5
    probs = np.array([H, H, L, L, H, H, L, L, H] + [H] * 8, np.float32)
    assert R.first_max([(1, 5, 0), (2, 5, 0), (3, 4, 0)]) == (1, 5, 0)
    before = R.BRANCHES["split_longest"]
    got = ranges(R.segment_speech(probs, len(probs) * R.CHUNK, cfg))
    assert R.BRANCHES["split_longest"] > before
    assert got[0] == (0, 2 * R.CHUNK) and got[1][0] == 4 * R.CHUNK               # split at the FIRST silence, resumed behind it
    last = R.Config(maxSpeechDuration=3.0, minSilenceDuration=2.0, speechPadding=0.0, silenceThresholdForSplit=0.1, useMaxPossibleSilenceAtMaxSpeech=False)
    assert ranges(R.segment_speech(probs, len(probs) * R.CHUNK, last))[0] == (0, 6 * R.CHUNK)      # useMax off: the last one


def test_min_silence_zero_and_the_flushes_of_one_frame():
    """The cut that resumes lets its frame go on to the end-of-speech test (:163-196), which looks like two flushes in one frame once
    minSilenceSamples is 0.  It cannot happen: with minSilenceSamples == 0 the first low frame of a speech ends it at once (frameStart -
    tempEnd is 0), so no silence ever stays open until a high frame records it as a candidate, every cut is a hard one and does not
    resume; and with minSilenceSamples > 0 the cut clears tempEnd, the end test opens its silence at this very frame and 0 >= minSilence
    fails.  Walked over every sequence of 7 frames: no frame index appears twice among the flushes, for minSilenceDuration 0 and above."""
    zero = R.Config(minSpeechDuration=0.0, minSilenceDuration=0.0, maxSpeechDuration=0.9, speechPadding=0.0, minSilenceAtMaxSpeech=0.0,
                    negativeThreshold=0.5, negativeThresholdOffset=0.2)
    some = R.Config(minSpeechDuration=0.0, minSilenceDuration=0.3, maxSpeechDuration=0.9, speechPadding=0.0, minSilenceAtMaxSpeech=0.0,
                    negativeThreshold=0.5, negativeThresholdOffset=0.2)
    assert R.sample_counts(zero)["minSilence"] == 0 and R.sample_counts(zero)["maxSpeech"] == 14400 - 4096
    resumed, recorded = R.BRANCHES["resumed"], R.BRANCHES["candidate_recorded"]
    for seq in itertools.product((0.9, 0.6, 0.1), repeat=7):
        log = []
        R.raw_speeches(np.array(seq, np.float32), 7 * R.CHUNK, R.thresholds(zero)[0], zero, log)
        assert len(set(log)) == len(log), (seq, log)
    assert (R.BRANCHES["resumed"], R.BRANCHES["candidate_recorded"]) == (resumed, recorded)       # minSilence 0: never a candidate, never resumed
    for seq in itertools.product((0.9, 0.6, 0.1), repeat=7):
        log = []
        R.raw_speeches(np.array(seq, np.float32), 7 * R.CHUNK, R.thresholds(some)[0], some, log)
        assert len(set(log)) == len(log), (seq, log)
    assert R.BRANCHES["resumed"] > resumed                                       # the resuming cut was among them
    # the cut and the silence it leaves open, literally: high, low (candidate at frame 2), high, high; the cut at frame 3 resumes at frame 2
    assert R.raw_speeches(np.array([0.9, 0.1, 0.9, 0.9, 0.1], np.float32), 5 * R.CHUNK, R.thresholds(some)[0], some) == [(0, R.CHUNK), (2 * R.CHUNK, 5 * R.CHUNK)]


def test_a_recording_has_at_most_one_raw_speech_per_frame():
    """The workspace of fa_vad_segments holds one raw speech per frame: what the flushes append are disjoint speeches that each start on
    a frame of their own, so F frames bound their number (not 2 F + 1).
    Every sequence of up to 8 frames over the three bands, for configs with cuts at every frame, zero durations and short totals."""
    configs = [R.Config(),
               R.Config(minSilenceDuration=0, minSpeechDuration=0, maxSpeechDuration=0.3, speechPadding=0, minSilenceAtMaxSpeech=0),
               R.Config(minSilenceDuration=0, minSpeechDuration=0, maxSpeechDuration=0.6, speechPadding=0, minSilenceAtMaxSpeech=0, useMaxPossibleSilenceAtMaxSpeech=False),
               R.Config(minSilenceDuration=0.3, minSpeechDuration=0, maxSpeechDuration=0.9, speechPadding=0.01, minSilenceAtMaxSpeech=0)]
    reached = 0
    for cfg in configs:
        thr = R.thresholds(cfg)[0]
        for n in range(1, 9):
            for seq in itertools.product((0.9, 0.1, 0.75), repeat=n):
                for total in (n * R.CHUNK, n * R.CHUNK - 100, 5000):
                    raw = R.raw_speeches(seq, total, thr, cfg)
                    assert len(raw) <= n, (seq, total, raw)
                    starts = [a for a, _ in raw]                                 # the ends are clamped to the total, the starts are not
                    assert all(a % R.CHUNK == 0 for a in starts) and starts == sorted(set(starts))
                    reached += len(raw) == n
    assert reached > 0                                                           # the bound is met, e.g. by cuts at every frame


def test_time_round_trip_loses_a_sample():
    """segmentSpeechAudio cuts at Int(time * 16000.0), not at the sample the time was formed from."""
    assert int(float(1001) / 16000.0 * 16000.0) == 1000
    assert R.segment_bounds(1001 / 16000.0, 2000 / 16000.0, 5000) == (1000, 2000)
    assert sum(int(float(i) / 16000.0 * 16000.0) != i for i in range(2 * 10 ** 6)) == 11806
    assert R.segment_bounds(0.5, 9.0, 5000) == (5000, 5000) and R.segment_bounds(-1.0, 0.25, 5000) == (0, 4000)


def test_pack_chunks_rows():
    x = np.arange(1, 2 * R.CHUNK + 6, dtype=np.float32)
    rows = R.pack_chunks(x)
    assert rows.shape == (3, R.ROW) and R.chunk_count(x.size) == 3 and R.chunk_count(0) == 0 and R.chunk_count(R.CHUNK) == 1
    assert not rows[0, :R.CONTEXT].any() and np.array_equal(rows[0, R.CONTEXT:], x[:R.CHUNK])
    assert np.array_equal(rows[1, :R.CONTEXT], x[R.CHUNK - R.CONTEXT:R.CHUNK]) and np.array_equal(rows[2, :R.CONTEXT], x[2 * R.CHUNK - R.CONTEXT:2 * R.CHUNK])
    assert np.array_equal(rows[2, R.CONTEXT:R.CONTEXT + 5], x[2 * R.CHUNK:]) and (rows[2, R.CONTEXT + 5:] == x[-1]).all()
    short = R.pack_chunks(np.array([3.0, 7.0], np.float32))                      # the context behind a padded chunk is the padding
    assert short.shape == (1, R.ROW) and short[0, R.CONTEXT] == 3.0 and (short[0, R.CONTEXT + 1:] == 7.0).all()


# ---- VadStreamingTests.swift
def test_streaming_emits_start_and_end_events():
    cfg, state = R.Config(), R.StreamState()
    state, event = R.stream_step(0.9, R.CHUNK, state, cfg)
    assert event[:2] == (R.START, 0) and state.triggered
    captured = None
    for _ in range(5):
        state, event = R.stream_step(0.05, R.CHUNK, state, cfg)
        if event:
            captured = event
            break
    assert captured is not None and captured[0] == R.END and not state.triggered and captured[1] > 0


def test_streaming_returns_seconds_when_requested():
    cfg, state = R.Config(), R.StreamState()
    state, _ = R.stream_step(0.9, R.CHUNK, state, cfg, True, 2)
    end = None
    for _ in range(5):
        state, event = R.stream_step(0.05, R.CHUNK, state, cfg, True, 2)
        if event:
            end = event
            break
    assert end is not None and end[2] == R.swift_rounded(end[1] / 16000.0 * 100) / 100


def test_streaming_respects_threshold_override():
    cfg = R.Config(negativeThreshold=0.2, negativeThresholdOffset=0.05, defaultThreshold=0.8)
    below, event = R.stream_step(0.24, R.CHUNK, R.StreamState(), cfg)
    assert event is None
    _, event = R.stream_step(0.3, R.CHUNK, below, cfg)
    assert event[:2] == (R.START, max(0, R.CHUNK - int(cfg.speechPadding * 16000.0)))


def test_streaming_uses_default_threshold_without_override():
    cfg = R.Config(defaultThreshold=0.6)
    below, event = R.stream_step(0.59, R.CHUNK, R.StreamState(), cfg)
    assert event is None
    _, event = R.stream_step(0.7, R.CHUNK, below, cfg)
    assert event[:2] == (R.START, max(0, R.CHUNK - int(cfg.speechPadding * 16000.0)))


def test_rounding_is_half_away_from_zero():
    assert [R.swift_rounded(x) for x in (0.5, 1.5, 2.5, -0.5, 2.4999)] == [1.0, 2.0, 3.0, -1.0, 2.0]
