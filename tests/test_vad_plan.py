"""The argument pass and the plans of the VAD entries (csrc/vad_launch.h: the thresholds and sample counts derived from a config, every
refusal and the order of the refusals, the offsets and workspace sizes of a ragged batch) walked on the CPU by tests/cpu/vad_plan.cpp
against the expressions restated in tests/vad_restatement.py.  The program is stand-alone, reads its cases from stdin and is built with
the address and undefined-behaviour sanitizers.  No GPU."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vad_restatement as R  # noqa: E402

OK, INVALID_ARGUMENT, INDEX_OVERFLOW, OUTPUT_TOO_SMALL = 0, 1, 2, 3
INT64_MAX = 2 ** 63 - 1


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vad_plan") / "vad_plan")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "vad_plan.cpp"), "-o", exe], check=True)
    return exe


def f32hex(x):
    return f"{struct.unpack('<I', struct.pack('<f', x))[0]:08x}"


def f64hex(x):
    return f"{struct.unpack('<Q', struct.pack('<d', x))[0]:016x}"


def cfg_words(minSpeechDuration=0.15, minSilenceDuration=0.75, maxSpeechDuration=14.0, speechPadding=0.1, silenceThresholdForSplit=0.3, negativeThreshold=None,
              negativeThresholdOffset=0.15, minSilenceAtMaxSpeech=0.098, useMaxPossibleSilenceAtMaxSpeech=True, defaultThreshold=0.85):
    return [f32hex(defaultThreshold), f64hex(minSpeechDuration), f64hex(minSilenceDuration), f64hex(maxSpeechDuration), f64hex(speechPadding),
            f32hex(silenceThresholdForSplit), int(negativeThreshold is not None), f32hex(negativeThreshold or 0.0), f32hex(negativeThresholdOffset),
            f64hex(minSilenceAtMaxSpeech), int(useMaxPossibleSilenceAtMaxSpeech)]


def run(plan, *words):
    r = subprocess.run([plan], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    parts = [p.strip() for p in r.stdout.strip().split("|")]
    return int(parts[0]), parts[1:]


def derive(plan, **kw):
    return run(plan, "derive", *cfg_words(**kw))


def restated(**kw):
    cfg = R.Config(**kw)
    thr, neg = R.thresholds(cfg)
    c = R.sample_counts(cfg)
    ints = [c["minSpeech"], c["pad"], INT64_MAX if c["maxSpeech"] is None else c["maxSpeech"], c["minSilence"], c["minSilenceAtMaxSpeech"], int(cfg.useMaxPossibleSilenceAtMaxSpeech)]
    return OK, [" ".join(f32hex(float(x)) for x in (thr, neg, cfg.silenceThresholdForSplit)), " ".join(str(i) for i in ints)]


CONFIGS = [dict(), dict(maxSpeechDuration=4.0, minSilenceDuration=0.5, speechPadding=0.3, silenceThresholdForSplit=0.05, minSilenceAtMaxSpeech=0.3, useMaxPossibleSilenceAtMaxSpeech=False),
           dict(negativeThreshold=0.4, maxSpeechDuration=6.0, minSilenceDuration=1.5, speechPadding=0.5, silenceThresholdForSplit=0.02), dict(maxSpeechDuration=math.inf),
           dict(minSilenceDuration=0.0), dict(negativeThreshold=0.95, negativeThresholdOffset=0.15), dict(negativeThreshold=0.2, negativeThresholdOffset=0.05, defaultThreshold=0.8),
           dict(defaultThreshold=0.1), dict(defaultThreshold=0.6), dict(maxSpeechDuration=0.3, speechPadding=0.2), dict(minSpeechDuration=0.00007, speechPadding=1e9),
           dict(maxSpeechDuration=5.0e14)]


def test_the_operands_are_the_restated_ones(plan):
    for kw in CONFIGS:
        assert derive(plan, **kw) == restated(**kw), kw
    assert restated()[1] == [" ".join(f32hex(x) for x in (0.85, float(np.float32(0.85) - np.float32(0.15)), 0.3)), f"2400 1600 {224000 - 4096 - 3200} 12000 1568 1"]
    assert derive(plan, negativeThreshold=0.95)[1][0].split()[0] == f32hex(1.0)                # min(1, 0.95 + 0.15)
    assert derive(plan, defaultThreshold=0.1)[1][0].split()[1] == f32hex(0.01)                 # max(0.1 - 0.15, 0.01)
    assert derive(plan, maxSpeechDuration=0.3, speechPadding=0.2)[1][1].split()[2] == "0"      # max(0, 4800 - 4096 - 6400)
    assert derive(plan, maxSpeechDuration=math.inf)[1][1].split()[2] == str(INT64_MAX)
    assert derive(plan, minSpeechDuration=0.00007)[1][1].split()[0] == "1"                     # Int(1.12) truncates


def test_config_refusals_in_the_order_of_the_preconditions(plan):
    texts = {"minSpeechDuration": "minSpeechDuration must be non-negative", "minSilenceDuration": "minSilenceDuration must be non-negative",
             "maxSpeechDuration": "maxSpeechDuration must be positive", "speechPadding": "speechPadding must be non-negative",
             "silenceThresholdForSplit": "silenceThresholdForSplit must be in [0, 1]", "negativeThresholdOffset": "negativeThresholdOffset must be non-negative",
             "minSilenceAtMaxSpeech": "minSilenceAtMaxSpeech must be non-negative", "negativeThreshold": "negativeThreshold must be in [0, 1]"}
    bad = {"minSpeechDuration": -0.1, "minSilenceDuration": -1.0, "maxSpeechDuration": 0.0, "speechPadding": -0.5, "silenceThresholdForSplit": 1.5,
           "negativeThresholdOffset": -0.1, "minSilenceAtMaxSpeech": -0.01, "negativeThreshold": 1.5}
    order = list(texts)
    for i, name in enumerate(order):
        assert derive(plan, **{name: bad[name]}) == (INVALID_ARGUMENT, [texts[name]])
        assert derive(plan, **{n: bad[n] for n in order[i:]}) == (INVALID_ARGUMENT, [texts[name]])   # the first of several
    for name in ("minSpeechDuration", "minSilenceDuration", "maxSpeechDuration", "speechPadding", "minSilenceAtMaxSpeech"):
        assert derive(plan, **{name: math.nan}) == (INVALID_ARGUMENT, [texts[name]])                 # a NaN fails its precondition
    assert derive(plan, silenceThresholdForSplit=math.nan)[0] == derive(plan, negativeThreshold=math.nan)[0] == INVALID_ARGUMENT
    assert derive(plan, maxSpeechDuration=-math.inf)[0] == INVALID_ARGUMENT
    # Int(seconds * 16000.0) traps: 2^63 / 16000 seconds and more, infinities
    fits = 2.0 ** 63 / 16000.0
    for name in ("minSpeechDuration", "minSilenceDuration", "speechPadding", "minSilenceAtMaxSpeech", "maxSpeechDuration"):
        if name != "maxSpeechDuration":
            assert derive(plan, **{name: math.inf}) == (INVALID_ARGUMENT, ["a duration times the sample rate does not fit Int"])
        assert derive(plan, **{name: fits}) == (INVALID_ARGUMENT, ["a duration times the sample rate does not fit Int"])
        assert derive(plan, **{name: 1e300})[0] == INVALID_ARGUMENT
    assert derive(plan, speechPadding=fits * 0.75) == (INVALID_ARGUMENT, ["twice the padding does not fit Int"])
    # Int(0.1 * 16000) - 4096 - 2 * (2^62 - 1024) is below Int.min: Swift traps in the subtraction
    pad = next(x for x in (np.nextafter((2.0 ** 62 - 1024) / 16000.0, math.inf * d, dtype=np.float64) if d else (2.0 ** 62 - 1024) / 16000.0 for d in (0, 1, -1))
               if R.swift_int(float(x) * 16000.0) == 2 ** 62 - 1024)
    assert derive(plan, speechPadding=float(pad), maxSpeechDuration=0.1) == (INVALID_ARGUMENT, ["the maximal speech less the padding does not fit Int"])
    assert derive(plan, speechPadding=float(pad), maxSpeechDuration=1.0)[1][1].split()[1:3] == [str(2 ** 62 - 1024), "0"]
    assert derive(plan, minSpeechDuration=fits * 0.999)[0] == OK


def seg(plan, ranges, totals, cfg=None, device=0, have_probs=1, have_segs=1, capacity=100, have_count=1, B=None, have_ranges=1):
    B = len(totals) if B is None else B
    return run(plan, "seg", *cfg_words(**(cfg or {})), device, have_probs, have_segs, capacity, have_count, B, have_ranges, *(list(ranges) + list(totals) if have_ranges else []))


def test_segment_plan_of_a_ragged_batch(plan):
    frames = [0, 1, 63, 64, 65, 130, 400]
    ranges = [7] + list(7 + np.cumsum(frames))
    totals = [5, 4096, 0, 64 * 4096 - 100, -3, 130 * 4096, 1]
    st, (sizes, recs) = seg(plan, ranges, totals, capacity=500)
    active = [f if t > 0 else 0 for f, t in zip(frames, totals)]                 # no frames or no samples: the recording yields nothing and takes no slot
    raw0 = [0] + list(np.cumsum(active))[:-1]
    assert st == OK and sizes == f"{sum(frames)} {sum(active)} 500"
    want = [(r - 7, o, a, t) for r, o, a, t in zip(ranges, raw0, active, totals)]                  # the host entry uploads from frame_range[0] on
    assert [tuple(int(x) for x in recs.split()[i:i + 4]) for i in range(0, 4 * len(frames), 4)] == want
    st, (sizes, recs) = seg(plan, ranges, totals, device=1, capacity=3)
    assert sizes == f"{sum(frames)} {sum(active)} 3" and [int(x) for x in recs.split()[0::4]] == ranges[:-1]   # the device entry addresses the caller's array
    assert seg(plan, ranges, totals, have_segs=0)[1][0].split()[2] == "0"                           # no output: no arena
    assert seg(plan, [0], [], B=0) == (OK, ["0 0 0", ""])
    assert seg(plan, [], [], B=0, have_ranges=0, have_probs=0)[0] == OK


def test_segment_refusals_and_their_order(plan):
    bad, text = "vad_segments: bad arguments", "minSpeechDuration must be non-negative"
    assert seg(plan, [0, 1], [1], B=-1, have_ranges=0) == (INVALID_ARGUMENT, [bad])
    assert seg(plan, [0, 1], [1], capacity=-1) == seg(plan, [0, 1], [1], have_count=0) == (INVALID_ARGUMENT, [bad])
    assert seg(plan, [0, 1], [1], capacity=-1, cfg=dict(minSpeechDuration=-1.0)) == (INVALID_ARGUMENT, [bad])             # the sizes before the config
    assert seg(plan, [], [], B=1, have_ranges=0, cfg=dict(minSpeechDuration=-1.0)) == (INVALID_ARGUMENT, [text])          # the config before the ranges
    assert seg(plan, [], [], B=1, have_ranges=0) == (INVALID_ARGUMENT, ["vad_segments: frame_range and total_samples are required"])
    assert seg(plan, [-1, 3], [9]) == (INVALID_ARGUMENT, ["vad_segments: frame_range starts below 0"])
    assert seg(plan, [0, 5, 4], [9, 9]) == (INVALID_ARGUMENT, ["vad_segments: frame_range descends at recording 1"])
    assert seg(plan, [0, 2 ** 31], [9]) == (INDEX_OVERFLOW, ["vad_segments: recording 0 has 2^31 frames or more"])
    assert seg(plan, [0, 2 ** 31 - 1], [9])[0] == OK
    assert seg(plan, [0, 2 ** 31, 5], [9, 9])[1] == ["vad_segments: recording 0 has 2^31 frames or more"]                 # recording by recording
    assert seg(plan, [0, 5, 4, 4 + 2 ** 31], [9, 9, 9])[1] == ["vad_segments: frame_range descends at recording 1"]
    assert seg(plan, [0, 5], [9], have_probs=0) == (INVALID_ARGUMENT, ["vad_segments: probs is NULL"])
    assert seg(plan, [0, 5, 4], [9, 9], have_probs=0)[1] == ["vad_segments: frame_range descends at recording 1"]          # the ranges before the array
    assert seg(plan, [3, 3, 3], [9, 9], have_probs=0)[0] == OK                                                            # nothing to read: no array needed


def test_pack_plan_and_refusals(plan):
    lengths = [0, 1, 63, 4095, 4096, 4097, 2 * 4096 + 5]
    offsets = [11] + list(11 + np.cumsum(lengths))
    chunk_range = " ".join(str(x) for x in [0] + list(np.cumsum([R.chunk_count(n) for n in lengths])))
    assert chunk_range == "0 0 1 2 3 4 6 9"
    assert run(plan, "pack", 1, 1, 9, 7, 1, *offsets) == (OK, ["", chunk_range])
    assert run(plan, "pack", 1, 1, 8, 7, 1, *offsets) == (OUTPUT_TOO_SMALL, ["vad_pack_chunks: output holds 8 of 9 rows", chunk_range])      # the ranges are still written
    assert run(plan, "pack", 0, 1, 9, 7, 1, *offsets) == run(plan, "pack", 1, 0, 9, 7, 1, *offsets) == (INVALID_ARGUMENT, ["vad_pack_chunks: audio and rows are required", chunk_range])
    assert run(plan, "pack", 0, 0, 0, 2, 1, 5, 5, 5) == (OK, ["", "0 0 0"])                                                                  # no rows: no array needed
    assert run(plan, "pack", 1, 1, 9, -1, 0)[1][0] == run(plan, "pack", 1, 1, -1, 1, 1, 0, 5)[1][0] == "vad_pack_chunks: bad arguments"
    assert run(plan, "pack", 1, 1, 9, 1, 0) == (INVALID_ARGUMENT, ["vad_pack_chunks: audio_offsets and chunk_range are required", "-1 -1"])
    assert run(plan, "pack", 1, 1, 9, 2, 1, -1, 5, 6)[1][0] == "vad_pack_chunks: audio_offsets starts below 0"
    assert run(plan, "pack", 1, 1, 9, 2, 1, 0, 5, 4) == (INVALID_ARGUMENT, ["vad_pack_chunks: audio_offsets descends at recording 1", "-1 -1 -1"])
    assert run(plan, "pack", 1, 1, 2 ** 40, 1, 1, 0, 4096 * 2 ** 31) == (INDEX_OVERFLOW, ["vad_pack_chunks: more than INT32_MAX rows", f"0 {2 ** 31}"])
    assert run(plan, "pack", 1, 1, 0, 0, 0) == (OK, ["", "-1"])                                                                              # an empty batch writes nothing


def test_gather_plan_and_refusals(plan):
    offsets = [100, 100 + 5000, 100 + 5000 + 70000]
    segs = [(0, 1001 / 16000.0, 2000 / 16000.0), (1, 0.5, 1.0e6), (1, 1.0e6, 2.0e6), (0, -3.0, 0.01), (1, 0.0, 4097 / 16000.0)]
    bounds = [R.segment_bounds(s, e, offsets[r + 1] - offsets[r]) for r, s, e in segs]
    assert bounds[0] == (1000, 2000) and bounds[2] == (70000, 70000)
    lengths = [hi - lo for lo, hi in bounds]
    out_range = " ".join(str(x) for x in [0] + list(np.cumsum(lengths)))
    tiles = " ".join(str(x) for x in [0] + list(np.cumsum([-(-n // 2048) for n in lengths])))
    words = [w for r, s, e in segs for w in (r, f64hex(s), f64hex(e))]
    for device in (0, 1):
        src = " ".join(str(offsets[r] - (0 if device else offsets[0]) + lo) for (r, _, _), (lo, _) in zip(segs, bounds))
        assert run(plan, "gather", device, sum(lengths), 2, *offsets, len(segs), *words) == (OK, ["", out_range, src, tiles])
    st, parts = run(plan, "gather", 0, sum(lengths) - 1, 2, *offsets, len(segs), *words)
    assert st == OUTPUT_TOO_SMALL and parts[0] == f"vad_gather_segments: output holds {sum(lengths) - 1} of {sum(lengths)} samples" and parts[1] == out_range
    assert run(plan, "gather", 0, 9, 2, *offsets, 1, 2, f64hex(0.0), f64hex(1.0))[1][0] == "vad_gather_segments: segment 0 names recording 2"
    assert run(plan, "gather", 0, 9, 2, *offsets, 1, -1, f64hex(0.0), f64hex(1.0))[1][0] == "vad_gather_segments: segment 0 names recording -1"
    for t in (math.nan, math.inf, 2.0 ** 63 / 16000.0):
        assert run(plan, "gather", 0, 9, 2, *offsets, 2, 0, f64hex(0.0), f64hex(0.1), 1, f64hex(0.0), f64hex(t))[1][0] == "vad_gather_segments: a time of segment 1 does not fit Int"
    assert run(plan, "gather", 0, 9, 2, 0, 5, 4, 0)[1][0] == "vad_gather_segments: audio_offsets descends at recording 1"
    assert run(plan, "gather", 0, -1, 2, *offsets, 0)[1][0] == run(plan, "gather", 0, 9, 2, *offsets, -1)[1][0] == "vad_gather_segments: bad arguments"
    assert run(plan, "gather", 0, 0, 2, *offsets, 0) == (OK, ["", "0", "", "0"])


def stream(plan, counts, S=None, K=7, resolution=1, capacity=10, have_probs=1, have_count=1, cfg=None):
    return run(plan, "stream", *cfg_words(**(cfg or {})), len(counts) if S is None else S, K, resolution, capacity, have_probs, have_count, *counts)


def test_stream_plan_and_refusals(plan):
    for resolution in range(23):
        assert stream(plan, [1, 7, 0], resolution=resolution) == (OK, [f64hex(math.pow(10.0, float(resolution)))])        # pow(10, n) is exact up to 10^22
    for resolution in (-1, 23):
        assert stream(plan, [1], resolution=resolution) == (INVALID_ARGUMENT, ["vad_stream_advance: time_resolution is 0 ... 22"])
    assert stream(plan, [1], resolution=23, cfg=dict(speechPadding=-1.0)) == (INVALID_ARGUMENT, ["speechPadding must be non-negative"])     # the config first
    assert stream(plan, [1], capacity=-1)[1] == stream(plan, [1], have_count=0)[1] == stream(plan, [], S=-1)[1] == stream(plan, [1], K=-1)[1] == ["vad_stream_advance: bad arguments"]
    assert stream(plan, [1, 8])[1] == stream(plan, [1, -1])[1] == ["vad_stream_advance: stream 1 has a chunk count outside [0, max_chunks]"]
    assert stream(plan, [1], have_probs=0) == (INVALID_ARGUMENT, ["vad_stream_advance: probs is NULL"])
    assert stream(plan, [0, 0], have_probs=0)[0] == OK
    assert stream(plan, [0] * 3, K=2 ** 30)[0] == INDEX_OVERFLOW
