"""fa_vad_segments, fa_vad_pack_chunks, fa_vad_gather_segments and fa_vad_stream_advance (csrc/vad.hip) against the line-by-line
restatement of the reference (tests/vad_restatement.py).  No tolerances: integers as they are, fp64 and fp32 as bits.  The same file is
run on the poisoned-workspace library (make POISON=1).  Each expectation is computed once per module."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vad_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 130, 400)
DRAWS = 6
BANDS = ((0.85, 1.0), (0.0, 0.7), (0.7, 0.85))
CONFIGS = {
    "default": dict(),
    "cuts": dict(maxSpeechDuration=4.0, minSilenceDuration=0.5, speechPadding=0.3, silenceThresholdForSplit=0.05, minSilenceAtMaxSpeech=0.3,
                 useMaxPossibleSilenceAtMaxSpeech=False),
    "negative": dict(negativeThreshold=0.4, maxSpeechDuration=6.0, minSilenceDuration=1.5, speechPadding=0.5, silenceThresholdForSplit=0.02),
    "unbounded": dict(maxSpeechDuration=math.inf),
    "no_silence": dict(minSilenceDuration=0.0),
}


def draw_probs(rng, n):
    """Runs of 1 ... 11 frames, each from one of the three bands: speech, silence, the band between the thresholds."""
    out = []
    while len(out) < n:
        lo, hi = BANDS[rng.integers(3)]
        out += list(rng.uniform(lo, hi, rng.integers(1, 12)).astype(np.float32))
    return np.array(out[:n], np.float32)


def total_for(n, draw):
    """The whole span, a total inside the last frame, a total below half the span (the empty flush and the clamp's drop), none at all."""
    return (n * R.CHUNK, n * R.CHUNK - 100, n * R.CHUNK // 2 - 7, n * R.CHUNK, n * R.CHUNK - 4000, 0 if n == 1 else n * R.CHUNK // 3)[draw]


def expected_records(probs_list, totals, cfg):
    rows, counts = [], []
    for b, (p, t) in enumerate(zip(probs_list, totals)):
        segs = R.segment_speech(p, int(t), cfg)
        counts.append(len(segs))
        rows += [(b, 0, s, e, st, et) for s, e, st, et in segs]
    return rows, np.array(counts, np.int64)


@pytest.fixture(scope="module")
def seg_cases(fa):
    """Per config one ragged batch of DRAWS recordings per length; the restatement's answer as records of VAD_SEGMENT_DTYPE."""
    R.BRANCHES.clear()
    rng = np.random.default_rng(1)
    cases = {}
    for name, kw in CONFIGS.items():
        probs_list = [draw_probs(rng, n) for n in LENGTHS for _ in range(DRAWS)]
        totals = np.array([total_for(n, d) for n in LENGTHS for d in range(DRAWS)], np.int64)
        rows, counts = expected_records(probs_list, totals, R.Config(**kw))
        cases[name] = dict(cfg=fa.vad_config(**kw), probs=probs_list, totals=totals, want=np.array(rows, fa.VAD_SEGMENT_DTYPE), counts=counts)
    cases["branches"] = dict(R.BRANCHES)
    return cases


def test_the_inputs_reach_every_branch_of_the_reference(seg_cases):
    taken = seg_cases["branches"]
    print(taken)
    assert all(taken.get(name, 0) > 0 for name in R.BRANCH_NAMES), {n: taken.get(n, 0) for n in R.BRANCH_NAMES}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_segments_are_the_restated_ones(fa, gpu_ctx, seg_cases, name):
    import torch
    case = seg_cases[name]
    got, counts = fa.segment_speech_batch(case["probs"], case["totals"], config=case["cfg"], ctx=gpu_ctx)
    assert len(case["want"]) > 20
    assert counts.tolist() == case["counts"].tolist()
    assert got.tobytes() == case["want"].tobytes()                               # integers as they are, the times as bits
    flat = np.concatenate(case["probs"])
    frame_range = np.concatenate([[0], np.cumsum([p.size for p in case["probs"]])]).astype(np.int64)
    lead = 5                                                                     # the device entry addresses the caller's array from frame_range[0]
    dev = torch.from_numpy(np.concatenate([np.full(lead, 0.99, np.float32), flat, np.full(7, 0.99, np.float32)])).cuda()
    got_dev, counts_dev = fa.segment_speech_batch_dev(dev, frame_range + lead, case["totals"], config=case["cfg"], ctx=gpu_ctx)
    assert got_dev.tobytes() == case["want"].tobytes() and counts_dev.tolist() == case["counts"].tolist()


def test_segments_count_and_capacity(fa, gpu_ctx, seg_cases):
    case = seg_cases["cuts"]
    want, B = case["want"], len(case["probs"])
    flat = np.concatenate(case["probs"])
    frame_range = np.concatenate([[0], np.cumsum([p.size for p in case["probs"]])]).astype(np.int64)
    f, count, counts = fa.lib().fa_vad_segments, C.c_int64(-1), np.full(B, -1, np.int64)
    args = (gpu_ctx.handle, C.byref(case["cfg"]), flat.ctypes.data, frame_range.ctypes.data, case["totals"].ctypes.data, B)
    assert f(*args, None, 0, C.byref(count), counts.ctypes.data) == fa.SUCCESS                      # segs == NULL: the count
    assert count.value == len(want) and counts.tolist() == case["counts"].tolist()
    short = np.zeros(len(want) - 1, fa.VAD_SEGMENT_DTYPE)
    count.value = -1
    assert f(*args, short.ctypes.data, short.size, C.byref(count), None) == fa._lib.OUTPUT_TOO_SMALL
    assert count.value == len(want) and short.tobytes() == want[:-1].tobytes()
    count.value = -1
    assert f(gpu_ctx.handle, None, flat.ctypes.data, frame_range.ctypes.data, case["totals"].ctypes.data, 0, None, 0, C.byref(count), None) == fa.SUCCESS and count.value == 0
    # cfg == NULL is the default config
    got = np.zeros(len(seg_cases["default"]["want"]), fa.VAD_SEGMENT_DTYPE)
    d = seg_cases["default"]
    assert f(gpu_ctx.handle, None, np.concatenate(d["probs"]).ctypes.data, frame_range.ctypes.data, d["totals"].ctypes.data, B, got.ctypes.data, got.size, C.byref(count),
             None) == fa.SUCCESS
    assert got.tobytes() == d["want"].tobytes()


def test_nan_probabilities_are_in_neither_class(fa, gpu_ctx):
    rng = np.random.default_rng(5)
    probs = [draw_probs(rng, n) for n in (65, 130, 400)]
    for p in probs:
        p[rng.integers(0, p.size, p.size // 5)] = np.nan
    totals = np.array([p.size * R.CHUNK for p in probs], np.int64)
    kw = CONFIGS["cuts"]
    rows, counts = expected_records(probs, totals, R.Config(**kw))
    got, got_counts = fa.segment_speech_batch(probs, totals, config=fa.vad_config(**kw), ctx=gpu_ctx)
    assert got.tobytes() == np.array(rows, fa.VAD_SEGMENT_DTYPE).tobytes() and got_counts.tolist() == counts.tolist() and len(rows) > 5


# ---- the model rows
PACK_LENGTHS = (0, 1, 63, 4095, 4096, 4097, 2 * 4096 + 5)
POISON = np.uint32(0xDEADBEEF)


@pytest.fixture(scope="module")
def pack_case():
    """Every sample has its own bit pattern; one chunk is NaNs with distinct payloads; poison in front of and behind the batch."""
    lead, trail, n = 3, 9, sum(PACK_LENGTHS)
    bits = np.arange(1, n + 1, dtype=np.uint32) + np.uint32(0x3C000000)
    offsets = np.concatenate([[0], np.cumsum(PACK_LENGTHS)]).astype(np.int64)
    nan_at = offsets[6] + R.CHUNK                                                # the second chunk of the last recording
    bits[nan_at:nan_at + R.CHUNK] = np.uint32(0x7FC00000) + np.arange(1, R.CHUNK + 1, dtype=np.uint32)
    source = np.concatenate([np.full(lead, POISON), bits, np.full(trail, POISON)]).view(np.float32)
    want = np.concatenate([R.pack_chunks(bits[offsets[b]:offsets[b + 1]].view(np.float32)) for b in range(len(PACK_LENGTHS))])
    chunk_range = np.concatenate([[0], np.cumsum([R.chunk_count(n) for n in PACK_LENGTHS])]).astype(np.int64)
    return dict(source=source, offsets=offsets + lead, want=want, chunk_range=chunk_range, bits=bits)


def test_pack_chunks(fa, gpu_ctx, pack_case):
    import torch
    c = pack_case
    nan_row = int(c["chunk_range"][6]) + 1
    assert c["want"].shape == (9, R.ROW) and np.isnan(c["want"][nan_row, R.CONTEXT:]).all() and len(set(c["want"][nan_row, R.CONTEXT:].view(np.uint32).tolist())) == R.CHUNK
    rows, chunk_range = fa.pack_chunks(c["source"], c["offsets"], ctx=gpu_ctx)
    assert chunk_range.tolist() == c["chunk_range"].tolist() == [0, 0, 1, 2, 3, 4, 6, 9]
    assert np.array_equal(rows.view(np.int32), c["want"].view(np.int32))         # bits, NaN payloads included
    assert not (rows.view(np.uint32) == POISON).any()
    source = torch.from_numpy(c["source"]).cuda()
    dev_rows, dev_range = fa.pack_chunks_dev(source, c["offsets"], ctx=gpu_ctx)
    gpu_ctx.synchronize()                                                        # the device entry does not synchronise
    assert dev_range.tolist() == c["chunk_range"].tolist()
    assert np.array_equal(dev_rows.cpu().numpy().view(np.int32), c["want"].view(np.int32))
    # an output that starts 4 bytes off a 16-byte boundary takes the narrow stores
    buf = torch.zeros(c["want"].size + 1, dtype=torch.float32, device="cuda")
    chunk_range = np.zeros(len(PACK_LENGTHS) + 1, np.int64)
    with gpu_ctx.torch_ordered():
        gpu_ctx.check(fa.lib().fa_vad_pack_chunks_dev(gpu_ctx.handle, source.data_ptr(), c["offsets"].ctypes.data, len(PACK_LENGTHS),
                                                     buf.data_ptr() + 4, c["want"].shape[0], chunk_range.ctypes.data), "fa_vad_pack_chunks_dev")
    gpu_ctx.synchronize()
    assert np.array_equal(buf[1:].cpu().numpy().view(np.int32).reshape(c["want"].shape), c["want"].view(np.int32)) and float(buf[0]) == 0.0
    # too few rows: refused before any device work, the ranges are still written
    chunk_range[:] = -1
    small = np.zeros((c["want"].shape[0] - 1, R.ROW), np.float32)
    st = fa.lib().fa_vad_pack_chunks(gpu_ctx.handle, c["source"].ctypes.data, c["offsets"].ctypes.data, len(PACK_LENGTHS), small.ctypes.data, small.shape[0], chunk_range.ctypes.data)
    assert st == fa._lib.OUTPUT_TOO_SMALL and chunk_range.tolist() == c["chunk_range"].tolist() and not small.any()


def test_pack_chunks_more_recordings_than_one_launch_carries(fa, gpu_ctx):
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 3 * R.CHUNK, 130)
    audio = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    rows, chunk_range = fa.pack_chunks(audio, ctx=gpu_ctx)
    want = np.concatenate([R.pack_chunks(a) for a in audio])
    assert chunk_range[-1] == want.shape[0] and np.array_equal(rows.view(np.int32), want.view(np.int32))


# ---- the speech audio
def test_gather_segments(fa, gpu_ctx, seg_cases):
    import torch
    case = seg_cases["cuts"]
    keep = [b for b in range(len(case["probs"])) if case["probs"][b].size <= 130]
    totals = [max(int(case["totals"][b]), 0) for b in keep]
    offsets = np.concatenate([[0], np.cumsum(totals)]).astype(np.int64)
    audio = (np.arange(offsets[-1], dtype=np.uint32) + np.uint32(0x3C000000)).view(np.float32)
    segs = case["want"][np.isin(case["want"]["recording"], keep)].copy()
    segs["recording"] = [keep.index(r) for r in segs["recording"]]
    big = int(np.argmax(totals))
    hand = np.array([(big, 0, 0, 0, 1001 / 16000.0, 2000 / 16000.0),             # Int(1001 / 16000 * 16000) is 1000
                     (big, 0, 0, 0, 0.5, 1.0e6),                                 # beyond the audio's end: clamped
                     (big, 0, 0, 0, 1.0e6, 2.0e6),                               # starts beyond it: empty
                     (big, 0, 0, 0, -3.0, 0.01)], fa.VAD_SEGMENT_DTYPE)
    segs = np.concatenate([segs, hand])
    assert len(segs) > 20
    parts = []
    for s in segs:
        n = int(offsets[s["recording"] + 1] - offsets[s["recording"]])
        lo, hi = R.segment_bounds(float(s["start_time"]), float(s["end_time"]), n)
        parts.append(audio[offsets[s["recording"]] + lo:offsets[s["recording"]] + hi])
    want = np.concatenate(parts)
    want_range = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    assert [p.size for p in parts[-4:]] == [1000, totals[big] - 8000, 0, 160] and parts[-4][0] == audio[offsets[big] + 1000]
    got, out_range = fa.gather_segments(audio, segs, offsets, ctx=gpu_ctx)
    assert out_range.tolist() == want_range.tolist() and np.array_equal(got.view(np.int32), want.view(np.int32))
    lead = np.full(11, POISON).view(np.float32)
    dev, dev_range = fa.gather_segments_dev(torch.from_numpy(np.concatenate([lead, audio, lead])).cuda(), offsets + 11, segs, ctx=gpu_ctx)
    assert dev_range.tolist() == want_range.tolist() and np.array_equal(dev.cpu().numpy().view(np.int32), want.view(np.int32))
    out_range[:] = -1
    small = np.zeros(want.size - 1, np.float32)
    st = fa.lib().fa_vad_gather_segments(gpu_ctx.handle, audio.ctypes.data, offsets.ctypes.data, len(keep), segs.ctypes.data, segs.size, small.ctypes.data, small.size,
                                         out_range.ctypes.data)
    assert st == fa._lib.OUTPUT_TOO_SMALL and out_range.tolist() == want_range.tolist() and not small.any()


# ---- streaming
def restated_stream(probs, counts, samples, states, cfg, return_seconds, resolution):
    events = []
    for s in range(probs.shape[0]):
        for k in range(counts[s]):
            states[s], ev = R.stream_step(probs[s, k], int(samples[s, k]), states[s], cfg, return_seconds, resolution)
            if ev:
                events.append((s, k, ev[0], 0, ev[1], math.nan if ev[2] is None else ev[2]))
    return events


def same_events(fa, got, want):
    return got.tobytes() == np.array(want, fa.VAD_STREAM_EVENT_DTYPE).tobytes()


def state_keys(states):
    return [tuple(int(x) for x in s) for s in states]


def test_stream_reference_scenarios(fa, gpu_ctx):
    full = lambda p: np.full(p.shape, R.CHUNK, np.int64)   # noqa: E731
    # testStreamingEmitsStartAndEndEvents / testStreamingReturnsSecondsWhenRequested: a start at 0, then the end after 0.75 s of silence
    for seconds, resolution in ((False, 1), (True, 2)):
        probs = np.array([[0.9, 0.05, 0.05, 0.05, 0.05, 0.05]], np.float32)
        states, ref = fa.initial_stream_states(1), [R.StreamState()]
        got = fa.stream_advance(probs, states, return_seconds=seconds, time_resolution=resolution, ctx=gpu_ctx)
        want = restated_stream(probs, [6], full(probs), ref, R.Config(), seconds, resolution)
        assert same_events(fa, got, want) and [e[2] for e in want] == [R.START, R.END] and want[0][4] == 0 and want[1][4] > 0
        assert state_keys(states) == [ref[0].key()] and not states[0]["triggered"]
        if seconds:
            assert got[1]["time"] == R.swift_rounded(int(got[1]["sample_index"]) / 16000.0 * 100) / 100
    # testStreamingRespectsThresholdOverride, testStreamingUsesDefaultThresholdWithoutOverride
    for kw, probs in ((dict(negativeThreshold=0.2, negativeThresholdOffset=0.05, defaultThreshold=0.8), [0.24, 0.3]), (dict(defaultThreshold=0.6), [0.59, 0.7])):
        probs = np.array([probs], np.float32)
        states = fa.initial_stream_states(1)
        got = fa.stream_advance(probs, states, config=fa.vad_config(**kw), ctx=gpu_ctx)
        assert [(int(e["chunk"]), int(e["kind"]), int(e["sample_index"])) for e in got] == [(1, R.START, R.CHUNK - 1600)]
        assert same_events(fa, got, restated_stream(probs, [2], full(probs), [R.StreamState()], R.Config(**kw), False, 1))


@pytest.mark.parametrize("resolution", [0, 1, 2])
def test_stream_batch_in_two_calls(fa, gpu_ctx, resolution):
    import torch
    rng = np.random.default_rng(11 + resolution)
    S, K = 65, 7
    probs = np.stack([draw_probs(rng, 2 * K) for _ in range(S)])
    samples = np.where(rng.random((S, 2 * K)) < 0.8, R.CHUNK, rng.integers(0, R.CHUNK, (S, 2 * K))).astype(np.int32)
    first, second = rng.integers(0, K + 1, S).astype(np.int32), rng.integers(0, K + 1, S).astype(np.int32)
    kw = dict(minSilenceDuration=0.5, speechPadding=0.3)
    ref = [R.StreamState() for _ in range(S)]
    joined = np.stack([np.concatenate([probs[s, :first[s]], probs[s, K:K + second[s]], np.zeros(2 * K, np.float32)])[:2 * K] for s in range(S)])
    joined_samples = np.stack([np.concatenate([samples[s, :first[s]], samples[s, K:K + second[s]], np.zeros(2 * K, np.int32)])[:2 * K] for s in range(S)])
    want = restated_stream(joined, first + second, joined_samples, ref, R.Config(**kw), True, resolution)
    assert len(want) > 30 and {e[2] for e in want} == {R.START, R.END}
    for device in (False, True):
        states, got = fa.initial_stream_states(S), []
        for part, (lo, counts) in enumerate(((0, first), (K, second))):
            p, c = np.ascontiguousarray(probs[:, lo:lo + K]), np.ascontiguousarray(samples[:, lo:lo + K])
            if device:
                ev = fa.stream_advance_dev(torch.from_numpy(p).cuda(), states, counts, torch.from_numpy(c).cuda(), config=fa.vad_config(**kw), return_seconds=True,
                                           time_resolution=resolution, ctx=gpu_ctx)
            else:
                ev = fa.stream_advance(p, states, counts, c, config=fa.vad_config(**kw), return_seconds=True, time_resolution=resolution, ctx=gpu_ctx)
            got += [(int(e["stream"]), int(e["chunk"]) + (first[e["stream"]] if part else 0), int(e["kind"]), 0, int(e["sample_index"]), float(e["time"])) for e in ev]
        got.sort(key=lambda e: (e[0], e[1]))
        assert np.array(got, fa.VAD_STREAM_EVENT_DTYPE).tobytes() == np.array(want, fa.VAD_STREAM_EVENT_DTYPE).tobytes()
        assert state_keys(states) == [r.key() for r in ref]
    # without return_seconds the time is NaN; an output one short keeps the leading events
    states = fa.initial_stream_states(S)
    plain = fa.stream_advance(probs[:, :K], states, chunk_samples=samples[:, :K], config=fa.vad_config(**kw), ctx=gpu_ctx)
    assert len(plain) > 3 and np.isnan(plain["time"]).all()
    states, short, count = fa.initial_stream_states(S), np.zeros(len(plain) - 1, fa.VAD_STREAM_EVENT_DTYPE), C.c_int64(-1)
    p, c, full = np.ascontiguousarray(probs[:, :K]), np.ascontiguousarray(samples[:, :K]), np.full(S, K, np.int32)
    st = fa.lib().fa_vad_stream_advance(gpu_ctx.handle, C.byref(fa.vad_config(**kw)), p.ctypes.data, full.ctypes.data, c.ctypes.data, S, K, states.ctypes.data, 0, 1,
                                        short.ctypes.data, short.size, C.byref(count))
    assert st == fa._lib.OUTPUT_TOO_SMALL and count.value == len(plain) and short.tobytes() == plain[:-1].tobytes()
