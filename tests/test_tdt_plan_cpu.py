"""tests/tdt_plan_restatement.py against the reference's own known answers (no GPU): ChunkProcessorTests.swift:187-366 (the layouts and the
six chunk-start cases), EndAlignedFinalWindowTests.swift (every lastChunkWarmupSamples case, both speechEndSamples cases, the quiet
recording's threshold) and SeamGapRepairTests.swift:185-275 (speech-like seconds and the adaptive threshold)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_plan_restatement as R  # noqa: E402

F, RATE = 1280, 16000
NO_MEL_V3 = R.Config(**R.MODES["path_a"])
NO_MEL_V2 = R.Config(mel_chunk_context=False, silence_aligned=False, warmup_prefix_frames=0, end_aligned=False)
MEL_V3 = R.Config(**R.MODES["default"])
CHUNK = R.chunk_layout(MEL_V3)[0]


def tone(n, amplitude, lo=0, hi=None):
    """amplitude * sin(Float(i) * 0.1) on [lo, hi), zeros elsewhere"""
    x = np.zeros(n, np.float32)
    i = np.arange(lo, n if hi is None else hi)
    x[i] = np.float32(amplitude) * np.sin(i.astype(np.float32) * np.float32(0.1)).astype(np.float32)
    return x


def starts_of(audio, cfg=NO_MEL_V3):
    return R.Planner(audio, cfg).chunk_start_decisions()


def flat(seconds):
    return np.full(seconds * RATE, 0.02, np.float32)


# ---- ChunkProcessorTests.swift:187-226
def test_no_mel_v3_layout_keeps_warmup_disabled():
    chunk, stride, mel_context, warmup = R.chunk_layout(NO_MEL_V3)
    assert (mel_context, warmup) == (0, 0) and chunk <= 240000 and stride == chunk - 32000
    assert (chunk, stride) == (239360, 207360)


def test_warmup_prefix_is_v3_only():
    chunk, _, _, warmup = R.chunk_layout(NO_MEL_V2)
    assert warmup == 0 and chunk == (240000 - 160) // F * F
    _, _, mel_context, warmup = R.chunk_layout(MEL_V3)
    assert (mel_context, warmup) == (F, 0)
    assert R.chunk_layout(R.Config(**R.MODES["path_b"]))[3] == 7 * F
    assert R.chunk_layout(MEL_V3)[:2] == (238080, 206080)


# ---- :228-366
def test_chunk_starts_prefer_nearby_silence():
    audio, stride = flat(45), R.chunk_layout(NO_MEL_V3)[1]
    silent = stride + 3 * F
    assert silent == 211200
    audio[silent - F:silent + F] = 0
    starts = starts_of(audio)
    assert len(starts) >= 2 and starts[1] == (silent, False)      # also :291-314: the default path adds no warm-up


def test_flat_signal_is_not_shifted():
    starts = starts_of(flat(45))
    assert len(starts) >= 2 and starts[1][0] == 207360


def test_enough_overlap_for_the_lcs_merge():
    audio = flat(90)
    chunk, stride, _, _ = R.chunk_layout(NO_MEL_V3)
    first = stride - int(4.0 * RATE / F) * F
    audio[first - F:first + F] = 0
    collapse = first + chunk - F
    audio[collapse - F:min(collapse + F, audio.size)] = 0
    starts = starts_of(audio)
    assert len(starts) >= 3 and starts[2][0] <= starts[1][0] + chunk - 6 * F


def test_far_short_trough_is_taken_without_warmup():
    audio, stride = flat(45), R.chunk_layout(NO_MEL_V3)[1]
    trough = (stride // F - int(3.0 * RATE / F)) * F
    audio[trough - F:trough + F] = 0
    starts = starts_of(audio)
    assert len(starts) >= 2 and starts[1] == (trough, False)


def test_stable_quiet_behind_the_boundary_skips_the_warmup():
    audio, stride = flat(45), R.chunk_layout(NO_MEL_V3)[1]
    silent = stride + 3 * F
    audio[silent - F:silent + 4 * F] = 0
    assert starts_of(audio)[1] == (silent, False)
    assert starts_of(audio, R.Config(**R.MODES["path_b"]))[1] == (silent, False)      # 0.4 s of quiet: the probe's stable exit
    short = flat(45)
    short[silent - F:silent + F] = 0
    assert starts_of(short, R.Config(**R.MODES["path_b"]))[1] == (silent, True)       # 80 ms of quiet, then 0.02: the loud exit


# ---- EndAlignedFinalWindowTests.swift
def warmup(chunk_start, default, total, speech_end=None):
    return R.last_chunk_warmup_samples(chunk_start, default, CHUNK, total, total if speech_end is None else speech_end)


def test_short_final_chunk_is_filled_with_real_audio():
    total, chunk_start = int(17.28 * RATE), 206080
    w = warmup(chunk_start, 0, total)
    assert w % F == 0 and chunk_start - w >= 0 and w > 0 and CHUNK - F <= w + total - chunk_start <= CHUNK + F


def test_last_chunk_warmup_cases():
    assert warmup(CHUNK, 0, 2 * CHUNK) == 0                                            # a full final window
    assert warmup(0, 0, CHUNK // 2) == 0                                               # a single-chunk file
    total = CHUNK + CHUNK // 2
    assert warmup(CHUNK, 0, total, total - 40 * F) == warmup(CHUNK, 0, total) + 40 * F   # trailing silence grows the fill
    assert warmup(CHUNK, 0, total, total - 40 * F) + (total - 40 * F - CHUNK) >= CHUNK - F
    assert warmup(4 * F, 0, 5 * F) == 4 * F                                            # capped by the audio in front
    assert warmup(CHUNK, 2 * F, 4 * CHUNK) == 2 * F                                    # not the final chunk
    assert warmup(CHUNK, 2 * F, 2 * CHUNK - 4 * F) == 4 * F                            # never below the default
    w = warmup(5 * F + 137, 0, 7 * F + 137)
    assert w % F == 0 and 5 * F + 137 - w >= 0


def test_speech_end_samples():
    end = R.Planner(tone(4 * RATE, 0.05, 0, 2 * RATE)).speech_end_samples()
    assert 2 * RATE - F <= end <= 2 * RATE + F
    assert R.Planner(np.zeros(RATE, np.float32)).speech_end_samples() == RATE


def test_threshold_scales_to_a_quiet_recording():
    t = R.Planner(tone(4 * RATE, 0.004)).adaptive_speech_rms_threshold()
    assert R.SPEECH_RMS_FLOOR <= t < R.SPEECH_RMS_CEILING


# ---- SeamGapRepairTests.swift:185-275
def test_speech_like_seconds():
    assert R.Planner(np.zeros(4 * RATE, np.float32)).speech_like_seconds(0, 4 * RATE) == 0.0
    assert R.Planner(tone(4 * RATE, 0.1, RATE, 2 * RATE)).speech_like_seconds(0, 4 * RATE) == pytest.approx(1.0, abs=0.1)
    mixed = tone(5 * RATE, 0.1, 0, 3 * RATE) + tone(5 * RATE, 0.004, 3 * RATE)
    assert R.Planner(mixed).speech_like_seconds(3 * RATE, 5 * RATE) == 0.0
    assert R.Planner(tone(4 * RATE, 0.005, RATE, 2 * RATE)).speech_like_seconds(0, 4 * RATE) == pytest.approx(1.0, abs=0.1)


def test_adaptive_threshold():
    assert R.adaptive_threshold(0.07) == np.float32(0.008)
    assert float(R.adaptive_threshold(0.004)) == pytest.approx(0.0012, abs=0.0001)
    assert R.adaptive_threshold(0.0) == np.float32(0.0005)
    t = R.Planner(tone(4 * RATE, 0.004, 0, 4 * RATE // 5)).adaptive_speech_rms_threshold()
    assert t > R.SPEECH_RMS_FLOOR and float(t) == pytest.approx(0.0028 * 0.3, abs=0.0002)
    assert R.Planner(np.zeros(2 * RATE, np.float32)).adaptive_speech_rms_threshold() == R.SPEECH_RMS_CEILING


# ---- the window loop
def test_the_bound_holds_and_the_windows_tile_the_recording():
    rng = np.random.default_rng(0)
    for mode in R.MODES.values():
        cfg = R.Config(**mode)
        for n in (1, F, 239360, 239361, 500000, 1000001):
            x = (rng.standard_normal(n) * 0.02).astype(np.float32)
            windows, speech_end = R.Planner(x, cfg).plan()
            assert 1 <= len(windows) <= R.window_count_bound(cfg, n)
            assert windows[0]["chunk_start"] == 0 and windows[-1]["is_last"] == 1 and speech_end == n
            assert all(0 <= w["context_start"] and w["context_start"] + w["length"] <= n and 0 < w["length"] <= 240000 for w in windows)
    assert R.Planner(np.zeros(0, np.float32)).plan() == ([], 0) and R.window_count_bound(R.Config(), 0) == 0
