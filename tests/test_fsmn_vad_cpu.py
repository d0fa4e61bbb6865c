"""FSMN-VAD without a GPU: the restatement (tests/fsmn_vad_restatement.py) against the reference's FsmnVadChunkingTests
(Tests/FluidAudioTests/VAD/FsmnVadChunkingTests.swift) and against values worked out from the Swift lines; the library's chunk schedule
against the restatement; the word-stepped machine of csrc/fsmn_vad_core.h against the naive per-frame loop, exhaustively, in a stand-alone
program (tests/cpu/fsmn_vad_core_main.cpp) built with the address and undefined-behaviour sanitizers; and the condition on the input
generators of the GPU test: every event kind occurs under the config that can produce it.

The exhaustive walk is 191 million sequence-config pairs: about half a minute on eight cores."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsmn_vad_cases as K  # noqa: E402
import fsmn_vad_restatement as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HOP, PAD = R.HOP_SAMPLES, R.LFR_PAD_FRAMES
FULL = 488_320                                                        # (3072 - 20) * 160: the samples of a full chunk


def kept_tiles(chunks):
    """The absolute frames of every kept frame: chunk frame i lands at start / hop + i."""
    out = []
    for _, start, _, frames, keep_from, _ in chunks:
        out += [start // HOP + i for i in range(keep_from, frames)]
    return out


# ---- FsmnVadChunkingTests.swift
def test_frame_count_matches_the_preprocessor_geometry():
    assert R.lfr_frame_count(FULL) == 3048 and R.lfr_frame_count(399) == 0


@pytest.mark.parametrize("samples, chunks_pinned, frames_pinned", [(100 * 60 * 16000, 197, 599_996), (60 * 60 * 16000, 119, 359_996)])
def test_long_audio_stays_on_the_grid(samples, chunks_pinned, frames_pinned):
    chunks, total = R.plan_chunks(samples)
    assert len(chunks) > 100 and all(start % HOP == 0 for _, start, _, _, _, _ in chunks)
    assert kept_tiles(chunks) == list(range(total))                   # 0, 1, 2, ...: no gap and no repeat across a boundary
    assert R.lfr_frame_count(samples) - PAD <= total <= R.lfr_frame_count(samples)
    assert (len(chunks), total) == (chunks_pinned, frames_pinned)
    if samples == 60 * 60 * 16000:
        assert 359_995 <= total <= 360_000
    assert all(first == start // HOP + keep for _, start, _, _, keep, first in chunks)


def test_short_audio_is_one_chunk():
    chunks, total = R.plan_chunks(320_000)
    assert [(s, e) for _, s, e, _, _, _ in chunks] == [(0, 320_000)] and total == R.lfr_frame_count(320_000) and chunks[0][0] == 2048
    assert R.plan_chunks(300) == ([], 0)


def test_a_short_tail_terminates_and_tiles():
    chunks, total = R.plan_chunks(FULL + 7_213)
    assert [(c[3], c[4]) for c in chunks] == [(3048, 0), (47, 2)] and total == 3093 and kept_tiles(chunks) == list(range(total))
    chunks, total = R.plan_chunks(FULL + 1)                           # the second chunk would hold only its two pad frames
    assert len(chunks) == 1 and total == 3048


# ---- the library's schedule
SCHEDULE_LENGTHS = [0, -5, 1, 399, 400, 1039, 1040, FULL - 1, FULL, FULL + 1, FULL + 7_213, 320_000, 300, 60 * 60 * 16000]


def chunk_rows(chunks):
    return [tuple(int(c[f]) for f in ("recording", "bucket", "start_sample", "end_sample", "frames", "keep_from", "first_frame")) for c in chunks]


def expected_plan(lengths):
    rows, chunk_range, frame_range = [], [0], [0]
    for b, n in enumerate(lengths):
        chunks, total = R.plan_chunks(int(n))
        rows += [(b,) + c for c in chunks]
        chunk_range.append(len(rows))
        frame_range.append(frame_range[-1] + total)
    return rows, chunk_range, frame_range


def test_library_schedule_equals_the_restatement(fa):
    rng = np.random.default_rng(3)
    lengths = SCHEDULE_LENGTHS + [int(x) for x in rng.integers(0, 3 * FULL, 300)] + [int(x) for x in rng.integers(0, 3000, 100)]
    for n in lengths:
        assert fa.fsmn_vad_frame_count(n) == R.lfr_frame_count(n), n
    chunks, chunk_range, frame_range = fa.fsmn_vad_plan_chunks(lengths)
    rows, want_chunks, want_frames = expected_plan(lengths)
    assert chunk_rows(chunks) == rows and chunk_range.tolist() == want_chunks and frame_range.tolist() == want_frames
    assert fa.fsmn_vad_plan_chunks([])[0].size == 0


# ---- the shared headers on the CPU, under the sanitizers
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fsmn_vad_core") / "fsmn_vad_core_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "fsmn_vad_core_main.cpp"), "-o", exe], check=True)

    def ask(*lines, timeout=60):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        return [l.split()[1:] for l in r.stdout.strip().splitlines()]
    return ask


def test_word_step_equals_the_naive_loop_exhaustively(core):
    (line,) = core("exhaustive", timeout=1500)
    runs, mismatches, opens, end_silence, max_length, end_of_audio, toggles, holds = (int(x) for x in line)
    # 2^17 - 1 sequences of 0 ... 16 frames; windows 1 ... 4 with (window + 1)^2 threshold pairs; 3^3 for the other three
    assert runs == (2 ** 17 - 1) * (4 + 9 + 16 + 25) * 27 and mismatches == 0
    assert min(opens, end_silence, max_length, end_of_audio, toggles, holds) > 0


def cfg_words(cfg):
    return " ".join([f"{struct.unpack('<I', struct.pack('<f', cfg.silence_threshold))[0]:08x}"] + [str(x) for x in (
        cfg.window_frames, cfg.sil_to_speech, cfg.speech_to_sil, cfg.max_end_silence_frames, cfg.lookback_frames, cfg.lookahead_frames, cfg.max_segment_frames, cfg.frame_ms)])


def test_word_step_equals_the_restatement_on_the_generators(core):
    """The host's word step at the kernel's width, and at widths that move the step boundaries, on the GPU test's inputs."""
    asks, wants = [], []
    for name, cfg in K.CONFIGS.items():
        for i, p in enumerate(K.recordings(11)):
            bits = "".join("1" if x else "0" for x in (p <= np.float32(cfg.silence_threshold))) or "-"
            asks.append(f"decide {cfg_words(cfg)} {(64, 64, 37, 1)[i % 4] if p.size < 1000 or i % 4 != 3 else 64} {bits}")
            wants.append([(s, e, r) for s, e, r, _, _ in R.decide(p, cfg)])
    for want, got in zip(wants, core(*asks)):
        vals = [int(x) for x in got if x != "|"]
        assert vals[0] == len(want) and list(zip(vals[1::3], vals[2::3], vals[3::3])) == want


def test_core_schedule_and_plan(core):
    lengths = SCHEDULE_LENGTHS[:-1]
    rows, chunk_range, frame_range = expected_plan(lengths)
    flat = lambda rs: [str(x) for r in rs for x in r]   # noqa: E731
    text = " ".join(str(n) for n in lengths)
    full, counted, short, negative = core(f"chunks {len(rows)} {len(lengths)} {text}", f"chunks 0 {len(lengths)} {text}", f"chunks 3 {len(lengths)} {text}", "chunks 4 -1")
    head = lambda status: [str(status), str(len(rows)), "|"] + [str(x) for x in chunk_range] + ["|"] + [str(x) for x in frame_range] + ["|"]   # noqa: E731
    assert full == head(0) + flat(rows) and counted == head(0)
    assert short == head(3) + flat(rows[:3])                          # OUTPUT_TOO_SMALL: the ranges and the first records are written
    assert negative[:2] == ["1", "-1"]
    assert [g[0] for g in core(*[f"frames {n}" for n in lengths])] == [str(R.lfr_frame_count(n)) for n in lengths]
    d = cfg_words(R.Config())
    # the arena: a slice holds min(frames, capacity) records, none without an output; the host entry uploads from frame_range[0] on
    assert core(f"seg {d} 0 1 1 5 1 3 10 10 13 113", f"seg {d} 1 1 0 5 1 3 10 10 13 113", f"seg {d} 1 1 1 500 1 2 0 7 7") == [
        ["0", "|", "103", "8", "5", "|", "0", "0", "0", "0", "0", "0", "3", "3", "3", "3", "100", "5"],
        ["0", "|", "103", "0", "0", "|", "10", "0", "0", "0", "10", "0", "3", "0", "13", "0", "100", "0"],
        ["0", "|", "7", "7", "7", "|", "0", "0", "7", "7", "7", "7", "0", "0"]]
    bad = lambda **kw: cfg_words(R.Config(**kw))   # noqa: E731
    refusals = [f"seg {d} 0 1 1 -1 1 1 0 4", f"seg {d} 0 1 1 4 0 1 0 4", f"seg {d} 0 0 1 4 1 1 0 4", f"seg {d} 0 1 1 4 1 2 0 4 3", f"seg {d} 0 1 1 4 1 1 -1 4",
                f"seg {bad(silence_threshold=float('nan'))} 0 1 1 4 1 1 0 4", f"seg {bad(window_frames=0)} 0 1 1 4 1 1 0 4", f"seg {bad(window_frames=65, sil_to_speech=15)} 0 1 1 4 1 1 0 4",
                f"seg {bad(sil_to_speech=21)} 0 1 1 4 1 1 0 4", f"seg {bad(speech_to_sil=-1)} 0 1 1 4 1 1 0 4", f"seg {bad(max_end_silence_frames=0)} 0 1 1 4 1 1 0 4",
                f"seg {bad(max_segment_frames=0)} 0 1 1 4 1 1 0 4", f"seg {bad(frame_ms=0)} 0 1 1 4 1 1 0 4", f"seg {bad(lookback_frames=-1)} 0 1 1 4 1 1 0 4",
                f"seg {bad(lookahead_frames=-1)} 0 1 1 4 1 1 0 4"]
    assert [g[0] for g in core(*refusals)] == ["1"] * len(refusals)
    assert [g[0] for g in core(f"seg {d} 1 1 1 4 1 1 0 {2 ** 31}", f"seg {d} 1 1 1 4 1 1 0 {2 ** 31 - 5}", f"seg {d} 1 1 1 4 1 1 0 {2 ** 31 - 11}")] == ["2", "2", "0"]


# ---- the two quirks, and the condition on the generators
def test_equal_thresholds_flip_on_a_plateau_and_the_overlap_after_a_maximal_close():
    assert [s[:3] for s in R.decide(np.full(7000, 0.1, np.float32))] == [(0, 6000, R.MAX_LENGTH), (5966, 7000, R.END_OF_AUDIO)]
    ev = R.Events()
    segs = R.decide(K.plateau(15, 400), events=ev)
    # from frame 19 on every frame is in the toggle class: preSpeech is false on every other frame, so the silence run never exceeds 1
    assert ev.toggle_frames == 400 - 19 + 5 and [s[:3] for s in segs] == [(0, 400, R.END_OF_AUDIO)]
    # opened at frame 14 (the count reaches 15), flipped off at 15: with max_end_silence 1 that closes at 15 - 1 + 10; on again at 16, off at 17
    assert [s[:3] for s in R.decide(K.plateau(15, 400), R.Config(max_end_silence_frames=1))][:2] == [(0, 15 - 1 + 10, R.END_SILENCE), (0, 17 - 1 + 10, R.END_SILENCE)]


def test_generators_reach_every_event_kind():
    """A condition on the inputs, not a measurement: under every config the GPU test runs, the restatement alone sees opens and every close
    reason; the toggle class under the configs with on <= off, the hold class under those with on > off."""
    for name, cfg in K.CONFIGS.items():
        ev = R.Events()
        K.expected_records(K.recordings(11), cfg, ev)
        assert ev.opens > 0 and min(ev.closes) > 0, (name, ev)
        if cfg.sil_to_speech <= cfg.speech_to_sil:
            assert ev.toggle_frames > 0 and ev.hold_frames == 0, (name, ev)
        else:
            assert ev.hold_frames > 0 and ev.toggle_frames == 0, (name, ev)
