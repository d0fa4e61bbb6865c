"""The Nemotron streaming session without a GPU: the restatement (tests/rnnt_stream_restatement.py) against the reference's known answers
(Tests/FluidAudioTests/ASR/Parakeet/Streaming/NemotronMultilingualTests.swift:283-383: the four testMergeRescuedTokens* cases, both
testContainsLexicalContent* lists, the defaults of testBlankRescueDefaults); the library's host emulation of its RMS order against the
restatement's float64 RMS; the independence claim (the reference's immediate order and the library's deferred order give the same ids,
timings, requests and counters) on seeded random sessions; the shared header's window machine and merge indices against naive loops,
exhaustively, in a stand-alone program (tests/cpu/rnnt_stream_core_main.cpp) built with the address and undefined-behaviour sanitizers;
and the conditions on the inputs of the GPU test: every RMS away from its threshold, every listed situation present."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_stream_cases as K  # noqa: E402
import rnnt_stream_restatement as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
T = R.Timing


# ---- NemotronMultilingualTests.swift:283-383
def test_contains_lexical_content():
    for word in ("▁Gemma", "hello", "A", "42", "你好", "こんにちは", "▁afternoon."):          # testContainsLexicalContentWords
        assert R.contains_lexical_content(word), word
    for mark in (".", ",", "?", "。", "▁", "▁...", ""):                                      # testContainsLexicalContentPunctuationOnly
        assert not R.contains_lexical_content(mark), mark
    table = K.class_table()
    assert all(table[i] & R.LEXICAL for i in K.LEXICAL_IDS) and not any(table[i] & R.LEXICAL for i in K.PUNCT_IDS)
    assert [i for i in range(len(table)) if table[i] & R.LANG_TAG] == list(K.LANG_TAGS)


def test_merge_rescued_tokens_reference_cases():
    ids, tm = R.merge_rescued_tokens([10, 20], [T(10, 1.0), T(20, 5.0)], [30], [T(30, 3.0)], set(), 2.9)   # InsertsAtTimestampPosition
    assert ids == [10, 30, 20] and [t.token_id for t in tm] == [10, 30, 20] and [t.start_time for t in tm] == [1.0, 3.0, 5.0]
    ids, tm = R.merge_rescued_tokens([10], [T(10, 1.0)], [30, 31], [T(30, 3.0), T(31, 3.1)], set(), 2.9)    # AppendsWhenSpanIsLatest
    assert ids == [10, 30, 31] and [t.start_time for t in tm] == [1.0, 3.0, 3.1]
    ids, tm = R.merge_rescued_tokens([13000, 10], [T(10, 5.0)], [30], [T(30, 2.0)], {13000}, 1.9)           # SkipsLeadingLangTag
    assert ids == [13000, 30, 10] and [t.start_time for t in tm] == [2.0, 5.0]
    ids, tm = R.merge_rescued_tokens([], [], [30], [T(30, 0.5)], set(), 0.4)                                # EmptyLive
    assert ids == [30] and len(tm) == 1


def test_defaults(fa):
    import ctypes as C
    assert R.Config().rescue_rms_threshold == 0.0025                                                        # testBlankRescueDefaults
    raw = fa._lib.RnntStreamConfig()
    fa.lib().fa_rnnt_stream_default_config(C.byref(raw))
    want = R.Config(total_mel_frames=0)
    assert all(getattr(raw, f) == getattr(want, f) for f in vars(want) if "threshold" not in f)
    assert raw.rescue_rms_threshold == np.float32(0.0025) and raw.vad_rms_threshold == 0.0 and raw.vad_hangover_chunks == 2
    cfg = fa.RnntStreamConfig(total_mel_frames=65)
    assert all(getattr(cfg, f) == getattr(R.Config(), f) for f in vars(R.Config()))
    g = cfg.geometry()
    assert (g.span_capacity, g.pre_roll_capacity, g.mel_cache_capacity) == (240640 + 1280, 3 * 1280, 128 * 9)     # 15 s is 187.5 windows
    assert np.array_equal(fa.rnnt_stream_token_classes(K.PIECES, K.LANG_TAGS), K.class_table())
    assert fa.rnnt_stream_seconds([0, 37, 1000]).tolist() == [0.0, 37 * 0.08, 1000 * 0.08]


# ---- the RMS order
def rms_bound(n):
    return (n / 64 + 8) * 2.0 ** -24


@pytest.mark.parametrize("n, gate", [(1280, False), (320, False), (4, False), (8960, True), (8962, True), (71680, True), (1, True), (255, True), (1023, False)])
def test_host_rms_against_float64(fa, n, gate):
    rng = np.random.default_rng(n)
    for scale in (0.05, 0.0005, 1.0):
        x = (rng.uniform(-1, 1, n) * scale).astype(np.float32)
        got, want = float(fa.rnnt_stream_rms(x, gate=gate)), R.rms64(x)
        assert abs(got ** 2 / want ** 2 - 1.0) <= rms_bound(n) + 2.0 ** -22, (n, scale, got, want)             # + the divide's and the root's roundings
    assert fa.rnnt_stream_rms(np.zeros(0, np.float32)) == 0.0 and fa.rnnt_stream_rms(np.zeros(n, np.float32), gate=gate) == 0.0
    assert fa.rnnt_stream_rms(np.full(n, 0.5, np.float32), gate=gate) == 0.5                                    # exact sums: every order agrees


# ---- the shared header on the CPU, under the sanitizers
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rnnt_stream_core") / "rnnt_stream_core_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "rnnt_stream_core_main.cpp"), "-o", exe], check=True)

    def ask(*lines, timeout=600):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        return [l.split()[1:] for l in r.stdout.strip().splitlines()]
    return ask


def test_window_machine_and_merge_indices_exhaustively(core):
    (line,) = core("exhaustive")
    runs, bad, closures, overflows, reopen, index_runs, index_bad = (int(x) for x in line)
    assert runs == (2 ** 17 - 1) * 3 * 4 * 4 and bad == 0 and min(closures, overflows, reopen) > 0
    assert index_runs == sum((n + 1) * 2 ** n for n in range(17)) and index_bad == 0


def test_core_rms_is_the_library_s_and_the_gate_counts(fa, core):
    rng = np.random.default_rng(11)
    asks, wants = [], []
    for n, waves in ((1280, 1), (322, 1), (8962, 4), (7, 4)):
        x = (rng.uniform(-1, 1, n) * 0.05).astype(np.float32)
        asks.append(f"rms {waves} " + " ".join(f"{u:08x}" for u in x.view(np.uint32)))
        wants.append([f"{struct.unpack('<I', struct.pack('<f', float(fa.rnnt_stream_rms(x, gate=waves == 4))))[0]:08x}"])
    assert core(*asks) == wants
    # PL:86-104: the second low chunk skips, a loud one resets, the skipped chunk advances the base by its nominal frames
    assert core("gate 0.01 2 1280 8960 110100111", "gate 0 2 1280 8960 1111", "gate 0.01 1 1280 8961 101") == [
        ["0", "1", "0", "0", "0", "0", "0", "1", "1", "|", "3", "3", "21"], ["0", "0", "0", "0", "|", "0", "0", "0"], ["1", "0", "1", "|", "1", "2", "14"]]
    seq, s = "110100111", R.Session(R.Config(vad_rms_threshold=0.01), K.class_table())
    got = [int(s.gate(K.audio(["0000000" if ch == "1" else "1111111"], 1280, i)[0])) for i, ch in enumerate(seq)]
    assert got == [0, 1, 0, 0, 0, 0, 0, 1, 1] and (s.vad_low, s.vad_skips, s.absolute_frame_base) == (3, 3, 21)


# ---- the independence claim
def run_order(cfg, steps, immediate: bool):
    s, log = R.Session(cfg, K.class_table()), []
    for pattern, tokens in steps:
        K.append_tokens(s, tokens)
        chunk = K.audio([pattern], cfg.window_samples, 0)[0]
        (s.track_immediate if immediate else s.track_deferred)(chunk, K.random_decoder, log)
    (lambda rescue: s.finalize(rescue))(lambda q: (log.append(q), s.commit(q, *K.random_decoder(q))))
    return s, log


def test_deferred_order_equals_the_immediate_order():
    shared, rescued, clamped = 0, 0, 0
    for seed in range(400):
        cfg, steps = K.random_session(seed)
        a, la = run_order(cfg, steps, True)
        b, lb = run_order(cfg, steps, False)
        assert a.ids == b.ids and [(t.token_id, t.start_time) for t in a.timings] == [(t.token_id, t.start_time) for t in b.timings], seed
        assert [(q.span_start_frame, q.span_end_frame, q.speech_windows, q.audio.tobytes()) for q in la] == [(q.span_start_frame, q.span_end_frame, q.speech_windows, q.audio.tobytes()) for q in lb], seed
        assert (a.detected, a.rescued, a.rescue_frame_cursor, a.span_open) == (b.detected, b.rescued, b.rescue_frame_cursor, b.span_open), seed
        windows = len(steps[0][0])
        starts = [q.span_end_frame // windows for q in la]
        shared += len(starts) - len(set(starts))
        rescued += a.rescued
        clamped += sum(1 for q in la if any(f > q.span_end_frame for f in K.random_decoder(q)[1]))
    assert shared > 50 and rescued > 200 and clamped > 100, (shared, rescued, clamped)   # closures that share a chunk, commits, late tokens


# ---- the conditions on the GPU test's inputs
@pytest.fixture(scope="module")
def expectations():
    return {name: K.expected(sc) for name, sc in K.SCENARIOS.items()}


def test_every_rms_is_away_from_its_threshold():
    for sc in K.SCENARIOS.values():
        W = sc.cfg.window_samples
        for t in range(len(sc.steps)):
            chunk = sc.chunk(t)
            for row in chunk:
                for w in range(len(row) // W):
                    r = R.rms64(row[w * W:(w + 1) * W])
                    assert abs(r / float(np.float32(sc.cfg.rescue_rms_threshold)) - 1.0) > 1e-3
                if sc.cfg.vad_rms_threshold > 0:
                    assert abs(R.rms64(row) / float(np.float32(sc.cfg.vad_rms_threshold)) - 1.0) > 1e-3


def test_the_cases_contain_what_the_gpu_test_claims(expectations):
    main, over, w320, long_ = (expectations[n] for n in ("main", "overflow", "w320", "long"))
    sc = K.SCENARIOS["main"]
    closes = {}
    for b, t, start, last, outcome in main.closes:
        closes.setdefault((b, t), []).append((start, last, outcome))
    per = 7
    assert any(start // per == t and outcome == "request" for (b, t), v in closes.items() for start, last, outcome in v)            # opens and closes inside one chunk
    spans = [(t - start // per) for (b, t), v in closes.items() for start, last, outcome in v if t < len(sc.steps)]
    assert 1 in spans and 2 in spans                                                                                              # a span over two and over three chunks
    assert any(len(v) == 2 for v in closes.values())                                                                              # two closures in one chunk
    assert any(pre == 0 and any(s < frame for s, _, _ in closes.get((b, t), [])) for b, t, frame, pre in main.opens)              # close and reopen, the pre-roll empty
    first = main.requests[0][0]
    assert first.stream == 0 and first.span_start_frame == 0 and len(first.audio) == (1 + 2 + 2) * 1280                             # a one-window pre-roll at the stream's start
    assert (2, 0, 2, 3, "emitted") in main.closes and (1, 22) in sc.steps[0].tokens[2]                                            # a token at start - 1
    assert (2, 2, 16, 17, "emitted") in main.closes and (22, 24) in sc.steps[2].tokens[2]                                         # at last + 5
    assert (2, 4, 30, 31, "request") in main.closes and sc.steps[4].tokens[2] == [(28, 25), (37, 26)]                             # at start - 2 and last + 6
    assert (2, 6, 44, 45, "request") in main.closes and sc.steps[6].tokens[2] == [(44, K.DOT)]                                    # only punctuation inside
    assert any(o == "short" for *_, o in main.closes) and any(o == "overflow" for *_, o in over.closes)
    assert over.requests[0] and len(over.requests[0][0].audio) == 7 * 1280                                                        # a span of exactly the room minus one
    assert main.final_requests and len(sc.finalize) > len(main.final_requests)                                                    # finalize with an open span and with none
    assert any(s.active and 0 in s.active for s in sc.steps)
    assert any(s.tail % 4 for s in K.SCENARIOS["overflow"].steps) and any(s.tail and s.tail % 4 == 0 for s in K.SCENARIOS["long"].steps) and K.SCENARIOS["w320"].steps[0].tail == 2
    skips = [g[0][4] for g in main.gate]
    assert skips == [0, 1, 1, 0, 0, 1, 1, 1]                                                                                      # the second low chunk skips, a loud one resets
    assert any(len(run) < sc.streams for _, run in main.gate)                                                                     # a stream left out of the mel list
    frames = [s.chunk_frames for s in sc.steps]
    room = sc.cfg.total_mel_frames - sc.cfg.pre_encode_cache
    assert frames[0] < sc.cfg.pre_encode_cache and room in frames and max(frames) > room and any(s.mel_stride > 1 for s in sc.steps)
    assert any(len(v) == 2 for v in [[q for q in reqs if q.stream == 0] for reqs in main.requests])                               # two requests of one stream
    assert any(True in c for c in main.commits) and any(False in c for c in main.commits)
    assert len(K.SCENARIOS["long"].steps[0].patterns[0]) == 67 and any(q.span_end_frame + 1 >= 64 for q in long_.requests[0]) and any(q.span_end_frame + 1 < 64 for q in long_.requests[0])   # closing windows in both words
    assert w320.requests[0] and K.SCENARIOS["w320"].cfg.window_samples == 320
