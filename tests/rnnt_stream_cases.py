"""Shared case generators of the Nemotron streaming session's tests (test_rnnt_stream_cpu.py, test_gpu_rnnt_stream.py): the toy
vocabulary with its class table, loud / silent audio from window patterns, the scripted sessions (a window pattern, the live tokens of
every step, the chunk's mel and the active mask per stream), the stub rescue decoder, and the random sessions of the independence claim.

Loud windows are uniform noise of amplitude 0.05 (RMS 0.029), silent ones of amplitude 0.0005 (RMS 0.00029): an order of magnitude
either side of both thresholds, whatever the summation order."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_stream_restatement as R  # noqa: E402

M = "▁"
TAG_EN, TAG_DE, DOT, COMMA = 4, 5, 1, 2
PIECES = {0: M, 1: ".", 2: ",", 3: "?", 4: "<en-US>", 5: "<de-DE>", 10: M + "Gemma", 11: "hello", 12: "A", 13: "42", 14: "你好", 15: M + "afternoon.",
          16: "。", 17: M + "...", 18: "", 19: "こんにちは"}
PIECES.update({i: f"{M}w{i}" for i in range(20, 40)})
LANG_TAGS = (TAG_EN, TAG_DE)
LEXICAL_IDS = [10, 11, 12, 13, 14, 19, 15] + list(range(20, 40))      # testContainsLexicalContentWords, then the filler words
PUNCT_IDS = [1, 2, 3, 16, 0, 17, 18]                                  # testContainsLexicalContentPunctuationOnly


def class_table() -> np.ndarray:
    """The class byte per id, from the restatement's containsLexicalContent."""
    table = np.zeros(max(PIECES) + 1, np.uint8)
    for i, piece in PIECES.items():
        table[i] = (R.LEXICAL if R.contains_lexical_content(piece) else 0) | (R.LANG_TAG if i in LANG_TAGS else 0)
    return table


def audio(patterns, window: int, seed: int, tail: int = 0) -> np.ndarray:
    """[streams, windows * window + tail] float32: window w of stream b loud where patterns[b][w] == '1'."""
    rng = np.random.default_rng(seed)
    rows = []
    for p in patterns:
        amp = np.repeat(np.array([0.05 if ch == "1" else 0.0005 for ch in p]), window)
        amp = np.concatenate([amp, np.full(tail, 0.0005)])
        rows.append((rng.uniform(-1.0, 1.0, amp.size) * amp).astype(np.float32))
    return np.stack(rows)


def stub_decoder(request: R.Request):
    """What a rescue decode might return, decided by the span alone: lexical tokens (one stamped late, one tag among the ids), punctuation
    only, or tags only.  (staged ids with tags, one absolute frame per id that is no tag)."""
    kind = request.span_start_frame % 3
    s, e = request.span_start_frame, request.span_end_frame
    if kind == 0:
        return [TAG_EN, 20 + s % 20, DOT, 21 + e % 19], [max(0, s) + 1, e, e + 3]
    if kind == 1:
        return [DOT, COMMA], [s + 1, e + 2]
    return [TAG_EN, TAG_DE], []


@dataclass
class Step:
    patterns: list                       # per stream: '0' / '1' per window
    tokens: dict = field(default_factory=dict)   # stream -> [(frame, id)] appended to the live tokens before track; a tag id has no frame
    active: list | None = None           # per stream, None: all
    chunk_frames: int = 56               # mel frames of this chunk
    mel_stride: int = 1                  # element stride of the mel's frame axis
    tail: int = 0                        # samples behind the last whole window


@dataclass
class Scenario:
    name: str
    cfg: R.Config
    steps: list
    streams: int = 5
    seed: int = 1
    rescue_chunk_samples: int = 4480     # the rescue decode's chunk: 3.5 windows of 1280
    request_capacity: int = 8
    arena_capacity: int = 8 * 6 * 4480
    token_capacity: int = 48
    staged_capacity: int = 6
    enc_frames: int = 7                  # what the encoder reports for a chunk that ran
    finalize: tuple = ()                 # streams finalized after the last step

    def chunk(self, t: int) -> np.ndarray:
        return audio(self.steps[t].patterns, self.cfg.window_samples, self.seed * 1000 + t, self.steps[t].tail)

    def mel(self, t: int) -> np.ndarray:
        """[streams, mel_features, chunk_frames * mel_stride]: the chunk's mel lives at every mel_stride-th column."""
        s = self.steps[t]
        return np.random.default_rng(self.seed * 7000 + t).standard_normal((self.streams, self.cfg.mel_features, s.chunk_frames * s.mel_stride)).astype(np.float32)


def _main() -> Scenario:
    cfg = R.Config(total_mel_frames=65, mel_features=8, vad_rms_threshold=0.003)
    rows = [
        # a span inside one chunk with a one-window pre-roll; a span over two chunks; close and reopen (empty pre-roll); two closures; open at the end
        ["0110000", "0000110", "0000000", "1100110", "0011000", "0000000", "0000000", "0000011"],
        # a span over three chunks that emitted; one speech window; a span with only punctuation inside
        ["0000011", "1111111", "1000000", "0100000", "0000000", "0000001", "1000000", "0000000"],
        # tokens at start - 1, last + 5 (no request), start - 2 and last + 6, punctuation inside (requests)
        ["0011000", "0000000", "0011000", "0000000", "0011000", "0000000", "0011000", "0000000"],
        # inactive at steps 2 and 5
        ["1100000", "0000000", "1111111", "0110000", "0000000", "1111111", "0000000", "0000000"],
        # silence: the gate's hangover, a loud chunk that resets it
        ["0000000", "0000000", "0000000", "0001000", "0000000", "0000000", "0000000", "0000000"],
    ]
    tokens = [
        {1: [(None, TAG_EN)], 2: [(None, TAG_DE), (1, 22)]},
        {1: [(10, 23), (11, DOT)]},
        {2: [(22, 24)]},
        {},
        {2: [(28, 25), (37, 26)]},
        {1: [(41, COMMA)]},
        {2: [(44, DOT)]},
        {},
    ]
    frames = [5, 56, 60, 56, 56, 3, 56, 56]          # shorter than the cache, the room exactly, more than the room
    strides = [1, 1, 1, 2, 1, 3, 1, 1]
    steps = [Step([r[t] for r in rows], tokens[t], [1, 1, 1, 0 if t in (2, 5) else 1, 1], frames[t], strides[t]) for t in range(8)]
    return Scenario("main", cfg, steps, finalize=(4, 0, 2))


def _overflow() -> Scenario:
    """max_span_samples = 8 windows: a span that outgrows it drops its audio, keeps running until it closes and asks for nothing; threshold 0
    turns the gate off; the tail behind the last window moves the rows off the 16-byte grid."""
    cfg = R.Config(total_mel_frames=20, mel_features=3, pre_encode_cache=4, max_span_samples=8 * 1280, vad_rms_threshold=0.0)
    rows = [["0001111", "1111111", "1100000", "0110000", "0000000"],      # 3 pre-roll + 6 windows > 8: overflow at the sixth; then a span that fits
            ["1111100", "0000000", "0000000", "1111111", "1000000"],      # 5 + 2 closing windows = 7 <= 8: kept; 1 pre-roll ... overflow
            ["0000000", "0111111", "0000000", "0000000", "0011000"]]
    steps = [Step([r[t] for r in rows], {}, None, 16, 1, tail=(0, 641, 0, 2, 0)[t]) for t in range(5)]
    return Scenario("overflow", cfg, steps, streams=3, seed=2, finalize=(0, 1, 2))


def _w320() -> Scenario:
    """window_samples 320: lanes with two and with one 16-byte load; every chunk two samples longer than its windows."""
    cfg = R.Config(total_mel_frames=12, mel_features=2, pre_encode_cache=2, window_samples=320, max_span_samples=100 * 320, vad_rms_threshold=0.003, vad_hangover_chunks=1)
    rows = [["0110000", "0000110", "0000000"], ["0000000", "0000000", "1100000"]]
    steps = [Step([r[t] for r in rows], {}, None, 10, 1, tail=2) for t in range(3)]
    return Scenario("w320", cfg, steps, streams=2, seed=3, rescue_chunk_samples=1000, arena_capacity=8 * 4000, finalize=(1,))


def _long() -> Scenario:
    """67 windows a chunk: two ballot words, with closures on both sides of the word boundary."""
    cfg = R.Config(total_mel_frames=30, mel_features=2, vad_rms_threshold=0.003)
    a = "0" * 5 + "11" + "0" * 50 + "0001110" + "011"           # closes in word 0; opens at 60, closes at 65 (word 1); open at the end
    b = "0" * 60 + "1111" + "000"                               # opens in word 0, closes in word 1
    steps = [Step([a, b], {1: [(61, 30)]}, None, 20, 1, tail=640), Step(["0" * 67, "1" + "0" * 66], {}, None, 20, 1)]
    return Scenario("long", cfg, steps, streams=2, seed=4, request_capacity=8, arena_capacity=8 * 4 * 4480, finalize=(0,))


SCENARIOS = {s.name: s for s in (_main(), _overflow(), _w320(), _long())}


@dataclass
class Expected:
    """One scenario run through the restatement in the library's order: per step what every device step should leave."""
    gate: list = field(default_factory=list)          # per step: (skip per stream or None when inactive, run list)
    rows: list = field(default_factory=list)          # per step: mel rows [len(run), F, total]
    requests: list = field(default_factory=list)      # per step: [Request] in stream order
    commits: list = field(default_factory=list)       # per step: [bool] per request
    states: list = field(default_factory=list)        # per step: deep copies of the sessions
    final_requests: list = field(default_factory=list)
    final_commits: list = field(default_factory=list)
    final_states: list = field(default_factory=list)
    closes: list = field(default_factory=list)        # (stream, step, start, last, outcome): the closures seen (the CPU test's conditions)
    opens: list = field(default_factory=list)         # (stream, step, frame, pre_roll_frames)


class LoggedSession(R.Session):
    def close_span_and_maybe_rescue(self, rescue):
        before, info = self.detected, (self.span_start_frame, self.span_last_speech_frame, self.span_speech_windows, self.span_overflowed)
        hit = []
        super().close_span_and_maybe_rescue(lambda q: (hit.append(q), rescue(q)))
        outcome = "overflow" if info[3] else "short" if info[2] < self.cfg.min_speech_windows else "request" if self.detected > before else "emitted"
        self.events.append(("close", info[0], info[1], outcome))


def append_tokens(session: R.Session, tokens):
    for frame, token_id in tokens:
        session.ids.append(token_id)
        if frame is not None:
            session.timings.append(R.Timing(token_id, float(frame) * R.SECONDS_PER_FRAME))


def copy_session(s: R.Session):
    import copy
    return copy.deepcopy(s)


def expected(sc: Scenario) -> Expected:
    table = class_table()
    sessions = [LoggedSession(sc.cfg, table, b) for b in range(sc.streams)]
    for s in sessions:
        s.events = []
    out = Expected()
    for t, step in enumerate(sc.steps):
        chunk, mel = sc.chunk(t), sc.mel(t)[:, :, ::step.mel_stride]
        active = step.active or [1] * sc.streams
        skips, run = [], []
        for b, s in enumerate(sessions):
            if not active[b]:
                skips.append(None)
                continue
            skips.append(int(s.gate(chunk[b])))
            if not skips[-1]:
                run.append(b)
        out.gate.append((skips, run))
        out.rows.append(np.stack([sessions[b].mel_input(mel[b]) for b in run]) if run else np.zeros((0, sc.cfg.mel_features, sc.cfg.total_mel_frames), np.float32))
        for b in run:
            sessions[b].absolute_frame_base += sc.enc_frames
        found = []
        for b, s in enumerate(sessions):
            append_tokens(s, step.tokens.get(b, []))
            if active[b]:
                n = len(s.events)
                opened = (s.span_open, s.span_start_frame)
                s.track(chunk[b], found.append)
                out.closes += [(b, t) + e[1:] for e in s.events[n:]]
                if s.span_open and (s.span_open, s.span_start_frame) != opened:
                    out.opens.append((b, t, s.span_start_frame, s.span_pre_roll_frames))
        out.requests.append(found)
        out.commits.append([sessions[q.stream].commit(q, *stub_decoder(q)) for q in found])
        out.states.append([copy_session(s) for s in sessions])
    found = []
    for b in sc.finalize:
        n = len(sessions[b].events)
        sessions[b].finalize(found.append)
        out.closes += [(b, len(sc.steps)) + e[1:] for e in sessions[b].events[n:]]
    out.final_requests = found
    out.final_commits = [sessions[q.stream].commit(q, *stub_decoder(q)) for q in found]
    out.final_states = [copy_session(s) for s in sessions]
    return out


# ---- the independence claim's random sessions
def random_session(seed: int):
    """(config, chunks of loud / silent patterns, live tokens per chunk): spans of every length, closures that share a chunk, tokens on and
    around the spans."""
    rng = np.random.default_rng(seed)
    close = int(rng.integers(1, 4))
    cfg = R.Config(total_mel_frames=20, window_samples=8, max_span_samples=int(rng.choice([6, 12, 40])) * 8, close_silent_windows=close,
                   open_slack_frames=int(rng.integers(0, close)),   # the claim's condition: the closing silence is longer than the onset slack
                   pre_roll_windows=int(rng.integers(0, 4)), min_speech_windows=int(rng.integers(1, 3)))
    windows = int(rng.choice([7, 14, 28]))
    steps = []
    for t in range(int(rng.integers(3, 7))):
        run = rng.random(windows) < rng.choice([0.2, 0.5, 0.8])
        pattern = "".join("1" if x else "0" for x in run)
        count = int(rng.integers(0, 4))
        frames = rng.integers(max(0, t * windows - 8), (t + 1) * windows + 8, count)
        ids = rng.choice([20, 21, DOT, COMMA, 22], count)
        steps.append((pattern, [(int(f), int(i)) for f, i in zip(frames, ids)] + ([(None, TAG_EN)] if rng.random() < 0.2 else [])))
    return cfg, steps


def random_decoder(request: R.Request):
    """Deterministic in the span; the late tokens get clamped."""
    rng = np.random.default_rng(request.span_start_frame * 7919 + request.span_end_frame)
    n = int(rng.integers(0, 4))
    ids = [int(x) for x in rng.choice([20, 23, DOT, 24], n)]
    frames = sorted(int(x) for x in rng.integers(max(0, request.span_start_frame), request.span_end_frame + 6, n))
    return ([TAG_EN] if rng.random() < 0.3 else []) + ids, frames
