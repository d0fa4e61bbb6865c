"""A line-by-line restatement of FsmnVadManager's host arithmetic (reference: Sources/FluidAudio/VAD/Fsmn/FsmnVadManager.swift), the
expectation of the FSMN-VAD tests: concatenateChunks (:91-109), lfrFrameCount (:113-117), the row, bucket and gather steps of
chunkSilence (:119-155) and decide (:159-201).  Test infrastructure: plain Python and numpy, nothing of the library.

decide is parameterised by the constants the reference keeps private (Config), and counts per run how often each event occurred
(Events): opens, each close reason, and the frames whose window count puts them into the toggle class (w >= on and w <= off) or the
hold class (w < on and w > off)."""
from dataclasses import dataclass, field

import numpy as np

BUCKETS = [512, 1024, 2048, 3072]                                    # :25
FEATURE_DIM = 400
WAVEFORM_SCALE = np.float32(32768.0)
HOP_SAMPLES, FBANK_WINDOW_SAMPLES, LFR_PAD_FRAMES, LFR_WIDTH = 160, 400, 2, 5   # :31-34
WINDOW_FRAMES = 20                                                   # :38, which concatenateChunks reads at :95
END_SILENCE, MAX_LENGTH, END_OF_AUDIO = 0, 1, 2


@dataclass
class Config:                                                        # :37-45
    silence_threshold: float = 0.2
    window_frames: int = 20
    sil_to_speech: int = 15
    speech_to_sil: int = 15
    max_end_silence_frames: int = 80
    lookback_frames: int = 20
    lookahead_frames: int = 10
    max_segment_frames: int = 6000
    frame_ms: int = 10


@dataclass
class Events:
    opens: int = 0
    closes: list = field(default_factory=lambda: [0, 0, 0])          # by reason
    toggle_frames: int = 0
    hold_frames: int = 0

    def add(self, other):
        self.opens += other.opens
        self.closes = [a + b for a, b in zip(self.closes, other.closes)]
        self.toggle_frames += other.toggle_frames
        self.hold_frames += other.hold_frames


def lfr_frame_count(samples):                                        # :113-117
    if not samples >= FBANK_WINDOW_SAMPLES:
        return 0
    fbank_frames = (samples - FBANK_WINDOW_SAMPLES) // HOP_SAMPLES + 1
    return max(0, fbank_frames + LFR_PAD_FRAMES - LFR_WIDTH + 1)


def concatenate_chunks(sample_count, score):                         # :91-109; score(start, end) -> a list
    chunk_samples = (BUCKETS[-1] - WINDOW_FRAMES) * HOP_SAMPLES
    sil = []
    start = 0
    while start < sample_count:
        end = min(start + chunk_samples, sample_count)
        chunk_sil = score(start, end)
        keep_from = 0 if start == 0 else LFR_PAD_FRAMES
        if not len(chunk_sil) > keep_from:
            break
        sil.extend(chunk_sil[keep_from:])
        if end == sample_count:
            break
        start = (len(sil) - LFR_PAD_FRAMES) * HOP_SAMPLES
    return sil


def bucket_for(t):                                                   # :131
    return next((b for b in BUCKETS if b >= t), BUCKETS[-1])


def plan_chunks(sample_count):
    """The chunks concatenateChunks scores when the scorer yields lfrFrameCount frames — the published preprocessor geometry the
    reference's FsmnVadChunkingTests stands on: (bucket, start, end, frames, keep_from, first_frame) per kept chunk, and the total."""
    chunks = []

    def score(start, end):
        frames = lfr_frame_count(end - start)
        chunks.append([start, end, frames])
        return [0.0] * frames
    total = len(concatenate_chunks(sample_count, score))
    out, so_far = [], 0
    for start, end, frames in chunks:
        keep_from = 0 if start == 0 else LFR_PAD_FRAMES
        if not frames > keep_from:
            break
        out.append((bucket_for(frames), start, end, frames, keep_from, so_far))
        so_far += frames - keep_from
    assert so_far == total
    return out, total


def waveform_row(audio, start, end, row_stride):                     # :120-123
    row = np.zeros(row_stride, np.float32)
    row[:end - start] = np.asarray(audio[start:end], np.float32) * WAVEFORM_SCALE
    return row


def bucket_rows(feats, t, bucket):                                   # :131-140: feats [>= t, 400], fp32 or fp16
    speech = np.zeros((bucket, FEATURE_DIM), np.float32)
    speech[:t] = np.asarray(feats[:t]).astype(np.float32)
    return speech


def gather_silence(scores, t):                                       # :146-153: scores [bucket, vocab]
    return [np.float32(scores[frame, 0]) for frame in range(t)]


def decide(silence, cfg=None, events=None):                          # :159-201
    """-> [(start_frame, end_frame, reason, start_ms, end_ms)]"""
    cfg = cfg or Config()
    ev = events if events is not None else Events()
    speech = (np.asarray(silence, np.float32) <= np.float32(cfg.silence_threshold)).tolist()   # :176, an fp32 comparison: a NaN is not speech
    T = len(silence)
    win = [0] * cfg.window_frames
    pos = 0
    win_sum = 0
    pre_speech = False
    in_seg = False
    seg_start = 0
    cont_sil = 0
    segs = []

    def close(at, reason):
        segs.append((seg_start, at, reason, seg_start * cfg.frame_ms, at * cfg.frame_ms))
        ev.closes[reason] += 1

    for t in range(T):
        cur = 1 if speech[t] else 0
        win_sum -= win[pos]
        win_sum += cur
        win[pos] = cur
        pos = (pos + 1) % cfg.window_frames
        at_on, at_off = win_sum >= cfg.sil_to_speech, win_sum <= cfg.speech_to_sil
        ev.toggle_frames += at_on and at_off
        ev.hold_frames += (not at_on) and (not at_off)
        if not pre_speech and at_on:
            pre_speech = True
            if not in_seg:
                in_seg = True
                seg_start = max(0, t - cfg.sil_to_speech - cfg.lookback_frames)
                cont_sil = 0
                ev.opens += 1
        elif pre_speech and at_off:
            pre_speech = False
        if in_seg and not pre_speech:
            cont_sil += 1
        else:
            cont_sil = 0
        if in_seg and cont_sil >= cfg.max_end_silence_frames:
            close(t - cfg.max_end_silence_frames + cfg.lookahead_frames, END_SILENCE)
            in_seg = False
        elif in_seg and (t - seg_start) >= cfg.max_segment_frames:
            close(t, MAX_LENGTH)
            in_seg = False
            pre_speech = False
    if in_seg:
        close(T, END_OF_AUDIO)
    return segs
