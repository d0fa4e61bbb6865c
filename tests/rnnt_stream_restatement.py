"""The Nemotron streaming session's glue, restated line by line from the reference (Sources/FluidAudio/ASR/Parakeet/Streaming/Nemotron/
StreamingNemotronMultilingualAsrManager+BlankRescue.swift = BR, +Pipeline.swift = PL, +Buffers.swift = BU): the VAD-gated skip, the mel cache,
the span machine, the closing test, the rescue's staging and mergeRescuedTokens.  Times are the reference's doubles (frame * 0.08); the RMS
is float64 (vDSP_rmsqv's order is unspecified: the cases keep every RMS away from its threshold).  The session keeps the reference's
"immediate" order — a rescue runs the moment its span closes, with the decoder passed in — and can also run the library's deferred order
(all closures of a chunk judged first, merged afterwards) for the independence claim."""
from __future__ import annotations

import unicodedata
from dataclasses import dataclass, field

import numpy as np

SECONDS_PER_FRAME = 0.08                      # ASRConstants.secondsPerEncoderFrame
LEXICAL, LANG_TAG = 1, 2


@dataclass
class Config:
    total_mel_frames: int = 65
    window_samples: int = 1280                # ASRConstants.samplesPerEncoderFrame
    close_silent_windows: int = 2             # BR:44
    pre_roll_windows: int = 3                 # BR:45
    min_speech_windows: int = 2               # BR:46
    max_span_samples: int = 15 * 16000        # BR:47
    open_slack_frames: int = 1                # BR:146
    close_slack_frames: int = 5               # BR:148
    rescue_rms_threshold: float = 0.0025      # BR:32
    vad_rms_threshold: float = 0.0            # BU:35-40
    vad_hangover_chunks: int = 2              # BU:46-51
    mel_features: int = 128
    pre_encode_cache: int = 9


def rms64(x) -> float:
    x = np.asarray(x, np.float64)
    return float(np.sqrt(np.mean(x * x))) if x.size else 0.0


def is_audio_silent(samples, threshold) -> bool:          # BU:56-63
    if len(samples) == 0:
        return True
    return rms64(samples) < float(np.float32(threshold))


def contains_lexical_content(raw: str) -> bool:            # BR:358-360: CharacterSet.alphanumerics = categories L*, M*, N*
    return any(unicodedata.category(ch)[0] in "LMN" for ch in raw)


@dataclass
class Timing:                                              # the fields of TokenTiming this path reads
    token_id: int
    start_time: float


def merge_rescued_tokens(live_ids, live_timings, rescued_ids, rescued_timings, lang_tags, span_start_sec):   # BR:323-354
    insert_key = rescued_timings[0].start_time if rescued_timings else span_start_sec                        # :331
    timing_insert_index = next((i for i, t in enumerate(live_timings) if t.start_time > insert_key), len(live_timings))   # :332-333
    ids_insert_index, timed_seen = len(live_ids), 0                                                           # :337-347
    for index, i in enumerate(live_ids):
        if timed_seen == timing_insert_index and i not in lang_tags:
            ids_insert_index = index
            break
        if i not in lang_tags:
            timed_seen += 1
    ids = list(live_ids[:ids_insert_index]) + list(rescued_ids) + list(live_ids[ids_insert_index:])           # :349-352
    timings = list(live_timings[:timing_insert_index]) + list(rescued_timings) + list(live_timings[timing_insert_index:])
    return ids, timings


@dataclass
class Request:
    stream: int
    span_start_frame: int
    span_end_frame: int
    speech_windows: int
    audio: np.ndarray

    def decode_chunks(self, chunk_samples: int) -> int:    # BR:243-259
        n = len(self.audio)
        if n % chunk_samples:
            n += chunk_samples - n % chunk_samples
        return (n + chunk_samples) // chunk_samples

    def padded(self, chunk_samples: int) -> np.ndarray:
        out = np.zeros(self.decode_chunks(chunk_samples) * chunk_samples, np.float32)
        out[:len(self.audio)] = self.audio
        return out


@dataclass
class Session:
    cfg: Config
    classes: np.ndarray                                    # the class byte per id
    stream: int = 0
    # resetRescueState (BR:398-412) and resetStates
    rescue_frame_cursor: int = 0
    span_open: bool = False
    span_start_frame: int = 0
    span_last_speech_frame: int = 0
    span_speech_windows: int = 0
    span_pre_roll_frames: int = 0
    silent_window_run: int = 0
    span_audio: list = field(default_factory=list)         # windows
    span_overflowed: bool = False
    pre_roll_tail: list = field(default_factory=list)      # windows
    detected: int = 0
    rescued: int = 0
    vad_low: int = 0
    vad_skips: int = 0
    absolute_frame_base: int = 0
    mel_cache: np.ndarray | None = None
    ids: list = field(default_factory=list)                # accumulatedTokenIds
    timings: list = field(default_factory=list)            # accumulatedTokenTimings

    def cls(self, i: int) -> int:
        return int(self.classes[i]) if 0 <= i < len(self.classes) else 0

    # ---- PL:86-104
    def gate(self, samples) -> bool:
        c = self.cfg
        if float(np.float32(c.vad_rms_threshold)) > 0:
            if is_audio_silent(samples, c.vad_rms_threshold):
                self.vad_low += 1
                if self.vad_low >= c.vad_hangover_chunks:
                    self.vad_skips += 1
                    self.absolute_frame_base += len(samples) // c.window_samples
                    return True
            else:
                self.vad_low = 0
        return False

    # ---- BU:170-210, 140-165
    def mel_input(self, chunk_mel: np.ndarray) -> np.ndarray:
        c = self.cfg
        chunk_frames = chunk_mel.shape[1]
        result = np.zeros((c.mel_features, c.total_mel_frames), np.float32)
        if self.mel_cache is not None:
            result[:, :self.mel_cache.shape[1]] = self.mel_cache
        copy_frames = min(chunk_frames, c.total_mel_frames - c.pre_encode_cache)
        result[:, c.pre_encode_cache:c.pre_encode_cache + copy_frames] = chunk_mel[:, :copy_frames]
        cache_frames = min(c.pre_encode_cache, chunk_frames)
        self.mel_cache = np.array(chunk_mel[:, chunk_frames - cache_frames:], np.float32)
        return result

    # ---- BR:51-60, 70-119.  rescue(request) is called for every span that asks for one.
    def track(self, chunk, rescue):
        c, W = self.cfg, self.cfg.window_samples
        if not float(np.float32(c.rescue_rms_threshold)) > 0:
            return
        chunk_start_frame = self.rescue_frame_cursor
        self.rescue_frame_cursor += len(chunk) // W
        for index in range(len(chunk) // W):
            window = np.asarray(chunk[index * W:(index + 1) * W], np.float32)
            silent = rms64(window) < float(np.float32(c.rescue_rms_threshold))
            frame = chunk_start_frame + index
            if self.span_open:
                if silent:
                    self.silent_window_run += 1
                else:
                    self.silent_window_run = 0
                    self.span_last_speech_frame = frame
                    self.span_speech_windows += 1
            elif not silent:
                self.span_open = True
                self.span_start_frame = frame
                self.span_last_speech_frame = frame
                self.span_speech_windows = 1
                self.silent_window_run = 0
                self.span_audio = list(self.pre_roll_tail)
                self.span_pre_roll_frames = len(self.pre_roll_tail)
                self.span_overflowed = False
            if self.span_open and not self.span_overflowed:
                self.span_audio.append(window)
                if len(self.span_audio) * W > c.max_span_samples:
                    self.span_overflowed = True
                    self.span_audio = []
            elif not self.span_open:
                self.pre_roll_tail.append(window)
                if len(self.pre_roll_tail) > c.pre_roll_windows:
                    del self.pre_roll_tail[:len(self.pre_roll_tail) - c.pre_roll_windows]
            if self.span_open and self.silent_window_run >= c.close_silent_windows:
                self.close_span_and_maybe_rescue(rescue)

    def finalize(self, rescue):                            # BR:64-67
        if float(np.float32(self.cfg.rescue_rms_threshold)) > 0 and self.span_open:
            self.close_span_and_maybe_rescue(rescue)

    def close_span_and_maybe_rescue(self, rescue):         # BR:123-164
        c = self.cfg
        span_audio, start_frame, last_speech_frame = self.span_audio, self.span_start_frame, self.span_last_speech_frame
        speech_windows, pre_roll_frames, overflowed = self.span_speech_windows, self.span_pre_roll_frames, self.span_overflowed
        self.span_open = False
        self.span_audio = []
        self.span_speech_windows = 0
        self.silent_window_run = 0
        self.span_overflowed = False
        self.pre_roll_tail = []
        if overflowed or speech_windows < c.min_speech_windows:
            return
        open_sec = (float(start_frame) - c.open_slack_frames) * SECONDS_PER_FRAME
        close_sec = (float(last_speech_frame) + c.close_slack_frames) * SECONDS_PER_FRAME
        if any(open_sec <= t.start_time <= close_sec and (self.cls(t.token_id) & LEXICAL) for t in self.timings):
            return
        self.detected += 1
        audio = np.concatenate(span_audio) if span_audio else np.zeros(0, np.float32)
        rescue(Request(self.stream, start_frame - pre_roll_frames, last_speech_frame + 1, speech_windows, audio))

    # ---- BR:264-305: what rescueDecode does with the trial decode's output.  staged_ids: with language tags; staged_frames: one absolute
    # frame per id that is no tag.  Returns True when the rescue was committed.
    def commit(self, request: Request, staged_ids, staged_frames) -> bool:
        tags = {i for i in set(staged_ids) | set(self.ids) if self.cls(i) & LANG_TAG}
        ids = [i for i in staged_ids if i not in tags]                                                       # :264-265
        assert len(ids) == len(staged_frames)
        span_end_sec = float(request.span_end_frame) * SECONDS_PER_FRAME                                     # :270
        timings = []
        for i, f in zip(ids, staged_frames):
            start = float(f) * SECONDS_PER_FRAME
            timings.append(Timing(i, start if start <= span_end_sec else span_end_sec))                      # :271-278
        if not any(self.cls(i) & LEXICAL for i in ids):                                                       # :285-294
            return False
        span_start_sec = float(max(0, request.span_start_frame)) * SECONDS_PER_FRAME                         # :296
        self.ids, self.timings = merge_rescued_tokens(self.ids, self.timings, ids, timings, tags, span_start_sec)
        self.rescued += 1                                                                                     # :305
        return True

    # ---- the two orders
    def track_immediate(self, chunk, decoder, log=None):
        """The reference's order: the rescue decode and its merge run inside the window loop."""
        def rescue(request):
            if log is not None:
                log.append(request)
            self.commit(request, *decoder(request))
        self.track(chunk, rescue)

    def track_deferred(self, chunk, decoder, log=None):
        """The library's order: every closure of the chunk judged against the live timings, the merges afterwards in request order."""
        found = []
        self.track(chunk, found.append)
        for request in found:
            if log is not None:
                log.append(request)
            self.commit(request, *decoder(request))
