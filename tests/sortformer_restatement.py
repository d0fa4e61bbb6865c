"""Plain numpy restatement of the offline Sortformer path around its network and of the diarizer timeline, loop for loop (test
infrastructure; the product never imports it).  Reference: Sources/FluidAudio/Diarizer/Sortformer/Offline/OfflineSortformerDiarizer.swift
(:98-119 the model input, :303-363 windows and stitching), Sortformer/Offline/SortformerSpeakerStitcher.swift (:27-90), and
Diarizer/DiarizerTimeline.swift (:9-164 config, :492-560 segment, :649-661 scratch, :821-891 addChunk / finalize, :945-1003 rebuild,
:1169-1336 updateSegments / commitSegment).  Every float is an np.float32 scalar; a product and the sum it feeds are two roundings."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F = np.float32
INT_MIN = -(2 ** 63)


@dataclass
class OfflineConfig:   # OfflineSortformerConfig (:14-58)
    window_output_frames: int = 384
    subsampling: int = 8
    speakers: int = 4
    n_mels: int = 128
    overlap_output_frames: int = 100

    @property
    def window_mel_frames(self):
        return self.window_output_frames * self.subsampling

    @property
    def frame_duration_seconds(self):
        return F(F(self.subsampling) * F(160) / F(16000))


def offline_windows(cfg: OfflineConfig, num_mel_frames: int):
    """The loop of :303-363 without the model: (windows, totalOut); a window = dict(mel_start, valid_mel, g_start, valid_out)."""
    window_mel, out_per_window, sub = cfg.window_mel_frames, cfg.window_output_frames, cfg.subsampling
    overlap_out = max(0, min(cfg.overlap_output_frames, out_per_window - 1))
    hop_mel = (out_per_window - overlap_out) * sub
    total_out = (num_mel_frames + sub - 1) // sub
    wins = []
    mel_start = 0
    while mel_start < num_mel_frames:
        valid_mel = min(window_mel, num_mel_frames - mel_start)
        wins.append(dict(mel_start=mel_start, valid_mel=valid_mel, g_start=mel_start // sub,
                         valid_out=min(out_per_window, (valid_mel + sub - 1) // sub)))
        if valid_mel < window_mel:
            break
        mel_start += hop_mel
    return wins, total_out


def pack_window(cfg: OfflineConfig, mel_time_major: np.ndarray, win) -> tuple:
    """runOffline's input (:98-119) from the recording's time-major mel [T, n_mels]: ([n_mels, windowMel] zero-padded, mel_length)."""
    frames = min(win["valid_mel"], cfg.window_mel_frames)
    dst = np.zeros((cfg.n_mels, cfg.window_mel_frames), np.float32)
    dst[:, :frames] = mel_time_major[win["mel_start"]:win["mel_start"] + frames].T
    return dst, frames


def _permute(array, k, body):   # SortformerSpeakerStitcher.permute (:80-90)
    if k == len(array):
        body(list(array))
        return
    for i in range(k, len(array)):
        array[k], array[i] = array[i], array[k]
        _permute(array, k + 1, body)
        array[k], array[i] = array[i], array[k]


def permutations(n: int) -> list:
    out = []
    _permute(list(range(n)), 0, out.append)
    return out


def alignment(global_, window, frames: int, num_speakers: int) -> list:
    """SortformerSpeakerStitcher.alignment (:27-77): mapping[windowSpeaker] == globalSpeaker."""
    identity = list(range(num_speakers))
    global_ = np.asarray(global_, np.float32).reshape(-1)
    window = np.asarray(window, np.float32).reshape(-1)
    if not (frames > 0 and num_speakers > 0 and global_.size >= frames * num_speakers and window.size >= frames * num_speakers):
        return identity
    corr = [[F(0)] * num_speakers for _ in range(num_speakers)]
    with np.errstate(all="ignore"):
        for f in range(frames):
            base = f * num_speakers
            for g in range(num_speakers):
                gv = global_[base + g]
                if not gv != 0:
                    continue
                for w in range(num_speakers):
                    corr[g][w] = F(corr[g][w] + F(gv * window[base + w]))
        best = {"perm": identity, "score": F(-np.finfo(np.float32).max)}

        def body(candidate):
            score = F(0)
            for g in range(num_speakers):
                score = F(score + corr[g][candidate[g]])
            if score > best["score"]:
                best["score"], best["perm"] = score, candidate

        _permute(list(identity), 0, body)
    mapping = list(identity)
    for g in range(num_speakers):
        mapping[best["perm"][g]] = g
    return mapping


def stitch(cfg: OfflineConfig, num_mel_frames: int, preds: np.ndarray):
    """:303-363 with the model's outputs given: preds [windows, windowOut, S] -> (global [totalOut, S], mappings [windows, S])."""
    wins, total_out = offline_windows(cfg, num_mel_frames)
    speakers, out_per_window = cfg.speakers, cfg.window_output_frames
    overlap_out = max(0, min(cfg.overlap_output_frames, out_per_window - 1))
    glob = np.zeros(total_out * speakers, np.float32)
    filled = np.zeros(total_out, bool)
    mappings = np.zeros((len(wins), speakers), np.int32)
    half = F(0.5)
    with np.errstate(all="ignore"):
        for wi, win in enumerate(wins):
            p = np.asarray(preds[wi], np.float32).reshape(-1)
            valid_out, g_start = win["valid_out"], win["g_start"]
            mapping = list(range(speakers))
            if wi > 0 and overlap_out > 0:
                ov = min(overlap_out, valid_out, max(0, total_out - g_start))
                if ov > 0:
                    mapping = alignment(glob[g_start * speakers:(g_start + ov) * speakers].copy(), p[:ov * speakers].copy(), ov, speakers)
            for j in range(valid_out):
                gf = g_start + j
                if not gf < total_out:
                    break
                for w in range(speakers):
                    idx = gf * speakers + mapping[w]
                    glob[idx] = F(F(glob[idx] + p[j * speakers + w]) * half) if filled[gf] else p[j * speakers + w]
                filled[gf] = True
            mappings[wi] = mapping
    return glob.reshape(total_out, speakers), mappings


def stitch_from_previous(cfg: OfflineConfig, num_mel_frames: int, preds: np.ndarray):
    """The same, with the overlap region read from the PREVIOUS window's own values moved by its mapping instead of from the global
    timeline (what the device's parallel path computes from); equal to stitch() when 2 * overlap <= window."""
    wins, total_out = offline_windows(cfg, num_mel_frames)
    speakers, out_per_window = cfg.speakers, cfg.window_output_frames
    overlap_out = max(0, min(cfg.overlap_output_frames, out_per_window - 1))
    hop = out_per_window - overlap_out
    mappings = np.zeros((len(wins), speakers), np.int32)
    for wi, win in enumerate(wins):
        mapping = list(range(speakers))
        if wi > 0 and overlap_out > 0:
            ov = min(overlap_out, win["valid_out"], max(0, total_out - win["g_start"]))
            if ov > 0:
                prev = np.asarray(preds[wi - 1], np.float32)[hop:hop + ov]
                moved = np.zeros((ov, speakers), np.float32)
                moved[:, mappings[wi - 1]] = prev
                mapping = alignment(moved, np.asarray(preds[wi], np.float32)[:ov], ov, speakers)
        mappings[wi] = mapping
    glob = np.zeros((total_out, speakers), np.float32)
    filled = np.zeros(total_out, bool)
    with np.errstate(all="ignore"):
        for wi, win in enumerate(wins):
            p = np.asarray(preds[wi], np.float32)
            for j in range(win["valid_out"]):
                gf = win["g_start"] + j
                if gf >= total_out:
                    break
                for w in range(speakers):
                    g = mappings[wi][w]
                    glob[gf, g] = F(F(glob[gf, g] + p[j, w]) * F(0.5)) if filled[gf] else p[j, w]
                filled[gf] = True
    return glob, mappings


# ------------------------------------------------------------------------------------------------ timeline

def swift_round(x) -> int:
    """Int(round(x)) on a Float: half away from zero."""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


@dataclass
class TimelineConfig:   # DiarizerTimelineConfig (:9-164)
    num_speakers: int = 1
    frame_duration_seconds: float = 0.08
    onset_threshold: float = 0.5
    offset_threshold: float = 0.5
    onset_pad_frames: int = 0
    offset_pad_frames: int = 0
    min_frames_on: int = 0
    min_frames_off: int = 0

    @staticmethod
    def sortformer_default():
        return TimelineConfig(num_speakers=4, frame_duration_seconds=0.08)

    @staticmethod
    def from_seconds(num_speakers=1, frame_duration_seconds=0.08, onset_threshold=0.5, offset_threshold=0.5, onset_pad_seconds=0.0,
                     offset_pad_seconds=0.0, min_duration_on=0.0, min_duration_off=0.0):
        """The second initialiser (:139-163)."""
        fd = F(frame_duration_seconds)
        return TimelineConfig(num_speakers, frame_duration_seconds, onset_threshold, offset_threshold,
                              swift_round(F(F(onset_pad_seconds) / fd)), swift_round(F(F(offset_pad_seconds) / fd)),
                              swift_round(F(F(min_duration_on) / fd)), swift_round(F(F(min_duration_off) / fd)))


@dataclass
class Segment:   # DiarizerSegment (:492-560)
    speaker_index: int
    start_frame: int
    end_frame: int
    finalized: bool
    frame_duration_seconds: float
    activity: np.float32 = F(0)

    @staticmethod
    def from_times(speaker_index, start_time, end_time, frame_duration_seconds, finalized=True):
        fd = F(frame_duration_seconds)
        return Segment(speaker_index, swift_round(F(F(start_time) / fd)), swift_round(F(F(end_time) / fd)), finalized, frame_duration_seconds)

    @property
    def start_time(self):
        return F(F(self.start_frame) * F(self.frame_duration_seconds))

    @property
    def end_time(self):
        return F(F(self.end_frame) * F(self.frame_duration_seconds))

    @property
    def duration(self):
        return F(F(self.end_frame - self.start_frame) * F(self.frame_duration_seconds))

    @property
    def length(self):
        return self.end_frame - self.start_frame


@dataclass
class _Scratch:   # SegmentScratch (:649-661)
    speaking: bool = False
    has_segment: bool = False
    start_frame: int = INT_MIN
    end_frame: int = INT_MIN
    activity_sum: np.float32 = F(0)
    active_frame_count: int = 0
    unmerged_start_frame: int = INT_MIN
    unmerged_activity_sum: np.float32 = F(0)
    unmerged_active_frame_count: int = 0

    def copy(self):
        return _Scratch(**self.__dict__)


@dataclass
class _Speaker:
    finalized_segments: list = field(default_factory=list)
    tentative_segments: list = field(default_factory=list)


class Timeline:
    """DiarizerTimeline: addChunk / finalize / rebuild and the segment detection behind them (.sigmoids activity)."""

    def __init__(self, config: TimelineConfig):
        self.config = config
        self.capacity = config.num_speakers
        self.reset()

    def reset(self):
        self.scratches = [_Scratch() for _ in range(self.capacity)]
        self.speakers: dict = {}
        self.cursor = 0

    def add_chunk(self, finalized, tentative=()):   # :827-872
        fin = np.asarray(finalized, np.float32).reshape(-1)
        tent = np.asarray(tentative, np.float32).reshape(-1)
        assert fin.size % self.capacity == 0 and tent.size % self.capacity == 0
        for sp in self.speakers.values():
            sp.tentative_segments.clear()
        new_fin, new_tent = [], []
        self._update(fin, True, False, new_fin, new_tent)
        self.cursor += fin.size // self.capacity
        self._update(tent, False, True, new_fin, new_tent)
        self._tentative_frames = tent.size // self.capacity
        return new_fin, new_tent

    def finalize(self):   # :883-891
        self.cursor += getattr(self, "_tentative_frames", 0)
        self._tentative_frames = 0
        for sp in self.speakers.values():
            sp.finalized_segments.extend(sp.tentative_segments)
            sp.tentative_segments = []

    def rebuild(self, finalized, tentative=(), is_complete=True):   # :945-1003, keepingSpeakers false
        fin = np.asarray(finalized, np.float32).reshape(-1)
        tent = np.asarray(tentative, np.float32).reshape(-1)
        assert fin.size % self.capacity == 0 and tent.size % self.capacity == 0
        new_fin, new_tent = [], []
        self.reset()
        self._update(fin, True, False, new_fin, new_tent)
        self.cursor = fin.size // self.capacity
        self._update(tent, False, True, new_fin, new_tent)
        self._tentative_frames = tent.size // self.capacity
        if is_complete:
            self.finalize()
        return new_fin, new_tent

    def records(self, recording: int = 0) -> list:
        """The speakers' lists after the call as the device entry reports them: (recording, speaker, start, end, activity bits, flag),
        flag bit 0 = isFinalized, bit 1 = held in the finalized list."""
        out = []
        for s in sorted(self.speakers):
            sp = self.speakers[s]
            for seg in sp.finalized_segments:
                out.append((recording, s, seg.start_frame, seg.end_frame, int(np.float32(seg.activity).view(np.uint32)), 2 | int(seg.finalized)))
            for seg in sp.tentative_segments:
                out.append((recording, s, seg.start_frame, seg.end_frame, int(np.float32(seg.activity).view(np.uint32)), int(seg.finalized)))
        return out

    def _update(self, predictions, is_finalized, add_trailing_tentative, finalized_result, tentative_result):   # :1169-1294
        if not (predictions.size > 0 or add_trailing_tentative):
            return
        c = self.config
        frame_offset = self.cursor
        onset, offset = F(c.onset_threshold), F(c.offset_threshold)
        pad_onset, pad_offset, min_frames_on, min_frames_off = c.onset_pad_frames, c.offset_pad_frames, c.min_frames_on, c.min_frames_off
        num_new_frames = predictions.size // self.capacity
        end_frame = frame_offset + num_new_frames
        pad = pad_onset + pad_offset
        min_segment_length = pad + min_frames_on
        finalized_end_frame = end_frame - min_frames_off - pad if is_finalized else INT_MIN
        preds = predictions.reshape(num_new_frames, self.capacity)
        with np.errstate(all="ignore"):
            for speaker_index in range(self.capacity):
                aux = self.scratches[speaker_index].copy()
                column = preds[:, speaker_index]
                for i in range(num_new_frames):
                    activity = column[i]
                    frame = frame_offset + i
                    if aux.speaking:
                        if activity >= offset:
                            aux.unmerged_activity_sum = F(aux.unmerged_activity_sum + activity)
                            aux.unmerged_active_frame_count += 1
                            continue
                        aux.speaking = False
                        end = frame + pad_offset
                        if not end >= aux.unmerged_start_frame + min_segment_length:
                            aux.has_segment = aux.end_frame >= aux.start_frame + min_segment_length
                            continue
                        aux.end_frame = end
                        aux.activity_sum = F(aux.activity_sum + aux.unmerged_activity_sum)
                        aux.active_frame_count += aux.unmerged_active_frame_count
                        aux.has_segment = True
                    elif activity > onset:
                        start = frame - pad_onset
                        aux.speaking = True
                        aux.unmerged_start_frame = start
                        aux.unmerged_activity_sum = F(activity)
                        aux.unmerged_active_frame_count = 1
                        if not (not aux.has_segment or start > aux.end_frame + min_frames_off):
                            aux.has_segment = False
                            continue
                        self._commit(aux, speaker_index, is_finalized, finalized_result, tentative_result)
                        aux.start_frame = start
                if aux.has_segment and (not is_finalized or aux.end_frame < finalized_end_frame):
                    self._commit(aux, speaker_index, is_finalized and aux.end_frame < finalized_end_frame, finalized_result, tentative_result)
                if is_finalized:
                    self.scratches[speaker_index] = aux
                    continue
                if not (add_trailing_tentative and aux.speaking):
                    continue
                padded_end = end_frame + pad_offset
                if not padded_end >= aux.start_frame + min_segment_length:
                    continue
                aux.has_segment = True
                if padded_end >= aux.unmerged_start_frame + min_segment_length:
                    aux.end_frame = padded_end
                    aux.activity_sum = F(aux.activity_sum + aux.unmerged_activity_sum)
                    aux.active_frame_count += aux.unmerged_active_frame_count
                self._commit(aux, speaker_index, False, finalized_result, tentative_result)

    def _commit(self, aux, slot, is_finalized, finalized_result, tentative_result):   # :1297-1336
        if not aux.has_segment:
            return
        activity = F(aux.activity_sum / F(aux.active_frame_count)) if aux.active_frame_count > 0 else F(0)
        seg = Segment(slot, aux.start_frame, aux.end_frame, is_finalized, self.config.frame_duration_seconds, activity)
        sp = self.speakers.setdefault(slot, _Speaker())
        (sp.finalized_segments if is_finalized else sp.tentative_segments).append(seg)
        (finalized_result if is_finalized else tentative_result).append(seg)
        aux.has_segment = False
        aux.activity_sum = F(0)
        aux.active_frame_count = 0


def timeline_records(config: TimelineConfig, finalized_list, tentative_list=None, is_complete=True) -> list:
    """rebuild per recording -> the concatenated records of Timeline.records."""
    out = []
    for r, fin in enumerate(finalized_list):
        t = Timeline(config)
        t.rebuild(fin, () if tentative_list is None else tentative_list[r], is_complete)
        out.extend(t.records(r))
    return out
