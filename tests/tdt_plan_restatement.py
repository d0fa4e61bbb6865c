"""A line-by-line Python restatement of how the reference plans the windows of a long recording for Parakeet-TDT
(Sources/FluidAudio/ASR/Parakeet/SlidingWindow/TDT/ChunkProcessor.swift; the numbers behind `# :` are its lines): chunkLayout :48-75 and
:140-161, lastChunkWarmupSamples :85-102, speechEndSamples :112-128, chunkStarts :163-177, regularChunkStarts :179-187,
silenceAlignedChunkStarts :189-268, bestBoundaryCandidate :270-310, the threshold tests :312-323, wouldCompressSpeechTail :325-348,
shouldUseWarmupPrefix :350-382, boundaryEnergyScore :384-396, the window loop of process :501-507, 520-565, 577, 626-636 (decodeOneChunk,
DualDecodeArbitration.swift:359-402, is the same arithmetic with mel context 0), transcribeChunk's frame counts :771-778,
padAudioIfNeeded (AsrManager+Pipeline.swift:153-156), adaptiveSpeechRmsThreshold :1245-1276 and speechLikeSeconds :1518-1534.

Every energy is the reference's `sum += sample * sample` in fp32, in order: np.cumsum(x * x, dtype=np.float32)[-1] — one rounded product
and one rounded addition per sample.  BRANCHES counts the routes taken, so that a test can say which ones its inputs reach.

One thing is this project's own: a recording is REFUSED (refused()) when the in-order sum of a window [f F - F, f F + F), clipped to the
recording, is not finite for some frame f.  Rounded addition of non-negative terms is monotone, so such a window's sum bounds the sum of
every run of consecutive samples inside it, and every run of at most F samples lies inside one: with all of them finite, every energy the
reference can take is finite."""
from __future__ import annotations

import collections
import dataclasses
import math

import numpy as np

F32 = np.float32
BRANCHES: collections.Counter = collections.Counter()
BRANCH_NAMES = ("near_silence", "valley", "target_fallback", "warmup_true", "warmup_false", "probe_loud", "probe_stable_quiet", "probe_end_of_audio",
                "tail_compression", "tail_eof_guard", "backfill", "pure_silence_tail", "step_beyond_list", "empty_candidates")
# what the argument checks leave no input for: targetStart lies above previousStart, as every candidate does, because a chunk is longer
# than the minimal overlap; and a window is at least one frame long.  (The empty candidate list IS reached: a start 4 s in front of its
# target puts latestCoveredStart below the next target's valley search, whose radius is 0.5 s.)
UNREACHABLE = ("repair_best_start", "chunk_end_le_start")
GREATEST_FINITE = np.finfo(np.float32).max

SPEECH_RMS_CEILING, SPEECH_RMS_FLOOR, SPEECH_RMS_REFERENCE_SCALE, SPEECH_RMS_REFERENCE_PERCENTILE = F32(0.008), F32(0.0005), F32(0.3), 0.75   # :1232-1241


@dataclasses.dataclass
class Config:
    sample_rate: int = 16000               # ASRConstants.sampleRate
    frame_samples: int = 1280              # ASRConstants.samplesPerEncoderFrame
    mel_hop: int = 160                     # ASRConstants.melHopSize
    max_model_samples: int = 240000        # ASRConstants.maxModelSamples
    overlap_seconds: float = 2.0           # ChunkProcessor.overlapSeconds
    mel_chunk_context: bool = True
    silence_aligned: bool = False          # preferSilenceAlignment: !melChunkContext && modelVersion == .v3
    warmup_prefix_frames: int = 0          # noMelWarmupPrefixFrames; path B of the arbitration: 7
    end_aligned: bool = True               # supportsSuppressedPrefix(modelVersion)


MODES = {                                  # the four combinations in use
    "default": dict(mel_chunk_context=True, silence_aligned=False, warmup_prefix_frames=0, end_aligned=True),
    "path_a": dict(mel_chunk_context=False, silence_aligned=True, warmup_prefix_frames=0, end_aligned=True),
    "path_b": dict(mel_chunk_context=False, silence_aligned=True, warmup_prefix_frames=7, end_aligned=True),
    "path_c": dict(mel_chunk_context=False, silence_aligned=False, warmup_prefix_frames=0, end_aligned=True),
}


def chunk_layout(cfg: Config):
    """(chunkSamples, strideSamples, melContextSamples, warmupPrefixSamples)"""
    f = cfg.frame_samples
    mel_context = f if cfg.mel_chunk_context else 0                                      # :34, :48-50
    warmup = 0 if cfg.mel_chunk_context else cfg.warmup_prefix_frames * f                # :43-45, :52-55
    raw = max(cfg.max_model_samples - mel_context - cfg.mel_hop, f)                      # :59-64
    chunk = raw // f * f
    requested = int(cfg.overlap_seconds * float(cfg.sample_rate))                        # :66-70
    overlap = min(requested, chunk // 2) // f * f
    stride = max(chunk - overlap, f) // f * f                                            # :72-75
    return chunk, stride, mel_context, warmup


def last_chunk_warmup_samples(chunk_start, default_warmup, chunk_samples, total, speech_end, frame_samples=1280):
    default_visible = max(frame_samples, chunk_samples - default_warmup)                 # :93
    is_last = chunk_start + default_visible >= total
    remaining = min(speech_end, total) - chunk_start
    if not (is_last and remaining > 0 and chunk_start > 0):                              # :96
        return default_warmup
    fill = (chunk_samples - remaining) // frame_samples * frame_samples
    if not fill > 0:
        return default_warmup
    available = chunk_start // frame_samples * frame_samples
    BRANCHES["backfill"] += 1
    return max(default_warmup, min(available, fill))


def calculate_encoder_frames(samples, frame_samples=1280):
    return int(math.ceil(float(samples) / float(frame_samples)))                         # ASRConstants.swift:71-73


def window_count_bound(cfg: Config, samples: int) -> int:
    """The list of starts holds 1 + (n - 1) / stride entries, strictly ascending and below n.  Regular starts: the list is every multiple
    of the stride below n, so stepping beyond it ends the loop.  Silence-aligned ones: the steps beyond the list advance by the stride
    from a start >= 0 and stay below n, at most (n - 1) / stride of them."""
    if samples <= 0:
        return 0
    _, stride, _, warmup = chunk_layout(cfg)
    listed = 1 + (samples - 1) // stride
    return listed if not (cfg.silence_aligned or warmup > 0) else listed + (samples - 1) // stride


def adaptive_threshold(reference_rms, floor=SPEECH_RMS_FLOOR, ceiling=SPEECH_RMS_CEILING):
    """min(ceiling, max(floor, referenceRms * speechRmsReferenceScale)) :1245-1247"""
    return min(F32(ceiling), max(F32(floor), F32(F32(reference_rms) * SPEECH_RMS_REFERENCE_SCALE)))


class Planner:
    def __init__(self, samples, cfg: Config | None = None):
        self.x = np.ascontiguousarray(samples, np.float32)
        self.total = int(self.x.size)
        self.cfg = cfg or Config()
        self.f = self.cfg.frame_samples
        self._scores = {}

    def sum_squares(self, offset, count):
        x = self.x[offset:offset + count]
        assert x.size == count and count > 0
        with np.errstate(over="ignore", invalid="ignore"):
            return np.cumsum(x * x, dtype=np.float32)[-1]

    def refused(self) -> bool:
        if self.total == 0:
            return False
        for f in range((self.total - 1) // self.f + 2):
            start, end = max(0, f * self.f - self.f), min(self.total, f * self.f + self.f)
            if end > start and not np.isfinite(self.sum_squares(start, end - start)):
                return True
        return False

    def speech_end_samples(self) -> int:                                                 # :112-128
        end = self.total
        while end > 0:
            frame_start = max(0, end - self.f)
            s = self.sum_squares(frame_start, end - frame_start)
            if np.sqrt(s / F32(end - frame_start)) >= SPEECH_RMS_FLOOR:
                return end
            end = frame_start
        return self.total

    def boundary_energy_score(self, center, half):                                       # :384-396
        key = (center, half)
        if key not in self._scores:
            start, end = max(0, center - half), min(self.total, center + half)
            count = end - start
            self._scores[key] = F32(0) if not count > 0 else self.sum_squares(start, count) / F32(count)
        return self._scores[key]

    def regular_chunk_starts(self, stride):                                              # :179-187
        starts, start = [(0, False)], stride
        while start < self.total:
            starts.append((start, False))
            start += stride
        return starts

    def best_boundary_candidate(self, target_frame, radius, previous_start, latest_covered_start, half):   # :270-310
        f = self.f
        lower, upper = max(1, target_frame - radius), min((self.total - 1) // f, target_frame + radius)
        target_start = min(max(target_frame * f, previous_start + f), latest_covered_start)
        best_start, best_score, scores = target_start, GREATEST_FINITE, []
        for frame in range(lower, upper + 1):
            candidate = frame * f
            if candidate <= previous_start or candidate > latest_covered_start:
                continue
            score = self.boundary_energy_score(candidate, half)
            scores.append(score)
            if score < best_score:
                best_score, best_start = score, candidate
        if not scores:
            BRANCHES["empty_candidates"] += 1
            return target_start, GREATEST_FINITE, F32(0)
        return best_start, best_score, sorted(scores)[len(scores) // 2]

    @staticmethod
    def adaptive_boundary_threshold(median, ratio):                                      # :320-323
        return F32(0) if not median > 0 else F32(median * F32(ratio))

    def would_compress_speech_tail(self, candidate_start, target_start, chunk, minimum_overlap, median, half):   # :325-348
        if not median > 0:
            return False
        forced = candidate_start + chunk - minimum_overlap
        if not forced < self.total:
            BRANCHES["tail_eof_guard"] += 1
            return False
        speech_like = F32(median * F32(0.8))
        return bool(self.boundary_energy_score(target_start, half) > speech_like and self.boundary_energy_score(forced, half) > speech_like)

    def should_use_warmup_prefix(self, center) -> bool:                                  # :350-382
        rate = self.cfg.sample_rate
        lookahead, minimum_stable_quiet, window = int(0.5 * float(rate)), int(0.2 * float(rate)), max(1, rate // 50)
        offset = quiet = 0
        while offset < lookahead:
            start = center + offset
            if not start < self.total:
                BRANCHES["probe_end_of_audio"] += 1
                break
            count = min(window, self.total - start, lookahead - offset)
            if not count > 0:
                break
            rms = np.sqrt(self.sum_squares(start, count) / F32(count))
            if not rms < F32(0.003):
                BRANCHES["probe_loud"] += 1
                break
            quiet += count
            if quiet >= minimum_stable_quiet:
                BRANCHES["probe_stable_quiet"] += 1
                return False
            offset += count
        return True

    def silence_aligned_chunk_starts(self, chunk, stride, can_use_warmup):               # :189-268
        f, rate = self.f, self.cfg.sample_rate
        silence_radius = max(1, int((4.0 * float(rate)) / float(f)))
        valley_radius = max(1, int((0.5 * float(rate)) / float(f)))
        half, minimum_overlap = f, f * 6
        starts, previous_start, target = [(0, False)], 0, stride
        while target < self.total:
            target_frame = target // f
            latest = previous_start + chunk - minimum_overlap
            target_start = min(max(target_frame * f, previous_start + f), latest)
            cand = self.best_boundary_candidate(target_frame, silence_radius, previous_start, latest, half)
            use_warmup = False
            if cand[1] <= self.adaptive_boundary_threshold(cand[2], 0.05):
                BRANCHES["near_silence"] += 1
                should_warmup = self.should_use_warmup_prefix(cand[0]) if can_use_warmup else False
                if can_use_warmup:
                    BRANCHES["warmup_true" if should_warmup else "warmup_false"] += 1
                compresses = (self.would_compress_speech_tail(cand[0], target_start, chunk, minimum_overlap, cand[2], half)
                              if should_warmup and cand[0] < target_start else False)
                if compresses:
                    BRANCHES["tail_compression"] += 1
                    best_start = target_start
                else:
                    best_start, use_warmup = cand[0], should_warmup
            else:
                valley = self.best_boundary_candidate(target_frame, valley_radius, previous_start, latest, half)
                if valley[1] <= self.adaptive_boundary_threshold(valley[2], 0.35):
                    BRANCHES["valley"] += 1
                    best_start = valley[0]
                else:
                    BRANCHES["target_fallback"] += 1
                    best_start = target_start
            if best_start <= previous_start:                                             # :253-255
                BRANCHES["repair_best_start"] += 1
                best_start = min(previous_start + stride, self.total)
            starts.append((best_start, use_warmup))
            previous_start = best_start
            target += stride
        return starts

    def chunk_start_decisions(self):                                                     # :163-177
        chunk, stride, _, warmup = chunk_layout(self.cfg)
        if not (self.cfg.silence_aligned or warmup > 0):
            return self.regular_chunk_starts(stride)
        return self.silence_aligned_chunk_starts(chunk, stride, warmup > 0)

    def plan(self):
        """The windows of process, one dict per window; ([], speech_end) for a recording without samples."""
        f, total, cfg = self.f, self.total, self.cfg
        chunk, stride, mel_context, warmup_prefix = chunk_layout(cfg)
        if total == 0:
            return [], 0
        starts = self.chunk_start_decisions()
        chunk_start, use_warmup = starts[0]
        chunk_index = 0
        speech_end = self.speech_end_samples() if cfg.end_aligned else total             # :507
        out = []
        while chunk_start < total:                                                       # :520
            default_warmup = min(warmup_prefix, chunk_start) if chunk_index > 0 and use_warmup else 0
            warmup = (last_chunk_warmup_samples(chunk_start, default_warmup, chunk, total, speech_end, f) if cfg.end_aligned else default_warmup)
            visible = max(f, chunk - warmup)
            candidate_end = chunk_start + visible
            is_last = candidate_end >= total
            chunk_end = total if is_last else candidate_end
            if chunk_end <= chunk_start:
                BRANCHES["chunk_end_le_start"] += 1
                break
            audio_end = min(chunk_end, speech_end) if is_last and cfg.end_aligned else chunk_end
            if audio_end <= chunk_start:
                BRANCHES["pure_silence_tail"] += 1
                break
            context = 0 if warmup > 0 else (mel_context if chunk_index > 0 else 0)       # :560
            context_start = chunk_start - max(warmup, context)
            length = audio_end - context_start
            emit_after = chunk_start // f if warmup > 0 else -1
            offset = context_start if warmup > 0 else chunk_start                        # :577
            out.append(dict(chunk_start=chunk_start, use_warmup_prefix=int(use_warmup), warmup_samples=warmup, context_samples=context,
                            context_start=context_start, length=length, is_last=int(is_last), emit_after_frame=emit_after,
                            global_frame_offset=offset // f, context_frames=context // f,
                            actual_audio_frames=calculate_encoder_frames(length - context, f)))
            chunk_index += 1
            if is_last:
                break
            if chunk_index < len(starts):                                                # :630-636
                chunk_start, use_warmup = starts[chunk_index]
            else:
                chunk_start, use_warmup = chunk_start + stride, False
                if chunk_start < total:                                                  # the step leads to a further turn of the loop
                    BRANCHES["step_beyond_list"] += 1
        return out, speech_end

    # ---- the half of the seam-gap repair that reads audio
    def adaptive_speech_rms_threshold(self):                                             # :1245-1276
        f, rms, offset = self.f, [], 0
        while offset + f <= self.total:
            s = self.sum_squares(offset, f)
            if s > 0:
                rms.append(np.sqrt(s / F32(f)))
            offset += f
        if not rms:
            return SPEECH_RMS_CEILING
        rms.sort()
        reference = rms[min(len(rms) - 1, int(float(len(rms)) * SPEECH_RMS_REFERENCE_PERCENTILE))]
        return adaptive_threshold(reference)

    def speech_like_frames(self, start, end, threshold):                                 # :1518-1532
        frames, offset = 0, start
        while offset + self.f <= end:
            if np.sqrt(self.sum_squares(offset, self.f) / F32(self.f)) > F32(threshold):
                frames += 1
            offset += self.f
        return frames

    def speech_like_seconds(self, start, end, threshold=None):                           # :1533
        threshold = self.adaptive_speech_rms_threshold() if threshold is None else threshold
        return float(self.speech_like_frames(start, end, threshold)) * (float(self.f) / float(self.cfg.sample_rate))


def pack_rows(samples, windows, max_model_samples=240000):
    """padAudioIfNeeded: the window's samples as bits, zeros behind them."""
    x = np.ascontiguousarray(samples, np.float32).view(np.uint32)
    rows = np.zeros((len(windows), max_model_samples), np.uint32)
    for i, w in enumerate(windows):
        rows[i, :w["length"]] = x[w["context_start"]:w["context_start"] + w["length"]]
    return rows.view(np.float32), np.array([w["length"] for w in windows], np.int32)
