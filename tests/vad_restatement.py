"""The four VAD routines of the reference, line by line (Sources/FluidAudio/VAD): segmentSpeech(from:totalSamples:config:) with
detectSpeechSampleRanges (VadManager+SpeechSegmentation.swift:22-51, 71-234), the model rows of processAudioSamples / processChunk
(VadManager.swift:162-206, 352-376), the sample bounds of segmentSpeechAudio (:55-67) and streamingStateMachine with makeStreamEvent
(VadManager+Streaming.swift:31-107).  fp32 goes through np.float32, integers are Python ints, times are Python floats (fp64).  BRANCHES
counts how often each branch of the segmentation was taken: the GPU test asserts that its inputs reach every one of them."""
import collections
import math

import numpy as np

CHUNK, CONTEXT, RATE = 4096, 64, 16000
ROW = CONTEXT + CHUNK
F = np.float32
BRANCH_NAMES = ("speech_end", "short_speech_dropped", "candidate_recorded", "split_below_threshold", "split_longest", "split_last", "hard_cut",
                "resumed", "not_resumed", "tail_flush", "half_padding", "empty_flush", "dropped_by_clamp")
BRANCHES = collections.Counter()


class Config:
    """VadSegmentationConfig (VadTypes.swift:24-81) with VadConfig.defaultThreshold (:6) beside it."""

    def __init__(self, minSpeechDuration=0.15, minSilenceDuration=0.75, maxSpeechDuration=14.0, speechPadding=0.1, silenceThresholdForSplit=0.3,
                 negativeThreshold=None, negativeThresholdOffset=0.15, minSilenceAtMaxSpeech=0.098, useMaxPossibleSilenceAtMaxSpeech=True,
                 defaultThreshold=0.85):
        assert minSpeechDuration >= 0 and minSilenceDuration >= 0 and maxSpeechDuration > 0 and speechPadding >= 0
        assert 0 <= silenceThresholdForSplit <= 1 and negativeThresholdOffset >= 0 and minSilenceAtMaxSpeech >= 0
        assert negativeThreshold is None or 0 <= negativeThreshold <= 1
        self.minSpeechDuration, self.minSilenceDuration, self.maxSpeechDuration = float(minSpeechDuration), float(minSilenceDuration), float(maxSpeechDuration)
        self.speechPadding, self.minSilenceAtMaxSpeech = float(speechPadding), float(minSilenceAtMaxSpeech)
        self.silenceThresholdForSplit, self.negativeThresholdOffset = F(silenceThresholdForSplit), F(negativeThresholdOffset)
        self.negativeThreshold = None if negativeThreshold is None else F(negativeThreshold)
        self.useMaxPossibleSilenceAtMaxSpeech = bool(useMaxPossibleSilenceAtMaxSpeech)
        self.defaultThreshold = F(defaultThreshold)


def swift_int(x: float) -> int:
    """Int(_: Double): truncates; traps on NaN, infinities and values outside Int."""
    if math.isnan(x) or math.isinf(x) or not -2.0 ** 63 <= x < 2.0 ** 63:
        raise OverflowError(x)
    return int(x)


def thresholds(cfg: Config):
    """(threshold, negativeThreshold) of :31-35 and effectiveNegativeThreshold (VadTypes.swift:85-90), in fp32."""
    if cfg.negativeThreshold is not None:
        return min(F(1.0), F(cfg.negativeThreshold + cfg.negativeThresholdOffset)), cfg.negativeThreshold
    threshold = cfg.defaultThreshold
    return threshold, max(F(threshold - cfg.negativeThresholdOffset), F(0.01))


def sample_counts(cfg: Config) -> dict:
    """:85-99.  maxSpeech None stands for Int.max."""
    pad = swift_int(cfg.speechPadding * float(RATE))
    if math.isinf(cfg.maxSpeechDuration):
        max_speech = None
    else:
        max_speech = max(0, swift_int(cfg.maxSpeechDuration * float(RATE)) - CHUNK - 2 * pad)
    return dict(minSpeech=swift_int(cfg.minSpeechDuration * float(RATE)), pad=pad, maxSpeech=max_speech,
                minSilence=swift_int(cfg.minSilenceDuration * float(RATE)), minSilenceAtMaxSpeech=swift_int(cfg.minSilenceAtMaxSpeech * float(RATE)))


def raw_speeches(probabilities, audioLengthSamples: int, threshold, cfg: Config, flush_log=None):
    """:102-201: the state machine, before the padding.  flush_log (a list) receives the frame index of every call of
    flushCurrentSpeechEnd, len(probabilities) for the one behind the loop."""
    c = sample_counts(cfg)
    minSpeech, maxSpeech, minSilence, minSilenceAtMax = c["minSpeech"], c["maxSpeech"], c["minSilence"], c["minSilenceAtMaxSpeech"]
    negativeThreshold = thresholds(cfg)[1]
    triggered, currentSpeechStart, tempEnd, tempSilenceMinProb = False, 0, None, None
    possibleEnds, speeches = [], []

    index = 0

    def flush(endSample):
        if flush_log is not None:
            flush_log.append(index)
        if not endSample > currentSpeechStart:
            BRANCHES["empty_flush"] += 1
            return
        if endSample - currentSpeechStart >= minSpeech:
            speeches.append((currentSpeechStart, min(endSample, audioLengthSamples)))
        else:
            BRANCHES["short_speech_dropped"] += 1

    for index, prob in enumerate(probabilities):
        prob = F(prob)
        frameStart = index * CHUNK
        if prob >= threshold:
            if tempEnd is not None:
                silenceDuration = frameStart - tempEnd
                if silenceDuration > minSilenceAtMax:
                    possibleEnds.append((tempEnd, silenceDuration, F(1.0) if tempSilenceMinProb is None else tempSilenceMinProb))
                    BRANCHES["candidate_recorded"] += 1
            tempEnd = tempSilenceMinProb = None
            if not triggered:
                triggered, currentSpeechStart = True, frameStart
                continue
        if triggered and maxSpeech is not None:
            if frameStart - currentSpeechStart > maxSpeech:
                chosen = None
                if possibleEnds:
                    below = [p for p in possibleEnds if p[2] <= cfg.silenceThresholdForSplit]
                    if below:
                        chosen = first_max(below)
                        BRANCHES["split_below_threshold"] += 1
                    elif cfg.useMaxPossibleSilenceAtMaxSpeech:
                        chosen = first_max(possibleEnds)
                        BRANCHES["split_longest"] += 1
                    else:
                        chosen = possibleEnds[-1]
                        BRANCHES["split_last"] += 1
                else:
                    BRANCHES["hard_cut"] += 1
                flush(chosen[0] if chosen else frameStart)
                if chosen:
                    newStart = chosen[0] + chosen[1]
                    if newStart < frameStart:
                        currentSpeechStart, triggered = newStart, True
                        BRANCHES["resumed"] += 1
                    else:
                        triggered = False
                        BRANCHES["not_resumed"] += 1
                else:
                    triggered = False
                possibleEnds = []
                tempEnd = tempSilenceMinProb = None
                if not triggered:
                    continue
        if prob < negativeThreshold and triggered:
            if tempEnd is None:
                tempEnd = frameStart
            tempSilenceMinProb = prob if tempSilenceMinProb is None or prob < tempSilenceMinProb else tempSilenceMinProb
            if frameStart - tempEnd >= minSilence:
                flush(tempEnd)
                BRANCHES["speech_end"] += 1
                triggered, tempEnd, tempSilenceMinProb, possibleEnds = False, None, None, []
                continue
    if triggered:
        index = len(probabilities)
        BRANCHES["tail_flush"] += 1
        flush(audioLengthSamples)
    return speeches


def first_max(candidates):
    """Sequence.max(by: { $0.duration < $1.duration }): the result is replaced only by a strictly longer element, so the FIRST of equal
    maxima is kept."""
    best = candidates[0]
    for c in candidates[1:]:
        if best[1] < c[1]:
            best = c
    return best


def detect_speech_sample_ranges(probabilities, audioLengthSamples: int, threshold, cfg: Config):
    """:71-234"""
    if len(probabilities) == 0:
        return []
    speeches = raw_speeches(probabilities, audioLengthSamples, threshold, cfg)
    if not speeches:
        return []
    pad = sample_counts(cfg)["pad"]
    adjusted = [list(s) for s in speeches]
    for index in range(len(adjusted)):
        if index == 0:
            adjusted[index][0] = max(0, adjusted[index][0] - pad)
        if index < len(adjusted) - 1:
            silence = adjusted[index + 1][0] - adjusted[index][1]
            if silence < 2 * pad:
                half = int(silence / 2) if silence < 0 else silence // 2          # Int division truncates
                adjusted[index][1] = min(audioLengthSamples, adjusted[index][1] + half)
                adjusted[index + 1][0] = max(0, adjusted[index + 1][0] - half)
                BRANCHES["half_padding"] += 1
            else:
                adjusted[index][1] = min(audioLengthSamples, adjusted[index][1] + pad)
                adjusted[index + 1][0] = max(0, adjusted[index + 1][0] - pad)
        else:
            adjusted[index][1] = min(audioLengthSamples, adjusted[index][1] + pad)
    out = []
    for s, e in adjusted:
        start = max(0, min(s, audioLengthSamples))
        end = max(start, min(e, audioLengthSamples))
        if end > start:
            out.append((start, end))
        else:
            BRANCHES["dropped_by_clamp"] += 1
    return out


def segment_speech(probabilities, totalSamples: int, cfg: Config = None):
    """:22-51.  Returns [(start_sample, end_sample, startTime, endTime)]: the samples are what the times are formed from."""
    cfg = cfg or Config()
    if len(probabilities) == 0 or not totalSamples > 0:
        return []
    threshold = thresholds(cfg)[0]
    out = []
    for s, e in detect_speech_sample_ranges(probabilities, totalSamples, threshold, cfg):
        start = max(0, min(s, totalSamples))
        end = max(start, min(e, totalSamples))
        out.append((start, end, float(start) / float(RATE), float(end) / float(RATE)))
    return out


def chunk_count(n: int) -> int:
    return -(-n // CHUNK) if n > 0 else 0


def pack_chunks(samples) -> np.ndarray:
    """The model's audio_input rows of processAudioSamples (:352-376): chunk k of up to 4096 samples, filled with its last sample
    (processChunk :172-182), behind the last 64 samples of the padded chunk k - 1 (:184; zeros in front of the first chunk).  Bits are
    kept: the rows are built on uint32 views."""
    bits = np.ascontiguousarray(samples, np.float32).view(np.uint32)
    rows = np.zeros((chunk_count(bits.size), ROW), np.uint32)
    context = np.zeros(CONTEXT, np.uint32)
    for k in range(rows.shape[0]):
        chunk = bits[k * CHUNK:(k + 1) * CHUNK]
        if chunk.size < CHUNK:
            chunk = np.concatenate([chunk, np.full(CHUNK - chunk.size, chunk[-1], np.uint32)])
        rows[k, :CONTEXT], rows[k, CONTEXT:] = context, chunk
        context = chunk[-CONTEXT:]
    return rows.view(np.float32)


def segment_bounds(startTime: float, endTime: float, n: int):
    """segmentSpeechAudio :61-64: VadSegment.startSample / endSample (VadTypes.swift:145-151) go through fp64 seconds."""
    startSample, endSample = swift_int(startTime * float(RATE)), swift_int(endTime * float(RATE))
    clampedStart = max(0, min(startSample, n))
    return clampedStart, max(clampedStart, min(endSample, n))


def swift_rounded(x: float) -> float:
    """Double.rounded(): to nearest, halves away from zero."""
    return math.copysign(math.floor(abs(x) + 0.5), x) if abs(x) < 2.0 ** 52 else x


class StreamState:
    """VadStreamState (VadTypes.swift:166-187) without the model's state."""

    def __init__(self, triggered=False, tempEndSample=None, processedSamples=0):
        self.triggered, self.tempEndSample, self.processedSamples = triggered, tempEndSample, processedSamples

    def key(self):
        return (int(self.triggered), int(self.tempEndSample is not None), self.tempEndSample or 0, self.processedSamples)


START, END = 0, 1


def stream_step(probability, chunkSampleCount: int, state: StreamState, cfg: Config, returnSeconds=False, timeResolution=1):
    """streamingStateMachine (:31-91).  Returns (nextState, event): event None or (kind, sampleIndex, time or None)."""
    probability = F(probability)
    nxt = StreamState(state.triggered, state.tempEndSample, state.processedSamples + chunkSampleCount)
    threshold, negativeThreshold = thresholds(cfg)
    pad = swift_int(cfg.speechPadding * float(RATE))
    minSilence = swift_int(cfg.minSilenceDuration * float(RATE))

    def make(kind, sampleIndex):
        clamped = max(0, sampleIndex)
        if not returnSeconds:
            return (kind, clamped, None)
        seconds = float(clamped) / float(RATE)
        factor = math.pow(10.0, float(timeResolution))
        return (kind, clamped, swift_rounded(seconds * factor) / factor)

    event = None
    if probability >= threshold:
        nxt.tempEndSample = None
        if not nxt.triggered:
            nxt.triggered = True
            event = make(START, max(0, nxt.processedSamples - pad - chunkSampleCount))
    elif probability < negativeThreshold and nxt.triggered:
        if nxt.tempEndSample is None:
            nxt.tempEndSample = nxt.processedSamples
        silenceStart = nxt.tempEndSample
        if nxt.processedSamples - silenceStart >= minSilence:
            nxt.triggered, nxt.tempEndSample = False, None
            event = make(END, max(0, silenceStart + pad - chunkSampleCount))
    return nxt, event


def make_vad_results(pattern):
    """makeVadResults (Tests/FluidAudioTests/TestHelpers/VadTestHelpers.swift:7-57): 0.95 / 0.05 per chunk of 256 ms."""
    probs = []
    for active, seconds in pattern:
        chunks = max(0, int(swift_rounded(seconds / (CHUNK / float(RATE)))))
        probs += [F(0.95) if active else F(0.05)] * chunks
    return np.array(probs, np.float32), len(probs) * CHUNK
