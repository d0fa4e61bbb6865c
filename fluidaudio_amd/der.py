"""Frame-wise diarization error rate with the optimal speaker mapping (csrc/der.hip, csrc/der_host.hip): DiarizationDER.compute (reference:
Sources/FluidAudio/Diarizer/DiarizationDER.swift:52-231, Diarizer/HungarianAssignment.swift:8-61), batched over recordings — the
score the reference's Sortformer and LS-EEND benchmarks print (Sources/FluidAudioCLI/Commands/SortformerBenchmark.swift:622-640).

The strings are numbered here, by first appearance; the device counts frames; the seconds and the rate are formed here with the
reference's expressions.  A side of a recording holds at most MAX_LABELS speakers."""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass, field

import numpy as np

from . import _args as A, _lib as L

MAX_LABELS = 64
DER_SEGMENT_DTYPE, DER_COUNTS_DTYPE = np.dtype(L.DerSegment), np.dtype(L.DerCounts)


@dataclass(frozen=True)
class DERSpeakerSegment:   # DERSpeakerSegment (:26-35)
    speaker: str
    start: float
    end: float


@dataclass
class DERResult:   # DERResult (:37-46), and the integers behind it
    der: float
    confusion: float
    false_alarm: float
    miss: float
    total_ref_speech: float
    mapping: dict                                       # hyp label -> ref label; hyp labels without a partner are left out
    frames: int = 0                                     # numFrames (0: neither side has a label)
    miss_frames: int = 0
    false_alarm_frames: int = 0
    confusion_frames: int = 0
    ref_frames: int = 0
    ref_labels: list = field(default_factory=list)      # by first appearance
    hyp_labels: list = field(default_factory=list)
    index_mapping: list = field(default_factory=list)   # hyp index -> ref index or -1
    overlap: np.ndarray | None = None                   # int64 [H, R]: frames both are active in, counted before the collar


def segments_from_timed(segments) -> list:
    """TimedSpeakerSegment (what RTTMParser.parse returns) -> DERSpeakerSegment: Double(Float) widening, as SortformerBenchmark.swift:622-628."""
    return [DERSpeakerSegment(s.speaker_id, float(np.float32(s.start_time_seconds)), float(np.float32(s.end_time_seconds))) for s in segments]


def segments_from_timeline(records, frame_duration_seconds) -> list:
    """The timeline's segment records of ONE recording (timeline_segments' structured array, or [DiarizerSegment]) -> DERSpeakerSegment, per
    segmentsToDERSegments (SortformerBenchmark.swift:735-747): start = Double(Float(startFrame) * frameDuration), likewise the end; the
    label is the speaker index, spelled as DiarizerSegment.speakerLabel spells it."""
    f = np.float32
    fd = f(frame_duration_seconds)
    out = []
    for r in records:
        if isinstance(r, np.void):
            spk, a, b = int(r["speaker"]), int(r["start_frame"]), int(r["end_frame"])
        else:
            spk, a, b = r.speaker_index, r.start_frame, r.end_frame
        out.append(DERSpeakerSegment(f"Speaker {spk}", float(f(f(a) * fd)), float(f(f(b) * fd))))
    return out


def index_labels(segments):
    """(labels by first appearance, structured array of DER_SEGMENT_DTYPE) of one side of one recording (:61-80)."""
    labels, idx = [], {}
    for s in segments:
        if s.speaker not in idx:
            idx[s.speaker] = len(labels)
            labels.append(s.speaker)
    arr = np.zeros(len(segments), DER_SEGMENT_DTYPE)
    arr["label"] = [idx[s.speaker] for s in segments]
    arr["start"] = [float(s.start) for s in segments]
    arr["end"] = [float(s.end) for s in segments]
    return labels, arr


_invalid = functools.partial(A.invalid, "compute_der")


def _check(frame_step, collar, sides):
    """The argument contract of fa_der_score_batch, answered here as well so that it needs no device: Swift traps where this raises."""
    if not (np.isfinite(frame_step) and frame_step > 0):
        raise _invalid("frame_step must be positive and finite")
    if not (np.isfinite(collar) and collar >= 0):
        raise _invalid("collar must be non-negative and finite")
    for labels, arr in sides:
        if len(labels) > MAX_LABELS:
            raise _invalid(f"{len(labels)} labels on one side of a recording; at most {MAX_LABELS} are supported")
        if not (np.isfinite(arr["start"]).all() and np.isfinite(arr["end"]).all()):
            raise _invalid("a segment has a non-finite time")


def compute_der_batch(pairs, frame_step: float = 0.01, collar: float = 0.0, ctx: L.Context | None = None) -> list:
    """DiarizationDER.compute for every (ref, hyp) pair of segment lists, in one device call.  Returns [DERResult]."""
    frame_step, collar = float(frame_step), float(collar)
    sides = [(index_labels(ref), index_labels(hyp)) for ref, hyp in pairs]
    _check(frame_step, collar, [s for pair in sides for s in pair])
    n = len(sides)
    if n == 0:
        return []
    ctx = ctx or L.default_context()
    ref, ref_range = A.ragged([r[1] for r, _ in sides], None, DER_SEGMENT_DTYPE)
    hyp, hyp_range = A.ragged([h[1] for _, h in sides], None, DER_SEGMENT_DTYPE)
    map_range = np.concatenate([[0], np.cumsum([len(h[0]) for _, h in sides])]).astype(np.int64)
    ov_range = np.concatenate([[0], np.cumsum([len(h[0]) * len(r[0]) for r, h in sides])]).astype(np.int64)
    counts = np.zeros(n, DER_COUNTS_DTYPE)
    mapping = np.full(max(int(map_range[-1]), 1), -1, np.int32)
    overlap = np.zeros(max(int(ov_range[-1]), 1), np.int64)
    cfg = L.DerConfig(frame_step, collar)
    ctx.check(L.lib().fa_der_score_batch(ctx.handle, C.byref(cfg), ref.ctypes.data, ref_range.ctypes.data, hyp.ctypes.data, hyp_range.ctypes.data, n,
                                         counts.ctypes.data, mapping.ctypes.data, map_range.ctypes.data, overlap.ctypes.data, int(ov_range[-1])),
              "fa_der_score_batch")
    out = []
    for b, ((ref_labels, _), (hyp_labels, _)) in enumerate(sides):
        c = counts[b]
        assert int(c["ref_labels"]) == len(ref_labels) and int(c["hyp_labels"]) == len(hyp_labels)
        m = mapping[map_range[b]:map_range[b + 1]].tolist()
        # :160-164
        miss_s = float(int(c["miss"])) * frame_step
        fa_s = float(int(c["false_alarm"])) * frame_step
        conf_s = float(int(c["confusion"])) * frame_step
        ref_s = float(int(c["ref"])) * frame_step
        der = (miss_s + fa_s + conf_s) / ref_s if ref_s > 0 else 0.0
        out.append(DERResult(der, conf_s, fa_s, miss_s, ref_s, {hyp_labels[h]: ref_labels[r] for h, r in enumerate(m) if r >= 0},
                             int(c["frames"]), int(c["miss"]), int(c["false_alarm"]), int(c["confusion"]), int(c["ref"]), ref_labels, hyp_labels, m,
                             overlap[ov_range[b]:ov_range[b + 1]].reshape(len(hyp_labels), len(ref_labels)).copy()))
    return out


def compute_der(ref, hyp, frame_step: float = 0.01, collar: float = 0.0, ctx: L.Context | None = None) -> DERResult:
    """DiarizationDER.compute(ref:hyp:frameStep:collar:) (:52-175) for one recording."""
    return compute_der_batch([(ref, hyp)], frame_step, collar, ctx)[0]
