"""Speaker segments from the segmentation output and the per-chunk clusters (csrc/reconstruct.hip, csrc/reconstruct_host.hip): the powerset decode of
OfflineSegmentationProcessor (reference: Sources/FluidAudio/Diarizer/Offline/Segmentation/OfflineSegmentationProcessor.swift:316-409)
and OfflineReconstruction.buildSegments / buildSpeakerDatabase (Diarizer/Offline/Utils/OfflineReconstruction.swift:24-357).

The accumulation over global frames, the per-frame speaker selection and the segment walk run on the device; merge / sanitize /
excludeOverlaps run as host code inside the same library call.  Raw segments closing at the same frame are ordered by cluster index
(the reference's Dictionary order is hash-seeded)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _args as A, _lib as L
from .formats import RttmSegment, TimedSpeakerSegment


@dataclass
class ReconstructionConfig:   # OfflineDiarizerTypes.swift:46-55, 97-103, 204-214, 232-247
    window_duration: float = 10.0
    min_duration_on: float = 0.0
    min_duration_off: float = 0.0
    min_segment_duration: float = 1.0
    min_gap_duration: float = 0.1
    exclusive: bool = True
    zero_vote_enabled: bool = False
    zero_vote_min_duration: float = 0.4

    def c_config(self, frame_duration: float = 0.0) -> L.ReconstructConfig:
        c = L.ReconstructConfig()
        L.lib().fa_reconstruct_default_config(C.byref(c))
        c.window_duration, c.frame_duration = float(self.window_duration), float(frame_duration)
        c.min_duration_on, c.min_duration_off = float(self.min_duration_on), float(self.min_duration_off)
        c.min_segment_duration, c.min_gap_duration = float(self.min_segment_duration), float(self.min_gap_duration)
        c.exclusive, c.zero_vote_enabled = int(bool(self.exclusive)), int(bool(self.zero_vote_enabled))
        c.zero_vote_min_duration = float(self.zero_vote_min_duration)
        return c


@dataclass
class SegmentationOutput:
    """SegmentationOutput (OfflineDiarizerTypes.swift:567-594) in dense form: speaker_weights [chunks, frames, speakers] fp32 (numpy,
    or a torch CUDA tensor that stays on the device), chunk_offsets [chunks] seconds (fewer entries: the rest start at index *
    window_duration), frame_duration seconds (0: window_duration / frames), log_probs [chunks, frames, classes] or None."""
    speaker_weights: object
    chunk_offsets: object = None
    frame_duration: float = 0.0
    log_probs: object = None

    @property
    def shape(self):
        return tuple(int(x) for x in self.speaker_weights.shape)


def powerset_decode(logits, chunk_offsets=None, frame_duration: float = 0.0, log_probs: bool = False, window_duration: float = 10.0,
                    ctx: L.Context | None = None) -> SegmentationOutput:
    """logits [chunks, frames, classes] fp32 (numpy / CPU tensor, or a torch CUDA tensor on ctx's device: the result stays there) -> SegmentationOutput with
    binary per-speaker weights [chunks, frames, 3] and, if asked, the log-probabilities.  frame_duration 0 = window_duration / frames
    (OfflineSegmentationProcessor.swift:286)."""
    ctx = ctx or L.default_context()
    x, on_device = A.placed(logits, ctx)
    nc, nf, k = (int(v) for v in x.shape)
    w = A.beside(x, (nc, nf, 3), "float32", torch_empty=True)
    lp = A.beside(x, (nc, nf, k), "float32", torch_empty=True) if log_probs else None
    name = "fa_powerset_decode_dev" if on_device else "fa_powerset_decode"
    with ctx.torch_ordered(on_device):
        ctx.check(getattr(L.lib(), name)(ctx.handle, A.ptr(x), nc, nf, k, A.ptr(w), A.ptr(lp)), name)
    fd = float(frame_duration) if frame_duration > 0 else (window_duration / nf if nf else 0.0)
    return SegmentationOutput(w, chunk_offsets, fd, lp)


def chunk_assignments(chunk_indices, speaker_indices, labels, cluster_count: int, chunks: int, speakers: int) -> np.ndarray:
    """buildChunkAssignments (OfflineDiarizerManager.swift:885-911): int32 [chunks, speakers], -2 where no embedding landed."""
    ci = np.ascontiguousarray(chunk_indices, np.int32)
    si = np.ascontiguousarray(speaker_indices, np.int32)
    lab = np.ascontiguousarray(labels, np.int32)
    if not ci.size == si.size == lab.size:
        raise ValueError(f"chunk_indices ({ci.size}), speaker_indices ({si.size}) and labels ({lab.size}) differ in length")
    n = ci.size
    hard = np.zeros((chunks, speakers), np.int32)
    st = L.lib().fa_offline_chunk_assignments(n, ci.ctypes.data, si.ctypes.data, lab.ctypes.data, int(cluster_count), int(chunks), int(speakers),
                                              hard.ctypes.data)
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_offline_chunk_assignments")
    return hard


def _segments(arr, n) -> list:
    return [TimedSpeakerSegment(s.speaker_id.decode(), float(s.start_seconds), float(s.end_seconds), float(s.quality)) for s in arr[:n]]


def zero_vote_assignment(embedding, centroids):
    """ZeroVoteReembedder.assignment (ZeroVoteReembedder.swift:90-130): the centroid of the best cosine, ties to the lowest index;
    None for an empty / non-finite embedding or empty / mismatched centroids."""
    e = [float(v) for v in embedding] if embedding is not None else []
    if not e or len(centroids) == 0 or not all(np.isfinite(e)):
        return None
    best, best_cos = -1, -np.inf
    for i, c in enumerate(centroids):
        c = [float(v) for v in c]
        if len(c) != len(e):
            return None
        dot = na = nb = 0.0
        for x, y in zip(e, c):
            dot += x * y
            na += x * x
            nb += y * y
        cos = dot / np.sqrt(na * nb) if na * nb > 0 else (np.nan if dot == 0 else np.inf)
        if not np.isfinite(cos):
            return None
        if cos > best_cos:
            best, best_cos = i, cos
    return best if best >= 0 else None


class OfflineReconstruction:
    """OfflineReconstruction (OfflineReconstruction.swift): build_segments on the device, build_speaker_database on the host."""

    def __init__(self, config: ReconstructionConfig | None = None, ctx: L.Context | None = None):
        self.config = config or ReconstructionConfig()
        self.ctx = ctx
        self.last_info: dict = {}

    def _call(self, seg: SegmentationOutput, hard, clusters: int, overrides=None, runs_capacity: int = 0, frame_records: bool = False):
        ctx = self.ctx or L.default_context()
        w, on_device = A.placed(seg.speaker_weights, ctx)
        nc, nf, ns = (int(v) for v in w.shape)
        wptr = A.ptr(w)
        offs = np.ascontiguousarray([] if seg.chunk_offsets is None else seg.chunk_offsets, np.float64)
        hard = np.ascontiguousarray(hard, np.int32).reshape(-1)
        assert hard.size == nc * ns, "hard_clusters must be [chunks, speakers]"
        ov = np.ascontiguousarray(overrides if overrides is not None and len(overrides) else np.zeros((0, 3)), np.int64).reshape(-1, 3)
        cfg = self.config.c_config(seg.frame_duration)
        info = L.ReconstructInfo()
        runs = np.zeros((max(runs_capacity, 1), 2), np.int64)
        if runs_capacity:
            info.zero_vote_runs, info.zero_vote_capacity = runs.ctypes.data, runs_capacity
        cnt = C.c_int64()
        cap = max(4096, self._total_frames(offs, nc, nf, seg.frame_duration) // 8)   # one call in practice; a larger count is asked again
        f = L.lib().fa_offline_reconstruct_dev if on_device else L.lib().fa_offline_reconstruct
        name = "fa_offline_reconstruct_dev" if on_device else "fa_offline_reconstruct"
        for attempt in range(2):
            out = (RttmSegment * cap)()
            count_buf = None
            if frame_records:
                tf = max(self._total_frames(offs, nc, nf, seg.frame_duration), 1)
                slots = max(min(max(int(clusters), 1), ns), 1)
                count_buf, esum = np.zeros(tf, np.int32), np.zeros(tf)
                fcl, favg = np.zeros((tf, slots), np.int32), np.zeros((tf, slots))
                info.speaker_counts, info.speaker_counts_capacity = count_buf.ctypes.data, count_buf.size
                info.frame_capacity, info.frame_clusters, info.frame_averages = tf, fcl.ctypes.data, favg.ctypes.data
                info.expected_count_sums = esum.ctypes.data
            with ctx.torch_ordered(on_device):
                st = f(ctx.handle, C.byref(cfg), wptr, nc, nf, ns, offs.ctypes.data if offs.size else None, offs.size, hard.ctypes.data,
                       int(clusters), ov.ctypes.data if ov.size else None, ov.shape[0], out, cap, C.byref(cnt), C.byref(info))
            if st == L.OUTPUT_TOO_SMALL and attempt == 0:
                cap = int(cnt.value)
                continue
            ctx.check(st, name)
            break
        self.last_info = {"total_frames": info.total_frames, "raw_segments": info.raw_segments, "frame_duration": info.frame_duration,
                          "zero_vote_runs": [tuple(r) for r in runs[:min(info.zero_vote_run_count, runs_capacity)].tolist()] if runs_capacity else []}
        if frame_records:
            t = info.total_frames
            self.last_info.update(speaker_counts=count_buf[:t], frame_clusters=fcl[:t], frame_averages=favg[:t], expected_count_sums=esum[:t])
        return _segments(out, cnt.value)

    def _total_frames(self, offs, nc, nf, frame_duration):
        """totalFrames (OfflineReconstruction.swift:37-47): a bound for the caller's buffers (the library computes its own)."""
        fd = frame_duration if frame_duration > 0 else (self.config.window_duration / nf if nf else 0.0)
        if not fd > 0 or nc == 0:
            return 1
        starts = np.arange(nc, dtype=np.float64) * self.config.window_duration
        starts[:min(offs.size, nc)] = offs[:nc]
        max_time = max(0.0, float((starts + float(nf) * fd).max()))
        return max(1, int(np.ceil(max_time / fd))) + 1

    def build_segments(self, segmentation: SegmentationOutput, hard_clusters, centroids, span_embedder=None, frame_records: bool = False) -> list:
        """buildSegments (:24-237) -> [TimedSpeakerSegment].  hard_clusters [chunks, speakers] (chunk_assignments); centroids [K, d]
        (K = len(centroids)).  With config.zero_vote_enabled, a span_embedder(start_s, end_s) -> embedding or None and centroids, the
        zero-vote runs are re-embedded and assigned to the best-cosine centroid (:176-186, :249-298): one call finds the runs, a second
        one applies the assignments.  frame_records: last_info also gets the per-frame decision (speaker_counts, frame_clusters,
        frame_averages, expected_count_sums; verification)."""
        k = len(centroids)
        zero_vote = self.config.zero_vote_enabled and span_embedder is not None and k > 0
        nc, nf = segmentation.shape[0], segmentation.shape[1]
        offs = np.ascontiguousarray([] if segmentation.chunk_offsets is None else segmentation.chunk_offsets, np.float64)
        runs_cap = self._total_frames(offs, nc, nf, segmentation.frame_duration) // 2 + 1 if zero_vote else 0
        segs = self._call(segmentation, hard_clusters, k, None, runs_cap, frame_records)
        if not zero_vote or not self.last_info["zero_vote_runs"]:
            return segs
        fd = self.last_info["frame_duration"]
        overrides = []
        for lo, hi in self.last_info["zero_vote_runs"]:
            emb = span_embedder(float(lo) * fd, float(hi) * fd)
            a = zero_vote_assignment(emb, centroids) if emb is not None else None
            if a is not None:
                overrides.append((lo, hi, a))
        if not overrides:
            return segs
        runs = self.last_info["zero_vote_runs"]
        segs = self._call(segmentation, hard_clusters, k, overrides, 0, frame_records)
        self.last_info["zero_vote_runs"] = runs
        return segs

    @staticmethod
    def build_speaker_database(segments, centroids) -> dict:
        """buildSpeakerDatabase (:300-357): per speaker id, the fp32 sum of its segments' Float(centroid) in segment order times
        1 / Float(count).  A segment's embedding is the centroid of its cluster (zeros past the end, :415-419)."""
        cen = np.asarray(centroids, np.float64)
        dim = cen.shape[1] if cen.ndim == 2 and cen.shape[0] else 0
        sums, counts = {}, {}
        for s in segments:
            k = int(s.speaker_id[1:]) - 1
            e = cen[k].astype(np.float32) if 0 <= k < cen.shape[0] else np.zeros(dim, np.float32)
            sums[s.speaker_id] = e.copy() if s.speaker_id not in sums else (sums[s.speaker_id] + e).astype(np.float32)
            counts[s.speaker_id] = counts.get(s.speaker_id, 0) + 1
        return {spk: (v * (np.float32(1) / np.float32(counts[spk]))).astype(np.float32) for spk, v in sums.items()}


def finalize_segments(raw_segments, config: ReconstructionConfig | None = None) -> list:
    """mergeSegments -> sanitize (-> excludeOverlaps) over raw segments in their raw order (fa_segments_finalize, host code)."""
    cfg = (config or ReconstructionConfig()).c_config()
    n = len(raw_segments)
    arr = (RttmSegment * max(n, 1))()
    for i, s in enumerate(raw_segments):
        arr[i].start_seconds, arr[i].end_seconds, arr[i].quality = s.start_time_seconds, s.end_time_seconds, s.quality_score
        arr[i].speaker_id = s.speaker_id.encode()[:63]
    out = (RttmSegment * max(n, 1))()
    cnt = C.c_int64()
    st = L.lib().fa_segments_finalize(C.byref(cfg), arr, n, out, max(n, 1), C.byref(cnt))
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_segments_finalize")
    return _segments(out, cnt.value)
