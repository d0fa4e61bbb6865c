"""The online diarizer's speaker database (reference: Sources/FluidAudio/Diarizer/Clustering/SpeakerManager.swift:135-212, 282-328,
411-492, 552-628, SpeakerTypes.swift:36-162, 213-217, SpeakerOperations.swift:62-126) as device-resident state batched over streams, over
the HIP C ABI (csrc/online.hip, csrc/online_host.hip, csrc/speaker_db_core.h).  One stream is one SpeakerManager.

Ids are ints counting from 1 per stream (0: none), dates are caller-supplied integer ticks, and the fp32 arithmetic is the library's own
definition (include/fluidaudio_hip.h: dot256); names and non-numeric ids stay with the caller.

chunk_plan, pack_waveforms and chunk_finish are the host work of DiarizerManager.processChunkWithSpeakerTracking (Core/DiarizerManager.swift:
255-531) and EmbeddingExtractor.getEmbeddings (Extraction/EmbeddingExtractor.swift:60-199) around the two networks, batched over streams."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _args as A, _lib as L

EMBEDDING_SIZE = 256   # SpeakerManager.embeddingSize
SPEAKER_KINDS = ("SKIPPED", "UPDATED", "DURATION_ONLY", "LOW_ENERGY", "CREATED", "TOO_SHORT", "INVALID", "FULL")   # FA_SPEAKER_*
SPEAKER_ASSIGNMENT_DTYPE, SPEAKER_PAIR_DTYPE = np.dtype(L.SpeakerAssignment), np.dtype(L.SpeakerPair)


@dataclass
class SpeakerDbConfig:  # fa_speaker_db_config
    speaker_threshold: float = 0.65
    embedding_threshold: float = 0.45
    min_speech_duration: float = 1.0
    ema_alpha: float = 0.9
    validate_min_magnitude: float = -1.0   # negative: plain SpeakerManager; 0.1: DiarizerManager's validateEmbedding
    max_speakers: int = 16
    raw_capacity: int = 50

    def c(self) -> L.SpeakerDbConfig:
        return L.SpeakerDbConfig(float(self.speaker_threshold), float(self.embedding_threshold), float(self.min_speech_duration), float(self.ema_alpha),
                                 float(self.validate_min_magnitude), int(self.max_speakers), int(self.raw_capacity))


@dataclass
class Speaker:  # the fields of Speaker the database keeps; raw_embeddings oldest first, [n, 256]
    id: int
    current_embedding: np.ndarray
    duration: float = 0.0
    raw_embeddings: np.ndarray = field(default_factory=lambda: np.zeros((0, EMBEDDING_SIZE), np.float32))
    update_count: int = 1
    created_tick: int = 0
    updated_tick: int = 0
    is_permanent: bool = False
    slot: int = -1


ONLINE_RUN_DTYPE, ONLINE_SEGMENT_DTYPE = np.dtype(L.OnlineRun), np.dtype(L.OnlineSegment)
ONLINE_PACK_ZERO_TAIL, ONLINE_PACK_REPEAT = 0, 1


@dataclass
class OnlineChunkConfig:  # fa_online_chunk_config
    frames: int = 589
    chunk_samples: int = 160000
    min_active_frames: float = 10.0
    min_speech_duration: float = 1.0
    validate_min_magnitude: float = 0.1
    frame_step: float = 0.016875

    def c(self) -> L.OnlineChunkConfig:
        return L.OnlineChunkConfig(int(self.frames), int(self.chunk_samples), float(self.min_active_frames), float(self.min_speech_duration),
                                   float(self.validate_min_magnitude), 0, float(self.frame_step))


def l2_normalize(embedding) -> np.ndarray:
    """VDSPOperations.l2Normalize with the library's sums."""
    e = np.ascontiguousarray(embedding, np.float32)
    assert e.shape == (EMBEDDING_SIZE,), "l2_normalize: 256 elements"
    out = np.zeros(EMBEDDING_SIZE, np.float32)
    L.lib().fa_speaker_l2_normalize(e.ctypes.data, out.ctypes.data)
    return out


def cosine_distance(a, b) -> np.float32:
    """SpeakerUtilities.cosineDistance; infinity for embeddings of another size than 256, as for a mismatch in the reference."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != (EMBEDDING_SIZE,) or b.shape != (EMBEDDING_SIZE,):
        return np.float32(np.inf)
    return np.float32(L.lib().fa_speaker_cosine_distance(a.ctypes.data, b.ctypes.data))


def validate_embedding(embedding, min_magnitude: float = 0.1) -> bool:
    """SpeakerUtilities.validateEmbedding."""
    e = np.ascontiguousarray(embedding, np.float32)
    return e.shape == (EMBEDDING_SIZE,) and bool(L.lib().fa_speaker_validate_embedding(e.ctypes.data, float(min_magnitude)))


class SpeakerDatabase:
    """fa_speaker_db: `streams` independent speaker tables on the context's device."""

    def __init__(self, streams: int, config: SpeakerDbConfig | None = None, ctx: L.Context | None = None):
        self.ctx = ctx or L.default_context()
        self.config = config or SpeakerDbConfig()
        self.streams = int(streams)
        self._h = C.c_void_p()
        cfg = self.config.c()
        self.ctx.check(L.lib().fa_speaker_db_create(self.ctx.handle, C.byref(cfg), self.streams, C.byref(self._h)), "fa_speaker_db_create")

    def close(self):
        if self._h:
            L.lib().fa_speaker_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, x, per=None):
        """[streams, per, 256] float32 on the device: a CUDA tensor as it is, anything else copied there."""
        if not (hasattr(x, "data_ptr") and x.is_cuda):
            x = A.to_device(x, np.float32, f"cuda:{self.ctx.device}")
        assert x.device.index == self.ctx.device, "speaker database: the embeddings live on another device than the context"
        assert A.is_dev(x, "float32", 3) and x.shape[0] == self.streams and x.shape[2] == EMBEDDING_SIZE, \
            f"speaker database: embeddings must be contiguous float32 [{self.streams}, per, {EMBEDDING_SIZE}], not {tuple(x.shape)}"
        assert per is None or x.shape[1] == per
        return x

    def assign_dev(self, d_embeddings, d_durations, d_skip=None, tick: int = 0):
        """fa_speaker_db_assign_dev on CUDA tensors; returns the records as an int32 CUDA tensor [streams, per, 4] (id, slot, kind, the
        distance's bits) without synchronising."""
        import torch
        d_embeddings = self._rows(d_embeddings)
        per = d_embeddings.shape[1]
        for t, dt, what in ((d_durations, torch.float32, "durations"), (d_skip, torch.int32, "skip")):
            assert t is None and what == "skip" or (isinstance(t, torch.Tensor) and t.device == d_embeddings.device and t.dtype == dt and t.is_contiguous()
                                                    and tuple(t.shape) == (self.streams, per)), f"speaker database: {what} must be contiguous {dt} [{self.streams}, {per}] beside the embeddings"
        out = torch.zeros((self.streams, per, 4), dtype=torch.int32, device=d_embeddings.device)
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_speaker_db_assign_dev(self.ctx.handle, self._h, A.ptr(d_embeddings), A.ptr(d_durations), A.ptr(d_skip), per, int(tick),
                                                            A.ptr(out)), "fa_speaker_db_assign_dev")
        return out

    def assign(self, embeddings, durations, skip=None, tick: int = 0) -> np.ndarray:
        """assignSpeaker for [streams, per] items, in index order within a stream: records of SPEAKER_ASSIGNMENT_DTYPE [streams, per]."""
        emb = self._rows(embeddings)
        per = emb.shape[1]

        def vec(v, dt):
            return v if hasattr(v, "data_ptr") and v.is_cuda else A.to_device(v, dt, emb.device, (self.streams, per))

        out = self.assign_dev(emb, vec(durations, np.float32), vec(skip, np.int32), tick)
        self.ctx.synchronize()
        return out.cpu().numpy().view(SPEAKER_ASSIGNMENT_DTYPE).reshape(self.streams, per)

    def distances(self, queries):
        """findSpeaker's distances: the queries as they are (not normalised) against every slot -> (float32 [streams, per, max_speakers], +inf
        on a free slot; int32 [streams, per] the closest slot, -1: none)."""
        q = self._rows(queries)
        per = q.shape[1]
        dist, best = A.beside(q, (self.streams, per, self.config.max_speakers), "float32"), A.beside(q, (self.streams, per), "int32")
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_speaker_db_distances_dev(self.ctx.handle, self._h, A.ptr(q), per, A.ptr(dist), A.ptr(best)), "fa_speaker_db_distances_dev")
        self.ctx.synchronize()
        return dist.cpu().numpy(), best.cpu().numpy()

    def _one_query(self, stream, embedding):
        q = np.zeros((self.streams, 1, EMBEDDING_SIZE), np.float32)
        q[stream, 0] = embedding
        dist, best = self.distances(q)
        return dist[stream, 0], int(best[stream, 0]), self.ids(stream, by_slot=True)

    def find_speaker(self, stream: int, embedding, speaker_threshold: float | None = None):
        """findSpeaker (:184-191): (id, distance) of the closest speaker when within the threshold, else (None, inf)."""
        dist, best, ids = self._one_query(stream, embedding)
        thr = np.float32(self.config.speaker_threshold if speaker_threshold is None else speaker_threshold)
        if best >= 0 and dist[best] <= thr:
            return ids[best], dist[best]
        return None, np.float32(np.inf)

    def find_matching_speakers(self, stream: int, embedding, speaker_threshold: float | None = None):
        """findMatchingSpeakers (:198-212): [(id, distance)] within the threshold, ascending by distance, ties by slot."""
        dist, _, ids = self._one_query(stream, embedding)
        thr = np.float32(self.config.speaker_threshold if speaker_threshold is None else speaker_threshold)
        found = [(ids[s], dist[s]) for s in range(len(dist)) if s in ids and dist[s] <= thr]
        return sorted(found, key=lambda m: m[1])

    def mergeable_pairs(self, speaker_threshold: float | None = None, exclude_if_both_permanent: bool = True):
        """findMergeablePairs (:282-328) of every stream: a list per stream of SPEAKER_PAIR_DTYPE records."""
        import torch
        S = self.config.max_speakers
        cap = max(S * (S - 1) // 2, 1)
        dev = f"cuda:{self.ctx.device}"
        pairs = torch.zeros((self.streams, cap, 5), dtype=torch.int32, device=dev)
        counts = torch.zeros(self.streams, dtype=torch.int32, device=dev)
        thr = float(self.config.speaker_threshold if speaker_threshold is None else speaker_threshold)
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_speaker_db_mergeable_pairs_dev(self.ctx.handle, self._h, thr, 1 if exclude_if_both_permanent else 0, A.ptr(pairs), cap,
                                                                     A.ptr(counts)), "fa_speaker_db_mergeable_pairs_dev")
        self.ctx.synchronize()
        rec, n = pairs.cpu().numpy().view(SPEAKER_PAIR_DTYPE).reshape(self.streams, cap), counts.cpu().numpy()
        return [rec[b, :n[b]].copy() for b in range(self.streams)]

    # ---- management: host data, complete on return
    def upsert(self, stream: int, speaker: Speaker):
        """upsertSpeaker (:552-606).  speaker.raw_embeddings are stored as they are (RawEmbedding.init's normalisation is the caller's)."""
        cur = np.ascontiguousarray(speaker.current_embedding, np.float32)
        raws = np.ascontiguousarray(speaker.raw_embeddings, np.float32).reshape(-1, EMBEDDING_SIZE)
        assert cur.shape == (EMBEDDING_SIZE,), "speaker database: the current embedding has 256 elements"
        info = L.SpeakerInfo(int(speaker.id), -1, len(raws), int(speaker.update_count), 1 if speaker.is_permanent else 0, float(speaker.duration),
                             int(speaker.created_tick), int(speaker.updated_tick))
        self.ctx.check(L.lib().fa_speaker_db_upsert(self.ctx.handle, self._h, int(stream), C.byref(info), cur.ctypes.data, raws.ctypes.data if len(raws) else None),
                       "fa_speaker_db_upsert")

    def get(self, stream: int, id: int) -> Speaker | None:
        """getSpeaker: the whole record, or None."""
        info = L.SpeakerInfo()
        cur = np.zeros(EMBEDDING_SIZE, np.float32)
        raws = np.zeros((self.config.raw_capacity, EMBEDDING_SIZE), np.float32)
        self.ctx.check(L.lib().fa_speaker_db_get(self.ctx.handle, self._h, int(stream), int(id), C.byref(info), cur.ctypes.data, raws.ctypes.data,
                                                 self.config.raw_capacity), "fa_speaker_db_get")
        if info.id == 0:
            return None
        return Speaker(info.id, cur, float(np.float32(info.duration)), raws[:info.raw_count].copy(), info.update_count, info.created_tick, info.updated_tick,
                       bool(info.is_permanent), info.slot)

    def ids(self, stream: int, by_slot: bool = False):
        """speakerIds in slot order; by_slot: {slot: id}."""
        ids = np.zeros(self.config.max_speakers, np.int32)
        n = C.c_int32()
        self.ctx.check(L.lib().fa_speaker_db_ids(self.ctx.handle, self._h, int(stream), ids.ctypes.data, C.byref(n)), "fa_speaker_db_ids")
        found = [int(i) for i in ids[:n.value]]
        if not by_slot:
            return found
        slots, info = {}, L.SpeakerInfo()
        for i in found:   # the slot's scalars only: no embedding is copied
            self.ctx.check(L.lib().fa_speaker_db_get(self.ctx.handle, self._h, int(stream), i, C.byref(info), None, None, 0), "fa_speaker_db_get")
            slots[info.slot] = i
        return slots

    def counts(self) -> np.ndarray:
        """speakerCount of every stream."""
        out = np.zeros(self.streams, np.int32)
        self.ctx.check(L.lib().fa_speaker_db_count(self.ctx.handle, self._h, out.ctypes.data), "fa_speaker_db_count")
        return out

    def remove(self, stream: int, id: int, keep_if_permanent: bool = True):
        self.ctx.check(L.lib().fa_speaker_db_remove(self.ctx.handle, self._h, int(stream), int(id), 1 if keep_if_permanent else 0), "fa_speaker_db_remove")

    def remove_inactive(self, since_tick: int, stream: int = -1, keep_if_permanent: bool = True):
        self.ctx.check(L.lib().fa_speaker_db_remove_inactive(self.ctx.handle, self._h, int(stream), int(since_tick), 1 if keep_if_permanent else 0),
                       "fa_speaker_db_remove_inactive")

    def set_permanent(self, stream: int, id: int, permanent: bool = True):
        self.ctx.check(L.lib().fa_speaker_db_set_permanent(self.ctx.handle, self._h, int(stream), int(id), 1 if permanent else 0), "fa_speaker_db_set_permanent")

    def reset(self, stream: int = -1, keep_if_permanent: bool = False):
        self.ctx.check(L.lib().fa_speaker_db_reset(self.ctx.handle, self._h, int(stream), 1 if keep_if_permanent else 0), "fa_speaker_db_reset")


def _dev_f32(x, shape, what, device):
    assert A.is_dev(x, "float32") and x.device.index == device and tuple(x.shape) == tuple(shape), \
        f"{what} must be a contiguous float32 CUDA tensor {tuple(shape)} on the context's device"
    return x


def chunk_plan(d_weights, samples_in_chunk=None, config: OnlineChunkConfig | None = None, ctx: L.Context | None = None):
    """fa_online_chunk_plan on d_weights [streams, chunks, frames, 3] (CUDA): activities [streams, chunks, 3] and the model's mask rows
    [runs, frames] as CUDA tensors, the run list as ONLINE_RUN_DTYPE records.  samples_in_chunk: ints [streams, chunks] or None."""
    ctx = ctx or L.default_context()
    cfg = config or OnlineChunkConfig()
    assert d_weights.dim() == 4, "chunk_plan: weights [streams, chunks, frames, 3]"
    B, Cn = d_weights.shape[:2]
    _dev_f32(d_weights, (B, Cn, cfg.frames, 3), "chunk_plan: weights", ctx.device)
    dev = d_weights.device
    d_samples = A.to_device(samples_in_chunk, np.int32, dev, (B, Cn))
    cap = B * Cn * 3
    act, runs, rows = A.beside(d_weights, (B, Cn, 3), "float32"), A.beside(d_weights, (cap, 3), "int32"), A.beside(d_weights, (cap, cfg.frames), "float32")
    n, c = C.c_int32(), cfg.c()
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_online_chunk_plan(ctx.handle, C.byref(c), A.ptr(d_weights), A.ptr(d_samples), B, Cn, A.ptr(act), A.ptr(runs), cap, C.byref(n), A.ptr(rows)),
                  "fa_online_chunk_plan")
    return act, runs[:n.value].cpu().numpy().view(ONLINE_RUN_DTYPE).reshape(-1), rows[:n.value]


def pack_waveforms(d_audio, offsets, lengths, chunk_samples: int = 160000, mode: int = ONLINE_PACK_ZERO_TAIL, ctx: L.Context | None = None):
    """fa_online_pack_waveforms_dev: rows [len(offsets), chunk_samples] (CUDA) from the flat CUDA tensor d_audio."""
    ctx = ctx or L.default_context()
    offsets, lengths = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(lengths, np.int32)
    assert A.is_dev(d_audio, "float32", 1) and d_audio.device.index == ctx.device, "pack_waveforms: a flat contiguous float32 CUDA tensor on the context's device"
    assert offsets.shape == lengths.shape and offsets.ndim == 1 and offsets.size >= 1 and bool(np.all(lengths >= 0)) and bool(np.all(offsets >= 0)) and \
        bool(np.all(offsets + np.minimum(lengths, chunk_samples) <= d_audio.numel())), "pack_waveforms: a row reaches outside the audio"
    out = A.beside(d_audio, (offsets.size, int(chunk_samples)), "float32")
    d_off, d_len = A.to_device(offsets, np.int64, d_audio.device), A.to_device(lengths, np.int32, d_audio.device)
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_online_pack_waveforms_dev(ctx.handle, A.ptr(d_audio), A.ptr(d_off), A.ptr(d_len), offsets.size, int(chunk_samples), int(mode), A.ptr(out)),
                  "fa_online_pack_waveforms_dev")
    return out


def chunk_finish(db: SpeakerDatabase, d_weights, d_activities, d_embeddings, chunk_offsets, config: OnlineChunkConfig | None = None, tick: int = 0,
                 capacity: int | None = None):
    """fa_online_chunk_finish_dev: the gate, the assignment into db and the timed segments of [streams, chunks] chunks.  Returns (segments as
    ONLINE_SEGMENT_DTYPE records, assignments SPEAKER_ASSIGNMENT_DTYPE [streams, chunks, 3], chunk_counts [streams, chunks]).  With a
    capacity below the segments' count FluidAudioHipError(OUTPUT_TOO_SMALL) carries the count as .count."""
    cfg = config or OnlineChunkConfig()
    ctx = db.ctx
    assert d_weights.dim() == 4, "chunk_finish: weights [streams, chunks, frames, 3]"
    B, Cn = d_weights.shape[:2]
    assert B == db.streams, "chunk_finish: one row of chunks per stream of the database"
    _dev_f32(d_weights, (B, Cn, cfg.frames, 3), "chunk_finish: weights", ctx.device)
    _dev_f32(d_activities, (B, Cn, 3), "chunk_finish: activities", ctx.device)
    _dev_f32(d_embeddings, (B, Cn, 3, EMBEDDING_SIZE), "chunk_finish: embeddings", ctx.device)
    off = np.ascontiguousarray(chunk_offsets, np.float64).reshape(B, Cn)
    cap = B * Cn * 3 * ((cfg.frames + 1) // 2) if capacity is None else int(capacity)
    seg = np.zeros(max(cap, 1), ONLINE_SEGMENT_DTYPE)
    counts = np.zeros((B, Cn), np.int32)
    assign = A.beside(d_weights, (B, Cn, 3, 4), "int32")
    n, c = C.c_int64(), cfg.c()
    with ctx.torch_ordered():
        st = L.lib().fa_online_chunk_finish_dev(ctx.handle, C.byref(c), db._h, A.ptr(d_weights), A.ptr(d_activities), A.ptr(d_embeddings), off.ctypes.data, Cn, int(tick),
                                                seg.ctypes.data, cap, C.byref(n), counts.ctypes.data, A.ptr(assign))
    if st != L.SUCCESS:
        err = L.FluidAudioHipError(st, "fa_online_chunk_finish_dev", ctx.last_error())
        err.count = int(n.value)
        raise err
    return seg[:n.value].copy(), assign.cpu().numpy().view(SPEAKER_ASSIGNMENT_DTYPE).reshape(B, Cn, 3), counts
