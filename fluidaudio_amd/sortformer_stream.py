"""Streaming Sortformer's state between chunks (reference: Sources/FluidAudio/Diarizer/Sortformer/SortformerStateUpdater.swift:31-578,
SortformerTypes.swift:26-97, 219-255, 264-385, SortformerDiarizer.swift:514-578, 933-979) as device-resident state batched over streams,
over the HIP C ABI (csrc/sortformer_stream.hip, csrc/sortformer_stream_host.hip, csrc/sortformer_stream_core.h): the FIFO of recent
embeddings, the speaker cache with its compression, the silence profile.  One stream is one SortformerStreamingState.

The network stays the caller's: it reads SortformerStreamState.inputs() in place — four tensors whose addresses never change — and its
embeddings and predictions go to update_dev.  chunk_plan / file_chunks / pack_chunks are the mel-side chunk geometry."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _args as A, _lib as L

SORTFORMER_CHUNK_DTYPE = np.dtype(L.SortformerChunk)
SORTFORMER_STREAM_STATUS = ("OK", "INACTIVE", "SHORT_PREDS_FIFO", "SHORT_CHUNK", "SHORT_PREDS_CHUNK", "SHORT_PREDS_TENTATIVE", "NEGATIVE_CORE", "BAD_PRED",
                            "BAD_OPERAND")   # FA_SORTFORMER_STREAM_*
SORTFORMER_STREAM_PRESETS = {"default": 0, "fast": 0, "balanced": 1, "high_context": 2, "efficient": 3}


@dataclass
class SortformerStreamConfig:  # fa_sortformer_stream_config = SortformerConfig
    speakers: int = 4
    d_model: int = 512
    chunk_len: int = 6
    chunk_left_context: int = 1
    chunk_right_context: int = 7
    fifo_len: int = 40
    spkcache_len: int = 188
    spkcache_update_period: int = 31
    sil_frames_per_spk: int = 3
    max_index: int = 99999
    max_chunk_frames: int = 0          # 0: chunk_len + both contexts
    subsampling: int = 8
    n_mels: int = 128
    silence_threshold: float = 0.2
    pred_score_threshold: float = 0.25
    scores_boost_latest: float = 0.05
    strong_boost_rate: float = 0.75
    weak_boost_rate: float = 1.5
    min_pos_scores_rate: float = 0.5

    @classmethod
    def preset(cls, name: str) -> "SortformerStreamConfig":
        c = L.SortformerStreamConfig()
        st = L.lib().fa_sortformer_stream_preset_config(SORTFORMER_STREAM_PRESETS[name], C.byref(c))
        if st != L.SUCCESS:
            raise L.FluidAudioHipError(st, "fa_sortformer_stream_preset_config")
        return cls(**{f: getattr(c, f) for f, _ in L.SortformerStreamConfig._fields_ if f != "reserved"})

    def c(self) -> L.SortformerStreamConfig:
        frames = self.max_chunk_frames or max(1, self.chunk_len) + self.chunk_left_context + self.chunk_right_context
        return L.SortformerStreamConfig(int(self.speakers), int(self.d_model), int(self.chunk_len), int(self.chunk_left_context), int(self.chunk_right_context),
                                        int(self.fifo_len), int(self.spkcache_len), int(self.spkcache_update_period), int(self.sil_frames_per_spk), int(self.max_index),
                                        int(frames), int(self.subsampling), int(self.n_mels), 0, float(self.silence_threshold), float(self.pred_score_threshold),
                                        float(self.scores_boost_latest), float(self.strong_boost_rate), float(self.weak_boost_rate), float(self.min_pos_scores_rate))

    def geometry(self) -> L.SortformerStreamGeometry:
        """The clamps applied and the derived integers (fa_sortformer_stream_geometry)."""
        g, c = L.SortformerStreamGeometry(), self.c()
        st = L.lib().fa_sortformer_stream_geometry(C.byref(c), C.byref(g))
        if st != L.SUCCESS:
            raise A.invalid("fa_sortformer_stream_geometry", "the config is refused")
        return g


@dataclass
class SortformerStreamSnapshot:  # one stream's SortformerStreamingState; rows past a length are zero
    spkcache_length: int
    fifo_length: int
    spkcache_preds_present: bool
    fifo_preds_present: bool
    silence_frame_count: int
    spkcache: np.ndarray           # [spkcache_len, d_model]
    spkcache_preds: np.ndarray     # [spkcache_len, speakers]
    fifo: np.ndarray               # [fifo_len, d_model]
    fifo_preds: np.ndarray         # [fifo_len, speakers]
    mean_silence: np.ndarray       # [d_model]


@dataclass
class SortformerStreamUpdate:  # CUDA tensors; nothing has been waited for
    confirmed: object       # float32 [streams, out_rows, speakers]
    tentative: object       # float32 [streams, out_rows, speakers]
    counts: object          # int32 [streams, 2]: confirmed rows, tentative rows
    status: object          # int32 [streams]
    log_scores: object      # float32 [streams, score_rows, speakers] or None


class SortformerStreamState:
    """fa_sortformer_stream: `streams` independent streaming states on the context's device."""

    def __init__(self, streams: int, config: SortformerStreamConfig | None = None, ctx: L.Context | None = None):
        self.ctx = ctx or L.default_context()
        self.config = config or SortformerStreamConfig()
        self.streams = int(streams)
        self._h = C.c_void_p()
        cfg = self.config.c()
        self.ctx.check(L.lib().fa_sortformer_stream_create(self.ctx.handle, C.byref(cfg), self.streams, C.byref(self._h)), "fa_sortformer_stream_create")
        self.geometry = self.config.geometry()

    def close(self):
        if self._h:
            L.lib().fa_sortformer_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def input_pointers(self):
        """The four device addresses the network reads (spkcache, its lengths, fifo, its lengths): fixed for the object's lifetime."""
        p = [C.c_void_p() for _ in range(4)]
        self.ctx.check(L.lib().fa_sortformer_stream_inputs(self.ctx.handle, self._h, *[C.byref(x) for x in p]), "fa_sortformer_stream_inputs")
        return tuple(int(x.value) for x in p)

    def _out(self, shape, dtype_name, zero=False):
        import torch
        return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, dtype_name), device=f"cuda:{self.ctx.device}")

    def update_dev(self, d_chunk_embs, d_emb_len, d_preds, d_pred_rows, d_left, d_right, d_active=None, log_scores=False, out: SortformerStreamUpdate | None = None):
        """fa_sortformer_stream_update_dev on CUDA tensors: d_chunk_embs float32 or float16 [streams, max_chunk_frames, d_model], d_preds float32
        [streams, pred_stride, speakers], the five int32 [streams] vectors.  Enqueued; nothing is waited for.  `out` reuses the outputs of an
        earlier call (then nothing is allocated either)."""
        import torch
        g, cfg, B = self.geometry, self.config, self.streams
        assert A.is_dev(d_chunk_embs, "float32", 3) or A.is_dev(d_chunk_embs, "float16", 3), "update: embeddings must be a contiguous float32 / float16 CUDA tensor"
        assert tuple(d_chunk_embs.shape) == (B, g.out_rows, cfg.d_model) and d_chunk_embs.device.index == self.ctx.device, \
            f"update: embeddings [{B}, {g.out_rows}, {cfg.d_model}] on the context's device, not {tuple(d_chunk_embs.shape)}"
        assert A.is_dev(d_preds, "float32", 3) and d_preds.shape[0] == B and d_preds.shape[2] == cfg.speakers and d_preds.device == d_chunk_embs.device, \
            f"update: preds must be contiguous float32 [{B}, pred_stride, {cfg.speakers}] beside the embeddings"
        for t, what in ((d_emb_len, "emb_len"), (d_pred_rows, "pred_rows"), (d_left, "left"), (d_right, "right"), (d_active, "active")):
            assert (t is None and what == "active") or (A.is_dev(t, "int32", 1) and t.shape[0] == B and t.device == d_chunk_embs.device), \
                f"update: {what} must be a contiguous int32 CUDA tensor [{B}] beside the embeddings"
        if out is None:
            out = SortformerStreamUpdate(self._out((B, g.out_rows, cfg.speakers), "float32", True), self._out((B, g.out_rows, cfg.speakers), "float32", True),
                                         self._out((B, 2), "int32"), self._out((B,), "int32"), self._out((B, g.score_rows, cfg.speakers), "float32", True) if log_scores else None)
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_sortformer_stream_update_dev(self.ctx.handle, self._h, A.ptr(d_chunk_embs), L.DTYPE_F16 if d_chunk_embs.dtype == torch.float16 else L.DTYPE_F32,
                                                                   A.ptr(d_emb_len), A.ptr(d_preds), int(d_preds.shape[1]), A.ptr(d_pred_rows), A.ptr(d_left), A.ptr(d_right),
                                                                   A.ptr(d_active), A.ptr(out.confirmed), A.ptr(out.tentative), A.ptr(out.counts), A.ptr(out.status),
                                                                   A.ptr(out.log_scores)), "fa_sortformer_stream_update_dev")
        return out

    def update(self, chunk_embs, emb_len, preds, pred_rows, left, right, active=None, log_scores=False):
        """The same on host arrays (fa_sortformer_stream_update, one synchronisation): (confirmed, tentative, counts [streams, 2], status [streams],
        log_scores or None) as numpy arrays."""
        g, cfg, B = self.geometry, self.config, self.streams
        embs = np.ascontiguousarray(chunk_embs)
        embs = embs if embs.dtype == np.float16 else np.ascontiguousarray(embs, np.float32)
        preds = np.ascontiguousarray(preds, np.float32)
        assert embs.shape == (B, g.out_rows, cfg.d_model) and preds.ndim == 3 and preds.shape[0] == B and preds.shape[2] == cfg.speakers, "update: embeddings / preds shapes"
        vec = [None if v is None else np.ascontiguousarray(v, np.int32).reshape(B) for v in (emb_len, pred_rows, left, right, active)]
        conf, tent = np.zeros((B, g.out_rows, cfg.speakers), np.float32), np.zeros((B, g.out_rows, cfg.speakers), np.float32)
        counts, status = np.zeros((B, 2), np.int32), np.zeros(B, np.int32)
        scores = np.zeros((B, g.score_rows, cfg.speakers), np.float32) if log_scores else None
        self.ctx.check(L.lib().fa_sortformer_stream_update(self.ctx.handle, self._h, A.ptr(embs), L.DTYPE_F16 if embs.dtype == np.float16 else L.DTYPE_F32, A.ptr(vec[0]), A.ptr(preds),
                                                           int(preds.shape[1]), A.ptr(vec[1]), A.ptr(vec[2]), A.ptr(vec[3]), A.ptr(vec[4]), A.ptr(conf), A.ptr(tent), A.ptr(counts),
                                                           A.ptr(status), A.ptr(scores)), "fa_sortformer_stream_update")
        return conf, tent, counts, status, scores

    # ---- whole-state records: host data, complete on return
    def get(self, stream: int) -> SortformerStreamSnapshot:
        cfg, info = self.config, L.SortformerStreamInfo()
        cap = self.geometry.spkcache_len
        a = [np.zeros(s, np.float32) for s in ((cap, cfg.d_model), (cap, cfg.speakers), (cfg.fifo_len, cfg.d_model), (cfg.fifo_len, cfg.speakers), (cfg.d_model,))]
        self.ctx.check(L.lib().fa_sortformer_stream_get(self.ctx.handle, self._h, int(stream), C.byref(info), *[A.ptr(x) for x in a]), "fa_sortformer_stream_get")
        return SortformerStreamSnapshot(info.spkcache_length, info.fifo_length, bool(info.spkcache_preds_present), bool(info.fifo_preds_present), info.silence_frame_count, *a)

    def set(self, stream: int, s: SortformerStreamSnapshot):
        info = L.SortformerStreamInfo(int(s.spkcache_length), int(s.fifo_length), int(bool(s.spkcache_preds_present)), int(bool(s.fifo_preds_present)),
                                      int(s.silence_frame_count), 0)
        a = [np.ascontiguousarray(x, np.float32) for x in (s.spkcache, s.spkcache_preds, s.fifo, s.fifo_preds, s.mean_silence)]
        assert a[0].shape[0] >= s.spkcache_length and a[1].shape[0] >= s.spkcache_length and a[2].shape[0] >= s.fifo_length and a[3].shape[0] >= s.fifo_length and \
            a[4].shape == (self.config.d_model,), "set: rows for every length"
        self.ctx.check(L.lib().fa_sortformer_stream_set(self.ctx.handle, self._h, int(stream), C.byref(info), *[A.ptr(x) for x in a]), "fa_sortformer_stream_set")

    def reset(self, stream: int = -1):
        """cleanup() for one stream, or for all."""
        self.ctx.check(L.lib().fa_sortformer_stream_reset(self.ctx.handle, self._h, int(stream)), "fa_sortformer_stream_reset")

    cleanup = reset


def chunk_plan(feat_frames, start_feat, config: SortformerStreamConfig | None = None) -> np.ndarray:
    """getNextChunkFeaturesLocked for every stream: SORTFORMER_CHUNK_DTYPE records [streams].  Pure host function."""
    cfg = (config or SortformerStreamConfig()).c()
    ff, sf = np.ascontiguousarray(feat_frames, np.int64).reshape(-1), np.ascontiguousarray(start_feat, np.int64).reshape(-1)
    assert ff.shape == sf.shape and ff.size >= 1, "chunk_plan: one buffer length and one start per stream"
    out = np.zeros(ff.size, SORTFORMER_CHUNK_DTYPE)
    st = L.lib().fa_sortformer_stream_chunk_plan(C.byref(cfg), A.ptr(ff), A.ptr(sf), ff.size, A.ptr(out))
    if st != L.SUCCESS:
        raise A.invalid("fa_sortformer_stream_chunk_plan", "a refused config or a negative frame count")
    return out


def file_chunks(feat_length: int, feat_seq_length: int, config: SortformerStreamConfig | None = None):
    """SortformerFeatureLoader: (numChunks, SORTFORMER_CHUNK_DTYPE records of every chunk next() returns).  Pure host function."""
    cfg = (config or SortformerStreamConfig()).c()
    n, num = C.c_int64(), C.c_int64()
    st = L.lib().fa_sortformer_stream_file_chunks(C.byref(cfg), int(feat_length), int(feat_seq_length), None, 0, C.byref(n), C.byref(num))
    if st not in (L.SUCCESS, L.OUTPUT_TOO_SMALL):
        raise A.invalid("fa_sortformer_stream_file_chunks", "a refused config or a negative length")
    out = np.zeros(max(n.value, 1), SORTFORMER_CHUNK_DTYPE)
    st = L.lib().fa_sortformer_stream_file_chunks(C.byref(cfg), int(feat_length), int(feat_seq_length), A.ptr(out), out.size, C.byref(n), C.byref(num))
    assert st == L.SUCCESS
    return int(num.value), out[:n.value]


def pack_chunks(d_mel, stream_offsets, chunks, config: SortformerStreamConfig | None = None, ctx: L.Context | None = None):
    """fa_sortformer_stream_pack_chunks_dev: the network's rows [streams, chunk_mel_frames, n_mels] (CUDA) from the flat frame-major CUDA tensor
    d_mel, stream b's buffer beginning at frame stream_offsets[b].  Enqueued; nothing is waited for."""
    ctx = ctx or L.default_context()
    config = config or SortformerStreamConfig()
    cfg, g = config.c(), config.geometry()
    off = np.ascontiguousarray(stream_offsets, np.int64).reshape(-1)
    chunks = np.ascontiguousarray(chunks, SORTFORMER_CHUNK_DTYPE).reshape(-1)
    assert A.is_dev(d_mel, "float32") and d_mel.device.index == ctx.device, "pack_chunks: a contiguous float32 CUDA tensor on the context's device"
    assert off.shape == chunks.shape and off.size >= 1, "pack_chunks: one offset and one chunk per stream"
    ready = chunks["ready"] != 0
    assert bool(np.all(off >= 0)) and bool(np.all(chunks["start_frame"][ready] >= 0)) and \
        bool(np.all((off + chunks["start_frame"] + chunks["rows"])[ready] * config.n_mels <= d_mel.numel())), "pack_chunks: a chunk reaches outside the mel"
    out = A.beside(d_mel, (off.size, g.chunk_mel_frames, config.n_mels), "float32", torch_empty=True)
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_sortformer_stream_pack_chunks_dev(ctx.handle, C.byref(cfg), A.ptr(d_mel), A.ptr(off), A.ptr(chunks), off.size, A.ptr(out)),
                  "fa_sortformer_stream_pack_chunks_dev")
    return out
