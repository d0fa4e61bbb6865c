"""The embedding model's inputs on the device (csrc/embedding.hip, csrc/embedding_host.hip): OfflineEmbeddingExtractor.extractEmbeddings up to the networks
(reference: Sources/FluidAudio/Diarizer/Offline/Extraction/OfflineEmbeddingExtractor.swift:177-711) and WeightInterpolation
(Diarizer/Offline/Utils/WeightInterpolation.swift:19-116).

plan_embeddings decides which (chunk, local speaker) pairs get an embedding, writes each model run's resampled mask on the device and
returns the TimedEmbedding metadata; EmbeddingPlan.windows cuts one fbank batch of audio windows at a time; span_inputs builds embedSpan's
window and all-active mask for the zero-vote pass.  The networks themselves are the caller's (pipeline.extract_embeddings)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _args as A, _lib as L
from .reconstruct import SegmentationOutput

RECORD_DTYPE = np.dtype(L.ExportEmbedding)


@dataclass
class EmbeddingConfig:   # OfflineDiarizerTypes.swift:46-55, 82-105, 297-303, 348-353
    window_duration: float = 10.0
    sample_rate: int = 16000
    samples_per_window: int = 0          # 0 = Int(sample_rate * window_duration)
    overlap_threshold: float = 1e-3
    exclude_overlap: bool = True
    min_segment_duration: float = 1.0
    batch_size: int = 32
    skip_threshold: float | None = None  # None: EmbeddingSkipStrategy.none; a value: maskSimilarity(threshold)
    weight_frames: int = 589

    def c_config(self, frame_duration: float = 0.0) -> L.EmbeddingConfig:
        c = L.EmbeddingConfig()
        L.lib().fa_embedding_default_config(C.byref(c))
        c.window_duration, c.sample_rate, c.samples_per_window = float(self.window_duration), int(self.sample_rate), int(self.samples_per_window)
        c.overlap_threshold, c.exclude_overlap = float(self.overlap_threshold), int(bool(self.exclude_overlap))
        c.min_segment_duration, c.batch_size = float(self.min_segment_duration), int(self.batch_size)
        c.skip_enabled = int(self.skip_threshold is not None)
        if self.skip_threshold is not None:
            c.skip_threshold = float(self.skip_threshold)
        c.weight_frames, c.frame_duration = int(self.weight_frames), float(frame_duration)
        return c

    @property
    def window_samples(self) -> int:
        return int(self.samples_per_window) if self.samples_per_window > 0 else int(float(self.sample_rate) * self.window_duration)


@dataclass
class EmbeddingPlan:
    """records: RECORD_DTYPE [jobs] (chunk, local speaker, first / last active frame, start / end time), chunk-major, speaker-minor;
    run_of_job int32 [jobs]; window_of_run int32 [runs]; window_start int64 / window_chunk int32 [planned windows]; run_weights [runs,
    weight_frames] fp32 (a torch CUDA tensor when the weights were on the device, else numpy): the embedding model's weights input;
    mask_rows [jobs, frames] or None (TimedEmbedding.frameWeights); info: the fa_embedding_info counters."""
    records: np.ndarray
    run_of_job: np.ndarray
    window_of_run: np.ndarray
    window_start: np.ndarray
    window_chunk: np.ndarray
    run_weights: object
    mask_rows: object
    info: dict
    samples_per_window: int
    ctx: L.Context

    @property
    def chunk_indices(self) -> np.ndarray:
        return self.records["chunk_index"].copy()

    @property
    def speaker_indices(self) -> np.ndarray:
        return self.records["speaker_index"].copy()

    @property
    def batch_size(self) -> int:
        return int(self.info["batch_size"])

    @property
    def batches(self) -> int:
        return int(self.info["batches"])

    def batch_windows(self, batch: int) -> range:
        b = self.batch_size
        return range(batch * b, min((batch + 1) * b, self.window_start.size))

    def batch_runs(self, batch: int) -> range:
        """The runs whose fbank window is in this batch (runs are in window order)."""
        w = self.batch_windows(batch)
        return range(int(np.searchsorted(self.window_of_run, w.start)), int(np.searchsorted(self.window_of_run, w.stop)))

    def windows(self, batch: int, audio):
        """The fbank inputs of one batch: a torch CUDA tensor [windows, samples_per_window] = audio[start : start + S] then zeros.
        audio: a torch CUDA fp32 tensor on the plan's device (the whole recording)."""
        w = self.batch_windows(batch)
        x, on_device = A.placed(audio, self.ctx)
        if not on_device:
            raise ValueError("EmbeddingPlan.windows needs the audio as a torch CUDA tensor")
        out = A.beside(x, (len(w), self.samples_per_window), "float32", torch_empty=True)
        starts = np.ascontiguousarray(self.window_start[w.start:w.stop], np.int64)
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_embedding_windows_dev(self.ctx.handle, x.data_ptr(), x.numel(), starts.ctypes.data if starts.size else None,
                                                            starts.size, self.samples_per_window, out.data_ptr()), "fa_embedding_windows_dev")
        return out


def plan_embeddings(segmentation: SegmentationOutput, total_samples: int, config: EmbeddingConfig | None = None, mask_rows: bool = False,
                    ctx: L.Context | None = None) -> EmbeddingPlan:
    """extractEmbeddings' mask selection, skip chain and model inputs for one recording of total_samples samples.  The speaker weights may be
    numpy / a CPU tensor (host entry, numpy results) or a torch CUDA tensor on ctx's device (device entry: run_weights and mask_rows stay
    on the device, ordered against torch's current stream)."""
    cfg = config or EmbeddingConfig()
    ctx = ctx or L.default_context()
    w, on_device = A.placed(segmentation.speaker_weights, ctx)
    nc, nf, ns = (int(v) for v in w.shape)
    cap = nc * ns
    offs = np.ascontiguousarray([] if segmentation.chunk_offsets is None else segmentation.chunk_offsets, np.float64)
    recs = np.zeros(max(cap, 1), RECORD_DTYPE)
    roj, wor = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
    wst, wch = np.zeros(max(nc, 1), np.int64), np.zeros(max(nc, 1), np.int32)
    W = int(cfg.weight_frames)
    info = L.EmbeddingInfo()
    c = cfg.c_config(segmentation.frame_duration)
    rows = A.beside(w, (max(cap, 1), W), "float32", torch_empty=True)
    mrows = A.beside(w, (max(cap, 1), nf), "float32", torch_empty=True) if mask_rows else None
    name = "fa_embedding_plan_dev" if on_device else "fa_embedding_plan"
    with ctx.torch_ordered(on_device):
        st = getattr(L.lib(), name)(ctx.handle, C.byref(c), A.ptr(w), nc, nf, ns, offs.ctypes.data if offs.size else None, offs.size, int(total_samples),
                                    recs.ctypes.data, roj.ctypes.data, wor.ctypes.data, wst.ctypes.data, wch.ctypes.data, A.ptr(rows), A.ptr(mrows), C.byref(info))
    ctx.check(st, name)
    jobs, runs, nw = info.jobs, info.runs, info.planned_chunks
    return EmbeddingPlan(recs[:jobs].copy(), roj[:jobs].copy(), wor[:runs].copy(), wst[:nw].copy(), wch[:nw].copy(), rows[:runs],
                         mrows[:jobs] if mrows is not None else None, info.as_dict(), int(info.samples_per_window), ctx)


def weight_resample(rows, out_frames: int, ctx: L.Context | None = None):
    """WeightInterpolation.resample2D: rows [n, in_frames] (or one row [in_frames]) -> [n, out_frames]; a torch CUDA tensor stays on the
    device.  An empty input or out_frames 0 gives an empty result (resample's `[]`)."""
    ctx = ctx or L.default_context()
    x, on_device = A.placed(rows, ctx)
    one = x.ndim == 1
    x = x.reshape(1, -1) if one else x
    n, k = int(x.shape[0]), int(x.shape[1])
    m = int(out_frames) if k > 0 else 0
    out = A.beside(x, (n, max(m, 0)), "float32", torch_empty=True)
    name = "fa_weight_resample_dev" if on_device else "fa_weight_resample"
    with ctx.torch_ordered(on_device):
        ctx.check(getattr(L.lib(), name)(ctx.handle, A.ptr(x), n, k, m, A.ptr(out)), name)
    return out[0] if one else out


def span_inputs(audio, spans, config: EmbeddingConfig | None = None, ctx: L.Context | None = None):
    """embedSpan's inputs (:243-297) for spans [(start_s, end_s)]: (windows [n, samples_per_window], weights [n, weight_frames], ok [n] bool).
    audio numpy / CPU tensor -> numpy results; a torch CUDA tensor -> device results.  A span without samples is not ok (zero rows)."""
    cfg = config or EmbeddingConfig()
    ctx = ctx or L.default_context()
    x, on_device = A.placed(audio, ctx)
    sp = np.ascontiguousarray(spans, np.float64).reshape(-1, 2)
    n, spw, W = sp.shape[0], cfg.window_samples, int(cfg.weight_frames)
    stat = np.zeros(max(n, 1), np.int32)
    c = cfg.c_config()
    win, wts = A.beside(x, (n, spw), "float32"), A.beside(x, (n, W), "float32")
    name = "fa_embedding_span_inputs_dev" if on_device else "fa_embedding_span_inputs"
    with ctx.torch_ordered(on_device):
        st = getattr(L.lib(), name)(ctx.handle, C.byref(c), A.ptr(x), x.numel() if on_device else x.size, sp.ctypes.data if n else None, n, A.ptr(win), A.ptr(wts),
                                    stat.ctypes.data)
    ctx.check(st, name)
    return win, wts, stat[:n] == L.SUCCESS
