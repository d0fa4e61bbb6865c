"""numpy restatement of OfflineEmbeddingExtractor.extractEmbeddings up to the networks (OfflineEmbeddingExtractor.swift:177-711) and of
WeightInterpolation (WeightInterpolation.swift:19-116), in the reference's order with scalar fp32 / fp64 semantics: every fp32 sum and dot
product is sequential in frame order (np.add.accumulate, never numpy's pairwise sum), every fp32 operation rounds on its own (numpy does
not fuse), sample indices round half away from zero.  The test oracle of csrc/embedding.hip and csrc/embedding_geom.h."""
import math
from dataclasses import dataclass

import numpy as np

f32 = np.float32


@dataclass
class Config:
    window_duration: float = 10.0
    sample_rate: int = 16000
    samples_per_window: int = 0
    overlap_threshold: float = 1e-3
    exclude_overlap: bool = True
    min_segment_duration: float = 1.0
    batch_size: int = 32
    skip_threshold: float | None = None
    weight_frames: int = 589

    @property
    def spw(self):
        return self.samples_per_window if self.samples_per_window > 0 else int(float(self.sample_rate) * self.window_duration)


def round_half_away(x: float) -> float:
    """Swift's Double.rounded() (.toNearestOrAwayFromZero)."""
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1.0
    return math.copysign(r, x)


def seq_sum(x, axis=-1):
    """fp32 sum in index order along axis (0 for an empty axis)."""
    x = np.asarray(x, f32)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis % x.ndim), f32)
    return np.take(np.add.accumulate(x, axis=axis, dtype=f32), -1, axis=axis)


def coefficients(n_in: int, n_out: int):
    """InterpolationCoefficients (:19-52): left, right, weightLeft, weightRight."""
    scale = f32(n_out) / f32(n_in)
    i = np.arange(n_out, dtype=f32)
    pos = (i + f32(0.5)) / scale - f32(0.5)
    cl = np.minimum(np.maximum(pos, f32(0)), f32(n_in - 1))
    left = np.floor(cl).astype(np.int64)
    right = np.minimum(left + 1, n_in - 1)
    wr = (cl - left.astype(f32)).astype(f32)
    wl = (f32(1) - wr).astype(f32)
    return left, right, wl, wr


def resample(x, n_out: int):
    """WeightInterpolation.resample (:96-108) over the last axis (rows: resample2D)."""
    x = np.asarray(x, f32)
    n_in = x.shape[-1]
    if n_in == 0 or n_out <= 0:
        return np.zeros(x.shape[:-1] + (0,), f32)
    if n_in == n_out:
        return x.copy()
    left, right, wl, wr = coefficients(n_in, n_out)
    return (x[..., left] * wl + x[..., right] * wr).astype(f32)


def chunk_plan(C, offsets, total_samples, cfg: Config):
    """Planned chunks (:650-668): (chunk, offset seconds, start sample) of every chunk whose window holds audio."""
    out = []
    offsets = [] if offsets is None else list(offsets)
    for c in range(C):
        off = float(offsets[c]) if c < len(offsets) else float(c) * cfg.window_duration
        if not math.isfinite(off):
            off = float(c) * cfg.window_duration
        r = round_half_away(off * float(cfg.sample_rate))
        start = 0 if not r > 0 else (total_samples if r >= total_samples else int(r))
        end = min(start + cfg.spw, total_samples)
        if start < end:
            out.append((c, off, start))
    return out


def cosine(a, b):
    """maskCosineSimilarity (:835-842), sequential fp32 dots."""
    dot, na, nb = seq_sum(a * b), seq_sum(a * a), seq_sum(b * b)
    denom = f32(np.sqrt(na)) * f32(np.sqrt(nb))
    return f32(dot / denom) if denom > 0 else f32(0)


def plan(weights, offsets, total_samples, cfg: Config, frame_duration: float = 0.0):
    """-> dict: windows [(chunk, offset, start)], records [(chunk, speaker, first, last, start_time, end_time)], run_of_job, window_of_run,
    run_rows [runs, W], mask_rows [jobs, F], counters (evaluated, empty, fallback, skipped), batch size."""
    w = np.asarray(weights, f32)
    C, F, S = w.shape
    B = max(1, min(cfg.batch_size, 32))
    out = dict(windows=[], records=[], run_of_job=[], window_of_run=[], run_rows=[], mask_rows=[], evaluated=0, empty=0, fallback=0, skipped=0, batch=B)
    if C == 0 or F == 0:
        return _arrays(out, F, cfg.weight_frames)
    fd = frame_duration if frame_duration > 0 else cfg.window_duration / F
    min_frames = max(1, int(math.ceil(cfg.min_segment_duration / fd))) if fd > 0 else 1
    thr = f32(cfg.overlap_threshold)
    wins = chunk_plan(C, offsets, total_samples, cfg)
    out["windows"] = wins
    W = cfg.weight_frames
    # per planned chunk: every slot's base / clean masks, sums and resampled energies, sequential in frame order
    idx = np.array([c for c, _, _ in wins], np.int64)
    if not np.isfinite(w[idx]).all():                                  # only planned chunks are read (the library's documented rule)
        raise ValueError("non-finite weight in a planned chunk")
    if idx.size == 0 or S == 0:
        return _arrays(out, F, W)
    base = np.transpose(w[idx], (0, 2, 1))                                # [nw, S, F]
    ovl = ((w[idx] > thr).sum(axis=2) > 1)[:, None, :] if cfg.exclude_overlap else np.zeros((idx.size, 1, F), bool)
    clean = np.where(ovl, f32(0), base).astype(f32)
    base_sum, clean_sum = seq_sum(base), seq_sum(clean)
    e_base, e_clean = seq_sum(resample(base, W)), seq_sum(resample(clean, W))
    min_active = f32(F) * f32(0.2)
    cache = {}
    for wi, (c, off, _) in enumerate(wins):
        if wi % B == 0:
            cache = {}                                                     # cleared after every fbank batch (:632-640)
        for s in range(S):
            out["evaluated"] += 1
            if not base_sum[wi, s] > 0 or clean_sum[wi, s] < min_active:
                out["empty"] += 1
                continue
            use_clean = clean_sum[wi, s] >= f32(min_frames)
            if not use_clean:
                out["fallback"] += 1
            mask = clean[wi, s] if use_clean else base[wi, s]
            if not (e_clean[wi, s] if use_clean else e_base[wi, s]) > 0:
                out["empty"] += 1
                continue
            job = len(out["records"])
            hit = cfg.skip_threshold is not None and s in cache and cosine(mask, cache[s][0]) >= f32(cfg.skip_threshold)
            if hit:
                out["run_of_job"].append(cache[s][1])
                out["skipped"] += 1
            else:
                run = len(out["window_of_run"])
                out["window_of_run"].append(wi)
                out["run_rows"].append(resample(mask, W))
                out["run_of_job"].append(run)
                if cfg.skip_threshold is not None:
                    cache[s] = (mask, run)
            act = np.nonzero(mask > thr)[0]
            first = int(act[0]) if act.size else 0
            last = int(act[-1]) if act.size else first
            out["records"].append((c, s, first, last, off + float(first) * fd, off + float(last + 1) * fd))
            out["mask_rows"].append(mask.copy())
            assert job == len(out["run_of_job"]) - 1
    return _arrays(out, F, W)


def _arrays(out, F, W):
    out["run_of_job"] = np.asarray(out["run_of_job"], np.int32)
    out["window_of_run"] = np.asarray(out["window_of_run"], np.int32)
    out["run_rows"] = np.asarray(out["run_rows"], f32).reshape(-1, W)
    out["mask_rows"] = np.asarray(out["mask_rows"], f32).reshape(-1, F)
    return out


def windows(audio, starts, spw):
    """audio[start : start + spw] then zeros, per start."""
    a = np.asarray(audio, f32)
    out = np.zeros((len(starts), spw), f32)
    for i, s in enumerate(starts):
        seg = a[s:s + spw]
        out[i, :seg.size] = seg
    return out


def span_inputs(audio, spans, cfg: Config):
    """embedSpan (:243-297): (windows, weights, ok) per span."""
    a = np.asarray(audio, f32)
    spw, W, total = cfg.spw, cfg.weight_frames, a.size
    win, wts, ok = np.zeros((len(spans), spw), f32), np.zeros((len(spans), W), f32), np.zeros(len(spans), bool)
    for i, (t0, t1) in enumerate(spans):
        if not (math.isfinite(t0) and math.isfinite(t1)):     # the library refuses the span (the reference traps in Int(...))
            continue
        s = max(0, int(round_half_away(t0 * cfg.sample_rate)))
        e = min(total, int(round_half_away(t1 * cfg.sample_rate)))
        n = min(e - s, spw)
        if n <= 0:
            continue
        ok[i] = True
        win[i, :n] = a[s:s + n]
        k = max(1, min(W, int(round_half_away(float(n) / float(spw) * float(W)))))
        wts[i, :k] = 1
    return win, wts, ok
