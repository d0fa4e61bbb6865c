"""numpy restatement of the powerset decode, the chunk assignments and OfflineReconstruction (reference:
Sources/FluidAudio/Diarizer/Offline/Segmentation/OfflineSegmentationProcessor.swift:316-409,
Sources/FluidAudio/Diarizer/Offline/Core/OfflineDiarizerManager.swift:885-911,
Sources/FluidAudio/Diarizer/Offline/Utils/OfflineReconstruction.swift:24-496,
Sources/FluidAudio/Diarizer/Offline/Utils/ZeroVoteReembedder.swift:42-130).  Test infrastructure, like vbx_shard_numpy.py: it lives
outside oracle/ and is never imported by the product.

Every fp64 sum is sequential in the reference's order (np.add.at in index order, np.cumsum(...)[-1]); np.sum is never used.  The
one rule the reference leaves open: raw segments closing at the same frame (and those flushed after the last frame, which close at
frame totalFrames) are taken in increasing cluster index — the reference appends them in Dictionary order, which is hash-seeded."""
from __future__ import annotations

import numpy as np

POWERSET = [[], [0], [1], [2], [0, 1], [0, 2], [1, 2], [0, 1, 2]]   # OfflineSegmentationProcessor.swift:15-24

DEFAULTS = dict(window_duration=10.0, min_duration_on=0.0, min_duration_off=0.0, min_segment_duration=1.0, min_gap_duration=0.1,
                exclusive=True, zero_vote_min_duration=0.4)   # OfflineDiarizerTypes.swift:46-55, 97-103, 204-214, 232-247


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def powerset_decode(logits):
    """(weights [C, F, 3] fp32, log-probs [C, F, classes] fp64) — :316-409.  bestIndex = first strict maximum seeded at
    -Float.greatestFiniteMagnitude (:326-335); log-probs = logits - logSumExp (VDSPOperations.swift:142-155), here in fp64."""
    x = np.asarray(logits, np.float32)
    nc, nf, k = x.shape
    best = np.zeros((nc, nf), np.int64)
    bv = np.full((nc, nf), -np.finfo(np.float32).max, np.float32)
    for c in range(k):
        better = x[:, :, c] > bv
        best[better] = c
        bv[better] = x[:, :, c][better]
    w = np.zeros((nc, nf, 3), np.float32)
    win = np.minimum(best, len(POWERSET) - 1)
    for cls, spk in enumerate(POWERSET):
        for s in spk:
            w[:, :, s][win == cls] = 1.0
    xd = x.astype(np.float64)
    with np.errstate(invalid="ignore"):   # rows holding NaN / -inf: their log-probs are not compared
        m = xd.max(axis=2, keepdims=True)
        lse = np.log(np.exp(xd - m).sum(axis=2, keepdims=True)) + m
        return w, xd - lse


def chunk_assignments(chunk_idx, speaker_idx, labels, K, C, S):
    """buildChunkAssignments (OfflineDiarizerManager.swift:885-911)."""
    hard = np.full((C, S), -2, np.int32)
    for c, s, k in zip(np.asarray(chunk_idx).tolist(), np.asarray(speaker_idx).tolist(), np.asarray(labels).tolist()):
        if 0 <= c < C and 0 <= s < S and 0 <= k < K:
            hard[c, s] = k
    return hard


def chunk_starts(C, offsets, window):
    """chunkStartTime (:498-507)."""
    off = np.asarray([] if offsets is None else offsets, np.float64)
    st = np.arange(C, dtype=np.float64) * window
    n = min(off.size, C)
    st[:n] = off[:n]
    return st


def global_frames(start, F, fd, T):
    """:69-77: frameStart = offset + Double(f) * fd (two roundings, no FMA), rounded half away from zero, clamped."""
    fs = start + np.arange(F, dtype=np.float64) * fd
    q = fs / fd
    frac = q - np.trunc(q)                   # exact; floor(q + 0.5) would round q just below x.5 up
    r = np.where(np.abs(frac) == 0.5, np.trunc(q) + np.sign(q), np.where(np.abs(frac) < 0.5, np.trunc(q), np.trunc(q) + np.sign(q)))
    return np.clip(r, 0, T - 1).astype(np.int64)


def frame_stats(weights, hard, K, offsets=None, frame_duration=0.0, window=10.0):
    """:35-156 -> dict(T, fd, sums [T, Kc], counts [T, Kc], averages, speaker_count [T]); None for an empty input (:30-33)."""
    w = np.asarray(weights, np.float32)
    C, F, S = w.shape
    if C == 0 or F == 0:
        return None
    fd = frame_duration if frame_duration > 0 else window / F
    if not fd > 0:
        return None
    Kc = max(K, 1)
    starts = chunk_starts(C, offsets, window)
    max_time = 0.0
    for c in range(C):
        e = starts[c] + float(F) * fd
        if e > max_time:
            max_time = e
    T = max(1, int(np.ceil(max_time / fd)))
    sums = np.zeros((T, Kc))
    counts = np.zeros((T, Kc))
    exp_sum = np.zeros(T)
    exp_w = np.zeros(T)
    hard = np.asarray(hard, np.int64).reshape(C, S)
    wd = w.astype(np.float64)
    for c in range(C):
        g = global_frames(starts[c], F, fd, T)
        act = np.zeros((F, Kc))
        for s in range(S):
            k = hard[c, s]
            if 0 <= k < Kc:
                act[:, k] = np.where(wd[c, :, s] > act[:, k], wd[c, :, s], act[:, k])
        e = np.zeros(F)
        for s in range(S):
            e = e + wd[c, :, s]
        np.add.at(exp_sum, g, e)
        np.add.at(exp_w, g, 1.0)
        np.add.at(sums, g, act)              # a zero activation adds +0.0: the sum is unchanged (:96-101 adds only > 0)
        np.add.at(counts, g, (act > 0).astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.where(counts > 0, sums / np.where(counts > 0, counts, 1), 0.0)
    maxc = min(Kc, S)
    cnt = np.zeros(T, np.int64)
    ok = exp_w > 0
    cnt[ok] = np.clip(np.rint(exp_sum[ok] / exp_w[ok]), 0, maxc).astype(np.int64)
    return dict(T=T, fd=fd, Kc=Kc, S=S, sums=sums, counts=counts, averages=avg, speaker_count=cnt, expected_sums=exp_sum)


def select_clusters(st):
    """:167-174: the first `count` clusters by activation sum descending, ties to the lower index.  [T][<= S] lists."""
    sums = st["sums"].copy()
    cnt = st["speaker_count"]
    T = sums.shape[0]
    sel = [[] for _ in range(T)]
    work = sums.copy()
    for r in range(int(cnt.max()) if T else 0):
        rows = np.nonzero(cnt > r)[0]
        k = np.argmax(work[rows], axis=1)        # first maximum: the lower index wins ties
        work[rows, k] = -1.0
        for g, kk in zip(rows.tolist(), k.tolist()):
            sel[g].append(kk)
    return sel


def detect_runs(speaker_count, sums, fd, min_duration):
    """ZeroVoteReembedder.detectRuns (ZeroVoteReembedder.swift:42-79): [(lo, hi)]."""
    if not fd > 0:
        return []
    n = min(len(speaker_count), len(sums))
    runs, start = [], None
    for g in range(n):
        zero = speaker_count[g] == 1 and all(v == 0 for v in sums[g])
        if zero:
            if start is None:
                start = g
        elif start is not None:
            runs.append((start, g))
            start = None
    if start is not None:
        runs.append((start, n))
    return [(a, b) for a, b in runs if float(b - a) * fd >= min_duration]


def zero_vote_assignment(embedding, centroids):
    """ZeroVoteReembedder.assignment (:90-130)."""
    if embedding is None or len(embedding) == 0 or len(centroids) == 0:
        return None
    e = [float(v) for v in embedding]
    if not all(np.isfinite(e)):
        return None
    best, bc = -1, -np.inf
    for i, c in enumerate(centroids):
        if len(c) != len(e):
            return None
        dot = na = nb = 0.0
        for x, y in zip(e, c):
            dot += x * float(y)
            na += x * x
            nb += float(y) * float(y)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = float(np.float64(dot) / np.sqrt(np.float64(na * nb)))
        if not np.isfinite(cos):
            return None
        if cos > bc:
            bc, best = cos, i
    return best if best >= 0 else None


def apply_overrides(sel, overrides):
    """perFrameClusters[frame] = [cluster] for every override run, in order (:284-286)."""
    sel = [list(s) for s in sel]
    for lo, hi, k in overrides:
        for g in range(lo, hi):
            sel[g] = [k]
    return sel


def frame_records(st, sel):
    """The per-frame decision as the library reports it (fa_reconstruct_info): clusters [T, slots] by rank, -1 past them, and their
    fp64 averages, 0 past them.  slots = max(min(Kc, S), 1)."""
    T = st["T"]
    slots = max(min(st["Kc"], st["S"]), 1)
    cl = np.full((T, slots), -1, np.int32)
    av = np.zeros((T, slots))
    for g, ks in enumerate(sel):
        for j, k in enumerate(ks):
            cl[g, j] = k
            av[g, j] = st["averages"][g, k]
    return cl, av


def raw_segments(st, sel, overrides=()):
    """The segment walk (:188-233) + appendSegment (:400-429): [(speaker_id, start f32, end f32, quality f32)] in the declared raw
    order (closing frame, cluster).  overrides: (lo, hi, cluster) applied in order (:284-286)."""
    T, fd, avg = st["T"], st["fd"], st["averages"]
    sel = apply_overrides(sel, overrides)
    per_k = {}
    for g, ks in enumerate(sel):
        for k in ks:
            per_k.setdefault(k, []).append(g)
    recs = []
    for k, frames in per_k.items():
        fr = np.asarray(frames)
        brk = np.nonzero(np.diff(fr) != 1)[0]
        lo_i = np.concatenate([[0], brk + 1])
        hi_i = np.concatenate([brk, [fr.size - 1]])
        for a, b in zip(lo_i.tolist(), hi_i.tolist()):
            g0, g_last = int(fr[a]), int(fr[b])
            g1 = g_last + 1
            score = np.cumsum(avg[g0:g1, k])[-1]
            start = float(g0) * fd
            end = float(g1) * fd if g1 < T else float(g_last) * fd + fd
            if not end > start:
                continue
            q = np.float32(min(max(score / float(g1 - g0), 0.0), 1.0))
            recs.append((g1, k, (f"S{k + 1}", np.float32(start), np.float32(end), q)))
    recs.sort(key=lambda r: (r[0], r[1]))
    return [r[2] for r in recs]


def _blend(a, b):
    """blendedQuality (:465-479)."""
    ld, rd = float(np.float32(a[2] - a[1])), float(np.float32(b[2] - b[1]))
    tot = ld + rd
    if not tot > 0:
        return np.float32(min(max((a[3] + b[3]) / np.float32(2), np.float32(0)), np.float32(1)))
    return np.float32(min(max((float(a[3]) * ld + float(b[3]) * rd) / tot, 0.0), 1.0))


def finalize(raw, cfg):
    """mergeSegments (:431-463) -> sanitize (:481-496) -> excludeOverlaps (:359-398).  Segments: (id, start, end, quality) fp32."""
    merged = []
    if raw:
        gap = max(cfg["min_gap_duration"], cfg["min_duration_off"])
        srt = sorted(raw, key=lambda s: s[1])            # Python's sort is stable, like Swift's
        cur = srt[0]
        for s in srt[1:]:
            if s[0] == cur[0] and float(s[1]) - float(cur[2]) <= gap:
                cur = (cur[0], cur[1], max(cur[2], s[2]), _blend(cur, s))
                continue
            merged.append(cur)
            cur = s
        merged.append(cur)
    merged = sorted(merged, key=lambda s: s[1])
    mind = max(np.float32(cfg["min_segment_duration"]), np.float32(cfg["min_duration_on"]))
    kept = [s for s in merged if np.float32(s[2] - s[1]) >= mind]
    if not cfg["exclusive"]:
        return kept
    out = []
    mseg = np.float32(cfg["min_segment_duration"])
    for s in kept:
        start, end = s[1], s[2]
        if out and start < out[-1][2]:
            start = out[-1][2]
        if start >= end:
            continue
        dur = np.float32(end - start)
        if dur < mseg:
            continue
        orig = np.float32(s[2] - s[1])
        scale = np.float32(dur / orig) if orig > 0 else np.float32(1)
        out.append((s[0], start, end, np.float32(max(np.float32(0), min(np.float32(1), np.float32(s[3] * scale))))))
    return out


def build_segments(weights, hard, centroids, offsets=None, frame_duration=0.0, cfg=None, span_embedder=None, zero_vote=False,
                   overrides=None, return_state=False):
    """buildSegments (:24-237).  centroids: [K][d] (K = len); span_embedder(start_s, end_s) -> embedding or None.  overrides: explicit
    (lo, hi, cluster) list instead of the re-embed pass."""
    cfg = cfg or config()
    K = len(centroids)
    st = frame_stats(weights, hard, K, offsets, frame_duration, cfg["window_duration"])
    if st is None:
        return ([], None) if return_state else []
    sel = select_clusters(st)
    ov = list(overrides or [])
    runs = []
    if zero_vote and span_embedder is not None and K > 0:
        runs = detect_runs(st["speaker_count"], st["sums"], st["fd"], cfg["zero_vote_min_duration"])
        for lo, hi in runs:
            emb = span_embedder(float(lo) * st["fd"], float(hi) * st["fd"])
            a = zero_vote_assignment(emb, centroids) if emb is not None else None
            if a is not None:
                ov.append((lo, hi, a))
    raw = raw_segments(st, sel, ov)
    segs = finalize(raw, cfg)
    if return_state:
        st = dict(st, raw=raw, runs=runs, selected=sel, final=apply_overrides(sel, ov))
        return segs, st
    return segs


def speaker_database(segments, centroids):
    """buildSpeakerDatabase (:300-357)."""
    cen = np.asarray(centroids, np.float64)
    dim = cen.shape[1] if cen.ndim == 2 and cen.shape[0] else 0
    sums, counts = {}, {}
    for s in segments:
        k = int(s[0][1:]) - 1
        e = cen[k].astype(np.float32) if 0 <= k < cen.shape[0] else np.zeros(dim, np.float32)
        sums[s[0]] = e.copy() if s[0] not in sums else (sums[s[0]] + e).astype(np.float32)
        counts[s[0]] = counts.get(s[0], 0) + 1
    return {k: (v * (np.float32(1) / np.float32(counts[k]))).astype(np.float32) for k, v in sums.items()}


def session_logits(n_chunks, seed=7, F=589):
    """Seeded segmentation logits of a long session (input generator of the full-size tests and scripts/reconstruct_timing.py):
    per chunk, runs of one powerset class lasting 0.5-3 s (30-177 frames of 10/589 s), +4 on that class over N(0, 1) noise."""
    rng = np.random.default_rng(seed)
    cls = np.empty((n_chunks, F), np.int64)
    for c in range(n_chunks):
        f = 0
        while f < F:
            d = int(rng.integers(30, 178))
            cls[c, f:f + d] = rng.choice(7, p=[0.15, 0.25, 0.2, 0.2, 0.1, 0.05, 0.05])
            f += d
    x = rng.standard_normal((n_chunks, F, 7)).astype(np.float32)
    np.put_along_axis(x, cls[:, :, None], np.take_along_axis(x, cls[:, :, None], 2) + 4.0, 2)
    return x
