"""A line-by-line numpy restatement of streaming Sortformer's state (reference: Sources/FluidAudio/Diarizer/Sortformer/
SortformerStateUpdater.swift:31-578, SortformerTypes.swift:219-255, 264-385, SortformerDiarizer.swift:933-979).  Every fp32 operation is a
numpy float32 operation in the reference's order, unfused; the two insertion loops are kept as they are.  The logs are numpy's: `compress`
takes `log_scores` to replace them, since no two fp32 log implementations agree to the last bit.  `log_scores_f64` is the yardstick for
the base scores, `log_scores_f32` a float32 emulation in the device's operation order.  BRANCHES counts the decision kinds a run took."""
from __future__ import annotations

import collections
import struct
from dataclasses import dataclass, field

import numpy as np

F = np.float32
LN2 = np.frombuffer(struct.pack("<I", 0x3F317218), np.float32)[0]   # logf(2) as the fp32 literal
NEG_INF, POS_INF = F(-np.inf), F(np.inf)
BRANCHES = collections.Counter()

OK, INACTIVE, SHORT_PREDS_FIFO, SHORT_CHUNK, SHORT_PREDS_CHUNK, SHORT_PREDS_TENTATIVE, NEGATIVE_CORE, BAD_PRED, BAD_OPERAND = range(9)


def trunc_product(x: int, rate) -> int:
    """Int(Float(x) * rate)"""
    return int(F(x) * F(rate))


@dataclass
class Config:  # SortformerConfig with its clamps (:239-254)
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

    def __post_init__(self):
        self.chunk_len = max(1, self.chunk_len)
        self.spkcache_len = max(self.spkcache_len, (1 + self.sil_frames_per_spk) * self.speakers)
        self.spkcache_update_period = max(min(self.spkcache_update_period, self.fifo_len + self.chunk_len), self.chunk_len)
        if self.max_chunk_frames == 0:
            self.max_chunk_frames = self.chunk_len + self.chunk_left_context + self.chunk_right_context

    # :229-232
    @property
    def len_per_spk(self):
        return self.spkcache_len // self.speakers - self.sil_frames_per_spk

    def quotas(self):
        n = self.len_per_spk
        return n, trunc_product(n, self.strong_boost_rate), trunc_product(n, self.weak_boost_rate), trunc_product(n, self.min_pos_scores_rate)

    @property
    def max_pop(self):
        return min(max(self.spkcache_update_period, self.max_chunk_frames), self.fifo_len + self.max_chunk_frames)

    @property
    def score_rows(self):
        return self.spkcache_len + self.max_pop


def pop_out_length(cfg: Config, context: int) -> int:   # :119-121
    return min(max(cfg.spkcache_update_period, context - cfg.fifo_len), context)


@dataclass
class State:  # SortformerStreamingState: rows as arrays [n, d_model] / [n, speakers]; None is the reference's nil
    d_model: int
    speakers: int
    spkcache: np.ndarray = None
    spkcache_preds: np.ndarray | None = None
    fifo: np.ndarray = None
    fifo_preds: np.ndarray | None = None
    mean_silence: np.ndarray = None
    silence_frame_count: int = 0

    def __post_init__(self):
        if self.spkcache is None:
            self.spkcache = np.zeros((0, self.d_model), F)
        if self.fifo is None:
            self.fifo = np.zeros((0, self.d_model), F)
        if self.mean_silence is None:
            self.mean_silence = np.zeros(self.d_model, F)

    @property
    def spkcache_length(self):
        return len(self.spkcache)

    @property
    def fifo_length(self):
        return len(self.fifo)

    def copy(self):
        return State(self.d_model, self.speakers, self.spkcache.copy(), None if self.spkcache_preds is None else self.spkcache_preds.copy(), self.fifo.copy(),
                     None if self.fifo_preds is None else self.fifo_preds.copy(), self.mean_silence.copy(), self.silence_frame_count)


class Refused(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


# ---- the scores
def log_scores_f64(cfg: Config, preds) -> np.ndarray:
    """The yardstick: getLogPredScores in float64 on the float32 preds (the clip bounds are the reference's float32 values)."""
    p = np.asarray(preds, F).astype(np.float64)
    thr = np.float64(F(cfg.pred_score_threshold))
    hi = np.float64(F(1) - F(cfg.pred_score_threshold))
    l = np.log1p(-np.clip(p, 0.0, hi))
    return np.log(np.maximum(p, thr)) - l + np.float64(LN2) + l.sum(axis=1, keepdims=True)


def log_scores_f32(cfg: Config, preds) -> np.ndarray:
    """getLogPredScores (:311-348) in float32 with numpy's logs, in the device's (= the reference's) operation order."""
    p = np.asarray(preds, F)
    thr = F(cfg.pred_score_threshold)
    s = np.log(np.minimum(np.maximum(p, thr), np.finfo(F).max)).astype(F)
    l = np.log1p(-np.minimum(np.maximum(p, F(0)), F(1) - thr)).astype(F)
    s = (s - l).astype(F)
    s = (LN2 + s).astype(F)
    total = np.zeros(len(p), F)
    for spk in range(p.shape[1]):
        total = (total + l[:, spk]).astype(F)
    return (s + total[:, None]).astype(F)


def disable_low_scores(cfg, preds, scores, min_pos):   # :351-390
    S = preds.shape[1]
    result = scores.copy()
    pos = [int(np.sum((preds[:, spk] > F(0.5)) & (scores[:, spk] > 0))) for spk in range(S)]
    for spk in range(S):
        for frame in range(len(preds)):
            if preds[frame, spk] <= F(0.5):
                result[frame, spk] = NEG_INF
                continue
            if result[frame, spk] <= 0 and pos[spk] >= min_pos:
                result[frame, spk] = NEG_INF
                BRANCHES["quota_disabled"] += 1
    return result


def boost_insertion(column, k_eff):
    """The insertion loop of boostTopKScores (:412-446) for one speaker column: the frames it boosts."""
    top_frames, top_scores, count = [0] * k_eff, [-np.finfo(F).max] * k_eff, 0
    candidates = 0
    for frame, v in enumerate(column):
        if v == NEG_INF:
            continue
        candidates += 1
        if count < k_eff:
            pos = count
            while pos > 0 and v > top_scores[pos - 1]:
                top_scores[pos], top_frames[pos] = top_scores[pos - 1], top_frames[pos - 1]
                pos -= 1
            top_scores[pos], top_frames[pos] = v, frame
            count += 1
        else:
            if v <= top_scores[count - 1]:
                continue
            pos = count - 1
            while pos > 0 and v > top_scores[pos - 1]:
                top_scores[pos], top_frames[pos] = top_scores[pos - 1], top_frames[pos - 1]
                pos -= 1
            top_scores[pos], top_frames[pos] = v, frame
    if candidates > k_eff:
        BRANCHES["boost_cuts"] += 1
    return top_frames[:count]


def boost_rank_order(column, k_eff):
    """The stated order: the first min(k_eff, finite ones) frames by (score descending, frame ascending)."""
    live = [f for f, v in enumerate(column) if v != NEG_INF]
    return sorted(live, key=lambda f: (-float(column[f]), f))[:k_eff]


def boost_top_k(scores, k, scale):   # :393-457
    frames, S = scores.shape
    if frames <= 0 or S <= 0 or k <= 0:
        return scores
    delta = F(F(scale) * LN2)   # -scaleFactor * logf(0.5)
    result = scores.copy()
    k_eff = min(k, frames)
    for spk in range(S):
        for frame in boost_insertion(result[:, spk].copy(), k_eff):
            result[frame, spk] = F(result[frame, spk] + delta)
    return result


def topk_insertion(scores, frame_count, k):
    """The insertion loop of getTopKIndices (:486-541): (bestIdx, bestVal) in its kept order."""
    S = scores.shape[1]
    N = frame_count * S
    k_eff = min(k, N)
    best_idx, best_val, count = [0] * k_eff, [NEG_INF] * k_eff, 0
    for spk in range(S):
        for frame in range(frame_count):
            pi, v = spk * frame_count + frame, scores[frame, spk]
            if count < k_eff:
                pos = count
                while pos > 0:
                    pv, pidx = best_val[pos - 1], best_idx[pos - 1]
                    if v > pv or (v == pv and pi < pidx):
                        best_val[pos], best_idx[pos] = pv, pidx
                        pos -= 1
                    else:
                        break
                best_val[pos], best_idx[pos] = v, pi
                count += 1
            else:
                wv, wi = best_val[k_eff - 1], best_idx[k_eff - 1]
                if v < wv or (v == wv and pi >= wi):
                    if v == wv and np.isfinite(v):
                        BRANCHES["tie_at_cut"] += 1
                    continue
                pos = k_eff - 1
                while pos > 0:
                    pv, pidx = best_val[pos - 1], best_idx[pos - 1]
                    if v > pv or (v == pv and pi < pidx):
                        best_val[pos], best_idx[pos] = pv, pidx
                        pos -= 1
                    else:
                        break
                best_val[pos], best_idx[pos] = v, pi
    return best_idx, best_val


def topk_rank_order(scores, frame_count, k):
    """The stated order: the first min(k, N) permuted indices by (score descending, permuted index ascending)."""
    S = scores.shape[1]
    keys = [(-float(scores[f, s]), s * frame_count + f) for s in range(S) for f in range(frame_count)]
    keys.sort()
    keys = keys[:min(k, len(keys))]
    return [pi for _, pi in keys], [F(-v) for v, _ in keys]


def get_top_k_indices(cfg, scores, frame_count, k):   # :465-578
    if k <= 0:
        return [], []
    no_sil = frame_count - cfg.sil_frames_per_spk
    best_idx, best_val = topk_insertion(scores, frame_count, k)
    top = [cfg.max_index] * k
    for i in range(len(best_idx)):
        top[i] = cfg.max_index if best_val[i] == NEG_INF else best_idx[i]
        if best_val[i] == NEG_INF:
            BRANCHES["neg_inf_selected"] += 1
    top.sort()
    disabled = [t == cfg.max_index for t in top]
    for i in range(k):
        if not disabled[i]:
            top[i] %= frame_count
    for i in range(k):
        if not disabled[i] and top[i] >= no_sil:
            disabled[i] = True
    for i in range(k):
        if disabled[i]:
            top[i] = 0
    return top, disabled


def compress(cfg: Config, state: State, log_scores=None):   # :220-305
    if state.spkcache_preds is None:
        return None
    preds = state.spkcache_preds
    current = state.spkcache_length
    _, strong, weak, min_pos = cfg.quotas()
    base = log_scores_f32(cfg, preds) if log_scores is None else np.asarray(log_scores, F)[:current].copy()
    scores = disable_low_scores(cfg, preds, base, min_pos)
    if current > cfg.spkcache_len:
        scores[cfg.spkcache_len:current] = (scores[cfg.spkcache_len:current] + F(cfg.scores_boost_latest)).astype(F)
    scores = boost_top_k(scores, strong, 2.0)
    scores = boost_top_k(scores, weak, 1.0)
    total = current + cfg.sil_frames_per_spk
    scores = np.concatenate([scores, np.full((cfg.sil_frames_per_spk, cfg.speakers), POS_INF, F)])
    top, disabled = get_top_k_indices(cfg, scores, total, cfg.spkcache_len)
    new_cache = np.zeros((cfg.spkcache_len, cfg.d_model), F)
    new_preds = np.zeros((cfg.spkcache_len, cfg.speakers), F)
    live = []
    for i, frame in enumerate(top):
        if disabled[i]:
            new_cache[i] = state.mean_silence
        elif frame < current:
            new_cache[i] = state.spkcache[frame]
            new_preds[i] = preds[frame]
            live.append(frame)
    if len(set(live)) < len(live):
        BRANCHES["frame_twice"] += 1
    if any(b < a for a, b in zip(live, live[1:])):
        BRANCHES["non_monotone"] += 1
    state.spkcache, state.spkcache_preds = new_cache, new_preds
    state.scored_preds = preds   # what the base scores were taken of: the tests hold them to the yardstick
    return base


def update_silence_profile(cfg, state, embs, preds):   # :175-212
    for frame in range(len(embs)):
        prob = F(0)
        for spk in range(cfg.speakers):
            prob = F(prob + preds[frame, spk])
        if prob < F(cfg.silence_threshold):
            BRANCHES["silent_frame"] += 1
            n = F(state.silence_frame_count)
            new_n = F(n + F(1))
            state.mean_silence = ((state.mean_silence * n).astype(F) + embs[frame]).astype(F) / new_n
            state.mean_silence = state.mean_silence.astype(F)
            state.silence_frame_count += 1


def validate(cfg: Config, state: State, emb_len, preds, lc, rc, pred_stride=None):
    """The reference's throws in its order (:47-92), between the library's own refusals; returns (core, chunk_start)."""
    rows = len(preds)
    if emb_len < 0 or emb_len > cfg.max_chunk_frames or lc < 0 or (pred_stride is not None and rows > pred_stride):
        raise Refused(BAD_OPERAND)
    spk, fifo = state.spkcache_length, state.fifo_length
    if fifo > 0 and spk + fifo > rows:
        raise Refused(SHORT_PREDS_FIFO)
    if rc < 0:   # (lc + coreFrames) * d <= chunk.count is rc >= 0
        raise Refused(SHORT_CHUNK)
    core = emb_len - lc - rc
    if core < 0:
        raise Refused(NEGATIVE_CORE)
    start = spk + fifo + lc
    if start + core + rc > rows:
        raise Refused(SHORT_PREDS_CHUNK if start + core > rows else SHORT_PREDS_TENTATIVE)
    context = core + fifo
    first_overflow = context > cfg.fifo_len and spk + pop_out_length(cfg, context) > cfg.spkcache_len and state.spkcache_preds is None
    read = np.concatenate([preds[spk:spk + fifo] if fifo > 0 else preds[:0], preds[start:start + core + rc], preds[:spk] if first_overflow else preds[:0]])
    if not np.all((read >= 0) & (read <= 1)):
        raise Refused(BAD_PRED)
    return core, start


def streaming_update(cfg: Config, state: State, chunk, preds, lc, rc, log_scores=None):
    """streamingUpdate (:31-165): chunk [emb_len, d_model], preds [rows, speakers].  Returns (confirmed, tentative, base scores or None);
    raises Refused with the state unchanged."""
    chunk, preds = np.asarray(chunk, F), np.asarray(preds, F)
    core, start = validate(cfg, state, len(chunk), preds, lc, rc)
    spk, fifo = state.spkcache_length, state.fifo_length
    if lc == 0:
        BRANCHES["lc_zero"] += 1
    if fifo > 0:
        state.fifo_preds = preds[spk:spk + fifo].copy()
    chunk_embs = chunk[lc:lc + core]
    chunk_preds, tentative = preds[start:start + core].copy(), preds[start + core:start + core + rc].copy()
    state.fifo = np.concatenate([state.fifo, chunk_embs])
    state.fifo_preds = chunk_preds.copy() if state.fifo_preds is None else np.concatenate([state.fifo_preds, chunk_preds])
    context = core + fifo
    base = None
    if context <= cfg.fifo_len:
        BRANCHES["append_only"] += 1
    else:
        pop = pop_out_length(cfg, context)
        pop_embs, pop_preds = state.fifo[:pop].copy(), state.fifo_preds[:pop].copy()
        update_silence_profile(cfg, state, pop_embs, pop_preds)
        state.fifo, state.fifo_preds = state.fifo[pop:], state.fifo_preds[pop:]
        state.spkcache = np.concatenate([state.spkcache, pop_embs])
        if state.spkcache_preds is not None:
            state.spkcache_preds = np.concatenate([state.spkcache_preds, pop_preds])
        if state.spkcache_length > cfg.spkcache_len:
            if state.spkcache_preds is None:
                BRANCHES["first_overflow_nonempty" if spk > 0 else "first_overflow_empty"] += 1
                state.spkcache_preds = np.concatenate([preds[:spk], pop_preds]) if spk > 0 else pop_preds
            else:
                BRANCHES["later_compression"] += 1
            base = compress(cfg, state, log_scores)
        else:
            BRANCHES["pop_no_overflow"] += 1
    return chunk_preds, tentative, base


# ---- the chunk geometry
@dataclass
class Chunk:
    ready: int = 0
    chunk_length: int = 0
    left_offset: int = 0
    right_offset: int = 0
    start_frame: int = 0
    rows: int = 0
    new_start_feat: int = 0
    frames_to_drop: int = 0

    def tuple(self):
        return (self.ready, self.chunk_length, self.left_offset, self.right_offset, self.start_frame, self.rows, self.new_start_feat, self.frames_to_drop)


def next_chunk_features(cfg: Config, feat_length: int, start_feat: int) -> Chunk:
    """getNextChunkFeaturesLocked (SortformerDiarizer.swift:933-979) on a buffer of feat_length frames."""
    core, lcf, rcf = cfg.chunk_len * cfg.subsampling, cfg.chunk_left_context * cfg.subsampling, cfg.chunk_right_context * cfg.subsampling
    end_feat = min(start_feat + core, feat_length)
    if not end_feat > start_feat or not end_feat + rcf <= feat_length:
        return Chunk(new_start_feat=start_feat)
    left = min(lcf, start_feat)
    chunk_start, chunk_end = start_feat - left, end_feat + rcf
    start_feat = end_feat
    remove = max(0, start_feat - lcf)
    if remove > 0:
        start_feat -= remove
    return Chunk(1, chunk_end - chunk_start, left, rcf, chunk_start, chunk_end - chunk_start, start_feat, remove)


def file_chunks(cfg: Config, feat_length: int, feat_seq_length: int):
    """SortformerFeatureLoader (SortformerTypes.swift:347-383): (numChunks, every chunk next() returns)."""
    core, lcf, rcf = cfg.chunk_len * cfg.subsampling, cfg.chunk_left_context * cfg.subsampling, cfg.chunk_right_context * cfg.subsampling
    num = max(0, int((feat_length - rcf) / core))   # Swift's / truncates towards zero
    out, start = [], 0
    while True:
        end = min(start + core, feat_length)
        if not end > start or not end + rcf <= feat_length:
            break
        left = min(lcf, start)
        cs, ce = start - left, end + rcf
        out.append(Chunk(1, max(min(feat_seq_length - start + left, ce - cs), 0), left, rcf, cs, ce - cs, end, 0))
        start = end
    return num, out
