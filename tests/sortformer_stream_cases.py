"""The shared cases of the streaming Sortformer state: a geometry, a seed, a pred distribution and a chunk count each, with the operands of
every step for every stream — what the CPU test proves to contain every decision kind is exactly what the GPU test runs.  The operands
depend on the state's lengths only (never on a log), so they are generated once, by a length tracker."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import sortformer_stream_restatement as R

F = np.float32

GEOMETRIES = {
    # speakers, spkcache, fifo, chunk, lc, rc, period, sil, d_model, streams, steps
    "small": (4, 32, 5, 3, 1, 2, 4, 3, 24, 5, 40),
    "small_s2": (2, 32, 5, 3, 1, 2, 4, 3, 24, 5, 40),
    "small_s3": (3, 32, 5, 3, 1, 2, 4, 3, 24, 5, 40),
    "default": (4, 188, 40, 6, 1, 7, 31, 3, 512, 3, 60),
    "high_latency": (4, 188, 40, 340, 1, 40, 300, 3, 64, 2, 4),
}


def geometry(name) -> R.Config:
    S, cache, fifo, chunk, lc, rc, period, sil, d, _, _ = GEOMETRIES[name]
    return R.Config(speakers=S, d_model=d, chunk_len=chunk, chunk_left_context=lc, chunk_right_context=rc, fifo_len=fifo, spkcache_len=cache,
                    spkcache_update_period=period, sil_frames_per_spk=sil)


@dataclass(frozen=True)
class Case:
    geometry: str
    seed: int
    dist: str        # uniform | eighths | sparse
    f16: bool = False

    @property
    def name(self):
        return f"{self.geometry}-{self.dist}-{self.seed}" + ("-f16" if self.f16 else "")

    @property
    def streams(self):
        return GEOMETRIES[self.geometry][9]

    @property
    def steps(self):
        return GEOMETRIES[self.geometry][10]


CASES = [Case("small", 1, "uniform"), Case("small", 2, "eighths"), Case("small", 3, "sparse"), Case("small_s2", 4, "eighths"), Case("small_s3", 5, "sparse"),
         Case("default", 6, "eighths"), Case("default", 7, "sparse", f16=True), Case("high_latency", 8, "uniform")]

REFUSALS = (R.SHORT_PREDS_FIFO, R.SHORT_CHUNK, R.SHORT_PREDS_CHUNK, R.SHORT_PREDS_TENTATIVE, R.NEGATIVE_CORE, R.BAD_PRED, R.BAD_OPERAND)


def draw_preds(rng, dist, rows, S):
    if dist == "uniform":
        return rng.random((rows, S), dtype=F)
    if dist == "eighths":   # multiples of 1/8: scores tie exactly
        return (rng.integers(0, 9, (rows, S)) / 8).astype(F)
    p = (rng.random((rows, S), dtype=F) * F(0.3)).astype(F)   # sparse: mostly below 0.3, 15 % of the rows at 0.9 for one speaker; a few silent rows
    loud = rng.random(rows) < 0.15
    p[loud, rng.integers(0, S, int(loud.sum()))] = F(0.9)
    p[rng.random(rows) < 0.1] = F(0.03)
    return p


@dataclass
class Step:
    chunk: np.ndarray       # [B, max_chunk_frames, d_model] float32 (exact in fp16)
    emb_len: np.ndarray     # [B]
    preds: np.ndarray       # [B, pred_stride, S]
    pred_rows: np.ndarray
    left: np.ndarray
    right: np.ndarray
    active: np.ndarray
    expect: np.ndarray      # [B] the status every stream must report


def pred_stride(cfg: R.Config):
    return cfg.spkcache_len + cfg.fifo_len + cfg.max_chunk_frames


def operands(case: Case):
    """Every step's operands.  Streams are staggered (stream b starts at step b and rests every fifth step of its own), so that one call holds
    streams that only append, that pop and that compress; one refusal of every kind is injected per case where the state allows it."""
    cfg = geometry(case.geometry)
    B, S, D, M = case.streams, cfg.speakers, cfg.d_model, cfg.max_chunk_frames
    rng = np.random.default_rng(case.seed)
    spk, fifo, present, chunks = [0] * B, [0] * B, [False] * B, [0] * B
    stride = pred_stride(cfg)
    pending = list(REFUSALS)
    steps = []
    for t in range(case.steps):
        st = Step(np.zeros((B, M, D), F), np.zeros(B, np.int32), np.zeros((B, stride, S), F), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32),
                  np.zeros(B, np.int32), np.zeros(B, np.int32))
        for b in range(B):
            st.active[b] = 1 if t >= b and (t + b) % 5 != 4 else 0
            if not st.active[b]:
                st.expect[b] = R.INACTIVE
                # an inactive stream's operands are garbage on purpose
                st.emb_len[b], st.pred_rows[b], st.left[b], st.right[b] = -7, -7, -7, -7
                continue
            lc, rc = (cfg.chunk_left_context if chunks[b] > 0 else 0), cfg.chunk_right_context
            emb_len = lc + cfg.chunk_len + rc
            rows = spk[b] + fifo[b] + emb_len
            st.chunk[b, :emb_len] = rng.integers(-256, 257, (emb_len, D)).astype(F) / F(64)
            st.preds[b, :rows] = draw_preds(rng, case.dist, rows, S)
            st.emb_len[b], st.pred_rows[b], st.left[b], st.right[b] = emb_len, rows, lc, rc
            # a refusal: the last stream, every third step from the sixth on, while kinds are left
            if b == B - 1 and t >= 6 and t % 3 == 0 and pending and (pending[0] != R.SHORT_PREDS_FIFO or fifo[b] > 0):
                kind = pending.pop(0)
                st.expect[b] = kind
                if kind == R.SHORT_PREDS_FIFO:
                    st.pred_rows[b] = spk[b] + fifo[b] - 1
                elif kind == R.SHORT_CHUNK:
                    st.right[b] = -1
                elif kind == R.SHORT_PREDS_CHUNK:
                    st.pred_rows[b] = rows - rc - 1
                elif kind == R.SHORT_PREDS_TENTATIVE:
                    st.pred_rows[b] = rows - 1
                elif kind == R.NEGATIVE_CORE:
                    st.left[b] = emb_len
                elif kind == R.BAD_PRED:
                    st.preds[b, spk[b] + fifo[b] + lc + 1, S - 1] = np.nan if t % 2 else F(1.5)
                else:
                    st.emb_len[b] = M + 1
                continue
            st.expect[b] = R.OK
            chunks[b] += 1
            context = cfg.chunk_len + fifo[b]
            fifo[b] = context
            if context > cfg.fifo_len:
                pop = R.pop_out_length(cfg, context)
                fifo[b] = context - pop
                spk[b] += pop
                if spk[b] > cfg.spkcache_len:
                    spk[b], present[b] = cfg.spkcache_len, True
        steps.append(st)
    return cfg, steps


def stream_view(step: Step, b: int):
    """Stream b's operands as the restatement takes them: (chunk rows, preds rows, lc, rc), or None when it is inactive."""
    if not step.active[b]:
        return None
    return step.chunk[b, :max(int(step.emb_len[b]), 0)], step.preds[b, :max(int(step.pred_rows[b]), 0)], int(step.left[b]), int(step.right[b])


def advance(cfg, state: R.State, step: Step, b: int, log_scores=None):
    """One step of stream b on the restatement: (status, confirmed, tentative, base scores or None).  A refusal leaves the state unchanged."""
    v = stream_view(step, b)
    if v is None:
        return R.INACTIVE, None, None, None
    chunk, preds, lc, rc = v
    try:
        if step.emb_len[b] > cfg.max_chunk_frames or step.emb_len[b] < 0:
            raise R.Refused(R.BAD_OPERAND)
        conf, tent, base = R.streaming_update(cfg, state, chunk, preds, lc, rc, log_scores)
    except R.Refused as e:
        R.BRANCHES[f"refused_{e.status}"] += 1
        return e.status, None, None, None
    return R.OK, conf, tent, base
