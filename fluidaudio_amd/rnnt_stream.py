"""What a Nemotron streaming session does around its networks and its decode walk (reference: Sources/FluidAudio/ASR/Parakeet/Streaming/Nemotron/
StreamingNemotronMultilingualAsrManager+Pipeline.swift:78-104, +Buffers.swift:35-63, 140-210, +BlankRescue.swift) as device-resident state batched
over streams, over the HIP C ABI (csrc/rnnt_stream.hip, csrc/rnnt_stream_host.hip, csrc/rnnt_stream_core.h): the VAD-gated skip with its
hangover, the mel cache in front of the encoder's input, and the blank-span rescue's span machine, requests and token merge.

Per chunk: gate_dev, mel_inputs_dev, the caller's encoder, rnnt_decode_logits, advance_dev, track_dev, the caller's rescue decode of the
requests, merge_rescued_dev.  Frames are int32 on the device; seconds(frames) gives the reference's Double(frame) * 0.08."""
from __future__ import annotations

import ctypes as C
import unicodedata
from dataclasses import dataclass

import numpy as np

from . import _args as A, _lib as L

RNNT_STREAM_REQUEST_DTYPE = np.dtype(L.RnntStreamRequest)
RNNT_STREAM_STATUS = ("OK", "INACTIVE", "BAD_OPERAND", "OUTPUT_TOO_SMALL", "NO_LEXICAL")   # FA_RNNT_STREAM_*
RNNT_STREAM_CLASS_LEXICAL, RNNT_STREAM_CLASS_LANG_TAG = 1, 2
SECONDS_PER_ENCODER_FRAME = 0.08                                                          # ASRConstants.secondsPerEncoderFrame
_INFO_FIELDS = [f for f, _ in L.RnntStreamInfo._fields_]


def seconds(frames) -> np.ndarray:
    """The reference's startTime of integer frames: Double(frame) * 0.08."""
    return np.asarray(frames, np.float64) * SECONDS_PER_ENCODER_FRAME


def rms(x, gate: bool = False) -> np.float32:
    """The library's host emulation of its kernels' RMS order (fa_rnnt_stream_rms): one window's, or (gate) a gated chunk's."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = C.c_float()
    st = L.lib().fa_rnnt_stream_rms(A.ptr(x) if x.size else None, x.size, int(bool(gate)), C.byref(out))
    if st != L.SUCCESS:
        raise A.invalid("fa_rnnt_stream_rms", "an array of samples")
    return np.float32(out.value)


def token_classes(pieces, lang_tag_ids=()) -> np.ndarray:
    """The class byte per vocabulary id: bit 0 where the raw piece holds a letter, mark or number (CharacterSet.alphanumerics = the Unicode
    categories L*, M*, N*: containsLexicalContent), bit 1 for the language tags.  `pieces`: a list (None: no piece) or an {id: piece} dict."""
    items = list(pieces.items()) if isinstance(pieces, dict) else list(enumerate(pieces))
    n = max([i for i, _ in items] + [int(i) for i in lang_tag_ids] + [-1]) + 1
    table = np.zeros(n, np.uint8)
    for i, piece in items:
        if piece is not None and any(unicodedata.category(ch)[0] in "LMN" for ch in piece):
            table[i] |= RNNT_STREAM_CLASS_LEXICAL
    for i in lang_tag_ids:
        table[int(i)] |= RNNT_STREAM_CLASS_LANG_TAG
    return table


@dataclass
class RnntStreamConfig:  # fa_rnnt_stream_config
    total_mel_frames: int                  # the encoder's frame axis: the caller's
    window_samples: int = 1280
    close_silent_windows: int = 2
    pre_roll_windows: int = 3
    min_speech_windows: int = 2
    max_span_samples: int = 240000
    open_slack_frames: int = 1
    close_slack_frames: int = 5
    rescue_rms_threshold: float = 0.0025
    vad_rms_threshold: float = 0.0
    vad_hangover_chunks: int = 2
    mel_features: int = 128
    pre_encode_cache: int = 9

    def c(self) -> L.RnntStreamConfig:
        return L.RnntStreamConfig(int(self.window_samples), int(self.close_silent_windows), int(self.pre_roll_windows), int(self.min_speech_windows),
                                  int(self.max_span_samples), int(self.open_slack_frames), int(self.close_slack_frames), int(self.vad_hangover_chunks),
                                  int(self.mel_features), int(self.pre_encode_cache), int(self.total_mel_frames), 0, float(self.rescue_rms_threshold),
                                  float(self.vad_rms_threshold))

    def geometry(self) -> L.RnntStreamGeometry:
        g, c = L.RnntStreamGeometry(), self.c()
        if L.lib().fa_rnnt_stream_geometry(C.byref(c), C.byref(g)) != L.SUCCESS:
            raise A.invalid("fa_rnnt_stream_geometry", "the config is refused")
        return g


@dataclass
class RnntStreamSnapshot:  # one stream's state; the fields of fa_rnnt_stream_info and the three arrays, cut to their counts
    frame_cursor: int = 0
    span_open: int = 0
    span_start_frame: int = 0
    span_last_speech_frame: int = 0
    span_speech_windows: int = 0
    span_pre_roll_frames: int = 0
    silent_window_run: int = 0
    span_overflowed: int = 0
    span_samples: int = 0
    pre_roll_samples: int = 0
    vad_consecutive_low_chunks: int = 0
    vad_skip_count: int = 0
    absolute_frame_base: int = 0
    detected_blank_spans: int = 0
    blank_rescues: int = 0
    mel_cache_frames: int = 0
    span_audio: np.ndarray = None          # float32 [span_samples]
    pre_roll: np.ndarray = None            # float32 [pre_roll_samples], oldest window first
    mel_cache: np.ndarray = None           # float32 [mel_features, mel_cache_frames]


@dataclass
class RnntStreamTracked:  # CUDA tensors; nothing has been waited for
    requests: object        # uint8 [request_capacity, 40]: fa_rnnt_stream_request records (records(): a numpy view)
    arena: object           # float32 [arena_capacity]
    request_count: object   # int32 [1]: the requests found, whatever fitted
    status: object          # int32 [streams] (finalize: [max_count])

    def records(self) -> np.ndarray:
        n = min(int(self.request_count.cpu()[0]), int(self.requests.shape[0]))
        return self.requests.cpu().numpy().reshape(-1).view(RNNT_STREAM_REQUEST_DTYPE)[:n].copy()


class RnntStreamState:
    """fa_rnnt_stream: `streams` independent streaming sessions' state on the context's device."""

    def __init__(self, streams: int, config: RnntStreamConfig, ctx: L.Context | None = None):
        self.ctx = ctx or L.default_context()
        self.config = config
        self.streams = int(streams)
        self._h = C.c_void_p()
        cfg = config.c()
        self.ctx.check(L.lib().fa_rnnt_stream_create(self.ctx.handle, C.byref(cfg), self.streams, C.byref(self._h)), "fa_rnnt_stream_create")
        self.geometry = config.geometry()

    def close(self):
        if self._h:
            L.lib().fa_rnnt_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _new(self, shape, dtype_name, zero=False):
        import torch
        return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, dtype_name), device=f"cuda:{self.ctx.device}")

    def _vec(self, t, what, n=None, optional=False, dtype="int32"):
        assert (t is None and optional) or (A.is_dev(t, dtype, 1) and (n is None or t.shape[0] == n) and t.device.index == self.ctx.device), \
            f"{what} must be a contiguous {dtype} CUDA tensor{'' if n is None else f' [{n}]'} on the context's device"

    def _chunks(self, d_chunks, what):
        assert A.is_dev(d_chunks, "float32", 2) and d_chunks.shape[0] == self.streams and d_chunks.device.index == self.ctx.device, \
            f"{what}: chunk rows must be a contiguous float32 CUDA tensor [{self.streams}, chunk_samples] on the context's device"
        return int(d_chunks.shape[1])

    # ---- the device steps: enqueued, nothing is waited for; `out` reuses an earlier call's outputs (then nothing is allocated either)
    def gate_dev(self, d_chunks, d_active=None, out=None):
        """fa_rnnt_stream_gate_dev: (rms float32 [streams], skip int32 [streams], run_list int32 [streams], run_count int32 [1], status int32 [streams])."""
        B, n = self.streams, self._chunks(d_chunks, "gate")
        self._vec(d_active, "gate: active", B, optional=True)
        out = out or (self._new((B,), "float32", True), self._new((B,), "int32", True), self._new((B,), "int32", True), self._new((1,), "int32"), self._new((B,), "int32"))
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_rnnt_stream_gate_dev(self.ctx.handle, self._h, A.ptr(d_chunks) if n else None, n, A.ptr(d_active), *[A.ptr(x) for x in out]),
                           "fa_rnnt_stream_gate_dev")
        return out

    def mel_inputs_dev(self, d_mel, d_streams, d_count, out=None):
        """fa_rnnt_stream_mel_inputs_dev: d_mel float32 [streams, mel_features, chunk_frames] with any strides; the streams of d_streams[:d_count[0]]
        -> (rows float32 [len(d_streams), mel_features, total_mel_frames], status int32 [len(d_streams)])."""
        cfg, B = self.config, self.streams
        assert A.is_dev(d_mel, "float32", 3, contiguous=False) and tuple(d_mel.shape[:2]) == (B, cfg.mel_features) and d_mel.device.index == self.ctx.device, \
            f"mel_inputs: mel must be a float32 CUDA tensor [{B}, {cfg.mel_features}, chunk_frames] on the context's device"
        self._vec(d_streams, "mel_inputs: streams")
        self._vec(d_count, "mel_inputs: count", 1)
        K, T = int(d_streams.shape[0]), int(d_mel.shape[2])
        assert K <= B and all(int(s) >= 0 for s in d_mel.stride()), "mel_inputs: at most one slot per stream, strides >= 0"
        out = out or (self._new((K, cfg.mel_features, cfg.total_mel_frames), "float32"), self._new((K,), "int32", True))
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_rnnt_stream_mel_inputs_dev(self.ctx.handle, self._h, A.ptr(d_mel) if T else None, T, int(d_mel.stride(0)), int(d_mel.stride(1)),
                                                                 max(1, int(d_mel.stride(2))), A.ptr(d_streams), A.ptr(d_count), K, A.ptr(out[0]), A.ptr(out[1])),
                           "fa_rnnt_stream_mel_inputs_dev")
        return out

    def advance_dev(self, d_streams, d_count, frames: int = 0, d_frames=None):
        """fa_rnnt_stream_advance_dev: absoluteFrameBase += frames (or d_frames[k]) for the streams of d_streams[:d_count[0]]."""
        self._vec(d_streams, "advance: streams")
        self._vec(d_count, "advance: count", 1)
        self._vec(d_frames, "advance: frames", int(d_streams.shape[0]), optional=True)
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_rnnt_stream_advance_dev(self.ctx.handle, self._h, A.ptr(d_streams), A.ptr(d_count), int(d_streams.shape[0]), A.ptr(d_frames), int(frames)),
                           "fa_rnnt_stream_advance_dev")

    def _tokens(self, what, d_tok_frame, d_tok_id, d_tok_count, d_class):
        B = self.streams
        for t, name in ((d_tok_frame, "tok_frame"), (d_tok_id, "tok_id")):
            assert A.is_dev(t, "int32", 2) and t.shape[0] == B and t.shape == d_tok_frame.shape and t.device.index == self.ctx.device, \
                f"{what}: {name} must be a contiguous int32 CUDA tensor [{B}, capacity] on the context's device"
        self._vec(d_tok_count, f"{what}: tok_count", B)
        self._vec(d_class, f"{what}: class table", dtype="uint8")
        return int(d_tok_frame.shape[1])

    def _tracked(self, out, request_capacity, arena_capacity, slots):
        return out or RnntStreamTracked(self._new((int(request_capacity), RNNT_STREAM_REQUEST_DTYPE.itemsize), "uint8", True), self._new((int(arena_capacity),), "float32"),
                                        self._new((1,), "int32"), self._new((slots,), "int32", True))

    def track_dev(self, d_chunks, d_tok_frame, d_tok_id, d_tok_count, d_class, rescue_chunk_samples: int, request_capacity: int, arena_capacity: int, d_active=None,
                  out: RnntStreamTracked | None = None) -> RnntStreamTracked:
        """fa_rnnt_stream_track_dev: the chunk rows of gate_dev, the live timed tokens int32 [streams, capacity] (absolute frames, ids) with their
        counts, the class table uint8 [vocab] (token_classes)."""
        B, n = self.streams, self._chunks(d_chunks, "track")
        cap = self._tokens("track", d_tok_frame, d_tok_id, d_tok_count, d_class)
        self._vec(d_active, "track: active", B, optional=True)
        out = self._tracked(out, request_capacity, arena_capacity, B)
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_rnnt_stream_track_dev(self.ctx.handle, self._h, A.ptr(d_chunks) if n else None, n, A.ptr(d_active), A.ptr(d_tok_frame) if cap else None,
                                                            A.ptr(d_tok_id) if cap else None, A.ptr(d_tok_count), cap, A.ptr(d_class) if d_class.numel() else None,
                                                            int(d_class.numel()), int(rescue_chunk_samples), A.ptr(out.requests) if out.requests.numel() else None,
                                                            int(out.requests.shape[0]), A.ptr(out.arena) if out.arena.numel() else None, int(out.arena.numel()),
                                                            A.ptr(out.request_count), A.ptr(out.status)), "fa_rnnt_stream_track_dev")
        return out

    def finalize_dev(self, d_streams, d_count, d_tok_frame, d_tok_id, d_tok_count, d_class, rescue_chunk_samples: int, request_capacity: int, arena_capacity: int,
                     out: RnntStreamTracked | None = None) -> RnntStreamTracked:
        """fa_rnnt_stream_finalize_dev (finalizeRescueSpanIfNeeded) for the streams of d_streams[:d_count[0]]; status per listed slot."""
        self._vec(d_streams, "finalize: streams")
        self._vec(d_count, "finalize: count", 1)
        cap = self._tokens("finalize", d_tok_frame, d_tok_id, d_tok_count, d_class)
        out = self._tracked(out, request_capacity, arena_capacity, int(d_streams.shape[0]))
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_rnnt_stream_finalize_dev(self.ctx.handle, self._h, A.ptr(d_streams), A.ptr(d_count), int(d_streams.shape[0]),
                                                               A.ptr(d_tok_frame) if cap else None, A.ptr(d_tok_id) if cap else None, A.ptr(d_tok_count), cap,
                                                               A.ptr(d_class) if d_class.numel() else None, int(d_class.numel()), int(rescue_chunk_samples),
                                                               A.ptr(out.requests) if out.requests.numel() else None, int(out.requests.shape[0]),
                                                               A.ptr(out.arena) if out.arena.numel() else None, int(out.arena.numel()), A.ptr(out.request_count), A.ptr(out.status)),
                           "fa_rnnt_stream_finalize_dev")
        return out

    def merge_rescued_dev(self, tracked: RnntStreamTracked, d_staged_ids, d_staged_frames, d_staged_id_count, d_staged_frame_count, d_live_ids, d_live_frames,
                          d_live_timed_ids, d_live_id_count, d_live_timed_count, d_class, out=None):
        """fa_rnnt_stream_merge_rescued_dev: the staged ids / absolute frames int32 [request_capacity, staged_capacity] of every request's rescue decode
        with their counts, merged in place into the live int32 [streams, capacity] arrays -> request_status int32 [request_capacity]."""
        B, R = self.streams, int(tracked.requests.shape[0])
        for t, name in ((d_staged_ids, "staged_ids"), (d_staged_frames, "staged_frames")):
            assert A.is_dev(t, "int32", 2) and t.shape[0] == R and t.shape == d_staged_ids.shape, f"merge_rescued: {name} must be a contiguous int32 CUDA tensor [{R}, capacity]"
        for t, name in ((d_live_ids, "live_ids"), (d_live_frames, "live_frames"), (d_live_timed_ids, "live_timed_ids")):
            assert (t is None and name == "live_timed_ids") or (A.is_dev(t, "int32", 2) and t.shape[0] == B and t.shape == d_live_ids.shape), \
                f"merge_rescued: {name} must be a contiguous int32 CUDA tensor [{B}, capacity]"
        self._vec(d_staged_id_count, "merge_rescued: staged_id_count", R)
        self._vec(d_staged_frame_count, "merge_rescued: staged_frame_count", R)
        self._vec(d_live_id_count, "merge_rescued: live_id_count", B)
        self._vec(d_live_timed_count, "merge_rescued: live_timed_count", B)
        self._vec(d_class, "merge_rescued: class table", dtype="uint8")
        out = out if out is not None else self._new((R,), "int32", True)
        scap, lcap = int(d_staged_ids.shape[1]), int(d_live_ids.shape[1])
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_rnnt_stream_merge_rescued_dev(self.ctx.handle, self._h, A.ptr(tracked.requests) if R else None, A.ptr(tracked.request_count), R,
                                                                    A.ptr(d_staged_ids) if scap else None, A.ptr(d_staged_frames) if scap else None, A.ptr(d_staged_id_count),
                                                                    A.ptr(d_staged_frame_count), scap, A.ptr(d_live_ids) if lcap else None, A.ptr(d_live_frames) if lcap else None,
                                                                    A.ptr(d_live_timed_ids) if lcap else None, A.ptr(d_live_id_count), A.ptr(d_live_timed_count), lcap,
                                                                    A.ptr(d_class) if d_class.numel() else None, int(d_class.numel()), A.ptr(out)),
                           "fa_rnnt_stream_merge_rescued_dev")
        return out

    # ---- the same on host arrays: one synchronisation each
    def gate(self, chunks, active=None):
        """fa_rnnt_stream_gate: (rms, skip, run_list[:run_count], status) as numpy arrays."""
        B = self.streams
        chunks = np.ascontiguousarray(chunks, np.float32).reshape(B, -1)
        active = None if active is None else np.ascontiguousarray(active, np.int32).reshape(B)
        r, skip, run, n, status = np.zeros(B, np.float32), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(1, np.int32), np.zeros(B, np.int32)
        self.ctx.check(L.lib().fa_rnnt_stream_gate(self.ctx.handle, self._h, A.ptr(chunks) if chunks.size else None, chunks.shape[1], A.ptr(active), A.ptr(r), A.ptr(skip), A.ptr(run),
                                                   A.ptr(n), A.ptr(status)), "fa_rnnt_stream_gate")
        return r, skip, run[:n[0]], status

    def track(self, chunks, tok_frame, tok_id, tok_count, class_table, rescue_chunk_samples: int, request_capacity: int, arena_capacity: int, active=None):
        """fa_rnnt_stream_track: (the records that have one [RNNT_STREAM_REQUEST_DTYPE], arena, requests found, status)."""
        B = self.streams
        chunks = np.ascontiguousarray(chunks, np.float32).reshape(B, -1)
        tf, ti = np.ascontiguousarray(tok_frame, np.int32).reshape(B, -1), np.ascontiguousarray(tok_id, np.int32).reshape(B, -1)
        tc, cls = np.ascontiguousarray(tok_count, np.int32).reshape(B), np.ascontiguousarray(class_table, np.uint8).reshape(-1)
        assert tf.shape == ti.shape, "track: one id per timed token"
        active = None if active is None else np.ascontiguousarray(active, np.int32).reshape(B)
        req, arena = np.zeros(int(request_capacity), RNNT_STREAM_REQUEST_DTYPE), np.zeros(int(arena_capacity), np.float32)
        n, status = np.zeros(1, np.int32), np.zeros(B, np.int32)
        self.ctx.check(L.lib().fa_rnnt_stream_track(self.ctx.handle, self._h, A.ptr(chunks) if chunks.size else None, chunks.shape[1], A.ptr(active), A.ptr(tf) if tf.size else None,
                                                    A.ptr(ti) if ti.size else None, A.ptr(tc), tf.shape[1], A.ptr(cls) if cls.size else None, cls.size, int(rescue_chunk_samples),
                                                    A.ptr(req) if req.size else None, req.size, A.ptr(arena) if arena.size else None, arena.size, A.ptr(n), A.ptr(status)),
                       "fa_rnnt_stream_track")
        return req[:min(int(n[0]), req.size)], arena, int(n[0]), status

    def merge_rescued(self, requests, staged_ids, staged_frames, staged_id_count, staged_frame_count, live_ids, live_frames, live_timed_ids, live_id_count, live_timed_count,
                      class_table):
        """fa_rnnt_stream_merge_rescued on copies of the live arrays: (ids, frames, timed_ids or None, id_count, timed_count, request_status); the timings in
        seconds are seconds(frames)."""
        B = self.streams
        req = np.ascontiguousarray(requests, RNNT_STREAM_REQUEST_DTYPE).reshape(-1)
        N = req.size
        sid, sfr = np.ascontiguousarray(staged_ids, np.int32).reshape(N, -1), np.ascontiguousarray(staged_frames, np.int32).reshape(N, -1)
        sic, sfc = np.ascontiguousarray(staged_id_count, np.int32).reshape(N), np.ascontiguousarray(staged_frame_count, np.int32).reshape(N)
        ids, fr = np.array(live_ids, np.int32, order="C").reshape(B, -1), np.array(live_frames, np.int32, order="C").reshape(B, -1)
        tid = None if live_timed_ids is None else np.array(live_timed_ids, np.int32, order="C").reshape(B, -1)
        idc, tc = np.array(live_id_count, np.int32).reshape(B), np.array(live_timed_count, np.int32).reshape(B)
        cls = np.ascontiguousarray(class_table, np.uint8).reshape(-1)
        assert sid.shape == sfr.shape and ids.shape == fr.shape and (tid is None or tid.shape == ids.shape), "merge_rescued: array shapes"
        status = np.zeros(N, np.int32)
        self.ctx.check(L.lib().fa_rnnt_stream_merge_rescued(self.ctx.handle, self._h, A.ptr(req) if N else None, N, A.ptr(sid) if sid.size else None, A.ptr(sfr) if sfr.size else None,
                                                            A.ptr(sic) if N else None, A.ptr(sfc) if N else None, sid.shape[1] if N else 0, A.ptr(ids) if ids.size else None,
                                                            A.ptr(fr) if fr.size else None, A.ptr(tid) if tid is not None and tid.size else None, A.ptr(idc), A.ptr(tc), ids.shape[1],
                                                            A.ptr(cls) if cls.size else None, cls.size, A.ptr(status) if N else None), "fa_rnnt_stream_merge_rescued")
        return ids, fr, tid, idc, tc, status

    # ---- whole-state records: host data, complete on return
    def get(self, stream: int) -> RnntStreamSnapshot:
        g, cfg, info = self.geometry, self.config, L.RnntStreamInfo()
        span, pre, mel = np.zeros(g.span_capacity, np.float32), np.zeros(g.pre_roll_capacity, np.float32), np.zeros(g.mel_cache_capacity, np.float32)
        self.ctx.check(L.lib().fa_rnnt_stream_get(self.ctx.handle, self._h, int(stream), C.byref(info), A.ptr(span), A.ptr(pre), A.ptr(mel)), "fa_rnnt_stream_get")
        rows = mel[:cfg.mel_features * cfg.pre_encode_cache].reshape(cfg.mel_features, cfg.pre_encode_cache)
        return RnntStreamSnapshot(**{f: getattr(info, f) for f in _INFO_FIELDS}, span_audio=span[:info.span_samples].copy(), pre_roll=pre[:info.pre_roll_samples].copy(),
                                  mel_cache=rows[:, :info.mel_cache_frames].copy())

    def set(self, stream: int, s: RnntStreamSnapshot):
        g, cfg = self.geometry, self.config
        info = L.RnntStreamInfo(*[int(getattr(s, f)) for f in _INFO_FIELDS])
        span, pre, mel = np.zeros(g.span_capacity, np.float32), np.zeros(g.pre_roll_capacity, np.float32), np.zeros(g.mel_cache_capacity, np.float32)
        assert 0 <= s.span_samples <= span.size and 0 <= s.pre_roll_samples <= pre.size and 0 <= s.mel_cache_frames <= cfg.pre_encode_cache, "set: counts within the slabs"
        span[:s.span_samples] = np.asarray(s.span_audio, np.float32).reshape(-1)[:s.span_samples]
        pre[:s.pre_roll_samples] = np.asarray(s.pre_roll, np.float32).reshape(-1)[:s.pre_roll_samples]
        if s.mel_cache_frames:
            mel[:cfg.mel_features * cfg.pre_encode_cache].reshape(cfg.mel_features, cfg.pre_encode_cache)[:, :s.mel_cache_frames] = np.asarray(s.mel_cache, np.float32)
        self.ctx.check(L.lib().fa_rnnt_stream_set(self.ctx.handle, self._h, int(stream), C.byref(info), A.ptr(span), A.ptr(pre), A.ptr(mel)), "fa_rnnt_stream_set")

    def reset(self, stream: int = -1):
        """resetRescueState plus the gate's counters, the frame base and the mel cache, for one stream or for all."""
        self.ctx.check(L.lib().fa_rnnt_stream_reset(self.ctx.handle, self._h, int(stream)), "fa_rnnt_stream_reset")
