"""The PocketTTS session (reference: TTS/PocketTTS/Pipeline/PocketTtsVoiceCloner.swift, PocketTtsSynthesizer+KVCache.swift,
PocketTtsStateEngine.swift, PocketTtsSynthesizer.swift): the host work round PocketTTS's networks for a set of concurrent streams on
device slabs (fluidaudio_amd/csrc/pockettts.hip) — the encoder's input rows and the conditioning extraction fused with the speaker
re-projection on the fp32 matrix instructions, the voice table, the per-chunk KV cache reset from a voice's snapshot in the three
at-rest formats and its capture, the zero-padded 256-token prefill windows, and the generation loop's scalar side (EOS machine,
`sequence` feedback, running list, audio frames).  include/fluidaudio_hip.h, section "PocketTTS session", states the arithmetic.

Host arrays in, host arrays out.  The device-pointer entries, which take the networks' outputs where they lie in HBM, are served by the
C ABI and the C++ mirror (``fluidaudio::PocketTtsSession``); this module has no device-tensor form yet.  The networks, the tokenizer,
text normalisation and chunking, audio file loading, the pipelined scheduling variant and the start noise stay the caller's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args as A
from . import _lib as L

DIM, LATENT, WINDOW, KV_SEQ, KV_ROW, FRAME_SAMPLES, ENCODER_SAMPLES, MAX_VOICE_FRAMES = 1024, 32, 256, 512, 1024, 1920, 240000, 125
KV_FORMATS = {"combined": 0, "split": 1, "fp16": 2}
SLABS = {"kv": (0, None), "positions": (1, np.float32), "voice_rows": (2, np.float32), "voice_kv": (3, np.float32), "encoder_input": (4, np.float32),
         "windows": (5, np.float32), "valid_len": (6, np.float32), "window_position": (7, np.float32), "sequence": (8, np.float32), "state": (9, np.int32),
         "running": (10, np.int32), "n_running": (11, np.int32), "audio": (12, np.float32)}
STATE_FIELDS = ("step", "eos_step", "max_gen", "after", "frames", "reason", "emit", "pad")


def pockettts_config(**fields) -> L.PocketTtsConfig:
    """fa_pockettts_default_config (6 layers, fp32 combined cache, 4 streams, 4 voices of up to 512 positions, 2 projections, 4001
    vocabulary rows, 16 windows, 4 clones, 256 audio frames, NaN start sequence) with `fields` set over it; kv_format by name or number."""
    cfg = L.PocketTtsConfig()
    L.lib().fa_pockettts_default_config(C.byref(cfg))
    for name, value in fields.items():
        if not hasattr(cfg, name):
            raise A.invalid("pockettts_config", f"no field {name}")
        setattr(cfg, name, KV_FORMATS[value] if name == "kv_format" and isinstance(value, str) else int(value))
    return cfg


def pockettts_clone_plan(samples, available=None):
    """Per clip (status, usable frames) without a device: under 1 s is refused; usable = min(available, ceil(min(n, 240000) / 1920), 125)."""
    n = np.ascontiguousarray(samples, np.int64).reshape(-1)
    av = None if available is None else np.ascontiguousarray(np.broadcast_to(np.asarray(available, np.int32), n.shape))
    usable, status = np.zeros(n.size, np.int32), np.zeros(n.size, np.int32)
    st = L.lib().fa_pockettts_clone_plan(n.size, A.ptr(n), A.ptr(av), A.ptr(usable), A.ptr(status))
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_pockettts_clone_plan")
    return usable, status


def _ints(v, n=None):
    a = np.ascontiguousarray(v, np.int32).reshape(-1)
    return a if n is None else np.ascontiguousarray(np.broadcast_to(a, (n,)))


class PocketTtsSession:
    """The slabs of `cfg.streams` streams, the voice table and the projection table, kept on the device between the calls."""

    def __init__(self, cfg: L.PocketTtsConfig | None = None, ctx: L.Context | None = None):
        self.cfg, self.ctx = cfg or pockettts_config(), ctx or L.default_context()
        self._h = C.c_void_p()
        self.ctx.check(L.lib().fa_pockettts_session_create(self.ctx.handle, C.byref(self.cfg), C.byref(self._h)), "fa_pockettts_session_create")
        self.n_positions = 1 if self.cfg.kv_format == 2 else self.cfg.layers

    def close(self):
        if self._h and L is not None and L.lib is not None:   # at interpreter exit the module may be gone before a cached session
            L.lib().fa_pockettts_session_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _call(self, name, *args):
        self.ctx.check(getattr(L.lib(), name)(self.ctx.handle, self._h, *args), name)

    def slabs(self) -> L.PocketTtsSlabs:
        """the fixed device addresses the batched networks read and write in place"""
        out = L.PocketTtsSlabs()
        st = L.lib().fa_pockettts_session_slabs(self._h, C.byref(out))
        if st != L.SUCCESS:
            raise L.FluidAudioHipError(st, "fa_pockettts_session_slabs")
        return out

    def _dtype(self, name):
        if name not in SLABS:
            raise A.invalid("PocketTtsSession", f"no slab {name}")
        return np.dtype(SLABS[name][1] or (np.float16 if self.cfg.kv_format == 2 else np.float32))

    def get(self, name: str, first: int = 0, count: int = 1) -> np.ndarray:
        """`count` elements of a slab from element `first` on, as a flat host array of the slab's type (kv: float16 in the fp16 format)"""
        dt = self._dtype(name)
        out = np.zeros(int(count), dt)
        self._call("fa_pockettts_session_get", SLABS[name][0], int(first) * dt.itemsize, out.nbytes, A.ptr(out))
        return out

    def put(self, name: str, values, first: int = 0):
        """overwrites elements of a slab from element `first` on"""
        dt = self._dtype(name)
        v = np.ascontiguousarray(values, dt).reshape(-1)
        self._call("fa_pockettts_session_put", SLABS[name][0], int(first) * dt.itemsize, v.nbytes, A.ptr(v))
        self.ctx.synchronize()

    def kv_plane(self, stream: int, layer: int, side: int) -> np.ndarray:
        """K (side 0) or V (side 1) of one layer of one stream's cache: [512, 1024]"""
        c, sl = self.cfg, stream * self.cfg.layers + layer
        plane = sl * 2 + side if c.kv_format == 0 else side * c.streams * c.layers + sl
        return self.get("kv", plane * KV_SEQ * KV_ROW, KV_SEQ * KV_ROW).reshape(KV_SEQ, KV_ROW)

    def positions(self) -> np.ndarray:
        return self.get("positions", 0, self.cfg.streams * self.n_positions).reshape(self.cfg.streams, self.n_positions)

    def state(self) -> dict:
        """the streams' EOS machines: one int32 array per field of fa_pockettts_stream_state"""
        a = self.get("state", 0, self.cfg.streams * 8).reshape(self.cfg.streams, 8)
        return {name: a[:, i] for i, name in enumerate(STATE_FIELDS)}

    def running(self) -> np.ndarray:
        return self.get("running", 0, self.cfg.streams)[:int(self.get("n_running")[0])]

    def set_projection(self, index: int, pinv, w):
        """speaker projection `index`: encoderRecoverPinv and targetProj, float32 [1024, 32] each"""
        p, w = (np.ascontiguousarray(a, np.float32) for a in (pinv, w))
        if p.shape != (DIM, LATENT) or w.shape != (DIM, LATENT):
            raise A.invalid("PocketTtsSession.set_projection", "float32 [1024, 32] twice")
        self._call("fa_pockettts_projection_set", int(index), A.ptr(p), A.ptr(w))
        self.ctx.synchronize()

    def set_constants(self, table, bos_before_voice=None, bos_embedding=None):
        """the text embedding table float32 [vocab, 1024] (the vocabulary is its row count), bos_before_voice [1024] and bos_emb [32]"""
        t = np.ascontiguousarray(table, np.float32)
        b, e = (None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1) for a in (bos_before_voice, bos_embedding))
        if t.ndim != 2 or t.shape[1] != DIM or (b is not None and b.size != DIM) or (e is not None and e.size != LATENT):
            raise A.invalid("PocketTtsSession.set_constants", "table [vocab, 1024], bos_before_voice [1024], bos_embedding [32]")
        self._call("fa_pockettts_constants_set", A.ptr(b), A.ptr(e), A.ptr(t), t.shape[0])
        self.ctx.synchronize()

    def add_voice(self, voice: int, layers, offsets, src_seq: int) -> int:
        """A shipped voice: `layers` one float32 array per layer ([2, 1, src_seq, 16, 64], K then V), `offsets` one per layer.  Returns the
        status (FA_POCKETTTS_*): a refused voice leaves the slot empty."""
        layers = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in layers]
        counts, off, status = np.array([a.size for a in layers], np.int64), np.ascontiguousarray(offsets, np.int64).reshape(-1), C.c_int32(0)
        if off.size != len(layers):
            raise A.invalid("PocketTtsSession.add_voice", "one offset per layer")
        flat = np.concatenate(layers) if layers else np.zeros(0, np.float32)
        self._call("fa_pockettts_voice_add", int(voice), len(layers), int(src_seq), A.ptr(flat), A.ptr(counts), A.ptr(off), C.byref(status))
        self.ctx.synchronize()
        return status.value

    def encoder_input(self, waves, offsets=None):
        """the clips as the Mimi encoder's rows (slab encoder_input): -> (usable frames, status) per clip"""
        pcm, offsets = A.ragged(waves, offsets, np.float32, "PocketTtsSession.encoder_input", "offsets: one-dimensional, clips + 1 entries")
        n = offsets.size - 1
        usable, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._call("fa_pockettts_encoder_input", n, A.ptr(pcm), A.ptr(offsets), A.ptr(usable), A.ptr(status))
        return usable, status

    def clone(self, voices, projections, usable, cond):
        """`cond`: the encoder's output, float32 or float16 [clones, >= usable frames, 1024], any strides (a view is read in place): its
        first usable[b] frames through projection projections[b] (-1: none) into voice slot voices[b]."""
        cond = np.asarray(cond)
        if cond.dtype not in (np.float32, np.float16) or cond.ndim != 3 or cond.shape[2] != DIM or any(s % cond.itemsize or s < 0 for s in cond.strides):
            raise A.invalid("PocketTtsSession.clone", "float32 or float16 [clones, frames, 1024]")
        n = cond.shape[0]
        v, p, u = _ints(voices, n), _ints(projections, n), _ints(usable, n)
        if u.max(initial=0) > cond.shape[1]:
            raise A.invalid("PocketTtsSession.clone", "more usable frames than the array holds")
        strides = [s // cond.itemsize for s in cond.strides]
        self._call("fa_pockettts_clone", n, A.ptr(v), A.ptr(p), A.ptr(u), cond.ctypes.data, 1 if cond.dtype == np.float16 else 0, *strides)

    def voice_rows(self, voice: int, frames: int = MAX_VOICE_FRAMES) -> np.ndarray:
        return self.get("voice_rows", voice * MAX_VOICE_FRAMES * DIM, frames * DIM).reshape(frames, DIM)

    def kv_reset(self, streams, voices):
        """every listed stream's cache and positions from its voice's snapshot (zeros and 0 for a voice without one), one launch"""
        s = _ints(streams)
        v = _ints(voices, s.size)
        self._call("fa_pockettts_kv_reset", s.size, A.ptr(s), A.ptr(v))

    def kv_capture(self, stream: int, voice: int, seq: int):
        """rows [0, seq) of the stream's cache and its positions become the voice's snapshot"""
        self._call("fa_pockettts_kv_capture", int(stream), int(voice), int(seq))

    def plan(self, streams, voices, token_counts):
        """-> (windows, statuses): the prefill windows of the listed streams (voice block first, then the text block), kept for prefill_inputs"""
        s = _ints(streams)
        v, t = _ints(voices, s.size), _ints(token_counts, s.size)
        n, wins, status = C.c_int32(0), (L.PocketTtsWindow * self.cfg.windows)(), np.zeros(s.size, np.int32)
        st = L.lib().fa_pockettts_plan(self._h, s.size, A.ptr(s), A.ptr(v), A.ptr(t), C.byref(n), wins, A.ptr(status))
        if st != L.SUCCESS:
            raise L.FluidAudioHipError(st, "fa_pockettts_plan")
        return list(wins)[:n.value], status

    def prefill_inputs(self, token_ids):
        """fills the planned windows (slabs windows, valid_len, window_position) and advances the positions; `token_ids`: one int array per
        planned stream, in plan order"""
        ids, _ = A.ragged(token_ids, None, np.int32)
        self._call("fa_pockettts_prefill_inputs", A.ptr(ids))

    def set_position(self, stream: int, position: float):
        self._call("fa_pockettts_position_set", int(stream), float(position))

    def step_begin(self, streams, max_gen_len, frames_after_eos) -> np.ndarray:
        s = _ints(streams)
        g, a, status = _ints(max_gen_len, s.size), _ints(frames_after_eos, s.size), np.zeros(s.size, np.int32)   # named: alive through the call
        self._call("fa_pockettts_step_begin", s.size, A.ptr(s), A.ptr(g), A.ptr(a), A.ptr(status))
        return status

    def step(self, eos_logit, latent):
        """one generation step of every stream: `eos_logit` float32 [streams], `latent` float32 [streams, 32]"""
        e, l = np.ascontiguousarray(eos_logit, np.float32).reshape(-1), np.ascontiguousarray(latent, np.float32).reshape(-1)
        if e.size != self.cfg.streams or l.size != self.cfg.streams * LATENT:
            raise A.invalid("PocketTtsSession.step", "one logit and 32 latents per stream")
        self._call("fa_pockettts_step", A.ptr(e), A.ptr(l))

    def append_audio(self, samples):
        """`samples` float32 [streams, 1920]: the frame of every stream whose last step emitted"""
        a = np.ascontiguousarray(samples, np.float32).reshape(-1)
        if a.size != self.cfg.streams * FRAME_SAMPLES:
            raise A.invalid("PocketTtsSession.append_audio", "1920 samples per stream")
        self._call("fa_pockettts_append_audio", A.ptr(a))

    def audio(self, stream: int, frames: int) -> np.ndarray:
        return self.get("audio", stream * self.cfg.max_frames * FRAME_SAMPLES, frames * FRAME_SAMPLES).reshape(frames, FRAME_SAMPLES)
