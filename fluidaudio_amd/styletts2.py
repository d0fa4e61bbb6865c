"""The StyleTTS2 session (reference: TTS/StyleTTS2/Pipeline/Synthesize/StyleTTS2Synthesizer.swift, StyleTTS2GlueOps.swift,
Preprocess/StyleTTS2MelExtractor.swift, Sampler/StyleTTS2DiffusionSchedule.swift): everything `synthesize` computes on the host between
its eight networks — the 2048-point power mel of the reference clip, the padded BERT inputs, the seeded noise stack, the style blend, the
rounded durations with their scan, the alignment of both feature maps with the causal shift, the tail trim — batched over (reference
clip, text) pairs on device slabs (fluidaudio_amd/csrc/styletts2.hip).  include/fluidaudio_hip.h, section "StyleTTS2 session", states
the arithmetic.

Host arrays in, host arrays out (the host-pointer entries, one synchronisation each).  The device-pointer entries, which leave the slabs
in HBM from the clip to the waveform, are served by the C ABI and the C++ mirror (``fluidaudio::StyleTts2Session``); this module has no
device-tensor form yet.  The networks, the phonemizer, the text cleaner and the chunker stay the caller's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args as A
from . import _lib as L

SLABS = {"mel": (0, np.float32), "tokens": (1, np.int32), "attention_mask": (2, np.int32), "noise_init": (3, np.float32), "noises_aux": (4, np.float32),
         "ref": (5, np.float32), "s": (6, np.float32), "durations": (7, np.int32), "starts": (8, np.int32), "total_frames": (9, np.int32), "status": (10, np.int32)}


def styletts2_config(**fields) -> L.StyleTts2Config:
    """fa_styletts2_default_config (StyleTTS2Constants: n_fft 2048, window 1200, hop 300, 80 mels built for 16 kHz, buckets 57 / 64 /
    128 / 256, 5 diffusion steps, 640 + 512 channels, tail trim 50; 2400 reference frames, 4096 frames) with `fields` set over it."""
    cfg = L.StyleTts2Config()
    L.lib().fa_styletts2_default_config(C.byref(cfg))
    for name, value in fields.items():
        if not hasattr(cfg, name):
            raise A.invalid("styletts2_config", f"no field {name}")
        if name == "buckets":
            value = list(value)
            cfg.n_buckets, value = len(value), (C.c_int32 * 4)(*value)
        setattr(cfg, name, value)
    return cfg


def _check(status: int, where: str):
    if status != L.SUCCESS:
        raise L.FluidAudioHipError(status, where)


def _plan_inputs(where, samples, tokens):
    n = np.ascontiguousarray(samples, np.int64).reshape(-1)
    if n.size < 1:
        raise A.invalid(where, "empty batch")
    return n, np.ascontiguousarray(np.broadcast_to(np.asarray(tokens, np.int32), n.shape))


def styletts2_plan(samples, tokens, cfg: L.StyleTts2Config | None = None) -> list:
    """What the session does to a batch, without a device: per item the reference frames, the BERT / sampler bucket and the status
    (FA_STYLETTS2_*); a refused item has its status and zeros."""
    cfg = cfg or styletts2_config()
    n, t = _plan_inputs("styletts2_plan", samples, tokens)
    plans = (L.StyleTts2ItemPlan * n.size)()
    _check(L.lib().fa_styletts2_plan(C.byref(cfg), n.size, A.ptr(n), A.ptr(t), plans), "fa_styletts2_plan")
    return list(plans)


def styletts2_karras_sigmas(steps: int | None = None, cfg: L.StyleTts2Config | None = None) -> np.ndarray:
    """StyleTTS2DiffusionSchedule.karrasSigmas: steps + 1 doubles, the last one 0"""
    cfg = cfg or styletts2_config()
    steps = cfg.diffusion_steps if steps is None else int(steps)
    out = np.zeros(max(steps, 0) + 1, np.float64)
    _check(L.lib().fa_styletts2_karras_sigmas(C.byref(cfg), steps, A.ptr(out)), "fa_styletts2_karras_sigmas")
    return out


def styletts2_window(cfg: L.StyleTts2Config | None = None) -> np.ndarray:
    """the `win` samples of the periodic Hann that lies centred in n_fft"""
    cfg = cfg or styletts2_config()
    out = np.zeros(cfg.win, np.float32)
    _check(L.lib().fa_styletts2_window(C.byref(cfg), A.ptr(out)), "fa_styletts2_window")
    return out


def styletts2_filterbank(cfg: L.StyleTts2Config | None = None) -> np.ndarray:
    """float32 [n_mels, n_fft / 2 + 1]: HTK triangles, no normalisation, for the filter rate"""
    cfg = cfg or styletts2_config()
    out = np.zeros((cfg.n_mels, cfg.n_fft // 2 + 1), np.float32)
    _check(L.lib().fa_styletts2_filterbank(C.byref(cfg), A.ptr(out)), "fa_styletts2_filterbank")
    return out


def _rows(a, where, shape_text, ok):
    a = np.asarray(a)
    if a.dtype != np.float32 or not a.flags.c_contiguous or not ok(a):
        raise A.invalid(where, f"float32 {shape_text}, C-contiguous (the last axis may be stride-padded)")
    return a


class StyleTts2Session:
    """`batch` (reference clip, text) pairs whose mel, BERT inputs, noises, styles and durations stay on the device between the calls."""

    def __init__(self, batch: int, cfg: L.StyleTts2Config | None = None, ctx: L.Context | None = None):
        self.cfg, self.ctx, self.batch, self.plans, self.totals = cfg or styletts2_config(), ctx or L.default_context(), int(batch), None, None
        self._h = C.c_void_p()
        self.ctx.check(L.lib().fa_styletts2_session_create(self.ctx.handle, C.byref(self.cfg), self.batch, C.byref(self._h)), "fa_styletts2_session_create")

    def close(self):
        if self._h:
            L.lib().fa_styletts2_session_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def slabs(self) -> L.StyleTts2Slabs:
        """the fixed device addresses the batched networks read in place"""
        out = L.StyleTts2Slabs()
        _check(L.lib().fa_styletts2_session_slabs(self._h, C.byref(out)), "fa_styletts2_session_slabs")
        return out

    def reference_mel(self, waves, tokens, offsets=None):
        """Plans the batch and runs the reference mel.  `waves`: one 24 kHz float array per item (or one flat array with its batch + 1
        `offsets`); `tokens`: the token count per item or one for all.  Returns the plans."""
        pcm, offsets = A.ragged(waves, offsets, np.float32, "StyleTts2Session.reference_mel", "offsets: one-dimensional, batch + 1 entries")
        if offsets.size - 1 != self.batch:
            raise A.invalid("StyleTts2Session.reference_mel", f"{offsets.size - 1} clips for a session of {self.batch}")
        n, t = _plan_inputs("StyleTts2Session.reference_mel", np.diff(offsets), tokens)
        plans = (L.StyleTts2ItemPlan * self.batch)()
        self.ctx.check(L.lib().fa_styletts2_session_begin(self.ctx.handle, self._h, A.ptr(n), A.ptr(t), plans), "fa_styletts2_session_begin")
        self.ctx.check(L.lib().fa_styletts2_reference_mel(self.ctx.handle, self._h, A.ptr(pcm), A.ptr(offsets)), "fa_styletts2_reference_mel")
        self.plans, self.totals = list(plans), None
        return self.plans

    def inputs(self, token_ids, seeds, offsets=None):
        """padded tokens, attention mask and the seeded noise stack: `token_ids` one int array per item, `seeds` uint64."""
        ids, offsets = A.ragged(token_ids, offsets, np.int32, "StyleTts2Session.inputs", "offsets: one-dimensional, batch + 1 entries")
        seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, np.uint64), (self.batch,)))
        if offsets.size - 1 != self.batch:
            raise A.invalid("StyleTts2Session.inputs", f"{offsets.size - 1} token lists for a session of {self.batch}")
        self.ctx.check(L.lib().fa_styletts2_inputs(self.ctx.handle, self._h, A.ptr(ids), A.ptr(offsets), A.ptr(seeds)), "fa_styletts2_inputs")

    def blend(self, s_pred, ref_s, alpha=0.3, beta=0.7):
        """ref and s (slabs of those names) from the sampler's `s_pred` and the reference encoder's `ref_s`, float32 [batch, >= 256];
        `alpha` / `beta` per item or one for all."""
        where = "StyleTts2Session.blend"
        p, r = (_rows(a, where, f"[{self.batch}, >= 256]", lambda a: a.ndim == 2 and a.shape[0] == self.batch and a.shape[1] >= 256) for a in (s_pred, ref_s))
        al, be = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (self.batch,))) for v in (alpha, beta))
        self.ctx.check(L.lib().fa_styletts2_blend(self.ctx.handle, self._h, A.ptr(p), p.shape[1], A.ptr(r), r.shape[1], A.ptr(al), A.ptr(be)), "fa_styletts2_blend")

    def durations(self, logits):
        """`logits`: the duration predictor's output, float32 [batch, >= tokens, C <= 64] -> (total_frames, status) per item; the
        durations and their exclusive scan are the slabs `durations` and `starts`."""
        a = _rows(logits, "StyleTts2Session.durations", f"[{self.batch}, tokens, channels]", lambda a: a.ndim == 3 and a.shape[0] == self.batch)
        if self.plans is None or a.shape[1] < max(p.tokens for p in self.plans):
            raise A.invalid("StyleTts2Session.durations", "reference_mel() first, and one row per token")
        totals, status = np.zeros(self.batch, np.int32), np.zeros(self.batch, np.int32)
        self.ctx.check(L.lib().fa_styletts2_durations(self.ctx.handle, self._h, A.ptr(a), a.shape[2], a.shape[1] * a.shape[2], a.shape[2], 1, A.ptr(totals), A.ptr(status)),
                       "fa_styletts2_durations")
        self.totals = np.where(status == 0, totals, 0)
        return totals, status

    def align(self, d, t_en, shift: bool = True, frame_stride: int | None = None):
        """`d`: float32 [batch, >= tokens, >= d_channels] (token-major), `t_en`: float32 [batch, asr_channels, >= tokens] (channel-major)
        -> (en [batch, d_channels, frame_stride], asr [batch, asr_channels, frame_stride]): every frame its token's features, shifted
        one frame to the right with `shift`, zeros behind the item's total."""
        c, n = self.cfg, max(p.tokens for p in self.plans) if self.plans else 0
        if self.totals is None:
            raise A.invalid("StyleTts2Session.align", "durations() first")
        d = _rows(d, "StyleTts2Session.align", f"[{self.batch}, tokens, >= {c.d_channels}]", lambda a: a.ndim == 3 and a.shape[0] == self.batch and a.shape[1] >= n and a.shape[2] >= c.d_channels)
        t = _rows(t_en, "StyleTts2Session.align", f"[{self.batch}, {c.asr_channels}, >= tokens]", lambda a: a.ndim == 3 and a.shape[:2] == (self.batch, c.asr_channels) and a.shape[2] >= n)
        stride = int(frame_stride) if frame_stride is not None else max(4, -(-int(self.totals.max()) // 4) * 4)
        en, asr = np.zeros((self.batch, c.d_channels, stride), np.float32), np.zeros((self.batch, c.asr_channels, stride), np.float32)
        self.ctx.check(L.lib().fa_styletts2_align(self.ctx.handle, self._h, A.ptr(d), d.shape[2], d.shape[1] * d.shape[2], A.ptr(t), t.shape[2], t.shape[1] * t.shape[2],
                                                  int(bool(shift)), A.ptr(en), A.ptr(asr), stride), "fa_styletts2_align")
        return en, asr

    def finish(self, audio, lengths) -> list:
        """`audio`: the decoder's rows, float32 [batch, >= lengths] -> one float32 array per item without its last min(50, len) samples;
        the arrays are views of one buffer in which the items lie back to back."""
        audio, lengths = np.asarray(audio), np.ascontiguousarray(lengths, np.int64).reshape(-1)
        if self.plans is None or audio.dtype != np.float32 or audio.ndim != 2 or audio.shape[0] != self.batch or not audio.flags.c_contiguous or lengths.size != self.batch:
            raise A.invalid("StyleTts2Session.finish", f"reference_mel() first; float32 [{self.batch}, samples], C-contiguous, one length per item")
        out, offsets = np.zeros(max(int(np.maximum(lengths, 0).sum()), 1), np.float32), np.zeros(self.batch + 1, np.int64)
        self.ctx.check(L.lib().fa_styletts2_finish(self.ctx.handle, self._h, A.ptr(audio), audio.shape[1], A.ptr(lengths), A.ptr(out), out.size, A.ptr(offsets)), "fa_styletts2_finish")
        return [out[offsets[b]:offsets[b + 1]] for b in range(self.batch)]

    def get(self, name: str) -> np.ndarray:
        """one slab as a host array: mel [batch, n_mels, max_ref_frames]; tokens / attention_mask / durations / starts [batch, largest
        bucket]; noise_init [batch, 256]; noises_aux [steps - 1, batch, 256]; ref / s [batch, 128]; total_frames / status [batch]"""
        if name not in SLABS:
            raise A.invalid("StyleTts2Session.get", f"no slab {name}")
        c, B, T = self.cfg, self.batch, self.cfg.buckets[self.cfg.n_buckets - 1]
        which, dtype = SLABS[name]
        shape = {"mel": (B, c.n_mels, c.max_ref_frames), "noise_init": (B, 256), "noises_aux": (c.diffusion_steps - 1, B, 256), "ref": (B, 128), "s": (B, 128),
                 "total_frames": (B,), "status": (B,)}.get(name, (B, T))
        out = np.zeros(shape, dtype)
        self.ctx.check(L.lib().fa_styletts2_session_get(self.ctx.handle, self._h, which, A.ptr(out)), "fa_styletts2_session_get")
        return out
