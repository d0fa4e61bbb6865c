"""The LuxTTS (ZipVoice-Distill) session (reference: TTS/LuxTts/LuxTtsSynthesizer.swift:59-299, LuxTtsSolver.swift,
LuxTtsMelExtractor.swift:52-132): everything `synthesize` computes on the host between its three networks — prompt loudness and mel into
the speech condition, tokens, masks and the seeded start noise, the token-to-frame expansion, the anchor-Euler updates, the vocoder's
transposed input, the clip and loudness restore — batched over utterances on device slabs (fluidaudio_amd/csrc/luxtts.hip).
include/fluidaudio_hip.h, section "LuxTTS session", states the arithmetic.

Host arrays in, host arrays out (the host-pointer entries, one synchronisation each).  The device-pointer entries, which leave the slabs
in HBM from the prompt to the waveform, are served by the C ABI and the C++ mirror (``fluidaudio::LuxTtsSession``); this module has no
device-tensor form yet.  The networks, the G2P and the tokenizer stay the caller's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args as A
from . import _lib as L

SLABS = {"tokens": (0, np.int32, "max_tokens"), "token_mask": (1, np.float32, "max_tokens"), "text_condition": (2, np.float32, "rows"),
         "speech_condition": (3, np.float32, "rows"), "x": (4, np.float32, "rows"), "frame_mask": (5, np.float32, "max_frames")}
RECORD = np.dtype([("mean_square", np.float32), ("rms", np.float32), ("gain", np.float32), ("status", np.int32)])


def luxtts_config(**fields) -> L.LuxTtsConfig:
    """fa_luxtts_default_config (LuxTtsConstants: 24 kHz, n_fft 1024, hop 256, 100 mels, 256 tokens, 1024 frames, buckets 282 / 555,
    4 steps, t_shift 0.5, target RMS 0.1, prompt cap 5 s) with `fields` set over it; `buckets` takes a list."""
    cfg = L.LuxTtsConfig()
    L.lib().fa_luxtts_default_config(C.byref(cfg))
    for name, value in fields.items():
        if not hasattr(cfg, name):
            raise A.invalid("luxtts_config", f"no field {name}")
        if name == "buckets":
            value = list(value)
            cfg.n_buckets, value = len(value), (C.c_int32 * 4)(*value)
        setattr(cfg, name, value)
    return cfg


def _check(status: int, where: str):
    if status != L.SUCCESS:
        raise L.FluidAudioHipError(status, where)


def _plan_inputs(where, prompt_samples, prompt_tokens, text_tokens, speeds):
    n = np.ascontiguousarray(prompt_samples, np.int64).reshape(-1)
    if n.size < 1:
        raise A.invalid(where, "empty batch")
    pt, tt, sp = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, t), n.shape)) for v, t in ((prompt_tokens, np.int32), (text_tokens, np.int32), (speeds, np.float32)))
    return n, pt, tt, sp


def luxtts_plan(prompt_samples, prompt_tokens, text_tokens, speeds=1.0, cfg: L.LuxTtsConfig | None = None):
    """What the session does to a batch, without a device: (plans, {bucket: [items]}).  A refused item has its status
    (FA_LUXTTS_*, in the reference's order of guards) and zeros."""
    cfg = cfg or luxtts_config()
    n, pt, tt, sp = _plan_inputs("luxtts_plan", prompt_samples, prompt_tokens, text_tokens, speeds)
    plans, counts, lists = (L.LuxTtsItemPlan * n.size)(), np.zeros(4, np.int32), np.zeros((4, n.size), np.int32)
    _check(L.lib().fa_luxtts_plan(C.byref(cfg), n.size, A.ptr(n), A.ptr(pt), A.ptr(tt), A.ptr(sp), plans, A.ptr(counts), A.ptr(lists)), "fa_luxtts_plan")
    return list(plans), {int(cfg.buckets[k]): lists[k, :counts[k]].tolist() for k in range(cfg.n_buckets)}


def luxtts_time_steps(cfg: L.LuxTtsConfig | None = None) -> np.ndarray:
    cfg = cfg or luxtts_config()
    out = np.zeros(cfg.num_steps + 1, np.float64)
    _check(L.lib().fa_luxtts_time_steps(C.byref(cfg), A.ptr(out)), "fa_luxtts_time_steps")
    return out


def luxtts_prompt_loudness(pcm, cfg: L.LuxTtsConfig | None = None) -> L.LuxTtsRecord:
    """mean square, rms, gain and status of one prompt in the fixed fp32 order of csrc/luxtts_core.h, on the host"""
    cfg, pcm, rec = cfg or luxtts_config(), np.ascontiguousarray(pcm, np.float32).reshape(-1), L.LuxTtsRecord()
    _check(L.lib().fa_luxtts_prompt_loudness(C.byref(cfg), A.ptr(pcm), pcm.size, C.byref(rec)), "fa_luxtts_prompt_loudness")
    return rec


def luxtts_anchor_euler(x, v, step: int, cfg: L.LuxTtsConfig | None = None) -> np.ndarray:
    """one anchor-Euler update of float32 `x` on `v` in the fp32 order of csrc/luxtts_core.h, on the host"""
    cfg, out, v = cfg or luxtts_config(), np.array(x, np.float32), np.ascontiguousarray(v, np.float32)
    if out.shape != v.shape:
        raise A.invalid("luxtts_anchor_euler", "x and v differ in shape")
    _check(L.lib().fa_luxtts_anchor_euler(C.byref(cfg), int(step), A.ptr(out), A.ptr(v), out.size), "fa_luxtts_anchor_euler")
    return out


def _strided(a, where, batch, n_mels):
    """float32 [batch, rows, >= n_mels] with a dense last axis -> (flat array over its span, row stride, item stride)"""
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 3 or a.shape[0] != batch or a.shape[2] < n_mels or not a.flags.c_contiguous:
        raise A.invalid(where, f"float32 [{batch}, rows, >= {n_mels}], C-contiguous (the last axis may be stride-padded)")
    return a, a.shape[2], a.shape[1] * a.shape[2]


class LuxTtsSession:
    """`batch` utterances whose tokens, masks, conditions and solver state stay on the device between the calls."""

    def __init__(self, batch: int, cfg: L.LuxTtsConfig | None = None, ctx: L.Context | None = None):
        self.cfg, self.ctx, self.batch, self.plans = cfg or luxtts_config(), ctx or L.default_context(), int(batch), None
        self._h = C.c_void_p()
        self.ctx.check(L.lib().fa_luxtts_session_create(self.ctx.handle, C.byref(self.cfg), self.batch, C.byref(self._h)), "fa_luxtts_session_create")

    def close(self):
        if self._h:
            L.lib().fa_luxtts_session_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def slabs(self) -> L.LuxTtsSlabs:
        """the fixed device addresses the batched networks read in place"""
        out = L.LuxTtsSlabs()
        _check(L.lib().fa_luxtts_session_slabs(self._h, C.byref(out)), "fa_luxtts_session_slabs")
        return out

    def prompt(self, waves, prompt_tokens, text_tokens, speeds=1.0, offsets=None):
        """Plans the batch and runs the prompt: loudness records and the speech condition.  `waves`: one 24 kHz float array per item
        (or one flat array with its batch + 1 `offsets`); token counts and speeds per item or one for all.  Returns the plans."""
        pcm, offsets = A.ragged(waves, offsets, np.float32, "LuxTtsSession.prompt", "offsets: one-dimensional, batch + 1 entries")
        if offsets.size - 1 != self.batch:
            raise A.invalid("LuxTtsSession.prompt", f"{offsets.size - 1} prompts for a session of {self.batch}")
        n, pt, tt, sp = _plan_inputs("LuxTtsSession.prompt", np.diff(offsets), prompt_tokens, text_tokens, speeds)
        plans = (L.LuxTtsItemPlan * self.batch)()
        self.ctx.check(L.lib().fa_luxtts_session_begin(self.ctx.handle, self._h, A.ptr(n), A.ptr(pt), A.ptr(tt), A.ptr(sp), plans), "fa_luxtts_session_begin")
        self.ctx.check(L.lib().fa_luxtts_prompt(self.ctx.handle, self._h, A.ptr(pcm), A.ptr(offsets)), "fa_luxtts_prompt")
        self.plans = list(plans)
        return self.plans

    def inputs(self, token_ids, seeds, offsets=None):
        """tokens, both masks and the seeded start noise: `token_ids` one int array per item (prompt ids then text ids), `seeds` uint64."""
        ids, offsets = A.ragged(token_ids, offsets, np.int32, "LuxTtsSession.inputs", "offsets: one-dimensional, batch + 1 entries")
        seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, np.uint64), (self.batch,)))
        if offsets.size - 1 != self.batch:
            raise A.invalid("LuxTtsSession.inputs", f"{offsets.size - 1} token lists for a session of {self.batch}")
        self.ctx.check(L.lib().fa_luxtts_inputs(self.ctx.handle, self._h, A.ptr(ids), A.ptr(offsets), A.ptr(seeds)), "fa_luxtts_inputs")

    def text_condition(self, embeds):
        """`embeds`: the text encoder's output, float32 [batch, >= tokens + 1, >= n_mels] (rows may be stride-padded)."""
        a, row, item = _strided(embeds, "LuxTtsSession.text_condition", self.batch, self.cfg.n_mels)
        if self.plans is None or a.shape[1] < max(p.tokens for p in self.plans) + 1:
            raise A.invalid("LuxTtsSession.text_condition", "prompt() first, and tokens + 1 rows per item")
        self.ctx.check(L.lib().fa_luxtts_text_condition(self.ctx.handle, self._h, A.ptr(a), row, item), "fa_luxtts_text_condition")

    def step(self, step: int, v):
        """one anchor-Euler update of x on the decoder's velocity, float32 [batch, >= features_length, >= n_mels]"""
        a, row, item = _strided(v, "LuxTtsSession.step", self.batch, self.cfg.n_mels)
        if self.plans is None or a.shape[1] < max(p.features_length for p in self.plans):
            raise A.invalid("LuxTtsSession.step", "prompt() first, and features_length rows per item")
        self.ctx.check(L.lib().fa_luxtts_step(self.ctx.handle, self._h, int(step), A.ptr(a), row, item), "fa_luxtts_step")

    def vocoder_input(self, bucket: int, items) -> np.ndarray:
        """float32 [len(items), n_mels, bucket]: the listed items' generated frames, unscaled and transposed, the log floor behind"""
        items = np.ascontiguousarray(items, np.int32).reshape(-1)
        mel = np.zeros((items.size, self.cfg.n_mels, int(bucket)), np.float32)
        self.ctx.check(L.lib().fa_luxtts_vocoder_input(self.ctx.handle, self._h, int(bucket), A.ptr(items), items.size, A.ptr(mel)), "fa_luxtts_vocoder_input")
        return mel

    def finish(self, audio) -> list:
        """`audio`: the vocoders' rows, float32 [batch, >= sample_count] -> one clipped, loudness-restored float32 array per item"""
        audio = np.asarray(audio)
        if self.plans is None or audio.dtype != np.float32 or audio.ndim != 2 or audio.shape[0] != self.batch or not audio.flags.c_contiguous:
            raise A.invalid("LuxTtsSession.finish", f"prompt() first; float32 [{self.batch}, samples], C-contiguous")
        offsets = np.concatenate([[0], np.cumsum([p.sample_count for p in self.plans])]).astype(np.int64)
        out = np.zeros(int(offsets[-1]), np.float32)
        self.ctx.check(L.lib().fa_luxtts_finish(self.ctx.handle, self._h, A.ptr(audio), audio.shape[1], A.ptr(offsets), A.ptr(out)), "fa_luxtts_finish")
        return [out[offsets[b]:offsets[b + 1]] for b in range(self.batch)]

    def get(self, name: str) -> np.ndarray:
        """one slab as a host array: tokens / token_mask [batch, max_tokens], text_condition / speech_condition / x [batch, max_frames,
        n_mels], frame_mask [batch, max_frames], records [batch] (mean_square, rms, gain, status)"""
        c = self.cfg
        if name == "records":
            which, out = 6, np.zeros(self.batch, RECORD)
        elif name in SLABS:
            which, dtype, shape = SLABS[name]
            out = np.zeros((self.batch,) + {"max_tokens": (c.max_tokens,), "max_frames": (c.max_frames,), "rows": (c.max_frames, c.n_mels)}[shape], dtype)
        else:
            raise A.invalid("LuxTtsSession.get", f"no slab {name}")
        self.ctx.check(L.lib().fa_luxtts_session_get(self.ctx.handle, self._h, which, A.ptr(out)), "fa_luxtts_session_get")
        return out
