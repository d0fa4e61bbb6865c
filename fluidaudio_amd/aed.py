"""Greedy decoding for the attention encoder-decoder (AED) models over the HIP C ABI (csrc/aed.hip, csrc/aed_host.hip,
csrc/aed_core.h): the host loop of Cohere Transcribe (reference: Sources/FluidAudio/ASR/Cohere/CoherePipeline.swift:525-959) and of
Canary (Sources/FluidAudio/ASR/Canary/CanaryManager.swift:50-275) — the decode step with its repetition penalty and no-repeat
n-gram ban, the attention masks, Canary's encoder transpose and hidden-row gather, the long-form window plan and the
longest-common-substring seam merge.  The networks, the mel front end, tokenizers and detokenisation stay the caller's.

A NaN logit never wins an argmax: that is this library's definition, NaN logits are outside the reference's contract."""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import _args as A, _lib as L

AED_MODEL_COHERE, AED_MODEL_CANARY = 0, 1
AED_FEED_TOKEN, AED_FEED_SEQUENCE = 0, 1
AED_RUNNING, AED_END_EOS, AED_END_CAP = 0, 1, 2
AED_MAX_WINDOW_TOKENS = 64

_invalid = functools.partial(A.invalid, "aed")


@dataclass
class AedConfig:  # fa_aed_config
    mode: int = AED_FEED_TOKEN
    vocab: int = 16384
    eos_id: int = 3
    max_seq: int = 108
    max_new: int = 108
    no_repeat_ngram: int = 3
    repetition_penalty: float = 1.1
    window_tokens: int = 32
    min_match: int = 4
    chunk_samples: int = 560_000
    hop_samples: int = 480_000

    @classmethod
    def preset(cls, model: int) -> "AedConfig":
        c = L.AedConfig()
        L.lib().fa_aed_default_config(C.byref(c), int(model))
        return cls(c.mode, c.vocab, c.eos_id, c.max_seq, c.max_new, c.no_repeat_ngram, float(np.float32(c.repetition_penalty)), c.window_tokens, c.min_match,
                   c.chunk_samples, c.hop_samples)

    @classmethod
    def cohere(cls) -> "AedConfig":
        return cls.preset(AED_MODEL_COHERE)

    @classmethod
    def canary(cls) -> "AedConfig":
        return cls.preset(AED_MODEL_CANARY)

    def c(self) -> L.AedConfig:
        return L.AedConfig(int(self.mode), int(self.vocab), int(self.eos_id), int(self.max_seq), int(self.max_new), int(self.no_repeat_ngram),
                           float(self.repetition_penalty), int(self.window_tokens), int(self.min_match), 0, int(self.chunk_samples), int(self.hop_samples))

    @property
    def max_out(self) -> int:
        c = self.c()
        return int(L.lib().fa_aed_max_out(C.byref(c)))


AedResult = namedtuple("AedResult", "tokens counts reasons steps")   # tokens: one int32 array per utterance


def _mask_dtype(name):
    if name in (None, "float32", "float16"):
        return L.DTYPE_F16 if name == "float16" else L.DTYPE_F32
    raise _invalid("a mask is float32 or float16")


class AedDecodeState:
    """The decode state of a batch of utterances on the device (fa_aed_begin_dev / fa_aed_step_dev / fa_aed_finish).  prompts: one
    sequence of token ids per utterance (at least one token each).  What the network takes for the coming step stays on the device:
    token feed ``input_id`` / ``position_id`` [B] int32 and, with self_mask="float32" / "float16", ``self_mask`` [B, max_seq] of that dtype (0 /
    -1e4; in float16 the bits 0xF0E2); sequence feed ``input_ids`` [B, max_seq] int32 and ``decoder_mask`` float32."""

    def __init__(self, prompts, config: AedConfig | None = None, self_mask: str | None = None, ctx: L.Context | None = None):
        import torch
        self.config = config or AedConfig.cohere()
        self.ctx = ctx or L.default_context()
        self._cfg = self.config.c()
        prompts = [np.ascontiguousarray(p, np.int32).reshape(-1) for p in prompts]
        B = self.batch = len(prompts)
        lens = np.array([p.size for p in prompts], np.int32)
        nbytes = int(L.lib().fa_aed_state_bytes(C.byref(self._cfg), B))
        if nbytes <= 0 or (lens < 1).any():
            raise _invalid("a config the library accepts, at least one utterance and at least one prompt token each")
        dev = torch.device("cuda", self.ctx.device)
        stride = int(lens.max())
        packed = np.zeros((B, stride), np.int32)
        for b, p in enumerate(prompts):
            packed[b, :p.size] = p
        S = self.config.max_seq
        seq = self.config.mode == AED_FEED_SEQUENCE
        self._mask_dtype = _mask_dtype(self_mask)
        self.state = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        self.input_id = self.position_id = self.self_mask = self.input_ids = self.decoder_mask = None
        if seq:
            self.input_ids = torch.zeros((B, S), dtype=torch.int32, device=dev)
            self.decoder_mask = torch.zeros((B, S), dtype=torch.float32, device=dev)
        else:
            self.input_id = torch.zeros(B, dtype=torch.int32, device=dev)
            self.position_id = torch.zeros(B, dtype=torch.int32, device=dev)
            if self_mask is not None:
                self.self_mask = torch.zeros((B, S), dtype=torch.float16 if self_mask == "float16" else torch.float32, device=dev)
        d_prompts = A.to_device(packed, np.int32, dev)
        p = A.ptr
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_aed_begin_dev(self.ctx.handle, C.byref(self._cfg), B, p(d_prompts), stride, p(lens), p(self.state), p(self.input_id),
                                                    p(self.position_id), p(self.self_mask), self._mask_dtype, p(self.input_ids), p(self.decoder_mask)),
                           "fa_aed_begin_dev")

    def step(self, d_logits, ordered: bool = True):
        """One decode step (fa_aed_step_dev): d_logits a float32 / float16 CUDA tensor [B, W], W >= vocab, rows at stride(0), elements
        contiguous.  One launch; nothing is allocated and nothing waits."""
        import torch
        if not (isinstance(d_logits, torch.Tensor) and d_logits.is_cuda and d_logits.dtype in (torch.float16, torch.float32) and d_logits.dim() == 2
                and d_logits.shape[0] == self.batch and d_logits.shape[1] >= self.config.vocab and (d_logits.shape[1] == 1 or d_logits.stride(1) == 1)):
            raise _invalid("the logits are a float16 / float32 CUDA tensor [batch, >= vocab] with contiguous rows")
        stride = int(d_logits.stride(0)) if self.batch > 1 else int(d_logits.shape[1])
        dt = L.DTYPE_F16 if d_logits.dtype == torch.float16 else L.DTYPE_F32
        p = A.ptr
        with self.ctx.torch_ordered(ordered):
            self.ctx.check(L.lib().fa_aed_step_dev(self.ctx.handle, C.byref(self._cfg), self.batch, p(self.state), p(d_logits), dt, stride, p(self.input_id),
                                                   p(self.position_id), p(self.self_mask), self._mask_dtype, p(self.input_ids), p(self.decoder_mask)), "fa_aed_step_dev")

    def finish(self) -> AedResult:
        """fa_aed_finish: the tokens, counts, end reasons (AED_RUNNING / AED_END_EOS / AED_END_CAP) and steps so far, in one synchronisation."""
        B, M = self.batch, self.config.max_out
        tok, cnt, why, steps = np.zeros((B, M), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_aed_finish(self.ctx.handle, C.byref(self._cfg), B, A.ptr(self.state), M, A.ptr(tok), A.ptr(cnt), A.ptr(why), A.ptr(steps)), "fa_aed_finish")
        return AedResult([tok[b, :cnt[b]].copy() for b in range(B)], cnt, why, steps)

    def finish_dev(self):
        """fa_aed_finish_dev: (tokens [B, max_out], counts, reasons, steps) as int32 tensors on the device, no synchronisation."""
        import torch
        B, M = self.batch, self.config.max_out
        tok = torch.zeros((B, M), dtype=torch.int32, device=self.state.device)
        cnt, why, steps = (torch.zeros(B, dtype=torch.int32, device=self.state.device) for _ in range(3))
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_aed_finish_dev(self.ctx.handle, C.byref(self._cfg), B, A.ptr(self.state), M, A.ptr(tok), A.ptr(cnt), A.ptr(why), A.ptr(steps)),
                           "fa_aed_finish_dev")
        return tok, cnt, why, steps

    def gather_hidden(self, d_dec):
        """The decoder's hidden row pos - 1 of every running utterance (fa_aed_gather_hidden_dev): d_dec a float16 / float32 CUDA tensor
        [B, S, D] with any strides -> float32 [B, D] (rows of finished utterances stay zero)."""
        import torch
        if not (isinstance(d_dec, torch.Tensor) and d_dec.is_cuda and d_dec.dtype in (torch.float16, torch.float32) and d_dec.dim() == 3 and d_dec.shape[0] == self.batch):
            raise _invalid("the decoder output is a float16 / float32 CUDA tensor [batch, S, D]")
        _, S, D = d_dec.shape
        out = torch.zeros((self.batch, D), dtype=torch.float32, device=d_dec.device)
        dt = L.DTYPE_F16 if d_dec.dtype == torch.float16 else L.DTYPE_F32
        with self.ctx.torch_ordered():
            self.ctx.check(L.lib().fa_aed_gather_hidden_dev(self.ctx.handle, C.byref(self._cfg), self.batch, A.ptr(self.state), A.ptr(d_dec), dt, S, D,
                                                            *[int(s) for s in d_dec.stride()], A.ptr(out)), "fa_aed_gather_hidden_dev")
        return out


def encoder_valid_frames(feature_length: int, encoder_seq_len: int, mel_frames: int = 3500, encoder_frames: int = 438) -> int:
    """CoherePipeline.encoderValidFrames: ceil(feature_length * 438 / 3500) through fp64, clamped to [1, encoder_seq_len]."""
    return int(L.lib().fa_aed_encoder_valid_frames(int(feature_length), int(encoder_seq_len), int(mel_frames), int(encoder_frames)))


def cross_attention_mask(valid, encoder_seq_len: int, dtype: str = "float32", ctx: L.Context | None = None):
    """buildCrossAttentionMask for a batch (fa_aed_cross_mask_dev): valid per utterance -> a CUDA tensor [B, encoder_seq_len] of `dtype`."""
    import torch
    ctx = ctx or L.default_context()
    dev = torch.device("cuda", ctx.device)
    v = valid if A.is_dev(valid, "int32", 1) else A.to_device(np.clip(np.asarray(valid, np.int64), -2**31, 2**31 - 1), np.int32, dev)
    out = torch.zeros((v.numel(), int(encoder_seq_len)), dtype=torch.float16 if dtype == "float16" else torch.float32, device=dev)
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_aed_cross_mask_dev(ctx.handle, A.ptr(v), v.numel(), int(encoder_seq_len), _mask_dtype(dtype), A.ptr(out)), "fa_aed_cross_mask_dev")
    return out


def encoder_context(d_enc, lengths, ctx: L.Context | None = None):
    """makeDecoderContext for a batch (fa_aed_encoder_context_dev): d_enc a float16 / float32 CUDA tensor [B, D, T] with any strides (a
    padded time stride included) -> (embeddings float32 [B, T, D], mask float32 [B, T])."""
    import torch
    if not (isinstance(d_enc, torch.Tensor) and d_enc.is_cuda and d_enc.dtype in (torch.float16, torch.float32) and d_enc.dim() == 3):
        raise _invalid("the encoder output is a float16 / float32 CUDA tensor [batch, D, T]")
    ctx = A.context_beside(ctx, d_enc)
    B, D, T = d_enc.shape
    lens = lengths if A.is_dev(lengths, "int32", 1) else A.to_device(lengths, np.int32, d_enc.device)
    if lens.numel() != B:
        raise _invalid("one length per utterance")
    emb = torch.empty((B, T, D), dtype=torch.float32, device=d_enc.device)
    mask = torch.empty((B, T), dtype=torch.float32, device=d_enc.device)
    dt = L.DTYPE_F16 if d_enc.dtype == torch.float16 else L.DTYPE_F32
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_aed_encoder_context_dev(ctx.handle, A.ptr(d_enc), dt, B, D, T, *[int(s) for s in d_enc.stride()], A.ptr(lens), A.ptr(emb), A.ptr(mask)),
                  "fa_aed_encoder_context_dev")
    return emb, mask


AedWindows = namedtuple("AedWindows", "window_range starts lengths")   # recording r owns windows [window_range[r], window_range[r + 1])


def plan_windows(samples, config: AedConfig | None = None) -> AedWindows:
    """The long-form window loop for a batch of recording lengths in samples (fa_aed_plan_windows): no device."""
    cfg = (config or AedConfig.cohere()).c()
    samples = np.ascontiguousarray(samples, np.int64).reshape(-1)
    rng = np.zeros(samples.size + 1, np.int64)
    count = C.c_int64()
    st = L.lib().fa_aed_plan_windows(C.byref(cfg), A.ptr(samples), samples.size, A.ptr(rng), None, None, 0, C.byref(count))
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_aed_plan_windows", "1 <= hop_samples <= chunk_samples and no negative length")
    starts, lens = np.zeros(count.value, np.int64), np.zeros(count.value, np.int64)
    st = L.lib().fa_aed_plan_windows(C.byref(cfg), A.ptr(samples), samples.size, A.ptr(rng), A.ptr(starts), A.ptr(lens), count.value, C.byref(count))
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_aed_plan_windows")
    return AedWindows(rng, starts, lens)


# tokens: flat (numpy, or a torch tensor on the device for merge_token_windows_dev); recording r owns [out_range[r], out_range[r] + counts[r]);
# best_len / best_s_end per window (0 where a side of the seam was empty)
MergedTokens = namedtuple("MergedTokens", "tokens out_range counts best_len best_s_end")


def _merge(where, ctx, tokens, window_offsets, recording_range, window_tokens, min_match, ordered):
    window_offsets, recording_range = np.ascontiguousarray(window_offsets, np.int64), np.ascontiguousarray(recording_range, np.int64)
    if window_offsets.ndim != 1 or window_offsets.size < 1 or recording_range.ndim != 1 or recording_range.size < 1 or (np.diff(window_offsets) < 0).any() or \
            (np.diff(recording_range) < 0).any() or recording_range[0] < 0 or recording_range[-1] > window_offsets.size - 1 or window_offsets[0] < 0 or \
            window_offsets[-1] > (tokens.numel() if hasattr(tokens, "numel") else tokens.size):
        raise _invalid("window_offsets and recording_range ascend inside the tokens and the windows")
    cfg = AedConfig(window_tokens=window_tokens, min_match=min_match).c()
    n, W = recording_range.size - 1, window_offsets.size - 1
    out_range = window_offsets[recording_range] - window_offsets[recording_range[0]]
    out = A.beside(tokens, int(out_range[-1]), "int32")
    counts, best_len, best_end = np.zeros(n, np.int32), np.zeros(W, np.int32), np.zeros(W, np.int32)
    ctx = A.context_beside(ctx, tokens)
    with ctx.torch_ordered(ordered):
        ctx.check(getattr(L.lib(), where)(ctx.handle, C.byref(cfg), A.ptr(tokens), A.ptr(window_offsets), A.ptr(recording_range), n, A.ptr(out), A.ptr(out_range),
                                          A.ptr(counts), A.ptr(best_len), A.ptr(best_end)), where)
    return MergedTokens(out, out_range, counts, best_len, best_end)


def merge_token_windows(windows, window_offsets=None, recording_range=None, window_tokens: int = 32, min_match: int = 4, ctx: L.Context | None = None) -> MergedTokens:
    """mergeTokenStreams folded over each recording's windows (fa_aed_merge_windows).  windows: a list of recordings, each a list of
    token-id sequences — or flat ids with window_offsets [windows + 1] and recording_range [recordings + 1]."""
    if window_offsets is None:
        recording_range = np.concatenate([[0], np.cumsum([len(r) for r in windows])]).astype(np.int64)
        windows, window_offsets = A.ragged([w for r in windows for w in r], None, np.int32)
    tokens = np.ascontiguousarray(windows, np.int32).reshape(-1)
    return _merge("fa_aed_merge_windows", ctx, tokens, window_offsets, recording_range, window_tokens, min_match, False)


def merge_token_windows_dev(d_tokens, window_offsets, recording_range, window_tokens: int = 32, min_match: int = 4, ctx: L.Context | None = None,
                            ordered: bool = True) -> MergedTokens:
    """fa_aed_merge_windows_dev: d_tokens a flat int32 CUDA tensor; the merged streams stay on the device."""
    if not A.is_dev(d_tokens, "int32", 1):
        raise _invalid("the tokens must be a flat contiguous int32 tensor on the device")
    return _merge("fa_aed_merge_windows_dev", ctx, d_tokens, window_offsets, recording_range, window_tokens, min_match, ordered)


def merge_token_streams(prefix, suffix, window_tokens: int = 32, min_match: int = 4, ctx: L.Context | None = None) -> list:
    """CoherePipeline.mergeTokenStreams / CanaryManager.mergeTokenStreams for one seam."""
    m = merge_token_windows([[prefix, suffix]], window_tokens=window_tokens, min_match=min_match, ctx=ctx)
    return m.tokens[:int(m.counts[0])].tolist()
