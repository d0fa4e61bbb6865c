"""Host-side mirror of the streaming RNN-T greedy decoder and its decode-time hotword biasing (reference:
Sources/FluidAudio/ASR/Parakeet/Streaming/RnntDecoder.swift:73-127, Streaming/Nemotron/NemotronVocabularyBias.swift:55-340, 465-498)
over the HIP C ABI (csrc/rnnt.hip, csrc/rnnt_host.hip, csrc/rnnt_bias_core.h).

The decoder and joint networks are CoreML bundles outside the reference's source tree, so ``decode_logits`` walks joint logits indexed by
(decoder steps taken, encoder frame), as ``tdt.decode_logits`` does.  Text folding — lower-casing and NFC — happens here (``fold``); the
reference's letter-count guard (``usableSurfaces``: three grapheme clusters, two for CJK) counts grapheme clusters and stays with the
caller."""
from __future__ import annotations

import ctypes as C
import unicodedata
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _args as A, _lib as L

RNNT_BIAS_DEFAULT_BOOST = 4.5   # NemotronVocabularyBias.defaultBoost
RNNT_BIAS_MAX_BOOST = 6.0       # NemotronVocabularyBias.maxBoost
RNNT_BIAS_MAX_FORM = 256        # FA_RNNT_BIAS_MAX_FORM


@dataclass
class RnntConfig:  # fa_rnnt_config
    blank_id: int = 1024
    eou_id: int = -1
    max_symbols_per_step: int = 10

    def c(self) -> L.RnntConfig:
        return L.RnntConfig(int(self.blank_id), int(self.eou_id), int(self.max_symbols_per_step))


@dataclass
class VocabularyTerm:  # CustomVocabularyTerm: the fields the bias reads
    text: str
    weight: float | None = None
    aliases: tuple = ()


class RnntBias(NamedTuple):
    blob: np.ndarray    # int32 words; empty: decode without a bias
    tail_cap: int
    vocab: int


def fold(text: str) -> str:
    """lowercased().precomposedStringWithCanonicalMapping"""
    return unicodedata.normalize("NFC", text.lower())


def bias_effective_boost(weight, default_boost: float = RNNT_BIAS_DEFAULT_BOOST) -> float:
    """effectiveBoost (:196-199): the weight when one is set and <= 6.0, the default otherwise."""
    return float(L.lib().fa_rnnt_bias_effective_boost(0 if weight is None else 1, 0.0 if weight is None else float(weight), float(default_boost)))


def _utf8(texts):
    out = [None if t is None else (t if isinstance(t, bytes) else str(t).encode("utf-8", "surrogatepass")) for t in texts]
    if any(t is not None and b"\0" in t for t in out):
        raise ValueError("rnnt bias: a text holds a NUL")
    return out


def bias_build(terms, pieces, default_boost: float = RNNT_BIAS_DEFAULT_BOOST, vocab: int | None = None) -> RnntBias:
    """NemotronVocabularyBias.init (:126-182) as the blob fa_rnnt_bias_build lays out.  terms: VocabularyTerm, plain texts or (text, weight)
    pairs; every text and alias is folded and carries the term's effectiveBoost, terms whose boost is not above 0 are dropped (:206).  pieces:
    a sequence of piece texts (None: no piece) or the reference's dict id -> piece; folded here; vocab (default: the largest id + 1) must be the
    vocab_with_blank of the logits the blob is used with.  bytes are taken as already folded UTF-8.  Returns RnntBias(blob, tail_cap, vocab);
    an empty blob means no usable term.  Raises ValueError for text that is not UTF-8 or a form above 256 scalars."""
    if isinstance(pieces, dict):
        n = max(pieces) + 1 if pieces else 0
        pieces = [pieces.get(i) for i in range(n)]
    pieces = list(pieces)
    vocab = len(pieces) if vocab is None else int(vocab)
    assert vocab >= len(pieces), "bias_build: vocab is smaller than the piece table"
    pieces += [None] * (vocab - len(pieces))
    surfaces, boosts = [], []
    for term in terms:
        if isinstance(term, (str, bytes)):
            term = VocabularyTerm(term)
        elif not isinstance(term, VocabularyTerm):
            term = VocabularyTerm(*term)
        boost = bias_effective_boost(term.weight, default_boost)
        if not boost > 0:
            continue
        for surface in (term.text, *(term.aliases or ())):
            surfaces.append(surface)
            boosts.append(boost)
    p_texts = _utf8([p if p is None or isinstance(p, bytes) else fold(p) for p in pieces])
    s_texts = _utf8([s if isinstance(s, bytes) else fold(s) for s in surfaces])
    p_arr = (C.c_char_p * max(vocab, 1))(*p_texts)
    s_arr = (C.c_char_p * max(len(s_texts), 1))(*s_texts)
    b_arr = np.ascontiguousarray(boosts, np.float32)
    need, cap = C.c_int64(), C.c_int32()
    args = (C.cast(p_arr, C.c_void_p), vocab, C.cast(s_arr, C.c_void_p), b_arr.ctypes.data if b_arr.size else None, len(s_texts))
    st = L.lib().fa_rnnt_bias_build(*args, None, 0, C.byref(need), C.byref(cap))
    if st != L.SUCCESS:
        raise ValueError("bias_build: a text is not UTF-8, a boost is not above 0, or a term's piece form is longer than 256 scalars")
    blob = np.zeros(need.value, np.int32)
    if need.value:
        st = L.lib().fa_rnnt_bias_build(*args, blob.ctypes.data, need.value, C.byref(need), C.byref(cap))
        if st != L.SUCCESS:
            raise L.FluidAudioHipError(st, "fa_rnnt_bias_build")
    return RnntBias(blob, int(cap.value), vocab)


def bias_candidates(bias, observed=()) -> dict:
    """candidates() (:280-306) after observe (:254-261) of the token ids `observed` from a reset match state: {token id: boost}, ascending
    ids.  bias: RnntBias or the blob.  Raises ValueError for a malformed blob."""
    blob = np.ascontiguousarray(bias.blob if isinstance(bias, RnntBias) else bias, np.int32)
    obs = np.ascontiguousarray(list(observed), np.int32)
    count = C.c_int32()
    args = (blob.ctypes.data if blob.size else None, int(blob.size), obs.ctypes.data if obs.size else None, int(obs.size))
    st = L.lib().fa_rnnt_bias_candidates(*args, None, None, 0, C.byref(count))
    if st not in (L.SUCCESS, L.OUTPUT_TOO_SMALL):
        raise ValueError("bias_candidates: not a blob of bias_build")
    ids, boosts = np.zeros(count.value, np.int32), np.zeros(count.value, np.float32)
    if count.value:
        st = L.lib().fa_rnnt_bias_candidates(*args, ids.ctypes.data, boosts.ctypes.data, count.value, C.byref(count))
        if st != L.SUCCESS:
            raise L.FluidAudioHipError(st, "fa_rnnt_bias_candidates")
    return {int(i): float(b) for i, b in zip(ids, boosts)}


def decode_logits(d_logits, vocab_with_blank: int, frames, skip=None, bias: RnntBias | None = None, tails=None, config: RnntConfig | None = None,
                  max_out: int = 256, ctx: L.Context | None = None):
    """The batched streaming greedy walk (fa_rnnt_greedy_logits_dev).  d_logits: a contiguous float32 / float16 CUDA tensor [B, U, T, W],
    W >= vocab_with_blank; frames (validOutLen) and skip (skipFrames, default 0): per-stream ints.  bias: bias_build(...) for this
    vocab_with_blank, or None / an empty blob for the plain walk; tails: per stream the match state a previous call returned (None or
    empty: resetMatchState).  Returns per stream a dict: tokens, frames (chunk-local), flips (the displaced plain argmax where the bias
    flipped the token, else -1), count, final_u, eou, status and tail (the folded scalars to carry into the next call)."""
    import torch
    ctx = ctx or L.default_context()
    cfg = (config or RnntConfig()).c()
    assert isinstance(d_logits, torch.Tensor) and d_logits.is_cuda, "rnnt.decode_logits: d_logits must be a CUDA tensor"
    assert d_logits.dtype in (torch.float16, torch.float32), f"rnnt.decode_logits: d_logits must be float16 or float32, not {d_logits.dtype}"
    assert d_logits.dim() == 4 and d_logits.is_contiguous(), f"rnnt.decode_logits: d_logits must be contiguous [B, U, T, W], not {tuple(d_logits.shape)}"
    B, U, T, W = d_logits.shape
    assert 1 <= int(vocab_with_blank) <= W, f"rnnt.decode_logits: rows of {W} logits cannot hold {int(vocab_with_blank)}"
    dev = d_logits.device
    biased = bias is not None and bias.blob.size > 0
    cap = int(bias.tail_cap) if biased else 0
    v_frames, v_skip = A.to_device(frames, np.int32, dev), A.to_device(skip, np.int32, dev)
    assert v_frames.numel() == B and (v_skip is None or v_skip.numel() == B), "rnnt.decode_logits: one frame count (and skip) per stream"
    d_blob = d_tail = d_len = None
    if biased:
        d_blob = A.to_device(bias.blob, np.int32, dev)
        h_tail, h_len = np.zeros((B, cap), np.int32), np.zeros(B, np.int32)
        for b, t in enumerate(tails or ()):
            t = np.asarray([] if t is None else t, np.int64)[-cap:]
            h_tail[b, :t.size], h_len[b] = t, t.size
        d_tail, d_len = A.to_device(h_tail, np.int32, dev), A.to_device(h_len, np.int32, dev)
    o_tok, o_frame, o_plain = (A.beside(d_logits, (B, max_out), "int32") for _ in range(3))
    o_cnt, o_fu, o_eou, o_st = (A.beside(d_logits, B, "int32") for _ in range(4))
    p = A.ptr
    dt = L.DTYPE_F16 if d_logits.dtype == torch.float16 else L.DTYPE_F32
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_rnnt_greedy_logits_dev(ctx.handle, C.byref(cfg), p(d_logits), dt, B, U, T, int(vocab_with_blank), W, p(v_frames), p(v_skip),
                                                    p(d_blob), int(bias.blob.size) if biased else 0, cap, p(d_tail), p(d_len), max_out, p(o_tok),
                                                    p(o_frame), p(o_plain), p(o_cnt), p(o_fu), p(o_eou), p(o_st)), "fa_rnnt_greedy_logits_dev")
    ctx.synchronize()
    tok, frm, pln = o_tok.cpu().numpy(), o_frame.cpu().numpy(), o_plain.cpu().numpy()
    cnt, fu, eou, st = o_cnt.cpu().numpy(), o_fu.cpu().numpy(), o_eou.cpu().numpy(), o_st.cpu().numpy()
    tail, tlen = (d_tail.cpu().numpy(), d_len.cpu().numpy()) if biased else (np.zeros((B, 0), np.int32), np.zeros(B, np.int32))
    out = []
    for b in range(B):
        n = min(int(cnt[b]), max_out)
        out.append(dict(status=int(st[b]), tokens=tok[b, :n].copy(), frames=frm[b, :n].copy(), flips=pln[b, :n].copy(), count=int(cnt[b]),
                        final_u=int(fu[b]), eou=bool(eou[b]), tail=tail[b, :int(tlen[b])].copy()))
    return out
