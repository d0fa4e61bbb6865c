"""The vocabulary rescorer's term-centric path on the device (csrc/vocab_rescore.hip, vocab_rescore_host.hip, vocab_rescore_core.h):
candidate discovery by string similarity (VocabularyRescorer+TokenRescoring.swift:755-1033), the CTC verdicts (evaluateCTCMatch,
+TokenEvaluation.swift:29-173) through the word spotter's window kernels, and arbitratePendingReplacements (:272-307).

A word or a form is a sequence of ints, one per Character of the normalized string — any injective numbering with SPACE for the space;
symbols(text) uses the code points.  normalizeForSimilarity, both tokenizers, the word timings and the stopword lists stay with the
caller.  Similarities are the reference's fp32 values bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args as A, _lib as L
from .kws import _Matrix

SPACE = 32
MAX_FORM = 64
ORIGIN_MULTI_WORD, ORIGIN_SINGLE_WORD = 1, 2
WORD_STOPWORD, WORD_MULTI_WORD_STOPWORD = 1, 2
APPLIED, SUPERSEDED, REJECTED, UNAVAILABLE = 1, 2, 3, 4
MIN_SIMILARITY_FLOOR = 0.50        # ContextBiasingConstants.minSimilarityFloor
VR_CANDIDATE_DTYPE, VR_VERDICT_DTYPE = np.dtype(L.VrCandidate), np.dtype(L.VrVerdict)


def symbols(text: str) -> tuple:
    """A normalized string as a row of symbols: the code point of each character (SPACE is the space's)."""
    return tuple(ord(c) for c in text)


def boost(cbw: float, token_count: int, config: L.VrBoostConfig | None = None) -> float:
    """adaptiveCbw (VocabularyRescorer.swift:111-129); config None: the reference's defaults."""
    return float(L.lib().fa_vocab_rescore_boost(float(cbw), int(token_count), A.cfg_ref(config)))


def default_config() -> L.VrDecideConfig:
    cfg = L.VrDecideConfig()
    L.lib().fa_vocab_rescore_default_config(C.byref(cfg))
    return cfg


def build(terms, min_term_length: int = 3) -> np.ndarray:
    """The vocabulary blob (int32 words, position independent).  terms: a sequence of (char_count, min_similarity or None, forms) or of
    dicts with those keys, in file order; forms are the term's normalized forms in buildNormalizedForms' order, the canonical one first
    (it may be empty)."""
    recs = [(t["char_count"], t["min_similarity"], t["forms"]) if isinstance(t, dict) else tuple(t) for t in terms]
    counts = np.asarray([int(c) for c, _, _ in recs] or [0], np.int32)
    mins = np.asarray([-1.0 if m is None else float(m) for _, m, _ in recs] or [0.0], np.float32)
    term_rows = np.concatenate([[0], np.cumsum([len(f) for _, _, f in recs])]).astype(np.int64)
    flat, row_off = A.ragged([r for _, _, f in recs for r in f], None, np.int32)
    if flat.size == 0:
        flat = np.zeros(1, np.int32)
    need, text = C.c_int64(), C.create_string_buffer(256)
    f = L.lib().fa_vocab_rescore_build

    def call(blob, cap):
        return f(counts.ctypes.data, mins.ctypes.data, term_rows.ctypes.data, row_off.ctypes.data, flat.ctypes.data, len(recs), int(min_term_length),
                 A.ptr(blob), cap, C.byref(need), text, len(text))
    st = call(None, 0)
    if st == L.SUCCESS:
        blob = np.zeros(max(need.value, 1), np.int32)
        st = call(blob, need.value) if need.value else st
    if st != L.SUCCESS:
        raise L.FluidAudioHipError(st, "fa_vocab_rescore_build", text.value.decode())
    return blob[:need.value]


def _pack_words(utterances):
    """[(words, flags)] -> utterance offsets, word offsets, flat symbols, flag bytes"""
    utt_off = np.concatenate([[0], np.cumsum([len(w) for w, _ in utterances])]).astype(np.int64)
    flat, word_off = A.ragged([r for w, _ in utterances for r in w], None, np.int32)
    flags = np.asarray([int(f) for _, fl in utterances for f in fl] or [0], np.uint8)
    if sum(len(fl) for _, fl in utterances) != int(utt_off[-1]):
        raise A.invalid("vocab_rescore", "a flag byte per word is required")
    if flat.size == 0:
        flat = np.zeros(1, np.int32)
    return utt_off, word_off, flat, flags


def candidates(blob, utterances, min_similarity: float = MIN_SIMILARITY_FLOOR, capacity: int | None = None, ctx: L.Context | None = None):
    """The candidate records of every (utterance, term) -> (structured array of VR_CANDIDATE_DTYPE in the reference's append order,
    int64 counts per utterance).  utterances: [(words, flags)], a word a sequence of symbols (possibly empty), a flag byte per word
    (WORD_STOPWORD, WORD_MULTI_WORD_STOPWORD).  capacity None: the call is repeated once with the count it reported if 1024 records
    were too few."""
    ctx = ctx or L.default_context()
    blob = np.ascontiguousarray(blob, np.int32)
    utt_off, word_off, flat, flags = _pack_words(utterances)
    B = len(utterances)
    counts = np.zeros(max(B, 1), np.int64)
    n = C.c_int64()
    f = L.lib().fa_vocab_rescore_candidates
    cap = 1024 if capacity is None else int(capacity)

    def call(recs):
        return f(ctx.handle, blob.ctypes.data, blob.size, utt_off.ctypes.data, B, word_off.ctypes.data, flat.ctypes.data, flags.ctypes.data,
                 float(min_similarity), recs.ctypes.data, recs.size, C.byref(n), counts.ctypes.data)
    recs = np.zeros(max(cap, 1), VR_CANDIDATE_DTYPE)
    st = call(recs[:cap])
    if st == L.OUTPUT_TOO_SMALL and capacity is None:
        recs = np.zeros(n.value, VR_CANDIDATE_DTYPE)
        st = call(recs)
    ctx.check(st, f.__name__)
    return recs[:min(n.value, recs.size)].copy(), counts[:B]


def decide(log_probs, cands, words_per_utterance, word_starts, word_ends, term_tokens, alt_tokens, phrase_tokens, config: L.VrDecideConfig | None = None,
           occupied=None, valid_frames=None, vocab: int | None = None, ctx: L.Context | None = None, order: bool = True):
    """evaluateCTCMatch for every candidate and the arbitration per utterance -> (structured array of VR_VERDICT_DTYPE, one record per
    candidate; the applied candidates' indices per utterance in application order).  log_probs [B, T, V]: a torch device tensor or a
    numpy array; cands: VR_CANDIDATE_DTYPE records from candidates() or of the caller's making; word_starts / word_ends: seconds, flat
    over the words of all utterances (words_per_utterance says how many each has); term_tokens / alt_tokens: a token row per term (an
    empty alternative row: none); phrase_tokens: the original phrase's tokens per candidate; occupied: a byte per word."""
    ctx = ctx or L.default_context()
    m = _Matrix(log_probs, vocab)
    cands = np.ascontiguousarray(cands, VR_CANDIDATE_DTYPE)
    n = cands.size
    utt_off = np.concatenate([[0], np.cumsum([int(w) for w in words_per_utterance])]).astype(np.int64)
    if utt_off.size != m.B + 1:
        raise A.invalid("vocab_rescore.decide", "words_per_utterance has to name every utterance of log_probs")
    starts, ends = np.ascontiguousarray(word_starts, np.float64).reshape(-1), np.ascontiguousarray(word_ends, np.float64).reshape(-1)
    if starts.size != utt_off[-1] or ends.size != utt_off[-1] or len(phrase_tokens) != n or len(alt_tokens) != len(term_tokens):
        raise A.invalid("vocab_rescore.decide", "a start and an end per word, a phrase row per candidate and an alternative row per term are required")
    tt, toff = A.ragged(list(term_tokens), None, np.int32)
    at, aoff = A.ragged(list(alt_tokens), None, np.int32)
    pt, poff = A.ragged(list(phrase_tokens), None, np.int32)
    occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(-1)
    if occ is not None and occ.size != utt_off[-1]:
        raise A.invalid("vocab_rescore.decide", "occupied: a byte per word")
    vf = None if valid_frames is None else np.ascontiguousarray(valid_frames, np.int32)
    verdicts = np.zeros(max(n, 1), VR_VERDICT_DTYPE)
    applied, applied_counts = np.zeros(max(n, 1), np.int32), np.zeros(max(m.B, 1), np.int64)
    keep = [np.zeros(1, a.dtype) if a.size == 0 else a for a in (tt, at, pt, starts, ends)]
    f = L.lib().fa_vocab_rescore_decide_dev if m.device else L.lib().fa_vocab_rescore_decide
    with ctx.torch_ordered(order and m.device):
        ctx.check(f(ctx.handle, m.ptr, m.B, m.T, m.V, m.row_stride, m.matrix_stride, A.ptr(vf), A.cfg_ref(config), cands.ctypes.data, n, utt_off.ctypes.data,
                    keep[3].ctypes.data, keep[4].ctypes.data, len(term_tokens), keep[0].ctypes.data, toff.ctypes.data, keep[1].ctypes.data, aoff.ctypes.data,
                    keep[2].ctypes.data, poff.ctypes.data, A.ptr(occ), verdicts.ctypes.data, applied.ctypes.data, applied_counts.ctypes.data), f.__name__)
    ends_at = np.cumsum(applied_counts[:m.B])
    lists = [applied[int(e - c):int(e)].tolist() for e, c in zip(ends_at, applied_counts[:m.B])]
    return verdicts[:n].copy(), lists


def rescore_batch(log_probs, blob, utterances, raw_words, word_starts, word_ends, term_tokens, alt_tokens, encode, min_similarity: float = MIN_SIMILARITY_FLOOR,
                  config: L.VrDecideConfig | None = None, valid_frames=None, vocab: int | None = None, ctx: L.Context | None = None, order: bool = True):
    """ctcTokenRescore's term-centric path round the caller's tokenizer: candidates(), then decide() with the original phrase of every
    candidate — the raw words of its span joined by a space — tokenized by encode(phrase), which is called once per distinct phrase.
    raw_words: the transcript's words per utterance as strings; word_starts / word_ends: a list of times per utterance.
    -> (candidates, verdicts, applied indices per utterance)."""
    ctx = ctx or L.default_context()
    cands, _ = candidates(blob, utterances, min_similarity, ctx=ctx)
    cache, phrases = {}, []
    for c in cands:
        u, first, span = int(c["utterance"]), int(c["first_word"]), int(c["span_len"])
        phrase = " ".join(raw_words[u][first:first + span])
        if phrase not in cache:
            cache[phrase] = [int(t) for t in encode(phrase)]
        phrases.append(cache[phrase])
    flat = lambda rows: [x for r in rows for x in r]   # noqa: E731
    verdicts, applied = decide(log_probs, cands, [len(w) for w, _ in utterances], flat(word_starts), flat(word_ends), term_tokens, alt_tokens, phrases,
                               config=config, valid_frames=valid_frames, vocab=vocab, ctx=ctx, order=order)
    return cands, verdicts, applied
