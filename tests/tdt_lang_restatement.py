"""The float64 yardstick of the TDT walk's language mode (fa_tdt_greedy_logits_lang_dev, fa_tdt_topk_rows_dev, fa_tdt_token_classes;
csrc/tdt_lang.h, csrc/tdt_lang_host.hip): `matches`, `filter_top_k` and `apply_english_blocklist` as the reference has them
(Shared/TokenLanguageFilter.swift:81-186, TdtDecoderV3.swift:635-703), the ordered top-K list as THIS LIBRARY defines it, the control
loop of TdtDecoderV3.decodeWithTimings taking raw or filtered decisions, the bound a replaced token's confidence is held to, a float32
emulation of the device's order of operations, and the table of cases tests/test_tdt_lang_cpu.py checks and tests/test_gpu_tdt_lang.py
runs.  Plain numpy, no GPU.

The list (CoreML's top_k_ids / top_k_logits come from a model outside the reference tree, and their order among equal logits is not
specified; this is the library's definition): the key of token i is its logit widened to float32, NaN counting as -inf; the list is the
min(K, V1) tokens in order of descending key, then ascending id, compared by value (-0.0 == +0.0); the reported logit is the widened
value, NaN reported as -inf."""
from __future__ import annotations

import dataclasses
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_logits_restatement as R  # noqa: E402

LATIN, CYRILLIC, GREEK = 0, 1, 2
SCRIPTS = (LATIN, CYRILLIC, GREEK)
LATIN_OK, CYRILLIC_OK, GREEK_OK, IN_VOCAB, BLOCKLISTED = 1, 2, 4, 8, 16
ROUTE_SCRIPT, ROUTE_BLOCK = 1, 2
BOUNDARY = "▁"
OUTER, INNER, FLUSH = 0, 1, 2
OUTPUT_TOO_SMALL, RUNTIME_ERROR = 3, 5
U24 = R.U24
LANES = R.LANES


# Language.script (TokenLanguageFilter.swift:4-52) by raw value, and TdtDecoderV3.englishBlocklistApplies (:623-625)
LANGUAGES = {**{c: LATIN for c in "en es fr de it pt ro nl da sv fi hu et lv lt mt pl cs sk sl hr bs".split()},
             **{c: CYRILLIC for c in "ru uk be bg sr".split()}, "el": GREEK}


def english_blocklist_applies(language) -> bool:
    return language == "fr"


# ---- TokenLanguageFilter

def _letter(v: int) -> bool:
    return 0x41 <= v <= 0x5A or 0x61 <= v <= 0x7A


def _scalar_ok(v: int, script: int) -> bool:
    if script == LATIN:
        return (0x20 <= v <= 0x7F or 0xA0 <= v <= 0xFF or 0x100 <= v <= 0x17F or 0x180 <= v <= 0x24F or 0x300 <= v <= 0x36F
                or 0x1E00 <= v <= 0x1EFF)
    if script == CYRILLIC:
        return 0x400 <= v <= 0x4FF or (0x20 <= v <= 0x7F and not _letter(v))
    assert script == GREEK
    return 0x370 <= v <= 0x3FF or 0x1F00 <= v <= 0x1FFF or 0x300 <= v <= 0x36F or (0x20 <= v <= 0x7F and not _letter(v))


def matches(text: str, script: int) -> bool:
    """TokenLanguageFilter.matches (:81-134).  Every U+2581 scalar is stripped, an empty remainder matches every script, the rest is
    checked scalar by scalar.  Where U+2581 is directly followed by a combining mark (U+0300-036F) Foundation's string search may treat
    the pair as one character and leave it in; the reference's tests pin no such token, and this restatement strips the marker."""
    return all(_scalar_ok(ord(ch), script) for ch in text.replace(BOUNDARY, ""))


def filter_top_k(top_k_ids, top_k_logits, vocabulary: dict, script: int):
    """TokenLanguageFilter.filterTopK (:143-186) in float64 -> (token id, probability) or None."""
    count = min(len(top_k_ids), len(top_k_logits))
    if count <= 0:
        return None
    lg = np.asarray(top_k_logits[:count], np.float64)
    best, best_logit = -1, -np.inf
    for i in range(count):
        text = vocabulary.get(int(top_k_ids[i]))
        if text is None or not matches(text, script):
            continue
        if best < 0 or lg[i] > best_logit:
            best, best_logit = i, lg[i]
    if best < 0:
        return None
    mx = -np.inf
    for v in lg:
        if v > mx:
            mx = v
    if not np.isfinite(mx):
        return int(top_k_ids[best]), 0.0
    with np.errstate(all="ignore"):
        s = float(np.exp(lg - mx).sum())
        if not s > 0:
            return int(top_k_ids[best]), 0.0
        p = float(np.exp(lg[best] - mx)) / s
    return int(top_k_ids[best]), max(0.0, min(1.0, p))


def apply_english_blocklist(label: int, score: float, top_k_ids, top_k_logits, vocabulary: dict, blank_id: int, blocklist):
    """TdtDecoderV3.applyEnglishBlocklist (:635-667) in float64 -> (label, score).  The reference sums over all of topKLogits and
    indexes the common prefix; its callers hand it lists of equal length."""
    if label == blank_id or label not in blocklist:
        return label, score
    count = min(len(top_k_ids), len(top_k_logits))
    lg = np.asarray(top_k_logits, np.float64)
    best, best_logit = -1, -np.inf
    for i in range(count):
        tid = int(top_k_ids[i])
        if tid == blank_id or tid in blocklist:
            continue
        text = vocabulary.get(tid)
        if text is not None and matches(text, LATIN):
            if best < 0 or lg[i] > best_logit:
                best, best_logit = i, lg[i]
    if best < 0:
        return label, score
    mx = -np.inf
    for v in lg:
        if v > mx:
            mx = v
    with np.errstate(all="ignore"):
        s = float(np.exp(lg - mx).sum())
        new = float(np.exp(best_logit - mx)) / s if s > 0 else 0.0     # a NaN sum is not > 0
    return int(top_k_ids[best]), new


def token_classes(vocabulary: dict, V1: int, blocklist=()) -> np.ndarray:
    """The class bytes fa_tdt_token_classes computes, from `matches`."""
    out = np.zeros(V1, np.uint8)
    for i in range(V1):
        text = vocabulary.get(i)
        bits = sum(bit for bit, s in ((LATIN_OK, LATIN), (CYRILLIC_OK, CYRILLIC), (GREEK_OK, GREEK)) if matches(text or "", s))
        out[i] = bits | (IN_VOCAB if text is not None else 0) | (BLOCKLISTED if i in blocklist else 0)
    return out


# ---- the list

def ordered_list(row, V1: int, K: int):
    """(ids int32 [min(K, V1)], logits float32) of one fp32 / fp16 row: the definition of the module docstring."""
    x = np.asarray(row)[:V1].astype(np.float32)
    key = np.where(np.isnan(x), np.float32(-np.inf), x)
    order = np.argsort(-key, kind="stable")[:min(K, V1)]               # stable: ascending id among equal keys; -0.0 == +0.0 by value
    return order.astype(np.int32), key[order]


def topk_rows(rows, V1: int, K: int):
    """ordered_list on [R, W] rows, padded to K slots with id -1 and logit -inf -> (ids [R, K], logits [R, K], counts [R])."""
    rows = np.asarray(rows)
    ids = np.full((rows.shape[0], K), -1, np.int32)
    lg = np.full((rows.shape[0], K), -np.inf, np.float32)
    for r in range(rows.shape[0]):
        i, v = ordered_list(rows[r], V1, K)
        ids[r, :i.size], lg[r, :i.size] = i, v
    return ids, lg, np.full(rows.shape[0], min(K, V1), np.int32)


# ---- the bound of a replaced token's confidence

def swap_probability(list_logits, x_best: float) -> float:
    """exp(x_best - M) / sum over the list of exp(x_j - M) in float64; 0 where the list's maximum is not finite (:176, :666)."""
    lg = np.asarray(list_logits, np.float64)
    M = lg.max()
    if not np.isfinite(M):
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.exp(np.float64(x_best) - M) / np.exp(lg - M).sum())


def swap_tolerance(list_logits, x_best: float, V1: int) -> float:
    """Bound on |device confidence - swap_probability| for a replaced token:

        2**-24 * p * (min(n, ceil(V1 / 64)) + 13 + 2.25 (sum_j p_j (M - x_j) + (M - x_best))) + 2**-125

    n = len(list) = min(K, V1), p_j the list's soft-max, p = p_best.  The device computes S = sum over the list of exp(x_j - M), M the
    row's maximum (exact), and returns exp(x_best - M) / S; the count is that of tdt_logits_restatement.tolerance, over the n terms of the
    list in place of the V1 of the row.  Every term is positive, so a relative error of a term or of a partial sum is at most that
    relative error of S, and of p.  In units of 2**-24, one float32 rounding:

    - min(n, ceil(V1 / 64)): the additions on one lane's partial sum.  A lane adds those of its elements l, l + 64, ... that are above
      the K-th key: at most its ceil(V1 / 64) elements and at most the list.
    - 6: the DPP additions of the wavefront's sum.
    - 2: a term is ONE hardware exponential __expf(x_j - M), one ulp = 2; there is no rescale, M is known before the sum starts.
    - 2: the tokens at the K-th key enter as (their number) * __expf(tau - M): the product, 1 (the number is exact), and its addition
      to the wavefront's sum, 1.
    - 2: the numerator's exponential.
    - 1: the division, correctly rounded.  Together 13.
    - 2.25 (sum_j p_j (M - x_j) + (M - x_best)): __expf(d) is exp2(fl(log2e * d)) with d = fl(x - M): the rounding of d, that of the
      product and float32's log2e change the result by 2.25 d 2**-24 relative.  A term's share of S is p_j, the numerator counts whole.
      The sum is computed from the list itself: no entropy bound is needed, the reference knows the list.
    - 2**-125 absolute: a numerator or a quotient below 2**-126 may be flushed to zero, and the sum is at least 1.
    - Widening fp16 is exact, the maximum and the selection of the K-th key are exact, comparing float32 with float64 adds nothing the
      division's rounding has not counted.

    Where swap_probability is 0 by definition (a maximum that is not finite, x_best = -inf) the device must return exactly 0."""
    lg = np.asarray(list_logits, np.float64)
    M = lg.max()
    p = swap_probability(lg, x_best)
    if not np.isfinite(M) or p == 0.0 and np.isneginf(x_best):
        return 0.0
    with np.errstate(all="ignore"):
        w = np.exp(lg - M)
        gap = np.where(w > 0, M - lg, 0.0)
        spread = float((w / w.sum() * gap).sum())
    n_add = min(lg.size, math.ceil(V1 / LANES))
    return U24 * p * (n_add + 13.0 + 2.25 * (spread + (M - float(x_best)))) + 2.0 ** -125


def device_order_emulation(row, V1: int, K: int, x_best: float) -> np.float32:
    """tdt_list_sum and the quotient in float32 and in the device's order, for a row whose maximum is finite: lane l adds
    exp(x - M) over its elements l, l + 64, ... above the K-th key tau, the DPP sum over the lanes, + ties * exp(tau - M),
    exp(x_best - M) / that.  numpy's float32 exp stands in for __expf."""
    x = np.asarray(row)[:V1].astype(np.float32)
    key = np.where(np.isnan(x), np.float32(-np.inf), x)
    _, lst = ordered_list(row, V1, K)
    M, tau = lst[0], lst[-1]
    ties = int((lst == tau).sum())
    s = np.zeros((1, LANES), np.float32)
    with np.errstate(all="ignore"):
        for k in range(V1):
            if key[k] > tau:
                s[0, k % LANES] = np.float32(s[0, k % LANES] + np.exp(np.float32(key[k] - M)))
        S = np.float32(R._wave_sum(s)[0] + np.float32(np.float32(ties) * np.exp(np.float32(tau - M))))
        return np.float32(np.exp(np.float32(np.float32(x_best) - M)) / S)


# ---- the control loop, on raw or filtered decisions

@dataclasses.dataclass
class LanguageMode:
    """What transcribe(..., language:) adds to a decision: the script, the vocabulary, the list length, and the blocklist (None: the
    language is not French)."""
    script: int
    vocabulary: dict
    top_k: int = 64
    blocklist: frozenset | None = None


def filter_decision(tok: int, prob: float, row, V1: int, blank_id: int, mode: LanguageMode):
    """The two filters on one main-loop or blank-advance decision (TdtDecoderV3.swift:284-299 / 371-387) -> (token, score, route).
    score is the clamped probability; route 0 leaves (tok, prob) alone."""
    route = 0
    label, score = tok, prob
    ids, lg = ordered_list(row, V1, mode.top_k)
    text = mode.vocabulary.get(label)
    if label != blank_id and text is not None and ids.size and not matches(text, mode.script):     # tokenLanguageFilter (:676-703)
        got = filter_top_k(ids, lg, mode.vocabulary, mode.script)
        if got is not None:
            label, score = got[0], float(R.clamp(got[1]))
            route |= ROUTE_SCRIPT
    if mode.blocklist is not None:
        new, sc = apply_english_blocklist(label, score, ids, lg, mode.vocabulary, blank_id, mode.blocklist)
        if new != label:
            label, score = new, float(R.clamp(sc))
            route |= ROUTE_BLOCK
    return label, score, route


def walk(decide, U: int, T: int, enc_len: int, audio_frames=None, t0: int = 0, is_last: bool = False, global_offset: int = 0, emit_after=None,
         blank_id: int = 8192, max_symbols: int = 10, max_tokens: int = 150, blank_limit: int = 5, bins=(0, 1, 2, 3, 4), max_out: int = 512,
         on_decision=None):
    """One chunk of TdtDecoderV3.decodeWithTimings (:103-607).  decide(u, frame, phase) -> (token, bin, probability, route): one joint
    decision, already filtered where the caller is in language mode (phase tells it: the flush is never filtered).  The dict of
    oracle.tdt_greedy plus routes, swap_counts and trace, the decisions in order as (phase, u, frame, token, route, emitted index or -1)."""
    out = dict(tokens=[], timestamps=[], durations=[], confidences=[], routes=[])
    count, st, u, calls = 0, 0, 0, 0
    swaps = [0, 0]
    trace = []
    final_time = None

    def done():
        n = min(count, max_out)
        return dict(status=st, tokens=np.array(out["tokens"][:n], np.int32), timestamps=np.array(out["timestamps"][:n], np.int32),
                    durations=np.array(out["durations"][:n], np.int32), confidences=np.array(out["confidences"][:n], np.float64),
                    routes=np.array(out["routes"][:n], np.int32), count=count, final_time=final_time, final_u=u, joint_calls=calls,
                    swap_counts=tuple(swaps), trace=trace)

    if enc_len <= 1:
        return done()
    Teff = min(enc_len, enc_len if audio_frames is None else audio_frames)
    t = t0
    if t >= Teff:
        return done()
    last = Teff - 1
    phase, last_emit_t, n_at_t, processed, t_label = OUTER, -1, 0, 0, t
    steps = blanks = fp = 0

    def emit(ts, tok, dur, prob, route):
        nonlocal count, st
        if emit_after is not None and ts < emit_after:
            return -1
        if count < max_out:
            for key, v in (("tokens", tok), ("timestamps", ts), ("durations", dur), ("confidences", float(R.clamp(prob))), ("routes", route)):
                out[key].append(v)
        else:
            st = OUTPUT_TOO_SMALL
        count += 1
        return count - 1

    while True:
        if phase == FLUSH:
            if not (steps < max_symbols and blanks < blank_limit):
                break
            sel = steps % 3
            frame = min(fp, enc_len - 1) if sel == 0 else (min(Teff - 1, enc_len - 1) if sel == 1 else min(max(0, Teff - 2), enc_len - 1))
        else:
            if phase == INNER:
                t_label = t
            frame = min(t, last)
        if u >= U or frame < 0 or frame >= T:
            st = OUTPUT_TOO_SMALL
            return done()
        tok, bi, prob, route = decide(u, frame, phase)
        calls += 1
        swaps[0] += route & 1
        swaps[1] += (route >> 1) & 1
        trace.append([phase, u, frame, tok, route, -1])
        if bi < 0 or bi >= len(bins):
            st = RUNTIME_ERROR
            return done()
        dur = bins[bi]
        blank = tok == blank_id
        if phase == FLUSH:
            if blank:
                blanks += 1
            else:
                blanks = 0
                trace[-1][5] = emit(min(fp, Teff - 1) + global_offset, tok, dur, prob, route)
                u += 1
            fp = min(fp + max(1, dur), Teff)
            steps += 1
            continue
        if phase == OUTER:
            if not blank and dur == 0 and t == last_emit_t and n_at_t >= 1:
                dur = 1
            t_label = t
        if blank and dur == 0:
            dur = 1
        t += dur
        active = t < Teff
        if active and blank:
            phase = INNER
            continue
        stop = False
        if active and not blank:
            processed += 1
            if processed > max_tokens:
                stop = True
            else:
                trace[-1][5] = emit(t_label + global_offset, tok, dur, prob, route)
                u += 1
                if t_label == last_emit_t:
                    n_at_t += 1
                else:
                    last_emit_t, n_at_t = t_label, 1
                if n_at_t >= max_symbols:
                    t = min(t + 1, last)
                    n_at_t, last_emit_t = 0, -1
        active = t < Teff
        if active and not stop:
            phase = OUTER
            continue
        if not is_last:
            break
        phase, steps, blanks, fp = FLUSH, 0, 0, t
    final_time = t
    return done()


def walk_tables(tok, dur_bin, prob, enc_len, audio_frames=None, t0=0, is_last=False, global_offset=0, emit_after=None, **kw):
    """walk on [U, T] decision tables with language = nil: what oracle.tdt_greedy computes."""
    U, T = np.asarray(tok).shape
    return walk(lambda u, f, phase: (int(tok[u][f]), int(dur_bin[u][f]), float(prob[u][f]), 0), U, T, enc_len, audio_frames, t0, is_last,
                global_offset, emit_after, **kw)


def walk_logits(logits, V1: int, nd: int, enc_len: int, mode: LanguageMode | None, on_row=None, **kw):
    """walk on the joint logits [U, T, W] of one chunk: every decision is tdt_logits_restatement.reference on its row, filtered by
    filter_decision outside the flush when mode is given.  on_row(u, frame, phase): called before a cell is read (the case table lays
    its rows out with it).  Adds `decisions`: per trace entry (raw token, probability, list logits or None, x_best or None)."""
    U, T = logits.shape[:2]
    blank_id = kw.get("blank_id", 8192)
    decisions = []

    def decide(u, frame, phase):
        if on_row is not None:
            on_row(u, frame, phase)
        row = logits[u, frame]
        tok, bn, prob = (v.item() for v in R.reference(row, V1, nd))
        raw = tok
        route, lst, xb = 0, None, None
        if mode is not None and phase != FLUSH:
            tok, score, route = filter_decision(tok, prob, row, V1, blank_id, mode)
            if route:
                lst = ordered_list(row, V1, mode.top_k)[1]
                key = np.asarray(row)[tok].astype(np.float32)
                xb = float(-np.inf if np.isnan(key) else key)
                prob = score
        decisions.append((raw, prob, lst, xb))
        return tok, bn, prob, route

    r = walk(decide, U, T, enc_len, **kw)
    r["decisions"] = decisions
    return r


# ---- the case table of the GPU test

KINDS = ("swap_rank1", "swap_rankKm1", "match_at_rankK", "tie_in", "tie_out", "swap_to_blank", "swap_inner", "winner_absent", "no_match",
         "block_swap", "block_after_script", "block_no_alternative", "max_pinf", "match_ninf", "flush_wrong_script")
BLOCK_KINDS = ("block_swap", "block_after_script", "block_no_alternative")
MUST_DIFFER = ("swap_rank1", "swap_rankKm1", "swap_to_blank", "swap_inner", "block_swap", "block_after_script")   # a build without filters fails these
ND = 5
TOP, NOISE_MAX = 20.0, 3.0


def vocabulary_of(V1: int):
    """A synthetic vocabulary of V1 tokens, blank = V1 - 1, and its blocklist.  By id mod 16: 0, 4, 8, 12 Latin; 1, 9, 13 Cyrillic;
    2, 10, 14 Greek; 3 / 5 / 6 a blocklisted Latin / Cyrillic / Greek token; 7 absent from the vocabulary; 11 digits (every script);
    15 the bare boundary marker (every script).  The blank is the bare marker: a legal candidate of the script filter in every script."""
    vocab, block = {}, set()
    for i in range(V1):
        m = i % 16
        if m == 7:
            continue
        if m in (0, 4, 8, 12, 3):
            vocab[i] = f"{BOUNDARY}le{'abcdefgh'[i % 8]}"
        elif m in (1, 9, 13, 5):
            vocab[i] = f"{BOUNDARY}при{'абвгдежз'[i % 8]}"
        elif m in (2, 10, 14, 6):
            vocab[i] = f"{BOUNDARY}λό{'αβγδεζηθ'[i % 8]}"
        elif m == 11:
            vocab[i] = f"{i}"
        else:
            vocab[i] = BOUNDARY
        if m in (3, 5, 6):
            block.add(i)
    vocab[V1 - 1] = BOUNDARY
    block.discard(V1 - 1)
    return vocab, frozenset(block)


@dataclasses.dataclass(frozen=True)
class LangCall:
    name: str
    f16: bool
    V1: int
    script: int
    K: int = 64
    blocklist: bool = True
    pad: int = 0

    @property
    def W(self) -> int:
        return self.V1 + ND + self.pad

    @property
    def np_dtype(self):
        return np.float16 if self.f16 else np.float32

    @property
    def kinds(self):
        return tuple(k for k in KINDS if self.blocklist or k not in BLOCK_KINDS)

    def instance(self, tdt_route) -> str:
        return R.Call(self.name, "lang", self.f16, self.V1, pad=self.pad).instance(tdt_route)

    def form(self, tdt_route) -> str:
        return R.Call(self.name, "lang", self.f16, self.V1, pad=self.pad).form(tdt_route)


# one call per kernel instance (fp16 rows of an even length are pairs, of an odd length halves; pad elements are poison), V1 = 129, 1 088, 1 089 and 8 193 at
# K = 64, one call at K = 3, every script, and the rows of one call again without the blocklist
LANG_CALLS = (
    LangCall("f32_registers_V129_latin", False, 129, LATIN),
    LangCall("f16_pairs_V129_cyrillic", True, 129, CYRILLIC, pad=2),
    LangCall("f16_halves_V1088_greek", True, 1088, GREEK),
    LangCall("f32_streaming_V1089_cyrillic", False, 1089, CYRILLIC, pad=1),
    LangCall("f16_streaming_V8193_latin", True, 8193, LATIN),
    LangCall("f32_streaming_V8193_greek", False, 8193, GREEK),
    LangCall("f32_registers_V129_latin_K3", False, 129, LATIN, K=3),
    LangCall("f32_registers_V129_latin_no_blocklist", False, 129, LATIN, blocklist=False),
    LangCall("f16_pairs_V129_cyrillic_no_blocklist", True, 129, CYRILLIC, blocklist=False, pad=2),
)
LANG_BY_NAME = {c.name: c for c in LANG_CALLS}
CHUNK_T = 24          # T == enc_len of every chunk
CHUNK_U = CHUNK_T + 4 # decoder steps a chunk has room for, the flush's included; max_out too


def _pools(call: LangCall, vocab, block):
    V1, blank = call.V1, call.V1 - 1
    ids = [i for i in range(V1 - 1)]
    ok = lambda i, s: i in vocab and matches(vocab[i], s)  # noqa: E731
    letters = lambda i: i in vocab and not all(matches(vocab[i], s) for s in SCRIPTS)  # noqa: E731  (not script-neutral)
    return dict(
        good=[i for i in ids if ok(i, call.script) and letters(i) and i not in block],                  # right script, not blocklisted
        wrong=[i for i in ids if i in vocab and not matches(vocab[i], call.script) and i not in block],   # in the vocabulary, wrong script
        wrong_not_latin=[i for i in ids if i in vocab and not matches(vocab[i], call.script) and not matches(vocab[i], LATIN) and i not in block],
        filler=[i for i in ids if i not in vocab or not matches(vocab[i], call.script)],                  # never a candidate of the script filter
        absent=[i for i in ids if i not in vocab],
        blocked=[i for i in ids if i in block and ok(i, call.script)],                                   # right script, blocklisted
        latin=[i for i in ids if ok(i, LATIN) and letters(i) and i not in block],
        not_latin=[i for i in ids if i not in vocab or not matches(vocab[i], LATIN)],                     # never a candidate of the blocklist
        blank=blank)


def _row(call: LangCall, kind: str, pools, rng):
    """One row [V1 + ND] of the kind, float32 values the call's dtype holds exactly: noise below NOISE_MAX, the tokens that make the
    kind at TOP and in steps of 1 / 8 below it, duration bin 1 (one frame) by a margin."""
    V1, K = call.V1, call.K
    dt = call.np_dtype
    x = np.minimum(rng.standard_normal(V1 + ND), NOISE_MAX).astype(dt).astype(np.float32)
    x[V1:] = np.array([0.0, 9.0, 1.0, -1.0, 0.5], np.float32)
    level = lambda r: np.float32(TOP - 0.125 * r)  # noqa: E731  (rank r of the list)
    P = pools
    pick = lambda pool, n, avoid=(): [int(i) for i in rng.permutation([j for j in pool if j not in avoid])[:n]]  # noqa: E731

    def ranked(tokens):
        for r, i in enumerate(tokens):
            x[i] = level(r)

    if kind in ("swap_rank1", "swap_inner", "max_pinf"):
        ranked(pick(P["wrong"], 1) + pick(P["good"], 1))
        if kind == "max_pinf":
            x[np.argmax(x[:V1])] = np.inf
    elif kind in ("swap_rankKm1", "match_at_rankK", "no_match"):
        n_wrong = {"swap_rankKm1": K - 1, "match_at_rankK": K, "no_match": K}[kind]
        first = pick(P["wrong"], 1)
        ranked(first + pick(P["filler"], n_wrong - 1, avoid=first) + (pick(P["good"], 1) if kind != "no_match" else []))
    elif kind in ("tie_in", "tie_out"):
        # ranks 0 .. K - 2 wrong-script tokens; the key of rank K - 1 is shared by a wrong-script and a right-script token: the lower id is in
        assert K >= 2
        good = pick(P["good"][1:-1], 1)[0]
        rival = int(rng.choice([i for i in P["filler"] if (i < good) == (kind == "tie_out")]))
        first = pick(P["wrong"], 1, avoid=(rival,))
        ranked(first + pick(P["filler"], K - 2, avoid=first + [rival]))
        x[rival] = x[good] = level(K - 1)
    elif kind == "swap_to_blank":
        ranked(pick(P["wrong"], 1) + [P["blank"]] + pick(P["good"], 1))
    elif kind == "winner_absent":
        ranked(pick(P["absent"], 1) + pick(P["good"], 1))
    elif kind == "block_swap":
        ranked(pick(P["blocked"], 1) + pick(P["not_latin"], 1) + pick(P["latin"], 1))
    elif kind == "block_after_script":
        ranked(pick(P["wrong_not_latin"], 1) + pick(P["blocked"], 1) + pick(P["latin"], 1))
    elif kind == "block_no_alternative":
        first = pick(P["blocked"], 1)
        ranked(first + [P["blank"]] + pick(sorted(set(P["blocked"] + P["not_latin"])), K - 2, avoid=first))
    elif kind == "match_ninf":                                        # nothing above -inf but the winner: the list goes on by ascending id
        x[:V1] = -np.inf
        x[pick([i for i in P["wrong"] if i > 2 * K + 16] or P["wrong"], 1)[0]] = np.float32(TOP)
    elif kind == "flush_wrong_script":
        ranked(pick(P["wrong"], 1) + pick(P["good"], 1))
    elif kind == "blank":
        x[P["blank"]] = np.float32(TOP)
    elif kind == "plain":                                             # a right-script winner: the common case, one byte load
        ranked(pick(P["good"], 1))
    else:
        assert kind == "random", kind
        x[:V1] = (rng.standard_normal(V1) * 3.0).astype(dt).astype(np.float32)
    return x.astype(dt)


@dataclasses.dataclass
class LangTable:
    call: LangCall
    vocabulary: dict
    blocklist: frozenset
    classes: np.ndarray            # uint8 [V1]
    logits: np.ndarray             # [B, U, T, W] of the call's dtype
    is_last: np.ndarray            # int32 [B]
    cells: list                    # [B] {(u, frame): kind}: where the rows of the kinds lie
    expected: list                 # [B] walk_logits in language mode
    unfiltered: list               # [B] walk_logits with language = nil

    @property
    def B(self) -> int:
        return self.logits.shape[0]

    def mode(self) -> LanguageMode:
        return LanguageMode(self.call.script, self.vocabulary, self.call.K, self.blocklist if self.call.blocklist else None)


def lang_table(call: LangCall) -> LangTable:
    """The call's chunks.  As tdt_logits_restatement.diagonal puts row k of a chunk at (k, k) because its walk emits one token per frame,
    a chunk here puts the next row of its list at the cell the walk reads next — the walk itself lays the rows out —: the path leaves
    the diagonal where a decision is (or becomes) a blank.  Cells the walk never reads hold random rows.  Chunk 0: the kinds up to the
    inner-loop swap; chunk 1: the rest, random rows, and as the last chunk its flush rows, the first with a wrong-script winner."""
    vocab, block = vocabulary_of(call.V1)
    pools = _pools(call, vocab, block)
    rng = np.random.default_rng([call.V1, int(call.f16), call.script, call.K])
    kinds = list(call.kinds)
    split = kinds.index("winner_absent")
    main = [kinds[:split], kinds[split:-1]]
    main[0] = [k for kind in main[0] for k in ((["blank", kind] if kind == "swap_inner" else [kind]) + ["plain"])]
    main[1] = [k for kind in main[1] for k in (kind, "plain")] + ["random"] * 4
    flush = [[], ["flush_wrong_script", "blank", "plain"]]
    T, U, V1, W, dt = CHUNK_T, CHUNK_U, call.V1, call.W, call.np_dtype
    B = 2
    lg = np.empty((B, U, T, W), dt)
    lg[..., :V1 + ND] = (rng.standard_normal((B, U, T, V1 + ND), dtype=np.float32) * 3.0).astype(dt)
    lg[..., V1 + 1] = dt(12.0)                                      # (off the path too every row takes one frame)
    if call.pad:
        lg[..., V1 + ND:] = R.poison(B * U * T * call.pad, dt, call.pad).reshape(B, U, T, call.pad)
    mode = LanguageMode(call.script, vocab, call.K, block if call.blocklist else None)
    is_last = np.array([0, 1], np.int32)
    cells, expected, unfiltered = [], [], []
    kw = dict(blank_id=V1 - 1, max_out=U)
    for b in range(B):
        placed, queue, fqueue = {}, list(main[b]), list(flush[b])

        def on_row(u, frame, phase, b=b, placed=placed, queue=queue, fqueue=fqueue):
            if (u, frame) in placed:
                return
            src = fqueue if phase == FLUSH else queue
            kind = src.pop(0) if src else ("blank" if phase == FLUSH else "plain")
            if phase == OUTER and kind == "swap_inner":               # (kept for the cell behind a blank)
                src.insert(0, kind)
                kind = "blank"
            placed[(u, frame)] = kind
            lg[b, u, frame, :V1 + ND] = _row(call, kind, pools, rng)

        walk_logits(lg[b], V1, ND, T, mode, on_row=on_row, is_last=bool(is_last[b]), **kw)
        assert not queue and not fqueue, (call.name, b, queue, fqueue)
        cells.append(placed)
        expected.append(walk_logits(lg[b], V1, ND, T, mode, is_last=bool(is_last[b]), **kw))
        unfiltered.append(walk_logits(lg[b], V1, ND, T, None, is_last=bool(is_last[b]), **kw))
    lg.setflags(write=False)
    return LangTable(call, vocab, block, token_classes(vocab, V1, block), lg, is_last, cells, expected, unfiltered)


def kind_outcomes(table: LangTable):
    """{kind: [(chunk, trace entry, decision)]} of the language-mode walk: every decision read from a cell that holds a row of a kind."""
    out = {}
    for b, r in enumerate(table.expected):
        for entry, dec in zip(r["trace"], r["decisions"]):
            kind = table.cells[b].get((entry[1], entry[2]))
            if kind in KINDS:
                out.setdefault(kind, []).append((b, entry, dec))
    return out


def check_outcomes(table: LangTable):
    """Every kind of the call is there and got the outcome its name says — from the restatement alone."""
    call, vocab, block, blank = table.call, table.vocabulary, table.blocklist, table.call.V1 - 1
    K = min(call.K, call.V1)
    seen = kind_outcomes(table)
    assert set(seen) >= set(call.kinds), (call.name, sorted(set(call.kinds) - set(seen)))
    script_ok = lambda i: i in vocab and matches(vocab[i], call.script)  # noqa: E731
    for kind in call.kinds:
        hits = [h for h in seen[kind] if (h[1][0] == FLUSH) == (kind == "flush_wrong_script")]
        assert hits, (call.name, kind)
        for b, (phase, u, frame, tok, route, emitted), (raw, prob, lst, xb) in hits:
            where = (call.name, kind, b, u, frame)
            row = table.logits[b, u, frame]
            ids, lgs = ordered_list(row, call.V1, call.K)
            rank = {int(i): r for r, i in enumerate(ids)}
            if kind in ("swap_rank1", "swap_inner", "max_pinf"):
                assert route == ROUTE_SCRIPT and rank[tok] == 1 and script_ok(tok) and not script_ok(raw), where
                assert (phase == INNER) == (kind == "swap_inner"), where
                if kind == "max_pinf":
                    assert np.isposinf(lgs[0]) and prob == 0.0, where
            elif kind == "swap_rankKm1":
                assert route == ROUTE_SCRIPT and rank[tok] == K - 1 and script_ok(tok) and not script_ok(raw), where
            elif kind in ("match_at_rankK", "no_match", "winner_absent", "tie_out"):
                assert route == 0 and tok == raw, where
                if kind == "winner_absent":
                    assert raw not in vocab and script_ok(int(ids[1])), where
                else:
                    assert raw in vocab and not script_ok(raw) and not any(script_ok(int(i)) for i in ids), where
                if kind in ("match_at_rankK", "tie_out"):            # the best match is the first token behind the list
                    nxt = ordered_list(row, call.V1, min(call.K + 1, call.V1))[0][-1]
                    assert script_ok(int(nxt)), where
                if kind == "tie_out":
                    full = ordered_list(row, call.V1, call.V1)
                    assert full[1][K] == full[1][K - 1] and full[0][K - 1] < full[0][K], where
            elif kind == "tie_in":
                full = ordered_list(row, call.V1, call.V1)
                assert route == ROUTE_SCRIPT and rank[tok] == K - 1 and full[1][K] == full[1][K - 1] and tok < full[0][K], where
            elif kind == "swap_to_blank":
                assert route == ROUTE_SCRIPT and tok == blank and raw != blank and emitted == -1, where
                nxt = table.expected[b]["trace"]
                i = next(j for j, e in enumerate(nxt) if e[1] == u and e[2] == frame and e[0] == phase)
                assert nxt[i + 1][0] == INNER and nxt[i + 1][3] != blank and nxt[i + 1][5] >= 0, where   # ... and leaves through the inner loop
            elif kind == "block_swap":
                assert route == ROUTE_BLOCK and raw in block and tok not in block and matches(vocab[tok], LATIN) and tok != blank, where
            elif kind == "block_after_script":
                assert route == ROUTE_SCRIPT | ROUTE_BLOCK and not script_ok(raw) and int(ids[1]) in block and tok == int(ids[2]), where
            elif kind == "block_no_alternative":
                assert route == 0 and tok == raw and raw in block, where
                assert all(int(i) == blank or int(i) in block or int(i) not in vocab or not matches(vocab[int(i)], LATIN) for i in ids), where
            elif kind == "match_ninf":
                assert route == ROUTE_SCRIPT and np.isneginf(xb) and prob == 0.0 and np.isfinite(lgs[0]) and np.isneginf(lgs[1:]).all(), where
            else:
                assert kind == "flush_wrong_script" and phase == FLUSH and route == 0 and tok == raw, where
                assert raw in vocab and not script_ok(raw) and emitted >= 0 and table.expected[b]["routes"][emitted] == 0, where


def differs_without_filters(table: LangTable):
    """The kinds whose cell decides another token when the filters are ignored (language = nil)."""
    out = set()
    for kind, hits in kind_outcomes(table).items():
        for b, entry, dec in hits:
            if entry[0] != FLUSH and entry[3] != dec[0]:
                out.add(kind)
    same_tokens = all(np.array_equal(e["tokens"], n["tokens"]) for e, n in zip(table.expected, table.unfiltered))
    return out, same_tokens
