"""A line-by-line restatement of the host loops round the attention encoder-decoder models: Cohere Transcribe
(Sources/FluidAudio/ASR/Cohere/CoherePipeline.swift:525-634, 670-676, 728-876, 924-969) and Canary
(Sources/FluidAudio/ASR/Canary/CanaryManager.swift:50-130, 187-275).  Plain Python; the repetition penalty in numpy float32, which is
IEEE single precision as Swift's Float is.  Nothing here is computed by the library under test.

NaN logits are outside the reference's contract; the library defines that a NaN never wins, and ``argmax_first`` / ``argmax_strict``
restate that definition (for NaN-free rows they are vDSP_maxvi's first-index maximum and CanaryManager.argmax)."""
import math

import numpy as np

EOS, CAP, RUNNING = 1, 2, 0
MASKED = np.float32(-1.0e4)
MASKED_F16_BITS = 0xF0E2          # float16Bits(-1e4)
COHERE = dict(mode=0, vocab=16384, eos_id=3, max_seq=108, max_new=108, no_repeat_ngram=3, repetition_penalty=1.1, window_tokens=32, min_match=4,
              chunk_samples=560_000, hop_samples=480_000)
CANARY = dict(mode=1, vocab=16384, eos_id=3, max_seq=128, max_new=128, no_repeat_ngram=0, repetition_penalty=1.0, window_tokens=32, min_match=4,
              chunk_samples=240_000, hop_samples=192_000)


def widen(logits):
    """copyLogitsFloat32: fp32 as it is, fp16 widened exactly."""
    return np.asarray(logits).astype(np.float32)


def apply_repetition_penalty(logits, history, penalty):
    """:924-935; logits is a float32 array changed in place."""
    penalty = np.float32(penalty)
    if not (penalty != np.float32(1.0) and len(history) > 0):
        return
    seen = set()
    for t in history:
        if 0 <= t < logits.size:
            seen.add(t)
    for t in seen:
        v = logits[t]
        with np.errstate(all="ignore"):
            logits[t] = v / penalty if v >= 0 else v * penalty


def apply_no_repeat_ngram(logits, history, n):
    """:937-959"""
    if not (n > 0 and len(history) >= n - 1):
        return
    if n == 1:
        for t in history:
            if 0 <= t < logits.size:
                logits[t] = np.float32(-1e9)
        return
    prefix = history[len(history) - (n - 1):]
    forbidden = set()
    upper = len(history) - (n - 1)
    if upper <= 0:
        return
    for i in range(upper):
        match = True
        for j in range(n - 1):
            if history[i + j] != prefix[j]:
                match = False
                break
        if match:
            idx = i + (n - 1)
            if idx < len(history):
                forbidden.add(history[idx])
    for t in forbidden:
        if 0 <= t < logits.size:
            logits[t] = np.float32(-1e9)


def argmax_first(logits):
    """vDSP_maxvi: the first index of the maximum; a NaN never wins, no number at all yields 0."""
    numbers = ~np.isnan(logits)
    if not numbers.any():
        return 0
    return int(np.flatnonzero(numbers & (logits == logits[numbers].max()))[0])


def argmax_strict(logits):
    """CanaryManager.argmax: `for i in 0..<n where p[i] > bestVal` from -greatestFiniteMagnitude — the first index of the largest value above it, else 0."""
    above = logits > -np.finfo(np.float32).max      # false for a NaN
    if not above.any():
        return 0
    return int(np.flatnonzero(above & (logits == logits[above].max()))[0])


def self_mask_row(step, max_seq, f16):
    """buildSelfAttentionMask, static path (:827-848): 0 up to and including step, -1e4 beyond."""
    if f16:
        return np.array([0 if i <= step else MASKED_F16_BITS for i in range(max_seq)], np.uint16)
    return np.array([0.0 if i <= step else MASKED for i in range(max_seq)], np.float32)


def dynamic_self_mask(step, f16):
    return np.zeros(step + 1, np.uint16 if f16 else np.float32)


def cross_mask(encoder_seq_len, encoder_valid, f16):
    """buildCrossAttentionMask (:851-876)"""
    valid = max(0, min(encoder_valid, encoder_seq_len))
    if f16:
        return np.array([0 if i < valid else MASKED_F16_BITS for i in range(encoder_seq_len)], np.uint16)
    return np.array([0.0 if i < valid else MASKED for i in range(encoder_seq_len)], np.float32)


def encoder_valid_frames(feature_length, encoder_seq_len, mel_frames=3500, encoder_frames=438):
    """:670-676"""
    raw = int(math.ceil(float(feature_length * encoder_frames) / float(mel_frames)))
    return max(1, min(raw, encoder_seq_len))


def context_mask(encoder_length, t):
    """makeDecoderContext's mask (CanaryManager.swift:204-207)"""
    valid = min(max(encoder_length, 1), t)
    return np.array([1.0 if i < valid else 0.0 for i in range(t)], np.float32)


def decoder_context(enc, encoder_length):
    """makeDecoderContext: enc [D, T] (any dtype / strides) -> ([T, D] float32, mask [T])."""
    d, t = enc.shape
    emb = np.zeros((t, d), np.float32)
    for ti in range(t):
        for di in range(d):
            emb[ti, di] = np.float32(enc[di, ti])
    return emb, context_mask(encoder_length, t)


class TokenFeed:
    """decodeCacheExternal's loop (:728-803), one call of ``step`` per loop iteration."""

    def __init__(self, prompt, cfg):
        assert len(prompt) >= 1
        self.cfg, self.prompt = cfg, list(prompt)
        self.all_tokens, self.output_tokens = [], []
        self.current = self.prompt[0]
        self.effective_max = min(cfg["max_new"] + len(self.prompt), cfg["max_seq"])
        self.step_index = 0
        self.reason = RUNNING if self.effective_max > 0 else CAP
        self.kind = None          # what the last decision was made of (tests prove their cases hold every kind)

    def decides(self):
        return self.step_index >= len(self.prompt) - 1

    def step(self, logits_row):
        """logits_row: the decoder's row for this step (never looked at when the decision is discarded)."""
        assert self.reason == RUNNING
        step, prompt, cfg = self.step_index, self.prompt, self.cfg
        if step < len(prompt):
            self.current = prompt[step]
        next_token = None
        if self.decides():
            buf = widen(logits_row)[:cfg["vocab"]].copy()
            plain = argmax_first(buf)
            apply_repetition_penalty(buf, self.all_tokens, cfg["repetition_penalty"])
            penalised = buf.copy()
            after_penalty = argmax_first(buf)
            apply_no_repeat_ngram(buf, self.all_tokens, cfg["no_repeat_ngram"])
            next_token = argmax_first(buf)
            banned = {i for i in set(self.all_tokens) if 0 <= i < buf.size and not (buf[i] == penalised[i] or (buf[i] != buf[i] and penalised[i] != penalised[i]))}
            self.kind = dict(plain=plain, after_penalty=after_penalty, final=next_token, history=len(self.all_tokens), banned=banned,
                             penalised={i for i in set(self.all_tokens) if 0 <= i < buf.size} if cfg["repetition_penalty"] != 1.0 and self.all_tokens else set(),
                             raw=widen(logits_row)[:cfg["vocab"]], values=buf)
        self.all_tokens.append(self.current)
        if step >= len(prompt) - 1 and next_token == cfg["eos_id"]:
            self.reason = EOS
            return
        if step >= len(prompt) - 1:
            self.output_tokens.append(next_token)
        self.current = prompt[step + 1] if step < len(prompt) - 1 else next_token
        self.step_index = step + 1
        if self.step_index >= self.effective_max:
            self.reason = CAP

    # what the library hands the network for the coming step
    def input_id(self):
        return self.current

    def position_id(self):
        return self.step_index


class SequenceFeed:
    """greedyDecode (CanaryManager.swift:212-275)"""

    def __init__(self, prompt, cfg):
        s = cfg["max_seq"]
        self.cfg, self.s = cfg, s
        self.input_ids, self.decoder_mask = np.zeros(s, np.int32), np.zeros(s, np.float32)
        prompt_len = min(len(prompt), s)
        for i in range(prompt_len):
            self.input_ids[i] = prompt[i]
            self.decoder_mask[i] = 1
        self.pos = prompt_len
        self.generated = []
        self.reason = RUNNING if self.pos < s else CAP

    def step(self, logits_row):
        assert self.reason == RUNNING
        nxt = argmax_strict(widen(logits_row)[:self.cfg["vocab"]])
        if nxt == self.cfg["eos_id"]:
            self.reason = EOS
            return
        self.generated.append(nxt)
        self.input_ids[self.pos] = nxt
        self.decoder_mask[self.pos] = 1
        self.pos += 1
        if not self.pos < self.s:
            self.reason = CAP

    @property
    def output_tokens(self):
        return self.generated


def plan_windows(samples, chunk, hop):
    """The window loop of transcribeLong (:525-572) = CanaryManager.transcribe (:50-71): [(start, length)]."""
    if samples <= chunk:
        return [(0, samples)]
    out, start, index = [], 0, 0
    while start < samples:
        end = min(start + chunk, samples)
        if index > 0 and (end - start) <= (chunk - hop):
            break
        out.append((start, end - start))
        index += 1
        if end >= samples:
            break
        start += hop
    return out


def merge_token_streams(prefix, suffix, window_tokens=32, min_match=4, detail=False):
    """mergeTokenStreams (CoherePipeline.swift:592-634, identical in CanaryManager.swift:92-130)."""
    prefix, suffix = list(prefix), list(suffix)

    def ret(v, best_len=0, best_s_end=0):
        return (v, best_len, best_s_end) if detail else v

    if not prefix:
        return ret(suffix)
    if not suffix:
        return ret(prefix)
    p_tail = prefix[max(0, len(prefix) - window_tokens):] if window_tokens > 0 else []
    s_head = suffix[:max(0, window_tokens)]
    m, n = len(p_tail), len(s_head)
    if m == 0 or n == 0:
        return ret(prefix + suffix)
    dp = [0] * (n + 1)
    best_len, best_s_end = 0, 0
    for i in range(1, m + 1):
        prev = 0
        for j in range(1, n + 1):
            temp = dp[j]
            if p_tail[i - 1] == s_head[j - 1]:
                dp[j] = prev + 1
                if dp[j] > best_len:
                    best_len, best_s_end = dp[j], j
            else:
                dp[j] = 0
            prev = temp
    if not best_len >= min_match:
        return ret(prefix + suffix, best_len, best_s_end)
    return ret(prefix + suffix[best_s_end:], best_len, best_s_end)


def merge_recording(windows, window_tokens=32, min_match=4):
    """The fold of transcribeLong over a recording's windows: (merged, [(bestLen, bestSEnd) per window])."""
    merged, seams = [], []
    for w in windows:
        merged, bl, be = merge_token_streams(merged, w, window_tokens, min_match, detail=True)
        seams.append((bl, be))
    return merged, seams
