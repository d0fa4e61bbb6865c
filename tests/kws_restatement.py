"""Line-by-line Python restatement of CtcDPAlgorithm (Sources/FluidAudio/ASR/Parakeet/SlidingWindow/CustomVocabulary/WordSpotting/
CtcDPAlgorithm.swift): fillDPTable (:121-229), nonWildcardCount (:232-234), ctcWordSpotConstrained (:250-300), ctcWordSpotMultiple
(:311-392), and the per-term loop of CtcKeywordSpotter.spotKeywordsFromLogProbs (CtcKeywordSpotter.swift:191-254).  It builds the full
tables, as the reference does; every fp32 operation goes through numpy.float32.  Test infrastructure: the device code is compared with it."""
import numpy as np

F = np.float32
WILDCARD = -1                      # ContextBiasingConstants.wildcardTokenId
DEFAULT_BLANK = 1024               # .defaultBlankId
DEFAULT_MIN_SCORE = F(-15.0)       # .defaultMinSpotterScore
BASELINE_TOKENS = 3                # .baselineTokenCountForThreshold
RELAXATION = F(1.0)                # .thresholdRelaxationPerToken
NEG = F(-np.finfo(np.float32).max)   # -Float.greatestFiniteMagnitude
BLANK, TOKEN, WILD = 0, 1, 2


def build_expanded(tokens):        # :30-39
    s = []
    for t in tokens:
        s.append((BLANK, 0))
        s.append((WILD, 0) if t == WILDCARD else (TOKEN, int(t)))
    s.append((BLANK, 0))
    return s


def emission(sym, frame, blank_id):   # :47-60
    kind, tid = sym
    if kind == BLANK:
        return F(frame[blank_id]) if 0 <= blank_id < len(frame) else F(0)
    if kind == TOKEN:
        return F(frame[tid]) if 0 <= tid < len(frame) else NEG
    return F(0)


def can_skip_blank(s, idx):        # :68-80
    if idx < 2:
        return False
    kind, tid = s[idx]
    if kind == BLANK:
        return False
    if kind == TOKEN:
        return not (s[idx - 2][0] == TOKEN and s[idx - 2][1] == tid)
    return s[idx - 2][0] != WILD


def fill_dp_table(log_probs, tokens, blank_id=DEFAULT_BLANK):   # :121-229
    T, N = len(log_probs), len(tokens)
    dp = [[NEG] * (N + 1) for _ in range(T + 1)]
    backtrack = [[0] * (N + 1) for _ in range(T + 1)]
    last_match = [[0] * (N + 1) for _ in range(T + 1)]
    for t in range(T + 1):
        dp[t][0] = F(0)
    if N == 0:
        return dp, backtrack, last_match
    s = build_expanded(tokens)
    s_len = len(s)
    dp_i = [[NEG] * s_len for _ in range(T + 1)]
    start_i = [[0] * s_len for _ in range(T + 1)]
    last_i = [[0] * s_len for _ in range(T + 1)]
    for t in range(T + 1):
        dp_i[t][0] = F(0)
        start_i[t][0] = t
    half = NEG / F(2)
    with np.errstate(over="ignore"):
        for t in range(1, T + 1):
            frame = log_probs[t - 1]
            for i in range(1, s_len):
                sym = s[i]
                emit = emission(sym, frame, blank_id)
                is_wild, is_token = sym[0] == WILD, sym[0] == TOKEN
                added = F(0) if is_wild else emit
                stay = dp_i[t - 1][i]
                advance = dp_i[t - 1][i - 1]
                skip = dp_i[t - 1][i - 2] if can_skip_blank(s, i) else NEG
                best, kind = stay, 0
                if advance > best:
                    best, kind = advance, 1
                if skip > best:
                    best, kind = skip, 2
                if best <= half:
                    dp_i[t][i] = NEG
                    continue
                dp_i[t][i] = F(best + added)
                is_match = is_token or is_wild
                if kind == 0:
                    start_i[t][i] = start_i[t - 1][i]
                    last_i[t][i] = t if is_match else last_i[t - 1][i]
                elif kind == 1:
                    start_i[t][i] = t - 1 if i == 1 else start_i[t - 1][i - 1]
                    last_i[t][i] = t if is_match else last_i[t - 1][i - 1]
                else:
                    start_i[t][i] = start_i[t - 1][i - 2]
                    last_i[t][i] = t if is_match else last_i[t - 1][i - 2]
    for t in range(T + 1):
        for n in range(1, N + 1):
            s_tok, s_blank = 2 * n - 1, 2 * n
            sc_tok = dp_i[t][s_tok] if s_tok < s_len else NEG
            sc_blank = dp_i[t][s_blank] if s_blank < s_len else NEG
            if sc_tok >= sc_blank:
                dp[t][n], backtrack[t][n], last_match[t][n] = sc_tok, start_i[t][s_tok], last_i[t][s_tok]
            else:
                dp[t][n], backtrack[t][n], last_match[t][n] = sc_blank, start_i[t][s_blank], last_i[t][s_blank]
    return dp, backtrack, last_match


def non_wildcard_count(tokens):    # :232-234
    return sum(1 for t in tokens if t != WILDCARD)


def word_spot_constrained(log_probs, tokens, search_start, search_end, blank_id=DEFAULT_BLANK):   # :250-300
    T, N = len(log_probs), len(tokens)
    cs, ce = max(0, search_start), min(T, search_end)
    if N == 0 or ce <= cs:
        return F(-np.inf), cs, cs
    window = log_probs[cs:ce]
    wt = len(window)
    if wt < N:
        return F(-np.inf), cs, cs
    dp, backtrack, last_match = fill_dp_table(window, tokens, blank_id)
    best_end, best = 0, NEG
    for t in range(N, wt + 1):
        if dp[t][N] > best:
            best, best_end = dp[t][N], t
    nf = non_wildcard_count(tokens)
    score = F(best / F(nf)) if nf > 0 else best
    return score, cs + backtrack[best_end][N], cs + last_match[best_end][N]


def word_spot_multiple(log_probs, tokens, min_score=DEFAULT_MIN_SCORE, merge_overlap=True, blank_id=DEFAULT_BLANK):   # :311-392
    T, N = len(log_probs), len(tokens)
    min_score = F(min_score)
    if N == 0 or T == 0:
        return []
    dp, backtrack, last_match = fill_dp_table(log_probs, tokens, blank_id)
    free = non_wildcard_count(tokens)
    norm = F(free) if free > 0 else F(1.0)
    cands = []
    if T < N:
        return []
    for t in range(N, T + 1):
        x = F(dp[t][N] / norm)
        prev = F(dp[t - 1][N] / norm) if t > N else NEG
        nxt = F(dp[t + 1][N] / norm) if t < T else NEG
        if x >= prev and x > nxt and x >= min_score:
            cands.append((x, backtrack[t][N], last_match[t][N]))
    if not cands:
        best_end, best = 0, NEG
        for t in range(N, T + 1):
            x = F(dp[t][N] / norm)
            if x > best:
                best, best_end = x, t
        if best >= min_score:
            cands.append((best, backtrack[best_end][N], last_match[best_end][N]))
    if not merge_overlap:
        return cands
    merged = []
    for c in sorted(cands, key=lambda c: c[1]):   # stable, as the standard library's sort is
        if merged and c[1] <= merged[-1][2]:
            last = merged[-1]
            best = c if c[0] > last[0] else last
            merged[-1] = (best[0], best[1], max(last[2], c[2]))
        else:
            merged.append(c)
    return merged


def adjusted_threshold(min_score, token_count):   # CtcKeywordSpotter.swift:217-222
    if min_score is None:
        return DEFAULT_MIN_SCORE
    return F(F(min_score) - F(F(max(0, token_count - BASELINE_TOKENS)) * RELAXATION))


def spot_keywords(log_probs, terms, min_score=None, blank_id=DEFAULT_BLANK, merge_overlap=True, frame_duration=None):
    """The per-term loop (:204-246): terms are token-id lists (the caller has applied minTermLength); -> [(term index, score, start,
    end)] in the reference's order, with (startTime, endTime) appended when frame_duration is given."""
    if len(log_probs) == 0:
        return []
    out = []
    for k, ids in enumerate(terms):
        if len(ids) == 0:
            continue
        for score, start, end in word_spot_multiple(log_probs, list(ids), adjusted_threshold(min_score, len(ids)), merge_overlap, blank_id):
            out.append((k, score, start, end) + ((float(start) * frame_duration, float(end) * frame_duration) if frame_duration is not None else ()))
    return out


def bits(x):
    return int(np.float32(x).view(np.uint32))
