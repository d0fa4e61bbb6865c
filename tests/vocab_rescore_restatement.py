"""The vocabulary rescorer's term-centric path restated line by line from the reference, with numpy float32 scalars and the plain DP:
Sources/FluidAudio/ASR/Parakeet/SlidingWindow/CustomVocabulary/Rescorer/VocabularyRescorer+TokenRescoring.swift (:272-307 arbitration,
:693-1034 the term-centric loops), +TokenEvaluation.swift (:29-173 evaluateCTCMatch, :319-377 the stopword and length-ratio rules),
+Utilities.swift (:8-17 stringSimilarity, :43-62 normalizedForms, :87-96 requiredSimilarity, :112-131 normalizeForSimilarity, :321-339
the normalized set), VocabularyRescorer.swift:111-129 (adaptiveCbw), ContextBiasingConstants.swift, Shared/StringUtils.swift:12-41.

A word or a form is a tuple of ints, one per Character (SPACE for the space); a term is a dict(char_count, min_similarity or None,
forms = [canonical, alias, ...] as buildNormalizedForms hands them to normalizedForms, already normalized).  This file is the yardstick
of the library's candidate and verdict records; it shares no code with the library."""
import math
import struct

import numpy as np

f32 = np.float32
SPACE = 32
MULTI_WORD, SINGLE_WORD = 1, 2                       # CandidateOrigin.termCentricMultiWord / .termCentricSingleWord
APPLIED, SUPERSEDED, REJECTED, UNAVAILABLE = 1, 2, 3, 4
STOPWORD, MULTI_WORD_STOPWORD = 1, 2                 # the caller's flag bits per word

# ContextBiasingConstants.swift
MIN_SIMILARITY_FLOOR = f32(0.50)
DEFAULT_MIN_SIMILARITY = f32(0.52)
LENGTH_RATIO_THRESHOLD = f32(0.75)
SHORT_WORD_SIMILARITY = f32(0.80)
STOPWORD_SPAN_SIMILARITY = f32(0.85)
SHORT_WORD_MAX_LENGTH = 4
DEFAULT_CBW = f32(3.0)
DEFAULT_MARGIN_SECONDS = 0.10
DEFAULT_CONFIG = dict(use_adaptive_thresholds=True, reference_token_count=3, short_term_taper_pivot=1, short_term_taper_exponent=f32(2.0))


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def symbols(text):
    """A normalized string as a row of symbols: the code point of each character."""
    return tuple(ord(c) for c in text)


def levenshtein(a, b):
    """StringUtils.levenshteinDistance (:12-41): the full table."""
    m, n = len(a), len(b)
    if m == 0:
        return n
    if n == 0:
        return m
    dp = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        dp[i][0] = i
    for j in range(n + 1):
        dp[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            cost = 0 if a[i - 1] == b[j - 1] else 1
            dp[i][j] = min(dp[i - 1][j] + 1, dp[i][j - 1] + 1, dp[i - 1][j - 1] + cost)
    return dp[m][n]


def string_similarity(a, b):
    """+Utilities.swift:8-17 (the lowercasing is the caller's)."""
    distance = levenshtein(a, b)
    max_len = max(len(a), len(b))
    if not max_len > 0:
        return f32(1.0)
    return f32(1.0) - f32(distance) / f32(max_len)


def normalize_for_similarity(text):
    """+Utilities.swift:112-131, for the known answers (the library leaves it to the caller)."""
    result, last_was_space = "", True
    for ch in text.lower():
        if ch.isalnum() or ch in "'-":
            result += ch
            last_was_space = False
        elif ch in " \t\n":
            if not last_was_space and result:
                result += " "
                last_was_space = True
    return result.strip()


def word_count(form):
    """normalized.split(separator: " ").count: the non-empty runs."""
    count, inside = 0, False
    for s in form:
        if s == SPACE:
            inside = False
        elif not inside:
            count, inside = count + 1, True
    return count


def normalized_forms(rows):
    """+Utilities.swift:43-62 over rows that are normalized already -> [(form, word count)]; matchedAlias is the index in this list."""
    seen, forms = set(), []
    for row in rows:
        row = tuple(row)
        if not row or row in seen:
            continue
        seen.add(row)
        forms.append((row, word_count(row)))
    return forms


def vocabulary_normalized_set(terms):
    """:321-339.  A term's rows hold its own text and aliases, and the aliases buildNormalizedForms collects from the terms that share
    its lowercased text (:65-81) — which are those terms' own: the union over the rows is the reference's set."""
    return {tuple(r) for t in terms for r in t["forms"] if len(r)}


def required_similarity(min_similarity, span_length):
    """:87-96"""
    if span_length >= 2:
        return max(min_similarity, f32(0.55))
    return min_similarity


def check_length_ratio_rules(word_len, char_count, min_similarity):
    """+TokenEvaluation.swift:357-377"""
    with np.errstate(divide="ignore", invalid="ignore"):
        length_ratio = f32(word_len) / f32(char_count)
    if length_ratio < LENGTH_RATIO_THRESHOLD and word_len <= SHORT_WORD_MAX_LENGTH:
        return max(min_similarity, SHORT_WORD_SIMILARITY)
    return min_similarity


def check_stopword_rules(flags, span_length, current):
    """+TokenEvaluation.swift:319-347 on the caller's flag bits -> (shouldSkip, adjustedMinSimilarity)"""
    if span_length == 1 and flags[0] & STOPWORD:
        return True, current
    if span_length >= 2 and any(f & MULTI_WORD_STOPWORD for f in flags[:span_length]):
        current = max(current, STOPWORD_SPAN_SIMILARITY)
    return False, current


def kept_terms(terms, min_term_length):
    """[(input index, term, forms)] of the terms the loop does not leave at :732 or :746."""
    out = []
    for k, term in enumerate(terms):
        if term["char_count"] < min_term_length:
            continue
        forms = normalized_forms(term["forms"])
        if not forms:
            continue
        out.append((k, term, forms))
    return out


def candidates(terms, min_term_length, utterances, min_similarity=MIN_SIMILARITY_FLOOR):
    """The two loops of :723-1033 without the CTC verdict: [(utterance, term, first word, span, origin, form index, similarity)] in the
    reference's append order.  utterances: [(words, flags)]."""
    min_similarity = f32(min_similarity)
    vocabulary_set = vocabulary_normalized_set(terms)
    kept = kept_terms(terms, min_term_length)
    out = []
    for u, (words, flags) in enumerate(utterances):
        words = [tuple(w) for w in words]
        W = len(words)
        for k, term, forms in kept:
            term_min = min_similarity if term["min_similarity"] is None else f32(term["min_similarity"])          # :729
            canonical = tuple(term["forms"][0]) if term["forms"] else ()
            current_set = {f for f, _ in forms}
            multi = [(i, f) for i, (f, n) in enumerate(forms) if n > 1]
            single = [(i, f) for i, (f, n) in enumerate(forms) if n == 1]
            if multi:                                                                                          # :755
                max_words = max(forms[i][1] for i, _ in multi)
                min_words = min(forms[i][1] for i, _ in multi)
                max_span, min_span = min(4, max_words + 1), max(2, min_words)
                if not min_span <= max_span:
                    continue                                                                                    # :762: the next TERM
                for span in range(min_span, max_span + 1):
                    if not span <= W:
                        break
                    for start in range(W - span + 1):
                        phrase = ()
                        for w in words[start:start + span]:                                                    # normalize(joined): empty words vanish
                            if w:
                                phrase = phrase + ((SPACE,) if phrase else ()) + w
                        if not phrase:
                            continue
                        best, alias = f32(0), -1
                        for i, f in multi:
                            s = string_similarity(phrase, f)
                            if s > best:
                                best, alias = s, i
                        if phrase == canonical:
                            continue
                        if phrase in vocabulary_set and phrase not in current_set:
                            continue
                        if best < required_similarity(term_min, span):
                            continue
                        out.append((u, k, start, span, MULTI_WORD, alias, best))
            if single:                                                                                         # :857
                for idx, word in enumerate(words):
                    if not word:
                        continue
                    if word == canonical:
                        continue
                    if word in vocabulary_set and word not in current_set:
                        continue
                    best, matched, alias = f32(0), 1, -1
                    for i, f in single:
                        s = string_similarity(word, f)
                        if s > best:
                            best, alias = s, i
                    norm2 = words[idx + 1] if idx + 1 < W else None
                    norm3 = words[idx + 2] if idx + 2 < W else None
                    if norm2 is not None and norm2 and term["char_count"] >= 4:                               # :910
                        if not any(string_similarity(norm2, f) >= f32(0.9) for _, f in single):
                            for i, f in single:
                                s = string_similarity(word + norm2, f)
                                if s > best:
                                    best, matched, alias = s, 2, i
                    if norm2 is not None and norm3 is not None and norm2 and norm3 and term["char_count"] >= 8:   # :929
                        if not any(string_similarity(norm2, f) >= f32(0.9) or string_similarity(norm3, f) >= f32(0.9) for _, f in single):
                            for i, f in single:
                                s = string_similarity(word + norm2 + norm3, f)
                                if s > best:
                                    best, matched, alias = s, 3, i
                    threshold = required_similarity(term_min, matched)                                         # :950
                    if matched == 1:
                        threshold = check_length_ratio_rules(len(word), term["char_count"], threshold)
                    skip, threshold = check_stopword_rules(flags[idx:idx + matched], matched, threshold)
                    if skip:
                        continue
                    if best < threshold:
                        continue
                    out.append((u, k, idx, matched, SINGLE_WORD, alias, best))
    return out


def thresholds_near(found, terms, min_term_length, utterances, min_similarity=MIN_SIMILARITY_FLOOR):
    """How many of the candidates `found` lie within one distance step of the threshold that admitted them (the random differential's condition)."""
    near = 0
    kept = dict((k, (t, forms)) for k, t, forms in kept_terms(terms, min_term_length))
    for u, k, start, span, origin, alias, sim in found:
        if alias < 0:
            continue
        term, forms = kept[k]
        words, flags = utterances[u]
        term_min = f32(min_similarity) if term["min_similarity"] is None else f32(term["min_similarity"])
        thr = required_similarity(term_min, span)
        if origin == SINGLE_WORD:
            if span == 1:
                thr = check_length_ratio_rules(len(words[start]), term["char_count"], thr)
            thr = check_stopword_rules(flags[start:start + span], span, thr)[1]
            text_len = sum(len(w) for w in words[start:start + span])
        else:
            text_len = sum(len(w) for w in words[start:start + span]) + sum(1 for w in words[start:start + span] if len(w)) - 1
        longest = max(text_len, len(forms[alias][0]))
        if sim - f32(1) / f32(longest) < thr:
            near += 1
    return near


def adaptive_cbw(cbw, token_count, config=None):
    """VocabularyRescorer.swift:111-129.  log2 and pow: evaluated in float64 and rounded once to float32 (the library's definition)."""
    c = dict(DEFAULT_CONFIG, **(config or {}))
    cbw = f32(cbw)
    if not c["use_adaptive_thresholds"]:
        return cbw
    pivot = c["short_term_taper_pivot"]
    if pivot > 1 and token_count < pivot:
        ratio = f32(max(1, token_count)) / f32(pivot)
        return cbw * f32(math.pow(float(ratio), float(f32(c["short_term_taper_exponent"]))))
    if not token_count > c["reference_token_count"]:
        return cbw
    with np.errstate(divide="ignore"):
        ratio = f32(token_count) / f32(c["reference_token_count"])
    return cbw * (f32(1.0) + f32(math.log2(float(ratio))) * f32(0.3))


def frame_window(start_time, end_time, frame_duration, margin_seconds, frames):
    """+TokenEvaluation.swift:37-42, then clamped to [0, frames] as the scan clamps it."""
    margin = int(margin_seconds / frame_duration)      # Int(_:) truncates
    start = int(start_time / frame_duration)
    end = int(end_time / frame_duration)
    search_start, search_end = max(0, start - margin), min(frames, end + margin)
    return min(search_start, frames), max(search_end, 0)


def evaluate(score, window, term_tokens, alt_tokens, phrase_tokens, cbw, config=None):
    """evaluateCTCMatch (:29-173) behind the window; score(tokens, start, end) is ctcWordSpotConstrained's score.
    -> dict(term_score, alt_won, original_score, boost, boosted_score, compared, should_replace)"""
    start, end = window
    used = list(term_tokens)
    vocab_score = f32(score(used, start, end))
    alt_won = 0
    if alt_tokens and list(alt_tokens) != list(term_tokens):                                                   # :63
        alt_score = f32(score(list(alt_tokens), start, end))
        if alt_score > vocab_score:
            vocab_score, used, alt_won = alt_score, list(alt_tokens), 1
    if not phrase_tokens:                                                                                      # :93-107
        return dict(term_score=vocab_score, alt_won=alt_won, original_score=f32(-np.inf), boost=f32(0), boosted_score=vocab_score, compared=0, should_replace=0)
    original = f32(score(list(phrase_tokens), start, end))
    boost = adaptive_cbw(cbw, len(used), config)
    with np.errstate(invalid="ignore"):
        boosted = vocab_score + boost
    return dict(term_score=vocab_score, alt_won=alt_won, original_score=original, boost=boost, boosted_score=boosted, compared=1,
                should_replace=1 if boosted > original else 0)


def swift_rounded(x):
    """Float.rounded(): to nearest, halves away from zero."""
    x = f32(x)
    return int(math.floor(float(x) + 0.5)) if x >= 0 else -int(math.floor(float(-x) + 0.5))


def quantized(similarity):
    """:276"""
    return swift_rounded(f32(similarity) / f32(0.05))


def arbitrate(pending, occupied=()):
    """arbitratePendingReplacements (:272-307).  pending: [(id, similarity, first word, span)] in candidate order -> (applied ids in
    application order, superseded ids).  The order is bucket descending, span ascending, similarity descending, ties in candidate order."""
    import functools

    def before(a, b):
        qa, qb = quantized(a[1]), quantized(b[1])
        if qa != qb:
            return qa > qb
        if a[3] != b[3]:
            return a[3] < b[3]
        return f32(a[1]) > f32(b[1])

    ordered = sorted(pending, key=functools.cmp_to_key(lambda a, b: -1 if before(a, b) else (1 if before(b, a) else 0)))   # sorted() is stable
    taken, applied, superseded = set(occupied), [], []
    for cid, _, first, span in ordered:
        indices = range(first, first + span)
        if not all(i not in taken for i in indices):
            superseded.append(cid)
            continue
        applied.append(cid)
        taken |= set(indices)
    return applied, superseded


def blob_contents(terms, min_term_length):
    """What fa_vocab_rescore_build has to hold: the alphabet, the sorted strings, and per kept term its forms with sid, word count and
    match masks (bit i of masks[symbol] set where the form's position i holds the symbol)."""
    alphabet = sorted({s for t in terms for r in t["forms"] for s in r})
    strings = sorted(vocabulary_normalized_set(terms))      # tuples of code points: ascending symbols, a prefix before its extensions
    sid = {s: i for i, s in enumerate(strings)}
    out = []
    for k, term, forms in kept_terms(terms, min_term_length):
        canonical = tuple(term["forms"][0]) if term["forms"] else ()
        recs = []
        for f, n in forms:
            masks = {}
            for i, s in enumerate(f):
                masks[s] = masks.get(s, 0) | (1 << i)
            recs.append(dict(sid=sid[f], symbols=list(f), words=n, masks=masks))
        out.append(dict(term=k, char_count=term["char_count"], min_similarity=term["min_similarity"], canonical_sid=sid[canonical] if canonical else -1, forms=recs))
    return dict(alphabet=alphabet, strings=[list(s) for s in strings], terms=out)
