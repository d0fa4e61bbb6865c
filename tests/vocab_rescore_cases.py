"""The problems of the vocabulary rescorer's tests, shared by the CPU tier (tests/test_vocab_rescore_cpu.py: the restatement against the
plain C++ of vocab_rescore_core.h) and the GPU tier (tests/test_gpu_vocab_rescore.py: the restatement against the device).  A problem is
dict(terms, min_term_length, utterances, min_similarity) as tests/vocab_rescore_restatement.py takes them; the expected records are the
restatement's, computed once per problem and kept (want())."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocab_rescore_restatement as R  # noqa: E402

S = R.symbols
_want = {}


def term(text, aliases=(), char_count=None, min_similarity=None):
    """A term from normalized strings; char_count defaults to the text's length."""
    return dict(char_count=len(text) if char_count is None else char_count, min_similarity=min_similarity, forms=[S(text)] + [S(a) for a in aliases])


def want(name, problem):
    if name not in _want:
        _want[name] = R.candidates(problem["terms"], problem["min_term_length"], problem["utterances"], problem["min_similarity"])
    return _want[name]


def swap(text, positions, foreign="#"):
    """text with the characters at `positions` replaced by one no form holds: exactly len(positions) edits away."""
    out = list(text)
    for p in positions:
        out[p] = foreign
    return "".join(out)


def pattern(n, seed):
    rng = np.random.default_rng(seed)
    return "".join("abcd"[i] for i in rng.integers(0, 4, n))


# ---- shapes: utterances of 0, 1, 2, 3, 63, 64, 65 and 130 words; a wavefront takes 62 word starts and two neighbours
SHAPE_WORDS = (0, 1, 2, 3, 63, 64, 65, 130)
LONG = {n: pattern(n, 100 + n) for n in (31, 32, 33, 63, 64)}
COMPOUNDS = ["abc", "dabc", "d", "abc", "dabc"]


def shapes_problem():
    terms = [
        term("abcdabcd"),                                            # 8 characters: compounds of 2 and 3 words
        term("abdc", aliases=("abdc", "ab dc", "abdc", "dcba")),     # duplicated aliases, a two-word alias
        term("ab", aliases=("ba",)),                                 # below min_term_length
        term("", aliases=("cab", "b ad"), char_count=5),             # the canonical form is empty
        term("bad cab", aliases=("bad cab dab", "a b c d", "a b c d a")),   # 2 ... 5 words: spans 2 ... 4
        term("dab", aliases=("dabb",), min_similarity=0.3),          # a minimum below the call's
        term("dab", aliases=("dabb",), min_similarity=0.9),          # the same lowercased text, a minimum above the call's
        term("a b c d a"),                                           # five words alone: no span, and the term is left
        term("c"),                                                   # one symbol (min_term_length 1 would keep it; here it is skipped)
        term("cccc", aliases=("c",)),                                # ... and kept as an alias
        term("d a b", aliases=("dab",)),                             # "dab" is another term's form as well
    ] + [term(LONG[n], min_similarity=0.45) for n in (31, 32, 33, 63, 64)]
    rng = np.random.default_rng(11)
    utterances = []
    for W in SHAPE_WORDS:
        words = []
        for _ in range(W):
            n = int(rng.integers(0, 6)) if rng.random() < 0.9 else int(rng.integers(6, 12))
            words.append("".join("abcd#"[i] for i in rng.integers(0, 5, n)) if rng.random() < 0.8 else "")
        flags = [int(f) for f in rng.integers(0, 4, W)]
        if W >= 63:
            # "abcdabcd" as compounds of three words that start on the last two word starts of a wavefront (60, 61: their words 2 and 3
            # are its neighbour lanes 62, 63) and on the first of the next one (62); the shorter utterances end inside them
            n = min(len(COMPOUNDS), W - 60)
            words[60:60 + n], flags[60:60 + n] = COMPOUNDS[:n], [0] * n
            words[3:9] = ["bad", "", "cab", "dab", "", "bad"]      # empty inside, at the start and at the end of a span
            words[10:13] = ["a", "b", "c"]
            words[20] = LONG[31][:30]
            words[21] = swap(LONG[32], (5,))
            words[22] = LONG[33] + "a"
            words[23:25] = [LONG[63][:40], LONG[63][40:]]           # a compound of 63 symbols
            words[25] = swap(LONG[64], (0, 63))
            words[26] = LONG[64] + LONG[64][:9]                      # longer than any form
        if W == 130:
            words[122:127], flags[122:127] = COMPOUNDS, [0] * 5    # the same round the next edge (starts 62 ... 123, then 124 ...)
            words[128:130], flags[128:130] = ["abcda", "bcd"], [0, 0]   # the last two words have no neighbours
        utterances.append(([S(w) for w in words], flags))
    return dict(terms=terms, min_term_length=3, utterances=utterances, min_similarity=R.MIN_SIMILARITY_FLOOR)


# ---- threshold boundaries: (distance, longest length) pairs whose similarity is the threshold itself in fp32
def boundary_problem():
    f20, f25, f10 = pattern(20, 1), pattern(25, 2), pattern(10, 3)
    two = pattern(9, 4) + " " + pattern(10, 5)                       # 20 symbols, two words
    terms = [
        term("ab", min_similarity=0.5),                               # 0: (1, 2) at 0.50
        term(f25, min_similarity=0.52),                               # 1: (12, 25) at 0.52
        term(two),                                                    # 2: (9, 20) at 0.55, the multi-word floor
        term("abcda", min_similarity=0.6),                            # 3: (2, 5) at 0.60
        term("dcbad", char_count=6),                                  # 4: (1, 5) at 0.80, the length-ratio rule (4 of 6 characters)
        term(f10, min_similarity=0.8),                                # 5: (2, 10) at 0.80
        term(f20),                                                    # 6: (3, 20) at 0.85, a compound with a multi-word stopword
        term("ddccbbaadd"),                                           # 7: (1, 10) at 0.90, the compound guard on word 2
        term("dcdcdcdcdcbabababab" + "a"),                            # 8: (2, 20) at 0.90, the compound guard on word 3
        term("bcda"),                                                 # 9: 3 of 4 characters, a ratio of exactly 3/4: the rule stays off
    ]
    rows = [
        ("a#", 0), ("##", 0),
        (swap(f25, range(0, 24, 2)), 0), (swap(f25, range(0, 25, 2)), 0),
        (swap(two[:9], (0, 2, 4, 6)), 0), (swap(two[10:], (0, 2, 4, 6, 8)), 0), (swap(two[10:], (0, 2, 4, 6, 8, 9)), 0),
        ("a#cd#", 0), ("a#c##", 0),
        ("dcba", 0), ("dcb#", 0),
        (swap(f10, (1, 8)), 0), (swap(f10, (1, 5, 8)), 0),
        (swap(f20[:8], (0, 3)), 0), (swap(f20[8:], (4,)), R.MULTI_WORD_STOPWORD), (swap(f20[:8], (0, 3)), 0), (swap(f20[8:], (4, 7)), R.MULTI_WORD_STOPWORD),
        ("ddcc", 0), ("ddccbbaad#", 0), ("ddcc", 0), ("ddccbbaa##", 0),
        ("dcdc", 0), ("dcdcdc", 0), ("dcdcdcdcdcbabababa##", 0), ("dcdc", 0), ("dcdcdc", 0), ("dcdcdcdcdcbababab###", 0),
        ("bcd", 0), ("bc", 0),
    ]
    words = [S(w) for w, _ in rows]
    flags = [f for _, f in rows]
    return dict(terms=terms, min_term_length=2, utterances=[(words, flags)], min_similarity=R.MIN_SIMILARITY_FLOOR)


# ---- the alphabet: 1022 distinct symbols make A = 1023 (accepted), one more is refused
def alphabet_terms(distinct):
    syms = list(range(1000, 1000 + distinct))
    return [dict(char_count=len(row), min_similarity=None, forms=[tuple(row)]) for row in (syms[i:i + 60] for i in range(0, distinct, 60))]


# ---- the random differential: 200 problems over a 4-letter alphabet
RANDOM_SEED = 2


def random_problems(seed=RANDOM_SEED, count=200):
    rng = np.random.default_rng(seed)

    def word(lo, hi):
        return "".join("abcd"[i] for i in rng.integers(0, 4, int(rng.integers(lo, hi + 1))))

    def mutated(text):
        out = list(text)
        for _ in range(int(rng.integers(0, 3))):
            at = int(rng.integers(0, len(out) + 1))
            kind = rng.random()
            if kind < 0.4 and at < len(out):
                out[at] = "abcd"[int(rng.integers(0, 4))]
            elif kind < 0.7 and at < len(out):
                del out[at]
            else:
                out.insert(at, "abcd"[int(rng.integers(0, 4))])
        return "".join(out)

    out = []
    for _ in range(count):
        terms, pieces = [], []
        for _ in range(int(rng.integers(3, 7))):
            forms = []
            for _ in range(int(rng.integers(1, 4))):
                forms.append(" ".join(word(1, 4) for _ in range(int(rng.integers(2, 5)))) if rng.random() < 0.35 else word(2, 9))
            for f in forms:   # what an utterance is made of: a form's words, or a form cut in two or three
                if " " in f:
                    pieces.append(f.split(" "))
                else:
                    cuts = sorted(int(c) for c in rng.integers(0, len(f) + 1, int(rng.integers(0, 3))))
                    pieces.append([f[a:b] for a, b in zip([0] + cuts, cuts + [len(f)])])
            if rng.random() < 0.1:
                forms[0] = ""
            mins = None if rng.random() < 0.6 else float(rng.choice([0.3, 0.5, 0.6, 0.75]))
            terms.append(term(forms[0], aliases=forms[1:], char_count=int(rng.integers(2, 10)) if rng.random() < 0.3 else max(len(forms[0]), 3), min_similarity=mins))
        utterances = []
        for _ in range(int(rng.integers(1, 4))):
            words = []
            for _ in range(int(rng.integers(0, 11))):
                if rng.random() < 0.75:
                    words += [mutated(w) for w in pieces[int(rng.integers(0, len(pieces)))]]
                else:
                    words.append(word(0, 5))
            utterances.append(([S(w) for w in words], [int(f) for f in rng.choice([0, 0, 0, 1, 2, 3], len(words))]))
        out.append(dict(terms=terms, min_term_length=3, utterances=utterances, min_similarity=np.float32(rng.choice([0.4, 0.5, 0.52]))))
    return out


# ---- verdicts: one utterance of 12 words over 40 frames (36 valid), a coarse grid of log-probs so that scores tie
def verdict_problem():
    rng = np.random.default_rng(5)
    V, T = 8, 40
    lp = (np.float32(-0.5) * rng.integers(0, 8, (2, T, V)).astype(np.float32)).astype(np.float32)
    valid = [36, 40]
    frame_duration, margin = 0.08, 0.10
    starts = [[0.0, 0.2, 0.45, 0.8, 1.0, 1.3, 1.6, 1.9, 2.2, 2.5, 2.7, 2.95], [0.0, 0.5, 1.0, 3.0]]
    ends = [[0.2, 0.45, 0.8, 1.0, 1.3, 1.6, 1.9, 2.2, 2.5, 2.7, 2.95, 3.4], [0.5, 1.0, 3.0, 3.3]]
    term_tokens = [[1, 2], [3], [4, 5, 6, 1, 2, 3], [2, 2], [5], [1] * 9]
    alt_tokens = [[2], [3], [], [2, 2, 1], [6, 5], []]          # a different row, an equal one, none, longer, another, none
    f = np.float32
    #            utt term first span origin form similarity   phrase tokens
    cands = [((0, 0, 0, 1, 2, 0, f(0.875)), [3, 1]),          # the window starts at frame 0 (clamped below)
             ((0, 1, 0, 2, 2, 0, f(0.875)), [4]),             # the same bucket (17.5 -> 18), a longer span
             ((0, 2, 1, 3, 1, 1, f(0.7)), [1, 1]),
             ((0, 3, 2, 2, 1, 0, f(0.66)), [6]),
             ((0, 4, 3, 1, 2, 0, f(0.62)), [2, 3]),
             ((0, 0, 5, 1, 2, 0, f(0.625)), []),              # an empty phrase row: nothing compared
             ((0, 1, 6, 1, 2, 0, f(0.625)), [0]),             # 12.5 -> 13
             ((0, 3, 6, 1, 2, 0, f(0.625)), [7]),             # a tie in bucket, span and similarity: candidate order decides
             ((0, 4, 6, 2, 2, 0, f(0.64)), [5, 5]),
             ((0, 5, 8, 1, 2, 0, f(0.9)), [2]),               # 9 tokens in a window of 7 frames: -inf, and -inf > x is false
             ((0, 1, 9, 1, 2, 0, f(0.6)), [1, 2, 3, 4, 5, 6, 7, 1, 2, 3]),   # the phrase is longer than the window: original -inf
             ((0, 0, 10, 2, 2, 0, f(0.99)), [3]),             # the window ends behind the valid frames (clamped above)
             ((0, 1, 11, 1, 2, 0, f(0.8)), [1]),              # an occupied index
             ((1, 1, 0, 2, 1, 0, f(0.75)), [2, 2]),
             ((1, 4, 1, 1, 2, 0, f(0.8)), [3, 3]),
             ((1, 3, 3, 1, 2, 0, f(0.7)), [4]),
             ((1, 0, 2, 2, 1, 0, f(0.7)), [6])]
    occupied = [[0] * 11 + [1], [0, 0, 0, 0]]
    return dict(lp=lp, valid=valid, frame_duration=frame_duration, margin=margin, starts=starts, ends=ends, term_tokens=term_tokens, alt_tokens=alt_tokens,
                cands=[c for c, _ in cands], phrase_tokens=[p for _, p in cands], occupied=occupied, blank=7, cbw=np.float32(3.0),
                config=dict(reference_token_count=3))


def verdict_want(p, score):
    """The restatement's verdicts and applied lists; score(utterance, tokens, start, end) is ctcWordSpotConstrained's score."""
    verdicts, pending = [], [[] for _ in p["valid"]]
    for c, (cand, phrase) in enumerate(zip(p["cands"], p["phrase_tokens"])):
        u, t, first, span = cand[:4]
        window = R.frame_window(p["starts"][u][first], p["ends"][u][first + span - 1], p["frame_duration"], p["margin"], p["valid"][u])
        v = R.evaluate(lambda tok, a, b: score(u, tok, a, b), window, p["term_tokens"][t], p["alt_tokens"][t], phrase, p["cbw"], p["config"])
        v["window"] = window
        v["outcome"] = R.UNAVAILABLE if not v["compared"] else (R.SUPERSEDED if v["should_replace"] else R.REJECTED)
        if v["should_replace"]:
            pending[u].append((c, cand[6], first, span))
        verdicts.append(v)
    applied = []
    for u, pend in enumerate(pending):
        a, _ = R.arbitrate(pend, [i for i, o in enumerate(p["occupied"][u]) if o])
        for c in a:
            verdicts[c]["outcome"] = R.APPLIED
        applied.append(a)
    return verdicts, applied


# ---- the stand-alone program's input (tests/cpu/vocab_rescore_core_main.cpp)
def vocabulary_words(terms, min_term_length):
    out = [min_term_length, len(terms)]
    for t in terms:
        m = t["min_similarity"]
        out += [t["char_count"], 0 if m is None else 1, R.bits(0.0 if m is None else np.float32(m)), len(t["forms"])]
        for f in t["forms"]:
            out += [len(f)] + list(f)
    return out


def utterance_words(utterances):
    out = [len(utterances)]
    for words, flags in utterances:
        out.append(len(words))
        for w, f in zip(words, flags):
            out += [f, len(w)] + list(w)
    return out
