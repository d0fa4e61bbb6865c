"""A literal restatement of WERCalculator.editDistance (reference: Sources/FluidAudioCLI/Utils/WERCalculator.swift:178-239) — the full
(m + 1) x (n + 1) table and the walk back over it — and of StringUtils.levenshteinDistance (Sources/FluidAudio/Shared/StringUtils.swift:
12-40).  The independent check of csrc/wer.hip, which carries the counts forward instead: nothing here does.  Test infrastructure."""
from __future__ import annotations

from collections import namedtuple

EditDistanceResult = namedtuple("EditDistanceResult", "total insertions deletions substitutions")   # :171-176

# the reference's own pinned answers
# Tests/FluidAudioTests/Shared/StringUtilsTests.swift:10-66 (a, b, distance); strings are compared character by character
LEVENSHTEIN_CASES = [
    ("hello", "hello", 0), ("", "abc", 3), ("abc", "", 3), ("", "", 0), ("kitten", "sitten", 1), ("abc", "abcd", 1), ("abcd", "abc", 1),
    ("abc", "xyz", 3), ("kitten", "sitting", 3), ("ABC", "abc", 3), ([1, 2, 3], [1, 3, 3], 1), ([], [1, 2], 2), ([5, 10, 15], [5, 10, 15], 0),
    ("xyz", "abc", 3),
]
# Tests/FluidAudioTests/ASR/Parakeet/NemotronBenchmarkTests.swift:15-120 (reference, hypothesis, errors, words), the texts as that
# file's normalizeText leaves them (lower case, punctuation and runs of blanks folded to one blank)
WER_CASES = [
    ("hello world", "hello world", 0, 2), ("hello world", "hello ward", 1, 2), ("hello world", "hello big world", 1, 2),
    ("hello big world", "hello world", 1, 3), ("the quick brown fox", "the fast brown cat", 2, 4), ("hello world", "foo bar", 2, 2),
    ("hello world", "", 2, 2), ("", "hello world", 2, 0), ("", "", 0, 0),
    ("hello world", "hello world", 0, 2), ("hello world", "hello world", 0, 2), ("hello world", "hello world", 0, 2),   # :82-110, normalised
    ("the quick brown fox jumps over the lazy dog", "the fast brown fox jumped over a lazy dog", 3, 9),
]


def edit_distance(seq1, seq2) -> EditDistanceResult:
    """:178-239.  seq1 is the hypothesis (rows), seq2 the reference text (columns)."""
    m, n = len(seq1), len(seq2)
    if m == 0:
        return EditDistanceResult(n, n, 0, 0)
    if n == 0:
        return EditDistanceResult(m, 0, m, 0)
    dp = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        dp[i][0] = i
    for j in range(n + 1):
        dp[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if seq1[i - 1] == seq2[j - 1]:
                dp[i][j] = dp[i - 1][j - 1]
            else:
                dp[i][j] = 1 + min(dp[i - 1][j], min(dp[i][j - 1], dp[i - 1][j - 1]))
    i, j = m, n
    insertions = deletions = substitutions = 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and seq1[i - 1] == seq2[j - 1]:
            i -= 1
            j -= 1
        elif i > 0 and j > 0 and dp[i][j] == dp[i - 1][j - 1] + 1:
            substitutions += 1
            i -= 1
            j -= 1
        elif i > 0 and dp[i][j] == dp[i - 1][j] + 1:
            deletions += 1
            i -= 1
        elif j > 0 and dp[i][j] == dp[i][j - 1] + 1:
            insertions += 1
            j -= 1
        else:
            break
    return EditDistanceResult(dp[m][n], insertions, deletions, substitutions)


def levenshtein_distance(a, b) -> int:
    """StringUtils.levenshteinDistance (:12-40)."""
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


def wer_metrics(hyp_words, ref_words):
    """calculateWERMetrics (:7-22) behind the normalizer and the split: (wer, insertions, deletions, substitutions, totalWords)."""
    d = edit_distance(hyp_words, ref_words)
    return (0.0 if len(ref_words) == 0 else float(d.total) / float(len(ref_words)), d.insertions, d.deletions, d.substitutions, len(ref_words))


def wer_and_cer(hypothesis: str, reference: str):
    """calculateWERAndCER (:25-56) behind the normalizer, for texts whose words are separated by single blanks (ASCII: a Character is a
    byte): (wer, cer, insertions, deletions, substitutions, totalWords, totalCharacters)."""
    hyp_words, ref_words = [w for w in hypothesis.split(" ") if w], [w for w in reference.split(" ") if w]
    w = edit_distance(hyp_words, ref_words)
    wer = 0.0 if not ref_words else float(w.total) / float(len(ref_words))
    hyp_chars, ref_chars = list(hypothesis.replace(" ", "")), list(reference.replace(" ", ""))
    c = edit_distance(hyp_chars, ref_chars)
    cer = 0.0 if not ref_chars else float(c.total) / float(len(ref_chars))
    return (wer, cer, w.insertions, w.deletions, w.substitutions, len(ref_words), len(ref_chars))
