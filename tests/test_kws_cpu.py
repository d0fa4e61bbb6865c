"""Pins tests/kws_restatement.py — what the device word spotter is compared with — on the literal inputs and assertions of the
reference's own CtcDPAlgorithmTests.swift (all 17 cases, :30-329, copied in as data) and on three hand-derived cases with exact values.
No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kws_restatement as R  # noqa: E402

F = np.float32
W = R.WILDCARD
FLT_MAX = np.finfo(np.float32).max


def make_log_probs(frames, vocab, hot, high=-0.1, cold=-10.0):   # CtcDPAlgorithmTests.makeLogProbs (:11-26)
    m = np.full((frames, vocab), cold, np.float32)
    for f, t in hot:
        if f < frames and t < vocab:
            m[f, t] = high
    return list(m)


def make_frame(vocab, hot, high, blank_id, blank, cold):   # makeFrame (:190-202)
    row = np.full(vocab, cold, np.float32)
    if blank_id < vocab:
        row[blank_id] = blank
    if hot is not None and hot < vocab:
        row[hot] = high
    return row


# ---- nonWildcardCount (:30-46)
def test_non_wildcard_count_all_regular():
    assert R.non_wildcard_count([0, 1, 2]) == 3


def test_non_wildcard_count_mixed():
    assert R.non_wildcard_count([0, W, 1]) == 2


def test_non_wildcard_count_all_wildcards():
    assert R.non_wildcard_count([W, W, W]) == 0


def test_non_wildcard_count_empty():
    assert R.non_wildcard_count([]) == 0


# ---- ctcWordSpotConstrained (:50-121)
def test_constrained_window_basic():
    lp = make_log_probs(20, 5, [(5, 0), (6, 1)])
    score, start, end = R.word_spot_constrained(lp, [0, 1], 3, 12)
    assert score > -1.0 and start >= 3 and end <= 12


def test_constrained_window_misses_keyword():
    lp = make_log_probs(20, 5, [(15, 0), (16, 1)])
    assert R.word_spot_constrained(lp, [0, 1], 0, 10)[0] < -5.0


def test_constrained_window_clamped():
    lp = make_log_probs(5, 3, [(2, 0)])
    assert R.word_spot_constrained(lp, [0], -5, 100)[0] > -np.inf


def test_constrained_window_too_small():
    lp = make_log_probs(20, 5, [])
    assert R.word_spot_constrained(lp, [0, 1, 2], 5, 7)[0] == -np.inf


def test_constrained_empty_window():
    lp = make_log_probs(10, 5, [])
    assert R.word_spot_constrained(lp, [0], 5, 5)[0] == -np.inf


# ---- ctcWordSpotMultiple (:125-163)
def test_multiple_empty_keyword():
    assert R.word_spot_multiple(make_log_probs(5, 3, []), []) == []


def test_multiple_empty_log_probs():
    assert R.word_spot_multiple([], [0]) == []


def test_multiple_below_min_score():
    assert R.word_spot_multiple(make_log_probs(5, 3, []), [0], min_score=-5.0) == []


def test_multiple_single_occurrence():
    res = R.word_spot_multiple(make_log_probs(10, 5, [(2, 0)], high=-0.1), [0], min_score=-1.0)
    assert len(res) >= 1 and res[0][0] > -1.0


# ---- fillDPTable through ctcWordSpotConstrained (:167-183)
def test_dp_table_score_monotonicity():
    lp = make_log_probs(3, 3, [(0, 0), (1, 1), (2, 2)], high=-0.05)
    assert abs(float(R.word_spot_constrained(lp, [0, 1, 2], 0, len(lp))[0]) - (-0.05)) <= 0.01


# ---- blank-aware behaviour (:208-329)
def test_blank_emission_cost_is_accumulated():
    b, v, hi, bl, cold = 3, 4, -0.1, -0.5, -10.0
    lp = [make_frame(v, 0, hi, b, bl, cold), make_frame(v, None, hi, b, bl, cold), make_frame(v, None, hi, b, bl, cold),
          make_frame(v, None, hi, b, bl, cold), make_frame(v, 1, hi, b, bl, cold)]
    assert abs(float(R.word_spot_constrained(lp, [0, 1], 0, len(lp), blank_id=b)[0]) - (-0.85)) <= 0.01


def test_repeated_tokens_require_intervening_blank():
    b, v, hi, bl, cold = 2, 3, -0.1, -0.5, -10.0
    no_blank = [make_frame(v, 0, hi, b, bl, cold), make_frame(v, 0, hi, b, bl, cold)]
    with_blank = [make_frame(v, 0, hi, b, bl, cold), make_frame(v, None, hi, b, bl, cold), make_frame(v, 0, hi, b, bl, cold)]
    a = R.word_spot_constrained(no_blank, [0, 0], 0, len(no_blank), blank_id=b)
    c = R.word_spot_constrained(with_blank, [0, 0], 0, len(with_blank), blank_id=b)
    assert c[0] > a[0] + 1.0


def test_wildcard_still_free_cost():
    b, v, hi, cold = 3, 4, -0.1, -10.0
    lp = [make_frame(v, 0, hi, b, cold, cold), make_frame(v, None, hi, b, hi, cold), make_frame(v, 2, hi, b, cold, cold)]
    assert abs(float(R.word_spot_constrained(lp, [0, W, 2], 0, len(lp), blank_id=b)[0]) - (-0.1)) <= 0.05


# ---- hand-derived, exact
def test_unreachable_state_keeps_the_rows_zeroes():
    """[a, a, a] needs five frames; in a 3-frame window the end column stays at -FLT_MAX, no sample is a strict maximum, bestEnd stays 0
    and the frames are the zero-initialised row's — not inherited from any path: (-FLT_MAX / 3, clampedStart, clampedStart)."""
    lp = make_log_probs(8, 3, [(2, 0), (3, 0), (4, 0)])
    score, start, end = R.word_spot_constrained(lp, [0, 0, 0], 2, 5, blank_id=2)
    assert (R.bits(score), start, end) == (R.bits(F(-FLT_MAX) / F(3)), 2, 2)
    assert R.bits(score) == 0xFEAAAAAA
    dp, bt, lm = R.fill_dp_table(lp[2:5], [0, 0, 0], 2)
    assert [R.bits(dp[t][3]) for t in range(4)] == [R.bits(-FLT_MAX)] * 4 and bt[3][3] == 0 and lm[3][3] == 0
    # the second a IS reached at t = 3 (a, blank, a) and then loses it again: nothing is carried into an unreachable state
    assert (R.bits(dp[3][2]), bt[3][2], lm[3][2]) == (R.bits(F(F(-0.1) + F(-10.0)) + F(-0.1)), 0, 3)


def test_projection_tie_takes_the_token_state():
    """One token a = 0, blank 1.  Frame 0: a -1, blank -2; frame 1: a -1, blank 0.  At t = 2 the token state (a fresh start: 0 + -1, start 1,
    last 2) and the blank after it (-1 + 0, start 0, last 1) tie at -1: scTok >= scBlank takes the token's frames.  t = 1 scores -1 too, so
    only t = 2 is a candidate (>= prev, > the -FLT_MAX behind the end)."""
    lp = [np.array([-1.0, -2.0], np.float32), np.array([-1.0, 0.0], np.float32)]
    dp, bt, lm = R.fill_dp_table(lp, [0], 1)
    assert [(float(dp[t][1]), bt[t][1], lm[t][1]) for t in (1, 2)] == [(-1.0, 0, 1), (-1.0, 1, 2)]
    res = R.word_spot_multiple(lp, [0], min_score=-100.0, merge_overlap=False, blank_id=1)
    assert [(R.bits(s), a, b) for s, a, b in res] == [(R.bits(-1.0), 1, 2)]


def test_plateau_yields_only_its_last_sample():
    """Four frames of a -1, blank 0: the end column is -1 at t = 1 ... 4.  score >= prev && score > next fails on the plateau (== next) and
    holds only at t = 4, whose next is -FLT_MAX; the tie there takes the token state: start 3, last 4."""
    lp = [np.array([-1.0, 0.0], np.float32) for _ in range(4)]
    dp, _, _ = R.fill_dp_table(lp, [0], 1)
    assert [float(dp[t][1]) for t in range(1, 5)] == [-1.0] * 4
    for merge in (False, True):
        res = R.word_spot_multiple(lp, [0], min_score=-1.0, merge_overlap=merge, blank_id=1)
        assert [(R.bits(s), a, b) for s, a, b in res] == [(R.bits(-1.0), 3, 4)]
    assert R.word_spot_multiple(lp, [0], min_score=-0.5, blank_id=1) == []   # the fallback's maximum misses the threshold too


def test_threshold_rule():
    assert R.adjusted_threshold(None, 9) == F(-15.0)
    assert [float(R.adjusted_threshold(-8.5, n)) for n in (1, 3, 4, 10)] == [-8.5, -8.5, -9.5, -15.5]
