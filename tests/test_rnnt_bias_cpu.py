"""The hotword-bias matcher against the reference's own known answers (no GPU): every case of
Tests/FluidAudioTests/ASR/Parakeet/Streaming/NemotronVocabularyBiasTests.swift from testFreshStartBoostsAnchoredPrefixPieces (:54) through
testPickBiasedCanOvertakeBlank (:237) and testLargeVocabularySmoke (:251), with its toy piece table, run against
tests/rnnt_restatement.py AND against fa_rnnt_bias_build + fa_rnnt_bias_candidates; the effectiveBoost halves of the two weight tests;
a differential case on random vocabularies; malformed blobs.  testInitReturnsNilWithNoUsableTerms (:34) and
testIsUsableMatchesEngineGuards (:41) test the letter-count guard of usableSurfaces, which counts grapheme clusters and stays with the
caller of this library: they are left out; the weight halves of the former (a boost that is not above 0 drops the
term) are kept in test_terms_without_a_positive_boost_leave_no_bias."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_restatement as R  # noqa: E402

PIECES = {0: "▁", 1: "▁to", 2: "r", 3: "vane", 4: "▁tor", 5: "▁torvane", 6: "▁The", 7: "▁the", 8: "▁ran", 9: "▁t", 10: "▁cr", 11: "an",
          13: "东", 14: "京", 15: "▁नम", 16: "स्", 17: "ते", 18: "<unk>", 19: "<en-US>", 21: "▁ab", 22: "▁c", 23: "v", 24: "▁vor"}


class Restated:
    def __init__(self, fa, terms, pieces=PIECES, default_boost=R.DEFAULT_BOOST):
        self.bias = R.VocabularyBias(terms, pieces, default_boost)
        assert self.bias.usable

    def observe(self, i):
        self.bias.observe(i)

    def reset(self):
        self.bias.reset_match_state()

    def candidates(self):
        return {i: float(b) for i, b in self.bias.candidates().items()}


class Library:
    def __init__(self, fa, terms, pieces=PIECES, default_boost=R.DEFAULT_BOOST):
        self.fa = fa
        self.bias = fa.rnnt_bias_build(terms, pieces, default_boost)
        assert self.bias.blob.size
        self.seen = []

    def observe(self, i):
        self.seen.append(i)

    def reset(self):
        self.seen = []

    def candidates(self):
        return self.fa.rnnt_bias_candidates(self.bias, self.seen)


@pytest.fixture(params=[Restated, Library], ids=["restatement", "library"])
def make(request, fa):
    return lambda terms, **kw: request.param(fa, terms, **kw)


def test_fresh_start_boosts_anchored_prefix_pieces(make):
    m = make(["Torvane"]).candidates()
    assert 1 in m and 4 in m and 5 in m and 3 not in m and 2 not in m


def test_fresh_start_excludes_single_letter_and_bare_marker_pieces(make):
    m = make(["torvane"]).candidates()
    assert 9 not in m and 0 not in m


def test_case_variants_of_a_piece_all_fold(make):
    m = make(["the"]).candidates()
    assert 6 in m and 7 in m


def test_continuation_after_partial_match(make):
    b = make(["torvane"])
    b.observe(4)
    m = b.candidates()
    assert 3 in m and 23 in m and 5 in m


def test_word_start_anchoring_blocks_mid_word_match(make):
    b = make(["ran"])
    b.observe(10)
    m = b.candidates()
    assert 11 not in m and 8 in m and len(m) == 1


def test_multi_offset_overlap_survives_repeated_leading_word(make):
    b = make(["ab ab c"])
    b.observe(21)
    b.observe(21)
    m = b.candidates()
    assert 22 in m and 21 in m
    b.observe(21)
    assert 22 in b.candidates()


def test_cjk_term_is_unanchored_and_accepts_two_clusters(make):
    b = make(["东京"])
    m = b.candidates()
    assert 13 in m and 14 not in m
    b.observe(13)
    assert 14 in b.candidates()


def test_devanagari_conjunct_rejoins_in_scalar_space(make):
    b = make(["नमस्ते"])
    assert 15 in b.candidates()
    b.observe(15)
    assert 16 in b.candidates()
    b.observe(16)
    assert 17 in b.candidates()


def test_alias_is_boosted_as_itself(make):
    m = make([("torvane", None, ("vortane",))]).candidates()
    assert 4 in m and 24 in m


def test_default_and_override_boosts(make):
    assert make(["torvane"]).candidates()[5] == R.DEFAULT_BOOST
    assert make([("torvane", 5.5)]).candidates()[5] == 5.5


def test_legacy_weights_fall_back_to_default(make, fa):
    assert make([("torvane", 10.0)]).candidates()[5] == R.DEFAULT_BOOST
    for boost in (fa.rnnt_bias_effective_boost, R.effective_boost):
        assert boost(10) == R.DEFAULT_BOOST and boost(R.MAX_BOOST) == R.MAX_BOOST and boost(None) == R.DEFAULT_BOOST
        assert boost(None, 3.0) == 3.0 and boost(float("nan")) == R.DEFAULT_BOOST and boost(-1.0) == -1.0
    assert fa.RNNT_BIAS_DEFAULT_BOOST == R.DEFAULT_BOOST and fa.RNNT_BIAS_MAX_BOOST == R.MAX_BOOST


def test_strongest_boost_wins_per_token(make):
    assert make([("torvane", 2.0), ("torment", 5.0)]).candidates()[4] == 5.0


def test_special_pieces_never_disturb_match_state(make):
    b = make(["torvane"])
    for i in (4, 19, 18):
        b.observe(i)
    assert 3 in b.candidates()


def test_unmatched_emission_drops_continuation(make):
    b = make(["torvane"])
    b.observe(4)
    b.observe(7)
    m = b.candidates()
    assert 3 not in m and 4 in m


def test_reset_match_state_clears_continuations_keeps_vocabulary(make):
    b = make(["torvane"])
    b.observe(4)
    assert 3 in b.candidates()
    b.reset()
    m = b.candidates()
    assert 3 not in m and 5 in m


def test_pick_biased_flips_only_when_boosted_logit_wins():
    logits = np.asarray([1.0, 5.0, 3.0], np.float32)
    assert R.pick_biased(1, {2: 4.5}, logits) == 2
    assert R.pick_biased(1, {0: 3.0}, logits) == 1
    assert R.pick_biased(1, {7: 100.0}, logits) == 1          # out-of-range ids are ignored, never read


def test_pick_biased_can_overtake_blank():
    assert R.pick_biased(2, {0: 4.5}, np.asarray([2.0, 1.0, 4.0], np.float32)) == 0


def test_pick_biased_tie_order_and_nan():
    """This library's definitions: the lowest id among equal scores; a score equal to logit[plain] does not flip; NaN never flips."""
    f = np.float32
    assert R.pick_biased(3, {2: 2.0, 1: 2.0}, np.asarray([0, 4, 4, 5], f)) == 1
    assert R.pick_biased(3, {1: 1.0}, np.asarray([0, 4, 4, 5], f)) == 3
    assert R.pick_biased(3, {1: 9.0}, np.asarray([0, np.nan, 4, 5], f)) == 3
    assert R.pick_biased(0, {1: 9.0}, np.asarray([np.nan, 1, np.nan], f)) == 0
    assert R.pick_biased(3, {1: 9.0}, np.asarray([0, -np.inf, 4, 5], f)) == 3


def test_large_vocabulary_smoke(make):
    b = make([f"zqterm{i}vx" for i in range(2000)] + ["torvane"])
    for _ in range(200 if isinstance(b, Restated) else 12):    # (the library's entry replays the emissions from a reset state)
        b.observe(4)
        assert 3 in b.candidates()
        b.observe(7)
        assert b.candidates()


def test_terms_without_a_positive_boost_leave_no_bias(fa):
    for terms in ([("torvane", 0.0)], [("torvane", -1.0)], [], ["   "]):
        assert not R.VocabularyBias(terms, PIECES).usable
        bias = fa.rnnt_bias_build(terms, PIECES)
        assert bias.blob.size == 0 and bias.tail_cap == 0


def test_piece_form_and_tail_cap(fa):
    assert R.piece_form("Steve Jobs") == "▁steve▁jobs" and R.piece_form(" a　b\tc ") == "▁a▁b▁c" and R.piece_form("东京 タワー") == "东京タワー"
    assert R.piece_form("x东") == "▁x东"
    for terms in (["Steve Jobs", "ran"], ["东京 タワー"], ["école"]):
        assert fa.rnnt_bias_build(terms, PIECES).tail_cap == R.VocabularyBias(terms, PIECES).tail_cap
    assert R.VocabularyBias(["école"], PIECES).tail_cap == 6                       # NFC: one scalar for the accented letter


def random_case(rng):
    alphabet = ["a", "b", "c", "▁"]
    word = lambda lo, hi: "".join(rng.choice(alphabet[:3], rng.integers(lo, hi)))  # noqa: E731
    pieces = {}
    n = int(rng.integers(6, 40))
    for i in range(n):
        kind = rng.integers(0, 10)
        if kind == 0:
            pieces[i] = None if rng.integers(0, 2) else "<s>"
        elif kind == 1 and i:
            prev = [p for p in pieces.values() if p]
            pieces[i] = str(rng.choice(prev)).upper() if prev and rng.integers(0, 2) else (str(rng.choice(prev)) if prev else "a")   # twins and duplicates
        elif kind == 2:
            pieces[i] = "▁"
        else:
            pieces[i] = ("▁" if rng.integers(0, 2) else "") + word(1, 4)
    pieces = {i: p for i, p in pieces.items() if p is not None}
    terms = []
    for _ in range(int(rng.integers(1, 6))):
        text = " ".join(word(1, 5) for _ in range(int(rng.integers(1, 4))))
        terms.append((text.upper() if rng.integers(0, 3) == 0 else text, [None, 2.0, 5.5, 10.0, 0.5][int(rng.integers(0, 5))]))
    emitted = [int(rng.integers(0, n + 2)) for _ in range(int(rng.integers(0, 14)))]
    return pieces, terms, emitted, n


def test_differential_random_vocabularies(fa):
    """Random vocabularies over {a, b, c, ▁} with duplicate pieces and case-folded twins, random terms and emission sequences: the
    library's candidate ids and boosts after every prefix of the emissions equal the restatement's."""
    rng = np.random.default_rng(20251)
    live = 0
    for _ in range(300):
        pieces, terms, emitted, n = random_case(rng)
        ref = R.VocabularyBias(terms, pieces)
        bias = fa.rnnt_bias_build(terms, pieces, vocab=n + 2)
        assert bias.tail_cap == ref.tail_cap and bias.blob.size > 0
        for k in range(len(emitted) + 1):
            if k:
                ref.observe(emitted[k - 1])
            want = {i: float(b) for i, b in ref.candidates().items()}
            got = fa.rnnt_bias_candidates(bias, emitted[:k])
            assert got == want and list(got) == sorted(got), (pieces, terms, emitted[:k], got, want)
            live += bool(ref.continuation_only())
    assert live > 300          # the cases do reach partial matches


def test_malformed_blobs_are_refused(fa):
    import ctypes as C
    L, lib = fa._lib, fa.lib()
    bias = fa.rnnt_bias_build(["torvane", "ab ab c"], PIECES)
    count = C.c_int32()
    obs = np.asarray([4, 21, 21], np.int32)

    def status(blob, words=None):
        blob = np.ascontiguousarray(blob, np.int32)
        return lib.fa_rnnt_bias_candidates(blob.ctypes.data, blob.size if words is None else words, obs.ctypes.data, obs.size, None, None, 0, C.byref(count))

    assert status(bias.blob) == L.OUTPUT_TOO_SMALL and count.value == len(fa.rnnt_bias_candidates(bias, obs))
    for words in (0, 1, 15, 16, bias.blob.size // 2, bias.blob.size - 1):                   # truncated
        assert status(bias.blob[:words].copy()) == L.INVALID_ARGUMENT, words
    for word in (0, 1):                                                                     # magic, version
        bad = bias.blob.copy()
        bad[word] ^= 0x10
        assert status(bad) == L.INVALID_ARGUMENT
    for word in (5, 7, 8, 10, 11, 13):                                                      # a section offset past the end
        for value in (bias.blob.size, bias.blob.size + 7, 2 ** 31 - 1, -4, 3):
            bad = bias.blob.copy()
            bad[word] = value
            assert status(bad) == L.INVALID_ARGUMENT, (word, value)
    for word in (4, 6, 9, 12):                                                              # a section length past the end
        bad = bias.blob.copy()
        bad[word] = 2 ** 31 - 1
        assert status(bad) == L.INVALID_ARGUMENT, word
    bad = bias.blob.copy()
    bad[bad[5] + 2] = bad[9]                                                                # the root's candidate list leaves its section
    bad[bad[5] + 3] = 5
    assert status(bad) == L.INVALID_ARGUMENT
    assert lib.fa_rnnt_bias_candidates(None, 64, None, 0, None, None, 0, C.byref(count)) == L.INVALID_ARGUMENT
    assert lib.fa_rnnt_bias_candidates(bias.blob.ctypes.data, bias.blob.size, None, 0, None, None, 0, None) == L.INVALID_ARGUMENT


def test_build_contract(fa):
    import ctypes as C
    L, lib = fa._lib, fa.lib()
    pieces = (C.c_char_p * 3)(b"\xe2\x96\x81ab", None, b"\xe2\x96\x81c")
    surf = (C.c_char_p * 1)(b"ab c")
    boost = np.asarray([4.5], np.float32)
    need, cap = C.c_int64(-1), C.c_int32(-1)
    P, S = C.cast(pieces, C.c_void_p), C.cast(surf, C.c_void_p)
    assert lib.fa_rnnt_bias_build(P, 3, S, boost.ctypes.data, 1, None, 0, C.byref(need), C.byref(cap)) == L.SUCCESS
    assert need.value > 16 and cap.value == 5
    blob = np.zeros(need.value, np.int32)
    words = need.value
    assert lib.fa_rnnt_bias_build(P, 3, S, boost.ctypes.data, 1, blob.ctypes.data, words - 1, C.byref(need), C.byref(cap)) == L.OUTPUT_TOO_SMALL
    assert lib.fa_rnnt_bias_build(P, 3, S, boost.ctypes.data, 1, blob.ctypes.data, words, C.byref(need), C.byref(cap)) == L.SUCCESS
    assert fa.rnnt_bias_candidates(blob) == {0: 4.5} and fa.rnnt_bias_candidates(blob, [0]) == {0: 4.5, 2: 4.5}
    assert lib.fa_rnnt_bias_build(P, 3, S, boost.ctypes.data, 0, None, 0, C.byref(need), C.byref(cap)) == L.SUCCESS and need.value == 0
    assert lib.fa_rnnt_bias_build(P, 3, S, boost.ctypes.data, 1, None, 0, None, C.byref(cap)) == L.INVALID_ARGUMENT
    assert lib.fa_rnnt_bias_build(P, 3, S, boost.ctypes.data, 1, None, 0, C.byref(need), None) == L.INVALID_ARGUMENT
    for bad in (0.0, -1.0, float("nan")):
        assert lib.fa_rnnt_bias_build(P, 3, S, np.asarray([bad], np.float32).ctypes.data, 1, None, 0, C.byref(need), C.byref(cap)) == L.INVALID_ARGUMENT
    for text in (b"\xff", b"\xc0\x80", b"\xed\xa0\x80", b"\xe2\x96"):                      # not UTF-8: a surface, then a piece
        assert lib.fa_rnnt_bias_build(P, 3, C.cast((C.c_char_p * 1)(text), C.c_void_p), boost.ctypes.data, 1, None, 0, C.byref(need), C.byref(cap)) == L.INVALID_ARGUMENT
        assert lib.fa_rnnt_bias_build(C.cast((C.c_char_p * 3)(b"a", text, None), C.c_void_p), 3, S, boost.ctypes.data, 1, None, 0, C.byref(need), C.byref(cap)) == L.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        fa.rnnt_bias_build(["a" * 256], PIECES)                                             # 257 scalars with the marker
    assert fa.rnnt_bias_build(["a" * 255], PIECES).tail_cap == 256 == fa.RNNT_BIAS_MAX_FORM
