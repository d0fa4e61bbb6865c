"""The language mode of the TDT walk without a GPU: the reference's 47 unit tests (Tests/FluidAudioTests/Shared/
TokenLanguageFilterTests.swift: 40, Tests/FluidAudioTests/ASR/Parakeet/EnglishBlocklistTests.swift: 7) as literal known answers against
tests/tdt_lang_restatement.py — the `matches` cases against fa_tdt_token_classes too —, the restatement's control loop against the
oracle on the hand-traced walks of tests/test_oracle_tdt.py, the bound of a replaced token's confidence against a float32 emulation of
the device's order, and the completeness of the case table tests/test_gpu_tdt_lang.py runs."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_lang_restatement as G  # noqa: E402
from test_decoder_routes import tdt_route  # noqa: E402

LA, CY, GR = G.LATIN, G.CYRILLIC, G.GREEK
M = "▁"

# (text, script, expected) per reference test, in the reference's order
MATCHES = {
    "testMatchesLatinText": [("hello", LA, True), ("world", LA, True), ("Hello World!", LA, True), ("123 abc", LA, True)],
    "testMatchesCyrillicText": [("привет", CY, True), ("мир", CY, True), ("Привет мир!", CY, True), ("123 абв", CY, True)],
    "testDoesNotMatchMixedScripts": [("hello мир", LA, False), ("hello мир", CY, False), ("привет world", LA, False), ("привет world", CY, False)],
    "testStripsSentencePieceBoundaryMarker": [(M + "hello", LA, True), (M + "world", LA, True), (M + "привет", CY, True), (M + "мир", CY, True)],
    "testMultipleBoundaryMarkers": [(M + M + "hello", LA, True), (M + M + "привет", CY, True)],
    "testBoundaryMarkerOnly": [(M, LA, True), (M, CY, True), (M + M, LA, True)],
    "testPolishLatinCharacters": [(ch, LA, True) for ch in "ąćęłńóśźż"],
    "testPolishWords": [(w, LA, True) for w in ("cześć", "świat", "Polska", "zażółć")],
    "testPolishWordsWithBoundaryMarker": [(M + "cześć", LA, True), (M + "świat", LA, True)],
    "testRejectsPolishTextAsCyrillic": [("cześć", CY, False), ("świat", CY, False)],
    "testCzechDiacritics": [(w, LA, True) for w in ("Příliš", "žluťoučký", "kůň", "ďábelské", "ódy")],
    "testSlovakDiacritics": [(w, LA, True) for w in ("Kŕdeľ", "šťastných", "ďatľov", "mĺkveho", "ústí", "koňa")],
    "testSlovenianAndCroatianDiacritics": [(w, LA, True) for w in ("Češnja", "sočna", "Džemper", "čokolada", "svježe")],
    "testRomanianDiacritics": [(w, LA, True) for w in ("Înșelător", "mâine", "scrisoare", "ți-a")],
    "testSlavicLatinLanguagesRejectedAsCyrillic": [(w, CY, False) for w in ("Příliš", "žluťoučký", "Kŕdeľ", "Džemper", "Înșelător")],
    "testPunctuationWithLatin": [(w, LA, True) for w in ("hello!", "world?", "test.", "hello, world!")],
    "testPunctuationWithCyrillic": [(w, CY, True) for w in ("привет!", "мир?", "тест.", "привет, мир!")],
    "testSpacesAndWhitespace": [("hello world", LA, True), ("  hello  ", LA, True), ("привет мир", CY, True), ("  привет  ", CY, True)],
    "testEmptyString": [("", LA, True), ("", CY, True)],
    "testWhitespaceOnly": [(" ", LA, True), ("   ", LA, True), (" ", CY, True), ("   ", CY, True)],
    "testNumbers": [("123", LA, True), ("123", CY, True), ("456 789", LA, True), ("456 789", CY, True)],
    "testLatinExtendedARange": [("Ā", LA, True), ("ž", LA, True), ("ſ", LA, True)],
    "testLatinExtendedBRange": [("ƀ", LA, True), ("ș", LA, True), ("ț", LA, True), ("ɏ", LA, True)],
    "testLatinExtendedAdditionalRange": [("Ḁ", LA, True), ("ế", LA, True)],
    "testCombiningDiacriticsRange": [("e\u0301", LA, True), ("a\u0300", LA, True), ("n\u0303", LA, True), ("e\u0301", CY, False)],
    "testCyrillicRange": [("Ѐ", CY, True), ("ӿ", CY, True), ("Ӏ", CY, True)],
}

# (ids, logits, vocabulary, script) -> expected token id or None, and the probability the reference's comment gives (accuracy 0.01)
FILTER_TOP_K = {
    "testFilterTopKReturnsHighestLogitMatch": (([1, 2, 3, 4], [0.9, 0.7, 0.5, 0.3], {1: "привет", 2: "hello", 3: "мир", 4: "world"}, LA), 2, 0.2695),
    "testFilterTopKArgmaxOverUnsortedLogits": (([1, 2, 3, 4], [0.9, 0.4, 0.1, 0.8], {1: "привет", 2: "hi", 3: "мир", 4: "world"}, LA), 4, None),
    "testFilterTopKWithSentencePieceBoundaryMarker": (([1, 2, 3], [0.9, 0.7, 0.5], {1: M + "привет", 2: M + "hello", 3: M + "мир"}, LA), 2, 0.329),
    "testFilterTopKReturnsNilWhenNoMatch": (([1, 2, 3], [0.9, 0.7, 0.5], {1: "привет", 2: "мир", 3: "тест"}, LA), None, None),
    "testFilterTopKSkipsMissingVocabularyEntries": (([1, 2, 3, 4], [0.9, 0.7, 0.5, 0.3], {1: "привет", 3: "мир", 4: "world"}, LA), 4, 0.1806),
    "testFilterTopKPicksNegativeInfinityLogit": (([1, 2], [0.9, -np.inf], {1: "привет", 2: "hello"}, LA), 2, None),
    "testFilterTopKEmptyArrays": (([], [], {}, LA), None, None),
    "testFilterTopKHandlesLengthMismatch": (([1, 2, 3], [0.9, 0.7], {1: "привет", 2: "hello", 3: "world"}, LA), 2, None),
    "testFilterTopKProbabilityInValidRange": (([1, 2, 3, 4, 5], [10.0, 5.0, 2.0, 1.0, 0.0], {1: "привет", 2: "hello", 3: "world", 4: "test", 5: "foo"}, LA), 2, None),
    "testFilterTopKPolishScenario": (([1, 2, 3], [0.9, 0.6, 0.4], {1: M + "при", 2: M + "prz", 3: M + "прі"}, LA), 2, 0.3156),
}

LATIN_LANGUAGES = "en es fr de it pt ro pl cs sk sl hr bs".split()          # testLatinScriptLanguages
CYRILLIC_LANGUAGES = "ru uk be bg sr".split()                                # testCyrillicScriptLanguages
RAW_VALUES = {"ENGLISH": "en", "POLISH": "pl", "RUSSIAN": "ru", "UKRAINIAN": "uk", "CZECH": "cs", "SLOVAK": "sk", "SLOVENIAN": "sl", "CROATIAN": "hr",
              "BOSNIAN": "bs", "ROMANIAN": "ro"}                             # testLanguageRawValues

BLOCK_VOCAB = {506: " the", 575: " and", 1868: " with", 481: " le", 393: " la", 453: " et", 999: " rendre", 8192: "<blank>"}
BLANK = 8192


@pytest.fixture(scope="module")
def blocklist():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tdt_english_blocklist.json")) as f:
        return frozenset(json.load(f)["ids"])


def test_reference_case_count():
    assert len(MATCHES) + len(FILTER_TOP_K) + 4 == 40                        # + the two script lists, all-have-a-script, the raw values


@pytest.mark.parametrize("name", sorted(MATCHES))
def test_matches_known_answers(fa, name):
    for text, script, expected in MATCHES[name]:
        assert G.matches(text, script) is expected, (name, text, script)
        assert fa.tdt_matches(text, fa.Script(script)) is expected, (name, text, script)
        bits = int(fa.tdt_token_classes([text])[0])
        assert bits & G.IN_VOCAB and bits == int(G.token_classes({0: text}, 1)[0]), (name, text)


@pytest.mark.parametrize("name", sorted(FILTER_TOP_K))
def test_filter_top_k_known_answers(name):
    (ids, logits, vocab, script), token, prob = FILTER_TOP_K[name]
    got = G.filter_top_k(ids, np.asarray(logits, np.float32), vocab, script)
    if token is None:
        assert got is None
        return
    assert got is not None and got[0] == token and 0.0 <= got[1] <= 1.0
    if prob is not None:
        assert 0.0 < got[1] < 1.0 and abs(got[1] - prob) <= 0.01


def test_language_scripts(fa):
    """testLatinScriptLanguages, testCyrillicScriptLanguages, testAllLanguagesHaveScript, testLanguageRawValues — on the restatement's table
    and on the package's Language."""
    assert all(G.LANGUAGES[c] == LA for c in LATIN_LANGUAGES) and all(G.LANGUAGES[c] == CY for c in CYRILLIC_LANGUAGES)
    assert len(G.LANGUAGES) == 28 and set(G.LANGUAGES.values()) == {LA, CY, GR}
    assert {lang.value: int(lang.script) for lang in fa.Language} == G.LANGUAGES
    for name, raw in RAW_VALUES.items():
        assert fa.Language[name].value == raw and raw in G.LANGUAGES


def test_english_blocklist_known_answers(fa, blocklist):
    """EnglishBlocklistTests.swift:21-127, its seven tests in order."""
    f = lambda label, score, ids, lg: G.apply_english_blocklist(label, score, ids, np.asarray(lg, np.float32), BLOCK_VOCAB, BLANK, blocklist)  # noqa: E731
    assert f(BLANK, 1.0, [481, 393], [1.0, 0.5]) == (BLANK, 1.0)                         # testNoSubstitutionWhenLabelIsBlank
    assert f(999, 0.9, [999, 481], [2.0, 1.0]) == (999, 0.9)                             # testNoSubstitutionWhenLabelNotInBlocklist
    assert f(506, 0.8, [506, 575, BLANK], [3.0, 2.0, 1.0]) == (506, 0.8)                 # testNoSubstitutionWhenNoValidAlternativeInTopK
    label, score = f(506, 0.7, [506, 481, 453], [5.0, 4.0, 2.0])                         # testSubstitutesEnglishTokenWithBestLatinAlternative
    assert label == 481 and 0.0 < score <= 1.0
    label, score = f(575, 0.5, [575, 393, 453], [4.0, 3.0, 1.0])                         # testSubstitutedScoreIsNormalisedProbability
    expected = np.exp(3.0 - 4.0) / (np.exp(0.0) + np.exp(-1.0) + np.exp(-3.0))
    assert label == 393 and abs(score - expected) <= 1e-5
    for code in G.LANGUAGES:                                                             # testBlocklistAppliesOnlyToFrench
        assert G.english_blocklist_applies(code) == (code == "fr") and fa.Language(code).english_blocklist_applies == (code == "fr")
    assert not G.english_blocklist_applies(None)
    assert {506, 575, 1868} <= blocklist and not ({481, 453} & blocklist)                # testBlocklistContainsExpectedTokens
    assert len(blocklist) == 44


def test_token_classes_contract(fa):
    """fa_tdt_token_classes: the bytes of a vocabulary with absent ids and a blocklist equal the restatement's; text that is not UTF-8
    and a blocklist id outside [0, V1) are refused."""
    vocab, block = G.vocabulary_of(129)
    np.testing.assert_array_equal(fa.tdt_token_classes(vocab, sorted(block)), G.token_classes(vocab, 129, block))
    texts = [vocab.get(i) for i in range(129)]
    assert texts[7] is None and not fa.tdt_token_classes(texts)[7] & G.IN_VOCAB
    assert fa.tdt_token_classes(texts)[7] & 7 == 7                                        # no text: the empty text's script bits
    assert int(fa.tdt_token_classes(["the"], [0])[0]) == G.LATIN_OK | G.IN_VOCAB | G.BLOCKLISTED
    assert int(fa.tdt_token_classes(["λόγος"])[0]) == G.GREEK_OK | G.IN_VOCAB
    assert int(fa.tdt_token_classes(["\u1f00\u03c1\u03c7\u03ae\u0301"])[0]) == G.GREEK_OK | G.IN_VOCAB                 # Greek Extended + a combining mark
    for bad in (b"\xff", b"ab\xc3", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80abc", b"\xe2\x96"):
        with pytest.raises(ValueError):
            fa.tdt_token_classes([b"ok", bad])
    for ids in ([1], [-1], [0, 5]):
        with pytest.raises(ValueError):
            fa.tdt_token_classes(["a"], ids)
    assert fa.tdt_token_classes([]).size == 0
    assert fa.lib().fa_tdt_token_classes(None, None, 3, None, 0, None) == fa._lib.INVALID_ARGUMENT


def _tables(U, T, fill_tok=8192, fill_bin=1):
    return np.full((U, T), fill_tok, np.int32), np.full((U, T), fill_bin, np.int32), np.full((U, T), 0.5, np.float32)


def test_walk_without_a_language_is_the_oracle(oracle_mod):
    """The hand-traced walks of tests/test_oracle_tdt.py::test_control_loop_hand_traced, and a random batch with every option."""
    cases = []
    tok, bn, pr = _tables(4, 10)
    cases.append((tok, bn, pr, dict(enc_len=10)))
    tok, bn, pr = _tables(4, 10, fill_bin=0)
    cases.append((tok, bn, pr, dict(enc_len=10)))
    tok, bn, pr = _tables(4, 10)
    tok[0, 2], bn[0, 2], pr[0, 2] = 7, 2, 0.9
    cases += [(tok, bn, pr, dict(enc_len=10, global_offset=162)), (tok, bn, pr, dict(enc_len=10, global_offset=162, emit_after=165))]
    tok, bn, pr = _tables(6, 10)
    tok[0, 0], bn[0, 0] = 5, 0
    tok[1, 0], bn[1, 0] = 6, 0
    cases.append((tok, bn, pr, dict(enc_len=10)))
    tok, bn, pr = _tables(4, 10)
    tok[0, 9], bn[0, 9] = 9, 4
    cases += [(tok, bn, pr, dict(enc_len=10)), (tok, bn, pr, dict(enc_len=10, is_last=True)), (tok, bn, pr, dict(enc_len=1)), (tok, bn, pr, dict(enc_len=10, t0=10))]
    tok, bn, pr = tok.copy(), bn.copy(), pr
    bn[0, 0] = 7
    cases.append((tok, bn, pr, dict(enc_len=10)))
    rng = np.random.default_rng(5)
    for i in range(24):
        U, T = int(rng.integers(3, 12)), int(rng.integers(4, 18))
        tok = np.where(rng.random((U, T)) < 0.55, 8192, rng.integers(0, 50, (U, T))).astype(np.int32)
        bn = rng.integers(0, 5, (U, T)).astype(np.int32)
        pr = rng.random((U, T)).astype(np.float32)
        enc = int(rng.integers(1, T + 1))
        cases.append((tok, bn, pr, dict(enc_len=enc, audio_frames=int(rng.integers(max(enc - 3, 1), enc + 3)), t0=int(rng.integers(0, 4)), is_last=bool(i % 2),
                                        global_offset=int(rng.integers(0, 200)), emit_after=None if i % 3 else 3, max_out=64 if i % 4 else 2)))
    for tok, bn, pr, kw in cases:
        r, g = oracle_mod.tdt_greedy(tok, bn, pr, **kw), G.walk_tables(tok, bn, pr, **kw)
        for key in ("status", "count", "final_time", "final_u", "joint_calls"):
            assert g[key] == r[key], (key, kw, g[key], r[key])
        for key in ("tokens", "timestamps", "durations"):
            np.testing.assert_array_equal(g[key], r[key], err_msg=str(kw))
        np.testing.assert_array_equal(g["confidences"].astype(np.float32), r["confidences"])
        assert not g["routes"].any() and g["swap_counts"] == (0, 0)


@pytest.fixture(scope="module")
def tables():
    return {c.name: G.lang_table(c) for c in G.LANG_CALLS}


def test_calls_cover_every_kernel_instance_and_option(tables):
    inst = {c.instance(tdt_route) for c in G.LANG_CALLS}
    assert inst == {"f32_registers", "f16_halves", "f16_pairs", "f32_streaming", "f16_streaming"}
    for c in G.LANG_CALLS:
        assert c.name.startswith(c.instance(tdt_route)), c.name
    k64 = [c for c in G.LANG_CALLS if c.K == 64]
    assert {c.V1 for c in k64} == {129, 1088, 1089, 8193} and {c.instance(tdt_route) for c in k64} == inst
    assert any(c.K == 3 for c in G.LANG_CALLS) and {c.script for c in G.LANG_CALLS} == set(G.SCRIPTS)
    assert {c.blocklist for c in G.LANG_CALLS} == {True, False} and any(c.pad for c in G.LANG_CALLS)
    assert all(t.logits.shape[2] <= 33 for t in tables.values())


@pytest.mark.parametrize("call", G.LANG_CALLS, ids=[c.name for c in G.LANG_CALLS])
def test_case_table_is_complete(tables, call):
    """From the restatement alone: the call holds a row of every kind (without the blocklist the three blocklist kinds do not exist),
    each gets the outcome its name says, the walks end regularly, and a build that ignored the filters would decide other tokens at the
    kinds that replace one."""
    t = tables[call.name]
    assert set(call.kinds) == set(G.KINDS) - (set() if call.blocklist else set(G.BLOCK_KINDS))
    G.check_outcomes(t)
    np.testing.assert_array_equal(t.classes, G.token_classes(t.vocabulary, call.V1, t.blocklist))
    for r in t.expected:
        assert r["status"] == 0 and r["count"] > 12 and r["final_time"] == G.CHUNK_T
    assert t.expected[1]["swap_counts"][1] > 0 or not call.blocklist
    assert any(e[0] == G.FLUSH and e[5] >= 0 for e in t.expected[1]["trace"])
    differ, same_tokens = G.differs_without_filters(t)
    assert differ >= set(G.MUST_DIFFER) & set(call.kinds), sorted(set(G.MUST_DIFFER) & set(call.kinds) - differ)
    assert not same_tokens


def test_swap_bound_against_the_device_order_emulation(tables):
    """Every replaced token of the table with a positive confidence: the float32 emulation of tdt_list_sum lies within swap_tolerance of
    the float64 value, and the bound is the count of its docstring (the worst share is printed; read it with -s)."""
    worst, n = 0.0, 0
    for name, t in tables.items():
        for b, r in enumerate(t.expected):
            for (phase, u, frame, tok, route, emitted), (raw, prob, lst, xb) in zip(r["trace"], r["decisions"]):
                if not route:
                    continue
                ref, tol = G.swap_probability(lst, xb), G.swap_tolerance(lst, xb, t.call.V1)
                assert abs(ref - prob) <= 1e-15 or prob in (0.0, 1.0)
                if tol == 0.0:
                    assert ref == 0.0
                    continue
                emu = float(G.device_order_emulation(t.logits[b, u, frame], t.call.V1, t.call.K, xb))
                share = abs(emu - ref) / tol
                assert share <= 1.0, (name, b, u, frame, emu, ref, tol)
                worst, n = max(worst, share), n + 1
    print(f"tdt-lang-emulation worst |error| / swap_tolerance {worst:.3f} over {n} replaced tokens")
    assert n > 40
    lst = np.array([4.0, 3.0, 1.0], np.float32)                                           # the count itself, on a list of three
    p = G.swap_probability(lst, 3.0)
    w = np.exp(lst.astype(np.float64) - 4.0)
    spread = float((w / w.sum() * (4.0 - lst)).sum())
    assert G.swap_tolerance(lst, 3.0, 129) == pytest.approx(2.0 ** -24 * p * (3 + 13 + 2.25 * (spread + 1.0)) + 2.0 ** -125, rel=1e-12)
    assert G.swap_tolerance(np.array([np.inf, 1.0], np.float32), 1.0, 129) == 0.0 and G.swap_probability([np.inf, 1.0], 1.0) == 0.0
    assert G.swap_tolerance(np.array([2.0, -np.inf], np.float32), -np.inf, 129) == 0.0


def test_ordered_list_definition():
    """Descending key, then ascending id; NaN as -inf; -0.0 == +0.0 (a raw-bit order would put +0.0 first); fewer than K: by id."""
    x = np.array([-0.0, 0.0, np.nan, 1.0, -np.inf, 1.0, 0.0], np.float32)
    ids, lg = G.ordered_list(x, 7, 64)
    assert ids.tolist() == [3, 5, 0, 1, 6, 2, 4]
    assert np.signbit(lg[2]) and not np.signbit(lg[3]) and np.isneginf(lg[5]) and np.isneginf(lg[6])
    assert G.ordered_list(x, 7, 3)[0].tolist() == [3, 5, 0]
    i, v, c = G.topk_rows(x[None, :], 3, 5)
    assert i.tolist() == [[0, 1, 2, -1, -1]] and c.tolist() == [3] and np.isneginf(v[0, 2:]).all()


def test_cpp_mirror_builds_and_agrees(fa, tmp_path):
    """Language, Script, TokenLanguageFilter and TdtDecoderV3 of include/fluidaudio.hpp from a C++ host built with g++ -Werror
    (tests/cabi/tdt_lang.cpp)."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path / "tdt_lang_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(os.path.dirname(here), "include"),
                    os.path.join(here, "cabi", "tdt_lang.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines()}
    assert out["MATCH"] == ["1", "0", "1", "1", "0", "1"]
    assert out["LANG"] == ["pl", "0", "ru", "1", "sr", "1", "el", "2"]
    assert out["BLOCK"] == ["1", "0", "0"]
    assert out["CLASSES"] == [str(G.LATIN_OK | G.IN_VOCAB | G.BLOCKLISTED), str(G.LATIN_OK | G.CYRILLIC_OK | G.GREEK_OK), str(G.CYRILLIC_OK | G.IN_VOCAB)]
    assert out["THROWN"] == ["2"] and out["ST"] == ["1", "1"]
