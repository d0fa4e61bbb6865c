"""The compiled restatement of ctcBeamSearch (oracle.ctc_beam_search_c, fa_oracle_ctc_beam_search) against the Python one, which stays
the reviewed statement: token ids identical and scores equal as float32 bits on seeded small cases that cover the tie and text rules;
and the ARPA model at scale (thousands of unigrams, tens of thousands of bigrams): the library's host-side parser and score, the Python
restatement and the C tables give the same float for every probed (word, context) pair.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from beam_fixtures import W, large_arpa, spelling_vocab, words_of  # noqa: E402
from test_beam import (CATDOG_BI, CATDOG_UNI, DEMO1_LP, DEMO1_VOCAB, DEMO2_LP, DEMO2_VOCAB, MEDICAL_BI, MEDICAL_UNI,  # noqa: E402
                       SAMPLE_ARPA, oracle_lm)

SMALL_WORDS = ["the", "cat", "sat", "dog", "on", "mat", "a", "über", "中文", "ß"]
SMALL_ARPA = ("\\data\\\n\\1-grams:\n" + "".join(f"-{1 + 0.15 * i:.2f}\t{w}\t-{0.1 * (i % 4):.1f}\n" for i, w in enumerate(SMALL_WORDS)) +
              "-2.5\t<unk>\t0.0\n\\2-grams:\n" + "".join(f"-0.{3 + i}\t{SMALL_WORDS[i]}\t{SMALL_WORDS[(3 * i + 1) % len(SMALL_WORDS)]}\n"
                                                          for i in range(len(SMALL_WORDS))) + "\\end\\\n")
PIECES = [W + "the", W + "cat", W + "c", "at", "s", "og", "t", "he", W, "", W + "über", "über", W + "中", "文", "ß", W + "a", "a", W + "dog"]


def same(a, b):
    """(ids, score) results equal: ids identical, scores both None or equal as float32 bits"""
    if a[0] != b[0] or (a[1] is None) != (b[1] is None):
        return False
    return a[1] is None or np.float32(a[1]).view(np.uint32) == np.float32(b[1]).view(np.uint32)


def small_case(seed):
    """one seeded configuration: shapes at the edges (T 0 / 1 / 2, V 1, K 0 / 1 / V - 1 / > V - 1, beam 1), blank first, last, inside
    or out of range, peaky, flat or quantised log-probabilities (exact ties across the K-th place, -inf runs), repeated frames, pieces
    that are only the boundary, empty or missing, multi-byte pieces, with and without a model"""
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.choice([0, 1, 2])) if seed % 7 == 0 else int(rng.integers(3, 36))
    V = 1 if seed % 41 == 5 else int(rng.integers(2, 26))
    blank = [0, V - 1, int(rng.integers(0, V))][seed % 3] if seed % 11 else [V, -1][seed % 2]   # no blank in the row: -inf
    present = V - (1 if 0 <= blank < V else 0)
    K = [0, 1, max(present - 1, 0), present, present + 3, int(rng.integers(0, present + 2))][seed % 6]
    beam = 1 if seed % 9 == 0 else int(rng.integers(2, 17))
    kind = seed % 3
    if kind == 0:                                                               # quantised: exact ties everywhere, some -inf
        x = -rng.integers(1, 4, size=(T, V)).astype(np.float32) * np.float32(0.75)
        x[rng.random((T, V)) < 0.1] = -np.inf
    else:
        x = rng.standard_normal((T, V)).astype(np.float32) * np.float32([0.4, 3.0][kind - 1])
        x = (x - np.log(np.exp(x.astype(np.float64)).sum(1, keepdims=True))).astype(np.float32)
    if T > 3:
        x[1] = x[0]                                                             # repeated frames: repeats and their merges
        x[T - 1] = x[T - 2]
    voc = {}
    for v in range(V):
        if rng.random() < 0.85:
            voc[v] = PIECES[int(rng.integers(0, len(PIECES)))]
    if V > 1:
        voc[(max(blank, 0) + 1) % V] = W                                        # a bare boundary piece
    lm = [None, SAMPLE_ARPA, SMALL_ARPA][seed % 3 if seed % 4 else 0]
    lm_weight = [0.0, 0.3, 5.0][(seed // 3) % 3]
    word_bonus = [0.0, 0.5, -0.25][(seed // 5) % 3]
    return x, voc, lm, beam, lm_weight, word_bonus, blank, K


@pytest.mark.parametrize("chunk", range(8))
def test_c_restatement_equals_python_on_small_cases(oracle_mod, chunk):
    o = oracle_mod
    models = {t: o.ARPALanguageModel.parse(t) for t in (SAMPLE_ARPA, SMALL_ARPA)}
    for seed in range(chunk * 30, chunk * 30 + 30):
        x, voc, lm_text, beam, lw, wb, blank, K = small_case(seed)
        lm = models[lm_text] if lm_text else None
        want = o.ctc_beam_search(x, voc, lm, beam, lw, wb, blank, K)
        got = o.ctc_beam_search_c(x, voc, lm, beam, lw, wb, blank, K)
        assert same(got, want), (seed, got, want)
        if x.shape[0] > 2:                                                      # valid_frames decodes the leading rows only
            k = x.shape[0] // 2
            assert same(o.ctc_beam_search_c(x, voc, lm, beam, lw, wb, blank, K, valid_frames=k),
                        o.ctc_beam_search(x[:k], voc, lm, beam, lw, wb, blank, K)), seed


def test_c_restatement_reference_cases(oracle_mod):
    """CtcDecoderTests.swift:145-194 and the demo cases (CtcDecoderDemoTests.swift:11-137) through the C restatement: the reference's
    strings, and the Python restatement's ids and score bit for bit."""
    o = oracle_mod
    v = {0: W + "hello", 1: W + "world"}
    lp = [[0.0, -100.0, -100.0], [-100.0, -100.0, 0.0], [-100.0, 0.0, -100.0]]
    assert o.decode_ctc_token_ids(o.ctc_beam_search_c(lp, v, None, 5, 0.0, 0.0, 2)[0], v) == "hello world"
    assert o.ctc_beam_search_c([[-100.0, 0.0]] * 3, {0: W + "hello"}, None, 5, 0.0, 0.0, 1)[0] == []
    assert o.ctc_beam_search_c([], {0: W + "hello"}, None, 5, 0.0, 0.0, 1) == ([], None)
    assert o.ctc_beam_search_c([[0.0, -100.0]], {0: W + "hello"}, None, 5, 0.0, 0.0, 1)[0] == [0]
    lm = o.ARPALanguageModel.parse(SAMPLE_ARPA)
    v = {0: W + "the", 1: W + "cat", 2: W + "dog"}
    lp = [[0.0, -100.0, -100.0, -100.0], [-100.0, -1.0, -0.9, -100.0]]
    assert o.decode_ctc_token_ids(o.ctc_beam_search_c(lp, v, None, 10, 0.0, 0.0, 3)[0], v) == "the dog"
    assert o.decode_ctc_token_ids(o.ctc_beam_search_c(lp, v, lm, 10, 5.0, 0.0, 3)[0], v) == "the cat"
    cases = [(DEMO1_LP, DEMO1_VOCAB, None, 0.3, 8, "patient has die beetus"),
             (DEMO1_LP, DEMO1_VOCAB, oracle_lm(o, MEDICAL_UNI, MEDICAL_BI), 5.0, 8, "patient has diabetes"),
             (DEMO2_LP, DEMO2_VOCAB, oracle_lm(o, CATDOG_UNI, CATDOG_BI), 2.0, 4, "the cat sat")]
    for lp, voc, m, w, blank, text in cases:
        got = o.ctc_beam_search_c(lp, voc, m, 10, w, 0.0, blank)
        assert o.decode_ctc_token_ids(got[0], voc) == text
        assert same(got, o.ctc_beam_search(lp, voc, m, 10, w, 0.0, blank))


@pytest.fixture(scope="module")
def large_lm(oracle_mod):
    text, words = large_arpa(seed=0)
    return text, words, oracle_mod.ARPALanguageModel.parse(text)


def test_large_model_scores_agree_everywhere(fa, oracle_mod, large_lm):
    """4 000+ unigrams and 32 000 bigrams: the host tables of the library hold displaced entries at this size (pow2(2n + 1) slots),
    so its probing is exercised; score(word, prev) of the library, the Python restatement and the C tables are the same float on every
    unigram (with and without a context), 24 000 sampled (word, context) pairs with and without a bigram, unknown words and contexts."""
    text, words, py = large_lm
    n_bi = sum(len(d) for d in py.bigrams.values())
    assert len(py.unigrams) >= 4096 and n_bi >= 30000 and "<unk>" in py.unigrams
    lib = fa.ARPALanguageModel(text)
    assert lib.unigram_count == len(py.unigrams) and lib.bigram_context_count == len(py.bigrams)
    rng = np.random.default_rng(5)
    uni = list(py.unigrams)
    ctxs = list(py.bigrams)
    pairs = [(w, None) for w in uni] + [(w, uni[int(rng.integers(0, len(uni)))]) for w in uni]
    bi_pairs = [(w, c) for c, d in py.bigrams.items() for w in d]
    pairs += [bi_pairs[int(i)] for i in rng.choice(len(bi_pairs), 12000, replace=False)]
    pairs += [(uni[int(rng.integers(0, len(uni)))], ctxs[int(rng.integers(0, len(ctxs)))]) for _ in range(12000)]
    unknown = ["xyzzy", "kat", "ka" * 9, "", "über", "ka▁"]
    pairs += [(u, p) for u in unknown for p in [None, "ka", "zzzctx", "nope", ""]] + [("ka", u) for u in unknown]
    hits = sum(1 for w, p in pairs if p is not None and w in py.bigrams.get(p, {}))
    assert hits >= 12000 and len(pairs) - hits >= 12000                    # both routes of score() are well covered
    with oracle_mod.CLanguageModel(py) as cm:
        for w, p in pairs:
            want = py.score(w, p)
            assert np.float32(lib.score(w, p)).view(np.uint32) == want.view(np.uint32), (w, p)
            assert cm.score(w, p).view(np.uint32) == want.view(np.uint32), (w, p)


def test_c_restatement_equals_python_with_the_large_model(oracle_mod, large_lm):
    """The beam walk with the large model and a vocabulary that spells its words, beyond the toy models: C equals Python, and the model
    is not idle (most decoded words are model words, and the model changes the best prefix)."""
    o = oracle_mod
    _, words, py = large_lm
    rng = np.random.default_rng(11)
    V, blank, T = 120, 119, 90
    voc = spelling_vocab(V, blank, seed=3, boundary_share=0.85)
    changed = 0
    for case in range(3):
        x = rng.standard_normal((T, V)).astype(np.float32) * np.float32(3.0)
        x[:, blank] += np.float32(2.0)
        x = (x - np.log(np.exp(x.astype(np.float64)).sum(1, keepdims=True))).astype(np.float32)
        want = o.ctc_beam_search(x, voc, py, 12, 0.3, 0.5 * case, blank, 10)
        assert same(o.ctc_beam_search_c(x, voc, py, 12, 0.3, 0.5 * case, blank, 10), want), case
        ws = words_of(want[0], voc)
        assert sum(w in py.unigrams for w in ws) > len(ws) / 2
        changed += want[0] != o.ctc_beam_search_c(x, voc, None, 12, 0.3, 0.5 * case, blank, 10)[0]
    assert changed > 0
