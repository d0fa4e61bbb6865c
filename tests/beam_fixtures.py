"""Seeded inputs of the beam-search tests at production scale: a large ARPA model written as text, vocabularies whose pieces spell
its words, and log-probabilities shaped like the benchmark's (randn * 3, blank boosted, log-softmax).  Everything is generated
in code; nothing is read from disk."""
import numpy as np

W = "▁"                                      # ASRConstants.sentencePieceWordBoundary

# syllables of the synthetic language: every one- and two-syllable word is a unigram, three-syllable words are sampled
SYLLABLES = ["ka", "to", "mi", "ne", "ru", "sa", "lo", "pe", "di", "gu", "fa", "zo", "be", "ti", "mu", "ra", "ko", "le", "ni", "so",
             "da", "pu", "ve", "hi", "jo", "wa", "ce", "yu", "xo", "qi", "ba", "te", "an", "el", "or", "is", "um", "ex", "ok", "ul"]
# non-ASCII syllables (2-, 3- and 4-byte UTF-8) for the text edge cases
WIDE_SYLLABLES = ["über", "ß", "é", "ñu", "中", "文", "語", "ア", "イ", "🙂", "ø", "ł"]


def _log10(rng, lo, hi):
    return f"{-rng.uniform(lo, hi):.4f}"


def large_arpa(seed=0, n_three=2500, n_bigrams=32000, syllables=SYLLABLES, extra_words=()):
    """ARPA text of a model with every 1- and 2-syllable word, n_three sampled 3-syllable words, `extra_words`, `<unk>`, and n_bigrams
    distinct bigrams (a few with a context that is no unigram).  Returns (text, unigram words)."""
    rng = np.random.default_rng(seed)
    words = list(syllables) + [a + b for a in syllables for b in syllables]
    three = set()
    while len(three) < n_three:
        three.add("".join(syllables[i] for i in rng.integers(0, len(syllables), 3)))
    words += sorted(three - set(words)) + [w for w in extra_words if w not in words]
    words = list(dict.fromkeys(words))
    lines = ["\\data\\", f"ngram 1={len(words) + 1}", f"ngram 2={n_bigrams}", "", "\\1-grams:", f"-3.5000\t<unk>\t0.0000"]
    lines += [f"{_log10(rng, 0.8, 5.0)}\t{w}\t{_log10(rng, 0.0, 1.2)}" for w in words]
    lines += ["", "\\2-grams:"]
    ctx_pool = words[:600] + ["zzzctx", "<s>"]        # most contexts are frequent words; two contexts are not unigrams
    pairs = set()
    while len(pairs) < n_bigrams:
        c = ctx_pool[int(rng.integers(0, len(ctx_pool)))]
        w = words[int(rng.integers(0, len(words)))] if rng.random() < 0.97 else "<unk>"
        pairs.add((c, w))
    lines += [f"{_log10(rng, 0.05, 2.5)}\t{c}\t{w}" for c, w in sorted(pairs)]
    lines += ["", "\\end\\", ""]
    return "\n".join(lines), words


def spelling_vocab(V, blank, seed=0, syllables=SYLLABLES, boundary_share=0.7):
    """{id: piece} for ids != blank: mostly word starts ("▁" + syllable), the rest continuations (a bare syllable), so that the
    pieces spell words of the model."""
    rng = np.random.default_rng(seed)
    voc = {}
    for v in range(V):
        if v == blank:
            continue
        s = syllables[int(rng.integers(0, len(syllables)))]
        voc[v] = (W + s) if rng.random() < boundary_share else s
    return voc


def bench_log_probs(B, T, V, blank, seed=0):
    """[B, T, V] float32 like bench.py's beam leg: randn * 3, the blank + 4, log-softmax (in float64, rounded once)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V), dtype=np.float32) * np.float32(3.0)
    x[:, :, blank] += np.float32(4.0)
    x64 = x.astype(np.float64)
    m = x64.max(axis=2, keepdims=True)
    return (x64 - m - np.log(np.exp(x64 - m).sum(axis=2, keepdims=True))).astype(np.float32)


def words_of(ids, vocabulary):
    """the words a token sequence spells (CtcDecoder.decodeCtcTokenIds split at the boundaries)"""
    text = "".join(vocabulary.get(i, "") for i in ids).replace(W, " ")
    return [w for w in text.split(" ") if w]


def lm_vocab(V, blank, words, seed=0, word_share=0.95, syllables=SYLLABLES):
    """{id: piece} for ids != blank: a share `word_share` of word starts spelling a whole model word ("▁" + word), the rest bare
    syllables that continue a word.  (The model charges a word when it is completed, so continuations are free until then: with many
    of them the search strings pieces into long unknown words; with few, most decoded words are model words.)"""
    rng = np.random.default_rng(seed)
    voc = {}
    for v in range(V):
        if v == blank:
            continue
        voc[v] = (W + words[int(rng.integers(0, len(words)))]) if rng.random() < word_share else syllables[int(rng.integers(0, len(syllables)))]
    return voc


def peaky_log_probs(B, T, V, peaky, seed=0):
    """[B, T, V] float32 log-softmax of randn * peaky (test_beam.random_case, batched)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32) * np.float32(peaky)
    return (x - np.log(np.exp(x.astype(np.float64)).sum(2, keepdims=True))).astype(np.float32)
