"""fa_vocab_rescore_candidates and fa_vocab_rescore_decide(_dev) on the device against the Python restatement of the reference's
term-centric rescorer (tests/vocab_rescore_restatement.py) on the problems of tests/vocab_rescore_cases.py: every field of a candidate
record as an integer, the similarity by its 32 bits; the verdict records likewise, given that tests/test_gpu_kws.py pins the window
scores to tests/kws_restatement.py.  No tolerances.  The same file is run on the poisoned-workspace library (make POISON=1).

Shapes: a wavefront takes 62 word starts and two neighbour lanes (utterances of 0, 1, 2, 3, 63, 64, 65 and 130 words, compounds planted
round the edges); a form is one 64-bit pattern (1, 31, 32, 33, 63, 64 symbols); a form's masks are A * 8 bytes of LDS (A = 1023 is the
most); survivors go through an arena that a switch shrinks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kws_restatement as KR  # noqa: E402
import vocab_rescore_cases as K  # noqa: E402
import vocab_rescore_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def records(recs):
    return [(int(r["utterance"]), int(r["term"]), int(r["first_word"]), int(r["span_len"]), int(r["origin"]), int(r["form"]), R.bits(r["similarity"])) for r in recs]


def wanted(name, p):
    return [(u, k, a, n, o, f, R.bits(s)) for u, k, a, n, o, f, s in K.want(name, p)]


def on_device(fa, ctx, p, **kw):
    blob = fa.vocab_rescore.build(p["terms"], p["min_term_length"])
    recs, counts = fa.vocab_rescore.candidates(blob, p["utterances"], float(p["min_similarity"]), ctx=ctx, **kw)
    return records(recs), counts.tolist()


def test_shapes(fa, gpu_ctx):
    p = K.shapes_problem()
    want = wanted("shapes", p)
    got, counts = on_device(fa, gpu_ctx, p)
    assert len(want) > 300 and got == want
    assert counts == [sum(1 for w in want if w[0] == u) for u in range(len(K.SHAPE_WORDS))]


def test_threshold_boundaries(fa, gpu_ctx):
    p = K.boundary_problem()
    want = wanted("boundary", p)
    assert on_device(fa, gpu_ctx, p)[0] == want
    exact = {R.bits(f32(x)) for x in (0.5, 0.52, 0.55, 0.6, 0.8, 0.85)}
    assert exact <= {w[6] for w in want}


def test_small_arena_walks_again(fa, gpu_ctx, switch):
    """FA_VR_ARENA shrinks the survivor arena: the first walk only counts, the second has room; the records are those of the roomy arena."""
    p = K.shapes_problem()
    want = wanted("shapes", p)
    for arena in (0, 16, len(want) - 1, len(want)):
        switch("FA_VR_ARENA", arena)
        assert on_device(fa, gpu_ctx, p)[0] == want, arena
    switch("FA_VR_ARENA", None)
    assert on_device(fa, gpu_ctx, p, capacity=len(want))[0] == want


def test_largest_alphabet(fa, gpu_ctx):
    """A = 1023: 8184 bytes of masks per form.  The words hold the lowest and the highest symbols, two that only a skipped term holds and
    one that no form holds."""
    terms = K.alphabet_terms(1022)
    rng = np.random.default_rng(8)
    words = []
    for t in (terms[0], terms[16]):
        w = list(t["forms"][0])
        for at, to in zip(rng.integers(0, len(w), 6), (5, 2020, 2021, 5, 1000, 2019)):
            w[int(at)] = to
        words += [tuple(w), tuple(w[:20]), tuple(w[20:])]
    p = dict(terms=terms, min_term_length=3, utterances=[(words, [0] * len(words))], min_similarity=f32(0.5))
    want = wanted("alphabet", p)
    assert len(terms[17]["forms"][0]) == 2 and len(want) >= 4 and {w[3] for w in want} >= {1, 2} and {w[1] for w in want} == {0, 16}
    assert on_device(fa, gpu_ctx, p)[0] == want


def test_random_differential(fa, gpu_ctx):
    """200 random problems over a 4-letter alphabet (tests/test_vocab_rescore_cpu.py checks what they cover)."""
    total = 0
    for i, p in enumerate(K.random_problems()):
        want = wanted(("random", i), p)
        got, counts = on_device(fa, gpu_ctx, p)
        assert got == want, i
        total += len(got)
    assert total >= 2000


def verdict_records(verdicts):
    return [(R.bits(v["term_score"]), int(v["alt_won"]), R.bits(v["original_score"]), R.bits(v["boost"]), R.bits(v["boosted_score"]), int(v["compared"]),
             int(v["should_replace"]), int(v["outcome"]), int(v["start_frame"]), int(v["end_frame"])) for v in verdicts]


def test_verdicts(fa, gpu_ctx):
    import torch
    V = fa.vocab_rescore
    p = K.verdict_problem()
    lp, valid = p["lp"], p["valid"]
    want, want_applied = K.verdict_want(p, lambda u, tok, a, b: KR.word_spot_constrained(list(lp[u, :valid[u]]), tok, a, b, p["blank"])[0])
    want_records = [(R.bits(v["term_score"]), v["alt_won"], R.bits(v["original_score"]), R.bits(v["boost"]), R.bits(v["boosted_score"]), v["compared"], v["should_replace"],
                     v["outcome"], v["window"][0], v["window"][1]) for v in want]
    cands = np.zeros(len(p["cands"]), V.VR_CANDIDATE_DTYPE)
    for i, c in enumerate(p["cands"]):
        cands[i] = tuple(c)
    cfg = V.default_config()
    cfg.frame_duration, cfg.margin_seconds, cfg.cbw, cfg.blank_id = p["frame_duration"], p["margin"], float(p["cbw"]), p["blank"]
    flat = lambda rows: [x for r in rows for x in r]   # noqa: E731
    for matrix in (torch.from_numpy(lp).cuda(), lp):
        verdicts, applied = V.decide(matrix, cands, [len(s) for s in p["starts"]], flat(p["starts"]), flat(p["ends"]), p["term_tokens"], p["alt_tokens"], p["phrase_tokens"],
                                     config=cfg, occupied=flat(p["occupied"]), valid_frames=valid, ctx=gpu_ctx)
        assert verdict_records(verdicts) == want_records
        assert applied == want_applied
    # without occupied indices candidate 11 is applied; a term without tokens leaves its candidates unavailable
    verdicts, applied = V.decide(lp, cands, [12, 4], flat(p["starts"]), flat(p["ends"]), p["term_tokens"], p["alt_tokens"], p["phrase_tokens"], config=cfg,
                                 valid_frames=valid, ctx=gpu_ctx)
    assert int(verdicts[11]["outcome"]) == R.APPLIED and 11 in applied[0] and want[11]["outcome"] == R.SUPERSEDED
    verdicts, applied = V.decide(lp, cands, [12, 4], flat(p["starts"]), flat(p["ends"]), [[]] + p["term_tokens"][1:], p["alt_tokens"], p["phrase_tokens"], config=cfg,
                                 valid_frames=valid, ctx=gpu_ctx)
    assert [int(verdicts[c]["outcome"]) for c, cand in enumerate(p["cands"]) if cand[1] == 0] == [R.UNAVAILABLE] * 4
    verdicts, applied = V.decide(lp, cands[:0], [12, 4], flat(p["starts"]), flat(p["ends"]), p["term_tokens"], p["alt_tokens"], [], config=cfg, ctx=gpu_ctx)
    assert len(verdicts) == 0 and applied == [[], []]


def test_rescore_batch_composes_the_two_entries(fa, gpu_ctx):
    """candidates -> the caller's tokenizer once per distinct phrase -> decide, on the verdict problem's log-probs."""
    V = fa.vocab_rescore
    q = K.verdict_problem()
    lp = q["lp"]
    raw = [["liv", "Marli,", "", "new", "res", "the", "livmarli", "nwerez", "x", "y", "liv", "marly"], ["New", "Rez", "z", "livmarl"]]
    norm = [[R.symbols(R.normalize_for_similarity(w)) for w in u] for u in raw]
    flags = [[3 if w == "the" else 0 for w in u] for u in raw]
    terms = [K.term("livmarli"), K.term("newrez", aliases=("new rez",), min_similarity=0.6), K.term("ab")]
    term_tokens, alt_tokens = [[1, 2], [3, 4, 5, 6], [1]], [[2], [], []]
    asked = []

    def encode(phrase):
        asked.append(phrase)
        return [1 + (ord(c) % 6) for c in phrase.replace(" ", "")][:5]
    cfg = V.default_config()
    cfg.blank_id = q["blank"]
    utterances = list(zip(norm, flags))
    cands, verdicts, applied = V.rescore_batch(lp, V.build(terms), utterances, raw, q["starts"], q["ends"], term_tokens, alt_tokens, encode, config=cfg,
                                               valid_frames=q["valid"], ctx=gpu_ctx)
    found = R.candidates(terms, 3, utterances)
    assert records(cands) == [(u, k, a, n, o, f, R.bits(s)) for u, k, a, n, o, f, s in found] and len(found) >= 6
    phrases = [" ".join(raw[c[0]][c[2]:c[2] + c[3]]) for c in found]
    assert sorted(asked) == sorted(set(phrases)) and len(set(phrases)) < len(phrases)
    p = dict(q, cands=found, phrase_tokens=[[1 + (ord(c) % 6) for c in ph.replace(" ", "")][:5] for ph in phrases], term_tokens=term_tokens, alt_tokens=alt_tokens,
             occupied=[[0] * 12, [0] * 4], cbw=f32(3.0), config=None)
    want, want_applied = K.verdict_want(p, lambda u, tok, a, b: KR.word_spot_constrained(list(lp[u, :q["valid"][u]]), tok, a, b, q["blank"])[0])
    assert verdict_records(verdicts) == [(R.bits(v["term_score"]), v["alt_won"], R.bits(v["original_score"]), R.bits(v["boost"]), R.bits(v["boosted_score"]), v["compared"],
                                          v["should_replace"], v["outcome"], v["window"][0], v["window"][1]) for v in want]
    assert applied == want_applied and any(want_applied)
