"""The vocabulary rescorer without a GPU: the restatement (tests/vocab_rescore_restatement.py) reproduces the reference's own test
values (tests/golden/vocab_rescore_known_answers.json, vocab_rescore_stopwords.json), and the plain C++ of
fluidaudio_amd/csrc/vocab_rescore_core.h — the bit-vector step, the blob build and its validation, the host's reference walk, the
arbitration, the window arithmetic, the boost — equals the restatement when tests/cpu/vocab_rescore_core_main.cpp, a stand-alone
program built with the address and undefined-behaviour sanitizers, drives it.  The conditions the shared cases have to meet
(tests/vocab_rescore_cases.py) are checked here with the restatement alone."""
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vocab_rescore_cases as K  # noqa: E402
import vocab_rescore_restatement as R  # noqa: E402

f32 = np.float32
OK, INVALID = 0, 1


def golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vocab_rescore") / "vocab_rescore_core_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "vocab_rescore_core_main.cpp"), "-o", path], check=True)
    return path


def run(exe, words):
    r = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        tag, _, rest = line.partition(" ")
        out.setdefault(tag, []).append(rest)
    assert "SMALL" not in out and "ORDER" not in out and "INPUT" not in out, r.stdout[-400:]
    return out


def verdict(out):
    code, _, text = out["VERDICT"][-1].partition(" ")
    return int(code), text


def dbits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


# ---- the restatement against the reference's own tests
def test_restatement_reproduces_the_known_answers():
    known = golden("vocab_rescore_known_answers.json")
    for c in known["similarities"]:
        assert abs(float(R.string_similarity(R.symbols(c["a"]), R.symbols(c["b"]))) - c["expected"]) <= c["accuracy"], c
    assert R.bits(R.string_similarity(R.symbols("nvida"), R.symbols("nvidia"))) == R.bits(f32(1) - f32(1) / f32(6))
    for c in known["normalized"]:
        assert R.normalize_for_similarity(c["text"]) == c["expected"], c
    for c in known["adaptive_cbw"]:
        assert abs(float(R.adaptive_cbw(c["cbw"], c["tokens"], c["config"])) - c["expected"]) <= c["accuracy"], c
    for c in known["arbitration"]:
        applied, superseded = R.arbitrate([(p["id"], f32(p["similarity"]), p["indices"][0], len(p["indices"])) for p in c["pending"]])
        if "applied" in c:
            assert applied == c["applied"], c["name"]
        else:
            assert sorted(applied) == c["applied_set"], c["name"]
        assert sorted(superseded) == c["superseded"], c["name"]
    forms = R.normalized_forms([R.symbols(R.normalize_for_similarity(t)) for t in ("New Rez", "newrez", "", "NEW  REZ!", "Newrez", "new rez llc")])
    assert [("".join(map(chr, f)), n) for f, n in forms] == [("new rez", 2), ("newrez", 1), ("new rez llc", 3)]   # :43-62: empty and repeated forms go


def test_stopword_lists():
    lists = golden("vocab_rescore_stopwords.json")
    stop, multi = set(lists["stopwords"]), set(lists["multi_word_stopwords"])
    assert len(stop) == len(lists["stopwords"]) == 122 and len(multi) == len(lists["multi_word_stopwords"]) == 83 and multi < stop
    assert set(lists["must_be_multi_word_stopwords"]) <= multi and not set(lists["must_not_be_multi_word_stopwords"]) & multi
    assert set(lists["must_be_stopwords"]) <= stop


# ---- the conditions of the shared cases, with the restatement alone
def test_boundary_pairs_land_on_their_thresholds():
    """Each (distance, length) pair of the table is the threshold itself in fp32, and the boundary problem has a candidate there."""
    table = {0.50: [(1, 2)], 0.52: [(12, 25)], 0.55: [(9, 20)], 0.60: [(2, 5)], 0.80: [(1, 5), (2, 10)], 0.85: [(3, 20)], 0.90: [(1, 10), (2, 20)]}
    for thr, pairs in table.items():
        for d, n in pairs:
            assert R.bits(f32(1) - f32(d) / f32(n)) == R.bits(f32(thr)), (thr, d, n)
    assert f32(3) / f32(4) == R.LENGTH_RATIO_THRESHOLD
    assert R.quantized(f32(0.875)) == 18 and R.quantized(f32(0.625)) == 13 and R.quantized(f32(0.7)) == 14
    p = K.boundary_problem()
    got = K.want("boundary", p)
    by_term = {}
    for u, k, start, span, origin, alias, sim in got:
        by_term.setdefault(k, []).append((start, span, origin, R.bits(sim)))
    b = lambda x: R.bits(f32(x))   # noqa: E731
    at = lambda k, start: [c for c in by_term.get(k, []) if c[0] == start]   # noqa: E731
    assert at(0, 0) == [(0, 1, R.SINGLE_WORD, b(0.5))] and not at(0, 1)                     # "a#" stays, "##" (similarity 0) goes
    assert at(1, 2) == [(2, 1, R.SINGLE_WORD, b(0.52))] and not at(1, 3)                    # 12 of 25 stays, 13 of 25 goes
    assert (4, 2, R.MULTI_WORD, b(0.55)) in at(2, 4) and not at(2, 5)                       # 9 of 20 stays, 10 of 20 goes
    assert at(3, 7) == [(7, 1, R.SINGLE_WORD, b(0.6))] and not at(3, 8)
    assert at(4, 9) == [(9, 1, R.SINGLE_WORD, b(0.8))] and not at(4, 10)                    # 4 of 6 characters: the rule lifts the bar to 0.8
    assert at(5, 11) == [(11, 1, R.SINGLE_WORD, b(0.8))] and not at(5, 12)
    assert at(6, 13) == [(13, 2, R.SINGLE_WORD, b(0.85))] and not at(6, 15)                 # ... and 4 of 20 with the stopword goes
    assert not at(7, 17) and [c[1] for c in at(7, 19)] == [2]                               # word 2 at 0.9 alone bars the compound
    assert not at(8, 21) and [c[1] for c in at(8, 24)] == [3]                               # word 3 at 0.9 alone bars it
    assert at(9, 27) == [(27, 1, R.SINGLE_WORD, b(0.75))]                                   # 3 of 4 characters: no lift, 0.75 passes 0.5


def test_shapes_problem_covers_the_block_edges():
    p = K.shapes_problem()
    got = K.want("shapes", p)
    assert [len(w) for w, _ in p["utterances"]] == list(K.SHAPE_WORDS)
    kept = {k for k, _, _ in R.kept_terms(p["terms"], p["min_term_length"])}
    assert 2 not in kept and 8 not in kept and 3 in kept                                   # below min_term_length; an empty canonical form is no reason
    assert not any(c[1] == 7 for c in got)                                                 # five words alone: no span
    for u, W in enumerate(K.SHAPE_WORDS):
        mine = [c for c in got if c[0] == u]
        assert (len(mine) > 0) == (W > 0) or W <= 3
        starts = {(c[2], c[3]) for c in mine if c[4] == R.SINGLE_WORD and c[1] == 0}
        if W >= 63:   # compounds of three words from the last word starts of a wavefront (62 starts and two neighbour lanes) and from the next one's first
            assert {(60 + k, 3) for k in range(min(3, W - 62))} <= starts, sorted(starts)
            assert {c[3] for c in mine if c[4] == R.MULTI_WORD} == {2, 3, 4}
        if W == 130:
            assert {(122, 3), (123, 3), (124, 3), (128, 2)} <= starts, sorted(starts)
    long_terms = {k for k, t in enumerate(p["terms"]) if len(t["forms"][0]) >= 31}
    assert {len(p["terms"][c[1]]["forms"][0]) for c in got if c[1] in long_terms} == {31, 32, 33, 63, 64}
    assert any(c[1] == 5 for c in got) and {c for c in got if c[1] == 6} < {c[:1] + (6,) + c[2:] for c in got if c[1] == 5}   # the higher minimum keeps fewer


def test_random_problems_meet_the_condition():
    problems = K.random_problems()
    assert len(problems) == 200
    total, near, classes = 0, 0, set()
    for i, p in enumerate(problems):
        got = K.want(("random", i), p)
        total += len(got)
        classes |= {(c[4], c[3]) for c in got}
        near += R.thresholds_near(got, p["terms"], p["min_term_length"], p["utterances"], p["min_similarity"])
    assert total >= 2000, total
    assert classes == {(R.MULTI_WORD, 2), (R.MULTI_WORD, 3), (R.MULTI_WORD, 4), (R.SINGLE_WORD, 1), (R.SINGLE_WORD, 2), (R.SINGLE_WORD, 3)}, classes
    assert near >= 50, near


def test_verdict_problem_covers_its_cases():
    import kws_restatement as KR
    p = K.verdict_problem()
    lp, valid = p["lp"], p["valid"]
    want, applied = K.verdict_want(p, lambda u, tok, a, b: KR.word_spot_constrained(list(lp[u, :valid[u]]), tok, a, b, p["blank"])[0])
    assert want[0]["window"][0] == 0 and want[11]["window"][1] == valid[0] and want[15]["window"] == (36, 40)          # clamped below and above
    assert want[5]["compared"] == 0 and want[5]["outcome"] == R.UNAVAILABLE                                           # an empty phrase row
    assert want[0]["alt_won"] == 1 and want[11]["alt_won"] == 0 and want[1]["alt_won"] == 0 and want[2]["alt_won"] == 0   # won, lost, equal rows, absent
    assert np.isneginf(want[9]["term_score"]) and want[9]["should_replace"] == 0 and want[9]["outcome"] == R.REJECTED  # the window is shorter than the keyword
    assert np.isneginf(want[10]["original_score"]) and want[10]["should_replace"] == 1
    assert want[12]["should_replace"] == 1 and want[12]["outcome"] == R.SUPERSEDED and want[11]["outcome"] == R.SUPERSEDED   # word 11 is occupied
    assert want[6]["should_replace"] == want[7]["should_replace"] == 1 and want[6]["outcome"] == R.APPLIED and want[7]["outcome"] == R.SUPERSEDED   # ties in all three keys
    assert R.quantized(p["cands"][0][6]) == 18 and R.quantized(p["cands"][5][6]) == 13                                # the bucket halves
    assert {v["outcome"] for v in want} == {R.APPLIED, R.SUPERSEDED, R.REJECTED, R.UNAVAILABLE} and all(applied)


# ---- vocab_rescore_core.h under the sanitizers
def test_bit_vector_step_equals_the_plain_dp(exe):
    pairs, prefixes, wrong = (int(x) for x in run(exe, ["bitdp"])["BITDP"][0].split())
    assert pairs == (1093 - 1) * 1093 + 5 * 200 and prefixes > 5 * pairs and wrong == 0


def check_blob(exe, terms, min_term_length):
    out = run(exe, ["build"] + K.vocabulary_words(terms, min_term_length))
    assert verdict(out) == (OK, "")
    want = R.blob_contents(terms, min_term_length)
    assert [int(x) for x in out.get("ALPHABET", [""])[0].split()] == want["alphabet"]
    assert [[int(x) for x in s.split()][1:] for s in out.get("STRING", [])] == want["strings"]
    assert [int(s.split()[0]) for s in out.get("STRING", [])] == list(range(len(want["strings"])))
    forms = iter(out.get("FORM", []))
    assert len(out.get("TERM", [])) == len(want["terms"])
    for line, t in zip(out.get("TERM", []), want["terms"]):
        src, cc, has_min, min_bits, canon, n_forms = (int(x) for x in line.split())
        assert (src, cc, canon, n_forms) == (t["term"], t["char_count"], t["canonical_sid"], len(t["forms"]))
        assert (has_min, min_bits) == ((0, 0) if t["min_similarity"] is None else (1, R.bits(f32(t["min_similarity"]))))
        for f in t["forms"]:
            rec = next(forms).split()
            assert [int(x) for x in rec[:3]] == [f["sid"], len(f["symbols"]), f["words"]]
            assert {int(a): int(b, 16) for a, b in (m.split(":") for m in rec[3:])} == f["masks"]
    return out


def test_blob_build_equals_the_restatement(exe):
    p = K.shapes_problem()
    check_blob(exe, p["terms"], p["min_term_length"])
    check_blob(exe, p["terms"], 1)
    check_blob(exe, K.boundary_problem()["terms"], 2)
    check_blob(exe, [], 3)
    check_blob(exe, [K.term("", char_count=9)], 3)
    check_blob(exe, K.alphabet_terms(1022), 3)                                             # A = 1023
    out = run(exe, ["build"] + K.vocabulary_words(K.alphabet_terms(1023), 3))
    assert verdict(out) == (INVALID, "the forms use 1023 distinct symbols, at most 1022 are supported")
    out = run(exe, ["build"] + K.vocabulary_words([K.term("abc"), K.term("ab", aliases=("a" * 64, "b" * 65))], 3))
    assert verdict(out) == (INVALID, "term 1 form 2 has 65 symbols, at most 64 are supported")
    out = run(exe, ["build"] + K.vocabulary_words([dict(char_count=3, min_similarity=float("nan"), forms=[R.symbols("abc")])], 3))
    assert verdict(out) == (INVALID, "term 0: min_similarity is not a number")


def test_corrupted_blob_is_refused_before_it_is_used(exe):
    """Every header word and every index of a blob damaged in turn: validate() refuses each, and the sanitizers saw no read outside it."""
    p = K.shapes_problem()
    tried, refused = (int(x) for x in run(exe, ["corrupt"] + K.vocabulary_words(p["terms"][:6], 3))["CORRUPT"][0].split())
    assert tried > 200 and refused == tried


def walk(exe, p):
    out = run(exe, ["walk"] + K.vocabulary_words(p["terms"], p["min_term_length"]) + [R.bits(p["min_similarity"])] + K.utterance_words(p["utterances"]))
    assert verdict(out) == (OK, "")
    return [tuple(int(x) for x in line.split()) for line in out.get("CAND", [])]


def as_records(cands):
    return [(u, k, start, span, origin, alias, R.bits(sim)) for u, k, start, span, origin, alias, sim in cands]


def test_reference_walk_equals_the_restatement(exe):
    for name, p in (("shapes", K.shapes_problem()), ("boundary", K.boundary_problem())):
        want = as_records(K.want(name, p))
        assert len(want) > 10 and walk(exe, p) == want, name
    for i, p in enumerate(K.random_problems()[:40]):
        assert walk(exe, p) == as_records(K.want(("random", i), p)), i


def test_arbitration_equals_the_restatement(exe):
    rng = np.random.default_rng(4)
    cases = [[(i, f32(p["similarity"]), p["indices"][0], len(p["indices"])) for i, p in enumerate(c["pending"])] for c in golden("vocab_rescore_known_answers.json")["arbitration"]]
    cases.append([(0, f32(0.875), 0, 2), (1, f32(0.625), 1, 1), (2, f32(0.875), 1, 1), (3, f32(0.625), 3, 1), (4, f32(0.625), 3, 1), (5, f32(0.624), 2, 2)])   # halves; ties in all keys
    for _ in range(60):
        n = int(rng.integers(0, 12))
        cases.append([(i, f32(rng.choice([0.5, 0.55, 0.6, 0.625, 0.66, 0.7, 0.75, 0.874, 0.875, 0.9, 1.0])), int(rng.integers(0, 9)), int(rng.integers(1, 4))) for i in range(n)])
    for k, pending in enumerate(cases):
        W = 12
        occupied = [int(x) for x in (rng.random(W) < (0.2 if k % 3 == 0 else 0.0))]
        out = run(exe, ["arbitrate", len(pending)] + [x for _, s, first, span in pending for x in (R.bits(s), first, span)] + [W] + occupied)
        applied, superseded = R.arbitrate(pending, [i for i, o in enumerate(occupied) if o])
        assert [int(x) for x in out["APPLIED"][0].split()] == applied, pending
        assert [int(x) for x in out["SUPERSEDED"][0].split()] == sorted(superseded)
        assert [int(x) for x in out["BUCKETS"][0].split()] == [R.quantized(s) for _, s, _, _ in pending]


def test_window_arithmetic_equals_the_restatement(exe):
    cases = [(0.0, 0.2, 0.08, 0.1, 36), (2.7, 3.4, 0.08, 0.1, 36), (1.0, 1.3, 0.08, 0.1, 36), (0.04, 0.05, 0.08, 0.1, 36), (5.0, 6.0, 0.08, 0.1, 36), (0.24, 0.32, 0.08, 0.0, 36),
             (0.3, 0.1, 0.04, 0.25, 10), (1e9, 2e9, 0.08, 0.1, 36), (-1.0, -0.5, 0.08, 0.1, 36), (0.56, 0.5600000000000001, 0.07, 0.1, 50), (3 * 0.1, 7 * 0.1, 0.1, 0.1, 50)]
    for a, b, fd, margin, valid in cases:
        out = run(exe, ["window", dbits(a), dbits(b), dbits(fd), dbits(margin), valid])
        assert out["WINDOW"][0] == "%d %d" % R.frame_window(a, b, fd, margin, valid), (a, b, fd, margin, valid)
    for a, b in ((float("nan"), 1.0), (0.0, float("inf")), (0.0, 1e30)):
        assert run(exe, ["window", dbits(a), dbits(b), dbits(0.08), dbits(0.1), 36])["WINDOW"][0] == "none"


def test_boost_is_within_one_ulp_of_float64(exe):
    """fa_vocab_rescore_boost (the same function as vr::boost): its log2 / pow value is within 1 fp32 ulp of a float64 evaluation — the
    result lies between the reference's fp32 arithmetic applied to that value's two neighbours — and exact where the ratio is a power of two."""
    def arithmetic(l, cbw):
        return f32(cbw) * (f32(1.0) + f32(l) * f32(0.3))

    def boosts(queries):
        out = run(exe, ["boost", len(queries)] + [x for cbw, tokens, on, ref, pivot, exponent in queries for x in (R.bits(f32(cbw)), tokens, on, ref, pivot, R.bits(f32(exponent)))])
        return [int(x) for x in out["BOOST"]]
    queries = [(cbw, tokens, 1, ref, 1, 2.0) for cbw in (3.0, 4.5, 0.7) for ref in (1, 3, 5) for tokens in range(1, 40)]
    for (cbw, tokens, _, ref, _, _), got in zip(queries, boosts(queries)):
        assert got == R.bits(R.adaptive_cbw(cbw, tokens, dict(reference_token_count=ref)))
        if tokens > ref:
            ratio = f32(tokens) / f32(ref)
            l = f32(math.log2(float(ratio)))
            lo, hi = arithmetic(np.nextafter(l, f32(-np.inf)), cbw), arithmetic(np.nextafter(l, f32(np.inf)), cbw)
            assert R.bits(lo) <= got <= R.bits(hi)
            if tokens % ref == 0 and (tokens // ref) & (tokens // ref - 1) == 0:
                assert got == R.bits(arithmetic(f32(int(math.log2(tokens // ref))), cbw))
        else:
            assert got == R.bits(f32(cbw))
    queries = [(4.5, tokens, 1, 5, pivot, exponent) for pivot, exponent in ((5, 2.0), (8, 1.5), (4, 0.5)) for tokens in range(0, 9)]
    for (_, tokens, _, _, pivot, exponent), got in zip(queries, boosts(queries)):
        assert got == R.bits(R.adaptive_cbw(4.5, tokens, dict(reference_token_count=5, short_term_taper_pivot=pivot, short_term_taper_exponent=exponent)))
        if tokens < pivot:
            x = f32(math.pow(float(f32(max(1, tokens)) / f32(pivot)), exponent))
            assert R.bits(f32(4.5) * np.nextafter(x, f32(0))) <= got <= R.bits(f32(4.5) * np.nextafter(x, f32(2)))
    assert boosts([(3.0, 10, 0, 3, 1, 2.0)]) == [R.bits(f32(3.0))]
