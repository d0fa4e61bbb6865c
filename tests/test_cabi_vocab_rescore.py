"""The vocabulary rescorer's C ABI: VocabularyRescorer of include/fluidaudio.hpp from a C++ host built with g++ -Werror
(tests/cabi/vocab_rescore.cpp) and the entries through ctypes, against the Python restatement (tests/vocab_rescore_restatement.py).
CPU tier: the build with its refusals and their texts, every entry's answer to a missing context.  GPU tier: the refusals of the
candidate and the verdict entry with their texts — answered before any device work —, the capacity contract, and ctcTokenRescore."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kws_restatement as KR  # noqa: E402
import vocab_rescore_cases as K  # noqa: E402
import vocab_rescore_restatement as R  # noqa: E402

f32 = np.float32
OK, INVALID, TOO_SMALL = 0, 1, 3


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "vocab_rescore_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "vocab_rescore.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def hex32(x):
    return f"{R.bits(x):08x}"


def vocabulary():
    """tests/cabi/vocab_rescore.cpp's"""
    return [K.term("livmarli"), K.term("newrez", aliases=("new rez",), min_similarity=0.6), K.term("ab")]


def test_build_and_missing_context_without_a_device(host, fa):
    r = subprocess.run([host, "args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [l.split(" ", 1) for l in r.stdout.splitlines()]
    builds = [l[1] for l in out if l[0] == "BUILD"]
    assert builds[0] == "0"
    assert builds[1] == "1 fa_vocab_rescore_build: status 1 (term 0 form 1 has 65 symbols, at most 64 are supported)"
    assert builds[2] == "1 fa_vocab_rescore_build: status 1 (the forms use 1023 distinct symbols, at most 1022 are supported)"
    blob = fa.vocab_rescore.build(vocabulary())
    assert [l[1] for l in out if l[0] == "BLOB"] == [str(blob.size)]
    assert [l[1] for l in out if l[0] == "ST"] == ["1 1 1 1 0"]
    assert [l[1] for l in out if l[0] == "COUNT"] == ["0 24"]   # *count is set whatever the status; an empty vocabulary is a header
    assert [l[1] for l in out if l[0] == "CFG"] == [f"0.080 0.100 {hex32(3.0)} 1024 1 3 1 {hex32(2.0)}"]
    assert [l[1] for l in out if l[0] == "BOOST"] == [" ".join(hex32(R.adaptive_cbw(3.0, n)) for n in (3, 6, 12))]
    assert fa.vocab_rescore.boost(3.0, 6) == float(f32(3.0) * f32(1.3))


def test_build_refusals_through_ctypes(fa):
    V = fa.vocab_rescore
    for terms, text in (([K.term("abc", aliases=("a" * 65,))], "term 0 form 1 has 65 symbols, at most 64 are supported"),
                        (K.alphabet_terms(1023), "the forms use 1023 distinct symbols, at most 1022 are supported"),
                        ([dict(char_count=3, min_similarity=float("nan"), forms=[R.symbols("abc")])], "term 0: min_similarity is not a number")):
        with pytest.raises(fa.FluidAudioHipError) as e:
            V.build(terms)
        assert e.value.status == INVALID and text in str(e.value)
    assert V.build(K.alphabet_terms(1022)).size > 1022 * 2 * 18
    lib = fa.lib()
    counts, rows, off, syms = np.asarray([3], np.int32), np.asarray([0, 1], np.int64), np.asarray([0, 3], np.int64), np.asarray([1, 2, 3], np.int32)
    need, text, blob = C.c_int64(), C.create_string_buffer(128), np.full(64, -1, np.int32)
    build = lambda *a: lib.fa_vocab_rescore_build(counts.ctypes.data, None, *a)   # noqa: E731
    assert build(rows.ctypes.data, off.ctypes.data, syms.ctypes.data, 1, 3, None, 0, C.byref(need), text, 128) == OK and need.value == 24 + 8 + 4 + 2 + 3 + 3 + 4 * 2
    assert build(rows.ctypes.data, off.ctypes.data, syms.ctypes.data, 1, 3, blob.ctypes.data, need.value - 1, C.byref(need), text, 128) == TOO_SMALL
    assert text.value == b"the blob needs 52 words, the buffer holds 51" and blob[0] == -1
    assert build(rows.ctypes.data, off.ctypes.data, syms.ctypes.data, 1, 3, None, 5, C.byref(need), text, 128) == INVALID
    assert build(rows.ctypes.data, off.ctypes.data, None, 1, 3, None, 0, C.byref(need), text, 128) == INVALID and text.value == b"symbols is required"
    assert build(rows.ctypes.data, None, syms.ctypes.data, 1, 3, None, 0, C.byref(need), text, 128) == INVALID and text.value == b"row_offsets is required"
    bad = np.asarray([0, -1], np.int64)
    assert build(bad.ctypes.data, off.ctypes.data, syms.ctypes.data, 1, 3, None, 0, C.byref(need), text, 128) == INVALID and text.value == b"term_rows does not ascend at term 0"
    assert build(rows.ctypes.data, off.ctypes.data, syms.ctypes.data, 1, 3, blob.ctypes.data, 64, C.byref(need), None, 0) == OK and blob[0] != -1


@pytest.fixture(scope="module")
def small(fa):
    p = dict(terms=vocabulary(), min_term_length=3, min_similarity=R.MIN_SIMILARITY_FLOOR,
             utterances=[([R.symbols(w) for w in ("liv", "marli", "", "new", "res", "the")], [0, 0, 0, 0, 0, 3]), ([], []), ([R.symbols("nevrez")], [0])])
    return p, fa.vocab_rescore.build(p["terms"]), [(u, k, a, n, o, f, R.bits(s)) for u, k, a, n, o, f, s in K.want("cabi-small", p)]


def records(recs):
    return [(int(r["utterance"]), int(r["term"]), int(r["first_word"]), int(r["span_len"]), int(r["origin"]), int(r["form"]), R.bits(r["similarity"])) for r in recs]


@pytest.mark.gpu
def test_capacity_contract(fa, gpu_ctx, small):
    """fa_ctc_kws_spot_batch's: *count and the utterance counts are whole, the first `capacity` records are written, the rest is untouched."""
    p, blob, want = small
    V = fa.vocab_rescore
    total = len(want)
    assert total >= 4 and {w[0] for w in want} == {0, 2}
    for capacity in (0, 1, total - 1, total, total + 3):
        utt_off, word_off, flat, flags = V._pack_words(p["utterances"])
        recs, counts, n = np.zeros(total + 4, V.VR_CANDIDATE_DTYPE), np.full(3, -1, np.int64), C.c_int64(-1)
        recs["utterance"] = -7
        st = fa.lib().fa_vocab_rescore_candidates(gpu_ctx.handle, blob.ctypes.data, blob.size, utt_off.ctypes.data, 3, word_off.ctypes.data, flat.ctypes.data, flags.ctypes.data,
                                                  0.5, recs.ctypes.data, capacity, C.byref(n), counts.ctypes.data)
        assert st == (OK if capacity >= total else TOO_SMALL), capacity
        if st != OK:
            assert gpu_ctx.last_error() == f"vocab_rescore_candidates: output holds {capacity} of {total} candidates"
        assert n.value == total and counts.tolist() == [sum(1 for w in want if w[0] == u) for u in range(3)]
        assert records(recs[:min(capacity, total)]) == want[:capacity] and (recs["utterance"][min(capacity, total):] == -7).all()
    n = C.c_int64(-1)   # no output at all: the count alone
    assert fa.lib().fa_vocab_rescore_candidates(gpu_ctx.handle, blob.ctypes.data, blob.size, utt_off.ctypes.data, 3, word_off.ctypes.data, flat.ctypes.data, flags.ctypes.data,
                                                0.5, None, 0, C.byref(n), None) == OK and n.value == total


@pytest.mark.gpu
def test_refusals_with_their_texts(fa, gpu_ctx, small):
    p, blob, want = small
    V = fa.vocab_rescore
    lib, h = fa.lib(), gpu_ctx.handle
    utt_off, word_off, flat, flags = V._pack_words(p["utterances"])
    n = C.c_int64(-1)

    def cand(blob=blob, words=blob.size, utt=utt_off, batch=3, woff=word_off, syms=flat, fl=flags, min_similarity=0.5, capacity=0, out=None):
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        st = lib.fa_vocab_rescore_candidates(h, ptr(blob), words, ptr(utt), batch, ptr(woff), ptr(syms), ptr(fl), min_similarity, out, capacity, C.byref(n), None)
        return st, gpu_ctx.last_error()
    where = "vocab_rescore_candidates: "
    assert cand(capacity=-1) == (INVALID, where + "negative capacity, or a capacity without an output")
    assert cand(capacity=4) == (INVALID, where + "negative capacity, or a capacity without an output")
    assert cand(words=blob.size - 1) == (INVALID, where + "not a vocabulary blob, or a section leaves it")
    broken = blob.copy()
    broken[6] = blob.size   # the forms begin where the blob ends
    assert cand(blob=broken) == (INVALID, where + "not a vocabulary blob, or a section leaves it")
    broken = blob.copy()
    broken[int(blob[6])] = int(blob[7])   # form 0 names a string behind the table
    assert cand(blob=broken) == (INVALID, where + f"blob: form 0 names string {int(blob[7])}")
    assert cand(min_similarity=float("nan")) == (INVALID, where + "min_similarity is not a number")
    assert cand(utt=np.asarray([0, 6, 5, 7], np.int64)) == (INVALID, where + "utterance_offsets does not ascend at utterance 1")
    bad = word_off.copy()
    bad[3] = 1
    assert cand(woff=bad) == (INVALID, where + "word_offsets does not ascend at word 2")
    assert cand(fl=None) == (INVALID, where + "word_offsets and word_flags are required")
    assert cand(syms=None) == (INVALID, where + "word_symbols is required")
    assert cand(batch=-1) == (INVALID, where + "negative batch")
    assert n.value == 0
    assert cand()[0] == OK and n.value == len(want)

    lp = np.zeros((3, 12, 8), np.float32)
    cands = np.zeros(1, V.VR_CANDIDATE_DTYPE)
    cands[0] = (0, 0, 0, 2, 2, 0, 0.75)
    starts, ends = [0.0] * 7, [0.1] * 7

    def decide(c=cands, words=(6, 0, 1), st=starts, en=ends, terms=([1, 2], [3], [1]), alts=([], [], []), phrases=([1],), config=None, occupied=None):
        with pytest.raises(fa.FluidAudioHipError) as e:
            V.decide(lp, c, words, st, en, list(terms), list(alts), list(phrases), config=config, occupied=occupied, ctx=gpu_ctx)
        assert e.value.status == INVALID
        return str(e.value).split("(", 1)[1][:-1]
    where = "vocab_rescore_decide: "
    for field, value, text in (("utterance", 3, "candidate 0 names utterance 3, term 0"), ("term", 3, "candidate 0 names utterance 0, term 3"),
                               ("first_word", 5, "candidate 0 spans the words 5 + 2 of 6"), ("span_len", 0, "candidate 0 spans the words 0 + 0 of 6"),
                               ("similarity", float("nan"), "candidate 0's similarity is not a usable number")):
        c = cands.copy()
        c[field] = value
        assert decide(c=c) == where + text
    cfg = V.default_config()
    cfg.frame_duration = 0.0
    assert decide(config=cfg) == where + "frame_duration has to be positive and finite, margin_seconds finite"
    assert decide(st=[float("inf")] * 7) == where + "candidate 0's times give no frame window"
    assert decide(terms=([1] * 128, [3], [1])) == where + "term 0 has 128 tokens, at most 127 are supported"
    assert decide(phrases=([1] * 128,)) == where + "candidate 0's phrase has 128 tokens, at most 127 are supported"
    verdicts, applied = V.decide(lp, cands, (6, 0, 1), starts, ends, [[1, 2], [3], [1]], [[], [], []], [[1]], ctx=gpu_ctx)
    assert len(verdicts) == 1 and applied[1:] == [[], []]


@pytest.mark.gpu
def test_token_rescore_from_cpp(host):
    r = subprocess.run([host, "rescore"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    words = [R.symbols(w) for w in ("liv", "marli", "", "new", "res", "the")]
    terms = vocabulary()
    found = R.candidates(terms, 3, [(words, [0, 0, 0, 0, 0, 3])])
    lp = [np.asarray([f32(-0.5) * f32((t * 5 + v * 3) % 7) for v in range(8)], np.float32) for t in range(12)]
    term_tokens, alt_tokens = [[1, 2], [3, 4, 5, 6], [1]], [[2], [], []]
    p = dict(cands=found, phrase_tokens=[[(c[2] + k) % 7 for k in range(c[3])] for c in found], valid=[12], frame_duration=0.08, margin=0.10,
             starts=[[0.16 * i for i in range(6)]], ends=[[0.16 * (i + 1) for i in range(6)]], term_tokens=term_tokens, alt_tokens=alt_tokens, cbw=f32(3.0), config=None,
             occupied=[[0] * 6])
    verdicts, applied = K.verdict_want(p, lambda u, tok, a, b: KR.word_spot_constrained(lp, tok, a, b, 7)[0])
    assert len(found) >= 3 and {c[3] for c in found} >= {1, 2} and any(v["should_replace"] for v in verdicts)
    want = [[str(c[1]), str(c[2]), str(c[3]), str(c[4]), str(c[5]), hex32(c[6]), "VERDICT", hex32(v["term_score"]), hex32(v["original_score"]), hex32(v["boost"]),
             hex32(v["boosted_score"]), str(v["alt_won"]), str(v["compared"]), str(v["should_replace"]), str(v["outcome"]), str(v["window"][0]), str(v["window"][1])]
            for c, v in zip(found, verdicts)]
    assert [l[1:] for l in out if l[0] == "CAND"] == want
    assert [l[1:] for l in out if l[0] == "APPLIED"] == [[str(i) for i in applied[0]]]
    assert [l[1:] for l in out if l[0] == "ASKED"] == [[str(len({(c[2], c[3]) for c in found}))]]
