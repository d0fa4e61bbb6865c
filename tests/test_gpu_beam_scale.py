"""CTC prefix beam search on the device (kernels: csrc/beam.hip, host side: csrc/beam_host.hip) against the compiled restatement (oracle.ctc_beam_search_c) at the shapes the
kernel exists for and at its limits: the benchmark's shape with a 4 000-word / 32 000-bigram model, beam 128 x 64 candidates on an 8 193-token
vocabulary, a ragged batch, a batch split over two launches, the strided device entry over poisoned padding, and multi-byte pieces.
Per utterance: token ids identical, scores within the tolerance of test_beam.py.  Every case with a model shows that the model acts: most
decoded words are model words, and the model changes the best prefix of at least one utterance."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from beam_fixtures import (SYLLABLES, W, WIDE_SYLLABLES, bench_log_probs, large_arpa, lm_vocab, peaky_log_probs,  # noqa: E402
                           words_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big_model(oracle_mod):
    """(ARPA text, its words, the Python model, its C tables)"""
    text, words = large_arpa(seed=0)
    py = oracle_mod.ARPALanguageModel.parse(text)
    with oracle_mod.CLanguageModel(py) as cm:
        yield text, words, py, cm


def oracle_batch(o, x, voc, lm, beam, lw, wb, blank, K, valid=None, which=None):
    """the restatement per utterance, utterances side by side on host threads (the C walk runs without the GIL)"""
    which = range(x.shape[0]) if which is None else which
    jobs = [(x[b], None if valid is None else valid[b]) for b in which]
    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(lambda j: o.ctc_beam_search_c(j[0], voc, lm, beam, lw, wb, blank, K, valid_frames=j[1]), jobs))


def assert_matches(ids, scores, wants, which=None):
    which = range(len(wants)) if which is None else which
    for b, (want, total) in zip(which, wants):
        assert ids[b] == want, (b, len(ids[b]), len(want), next((i for i, (p, q) in enumerate(zip(ids[b], want)) if p != q), None))
        if total is None:
            assert scores[b] == 0.0, b
        else:
            assert scores[b] == pytest.approx(total, rel=2e-6, abs=2e-5), b


def assert_model_acts(ids_lm, ids_plain, voc, py):
    """most decoded words are model words; the model changes at least one best prefix"""
    words = [w for ids in ids_lm for w in words_of(ids, voc)]
    known = sum(w in py.unigrams for w in words)
    assert words and known > len(words) / 2, (known, len(words))
    assert any(a != b for a, b in zip(ids_lm, ids_plain))


@pytest.mark.parametrize("word_bonus", [0.0, 0.5])
def test_bench_shape_with_a_large_model(fa, gpu_ctx, oracle_mod, big_model, word_bonus):
    """bench.py's beam leg per utterance: T = 1 500, V = 1 025 (blank last), beam 100, 40 candidates, lm_weight 0.3 — with a model of
    4 000+ words whose device tables are probed on and past their first slot"""
    o = oracle_mod
    text, words, py, cm = big_model
    B, T, V, blank = 8, 1500, 1025, 1024
    x = bench_log_probs(B, T, V, blank, seed=21)
    voc = lm_vocab(V, blank, words, seed=4)
    lm = fa.ARPALanguageModel(text, ctx=gpu_ctx)
    ids, scores = fa.ctc_beam_search_ids_batch(x, voc, lm, 100, 0.3, word_bonus, blank, 40, ctx=gpu_ctx)
    assert_matches(ids, scores, oracle_batch(o, x, voc, cm, 100, 0.3, word_bonus, blank, 40))
    plain, plain_scores = fa.ctc_beam_search_ids_batch(x, None, None, 100, 0.3, word_bonus, blank, 40, ctx=gpu_ctx)
    if word_bonus == 0.0:
        assert_matches(plain, plain_scores, oracle_batch(o, x, voc, None, 100, 0.3, 0.0, blank, 40))
    assert_model_acts(ids, plain, voc, py)


@pytest.mark.parametrize("use_lm", [False, True])
def test_limits_against_the_restatement(fa, gpu_ctx, oracle_mod, big_model, use_lm):
    """the largest configuration (beam 128, 64 candidates: 8 320 candidates a frame, the ctc_beam_kernel<32> instance) on a TDT-sized
    vocabulary (8 193 tokens: keys re-read from HBM by the top-token pre-pass) over 400 frames"""
    o = oracle_mod
    text, words, py, cm = big_model
    B, T, V, blank = 2, 400, 8193, 8192
    x = peaky_log_probs(B, T, V, 4.0, seed=3)
    voc = lm_vocab(V, blank, words, seed=5)
    lm = fa.ARPALanguageModel(text, ctx=gpu_ctx) if use_lm else None
    ids, scores = fa.ctc_beam_search_ids_batch(x, voc, lm, 128, 0.3, 0.25, blank, 64, ctx=gpu_ctx)
    assert_matches(ids, scores, oracle_batch(o, x, voc, cm if use_lm else None, 128, 0.3, 0.25, blank, 64))
    if use_lm:
        plain, _ = fa.ctc_beam_search_ids_batch(x, None, None, 128, 0.3, 0.25, blank, 64, ctx=gpu_ctx)
        assert_model_acts(ids, plain, voc, py)


def test_ragged_batch(fa, gpu_ctx, oracle_mod, big_model):
    """14 utterances in one launch with valid frame counts 0, 1, 2, ..., T: workgroups that finish at once or early sit next to long ones"""
    o = oracle_mod
    text, words, py, cm = big_model
    B, T, V, blank = 14, 320, 1025, 0
    x = bench_log_probs(B, T, V, blank, seed=8)
    voc = lm_vocab(V, blank, words, seed=6)
    valid = [0, 1, T, 2, 150, T, 7, T - 1, 0, 64, T, 1, 33, 250]
    lm = fa.ARPALanguageModel(text, ctx=gpu_ctx)
    ids, scores = fa.ctc_beam_search_ids_batch(x, voc, lm, 64, 0.5, 0.25, blank, 40, valid_frames=valid, ctx=gpu_ctx)
    wants = oracle_batch(o, x, voc, cm, 64, 0.5, 0.25, blank, 40, valid=valid)
    assert_matches(ids, scores, wants)
    assert [len(i) == 0 for i in ids[:2]] == [True, False]
    plain, _ = fa.ctc_beam_search_ids_batch(x, None, None, 64, 0.5, 0.25, blank, 40, valid_frames=valid, ctx=gpu_ctx)
    assert_model_acts(ids, plain, voc, py)


def test_two_launches_against_the_restatement(fa, gpu_ctx, oracle_mod, big_model):
    """258 utterances x 2 049 frames x beam 128 exceed the 2 GiB trie cap of a launch: 256 + 2 go through two launches, each with its own
    pre-pass and table; utterances on both sides of the cut equal the restatement, with a model"""
    o = oracle_mod
    text, words, py, cm = big_model
    B, T, V, blank = 258, 2049, 6, 5
    plan = (C.c_int64 * 4)()
    assert fa.lib().fa_ctc_beam_plan(B, T, V, 128, blank, 3, plan) == 0 and (plan[1], plan[2]) == (256, 2)
    x = peaky_log_probs(B, T, V, 1.5, seed=77)
    voc = {0: W + "ka", 1: "to", 2: W + "mi", 3: W + "neru", 4: W}
    valid = [T] * B
    valid[255], valid[257] = T - 7, 11
    lm = fa.ARPALanguageModel(text, ctx=gpu_ctx)
    ids, scores = fa.ctc_beam_search_ids_batch(x, voc, lm, 128, 0.3, 0.1, blank, 3, valid_frames=valid, ctx=gpu_ctx)
    which = [0, 1, 254, 255, 256, 257]
    assert_matches(ids, scores, oracle_batch(o, x, voc, cm, 128, 0.3, 0.1, blank, 3, valid=valid, which=which), which=which)
    assert all(len(ids[b]) > 0 for b in which)
    plain, _ = fa.ctc_beam_search_ids_batch(x, None, None, 128, 0.3, 0.1, blank, 3, valid_frames=valid, ctx=gpu_ctx)
    assert_model_acts([ids[b] for b in which], [plain[b] for b in which], voc, py)


def test_strided_device_entry_reads_no_padding(fa, gpu_ctx, oracle_mod, big_model):
    """fa_ctc_beam_search_batch_dev with rows of 1 032 floats for 1 025 tokens, a gap between utterances and device valid-frame counts:
    the row padding, the gaps and the rows past an utterance's end hold +inf / NaN (a read of any of them would change the top tokens);
    the result equals the contiguous call bit for bit, and the restatement"""
    import torch
    o = oracle_mod
    text, words, py, cm = big_model
    B, T, V, blank, RS = 6, 200, 1025, 1024, 1032
    MS = T * RS + 517
    x = bench_log_probs(B, T, V, blank, seed=13)
    voc = lm_vocab(V, blank, words, seed=7)
    valid = [T, 0, 1, 120, T - 3, T]
    buf = np.full(B * MS, np.nan, np.float32)
    rows = buf[:B * MS].reshape(B, MS)
    for b in range(B):
        m = rows[b, :T * RS].reshape(T, RS)
        m[:, V:] = np.inf if b % 2 else np.nan                               # row padding
        m[:valid[b], :V] = x[b, :valid[b]]                                   # rows past valid[b] stay NaN / +inf
        m[valid[b]:, :] = np.inf if b % 2 == 0 else np.nan
        rows[b, T * RS:] = np.inf if b % 3 == 0 else np.nan                  # the gap behind the utterance
    lm = fa.ARPALanguageModel(text, ctx=gpu_ctx)
    vocab = fa.CtcVocabulary(voc, V, gpu_ctx)
    d_lp = torch.from_numpy(buf).to("cuda")
    d_valid = torch.tensor(valid, dtype=torch.int32, device="cuda")
    tok = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((B,), np.nan, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.check(fa.lib().fa_ctc_beam_search_batch_dev(gpu_ctx.handle, d_lp.data_ptr(), B, T, V, RS, MS, d_valid.data_ptr(), vocab.handle,
                                                        lm.handle, 100, 0.3, 0.25, blank, 40, tok.data_ptr(), lens.data_ptr(), sc.data_ptr()),
                  "fa_ctc_beam_search_batch_dev")
    tok, lens, sc = tok.cpu().numpy(), lens.cpu().numpy(), sc.cpu().numpy()
    got = [tok[b, :lens[b]].tolist() for b in range(B)]
    ids, scores = fa.ctc_beam_search_ids_batch(x, voc, lm, 100, 0.3, 0.25, blank, 40, valid_frames=valid, ctx=gpu_ctx)
    assert got == ids
    assert sc.view(np.uint32).tolist() == scores.view(np.uint32).tolist()
    assert_matches(got, sc, oracle_batch(o, x, voc, cm, 100, 0.3, 0.25, blank, 40, valid=valid))


def test_multibyte_pieces_and_words(fa, gpu_ctx, oracle_mod):
    """pieces with 2-, 3- and 4-byte characters right after the boundary ("▁über", "▁中", "▁🙂"), pieces that are only "▁", empty
    pieces and ids without one; the model's words are made of the same characters"""
    o = oracle_mod
    syl = WIDE_SYLLABLES + SYLLABLES[:6]
    text, words = large_arpa(seed=2, n_three=400, n_bigrams=3000, syllables=syl)
    py = o.ARPALanguageModel.parse(text)
    assert any(not w.isascii() for w in py.unigrams)
    B, T, V, blank = 4, 400, 301, 300
    voc = lm_vocab(V, blank, words, seed=9, word_share=0.97, syllables=syl)
    for v in range(0, V - 1, 13):
        voc[v] = W                                                           # only the boundary
    for v in range(5, V - 1, 17):
        voc[v] = ""                                                          # an empty piece
    for v in range(7, V - 1, 19):
        voc.pop(v, None)                                                     # no piece
    x = bench_log_probs(B, T, V, blank, seed=31)
    lm = fa.ARPALanguageModel(text, ctx=gpu_ctx)
    ids, scores = fa.ctc_beam_search_ids_batch(x, voc, lm, 48, 0.5, 0.3, blank, 24, ctx=gpu_ctx)
    with o.CLanguageModel(py) as cm:
        assert_matches(ids, scores, oracle_batch(o, x, voc, cm, 48, 0.5, 0.3, blank, 24))
    assert any(not w.isascii() for i in ids for w in words_of(i, voc))
    plain, _ = fa.ctc_beam_search_ids_batch(x, None, None, 48, 0.5, 0.3, blank, 24, ctx=gpu_ctx)
    assert_model_acts(ids, plain, voc, py)
