"""fa_edit_distance_batch / fa_edit_distance_batch_dev (csrc/wer.hip, csrc/wer_host.hip) on the device against the restatement with the full table and the
traceback (tests/wer_restatement.py).  No tolerances: all four integers and both lengths of every pair.  The same file is run on the
poisoned-workspace library (make POISON=1).  The restatement fills fewer than 3e6 table cells for the whole file, once."""
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wer_cases as W  # noqa: E402
import wer_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def expected(pairs):
    out = np.zeros(len(pairs), [("total", np.int32), ("insertions", np.int32), ("deletions", np.int32), ("substitutions", np.int32),
                                ("hyp_len", np.int32), ("ref_len", np.int32)])
    for k, (hyp, ref) in enumerate(pairs):
        out[k] = tuple(R.edit_distance(list(hyp), list(ref))) + (len(hyp), len(ref))
    return out


@pytest.fixture(scope="module")
def shapes():
    """Every boundary of the schedule in both families, and the restatement's answers — computed once, never modified."""
    pairs = W.shape_pairs()
    want = expected([(h.tolist(), r.tolist()) for h, r in pairs])
    want.setflags(write=False)
    return pairs, want


def same(got, want):
    assert got.dtype == want.dtype
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, [(k, got[k], want[k]) for k in bad[:5]]


def test_pinned_cases(fa, gpu_ctx):
    """The reference's own answers: StringUtilsTests.swift:10-66, NemotronBenchmarkTests.swift:15-120."""
    for a, b, d in R.LEVENSHTEIN_CASES:
        assert fa.levenshtein_distance(a, b, gpu_ctx) == d
    metrics, corpus = fa.wer_metrics_batch([(h.split(), r.split()) for r, h, _, _ in R.WER_CASES], gpu_ctx)
    assert [(m.insertions + m.deletions + m.substitutions, m.totalWords) for m in metrics] == [(e, w) for _, _, e, w in R.WER_CASES]
    for m, (r, h, _, _) in zip(metrics, R.WER_CASES):
        assert tuple(m) == R.wer_metrics(h.split(), r.split())
    assert (corpus.word_errors, corpus.ref_words) == (sum(c[2] for c in R.WER_CASES), sum(c[3] for c in R.WER_CASES))
    assert corpus.wer == float(corpus.word_errors) / float(corpus.ref_words)


def test_every_schedule_boundary_in_both_families(fa, gpu_ctx, shapes):
    pairs, want = shapes
    assert {len(r) for _, r in pairs} == set(W.NS) and {len(h) for h, _ in pairs} == set(W.MS)
    same(fa.edit_distance_batch(pairs, gpu_ctx), want)


def test_one_pair_per_call(fa, gpu_ctx, shapes):
    """A call of its own per three-panel pair and per class: the job list and the workspace start at zero."""
    pairs, want = shapes
    seen = set()
    for k, (hyp, ref) in enumerate(pairs):
        n = len(ref)
        route = (min(c for c in range(5) if n <= 64 << c or c == 4), (n + 1023) // 1024)   # strip class, panels
        if len(hyp) < 65 or n == 0 or route in seen:
            continue
        seen.add(route)
        same(fa.edit_distance_batch([(hyp, ref)], gpu_ctx), want[k:k + 1])


def test_mixed_call_answers_in_input_order(fa, gpu_ctx, shapes):
    """All classes, empty sides, m >> n and n >> m in shuffled order."""
    pairs, want = shapes
    order = np.random.default_rng(5).permutation(len(pairs))
    got = fa.edit_distance_batch([pairs[k] for k in order], gpu_ctx)
    same(got, want[order])
    lens = [(len(h), len(r)) for h, r in pairs]
    assert any(m == 0 for m, _ in lens) and any(n == 0 for _, n in lens) and (129, 1) in lens and (1, 2049) in lens


def test_no_pairs(fa, gpu_ctx):
    out = np.full(3, 7, np.int32)
    st = fa.lib().fa_edit_distance_batch(gpu_ctx.handle, None, None, None, None, 0, out.ctypes.data)
    assert st == 0 and out.tolist() == [7, 7, 7]
    assert fa.edit_distance_batch([], gpu_ctx).size == 0


def test_device_entry_gives_the_same_bytes(fa, gpu_ctx, shapes):
    import torch
    pairs, want = shapes
    hyp = np.concatenate([h for h, _ in pairs])
    ref = np.concatenate([r for _, r in pairs])
    hyp_range = np.concatenate([[0], np.cumsum([h.size for h, _ in pairs])])
    ref_range = np.concatenate([[0], np.cumsum([r.size for _, r in pairs])])
    got = fa.edit_distance_batch_dev(torch.from_numpy(hyp).cuda(), hyp_range, torch.from_numpy(ref).cuda(), ref_range, gpu_ctx)
    assert got.tobytes() == fa.edit_distance_batch(pairs, gpu_ctx).tobytes() == want.tobytes()


def test_repeated_call_on_one_context(fa, gpu_ctx, shapes):
    """The second call takes the first one's buffers back from the context's cache: no stale boundary column, in either order of sizes."""
    pairs, want = shapes
    multi = [k for k, (h, r) in enumerate(pairs) if len(r) > 1024 and len(h) > 0]
    first = fa.edit_distance_batch(pairs, gpu_ctx)
    part = fa.edit_distance_batch([pairs[k] for k in reversed(multi)], gpu_ctx)
    second = fa.edit_distance_batch(pairs, gpu_ctx)
    assert first.tobytes() == second.tobytes() == want.tobytes()
    same(part, want[list(reversed(multi))])


def bits(x):
    return struct.pack("<d", x)


def test_wer_and_cer_of_sentences(fa, gpu_ctx):
    """calculateWERAndCER behind the normalizer: words and characters of one call in one device call, the rates by their bits."""
    sentences = [("the quick brown fox jumps over the lazy dog", "the fast brown fox jumped over a lazy dog"),
                 ("hello world", "hello world"), ("hello big wide world", "hello world"), ("", "nothing was said"), ("something was said", ""),
                 ("", ""), ("a a a b a", "a b a a"), ("it s a long way to tipperary", "its a long long way to tip a rary"),
                 ("we will see you at ten past seven", "we ll see you at ten past eleven")]
    pairs = [(h, r) for r, h in sentences]
    got, corpus = fa.wer_and_cer_batch(pairs, gpu_ctx)
    want = [R.wer_and_cer(h, r) for h, r in pairs]
    for g, w in zip(got, want):
        assert tuple(g)[2:] == w[2:]
        assert bits(g.wer) == bits(w[0]) and bits(g.cer) == bits(w[1])
    char_errors = [R.edit_distance(list(h.replace(" ", "")), list(r.replace(" ", ""))).total for h, r in pairs]
    assert (corpus.word_errors, corpus.ref_words) == (sum(w[2] + w[3] + w[4] for w in want), sum(w[5] for w in want))
    assert (corpus.char_errors, corpus.ref_chars) == (sum(char_errors), sum(w[6] for w in want))
    assert bits(corpus.wer) == bits(float(corpus.word_errors) / float(corpus.ref_words))
    assert bits(corpus.cer) == bits(float(corpus.char_errors) / float(corpus.ref_chars))
