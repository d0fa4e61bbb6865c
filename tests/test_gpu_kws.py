"""fa_ctc_kws_spot_batch(_dev) and fa_ctc_kws_score_windows_dev on the device against the Python restatement of CtcDPAlgorithm
(tests/kws_restatement.py): utterance, keyword and frames as integers, scores by their 32 bits.  No tolerances.  The same file is run
on the poisoned-workspace library (make POISON=1).

Log-probs come from a coarse grid (multiples of -0.25, -0.0 included, a few denormals), so that stay / advance / skip ties, projection
ties and plateaus are frequent.  Shapes: one, two and four states per lane serve up to 31, 63 and 127 tokens (N = 31 | 32, 63 | 64, 127
are the edges); a wavefront has 8 frames of emissions in flight and walks 16 per trip of its loop (T = 1, 2, N - 1, N, N + 1, 70); a
workgroup takes 4 jobs and the grid is rounded up to 8 workgroups; a job reserves arena records 8 at a time."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kws_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
W = R.WILDCARD
NEG_INF = float("-inf")
_cache = {}


def grid(seed, shape):
    rng = np.random.default_rng(seed)
    x = (np.float32(-0.25) * rng.integers(0, 9, shape).astype(np.float32)).astype(np.float32)   # 0 * -0.25 is -0.0
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = np.float32(-1e-40)             # denormals
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = np.float32(-3e-45)
    return x


def want_spot(key, lp, valid, keywords, thresholds, merge, blank):
    """[(utterance, keyword, score bits, start, end)] of the restatement; the candidate lists are computed once per (key, merge)."""
    k = (key, merge)
    if k not in _cache:
        out = []
        for u in range(lp.shape[0]):
            rows = list(lp[u, :valid[u]])
            for i, kw in enumerate(keywords):
                for s, a, b in R.word_spot_multiple(rows, list(kw), thresholds[i], merge, blank):
                    out.append((u, i, R.bits(s), a, b))
        _cache[k] = out
    return _cache[k]


def records(dets):
    return [(int(d["utterance"]), int(d["keyword"]), R.bits(d["score"]), int(d["start_frame"]), int(d["end_frame"])) for d in dets]


def on_device(lp):
    import torch
    return torch.from_numpy(np.ascontiguousarray(lp)).cuda()


def spot(fa, ctx, lp, valid, keywords, thresholds, merge, blank, host=False, **kw):
    dets, counts = fa.spot_keywords_batch(lp if host else on_device(lp), keywords, blank_id=blank, merge_overlap=merge, valid_frames=valid,
                                          thresholds=thresholds, ctx=ctx, **kw)
    return records(dets), counts.tolist()


def pattern_keywords(V):
    """Keywords of one and two... 32 tokens over V columns (blank V - 1): the patterns the DP treats specially, then their thresholds."""
    rng = np.random.default_rng(V)
    kws = [[2], [1, 1], [3, 4, 3], [0, 1, 2], [5, 5, 5], [W, 2, 3], [2, 3, W], [1, W, W, 4], [W, W, W], [V], [1, V + 7, 2], [-2, 3], [3, -2],
           [], rng.integers(0, V - 1, 31).tolist(), rng.integers(0, V - 1, 32).tolist(), [0, 0, 1, 1, 0, 0], [2, W, 2], [4]]
    thr = [-100.0, -100.0, -1.0, -0.5, -2.0, -100.0, -0.75, -100.0, -100.0, NEG_INF, -100.0, NEG_INF, -3.0e38,
           -100.0, -100.0, -2.0, -0.1, -0.25, -0.0]
    return kws, np.asarray(thr, np.float32)


@pytest.mark.parametrize("V", [8, 37])
@pytest.mark.parametrize("merge", [False, True])
def test_patterns(fa, gpu_ctx, V, merge):
    lp = grid(V, (3, 70, V))
    valid = [70, 33, 0]
    kws, thr = pattern_keywords(V)
    want = want_spot(("patterns", V), lp, valid, kws, thr, merge, V - 1)
    got, counts = spot(fa, gpu_ctx, lp, valid, kws, thr, merge, V - 1)
    assert got == want
    assert counts == [sum(1 for w in want if w[0] == u) for u in range(3)] and counts[2] == 0
    assert [w[2:] for w in want if w[:2] == (0, 9)] == [(R.bits(R.NEG), 0, 0)]   # an id >= V under -inf: no candidate, the fallback's (-FLT_MAX, 0, 0)
    assert [w[2] for w in want if w[:2] == (0, 11)] == [R.bits(R.NEG / np.float32(2))]   # id -2 emits -FLT_MAX as well
    assert not any(w[1] == 13 for w in want)                                     # the empty keyword
    assert not any(w[1] == 16 for w in want) and any(w[1] == 2 for w in want)    # thresholds nothing reaches (the fallback fails), and reached ones
    if not merge:
        assert len(want) > len(want_spot(("patterns", V), lp, valid, kws, thr, True, V - 1))
        host, _ = spot(fa, gpu_ctx, lp, valid, kws, thr, merge, V - 1, host=True)        # the host-pointer entry: the same records
        assert host == want


@pytest.mark.parametrize("N", [1, 2, 3, 31, 32, 63, 64, 127])
def test_lengths_and_frame_counts(fa, gpu_ctx, N):
    """Utterances of 1, 2, N - 1, N, N + 1 and 70 valid frames, and one long enough for a keyword with repeats (2 N + 5)."""
    V = 8
    rng = np.random.default_rng(100 + N)
    valid = [1, 2, max(N - 1, 0), N, N + 1, 70, 2 * N + 5]
    lp = grid(200 + N, (len(valid), max(valid), V))
    distinct = [(i + N) % 7 for i in range(N)]   # no neighbour repeats: reachable in N frames
    kws = [distinct, rng.integers(0, 3, N).tolist()] + ([[1] * N] if N <= 32 else [])
    thr = np.asarray([-100.0, -1.0, -100.0][:len(kws)], np.float32)
    for merge in (False, True):
        want = want_spot(("lengths", N), lp, valid, kws, thr, merge, 7)
        got, _ = spot(fa, gpu_ctx, lp, valid, kws, thr, merge, 7)
        assert got == want
    assert any(w[:2] == (3, 0) for w in want) and not any(w[0] == 2 for w in want)   # T = N is walked, T = N - 1 is not


def strided(lp, row_stride, pad):
    """lp [B, T, V] laid out with row_stride floats per row and `pad` floats between matrices, NaN in every gap."""
    import torch
    B, T, V = lp.shape
    ms = T * row_stride + pad
    buf = np.full(B * ms, np.nan, np.float32)
    for b in range(B):
        for t in range(T):
            buf[b * ms + t * row_stride:b * ms + t * row_stride + V] = lp[b, t]
    d = torch.from_numpy(buf).cuda()
    return d, torch.as_strided(d, (B, T, V), (ms, row_stride, 1))


def test_production_vocabulary_strided(fa, gpu_ctx):
    V, blank = 1025, 1024
    lp = grid(7, (2, 24, V))
    kws = [[1023, 0, 512], [1024, 5], [1025, 5], [700, W, 701], [3] * 2, list(range(100, 112))]
    thr = np.asarray([-100.0] * len(kws), np.float32)
    keep, view = strided(lp, 1032, 40)
    want = want_spot("v1025", lp, [24, 19], kws, thr, True, blank)
    dets, _ = fa.spot_keywords_batch(view, kws, blank_id=blank, valid_frames=[24, 19], thresholds=thr, ctx=gpu_ctx)
    assert records(dets) == want and len(want) >= 6
    # a blank id outside the vocabulary emits 0
    want = want_spot("v1025_noblank", lp, [24, 19], kws, thr, True, 4000)
    dets, _ = fa.spot_keywords_batch(view, kws, blank_id=4000, valid_frames=[24, 19], thresholds=thr, ctx=gpu_ctx)
    assert records(dets) == want
    del keep


def test_threshold_rule_and_defaults(fa, gpu_ctx):
    """min_score goes through the per-term rule of spotKeywordsFromLogProbs; None is -15 for every term."""
    V = 8
    lp = grid(31, (2, 40, V))
    kws = [[1], [1, 2, 3], [1, 2, 3, 4, 5], [0, 1, 0, 1, 0, 1, 0, 1], []]
    d = on_device(lp)
    for base in (None, -1.25, -0.5):
        thr = [R.adjusted_threshold(base, len(k)) for k in kws]
        want = want_spot(("rule", base), lp, [40, 40], kws, thr, True, 7)
        dets, _ = fa.spot_keywords_batch(d, kws, min_score=base, blank_id=7, ctx=gpu_ctx)
        assert records(dets) == want
    assert R.bits(fa.adjusted_threshold(-0.5, 8)) == R.bits(R.adjusted_threshold(-0.5, 8)) == R.bits(-5.5)


def test_capacity_and_count(fa, gpu_ctx):
    L = fa._lib
    V = 8
    lp = grid(5, (2, 30, V))
    kws, thr = [[1], [2, 3], [4, W]], np.asarray([-100.0] * 3, np.float32)
    want = want_spot("capacity", lp, [30, 30], kws, thr, False, 7)
    total = len(want)
    assert total > 8
    d = on_device(lp)
    for cap in (0, 5, total, total + 3):
        dets, counts = np.zeros(max(cap, 1), fa.KWS_DETECTION_DTYPE), np.zeros(2, np.int64)
        dets["keyword"] = 99
        tok, off = fa.kws._pack_keywords(kws)
        n = C.c_int64(-1)
        st = fa.lib().fa_ctc_kws_spot_batch_dev(gpu_ctx.handle, C.c_void_p(d.data_ptr()), 2, 30, V, V, 30 * V, None, tok.ctypes.data, off.ctypes.data, 3,
                                                thr.ctypes.data, 7, 0, dets.ctypes.data, cap, C.byref(n), counts.ctypes.data)
        assert st == (L.OUTPUT_TOO_SMALL if cap < total else L.SUCCESS) and n.value == total and int(counts.sum()) == total
        assert records(dets[:min(cap, total)]) == want[:min(cap, total)]
        assert all(int(k) == 99 for k in dets["keyword"][min(cap, total):])
    n = C.c_int64(-1)   # a count query: no output buffer
    assert fa.lib().fa_ctc_kws_spot_batch_dev(gpu_ctx.handle, C.c_void_p(d.data_ptr()), 2, 30, V, V, 30 * V, None, tok.ctypes.data, off.ctypes.data, 3,
                                              thr.ctypes.data, 7, 0, None, 0, C.byref(n), None) == L.SUCCESS and n.value == total
    dets, _ = fa.spot_keywords_batch(d, kws, blank_id=7, merge_overlap=False, thresholds=thr, capacity=None, ctx=gpu_ctx)
    assert records(dets) == want


def test_argument_errors(fa, gpu_ctx):
    L = fa._lib
    d = on_device(grid(1, (1, 10, 8)))
    with pytest.raises(fa.FluidAudioHipError) as e:
        fa.spot_keywords_batch(d, [[1], [1] * 128], blank_id=7, ctx=gpu_ctx)
    assert e.value.status == L.INVALID_ARGUMENT
    dets, _ = fa.spot_keywords_batch(d, [[1], [1, 2] * 63 + [3]], blank_id=7, ctx=gpu_ctx)   # 127 tokens in 10 frames: nothing, no error
    assert all(int(k) == 0 for k in dets["keyword"])
    with pytest.raises(fa.FluidAudioHipError) as e:
        fa.score_windows(d, [[1]], [(0, 1, 0, 5)], blank_id=7, ctx=gpu_ctx)
    assert e.value.status == L.INVALID_ARGUMENT
    with pytest.raises(fa.FluidAudioHipError) as e:
        fa.score_windows(d, [[1]], [(1, 0, 0, 5)], blank_id=7, ctx=gpu_ctx)
    assert e.value.status == L.INVALID_ARGUMENT


def test_small_arena_walks_overflowed_jobs_again(fa, gpu_ctx, switch):
    """FA_KWS_ARENA shrinks the candidate arena to a few chunks: most jobs of the first pass report an overflow and are walked again by
    passes sized to fit; the records and their order are those of the roomy arena."""
    V = 8
    lp = grid(77, (3, 70, V))
    kws = [[1], [2], [3, 4], [5, W], [0, 1, 2], [6] * 2, np.random.default_rng(3).integers(0, 7, 40).tolist(), [4, 4]]
    thr = np.asarray([-100.0] * len(kws), np.float32)
    want = want_spot("arena", lp, [70, 51, 9], kws, thr, False, 7)
    assert len(want) > 200
    for arena in (0, 64, 200):
        switch("FA_KWS_ARENA", arena)
        got, _ = spot(fa, gpu_ctx, lp, [70, 51, 9], kws, thr, False, 7)
        assert got == want
    switch("FA_KWS_ARENA", None)
    got, _ = spot(fa, gpu_ctx, lp, [70, 51, 9], kws, thr, False, 7)
    assert got == want


def test_constrained_windows(fa, gpu_ctx):
    V = 8
    lp = grid(13, (2, 70, V))
    valid = [70, 44]
    rng = np.random.default_rng(9)
    kws = [[1], [2, 3], [1, 1, 1], [W, W], [3, W, 4], [9, 1], [], rng.integers(0, 7, 31).tolist(), rng.integers(0, 7, 33).tolist(), rng.integers(0, 7, 64).tolist()]
    spans = [(-5, 100), (0, 70), (10, 30), (30, 10), (12, 12), (69, 70), (43, 46), (60, 200), (-9, 2), (5, 8), (0, 44), (3, 40), (2, 68)]
    windows = [(u, k, a, b) for u in range(2) for k in range(len(kws)) for a, b in spans]
    got = fa.score_windows(on_device(lp), kws, windows, blank_id=7, valid_frames=valid, ctx=gpu_ctx)
    assert len(got) == len(windows)
    seen = set()
    for g, (u, k, a, b) in zip(got, windows):
        s, st, en = R.word_spot_constrained(list(lp[u, :valid[u]]), list(kws[k]), a, b, 7)
        assert (int(g["utterance"]), int(g["keyword"]), R.bits(g["score"]), int(g["start_frame"]), int(g["end_frame"])) == (u, k, R.bits(s), st, en), (u, k, a, b)
        seen.add("inf" if np.isneginf(s) else ("neg" if R.bits(s) == R.bits(R.NEG / np.float32(max(1, R.non_wildcard_count(kws[k])))) else "score"))
    assert seen == {"inf", "neg", "score"}
    # [a, a, a] in a 3-frame window: the row's zeroes, not inherited frames
    g = fa.score_windows(on_device(lp), [[1, 1, 1]], [(0, 0, 20, 23)], blank_id=7, ctx=gpu_ctx)[0]
    assert (R.bits(g["score"]), int(g["start_frame"]), int(g["end_frame"])) == (0xFEAAAAAA, 20, 20)


def test_hand_cases(fa, gpu_ctx):
    """The projection tie and the plateau of tests/test_kws_cpu.py on the device."""
    tie = np.asarray([[[-1.0, -2.0], [-1.0, 0.0]]], np.float32)
    dets, _ = fa.spot_keywords_batch(on_device(tie), [[0]], blank_id=1, merge_overlap=False, thresholds=[-100.0], ctx=gpu_ctx)
    assert records(dets) == [(0, 0, R.bits(-1.0), 1, 2)]
    flat = np.tile(np.asarray([-1.0, 0.0], np.float32), (1, 4, 1))
    for merge in (False, True):
        dets, _ = fa.spot_keywords_batch(on_device(flat), [[0]], blank_id=1, merge_overlap=merge, thresholds=[-1.0], ctx=gpu_ctx)
        assert records(dets) == [(0, 0, R.bits(-1.0), 3, 4)]
    dets, _ = fa.spot_keywords_batch(on_device(flat), [[0]], blank_id=1, thresholds=[-0.5], ctx=gpu_ctx)
    assert len(dets) == 0
