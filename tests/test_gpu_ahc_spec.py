"""The speculative round (csrc/ahc_round_body.h, SPEC): a launch that merges a pair also evaluates the merge most likely to follow, and the
next launch commits it when its records certify exactly that merge.  Whatever was committed, the dendrogram must be the one-merge round's bit for bit
(FA_AHC_SPEC=0 forces that round in the same process), and the commit counter (fa_debug_ahc_spec_hits) must show that the speculation did the work."""
import os
import sys

import numpy as np
import pytest

from conftest import speaker_mixture

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu


def _both_routes(fa, ctx, switch, x):
    """(Z, stats, hits) with the speculative round, then with the one-merge round."""
    out = []
    for value in (None, "0"):
        switch("FA_AHC_SPEC", value)
        st, z, stats = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=ctx, return_stats=True)
        assert st == 0, ctx.last_error()
        out.append((z, stats, ctx.ahc_spec_hits()))
    (z1, s1, h1), (z0, s0, h0) = out
    assert h0 == 0, "FA_AHC_SPEC=0 must not commit speculated merges"
    assert s1["merges"] == s0["merges"] == x.shape[0] - 1
    bad = np.nonzero((z1.view(np.uint64) != z0.view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, f"first differing row {bad[0]}: speculative {z1[bad[0]]} one-merge {z0[bad[0]]}"
    return z1, s1, h1, s0


def _session(hours, sigma=0.03):
    from e2e_inputs import e2e_session
    x = np.asarray(e2e_session(hours, sigma=sigma)["emb"], np.float64)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))


def test_session_8h_commits_most_merges(fa, gpu_ctx, switch):
    x = _session(8.0)
    _, s1, hits, s0 = _both_routes(fa, gpu_ctx, switch, x)
    merges = x.shape[0] - 1
    assert hits >= 0.95 * merges / 2, (hits, merges)           # a committed speculation is a second merge in the same launch
    assert s1["rounds"] < 0.6 * s0["rounds"], (s1["rounds"], s0["rounds"])


@pytest.mark.parametrize("hours,sigma", [(1.0, 0.03), (1.0, 0.041), (2.0, 0.03)])
def test_sessions(fa, gpu_ctx, switch, hours, sigma):
    x = _session(hours, sigma)
    _, _, hits, _ = _both_routes(fa, gpu_ctx, switch, x)
    assert hits > 0.4 * (x.shape[0] - 1)


@pytest.mark.parametrize("n,d", [(513, 16), (4097, 32), (20000, 64), (65535, 8), (65536, 8), (65537, 8)])
def test_iid_block_edges(fa, gpu_ctx, switch, n, d):
    x = np.random.default_rng(n + d).standard_normal((n, d))
    _, _, hits, _ = _both_routes(fa, gpu_ctx, switch, x)
    if n <= 65536:
        assert hits > 0
    else:
        assert hits == 0   # more than 65 536 slots: the one-merge round serves the problem


@pytest.mark.parametrize("n,d", [(20000, 256), (30000, 64)])
def test_speaker_mixtures(fa, gpu_ctx, switch, n, d):
    x = speaker_mixture(n, d, 64, 0.02, n + d)
    _both_routes(fa, gpu_ctx, switch, x)


def test_odd_dimension_keeps_the_one_merge_round(fa, gpu_ctx, switch):
    x = np.random.default_rng(7).standard_normal((3000, 33))
    _, _, hits, _ = _both_routes(fa, gpu_ctx, switch, x)
    assert hits == 0


def test_forced_handover(fa, gpu_ctx, switch):
    """AUTO's tie route hands the problem to the rounds (prob_adopt): no hypothesis survives the adoption, the dendrogram and the adopted state are the same."""
    n, d = 9000, 32
    rng = np.random.default_rng(3 * n + d)
    x = speaker_mixture(n, d, 12, 0.05, 3 * n + d)
    k = int(0.3 * n)
    x[rng.integers(0, n, k)] = x[rng.integers(0, n, k)]
    x = np.ascontiguousarray(x)
    switch("FA_AHC_RO_HANDOVER_AT", "3000")
    got = []
    for value in (None, "0"):
        switch("FA_AHC_SPEC", value)
        st, z, stats = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=gpu_ctx, return_stats=True)
        assert st == 0, gpu_ctx.last_error()
        got.append((z, stats, gpu_ctx.ahc_adopted(), gpu_ctx.ahc_spec_hits()))
    (z1, s1, a1, h1), (z0, s0, a0, h0) = got
    assert s1["handed_over_at"] == s0["handed_over_at"] > 0
    assert h1 > 0 and h0 == 0
    np.testing.assert_array_equal(z1, z0)
    for key in ("node", "d1", "nn", "nnnode", "e2"):
        np.testing.assert_array_equal(a1[key], a0[key])


def test_nan_input_fails_the_same_way(fa, gpu_ctx, switch):
    x = np.random.default_rng(11).standard_normal((3000, 16))
    x[1234, 5] = np.nan
    sts = []
    for value in (None, "0"):
        switch("FA_AHC_SPEC", value)
        st, _ = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=gpu_ctx)
        sts.append(st)
    assert sts[0] == sts[1]
