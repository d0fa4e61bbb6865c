"""The two-merge path of the speculative round (csrc/ahc_round_body.h, SPEC): a launch that commits the speculated merge B executes the merge C
that follows it from B's own values (size and scratch row of the first round trip) and the partner's (requested raw, sorted into slot order where they are first
used), and issues B's stores next to C's.  The rule is the one of tests/test_gpu_ahc_spec.py: the dendrogram equals the one-merge round's (FA_AHC_SPEC=0) bit for
bit, and up to 3 000 points also the reference's."""
import functools

import numpy as np
import pytest

from conftest import speaker_mixture

pytestmark = pytest.mark.gpu

MIXTURES = {513: (513, 8, 3, 0.05, 521), 769: (769, 16, 3, 0.05, 785)}   # the smallest multi-workgroup shapes: 3 and 4 blocks, one record per lane


@functools.lru_cache(maxsize=None)
def _mixture(n, reverse):
    x = speaker_mixture(*MIXTURES[n])
    x = np.ascontiguousarray(x[::-1] if reverse else x)
    x.setflags(write=False)
    return x


def _both_routes(fa, ctx, switch, x):
    """(Z, stats, hits) of the speculative round after checking it against the one-merge round."""
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
    return z1, s1, h1


def _chained_by_slot_order(z):
    """Merges that involve the cluster the previous merge made, split by where the partner's slot lies: (below, above) the cluster's.  A cluster lives in the
    slot of its lowest member, so `above` is the chained merge in which the cluster keeps its slot and `below` the one in which it moves to the partner's."""
    n = z.shape[0] + 1
    low = np.empty(2 * n - 1, np.int64)
    low[:n] = np.arange(n)
    below = above = 0
    for i in range(n - 1):
        a, b = int(z[i, 0]), int(z[i, 1])
        low[n + i] = min(low[a], low[b])
        if i > 0 and (n + i - 1) in (a, b):
            partner = b if a == n + i - 1 else a
            if low[partner] < low[n + i - 1]:
                below += 1
            else:
                above += 1
    return below, above


@pytest.mark.parametrize("reverse", [False, True], ids=["given", "reversed"])
@pytest.mark.parametrize("n", sorted(MIXTURES))
def test_both_slot_orders_of_the_chained_merge(fa, gpu_ctx, switch, oracle_mod, n, reverse):
    x = _mixture(n, reverse)
    sr, zr = oracle_mod.linkage_ref(x)
    assert sr == 0
    below, above = _chained_by_slot_order(zr)
    print(f"n {n} reversed {reverse}: chained merges with the partner below / above the cluster's slot: {below} / {above} of {n - 1}")
    assert below >= 25 and above >= 25, (below, above)            # a condition on the input, not a measurement: both selects of the chained merge are exercised
    z1, _, hits = _both_routes(fa, gpu_ctx, switch, x)
    bad = np.nonzero((z1.view(np.uint64) != zr.view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, f"first row differing from the reference {bad[0]}: {z1[bad[0]]} reference {zr[bad[0]]}"
    # only a fifth to a third of these merges chain: the two-merge path ran, and so did the paths around it (a miss, B alone, re-scan rounds)
    assert 0 < hits < (n - 1) / 2, (hits, n - 1)


def test_three_records_per_lane(fa, gpu_ctx, switch):
    """129 blocks: the smallest problem of the instance the 8 h session runs (three block records per lane)."""
    x = np.random.default_rng(32777).standard_normal((32769, 8))
    _, _, hits = _both_routes(fa, gpu_ctx, switch, x)
    assert hits > 0


def test_last_merges_with_a_commit_pending(fa, gpu_ctx, switch, oracle_mod):
    """The run ends (`done`) in a launch whose predecessor speculated: every row is written, the last two included, and the count is right."""
    n = 513
    x = np.random.default_rng(521).standard_normal((n, 8))
    z1, s1, hits = _both_routes(fa, gpu_ctx, switch, x)
    sr, zr = oracle_mod.linkage_ref(x)
    assert sr == 0 and s1["merges"] == n - 1 and hits > 0
    np.testing.assert_array_equal(z1[-2:].view(np.uint64), zr[-2:].view(np.uint64))
    np.testing.assert_array_equal(z1.view(np.uint64), zr.view(np.uint64))
