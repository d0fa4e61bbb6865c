"""The drive loop of the round replays (csrc/ahc_launch.h: drive_rounds; the plan: csrc/ahc_route.h, walked on the CPU by tests/test_ahc_drive_plan.py):
a replay is enqueued before the state of the one in front of it has been read while that one cannot finish the problem, and the last replays are shorter
ones.  FA_AHC_SYNC_DRIVE forces the drive from before: one replay of the full length at a time.  Both drives must give the same dendrogram bit for bit and
the same statistics, and that dendrogram is the reference build's (oracle/_ref)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 32                      # even: the speculative round is eligible
COUNTS = ("merges", "rounds", "rescans", "windows", "exact_fallback", "reference_order", "handed_over_at")


def _iid(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal((n, D)))


def _flat(n):
    """n iid rows whose last coordinate is 0: points far out along that coordinate stay away from them."""
    x = _iid(n, 5 * (n + 4))
    x[:, D - 1] = 0.0
    return x


@pytest.fixture(scope="module")
def refs(oracle_mod):
    cache = {}

    def ref(key, x):
        if key not in cache:
            st, z = oracle_mod.linkage_ref(x)
            assert st == 0
            z.setflags(write=False)
            cache[key] = z
        return cache[key]
    return ref


def _both_drives(fa, ctx, switch, x):
    """[(status, Z, counts, error text)] with the look-ahead drive, then with the synchronous one."""
    out = []
    for value in (None, "1"):
        switch("FA_AHC_SYNC_DRIVE", value)
        st, z, stats = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=ctx, return_stats=True)
        out.append((st, z, {k: stats[k] for k in COUNTS if k in stats} if stats else None, ctx.last_error() if st else ""))
    switch("FA_AHC_SYNC_DRIVE", None)
    return out


def _same(ahead, sync, zr):
    assert ahead[0] == sync[0] == 0, (ahead[3], sync[3])
    bad = np.nonzero((ahead[1].view(np.uint64) != sync[1].view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, f"first differing row {bad[0]}: look-ahead {ahead[1][bad[0]]} synchronous {sync[1][bad[0]]}"
    assert ahead[2] == sync[2], (ahead[2], sync[2])
    np.testing.assert_array_equal(ahead[1], zr)


@pytest.mark.parametrize("n", [3000, 1100])   # three replays of the full length: look-ahead and ladder both act; the bound turns synchronous inside the second
def test_tie_free_rows(fa, gpu_ctx, switch, refs, n):
    x = _iid(n, n)
    ahead, sync = _both_drives(fa, gpu_ctx, switch, x)
    _same(ahead, sync, refs(("iid", n), x))
    assert ahead[2]["merges"] == n - 1 and ahead[2]["reference_order"] == 0 and ahead[2]["exact_fallback"] == 0
    assert ahead[2]["rounds"] >= (n - 1) / 2                                # a round commits two merges at most: what the plan's bound rests on


def test_a_replay_queued_behind_a_halt(fa, gpu_ctx, switch, oracle_mod):
    """Two far-apart pairs at EXACTLY the same distance that the reference merges after more merges than the first replay can commit (2 x 512): the rounds halt
    on the tie inside a later replay, with another one queued behind it (tests/test_ahc_drive_plan.py walks the plan of N = 2 500: the second replay is
    enqueued before the first state is read, the third before the second, whatever the device did)."""
    n = 2500
    x = _flat(n - 4)
    _, z_data = oracle_mod.linkage_ref(x)
    delta = np.round(z_data[1500, 2] * 64) / 64                             # a height the data reaches at about row 1 500, exactly representable with its square
    extra = np.zeros((4, D))
    extra[:, D - 1] = [50.0, 50.0, -50.0, -50.0]
    extra[1, 0] = extra[3, 0] = delta                                       # |e0 - e1|^2 = |e2 - e3|^2 = delta^2, exactly
    x = np.ascontiguousarray(np.concatenate([x, extra]))
    sr, zr = oracle_mod.linkage_ref(x)
    at = np.nonzero(zr[:, 2] == delta)[0]
    assert sr == 0 and at.size == 2 and at[1] == at[0] + 1 and 1100 < at[0] < 2300, at   # behind the first replay, in front of the end
    ahead, sync = _both_drives(fa, gpu_ctx, switch, x)
    _same(ahead, sync, zr)
    assert ahead[2]["exact_fallback"] == 1 and ahead[2]["reference_order"] == 1, ahead[2]


@pytest.mark.parametrize("name,value", [("FA_AHC_SPEC", "0"), ("FA_AHC_CPT", "2")])
def test_one_merge_round_and_two_slots_per_thread(fa, gpu_ctx, switch, refs, name, value):
    x = _iid(3000, 3000)
    switch(name, value)
    ahead, sync = _both_drives(fa, gpu_ctx, switch, x)
    _same(ahead, sync, refs(("iid", 3000), x))
    assert ahead[2]["rounds"] >= 2999                                       # one merge per round: the plan counts one


def test_a_non_finite_row_fails_the_same_way(fa, gpu_ctx, switch):
    x = _iid(3000, 11)
    x[1234, 5] = np.nan
    ahead, sync = _both_drives(fa, gpu_ctx, switch, x)
    assert ahead[0] == sync[0] != 0
    assert ahead[3] == sync[3] != ""


def test_the_cached_ladder_is_renewed_and_reused(fa, gpu_ctx, switch, refs):
    """Two calls of different N on one context, then the first N again."""
    for n in (3000, 1100, 3000, 3000):
        x = _iid(n, n)
        st, z = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=gpu_ctx)
        assert st == 0, gpu_ctx.last_error()
        np.testing.assert_array_equal(z, refs(("iid", n), x))
