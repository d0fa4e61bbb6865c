"""AUTO's tie route hands the problem back to the filter-based rounds once the ties have stopped (round 6; csrc/ahc_rom.hip, prob_adopt in csrc/ahc_rounds_host.hip).
Ties at distance 0 only (duplicated rows): the rows behind the last tie have a unique closest pair, so the rounds produce what the reference's heap produces.
Whatever happens — handed over, handed over and a later tie met (everything again in reference order), never handed over — the dendrogram is the reference
build's (oracle/_ref) row for row."""
import numpy as np
import pytest

from conftest import speaker_mixture

pytestmark = pytest.mark.gpu


def _duplicated(n, d, dup, seed):
    rng = np.random.default_rng(seed)
    x = speaker_mixture(n, d, 12, 0.05, seed)
    k = int(dup * n)
    x[rng.integers(0, n, k)] = x[rng.integers(0, n, k)]
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("n,d,dup", [(9000, 32, 0.3), (12000, 16, 0.1)])
def test_duplicates_are_handed_over_and_equal_the_reference(fa, gpu_ctx, oracle_mod, switch, n, d, dup):
    x = _duplicated(n, d, dup, 3 * n + d)
    sr, zr = oracle_mod.linkage_ref(x)
    st, z, stats = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=gpu_ctx, return_stats=True)
    assert st == sr == 0, gpu_ctx.last_error()
    assert stats["reference_order"] == 1 and 0 < stats["handed_over_at"] < n - 1 - 4096, stats      # the tie route was taken, and left again
    assert int((zr[: stats["handed_over_at"], 2] == 0).sum()) > 0                                      # (the ties were duplicates)
    bad = np.nonzero((z != zr).any(axis=1))[0]
    assert bad.size == 0, f"first differing row {bad[0]} (handed over at {stats['handed_over_at']}): device {z[bad[0]]} reference {zr[bad[0]]}"
    # the same problem with the hand-over switched off, and in the mode that never hands over: the same rows
    switch("FA_AHC_RO_NO_HANDOVER", "1")
    st2, z2, stats2 = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=gpu_ctx, return_stats=True)
    assert st2 == 0 and stats2["handed_over_at"] == 0 and stats2["reference_order"] == 1
    np.testing.assert_array_equal(z2, zr)
    switch("FA_AHC_RO_NO_HANDOVER", None)
    st3, z3, stats3 = fa.linkage(x, mode=fa.AHC_MODE_REFERENCE_ORDER, ctx=gpu_ctx, return_stats=True)
    assert st3 == 0 and stats3["handed_over_at"] == 0
    np.testing.assert_array_equal(z3, zr)


def test_a_tie_behind_the_hand_over_sends_the_problem_back(fa, gpu_ctx, oracle_mod):
    """Duplicates first, then — long after the ties have stopped — two far-away pairs at EXACTLY the same distance: the rounds that adopted the problem halt on the
    exact tie at the minimum, and the whole problem runs again in reference order (handed_over_at == -1)."""
    n, d = 9000, 32
    x = _duplicated(n, d, 0.25, 77)
    x = np.concatenate([x, np.zeros((n, 1))], axis=1)                      # one more coordinate keeps the four extra points away from the data
    extra = np.zeros((4, d + 1))
    extra[:, d] = [50.0, 50.0, -50.0, -50.0]
    extra[1, 0] = 0.5                                                      # |e0 - e1|^2 = |e2 - e3|^2 = 0.25, exactly
    extra[3, 0] = 0.5
    x = np.ascontiguousarray(np.concatenate([x, extra]))
    sr, zr = oracle_mod.linkage_ref(x)
    at = np.nonzero(zr[:, 2] == 0.5)[0]
    assert at.size == 2 and at[1] == at[0] + 1 and at[0] > 6000, at        # the tied pairs merge one after the other, late
    st, z, stats = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=gpu_ctx, return_stats=True)
    assert st == sr == 0, gpu_ctx.last_error()
    assert stats["reference_order"] == 1 and stats["handed_over_at"] == -1, stats
    np.testing.assert_array_equal(z, zr)


def test_batch_problems_on_the_tie_route_hand_over_too(fa, gpu_ctx, oracle_mod):
    probs = [_duplicated(9000, 16, 0.2, 5), speaker_mixture(3000, 16, 6, 0.05, 8), _duplicated(12000, 16, 0.2, 6)]
    st, zs, stats = fa.linkage_batch(probs, ctx=gpu_ctx, return_stats=True)
    assert st == [0, 0, 0]
    for x, z in zip(probs, zs):
        np.testing.assert_array_equal(z, oracle_mod.linkage_ref(x)[1])
    assert stats[0]["handed_over_at"] > 0 and stats[2]["handed_over_at"] > 0 and stats[1]["reference_order"] == 0


# ---- the hand-over at rows a test chooses, and the state the rounds adopt there
# FA_AHC_RO_HANDOVER_AT puts the hand-over at the first replay boundary with >= row rows done, FA_AHC_RO_REPLAY_PAIRS=4 makes those boundaries 4 launch pairs
# apart (one row or one re-scan each), so the sweep meets both pending kinds: a merge decided but not yet applied (ROM_NEW: the extra scan writes the new node's
# row, not its column) and a re-scan (ROM_RESCAN).  fa_debug_ahc_adopted returns what prob_adopt built; it is held against exact fp64 centroid distances.
ROM_NEW = 0   # RomDev::kind (ahc_rom.hip); 1: a re-scan pending


def _iid_duplicated(n, d, dup, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    k = int(dup * n)
    x[rng.integers(0, n, k)] = x[rng.integers(0, n, k)]
    return np.ascontiguousarray(x)


SMALL = {"mixture_dup30": lambda: _duplicated(2500, 16, 0.3, 41), "iid_dup10": lambda: _iid_duplicated(3000, 32, 0.1, 42)}


def _set(fa, name, value):
    assert fa.lib().fa_debug_set_switch(name.encode(), None if value is None else str(value).encode()) == 0, name


def _zero_rows(zr):
    """Rows of height 0 (the duplicates): all of them lead the dendrogram — the first row a hand-over can take without meeting a tie."""
    zero = np.nonzero(zr[:, 2] == 0)[0]
    assert zero.size > 0 and np.array_equal(zero, np.arange(zero.size)), "the ties are not the leading rows"
    return int(zero.size)


def _sweep_rows(first, n):
    return sorted({first, *range(first + 1, first + 13), *np.linspace(first + 20, n - 10, 11).astype(int).tolist()})


@pytest.fixture(scope="module")
def sweeps(fa, gpu_ctx, oracle_mod):
    """Every input, forced to hand over at ~24 rows: (x, reference dendrogram, [(asked row, status, Z, stats, adopted state)])."""
    out = {}
    _set(fa, "FA_AHC_RO_REPLAY_PAIRS", 4)
    try:
        for name, make in SMALL.items():
            x = make()
            sr, zr = oracle_mod.linkage_ref(x)
            assert sr == 0
            runs = []
            for row in _sweep_rows(_zero_rows(zr), len(x)):
                _set(fa, "FA_AHC_RO_HANDOVER_AT", row)
                st, z, stats = fa.linkage(x, mode=fa.AHC_MODE_AUTO, ctx=gpu_ctx, return_stats=True)
                runs.append((row, st, z, stats, gpu_ctx.ahc_adopted(), gpu_ctx.last_error() if st else ""))
            out[name] = (x, zr, runs)
    finally:
        _set(fa, "FA_AHC_RO_HANDOVER_AT", None)
        _set(fa, "FA_AHC_RO_REPLAY_PAIRS", None)
    return out


def _node_centroids(x, zr):
    """Centroid of every node of the reference dendrogram (ids 0 .. 2N-2): member sums in extended precision, one rounding to fp64."""
    n = len(x)
    sums = np.zeros((2 * n - 1, x.shape[1]), np.longdouble)
    sums[:n] = x
    size = np.ones(2 * n - 1)
    for r, (a, b) in enumerate(zr[:, :2].astype(np.int64).tolist()):
        sums[n + r] = sums[a] + sums[b]
        size[n + r] = size[a] + size[b]
    return (sums / size[:, None].astype(np.longdouble)).astype(np.float64)


def _sq_distances(c):
    """Squared Euclidean distances between the rows of c in fp64, from the coordinate differences (the matrix holds squared distances); +inf on the diagonal."""
    ct = np.ascontiguousarray(c.T)
    D = np.zeros((len(c), len(c)))
    diff = np.empty_like(D)
    for k in range(len(ct)):
        np.subtract(ct[k][:, None], ct[k][None, :], out=diff)
        np.multiply(diff, diff, out=diff)
        D += diff
    np.fill_diagonal(D, np.inf)
    return D


def _check_adopted(x, zr, cent, a):
    """The adopted row records against the exact distances between the live clusters after the reference's first a["row"] merges (the rows before the
    hand-over are the reference's, so node ids agree): a list of violations, and whether the newest node — on a ROM_NEW boundary the merge the extra scan
    applied — is the true nearest neighbour of another live row (a row whose d1 / nn / e2 then come from the newest node's column)."""
    n, row, eps = len(x), a["row"], a["eps"]
    merged = np.zeros(n + row, bool)
    merged[zr[:row, :2].astype(np.int64).ravel()] = True
    live = np.nonzero(~merged)[0]
    slots = np.nonzero(a["node"] != np.iinfo(np.int32).max)[0]
    if not np.array_equal(np.sort(a["node"][slots]), live):
        return [f"live node ids differ from the reference's after {row} rows"], False
    T = _sq_distances(cent[a["node"][slots]])                # T[k]: exact distances of slot slots[k] to the other live slots, in slot order
    idx = np.full(len(a["node"]), -1)
    idx[slots] = np.arange(len(slots))
    node, d1, nn, nnnode, e2 = (a[k][slots] for k in ("node", "d1", "nn", "nnnode", "e2"))
    mt, arg = T.min(axis=1), T.argmin(axis=1)
    at = np.where((nn >= 0) & (nn < len(idx)), idx[np.clip(nn, 0, len(idx) - 1)], -1)
    k = np.arange(len(slots))
    t_nn = np.where(at >= 0, T[k, np.maximum(at, 0)], np.inf)
    T[k, np.maximum(at, 0)] = np.where(at >= 0, np.inf, T[k, np.maximum(at, 0)])
    rest = T.min(axis=1)                                     # smallest exact distance other than column nn
    nn_node = np.where(at >= 0, node[np.maximum(at, 0)], -1)
    bad = []
    for q in np.nonzero(~(np.abs(d1 - mt) <= eps))[0]:
        bad.append(f"slot {slots[q]} node {node[q]}: d1 {d1[q]!r} exact minimum {mt[q]!r} ({abs(d1[q] - mt[q]) / eps:.3g} eps)")
    for q in np.nonzero(~((at >= 0) & (t_nn <= mt + 2 * eps) & (nnnode == nn_node)))[0]:
        bad.append(f"slot {slots[q]} node {node[q]}: neighbour slot {nn[q]} (node {nnnode[q]}, holds {nn_node[q]}) at {t_nn[q]!r}, exact minimum {mt[q]!r} at node "
                   f"{node[arg[q]]}")
    for q in np.nonzero(~(np.abs(e2 - rest) <= eps))[0]:
        bad.append(f"slot {slots[q]} node {node[q]}: e2 {e2[q]!r} exact second minimum {rest[q]!r} ({abs(e2[q] - rest[q]) / eps:.3g} eps)")
    newest = n + row - 1
    return bad, bool(((node[arg] == newest) & (node != newest)).any())


@pytest.fixture(scope="module")
def adopted_checks(sweeps):
    """_check_adopted of every boundary the forced hand-overs landed on: {input: [(adopted state, violations, new node is a nearest neighbour)]}
    (requested rows that land on the same boundary are checked once when their states are equal)."""
    out = {}
    for name, (x, zr, runs) in sweeps.items():
        cent = _node_centroids(x, zr)
        seen = {}
        out[name] = []
        for _, _, _, _, a, _ in runs:
            if a is None:
                continue
            if a["row"] in seen and all(np.array_equal(a[k], seen[a["row"]][k]) for k in ("node", "d1", "nn", "nnnode", "e2")):
                continue
            seen[a["row"]] = a
            out[name].append((a, *_check_adopted(x, zr, cent, a)))
    return out


@pytest.mark.parametrize("name", list(SMALL))
def test_forced_hand_over_equals_the_reference_at_every_row(sweeps, name):
    x, zr, runs = sweeps[name]
    bad = []
    for row, st, z, stats, a, err in runs:
        if st != 0:
            bad.append(f"row {row}: status {st} ({err})")
        elif a is None or stats["handed_over_at"] != a["row"] or not 0 < a["row"] or not row <= a["row"] <= row + 3 or stats["reference_order"] != 1:
            bad.append(f"row {row}: handed_over_at {stats['handed_over_at']}, adopted at {None if a is None else a['row']}")
        elif not np.array_equal(z, zr):
            r = int(np.nonzero((z != zr).any(axis=1))[0][0])
            bad.append(f"row {row} (handed over at {a['row']}): first differing row {r}: device {z[r].tolist()} reference {zr[r].tolist()}")
    assert not bad, f"{len(bad)} of {len(runs)} forced hand-overs:\n" + "\n".join(bad)


@pytest.mark.parametrize("name", list(SMALL))
def test_adopted_state_equals_exact_centroid_distances(sweeps, adopted_checks, name):
    missing = [row for row, _, _, _, a, _ in sweeps[name][2] if a is None]
    assert not missing, f"forced hand-overs at rows {missing} recorded no adopted state"
    checks = adopted_checks[name]
    bad = []
    for a, v, _ in checks:
        bad += [f"hand-over at {a['row']} (pending {('new row', 're-scan')[a['kind']]}): {m}" for m in v[:5]] + ([f"  ... {len(v) - 5} more"] if len(v) > 5 else [])
    assert not bad, "\n".join(bad)


def test_the_sweep_adopts_a_pending_merge_whose_new_node_is_a_nearest_neighbour(adopted_checks):
    """What makes the state check bite: a hand-over with ROM_NEW pending, where some other live row's true nearest neighbour is the node that merge creates
    (its column copies are the ones the extra scan does not write)."""
    kinds = sorted({a["kind"] for checks in adopted_checks.values() for a, _, _ in checks})   # (shown with -rP)
    hits = [(name, a["row"]) for name, checks in adopted_checks.items() for a, _, hit in checks if a["kind"] == ROM_NEW and hit]
    print(f"pending kinds met: {kinds}; ROM_NEW boundaries whose new node is a nearest neighbour: {hits}")
    assert kinds == [ROM_NEW, ROM_NEW + 1], f"the sweep met only the pending kinds {kinds}"
    assert hits, "no forced hand-over had a pending merge whose new node is another row's nearest neighbour"


def test_forced_hand_over_through_the_batch_entry(fa, gpu_ctx, oracle_mod, switch):
    xa, xc = SMALL["mixture_dup30"](), _duplicated(2000, 16, 0.2, 43)
    probs = [xa, speaker_mixture(1500, 16, 6, 0.05, 44), xc]
    refs = [oracle_mod.linkage_ref(x)[1] for x in probs]
    row = max(_zero_rows(refs[0]), _zero_rows(refs[2])) + 37
    switch("FA_AHC_RO_REPLAY_PAIRS", 4)
    switch("FA_AHC_RO_HANDOVER_AT", row)
    st, zs, stats = fa.linkage_batch(probs, ctx=gpu_ctx, return_stats=True)
    assert st == [0, 0, 0], gpu_ctx.last_error()
    assert stats[1]["reference_order"] == 0 and stats[1]["handed_over_at"] == 0, stats[1]
    for k in (0, 2):
        assert stats[k]["reference_order"] == 1 and row <= stats[k]["handed_over_at"] <= row + 3, (k, stats[k])
        st1, z1, s1 = fa.linkage(probs[k], ctx=gpu_ctx, return_stats=True)
        assert st1 == 0 and s1["handed_over_at"] == stats[k]["handed_over_at"], (k, s1)
        np.testing.assert_array_equal(zs[k], z1)
    for z, zr in zip(zs, refs):
        np.testing.assert_array_equal(z, zr)


def test_replay_pairs_must_be_a_multiple_of_four(fa, gpu_ctx, oracle_mod, switch):
    x = _duplicated(600, 16, 0.3, 45)
    for bad in ("6", "0", "-4", "four"):
        switch("FA_AHC_RO_REPLAY_PAIRS", bad)
        st, _ = fa.linkage(x, mode=fa.AHC_MODE_REFERENCE_ORDER, ctx=gpu_ctx)
        assert st == 1, (bad, st)
    switch("FA_AHC_RO_REPLAY_PAIRS", 8)
    st, z = fa.linkage(x, mode=fa.AHC_MODE_REFERENCE_ORDER, ctx=gpu_ctx)
    assert st == 0
    np.testing.assert_array_equal(z, oracle_mod.linkage_ref(x)[1])
