"""The host decisions of the k-means fallback (csrc/kmeans_draws.h: the seeded generator with the Swift-stdlib draws, the shuffle whose
first k indices seed a run, the pre-drawn re-seeding picks, the guards of clusterWithCentroids, SpeakerCountConstraints.resolve) walked
on the CPU by tests/cpu/kmeans_draws.cpp against the oracle's generator and the cases of tests/test_oracle_kmeans.py.  The program is
stand-alone, reads its cases from stdin and is built with the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PICKS = 1024


@pytest.fixture(scope="module")
def draws(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kmeans_draws") / "kmeans_draws")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "kmeans_draws.cpp"), "-o", exe], check=True)
    return exe


def run(draws, lines):
    r = subprocess.run([draws], input="".join(" ".join(str(w) for w in ln) + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def test_next_and_below_are_the_oracles(draws, oracle_mod):
    bounds = (1, 2, 3, 10, 43200, 2 ** 31 + 11, 2 ** 63 + 5, 2 ** 64 - 1)         # the bounds of tests/test_host_logic.py
    got = run(draws, [("next", 1234, 50)] + [("below", 1234, b, 50) for b in bounds])
    rng = oracle_mod.SeededRNG(1234)
    assert [int(x) for x in got[0].split()] == [rng.next() for _ in range(50)]
    for b, line in zip(bounds, got[1:]):
        rng = oracle_mod.SeededRNG(1234)
        assert [int(x) for x in line.split()] == [rng.next_upper_bound(b) for _ in range(50)]
    assert run(draws, [("next", 0, 1)]) == ["1442695040888963407"]               # state * a + c with state 0


def restated_draws(rng, n, k):
    """shuffle(using:) of the Swift standard library over 0 ... n - 1, then the picks a run may use: randomElement is below(n)."""
    idx, amount, cur = list(range(n)), n, 0
    while amount > 1:
        j = rng.next_upper_bound(amount)
        amount -= 1
        idx[cur], idx[cur + j] = idx[cur + j], idx[cur]
        cur += 1
    return idx[:k], [rng.next_upper_bound(n) for _ in range(PICKS)]


def test_the_seeding_indices_and_the_picks_follow_the_shuffle(draws, oracle_mod):
    cases = [(seed, n, k) for n in (2, 3, 6, 1000) for k in (1, 2, 3) if k <= n for seed in (0, 7, 42)]
    for (seed, n, k), line in zip(cases, run(draws, [("draws",) + c for c in cases])):
        first, picks = ([int(x) for x in part.split()] for part in line.split("|"))
        want = restated_draws(oracle_mod.SeededRNG(seed), n, k)
        assert (first, picks) == want, (seed, n, k)
        assert len(set(first)) == k and all(0 <= p < n for p in picks) and len(picks) == PICKS
    # the whole walk, against the oracle's own shuffle
    for seed, n in ((3, 50), (42, 1000)):
        line = run(draws, [("draws", seed, n, n)])[0]
        assert [int(x) for x in line.split("|")[0].split()] == oracle_mod.SeededRNG(seed).shuffled_indices(n).tolist()


def guards(draws, n, d, k):
    head, labels, cen = (part.split() for part in run(draws, [("guards", n, d, k)])[0].split("|"))
    return int(head[0]), int(head[1]), [int(x) for x in labels], [float(x) for x in cen]


def test_guards(draws):
    """The cases of tests/test_oracle_kmeans.py (KMeansClustering.swift:46-59): no embeddings, no dimensions, no clusters, and as many
    clusters as embeddings or more."""
    assert guards(draws, 0, 4, 3) == (1, 0, [], [])
    assert guards(draws, 3, 0, 2) == (1, 0, [0, 0, 0], [])
    for k in (0, -2):
        assert guards(draws, 6, 2, k) == (1, 0, [0] * 6, [-1.0] * 12)            # the centroids are not touched
    emb = [100.0 * i + j for i in range(2) for j in range(2)]
    assert guards(draws, 2, 2, 5) == (1, 2, [0, 1], emb)                          # the raw embeddings come back as the centroids
    assert guards(draws, 2, 2, 2) == (1, 2, [0, 1], emb)                          # n == k
    assert guards(draws, 6, 2, 6)[:3] == (1, 6, [0, 1, 2, 3, 4, 5])
    assert guards(draws, 3, 2, 2) == (0, 0, [-7] * 3, [-1.0] * 6)                 # n > k: the device's work; out_k is set by the entry
    assert guards(draws, 6, 2, 3)[0] == 0


@pytest.mark.parametrize("args,expect", [
    ((100, None, None, None), (None, 1, 100)),
    ((100, 3, 1, 10), (3, 3, 3)),
    ((5, None, 2, 20), (None, 2, 5)),
    ((100, None, 10, 5), (5, 5, 5)),
    ((100, 0, None, None), (1, 1, 1)),
    ((100, -5, None, None), (1, 1, 1)),
    ((100, None, 0, 5), (None, 1, 5)),
    ((100, None, -3, 5), (None, 1, 5)),
])
def test_speaker_constraints_resolve(draws, args, expect):
    """The parametrised cases of tests/test_oracle_kmeans.py; an undecided count comes back as -1."""
    line = run(draws, [("resolve", args[0]) + tuple("-" if a is None else a for a in args[1:])])[0]
    assert tuple(int(x) for x in line.split()) == tuple(-1 if e is None else e for e in expect)
