"""The host arithmetic of the clustering stage's kernels (csrc/vbx_geom.h: slices of the frame axis, shards, record sizes, the tiled route,
the E-step's LDS limit; csrc/post_geom.h: rows grouped by chunk, the Hungarian scratch, the LDS-or-slab and centroid routes) walked on the
CPU by tests/cpu/cluster_geom.cpp against the conditions restated here.  The program is stand-alone, reads its cases from stdin and is
built with the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SPLIT = 64


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cluster_geom") / "cluster_geom")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "cluster_geom.cpp"), "-o", exe], check=True)
    return exe


def run(geom, lines):
    r = subprocess.run([geom], input="".join(" ".join(str(int(w) if isinstance(w, bool) else w) for w in ln) + "\n" for ln in lines),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


# ---- the conditions, restated

def slice_range(Tg, z):
    """Slices of ceil(Tg / 64) frames; the last ones are short or empty."""
    per = -(-Tg // SPLIT)
    return min(z * per, Tg), min((z + 1) * per, Tg)


def shard_range(Tg, rank, world):
    if Tg <= 0 or world <= 0 or SPLIT % world or not 0 <= rank < world:
        return 0, 0
    zn = SPLIT // world
    own = [slice_range(Tg, z) for z in range(rank * zn, (rank + 1) * zn)]      # the union of the rank's slices
    return own[0][0], own[-1][1]


def chunk_doubles(S, D, world):
    if S < 1 or D < 1 or world < 1 or SPLIT % world:
        return 0
    return (SPLIT // world) * (S * (D + 1) + 1)


def groups(ids, K):
    order = sorted(range(len(ids)), key=lambda i: ids[i])                        # sorted() is stable: ascending rows inside a chunk
    starts = [i for i in range(len(ids)) if i == 0 or ids[order[i]] != ids[order[i - 1]]] + [len(ids)]
    max_rows = max(b - a for a, b in zip(starts, starts[1:]))
    side = max(max_rows, K)
    return len(starts) - 1, max_rows, side, side > 256, order, starts


TG = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 43_200, 2**31 + 5)
WORLDS = (1, 2, 4, 8, 16, 32, 64)


# ---- the cases

def test_slices_are_the_restated_ranges_and_tile_the_frame_axis(geom):
    for Tg, line in zip(TG, run(geom, [("slices", Tg) for Tg in TG])):
        v = [int(w) for w in line.split()]
        got = list(zip(v[0::2], v[1::2]))
        assert got == [slice_range(Tg, z) for z in range(SPLIT)]
        assert got[0][0] == 0 and got[-1][1] == Tg
        assert all(lo <= hi for lo, hi in got)
        assert all(a[1] == b[0] for a, b in zip(got, got[1:]))                  # disjoint, ascending, no gap: they cover [0, Tg)
    assert slice_range(65, 32) == (64, 65) and slice_range(65, 33) == (65, 65)  # a slice of one frame, then empty ones
    assert slice_range(1, 0) == (0, 1) and slice_range(1, 1) == (1, 1)


def test_a_shard_holds_the_union_of_its_slices(geom):
    cases = [(Tg, r, w) for Tg in TG for w in WORLDS for r in range(w)]
    got = [tuple(int(x) for x in ln.split()) for ln in run(geom, [("shard",) + c for c in cases])]
    assert got == [shard_range(*c) for c in cases]
    for Tg in TG:
        for w in WORLDS:
            mine = [g for c, g in zip(cases, got) if c[0] == Tg and c[2] == w]
            assert mine[0][0] == 0 and mine[-1][1] == Tg and all(a[1] == b[0] for a, b in zip(mine, mine[1:]))
    bad = [(1000, 0, 0), (1000, 0, 3), (1000, 2, 3), (1000, 0, 128), (1000, -1, 4), (1000, 4, 4), (1000, 64, 64), (0, 0, 1), (-5, 0, 1)]
    assert [ln.split() for ln in run(geom, [("shard",) + c for c in bad])] == [["0", "0"]] * len(bad)


def test_chunk_doubles(geom):
    cases = [(S, D, w) for S in (1, 7, 597) for D in (1, 128) for w in WORLDS] + [(0, 128, 1), (3, 0, 1), (3, 128, 0), (3, 128, 3), (3, 128, 128), (3, 128, -1)]
    got = [int(ln) for ln in run(geom, [("chunk",) + c for c in cases])]
    assert got == [chunk_doubles(*c) for c in cases]
    assert got[-6:] == [0] * 6 and chunk_doubles(7, 128, 8) == 8 * (7 * 129 + 1)


def test_routes(geom):
    tiled = run(geom, [("tiled", S, on) for S in (47, 48) for on in (True, False)])
    assert tiled == ["0", "0", "1", "0"]                                         # from 48 speakers on, and only while the switch allows it
    assert [ln.split() for ln in run(geom, [("dim", 2048), ("dim", 2049), ("dim", 1)])] == [["1", "65536"], ["0", "65568"], ["1", "32"]]
    assert run(geom, [("cen", n) for n in (0, 511, 512, 43_200)]) == ["0", "0", "1", "1"]


def hung_case(geom, ids, K):
    line = run(geom, [("groups", K, len(ids), *ids)])[0]
    head, order, starts = (part.split() for part in line.split("|"))
    n_chunks, max_rows, side, slabs, slab_bytes = (int(x) for x in head)
    want = groups(ids, K)
    assert (n_chunks, max_rows, side, bool(slabs), [int(x) for x in order], [int(x) for x in starts]) == want
    e = side + 1
    assert slab_bytes % 16 == 0 and 3 * 8 * e + 2 * 4 * e + e <= slab_bytes < 3 * 8 * e + 2 * 4 * e + e + 16   # u, v, minv, p, way, used
    return want


def test_chunk_groups_match_a_stable_sort(geom):
    rng = np.random.default_rng(0)
    n = 500
    permuted = np.repeat(np.arange((n + 2) // 3), 3)[:n][rng.permutation(n)]
    for ids in (permuted.tolist(), (permuted - 80).tolist(),                     # permuted ids; negative ids
                [5] * 40, [7], [-3], rng.permutation(300).tolist()):            # one chunk; n = 1; all ids distinct
        n_chunks, max_rows, _, slabs, order, starts = hung_case(geom, ids, 3)
        assert sorted(order) == list(range(len(ids))) and not slabs
        for a, b in zip(starts, starts[1:]):
            assert len({ids[i] for i in order[a:b]}) == 1 and order[a:b] == sorted(order[a:b])
    assert hung_case(geom, [7], 3)[:3] == (1, 1, 3) and hung_case(geom, [5] * 40, 3)[:3] == (1, 40, 40)
    assert hung_case(geom, rng.permutation(300).tolist(), 3)[:2] == (300, 1)


def test_lds_or_slab_boundary(geom):
    for per, K, slabs in ((256, 3, False), (257, 3, True)):                      # the largest chunk decides ...
        ids = [0] * per + [1] * 5 + [2] * 2
        assert hung_case(geom, ids, K)[1:4] == (per, per, slabs)
    for K, slabs in ((256, False), (257, True)):                                 # ... or the number of clusters
        ids = [i // 2 for i in range(40)]
        assert hung_case(geom, ids, K)[1:4] == (2, K, slabs)
