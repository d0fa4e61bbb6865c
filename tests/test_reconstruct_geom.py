"""The host arithmetic of the reconstruction (csrc/reconstruct_geom.h: chunk starts, the global frame count, each chunk's first / last
global frame, the sanitised hard labels, the override table and the failures it reports) walked on the CPU by
tests/cpu/reconstruct_geom.cpp against the numpy restatement (tests/reconstruct_restatement.py).  The program is stand-alone, reads its
cases from stdin and is built with the address and undefined-behaviour sanitizers.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reconstruct_restatement as R  # noqa: E402

NONE, CHUNK_START, FRAMES, OVERRIDE = 0, 1, 2, 3   # fa::reconstruct::PlanError


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reconstruct_geom") / "reconstruct_geom")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "reconstruct_geom.cpp"), "-o", exe], check=True)
    return exe


def plan(geom, C, F, S, K, offsets=None, fd=0.0, window=10.0, hard=None, overrides=()):
    offsets = [] if offsets is None else [float(v) for v in offsets]
    words = ["plan", C, F, S, K, float(fd), float(window), len(offsets), *offsets]
    words += [0] if hard is None else [1, *np.asarray(hard).reshape(-1).tolist()]
    words += [len(overrides), *[v for o in overrides for v in o]]
    r = subprocess.run([geom], input=" ".join(w.hex() if isinstance(w, float) else str(w) for w in words) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [line.split() for line in r.stdout.split("\n")]
    out = dict(error=int(rows[0][0]), index=int(rows[0][1]), frames=float.fromhex(rows[0][2]), fd=float.fromhex(rows[0][3]))
    if out["error"] in (NONE, OVERRIDE):
        out.update(zip(("sorted", "T", "Kc", "maxc", "smax"), (int(v) for v in rows[1])))
    if out["error"] == NONE:
        out.update(start=[float.fromhex(v) for v in rows[2]], first_g=[int(v) for v in rows[3]], last_g=[int(v) for v in rows[4]],
                   hard=[int(v) for v in rows[5]], ovr=[int(v) for v in rows[6]])
    return out


def offsets_of(kind, C):
    rng = np.random.default_rng(["sorted", "shuffled", "duplicated", "negative", "off_grid", "missing"].index(kind) + 40)
    off = np.arange(C) * 2.0
    if kind == "shuffled":
        off = rng.permutation(off)
    elif kind == "duplicated":
        off = np.repeat(off[:C // 5], 5)
        off[-7:] = off[3]
        off = rng.permutation(off)
    elif kind == "negative":
        off = off - 30.0 + rng.uniform(-1, 1, C)
    elif kind == "off_grid":
        off = np.sort(rng.uniform(0, 60, C))
    elif kind == "missing":
        off = off[:C // 3] * 1.37
    return off


@pytest.mark.parametrize("F", [1, 7, 589])
@pytest.mark.parametrize("kind", ["sorted", "shuffled", "duplicated", "negative", "off_grid", "missing"])
def test_frame_plan_equals_the_restatement(geom, kind, F):
    C, S, K = 50, 3, 9
    off = offsets_of(kind, C)
    got = plan(geom, C, F, S, K, off)
    st = R.frame_stats(np.zeros((C, F, S), np.float32), np.zeros((C, S), np.int64), K, off)
    starts = R.chunk_starts(C, off, 10.0)
    assert got["error"] == NONE and got["fd"] == st["fd"] and got["T"] == st["T"]
    assert (got["Kc"], got["maxc"], got["smax"]) == (9, 3, 3)
    assert [v.hex() for v in got["start"]] == [float(v).hex() for v in starts]
    assert got["sorted"] == int(all(starts[c] >= starts[c - 1] for c in range(1, C)))
    g = [R.global_frames(starts[c], F, st["fd"], st["T"]) for c in range(C)]
    assert got["first_g"] == [int(x[0]) for x in g] and got["last_g"] == [int(x[-1]) for x in g]
    assert got["hard"] == [-1] * (C * S) and got["ovr"] == []          # no labels: no speaker has a cluster
    assert got["sorted"] == (0 if kind in ("shuffled", "duplicated") else 1)


def test_slots_per_frame(geom):
    for K, S, want in ((0, 3, (1, 1, 1)), (1, 3, (1, 1, 1)), (2, 3, (2, 2, 2)), (200, 3, (200, 3, 3)), (5, 0, (5, 0, 1))):
        got = plan(geom, 2, 4, S, K)
        assert (got["Kc"], got["maxc"], got["smax"]) == want and got["T"] == 8


def test_hard_labels_are_sanitised(geom):
    Kc = 6
    hard = [[-2, Kc, Kc - 1], [0, -1, 2 ** 31 - 1], [3, Kc + 1, -2 ** 31]]
    assert plan(geom, 3, 5, 3, Kc, hard=hard)["hard"] == [-1, -1, Kc - 1, 0, -1, -1, 3, -1, -1]
    assert plan(geom, 1, 5, 3, 0, hard=[[0, 1, -2]])["hard"] == [0, -1, -1]      # K = 0 counts as one cluster


def test_overrides_apply_in_order(geom):
    ov = [(0, 8, 3), (2, 5, 1), (4, 4, 2), (4, 6, 0), (19, 20, 5)]
    got = plan(geom, 2, 10, 3, 6, overrides=ov)
    assert got["T"] == 20
    want = R.apply_overrides([[] for _ in range(20)], ov)
    assert got["ovr"] == [s[0] if s else -1 for s in want]


@pytest.mark.parametrize("bad", [(0, 21, 0), (5, 4, 0), (0, 1, 6), (-1, 3, 0), (0, 1, -1)])
def test_a_bad_override_is_reported_by_its_index(geom, bad):
    """hi > T, hi < lo, k >= Kc (and lo < 0, k < 0), behind two overrides that are in range: T and the slots are still reported."""
    got = plan(geom, 2, 10, 3, 6, overrides=[(0, 20, 5), (3, 3, 0), bad, (0, 1, 99)])
    assert (got["error"], got["index"]) == (OVERRIDE, 2) and (got["T"], got["smax"]) == (20, 3)


def test_a_non_finite_chunk_start_is_reported_by_its_chunk(geom):
    for v in (math.nan, math.inf, -math.inf):
        got = plan(geom, 5, 10, 3, 6, [0.0, 2.0, 4.0, v, math.nan], overrides=[(0, 99, 0)])
        assert (got["error"], got["index"]) == (CHUNK_START, 3)


def test_more_frame_slots_than_an_int32(geom):
    """T * smax must stay below 2^31: 3 slots allow 715 827 882 frames."""
    fd, S = 1.0, 3
    fits = plan(geom, 1, 2, S, 3, [715827880.0], fd=fd)
    assert fits["error"] == NONE and fits["T"] == 715827882 and fits["first_g"] == [715827880] and fits["last_g"] == [715827881]
    got = plan(geom, 1, 2, S, 3, [715827881.0], fd=fd, overrides=[(0, 99, 99)])
    assert (got["error"], got["index"], got["frames"]) == (FRAMES, -1, 715827883.0)
    assert plan(geom, 1, 2, 1, 1, [715827881.0], fd=fd)["error"] == NONE         # one slot per frame: the same frames fit
    assert plan(geom, 1, 2, 1, 1, [1e300], fd=fd)["error"] == FRAMES


def test_powerset_table(geom):
    r = subprocess.run([geom], input="masks\n", capture_output=True, text=True, timeout=60)
    assert [int(v) for v in r.stdout.split()] == [sum(1 << s for s in spk) for spk in R.POWERSET]
