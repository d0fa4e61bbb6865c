"""The argument pass and the plan of the timeline (csrc/timeline_launch.h: the config checks, every recording's offsets into the two
prediction arrays, the tiles of the longest recording, the workgroups of the tile kernels and every refusal of a call) walked on the CPU
by tests/cpu/timeline_plan.cpp against the conditions restated here.  The program is stand-alone, reads its cases from stdin and is
built with the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID_ARGUMENT, INDEX_OVERFLOW = 0, 1, 2
SIGMOIDS, LOGITS = 0, 1
TILE = 256 * 8                                                                   # frames of a workgroup of the state scan
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("timeline_plan") / "timeline_plan")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "timeline_plan.cpp"), "-o", exe], check=True)
    return exe


def call(plan, fin, tent=None, S=4, activity=SIGMOIDS, pads=(0, 0, 0, 0), capacity=100, have_fin=True, have_tent=True, B=None):
    nb = len(fin) if B is None else B
    fin, tent = fin[:max(nb, 0)], tent and tent[:max(nb, 0)]
    words = ["call", S, activity, *pads, capacity, int(have_fin), int(have_tent), nb, *fin, *(["-"] if tent is None and nb > 0 else (tent or []))]
    r = subprocess.run([plan], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    parts = [p.strip() for p in r.stdout.strip().split("|")]
    if int(parts[0]) != OK:
        return int(parts[0]), parts[1]
    per = [int(x) for x in parts[2].split()]
    return OK, tuple(int(x) for x in parts[1].split()), [tuple(per[i:i + 4]) for i in range(0, len(per), 4)]


def restated(fin, tent, S):
    tent = tent or [0] * len(fin)
    recs, fsum, tsum = [], 0, 0
    for nf, nt in zip(fin, tent):
        recs.append((fsum, tsum, nf, nt))
        fsum += nf
        tsum += nt
    max_tiles = max(1, -(-max(nf + nt for nf, nt in zip(fin, tent)) // TILE))
    Q = len(fin) * S
    return OK, (fsum, tsum, Q, max_tiles, Q * max_tiles), recs


LENGTHS = (0, 1, 2047, 2048, 2049)


@pytest.mark.parametrize("S", [1, 4])
def test_the_plan_is_the_restated_one(plan, S):
    for n in LENGTHS:                                                            # one recording: finalized only, then with a tentative tail
        assert call(plan, [n], S=S) == restated([n], None, S)
        for nt in LENGTHS:
            assert call(plan, [n], [nt], S=S) == restated([n], [nt], S)
    fin, tent = list(LENGTHS), [7, 0, 1, 2048, 0]
    assert call(plan, fin, S=S) == restated(fin, None, S)                        # all in one call: the offsets are prefix sums
    assert call(plan, fin, tent, S=S) == restated(fin, tent, S)
    tiles = [call(plan, [n], S=S)[1][3] for n in LENGTHS]
    assert tiles == [1, 1, 1, 1, 2]                                              # an empty recording still has its one tile
    assert call(plan, [2047], [2], S=S)[1][3:] == (2, 2 * S)                     # the two sides of a recording share its tiles
    assert call(plan, fin, tent, S=S)[1][3:] == (2, 2 * 5 * S)


def test_verdicts(plan):
    assert call(plan, [5, -1]) == (INVALID_ARGUMENT, "timeline: recording 1 has a negative frame count")
    assert call(plan, [5], [-1]) == (INVALID_ARGUMENT, "timeline: recording 0 has a negative frame count")
    assert call(plan, [INT32_MAX - 5], [5]) == (INDEX_OVERFLOW, "timeline: recording 0 has 2^31 frames or more")
    assert call(plan, [INT32_MAX]) == (INDEX_OVERFLOW, "timeline: recording 0 has 2^31 frames or more")
    assert call(plan, [INT32_MAX - 6], [5])[0] == OK
    # blocks = B S max_tiles: 2^31 - 2 frames are 2^20 tiles, 2048 speakers make 2^31 workgroups
    assert call(plan, [INT32_MAX - 1], S=2048) == (INDEX_OVERFLOW, "timeline: 2147483648 tiles")
    assert call(plan, [INT32_MAX - 1], S=2047)[1][3:] == (2 ** 20, 2047 * 2 ** 20)
    assert call(plan, [TILE] * 1, S=INT32_MAX) == (INDEX_OVERFLOW, "timeline: 2147483647 tiles")        # blocks == INT32_MAX is refused too
    assert call(plan, [TILE] * 1, S=INT32_MAX - 1)[0] == OK
    assert call(plan, [3], have_fin=False) == (INVALID_ARGUMENT, "timeline: predictions are required")
    assert call(plan, [3], [2], have_tent=False) == (INVALID_ARGUMENT, "timeline: predictions are required")
    assert call(plan, [0, 0], have_fin=False, have_tent=False)[0] == OK                                  # nothing to read: no array needed
    assert call(plan, [3], [0], have_tent=False)[0] == OK
    assert call(plan, [3], activity=LOGITS) == (INVALID_ARGUMENT, "timeline: only the sigmoid activity type is supported")
    for kw in (dict(S=0), dict(capacity=-1), dict(B=-1), dict(pads=(-1, 0, 0, 0)), dict(pads=(0, -1, 0, 0)), dict(pads=(0, 0, -1, 0)), dict(pads=(0, 0, 0, -1))):
        assert call(plan, [3], **kw) == (INVALID_ARGUMENT, "timeline: bad arguments")
    assert call(plan, [], B=0) == (OK, (0, 0, 0, 1, 0), [])                                              # an empty batch is answered before the plan


def test_a_call_with_two_faults_reports_the_first_in_the_order_of_the_pass(plan):
    """The order timeline_segments has always checked in: the sizes and the config, the activity type; then recording by recording a
    negative count before too many frames; then the missing predictions; last the workgroup count."""
    assert call(plan, [3], S=0, activity=LOGITS)[1] == "timeline: bad arguments"
    assert call(plan, [-1], activity=LOGITS)[1] == "timeline: only the sigmoid activity type is supported"
    assert call(plan, [INT32_MAX, -1])[1] == "timeline: recording 0 has 2^31 frames or more"
    assert call(plan, [5, INT32_MAX], [-1, 0])[1] == "timeline: recording 0 has a negative frame count"
    assert call(plan, [5, -1], have_fin=False)[1] == "timeline: recording 1 has a negative frame count"
    assert call(plan, [INT32_MAX - 1], S=2048, have_fin=False)[1] == "timeline: predictions are required"
