"""The plan of the linkage's drive loop (csrc/ahc_route.h: drive_plan / plan_next / plan_retire — the look-ahead bound and the ladder of replay lengths)
walked on the CPU by tests/cpu/ahc_drive_plan.cpp against a model device, for N from 2 to 200 000, both merge rates of a round and adversarial progress:
none at all, the most a round can commit throughout, and the most until the end is near and none from then on.  The program is stand-alone, reads its
cases from stdin and is built with the address and undefined-behaviour sanitizers.  No GPU.

Properties: a replay goes behind others only while those cannot finish the problem (N - 1 - step - m * rounds in flight > 0, m = merges a round commits at
most) — so no replay is enqueued that the synchronous drive would not have enqueued —, never more than two replays are in flight, every length is a
multiple of 4, the rounds enqueued stay within replay_budget(N) replays of rounds_for(N) rounds (the budget bounds ROUNDS, as replay_budget's own comment says;
in replays: within replay_budget(N) while the device progresses, and never above replay_budget(N) x 512 / 32, reached only by a device that stalls), and with FA_AHC_SYNC_DRIVE the plan is the one from
before the look-ahead: one replay of rounds_for(N) rounds at a time."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FULL, LADDER = 512, (512, 128, 32)                         # ahc_route.h: kRoundsPerGraph, kLadder
NONE, ONE, TWO, STALL = 0, 1, 2, 3                          # progress of the model device per round


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ahc_drive_plan") / "ahc_drive_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "ahc_drive_plan.cpp"), "-o", exe], check=True)
    return exe


def run(prog, lines):
    r = subprocess.run([prog], input="".join(" ".join(str(w) for w in ln) + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def rounds_for(n):
    return (min(n + n // 8 + 8, FULL) + 3) & ~3


def budget(n):
    return 64 + 8 * n // rounds_for(n)


SWEEPS = [(2, 3000, 1), (3001, 200_000, 997), (43_200, 43_200, 1), (199_990, 200_000, 1)]


@pytest.mark.parametrize("spec", (0, 1))
@pytest.mark.parametrize("rate", (NONE, ONE, TWO, STALL))
def test_the_look_ahead_keeps_its_bound(prog, spec, rate):
    for lo, hi, stride in SWEEPS:
        got = [int(x) for x in run(prog, [("sweep", lo, hi, stride, spec, 0, rate)])[0].split()]
        replays, rounds, depth, behind_finishable, behind_done, bad_length, over_rounds, over_replays, not_done, _, over_stall = got
        assert replays > 0 and rounds >= replays
        assert depth <= 2
        assert behind_finishable == 0                      # the issue's inequality, evaluated by the walk from what the host has read
        assert behind_done == 0                            # even behind an infinitely fast device no replay starts on a finished problem unasked
        assert bad_length == 0
        assert over_rounds == 0                            # the loop ends within the budget, whatever the device does
        if rate in (ONE, TWO):                             # in replays as well while the device progresses (a device that does not may be asked for
            assert over_replays == 0                       # shorter replays: the budget is a bound on ROUNDS, replay_budget(N) x rounds_for(N), as it was)
        else:                                              # worst case: every replay the shortest rung, replay_budget(N) x 512 / 32 replays (16 x the synchronous drive's)
            assert over_stall == 0
        n_cases = len(range(lo, hi + 1, stride))
        if rate == NONE:                                   # the budget, not the device, ends these walks
            assert not_done == n_cases
        if rate in (ONE, TWO):                             # a device that makes progress finishes
            assert not_done == 0


@pytest.mark.parametrize("spec", (0, 1))
@pytest.mark.parametrize("rate", (NONE, ONE, TWO, STALL))
def test_the_switch_gives_the_synchronous_plan(prog, spec, rate):
    for lo, hi, stride in SWEEPS:
        got = [int(x) for x in run(prog, [("sweep", lo, hi, stride, spec, 1, rate)])[0].split()]
        assert got[2] == 1 and got[9] == 0                 # one in flight, every replay of rounds_for(N) rounds
        assert got[3] == got[4] == got[5] == got[6] == got[7] == 0


def parse(line):
    head, _, tail = line.partition(":")
    return [int(x) for x in head.split()], [int(x) for x in tail.split()]


def test_synchronous_replays_are_todays(prog):
    """Replays of the synchronous plan: ceil((N - 1) / (rate * rounds_for(N))) for a device that progresses, replay_budget(N) for one that does not."""
    cases = [(n, spec, rate) for n in (2, 50, 447, 448, 1100, 3000, 43_200, 200_000) for spec in (0, 1) for rate in (NONE, ONE, TWO)]
    for (n, spec, rate), line in zip(cases, run(prog, [("walk", n, spec, 1, rate) for n, spec, rate in cases])):
        (replays, rounds, depth, *_), lengths = parse(line)
        per = min(rate, 2 if spec else 1) * rounds_for(n)
        assert lengths == [rounds_for(n)] * replays and depth == 1 and rounds == replays * rounds_for(n)
        assert replays == (budget(n) if per == 0 else -(-(n - 1) // per))


def test_the_ladder(prog):
    """The lengths restated: the longest rung that the merges certainly left fill at the round's rate, else the shortest; small problems keep one length."""
    def plan(n, m, rate):
        total, left, step, fly, out = n - 1, n - 1, 0, [], []
        while True:
            while left > 0 and len(fly) < 2:
                floor = left - m * sum(r for r, _ in fly)
                if fly and floor <= 0:
                    break
                ln = rounds_for(n)
                if ln == FULL:
                    ln = next((r for r in LADDER if m * r <= floor), LADDER[-1])
                step = min(total, step + min(rate, m) * ln)
                fly.append((ln, step))
                out.append(ln)
            if not fly:
                return out
            left = total - fly.pop(0)[1]
    cases = [(n, spec, rate) for n in (2, 300, 447, 448, 600, 1100, 2500, 3000, 43_200, 50_000, 200_000) for spec in (0, 1) for rate in (ONE, TWO)]
    for (n, spec, rate), line in zip(cases, run(prog, [("walk", n, spec, 0, rate) for n, spec, rate in cases])):
        (replays, rounds, depth, *_, done), lengths = parse(line)
        assert done == 1 and lengths == plan(n, 2 if spec else 1, rate), (n, spec, rate)
        if rounds_for(n) < FULL:
            assert set(lengths) == {rounds_for(n)}
        # launches behind `done`: fewer than the shortest rung + one replay queued ahead of a state not yet read cannot happen (the bound), so < 2 rungs
        needed = -(-(n - 1) // min(rate, 2 if spec else 1))
        if rounds_for(n) == FULL:
            assert rounds - needed < 2 * LADDER[-1], (n, spec, rate, rounds, needed)
    # N = 2 500 (tests/test_gpu_ahc_drive.py halts on a tie between merges 1 100 and 2 300): even at two merges a round the second replay is enqueued before
    # the first state is read and the third before the second — the halt, which no replay in front of the second can reach, is read with a replay queued behind it
    for rate in (ONE, TWO):
        (_, _, depth, *_), lengths = parse(run(prog, [("walk", 2500, 1, 0, rate)])[0])
        assert depth == 2 and lengths[:2] == [512, 512] and len(lengths) >= 4 and 2 * 512 < 1100
        assert 2499 - 2 * sum(lengths[:2]) > 0                               # the third goes behind the second whatever the first did
    # the headline: 43 200 rows — the full length while 1 024 merges are certainly left, then shorter ones; in flight two deep; behind `done` less than a rung
    for rate, needed in ((TWO, 21_600), (ONE, 43_199)):
        (_, rounds, depth, *_), lengths = parse(run(prog, [("walk", 43_200, 1, 0, rate)])[0])
        assert depth == 2 and lengths == sorted(lengths, reverse=True) and lengths[0] == 512 and lengths[-1] == 32
        assert rounds - needed < 32
        assert rate == TWO or 128 in lengths
