#!/usr/bin/env python3
"""Where the stream is empty during one headline step: reduces a rocprofv3 kernel + memory-copy trace (CSV output, no counters in the same run) of
`python bench.py --gpus 1 --steps 2 --warmup 1` to the figures of profiles/r14_stage_gaps.txt.

    stage_gaps.py DIR [--events OUT.tsv.gz]      DIR holds *_kernel_trace.csv and *_memory_copy_trace.csv (searched recursively)
    stage_gaps.py --from-events FILE.tsv.gz      the reduced event list written by --events

The step looked at is the last one: the last run of round launches (ahc_round_t / ahc_rounds_single_block) with everything between the end of the
run before it and the next run's start.  Replay boundaries are taken by launch index, not by the length of a pause (under the tracer a graph of 512 nodes is
submitted in pieces, and pauses appear inside replays as well): in front of every k x REPLAY-th launch, and — a run whose launch count is no multiple of REPLAY
ends with shorter replays, all multiples of SHORT — in front of every k x SHORT-th launch behind the last but one multiple of REPLAY."""
import argparse
import csv
import glob
import gzip
import os
import statistics

GAP_US = 10.0          # a pause between two events longer than this is reported
STEP_PAUSE_US = 2e3    # round launches further apart than this belong to different steps (the start-up of the next step alone is > 10 ms)
REPLAY = 512           # launches of a full replay (ahc_route.h: kRoundsPerGraph)
SHORT = 32             # the shortest replay of the ladder (ahc_route.h: kLadder)


def load_dir(d):
    ev = []
    for path in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                ev.append(("K", kernel_name(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for path in glob.glob(os.path.join(d, "**", "*_memory_copy_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                ev.append(("C", r.get("Direction", "copy"), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    ev.sort(key=lambda e: e[2])
    return ev


def kernel_name(n):
    n = n.replace("(anonymous namespace)::", "").replace("void ", "")
    return n.split("(")[0][:96]


def is_round(e):
    return e[0] == "K" and ("ahc_round_t" in e[1] or "ahc_rounds_single_block" in e[1])


def histogram(us, edges=(5, 10, 20, 30, 40, 60, 80, 120, 200, 500)):
    rows, lo = [], 0
    for hi in edges + (float("inf"),):
        n = sum(1 for g in us if lo <= g < hi)
        if n:
            rows.append(f"    {lo:>5g} .. {hi:<5g} us: {n}")
        lo = hi
    return "\n".join(rows)


def report(ev):
    rounds = [i for i, e in enumerate(ev) if is_round(e)]
    runs, cur = [], [rounds[0]]
    for a, b in zip(rounds, rounds[1:]):
        if ev[b][2] - ev[a][3] > STEP_PAUSE_US * 1e3:
            runs.append(cur)
            cur = []
        cur.append(b)
    runs.append(cur)
    run = runs[-1]
    lo = runs[-2][-1] + 1 if len(runs) > 1 else 0
    step = ev[lo:]
    t0 = step[0][2]
    print(f"steps in the trace (runs of round launches): {len(runs)}; the last one: {len(run)} round launches, {len(step) - len(run)} other events, "
          f"{(step[-1][3] - t0) / 1e6:.3f} ms from its first event to its last")
    dur = [(ev[i][3] - ev[i][2]) / 1e3 for i in run]
    med = statistics.median(dur)
    print(f"round launches: median duration {med:.2f} us, sum {sum(dur) / 1e3:.2f} ms, first start to last end {(ev[run[-1]][3] - ev[run[0]][2]) / 1e6:.2f} ms")
    # (a) replay boundaries, by launch index
    pause = [0.0] + [(ev[b][2] - ev[a][3]) / 1e3 for a, b in zip(run, run[1:])]   # pause[k]: in front of launch k
    full_end = len(run) if len(run) % REPLAY == 0 else (len(run) // REPLAY - 1) * REPLAY
    at_full = [pause[k] for k in range(REPLAY, full_end + 1, REPLAY) if k < len(run)]
    at_short = [pause[k] for k in range(full_end + SHORT, len(run), SHORT)]
    is_boundary = set(range(REPLAY, full_end + 1, REPLAY)) | set(range(full_end + SHORT, len(run), SHORT))
    inside = [pause[k] for k in range(1, len(run)) if k not in is_boundary]
    print(f"(a) pauses in front of every {REPLAY}th launch (boundaries of full replays): {len(at_full)}, sum {sum(at_full) / 1e3:.3f} ms, "
          f"median {statistics.median(at_full) if at_full else 0:.1f} us, min {min(at_full, default=0):.1f}, max {max(at_full, default=0):.1f} us")
    print(histogram(at_full))
    if at_short:
        print(f"    in front of every {SHORT}th launch behind launch {full_end} (where the shorter replays of the ladder begin and end; at most that many boundaries): "
              f"{len(at_short)}, sum {sum(at_short) / 1e3:.3f} ms, above {GAP_US:g} us: {sum(1 for g in at_short if g > GAP_US)}")
    big = [g for g in inside if g > GAP_US]
    print(f"    pauses at all other launches (inside a replay; an artefact of the tracer, the untraced period leaves no room for them): above {GAP_US:g} us: {len(big)}, "
          f"sum {sum(big) / 1e3:.3f} ms; the rest: median {statistics.median(inside):.2f} us, sum {(sum(inside) - sum(big)) / 1e3:.2f} ms")
    # (b) the idle tail: trailing launches much shorter than a working round (a round behind `done` returns after the decision)
    tail, win = 0, 16   # in windows of 16 launches: single launches scatter (the last working rounds of a run are short as well)
    while tail + win <= len(run) and statistics.median(dur[len(run) - tail - win:len(run) - tail]) < 0.6 * med:
        tail += win
    if tail:
        first = run[len(run) - tail]
        print(f"(b) trailing round launches, in windows of 16 with a median below 0.6 x the median duration (behind `done`): {tail}, kernel time {sum(dur[-tail:]) / 1e3:.3f} ms, "
              f"from the first one's start to the last one's end {(ev[run[-1]][3] - ev[first][2]) / 1e6:.3f} ms (median duration {statistics.median(dur[-tail:]):.2f} us)")
    else:
        print("(b) no trailing short round launches")
    # (c) everything else of the step, with the pause in front of each event
    print(f"(c) events of the step other than round launches; `pause` = time since the end of the event before (marked * above {GAP_US:g} us)")
    print("    at_ms      pause_us   dur_us     event")
    prev_end, total, n_round = None, 0.0, 0
    for e in step:
        pause = (e[2] - prev_end) / 1e3 if prev_end is not None else 0.0
        if is_round(e):
            n_round += 1
        else:
            if n_round:
                print(f"    {'':10s} {'':10s} {'':10s} ... {n_round} round launches ...")
                n_round = 0
            if pause > GAP_US:
                total += pause
            print(f"    {(e[2] - t0) / 1e6:<10.3f} {pause:<9.1f}{'*' if pause > GAP_US else ' '} {(e[3] - e[2]) / 1e3:<10.1f} {e[0]} {e[1]}")
        prev_end = max(prev_end, e[3]) if prev_end is not None else e[3]
    print(f"    sum of the marked pauses in front of events other than round launches: {total / 1e3:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--events")
    ap.add_argument("--from-events")
    a = ap.parse_args()
    if a.from_events:
        with gzip.open(a.from_events, "rt") as f:
            ev = [(k, n, int(s), int(e)) for k, n, s, e in (ln.rstrip("\n").split("\t") for ln in f)]
    else:
        ev = load_dir(a.dir)
    if a.events:
        with gzip.open(a.events, "wt") as f:
            for e in ev:
                f.write("\t".join(str(x) for x in e) + "\n")
    report(ev)


if __name__ == "__main__":
    main()
