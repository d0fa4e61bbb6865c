"""The decisions of the linkage's host side (csrc/ahc_route.h: slots per thread, padded sizes, the round's form and kernel, rounds per replay and the
replay budget, the uniform batch's eligibility / slots per thread / groups / kernel, the batch dispatcher's route) walked on the CPU by
tests/cpu/ahc_route.cpp against the conditions restated here from the host code as it stood at commit 60a2ded, before the decisions had a header of
their own (the cited lines are that commit's).  The program is stand-alone, reads its cases from stdin and is built with the address and
undefined-behaviour sanitizers.  No GPU."""
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BLK, MAX_BLOCKS, ROUNDS_PER_GRAPH = 256, 768, 512          # ahc_ws.h:31-37
AUTO, EXACT, REFERENCE_ORDER = 0, 1, 2                      # fluidaudio_hip.h:387-390


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ahc_route") / "ahc_route")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "ahc_route.cpp"), "-o", exe], check=True)
    return exe


def run(prog, lines):
    r = subprocess.run([prog], input="".join(" ".join(str(int(w) if isinstance(w, bool) else w) for w in ln) + "\n" for ln in lines),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [ln.split() for ln in out]


# ---- the conditions, restated

def pad(n, cols=BLK):
    return -(-n // cols) * cols


def single(forced, no_single_block, N):
    """ahc_rounds.hip:324-329 (slots per thread, padded size, blocks), :29-30 and ahc_batch.hip:551 (the matrix-based rounds hold the problem)."""
    cpt = forced if forced in (1, 2, 4) else (1 if no_single_block or N <= BLK or N > 2 * BLK else 2)
    cols = BLK * cpt
    return cpt, pad(N, cols), pad(N, cols) // cols, int(pad(N) // BLK <= MAX_BLOCKS)


def form(cpt, nblk, mode, d, spec_on):
    """ahc_rounds.hip:216-219 (many-record form, records per lane), :230-231 (the speculative round), :232-245 (the ladder of 13 kernels)."""
    big = nblk > (4 // cpt) * 64
    kc = max(1, (nblk + 63) // 64) if cpt == 1 and not big else 4 // cpt
    spec = spec_on and cpt == 1 and not big and mode == AUTO and d % 2 == 0 and d <= 256
    if spec:
        kernel = {1: "spec_k1", 2: "spec_k2", 3: "spec_k3"}.get(kc, "spec_k4")
    elif cpt == 4:
        kernel = "c4_big" if big else "c4"
    elif cpt == 2:
        kernel = "c2_big" if big else "c2"
    elif big:
        kernel = "c1_big"
    else:
        kernel = {1: "k1", 2: "k2", 3: "k3"}.get(kc, "k4")
    return int(big), kc, int(spec), kernel


def rounds_for(n):
    """ahc_ws.h:315-319."""
    return (min(n + n // 8 + 8, ROUNDS_PER_GRAPH) + 3) & ~3


def budget(n):
    """ahc_rounds.hip:273, ahc_batch.hip:136 and :324: 64 + 8 N / rounds, the rounds those of a graph captured for N points."""
    return 64 + 8 * n // rounds_for(n)


def eligible(n, mode, no_uniform):
    """ahc_batch.hip:402-411."""
    if len(n) < 2 or mode == REFERENCE_ORDER or no_uniform or any(x < 2 for x in n):
        return False
    lo, hi = min(pad(x) for x in n), max(pad(x) for x in n)
    return hi // BLK >= 2 and lo * 2 >= hi and hi // BLK <= 4 * 64


def uniform_cpt(forced, count, nmax):
    """ahc_batch.hip:238-241 and :262-268 (the forced value)."""
    if forced in (1, 2, 4):
        return forced
    return 2 if count * (-(-nmax // BLK)) >= 450 and nmax >= 1024 else 1


def groups(n, forced):
    """ahc_batch.hip:485-491 (kInFlightMinN 16 384: :428, kUniGroupsMinN 4 096: :482)."""
    count = len(n)
    if 1 <= forced <= 4:
        return min(forced, count // 2 if count // 2 > 0 else 1)
    lo = min(n)
    return 2 if (count >= 6 and lo >= 16384) or (count >= 8 and lo >= 4096) else 1


def uniform_kernel(cpt, nblk, waves):
    """ahc_batch.hip:228-235 (the register budget: 6 -> the second, 8 -> the third) and :299-311 (the ladder of nine kernels)."""
    kernel = {6: 3, 8: 4}.get(waves, 2)
    lane_recs = (nblk + 63) // 64
    if cpt == 4:
        return "uni_c4"
    if cpt == 2:
        return "uni_c2k1" if lane_recs == 1 else "uni_c2"
    if kernel == 2 and lane_recs in (1, 2, 3):
        return f"uni_k{lane_recs}"
    return {4: "uni_w4", 3: "uni_w3"}.get(kernel, "uni")


def batch_route(n, mode, allow_groups, capped, in_flight, forced_groups, no_uniform):
    """ahc_batch.hip:539-589 (run_device_batch_impl), count >= 1."""
    count = len(n)
    if count > 1 and mode != REFERENCE_ORDER and any(pad(x) // BLK > MAX_BLOCKS and x >= 2 for x in n):          # :544-574
        return "oversize", 1
    if allow_groups and eligible(n, mode, no_uniform) and not capped:                                             # :576-579
        g = groups(n, forced_groups)
        if g > 1:
            return "groups", g
    if 2 <= count <= 4 and in_flight and all(x >= 16384 for x in n):                                              # :583-585 (kInFlightMax 4: :427)
        return "in_flight", 1
    return ("uniform" if eligible(n, mode, no_uniform) else "block_map"), 1                                       # :588-589


# ---- the cases

NS = (1, 2, 256, 257, 512, 513, 65_536, 65_537, 196_608, 196_609)


def test_slots_per_thread_padding_and_blocks(prog):
    cases = [(f, nsb, N) for f in (0, 1, 2, 3, 4, 7) for nsb in (False, True) for N in NS + (300, 43_200)]
    got = run(prog, [("single",) + c for c in cases])
    assert [tuple(int(x) for x in g) for g in got] == [single(*c) for c in cases]
    assert single(0, False, 256) == (1, 256, 1, 1) and single(0, False, 257) == (2, 512, 1, 1) and single(0, False, 512) == (2, 512, 1, 1)
    assert single(0, False, 513) == (1, 768, 3, 1) and single(0, True, 300) == (1, 512, 2, 1)
    assert single(0, False, 196_608)[2:] == (768, 1) and single(0, False, 196_609)[2:] == (769, 0)


def test_round_form_and_kernel(prog):
    blocks = (1, 2, 3, 64, 65, 128, 129, 192, 193, 256, 257, 768)
    cases = [(cpt, nblk, mode, d, on) for cpt in (1, 2, 4) for nblk in blocks for mode in (AUTO, EXACT) for d in (255, 256, 258) for on in (True, False)]
    got = run(prog, [("form",) + c for c in cases])
    assert [(int(g[0]), int(g[1]), int(g[2]), g[3]) for g in got] == [form(*c) for c in cases]
    for nblk, kc in ((64, 1), (65, 2), (128, 2), (129, 3), (192, 3), (193, 4), (256, 4)):     # records per lane at one slot per thread
        assert form(1, nblk, EXACT, 256, True) == (0, kc, 0, f"k{kc}") and form(1, nblk, AUTO, 256, True) == (0, kc, 1, f"spec_k{kc}")
    assert form(1, 257, AUTO, 256, True) == (1, 4, 0, "c1_big")                                # 65 537 points: the many-record kernel, not speculative
    assert form(2, 128, AUTO, 256, True) == (0, 2, 0, "c2") and form(2, 129, AUTO, 256, True) == (1, 2, 0, "c2_big")
    assert form(4, 64, AUTO, 256, True) == (0, 1, 0, "c4") and form(4, 65, AUTO, 256, True) == (1, 1, 0, "c4_big")
    for d, spec in ((255, 0), (256, 1), (258, 0)):
        assert form(1, 3, AUTO, d, True)[2] == spec and form(1, 3, AUTO, d, False)[2] == 0 and form(1, 3, EXACT, d, True)[2] == 0


def test_rounds_per_replay_and_the_budget(prog):
    ns = (1, 2, 50, 447, 448, 449, 512, 43_200, 196_608)
    got = run(prog, [("rounds", n) for n in ns])
    assert [(int(g[0]), int(g[1])) for g in got] == [(rounds_for(n), budget(n)) for n in ns]
    assert all(int(g[0]) % 4 == 0 and int(g[0]) <= 512 for g in got)
    assert [rounds_for(n) for n in (1, 50, 447, 448, 449, 43_200)] == [12, 64, 512, 512, 512, 512]
    assert budget(50) == 64 + 400 // 64 and budget(43_200) == 64 + 675


def test_uniform_eligibility(prog):
    sets = [[512, 1024], [512, 1280],                      # 2 lo == hi; 2 lo == hi - 256
            [200, 256], [300, 512], [40_000, 65_536], [40_000, 65_537],      # the largest padded size: 1, 2, 256, 257 blocks
            [1, 600], [600, 1], [2, 300], [600], [], [600, 500], [600, 200], [720, 1400, 720, 720]]
    cases = [(mode, off, n) for n in sets for mode in (AUTO, EXACT, REFERENCE_ORDER) for off in (False, True)]
    got = run(prog, [("elig", mode, off, len(n), *n) for mode, off, n in cases])
    assert [g == ["1"] for g in got] == [eligible(n, mode, off) for mode, off, n in cases]
    assert eligible([512, 1024], AUTO, False) and not eligible([512, 1280], AUTO, False)
    assert not eligible([200, 256], AUTO, False) and eligible([300, 512], AUTO, False)
    assert eligible([40_000, 65_536], AUTO, False) and not eligible([40_000, 65_537], AUTO, False)
    assert not eligible([1, 600], AUTO, False) and not eligible([600], AUTO, False) and not eligible([600, 500], REFERENCE_ORDER, False)


def test_uniform_slots_per_thread_groups_and_kernel(prog):
    cases = [(f, count, nmax) for f in (0, 1, 2, 3, 4) for count, nmax in ((449, 1024), (450, 1024), (450, 1023), (113, 1023), (113, 1024), (90, 1280), (89, 1280), (64, 1792), (3, 43_200), (2, 43_200))]
    assert [int(g[0]) for g in run(prog, [("ucpt",) + c for c in cases])] == [uniform_cpt(*c) for c in cases]
    assert uniform_cpt(0, 449, 256) == 1 and uniform_cpt(0, 450, 1024) == 2 and uniform_cpt(0, 450, 1023) == 1      # 449 / 450 workgroups, Nmax 1 023 / 1 024
    assert uniform_cpt(0, 90, 1280) == 2 and uniform_cpt(0, 64, 1792) == 1 and uniform_cpt(0, 89, 1280) == 1        # 450, 448 and 445 workgroups (449 is prime)
    gcases = [(f, [lo] + [20_000] * (count - 1)) for f in (0, 1, 2, 3, 4, 5) for count in (1, 2, 5, 6, 7, 8) for lo in (4095, 4096, 16_383, 16_384)]
    assert [int(g[0]) for g in run(prog, [("groups", f, len(n), *n) for f, n in gcases])] == [groups(n, f) for f, n in gcases]
    assert groups([16_384] * 6, 0) == 2 and groups([16_383] + [20_000] * 5, 0) == 1 and groups([4096] * 8, 0) == 2 and groups([4095] + [5000] * 7, 0) == 1
    assert groups([20_000] * 5, 0) == 1 and groups([5000] * 7, 0) == 1
    assert [groups([20_000] * 5, f) for f in (1, 2, 3, 4)] == [1, 2, 2, 2] and groups([20_000], 3) == 1             # the switch against count / 2
    kcases = [(cpt, nblk, waves) for cpt in (1, 2, 4) for nblk in (1, 64, 65, 128, 129, 192, 193, 256) for waves in (0, 5, 6, 8)]
    assert [g[0] for g in run(prog, [("ukern",) + c for c in kcases])] == [uniform_kernel(*c) for c in kcases]
    assert [uniform_kernel(1, b, 0) for b in (64, 65, 128, 129, 192, 193, 256)] == ["uni_k1", "uni_k2", "uni_k2", "uni_k3", "uni_k3", "uni", "uni"]
    assert uniform_kernel(1, 64, 6) == "uni_w3" and uniform_kernel(1, 64, 8) == "uni_w4" and uniform_kernel(2, 64, 8) == "uni_c2k1"
    assert uniform_kernel(2, 65, 0) == "uni_c2" and uniform_kernel(4, 64, 6) == "uni_c4"


def test_the_dispatchers_route(prog):
    sets = [[600], [1], [196_609], [600, 500], [600, 200], [1, 600], [196_609, 600, 500], [196_609, 1], [196_608, 196_608], [600, 500, 196_609, 0],
            [20_000] * 2, [20_000] * 4, [20_000] * 5, [16_383, 20_000], [20_000] * 6, [20_000] * 8, [5000] * 8, [5000] * 7, [20_000, 5000, 20_000],
            [720, 1400, 720, 720]]
    flags = list(itertools.product((False, True), repeat=4))                      # allow_groups, capped, in_flight, no_uniform
    cases = [(mode, a, c, f, g, off, n) for n in sets for mode in (AUTO, REFERENCE_ORDER) for a, c, f, off in flags for g in (0, 1, 3)]
    got = run(prog, [("route", mode, a, c, f, g, off, len(n), *n) for mode, a, c, f, g, off, n in cases])
    assert [(r[0], int(r[1])) for r in got] == [batch_route(n, mode, a, c, f, g, off) for mode, a, c, f, g, off, n in cases]
    assert batch_route([196_609, 600, 500], AUTO, True, False, False, 0, False) == ("oversize", 1)                 # mixed oversize
    assert batch_route([196_609, 600], REFERENCE_ORDER, True, False, False, 0, False) == ("block_map", 1)           # reference order: one after the other
    assert batch_route([20_000] * 6, AUTO, True, False, False, 0, False) == ("groups", 2)
    assert batch_route([20_000] * 6, AUTO, True, True, False, 0, False) == ("uniform", 1)                           # a capped context: one workspace
    assert batch_route([20_000] * 6, AUTO, False, False, False, 0, False) == ("uniform", 1)
    assert batch_route([20_000] * 6, AUTO, True, False, False, 3, False) == ("groups", 3)
    assert batch_route([20_000] * 4, AUTO, True, False, True, 0, False) == ("in_flight", 1)                         # in-flight-switched
    assert batch_route([20_000] * 5, AUTO, True, False, True, 0, False) == ("uniform", 1)
    assert batch_route([16_383, 20_000], AUTO, True, False, True, 0, False) == ("uniform", 1)
    assert batch_route([20_000] * 4, AUTO, True, False, True, 2, False) == ("groups", 2)                            # groups come first
    assert batch_route([600, 200], AUTO, True, False, False, 0, False) == ("block_map", 1)
    assert batch_route([600, 500], AUTO, True, False, False, 0, True) == ("block_map", 1)
