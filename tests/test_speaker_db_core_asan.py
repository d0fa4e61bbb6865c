"""fluidaudio_amd/csrc/speaker_db_core.h — the arithmetic and the state layout of the online speaker database that host and kernels share —
under the address and undefined-behaviour sanitizers: tests/cpu/speaker_db_core_main.cpp, a stand-alone program, assigns into databases
whose arrays have exactly their size (raw_capacity 1, 3 and 50), fills every slot, overflows the table and wraps the ring; it runs as a
child process and must end clean.  Every record and every current embedding it prints equals the restatement's, as bits.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import online_restatement as R  # noqa: E402

F = np.float32
M32 = 0xFFFFFFFF


def lcg(s):
    return (s * 1664525 + 1013904223) & M32


def draw(seed):
    out = np.zeros(256, F)
    for i in range(256):
        seed = lcg(seed)
        out[i] = F((seed >> 8 & 0xFFFF) - 32768) / F(32768)
    return out


def expected(S, Rcap, items):
    """The program's run(S, R, items), by the restatement: the records and the live slots."""
    m = R.SpeakerManager(R.Arith(R.dot256), max_speakers=S, raw_capacity=Rcap, validate_min_magnitude=0.1)
    pick = (12345 + S * 131 + Rcap) & M32
    recs = []
    for it in range(items):
        pick = lcg(pick)
        r = pick >> 10
        v = 0 if r & 3 else (r >> 2) % (S + 2)
        scale = (F(2.0), F(0.25), F(0.015625))[(r >> 12) % 3]
        duration = 0.5 if (r >> 16) & 7 == 0 else 2.0
        e = draw(1000 + v) + draw(77777 + it) * scale
        sp = m.assign_speaker(e, duration, tick=it)
        kind, slot, dist = m.last
        recs.append((sp.id if sp is not None else 0, slot, R.KINDS.index(kind), R.bits1(dist)))
    slots = [(s, sp.id, len(sp.raws), sp.update_count, R.bits1(sp.duration), sp.created, sp.updated, R.bits(sp.current).tolist())
             for s, sp in m.speakers()]
    return recs, slots


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("speaker_db") / "speaker_db_core_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "cpu", "speaker_db_core_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    runs = []
    for l in (l.split() for l in r.stdout.splitlines()):
        if l[0] == "CONFIG":
            runs.append(dict(cfg=tuple(int(x) for x in l[1:]), recs=[], slots=[]))
        elif l[0] == "REC":
            runs[-1]["recs"].append((int(l[1]), int(l[2]), int(l[3]), int(l[4], 16)))
        elif l[0] == "SLOT":
            runs[-1]["slots"].append((int(l[1]), int(l[2]), int(l[3]), int(l[4]), int(l[5], 16), int(l[6]), int(l[7]), [int(x, 16) for x in l[8:]]))
        elif l[0] == "COS":
            runs.append(dict(cos=[int(x, 16) for x in l[1:]]))
    return runs


def test_the_program_ends_clean_and_equals_the_restatement(out):
    R.BRANCHES.clear()
    configs = [r for r in out if "cfg" in r]
    assert [r["cfg"] for r in configs] == [(1, 1, 12), (3, 3, 60), (4, 50, 260), (64, 1, 40)]
    for run in configs:
        recs, slots = expected(*run["cfg"])
        assert run["recs"] == recs, run["cfg"]
        assert run["slots"] == slots, run["cfg"]
    taken = dict(R.BRANCHES)
    print(taken)
    # the sequences fill every slot of the small tables, overflow them, wrap the ring of 50 and take each band round both thresholds
    assert all(taken.get(k, 0) > 0 for k in ("UPDATED", "DURATION_ONLY", "CREATED", "TOO_SHORT", "FULL", "ring_wrap")), taken
    assert any(len(r["slots"]) == r["cfg"][0] for r in configs[:3])
    assert max(s[2] for s in configs[2]["slots"]) == 50


def test_the_cosine_branches(out):
    cos = [r for r in out if "cos" in r][0]["cos"]
    assert cos == [R.bits1(R.INF), R.bits1(0.0)]
