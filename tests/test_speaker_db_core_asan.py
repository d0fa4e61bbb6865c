"""fluidaudio_amd/csrc/speaker_db_core.h — the arithmetic and the state layout of the online speaker database that host and kernels share —
under the address and undefined-behaviour sanitizers: tests/cpu/speaker_db_core_main.cpp, a stand-alone program, assigns into databases
whose arrays have exactly their size (raw_capacity 1, 3 and 50), fills every slot, overflows the table and wraps the ring; it runs as a
child process and must end clean.  Every record and every current embedding it prints equals the restatement's, as bits.  It then runs
a script of management edits on tables of 1, 3 and 64 slots; the state after every step equals SpeakerManager's.  No GPU."""
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
        elif l[0] == "MANAGE":
            runs.append(dict(manage=(int(l[1]), int(l[2])), steps=[]))
        elif l[0] == "STEP":
            assert l[5] == "|" and "COUNT-MISMATCH" not in l
            slots = [tuple(int(x, 16) if i % 8 == 5 else int(x) for i, x in enumerate(l[6 + 8 * j: 14 + 8 * j])) for j in range((len(l) - 6) // 8)]
            runs[-1]["steps"].append([l[1], int(l[2]), int(l[3]), int(l[4]), slots, None])
        elif l[0] == "TEXT":
            runs[-1]["steps"][-1][5] = " ".join(l[1:])
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


def script(S, Rcap):
    """The program's manage(S, R) on the restatement: [step, status, next_id, count, [(slot, id, raws, updates, permanent, duration bits,
    created, updated)], text] after every step."""
    m = R.SpeakerManager(R.Arith(R.dot256), max_speakers=S, raw_capacity=Rcap)
    steps = []
    one = np.ones(256, F)

    def state(step, status=0, text=""):
        live = [(s, sp.id, len(sp.raws), sp.update_count, int(sp.permanent), R.bits1(sp.duration), sp.created, sp.updated) for s, sp in m.speakers()]
        assert [x[1] for x in live] == m.speaker_ids and sorted(x[1] for x in live) == sorted(m.state())
        steps.append([step, status, m.next_id, m.speaker_count, live, text])

    def upsert(id, raws, updates, permanent, duration, created, updated):
        if raws > Rcap:   # the C ABI's own refusal: the reference's ring has no such bound
            return 1, "speaker_db upsert: more raw embeddings than raw_capacity"
        ok = m.upsert_speaker(id, one, duration, [R.RawEmbedding(m.ar, one, 0)] * raws, updates, created, updated, permanent)
        return (0, "") if ok else (3, "speaker_db upsert: no free slot in stream 0")

    state("empty")
    state("upsert_new", *upsert(5, 0, 2, False, 1.5, 10, 11))
    state("upsert_existing", *upsert(5, Rcap, 7, True, 2.5, 99, 20))
    state("upsert_too_many_raws", *upsert(9, Rcap + 1, 1, False, 1.0, 0, 0))
    for i in range(S - 1):
        upsert(100 + i, i % (Rcap + 1), 1, i % 3 == 0, 0.25 * i, i, i)
    state("filled")
    state("upsert_full", *upsert(999, 0, 1, False, 1.0, 0, 0))
    m.remove_speaker(4242, True)
    state("remove_missing")
    m.remove_speaker(5, True)
    state("remove_permanent_kept")
    m.revoke_permanence(5)
    m.make_speaker_permanent(4242)
    state("revoked")
    m.remove_speaker(5, True)
    state("removed")
    state("upsert_low_id", *upsert(3, 1, 1, False, 3.0, 7, 8))
    m.make_speaker_permanent(3)
    state("made_permanent")
    m.remove_speaker(3, False)
    state("remove_permanent_forced")
    m.remove_speakers_inactive(S // 2, True)
    state("remove_inactive")
    m.reset(True)
    state("reset_keep")
    state("upsert_after_reset", *upsert(2, 0, 1, False, 1.0, 1, 1))
    m.reset(False)
    state("reset_all")
    return steps


def test_the_management_edits_equal_the_restatement(out):
    runs = [r for r in out if "manage" in r]
    assert [r["manage"] for r in runs] == [(1, 3), (3, 3), (64, 3)]
    for run in runs:
        want = script(*run["manage"])
        assert [s[0] for s in run["steps"]] == [s[0] for s in want]
        for got, exp in zip(run["steps"], want):
            assert got == exp, (run["manage"], got[0])
        by = {s[0]: s for s in run["steps"]}
        S = run["manage"][0]
        # the edges the script is for: each refusal, a table filled and emptied, speakers kept by their permanence and removed without it
        assert (by["upsert_too_many_raws"][1], by["upsert_full"][1], by["upsert_existing"][1]) == (1, 3, 0)
        assert by["filled"][3] == S and by["reset_all"][2:5] == [1, 0, []]
        assert by["remove_permanent_kept"][3] == S and by["removed"][3] == S - 1 and by["remove_permanent_forced"][3] == S - 1
        if S > 3:
            assert 0 < by["remove_inactive"][3] < by["remove_permanent_forced"][3]
            assert 0 < by["reset_keep"][3] < by["remove_inactive"][3] and by["reset_keep"][2] == max(x[1] for x in by["reset_keep"][4]) + 1
        else:
            assert by["reset_keep"][3] == (1 if S == 3 else 0) and by["reset_keep"][2] == (101 if S == 3 else 1)


def test_the_cosine_branches(out):
    cos = [r for r in out if "cos" in r][0]["cos"]
    assert cos == [R.bits1(R.INF), R.bits1(0.0)]
