"""The word spotter's host plan (fluidaudio_amd/csrc/kws_plan.h: the argument pass, the job lists, the arena rule, the passes with the
checks on what the device wrote, mergeOverlap, the delivery) walked on the CPU by tests/cpu/kws_plan.cpp, a stand-alone program built
with the address and undefined-behaviour sanitizers.  The program stands in for the device: it is given the candidates of every
(utterance, keyword) as tests/kws_restatement.py finds them without merging and serves them through the arena by the kernel's
protocol.  What it delivers equals the restatement, merged or not, at every arena and capacity.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kws_restatement as R  # noqa: E402

OK, INVALID, TOO_SMALL, RUNTIME = 0, 1, 3, 5
CHUNK = 8
BLANK = 7
UNTOUCHED = (-7, -7, 0, -7, -7)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("kws_plan") / "kws_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "kws_plan.cpp"), "-o", path], check=True)
    return path


def run(exe, words):
    r = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    out = dict(JOB=[], PASS=[], DET=[], OUT=[])
    for line in r.stdout.splitlines():
        tag, _, rest = line.partition(" ")
        if tag == "VERDICT":
            code, _, text = rest.partition(" ")
            out["VERDICT"] = (int(code), text)
        elif tag in ("DET", "OUT"):
            f = rest.split()
            out[tag].append((int(f[0]), int(f[1]), int(f[2], 16), int(f[3]), int(f[4])))
        elif tag in ("JOB", "PASS"):
            out[tag].append(tuple(int(x) for x in rest.split()))
        else:
            out[tag] = [int(x) for x in rest.split()]
    return out


def grid(seed, shape):   # scores that do not tie, so a threshold can cut behind any of a job's candidates
    return (np.float32(-8) * np.random.default_rng(seed).random(shape, np.float32)).astype(np.float32)


# ---- the spotting problem: three utterances of 70 frames (70, 64, 63 valid) and one without a valid frame; 8 columns
VALID = [70, 64, 63, 0]
WANTED_COUNTS = (0, 1, 7, 8, 9, 16, 17)


@pytest.fixture(scope="module")
def problem():
    """The keywords, the thresholds that leave utterance 0 exactly WANTED_COUNTS candidates for the first seven of them, and the
    restatement's answers: cands[u][k] unmerged (what the device would write), want[merge] the detections in the reference's order."""
    lp = grid(77, (4, 70, 8))
    rng = np.random.default_rng(3)
    kws = [[1], [2], [3], [4], [5], [6], [0], [3, 4], [], [5, R.WILDCARD], rng.integers(0, 7, 31).tolist(), rng.integers(0, 7, 32).tolist(),
           rng.integers(0, 7, 63).tolist(), rng.integers(0, 7, 64).tolist(), [0, 1, 2]]
    thr = [np.float32(-100.0)] * len(kws)
    for k, m in enumerate(WANTED_COUNTS):
        scores = sorted((c[0] for c in R.word_spot_multiple(list(lp[0, :VALID[0]]), kws[k], np.float32(-1e30), False, BLANK)), reverse=True)
        assert len(scores) > m and (m == 0 or scores[m - 1] > scores[m]), (k, m, len(scores))   # a threshold can cut behind the m-th
        thr[k] = np.float32(scores[0] + 1) if m == 0 else np.float32(scores[m - 1])
    cands = [[R.word_spot_multiple(list(lp[u, :VALID[u]]), kws[k], thr[k], False, BLANK) for k in range(len(kws))] for u in range(len(VALID))]
    want = {merge: [(u, k, R.bits(s), a, b) for u in range(len(VALID)) for k in range(len(kws))
                    for s, a, b in R.word_spot_multiple(list(lp[u, :VALID[u]]), kws[k], thr[k], merge, BLANK)] for merge in (False, True)}
    return dict(kws=kws, cands=cands, want=want)


def spot_words(problem, merge, capacity, forced, corrupt=0):
    kws, cands = problem["kws"], problem["cands"]
    words = ["spot", len(VALID), 70] + VALID + [len(kws)] + [len(k) for k in kws] + [int(merge), capacity, forced, corrupt]
    for u in range(len(VALID)):
        for k in range(len(kws)):
            words.append(len(cands[u][k]))
            for s, a, b in cands[u][k]:
                words += [R.bits(s), a, b]
    return words


def test_every_arena_delivers_the_restatement(exe, problem):
    kws, want = problem["kws"], problem["want"]
    lens = [len(k) for k in kws]
    assert {31, 32, 63, 64} <= set(lens) and 0 in lens
    for merge in (False, True):
        total = len(want[merge])
        assert total > 200 or merge
        roomy = None
        for forced in (-1, 0, 64, 200):
            got = run(exe, spot_words(problem, merge, total, forced))
            assert got["VERDICT"] == (OK, "")
            # the jobs: by utterance, then keyword, none for an empty keyword, an utterance without frames or T < n; T == n is one
            assert [j[:4] for j in got["JOB"]] == [(u, k, 0, T) for u, T in enumerate(VALID) for k, n in enumerate(lens) if n and T and T >= n]
            assert (2, lens.index(63), 0, 63) in [j[:4] for j in got["JOB"]] and (2, lens.index(64), 0, 63) not in [j[:4] for j in got["JOB"]]
            assert set(WANTED_COUNTS) <= {j[4] for j in got["JOB"]}
            cap, slice_, worst = got["ARENA"]
            assert worst == (((70 - 1 + 1) + 1) // 2 + CHUNK - 1) // CHUNK * CHUNK == 40
            J = len(got["JOB"])
            assert (cap, slice_) == {-1: (65536, 65536 // 40), 0: (40, 1), 64: (64, 1), 200: (200, 5)}[forced]
            first, later = got["PASS"][0], got["PASS"][1:]
            assert first[1] == J and all(n > 0 for n in first[2:5]) and first[7] == 1   # three width classes; order_by_class reordered
            if forced < 0:   # whole chunks, and none for a job without a candidate
                assert first[5] == 0 and not later and first[6] == sum((j[4] + CHUNK - 1) // CHUNK * CHUNK for j in got["JOB"])
            else:   # some of the first pass overflow, some do not; then passes of `slice` jobs, none of which overflows
                assert 0 < first[5] < J
                assert [p[1] for p in later] == [slice_] * (first[5] // slice_) + ([first[5] % slice_] if first[5] % slice_ else [])
                assert all(p[5] == 0 and p[6] <= cap for p in later)
            assert got["COUNT"] == [total]
            assert got["UTT"] == [sum(1 for d in want[merge] if d[0] == u) for u in range(len(VALID))]
            assert got["DET"] == want[merge], forced
            roomy = roomy or got["DET"]
            assert got["DET"] == roomy


def test_capacity(exe, problem):
    """Below, at and above the total: the counts are whole, min(total, capacity) detections are written, the rest is untouched."""
    want = problem["want"][True]
    total = len(want)
    for capacity in (0, total - 1, total, total + 3):
        got = run(exe, spot_words(problem, True, capacity, 64))
        assert got["COUNT"] == [total]
        assert got["UTT"] == [sum(1 for d in want if d[0] == u) for u in range(len(VALID))]
        assert got["DET"] == want[:capacity] + [UNTOUCHED] * max(0, capacity - total)
        assert got["VERDICT"] == ((OK, "") if capacity >= total else (TOO_SMALL, f"output holds {capacity} of {total} detections"))


def test_what_the_device_wrote_is_checked_before_it_indexes(exe, problem):
    """One corrupted pass each; the sanitizers stay silent (run() asserts it), so the check came before the index."""
    J = len(run(exe, spot_words(problem, False, 0, 64))["JOB"])
    got = run(exe, spot_words(problem, False, 0, 64, corrupt=1))
    assert got["VERDICT"] == (RUNTIME, f"a record names job {J} of {J}")
    got = run(exe, spot_words(problem, False, 0, 64, corrupt=2))
    assert got["VERDICT"] == (RUNTIME, f"a record names job {J + 5} of {J}")
    got = run(exe, spot_words(problem, False, 0, -1, corrupt=3))
    assert got["VERDICT"][0] == RUNTIME
    job, wrote, of = (int(x) for x in got["VERDICT"][1].replace("job ", "").replace(" wrote ", " ").replace(" of ", " ").replace(" records", "").split())
    assert of == wrote + 1 and 0 <= job < J, got["VERDICT"]
    got = run(exe, spot_words(problem, False, 0, 64, corrupt=4))
    assert got["VERDICT"] == (RUNTIME, "a job overflowed an arena sized for it") and len(got["PASS"]) == 2


def test_check_problem_refusals(exe):
    """The argument pass's texts, as kws_host.hip has reported them behind the entry's name."""
    #         batch frames vocab row matrix lp off tokens keywords offsets
    cases = [((-1, 4, 2, 2, 8, 1, 1, 1, 0), "bad shape"),
             ((1, 4, 0, 2, 8, 1, 1, 1, 0), "bad shape"),
             ((1, 4, 3, 2, 8, 1, 1, 1, 0), "bad shape"),
             ((1, 1, 1, 1, 1, 0, 1, 1, 0), "bad log-prob pointer or strides"),
             ((2, 3, 2, 2, 5, 1, 1, 1, 0), "bad log-prob pointer or strides"),
             ((1, 4, 2, 2, 8, 1, 0, 1, 1), "keyword_offsets is required"),
             ((1, 4, 2, 2, 8, 1, 1, 1, 1, -1, 0), "keyword_offsets starts below 0"),
             ((1, 4, 2, 2, 8, 1, 1, 1, 2, 0, 2, 1), "keyword_offsets does not ascend at keyword 1"),
             ((1, 4, 2, 2, 8, 1, 1, 1, 1, 0, 128), "keyword 0 has 128 tokens, at most 127 are supported"),
             ((1, 4, 2, 2, 8, 1, 1, 0, 1, 0, 1), "keyword_tokens is required")]
    for words, text in cases:
        assert run(exe, ("check",) + words)["VERDICT"] == (INVALID, text), words
    assert run(exe, ("check", 2, 3, 2, 2, 6, 1, 1, 1, 1, 0, 127))["VERDICT"] == (OK, "")
    assert run(exe, ("check", 1, 4, 2, 2, 8, 1, 1, 0, 2, 5, 5, 5))["VERDICT"] == (OK, "")   # no token at all: no array needed


def test_window_jobs(exe):
    """The spans of test_gpu_kws.py::test_constrained_windows: negative starts, ends beyond the valid frames, empty and inverted spans."""
    valid = [70, 44]
    lens = [1, 2, 3, 2, 3, 2, 0, 31, 33, 64]
    spans = [(-5, 100), (0, 70), (10, 30), (30, 10), (12, 12), (69, 70), (43, 46), (60, 200), (-9, 2), (5, 8), (0, 44), (3, 40), (2, 68)]
    windows = [(u, k, a, b) for u in range(2) for k in range(len(lens)) for a, b in spans]
    got = run(exe, ["window", 2, 70] + valid + [len(lens)] + lens + [len(windows)] + [x for w in windows for x in w])
    assert got["VERDICT"] == (OK, "")
    jobs, n_class = [], [0, 0, 0]
    lp = np.zeros((70, 8), np.float32)
    for w, (u, k, a, b) in enumerate(windows):
        t0, t1 = max(0, a), min(valid[u], b)
        assert got["OUT"][w] == (u, k, R.bits(-np.inf), t0, t0)
        if lens[k] and t1 > t0 and t1 - t0 >= lens[k]:
            jobs.append((u, k, t0, t1, w))
        else:   # answered without a walk, as the reference answers it
            s, st, en = R.word_spot_constrained(list(lp[:valid[u]]), [1] * lens[k], a, b, BLANK)
            assert got["OUT"][w] == (u, k, R.bits(s), st, en)
    cls = lambda j: 0 if lens[j[1]] <= 31 else (1 if lens[j[1]] <= 63 else 2)   # noqa: E731
    jobs.sort(key=lambda j: (cls(j), j[0]))   # stable: by class, within it by utterance, within that in the windows' order
    for j in jobs:
        n_class[cls(j)] += 1
    assert got["JOB"] == jobs and all(n_class)
    assert got["CLASSES"] == n_class
    assert sorted(j[4] for j in got["JOB"]) == sorted(set(j[4] for j in got["JOB"]))   # the map names each walked window once
    bad = run(exe, ["window", 2, 70] + valid + [len(lens)] + lens + [2, 0, 0, 0, 5, 2, 1, 0, 5])
    assert bad["VERDICT"] == (INVALID, "window 1 names utterance 2, keyword 1")
