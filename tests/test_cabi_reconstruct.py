"""fluidaudio::OfflineReconstruction (include/fluidaudio.hpp) from a C++ host built with g++ -Werror (tests/cabi/reconstruct_host.cpp):
the speaker database on the CPU tier; on the GPU tier the flattening of [[[Float]]] weights, the -2 padding of a ragged hardClusters,
the capacity retry past 4 096 segments and the database, all against the numpy restatement (tests/reconstruct_restatement.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reconstruct_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "reconstruct_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "reconstruct_host.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def write_input(path, w, offsets, hard_rows, centroids, fd, min_seg, min_gap, exclusive, segments=()):
    C, F, S = w.shape
    K, D = centroids.shape
    parts = [f"{C} {F} {S} {K} {D} {fd!r} {min_seg!r} {min_gap!r} {int(exclusive)} {len(offsets)} {len(hard_rows)} {len(segments)}"]
    parts.append(" ".join(f"{float(v):.9g}" for v in w.reshape(-1)))
    parts.append(" ".join(repr(float(v)) for v in offsets))
    parts += [" ".join(str(v) for v in [len(r)] + list(r)) for r in hard_rows]
    parts.append(" ".join(repr(float(v)) for v in centroids.reshape(-1)))
    parts += [f"{s[0]} {float(s[1]):.9g} {float(s[2]):.9g} {float(s[3]):.9g}" for s in segments]
    path.write_text("\n".join(parts) + "\n")


def parse(out):
    segs, db = [], {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "SEG":
            segs.append((f[1],) + tuple(int(x, 16) for x in f[2:]))
        elif f[0] == "DB":
            db[f[1]] = [int(x, 16) for x in f[2:]]
    return segs, db


def db_bits(db):
    return {k: v.view(np.uint32).tolist() for k, v in db.items()}


def test_speaker_database_on_the_host(host, tmp_path):
    rng = np.random.default_rng(2)
    cen = rng.standard_normal((5, 16))
    segs = [(f"S{int(k)}", np.float32(i), np.float32(i + 1), np.float32(0.5)) for i, k in enumerate(rng.integers(1, 8, 40))]   # S6, S7: no centroid
    p = tmp_path / "in.txt"
    write_input(p, np.zeros((1, 1, 1), np.float32), [], [], cen, 0.1, 0.0, 0.0, False, segs)
    r = subprocess.run([host, "db", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert parse(r.stdout)[1] == db_bits(R.speaker_database(segs, cen))


def bits(segs):
    return [(s[0],) + tuple(int(np.float32(v).view(np.uint32)) for v in s[1:]) for s in segs]


@pytest.mark.gpu
def test_build_on_the_device(host, tmp_path):
    rng = np.random.default_rng(4)
    C, F, S, K = 20, 1000, 3, 4
    w = (rng.random((C, F, S)) < 0.5).astype(np.float32)
    cen = rng.standard_normal((K, 8))
    offsets = np.arange(C) * 50.0                       # windows of 50 s that do not overlap: every frame flickers alone
    rows = [list(rng.integers(-2, K + 1, S)) for _ in range(C - 2)]
    rows[3] = rows[3][:2]                              # a short row and two missing chunks: -2 there
    hard = np.full((C, S), -2, np.int32)
    for c, r in enumerate(rows):
        hard[c, :len(r)] = r
    kw = dict(min_segment_duration=0.0, min_gap_duration=0.0, exclusive=False)
    want = R.build_segments(w, hard, cen, offsets, 0.05, R.config(**kw))
    assert len(want) > 4096                            # past the mirror's first capacity
    p = tmp_path / "in.txt"
    write_input(p, w, offsets, rows, cen, 0.05, 0.0, 0.0, False)
    r = subprocess.run([host, "segments", str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    segs, db = parse(r.stdout)
    assert segs == bits(want)
    assert db == db_bits(R.speaker_database(want, cen))
