"""The offline Sortformer / timeline mirrors of include/fluidaudio.hpp (csrc/sortformer_host.hip, csrc/timeline_host.hip) from a C++ host built
with g++ -Werror (tests/cabi/sortformer_host.cpp), against the numpy restatement (tests/sortformer_restatement.py): geometry, alignment,
rounding and statuses on the CPU tier; DiarizerTimeline::rebuild on the GPU tier."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sortformer_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "sortformer_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "sortformer_host.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def fmt(x):
    return " ".join(f"{float(v):.9g}" for v in np.asarray(x, np.float32).reshape(-1))


def test_host_side_without_a_device(host, tmp_path):
    rng = np.random.default_rng(1)
    cfg = R.OfflineConfig()
    lengths = [3072, 1, 0, 2273, 7 * 2272 + 5]
    aligns = []
    for s in (4, 4, 3, 2, 1):
        n = int(rng.integers(1, 30))
        g = (rng.random((n, s)) * (rng.random((n, s)) < 0.8)).astype(np.float32)
        aligns.append((n, s, g, rng.random((n, s)).astype(np.float32)))
    aligns[1][3][:, 2] = aligns[1][3][:, 0]              # an exact tie
    lines = [f"{cfg.window_output_frames} {cfg.subsampling} {cfg.overlap_output_frames} {len(lengths)} " + " ".join(map(str, lengths))]
    lines += [f"{n} {s} {fmt(g)} {fmt(w)}" for n, s, g, w in aligns]
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([host, "host", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    want_win, want_rec = [], []
    for b, n in enumerate(lengths):
        wins, total = R.offline_windows(cfg, n)
        want_rec.append([total, len(want_win), len(want_win) + len(wins)])
        want_win += [[b, w["valid_mel"], w["valid_out"], int(i == 0), w["mel_start"], w["g_start"]] for i, w in enumerate(wins)]
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "WIN"] == want_win
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "REC"] == want_rec
    assert [l[1:] for l in out if l[0] == "CFG"] == [["3072", f"{int(np.float32(cfg.frame_duration_seconds).view(np.uint32)):08x}"]]
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "MAP"] == [R.alignment(g, w, n, s) for n, s, g, w in aligns]
    t = R.TimelineConfig.from_seconds(1, 0.08, 0.5, 0.5, 0.12, 0.2, 0.04, 0.36)
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "SEC"] == [[t.onset_pad_frames, t.offset_pad_frames, t.min_frames_on, t.min_frames_off]]
    assert [l[1:] for l in out if l[0] == "ST"] == [["1", "1", "1"], ["1", "1"], ["1"]]   # INVALID_ARGUMENT everywhere, nothing thrown across the ABI


@pytest.mark.gpu
def test_rebuild_on_the_device(host, tmp_path):
    rng = np.random.default_rng(2)
    s = 3
    x = np.cumsum(rng.normal(0, 0.08, (6000, s)), axis=0)
    p = np.abs(((x + 1) % 2) - 1).astype(np.float32)
    p[-30:, 1] = 0.9                                      # still speaking at the end
    rcfg = R.TimelineConfig(s, 0.08, 0.6, 0.45, 2, 3, 4, 5)
    for complete, nt in ((1, 700), (0, 700), (1, 0)):
        fin, tent = p[:len(p) - nt], p[len(p) - nt:]
        f = tmp_path / "tl.txt"
        f.write_text(f"{s} {float(np.float32(0.6)):.9g} {float(np.float32(0.45)):.9g} 2 3 4 5 {complete} {len(fin)} {len(tent)}\n{fmt(fin)}\n{fmt(tent)}\n")
        r = subprocess.run([host, "timeline", str(f)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        got = [(int(l[1]), int(l[2]), int(l[3]), int(l[4], 16), int(l[5]), int(l[6], 16), int(l[7], 16)) for l in (x.split() for x in r.stdout.splitlines())]
        t = R.Timeline(rcfg)
        t.rebuild(fin, tent, bool(complete))
        fd = np.float32(0.08)
        want = [(w[1], w[2], w[3], w[4], w[5] & 1, int(np.float32(np.float32(w[2]) * fd).view(np.uint32)), int(np.float32(np.float32(w[3]) * fd).view(np.uint32)))
                for w in t.records()]
        assert got == want and len(want) > 20
