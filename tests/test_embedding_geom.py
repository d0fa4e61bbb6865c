"""The host arithmetic of the embedding inputs (csrc/embedding_geom.h: the config's geometry, the planned windows, the span geometry, the
slice check) walked on the CPU by tests/cpu/embedding_geom.cpp against the numpy restatement (tests/embedding_restatement.py).  The
program is stand-alone, reads its cases from stdin and is built with the address and undefined-behaviour sanitizers.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import embedding_restatement as E  # noqa: E402


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("embedding_geom") / "embedding_geom")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "embedding_geom.cpp"), "-o", exe], check=True)
    return exe


def run(geom, *words):
    r = subprocess.run([geom], input=" ".join(w.hex() if isinstance(w, float) else str(w) for w in words) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return [line.split() for line in r.stdout.splitlines()]


def windows(geom, C, offsets, total, cfg, F=589, fd=0.0):
    offsets = [] if offsets is None else [float(v) for v in offsets]
    out = run(geom, "windows", cfg.sample_rate, float(cfg.window_duration), cfg.samples_per_window, cfg.batch_size, cfg.weight_frames, float(fd),
              float(cfg.min_segment_duration), F, C, total, len(offsets), *offsets)
    head, rows = out[0], out[1:]
    assert int(head[5]) == len(rows)
    return head, [(int(c), float.fromhex(o), int(s)) for c, s, o in rows]


CASES = {
    "rounding": (3, [0.00003125, math.nan, 5.0], 16000 * 30, {}),                       # half a sample rounds away from zero; NaN -> c * window
    "fewer_offsets": (6, [0.0, 2.0], 16000 * 100, {}),
    "negative_and_inf": (6, [-1.0, -0.00003125, math.inf, -math.inf, 7.5, 1e300], 16000 * 55 + 3, {}),
    "starts_at_total": (4, [0.0, 10.0, 20.0, 30.0], 16000 * 20, {}),                    # chunk 2 starts exactly at total_samples: not planned
    "no_audio": (5, None, 0, {}),
    "spw_override": (5, [0.0, 1.0, 2.0, 3.0, 3.9], 16000 * 4, {"samples_per_window": 8000}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_planned_windows_equal_the_restatement(geom, name):
    C, offsets, total, kw = CASES[name]
    cfg = E.Config(**kw)
    head, got = windows(geom, C, offsets, total, cfg)
    want = E.chunk_plan(C, offsets, total, cfg)
    assert [(c, s) for c, _, s in got] == [(c, s) for c, _, s in want]
    assert [o.hex() for _, o, _ in got] == [float(o).hex() for _, o, _ in want]
    assert (int(head[0]), int(head[1]), int(head[2])) == (cfg.spw, cfg.weight_frames, 32)
    assert float.fromhex(head[3]) == cfg.window_duration / 589 and int(head[4]) == math.ceil(1.0 / (cfg.window_duration / 589))
    if name == "starts_at_total":
        assert [c for c, _, _ in got] == [0, 1]
    if name == "no_audio":
        assert got == []
    if name == "rounding":
        assert [s for _, _, s in got] == [1, 160000, 80000]


def test_geometry_of_a_config(geom):
    """batch clamp, a configured frame duration, the min-frames clamp."""
    for batch, fd, min_seg, want_b, want_mf in ((0, 0.0, 1.0, 1, 59), (64, 0.02, 3.0, 32, 150), (7, 0.0, -5.0, 7, 1), (7, 1e-12, 1.0, 7, 2**31 - 1)):
        cfg = E.Config(batch_size=batch, min_segment_duration=min_seg)
        head, _ = windows(geom, 1, None, 16000, cfg, fd=fd)
        assert (int(head[2]), int(head[4])) == (want_b, want_mf)
        assert float.fromhex(head[3]) == (fd if fd > 0 else 10.0 / 589)


def test_span_geometry_equals_the_restatement(geom):
    total = 16000 * 33 + 77
    audio = np.arange(1, total + 1, dtype=np.float32)               # sample i holds i + 1: a window's content names its start and length
    spans = [(1.0, 3.5), (5.0, 5.0), (30.0, 45.0), (0.00003125, 0.5), (-1.0, 0.25), (20.0, 40.0), (40.0, 41.0),
             (1.0, math.nan), (math.nan, 2.0), (1.0, math.inf), (-math.inf, 2.0), (-1e300, 1e300), (1e300, 2e300), (-2e300, -1e300), (0.0, 1e300),
             (3.0, 2.0), (1.0, 1.00003), (1.0, 1.00004)]          # end < start; 0.48 of a sample rounds to none, 0.64 to one
    cfg = E.Config()
    win, wts, ok = E.span_inputs(audio, spans, cfg)
    got = run(geom, "spans", cfg.sample_rate, float(cfg.window_duration), cfg.samples_per_window, cfg.weight_frames, total, len(spans), *[float(v) for sp in spans for v in sp])
    assert len(got) == len(spans)
    for i, (g, sp) in enumerate(zip(got, spans)):
        g_ok, start, n, active = (int(v) for v in g)
        assert bool(g_ok) == bool(ok[i]), sp
        assert n == int(np.count_nonzero(win[i])) and active == int(wts[i].sum()), sp
        assert start == (int(win[i, 0]) - 1 if ok[i] else 0), sp
    assert ok.tolist() == [True, False, True, True, True, True, False, False, False, False, False, True, False, False, True, False, False, True]


def test_slice_check(geom):
    assert [run(geom, "slice", s, 1000)[0][0] for s in (-1, 0, 999, 1000, 1001)] == ["0", "1", "1", "1", "0"]
    assert run(geom, "slice", 0, 0)[0][0] == "1" and run(geom, "slice", 1, 0)[0][0] == "0"
