"""The streaming Sortformer entries and their Swift-shaped mirror in include/fluidaudio.hpp (SortformerConfig, StreamingUpdateResult,
SortformerStreamingState) from a C++ host built with g++ -Werror (tests/cabi/sortformer_stream.cpp): the struct layouts as the compiler and
as ctypes / numpy see them, the defaults and presets, the derived integers and the two host plan functions against the restatement, and
every refusal answered without a device.  No GPU."""
import ctypes as C
import os
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sortformer_stream_restatement as R  # noqa: E402

# SortformerTypes.swift:121-216: chunkLen, left, right, fifoLen, spkcacheLen, spkcacheUpdatePeriod
PRESETS = [(6, 1, 7, 40, 188, 31), (6, 1, 7, 188, 188, 144), (340, 1, 40, 40, 188, 300), (25, 1, 7, 40, 188, 31)]


def f32hex(x):
    return f"{struct.unpack('<I', struct.pack('<f', x))[0]:08x}"


def preset(i) -> R.Config:
    chunk, lc, rc, fifo, cache, period = PRESETS[i]
    return R.Config(chunk_len=chunk, chunk_left_context=lc, chunk_right_context=rc, fifo_len=fifo, spkcache_len=cache, spkcache_update_period=period)


@pytest.fixture(scope="module")
def out(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "sortformer_stream_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cabi", "sortformer_stream.cpp"), "-o", exe, lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def rows(out, tag):
    return [l[1:] for l in out if l[0] == tag]


def test_struct_layouts(fa, out):
    L = fa._lib
    layouts = {l[0]: [int(x) for x in l[1:]] for l in rows(out, "LAYOUT")}
    cfg = L.SortformerStreamConfig
    assert layouts["config"] == [80, 0, 36, 48, 56, 76] == [C.sizeof(cfg), cfg.speakers.offset, cfg.max_index.offset, cfg.n_mels.offset, cfg.silence_threshold.offset,
                                                            cfg.min_pos_scores_rate.offset]
    assert layouts["geometry"] == [48, 12, 44] == [C.sizeof(L.SortformerStreamGeometry), L.SortformerStreamGeometry.max_pop.offset, L.SortformerStreamGeometry.lds_bytes.offset]
    assert layouts["info"] == [24, 16] == [C.sizeof(L.SortformerStreamInfo), L.SortformerStreamInfo.silence_frame_count.offset]
    dtype = fa.sortformer_stream.SORTFORMER_CHUNK_DTYPE
    assert layouts["chunk"] == [48, 0, 4, 8, 12, 16, 24, 32, 40] == [dtype.itemsize] + [dtype.fields[f][1] for f in dtype.names]


def test_defaults_presets_and_derived_integers(fa, out):
    floats = [f32hex(x) for x in (0.2, 0.25, 0.05, 0.75, 1.5, 0.5)]                              # SortformerTypes.swift:79-94
    cfgs, geos, pops = rows(out, "CFG"), rows(out, "GEO"), rows(out, "POP")
    for i, (chunk, lc, rc, fifo, cache, period) in enumerate(PRESETS):
        c = preset(i)   # the reference's own clamp lifts the high-context period of 300 to its chunk length, 340 (:254)
        assert cfgs[i] == [str(x) for x in (i, 4, 512, chunk, lc, rc, fifo, cache, c.spkcache_update_period, 3, 99999, chunk + lc + rc, 8, 128)] + floats
        assert geos[i] == [str(x) for x in (i, c.chunk_len, c.spkcache_len, c.spkcache_update_period, c.max_pop, c.score_rows, c.max_chunk_frames,
                                            (chunk + lc + rc) * 8) + c.quotas()]
        assert pops[i] == [str(i)] + [str(R.pop_out_length(c, x) if x > fifo else 0) for x in range(0, fifo + c.max_chunk_frames + 1, 3)]
    assert rows(out, "CLAMP") == [["0", "1", "16", "41"]]                                          # :239, :253-254
    py = fa.SortformerStreamConfig()
    assert [py.preset(n).c().spkcache_update_period for n in ("default", "balanced", "high_context", "efficient")] == [31, 144, 340, 31]
    d = py.c()
    assert [str(d.speakers), str(d.d_model), str(d.max_chunk_frames)] + [f32hex(getattr(d, f)) for f in ("silence_threshold", "pred_score_threshold", "scores_boost_latest",
                                                                                                           "strong_boost_rate", "weak_boost_rate", "min_pos_scores_rate")] == ["4", "512", "14"] + floats
    g = py.geometry()
    assert (g.max_pop, g.score_rows, g.spkcache_len_per_spk, g.strong_boost_per_spk, g.weak_boost_per_spk, g.min_pos_scores_per_spk) == (31, 219, 44, 33, 66, 22)
    assert fa.SORTFORMER_STREAM_STATUS.index("BAD_OPERAND") == R.BAD_OPERAND and fa.SORTFORMER_STREAM_STATUS.index("SHORT_PREDS_TENTATIVE") == R.SHORT_PREDS_TENTATIVE


def test_the_host_plan_functions_equal_the_restatement(fa, out):
    want_chunks, want_files = [], []
    for i in range(4):
        c = preset(i)
        buffered = start = 0
        for _ in range(40):
            buffered += 29
            while True:
                k = R.next_chunk_features(c, buffered, start)
                if not k.ready:
                    break
                want_chunks.append([str(x) for x in k.tuple()])
                buffered -= k.frames_to_drop
                start = k.new_start_feat
        for feat in (0, 103, 104, 1000):
            num, chunks = R.file_chunks(c, feat, feat - 20 if feat > 20 else feat)
            want_files.append(([str(feat), str(num), str(len(chunks))], [[str(x) for x in k.tuple()] for k in chunks]))
    assert rows(out, "CHUNK") == want_chunks and len(want_chunks) > 40
    assert rows(out, "FILE") == [f for f, _ in want_files]
    assert rows(out, "FCHUNK") == [k for _, ks in want_files for k in ks]
    # the same through the Python wrappers
    c = preset(0)
    got = fa.sortformer_stream_chunk_plan([50, 104, 300], [0, 0, 8])
    assert [tuple(int(x) for x in g) for g in got.tolist()] == [R.next_chunk_features(c, n, s).tuple() for n, s in ((50, 0), (104, 0), (300, 8))]
    num, chunks = fa.sortformer_stream_file_chunks(1000, 980)
    want_num, want = R.file_chunks(c, 1000, 980)
    assert num == want_num and [tuple(int(x) for x in g) for g in chunks.tolist()] == [w.tuple() for w in want]


def test_every_refusal_is_answered_without_a_device(out):
    INVALID, OK, TOO_SMALL = "1", "0", "3"
    st = {l[0]: l[1:] for l in rows(out, "ST")}
    assert st["config"] == [INVALID] * 9 + [OK, INVALID] + [INVALID, INVALID, "-1"]
    assert st["create"] == [INVALID] * 5 and st["calls"] == [INVALID] * 7
    assert st["plans"] == [INVALID] * 7
    assert st["small"] == [TOO_SMALL, str(len(R.file_chunks(preset(0), 1000, 1000)[1]))]
    assert st["preset"] == [INVALID] * 3
    assert rows(out, "THROW") == [["1"]]
