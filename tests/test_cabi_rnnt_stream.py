"""The Nemotron streaming session's entries and their Swift-shaped mirror in include/fluidaudio.hpp (NemotronStreamConfig,
NemotronStreamSession) from a C++ host built with g++ -Wall -Wextra -Werror (tests/cabi/rnnt_stream.cpp): the struct layouts as the
compiler and as ctypes / numpy see them, the defaults, and every refusal that needs no device; on the GPU the refusals that name their
bound and one pass of gate, track and merge through the mirror against the restatement."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import rnnt_stream_restatement as R  # noqa: E402


def f32hex(x):
    return f"{struct.unpack('<I', struct.pack('<f', x))[0]:08x}"


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "rnnt_stream_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cabi", "rnnt_stream.cpp"), "-o", exe, lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


@pytest.fixture(scope="module")
def out(host):
    r = subprocess.run([host], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def rows(out, tag):
    return [l[1:] for l in out if l[0] == tag]


def test_struct_layouts(fa, out):
    L = fa._lib
    layouts = {l[0]: [int(x) for x in l[1:]] for l in rows(out, "LAYOUT")}
    cfg, info, req = L.RnntStreamConfig, L.RnntStreamInfo, fa.rnnt_stream.RNNT_STREAM_REQUEST_DTYPE
    assert layouts["config"] == [56, 28, 40, 48] == [C.sizeof(cfg), cfg.vad_hangover_chunks.offset, cfg.total_mel_frames.offset, cfg.rescue_rms_threshold.offset]
    assert layouts["info"] == [64, 32, 60] == [C.sizeof(info), info.span_samples.offset, info.mel_cache_frames.offset]
    assert layouts["request"] == [40, 16, 24, 32] == [req.itemsize, req.fields["audio_samples"][1], req.fields["status"][1], req.fields["audio_offset"][1]]
    assert layouts["geometry"] == [16] == [C.sizeof(L.RnntStreamGeometry)]


def test_defaults(out):
    d = R.Config()
    assert rows(out, "CFG") == [[str(x) for x in (d.window_samples, d.close_silent_windows, d.pre_roll_windows, d.min_speech_windows, d.max_span_samples, d.open_slack_frames,
                                                  d.close_slack_frames, d.vad_hangover_chunks, d.mel_features, d.pre_encode_cache, 65)] + [f32hex(0.0025), f32hex(0.0)]]
    assert rows(out, "GEO") == [["241920", "3840", "1152"]]
    assert rows(out, "RMS") == [[f32hex(0.0), f32hex(2.5)]]


def test_every_refusal_is_answered_without_a_device(out):
    INVALID, OK = "1", "0"
    st = {l[0]: l[1:] for l in rows(out, "ST")}
    assert st["config"] == [INVALID] * 16 + [OK] + [INVALID, INVALID]
    assert st["null"] == [INVALID] * 13
    assert st["rms"] == [INVALID, INVALID, OK, f32hex(0.5)]


@pytest.mark.gpu
def test_one_pass_on_the_device(fa, gpu_ctx, host):
    r = subprocess.run([host, "device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    refused = {l[0]: (l[1], " ".join(l[2:])) for l in rows(out, "REFUSED")}
    assert all(status == "1" for status, _ in refused.values()) and len(refused) == 5
    assert "multiple of 4 in 4 .. 8192" in refused["window"][1] and "total_mel_frames <= 65536" in refused["total"][1] and "open_slack_frames" in refused["slack"][1]
    assert "vad_rms_threshold < 1" in refused["vad"][1] and "streams <= 65535" in refused["streams"][1]
    # the second silent chunk skips, the loud one runs; d_rms is the host emulation's
    (gate,) = rows(out, "GATE")
    assert gate[:3] == ["0", "1", "0"] and gate[3] == gate[4]
    # two pre-roll windows, two loud ones, two closing ones: frames 2, 3 -> start 0, end 4; 6 windows = 7680 samples in 2 + 1 chunks of 4480
    assert rows(out, "REQUEST") == [["0", "4", "2", "7680", "3", str(3 * 4480), str(4 * 1280 + 3 * 4480 - 6 * 1280)]]
    # the restatement: a live tag and a word at frame 40; staged tag + 6@1, punctuation@3, 7@9 (clamped to 4)
    table = np.array([0, 3, 1, 1, 1, 1, 1, 1, 1, 1], np.uint8)
    s = R.Session(R.Config(), table, ids=[1, 5], timings=[R.Timing(5, 40 * 0.08)])
    q = R.Request(0, 0, 4, 2, np.zeros(7680, np.float32))
    assert not s.commit(q, [1, 0], [2]) and s.commit(q, [1, 6, 0, 7], [1, 3, 9])
    (merge,) = rows(out, "MERGE")
    assert merge[:2] == ["0", "1"]
    text = " ".join(merge[2:])
    assert text == "| " + " ".join(str(i) for i in s.ids) + " | " + " ".join(f"{t.token_id}@{round(t.start_time / 0.08)}" for t in s.timings) + f" | 1 1 {float.hex(s.timings[0].start_time)}"
    assert [t.start_time for t in s.timings] == [f * 0.08 for f in (1, 3, 4, 40)]
    assert rows(out, "RESET") == [["0", "0"]]
