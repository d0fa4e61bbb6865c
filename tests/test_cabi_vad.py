"""The VAD entries and their Swift-shaped mirror in include/fluidaudio.hpp from a C++ host built with g++ -Werror (tests/cabi/vad.cpp):
the struct layouts as the compiler and as ctypes / numpy see them, the defaults, and every refusal answered without a device.  No GPU."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def f32hex(x):
    return f"{struct.unpack('<I', struct.pack('<f', x))[0]:08x}"


def f64hex(x):
    return f"{struct.unpack('<Q', struct.pack('<d', x))[0]:016x}"


@pytest.fixture(scope="module")
def out(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "vad_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cabi", "vad.cpp"), "-o", exe, lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def rows(out, tag):
    return [l[1:] for l in out if l[0] == tag]


def test_struct_layouts(fa, out):
    L = fa._lib
    layouts = {l[0]: [int(x) for x in l[1:]] for l in rows(out, "LAYOUT")}
    cfg_fields = ("default_threshold", "min_speech_duration", "min_silence_duration", "max_speech_duration", "speech_padding", "silence_threshold_for_split",
                  "has_negative_threshold", "negative_threshold", "negative_threshold_offset", "min_silence_at_max_speech", "use_max_possible_silence_at_max_speech")
    assert layouts["config"] == [72, 0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 64]
    assert layouts["config"] == [C.sizeof(L.VadSegmentationConfig)] + [getattr(L.VadSegmentationConfig, f).offset for f in cfg_fields]
    assert layouts["segment"] == [40, 0, 8, 16, 24, 32] == [C.sizeof(L.VadSegmentRecord)] + [getattr(L.VadSegmentRecord, f).offset
                                                                                         for f in ("recording", "start_sample", "end_sample", "start_time", "end_time")]
    assert layouts["state"] == [24, 0, 4, 8, 16] == [C.sizeof(L.VadStreamStateRecord)] + [getattr(L.VadStreamStateRecord, f).offset
                                                                                        for f in ("triggered", "has_temp_end", "temp_end_sample", "processed_samples")]
    assert layouts["event"] == [32, 0, 4, 8, 16, 24] == [C.sizeof(L.VadStreamEventRecord)] + [getattr(L.VadStreamEventRecord, f).offset
                                                                                            for f in ("stream", "chunk", "kind", "sample_index", "time")]
    for dtype, record in ((fa.VAD_SEGMENT_DTYPE, L.VadSegmentRecord), (fa.VAD_STREAM_STATE_DTYPE, L.VadStreamStateRecord), (fa.VAD_STREAM_EVENT_DTYPE, L.VadStreamEventRecord)):
        assert dtype.itemsize == C.sizeof(record) and all(dtype.fields[name][1] == getattr(record, name).offset for name, _ in record._fields_)


def test_defaults(fa, out):
    default = [f32hex(0.85), f64hex(0.15), f64hex(0.75), f64hex(14.0), f64hex(0.1), f32hex(0.3), "0", f32hex(0.0), f32hex(0.15), f64hex(0.098), "1"]    # VadTypes.swift:13, 37-47
    override = [f32hex(0.8), f64hex(0.15), f64hex(0.75), f64hex(math.inf), f64hex(0.1), f32hex(0.3), "1", f32hex(0.2), f32hex(0.05), f64hex(0.098), "1"]
    assert rows(out, "CFG") == [default, default, override]
    cfg = fa.vad_config()
    assert [f32hex(cfg.default_threshold), f64hex(cfg.min_speech_duration), f64hex(cfg.min_silence_duration), f64hex(cfg.max_speech_duration), f64hex(cfg.speech_padding),
            f32hex(cfg.silence_threshold_for_split), str(cfg.has_negative_threshold), f32hex(cfg.negative_threshold), f32hex(cfg.negative_threshold_offset),
            f64hex(cfg.min_silence_at_max_speech), str(cfg.use_max_possible_silence_at_max_speech)] == default
    assert rows(out, "NEG") == [[f32hex(float(np.float32(0.85) - np.float32(0.15))), f32hex(0.2)]]
    assert rows(out, "SEG") == [["1000", "2000", "1000"]]                        # VadSegment.startSample goes through fp64 seconds
    assert rows(out, "CHUNKS") == [["0", "0", "1", "1", "2"]]


def test_every_refusal_is_answered_without_a_device(out):
    INVALID, OVERFLOW, TOO_SMALL = "1", "2", "3"
    # the eight preconditions, a NaN duration, two products beyond Int; the good config reaches the missing context
    assert rows(out, "ST") == [["config"] + [INVALID] * 12,
                               ["segments"] + [INVALID] * 8 + [OVERFLOW],
                               ["pack"] + [INVALID] * 5 + [TOO_SMALL, "|", "0", "1", "2"],      # the ranges are written before the capacity is judged
                               ["gather"] + [INVALID] * 6 + [TOO_SMALL, "|", "0", "5", "4101"],
                               ["stream"] + [INVALID] * 9]
    assert rows(out, "COUNT") == [["-7"]]
    assert rows(out, "THROW") == [["1"]]
