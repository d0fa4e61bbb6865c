"""The FSMN-VAD entries and their Swift-shaped mirror in include/fluidaudio.hpp from a C++ host built with g++ -Werror
(tests/cabi/fsmn_vad.cpp): the struct layouts as the compiler and as ctypes / numpy see them, the defaults, every refusal answered
without a device, and the ranges written before a capacity is judged.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def f32hex(x):
    return f"{struct.unpack('<I', struct.pack('<f', x))[0]:08x}"


@pytest.fixture(scope="module")
def out(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "fsmn_vad_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cabi", "fsmn_vad.cpp"), "-o", exe, lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def rows(out, tag):
    return [l[1:] for l in out if l[0] == tag]


def test_struct_layouts(fa, out):
    L = fa._lib
    layouts = {l[0]: [int(x) for x in l[1:]] for l in rows(out, "LAYOUT")}
    assert layouts["config"] == [36] + list(range(0, 36, 4)) == [C.sizeof(L.FsmnVadConfig)] + [getattr(L.FsmnVadConfig, f).offset for f, _ in L.FsmnVadConfig._fields_]
    assert layouts["chunk"] == [40, 0, 4, 8, 16, 24, 28, 32] == [C.sizeof(L.FsmnVadChunkRecord)] + [getattr(L.FsmnVadChunkRecord, f).offset for f, _ in L.FsmnVadChunkRecord._fields_]
    assert layouts["segment"] == [32, 0, 4, 8, 12, 16, 24] == [C.sizeof(L.FsmnVadSegmentRecord)] + [getattr(L.FsmnVadSegmentRecord, f).offset
                                                                                                   for f, _ in L.FsmnVadSegmentRecord._fields_]
    for dtype, record in ((fa.fsmn_vad.FSMN_VAD_CHUNK_DTYPE, L.FsmnVadChunkRecord), (fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE, L.FsmnVadSegmentRecord)):
        assert dtype.itemsize == C.sizeof(record) and all(dtype.fields[name][1] == getattr(record, name).offset for name, _ in record._fields_)


def test_defaults(fa, out):
    default = [f32hex(0.2), "20", "15", "15", "80", "20", "10", "6000", "10"]                   # FsmnVadManager.swift:37-45
    assert rows(out, "CFG") == [default, default]
    cfg = fa.fsmn_vad_config()
    assert [f32hex(cfg.silence_threshold)] + [str(getattr(cfg, f)) for f, _ in fa._lib.FsmnVadConfig._fields_[1:]] == default
    assert rows(out, "FRAMES") == [["0", "0", "3", "3048"]]
    assert rows(out, "MIRROR") == [["2", "3093", "47", "2", "3048"]]


def test_every_refusal_is_answered_without_a_device(out):
    INVALID, OVERFLOW, TOO_SMALL = "1", "2", "3"
    # the twelve bounds of the config; the good config reaches the missing context
    assert rows(out, "ST") == [["config"] + [INVALID] * 13,
                               ["segments"] + [INVALID] * 7 + [OVERFLOW],
                               # the ranges and the count are written before the capacity is judged, and so are the first `capacity` records
                               ["plan"] + [INVALID] * 3 + [TOO_SMALL, "|", "2", "|", "0", "2", "2", "|", "0", "3093", "3093", "|", "488320"],
                               ["plan0", "0", "0"],
                               ["pack"] + [INVALID] * 8 + [TOO_SMALL],
                               ["feats"] + [INVALID] * 5,
                               ["gather"] + [INVALID] * 5 + [TOO_SMALL]]
    assert rows(out, "COUNT") == [["-7"]]
    assert rows(out, "THROW") == [["1"]]
