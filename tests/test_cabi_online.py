"""The online speaker database's entries and their Swift-shaped mirror in include/fluidaudio.hpp (SpeakerUtilities, RawEmbedding, Speaker,
SpeakerManager) from a C++ host built with g++ -Werror (tests/cabi/online.cpp): the struct layouts as the compiler and as ctypes / numpy
see them, the defaults, the arithmetic entries against the restatement as bits, and every refusal answered without a device.  No GPU."""
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
import online_restatement as R  # noqa: E402

F = np.float32


def f32hex(x):
    return f"{struct.unpack('<I', struct.pack('<f', x))[0]:08x}"


def distinct(pattern):
    return np.sin(((np.arange(256) + pattern * 100).astype(F) * F(0.1)).astype(np.float64)).astype(F)


def build_host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "online_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cabi", "online.cpp"), "-o", exe, lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


@pytest.fixture(scope="module")
def out(fa, tmp_path_factory):
    r = subprocess.run([build_host(fa, tmp_path_factory)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def rows(out, tag):
    return [l[1:] for l in out if l[0] == tag]


def test_struct_layouts(fa, out):
    L = fa._lib
    layouts = {l[0]: [int(x) for x in l[1:]] for l in rows(out, "LAYOUT")}
    assert layouts["config"] == [28, 0, 4, 8, 12, 16, 20, 24] == [C.sizeof(L.SpeakerDbConfig)] + [getattr(L.SpeakerDbConfig, f).offset for f, _ in L.SpeakerDbConfig._fields_]
    assert layouts["info"] == [40, 0, 4, 8, 12, 16, 20, 24, 32] == [C.sizeof(L.SpeakerInfo)] + [getattr(L.SpeakerInfo, f).offset for f, _ in L.SpeakerInfo._fields_]
    for name, dtype in (("assignment", fa.SPEAKER_ASSIGNMENT_DTYPE), ("pair", fa.SPEAKER_PAIR_DTYPE)):
        assert layouts[name] == [dtype.itemsize] + [dtype.fields[f][1] for f in dtype.names]


def test_defaults(fa, out):
    default = [f32hex(0.65), f32hex(0.45), f32hex(1.0), f32hex(0.9), f32hex(-1.0), "16", "50"]     # SpeakerManager.swift:45-50, :452; SpeakerTypes.swift:111
    assert rows(out, "CFG") == [default]
    cfg = fa.SpeakerDbConfig().c()
    assert [f32hex(cfg.speaker_threshold), f32hex(cfg.embedding_threshold), f32hex(cfg.min_speech_duration), f32hex(cfg.ema_alpha), f32hex(cfg.validate_min_magnitude),
            str(cfg.max_speakers), str(cfg.raw_capacity)] == default
    assert fa.SPEAKER_KINDS == R.KINDS


def test_the_arithmetic_entries_equal_the_restatement(fa, out):
    ar = R.Arith(R.dot256)
    assert rows(out, "NORM") == [[f"{b:08x}" for b in R.bits(ar.l2_normalize(distinct(p)))] for p in (1, 2, 3)]
    n1, n3 = ar.l2_normalize(distinct(1)), ar.l2_normalize(distinct(3))
    inf = f"{R.bits1(R.INF):08x}"
    assert rows(out, "COS") == [[f"{R.bits1(ar.cosine_distance(distinct(1), distinct(2))):08x}", f"{R.bits1(ar.cosine_distance(n1, n3)):08x}", inf, inf,
                                 f"{R.bits1(R.RawEmbedding(ar, distinct(2)).embedding[7]):08x}"]]
    assert rows(out, "VALID") == [["1", "0", "0", "1", "0"]]                                     # testValidateEmbedding, and a NaN
    assert R.bits(fa.speaker_l2_normalize(distinct(2))).tolist() == R.bits(ar.l2_normalize(distinct(2))).tolist()
    assert R.bits1(fa.speaker_cosine_distance(n1, distinct(2))) == R.bits1(ar.cosine_distance(n1, distinct(2)))
    assert fa.speaker_cosine_distance(n1, np.zeros(128, F)) == np.inf and fa.speaker_validate_embedding(distinct(1)) and not fa.speaker_validate_embedding(np.zeros(256, F))


def test_every_refusal_is_answered_without_a_device(out):
    INVALID = "1"
    assert rows(out, "ST") == [["create"] + [INVALID] * 7, ["calls"] + [INVALID] * 14, ["null", INVALID, f"{R.bits1(R.INF):08x}", "0"]]
    assert rows(out, "THROW") == [["1"]]
