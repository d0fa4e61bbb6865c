"""CtcKeywordSpotter of include/fluidaudio.hpp from a C++ host built with g++ -Werror (tests/cabi/kws.cpp), against the Python restatement
(tests/kws_restatement.py): the build, the argument errors and the threshold rule on the CPU tier, a five-frame utterance on the GPU tier."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kws_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "kws_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "kws.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def hex32(x):
    return f"{R.bits(x):08x}"


def hex64(x):
    return f"{struct.unpack('<Q', struct.pack('<d', x))[0]:016x}"


def test_argument_errors_without_a_device(host):
    r = subprocess.run([host, "args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    # INVALID_ARGUMENT for the bad arguments — and for the good ones, which reach the missing context; nothing thrown across the ABI
    assert [l[1:] for l in out if l[0] == "ST"] == [["1"] * 4, ["1"] * 4]
    assert [l[1:] for l in out if l[0] == "COUNT"] == [["0"]]   # *count is set whatever the status
    f = np.float32
    want = [f(-15.0), f(-8.5), f(f(-8.5) - f(7.0)), f(f(-0.1) - f(1.0)), f(f(16777216.0) - f(1.0))]
    assert [l[1:] for l in out if l[0] == "THR"] == [[hex32(v) for v in want]]
    assert [hex32(R.adjusted_threshold(b, n)) for b, n in ((None, 9), (-8.5, 3), (-8.5, 10), (-0.1, 4), (16777216.0, 4))] == [hex32(v) for v in want]


@pytest.mark.gpu
def test_spotter_on_the_device(host):
    r = subprocess.run([host, "spot"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    hi, bl, cold = -0.1, -0.5, -10.0
    lp = [np.asarray(row, np.float32) for row in ([hi, cold, cold, bl], [cold, cold, cold, bl], [cold, cold, cold, bl], [cold, cold, cold, bl], [cold, hi, cold, bl])]
    terms = [[0, 1], [], [0, R.WILDCARD, 1], [1, 0], [0, 1, 0, 1]]
    want = R.spot_keywords(lp, terms, min_score=-6.0, blank_id=3, frame_duration=0.08)
    assert [l[1:] for l in out if l[0] == "DET"] == [[str(k), hex32(s), "5", str(a), str(b), hex64(ta), hex64(tb)] for k, s, a, b, ta, tb in want]
    assert {k for k, *_ in want} >= {0, 2}
    assert [l[1:] for l in out if l[0] == "MUL"] == [[hex32(s), str(a), str(b)] for s, a, b in R.word_spot_multiple(lp, [0], -100.0, False, 3)]
    con = [R.word_spot_constrained(lp, [0, 1], 0, 5, 3), R.word_spot_constrained(lp, [0, 1], 4, 9, 3)]
    assert [l[1:] for l in out if l[0] == "CON"] == [[hex32(s), str(a), str(b)] for s, a, b in con]
    assert abs(float(con[0][0]) + 0.85) <= 0.01 and np.isneginf(con[1][0])
