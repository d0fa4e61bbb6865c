"""DiarizationDER::compute of include/fluidaudio.hpp from a C++ host built with g++ -Werror (tests/cabi/der.cpp), against the Python
restatement (tests/der_restatement.py): the build and the argument errors on the CPU tier, the two-speaker case on the GPU tier."""
import os
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import der_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "der_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "der.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def hexbits(x):
    return f"{struct.unpack('<Q', struct.pack('<d', x))[0]:016x}"


def test_argument_errors_without_a_device(host):
    r = subprocess.run([host, "args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    # INVALID_ARGUMENT for every bad argument — and for the good ones too, which reach the missing context; nothing thrown across the ABI
    assert [l[1:] for l in out if l[0] == "ST"] == [["1"] * 7, ["1", "1"]]
    assert [l[1:] for l in out if l[0] == "CFG"] == [[hexbits(0.01), hexbits(0.0)]]


@pytest.mark.gpu
@pytest.mark.parametrize("collar", [0.0, 0.5])
def test_compute_on_the_device(host, collar):
    r = subprocess.run([host, "score", "0.01", repr(collar)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    w = R.compute(*R.CASE1, 0.01, collar)
    assert [l[1:] for l in out if l[0] == "DER"] == [[hexbits(v) for v in (w.der, w.confusion, w.false_alarm, w.miss, w.total_ref_speech)]]
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "CNT"] == [[w.frames, *w.counts, 2, 2]]
    assert {l[1]: l[2] for l in out if l[0] == "MAP"} == w.mapping == {"x": "A", "y": "B"}
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "OV"] == [[1000, 200, 0, 800]]
    assert w.counts == ((0, 0, 175, 1900) if collar else (0, 0, 200, 2000))
