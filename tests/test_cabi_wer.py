"""WERCalculator / StringUtils of include/fluidaudio.hpp from a C++ host built with g++ -Werror (tests/cabi/wer.cpp), against the Python
restatement (tests/wer_restatement.py): the build and the argument errors on the CPU tier, a word pair and a two-panel pair on the GPU tier."""
import os
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import wer_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "wer_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "wer.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def hexbits(x):
    return f"{struct.unpack('<Q', struct.pack('<d', x))[0]:016x}"


def test_argument_errors_without_a_device(host):
    r = subprocess.run([host, "args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    # INVALID_ARGUMENT for every bad argument — and for the good ones too, which reach the missing context; INDEX_OVERFLOW for a side
    # of 2^31 symbols and for 2^31 - 1 pairs; nothing thrown across the ABI, nothing written
    assert [l[1:] for l in out if l[0] == "ST"] == [["1"] * 3, ["1"] * 8, ["2"] * 3]
    assert [l[1:] for l in out if l[0] == "OUT"] == [["1"]]


@pytest.mark.gpu
def test_pairs_on_the_device(host):
    m, n = 150, 1500
    r = subprocess.run([host, "score", str(m), str(n)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    ref, hyp = "the quick brown fox jumps over the lazy dog".split(), "the fast brown fox jumped over a lazy dog".split()
    words = R.edit_distance(hyp, ref)
    assert tuple(words) == (3, 0, 0, 3)
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "WORDS"] == [list(words)] * 2
    assert [l[1:] for l in out if l[0] == "WER"] == [[hexbits(3.0 / 9.0), "0", "0", "3", "9"], [hexbits(0.0), "0", "9", "0", "0"]]
    assert [l[1:] for l in out if l[0] == "LEV"] == [["1", "2"]]
    x, toks = 1, []
    for _ in range(m + n):
        x = (1103515245 * x + 12345) % 2 ** 31
        toks.append((x >> 16) % 3)
    a, b = toks[:m], toks[m:]
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "LONG"] == [list(R.edit_distance(a, b))]
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "SWAPPED"] == [list(R.edit_distance(b, a))]
