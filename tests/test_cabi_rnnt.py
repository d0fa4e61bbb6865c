"""The streaming RNN-T entries and their Swift-shaped mirror in include/fluidaudio.hpp (RnntConfig, NemotronVocabularyBias: observe,
candidates, resetMatchState) from a C++ host built with g++ -Wall -Wextra -Werror (tests/cabi/rnnt.cpp): the mirror against the
restatement, the defaults, and every refusal answered without a device.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import rnnt_restatement as R  # noqa: E402

PIECES = {0: "▁", 1: "▁to", 2: "r", 3: "vane", 4: "▁tor", 5: "▁torvane", 6: "▁The", 7: "▁the", 8: "▁ran", 9: "▁t", 10: "▁cr", 11: "an",
          18: "<unk>", 19: "<en-US>", 21: "▁ab", 22: "▁c", 23: "v", 24: "▁vor"}


@pytest.fixture(scope="module")
def out(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "rnnt_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cabi", "rnnt.cpp"), "-o", exe, lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return {l.split()[0] + ("_" + l.split()[1] if l.startswith("ST ") else ""): l.split()[(2 if l.startswith("ST ") else 1):] for l in r.stdout.splitlines()}


def test_defaults(fa, out):
    assert out["CFG"] == ["1024", "-1", "10", "1024", "-1", "10", "12"] and C.sizeof(fa._lib.RnntConfig) == 12
    cfg = fa.RnntConfig()
    assert (cfg.blank_id, cfg.eou_id, cfg.max_symbols_per_step) == (1024, -1, 10)
    assert out["BOOST"] == ["4.5", "4.5", "6", "5.5", "3"]


def test_mirror_equals_the_restatement(out):
    ref = R.VocabularyBias([("torvane", None, ("vortane",)), ("ab ab c", 5.5)], PIECES)
    assert out["CAP"] == [str(ref.tail_cap), "1"]

    def want():
        return [f"{i}={float(b):g}" for i, b in sorted(ref.candidates().items())]

    assert out["FRESH"] == want()
    for i in (4, 19, 12, 99, -1):
        ref.observe(i)
    assert out["TOR"] == want() and "3=4.5" in out["TOR"] and "23=4.5" in out["TOR"]
    ref.observe(7)
    assert out["THE"] == want() and "3=4.5" not in out["THE"]
    for _ in range(40):
        ref.observe(21)
    assert out["ABAB"] == want() and "22=5.5" in out["ABAB"]
    ref.reset_match_state()
    assert out["RESET"] == want() == out["FRESH"]
    assert out["NONE"] == ["0", "0", "0"] and out["THROWN"] == ["3"]


def test_every_refusal_is_answered_without_a_device(out):
    INVALID, TOO_SMALL, OK = "1", "3", "0"
    assert out["ST_build"] == [INVALID] * 6 + ["-7", "-7", TOO_SMALL, OK, "0"]
    assert out["ST_candidates"] == [INVALID] * 4
    assert out["ST_greedy"] == [INVALID, INVALID]
