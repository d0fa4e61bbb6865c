"""fluidaudio_amd/csrc/rnnt_bias_core.h — the bias tables' builder and the bounds-checked accessors host and kernel share — under the
address and undefined-behaviour sanitizers: tests/cpu/rnnt_bias_core_main.cpp, a stand-alone program, builds tables into buffers of
exactly their size, walks them, and walks truncated and bit-flipped copies; it runs as a child process and must end clean.  The
candidates it prints equal the restatement's.  This is where malformed blobs are exercised: no GPU test feeds the kernel one.  No GPU."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rnnt_restatement as R  # noqa: E402

PIECES = {0: "▁", 1: "▁to", 2: "r", 3: "vane", 4: "▁tor", 5: "▁torvane", 6: "▁the", 7: "▁the", 8: "▁ran", 9: "▁t", 10: "▁cr", 11: "an", 13: "东", 14: "京",
          15: "<unk>", 16: "▁ab", 17: "▁c", 18: "v", 19: "q" * 12}
TERMS = [("torvane", 2.0), ("ab ab c", 4.5), ("东京", 4.5), ("the", 5.5), ("torment", 5.0)]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rnnt_bias") / "rnnt_bias_core_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "rnnt_bias_core_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return [l.split() for l in r.stdout.splitlines()]


def test_tables_walk_clean_and_equal_the_restatement(out):
    ref = R.VocabularyBias(TERMS, PIECES)
    built = [l for l in out if l[0] == "BUILT"]
    assert len(built) == 1 and int(built[0][2]) == ref.tail_cap == 8
    states = [l for l in out if l[0] == "CAND"]
    assert len(states) == 10
    for l in states:
        sep = l.index(":")
        observed = [int(x) for x in l[1:sep]]
        got = {int(x.split("=")[0]): float(x.split("=")[1]) for x in l[sep + 1:]}
        ref.reset_match_state()
        for i in observed:
            ref.observe(i)
        assert got == {i: float(b) for i, b in ref.candidates().items()}, observed
    assert any(len(l) - l.index(":") > 6 for l in states)


def test_malformed_blobs_are_refused_or_walked_in_bounds(out):
    line = [l for l in out if l[0] == "MALFORMED"]
    assert len(line) == 1
    refused, walked = int(line[0][2]), int(line[0][4])
    assert refused > 1000 and walked > 1000          # both outcomes occur: a flipped boost walks, a flipped offset is refused
