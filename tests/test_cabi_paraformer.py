"""ParaformerConfig / ParaformerCif / ParaformerManager of include/fluidaudio.hpp from a C++ host built with g++ -Werror
(tests/cabi/paraformer.cpp), against the Python restatement (tests/paraformer_restatement.py): the build, the argument errors and the
text side on the CPU tier, one CIF case and one timestamp case on the GPU tier.  Floats and doubles travel as hex bits."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import paraformer_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "paraformer_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "paraformer.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def f32hex(x):
    return f"{struct.unpack('<I', struct.pack('<f', x))[0]:08x}"


def f64hex(x):
    return f"{struct.unpack('<Q', struct.pack('<d', x))[0]:016x}"


class Lcg:
    def __init__(self):
        self.x = 1

    def next(self, m):
        self.x = (1103515245 * self.x + 12345) % 2 ** 31
        return (self.x >> 16) % m


def test_argument_errors_without_a_device(host):
    r = subprocess.run([host, "args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    assert [l[1:] for l in out if l[0] == "CFG"] == [[f32hex(1.0), f32hex(0.45), "128", "512"]]
    # INVALID_ARGUMENT for every bad argument and for the good ones, which reach the missing context; INDEX_OVERFLOW for 2^25
    # utterances of 5 fire frames and for an utterance of 2^32 samples; the mirror throws what the entry answered
    assert [l[1:] for l in out if l[0] == "ST"] == [["1"] * 7, ["2"], ["1"] * 6, ["2"], ["1", "1"]]
    assert [l[1:] for l in out if l[0] == "OUT"] == [["1"]]
    vocab = {0: "<blank>", 1: "<s>", 2: "</s>", 3: "▁he", 4: "llo", 5: "cu@@", 6: "t", 7: "▁"}
    assert [l for l in r.stdout.splitlines() if l.startswith("TEXT")] == ["TEXT [" + R.decode_tokens([1, 3, 4, 0, 7, 5, 6, 2, 99], vocab) + "]"] == ["TEXT [hello cu@@t]"]
    want = R.segments_from_spans(["▁he", "llo", "cu@@", "t", "▁", "x@@"], [(-0.5, 0.1), (0.1, 0.2), (0.2, 0.3), (0.3, 0.4), (0.4, 0.5), (0.5, 0.6)])
    assert [l[1:] for l in out if l[0] == "SEG"] == [[f64hex(s), f64hex(e), t] for s, e, t in want] and [t for _, _, t in want] == ["he", "llo", "cut", "x"]


@pytest.mark.gpu
def test_cif_on_the_device(host):
    T, D = 70, 12
    r = subprocess.run([host, "cif", str(T), str(D)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    g = Lcg()
    rows = np.array([[np.float32(g.next(2001) - 1000) / np.float32(250.0) for _ in range(D)] for _ in range(T)], np.float32)
    alphas = np.array([np.float32(g.next(500)) / np.float32(1000.0) for _ in range(T)], np.float32)
    embeds, fires = R.integrate_and_fire(rows, alphas)
    assert len(fires) > 10
    assert [[int(v) for v in l[1:]] for l in out if l[0] == "FIRES"] == [fires]
    assert [l[1:] for l in out if l[0] == "EMBED"] == [[f32hex(v) for v in e] for e in embeds]
    assert [l[1:] for l in out if l[0] == "NONE"] == [["0", str(len(fires))]]


@pytest.mark.gpu
def test_timestamps_on_the_device(host):
    T = 50
    r = subprocess.run([host, "stamps", str(T)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    g = Lcg()
    alphas = np.array([np.float32(g.next(450)) / np.float32(1000.0) for _ in range(T)], np.float32)
    audio = np.zeros(T * 960, np.float32)
    for i in range(audio.size):
        noise, burst = np.float32(g.next(21) - 10) / np.float32(100000.0), np.float32(g.next(2001) - 1000) / np.float32(4000.0)
        audio[i] = burst if (i // 1600) % 2 == 0 else noise
    vocab = {0: "<blank>", 1: "<s>", 2: "</s>", 3: "▁he", 4: "llo", 5: "cu@@", 6: "t", 7: "▁", 8: ""}
    ids = [1, 3, 4, 0, 5, 6, 7, 8, 40, 4, 5, 6, 3, 2]
    trace = {}
    raw = R.raw_spans(ids, R.keep_table(vocab, 41), alphas, audio, trace)
    assert len(raw) == 9 and trace["fallback"] and len(trace["no_run"]) < 9
    assert [l[1:] for l in out if l[0] == "SPAN"] == [["0", str(i), f64hex(s), f64hex(e)] for i, s, e in raw]
    segs = R.segments_from_spans([vocab[ids[i]] for i, _, _ in raw], [(s, e) for _, s, e in raw])
    assert [l[1:] for l in out if l[0] == "SEG"] == [[f64hex(s), f64hex(e), t] for s, e, t in segs] and len(segs) < 9
    assert [l[1:] for l in out if l[0] == "EMPTY"] == [["0", "0"]]
