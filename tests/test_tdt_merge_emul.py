"""The seam merge's device code walked on the CPU (tests/cpu/tdt_merge_emul.cpp over csrc/tdt_merge_core.h and
csrc/tdt_merge_launch.h, the code the kernel is built from, with a wave of one lane) against the restatement
(tests/tdt_merge_restatement.py) on the batches of the device tests (tests/tdt_merge_cases.py): every field, count, status and route.
The program is stand-alone and is built with the address and undefined-behaviour sanitizers; each of its buffers has exactly the size
the plan promises and starts out poisoned.  Every batch runs twice: with the LDS limit of the kernel and with a limit of 4 tokens a
side, which sends nearly every seam through the workspace route.  No GPU."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tdt_merge_cases as K  # noqa: E402
import tdt_merge_restatement as R  # noqa: E402


def build(exe, flags):
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags,
                    os.path.join(HERE, "cpu", "tdt_merge_emul.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("tdt_merge") / "tdt_merge_emul"), ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def text_of(batch, lds_side=-1):
    p = K.pack(batch)
    out = [f"{len(batch.recs)} {batch.vocab} {int(p.safe is not None)} {int(p.canon is not None)} {lds_side} {p.max_out} {R.FRAME.hex()} {float(batch.overlap).hex()}"]
    if p.safe is not None:
        out.append(" ".join(str(int(v)) for v in p.safe))
    if p.canon is not None:
        out.append(" ".join(str(int(v)) for v in p.canon))
    at = 0
    for r, rec in enumerate(batch.recs):
        out.append(f"{int(p.caps[r])} {len(rec)}")
        for w in rec:
            out.append(f"{int(p.counts[at])} {len(w)}")
            out.extend(f"{t[0]} {t[1]} {t[2]} {bits(t[3])}" for t in w)
            at += 1
    return "\n".join(out) + "\n"


def run(emul, batch, lds_side=-1):
    r = subprocess.run([emul], input=text_of(batch, lds_side), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    got, at = [], 0
    while at < len(lines):
        head = lines[at].split()
        assert head[0] == "R", lines[at]
        status, count = int(head[1]), int(head[2])
        toks = [tuple(int(v) for v in l.split()) for l in lines[at + 1:at + 1 + count]]
        routes = [int(v) for v in lines[at + 1 + count].split()[1:]]
        got.append((toks, status, routes))
        at += count + 2
    return got


def same(batch, got):
    want = K.expected(batch)
    assert len(got) == len(want)
    for r, ((toks, status, routes), (w_toks, w_status, w_routes)) in enumerate(zip(got, want)):
        assert (status, routes) == (w_status, w_routes), (batch.name, r)
        assert toks == [(t[0], t[1], t[2], bits(t[3])) for t in w_toks], (batch.name, r)


@pytest.mark.parametrize("lds_side", [-1, K.SMALL_LDS_SIDE])
def test_every_batch_matches_the_restatement(emul, lds_side):
    for batch in K.all_batches():
        same(batch, run(emul, batch, lds_side))


def test_zero_recordings_and_the_argument_pass(emul):
    assert run(emul, K.Batch("none", [], None, None, 0, R.OVERLAP)) == []
    bad = K.Batch("bad", [[[K.tok(1, 1)]]], None, None, 4, -1.0)
    r = subprocess.run([emul], input=text_of(bad), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[:2] == ["CHECK", "1"]
