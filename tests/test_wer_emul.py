"""The edit-distance kernel's schedule walked on the CPU (tests/cpu/wer_emul.cpp over csrc/wer_core.h and csrc/wer_launch.h, the code
the kernel is built from) against the restatement with the full table and the traceback (tests/wer_restatement.py): every class, the
two- and three-panel routes, the 64-step refills.  The program is stand-alone and is built with the address and undefined-behaviour
sanitizers; it also ends on any workspace entry read before this run wrote it.  No GPU."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wer_cases as W  # noqa: E402
import wer_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wer") / "wer_emul")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "wer_emul.cpp"), "-o", exe], check=True)
    return exe


def run(emul, pairs):
    text = [str(len(pairs))]
    for hyp, ref in pairs:
        text.append(f"{len(hyp)} {len(ref)}")
        text.append(" ".join(str(int(x)) for x in hyp))
        text.append(" ".join(str(int(x)) for x in ref))
    r = subprocess.run([emul], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return [[int(v) for v in line.split()] for line in r.stdout.splitlines()]


def test_schedule_matches_the_restatement_on_every_route(emul):
    pairs = W.shape_pairs()
    got = run(emul, pairs)
    assert len(got) == len(pairs)
    seen = set()
    for (hyp, ref), g in zip(pairs, got):
        want = R.edit_distance(hyp.tolist(), ref.tolist())
        assert g[:6] == [want.total, want.insertions, want.deletions, want.substitutions, len(hyp), len(ref)], (len(hyp), len(ref))
        if len(hyp) and len(ref):
            seen.add((g[6], g[7]))
    # strips of 1, 2, 4, 8 and 16 columns in one panel, then two and three panels of 16
    assert seen == {(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (4, 2), (4, 3)}


def test_pinned_cases_and_input_order(emul):
    sym = {}
    number = lambda seq: [sym.setdefault(x, len(sym)) for x in seq]   # noqa: E731
    pairs = [(number(a), number(b)) for a, b, _ in R.LEVENSHTEIN_CASES] + [(number(h.split()), number(r.split())) for r, h, _, _ in R.WER_CASES]
    got = run(emul, pairs)
    assert [g[0] for g in got] == [d for _, _, d in R.LEVENSHTEIN_CASES] + [e for _, _, e, _ in R.WER_CASES]
    assert [g[5] for g in got[len(R.LEVENSHTEIN_CASES):]] == [w for _, _, _, w in R.WER_CASES]
    for (hyp, ref), g in zip(pairs, got):
        assert tuple(g[:4]) == tuple(R.edit_distance(hyp, ref))
