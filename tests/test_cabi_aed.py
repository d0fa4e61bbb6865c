"""The AED entries and their Swift-shaped mirror in include/fluidaudio.hpp (AedConfig, AedDecodeState, AedLongForm, CoherePipeline,
CanaryManager) from a C++ host built with g++ -Wall -Wextra -Werror (tests/cabi/aed.cpp): the defaults, the host integer functions and
the window plan against the restatement, every refusal answered without a device — and, on the GPU, the mirror's seam merge."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import aed_cases as K  # noqa: E402
import aed_restatement as R  # noqa: E402

INVALID, TOO_SMALL, OK = "1", "3", "0"


@pytest.fixture(scope="module")
def exe(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    path = str(tmp_path_factory.mktemp("cabi") / "aed_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cabi", "aed.cpp"), "-o", path, lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return path


@pytest.fixture(scope="module")
def out(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for l in r.stdout.splitlines():
        w = l.split()
        key, rest = (w[0] + "_" + w[1], w[2:]) if w[0] in ("ST", "PLAN") else (w[0], w[1:])
        got.setdefault(key, []).append(rest)
    return got


def test_defaults_and_sizes(fa, out):
    def row(c):
        words = 8 + 2 * c["max_seq"] + (c["max_seq"] if c["mode"] else min(c["max_new"] + 1, c["max_seq"]))
        return [str(c[k]) for k in ("mode", "vocab", "eos_id", "max_seq", "max_new", "no_repeat_ngram")] + [f"{c['repetition_penalty']:g}"] + \
               [str(c[k]) for k in ("window_tokens", "min_match", "chunk_samples", "hop_samples")] + [str(c["max_seq"] if c["mode"] else min(c["max_new"] + 1, c["max_seq"])), str(4 * words * 3)]
    assert out["COHERE"] == [row(R.COHERE)] == out["PLAIN"] and out["CANARY"] == [row(R.CANARY)]
    assert out["RAW"] == [["0", "108", "56"]] and C.sizeof(fa._lib.AedConfig) == 56
    assert out["SIZES"] == [["5", str(4 * (8 + 32 + 5) * 2), "0", "0", "0", "0"]]
    py = fa.AedConfig.cohere(), fa.AedConfig.canary()
    assert [(c.mode, c.vocab, c.eos_id, c.max_seq, c.max_new, c.no_repeat_ngram, c.window_tokens, c.min_match, c.chunk_samples, c.hop_samples) for c in py] == \
           [tuple(r[k] for k in ("mode", "vocab", "eos_id", "max_seq", "max_new", "no_repeat_ngram", "window_tokens", "min_match", "chunk_samples", "hop_samples")) for r in (R.COHERE, R.CANARY)]
    assert np.float32(py[0].repetition_penalty) == np.float32(1.1) and py[1].repetition_penalty == 1.0 and bytes(fa.AedConfig().c()) == bytes(py[0].c())


def test_host_functions_equal_the_restatement(fa, out):
    want = [R.encoder_valid_frames(f, 438) for f in (0, 1, 8, 1000, 3499, 3500, 9000)] + [R.encoder_valid_frames(3500, 400), 0, 0, R.encoder_valid_frames(5, 9, 7, 3)]
    assert out["VALID"] == [[str(v) for v in want]] and out["DYNAMIC"] == [["5", "1"]]
    assert [fa.aed_encoder_valid_frames(f, 438) for f in (0, 1, 8, 1000, 3499, 3500, 9000)] == want[:7]
    samples = [0, 560000, 560001, 1040000, 1040001, 240000, 300000, 432001]
    for model, preset in ((0, R.COHERE), (1, R.CANARY)):
        lines = out[f"PLAN_{model}"]
        assert [int(l[0]) for l in lines] == samples
        for s, l in zip(samples, lines):
            vals = [int(x) for x in l[1:]]
            assert list(zip(vals[0::2], vals[1::2])) == R.plan_windows(s, preset["chunk_samples"], preset["hop_samples"]), (model, s)
        plan = fa.aed_plan_windows(samples, fa.AedConfig.preset(model))
        flat = [w for s in samples for w in R.plan_windows(s, preset["chunk_samples"], preset["hop_samples"])]
        assert list(zip(plan.starts.tolist(), plan.lengths.tolist())) == flat and plan.window_range[-1] == len(flat)
    for chunk, hop, s, want in K.WINDOW_PLANS:
        plan = fa.aed_plan_windows([s], fa.AedConfig(chunk_samples=chunk, hop_samples=hop))
        assert list(zip(plan.starts.tolist(), plan.lengths.tolist())) == want
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 500, 200)
    plan = fa.aed_plan_windows(lens, fa.AedConfig(chunk_samples=40, hop_samples=13))
    for r, s in enumerate(lens.tolist()):
        lo, hi = plan.window_range[r], plan.window_range[r + 1]
        assert list(zip(plan.starts[lo:hi].tolist(), plan.lengths[lo:hi].tolist())) == R.plan_windows(s, 40, 13)
    assert out["THROWN"] == [["2"]]
    with pytest.raises(fa.FluidAudioHipError):
        fa.aed_plan_windows([5], fa.AedConfig(hop_samples=0))


def test_every_refusal_is_answered_without_a_device(out):
    assert out["ST_begin"] == [[INVALID] * 4] and out["ST_step"] == [[INVALID] * 4]
    assert out["ST_finish"] == [[INVALID, TOO_SMALL, INVALID, INVALID]]
    assert out["ST_masks"] == [[INVALID] * 6] and out["ST_gather"] == [[INVALID] * 3]
    assert out["ST_plan"] == [[OK, TOO_SMALL, "3", "3", INVALID, INVALID]]
    assert out["ST_merge"] == [[INVALID, TOO_SMALL, INVALID, INVALID, INVALID]]


@pytest.mark.gpu
def test_the_mirror_merges_on_the_device(exe, gpu_ctx):
    by_window = {}
    for _, windows, wt, mm, _ in K.MERGE_LITERAL + K.MERGE_OWN:
        by_window.setdefault((wt, mm), []).append(windows)
    text = "".join(f"group {wt} {mm}\n" + "".join("".join(" ".join(str(t) for t in w) + "\n" for w in r) + "end\n" for r in recordings) + "run\n"
                   for (wt, mm), recordings in by_window.items())
    r = subprocess.run([exe, "merge"], input=text, capture_output=True, text=True, timeout=120)                 # one process, one context
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    merged = [[int(t) for t in l[1:]] for l in lines if l[0] == "MERGED"]
    assert merged == [R.merge_recording(w, wt, mm)[0] for (wt, mm), recordings in by_window.items() for w in recordings]
    assert [l[1:] for l in lines if l[0] == "ONE"] == [[str(t) for t in (1, 2, 3, 7, 8, 9, 10, 11, 12)]]
