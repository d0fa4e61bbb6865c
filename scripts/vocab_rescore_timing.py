"""Times fa_vocab_rescore_candidates on one MI355X beside the single-thread plain-DP walk of fluidaudio_amd/csrc/vocab_rescore_core.h on
the same host (DESIGN.md quotes the figures): 64 utterances x 200 words against a vocabulary of 670 terms (5 - 12 letters, a fifth with
an alias, a tenth of the forms two words), one word in twenty a near match of some form.  The device figure is the host clock round
whole calls — packing, upload, the pre-pass and the walk, the one synchronisation, the sort — and, beside it, the device time between
the two events of fa_ctx_set_timing; both after two calls of warm-up, ten calls, the median and the spread.  The walk is
tests/cpu/vocab_rescore_core_main.cpp built with g++ -O2 (no sanitizer), given the same problem; it has to find as many candidates.
Not part of bench.py.  --dry prints the plan and the host walk's time and stops (no GPU needed)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LETTERS = "abcdefghijklmnopqrstuvwxyz"


def problem(utterances, terms, words, seed=0):
    rng = np.random.default_rng(seed)

    def word(lo, hi):
        return "".join(LETTERS[i] for i in rng.integers(0, 26, int(rng.integers(lo, hi + 1))))
    vocabulary, forms = [], []
    for _ in range(terms):
        text = word(5, 12) if rng.random() > 0.1 else word(3, 7) + " " + word(3, 7)
        aliases = [word(5, 12)] if rng.random() < 0.2 else []
        forms += [text] + aliases
        vocabulary.append(dict(char_count=len(text), min_similarity=None, forms=[tuple(ord(c) for c in f) for f in [text] + aliases]))
    batch = []
    for _ in range(utterances):
        row = []
        while len(row) < words:
            if rng.random() < 0.05:
                near = list(forms[int(rng.integers(0, len(forms)))])
                near[int(rng.integers(0, len(near)))] = LETTERS[int(rng.integers(0, 26))]
                row += "".join(near).split(" ")
            else:
                row.append(word(1, 9))
        row = row[:words]
        batch.append(([tuple(ord(c) for c in w) for w in row], [int(f) for f in rng.choice([0, 0, 0, 0, 3], words)]))
    return vocabulary, batch


def host_walk_ms(vocabulary, batch, min_similarity):
    import vocab_rescore_cases as K
    import vocab_rescore_restatement as R
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "walk")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpu", "vocab_rescore_core_main.cpp"), "-o", exe], check=True)
        words = ["walk"] + K.vocabulary_words(vocabulary, 3) + [R.bits(np.float32(min_similarity))] + K.utterance_words(batch) + ["time"]
        r = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, check=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("TIME")][0].split()
    return float(line[1]), int(line[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--terms", type=int, default=670)
    ap.add_argument("--words", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=None, help="also write the row as JSON to this file")
    args = ap.parse_args()
    vocabulary, batch = problem(args.utterances, args.terms, args.words)
    forms = sum(len(t["forms"]) for t in vocabulary)
    row = dict(utterances=args.utterances, terms=args.terms, words=args.words, forms=forms, date=time.strftime("%Y-%m-%d"),
               pairs=args.utterances * args.words * forms)
    row["host_walk_ms"], row["host_walk_candidates"] = host_walk_ms(vocabulary, batch, 0.5)
    if not args.dry:
        import fluidaudio_amd as fa
        ctx = fa.default_context(0)
        V = fa.vocab_rescore
        blob = V.build(vocabulary)
        fa.lib().fa_ctx_set_timing(ctx.handle, 1)
        wall, device = [], []
        for _ in range(args.repeats + 2):   # two calls of warm-up
            t0 = time.perf_counter()
            recs, _ = V.candidates(blob, batch, 0.5, capacity=65536, ctx=ctx)
            wall.append((time.perf_counter() - t0) * 1e3)
            device.append(fa.lib().fa_ctx_last_device_ms(ctx.handle))
        assert len(recs) == row["host_walk_candidates"], (len(recs), row["host_walk_candidates"])
        for name, ms in (("call", sorted(wall[2:])), ("device", sorted(device[2:]))):
            row[name + "_ms"], row[name + "_spread"] = ms[len(ms) // 2], (ms[-1] - ms[0]) / ms[len(ms) // 2]
        row["host_walk_over_call"] = row["host_walk_ms"] / row["call_ms"]
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
