"""Two numbers for fa_edit_distance_batch: a corpus-like batch (4 096 utterances of 20-200 words, hypotheses with ~10 % word errors, scored
as words and as characters in one call of 8 192 pairs) and one long pair (10 000 x 10 000 symbols, ten panels on one wavefront).  Prints
one JSON line: per leg the median host-clock time of the ABI call (it ends in the call's one stream synchronisation), the device time
between the call's two events (fa_ctx_set_timing), table cells per second, and the time of the single-core C++ baseline
(scripts/wer_baseline.cpp: the reference's full-table algorithm with its traceback) on the same machine, whose sums over the pairs must
equal the device's.  Fails without a GPU.

    python scripts/wer_probe.py [--pairs 4096] [--long 10000] [--repeats 15] [--out profiles/wer_probe.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluidaudio_amd as fa  # noqa: E402
from fluidaudio_amd import _lib as L, wer  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def edited(rng, ref, vocab):
    """~10 % substitutions, drops and insertions."""
    u = rng.random(ref.size)
    fresh = rng.integers(0, vocab, ref.size)
    out = []
    for x, v, w in zip(ref.tolist(), u.tolist(), fresh.tolist()):
        if v < 0.033:
            out += [w, x]
        elif v < 0.066:
            continue
        elif v < 0.1:
            out.append(w)
        else:
            out.append(x)
    return np.array(out, np.int32)


def corpus(rng, pairs, vocab=5000):
    """Word pairs, then the same utterances as characters (a word is 2-9 letters decided by its id)."""
    letters = [np.array([(w * 2654435761 >> (3 * k)) % 26 for k in range(2 + w % 8)], np.int32) for w in range(vocab)]
    words = []
    for _ in range(pairs):
        ref = np.minimum(rng.zipf(1.3, int(rng.integers(20, 201))) - 1, vocab - 1).astype(np.int32)
        words.append((edited(rng, ref, vocab), ref))
    spell = lambda s: np.concatenate([letters[w] for w in s.tolist()]) if s.size else np.zeros(0, np.int32)   # noqa: E731
    return words + [(spell(h), spell(r)) for h, r in words]


def baseline(exe, hyp, hyp_range, ref, ref_range):
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(np.int64(hyp_range.size - 1).tobytes() + hyp_range.tobytes() + ref_range.tobytes() + hyp.tobytes() + ref.tobytes())
        f.flush()
        r = subprocess.run([exe, f.name], capture_output=True, text=True, check=True)
    v = r.stdout.split()
    return float(v[0]), [int(x) for x in v[1:]]


def leg(ctx, name, pairs, exe, repeats, warmup):
    hyp, hyp_range = wer._pack([h for h, _ in pairs])
    ref, ref_range = wer._pack([r for _, r in pairs])
    out = np.zeros(len(pairs), wer.EDIT_COUNTS_DTYPE)

    def abi():
        ctx.check(L.lib().fa_edit_distance_batch(ctx.handle, hyp.ctypes.data, hyp_range.ctypes.data, ref.ctypes.data, ref_range.ctypes.data, len(pairs),
                                                 out.ctypes.data), "fa_edit_distance_batch")
    for _ in range(warmup):
        abi()
    host, dev = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        abi()
        host.append(time.perf_counter() - t0)
        dev.append(L.lib().fa_ctx_last_device_ms(ctx.handle))
    cells = int((out["hyp_len"].astype(np.int64) * out["ref_len"]).sum())
    sums = [int(out[k].astype(np.int64).sum()) for k in ("total", "insertions", "deletions", "substitutions")]
    res = dict(leg=name, pairs=len(pairs), symbols=int(hyp.size + ref.size), table_cells=cells, call_ms_median=1e3 * statistics.median(host),
               call_ms_min=1e3 * min(host), call_ms_max=1e3 * max(host), device_ms_median=statistics.median(dev),
               gcells_per_s_device=cells / statistics.median(dev) / 1e6, repeats=repeats, warmup=warmup, sums=sums)
    if exe:
        ms, want = baseline(exe, hyp, hyp_range, ref, ref_range)
        res.update(baseline_single_core_ms=ms, baseline_over_call=ms / (1e3 * statistics.median(host)), matches_baseline=want == sums)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--long", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("wer_probe: no GPU visible (there is no CPU fallback)")
    exe = None
    if not a.no_baseline:
        exe = os.path.join(HERE, "wer_baseline")
        if not os.path.exists(exe):
            subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(HERE, "wer_baseline.cpp"), "-o", exe], check=True)
    ctx = fa.default_context(0)
    L.lib().fa_ctx_set_timing(ctx.handle, 1)
    rng = np.random.default_rng(2024)
    legs = [leg(ctx, "corpus_words_and_characters", corpus(rng, a.pairs), exe, a.repeats, a.warmup)]
    ref = rng.integers(0, 1000, a.long).astype(np.int32)
    legs.append(leg(ctx, "one_long_pair", [(edited(rng, ref, 1000)[:a.long], ref)], exe, max(3, a.repeats // 3), 1))
    line = dict(probe="edit_distance_batch", sclk_mhz=ctx.sclk_mhz(), legs=legs)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(0 if all(l.get("matches_baseline", True) for l in legs) else 1)


if __name__ == "__main__":
    main()
