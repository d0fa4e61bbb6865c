"""One number for fa_der_score_batch: 16 recordings of 8 h at step 0.01, 4-8 speakers and about 10 000 segments per side, scored by one
call.  Prints one JSON line: the median host-clock time of the ABI call (it ends in the call's one stream synchronisation), the same for
the Python wrapper (label numbering and packing included), and the bytes of bit planes the kernels touch, computed from the shapes.
Recording 0 is checked at the timed size against a numpy evaluation of the same definition (vectorised over frames; the assignment by
tests/der_restatement.hungarian).  Fails without a GPU.

    python scripts/der_probe.py [--recordings 16] [--hours 8] [--repeats 15] [--out profiles/der_probe.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fluidaudio_amd as fa  # noqa: E402
from fluidaudio_amd import _lib as L, der  # noqa: E402


def recording(rng, dur, speakers, n, prefix):
    """n speech turns of `speakers` speakers over dur seconds: mean length dur * 1.2 / n, so about a fifth of the time is overlapped."""
    start = np.sort(rng.uniform(0.0, dur, n))
    end = np.minimum(start + rng.exponential(1.2 * dur / n, n), dur)
    who = rng.integers(speakers, size=n)
    return [fa.DERSpeakerSegment(f"{prefix}{w}", float(a), float(b)) for w, a, b in zip(who, start, end)]


def numpy_counts(ref, hyp, step, collar, frames):
    """The definition evaluated with numpy for one recording: (overlap [H][R], mapping, (miss, fa, conf, ref))."""
    import der_restatement as R

    def planes(side):
        labels, arr = der.index_labels(side)
        m = np.zeros((len(labels), frames), bool)
        for lab, a, b in zip(arr["label"], arr["start"], arr["end"]):
            if b > a:
                m[lab, max(0, int(np.ceil(a / step - 0.5))):min(frames, int(np.ceil(b / step - 0.5)))] = True
        return m, arr
    rm, rarr = planes(ref)
    hm, _ = planes(hyp)
    H, Rn = hm.shape[0], rm.shape[0]
    ov = [[int(np.count_nonzero(hm[h] & rm[r])) for r in range(Rn)] for h in range(H)]
    n = max(H, Rn)
    mx = max(max(row) for row in ov)
    cost = [mx] * (n * n)
    for h in range(H):
        for r in range(Rn):
            cost[h * n + r] = mx - ov[h][r]
    assign = R.hungarian(cost, n)
    mapping = [assign[h] if assign[h] < Rn and ov[h][assign[h]] > 0 else -1 for h in range(H)]
    ok = np.ones(frames, bool)
    if collar > 0:
        for a, b in zip(rarr["start"], rarr["end"]):
            if b > a:
                for x in (a, b):
                    ok[max(0, int(np.floor((x - collar / 2.0) / step))):min(frames, int(np.ceil((x + collar / 2.0) / step)))] = False
    n_ref, n_sys = rm.sum(0, dtype=np.int64), hm.sum(0, dtype=np.int64)
    correct = np.zeros(frames, np.int64)
    for h, r in enumerate(mapping):
        if r >= 0:
            correct += hm[h] & rm[r]
    return ov, mapping, tuple(int(v[ok].sum()) for v in (np.maximum(0, n_ref - n_sys), np.maximum(0, n_sys - n_ref), np.minimum(n_ref, n_sys) - correct, n_ref))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=16)
    ap.add_argument("--hours", type=float, default=8.0)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--collar", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("der_probe: no GPU visible (there is no CPU fallback)")
    ctx = fa.default_context(0)
    rng = np.random.default_rng(2024)
    step, dur = 0.01, a.hours * 3600.0
    pairs = [(recording(rng, dur, int(rng.integers(4, 9)), a.segments, "r"), recording(rng, dur, int(rng.integers(4, 9)), a.segments, "h"))
             for _ in range(a.recordings)]

    # the wrapper's packing, done once for the ABI timing
    sides = [(der.index_labels(r), der.index_labels(h)) for r, h in pairs]
    ref, hyp = np.concatenate([r[1] for r, _ in sides]), np.concatenate([h[1] for _, h in sides])
    cum = lambda xs: np.concatenate([[0], np.cumsum(xs)]).astype(np.int64)  # noqa: E731
    ref_range, hyp_range = cum([r[1].size for r, _ in sides]), cum([h[1].size for _, h in sides])
    map_range, ov_range = cum([len(h[0]) for _, h in sides]), cum([len(h[0]) * len(r[0]) for r, h in sides])
    counts = np.zeros(a.recordings, der.DER_COUNTS_DTYPE)
    mapping, overlap = np.zeros(int(map_range[-1]), np.int32), np.zeros(int(ov_range[-1]), np.int64)
    cfg = L.DerConfig(step, a.collar)

    def abi():
        ctx.check(L.lib().fa_der_score_batch(ctx.handle, C.byref(cfg), ref.ctypes.data, ref_range.ctypes.data, hyp.ctypes.data, hyp_range.ctypes.data,
                                             a.recordings, counts.ctypes.data, mapping.ctypes.data, map_range.ctypes.data, overlap.ctypes.data, overlap.size),
                  "fa_der_score_batch")

    def timed(f):
        for _ in range(a.warmup):
            f()
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return ts
    t_abi = timed(abi)
    t_wrap = timed(lambda: fa.compute_der_batch(pairs, step, a.collar, ctx))
    res = fa.compute_der_batch(pairs, step, a.collar, ctx)

    frames = int(counts["frames"][0])
    ov, mp, cnt = numpy_counts(*pairs[0], step, a.collar, frames)
    got = (int(counts["miss"][0]), int(counts["false_alarm"][0]), int(counts["confusion"][0]), int(counts["ref"][0]))
    checked = (res[0].overlap.tolist() == ov and res[0].index_mapping == mp and got == cnt
               and (res[0].miss_frames, res[0].false_alarm_frames, res[0].confusion_frames, res[0].ref_frames) == cnt)
    words = (counts["frames"].astype(np.int64) + 63) // 64
    plane_bytes = int((words * (counts["ref_labels"].astype(np.int64) + counts["hyp_labels"] + 1)).sum() * 8)
    line = dict(probe="der_score_batch", recordings=a.recordings, hours_each=a.hours, frame_step=step, collar=a.collar, segments_per_side=a.segments,
                speakers=[[int(c["ref_labels"]), int(c["hyp_labels"])] for c in counts], frames_each=frames,
                abi_call_ms_median=1e3 * statistics.median(t_abi), abi_call_ms_min=1e3 * min(t_abi), abi_call_ms_max=1e3 * max(t_abi),
                wrapper_call_ms_median=1e3 * statistics.median(t_wrap), repeats=a.repeats, warmup=a.warmup,
                plane_bytes=plane_bytes, segment_bytes_uploaded=int(ref.nbytes + hyp.nbytes),
                audio_hours_per_s=a.recordings * a.hours / statistics.median(t_abi), der_recording0=res[0].der, recording0_matches_numpy=bool(checked))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(0 if checked else 1)


if __name__ == "__main__":
    main()
