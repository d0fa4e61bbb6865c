"""Timing of the VAD stage on one MI355X: fa_vad_segments_dev at 4 096 recordings of 1 h (14 063 frames each) and at one recording of 8 h
(112 500 frames), fa_vad_pack_chunks_dev on 1 h and 8 h of audio (as many 1 h recordings as --pack-recordings says: 4 096 of them are
944 GB of samples and do not fit a device), and the Python restatement (tests/vad_restatement.py; a CPU restatement, not the Swift
reference) on the same probabilities — on the first --restated recordings of the batch, scaled, and on all of the 8 h recording.
Every timed call is warmed, ends in a device synchronise and is repeated --reps times: the best, and the spread (max - min) / min.
Prints one JSON line with the times, the bytes each call must move against the 8 TB/s HBM peak, and matches_restatement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12
BANDS = np.array([[0.85, 1.0], [0.0, 0.7], [0.7, 0.85]], np.float32)


def draw_probs(rng, n):
    """Runs of 1 ... 40 frames (10 s) from the three bands: speech, silence, the band between the thresholds."""
    lengths = rng.integers(1, 41, n // 20 + 64)
    while lengths.sum() < n:
        lengths = np.concatenate([lengths, rng.integers(1, 41, n // 20 + 64)])
    band = np.repeat(rng.integers(0, 3, lengths.size), lengths)[:n]
    return (BANDS[band, 0] + (BANDS[band, 1] - BANDS[band, 0]) * rng.random(n, dtype=np.float32)).astype(np.float32)


def timed(reps, fn, sync):
    ts = []
    for _ in range(reps + 2):                                                    # two warm-up calls
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    ts = ts[2:]
    return min(ts), (max(ts) - min(ts)) / min(ts), r


def restated(R, probs, frame_range, totals, first):
    t0 = time.perf_counter()
    rows = [(b, 0, s, e, st, et) for b in range(first) for s, e, st, et in R.segment_speech(probs[frame_range[b]:frame_range[b + 1]], int(totals[b]))]
    return time.perf_counter() - t0, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--recordings", type=int, default=4096)
    ap.add_argument("--restated", type=int, default=256)
    ap.add_argument("--pack-recordings", type=int, default=16)
    args = ap.parse_args()
    import torch
    import fluidaudio_amd as fa
    import vad_restatement as R
    ctx = fa.default_context(0)
    sync = ctx.synchronize
    rng = np.random.default_rng(16)
    out, ok = {}, True
    for name, B, frames in (("batch_1h", args.recordings, 14063), ("single_8h", 1, 112500)):
        probs = draw_probs(rng, B * frames)
        frame_range = (np.arange(B + 1, dtype=np.int64) * frames)
        totals = np.full(B, frames * R.CHUNK - 1234, np.int64)
        dev = torch.from_numpy(probs).cuda()
        f, count = fa.lib().fa_vad_segments_dev, C.c_int64(0)
        args_dev = (ctx.handle, None, dev.data_ptr(), frame_range.ctypes.data, totals.ctypes.data, B)
        t_count, s_count, _ = timed(args.reps, lambda: ctx.check(f(*args_dev, None, 0, C.byref(count), None), "fa_vad_segments_dev"), sync)
        segs = np.zeros(count.value, fa.VAD_SEGMENT_DTYPE)
        t_full, s_full, _ = timed(args.reps, lambda: ctx.check(f(*args_dev, segs.ctypes.data, segs.size, C.byref(count), None), "fa_vad_segments_dev"), sync)
        first = min(B, args.restated)
        t_cpu, rows = restated(R, probs, frame_range, totals, first)
        want = np.array(rows, fa.VAD_SEGMENT_DTYPE)
        same = segs[segs["recording"] < first].tobytes() == want.tobytes() and len(want) > 0
        ok = ok and same
        nbytes = probs.nbytes + 8 * count.value + 40 * count.value                # the probabilities once, a raw speech and a record per segment
        out[name] = {"recordings": B, "frames_each": frames, "segments": int(count.value), "count_only_ms": 1e3 * t_count, "count_only_spread": s_count,
                     "segments_dev_ms": 1e3 * t_full, "segments_dev_spread": s_full, "bytes": int(nbytes), "hbm_floor_ms": 1e3 * nbytes / HBM_PEAK,
                     "share_of_hbm_peak": nbytes / HBM_PEAK / t_full, "restated_recordings": first, "cpu_restatement_s": t_cpu,
                     "cpu_restatement_scaled_s": t_cpu * B / first, "matches_restatement": bool(same)}
        del dev
    for name, B, seconds in (("pack_1h", args.pack_recordings, 3600), ("pack_8h", 1, 8 * 3600)):
        n = seconds * 16000 - 777                                                # a short last chunk
        audio = torch.rand(B * n, dtype=torch.float32, device="cuda")
        offsets = np.arange(B + 1, dtype=np.int64) * n
        t_pack, s_pack, (rows, chunk_range) = timed(args.reps, lambda: fa.pack_chunks_dev(audio, offsets, ctx=ctx), sync)
        host = audio[:n].cpu().numpy()
        same = bool(np.array_equal(rows[:chunk_range[1]].cpu().numpy().view(np.int32), R.pack_chunks(host).view(np.int32)))
        ok = ok and same
        nbytes = audio.numel() * 4 + rows.numel() * 4
        out[name] = {"recordings": B, "samples_each": n, "rows": int(chunk_range[-1]), "pack_dev_ms": 1e3 * t_pack, "pack_dev_spread": s_pack, "bytes": int(nbytes),
                     "hbm_floor_ms": 1e3 * nbytes / HBM_PEAK, "share_of_hbm_peak": nbytes / HBM_PEAK / t_pack, "matches_restatement": same}
        del audio, rows
    out["matches_restatement"] = bool(ok)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
