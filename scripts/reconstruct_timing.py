"""Timing of the speaker-segment stage at 8 h (BASELINE config 5's geometry: 14 400 windows of 10 s at a 2 s step, 589 frames,
7 powerset classes): device time of the powerset decode and of fa_offline_reconstruct_dev (device-synchronised wall clock, best of
--reps), the host merge / sanitize pass alone (fa_segments_finalize on the same raw list), and the numpy CPU restatement on the same
input (tests/reconstruct_restatement.py; a CPU restatement, not the Swift reference).  Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split (--no-restatement skips the CPU part there)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    import torch
    import fluidaudio_amd as fa
    import reconstruct_restatement as R
    ctx = fa.default_context(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_8h.npz"))
    n = 14400
    cen = g["centroids"]
    hard = fa.chunk_assignments(np.repeat(np.arange(n), 3), np.tile(np.arange(3), n), g["assignments"].astype(np.int32), cen.shape[0], n, 3)
    x = torch.from_numpy(R.session_logits(n)).cuda()
    off = np.arange(n) * 2.0
    rec = fa.OfflineReconstruction(ctx=ctx)
    dec, tot = [], []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seg = fa.powerset_decode(x, off, ctx=ctx)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        segs = rec.build_segments(seg, hard, cen)
        t2 = time.perf_counter()
        dec.append(t1 - t0)
        tot.append(t2 - t1)
    out = {"segments": len(segs), "raw_segments": rec.last_info["raw_segments"], "total_frames": rec.last_info["total_frames"],
           "decode_ms": 1e3 * min(dec[1:]), "reconstruct_call_ms": 1e3 * min(tot[1:]),
           "decode_bytes": int(x.numel() * 4 + seg.speaker_weights.numel() * 4), "reconstruct_weight_bytes": int(seg.speaker_weights.numel() * 4)}
    w = seg.speaker_weights.cpu().numpy()
    if not args.no_restatement:
        t0 = time.perf_counter()
        want, st = R.build_segments(w, hard, cen, off, 0.0, R.config(), return_state=True)
        out["cpu_restatement_s"] = time.perf_counter() - t0
        raw = st["raw"]
        arr = (fa.reconstruct.RttmSegment * len(raw))()
        for i, s in enumerate(raw):
            arr[i].start_seconds, arr[i].end_seconds, arr[i].quality, arr[i].speaker_id = float(s[1]), float(s[2]), float(s[3]), s[0].encode()
        res = (fa.reconstruct.RttmSegment * len(raw))()
        cfg = fa.ReconstructionConfig().c_config()
        cnt = C.c_int64()
        best = 1e9
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fa._lib.lib().fa_segments_finalize(C.byref(cfg), arr, len(raw), res, len(raw), C.byref(cnt))
            best = min(best, time.perf_counter() - t0)
        out["host_finalize_ms"] = 1e3 * best
        out["matches_restatement"] = cnt.value == len(want) == len(segs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
