"""Times fa_fsmn_vad_segments_dev on one MI355X (DESIGN.md quotes the figures): 1, 16 and 64 recordings of 360 000 frames (one hour at
10 ms) of resident silence probabilities from the block generator of tests/fsmn_vad_cases.py, the default config.  The entry
synchronises once per call, so a call is timed whole: between two device events on the context's stream round it (the upload of the
recordings' table, the three kernels, the copies back) and on the host's clock; both are the median of --repeats calls behind two
warm-up calls.  Beside them: the 4 bytes per frame the kernel must read and the time they take at the copy rate, the time per 64-frame
step of the serial walk (5 625 steps per recording, all recordings in parallel), and the host restatement's time for one recording.
--dry stops before the device work (no GPU needed)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_SPEC = 8.0e12          # bytes / s, MI355X data sheet
HBM_COPY = 6.29e12         # bytes / s, what a float4 copy reaches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--frames", type=int, default=360_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    args = ap.parse_args()
    import fluidaudio_amd as fa
    import fsmn_vad_cases as K
    import fsmn_vad_restatement as R
    rng = np.random.default_rng(0)
    recordings = [K.blocks(rng, args.frames) for _ in range(max(args.batches))]
    t0 = time.perf_counter()
    want = R.decide(recordings[0])
    restatement_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(frames=args.frames, restatement_ms_one_recording=restatement_ms, segments_one_recording=len(want))), flush=True)
    if args.dry:
        return
    import torch
    ctx = fa.default_context(0)
    own = torch.cuda.ExternalStream(ctx.stream, device=ctx.device)
    rows = []
    for B in args.batches:
        dev = torch.from_numpy(np.concatenate(recordings[:B])).cuda()
        frame_range = np.arange(B + 1, dtype=np.int64) * args.frames
        torch.cuda.synchronize()
        segs, counts = fa.fsmn_vad_segments_dev(dev, frame_range, ctx=ctx)
        assert [(int(s["start_frame"]), int(s["end_frame"]), int(s["reason"])) for s in segs[:counts[0]]] == [s[:3] for s in want]
        capacity = len(segs)

        def call():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            with torch.cuda.stream(own):
                e0.record(own)
                fa.fsmn_vad_segments_dev(dev, frame_range, capacity=capacity, ctx=ctx, ordered=False)
                e1.record(own)
            ctx.synchronize()
            wall = (time.perf_counter() - t) * 1e6
            return e0.elapsed_time(e1) * 1e3, wall                   # microseconds

        call(), call()
        times = [call() for _ in range(args.repeats)]
        device_us, wall_us = (float(np.median([t[k] for t in times])) for k in (0, 1))
        nbytes, steps = 4 * B * args.frames, (args.frames + 63) // 64
        row = dict(B=B, frames=args.frames, segments=int(len(segs)), bytes_read=nbytes, device_us=device_us, wall_us=wall_us,
                   spread_device_us=[float(min(t[0] for t in times)), float(max(t[0] for t in times))], hbm_bound_us=nbytes / HBM_COPY * 1e6,
                   hbm_fraction_spec=nbytes / (device_us * 1e-6) / HBM_SPEC, hbm_fraction_copy=nbytes / (device_us * 1e-6) / HBM_COPY, steps=steps,
                   us_per_step=device_us / steps, sclk_mhz=ctx.sclk_mhz(), restatement_over_device=restatement_ms * 1e3 * B / device_us)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
