"""Timing of the offline Sortformer path around its network at 8 recordings x 8 h (2 880 001 mel frames and 1 268 windows each): wall
time of each call (device-synchronised, best of --reps) with its algorithmic bytes and the fraction of 8 TB/s they amount to, the mel
plan's achieved write bandwidth on the same input for scale, and the numpy restatement's time on one recording
(tests/sortformer_restatement.py; a CPU restatement, not the Swift reference).  Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split (--no-restatement skips the CPU part there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8e12   # bytes / s


def best(f, reps, sync):
    out, times = None, []
    for _ in range(reps + 1):
        sync()
        t0 = time.perf_counter()
        out = f()
        sync()
        times.append(time.perf_counter() - t0)
    return out, min(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=8)
    ap.add_argument("--hours", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    import torch
    import fluidaudio_amd as fa
    import sortformer_restatement as R
    from test_gpu_sortformer import synthetic_preds
    ctx = fa.default_context(0)
    sync = torch.cuda.synchronize
    B, samples = args.recordings, int(args.hours * 3600 * 16000)
    cfg, rcfg = fa.OfflineSortformerConfig(), R.OfflineConfig()
    out = {"recordings": B, "hours": args.hours}

    # mel of the batch through the plan path (centre padding, mel-major): its write bandwidth is the yardstick for the pack
    d_pcm = torch.empty(B * samples, dtype=torch.float32, device="cuda").uniform_(-0.1, 0.1)
    mel = fa.AudioMelSpectrogram(ctx=ctx)
    plan = mel.plan(np.arange(B + 1, dtype=np.int64) * samples, layout="mel_major")
    n_mel = min(1 + samples // 160, plan.frame_stride)
    d_mel = torch.empty(plan.out_shape(), dtype=torch.float32, device="cuda")
    _, t = best(lambda: plan.execute(d_pcm, d_mel), args.reps, sync)
    mel_bytes = d_mel.numel() * 4
    out["mel"] = {"ms": 1e3 * t, "write_bytes": mel_bytes, "read_bytes": d_pcm.numel() * 4, "write_GBps": mel_bytes / t / 1e9,
                  "write_fraction_of_peak": mel_bytes / t / PEAK}
    plan.close()
    del d_pcm
    lengths = [n_mel] * B
    geo = fa.offline_windows(lengths, cfg)
    W = int(geo["window_range"][-1])
    out.update(mel_frames=n_mel, windows_per_recording=W // B, total_out=int(geo["total_out"][0]))

    for layout in ("mel_major", "frame_major"):
        src = d_mel if layout == "mel_major" else d_mel.transpose(1, 2).contiguous()
        (d_win, d_len), t = best(lambda: fa.pack_windows(src, lengths, layout, cfg, ctx), args.reps, sync)
        rd, wr = B * n_mel * cfg.mel_features * 4, d_win.numel() * 4
        out[f"pack_{layout}"] = {"call_ms": 1e3 * t, "read_bytes": rd, "write_bytes": wr, "GBps": (rd + wr) / t / 1e9, "fraction_of_peak": (rd + wr) / t / PEAK,
                                 "launches": 1, "host_syncs": 1}
        del src, d_win, d_len
    del d_mel

    preds, _ = synthetic_preds(np.random.default_rng(0), rcfg, n_mel)
    d_preds = torch.from_numpy(preds).cuda().repeat(B, 1, 1)
    (d_global, d_map), t = best(lambda: fa.stitch(d_preds, lengths, cfg, ctx), args.reps, sync)
    out["stitch"] = {"call_ms": 1e3 * t, "read_bytes": d_preds.numel() * 4, "write_bytes": d_global.numel() * 4 + d_map.numel() * 4, "launches": 3,
                     "host_syncs": 1, "bound": "launch / latency"}
    tcfg = fa.DiarizerTimelineConfig.default(4, float(cfg.frame_duration_seconds))
    frames = geo["total_out"]
    (recs, per), t = best(lambda: fa.timeline_segments(d_global, frames, None, None, tcfg, True, ctx), args.reps, sync)
    out["timeline"] = {"call_ms_count_then_fill": 1e3 * t, "segments": int(recs.size), "read_bytes": d_global.numel() * 4, "write_bytes": int(recs.nbytes),
                       "launches_per_call": 9, "host_syncs_per_call": "2 for counts (raw runs, segments) + the record copy", "bound": "launch / latency"}
    if not args.no_restatement:
        t0 = time.perf_counter()
        g, m = R.stitch(rcfg, n_mel, preds)
        t1 = time.perf_counter()
        want = R.timeline_records(R.TimelineConfig(4, float(rcfg.frame_duration_seconds)), [g], None, True)
        t2 = time.perf_counter()
        out["cpu_restatement_one_recording"] = {"stitch_s": t1 - t0, "timeline_s": t2 - t1}
        n0 = int(frames[0])
        got = recs[recs["recording"] == 0]
        out["matches_restatement"] = bool(np.array_equal(d_global[:n0].cpu().numpy().view(np.uint32), g.view(np.uint32)) and
                                          np.array_equal(d_map[:W // B].cpu().numpy(), m) and len(want) == got.size and
                                          [w[2:4] for w in want] == [(int(r["start_frame"]), int(r["end_frame"])) for r in got])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
