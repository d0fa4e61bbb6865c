"""Timing of the TDT window planner on one MI355X: fa_tdt_plan_windows_dev + fa_tdt_pack_windows_dev for --long recordings of 1 h and for
--short recordings of 60 s (arbitration path B: aligned starts with the warm-up probe), the plan alone with regular starts (path C: the
energy table, the speech end and the window loop, no chain), and fa_tdt_speech_gate_dev without spans (the energy table and the
percentile).  From them: the energy pass's share of the HBM bound (4 bytes per sample, read once; the plan of path C less nothing, so
the share is a LOWER bound for the kernel alone) and the time per chain step ((path B - path C) / targets of a recording, the chains of
all recordings running side by side).  Beside them a single-thread C++ restatement of the reference's loops on the host
(scripts/tdt_plan_baseline.cpp; a CPU restatement, not the Swift reference) on ONE recording, scaled by the number of recordings.
Every timed call is warmed, ends in a device synchronise and is repeated --reps times: the best, and the spread (max - min) / min.
Prints one JSON line; matches_restatement compares the first recordings' windows with tests/tdt_plan_restatement.py."""
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
HBM_PEAK = 8.0e12
LEVELS = (0.0, 0.0003, 0.002, 0.02, 0.1)


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


def draw_audio(torch, B, n, seed):
    """Gaussian noise under an envelope in 0.2 s steps, the levels of the tests; made on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    steps = -(-B * n // 3200)
    levels = torch.tensor(LEVELS, device="cuda")[torch.randint(0, len(LEVELS), (steps,), generator=g, device="cuda")]
    audio = torch.randn(B * n, generator=g, device="cuda", dtype=torch.float32)
    audio *= levels.repeat_interleave(3200)[:B * n]
    return audio


def baseline(exe, host, mode, pack):
    with tempfile.NamedTemporaryFile(suffix=".f32") as f:
        host.tofile(f.name)
        out = subprocess.run([exe, f.name] + [str(int(v)) for v in mode] + [str(int(pack))], capture_output=True, text=True, check=True).stdout.split()
    return float(out[0]), float(out[1]), int(out[2]), int(out[3]), int(out[4]), int(out[5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long", type=int, default=64)
    ap.add_argument("--short", type=int, default=1024)
    ap.add_argument("--restated", type=int, default=2)
    args = ap.parse_args()
    import torch
    import fluidaudio_amd as fa
    import tdt_plan_restatement as R
    ctx = fa.default_context(0)
    sync = ctx.synchronize
    exe = os.path.join(tempfile.mkdtemp(), "tdt_plan_baseline")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "scripts", "tdt_plan_baseline.cpp"), "-o", exe], check=True)
    path_b, path_c = fa.tdt_window_config(False, True, 7), fa.tdt_window_config(False, False, 0)
    out, ok = {}, True
    for name, B, seconds in (("long_1h", args.long, 3600), ("short_60s", args.short, 60)):
        n = seconds * 16000 + 777
        audio = draw_audio(torch, B, n, 16 + B)
        offsets = np.arange(B + 1, dtype=np.int64) * n
        cap = B * fa.tdt_window_count_bound(n, path_b)                             # the bound of path C is smaller
        t_c, s_c, plan_c = timed(args.reps, lambda: fa.tdt_plan_windows_dev(audio, offsets, config=path_c, capacity=cap, ctx=ctx), sync)
        t_b, s_b, plan_b = timed(args.reps, lambda: fa.tdt_plan_windows_dev(audio, offsets, config=path_b, capacity=cap, ctx=ctx), sync)
        t_gate, s_gate, _ = timed(args.reps, lambda: fa.tdt_speech_gate_dev(audio, offsets, ctx=ctx), sync)
        t_pack, s_pack, (rows, _) = timed(args.reps, lambda: fa.tdt_pack_windows_dev(audio, offsets, plan_b.windows, config=path_b, ctx=ctx), sync)
        pack_bytes = 4 * rows.numel() + 4 * int(plan_b.windows["length"].sum())
        del rows
        host = audio[:n].cpu().numpy()
        cpu_plan_ms, cpu_pack_ms, cpu_windows, cpu_starts, cpu_lengths, cpu_end = baseline(exe, host, (0, 1, 7), True)
        mine = plan_b.windows[plan_b.windows["recording"] == 0]
        same = (cpu_windows, cpu_starts, cpu_lengths, cpu_end) == (len(mine), int(mine["chunk_start"].sum()), int(mine["length"].sum()), int(plan_b.speech_end[0]))
        for b in range(min(B, args.restated)):
            want, end = R.Planner(audio[b * n:(b + 1) * n].cpu().numpy(), R.Config(**R.MODES["path_b"])).plan()
            got = plan_b.windows[plan_b.windows["recording"] == b]
            same = same and end == plan_b.speech_end[b] and [int(w["chunk_start"]) for w in got] == [w["chunk_start"] for w in want] and \
                [int(w["length"]) for w in got] == [w["length"] for w in want] and [int(w["warmup_samples"]) for w in got] == [w["warmup_samples"] for w in want]
        ok = ok and same
        targets = (n - 1) // 207360
        audio_bytes = 4 * B * n
        out[name] = {"recordings": B, "samples_each": n, "windows": int(plan_b.window_range[-1]), "targets_each": targets,
                     "plan_path_c_ms": 1e3 * t_c, "plan_path_c_spread": s_c, "plan_path_b_ms": 1e3 * t_b, "plan_path_b_spread": s_b,
                     "gate_no_spans_ms": 1e3 * t_gate, "gate_spread": s_gate, "pack_ms": 1e3 * t_pack, "pack_spread": s_pack,
                     "plan_and_pack_ms": 1e3 * (t_b + t_pack),
                     "audio_bytes": audio_bytes, "hbm_floor_ms": 1e3 * audio_bytes / HBM_PEAK,
                     "energy_share_of_hbm_bound_at_least": audio_bytes / HBM_PEAK / min(t_c, t_gate),
                     "chain_step_us": 1e6 * (t_b - t_c) / max(targets, 1),
                     "pack_bytes": pack_bytes, "pack_share_of_hbm_peak": pack_bytes / HBM_PEAK / t_pack,
                     "host_single_thread_plan_ms_one_recording": cpu_plan_ms, "host_single_thread_pack_ms_one_recording": cpu_pack_ms,
                     "host_single_thread_plan_and_pack_ms_scaled": (cpu_plan_ms + cpu_pack_ms) * B, "matches_restatement": bool(same)}
        del audio
    out["matches_restatement"] = bool(ok)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
