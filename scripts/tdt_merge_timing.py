"""Numbers for fa_tdt_merge_windows_dev at a long-form batch: 64 recordings of 450 windows of 15 s (187 encoder frames, 2 s = 25 frames
of overlap) at about 4 tokens a second, each window dropping, substituting, inserting and shifting 5 % of its tokens, the windows
resident on the device as the greedy walk leaves them.  Prints one JSON line: the device time between the call's two events
(fa_ctx_set_timing) in total and per seam, the host-clock time of the call, and beside it what the call replaces — the device-to-host
copy of all windows, and the host fold itself: tests/cpu/tdt_merge_emul.cpp (the same merge code over a one-lane wave) built -O2
without sanitizers and timed on one core of the same machine, whose merged streams must equal the device's.  Fails without a GPU.

    python scripts/tdt_merge_timing.py [--recordings 64] [--windows 450] [--repeats 10] [--out profiles/tdt_merge_timing.json]"""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluidaudio_amd as fa  # noqa: E402
from fluidaudio_amd import _lib as L  # noqa: E402

FRAMES, OVERLAP_FRAMES, VOCAB, MAX_OUT, NOISE, DENSITY = 187, 25, 1024, 128, 0.05, 4.0 * 0.08


def recording(rng, n_windows):
    """[(ids, timestamps)] per window: one true stream seen through overlapping windows, with noise."""
    stride = FRAMES - OVERLAP_FRAMES
    total = stride * (n_windows - 1) + FRAMES
    ts = np.flatnonzero(rng.random(total) < DENSITY)
    ids = rng.integers(0, VOCAB, ts.size)
    out = []
    for k in range(n_windows):
        lo, hi = np.searchsorted(ts, [k * stride, k * stride + FRAMES])
        t, i = ts[lo:hi].copy(), ids[lo:hi].copy()
        u = rng.random((4, t.size))
        i[u[1] < NOISE] = rng.integers(0, VOCAB, int((u[1] < NOISE).sum()))
        t = np.clip(t + np.where(u[3] < NOISE, np.where(rng.random(t.size) < 0.5, 1, -1), 0), k * stride, k * stride + FRAMES - 1)
        keep = u[0] >= NOISE
        t, i = t[keep], i[keep]
        extra = np.flatnonzero(u[2][keep] < NOISE)
        t, i = np.insert(t, extra, t[extra]), np.insert(i, extra, rng.integers(0, VOCAB, extra.size))
        out.append((i[:MAX_OUT].astype(np.int32), t[:MAX_OUT].astype(np.int32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--windows", type=int, default=450)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host-fold", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tdt_merge_timing.py needs a GPU")

    rng = np.random.default_rng(2024)
    W = a.recordings * a.windows
    tok, tim, dur = np.zeros((W, MAX_OUT), np.int32), np.zeros((W, MAX_OUT), np.int32), np.ones((W, MAX_OUT), np.int32)
    conf = rng.random((W, MAX_OUT)).astype(np.float32)
    counts = np.zeros(W, np.int32)
    for r in range(a.recordings):
        for k, (i, t) in enumerate(recording(rng, a.windows)):
            w = r * a.windows + k
            tok[w, :i.size], tim[w, :i.size], counts[w] = i, t, i.size
    window_range = np.arange(0, W + 1, a.windows, dtype=np.int64)
    safe = (np.arange(VOCAB) % 3 != 0).astype(np.uint8)
    canon = np.full(VOCAB, -1, np.int32)
    canon[1::4], canon[2::4] = np.arange(1, VOCAB, 4), np.arange(1, VOCAB, 4)[:len(canon[2::4])]
    caps = fa.merge_capacity(counts, window_range)

    ctx = fa.default_context(0)
    d = [torch.from_numpy(x).cuda() for x in (tok, tim, dur, conf, counts)]
    torch.cuda.synchronize()
    lib = L.lib()
    lib.fa_ctx_set_timing(ctx.handle, 1)
    call = lambda: fa.merge_windows_dev(*d, window_range, splice_safe=safe, case_canon=canon, capacities=caps, ctx=ctx)   # noqa: E731
    host_ms, dev_ms, m = [], [], None
    for it in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        m = call()
        if it >= a.warmup:
            host_ms.append(1e3 * (time.perf_counter() - t0))
            dev_ms.append(lib.fa_ctx_last_device_ms(ctx.handle))
    lib.fa_ctx_set_timing(ctx.handle, 0)
    assert (m.statuses == 0).all()
    seams = W - a.recordings
    routes = np.bincount(m.routes[m.routes >= 0] & 15, minlength=5).tolist()

    copy_ms = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = [x.cpu() for x in d]
        copy_ms.append(1e3 * (time.perf_counter() - t0))
    del back

    res = dict(recordings=a.recordings, windows_per_recording=a.windows, seams=seams, tokens_in=int(counts.sum()), tokens_out=int(m.counts.sum()),
               routes_empty_concat_contiguous_lcs_midpoint=routes, device_ms_median=statistics.median(dev_ms), device_ms_min=min(dev_ms),
               device_us_per_seam=1e3 * statistics.median(dev_ms) / seams, call_ms_median=statistics.median(host_ms),
               d2h_copy_of_windows_ms_median=statistics.median(copy_ms), repeats=a.repeats)

    if not a.no_host_fold:
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "tdt_merge_fold")
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpu", "tdt_merge_emul.cpp"), "-o", exe], check=True)
            bits = np.ascontiguousarray(conf).view(np.uint32)
            lines = [f"{a.recordings} {VOCAB} 1 1 -1 {MAX_OUT} {(1280.0 / 16000.0).hex()} {2.0.hex()}", " ".join(map(str, safe.tolist())), " ".join(map(str, canon.tolist()))]
            for r in range(a.recordings):
                lines.append(f"{int(caps[r])} {a.windows}")
                for w in range(r * a.windows, (r + 1) * a.windows):
                    n = int(counts[w])
                    lines.append(f"{n} {n}")
                    lines.extend(f"{tok[w, i]} {tim[w, i]} 1 {bits[w, i]}" for i in range(n))
            text = "\n".join(lines) + "\n"
            t = subprocess.run([exe, "time", "3"], input=text, capture_output=True, text=True, check=True).stdout.split()
            res["host_fold_one_core_ms"] = 1e3 * float(t[1])
            res["host_fold_us_per_seam"] = 1e6 * float(t[1]) / seams
            # the host fold's streams are the device's
            out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
            flat = [x.cpu().numpy() for x in (m.tokens, m.timestamps, m.durations, m.confidences)]
            at = 0
            for r in range(a.recordings):
                head = out[at].split()
                assert head[0] == "R" and int(head[1]) == 0 and int(head[2]) == m.counts[r], (r, head)
                lo = int(m.out_range[r])
                for i in (0, int(m.counts[r]) // 2, int(m.counts[r]) - 1):
                    want = (int(flat[0][lo + i]), int(flat[1][lo + i]), int(flat[2][lo + i]), struct.unpack("<I", flat[3][lo + i].tobytes())[0])
                    assert tuple(int(v) for v in out[at + 1 + i].split()) == want, (r, i)
                at += int(head[2]) + 2
            res["host_fold_equals_device"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
