"""Times the Nemotron streaming session's gate and track steps on one device: device events round windows of calls on resident operands,
after a warm-up.  Prints one JSON line.  Usage: python scripts/rnnt_stream_timing.py [streams] [chunk_ms]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidaudio_amd as fa  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
MS = int(sys.argv[2]) if len(sys.argv) > 2 else 2240
W, WINDOWS, CALLS, WARM, REPEATS = 1280, (int(sys.argv[2]) if len(sys.argv) > 2 else 2240) // 80, 20, 5, 5
ctx = fa.default_context(0)
st = fa.RnntStreamState(B, fa.RnntStreamConfig(total_mel_frames=9 + MS // 10, vad_rms_threshold=0.003), ctx)
rng = np.random.default_rng(0)
loud = rng.random((B, WINDOWS)) < 0.5
amp = np.repeat(np.where(loud, 0.05, 0.0005), W, axis=1)
chunks = torch.from_numpy((rng.uniform(-1, 1, (B, WINDOWS * W)) * amp).astype(np.float32)).cuda()
# a lexical token every fourth frame: the spans emitted, as they do when the decode is healthy
T = (WARM + CALLS * REPEATS * 2) * WINDOWS // 4 + 1
frames = torch.arange(T, dtype=torch.int32, device="cuda").mul(4).repeat(B, 1).contiguous()
ids = torch.ones((B, T), dtype=torch.int32, device="cuda")
count = torch.full((B,), T, dtype=torch.int32, device="cuda")
table = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
gate_out, tracked = None, None


def gate():
    global gate_out
    gate_out = st.gate_dev(chunks, out=gate_out)


def track():
    global tracked
    tracked = st.track_dev(chunks, frames, ids, count, table, WINDOWS * W, 64, 64 * 3 * WINDOWS * W, out=tracked)


def timed(step):
    for _ in range(WARM):
        step()
    ctx.synchronize()
    windows = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            step()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) * 1000.0 / CALLS)
    return windows


g, t = timed(gate), timed(track)
chunk_bytes = B * WINDOWS * W * 4
print(json.dumps({"streams": B, "chunk_ms": MS, "chunk_bytes": chunk_bytes, "gate_us": [round(x, 1) for x in g], "track_us": [round(x, 1) for x in t],
                  "gate_hbm_share_of_8TBps": round(chunk_bytes / (min(g) * 1e-6) / 8e12, 3), "track_read_bytes": 2 * chunk_bytes, "track_written_bytes": chunk_bytes,
                  "track_hbm_share_of_8TBps": round(3 * chunk_bytes / (min(t) * 1e-6) / 8e12, 3), "requests_last_call": int(tracked.request_count.cpu()[0])}))
