"""Times fa_speaker_db_assign_dev alone, the whole fa_online_chunk_finish_dev (and fa_speaker_db_distances_dev) on one MI355X (DESIGN.md quotes the figures): 256 and 4 096 streams, 3
items per stream and call, databases of 4 and 16 speakers per stream whose rings of 50 raw embeddings are full, every item close enough to
one of the stream's speakers to take the update path (the ring's re-average).  The rings are filled by the entry itself (warm-up calls);
then 200 launches on resident operands between two device events, ten windows, the median and the spread.  Next to each time: the bytes
a call must touch divided by 6.3 TB/s, the HBM rate a float4 copy reaches on this part.  --dry prints the plan and stops (no GPU needed)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12
ROW = 1024   # one embedding


def assign_bytes(streams, per, speakers, ring):
    """Per item on the update path: the item, every speaker's current row, the ring read back for the mean, the raw written, the current row
    written twice and read once; the slot scalars are noise beside them."""
    return streams * per * ROW * (1 + speakers + ring + 1 + 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    args = ap.parse_args()
    per, ring = 3, 50
    results = []
    for streams in (256, 4096):
        for speakers in (4, 16):
            need = assign_bytes(streams, per, speakers, ring)
            row = dict(streams=streams, per=per, speakers=speakers, ring=ring, assign_bytes=need, assign_floor_ms=need / HBM_BYTES_PER_S * 1e3,
                       distances_bytes=streams * per * ROW * (1 + speakers), state_mib=streams * speakers * (ring + 1) * ROW / 2 ** 20)
            row["distances_floor_ms"] = row["distances_bytes"] / HBM_BYTES_PER_S * 1e3
            if args.dry:
                print(json.dumps(row), flush=True)
                continue
            import torch
            import fluidaudio_amd as fa
            ctx = fa.default_context(0)
            lib = fa.lib()
            db = fa.SpeakerDatabase(streams, fa.SpeakerDbConfig(max_speakers=speakers, raw_capacity=ring), ctx=ctx)
            g = torch.Generator(device="cuda").manual_seed(streams + speakers)
            voices = torch.nn.functional.normalize(torch.randn((streams, speakers, 256), generator=g, device="cuda"), dim=2)
            dur = torch.full((streams, per), 2.0, device="cuda")

            def batch(c):   # items of call c: the stream's voices in turn, a little noise on each
                idx = (torch.arange(per, device="cuda") + per * c) % speakers
                noise = torch.nn.functional.normalize(torch.randn((streams, per, 256), generator=g, device="cuda"), dim=2)
                return (voices[:, idx] + 0.1 * noise).contiguous()

            fill = (speakers * (ring + 1) + per - 1) // per + 2
            kinds = None
            for c in range(fill):                       # creates the speakers, then fills every ring
                kinds = db.assign_dev(batch(c), dur, tick=c)
            torch.cuda.synchronize()
            ctx.synchronize()
            one = db.get(0, 1)
            assert one is not None and len(one.raw_embeddings) == ring and db.counts().tolist() == [speakers] * streams
            assert bool((kinds[:, :, 2] == fa.SPEAKER_KINDS.index("UPDATED")).all()), "the timed items must take the update path"
            pool = [batch(fill + k) for k in range(8)]
            out = torch.zeros((streams, per, 4), dtype=torch.int32, device="cuda")
            dist = torch.zeros((streams, per, speakers), dtype=torch.float32, device="cuda")
            own = torch.cuda.ExternalStream(ctx.stream, device=ctx.device)
            torch.cuda.synchronize()
            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

            def timed(launch):
                ms = []
                for _ in range(args.repeats + 2):   # two windows of warm-up
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(own)
                    for k in range(args.launches):
                        launch(k)
                    b.record(own)
                    b.synchronize()
                    ms.append(a.elapsed_time(b) / args.launches)
                ms = sorted(ms[2:])
                return ms[len(ms) // 2], (ms[-1] - ms[0]) / ms[len(ms) // 2]

            def do_assign(k):
                st = lib.fa_speaker_db_assign_dev(ctx.handle, db._h, p(pool[k % 8]), p(dur), None, per, 1000 + k, p(out))
                assert st == 0, st

            def do_dist(k):
                st = lib.fa_speaker_db_distances_dev(ctx.handle, db._h, p(pool[k % 8]), per, p(dist), None)
                assert st == 0, st

            row["assign_ms"], row["assign_spread"] = timed(do_assign)
            row["distances_ms"], row["distances_spread"] = timed(do_dist)
            row["assign_gb_s"] = need / row["assign_ms"] / 1e6
            # the whole finish for one chunk of 589 frames per stream: the gate, the same three assignments, the timed segments; the entry
            # synchronises once per call, so this is wall-clock per call (the launches, the wait and the records' copy), not device time
            import time
            frames = 589
            w = torch.zeros((streams, 1, frames, 3), device="cuda")
            for s3 in range(3):
                w[:, :, s3 * 196:(s3 + 1) * 196, s3] = 1.0
            act = torch.full((streams, 1, 3), 196.0, device="cuda")
            embs = [b.reshape(streams, 1, 3, 256).contiguous() for b in pool]
            off = np.zeros((streams, 1))
            seg = np.zeros(streams * 3, fa.ONLINE_SEGMENT_DTYPE)
            assign = torch.zeros((streams, 1, 3, 4), dtype=torch.int32, device="cuda")
            ccfg, n_seg = fa.OnlineChunkConfig().c(), C.c_int64()
            torch.cuda.synchronize()

            def do_finish(k):
                st = lib.fa_online_chunk_finish_dev(ctx.handle, C.byref(ccfg), db._h, p(w), p(act), p(embs[k % 8]), off.ctypes.data, 1, 2000 + k, seg.ctypes.data,
                                                    seg.size, C.byref(n_seg), None, p(assign))
                assert st == 0 and n_seg.value == 3 * streams, (st, n_seg.value)

            ms = []
            for _ in range(args.repeats + 2):
                t0 = time.perf_counter()
                for k in range(50):
                    do_finish(k)
                ms.append((time.perf_counter() - t0) / 50 * 1e3)
            ms = sorted(ms[2:])
            row["finish_ms"], row["finish_spread"] = ms[len(ms) // 2], (ms[-1] - ms[0]) / ms[len(ms) // 2]
            row["finish_bytes"] = need + streams * (2 * frames * 3 * 4 + 3 * ROW + 3 * 36)
            row["finish_floor_ms"] = row["finish_bytes"] / HBM_BYTES_PER_S * 1e3
            ctx.synchronize()
            assert bool((out[:, :, 2] == fa.SPEAKER_KINDS.index("UPDATED")).all())
            db.close()
            results.append(row)
            print(json.dumps(row), flush=True)
    if args.out and results:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
