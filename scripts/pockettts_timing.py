"""Times two entries of the PocketTTS session (csrc/pockettts.hip) on one MI355X (DESIGN.md quotes the figures): the fused conditioning
extraction + re-projection (fa_pockettts_clone_dev) for --clones clones of 125 frames resident in HBM, beside torch.matmul on the same
tensors in the same run ((cond @ Pinv) @ W.T, two rocBLAS calls with the latents through HBM), and the KV cache reset
(fa_pockettts_kv_reset) for --streams streams x --layers layers from a snapshot of --src-seq positions in each at-rest format, as a share
of the HBM roofline (8 TB/s) for the bytes it must move: the snapshot rows in, the full slabs out.  The calls run in blocks of --calls
between a pair of device events on the context's stream after a warm-up block each, the clone and the matmul alternating; the median block
and the spread over --blocks are printed.  Not part of bench.py.  --dry prints the geometry and stops (no GPU needed)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12
FORMATS = ("combined", "split", "fp16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clones", type=int, default=256)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--src-seq", type=int, default=126)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import fluidaudio_amd as fa
    L = fa._lib
    B, S, layers, seq, frames = a.clones, a.streams, a.layers, a.src_seq, 125
    clone_bytes = 4 * (2 * B * frames * 1024 + 2 * 1024 * 32)                     # the conditioning in, the voice rows out, both matrices once
    kv_bytes = {f: S * layers * 2 * 1024 * (seq * 4 + 512 * (2 if f == "fp16" else 4)) for f in FORMATS}
    print(json.dumps(dict(clones=B, frames=frames, clone_bytes=clone_bytes, streams=S, layers=layers, src_seq=seq, kv_bytes=kv_bytes)))
    if a.dry:
        return
    import torch
    ctx = fa.default_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream, device=0)

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def report(name, times, nbytes, **more):
        ms = float(np.median(times))
        print(json.dumps(dict(kernel=name, ms_per_call=round(ms, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4), bytes=nbytes,
                              hbm_roofline_fraction=round(nbytes / HBM_BYTES_PER_S / (ms * 1e-3), 4), **more)))

    rng = np.random.default_rng(0)
    s = fa.PocketTtsSession(fa.pockettts_config(layers=1, streams=1, voices=B, voice_seq=1, projections=1, vocab=1, windows=1, clones=B, max_frames=1), ctx)
    pinv, w = rng.standard_normal((1024, 32)).astype(np.float32) / 32, rng.standard_normal((1024, 32)).astype(np.float32) / 6
    s.set_projection(0, pinv, w)
    cond = torch.randn(B, frames, 1024, device="cuda")
    d_pinv, d_w, out = torch.from_numpy(pinv).cuda(), torch.from_numpy(w).cuda(), torch.empty(B, frames, 1024, device="cuda")
    voices, projs, usable = np.arange(B, dtype=np.int32), np.zeros(B, np.int32), np.full(B, frames, np.int32)
    torch.cuda.synchronize()

    def run_clone():
        ctx.check(L.lib().fa_pockettts_clone_dev(ctx.handle, s._h, B, voices.ctypes.data, projs.ctypes.data, usable.ctypes.data, cond.data_ptr(), 0, frames * 1024, 1024, 1),
                  "fa_pockettts_clone_dev")

    def run_matmul():
        with torch.cuda.stream(stream):
            torch.matmul(torch.matmul(cond, d_pinv), d_w.T, out=out)
    block(run_clone), block(run_matmul)
    got = s.get("voice_rows", 0, B * frames * 1024).reshape(B, frames, 1024)
    diff = float(np.abs(got - out.cpu().numpy()).max())
    t = dict(clone=[], matmul=[])
    for _ in range(a.blocks):
        t["clone"].append(block(run_clone))
        t["matmul"].append(block(run_matmul))
    report("clone", t["clone"], clone_bytes, max_abs_difference_from_torch=diff)
    report("torch_matmul_pair", t["matmul"], clone_bytes + 2 * 4 * B * frames * 32)
    s.close()

    layer_caches = [rng.standard_normal(2 * seq * 1024).astype(np.float32) for _ in range(layers)]
    streams, zeros = np.arange(S, dtype=np.int32), np.zeros(S, np.int32)
    for name in FORMATS:
        s = fa.PocketTtsSession(fa.pockettts_config(layers=layers, kv_format=name, streams=S, voices=1, voice_seq=512, projections=0, vocab=1, windows=1, clones=1, max_frames=1), ctx)
        assert s.add_voice(0, layer_caches, [seq] * layers, seq) == 0

        def run_reset():
            ctx.check(L.lib().fa_pockettts_kv_reset(ctx.handle, s._h, S, streams.ctypes.data, zeros.ctypes.data), "fa_pockettts_kv_reset")
        block(run_reset)
        plane = s.kv_plane(S - 1, layers - 1, 1)
        assert np.array_equal(plane[:seq].astype(np.float32), layer_caches[-1][seq * 1024:].reshape(seq, 1024).astype(plane.dtype).astype(np.float32)) and not plane[seq:].any()
        report("kv_reset_" + name, [block(run_reset) for _ in range(a.blocks)], kv_bytes[name])
        s.close()


if __name__ == "__main__":
    main()
