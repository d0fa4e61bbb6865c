"""Times the LuxTTS prompt entry (fa_luxtts_prompt_dev: loudness, gain, fused 1024-point magnitude mel scaled into the speech condition)
on one MI355X and, beside it and in the same run, the generic mel plan (fa_mel_execute_dev with the LuxTTS configuration: power 1,
reflect, HTK, replicated tail), which is what served this mel before (DESIGN.md quotes the figures): --batch prompts of --seconds at
24 kHz resident in HBM.  The two alternate in blocks of --calls calls between a pair of device events on the context's stream, after a
warm-up block each; the median block and the spread over --blocks are printed, with the bytes each must move (audio in; the item's
speech-condition slab or the mel rows out) over the HBM roofline (8 TB/s).  The two outputs are compared first.  Not part of bench.py.
--dry prints the geometry and stops (no GPU needed)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import fluidaudio_amd as fa
    L = fa._lib
    cfg = fa.luxtts_config()
    n = int(a.seconds * cfg.sample_rate)
    plans, _ = fa.luxtts_plan([n] * a.batch, 80, 60, 1.0, cfg)
    frames = plans[0].prompt_frames
    bytes_prompt = a.batch * 4 * (2 * plans[0].samples + cfg.max_frames * cfg.n_mels)     # the audio twice (loudness, mel), the whole slab written
    bytes_mel = a.batch * 4 * (n + frames * cfg.n_mels)
    print(json.dumps(dict(batch=a.batch, samples=n, prompt_frames=frames, status=plans[0].status, prompt_bytes=bytes_prompt, mel_bytes=bytes_mel)))
    if a.dry:
        return
    import torch
    ctx = fa.default_context(0)
    offsets = np.arange(a.batch + 1, dtype=np.int64) * n
    mcfg = fa.LuxTtsMelExtractor(ctx=ctx).config()
    mplan = fa.MelPlan(ctx, mcfg, offsets, expected_frames=np.full(a.batch, frames, np.int32), frame_stride=frames)
    pcm = torch.randn(a.batch * n, device="cuda") * 0.2             # RMS 0.2: not boosted, so both paths see the same samples
    mout = torch.empty(mplan.out_shape(), device="cuda")
    session = fa.LuxTtsSession(a.batch, cfg, ctx)
    counts, ptok, ttok, speeds = np.full(a.batch, n, np.int64), np.full(a.batch, 80, np.int32), np.full(a.batch, 60, np.int32), np.ones(a.batch, np.float32)
    ctx.check(L.lib().fa_luxtts_session_begin(ctx.handle, session._h, counts.ctypes.data, ptok.ctypes.data, ttok.ctypes.data, speeds.ctypes.data, None), "fa_luxtts_session_begin")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream, device=0)

    def run_prompt():
        ctx.check(L.lib().fa_luxtts_prompt_dev(ctx.handle, session._h, pcm.data_ptr(), offsets.ctypes.data), "fa_luxtts_prompt_dev")

    def run_mel():
        mplan.execute(pcm, mout, order=False)

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls
    block(run_prompt), block(run_mel)
    speech = session.get("speech_condition")[:, :frames]
    diff = float(np.abs(speech - mout.cpu().numpy() * np.float32(cfg.feat_scale)).max())
    assert np.isfinite(speech).all() and diff < 1e-3, diff
    t = dict(prompt=[], mel=[])
    for _ in range(a.blocks):
        t["prompt"].append(block(run_prompt))
        t["mel"].append(block(run_mel))
    for name, nbytes in (("prompt", bytes_prompt), ("mel", bytes_mel)):
        ms = float(np.median(t[name]))
        print(json.dumps(dict(kernel=name, ms_per_call=round(ms, 4), min_ms=round(min(t[name]), 4), max_ms=round(max(t[name]), 4), bytes=nbytes,
                              hbm_roofline_fraction=round(nbytes / HBM_BYTES_PER_S / (ms * 1e-3), 4), max_abs_difference_between_the_two=diff)))
    mplan.close()
    session.close()


if __name__ == "__main__":
    main()
