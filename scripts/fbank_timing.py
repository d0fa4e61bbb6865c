"""Times the Kaldi fbank + LFR + CMVN plan (fa_fbank_execute_dev, WavFrontend configuration) on one MI355X and, beside it and in the same
run, fa_mel_execute_dev on the same batch, the nearest thing the library had before (DESIGN.md and the README quote the figures): 1024
utterances of 15 s resident in HBM, plan execution only.  The two alternate in blocks of --calls launches between a pair of device
events on the context's stream, after a warm-up block each; the median block and the spread over --blocks are printed, with the
fraction of the HBM roofline (8 TB/s): per utterance 960 000 B in and R * 560 * 4 B (fbank) or 128 * T * 4 B (mel) out.  Not part of
bench.py.  --dry prints the geometry and stops (no GPU needed)."""
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import fluidaudio_amd as fa
    L = fa._lib
    n = int(a.seconds * 16000)
    cfg = fa.fbank_config()
    rows = fa.fbank_num_rows(cfg, fa.fbank_num_frames(cfg, n))
    width = cfg.lfr_m * cfg.n_mels
    bytes_fbank = a.batch * (4 * n + rows * width * 4)
    print(json.dumps(dict(batch=a.batch, samples=n, rows=rows, width=width, fbank_bytes=bytes_fbank)))
    if a.dry:
        return
    import torch
    ctx = fa.default_context(0)
    mel = fa.AudioMelSpectrogram(ctx=ctx)
    mcfg = mel.config()
    offsets = np.arange(a.batch + 1, dtype=np.int64) * n
    rng = np.random.default_rng(0)
    shift, scale = rng.uniform(-12, -4, width).astype(np.float32), rng.uniform(0.1, 0.4, width).astype(np.float32)
    plan = C.c_void_p()
    ctx.check(L.lib().fa_fbank_plan_create(ctx.handle, C.byref(cfg), offsets.ctypes.data, a.batch, shift.ctypes.data, scale.ctypes.data, rows, C.byref(plan)), "fa_fbank_plan_create")
    mplan = mel.plan(offsets)
    frames = mplan.frame_stride
    bytes_mel = a.batch * (4 * n + mcfg.n_mels * L.lib().fa_mel_num_frames(C.byref(mcfg), n) * 4)
    pcm = (torch.rand(a.batch * n, device="cuda") * 2 - 1) * 0.5
    out = torch.empty((a.batch, rows, width), device="cuda")
    d_rows = torch.empty(a.batch, dtype=torch.int32, device="cuda")
    mout = torch.empty(mplan.out_shape(), device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream, device=0)

    def run_fbank():
        ctx.check(L.lib().fa_fbank_execute_dev(plan, pcm.data_ptr(), out.data_ptr(), d_rows.data_ptr()), "fa_fbank_execute_dev")

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
    block(run_fbank), block(run_mel)
    t = dict(fbank=[], mel=[])
    for _ in range(a.blocks):
        t["fbank"].append(block(run_fbank))
        t["mel"].append(block(run_mel))
    assert int(d_rows.min()) == rows == int(d_rows.max()) and bool(torch.isfinite(out).all())
    for name, nbytes in (("fbank", bytes_fbank), ("mel", bytes_mel)):
        ms = float(np.median(t[name]))
        print(json.dumps(dict(kernel=name, ms_per_call=round(ms, 4), min_ms=round(min(t[name]), 4), max_ms=round(max(t[name]), 4), bytes=nbytes,
                              hbm_roofline_fraction=round(nbytes / HBM_BYTES_PER_S / (ms * 1e-3), 3), frames=frames if name == "mel" else rows)))
    L.lib().fa_fbank_plan_destroy(plan)
    mplan.close()


if __name__ == "__main__":
    main()
