"""Times the offline LS-EEND front end (fa_lseend_features_dev: mel, log10, cumulative mean, windows, masks; EEND geometry, chunk 5) on
one MI355X and, beside it and in the same run, the generic mel kernel alone (fa_mel_execute_dev, LS-EEND flavour, n_fft 256, frame-major)
on the same batch, the part of this work the library served before (DESIGN.md quotes the figures): --batch recordings of --seconds at
8 kHz resident in HBM.  The two alternate in blocks of --calls calls between a pair of device events on the context's stream, after a
warm-up block each; the median block and the spread over --blocks are printed, with the bytes each must move (audio in; windows, masks,
warm-up counts and row offsets out, or the mel rows out) over the HBM roofline (8 TB/s).  Not part of bench.py.  --dry prints the
geometry and stops (no GPU needed)."""
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import fluidaudio_amd as fa
    L = fa._lib
    n = int(a.seconds * 8000)
    cfg = fa.lseend_config()
    plans, _, _ = fa.lseend_plan_file([n] * a.batch, cfg)
    W, F, mf = plans[-1].window0 + plans[-1].windows, plans[-1].frame0 + plans[-1].frames, fa.lseend_mel_frames(cfg)
    bytes_lseend = a.batch * 4 * n + W * (mf * cfg.n_mels * 4 + cfg.chunk_size * 4 + 4 + 8)
    print(json.dumps(dict(batch=a.batch, samples=n, frames=F, windows=W, mel_frames=mf, lseend_bytes=bytes_lseend)))
    if a.dry:
        return
    import torch
    ctx = fa.default_context(0)
    mel = fa.AudioMelSpectrogram(sample_rate=8000, n_mels=cfg.n_mels, n_fft=cfg.n_fft, hop_length=cfg.hop, win_length=cfg.win, preemph=0.0, log_floor=1e-10,
                                 log_floor_mode="clamped", window_periodic=True, ctx=ctx)
    offsets = np.arange(a.batch + 1, dtype=np.int64) * n
    mplan = mel.plan(offsets, layout="frame_major", padding_mode="prepadded")
    mshape = mplan.out_shape()
    bytes_mel = a.batch * 4 * n + int(np.prod(mshape)) * 4
    pcm = torch.randn(a.batch * n, device="cuda") * torch.linspace(0.02, 0.5, a.batch * n, device="cuda")
    windows = torch.empty((W, mf, cfg.n_mels), device="cuda")
    masks = torch.empty((W, cfg.chunk_size), device="cuda")
    warmups = torch.empty(W, dtype=torch.int32, device="cuda")
    out_rows = torch.empty(W, dtype=torch.int64, device="cuda")
    mout = torch.empty(mshape, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream, device=0)

    def run_lseend():
        ctx.check(L.lib().fa_lseend_features_dev(ctx.handle, C.byref(cfg), pcm.data_ptr(), offsets.ctypes.data, a.batch, windows.data_ptr(), masks.data_ptr(),
                                                 warmups.data_ptr(), out_rows.data_ptr(), None), "fa_lseend_features_dev")

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
    block(run_lseend), block(run_mel)
    t = dict(lseend=[], mel=[])
    for _ in range(a.blocks):
        t["lseend"].append(block(run_lseend))
        t["mel"].append(block(run_mel))
    assert bool(torch.isfinite(windows).all()) and int(warmups.max()) == cfg.chunk_size and int(out_rows.max()) == plans[-1].out_row0 + plans[-1].out_rows - cfg.chunk_size
    for name, nbytes in (("lseend", bytes_lseend), ("mel", bytes_mel)):
        ms = float(np.median(t[name]))
        print(json.dumps(dict(kernel=name, ms_per_call=round(ms, 4), min_ms=round(min(t[name]), 4), max_ms=round(max(t[name]), 4), bytes=nbytes,
                              hbm_roofline_fraction=round(nbytes / HBM_BYTES_PER_S / (ms * 1e-3), 4))))
    mplan.close()


if __name__ == "__main__":
    main()
