"""Times the StyleTTS2 reference-mel entry (fa_styletts2_reference_mel_dev: the fused 2048-point power mel of csrc/styletts2.hip) on one
MI355X and, beside it and in the same run, the generic mel plan (fa_mel_execute_dev at n_fft 2048, window 1200, hop 300, power 2, reflect,
HTK for 16 kHz, additive floor), and the alignment entry (fa_styletts2_align_dev) at --batch items x 256 tokens of duration 8 (DESIGN.md
quotes the figures): --batch clips of --seconds at 24 kHz resident in HBM.  The calls run in blocks of --calls between a pair of device
events on the context's stream, the two mels alternating, after a warm-up block each; the median block and the spread over --blocks are
printed, with the bytes each must move over the HBM roofline (8 TB/s).  The two mels are compared first.  Not part of bench.py.  --dry
prints the geometry and stops (no GPU needed)."""
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
    n, B, tokens, dur = int(a.seconds * 24000), a.batch, 256, 8
    frames = n // 300 + 1
    stride = -(-frames // 16) * 16
    cfg = fa.styletts2_config(max_ref_frames=stride)
    total = tokens * dur
    bytes_mel = B * 4 * (n + cfg.n_mels * stride)                                  # the audio in, the whole mel slab out
    bytes_align = B * 4 * (tokens * (cfg.d_channels + cfg.asr_channels) + total * (cfg.d_channels + cfg.asr_channels))
    print(json.dumps(dict(batch=B, samples=n, ref_frames=frames, stride=stride, status=fa.styletts2_plan([n], tokens, cfg)[0].status, mel_bytes=bytes_mel, align_bytes=bytes_align)))
    if a.dry:
        return
    import torch
    ctx = fa.default_context(0)
    offsets = np.arange(B + 1, dtype=np.int64) * n
    mcfg = fa.LuxTtsMelExtractor(ctx=ctx).config()
    mcfg.sample_rate, mcfg.n_mels, mcfg.n_fft, mcfg.hop, mcfg.win, mcfg.power, mcfg.log_floor = 16000, 80, 2048, 300, 1200, 2.0, 1e-5
    mcfg.floor_mode, mcfg.layout, mcfg.tail_mode = 0, 0, 0                           # additive floor, [n_mels, frames], no replicated tail
    mplan = fa.MelPlan(ctx, mcfg, offsets, expected_frames=np.full(B, frames, np.int32), frame_stride=stride)
    pcm = torch.randn(B * n, device="cuda") * 0.2
    mout = torch.empty(mplan.out_shape(), device="cuda")
    session = fa.StyleTts2Session(B, cfg, ctx)
    counts, toks = np.full(B, n, np.int64), np.full(B, tokens, np.int32)
    ctx.check(L.lib().fa_styletts2_session_begin(ctx.handle, session._h, counts.ctypes.data, toks.ctypes.data, None), "fa_styletts2_session_begin")
    logits = torch.full((B, tokens, dur), 100.0, device="cuda")                      # every duration is `dur`
    totals = np.zeros(B, np.int32)
    ctx.check(L.lib().fa_styletts2_durations_dev(ctx.handle, session._h, logits.data_ptr(), dur, tokens * dur, dur, 1, totals.ctypes.data, None), "fa_styletts2_durations_dev")
    assert totals.tolist() == [total] * B
    d, t_en = torch.randn(B, tokens, cfg.d_channels, device="cuda"), torch.randn(B, cfg.asr_channels, tokens, device="cuda")
    en, asr = torch.empty(B, cfg.d_channels, total, device="cuda"), torch.empty(B, cfg.asr_channels, total, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream, device=0)

    def run_reference():
        ctx.check(L.lib().fa_styletts2_reference_mel_dev(ctx.handle, session._h, pcm.data_ptr(), offsets.ctypes.data), "fa_styletts2_reference_mel_dev")

    def run_mel():
        mplan.execute(pcm, mout, order=False)

    def run_align():
        ctx.check(L.lib().fa_styletts2_align_dev(ctx.handle, session._h, d.data_ptr(), cfg.d_channels, tokens * cfg.d_channels, t_en.data_ptr(), tokens, cfg.asr_channels * tokens, 1,
                                                 en.data_ptr(), asr.data_ptr(), total), "fa_styletts2_align_dev")

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls
    block(run_reference), block(run_mel), block(run_align)
    got = session.get("mel")[:, :, :frames]
    diff = float(np.abs(got - (mout.cpu().numpy().reshape(B, cfg.n_mels, -1)[:, :, :frames] + 4.0) / 4.0).max())
    tok = np.maximum(np.arange(total) - 1, 0) // dur
    assert np.isfinite(got).all() and torch.equal(en.cpu(), d.cpu()[:, tok].transpose(1, 2)) and torch.equal(asr.cpu(), t_en.cpu()[:, :, tok])
    t = dict(reference_mel=[], generic_mel=[], align=[])
    for _ in range(a.blocks):
        t["reference_mel"].append(block(run_reference))
        t["generic_mel"].append(block(run_mel))
        t["align"].append(block(run_align))
    for name, nbytes in (("reference_mel", bytes_mel), ("generic_mel", bytes_mel), ("align", bytes_align)):
        ms = float(np.median(t[name]))
        print(json.dumps(dict(kernel=name, ms_per_call=round(ms, 4), min_ms=round(min(t[name]), 4), max_ms=round(max(t[name]), 4), bytes=nbytes,
                              hbm_roofline_fraction=round(nbytes / HBM_BYTES_PER_S / (ms * 1e-3), 4), max_abs_difference_between_the_two_mels=diff)))
    mplan.close()
    session.close()


if __name__ == "__main__":
    main()
