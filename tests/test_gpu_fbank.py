"""Kaldi fbank -> LFR -> CMVN on the device (fluidaudio_amd/csrc/fbank.hip) against a plain float64 restatement of the arithmetic
include/fluidaudio_hip.h states, on one ragged batch that holds every length at which the kernel takes another path.

The values: max|device - float64| has to stay within 4 x max|float32 emulation - float64| on the pre-CMVN log-fbank of the synth
inputs, the emulation being the reference's own method (steps 1-5 in float32, the DFT a float32 matmul against a cos / sin basis).
Everything else is exact by construction: row counts, the zero fill, the (row, slot) placement and the CMVN (bit-equal to the
m = n = 1 output gathered on the host), the silent and the constant utterance, caller-supplied tables.
Measured on an MI355X (Hamming / Povey): device 2.67e-04 / 3.16e-04, emulation 2.45e-04 / 1.73e-04."""
import functools

import numpy as np
import pytest

from conftest import synth_audio

pytestmark = pytest.mark.gpu

WIN, HOP, NFFT, MELS, FLOOR = 400, 160, 512, 80, np.float32(1.1920929e-07)
TILE = 32                                                     # frames per workgroup (fbank_core.h: kTileFrames)
FRAMES = [1, 1, 2, 3, 4, 6, 7, 13, TILE, TILE + 1, 2 * TILE + 6]     # T of the synth utterances (the first two: 400 and 559 samples)
SAMPLES = [0, 399, 400, 559, 560] + [WIN + (t - 1) * HOP + 37 * (t % 3) for t in FRAMES[3:]]
SILENT, CONSTANT = len(SAMPLES), len(SAMPLES) + 1             # two more utterances of 8 frames: all zero, all 0.5


@functools.lru_cache(None)
def batch():
    waves = [synth_audio(n, seed=n) + np.float32(0.25) for n in SAMPLES]
    return waves + [np.zeros(WIN + 7 * HOP, np.float32), np.full(WIN + 7 * HOP, 0.5, np.float32)]


@functools.lru_cache(None)
def tables(window):
    i = np.arange(WIN) * 2 * np.pi / (WIN - 1)
    w = 0.54 - 0.46 * np.cos(i) if window == "hamming" else (0.5 - 0.5 * np.cos(i)) ** 0.85
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    pts = np.linspace(mel(20.0), mel(8000.0), MELS + 2)
    mk = mel(np.arange(NFFT // 2) * 16000.0 / NFFT)
    up = (mk[None] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    down = (pts[2:, None] - mk[None]) / (pts[2:] - pts[1:-1])[:, None]
    bank = np.zeros((MELS, NFFT // 2 + 1))
    bank[:, :NFFT // 2] = np.maximum(0.0, np.minimum(up, down))
    return w.astype(np.float32), bank.astype(np.float32)


def log_fbank(x, window, dtype):
    """steps 1-5 for one utterance -> (log-fbank [T, MELS], smallest mel energy); float64: np.fft.rfft, float32: a DFT by matmul"""
    w, bank = (t.astype(dtype) for t in tables(window))
    T = 0 if x.size < WIN else 1 + (x.size - WIN) // HOP
    x = x.astype(dtype) * dtype(32768)
    fr = np.stack([x[t * HOP:t * HOP + WIN] for t in range(T)]) if T else np.zeros((0, WIN), dtype)
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    fr = (fr - dtype(0.97) * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)) * w
    if dtype == np.float64:
        power = np.abs(np.fft.rfft(fr, NFFT, axis=1)) ** 2
    else:
        a = 2 * np.pi * np.outer(np.arange(WIN), np.arange(NFFT // 2 + 1)) / NFFT
        power = (fr @ np.cos(a).astype(dtype)) ** 2 + (fr @ np.sin(a).astype(dtype)) ** 2
    e = power @ bank.T
    return np.log(np.maximum(e, dtype(FLOOR))), (e.min() if T else np.inf)


def stacked(feats, m, n, tail, shift, scale, row_stride):
    """steps 6-7 in float32 on per-utterance [T, MELS] features -> ([B, row_stride, m MELS], rows)"""
    out, rows = np.zeros((len(feats), row_stride, m * MELS), np.float32), []
    for b, f in enumerate(feats):
        T, lpad = len(f), (m - 1) // 2
        R = 0 if T == 0 else -(-T // n) if tail == "replicate" else max(0, (T + lpad - m) // n + 1)
        idx = np.clip(np.arange(R)[:, None] * n + np.arange(m)[None] - lpad, 0, T - 1)
        v = f[idx].reshape(R, m * MELS)
        out[b, :R] = (v if shift is None else (v + shift) * scale)
        rows.append(R)
    return out, np.array(rows, np.int32)


@functools.lru_cache(None)
def plain(fa, ctx, window):
    """the device's m = n = 1 output without CMVN, per utterance [T, MELS]: computed once, shared, left unchanged"""
    cfg = fa.fbank_config(window_type=window, lfr_m=1, lfr_n=1)
    out, rows = fa.fbank_batch(batch(), cfg=cfg, ctx=ctx)
    frames = [0, 0] + FRAMES + [8, 8]
    assert rows.tolist() == frames and out.shape == (len(frames), max(frames), MELS)
    for b, t in enumerate(frames):
        assert not out[b, t:].any(), b
    return [out[b, :t].copy() for b, t in enumerate(frames)]


@pytest.mark.parametrize("window", ["hamming", "povey"])
def test_values_within_four_times_the_float32_emulation(fa, gpu_ctx, window):
    got = plain(fa, gpu_ctx, window)
    dev_err = emu_err = 0.0
    for b in range(2, len(SAMPLES)):
        ref, floor = log_fbank(batch()[b], window, np.float64)
        assert floor > 1e3 * FLOOR, "the input, not the bound, has to change"
        dev_err = max(dev_err, np.abs(got[b] - ref).max())
        emu_err = max(emu_err, np.abs(log_fbank(batch()[b], window, np.float32)[0] - ref).max())
    print(f"fbank {window}: max|device - float64| {dev_err:.3e}, max|float32 emulation - float64| {emu_err:.3e}")
    assert dev_err <= 4 * emu_err, (dev_err, emu_err)
    # a silent frame and a constant one (its scaled value and its frame sum are exact in fp32) sit on the floor, exactly
    assert np.all(got[SILENT] == np.float32(np.log(np.float64(FLOOR)))) and np.all(got[CONSTANT] == got[SILENT])


@pytest.mark.parametrize("cmvn", [False, True])
@pytest.mark.parametrize("window", ["hamming", "povey"])
@pytest.mark.parametrize("m,n,tail", [(1, 1, "replicate"), (7, 6, "replicate"), (5, 1, "valid")])
def test_rows_placement_and_cmvn_are_exact(fa, gpu_ctx, m, n, tail, window, cmvn):
    rng = np.random.default_rng(m)
    shift = rng.uniform(-12, -4, m * MELS).astype(np.float32) if cmvn else None
    scale = rng.uniform(0.1, 0.4, m * MELS).astype(np.float32) if cmvn else None
    cfg = fa.fbank_config(window_type=window, lfr_m=m, lfr_n=n, tail_mode=tail)
    stride = fa.fbank_num_rows(cfg, max(FRAMES)) + 3
    got, rows = fa.fbank_batch(batch(), cfg=cfg, shift=shift, scale=scale, row_stride=stride, ctx=gpu_ctx)
    want, want_rows = stacked(plain(fa, gpu_ctx, window), m, n, tail, shift, scale, stride)
    assert rows.tolist() == want_rows.tolist()
    assert np.array_equal(got, want)


def test_caller_tables_equal_to_the_built_in_ones_change_nothing(fa, gpu_ctx):
    cfg = fa.fbank_config()
    own = fa.fbank_config(window=fa.fbank_window(cfg), filterbank=fa.fbank_filterbank(cfg))
    assert np.abs(fa.fbank_window(cfg) - tables("hamming")[0]).max() < 1e-7 and np.abs(fa.fbank_filterbank(cfg) - tables("hamming")[1]).max() < 1e-6
    a, b = fa.fbank_batch(batch(), cfg=cfg, ctx=gpu_ctx), fa.fbank_batch(batch(), cfg=own, ctx=gpu_ctx)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()
