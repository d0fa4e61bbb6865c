"""The LS-EEND front end on the device (fluidaudio_amd/csrc/lseend.hip) against a float64 restatement of the arithmetic
include/fluidaudio_hip.h states, at EEND geometry, on a batch of a recording of 8 tiles, one of 300 samples and an empty one.

Three checks on the values.  (1) Every slot that holds the same frame holds the same bits.  (2) The normalisation alone: with the
un-normalised rows x the same call hands out, the windows are within 2^-23 max|x| of the float64 cumulative mean of those rows (one
rounding of the mean, one of the subtraction); a lost or doubled tile carry is an error of the size of the mean, above 0.1 here.
(3) End to end: max|device - float64| <= 4 max|float32 emulation - float64|, the emulation being the reference's own method (DFT by a
float32 matmul, then the sequential fp32 recurrence of vDSP_vintb).  Counts, masks and warm-up counts equal the host plan exactly.
Measured on an MI355X (the same for chunk 1 and 5, offline and streamed): long recording CMN alone 5.35e-07 (bound 1.19e-06), device
2.32e-06, emulation 1.61e-06; short recording 4.77e-07, device 1.82e-06, emulation 5.07e-06; the empty one is exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIN, HOP, NFFT, MELS, CTX, SUB, DELAY, FLOOR = 200, 80, 256, 23, 7, 10, 9, float(np.float32(1e-10))
LENGTHS = [20000, 300, 0]                  # 250+ frames = 8 tiles of 32 (lseend_core.h: kTileFrames); a few hundred samples; empty
PIECES = [1, 79, 800, 4001]


@functools.lru_cache(None)
def waves():
    rng = np.random.default_rng(7)
    return [(rng.standard_normal(n) * np.linspace(0.02, 0.5, n)).astype(np.float32) for n in LENGTHS]   # noise on a slow ramp: the mean keeps moving


@functools.lru_cache(None)
def tables(fa):
    """the featurizer's own fp32 tables (they are part of the definition): the window centred in n_fft, the Slaney bank"""
    import ctypes as C
    cfg = fa.AudioMelSpectrogram(sample_rate=8000, n_mels=MELS, n_fft=NFFT, hop_length=HOP, win_length=WIN, window_periodic=True).config()
    win, bank = np.zeros(WIN, np.float32), np.zeros((MELS, NFFT // 2 + 1), np.float32)
    assert fa.lib().fa_mel_hann_window(C.byref(cfg), win.ctypes.data) == 0 and fa.lib().fa_mel_filterbank(C.byref(cfg), bank.ctypes.data) == 0
    return np.pad(win, ((NFFT - WIN) // 2,) * 2), bank


def rows_of(fa, x, plan, dtype):
    """un-normalised log10-mel rows and normalised rows of one recording, pushed whole and flushed, in dtype"""
    win, bank = (t.astype(dtype) for t in tables(fa))
    q = np.concatenate([np.zeros(NFFT // 2), x, np.zeros(plan.flush_samples)]).astype(dtype)
    fr = q[np.arange(plan.frames)[:, None] * HOP + np.arange(NFFT)[None]] * win
    if dtype == np.float64:
        power = np.abs(np.fft.rfft(fr, axis=1)) ** 2
    else:
        a = 2 * np.pi * np.outer(np.arange(NFFT), np.arange(NFFT // 2 + 1)) / NFFT
        power = (fr @ np.cos(a).astype(dtype)) ** 2 + (fr @ np.sin(a).astype(dtype)) ** 2
    x = np.log(np.maximum(power @ bank.T, dtype(FLOOR))) * dtype(1.0 / np.log(10.0))
    return x, cmn(x, dtype)


def cmn(x, dtype):
    if dtype == np.float64:
        return x - np.cumsum(x.astype(np.float64), axis=0) / np.arange(1, len(x) + 1)[:, None]
    mu, y = np.zeros(x.shape[1], np.float32), np.empty_like(x)
    for k in range(len(x)):                      # vDSP_vintb: mu + (x - mu) * (1 / k), then x - mu
        mu = mu + (x[k] - mu) * (np.float32(1) / np.float32(k + 1))
        y[k] = x[k] - mu
    return y


def windows_of(y, chunk, count):
    q = np.concatenate([np.zeros((CTX, MELS), y.dtype), y])
    mf = (chunk - 1) * SUB + 2 * CTX + 1
    return np.stack([q[c * SUB * chunk:c * SUB * chunk + mf] for c in range(count)])


@functools.lru_cache(None)
def offline(fa, ctx, chunk):
    """the offline call on the batch: computed once per chunk size, shared, left unchanged"""
    cfg = fa.lseend_config(chunk_size=chunk)
    out = fa.lseend_features(waves(), cfg=cfg, ctx=ctx)
    for a in out[:5]:
        a.setflags(write=False)
    return cfg, out


def check_values(fa, got_windows, raw, wave, plan, chunk, what):
    """checks (1), (2) and (3) on one recording's windows and rows"""
    W = len(got_windows)
    first = np.zeros((plan.frames, MELS), np.float32)         # frame f as its last slot holds it
    for c in range(W):
        lo = max(0, CTX - c * SUB * chunk)
        f0 = c * SUB * chunk + lo - CTX
        first[f0:f0 + got_windows.shape[1] - lo] = got_windows[c, lo:]
    assert np.array_equal(got_windows.view(np.uint32), windows_of(first, chunk, W).view(np.uint32)), f"{what}: slots of one frame differ, or a context row is not zero"
    mean = np.cumsum(raw.astype(np.float64), axis=0) / np.arange(1, len(raw) + 1)[:, None]
    assert np.abs(mean).min() > 0.1, "the input, not the bound, has to change"
    cmn_err = np.abs(got_windows - windows_of(cmn(raw, np.float64), chunk, W)).max()
    bound = 2.0 ** -23 * np.abs(raw).max()
    x64, y64 = rows_of(fa, wave, plan, np.float64)
    dev_err = np.abs(got_windows - windows_of(y64, chunk, W)).max()
    emu_err = np.abs(windows_of(rows_of(fa, wave, plan, np.float32)[1], chunk, W) - windows_of(y64, chunk, W)).max()
    print(f"lseend {what} chunk {chunk}: CMN alone {cmn_err:.3e} (bound {bound:.3e}); max|device - float64| {dev_err:.3e}, max|float32 emulation - float64| {emu_err:.3e}")
    assert cmn_err <= bound, (cmn_err, bound)
    assert dev_err <= 4 * emu_err, (dev_err, emu_err)


@pytest.mark.parametrize("chunk", [1, 5])
def test_offline_geometry_is_the_plan_and_values_meet_both_bounds(fa, gpu_ctx, chunk):
    cfg, out = offline(fa, gpu_ctx, chunk)
    plans, warmups, masks = fa.lseend_plan_file(LENGTHS, cfg)
    W, F = sum(p.windows for p in plans), sum(p.frames for p in plans)
    assert out.windows.shape == (W, fa.lseend_mel_frames(cfg), MELS) and out.raw.shape == (F, MELS) and plans[0].frames >= 8 * 32
    assert np.array_equal(out.warmups, warmups) and np.array_equal(out.masks, masks)
    for p in plans:                                           # per recording: the literal rule of emitNextChunk, rows in the dense output
        fed = np.arange(p.windows) * chunk
        assert out.warmups[p.window0:p.window0 + p.windows].tolist() == np.clip(DELAY - fed, 0, chunk).tolist()
        assert out.masks[p.window0:p.window0 + p.windows].tolist() == (np.minimum(fed, DELAY)[:, None] + np.arange(chunk)[None] >= DELAY).astype(float).tolist()
        assert out.out_rows[p.window0:p.window0 + p.windows].tolist() == (p.out_row0 + np.maximum(fed - DELAY, 0)).tolist()
    assert plans[2].frames > 0 and plans[2].windows > 0       # the empty recording: the flush windows alone
    for b, p in enumerate(plans):
        check_values(fa, out.windows[p.window0:p.window0 + p.windows], out.raw[p.frame0:p.frame0 + p.frames], waves()[b], p, chunk, f"offline[{b}]")


@pytest.mark.parametrize("chunk", [1, 5])
def test_stream_in_odd_pieces_equals_the_offline_geometry_and_meets_the_bounds(fa, gpu_ctx, chunk):
    cfg, off = offline(fa, gpu_ctx, chunk)
    plans = off.plans
    st = fa.LseendStream(streams=2, max_push_samples=max(PIECES), cfg=cfg, ctx=gpu_ctx)
    got = [dict(windows=[], masks=[], warmups=[], raw=[]) for _ in range(2)]

    def push(pieces, flush=False):
        r = st.push(pieces, flush)
        for s, p in enumerate(r.plans):
            got[s]["windows"].append(r.windows[p.window0:p.window0 + p.windows]); got[s]["masks"].append(r.masks[p.window0:p.window0 + p.windows])
            got[s]["warmups"].append(r.warmups[p.window0:p.window0 + p.windows]); got[s]["raw"].append(r.raw[p.frame0:p.frame0 + p.frames])
        return r
    at, i, snap, replay = 0, 0, None, []
    while at < LENGTHS[0]:
        n = min(PIECES[i % 4], LENGTHS[0] - at)
        pieces = [waves()[0][at:at + n], waves()[1] if i == 0 else waves()[2]]     # stream 1: the short recording at once, then nothing
        if i == 9:                                            # get -> further pushes -> set -> the same pushes again: the same bits
            snap = [st.snapshot(0), st.snapshot(1)]
            kept = [{k: list(v) for k, v in g.items()} for g in got]
        r = push(pieces)
        if snap is not None and i in (9, 10):
            replay.append((pieces, r))
        if i == 10:
            st.rollback(snap[0], 0); st.rollback(snap[1], 1)
            for k in range(2):
                got[k] = kept[k]
            for pcs, first in replay:
                again = push(pcs)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:5], again[:5]))
        at, i = at + n, i + 1
    push([waves()[2], waves()[2]], True)
    st.close()
    for s in range(2):
        p = plans[s]
        w, raw = np.concatenate(got[s]["windows"]), np.concatenate(got[s]["raw"])
        assert len(w) == p.windows and len(raw) == p.frames
        assert np.array_equal(np.concatenate(got[s]["masks"]), off.masks[p.window0:p.window0 + p.windows])
        assert np.array_equal(np.concatenate(got[s]["warmups"]), off.warmups[p.window0:p.window0 + p.windows])
        check_values(fa, w, raw, waves()[s], p, chunk, f"stream[{s}]")


@pytest.mark.parametrize("chunk", [1, 5])
def test_gather_probs_is_numpy_slicing(fa, gpu_ctx, chunk):
    cfg, off = offline(fa, gpu_ctx, chunk)
    speakers, W = 4, len(off.warmups)
    probs = np.random.default_rng(chunk).random((W, chunk, speakers + 3), dtype=np.float32)[:, :, :speakers]
    total = sum(p.out_rows for p in off.plans)
    want = np.concatenate([probs[w, off.warmups[w]:] for w in range(W)])
    assert want.shape == (total, speakers) and total > 0
    assert np.array_equal(fa.lseend_gather_probs(probs, off.warmups, off.out_rows, speakers, total, ctx=gpu_ctx), want)
