"""The LuxTTS session on the device (fluidaudio_amd/csrc/luxtts.hip) against float64 / numpy restatements of the arithmetic
include/fluidaudio_hip.h states, on one batch of four prompts through one session: the reference's fixture prompt (RMS 0.135, not boosted,
838 frames over 165 tokens: 13 remainder frames, bucket 555), the same scaled by 0.2 (boosted, 282 generated frames exactly), 300 samples
of noise (one frame, clamped reflect indices) and 4 096 zeros (silent).

Speech condition: max|device - float64| <= 4 max|float32 emulation - float64|, the emulation being the reference's method in float32
(windowed frames times a float32 DFT matrix, magnitude, bank, log) on the same gained samples.  Measured on an MI355X: fixture prompt device 1.627e-05, emulation
1.801e-05; boosted 2.487e-05 against 2.691e-05; 300 samples 5.72e-08 against 4.98e-08; the fixture item is 7.42e-05 from the reference's own
golden mel (bound 1e-4).  (A single float32 FFT of the windowed frame is at 1.0e-4 on the fixture: its speech has 80 dB between the bands of
a frame.  The kernel takes the bins from 256 on from the transform of the frame's first difference, see luxtts.hip.)  Records are bit-equal
to the host order, the noise is bit-equal to numpy's float64 restatement on every element of the batch."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NFFT, HOP, MELS, FLOOR, SCALE, TARGET = 1024, 256, 100, np.float32(1e-7), np.float32(0.1), np.float32(0.1)
PROMPT_TOKENS, TEXT_TOKENS, SPEEDS = [80, 80, 1, 4], [85, 56, 3, 4], [1.0, 1.01, 1.0, 1.0]
SEEDS = np.array([42, 0, 2 ** 63 + 12345, 7], np.uint64)
STRIDE = 112                                # CoreML's padded row of 100 floats; the padding lanes hold NaN


@functools.lru_cache(None)
def waves():
    audio = np.load(os.path.join(os.path.dirname(__file__), "golden", "luxtts_prompt.npz"))["audio"]
    return [audio, (audio * np.float32(0.2)).astype(np.float32), (np.random.default_rng(3).standard_normal(300) * 0.3).astype(np.float32), np.zeros(4096, np.float32)]


def padded(rng, shape):
    a = np.full(shape[:2] + (STRIDE,), np.nan, np.float32)
    a[:, :, :MELS] = rng.standard_normal(shape[:2] + (MELS,)).astype(np.float32)
    return a


@functools.lru_cache(None)
def session(fa, ctx):
    """the whole flow once, every slab fetched after the call that writes it: shared by the tests, left unchanged"""
    rng, r = np.random.default_rng(11), {}
    s = fa.LuxTtsSession(4, ctx=ctx)
    r["plans"] = plans = s.prompt(waves(), PROMPT_TOKENS, TEXT_TOKENS, SPEEDS)
    r["records"], r["speech"] = s.get("records"), s.get("speech_condition")
    r["ids"] = [rng.integers(1, 300, p.tokens).astype(np.int32) for p in plans]
    s.inputs(r["ids"], SEEDS)
    r.update({k: s.get(k) for k in ("tokens", "token_mask", "frame_mask")}, x=[s.get("x")])
    r["embeds"] = padded(rng, (4, 256))
    s.text_condition(r["embeds"])
    r["text"] = s.get("text_condition")
    r["v"] = [padded(rng, (4, 1024)) for _ in range(4)]
    for step in range(4):
        s.step(step, r["v"][step])
        r["x"].append(s.get("x"))
    r["buckets"] = fa.luxtts_plan([w.size for w in waves()], PROMPT_TOKENS, TEXT_TOKENS, SPEEDS)[1]
    r["mel"] = {b: s.vocoder_input(b, items) for b, items in r["buckets"].items()}
    r["audio"] = (rng.standard_normal((4, max(p.sample_count for p in plans) + 24)) * 0.8).astype(np.float32)   # a row stride beyond the row, values beyond +-1
    r["out"] = s.finish(r["audio"])
    s.close()
    return r


def test_plan_has_the_cases(fa, gpu_ctx):
    p = session(fa, gpu_ctx)["plans"]
    assert [q.status for q in p] == [0] * 4 and [q.prompt_frames for q in p] == [406, 406, 1, 16]
    assert p[0].features_length % p[0].avg and p[0].features_length > p[0].tokens * p[0].avg and p[0].bucket == 555 and p[1].gen_frames == 282


@functools.lru_cache(None)
def tables(fa):
    import ctypes as C
    cfg = fa.LuxTtsMelExtractor().config()
    win, bank = np.zeros(NFFT, np.float32), np.zeros((MELS, NFFT // 2 + 1), np.float32)
    assert fa.lib().fa_mel_hann_window(C.byref(cfg), win.ctypes.data) == 0 and fa.lib().fa_mel_filterbank(C.byref(cfg), bank.ctypes.data) == 0
    return win, bank


def mel_of(fa, x, frames, dtype):
    """log-mel rows times the feature scale of the gained prompt x (float32) in dtype: LuxTtsMelExtractor.extract"""
    win, bank = (t.astype(dtype) for t in tables(fa))
    n, i = x.size, np.arange(NFFT // 2)
    q = np.concatenate([x[np.minimum(NFFT // 2 - i, n - 1)], x, x[np.maximum(n - 2 - i, 0)]]).astype(dtype)
    fr = q[np.arange(frames)[:, None] * HOP + np.arange(NFFT)[None]] * win
    if dtype == np.float64:
        mag = np.abs(np.fft.rfft(fr, axis=1))
    else:
        a = 2 * np.pi * np.outer(np.arange(NFFT), np.arange(NFFT // 2 + 1)) / NFFT
        mag = np.sqrt((fr @ np.cos(a).astype(dtype)) ** 2 + (fr @ np.sin(a).astype(dtype)) ** 2)
    return np.log(np.maximum(mag @ bank.T, dtype(FLOOR))) * dtype(SCALE)


def test_prompt_records_and_speech_condition(fa, gpu_ctx):
    r = session(fa, gpu_ctx)
    rec, speech = r["records"], r["speech"]
    for b, w in enumerate(waves()):
        host = fa.luxtts_prompt_loudness(w)
        assert (rec[b]["status"], rec[b]["gain"].tobytes(), rec[b]["rms"].tobytes()) == (host.status, np.float32(host.gain).tobytes(), np.float32(host.rms).tobytes())
        ms = np.mean(w.astype(np.float64) ** 2)
        assert abs(rec[b]["mean_square"] - ms) <= (w.size / 64 + 8) * 2.0 ** -24 * ms
    assert rec["status"].tolist() == [0, 0, 0, 9] and rec["gain"][0] == 1.0 and rec["gain"][1] > 1.0 and rec["rms"][1] < TARGET
    errs = []
    for b in range(3):
        frames, x = r["plans"][b].prompt_frames, waves()[b] * rec[b]["gain"]
        f64 = mel_of(fa, x, frames, np.float64)
        errs.append((np.abs(speech[b, :frames] - f64).max(), np.abs(mel_of(fa, x, frames, np.float32) - f64).max()))
        print(f"luxtts speech condition [{b}]: max|device - float64| {errs[b][0]:.3e}, max|float32 emulation - float64| {errs[b][1]:.3e}")
        assert not speech[b, frames:].any()
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "luxtts_prompt.npz"))["mel_scaled"]
    print(f"luxtts speech condition [0] against the reference's golden mel: {np.abs(speech[0, :406] - gold).max():.3e}")
    assert np.abs(speech[0, :406] - gold).max() <= 1e-4
    assert not speech[3].any()
    assert all(dev <= 4 * emu for dev, emu in errs), errs


def test_inputs_are_exact_and_the_noise_is_the_float64_restatement(fa, gpu_ctx):
    r = session(fa, gpu_ctx)
    for b, p in enumerate(r["plans"]):
        assert r["tokens"][b].tolist() == r["ids"][b].tolist() + [0] * (256 - p.tokens)
        assert np.array_equal(r["token_mask"][b], (np.arange(256) >= p.tokens).astype(np.float32))
        assert np.array_equal(r["frame_mask"][b], (np.arange(1024) >= p.features_length).astype(np.float32))
        index = np.where(np.arange(p.features_length) < p.tokens * p.avg, np.arange(p.features_length) // p.avg, p.tokens)   # Solver :41-49
        assert np.array_equal(r["text"][b, :p.features_length], r["embeds"][b, index, :MELS]) and not r["text"][b, p.features_length:].any()
        n = p.features_length * MELS
        with np.errstate(over="ignore"):                      # StyleTTS2DiffusionSchedule.swift:49-73 as a counter
            state = (np.uint64(SEEDS[b]) if SEEDS[b] else np.uint64(0xdeadbeefcafebabe)) + np.arange(1, 2 * n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            z = (state ^ (state >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        u = ((z ^ (z >> np.uint64(31))) >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
        u = np.where(u <= 0, np.finfo(np.float64).tiny, u)
        want = (np.sqrt(-2.0 * np.log(u[0::2])) * np.cos(2.0 * np.pi * u[1::2])).astype(np.float32)
        got = r["x"][0][b].reshape(-1)
        assert np.all(np.abs(got[:n] - want) <= np.spacing(np.abs(want)))
        assert np.mean(got[:n].view(np.uint32) == want.view(np.uint32)) >= 0.999 and not got[n:].any()


@pytest.mark.parametrize("step", range(4))
def test_step_is_the_host_order_and_within_the_float64_bound(fa, gpu_ctx, step):
    r = session(fa, gpu_ctx)
    t = fa.luxtts_time_steps().astype(np.float32).astype(np.float64)
    for b, p in enumerate(r["plans"]):
        L = p.features_length
        x, v, got = r["x"][step][b, :L], r["v"][step][b, :L, :MELS], r["x"][step + 1][b]
        assert np.array_equal(got[:L].view(np.uint32), fa.luxtts_anchor_euler(x, v, step).view(np.uint32)) and not got[L:].any()
        x64, v64 = x.astype(np.float64), v.astype(np.float64)
        x1p = x64 + (1.0 - t[step]) * v64                        # LuxTtsSolver.anchorEulerUpdate
        want = x1p if step == 3 else (1.0 - t[step + 1]) * (x64 - t[step] * v64) + t[step + 1] * x1p
        assert np.all(np.abs(got[:L] - want) <= 6 * 2.0 ** -24 * (np.abs(x64) + np.abs(v64)))


def test_vocoder_input_and_finish_are_numpy_float32(fa, gpu_ctx):
    r = session(fa, gpu_ctx)
    assert sorted(r["buckets"]) == [282, 555] and r["buckets"][555] == [0] and r["buckets"][282] == [1, 2, 3]
    for bucket, items in r["buckets"].items():
        for k, b in enumerate(items):
            p = r["plans"][b]
            want = np.full((MELS, bucket), np.float32(np.log(np.float64(FLOOR))), np.float32)
            want[:, :p.gen_frames] = (r["x"][4][b, p.prompt_frames:p.features_length] * (np.float32(1.0) / SCALE)).T
            assert np.array_equal(r["mel"][bucket][k].view(np.uint32), want.view(np.uint32)), (bucket, b)
    for b, p in enumerate(r["plans"]):
        rms = r["records"][b]["rms"]
        want = np.clip(r["audio"][b, :p.sample_count], np.float32(-1), np.float32(1))
        want = want * (rms / TARGET) if rms < TARGET else want
        assert np.abs(r["audio"][b, :p.sample_count]).max() > 1 and r["out"][b].dtype == np.float32 and np.array_equal(r["out"][b], want), b
    assert np.abs(r["out"][1]).max() < 0.5 and not r["out"][3].any()      # the boosted item is scaled back; the silent one has rms 0
