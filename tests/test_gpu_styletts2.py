"""The StyleTTS2 session on the device (fluidaudio_amd/csrc/styletts2.hip) against float64 / numpy restatements of the arithmetic
include/fluidaudio_hip.h states, on one batch of four items through one session: the fixture's first second (81 frames: a partial last
tile; 1 token), the same scaled by 0.2 (57 tokens, the hand-made duration rows), 700 samples of noise (3 frames, both reflect clamps; 58
tokens of duration 50: two tokens under a tile) and 4 096 zeros (256 tokens of duration 1: 64 tokens under a tile).

Mel: max|device - float64| <= 4 max|float32 emulation - float64| per item, the emulation being the reference's method in float32
(windowed frames, torch.fft.rfft on float32, power, a float32 bank product, log) with the library's own window and bank.  Measured on an
MI355X: fixture device 4.761e-05, emulation 6.987e-05; scaled 1.186e-05 against 2.361e-05; 700 samples 2.288e-07 against 2.006e-07.  A
float32 matrix-DFT emulation (printed, not asserted) is at 1.166e-05 / 6.768e-06 / 3.391e-07: 4 x that holds for the second and third
item and misses on the first by 2 % (4.761e-05 against 4.664e-05).  The silent item is the floor value in every cell."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NFFT, WIN, HOP, LEAD, MELS, REF_STRIDE, C = 2048, 1200, 300, 424, 80, 96, 50
TOKENS, BUCKETS = [1, 57, 58, 256], [57, 57, 64, 256]
SEEDS = np.array([42, 0, 2 ** 63 + 12345, 7], np.uint64)
BLENDS = [(0.3, 0.7), (1.0, 1.0), (0.0, 0.0), (0.5, 0.25)]
LENGTHS = [49, 50, 51, 30000]
LOGIT_SEED = 5                                # chosen on the CPU: no float64 sum of these logits lies within 1e-4 of a half-integer


@functools.lru_cache(None)
def waves():
    audio = np.load(os.path.join(os.path.dirname(__file__), "golden", "luxtts_prompt.npz"))["audio"][:24000]
    return [audio, (audio * np.float32(0.2)).astype(np.float32), (np.random.default_rng(3).standard_normal(700) * 0.3).astype(np.float32), np.zeros(4096, np.float32)]


@functools.lru_cache(None)
def logits():
    x = (np.random.default_rng(LOGIT_SEED).standard_normal((4, 256, C)) * 2).astype(np.float32)
    x[1, 0], x[1, 1:3], x[1, 3], x[1, 4] = -100, -100, -100, 100          # the clamp; (below) the reference's [2, 2]; the tie 2.5 -> 3; 50
    x[1, 1:3, :4], x[1, 3, :5] = 0, 0
    x[2], x[3] = 100, -100
    return x


def padded(rng, shape, keep):
    a = np.full(shape, np.nan, np.float32)
    a[..., :keep] = rng.standard_normal(shape[:-1] + (keep,)).astype(np.float32)
    return a


@functools.lru_cache(None)
def session(fa, ctx):
    """the whole flow once, every slab fetched after the call that writes it: shared by the tests, left unchanged"""
    rng, r = np.random.default_rng(11), {}
    s = fa.StyleTts2Session(4, fa.styletts2_config(max_ref_frames=REF_STRIDE), ctx)
    r["plans"] = plans = s.reference_mel(waves(), TOKENS)
    r["mel"] = s.get("mel")
    r["ids"] = [rng.integers(1, 178, n).astype(np.int32) for n in TOKENS]
    s.inputs(r["ids"], SEEDS)
    r.update({k: s.get(k) for k in ("tokens", "attention_mask", "noise_init", "noises_aux")})
    r["s_pred"], r["ref_s"] = padded(rng, (4, 260), 256), padded(rng, (4, 260), 256)
    s.blend(r["s_pred"], r["ref_s"], [a for a, _ in BLENDS], [b for _, b in BLENDS])
    r["ref"], r["s"] = s.get("ref"), s.get("s")
    known = np.repeat(np.array([[1.0, 7.0], [3.0, 9.0]], np.float32), 128, axis=1)      # StyleTTS2GlueOpsTests.testBlendStyleSplitsAtIndex128...
    s.blend(np.tile(known[0], (4, 1)), np.tile(known[1], (4, 1)), 0.25, 0.75)
    r["known"] = s.get("ref"), s.get("s")
    r["totals"], r["status"] = s.durations(logits())
    r["durations"], r["starts"] = s.get("durations"), s.get("starts")
    r["d"], r["t_en"] = padded(rng, (4, 256, 648), 640), padded(rng, (4, 512, 260), 256)
    r["aligned"] = {shift: s.align(r["d"], r["t_en"], shift) for shift in (True, False)}
    r["audio"] = rng.standard_normal((4, max(LENGTHS) + 24)).astype(np.float32)
    r["out"] = s.finish(r["audio"], LENGTHS)
    s.close()
    return r


def mel_of(fa, x, dtype):
    """StyleTTS2MelExtractor.compute in dtype (float32: the reference's method, with a float32 FFT), the library's window and bank"""
    import torch
    win, bank = np.zeros(NFFT, dtype), fa.styletts2_filterbank().astype(dtype)
    win[LEAD:LEAD + WIN] = fa.styletts2_window()
    n, i = x.size, np.arange(NFFT // 2)
    q = np.concatenate([x[np.minimum(NFFT // 2 - i, n - 1)], x, x[np.maximum(n - 2 - i, 0)]]).astype(dtype)
    fr = q[np.arange(n // HOP + 1)[:, None] * HOP + np.arange(NFFT)[None]] * win
    spec = torch.fft.rfft(torch.from_numpy(fr), dim=1)
    assert spec.dtype == (torch.complex64 if dtype == np.float32 else torch.complex128)
    power = (spec.real ** 2 + spec.imag ** 2).numpy()
    return ((np.log(power @ bank.T + dtype(1e-5)) + dtype(4)) / dtype(4)).T, fr


def test_plan_and_buckets(fa, gpu_ctx):
    p = session(fa, gpu_ctx)["plans"]
    assert [q.status for q in p] == [0] * 4 and [q.ref_frames for q in p] == [81, 81, 3, 14] and [q.bucket for q in p] == BUCKETS


def test_reference_mel(fa, gpu_ctx):
    mel, errs = session(fa, gpu_ctx)["mel"], []
    for b in range(3):
        f64, fr = mel_of(fa, waves()[b], np.float64)
        f32, _ = mel_of(fa, waves()[b], np.float32)
        frames = f64.shape[1]
        a = 2 * np.pi * np.outer(np.arange(NFFT), np.arange(NFFT // 2 + 1)) / NFFT
        fr32, bank = fr.astype(np.float32), fa.styletts2_filterbank()
        dft = ((np.log(((fr32 @ np.cos(a).astype(np.float32)) ** 2 + (fr32 @ np.sin(a).astype(np.float32)) ** 2) @ bank.T + np.float32(1e-5)) + np.float32(4)) / np.float32(4)).T
        errs.append((np.abs(mel[b, :, :frames] - f64).max(), np.abs(f32 - f64).max(), np.abs(dft - f64).max()))
        print(f"styletts2 mel [{b}]: max|device - float64| {errs[b][0]:.3e}, float32 FFT emulation {errs[b][1]:.3e}, float32 matrix-DFT emulation {errs[b][2]:.3e}")
        assert not mel[b, :, frames:].any()
    floor = (np.log(np.float32(1e-5)) + np.float32(4)) / np.float32(4)
    assert np.all(mel[3, :, :14] == floor) and not mel[3, :, 14:].any()
    assert all(dev <= 4 * emu for dev, emu, _ in errs), errs


def test_inputs_are_exact_and_the_noise_is_the_float64_restatement(fa, gpu_ctx):
    r = session(fa, gpu_ctx)
    for b, n in enumerate(TOKENS):
        assert r["tokens"][b].tolist() == r["ids"][b].tolist() + [0] * (256 - n)
        assert r["attention_mask"][b].tolist() == [1] * n + [0] * (256 - n)
        with np.errstate(over="ignore"):                      # StyleTTS2DiffusionSchedule.swift:49-73 as a counter
            state = (np.uint64(SEEDS[b]) if SEEDS[b] else np.uint64(0xdeadbeefcafebabe)) + np.arange(1, 2 * 1280 + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            z = (state ^ (state >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        u = ((z ^ (z >> np.uint64(31))) >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
        u = np.where(u <= 0, np.finfo(np.float64).tiny, u)
        want = (np.sqrt(-2.0 * np.log(u[0::2])) * np.cos(2.0 * np.pi * u[1::2])).astype(np.float32)
        got = np.concatenate([r["noise_init"][b], r["noises_aux"][:, b].reshape(-1)])     # consecutive parts of one stream
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))) and np.mean(got.view(np.uint32) == want.view(np.uint32)) >= 0.999


def test_blend_is_numpy_float32_in_the_stated_order(fa, gpu_ctx):
    r = session(fa, gpu_ctx)
    for b, (alpha, beta) in enumerate(BLENDS):
        for got, w, lo in ((r["ref"][b], np.float32(alpha), 0), (r["s"][b], np.float32(beta), 128)):
            x, y = r["s_pred"][b, lo:lo + 128], r["ref_s"][b, lo:lo + 128]
            assert np.array_equal(got.view(np.uint32), (w * x + (np.float32(1) - w) * y).view(np.uint32)), (b, lo)
    assert np.array_equal(r["ref"][1], r["s_pred"][1, :128]) and np.array_equal(r["s"][1], r["s_pred"][1, 128:256])
    assert np.all(r["known"][0] == 2.5) and np.all(r["known"][1] == 7.5)


def test_durations_are_the_float64_restatement(fa, gpu_ctx):
    r = session(fa, gpu_ctx)
    sums = (1.0 / (1.0 + np.exp(-logits().astype(np.float64)))).sum(axis=2)
    exempt = np.abs(sums - np.floor(sums) - 0.5) <= 1e-4                   # ten times a 50-term float32 sum's error bound at 50
    exempt[1, 3] = False                                                   # the exact tie
    want = np.maximum(np.floor(sums + 0.5), 1).astype(np.int64)
    want[1, 3] = 3
    for b, n in enumerate(TOKENS):
        got = r["durations"][b, :n]
        assert exempt[b, :n].sum() <= n // 100 and np.all(np.abs(got - want[b, :n]) <= exempt[b, :n])
        assert r["starts"][b, :n].tolist() == (np.cumsum(got) - got).tolist() and r["totals"][b] == got.sum() and not r["durations"][b, n:].any()
    assert r["durations"][1, :5].tolist() == [1, 2, 2, 3, 50] and np.all(r["durations"][2, :58] == 50) and np.all(r["durations"][3] == 1)
    assert r["status"].tolist() == [0] * 4 and not exempt[0, :1].any() and not exempt[1, :57].any()


@pytest.mark.parametrize("shift", [True, False])
def test_alignment_is_repeat_and_shift(fa, gpu_ctx, shift):
    r = session(fa, gpu_ctx)
    en, asr = r["aligned"][shift]
    assert en.shape[2] == asr.shape[2] == 2900
    for b, n in enumerate(TOKENS):
        tok = np.repeat(np.arange(n), r["durations"][b, :n])
        tok = np.concatenate([tok[:1], tok[:-1]]) if shift else tok        # GlueOps.hifiganShift
        assert np.array_equal(en[b, :, :tok.size].view(np.uint32), r["d"][b, tok, :640].T.view(np.uint32)), b
        assert np.array_equal(asr[b, :, :tok.size].view(np.uint32), r["t_en"][b, :, tok].T.view(np.uint32)), b
        assert not en[b, :, tok.size:].any() and not asr[b, :, tok.size:].any()


@pytest.mark.parametrize("durations,features,shift,want", [
    ([2, 1, 3], [[1, 2, 3], [4, 5, 6]], False, [[1, 1, 2, 3, 3, 3], [4, 4, 5, 6, 6, 6]]),            # testMatmulAlignedExpandsFeaturesByDuration
    ([1, 1, 1, 1], [[10, 20, 30, 40], [50, 60, 70, 80]], True, [[10, 10, 20, 30], [50, 50, 60, 70]]),   # testHifiganShiftRightByOneAndCopiesColumnZero
    ([1], [[1], [2]], True, [[1], [2]]),                                                              # testHifiganShiftSingleFrameIsIdentity
])
def test_known_answers_of_the_glue_tests(fa, gpu_ctx, durations, features, shift, want):
    n, feats = len(durations), np.array(features, np.float32)
    s = fa.StyleTts2Session(1, fa.styletts2_config(d_channels=4, asr_channels=4, max_ref_frames=16), gpu_ctx)
    s.reference_mel([np.zeros(1, np.float32)], n)
    totals, _ = s.durations(np.where(np.arange(3)[None, None] < np.array(durations)[None, :, None], 100, -100).astype(np.float32))
    d, t_en = np.zeros((1, n, 4), np.float32), np.zeros((1, 4, n), np.float32)
    d[0, :, :2], t_en[0, :2] = feats.T, feats
    en, asr = s.align(d, t_en, shift, frame_stride=sum(durations))
    s.close()
    assert totals.tolist() == [sum(durations)] and en[0, :2].tolist() == want and asr[0, :2].tolist() == want and not en[0, 2:].any()


def test_finish_trims_and_packs(fa, gpu_ctx):
    r = session(fa, gpu_ctx)
    assert [o.size for o in r["out"]] == [0, 0, 1, 29950]
    for b, n in enumerate(LENGTHS):
        assert r["out"][b].dtype == np.float32 and np.array_equal(r["out"][b], r["audio"][b, :n - min(50, n)]), b
    base = r["out"][3].base                                               # the chunks lie back to back in their order
    assert np.array_equal(base[:29951], np.concatenate([r["audio"][2, :1], r["audio"][3, :29950]]))
