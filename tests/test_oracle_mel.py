"""Pins the mel oracle (oracle/fa_oracle.c) against what the reference's tests hold.

Ported from Tests/FluidAudioTests/ASR/Parakeet/Streaming/AudioMelSpectrogramTests.swift:22-122,
Diarizer/Sortformer/SortformerStreamingMelTests.swift:84-132, ASR/Parakeet/Streaming/
EouChunkSizeFrameCountTests.swift:10-60 and the one true golden vector of the repo,
TTS/LuxTts/LuxTtsMelExtractorTests.swift:18-41.
"""
import os

import numpy as np
import pytest
from conftest import synth_audio


def test_frame_counts(oracle_mod):
    cfg = oracle_mod.MelConfig()
    # 15 s / 10 s / 1 s -> 1501 / 1001 / 101 ; formula 1 + (n + nFFT - win) / hop
    for n, t in ((240000, 1501), (160000, 1001), (16000, 101), (1, 1), (0, 0)):
        assert oracle_mod.mel_frames(cfg, n) == t
    for n in (159, 160, 2560, 5120, 20480, 12345):
        assert oracle_mod.mel_frames(cfg, n) == 1 + (n + 512 - 400) // 160
    # EouChunkSizeFrameCountTests: 160 ms / 320 ms / 1280 ms chunks
    for ms in (160, 320, 1280):
        n = ms * 16
        assert oracle_mod.mel_frames(cfg, n) == 1 + (n + 112) // 160
    # prePadded: max(0, (n - nFFT)/hop + 1) with truncating division
    assert oracle_mod.mel_frames(cfg, 512, prepadded=True) == 1
    assert oracle_mod.mel_frames(cfg, 511, prepadded=True) == 1  # (-1)/160 truncates to 0
    assert oracle_mod.mel_frames(cfg, 352, prepadded=True) == 0
    assert oracle_mod.mel_frames(cfg, 1312, prepadded=True) == 6


def test_legacy_compute_frame_count(oracle_mod):
    # AudioMelSpectrogramTests.swift:32-45: 1 s -> 98 frames via compute()
    mel, T = oracle_mod.mel_legacy(synth_audio(16000))
    assert T == 98 and mel.shape == (128, 98)


def test_flat_size_and_guard(oracle_mod):
    mel, ml, nf = oracle_mod.mel_flat(synth_audio(16000))
    assert mel.size == 128 * nf and ml == 101 and nf == 101
    mel, ml, nf = oracle_mod.mel_flat(np.zeros(0, np.float32))
    assert ml == 0 and nf == 1 and mel.size == 128 and not mel.any()
    cfg = oracle_mod.MelConfig(pad_to=16)
    mel, ml, nf = oracle_mod.mel_flat(synth_audio(16000), cfg)
    assert ml == 101 and nf == 112 and not mel[:, 101:].any()


def test_hann_window_properties(oracle_mod):
    w = oracle_mod.hann(400)
    assert w[0] == 0.0 and abs(w[-1]) < 1e-6
    np.testing.assert_allclose(w, w[::-1], atol=1e-6)
    assert abs(w.max() - 1.0) < 1e-4
    wp = oracle_mod.hann(400, periodic=True)
    assert wp[0] == 0.0 and wp[-1] > 1e-5  # periodic window does not return to zero


def test_filterbank_properties(oracle_mod):
    fb = oracle_mod.slaney_filterbank()
    assert fb.shape == (128, 257) and (fb >= 0).all()
    assert (np.count_nonzero(fb, axis=0) <= 2).all()  # every bin feeds at most two triangles
    for row in fb:  # support of each triangle is one contiguous run (the kernel's sparse form relies on it)
        nz = np.flatnonzero(row)
        assert nz.size == 0 or nz[-1] - nz[0] + 1 == nz.size


def test_silence_gives_log_floor(oracle_mod):
    mel, ml, _ = oracle_mod.mel_flat(np.zeros(16000, np.float32))
    assert (mel[:, :ml] < 0).all()
    np.testing.assert_allclose(mel[:, :ml], np.log(np.float32(2.0 ** -24)), rtol=1e-6)


def test_stream_prepadded_equals_batch_center(oracle_mod):
    # SortformerStreamingMelTests.swift:100-132: .prePadded frames over a zero-padded copy == .center frames (1e-5)
    a = synth_audio(16000 * 2, 5)
    batch, T, _ = oracle_mod.mel_flat_transposed(a)
    # the padded stream carries the pre-emphasis state across the seam, so emulate with preemph applied once
    cfg0 = oracle_mod.MelConfig(preemph=0.0)
    y = np.empty_like(a)
    y[0] = a[0]
    y[1:] = a[1:] - np.float32(0.97) * a[:-1]
    padded = np.concatenate([np.zeros(256, np.float32), y, np.zeros(256, np.float32)])
    stream, Ts, _ = oracle_mod.mel_flat_transposed(padded, cfg0, prepadded=True)
    assert Ts == (padded.size - 512) // 160 + 1
    k = min(T, Ts)
    np.testing.assert_allclose(stream[:k], batch[:k], atol=1e-5)


def test_layouts_agree(oracle_mod):
    a = synth_audio(8000, 9)
    f, lf, nf = oracle_mod.mel_flat(a, last=0.1)
    t, lt, nt = oracle_mod.mel_flat_transposed(a, last=0.1)
    assert (lf, nf) == (lt, nt)
    np.testing.assert_array_equal(f[:, :lf], t[:lt].T)


def test_fft_restatement_against_float64(oracle_mod):
    rng = np.random.default_rng(3)
    for n in (512, 1024):
        x = rng.standard_normal(n).astype(np.float32)
        re, im = x.copy(), np.zeros(n, np.float32)
        oracle_mod.lib().fa_oracle_fft_f32(n, re, im)
        ref = np.fft.fft(x.astype(np.float64))
        assert np.abs(re + 1j * im - ref).max() < 2e-5 * np.abs(ref).max()


def test_luxtts_golden_fixture(oracle_mod):
    """The only golden mel in the reference: 103 936 samples -> 406 x 100 log-mel, gate max-abs < 1e-3
    (tests/golden/luxtts_prompt.npz holds the reference's prompt_24k_f32le.bin / prompt_mel_f32le.bin as they are)."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "luxtts_prompt.npz"))
    audio, gold = g["audio"], g["mel_scaled"]
    assert audio.size == 103936 and gold.shape == (406, 100)
    n_fft, hop, n_mels, sr = 1024, 256, 100, 24000
    win = (0.5 * (1 - np.cos(2 * np.float32(np.pi) * np.arange(n_fft, dtype=np.float32) / np.float32(n_fft)))).astype(np.float32)
    bins, fmax = n_fft // 2 + 1, sr / 2
    h2m = lambda hz: 2595 * np.log10(1 + hz / 700)  # noqa: E731  (LuxTtsMelExtractor.swift:159-160)
    m2h = lambda m: 700 * (10 ** (m / 2595) - 1)  # noqa: E731
    pts = m2h(h2m(0) + np.arange(n_mels + 2) * (h2m(fmax) - h2m(0)) / (n_mels + 1))
    fr = np.arange(bins) * fmax / (bins - 1)
    fb = np.stack([np.maximum(0, np.minimum((fr - pts[m]) / (pts[m + 1] - pts[m]), (pts[m + 2] - fr) / (pts[m + 2] - pts[m + 1])))
                   for m in range(n_mels)]).astype(np.float32)
    frames = (audio.size + hop // 2) // hop
    assert frames == 406
    out = oracle_mod.logmel_generic(audio, n_fft, hop, win, fb, 1, 1e-7, frames)
    assert np.abs(out * np.float32(0.1) - gold).max() < 1e-3


def test_committed_golden_matches_oracle(oracle_mod):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "mel_golden.npz"))
    m1, l1, _ = oracle_mod.mel_flat(g["a1"])
    np.testing.assert_array_equal(m1, g["flat1"])
    m2, l2, _ = oracle_mod.mel_flat_transposed(g["a2"], last=0.25)
    np.testing.assert_array_equal(m2, g["tr2"])


@pytest.mark.parametrize("n", [1, 400, 513, 16000, 24001, 160000])
def test_fp32_restatement_within_1e4_of_float64(oracle_mod, n):
    """The fp32 restatement against the float64 evaluation of the same formula on the same fp32 tables
    (oracle.mel_f64): pure relative error <= 1e-4 wherever |log-mel| >= 1e-2 -- the gate the device has to pass too
    (tests/test_gpu_mel.py::close64), so 'both fp32 paths agree' is not all that is shown."""
    from conftest import synth_audio
    a = synth_audio(n, seed=n)
    ref, ml, nf = oracle_mod.mel_flat(a, last=0.3)
    f = oracle_mod.mel_f64(a, last=0.3)
    assert f.shape == (ml, 128)
    assert oracle_mod.mel_f64_error(ref[:, :ml].T, f) <= 1e-4
    tr, ml2, _ = oracle_mod.mel_flat_transposed(a, prepadded=True)
    f2 = oracle_mod.mel_f64(a, padding="prepadded")
    assert f2.shape[0] == ml2
    if ml2:
        assert oracle_mod.mel_f64_error(tr[:ml2], f2) <= 1e-4


def test_float64_evaluation_other_configs(oracle_mod):
    from conftest import synth_audio
    a = synth_audio(20000, 8)
    cfg = oracle_mod.MelConfig(preemph=0.0, log_floor=1e-10, floor_clamped=True, window_periodic=True)
    ref, ml, _ = oracle_mod.mel_flat_transposed(a, cfg)
    assert oracle_mod.mel_f64_error(ref[:ml], oracle_mod.mel_f64(a, cfg=cfg)) <= 1e-4
    leg, T = oracle_mod.mel_legacy(a[:16000])
    assert oracle_mod.mel_f64_error(leg.T, oracle_mod.mel_f64(a[:16000], padding="legacy")) <= 1e-4
    ex, ml, nf = oracle_mod.mel_flat_transposed(a, expected_frames=140)
    assert oracle_mod.mel_f64_error(ex[:140], oracle_mod.mel_f64(a, expected_frames=140)) <= 1e-4
    # per-feature normalisation: fp32 restatement vs float64, within the north-star tolerance propagated through (x - mean) / std
    w = np.zeros(32000, np.float32)
    w[:12345] = synth_audio(12345, 41)
    z32, v = oracle_mod.unified_mel_features(w, 12345)
    z64, v64 = oracle_mod.unified_mel_features_f64(w, 12345)
    assert v == v64 == 77
    x64 = oracle_mod.mel_f64(w, expected_frames=201).T[:, :v]
    tol = 1e-4 * (np.abs(x64) + np.abs(x64.mean(1, keepdims=True))) / (x64.std(1, ddof=1, keepdims=True) + 1e-5) + 1e-4 * np.abs(z64[:, :v])
    assert np.all(np.abs(z32[:, :v] - z64[:, :v]) <= tol)
    assert not z64[:, v:].any() and not z32[:, v:].any()


# ---- an independent second opinion for the NeMo-flavoured configuration (the one the tuned kernel and the bench run) ----------
SECOND_OPINION_LENGTHS = [16000, 160000, 240000, 1600 + 47, 24001 - 1, 12345, 160 * 50 + 48, 160 * 50 + 159, 513, 400]


def test_tables_against_independent_librosa_formulas(oracle_mod):
    """Hann window and Slaney bank of the restatement (fp32, AudioMelSpectrogram.swift:553-642) against float64 tables built from
    the published torch / librosa formulas (tests/mel_second_opinion.py): equal to fp32 rounding of the Swift arithmetic."""
    import torch
    from mel_second_opinion import slaney_bank_f64
    w64 = torch.hann_window(400, periodic=False, dtype=torch.float64).numpy()
    assert np.abs(oracle_mod.hann(400).astype(np.float64) - w64).max() < 5e-7   # fp32 cos of an fp32 argument up to 2 pi (:553-562)
    fb64 = slaney_bank_f64()
    fb32 = oracle_mod.slaney_filterbank().astype(np.float64)
    assert fb32.shape == fb64.shape == (128, 257)
    assert np.abs(fb32 - fb64).max() < 1e-5 * fb64.max()   # fp32 ramps: ulp(8 kHz) = 4.9e-4 Hz over triangles ~100 Hz wide
    # same support except where a weight is below fp32 resolution of the ramp arithmetic
    assert ((fb32 > 0) != (fb64 > 0)).sum() <= 4 and np.abs(fb32 - fb64)[(fb32 > 0) != (fb64 > 0)].max(initial=0.0) < 1e-7   # [127][256]: the Nyquist bin sits ON the last triangle's right edge, 5e-8 in fp32


@pytest.mark.parametrize("n", SECOND_OPINION_LENGTHS)
def test_mel_f64_against_torch_stft_second_opinion(oracle_mod, n):
    """oracle.mel_f64 (written from the Swift file) against the torch.stft pipeline (written from NeMo's / librosa's published
    definitions): with the reference's fp32 tables plugged into both, framing, zero padding, pre-emphasis, DFT, power, bank product
    and log must agree to 1e-9 — including lengths where the reference emits one more (truncated) frame than torch; with the
    independent float64 tables the difference is the fp32 rounding of the reference's tables only."""
    from mel_second_opinion import nemo_logmel_f64
    a = synth_audio(n, seed=1000 + n)
    ref = oracle_mod.mel_f64(a)
    T = oracle_mod.mel_frames(oracle_mod.MelConfig(), n)
    assert ref.shape == (T, 128) and T == 1 + (n + 112) // 160
    same_tables = nemo_logmel_f64(a, T, window=oracle_mod.hann(400), bank=oracle_mod.slaney_filterbank())
    assert np.abs(same_tables - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    flat, ml, _ = oracle_mod.mel_flat(a)
    assert ml == T
    assert oracle_mod.mel_f64_error(flat[:, :ml].T, same_tables) <= 1e-4     # the fp32 restatement against the INDEPENDENT evaluation: north-star gate
    # With the independent float64 TABLES the difference is the fp32 rounding of the reference's tables (:553-642): 2.5e-7 on the Hann
    # window (fp32 cos of an fp32 argument) leaks ~1e-7 of the pre-emphasised high band into every bin — up to 1e-4 in the log domain
    # in the weakest low mel bands — and 2e-7 on bank weights of 1e-5 .. 4e-2.  A property of the reference's TABLES (part of its
    # definition), bounded here on a line-free signal; median difference ~2e-6.
    b = (np.random.default_rng(n).standard_normal(n) * 0.1).astype(np.float32)
    diff = np.abs(nemo_logmel_f64(b, T) - oracle_mod.mel_f64(b))
    assert diff.max() <= 5e-4 and np.median(diff) <= 1e-5
