"""The StyleTTS2 plan (fluidaudio_amd/csrc/styletts2_core.h through fa_styletts2_plan) against a line-by-line restatement of
StyleTTS2MelExtractor.swift:79-84 and StyleTTS2Synthesizer.swift:41-53, the Karras schedule against the double formula and the known
answers of StyleTTS2DiffusionScheduleTests.swift, and the mel bank against a float32 restatement of StyleTTS2MelExtractor.swift:174-221.
No device."""
import itertools

import numpy as np
import pytest

HOP, MAX_REF_FRAMES = 300, 80
GRID = list(itertools.product([0, 1, 299, 300, 1024, 1025, 24000], [0, 1, 57, 58, 64, 65, 256, 257]))


def restated(n, tokens):
    """(status, samples, ref_frames, tokens, bucket)"""
    if tokens < 1:
        return 1, 0, 0, 0, 0                                        # no tokens
    bucket = 57 if tokens <= 57 else next((b for b in (64, 128, 256) if tokens <= b), None)   # Synthesizer :45-50, ModelStore :200-205
    if bucket is None:
        return 2, 0, 0, 0, 0                                        # textTooLong
    frames = (n + 2048 - 2048) // HOP + 1                           # MelExtractor :79-84 on n + 2 * 1024 padded samples
    if frames > MAX_REF_FRAMES:
        return 3, 0, 0, 0, 0
    return 0, n, frames, tokens, bucket


def test_the_grid_meets_every_status_and_bucket():
    assert {restated(*c)[0] for c in GRID} == {0, 1, 2, 3} and {restated(*c)[4] for c in GRID} == {0, 57, 64, 128, 256}


@pytest.mark.parametrize("case", GRID)
def test_plan_is_the_restatement(fa, case):
    p = fa.styletts2_plan([case[0]], case[1], fa.styletts2_config(max_ref_frames=MAX_REF_FRAMES))[0]
    assert (p.status, p.samples, p.ref_frames, p.tokens, p.bucket) == restated(*case)


@pytest.mark.parametrize("steps", [2, 5, 30])
def test_karras_sigmas(fa, steps):
    got = fa.styletts2_karras_sigmas(steps)
    hi, lo = 3.0 ** (1.0 / 9.0), 0.0001 ** (1.0 / 9.0)
    assert got[:-1].tolist() == [(hi + (i / (steps - 1)) * (lo - hi)) ** 9.0 for i in range(steps)]      # DiffusionSchedule :23-34
    assert got.size == steps + 1 and abs(got[0] - 3.0) <= 1e-9 and abs(got[-2] - 0.0001) <= 1e-9 and np.all(np.diff(got) < 0) and got[-1] == 0.0


def bank(dt):
    """StyleTTS2MelExtractor.swift:174-221 in dtype dt"""
    to_mel = lambda hz: dt(2595.0) * np.log10(dt(1.0) + hz / dt(700.0))  # noqa: E731
    to_hz = lambda mel: dt(700.0) * (np.power(dt(10.0), mel / dt(2595.0)) - dt(1.0))  # noqa: E731
    freqs = np.arange(1025).astype(dt) * (dt(16000) / dt(2048))
    points = to_mel(dt(0.0)) + (to_mel(dt(8000.0)) - to_mel(dt(0.0))) * (np.arange(82).astype(dt) / dt(81))
    hz = to_hz(points.astype(dt)).astype(dt)
    fb = np.zeros((80, 1025), dt)
    for m in range(80):
        left, center, right = hz[m], hz[m + 1], hz[m + 2]
        val = np.where(freqs <= center, (freqs - left) / (center - left), (right - freqs) / (right - center))
        fb[m] = np.where((freqs < left) | (freqs > right), 0, np.maximum(val, 0))
    return fb


def test_bank_is_the_float32_restatement(fa):
    """Tolerance: 4 x the largest difference between the restatement run in float32 and in float64, measured 9.25e-6 (so 3.7e-5; the
    library's table is 5.1e-6 from the float32 restatement: powf and log10f differ from numpy's in the last place).  Every row is one
    contiguous range of bins and the rows cover all 1025 bins but the two ends, where the triangles are zero."""
    got, f32, f64 = fa.styletts2_filterbank(), bank(np.float32), bank(np.float64)
    tol = 4 * np.abs(f32 - f64).max()
    print(f"styletts2 bank: max|library - float32 restatement| {np.abs(got - f32).max():.3e}, tolerance {tol:.3e}")
    assert got.dtype == np.float32 and np.abs(got - f32).max() <= tol
    assert (got > 0).any(axis=0)[1:-1].all()
    for row in got:
        nz = np.flatnonzero(row)
        assert nz.size and np.all(np.diff(nz) == 1)
    win = fa.styletts2_window()
    assert win.size == 1200 and win[0] == 0 and np.abs(win - 0.5 * (1 - np.cos(2 * np.pi * np.arange(1200) / 1200))).max() <= 2.0 ** -21      # one float32 spacing of the cosine's argument below 2 pi
