"""The restatement of the embedding inputs (tests/embedding_restatement.py) on hand-built inputs with literal expected outputs, and the
reference's WeightInterpolationTests (Tests/FluidAudioTests/Diarizer/Offline/WeightInterpolationTests.swift).  No GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import embedding_restatement as E  # noqa: E402

f32 = np.float32


# ---- WeightInterpolationTests

def test_resample_identity_when_lengths_match():
    x = np.array([1, 2, 3, 4], f32)
    assert np.array_equal(E.resample(x, 4), x)


def test_resample_up_and_down():
    up = E.resample(np.array([0, 1], f32), 4)
    assert up.size == 4 and up[0] < up[3] and (up >= 0).all() and (up <= 1).all()
    down = E.resample(np.array([0, 0.5, 1, 0.5], f32), 2)
    assert down.size == 2 and (down >= 0).all() and (down <= 1).all()


def test_resample_half_pixel_offset_mapping():
    assert E.resample(np.array([0, 10, 20, 30], f32), 2).tolist() == [5.0, 25.0]


def test_resample_matches_coefficients():
    x = np.arange(16, dtype=f32) * f32(0.25)
    l, r, wl, wr = E.coefficients(16, 7)
    assert np.array_equal(E.resample(x, 7), x[l] * wl + x[r] * wr)


def test_resample_empty_and_zero_length():
    assert E.resample(np.zeros(0, f32), 5).size == 0
    assert E.resample(np.array([1, 2, 3], f32), 0).size == 0
    assert E.resample(np.zeros((0, 4), f32), 5).shape == (0, 5)


def test_resample_2d_consistency():
    x = np.array([[1, 2, 3], [4, 5, 6]], f32)
    two = E.resample(x, 5)
    assert np.array_equal(two[0], E.resample(x[0], 5)) and np.array_equal(two[1], E.resample(x[1], 5))
    b = E.resample(np.array([[1, 3, 5, 7], [2, 4, 6, 8]], f32), 2)
    assert b.tolist() == [[2.0, 6.0], [3.0, 7.0]]


# ---- hand-built chunks

def small_cfg(**kw):
    kw.setdefault("sample_rate", 100)
    kw.setdefault("weight_frames", 10)
    return E.Config(**kw)


def test_overlap_frames_are_excluded():
    w = np.zeros((1, 10, 3), f32)
    w[0, :, 0] = 1
    w[0, :3, 1] = 1                        # frames 0-2 overlap: speaker 0's clean mask is frames 3-9, speaker 1's is empty
    p = E.plan(w, None, 1000, small_cfg())
    assert p["records"] == [(0, 0, 3, 9, 3.0, 10.0)]
    assert (p["evaluated"], p["empty"], p["fallback"]) == (3, 2, 0)
    assert p["mask_rows"].tolist() == [[0, 0, 0, 1, 1, 1, 1, 1, 1, 1]]
    q = E.plan(w, None, 1000, small_cfg(exclude_overlap=False))
    assert q["records"] == [(0, 0, 0, 9, 0.0, 10.0), (0, 1, 0, 2, 0.0, 3.0)]


def test_twenty_percent_rule():
    w = np.zeros((2, 10, 3), f32)
    w[0, 4:6, 0] = 1                       # 2 frames = 0.2 * 10: kept
    w[1, 4, 0] = 1                         # 1 frame: empty, although it is at least minFrames = 1
    p = E.plan(w, None, 10000, small_cfg())
    assert p["records"] == [(0, 0, 4, 5, 4.0, 6.0)]
    assert p["empty"] == 5


def test_fallback_to_the_base_mask():
    # 589 frames per 10 s and min_segment_duration 3 s: minFrames = 177; the clean mask keeps 150 frames (>= 117.8, < 177)
    w = np.zeros((1, 589, 3), f32)
    w[0, :200, 0] = 1
    w[0, :50, 1] = 1
    p = E.plan(w, None, 160000, E.Config(min_segment_duration=3.0))
    fd = 10.0 / 589
    assert p["records"] == [(0, 0, 0, 199, 0.0, 200 * fd)]
    assert (p["fallback"], p["empty"]) == (1, 2)
    assert p["mask_rows"][0].sum() == 200
    # at the default 1 s, minFrames = 59 and the clean mask is used
    q = E.plan(w, None, 160000, E.Config())
    assert q["records"] == [(0, 0, 50, 199, 50 * fd, 200 * fd)] and q["fallback"] == 0


def test_energy_zero_job_under_downsampling():
    # one output frame samples input frame 294 only: a mask over frames 0-199 resamples to 0 and is dropped
    w = np.zeros((1, 589, 3), f32)
    w[0, :200, 0] = 1
    w[0, 250:401, 1] = 1
    p = E.plan(w, None, 160000, E.Config(weight_frames=1))
    assert [r[:2] for r in p["records"]] == [(0, 1)]
    assert p["run_rows"].tolist() == [[1.0]]
    assert p["empty"] == 2


def test_soft_weight_energy_zero():
    w = np.zeros((1, 10, 3), f32)
    w[0, 0, 0] = 5                         # sum 5 passes the sums, but frames 2, 3, 7, 8 are what 2 output frames sample
    p = E.plan(w, None, 1000, small_cfg(weight_frames=2))
    assert p["records"] == [] and p["empty"] == 3


def test_skip_hits_and_misses_across_a_batch_boundary():
    w = np.zeros((3, 10, 3), f32)
    w[:, :5, 0] = 1                        # speaker 0: the same mask in every chunk
    w[0, 5:, 1] = 1                        # speaker 1: disjoint masks in chunks 0 and 1 (cosine 0: a miss)
    w[1, 6:8, 1] = 1
    w[1, 9, 1] = 1
    offs = [0.0, 1.0, 2.0]
    p = E.plan(w, offs, 10000, small_cfg(batch_size=2, skip_threshold=0.95, exclude_overlap=False))
    assert [r[:2] for r in p["records"]] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    assert p["run_of_job"].tolist() == [0, 1, 0, 2, 3]      # chunk 2 opens a new batch: its cache is empty
    assert p["window_of_run"].tolist() == [0, 0, 1, 2]
    assert p["skipped"] == 1
    off = E.plan(w, offs, 10000, small_cfg(batch_size=2, exclude_overlap=False))
    assert off["run_of_job"].tolist() == [0, 1, 2, 3, 4]


def test_chunk_plan_rounding_and_cut_off():
    cfg = E.Config(sample_rate=16000)
    # 0.00003125 s * 16000 = 0.5 -> 1 (half away from zero); a NaN offset falls back to index * window; past the audio: not planned
    p = E.chunk_plan(4, [0.00003125, float("nan"), 5.0], 160000 * 2, cfg)
    assert p == [(0, 0.00003125, 1), (1, 10.0, 160000), (2, 5.0, 80000)]
    assert E.round_half_away(-2.5) == -3.0 and E.round_half_away(2.4999999999999996) == 2.0


def test_span_inputs():
    a = np.arange(1, 2001, dtype=f32)
    cfg = E.Config(sample_rate=100, weight_frames=10)          # 1000 samples per window
    win, wts, ok = E.span_inputs(a, [(1.0, 3.0), (5.0, 5.0), (19.0, 40.0)], cfg)
    assert ok.tolist() == [True, False, True]
    assert np.array_equal(win[0, :200], a[100:300]) and not win[0, 200:].any()
    assert wts[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert not win[1].any() and not wts[1].any()
    assert np.array_equal(win[2, :100], a[1900:]) and wts[2].tolist() == [1] + [0] * 9


def test_library_defaults_and_argument_contract(fa):
    """fa_embedding_default_config carries the reference's defaults; a missing context is refused before any device work."""
    import ctypes as C
    c = fa._lib.EmbeddingConfig()
    fa.lib().fa_embedding_default_config(C.byref(c))
    assert (c.window_duration, c.sample_rate, c.samples_per_window, c.exclude_overlap, c.min_segment_duration, c.batch_size, c.skip_enabled,
            c.weight_frames, c.frame_duration) == (10.0, 16000, 0, 1, 1.0, 32, 0, 589, 0.0)
    assert c.overlap_threshold == f32(1e-3) and c.skip_threshold == f32(0.95)
    assert fa.lib().fa_embedding_plan(None, C.byref(c), None, 0, 0, 0, None, 0, 0, None, None, None, None, None, None, None, None) == fa.INVALID_ARGUMENT
    assert fa.lib().fa_weight_resample(None, None, 1, 4, 2, None) == fa.INVALID_ARGUMENT
    cfg = fa.EmbeddingConfig()
    assert cfg.window_samples == 160000 and cfg.c_config().skip_enabled == 0 and fa.EmbeddingConfig(skip_threshold=0.5).c_config().skip_enabled == 1


def test_non_finite_weights_only_matter_in_planned_chunks():
    w = np.zeros((3, 10, 3), f32)
    w[:, :, 0] = 1
    w[2, 4, 1] = np.nan                    # chunk 2 starts at 20 s: past 15 s of audio it is not planned
    p = E.plan(w, None, 1500, small_cfg())
    assert [r[0] for r in p["records"]] == [0, 1]
    try:
        E.plan(w, None, 2500, small_cfg())
    except ValueError:
        pass
    else:
        raise AssertionError("a NaN in a planned chunk must be refused")
