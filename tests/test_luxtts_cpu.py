"""The LuxTTS plan (fluidaudio_amd/csrc/luxtts_core.h through fa_luxtts_plan) against a line-by-line restatement of
LuxTtsSynthesizer.swift:59-128 and LuxTtsSolver.swift:11-40, the solver's time steps, and the known answers of LuxTtsSolverTests.swift.
No device."""
import itertools
import math

import numpy as np
import pytest

HOP, CAP, MAX_TOKENS, MAX_FRAMES, BUCKETS, OUT_HOP = 256, 120000, 256, 1024, (282, 555), 512
GRID = list(itertools.product([0, 127, 128, 300, 103936, 120000, 200000], [1, 37], [1, 60, 230], [0.0, 0.7, 1.0, 1.3]))
GRID.append((103936, 37, 60, 1.1))          # the grid has no item whose generated frames pass the largest bucket inside 1024 frames


def restated(n, prompt_tokens, text_tokens, speed):
    """(status, samples, prompt_frames, tokens, features_length, gen_frames, avg, bucket, sample_count): the guards in the reference's order"""
    refuse = lambda s: (s, 0, 0, 0, 0, 0, 0, 0, 0)  # noqa: E731
    speed = float(np.float32(speed))
    if n == 0:
        return refuse(1)                                         # :59 no samples
    if not speed > 0:
        return refuse(2)                                         # :62
    samples = min(n, CAP)                                        # :71-73
    prompt_frames = (samples + HOP // 2) // HOP                  # MelExtractor :45-47
    if prompt_frames <= 0:
        return refuse(3)                                         # :95
    tokens = prompt_tokens + text_tokens
    if tokens + 1 > MAX_TOKENS:
        return refuse(4)                                         # :102
    generated = float(prompt_frames) / float(prompt_tokens) * float(text_tokens) / speed   # Solver :14-16
    features = prompt_frames + int(math.ceil(generated))
    if features > MAX_FRAMES:
        return refuse(5)                                         # :112
    gen = features - prompt_frames
    if gen < 2:
        return refuse(6)                                         # :118
    bucket = next((b for b in BUCKETS if b >= gen), None)
    if bucket is None:
        return refuse(7)                                         # :124
    avg = features // tokens
    if avg < 1:
        return refuse(8)                                         # Solver :37
    return 0, samples, prompt_frames, tokens, features, gen, avg, bucket, min((gen - 1) * OUT_HOP, (bucket - 1) * OUT_HOP)   # :275


def fields(p):
    return p.status, p.samples, p.prompt_frames, p.tokens, p.features_length, p.gen_frames, p.avg, p.bucket, p.sample_count


def test_the_grid_meets_every_status():
    assert {restated(*c)[0] for c in GRID} == set(range(9))


@pytest.mark.parametrize("case", GRID)
def test_plan_is_the_restatement(fa, case):
    plans, _ = fa.luxtts_plan([case[0]], case[1], case[2], case[3])
    assert fields(plans[0]) == restated(*case)


def test_plan_lists_the_items_of_every_bucket(fa):
    n, pt, tt, sp = (list(v) for v in zip(*GRID))
    plans, buckets = fa.luxtts_plan(n, pt, tt, sp)
    assert [fields(p) for p in plans] == [restated(*c) for c in GRID]
    assert buckets == {b: [i for i, p in enumerate(plans) if p.status == 0 and p.bucket == b] for b in BUCKETS} and all(buckets.values())


def test_time_steps_are_the_double_formula(fa):
    got = fa.luxtts_time_steps()
    assert got.tolist() == [0.5 * (i / 4) / (1.0 + (0.5 - 1.0) * (i / 4)) for i in range(5)]          # Solver :21-26
    assert np.allclose(got, [0, 1 / 7, 1 / 3, 3 / 5, 1], rtol=0, atol=1e-16) and got[0] == 0.0 and got[-1] == 1.0
    assert got.astype(np.float32).tolist() == [0.0, 0.1428571492433548, 0.3333333432674408, 0.6000000238418579, 1.0]   # the fixture's float32 steps


def test_known_answers_of_the_solver_tests(fa):
    """LuxTtsSolverTests.swift with luxtts_fixtures.json: 406 prompt frames, 80 prompt tokens; 85 text tokens -> 838 frames, 91 -> 868; the
    expansion of 165 tokens over 838 frames has avg 5 and 13 remainder frames on the pad slot; 10 tokens over 5 frames is degenerate, 4
    over 4 is not."""
    plans, _ = fa.luxtts_plan([103936, 103936, 512, 512], [80, 80, 4, 2], [85, 91, 6, 2], 1.0)
    assert (plans[0].prompt_frames, plans[0].features_length, plans[0].tokens, plans[0].avg) == (406, 838, 165, 5)
    assert plans[0].features_length - plans[0].tokens * plans[0].avg == 13 and plans[0].sample_count == 220672       # e2e.wav_samples
    assert (plans[1].features_length, plans[1].tokens, plans[1].avg) == (868, 171, 5)
    assert plans[2].status == 8                                                                                      # tokens 10, frames 5
    assert (plans[3].status, plans[3].tokens, plans[3].features_length, plans[3].avg) == (0, 4, 4, 1)
