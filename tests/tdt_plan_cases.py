"""The recordings tests/test_gpu_tdt_plan.py plans, and the restatement's answers for them, computed once per mode.

Lengths: 0, 1, F - 1, F, F + 1, 2 F, one chunk exactly, chunk +- 1, stride +- 1 and stride + 2 F + 100 for both layouts (with and
without the mel context), and DRAWS draws of 1 ... 100 s plus 0 ... F - 1 samples.  Signals: Gaussian noise under a piecewise-constant
envelope in 0.2 s steps, drawn from {0, 0.0003, 0.002, 0.02, 0.1}, every fourth draw from {0.008, 0.02, 0.03} (the valley route needs a
dip that is no silence); every fifth draw ends in 1 ... 7 s of zeros.  Beside them the reference's own constant-0.02 signals with a
zeroed boundary (ChunkProcessorTests.swift:228-366), and one of stride + 2 F + 100 samples zeroed from stride - F on, whose quiet
probe runs into the end of the audio."""
import numpy as np

import tdt_plan_restatement as R

F, RATE = 1280, 16000
DRAWS = 40
LEVELS, VALLEY_LEVELS = (0.0, 0.0003, 0.002, 0.02, 0.1), (0.008, 0.02, 0.03)
SPECIAL_LENGTHS = (0, 1, F - 1, F, F + 1, 2 * F, 238080, 238079, 238081, 239360, 239359, 239361, 206079, 206081, 207359, 207361, 206080 + 2 * F + 100,
                   207360 + 2 * F + 100)


def noise(rng, n, levels):
    steps = -(-n // (RATE // 5)) if n else 0
    envelope = np.repeat(rng.choice(levels, steps), RATE // 5)[:n]
    return (rng.standard_normal(n) * envelope).astype(np.float32)


def flat(seconds, zero=()):
    x = np.full(seconds * RATE, 0.02, np.float32)
    for lo, hi in zero:
        x[lo:min(hi, x.size)] = 0
    return x


def recordings():
    rng = np.random.default_rng(20240747)
    out = [noise(rng, n, LEVELS) for n in SPECIAL_LENGTHS]
    for d in range(DRAWS):
        n = int(rng.integers(1, 101)) * RATE + int(rng.integers(0, F))
        x = noise(rng, n, VALLEY_LEVELS if d % 4 == 3 else LEVELS)
        if d % 5 == 4:
            x[max(0, n - int(rng.integers(1, 8)) * RATE):] = 0
        out.append(x)
    stride, chunk = 207360, 239360
    silent, trough, first = stride + 3 * F, (stride // F - 37) * F, stride - 50 * F
    out += [flat(45, [(silent - F, silent + F)]), flat(45), flat(45, [(silent - F, silent + 4 * F)]), flat(45, [(trough - F, trough + F)]),
            flat(90, [(first - F, first + F), (first + chunk - 2 * F, first + chunk)])]
    tail = np.full(stride + 2 * F + 100, 0.02, np.float32)
    tail[stride - F:] = 0
    out.append(tail)
    return out


def expected(audio, mode):
    """(records as tuples in TDT_WINDOW_DTYPE's order, window_range, speech_end) of the restatement for every recording."""
    cfg = R.Config(**R.MODES[mode])
    rows, window_range, speech_end = [], [0], []
    for b, x in enumerate(audio):
        windows, end = R.Planner(x, cfg).plan()
        rows += [(b, w["use_warmup_prefix"], w["is_last"], w["emit_after_frame"], w["global_frame_offset"], w["context_frames"], w["actual_audio_frames"], 0,
                  w["chunk_start"], w["warmup_samples"], w["context_samples"], w["context_start"], w["length"]) for w in windows]
        window_range.append(len(rows))
        speech_end.append(end)
    return rows, np.array(window_range, np.int64), np.array(speech_end, np.int64)
