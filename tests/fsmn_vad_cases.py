"""The inputs of the FSMN-VAD tests: the recording lengths, the configs and the generators of silence probabilities.  Test
infrastructure; the expectation is tests/fsmn_vad_restatement.py."""
import numpy as np

import fsmn_vad_restatement as R

# 64 +- 1 and 128 +- 1: the two-word window and the carried silence run cross a step boundary there
LENGTHS = (0, 1, 14, 15, 19, 20, 21, 63, 64, 65, 127, 128, 129, 200, 1000, 7000)
DENSITIES = (0.05, 0.25, 0.5, 0.75, 0.95)
CONFIGS = {
    "default": R.Config(),
    "hysteresis": R.Config(sil_to_speech=12, speech_to_sil=8),                                       # on above off: the hold class
    "wide": R.Config(window_frames=64, sil_to_speech=40, speech_to_sil=30, max_segment_frames=300),
    "short": R.Config(max_segment_frames=200, max_end_silence_frames=5, lookahead_frames=0),
}


def probs_of(speech, rng):
    """Probabilities on either side of 0.2 for a 0 / 1 sequence (the reference compares p <= 0.2)."""
    speech = np.asarray(speech, bool)
    return np.where(speech, rng.uniform(0.0, 0.2, speech.size), rng.uniform(0.21, 1.0, speech.size)).astype(np.float32)


def blocks(rng, n):
    """Blocks of 1 ... 199 frames, each with a speech density of its own."""
    parts, have = [np.zeros(0, bool)], 0
    while have < n:
        draws = rng.random(int(rng.integers(1, 200)))
        parts.append(draws < DENSITIES[int(rng.integers(len(DENSITIES)))])
        have += draws.size
    return probs_of(np.concatenate(parts)[:n], rng)


def noise(rng, n):
    """Speech with probability 10 / 13: the window count of the defaults hovers at its threshold of 15, so preSpeech flips often and no
    silence lasts; the long recording runs into the maximal segment length."""
    return rng.uniform(0.0, 0.26, n).astype(np.float32)


def recordings(seed):
    """One recording per length from the block generator and one from uniform noise, empty recordings between."""
    rng = np.random.default_rng(seed)
    out = []
    for n in LENGTHS:
        out += [blocks(rng, n), np.zeros(0, np.float32), noise(rng, n)]
    return out


def plateau(count, frames, window=20):
    """A window count held at exactly `count` from frame window - 1 on: the speech bits repeat with period `window`."""
    period = np.array([1] * count + [0] * (window - count), bool)
    return np.where(np.resize(period, frames), np.float32(0.1), np.float32(0.9)).astype(np.float32)


def config_abi(fa, cfg):
    return fa.fsmn_vad_config(cfg.silence_threshold, cfg.window_frames, cfg.sil_to_speech, cfg.speech_to_sil, cfg.max_end_silence_frames, cfg.lookback_frames,
                              cfg.lookahead_frames, cfg.max_segment_frames, cfg.frame_ms)


def expected_records(probs_list, cfg, events=None):
    """(rows of FSMN_VAD_SEGMENT_DTYPE's fields, counts int64[B]) of the restatement."""
    rows, counts = [], []
    for b, p in enumerate(probs_list):
        segs = R.decide(p, cfg, events)
        counts.append(len(segs))
        rows += [(b, reason, s, e, sm, em) for s, e, reason, sm, em in segs]
    return rows, np.array(counts, np.int64)
