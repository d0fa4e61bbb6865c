"""fa_fsmn_vad_segments, fa_fsmn_vad_pack_waveforms, fa_fsmn_vad_pack_feats_dev and fa_fsmn_vad_gather_silence_dev (csrc/fsmn_vad.hip)
against the line-by-line restatement of the reference (tests/fsmn_vad_restatement.py).  No tolerances: integers as they are, fp32 as
bits.  The same file is run on the poisoned-workspace library (make POISON=1).  Each expectation is computed once per module."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsmn_vad_cases as K  # noqa: E402
import fsmn_vad_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def ranges_of(probs_list):
    return np.concatenate([[0], np.cumsum([p.size for p in probs_list])]).astype(np.int64)


@pytest.fixture(scope="module")
def seg_cases(fa):
    """Per config the mixed batch of tests/fsmn_vad_cases.py and the restatement's answer as records of FSMN_VAD_SEGMENT_DTYPE."""
    cases = {}
    for name, cfg in K.CONFIGS.items():
        probs_list = K.recordings(11)
        rows, counts = K.expected_records(probs_list, cfg)
        per_recording = np.split(np.array(rows, fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE), np.cumsum(counts)[:-1])
        cases[name] = dict(cfg=K.config_abi(fa, cfg), probs=probs_list, want=np.array(rows, fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE), counts=counts, per_recording=per_recording)
    return cases


@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_segments_are_the_restated_ones(fa, gpu_ctx, seg_cases, name):
    import torch
    case = seg_cases[name]
    assert len(case["want"]) > 20 and set(case["want"]["reason"].tolist()) == {0, 1, 2}
    got, counts = fa.fsmn_vad_segments(case["probs"], config=case["cfg"], ctx=gpu_ctx)            # one batch of mixed lengths, empty recordings between
    assert counts.tolist() == case["counts"].tolist()
    assert got.tobytes() == case["want"].tobytes()                                              # with the reason and the milliseconds
    flat, frame_range = np.concatenate(case["probs"]), ranges_of(case["probs"])
    lead = 5                                                                                    # the device entry addresses the caller's array from frame_range[0]
    dev = torch.from_numpy(np.concatenate([np.full(lead, 0.01, np.float32), flat, np.full(7, 0.01, np.float32)])).cuda()
    got_dev, counts_dev = fa.fsmn_vad_segments_dev(dev, frame_range + lead, config=case["cfg"], ctx=gpu_ctx)
    assert got_dev.tobytes() == case["want"].tobytes() and counts_dev.tolist() == case["counts"].tolist()


@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_single_recordings(fa, gpu_ctx, seg_cases, name):
    import torch
    case = seg_cases[name]
    for b, p in enumerate(case["probs"]):
        want = case["per_recording"][b].copy()
        want["recording"] = 0
        got, counts = fa.fsmn_vad_segments([p], config=case["cfg"], ctx=gpu_ctx)
        assert got.tobytes() == want.tobytes() and counts.tolist() == [len(want)], (name, b, p.size)
        if p.size in (63, 64, 65, 129):
            dev = torch.from_numpy(np.concatenate([np.full(3, 0.01, np.float32), p])).cuda()
            got, _ = fa.fsmn_vad_segments_dev(dev, np.array([3, 3 + p.size], np.int64), config=case["cfg"], ctx=gpu_ctx)
            assert got.tobytes() == want.tobytes(), (name, b, p.size)


def test_the_overlap_after_a_maximal_close_and_the_flip_on_a_plateau(fa, gpu_ctx):
    got, _ = fa.fsmn_vad_segments([np.full(7000, 0.1, np.float32)], ctx=gpu_ctx)
    assert [(int(s["start_frame"]), int(s["end_frame"]), int(s["reason"]), int(s["start_ms"]), int(s["end_ms"])) for s in got] == [
        (0, 6000, 1, 0, 60000), (5966, 7000, 2, 59660, 70000)]
    # a window count held at exactly 15: preSpeech flips on every frame, so with max_end_silence 1 every other frame closes a segment
    p = K.plateau(15, 400)
    for cfg in (R.Config(), R.Config(max_end_silence_frames=1), R.Config(max_end_silence_frames=2)):
        rows, counts = K.expected_records([p], cfg)
        got, got_counts = fa.fsmn_vad_segments([p], config=K.config_abi(fa, cfg), ctx=gpu_ctx)
        assert got.tobytes() == np.array(rows, fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE).tobytes() and got_counts.tolist() == counts.tolist()
    assert counts[0] == 1 and len(K.expected_records([p], R.Config(max_end_silence_frames=1))[0]) == (400 - 14) // 2


def test_segments_count_and_capacity(fa, gpu_ctx, seg_cases):
    case = seg_cases["short"]
    want, B = case["want"], len(case["probs"])
    flat, frame_range = np.concatenate(case["probs"]), ranges_of(case["probs"])
    f, count, counts = fa.lib().fa_fsmn_vad_segments, C.c_int64(-1), np.full(B, -1, np.int64)
    args = (gpu_ctx.handle, C.byref(case["cfg"]), flat.ctypes.data, frame_range.ctypes.data, B)
    assert f(*args, None, 0, C.byref(count), counts.ctypes.data) == fa.SUCCESS                      # segs == NULL: the count
    assert count.value == len(want) and counts.tolist() == case["counts"].tolist()
    none = np.zeros(1, fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE)
    count.value = -1
    assert f(*args, none.ctypes.data, 0, C.byref(count), None) == fa._lib.OUTPUT_TOO_SMALL and count.value == len(want) and not none.tobytes().strip(b"\0")
    for capacity in (len(want) - 1, 3):                                                             # 3: below what single recordings close
        short = np.zeros(capacity, fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE)
        count.value = -1
        assert f(*args, short.ctypes.data, short.size, C.byref(count), None) == fa._lib.OUTPUT_TOO_SMALL
        assert count.value == len(want) and short.tobytes() == want[:capacity].tobytes()
    count.value = -1
    assert f(gpu_ctx.handle, None, flat.ctypes.data, frame_range.ctypes.data, 0, None, 0, C.byref(count), None) == fa.SUCCESS and count.value == 0
    d = seg_cases["default"]                                                                        # cfg == NULL is the default config
    got = np.zeros(len(d["want"]), fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE)
    assert f(gpu_ctx.handle, None, np.concatenate(d["probs"]).ctypes.data, frame_range.ctypes.data, B, got.ctypes.data, got.size, C.byref(count), None) == fa.SUCCESS
    assert got.tobytes() == d["want"].tobytes()


def test_nan_probabilities_are_not_speech(fa, gpu_ctx):
    rng = np.random.default_rng(5)
    probs = [K.blocks(rng, n) for n in (65, 130, 1000)]
    for p in probs:
        p[rng.integers(0, p.size, p.size // 5)] = np.nan
    cfg = K.CONFIGS["short"]
    rows, counts = K.expected_records(probs, cfg)
    assert rows == K.expected_records([np.where(np.isnan(p), np.float32(0.9), p) for p in probs], cfg)[0] and len(rows) > 5
    got, got_counts = fa.fsmn_vad_segments(probs, config=K.config_abi(fa, cfg), ctx=gpu_ctx)
    assert got.tobytes() == np.array(rows, fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE).tobytes() and got_counts.tolist() == counts.tolist()


def test_more_recordings_than_one_scan_block_carries(fa, gpu_ctx):
    """A few hundred one-step recordings: the scan of the slices' fill runs over more than one block of its workgroup."""
    rng = np.random.default_rng(9)
    probs = [K.blocks(rng, int(n)) for n in rng.integers(0, 65, 600)]
    cfg = R.Config(max_end_silence_frames=3, max_segment_frames=40, lookahead_frames=1)
    rows, counts = K.expected_records(probs, cfg)
    got, got_counts = fa.fsmn_vad_segments(probs, config=K.config_abi(fa, cfg), ctx=gpu_ctx)
    assert len(probs) > 2 * 256 and len(rows) > 256                                             # the inputs: more than two blocks of the scan
    assert got_counts.tolist() == counts.tolist() and got.tobytes() == np.array(rows, fa.fsmn_vad.FSMN_VAD_SEGMENT_DTYPE).tobytes()


# ---- round the two networks
CHAIN_SAMPLES = (320_000, 495_533)


@pytest.fixture(scope="module")
def chain(fa):
    rng = np.random.default_rng(2)
    audio = [rng.uniform(-1, 1, n).astype(np.float32) for n in CHAIN_SAMPLES]
    chunks, chunk_range, frame_range = fa.fsmn_vad_plan_chunks(CHAIN_SAMPLES)
    assert chunk_range.tolist() == [0, 1, 3] and frame_range.tolist() == [0, R.lfr_frame_count(320_000), R.lfr_frame_count(320_000) + 3093]
    return dict(audio=audio, chunks=chunks, frame_range=frame_range)


def test_packed_waveforms_are_the_scaled_samples(fa, gpu_ctx, chain):
    import torch
    chunks, audio = chain["chunks"], chain["audio"]
    lengths = (chunks["end_sample"] - chunks["start_sample"]).tolist()
    offsets = np.array([0, CHAIN_SAMPLES[0], sum(CHAIN_SAMPLES)], np.int64)
    for lead, stride in ((0, max(lengths)), (3, max(lengths) + 4), (1, max(lengths) + 1)):        # 16-byte stores, and rows that are not aligned
        want = np.stack([R.waveform_row(audio[c["recording"]], int(c["start_sample"]), int(c["end_sample"]), stride) for c in chunks])
        dev = torch.from_numpy(np.concatenate([np.full(lead, np.nan, np.float32)] + audio)).cuda()
        rows = fa.fsmn_vad_pack_waveforms_dev(dev, offsets + lead, chunks, row_stride=stride, ctx=gpu_ctx)
        assert rows.cpu().numpy().tobytes() == want.tobytes()                                     # audio * float32(32768) bit for bit, zero tails
    host = fa.fsmn_vad_pack_waveforms(audio, chunks, ctx=gpu_ctx)
    assert host.shape == (3, max(lengths)) and host.tobytes() == np.stack([R.waveform_row(audio[c["recording"]], int(c["start_sample"]), int(c["end_sample"]), max(lengths))
                                                                           for c in chunks]).tobytes()
    with pytest.raises(fa.FluidAudioHipError) as e:
        fa.fsmn_vad_pack_waveforms(audio, chunks, row_stride=max(lengths) - 1, ctx=gpu_ctx)
    assert e.value.status == fa.INVALID_ARGUMENT


PACK_SLICE = 4096                                 # samples of a row one workgroup writes (csrc/row_pack_launch.h: kPackSlice)


@pytest.mark.parametrize("stride", (PACK_SLICE - 4, PACK_SLICE, PACK_SLICE + 4, PACK_SLICE + 3))
def test_packed_rows_round_a_slice_and_across_groups(fa, gpu_ctx, stride):
    """Rows one group of four short of a slice, a slice, one group into a second slice, and a stride that is no multiple of four (the
    dword path); 64, 65 and 129 chunks (a launch carries 64) of 0, 1, stride - 1 and stride samples, from sources that are not 16-byte
    aligned.  Every row is float32(x) * float32(32768) bit for bit, then zeros."""
    import torch
    rng = np.random.default_rng(stride)
    audio = rng.uniform(-1, 1, stride + 300).astype(np.float32)
    audio[:6] = (np.inf, -np.inf, 1e-40, -0.0, 3e38, 2.0 ** -15)                                 # the product overflows, leaves the denormals, is exact
    lead = 3
    dev = torch.from_numpy(np.concatenate([np.full(lead, np.nan, np.float32), audio, np.full(5, np.nan, np.float32)])).cuda()
    offsets = np.array([lead, lead + audio.size], np.int64)
    for count in (64, 65, 129):
        chunks = np.zeros(count, fa.fsmn_vad.FSMN_VAD_CHUNK_DTYPE)
        chunks["start_sample"] = rng.integers(0, 300, count)
        chunks["start_sample"][:4] = (0, 1, 2, 3)
        chunks["end_sample"] = chunks["start_sample"] + np.resize(np.array([0, 1, stride - 1, stride]), count)
        chunks["end_sample"][-1] = chunks["start_sample"][-1] + stride                           # the last row of the last group is a full one
        want = np.zeros((count, stride), np.float32)
        for i, c in enumerate(chunks):
            n = int(c["end_sample"] - c["start_sample"])
            with np.errstate(over="ignore"):
                want[i, :n] = audio[c["start_sample"]:c["end_sample"]] * np.float32(32768)
        rows = fa.fsmn_vad_pack_waveforms_dev(dev, offsets, chunks, row_stride=stride, ctx=gpu_ctx)
        assert rows.shape == (count, stride) and rows.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_gathered_silence_is_the_frame_grid(fa, gpu_ctx, chain, dtype):
    """The reference test's own stand-in scorer: column 0 of a chunk's frame i is its absolute frame start / 160 + i, so the gathered
    array is 0, 1, 2, ... with no gap or repeat across the chunk boundary."""
    import torch
    chunks, frame_range = chain["chunks"], chain["frame_range"]
    if dtype == "float16":                                                                      # indices below 2048 are exact in fp16
        samples = (200_000, 250_000)
        chunks, _, frame_range = fa.fsmn_vad_plan_chunks(samples)
        chunks = chunks.copy()
        chunks["frames"][0] = 700                                                               # two chunks for the first recording, as a scorer of a smaller bucket would see them
        second = np.array([(0, 1024, 698 * 160, 200_000, R.lfr_frame_count(200_000 - 698 * 160), 2, 700)], fa.fsmn_vad.FSMN_VAD_CHUNK_DTYPE)
        chunks = np.concatenate([chunks[:1], second, chunks[1:]])
        assert 700 + int(second["frames"][0]) - 2 == R.lfr_frame_count(200_000)
    bucket, vocab = 3072 if dtype == "float32" else 2048, 3
    scores = torch.full((chunks.size, bucket, vocab), -1.0, dtype=getattr(torch, dtype), device="cuda")
    for k, c in enumerate(chunks):
        scores[k, :, 0] = (int(c["start_sample"]) // 160 + torch.arange(bucket, device="cuda")).to(scores.dtype)
    silence = fa.fsmn_vad_gather_silence_dev(scores, chunks, frame_range, ctx=gpu_ctx).cpu().numpy()
    want = np.concatenate([np.arange(n, dtype=np.float32) for n in np.diff(frame_range)])
    assert silence.dtype == np.float32 and silence.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_packed_features_are_the_zero_padded_bucket(fa, gpu_ctx, dtype):
    import torch
    rng = np.random.default_rng(4)
    frames = (0, 1, 37, 512, 300)
    chunks = np.zeros(len(frames), fa.fsmn_vad.FSMN_VAD_CHUNK_DTYPE)
    chunks["frames"] = frames
    for lead in (0, 1):                                                                         # a base that is not aligned takes the narrow route
        feats = rng.standard_normal((len(frames), 515, 400)).astype(dtype)
        flat = torch.from_numpy(np.concatenate([np.zeros(lead, dtype), feats.reshape(-1)])).cuda()
        dev = flat[lead:].view(len(frames), 515, 400)
        out = fa.fsmn_vad_pack_feats_dev(dev, chunks, 512, ctx=gpu_ctx).cpu().numpy()
        want = np.stack([R.bucket_rows(feats[k], t, 512) for k, t in enumerate(frames)])
        assert out.tobytes() == want.tobytes()
    with pytest.raises(fa.FluidAudioHipError) as e:
        fa.fsmn_vad_pack_feats_dev(dev, chunks, 511, ctx=gpu_ctx)                                  # a chunk larger than the bucket
    assert e.value.status == fa.INVALID_ARGUMENT
