"""fa_paraformer_cif(_dev) and fa_paraformer_timestamps(_dev) (csrc/paraformer.hip) on the device against the numpy restatement of the
reference's loop (tests/paraformer_restatement.py).  No tolerances: fp32 as int32 bit patterns, fp64 as int64, integers as they are.
The same file is run on the poisoned-workspace library (make POISON=1).  Each expectation is computed once per module."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import paraformer_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = (0, 1, 7, 65, 130)      # none, one, fewer than a block of 64 alphas, one more than a block, more than two blocks
MAX_TOKENS, ENC_FRAMES = 24, 70  # below the fires of the long utterances and below their frames: both clamps act


def config(fa, max_tokens=MAX_TOKENS, enc_frames=ENC_FRAMES):
    cfg = fa.paraformer.default_config()
    cfg.max_tokens, cfg.enc_frames = max_tokens, enc_frames
    return cfg


def i32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def i64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def expect_cif(enc, alphas, valid, max_tokens, enc_frames):
    """The restatement per utterance in the shapes of the entry: ac, token counts, fire counts, fire frames, enc_packed."""
    B, T, D = enc.shape
    ac, packed = np.zeros((B, max_tokens, D), np.float32), np.zeros((B, enc_frames, D), np.float32)
    tc, fc, ff = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, T + 1), -1, np.int32)
    for b in range(B):
        v = int(valid[b])
        ac[b], tc[b], fires, packed[b] = R.decoder_inputs(enc[b, :v], alphas[b, :v], enc_frames, max_tokens)
        fc[b] = len(fires)
        ff[b, :len(fires)] = fires
    return ac, tc, fc, ff, packed


def same_cif(got, want):
    ac, tc, fc, ff, packed = want
    assert np.array_equal(got.token_counts, tc) and np.array_equal(got.fire_counts, fc), (got.token_counts, tc, got.fire_counts, fc)
    assert np.array_equal(got.fire_frames, ff)
    bad = np.argwhere(i32(got.ac) != i32(ac))
    assert bad.size == 0, (bad[:5], got.ac[tuple(bad[0])], ac[tuple(bad[0])])
    if got.enc_packed is not None:
        assert np.array_equal(i32(got.enc_packed), i32(packed))


def batch_of_five(dim, T, seed):
    rng = np.random.default_rng(seed)
    enc = rng.standard_normal((5, T, dim)).astype(np.float32)
    alphas = rng.uniform(0.0, 0.5, (5, T)).astype(np.float32)
    valid = np.array([T, 0, T // 2, max(T - 1, 0), T], np.int32)
    return enc, alphas, valid


def strided(enc, pad, fill):
    """The same rows with `pad` elements of padding behind each: nothing may read them."""
    out = np.full(enc.shape[:2] + (enc.shape[2] + pad,), fill, enc.dtype)
    out[:, :, :enc.shape[2]] = enc
    return out


@pytest.fixture(scope="module")
def grid_cases():
    """(dim, T) -> inputs and the restatement's answers for fp32 and for fp16 rows; never modified."""
    cases = {}
    for dim in (1, 63, 512, 516):
        for T in FRAMES:
            enc, alphas, valid = batch_of_five(dim, T, 1000 * dim + T)
            half = enc.astype(np.float16)
            cases[dim, T] = (enc, half, alphas, valid, expect_cif(enc, alphas, valid, MAX_TOKENS, ENC_FRAMES),
                             expect_cif(half.astype(np.float32), alphas, valid, MAX_TOKENS, ENC_FRAMES))
    return cases


@pytest.mark.parametrize("dim", [1, 63, 512, 516])
def test_cif_grid(fa, gpu_ctx, grid_cases, dim):
    """Mixed valid_frames in a batch of five (0 among them), every load width: rows without padding, and with 8, 4 and 3 elements of
    NaN behind them (16-byte loads of fp32 and fp16, 8-byte loads of fp16, element loads)."""
    cfg = config(fa)
    for T in FRAMES:
        enc, half, alphas, valid, want32, want16 = grid_cases[dim, T]
        assert T < 130 or (want32[2].max() > MAX_TOKENS and valid.max() > ENC_FRAMES)
        for pad in (0, 8, 4, 3):
            same_cif(fa.cif_batch(strided(enc, pad, np.nan), alphas, valid, dim=dim, config=cfg, pack_enc=True, ctx=gpu_ctx), want32)
            same_cif(fa.cif_batch(strided(half, pad, np.nan), alphas, valid, dim=dim, config=cfg, pack_enc=True, ctx=gpu_ctx), want16)


def test_cif_without_valid_frames_and_without_packing(fa, gpu_ctx, grid_cases):
    enc, _, alphas, _, _, _ = grid_cases[63, 65]
    got = fa.cif_batch(enc, alphas, None, ctx=gpu_ctx)
    assert got.enc_packed is None and got.ac.shape == (5, 128, 63)
    same_cif(got, expect_cif(enc, alphas, [65] * 5, 128, 512))


def test_cif_one_token_over_two_hundred_frames(fa, gpu_ctx):
    """Alphas of 0.004: the first token takes 250 rows into one accumulator, in order."""
    rng = np.random.default_rng(7)
    enc = rng.standard_normal((2, 260, 64)).astype(np.float32)
    alphas = np.full((2, 260), 0.004, np.float32)
    valid = np.array([260, 255], np.int32)
    want = expect_cif(enc, alphas, valid, MAX_TOKENS, ENC_FRAMES)
    assert want[3][:, 0].tolist() == [249, 249] and want[2].tolist() == [1, 1]   # 10 and 5 more frames and the tail stay below 1
    same_cif(fa.cif_batch(enc, alphas, valid, config=config(fa), pack_enc=True, ctx=gpu_ctx), want)


def test_cif_more_fires_than_tokens(fa, gpu_ctx):
    """T = 300 with alphas of 0.9: about 270 fires; ac is truncated at 128 tokens, the fire frames are complete."""
    rng = np.random.default_rng(8)
    enc = rng.standard_normal((1, 300, 8)).astype(np.float32)
    alphas = np.full((1, 300), 0.9, np.float32)
    want = expect_cif(enc, alphas, [300], 128, 512)
    assert 260 <= want[2][0] <= 280 and want[1][0] == 128
    got = fa.cif_batch(enc, alphas, ctx=gpu_ctx, pack_enc=True)
    same_cif(got, want)
    assert (got.fire_frames[0, :got.fire_counts[0]] >= 0).all() and (got.fire_frames[0, got.fire_counts[0]:] == -1).all()


def test_cif_signed_zeros_and_exact_leftover(fa, gpu_ctx):
    """Rows with -0.0 and negative values, fires whose leftover is exactly 0 (alphas of 0.5): the seed h * 0 keeps the sign of h."""
    rng = np.random.default_rng(9)
    enc = rng.standard_normal((1, 12, 16)).astype(np.float32)
    enc[0, :, ::3] = -0.0
    enc[0, 3] = -np.abs(enc[0, 3])
    enc[0, 4] = 0.0          # the token seeded with -0.0 then adds +0.0 products
    alphas = np.full((1, 12), 0.5, np.float32)
    want = expect_cif(enc, alphas, [12], MAX_TOKENS, ENC_FRAMES)
    assert want[3][0, :6].tolist() == [1, 3, 5, 7, 9, 11] and np.signbit(want[0][0]).any()
    same_cif(fa.cif_batch(enc, alphas, config=config(fa), pack_enc=True, ctx=gpu_ctx), want)


def test_cif_alphas_above_one(fa, gpu_ctx):
    rng = np.random.default_rng(10)
    enc = rng.standard_normal((2, 9, 20)).astype(np.float32)
    alphas = np.array([[2.5, 0.0, 1.7, 3.2, 0.1, 0.0, 0.0, 0.6, 1.0], [1.0, 1.0, 1.0, 0.0, 5.5, 0.0, 0.0, 0.0, 0.0]], np.float32)
    want = expect_cif(enc, alphas, [9, 9], MAX_TOKENS, ENC_FRAMES)
    assert want[3][1, :want[2][1]].tolist() == [0, 1, 2, 4, 5, 6, 7, 8] and (np.diff(want[3][0, :want[2][0]]) == 1).any()
    same_cif(fa.cif_batch(enc, alphas, config=config(fa), pack_enc=True, ctx=gpu_ctx), want)


def test_cif_packed_encoder_has_a_zero_tail(fa, gpu_ctx, grid_cases):
    enc, _, alphas, valid, _, _ = grid_cases[512, 7]
    got = fa.cif_batch(enc, alphas, valid, pack_enc=True, ctx=gpu_ctx)
    assert got.enc_packed.shape == (5, 512, 512)
    for b in range(5):
        assert np.array_equal(i32(got.enc_packed[b, :valid[b]]), i32(enc[b, :valid[b]])) and not i32(got.enc_packed[b, valid[b]:]).any()
    assert not i32(got.ac[1]).any() and got.token_counts[1] == 0


def test_cif_device_entry_gives_the_same_bytes(fa, gpu_ctx, grid_cases):
    import torch
    cfg = config(fa)
    for dim, dtype in ((512, np.float16), (516, np.float32), (63, np.float32)):
        enc, half, alphas, valid, want32, want16 = grid_cases[dim, 130]
        rows = strided(half if dtype == np.float16 else enc, 8, np.nan)
        d_enc = torch.from_numpy(rows).cuda()[:, :, :dim]          # a view: the padding stays between the rows
        got = fa.cif_batch_dev(d_enc, torch.from_numpy(alphas).cuda(), valid, config=cfg, pack_enc=True, ctx=gpu_ctx)
        host = fa.cif_batch(rows, alphas, valid, dim=dim, config=cfg, pack_enc=True, ctx=gpu_ctx)
        back = fa.paraformer.CifResult(got.ac.cpu().numpy(), got.token_counts, got.fire_counts, got.fire_frames, got.enc_packed.cpu().numpy())
        same_cif(back, want16 if dtype == np.float16 else want32)
        assert back.ac.tobytes() == host.ac.tobytes() and back.enc_packed.tobytes() == host.enc_packed.tobytes()
        assert back.fire_frames.tobytes() == host.fire_frames.tobytes()


# ---------------------------------------------------------------------------------------------------------------- timestamps
VOCAB = {i: p for i, p in enumerate(["<blank>", "<s>", "</s>", "▁he", "llo", "cu@@", "t", "▁", "", "▁wor@@", "▁ld", "x"])}
KEEP = R.keep_table(VOCAB, 12)
# 12 kept tokens between a few dropped ones (blank, <s>, </s>, the empty piece, an id beyond the table)
IDS_12 = [1, 3, 4, 0, 5, 6, 7, 8, 9, 10, 40, 11, 3, 4, 0, 5, 6, 2]
IDS_9 = [1, 3, 4, 0, 5, 6, 8, 2, 40, 4, 4, 4, 4, 4]


def gated_tone(seed=3):
    """4 s: a 220 Hz tone gated at 5 Hz, solid from 2.0 to 2.9 s, over noise of sigma 0.001."""
    rng = np.random.default_rng(seed)
    t = np.arange(4 * 16000) / 16000.0
    gate = ((np.floor(t * 10) % 2) == 0) | ((t >= 2.0) & (t < 2.9))
    return (0.3 * np.sin(2 * np.pi * 220 * t) * gate + 0.001 * rng.standard_normal(t.size)).astype(np.float32)


def utterances():
    """(token ids, alphas [66], valid frames, audio) for every case of the issue; index 0 is the main one."""
    tone = gated_tone()
    a_main = np.random.default_rng(189).uniform(0.0, 0.45, 66).astype(np.float32)   # a seed that also reaches the window without a run
    a_flat = np.full(66, 0.051, np.float32)
    tiny = tone.copy()
    tiny[16000:16000 + 480] = 1e-20                                  # three frames of denormal squares
    return [(IDS_12, a_main, 66, tone),                              # the fallback path, several runs in a window, a window without a run
            (IDS_9, a_flat, 66, tone),                               # 10 fires for 9 tokens: no fallback
            (IDS_12, a_main, 66, tone[:100]),                        # shorter than one hop: no envelope
            (IDS_12, a_main, 66, tone[:16000 + 500][16000:]),        # three envelope frames: no smoothing
            (IDS_12, a_main, 40, tiny),
            ([0, 1, 2, 8, 40], a_main, 66, tone),                    # no kept token
            (IDS_9, a_main, 0, tone),                                # no frames: the rescaled tail fires once
            ([], a_main, 66, tone),                                  # no tokens at all
            (IDS_12, a_flat, 66, np.zeros(0, np.float32))]           # no audio


@pytest.fixture(scope="module")
def stamp_cases():
    utts = utterances()
    want, traces = [], []
    for ids, alphas, valid, audio in utts:
        trace = {}
        want.append(R.raw_spans(ids, KEEP, alphas[:valid], audio, trace))
        traces.append(trace)
    return utts, want, traces


def run_stamps(fa, ctx, utts, cfg, order=None, dev=False, capacity=None):
    order = list(range(len(utts))) if order is None else order
    ids = np.zeros((len(order), cfg.max_tokens), np.int32)
    counts = np.zeros(len(order), np.int32)
    for k, u in enumerate(order):
        counts[k] = len(utts[u][0])
        ids[k, :counts[k]] = utts[u][0]
        ids[k, counts[k]:] = 3                                       # a kept id behind the count: never looked at
    alphas = np.stack([utts[u][1] for u in order])
    valid = np.array([utts[u][2] for u in order], np.int32)
    audio = [utts[u][3] for u in order]
    if not dev:
        return fa.timestamps_batch(alphas, valid, ids, counts, KEEP, audio, config=cfg, capacity=capacity, ctx=ctx)
    import torch
    off = np.concatenate([[5], 5 + np.cumsum([a.size for a in audio])]).astype(np.int64)   # the first utterance does not start the tensor
    flat = torch.from_numpy(np.concatenate([np.full(5, np.nan, np.float32)] + audio)).cuda()
    return fa.timestamps_batch_dev(torch.from_numpy(alphas).cuda(), valid, torch.from_numpy(ids).cuda(), counts, KEEP, flat, off, config=cfg, capacity=capacity, ctx=ctx)


def same_spans(got, want_lists):
    spans, per_utt = got
    assert per_utt.tolist() == [len(w) for w in want_lists]
    flat = [(u, tok, s, e) for u, w in enumerate(want_lists) for tok, s, e in w]
    assert spans["utterance"].tolist() == [f[0] for f in flat] and spans["token_index"].tolist() == [f[1] for f in flat]
    assert np.array_equal(i64(spans["start"]), i64([f[2] for f in flat])), (spans["start"], [f[2] for f in flat])
    assert np.array_equal(i64(spans["end"]), i64([f[3] for f in flat])), (spans["end"], [f[3] for f in flat])


def test_timestamp_inputs_take_the_paths_they_are_meant_to(stamp_cases):
    utts, want, traces = stamp_cases
    # the main case: the fallback rescale, windows with several runs, a chosen run that is not the first, a window without a run
    assert traces[0]["fallback"] and len(want[0]) == 12 and 0 < len(traces[0]["no_run"]) < 12
    assert any(n > 1 for n, _ in traces[0]["runs"]) and any(k > 0 for _, k in traces[0]["runs"])
    assert not traces[1]["fallback"] and len(traces[1]["fires"]) == 10 and len(want[1]) == 9
    assert [len(w) for w in want[2:]] == [12, 12, 12, 0, 0, 0, 12]
    assert traces[2]["no_run"] == list(range(12)) and traces[2]["threshold"] == np.float32(1e-4) and traces[6]["fires"] == [0]
    assert R.energy_envelope(utts[3][3]).size == 3 and R.energy_envelope(utts[4][3])[101] < 1.1e-20


def test_timestamps_main_and_non_fallback(fa, gpu_ctx, stamp_cases):
    utts, want, _ = stamp_cases
    cfg = config(fa)
    same_spans(run_stamps(fa, gpu_ctx, utts, cfg, [0]), [want[0]])
    same_spans(run_stamps(fa, gpu_ctx, utts, cfg, [1]), [want[1]])
    segs = fa.segments_from_spans(VOCAB, utts[0][0], run_stamps(fa, gpu_ctx, utts, cfg, [0])[0])
    assert [tuple(s) for s in segs] == R.segments_from_spans([VOCAB[utts[0][0][i]] for i, _, _ in want[0]], [(s, e) for _, s, e in want[0]])


def test_timestamps_mixed_batch_and_both_entries(fa, gpu_ctx, stamp_cases):
    utts, want, _ = stamp_cases
    cfg = config(fa)
    order = [4, 2, 0, 5, 3, 6, 1, 7, 8, 0]
    host = run_stamps(fa, gpu_ctx, utts, cfg, order)
    same_spans(host, [want[u] for u in order])
    dev = run_stamps(fa, gpu_ctx, utts, cfg, order, dev=True)
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tolist() == host[1].tolist()
    for u in (2, 3, 4, 5, 6, 7, 8):                                  # each edge case alone: the workspace starts at zero
        same_spans(run_stamps(fa, gpu_ctx, utts, cfg, [u]), [want[u]])


def test_timestamps_default_token_budget(fa, gpu_ctx, stamp_cases):
    utts, want, _ = stamp_cases
    same_spans(run_stamps(fa, gpu_ctx, utts, fa.paraformer.default_config(), [0, 1]), [want[0], want[1]])


def test_timestamps_arena_one_record_too_small(fa, gpu_ctx, stamp_cases):
    utts, want, _ = stamp_cases
    cfg = config(fa)
    total = len(want[0]) + len(want[1])
    same_spans(run_stamps(fa, gpu_ctx, utts, cfg, [0, 1], capacity=total), [want[0], want[1]])
    with pytest.raises(fa.FluidAudioHipError) as e:
        run_stamps(fa, gpu_ctx, utts, cfg, [0, 1], capacity=total - 1)
    assert e.value.status == fa._lib.OUTPUT_TOO_SMALL
    # the count alone: no output array
    count, per_utt = fa._lib.C.c_int64(-1), np.zeros(1, np.int64)
    ids = np.zeros((1, cfg.max_tokens), np.int32)
    ids[0, :len(IDS_12)] = IDS_12
    counts, off = np.array([len(IDS_12)], np.int32), np.array([0, utts[0][3].size], np.int64)
    st = fa.lib().fa_paraformer_timestamps(gpu_ctx.handle, fa._lib.C.byref(cfg), utts[0][1].ctypes.data, 66, 1, 66, None, ids.ctypes.data, counts.ctypes.data,
                                           KEEP.ctypes.data, KEEP.size, utts[0][3].ctypes.data, off.ctypes.data, None, 0, fa._lib.C.byref(count), per_utt.ctypes.data)
    assert st == 0 and count.value == 12 and per_utt.tolist() == [12]


def test_no_utterances(fa, gpu_ctx):
    count = fa._lib.C.c_int64(-1)
    assert fa.lib().fa_paraformer_timestamps(gpu_ctx.handle, None, None, 0, 0, 0, None, None, None, None, 0, None, None, None, 0, fa._lib.C.byref(count), None) == 0
    assert count.value == 0
    assert fa.lib().fa_paraformer_cif(gpu_ctx.handle, None, None, 0, 0, 4, 8, 8, 32, None, 4, None, None, None, None, None, None) == 0
    assert fa.cif_batch(np.zeros((0, 3, 4), np.float32), np.zeros((0, 3), np.float32), ctx=gpu_ctx).ac.shape == (0, 128, 4)
