"""fa_tdt_plan_windows, fa_tdt_pack_windows and fa_tdt_speech_gate (csrc/tdt_plan.hip) against the line-by-line restatement of the
reference (tests/tdt_plan_restatement.py) on the recordings of tests/tdt_plan_cases.py, for the four mode combinations in use.  No
tolerances: integers as they are, fp32 and fp64 as bits.  The same file is run on the poisoned-workspace library (make POISON=1).  Each
expectation is computed once per module.

The routes the inputs must reach are R.BRANCH_NAMES.  Two routes are named as unreachable under the argument checks and not claimed:
`bestStart <= previousStart` and `chunkEnd <= chunkStart` (R.UNREACHABLE says why).  The empty candidate list is NOT among them: a start
that lies 4 s in front of its target leaves the next target's valley search (+-0.5 s) without a candidate, and the inputs reach it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_plan_cases as K  # noqa: E402
import tdt_plan_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

F, RATE = K.F, K.RATE
INVALID_ARGUMENT, OUTPUT_TOO_SMALL = 1, 3
POISON = np.uint32(0xDEADBEEF)
MODE_ARGS = {"default": (True, False, 0), "path_a": (False, True, 0), "path_b": (False, True, 7), "path_c": (False, False, 0)}


def config_of(fa, mode):
    return fa.tdt_window_config(*MODE_ARGS[mode])


@pytest.fixture(scope="module")
def cases(fa):
    """The recordings, flat with their offsets, and per mode the restatement's records, ranges and speech ends."""
    R.BRANCHES.clear()
    audio = K.recordings()
    offsets = np.concatenate([[0], np.cumsum([x.size for x in audio])]).astype(np.int64)
    out = dict(audio=audio, flat=np.concatenate(audio), offsets=offsets)
    for mode in R.MODES:
        rows, window_range, speech_end = K.expected(audio, mode)
        out[mode] = dict(want=np.array(rows, fa.TDT_WINDOW_DTYPE), window_range=window_range, speech_end=speech_end)
    out["branches"] = dict(R.BRANCHES)
    return out


def five_of(records):
    return [records[k].astype(np.int32) for k in ("actual_audio_frames", "context_frames", "is_last", "global_frame_offset", "emit_after_frame")]


def test_the_inputs_reach_every_route_of_the_reference(cases):
    taken = cases["branches"]
    print(taken)
    assert all(taken.get(name, 0) > 0 for name in R.BRANCH_NAMES), {n: taken.get(n, 0) for n in R.BRANCH_NAMES}
    assert not any(taken.get(name, 0) for name in R.UNREACHABLE)                 # named, not claimed
    assert any(x.size and cases["offsets"][b] % 2 == 1 for b, x in enumerate(cases["audio"]))   # a recording at an odd offset


@pytest.mark.parametrize("mode", list(R.MODES))
def test_windows_are_the_restated_ones(fa, gpu_ctx, cases, mode):
    import torch
    case, cfg = cases[mode], config_of(fa, mode)
    want = case["want"]
    assert len(want) > 200 and len(cases["audio"]) >= 3
    counts = np.diff(case["window_range"])
    bounds = [fa.tdt_window_count_bound(x.size, cfg) for x in cases["audio"]]
    assert bounds == [R.window_count_bound(R.Config(**R.MODES[mode]), x.size) for x in cases["audio"]]
    assert all(c <= b for c, b in zip(counts, bounds))                            # the bound, on every input
    got = fa.tdt_plan_windows(cases["flat"], cases["offsets"], config=cfg, ctx=gpu_ctx)
    assert got.window_range.tolist() == case["window_range"].tolist()
    assert got.speech_end.tolist() == case["speech_end"].tolist() and not got.statuses.any()
    assert got.windows.tobytes() == want.tobytes()
    for mine, theirs in zip((got.audio_frames, got.t0, got.is_last, got.global_offset, got.emit_after), five_of(want)):
        assert mine.tolist() == theirs.tolist()
    # the device entry addresses the caller's array from audio_offsets[0]: a lead of one sample shifts every even offset to an odd one
    lead = 1
    dev = torch.from_numpy(np.concatenate([np.full(lead, POISON).view(np.float32), cases["flat"], np.full(5, POISON).view(np.float32)])).cuda()
    got_dev = fa.tdt_plan_windows_dev(dev, cases["offsets"] + lead, config=cfg, ctx=gpu_ctx)
    assert got_dev.windows.tobytes() == want.tobytes() and got_dev.window_range.tolist() == case["window_range"].tolist()
    assert got_dev.speech_end.tolist() == case["speech_end"].tolist() and not got_dev.statuses.any()
    for mine, theirs in zip((got_dev.audio_frames, got_dev.t0, got_dev.is_last, got_dev.global_offset, got_dev.emit_after), five_of(want)):
        assert mine.cpu().numpy().tolist() == theirs.tolist()


def raw_plan(fa, ctx, cfg, flat, offsets, capacity, five):
    """fa_tdt_plan_windows_dev as it is, status included; five: int32 torch tensors on the device."""
    B = offsets.size - 1
    windows, window_range = np.zeros(max(capacity, 1), fa.TDT_WINDOW_DTYPE), np.full(B + 1, -7, np.int64)
    speech_end, statuses = np.zeros(B, np.int64), np.full(B, -7, np.int32)
    st = fa.lib().fa_tdt_plan_windows_dev(ctx.handle, C.byref(cfg), flat.data_ptr(), offsets.ctypes.data, B, windows.ctypes.data, capacity, window_range.ctypes.data,
                                          *[t.data_ptr() for t in five], speech_end.ctypes.data, statuses.ctypes.data)
    return st, windows, window_range, speech_end, statuses


def test_refused_recordings_and_a_capacity_one_short(fa, gpu_ctx, cases):
    import torch
    picks = [19, 22, 58]                                                         # two draws and a flat signal with a silent boundary
    good = [cases["audio"][i] for i in picks]
    with_nan, huge = good[0].copy(), good[1].copy()
    with_nan[300000] = np.nan
    huge[250000] = 3e19                                                          # its square is not finite
    audio = [good[0], with_nan, good[1], huge, good[2]]
    offsets = np.concatenate([[0], np.cumsum([x.size for x in audio])]).astype(np.int64)
    flat = torch.from_numpy(np.concatenate(audio)).cuda()
    for mode in ("default", "path_b"):
        cfg, want, ranges = config_of(fa, mode), cases[mode]["want"], cases[mode]["window_range"]
        assert R.Planner(with_nan, R.Config(**R.MODES[mode])).refused() and R.Planner(huge, R.Config(**R.MODES[mode])).refused()
        assert not R.Planner(good[0], R.Config(**R.MODES[mode])).refused()
        neighbours = [want[ranges[i]:ranges[i + 1]].copy() for i in picks]
        for b, rec in zip((0, 2, 4), neighbours):
            rec["recording"] = b
        expect = np.concatenate(neighbours)
        total = len(expect)
        five = [torch.full((total,), -7, dtype=torch.int32, device="cuda") for _ in range(5)]
        st, windows, window_range, _, statuses = raw_plan(fa, gpu_ctx, cfg, flat, offsets, total, five)
        torch.cuda.synchronize()
        assert st == 0 and statuses.tolist() == [0, INVALID_ARGUMENT, 0, INVALID_ARGUMENT, 0]
        assert window_range.tolist() == np.concatenate([[0], np.cumsum([len(neighbours[0]), 0, len(neighbours[1]), 0, len(neighbours[2])])]).tolist()
        assert windows[:total].tobytes() == expect.tobytes()                     # the neighbours' plans are unchanged
        assert five[0].cpu().numpy().tolist() == expect["actual_audio_frames"].tolist()
        # one slot short: the ranges are written, nothing is planned
        five = [torch.full((total,), -7, dtype=torch.int32, device="cuda") for _ in range(5)]
        st, windows, window_range2, _, statuses = raw_plan(fa, gpu_ctx, cfg, flat, offsets, total - 1, five)
        torch.cuda.synchronize()
        assert st == OUTPUT_TOO_SMALL and window_range2.tolist() == window_range.tolist() and statuses.tolist() == [0, INVALID_ARGUMENT, 0, INVALID_ARGUMENT, 0]
        assert not windows.view(np.uint8).any() and all((t == -7).all().item() for t in five)


def test_rows_and_lengths_bit_for_bit(fa, gpu_ctx, cases):
    import torch
    keep = list(range(len(K.SPECIAL_LENGTHS))) + [19, 22, 31]                    # every special length and three draws
    for mode in ("default", "path_b"):
        want, cfg = cases[mode]["want"], config_of(fa, mode)
        windows = want[np.isin(want["recording"], keep)]
        chunk, _, context, _ = R.chunk_layout(R.Config(**R.MODES[mode]))
        assert (windows["length"] == chunk + context).any() and (windows["actual_audio_frames"] == 1).any() and (windows["length"] == 1).any()
        rows = np.zeros((len(windows), 240000), np.uint32)
        for i, w in enumerate(windows):
            x = cases["audio"][w["recording"]].view(np.uint32)
            rows[i, :w["length"]] = x[w["context_start"]:w["context_start"] + w["length"]]
        got_rows, got_lengths = fa.tdt_pack_windows(cases["flat"], windows, cases["offsets"], config=cfg, ctx=gpu_ctx)
        assert got_lengths.tolist() == windows["length"].tolist() and got_rows.view(np.uint32).tobytes() == rows.tobytes()
        lead = 3                                                                 # sources at odd offsets, poison around the samples
        dev = torch.from_numpy(np.concatenate([np.full(lead, POISON).view(np.float32), cases["flat"], np.full(9, POISON).view(np.float32)])).cuda()
        d_rows, d_lengths = fa.tdt_pack_windows_dev(dev, cases["offsets"] + lead, windows, config=cfg, ctx=gpu_ctx)
        torch.cuda.synchronize()
        assert d_lengths.cpu().numpy().tolist() == windows["length"].tolist()
        assert d_rows.cpu().numpy().view(np.uint32).tobytes() == rows.tobytes()


@pytest.mark.parametrize("row", (10400, 10402))
def test_rows_across_launch_groups(fa, gpu_ctx, row):
    """64, 65 and 129 windows (a launch carries 64) into rows of two slices and a part, with 16-byte stores (10400) and without (10402);
    lengths 0, 1, row - 1 and row from odd source offsets; the samples are arbitrary bit patterns, NaNs with payloads among them."""
    import torch
    cfg = fa.tdt_window_config(maxModelSamples=row)
    rng = np.random.default_rng(row)
    bits = rng.integers(0, 1 << 32, row + 300, dtype=np.uint64).astype(np.uint32)
    bits[:3] = (0x7FC00001, 0xFF800001, 0x7F800000)                              # a quiet NaN with a payload, a signalling one, +inf
    lead = 3
    dev = torch.from_numpy(np.concatenate([np.full(lead, POISON), bits, np.full(5, POISON)]).view(np.float32)).cuda()
    offsets = np.array([lead, lead + bits.size], np.int64)
    for count in (64, 65, 129):
        windows = np.zeros(count, fa.TDT_WINDOW_DTYPE)
        windows["context_start"] = rng.integers(0, 300, count)
        windows["context_start"][:4] = (0, 1, 2, 3)
        windows["length"] = np.resize(np.array([0, 1, row - 1, row]), count)
        windows["length"][-1] = row                                              # the last row of the last group is a full one
        want = np.zeros((count, row), np.uint32)
        for i, w in enumerate(windows):
            want[i, :w["length"]] = bits[w["context_start"]:w["context_start"] + w["length"]]
        rows, lengths = fa.tdt_pack_windows_dev(dev, offsets, windows, config=cfg, ctx=gpu_ctx)
        torch.cuda.synchronize()
        assert lengths.cpu().numpy().tolist() == windows["length"].tolist()
        assert rows.shape == (count, row) and rows.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()


def tone(n, amplitude, lo=0, hi=None):
    x = np.zeros(n, np.float32)
    i = np.arange(lo, n if hi is None else hi)
    x[i] = np.float32(amplitude) * np.sin(i.astype(np.float32) * np.float32(0.1)).astype(np.float32)
    return x


def test_the_speech_gate(fa, gpu_ctx, cases):
    import torch
    audio = [tone(4 * RATE + 77, 0.004), tone(4 * RATE, 0.1), np.zeros(2 * RATE + 5, np.float32), tone(4 * RATE + 1279, 0.004, 0, 2 * RATE), np.zeros(0, np.float32),
             np.zeros(F - 1, np.float32) + np.float32(0.01), tone(5 * RATE, 0.1, 0, 3 * RATE) + tone(5 * RATE, 0.004, 3 * RATE)] + [cases["audio"][i] for i in (19, 21, 22, 25)]
    planners = [R.Planner(x) for x in audio]
    want_thresholds = np.array([p.adaptive_speech_rms_threshold() for p in planners], np.float32)
    assert want_thresholds[2] == R.SPEECH_RMS_CEILING and want_thresholds[4] == R.SPEECH_RMS_CEILING and R.SPEECH_RMS_FLOOR < want_thresholds[0] < R.SPEECH_RMS_CEILING
    spans = []
    for b, x in enumerate(audio):
        n = x.size
        spans += [(b, 0, 0, n), (b, 0, min(137, n), n), (b, 0, 0, min(n, F - 1)), (b, 0, min(n, 1000), n), (b, 0, min(n, 3 * F + 1), min(n, 4 * F + 1)), (b, 0, n, n),
                  (b, 0, min(n, 5), max(0, n - 3))]
    spans = np.array(spans, fa.TDT_SPAN_DTYPE)
    override = np.array([0.001, 0.05, 0.0, 0.002, 0.1, 0.0099, 0.004, 0.01, 0.0005, 0.02, 0.1], np.float32)
    seconds_per_frame = float(F) / float(RATE)
    for over in (None, override):
        thr = want_thresholds if over is None else over
        want_frames = np.array([planners[s["recording"]].speech_like_frames(int(s["from_sample"]), int(s["to_sample"]), thr[s["recording"]]) for s in spans], np.int64)
        want_seconds = np.array([float(f) * seconds_per_frame for f in want_frames], np.float64)
        assert over is not None or (want_frames > 0).sum() > 10
        thresholds, frames, seconds, statuses = fa.tdt_speech_gate(audio, spans, override_thresholds=over, ctx=gpu_ctx)
        assert thresholds.tobytes() == want_thresholds.tobytes() and not statuses.any()
        assert frames.tolist() == want_frames.tolist() and seconds.tobytes() == want_seconds.tobytes()
    offsets = np.concatenate([[0], np.cumsum([x.size for x in audio])]).astype(np.int64)
    dev = torch.from_numpy(np.concatenate([np.full(1, POISON).view(np.float32)] + audio + [np.full(3, POISON).view(np.float32)])).cuda()
    thresholds, frames, seconds, statuses = fa.tdt_speech_gate_dev(dev, offsets + 1, spans, override_thresholds=override, ctx=gpu_ctx)
    assert thresholds.tobytes() == want_thresholds.tobytes() and frames.tolist() == want_frames.tolist() and seconds.tobytes() == want_seconds.tobytes()
    # a refused recording: its threshold is NaN, its spans count nothing, its neighbours are untouched
    bad = audio[1].copy()
    bad[777] = np.inf
    thresholds, frames, _, statuses = fa.tdt_speech_gate([audio[0], bad, audio[3]], np.array([(0, 0, 0, audio[0].size), (1, 0, 0, bad.size), (2, 0, 0, audio[3].size)],
                                                                                             fa.TDT_SPAN_DTYPE), ctx=gpu_ctx)
    assert statuses.tolist() == [0, INVALID_ARGUMENT, 0] and np.isnan(thresholds[1]) and thresholds[[0, 2]].tobytes() == want_thresholds[[0, 3]].tobytes()
    assert frames.tolist() == [planners[0].speech_like_frames(0, audio[0].size, want_thresholds[0]), 0, planners[3].speech_like_frames(0, audio[3].size, want_thresholds[3])]


def walk_and_merge(fa, ctx, tables, five, window_range, max_out=64):
    """fa_tdt_greedy_tables_dev on the five per-window arrays (device tensors), then fa_tdt_merge_windows_dev on what it left."""
    import torch
    tok, dur, prob = tables
    W, U, T = tok.shape
    enc = torch.full((W,), T, dtype=torch.int32, device="cuda")
    o_tok, o_time, o_dur = (torch.zeros((W, max_out), dtype=torch.int32, device="cuda") for _ in range(3))
    o_conf = torch.zeros((W, max_out), dtype=torch.float32, device="cuda")
    o_cnt, o_ft, o_fu, o_st = (torch.zeros(W, dtype=torch.int32, device="cuda") for _ in range(4))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    cfg = fa.TdtConfig().c()
    with ctx.torch_ordered():
        ctx.check(fa.lib().fa_tdt_greedy_tables_dev(ctx.handle, C.byref(cfg), p(tok), p(dur), p(prob), W, U, T, p(enc), *[p(t) for t in five], max_out, p(o_tok), p(o_time), p(o_dur),
                                                    p(o_conf), p(o_cnt), p(o_ft), p(o_fu), p(o_st)), "fa_tdt_greedy_tables_dev")
    merged = fa.merge_windows_dev(o_tok, o_time, o_dur, o_conf, o_cnt, window_range, ctx=ctx)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (o_tok, o_time, o_dur, o_conf, o_cnt, o_st, merged.tokens, merged.timestamps, merged.durations, merged.confidences)] + \
        [merged.counts, merged.statuses]


def test_the_plan_feeds_the_walk_and_the_merge(fa, gpu_ctx, cases):
    """The plan's five device arrays and window_range go straight into the greedy walk and the merge; the result equals the same two
    calls fed from the restatement's host arrays."""
    import torch
    picks = [19, 20, 58, 63]                                                     # two draws, a silent boundary, the end-of-audio probe
    audio = [cases["audio"][i] for i in picks]
    offsets = np.concatenate([[0], np.cumsum([x.size for x in audio])]).astype(np.int64)
    want = np.concatenate([cases["path_b"]["want"][cases["path_b"]["window_range"][i]:cases["path_b"]["window_range"][i + 1]] for i in picks])
    plan = fa.tdt_plan_windows_dev(torch.from_numpy(np.concatenate(audio)).cuda(), offsets, config=config_of(fa, "path_b"), ctx=gpu_ctx)
    W = len(want)
    assert W == len(plan.windows) >= 8 and (want["emit_after_frame"] >= 0).any()
    rng = np.random.default_rng(5)
    U, T = 48, 190
    tok = np.where(rng.random((W, U, T)) < 0.8, 8192, rng.integers(0, 40, (W, U, T))).astype(np.int32)
    tables = [torch.from_numpy(a).cuda() for a in (tok, rng.integers(0, 5, (W, U, T)).astype(np.int32), rng.uniform(0.2, 1.0, (W, U, T)).astype(np.float32))]
    got = walk_and_merge(fa, gpu_ctx, tables, [plan.audio_frames, plan.t0, plan.is_last, plan.global_offset, plan.emit_after], plan.window_range)
    ranges = cases["path_b"]["window_range"]
    want_range = np.concatenate([[0], np.cumsum([ranges[i + 1] - ranges[i] for i in picks])]).astype(np.int64)
    assert plan.window_range.tolist() == want_range.tolist()
    ref = walk_and_merge(fa, gpu_ctx, tables, [torch.from_numpy(a).cuda() for a in five_of(want)], want_range)
    assert got[4].sum() > 50 and not got[5].any()                                # the walks emitted tokens and ran out of nothing
    for mine, theirs in zip(got, ref):
        assert mine.tobytes() == theirs.tobytes()
