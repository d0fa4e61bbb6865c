"""csrc/sortformer.hip, csrc/sortformer_host.hip, csrc/timeline.hip and csrc/timeline_host.hip on the device against tests/sortformer_restatement.py, bit for bit: np.array_equal on the fp32 arrays viewed as
uint32 and on every integer field.  There are no tolerances here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sortformer_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def fa_cfg(fa, cfg):
    return fa.OfflineSortformerConfig(cfg.window_output_frames, cfg.subsampling, cfg.speakers, cfg.n_mels, cfg.overlap_output_frames)


# ---------------------------------------------------------------- pack

PACK_CASES = [
    # default geometry: shorter than a window, the extra tail window (exactly 3 072 frames), 40 windows
    (R.OfflineConfig(), [1500, 3072, 39 * 2272 + 1000]),
    # windowMel 48 (16-byte stores) with hopMel 30: melStart * 4 B is not 16-byte aligned
    (R.OfflineConfig(24, 2, 4, 16, 9), [47, 48, 500, 0, 131]),
    # windowMel 75: no 16-byte path at all; 80 mels: a partial tile of the transpose
    (R.OfflineConfig(25, 3, 4, 80, 8), [75, 400, 1]),
]


@pytest.mark.parametrize("layout", ["mel_major", "frame_major"])
@pytest.mark.parametrize("case", range(len(PACK_CASES)))
def test_pack_windows(fa, gpu_ctx, case, layout):
    import torch
    cfg, lengths = PACK_CASES[case]
    rng = np.random.default_rng(10 + case)
    t_max = max(lengths) + 3
    mels = [rng.standard_normal((n, cfg.n_mels)).astype(np.float32) for n in lengths]           # time-major per recording
    host = np.full((len(lengths), t_max, cfg.n_mels), 99.0, np.float32)                         # 99: past a recording's end, never packed
    for b, m in enumerate(mels):
        host[b, :m.shape[0]] = m
    d_mel = torch.from_numpy(host if layout == "frame_major" else np.ascontiguousarray(host.transpose(0, 2, 1))).cuda()
    d_win, d_len = fa.pack_windows(d_mel, lengths, layout, fa_cfg(fa, cfg), gpu_ctx)
    want, want_len = [], []
    for b, n in enumerate(lengths):
        for w in R.offline_windows(cfg, n)[0]:
            x, ml = R.pack_window(cfg, mels[b], w)
            want.append(x)
            want_len.append(ml)
    got = d_win.cpu().numpy()
    assert got.shape == (len(want), cfg.n_mels, cfg.window_mel_frames)
    assert np.array_equal(bits(got), bits(np.stack(want)))
    assert d_len.cpu().numpy().tolist() == want_len
    assert (got[np.array(want_len) < cfg.window_mel_frames][:, :, -1] == 0).all()               # tail zeros of the short windows


def test_pack_statuses(fa, gpu_ctx):
    import torch
    cfg = fa.OfflineSortformerConfig().c_config()
    n = np.array([5000], np.int64)
    d_mel = torch.zeros((1, 128, 5000), device="cuda")
    d_out = torch.zeros((2, 128, 3072), device="cuda")
    d_len = torch.zeros(2, dtype=torch.int32, device="cuda")
    f = fa.lib().fa_sortformer_pack_windows_dev
    args = (d_mel.data_ptr(), 0, 128 * 5000, 5000, n.ctypes.data, 1)
    assert f(gpu_ctx.handle, C.byref(cfg), *args, 3, d_out.data_ptr(), d_len.data_ptr()) == fa.INVALID_ARGUMENT       # 2 windows, not 3
    assert f(gpu_ctx.handle, C.byref(cfg), d_mel.data_ptr(), 0, 128 * 5000, 4999, n.ctypes.data, 1, 2, d_out.data_ptr(),
             d_len.data_ptr()) == fa.INVALID_ARGUMENT                                                                # longer than its rows
    assert f(gpu_ctx.handle, C.byref(cfg), *args, 2, None, d_len.data_ptr()) == fa.INVALID_ARGUMENT
    assert f(gpu_ctx.handle, C.byref(cfg), *args, 2, d_out.data_ptr(), d_len.data_ptr()) == fa.SUCCESS


# ---------------------------------------------------------------- stitch

def synthetic_activity(rng, frames, speakers):
    """Random on / off runs per speaker, sigmoid-like values: 0.7 to 1 while speaking, below 0.3 otherwise, some exact zeros."""
    act = np.zeros((frames, speakers), np.float32)
    for s in range(speakers):
        t, on = 0, bool(rng.integers(2))
        while t < frames:
            n = int(rng.integers(20, 400))
            act[t:t + n, s] = (0.7 + 0.29 * rng.random(min(n, frames - t))) if on else (0.3 * rng.random(min(n, frames - t)))
            t, on = t + n, not on
    act[rng.random(act.shape) < 0.05] = 0
    return act


def synthetic_preds(rng, cfg, n_mel, permute=True):
    """The model's outputs for one recording: each window sees the recording's activity plus noise under a fresh column permutation.
    Returns (preds [W, window, S], injected [W, S] with window column injected[w][g] holding global speaker g)."""
    wins, total = R.offline_windows(cfg, n_mel)
    act = synthetic_activity(rng, total + cfg.window_output_frames, cfg.speakers)
    preds = np.zeros((len(wins), cfg.window_output_frames, cfg.speakers), np.float32)
    injected = np.zeros((len(wins), cfg.speakers), np.int64)
    for i, w in enumerate(wins):
        x = act[w["g_start"]:w["g_start"] + cfg.window_output_frames].copy()
        x = np.clip(x + 0.005 * rng.standard_normal(x.shape).astype(np.float32) * (x != 0), 0, 1).astype(np.float32)
        p = rng.permutation(cfg.speakers) if permute and i > 0 else np.arange(cfg.speakers)
        preds[i][:, p] = x
        injected[i] = p
    return preds, injected


def run_stitch(fa, gpu_ctx, cfg, lengths, preds_list):
    import torch
    d_preds = torch.from_numpy(np.concatenate(preds_list)).cuda()
    d_global, d_map = fa.stitch(d_preds, lengths, fa_cfg(fa, cfg), gpu_ctx)
    want_g, want_m = zip(*(R.stitch(cfg, n, p) for n, p in zip(lengths, preds_list)))
    got_g, got_m = d_global.cpu().numpy(), d_map.cpu().numpy()
    assert np.array_equal(got_m, np.concatenate(want_m)), "mappings"
    assert np.array_equal(bits(got_g), bits(np.concatenate(want_g))), "global timeline"
    return got_g, got_m


def test_stitch_default_geometry_recovers_permutations(fa, gpu_ctx):
    rng = np.random.default_rng(20)
    cfg = R.OfflineConfig()
    lengths = [12 * 2272 + 700, 3072, 2000, 25 * 2272 + 3071]     # also: the extra tail window, a recording of one window
    preds, inj = zip(*(synthetic_preds(rng, cfg, n) for n in lengths))
    _, got_m = run_stitch(fa, gpu_ctx, cfg, lengths, list(preds))
    # the recovered mappings undo the injected permutations: window column injected[w][g] maps to global g
    inj = np.concatenate(inj)
    assert np.array_equal(np.take_along_axis(got_m, inj.astype(np.int64), axis=1), np.tile(np.arange(4), (inj.shape[0], 1)))
    assert len({tuple(m) for m in got_m.tolist()}) > 10


def test_stitch_exact_ties(fa, gpu_ctx):
    rng = np.random.default_rng(21)
    cfg = R.OfflineConfig()
    n = 6 * 2272 + 1500
    preds, _ = synthetic_preds(rng, cfg, n)
    preds[2, :100] = 0                   # window 2's side of its overlap all zero: every score 0, the first enumerated wins
    preds[2, 284:] = 0                   # and window 3 sees an all-zero global overlap (every term skipped)
    preds[4][:, 3] = preds[4][:, 1]      # two identical columns: pairs of bijections tie exactly
    preds[5][:, 0] = preds[5][:, 2]
    run_stitch(fa, gpu_ctx, cfg, [n], [preds])


def test_stitch_nan_and_inf_rows(fa, gpu_ctx):
    rng = np.random.default_rng(22)
    cfg = R.OfflineConfig()
    n = 8 * 2272 + 900
    preds, _ = synthetic_preds(rng, cfg, n)
    preds[1, 10] = np.nan                # in window 1's overlap with window 0
    preds[2, 50, 1] = np.inf
    preds[3, 7, 2] = -np.inf
    preds[3, 300, 0] = np.nan            # in the part window 4 correlates against
    preds[5, 290:384] = np.inf           # a previous side that is +inf
    preds[6, :100] = np.nan              # every score NaN: the identity stays
    preds[7, 20, :] = [np.inf, -np.inf, np.nan, 0.0]
    run_stitch(fa, gpu_ctx, cfg, [n], [preds])


@pytest.mark.parametrize("speakers", [1, 2, 3])
def test_stitch_fewer_speakers(fa, gpu_ctx, speakers):
    rng = np.random.default_rng(23 + speakers)
    cfg = R.OfflineConfig(speakers=speakers)
    lengths = [5 * 2272 + 100, 2 * 2272 + 2000]
    preds = [synthetic_preds(rng, cfg, n)[0] for n in lengths]
    run_stitch(fa, gpu_ctx, cfg, lengths, preds)


def test_stitch_no_overlap_and_speaker_limit(fa, gpu_ctx):
    import torch
    rng = np.random.default_rng(27)
    cfg = R.OfflineConfig(overlap_output_frames=0)
    lengths = [3 * 3072 + 5, 3072]
    preds = [synthetic_preds(rng, cfg, n)[0] for n in lengths]
    _, m = run_stitch(fa, gpu_ctx, cfg, lengths, preds)
    assert (m == np.arange(4)).all()
    c = fa.OfflineSortformerConfig(num_speakers=5).c_config()
    n = np.array([100], np.int64)
    d = torch.zeros(384 * 5, device="cuda")
    di = torch.zeros(5, dtype=torch.int32, device="cuda")
    assert fa.lib().fa_sortformer_stitch_dev(gpu_ctx.handle, C.byref(c), d.data_ptr(), n.ctypes.data, 1, 1, d.data_ptr(),
                                             di.data_ptr()) == fa.INVALID_ARGUMENT


def test_stitch_general_geometry(fa, gpu_ctx):
    """overlap 300 of 384: a frame is averaged by up to five windows and the overlap region is no copy of the previous window."""
    rng = np.random.default_rng(28)
    cfg = R.OfflineConfig(overlap_output_frames=300)
    lengths = [14 * 84 * 8 + 3072 + 77, 3072, 900]
    preds = [synthetic_preds(rng, cfg, n)[0] for n in lengths]
    preds[0][5, 3] = np.nan
    run_stitch(fa, gpu_ctx, cfg, lengths, preds)
    small = R.OfflineConfig(10, 2, 3, 8, 7)                       # 2 * 7 > 10
    lengths = [20 * 3 * 2 + 9, 41]
    run_stitch(fa, gpu_ctx, small, lengths, [synthetic_preds(rng, small, n)[0] for n in lengths])


@pytest.mark.parametrize("overlap", [5, 6])
def test_stitch_route_boundary(fa, gpu_ctx, overlap):
    """window 10: 2 * 5 = 10 is the last geometry of the parallel route (stitch_corr, stitch_chain, stitch_merge), 2 * 6 > 10 the first of
    the serial one (stitch_serial).  Recordings of many windows, of a short tail window, and of exactly one window's mel frames."""
    rng = np.random.default_rng(50 + overlap)
    cfg = R.OfflineConfig(10, 2, 4, 8, overlap)
    lengths = [207, 41, 20]
    run_stitch(fa, gpu_ctx, cfg, lengths, [synthetic_preds(rng, cfg, n)[0] for n in lengths])


@pytest.mark.parametrize("overlap", [64, 65])
def test_stitch_overlap_staging_boundary(fa, gpu_ctx, overlap):
    """stitch_corr stages 64 overlap frames per pass through LDS: 64 frames are one full pass, 65 a second pass of one frame (2 * 65 = 130:
    still the parallel route).  A NaN sits in the last overlap frame on either side — with 65 frames the one frame of the second pass:
    window 1's own frame overlap - 1, and window 2's last frame, which window 3 correlates against."""
    rng = np.random.default_rng(60 + overlap)
    cfg = R.OfflineConfig(130, 1, 4, 8, overlap)
    lengths = [370, 131, 130]
    preds = [synthetic_preds(rng, cfg, n)[0] for n in lengths]
    assert preds[0].shape[0] >= 4
    preds[0][1, overlap - 1, 2] = np.nan
    preds[0][2, 129, 1] = np.nan
    run_stitch(fa, gpu_ctx, cfg, lengths, preds)


def test_stitch_statuses(fa, gpu_ctx):
    import torch
    cfg = fa.OfflineSortformerConfig().c_config()
    n = np.array([5000], np.int64)                                # 2 windows, 625 frames of the global timeline
    d_preds = torch.zeros((2, 384, 4), device="cuda")
    d_global = torch.zeros((625, 4), device="cuda")
    d_map = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    f = fa.lib().fa_sortformer_stitch_dev
    args = (gpu_ctx.handle, C.byref(cfg), d_preds.data_ptr(), n.ctypes.data, 1)
    assert f(*args, 3, d_global.data_ptr(), d_map.data_ptr()) == fa.INVALID_ARGUMENT                                  # 2 windows, not 3
    assert gpu_ctx.last_error().startswith("sortformer stitch:")
    assert f(*args, 2, None, d_map.data_ptr()) == fa.INVALID_ARGUMENT
    assert f(*args, 2, d_global.data_ptr(), d_map.data_ptr()) == fa.SUCCESS


# ---------------------------------------------------------------- timeline

def random_walk(rng, frames, speakers, step=0.04):
    x = np.cumsum(rng.normal(0, step, (frames, speakers)), axis=0) + rng.random(speakers)
    return np.abs(((x + 1) % 2) - 1).astype(np.float32)          # folded into [0, 1]


PADDED = dict(onset_threshold=0.6, offset_threshold=0.45, onset_pad_frames=2, offset_pad_frames=3, min_frames_on=4, min_frames_off=5)


def configs(fa, speakers, **kw):
    return R.TimelineConfig(num_speakers=speakers, **kw), fa.DiarizerTimelineConfig(num_speakers=speakers, **kw)


def record_rows(recs):
    return [(int(r["recording"]), int(r["speaker"]), int(r["start_frame"]), int(r["end_frame"]), int(r["activity"].view(np.uint32)),
             int(r["finalized"])) for r in recs]


def check_timeline(fa, gpu_ctx, rcfg, cfg, fins, tents, complete):
    import torch
    s = rcfg.num_speakers
    d_fin = torch.from_numpy(np.concatenate(fins).reshape(-1, s)).cuda()
    d_tent = None if tents is None else torch.from_numpy(np.concatenate(tents).reshape(-1, s)).cuda()
    recs, per = fa.timeline_segments(d_fin, [len(f) for f in fins], d_tent, None if tents is None else [len(t) for t in tents], cfg, complete, gpu_ctx)
    want = R.timeline_records(rcfg, fins, tents, complete)
    assert record_rows(recs) == want
    assert per.tolist() == [sum(1 for w in want if w[0] == b) for b in range(len(fins))]
    return want


def special_speakers(p):
    """Column 0 all silent, column 1 all speaking, the last column still speaking at the end, NaN frames sprinkled elsewhere."""
    p[:, 0] = 0.0
    if p.shape[1] > 1:
        p[:, 1] = 0.97
    if p.shape[1] > 2:
        p[-50:, -1] = 0.9
        p[::997, 2] = np.nan
    return p


def test_timeline_large_default_config(fa, gpu_ctx):
    rng = np.random.default_rng(30)
    rcfg, cfg = configs(fa, 4)
    fins = [random_walk(rng, n, 4) for n in (100000, 131072, 100001, 120000)]
    special_speakers(fins[1])
    want = check_timeline(fa, gpu_ctx, rcfg, cfg, fins, None, True)
    assert len(want) > 2000 and {w[5] for w in want} == {3, 2}     # finalized ones, and trailing tentative ones finalize() moved


def test_timeline_large_padded_config_with_tentative(fa, gpu_ctx):
    rng = np.random.default_rng(31)
    rcfg, cfg = configs(fa, 4, **PADDED)
    full = [random_walk(rng, n, 4) for n in (100000, 110000, 100003, 102047)]
    special_speakers(full[2])
    fins = [f[:-10000] for f in full]
    tents = [f[-10000:] for f in full]
    want = check_timeline(fa, gpu_ctx, rcfg, cfg, fins, tents, False)
    assert len(want) > 1000 and {w[5] for w in want} == {3, 0}


@pytest.mark.parametrize("complete", [True, False])
@pytest.mark.parametrize("tentative", [True, False])
@pytest.mark.parametrize("padded", [True, False])
def test_timeline_combinations(fa, gpu_ctx, padded, tentative, complete):
    rng = np.random.default_rng(32)
    rcfg, cfg = configs(fa, 4, **(PADDED if padded else {}))
    full = [special_speakers(random_walk(rng, n, 4, 0.08)) for n in (5000, 1, 2048, 2049, 7)] + [np.zeros((0, 4), np.float32)]
    fins = [f[:len(f) - len(f) // 5] for f in full] if tentative else full
    tents = [f[len(f) - len(f) // 5:] for f in full] if tentative else None
    check_timeline(fa, gpu_ctx, rcfg, cfg, fins, tents, complete)
    if tentative:                                                 # a recording whose frames are all tentative
        check_timeline(fa, gpu_ctx, rcfg, cfg, [np.zeros((0, 4), np.float32), full[0][:100]], [full[0], full[2]], complete)


@pytest.mark.parametrize("speakers", [1, 7])
def test_timeline_speaker_counts(fa, gpu_ctx, speakers):
    rng = np.random.default_rng(33 + speakers)
    rcfg, cfg = configs(fa, speakers, **PADDED)
    full = [random_walk(rng, n, speakers, 0.07) for n in (6000, 4097)]
    if speakers > 1:
        special_speakers(full[0])
    check_timeline(fa, gpu_ctx, rcfg, cfg, [f[:-500] for f in full], [f[-500:] for f in full], True)


def test_timeline_host_twin_and_negative_start(fa, gpu_ctx):
    rcfg, cfg = configs(fa, 1, onset_pad_frames=3)
    # the second run starts at 7 - 3 = 4 > 2, a gap the padding does not bridge: two segments, (-3, 2) finalized and the trailing (4, 8)
    p = np.array([0.9, 0.9, 0.0, 0.0, 0.0, 0.0, 0.0, 0.8], np.float32).reshape(-1, 1)
    recs, _ = fa.timeline_segments(p, None, None, None, cfg, True, gpu_ctx)             # numpy input: the host-pointer entry
    assert record_rows(recs) == R.timeline_records(rcfg, [p], None, True)
    assert [r[2:4] + r[5:] for r in record_rows(recs)] == [(-3, 2, 3), (4, 8, 2)]      # frame - padOnset < 0 is kept
    with pytest.raises(fa.FluidAudioHipError):
        fa.timeline_segments(p, None, None, None, fa.DiarizerTimelineConfig(activity_type="logits"), True, gpu_ctx)


def test_timeline_count_then_fill(fa, gpu_ctx):
    import torch
    rng = np.random.default_rng(35)
    rcfg, cfg = configs(fa, 4)
    fin = random_walk(rng, 20000, 4, 0.08)
    want = R.timeline_records(rcfg, [fin], None, True)
    total, cap = len(want), len(want) // 3
    assert cap > 10
    d_fin = torch.from_numpy(fin).cuda()
    frames = np.array([fin.shape[0]], np.int64)
    out = np.zeros(total, fa.sortformer.SEGMENT_DTYPE)
    out["recording"] = -77                                        # sentinel
    cnt = C.c_int64()
    c = cfg.c_config()
    f = fa.lib().fa_timeline_segments_dev
    st = f(gpu_ctx.handle, C.byref(c), d_fin.data_ptr(), frames.ctypes.data, None, None, 1, 1, out.ctypes.data, cap, C.byref(cnt), None)
    assert st == 3 and cnt.value == total                         # OUTPUT_TOO_SMALL with the count
    assert record_rows(out[:cap]) == want[:cap]
    assert (out["recording"][cap:] == -77).all() and not out["end_frame"][cap:].any()   # nothing past the capacity
    st = f(gpu_ctx.handle, C.byref(c), d_fin.data_ptr(), frames.ctypes.data, None, None, 1, 1, None, 0, C.byref(cnt), None)
    assert st == 0 and cnt.value == total


# ---------------------------------------------------------------- end to end

def stand_in_model(windows, mel_length):
    """A fixed function of the packed windows made of operations that are exact on any device: the maximum over each of four mel bands and
    each group of eight frames, an affine map by powers of two, a clamp, and a per-window roll of the speaker columns."""
    import torch
    w, m, t = windows.shape
    x = windows.reshape(w, 4, m // 4, t // 8, 8).amax(dim=(2, 4))                      # [W, 4, T / 8]
    p = ((x + 10.0) * 0.0625).clamp(0.0, 1.0).transpose(1, 2).contiguous()              # [W, T / 8, 4]
    idx = (torch.arange(4, device=windows.device)[None, :] + torch.arange(w, device=windows.device)[:, None]) % 4
    return torch.gather(p, 2, idx[:, None, :].expand(w, t // 8, 4)).contiguous()


def test_process_complete_end_to_end(fa, gpu_ctx):
    rng = np.random.default_rng(40)

    def speech(n):
        env = np.repeat(rng.random(n // 8000 + 1) < 0.5, 8000)[:n] * 0.5 + 0.001
        return (rng.standard_normal(n) * env).astype(np.float32)

    audios = [speech(20 * 16000), speech(3071 * 160), speech(80 * 16000 + 123)]       # < one window; 3 072 mel frames: the extra window; 4 windows
    dia = fa.OfflineSortformerDiarizer(gpu_ctx)
    segs = dia.process_complete(audios, stand_in_model)
    last = dia.last
    n_mel = last["n_mel_frames"].tolist()
    assert n_mel[1] == 3072 and n_mel[0] < 3072
    cfg = R.OfflineConfig()
    mel = last["mel"].cpu().numpy()                                                    # [B, 128, T] from the device
    want_win, want_len = [], []
    for b, n in enumerate(n_mel):
        for w in R.offline_windows(cfg, n)[0]:
            x, ml = R.pack_window(cfg, np.ascontiguousarray(mel[b, :, :n].T), w)
            want_win.append(x)
            want_len.append(ml)
    assert np.array_equal(bits(last["windows"].cpu().numpy()), bits(np.stack(want_win)))
    assert last["mel_length"].cpu().numpy().tolist() == want_len
    cpu_preds = stand_in_model(last["windows"].cpu(), None).numpy()                    # the stand-in on the CPU from the device's windows
    glob, maps, recs, ofs = [], [], [], 0
    rcfg = R.TimelineConfig(num_speakers=4, frame_duration_seconds=float(cfg.frame_duration_seconds))
    for b, n in enumerate(n_mel):
        nw = len(R.offline_windows(cfg, n)[0])
        g, m = R.stitch(cfg, n, cpu_preds[ofs:ofs + nw])
        ofs += nw
        glob.append(g)
        maps.append(m)
        t = R.Timeline(rcfg)
        t.rebuild(g, (), True)
        recs += t.records(b)
    assert np.array_equal(last["mapping"].cpu().numpy(), np.concatenate(maps))
    assert np.array_equal(bits(last["global_"].cpu().numpy()), bits(np.concatenate(glob)))
    assert record_rows(last["records"]) == recs and len(recs) > 10
    assert [len(s) for s in segs] == [sum(1 for r in recs if r[0] == b) for b in range(3)]
    one = fa.OfflineSortformerDiarizer(gpu_ctx).process_complete(audios[0], stand_in_model)
    assert [(s.speaker_index, s.start_frame, s.end_frame) for s in one] == [(s.speaker_index, s.start_frame, s.end_frame) for s in segs[0]]
    assert abs(float(one[0].end_time) - one[0].end_frame * 0.08) < 1e-4
