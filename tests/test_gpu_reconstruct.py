"""Speaker segments on the device (csrc/reconstruct.hip, driven by csrc/reconstruct_host.hip) equal the numpy restatement (tests/reconstruct_restatement.py) bit for bit:
every segment's start / end / quality as fp32 bits and its speaker id, the per-frame speaker counts and the segment count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import reconstruct_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(segs):
    """(id, start bits, end bits, quality bits) of restatement tuples or TimedSpeakerSegment objects."""
    out = []
    for s in segs:
        if isinstance(s, tuple):
            sid, a, b, q = s
        else:
            sid, a, b, q = s.speaker_id, s.start_time_seconds, s.end_time_seconds, s.quality_score
        out.append((sid,) + tuple(int(np.float32(v).view(np.uint32)) for v in (a, b, q)))
    return out


def rcfg(fa, **kw):
    return fa.ReconstructionConfig(**kw), R.config(**kw)


def check(fa, ctx, w, hard, K, offsets=None, fd=0.0, overrides=None, **kw):
    """device vs restatement on one input; returns the device segments."""
    dcfg, rc = rcfg(fa, **kw)
    cen = np.zeros((K, 4))
    want, st = R.build_segments(w, hard, cen, offsets, fd, rc, overrides=overrides, return_state=True)
    rec = fa.OfflineReconstruction(dcfg, ctx=ctx)
    seg = fa.SegmentationOutput(w, offsets, fd)
    got = rec._call(seg, hard, K, overrides, 0, True) if overrides else rec.build_segments(seg, hard, cen, frame_records=True)
    assert rec.last_info["total_frames"] == st["T"]
    check_frames(rec.last_info, st)
    assert rec.last_info["raw_segments"] == len(st["raw"])
    assert bits(got) == bits(want)
    return got, st


def f64bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_frames(info, st):
    """The per-frame decision in fp64, bit for bit: a different summation order (chunk, frame or speaker) moves these sums by an ulp
    long before it moves a Float segment field."""
    assert np.array_equal(info["speaker_counts"], st["speaker_count"])
    assert np.array_equal(f64bits(info["expected_count_sums"]), f64bits(st["expected_sums"]))
    cl, av = R.frame_records(st, st["final"])
    assert np.array_equal(info["frame_clusters"], cl)
    assert np.array_equal(f64bits(info["frame_averages"]), f64bits(av))


def random_case(rng, C=40, F=97, S=3, K=12, binary=False, p_active=0.5):
    if binary:
        w = (rng.random((C, F, S)) < p_active).astype(np.float32)
    else:
        w = rng.uniform(-0.3, 1.2, (C, F, S)).astype(np.float32)   # non-binary: negative, > 1, exact zeros
        w[rng.random((C, F, S)) < 0.2] = 0
    hard = rng.integers(-3, K + 3, (C, S)).astype(np.int32)       # -2 / -3 / >= K: not a cluster
    return w, hard


@pytest.mark.parametrize("K", [1, 12, 63, 64, 65, 200, 600])
def test_sorted_offsets_every_k(fa, gpu_ctx, K):
    rng = np.random.default_rng(K)
    w, hard = random_case(rng, K=K)
    fd = 10.0 / 97
    off = np.arange(40) * 2.0
    check(fa, gpu_ctx, w, hard, K, off, 0.0, min_segment_duration=0.0, min_gap_duration=0.05)
    check(fa, gpu_ctx, w, hard, K, off, fd)   # defaults: merge, 1 s minimum, exclusive


@pytest.mark.parametrize("kind", ["shuffled", "duplicated", "negative", "off_grid", "missing"])
def test_irregular_offsets(fa, gpu_ctx, kind):
    rng = np.random.default_rng(["shuffled", "duplicated", "negative", "off_grid", "missing"].index(kind) + 40)
    C, F = 50, 83
    w, hard = random_case(rng, C=C, F=F, K=9)
    off = np.arange(C) * 2.0
    if kind == "shuffled":
        off = rng.permutation(off)
    elif kind == "duplicated":
        off = np.repeat(off[:C // 5], 5)
        off[-7:] = off[3]
        off = rng.permutation(off)
    elif kind == "negative":
        off = off - 30.0 + rng.uniform(-1, 1, C)
    elif kind == "off_grid":
        off = np.sort(rng.uniform(0, 60, C))           # sorted but off the frame grid: rounding collisions and skips
    elif kind == "missing":
        off = off[:C // 3] * 1.37                       # the rest start at c * window_duration
    check(fa, gpu_ctx, w, hard, 9, off, 0.0, min_segment_duration=0.0, min_gap_duration=0.0)
    check(fa, gpu_ctx, w, hard, 9, off, 0.0, window_duration=7.5)


def test_many_chunks_on_one_tile(fa, gpu_ctx):
    """More chunks cover one tile of global frames than the LDS list holds: every wavefront scans all chunks."""
    rng = np.random.default_rng(5)
    w, hard = random_case(rng, C=1500, F=31, K=5)
    off = rng.uniform(0, 0.5, 1500)
    check(fa, gpu_ctx, w, hard, 5, off, 0.05, min_segment_duration=0.0)


def test_duplicate_embeddings_and_labels_out_of_range(fa, gpu_ctx):
    rng = np.random.default_rng(8)
    C, S, K = 30, 3, 6
    n = 400
    ci, si, lab = rng.integers(-1, C + 1, n), rng.integers(0, S + 1, n), rng.integers(-2, K + 2, n)
    hard = fa.chunk_assignments(ci, si, lab, K, C, S)
    assert np.array_equal(hard, R.chunk_assignments(ci, si, lab, K, C, S))
    w, _ = random_case(rng, C=C, F=64, S=S, K=K, binary=True)
    check(fa, gpu_ctx, w, hard, K, np.arange(C) * 2.0, 0.0, min_segment_duration=0.0)


def test_flicker_and_capacity_query(fa, gpu_ctx):
    rng = np.random.default_rng(13)
    nc, F, S, K = 20, 200, 3, 4
    w, _ = random_case(rng, C=nc, F=F, S=S, K=K, binary=True, p_active=0.5)
    hard = np.tile(np.arange(S, dtype=np.int32), (nc, 1))
    offs = np.arange(nc) * 10.0                          # windows that do not overlap: every frame decides alone
    got, st = check(fa, gpu_ctx, w, hard, K, offs, 0.05, min_segment_duration=0.0, min_gap_duration=0.0, exclusive=False)
    assert len(st["raw"]) > 1000
    L = fa._lib
    cfg = fa.ReconstructionConfig(min_segment_duration=0.0, min_gap_duration=0.0, exclusive=False).c_config(0.05)
    cnt = C.c_int64()
    args = (gpu_ctx.handle, C.byref(cfg), w.ctypes.data, nc, F, S, offs.ctypes.data, nc, hard.ctypes.data, K, None, 0)
    f = L.lib().fa_offline_reconstruct
    assert f(*args, None, 0, C.byref(cnt), None) == L.SUCCESS and cnt.value == len(got)
    small = (fa.reconstruct.RttmSegment * (len(got) - 1))()
    assert f(*args, small, len(got) - 1, C.byref(cnt), None) == L.OUTPUT_TOO_SMALL and cnt.value == len(got)
    exact = (fa.reconstruct.RttmSegment * len(got))()
    assert f(*args, exact, len(got), C.byref(cnt), None) == L.SUCCESS and cnt.value == len(got)
    assert bits(fa.reconstruct._segments(exact, len(got))) == bits(got)


def test_zero_vote_overrides(fa, gpu_ctx):
    rng = np.random.default_rng(21)
    C, F, S, K = 30, 90, 3, 7
    w, hard = random_case(rng, C=C, F=F, S=S, K=K)
    hard[rng.random((C, S)) < 0.5] = -2                 # many zero-vote frames
    T = R.frame_stats(w, hard, K, np.arange(C) * 2.0, 0.0)["T"]
    ov = [(int(a), int(a) + int(b), int(k)) for a, b, k in zip(rng.integers(0, T - 50, 12), rng.integers(0, 50, 12), rng.integers(0, K, 12))]
    check(fa, gpu_ctx, w, hard, K, np.arange(C) * 2.0, 0.0, overrides=ov, min_segment_duration=0.0)
    check(fa, gpu_ctx, w, hard, 70, np.arange(C) * 2.0, 0.0, overrides=[(0, T, 69), (5, 9, 3)], min_segment_duration=0.0)


def test_zero_vote_pass_reference_scenario(fa, gpu_ctx):
    """ZeroVoteReembedderTests.swift:196-301 through the device: S1 / S2 / S1 with S2 at 1.0-2.0 s; a failing embedder = the disabled pass."""
    w = np.array([[[0, 1] if 10 <= f < 20 else [1, 0] for f in range(30)]], np.float32)
    kw = dict(min_segment_duration=0.1, min_gap_duration=0.05, zero_vote_min_duration=0.4)
    cen = [[1, 0, 0], [0, 1, 0]]
    seg = fa.SegmentationOutput(w, [0.0], 0.1)
    spans = []
    rec = fa.OfflineReconstruction(fa.ReconstructionConfig(zero_vote_enabled=True, **kw), ctx=gpu_ctx)
    got = rec.build_segments(seg, [[0, -2]], cen, lambda a, b: spans.append((a, b)) or [0.1, 0.9, 0.0])
    assert rec.last_info["zero_vote_runs"] == [(10, 20)] and len(spans) == 1
    assert [s.speaker_id for s in got] == ["S1", "S2", "S1"] and abs(got[1].start_time_seconds - 1.0) < 1e-3 and abs(got[1].end_time_seconds - 2.0) < 1e-3
    want = R.build_segments(w, [[0, -2]], cen, [0.0], 0.1, R.config(**kw), lambda a, b: [0.1, 0.9, 0.0], zero_vote=True)
    assert bits(got) == bits(want)
    failing = rec.build_segments(seg, [[0, -2]], cen, lambda a, b: None)
    off = fa.OfflineReconstruction(fa.ReconstructionConfig(**kw), ctx=gpu_ctx).build_segments(seg, [[0, -2]], cen)
    assert bits(failing) == bits(off) and [s.speaker_id for s in off] == ["S1"]
    db = rec.build_speaker_database(got, cen)
    assert {k: v.tolist() for k, v in db.items()} == {k: v.tolist() for k, v in R.speaker_database(want, cen).items()}


def test_dev_entry_equals_host_entry(fa, gpu_ctx):
    import torch
    rng = np.random.default_rng(34)
    w, hard = random_case(rng, C=64, F=589, K=12)
    off = np.arange(64) * 2.0
    cfg = fa.ReconstructionConfig(min_segment_duration=0.0)
    host = fa.OfflineReconstruction(cfg, ctx=gpu_ctx).build_segments(fa.SegmentationOutput(w, off), hard, np.zeros((12, 2)))
    dev = fa.OfflineReconstruction(cfg, ctx=gpu_ctx).build_segments(fa.SegmentationOutput(torch.from_numpy(w).cuda(), off), hard, np.zeros((12, 2)))
    assert bits(dev) == bits(host) and len(host) > 100


def test_invalid_and_empty_inputs(fa, gpu_ctx):
    rng = np.random.default_rng(1)
    w, hard = random_case(rng, C=4, F=20, K=3)
    rec = fa.OfflineReconstruction(ctx=gpu_ctx)
    for bad in (np.nan, np.inf, -np.inf):
        x = w.copy()
        x[2, 7, 1] = bad
        with pytest.raises(fa.FluidAudioHipError) as e:
            rec.build_segments(fa.SegmentationOutput(x, np.arange(4) * 2.0), hard, np.zeros((3, 2)))
        assert e.value.status == fa.INVALID_ARGUMENT
    assert rec.build_segments(fa.SegmentationOutput(np.zeros((0, 20, 3), np.float32)), np.zeros((0, 3)), np.zeros((3, 2))) == []
    assert rec.build_segments(fa.SegmentationOutput(np.zeros((4, 0, 3), np.float32)), hard, np.zeros((3, 2))) == []


@pytest.mark.parametrize("classes, rows", [(7, 4 * 333 + 3), (5, 999), (9, 640), (7, 12)])
def test_powerset_decode(fa, gpu_ctx, classes, rows):
    import torch
    rng = np.random.default_rng(classes * 1000 + rows)
    x = (1.5 * rng.standard_normal((1, rows, classes))).astype(np.float32)
    x[0, ::17, :] = np.round(x[0, ::17, :])            # ties: the first maximum wins
    x[0, 5, :] = np.nan
    x[0, 6, :] = -np.inf
    x[0, 7, 2] = np.nan
    ww, lp = R.powerset_decode(x)
    seg = fa.powerset_decode(x, log_probs=True, ctx=gpu_ctx)
    assert np.array_equal(seg.speaker_weights, ww)
    fin = np.isfinite(x).all(axis=2)
    assert np.abs(seg.log_probs[fin] - lp[fin]).max() <= 1e-6
    dev = fa.powerset_decode(torch.from_numpy(x).cuda(), ctx=gpu_ctx)
    assert np.array_equal(dev.speaker_weights.cpu().numpy(), ww) and dev.log_probs is None


# ---- full size: 8 h, BASELINE config 5's geometry (14 400 windows of 10 s at a 2 s step, 589 frames, 7 classes)
def test_full_size_8h_decode_and_reconstruct(fa, gpu_ctx):
    import torch
    g = np.load(os.path.join(HERE, "golden", "e2e_8h.npz"))
    n_chunks = 14400
    lab = g["assignments"].astype(np.int32)
    cen = g["centroids"]
    hard = fa.chunk_assignments(np.repeat(np.arange(n_chunks), 3), np.tile(np.arange(3), n_chunks), lab, cen.shape[0], n_chunks, 3)
    x = R.session_logits(n_chunks)
    off = np.arange(n_chunks) * 2.0
    seg = fa.powerset_decode(torch.from_numpy(x).cuda(), off, ctx=gpu_ctx)
    rec = fa.OfflineReconstruction(ctx=gpu_ctx)
    got = rec.build_segments(seg, hard, cen, frame_records=True)
    w = seg.speaker_weights.cpu().numpy()
    assert np.array_equal(w, R.powerset_decode(x)[0])
    want, st = R.build_segments(w, hard, cen, off, 0.0, R.config(), return_state=True)
    assert rec.last_info["total_frames"] == st["T"] > 1_690_000
    check_frames(rec.last_info, st)
    assert rec.last_info["raw_segments"] == len(st["raw"])
    assert bits(got) == bits(want) and len(got) > 1000
    db = rec.build_speaker_database(got, cen)
    assert {k: v.tobytes() for k, v in db.items()} == {k: v.tobytes() for k, v in R.speaker_database(want, cen).items()}


def test_diarize_segments_1h(fa, gpu_ctx):
    from e2e_inputs import e2e_session
    s = e2e_session(hours=1.0)
    n_chunks = len(s["chunks"]) // 3
    x = R.session_logits(n_chunks, seed=9)
    off = np.arange(n_chunks) * 2.0
    seg = fa.powerset_decode(x, off, ctx=gpu_ctx)
    spk = np.tile(np.arange(3), n_chunks)
    out = fa.diarize_segments(s["emb"], s["rho"], s["chunks"], spk, s["phi"], seg, ctx=gpu_ctx)
    lab = np.asarray(out.clustering.assignments)
    cen = out.clustering.centroids
    hard = R.chunk_assignments(s["chunks"], spk, lab, cen.shape[0], n_chunks, 3)
    assert np.array_equal(out.hard_clusters, hard)
    want = R.build_segments(seg.speaker_weights, hard, cen, off, 0.0, R.config())
    assert bits(out.segments) == bits(want) and len(want) > 100
    assert {k: v.tobytes() for k, v in out.speaker_database.items()} == {k: v.tobytes() for k, v in R.speaker_database(want, cen).items()}


@pytest.mark.parametrize("F", [2048, 2049])
def test_run_compaction_block_boundary(fa, gpu_ctx, F):
    """One workgroup of the run-start compaction covers 256 x 8 = 2048 (frame, slot) items: one cluster (one slot per frame) and one chunk
    of 2048 frames fill it exactly, 2049 frames spill one item into a second."""
    rng = np.random.default_rng(F)
    w = (rng.random((1, F, 3)) < 0.5).astype(np.float32)
    w[0, -3:, :] = [[0, 0, 0], [1, 0, 1], [1, 0, 0]]        # a run that starts on the last item but one
    hard = np.array([[0, -2, 0]], np.int32)
    _, st = check(fa, gpu_ctx, w, hard, 1, [0.0], 0.0625, min_segment_duration=0.0, min_gap_duration=0.0)
    assert st["T"] == F and len(st["raw"]) > 100
    _, st = check(fa, gpu_ctx, w, hard, 1, [0.0], 0.0625)     # defaults: merge, 1 s minimum, exclusive
    assert st["T"] == F


@pytest.mark.parametrize("F", [2047, 2048, 2049, 4095, 4096, 4097])
def test_run_compaction_kept_none_densest_and_the_last_item(fa, gpu_ctx, F):
    """One cluster, one slot per frame: F items end one short of, at, and one past the first and the second compaction workgroup (256 x 8
    items each).  No run; a run on every other frame, the most a cluster can start (a start needs the frame before it inactive); and one
    run that starts on the last item."""
    hard = np.array([[0, -2, 0]], np.int32)
    for kind, runs in (("none", 0), ("densest", (F + 1) // 2), ("last", 1)):
        w = np.zeros((1, F, 3), np.float32)
        if kind == "densest":
            w[0, ::2, 0] = 1
        elif kind == "last":
            w[0, -1, 2] = 1
        _, st = check(fa, gpu_ctx, w, hard, 1, [0.0], 0.0625, min_segment_duration=0.0, min_gap_duration=0.0)
        assert st["T"] == F and len(st["raw"]) == runs


def test_powerset_decode_of_misaligned_logits(fa, gpu_ctx):
    """7 classes whose logits start one float past a 16-byte boundary take the row kernel and give what the aligned tensor gives; fewer
    rows than one group of four run as the tail alone."""
    import torch
    rng = np.random.default_rng(77)
    for rows in (4 * 333 + 3, 3):
        x = (1.5 * rng.standard_normal((1, rows, 7))).astype(np.float32)
        x[0, ::5, :] = np.round(x[0, ::5, :])
        x[0, 1, :] = np.nan
        ww, lp = R.powerset_decode(x)
        aligned = torch.from_numpy(x).cuda(gpu_ctx.device)
        store = torch.zeros(rows * 7 + 4, dtype=torch.float32, device=aligned.device)
        shifted = store[1:1 + rows * 7].view(1, rows, 7)
        shifted.copy_(aligned)
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        a = fa.powerset_decode(aligned, log_probs=True, ctx=gpu_ctx)
        b = fa.powerset_decode(shifted, log_probs=True, ctx=gpu_ctx)
        assert np.array_equal(a.speaker_weights.cpu().numpy(), ww) and np.array_equal(b.speaker_weights.cpu().numpy(), ww)
        fin = np.isfinite(x).all(axis=2)
        la, lb = a.log_probs.cpu().numpy(), b.log_probs.cpu().numpy()
        assert np.array_equal(la[fin].view(np.uint32), lb[fin].view(np.uint32)) and np.abs(lb[fin] - lp[fin]).max() <= 1e-6
        assert np.array_equal(fa.powerset_decode(shifted, ctx=gpu_ctx).speaker_weights.cpu().numpy(), ww)


def test_reconstruct_early_exits(fa, gpu_ctx):
    """The status, the error text, *count and the fa_reconstruct_info fields at every exit fa_offline_reconstruct takes before it touches
    the device, in the order it checks: a call that is wrong in two ways reports the earlier one."""
    L = fa._lib
    f = L.lib().fa_offline_reconstruct
    nc, F, S, K = 2, 4, 3, 2
    w = np.zeros((nc, F, S), np.float32)
    hard = np.zeros((nc, S), np.int32)
    fields = ("total_frames", "raw_segments", "frame_duration", "zero_vote_run_count", "frame_slots")

    def cfg_of(**kw):
        return fa.ReconstructionConfig(**kw).c_config(0.0)

    def call(ctx, cfg, count=True, speakers=S, overrides=()):
        info = L.ReconstructInfo()
        for k in fields:
            setattr(info, k, -7)
        cnt = C.c_int64(-7)
        ov = np.asarray(overrides, np.int64).reshape(-1, 3)
        st = f(ctx, C.byref(cfg) if cfg is not None else None, w.ctypes.data, nc, F, speakers, None, 0, hard.ctypes.data, K,
               ov.ctypes.data if len(ov) else None, len(ov), None, 0, C.byref(cnt) if count else None, C.byref(info))
        return st, cnt.value, tuple(getattr(info, k) for k in fields), (gpu_ctx.last_error() if st != L.SUCCESS else None)

    good = cfg_of()
    untouched, cleared = (-7, -7, -7.0, -7, -7), (0, 0, 0.0, 0, 0)
    required = "reconstruct: ctx, config and count are required"
    bad_override = [(0, 8, 1), (0, 9, 0)]                      # the second one ends past the 8 global frames
    # 1. - 3. no context, no config, no count: nothing is written
    assert call(None, None, count=False)[:3] == (L.INVALID_ARGUMENT, -7, untouched)
    assert call(gpu_ctx.handle, None, speakers=2 ** 15) == (L.INVALID_ARGUMENT, -7, untouched, required)
    assert call(gpu_ctx.handle, good, count=False, speakers=2 ** 15) == (L.INVALID_ARGUMENT, -7, untouched, required)
    # 4. more local speakers than a frame word counts, before the frame duration is looked at
    assert call(gpu_ctx.handle, cfg_of(window_duration=np.inf), speakers=2 ** 15) == (L.INVALID_ARGUMENT, 0, cleared, "reconstruct: bad arguments")
    # 5. a frame duration that is not finite, before the overrides are looked at
    assert call(gpu_ctx.handle, cfg_of(window_duration=np.inf), overrides=bad_override) == (
        L.INVALID_ARGUMENT, 0, cleared, "reconstruct: frame duration is not finite")
    assert call(gpu_ctx.handle, cfg_of(window_duration=np.nan))[0] == L.INVALID_ARGUMENT
    # 6. a frame duration that is not positive: no segments, like the reference
    assert call(gpu_ctx.handle, cfg_of(window_duration=-10.0), overrides=bad_override) == (L.SUCCESS, 0, cleared, None)
    assert call(gpu_ctx.handle, cfg_of(window_duration=0.0)) == (L.SUCCESS, 0, cleared, None)
    # 7. an override out of range: the frame count, the frame duration and the slots are already reported
    assert call(gpu_ctx.handle, good, overrides=bad_override) == (L.INVALID_ARGUMENT, 0, (8, 0, 2.5, 0, 2), "reconstruct: override 1 is out of range")
