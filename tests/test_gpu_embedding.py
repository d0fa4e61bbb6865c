"""The embedding model's inputs on the device (csrc/embedding.hip, driven by csrc/embedding_host.hip) equal the numpy restatement (tests/embedding_restatement.py) bit for bit:
records (times as fp64 bits), run_of_job, window_of_run, the run rows, the mask rows and the counters; fbank windows and span inputs equal
numpy slicing; the chain powerset decode -> extract_embeddings -> diarize_segments gives the segments of the restatement's plan."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import embedding_restatement as E  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def configs(fa, **kw):
    return fa.EmbeddingConfig(**kw), E.Config(**kw)


def hard_weights(fa, ctx, C, F=589, seed=0):
    """fa_powerset_decode of random logits (biased toward silence and single speakers), on the device."""
    import torch
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((C, F, 7)).astype(f32)
    logits[..., 0] += 0.5
    logits[..., 1:4] += 1.0
    # runs of one class so that masks survive the 20 % rule
    for c in range(C):
        k = int(rng.integers(0, 7))
        a = int(rng.integers(0, F // 2))
        logits[c, a:a + F // 2, k] += 6.0
    seg = fa.powerset_decode(torch.from_numpy(logits).cuda(ctx.device), ctx=ctx)
    return seg


def check(fa, ctx, w, offsets, total, fd=0.0, on_device=True, **kw):
    import torch
    dcfg, rcfg = configs(fa, **kw)
    want = E.plan(w.cpu().numpy() if hasattr(w, "cpu") else w, offsets, total, rcfg, fd)
    ww = w if on_device or not hasattr(w, "cpu") else w.cpu().numpy()
    if on_device and not hasattr(ww, "cuda"):
        ww = torch.from_numpy(np.ascontiguousarray(ww)).cuda(ctx.device)
    p = fa.plan_embeddings(fa.SegmentationOutput(ww, offsets, fd), total, dcfg, mask_rows=True, ctx=ctx)
    rec = p.records
    got = [(int(r["chunk_index"]), int(r["speaker_index"]), int(r["start_frame"]), int(r["end_frame"])) for r in rec]
    assert got == [r[:4] for r in want["records"]]
    st = np.array([r[4] for r in want["records"]], np.float64).view(np.uint64)
    en = np.array([r[5] for r in want["records"]], np.float64).view(np.uint64)
    assert np.array_equal(rec["start_time"].view(np.uint64), st) and np.array_equal(rec["end_time"].view(np.uint64), en)
    assert np.array_equal(p.run_of_job, want["run_of_job"])
    assert np.array_equal(p.window_of_run, want["window_of_run"])
    assert p.window_chunk.tolist() == [c for c, _, _ in want["windows"]]
    assert p.window_start.tolist() == [s for _, _, s in want["windows"]]
    rows = p.run_weights.cpu().numpy() if hasattr(p.run_weights, "cpu") else p.run_weights
    mrows = p.mask_rows.cpu().numpy() if hasattr(p.mask_rows, "cpu") else p.mask_rows
    assert np.array_equal(rows.view(np.uint32), want["run_rows"].view(np.uint32))
    assert np.array_equal(mrows.view(np.uint32), want["mask_rows"].view(np.uint32))
    i = p.info
    assert (i["evaluated_masks"], i["empty_masks"], i["fallback_masks"], i["skipped_embeddings"]) == (want["evaluated"], want["empty"], want["fallback"], want["skipped"])
    assert i["batch_size"] == want["batch"] and i["planned_chunks"] == len(want["windows"])
    return p, want


@pytest.mark.parametrize("C", [1, 31, 32, 33])
@pytest.mark.parametrize("exclude", [True, False])
def test_hard_weights(fa, gpu_ctx, C, exclude):
    seg = hard_weights(fa, gpu_ctx, C, seed=C)
    offs = np.arange(C) * 2.0
    p, want = check(fa, gpu_ctx, seg.speaker_weights, offs, 16000 * (2 * C + 10), exclude_overlap=exclude)
    assert len(want["records"]) > 0


@pytest.mark.parametrize("batch", [1, 7, 32, 64])
@pytest.mark.parametrize("skip", [None, 0.95, 1.0, 0.0, -0.5])
def test_batches_and_skip(fa, gpu_ctx, batch, skip):
    seg = hard_weights(fa, gpu_ctx, 70, seed=7)
    _, want = check(fa, gpu_ctx, seg.speaker_weights, np.arange(70) * 1.5, 16000 * 120, batch_size=batch, skip_threshold=skip)
    if skip is not None and skip <= 0 and batch > 1:     # a threshold at or below 0 reuses every cached embedding of a batch
        assert want["skipped"] > 0


@pytest.mark.parametrize("W", [589, 998, 300, 1])
def test_weight_frames(fa, gpu_ctx, W):
    seg = hard_weights(fa, gpu_ctx, 40, seed=W)
    check(fa, gpu_ctx, seg.speaker_weights, None, 16000 * 400, weight_frames=W, skip_threshold=0.95)


def soft_weights(C=50, F=589, seed=3):
    """Soft weights whose masks survive: per chunk one dominant speaker per run of frames (values in (0.3, 1]), the others below, at or
    just above the 1e-3 threshold.  Exactly 1e-3 sits at the edges of active runs (inactive: it moves first / last active), inside them,
    and on a second speaker during another's run (not an overlap: the rule is > 1e-3); some frames hold a real second speaker."""
    rng = np.random.default_rng(seed)
    w = (rng.random((C, F, 3)) * f32(1e-3)).astype(f32)                 # below the threshold everywhere
    for c in range(C):
        e0 = int(rng.integers(120, 280))
        bounds = [0, e0, e0 + int(rng.integers(150, 250)), F]
        for r in range(3):
            a, b = bounds[r], bounds[r + 1]
            s = int(rng.integers(0, 3))
            w[c, a:b, s] = rng.uniform(0.3, 1.0, b - a).astype(f32)
            w[c, a, s] = w[c, b - 1, s] = f32(1e-3)                     # run edges exactly at the threshold
            w[c, rng.integers(a, b, 3), s] = f32(1e-3)                  # and inside the run
            o = (s + 1) % 3
            w[c, rng.integers(a, b, 12), o] = f32(1e-3)                 # a second speaker exactly at the threshold: no overlap
            k = int(rng.integers(a, b - 8))
            w[c, k:k + int(rng.integers(1, 8)), o] = rng.uniform(0.002, 0.5, 1).astype(f32)   # a real overlap
    w[:3] *= f32(0.01)                                                   # three quiet chunks: every mask empty
    return w


@pytest.mark.parametrize("on_device", [True, False])
def test_soft_weights(fa, gpu_ctx, on_device):
    w = soft_weights()
    for W, exclude, skip in ((589, True, 0.9), (589, False, None), (300, True, 0.5), (300, False, 0.9)):
        _, want = check(fa, gpu_ctx, w, np.arange(50) * 3.0, 16000 * 200, on_device=on_device, weight_frames=W, exclude_overlap=exclude,
                        skip_threshold=skip)
        assert len(want["records"]) > 50 and want["empty"] > 9
        if skip == 0.5:
            assert want["skipped"] > 10                                  # soft masks: cosine hits and misses


def fallback_weights(C=40, F=589, seed=4):
    """0/1 weights where, at min_segment_duration 3 s (minFrames 177), many clean masks keep 118-176 frames: the base mask is used."""
    rng = np.random.default_rng(seed)
    w = np.zeros((C, F, 3), f32)
    for c in range(C):
        a = int(rng.integers(0, 200))
        n0 = int(rng.integers(180, 280))
        w[c, a:a + n0, 0] = 1
        o = a + int(rng.integers(0, n0 - 20))
        w[c, o:o + int(rng.integers(20, 140)), 1] = 1                     # overlaps speaker 0: its clean mask shrinks
        b = int(rng.integers(0, F - 150))
        w[c, b:b + int(rng.integers(100, 150)), 2] = 1
    return w


@pytest.mark.parametrize("skip", [None, 0.95])
def test_fallback_to_the_base_mask(fa, gpu_ctx, skip):
    w = fallback_weights()
    for W in (589, 300):
        _, want = check(fa, gpu_ctx, w, np.arange(40) * 2.0, 16000 * 100, weight_frames=W, min_segment_duration=3.0, skip_threshold=skip)
        assert want["fallback"] > 5 and len(want["records"]) > want["fallback"]
        fb = [j for j, r in enumerate(want["records"]) if r[1] == 0 and want["mask_rows"][j].sum() > 177]
        assert fb                                                        # base masks that keep their overlap frames


def test_nan_in_a_chunk_that_is_not_planned(fa, gpu_ctx):
    """Only the weights of planned chunks are read: a NaN in a chunk past the audio is not an error."""
    w = fallback_weights(C=6)
    w[5, 10, 1] = np.nan
    _, want = check(fa, gpu_ctx, w, np.arange(6) * 10.0, 16000 * 45)
    assert len(want["windows"]) == 5
    with pytest.raises(ValueError):
        E.plan(w, np.arange(6) * 10.0, 16000 * 60, E.Config())


def test_offsets_cut_off_and_edge_cases(fa, gpu_ctx):
    seg = hard_weights(fa, gpu_ctx, 20, seed=11)
    w = seg.speaker_weights
    # irregular, non-finite and .5-sample offsets; total samples that cut the last chunks off
    offs = np.array([0.0, 0.00003125, np.nan, 7.5, 3.0, np.inf, 1e-9, 45.00003125, 50.0, -1.0, 2.0], np.float64)
    check(fa, gpu_ctx, w, offs, 16000 * 55 + 3)
    check(fa, gpu_ctx, w, offs, 16000 * 55 + 3, fd=0.02, min_segment_duration=3.0)
    check(fa, gpu_ctx, w, None, 0)                             # no audio: nothing planned
    p = fa.plan_embeddings(fa.SegmentationOutput(np.zeros((0, 589, 3), f32)), 1000, ctx=gpu_ctx)
    assert p.records.size == 0 and p.info["planned_chunks"] == 0


def test_eight_hours(fa, gpu_ctx):
    seg = hard_weights(fa, gpu_ctx, 14400, seed=8)
    offs = np.arange(14400) * 2.0
    p, want = check(fa, gpu_ctx, seg.speaker_weights, offs, 16000 * 28810)
    assert p.info["jobs"] > 5000
    check(fa, gpu_ctx, seg.speaker_weights, offs, 16000 * 28810, skip_threshold=0.95)


def test_nan_weight_is_invalid(fa, gpu_ctx):
    import torch
    w = torch.zeros((4, 589, 3), device=f"cuda:{gpu_ctx.device}")
    w[2, 100, 1] = float("nan")
    with pytest.raises(fa.FluidAudioHipError) as e:
        fa.plan_embeddings(fa.SegmentationOutput(w), 16000 * 100, ctx=gpu_ctx)
    assert e.value.status == fa.INVALID_ARGUMENT


def test_windows_and_spans(fa, gpu_ctx):
    import torch
    rng = np.random.default_rng(5)
    total = 16000 * 33 + 77
    audio = rng.standard_normal(total).astype(f32)
    da = torch.from_numpy(audio).cuda(gpu_ctx.device)
    seg = hard_weights(fa, gpu_ctx, 17, seed=17)
    cfg = fa.EmbeddingConfig(batch_size=3)
    p = fa.plan_embeddings(seg, total, cfg, ctx=gpu_ctx)
    assert p.batches == 2                                      # chunks at 0, 10, 20, 30 s (33 s of audio): the last window is partial
    for b in range(p.batches):
        got = p.windows(b, da).cpu().numpy()
        want = E.windows(audio, p.window_start[p.batch_windows(b).start:p.batch_windows(b).stop], cfg.window_samples)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    spans = [(1.0, 3.5), (5.0, 5.0), (30.0, 45.0), (0.00003125, 0.5), (-1.0, 0.25), (20.0, 40.0), (40.0, 41.0)]
    rcfg = E.Config()
    wv, wt, ok = E.span_inputs(audio, spans, rcfg)
    for x in (da, audio):
        gw, gt, gok = fa.span_inputs(x, spans, cfg, ctx=gpu_ctx)
        gw = gw.cpu().numpy() if hasattr(gw, "cpu") else gw
        gt = gt.cpu().numpy() if hasattr(gt, "cpu") else gt
        assert gok.tolist() == ok.tolist() == [True, False, True, True, True, True, False]
        assert np.array_equal(gw.view(np.uint32), wv.view(np.uint32)) and np.array_equal(gt.view(np.uint32), wt.view(np.uint32))


def test_weight_resample_matches_reference_cases(fa, gpu_ctx):
    import torch
    assert fa.weight_resample(np.array([0, 10, 20, 30], f32), 2, ctx=gpu_ctx).tolist() == [5.0, 25.0]
    x = np.array([1, 2, 3, 4], f32)
    assert np.array_equal(fa.weight_resample(x, 4, ctx=gpu_ctx), x)
    assert fa.weight_resample(np.zeros(0, f32), 5, ctx=gpu_ctx).size == 0
    assert fa.weight_resample(np.array([1, 2, 3], f32), 0, ctx=gpu_ctx).size == 0
    assert fa.weight_resample(np.array([[1, 3, 5, 7], [2, 4, 6, 8]], f32), 2, ctx=gpu_ctx).tolist() == [[2.0, 6.0], [3.0, 7.0]]
    rng = np.random.default_rng(9)
    for n_in, n_out in ((589, 589), (589, 998), (589, 300), (16, 7), (3, 5), (589, 1)):
        rows = rng.standard_normal((13, n_in)).astype(f32)
        want = E.resample(rows, n_out)
        got = fa.weight_resample(torch.from_numpy(rows).cuda(gpu_ctx.device), n_out, ctx=gpu_ctx).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def synthetic_embedder(proj):
    """A deterministic stand-in for fbank + embedding: a fixed projection of masked window statistics."""
    import torch

    def embed(windows, weights, window_of_run):
        x = windows.double().reshape(windows.shape[0], 100, -1)        # 100 blocks of samples per window
        blocks = torch.stack([x.abs().mean(-1), x.std(-1)], dim=-1)    # [Bw, 100, 2]
        w = torch.nn.functional.interpolate(weights.double()[:, None, :], size=100, mode="nearest")[:, 0]   # [Br, 100]
        feats = (blocks[window_of_run] * w[..., None]).reshape(weights.shape[0], -1)
        return (feats @ proj).float()
    return embed


def test_end_to_end_against_the_restatement_plan(fa, gpu_ctx):
    import torch
    from fluidaudio_amd.pipeline import extract_embeddings, span_embedder
    rng = np.random.default_rng(21)
    C, total = 60, 16000 * 130
    seg = hard_weights(fa, gpu_ctx, C, seed=21)
    seg.chunk_offsets = np.arange(C) * 2.0
    spk = rng.standard_normal((3, total // 16000 + 1)).astype(f32)
    t = np.arange(total) // 16000
    audio = (rng.standard_normal(total) * 0.1 + np.sin(np.arange(total) * 0.05) * spk[0, t]).astype(f32)
    proj = torch.from_numpy(rng.standard_normal((200, 256))).double().cuda(gpu_ctx.device)
    pl = torch.from_numpy(rng.standard_normal((256, 128))).double().cuda(gpu_ctx.device)
    embed = synthetic_embedder(proj)

    def plda(e):
        return torch.as_tensor(np.asarray(e), dtype=torch.float64, device=pl.device) @ pl
    cfg = fa.EmbeddingConfig(skip_threshold=0.95)
    out = extract_embeddings(seg, audio, embed, plda, cfg, ctx=gpu_ctx)
    # the same chain driven by the restatement's plan
    w = seg.speaker_weights.cpu().numpy()
    want = E.plan(w, seg.chunk_offsets, total, E.Config(skip_threshold=0.95))
    da = torch.from_numpy(audio).cuda(gpu_ctx.device)
    B = want["batch"]
    run_emb = []
    for b in range(0, len(want["windows"]), B):
        starts = [s for _, _, s in want["windows"][b:b + B]]
        wins = torch.from_numpy(E.windows(audio, starts, 160000)).cuda(gpu_ctx.device)
        sel = [r for r, wi in enumerate(want["window_of_run"]) if b <= wi < b + B]
        if not sel:
            continue
        rows = torch.from_numpy(want["run_rows"][sel]).cuda(gpu_ctx.device)
        wor = torch.as_tensor(want["window_of_run"][sel] - b, device=da.device)
        run_emb.append(embed(wins, rows, wor).cpu().numpy())
    emb = np.concatenate(run_emb)[want["run_of_job"]]
    assert np.array_equal(out.embedding256.view(np.uint32), emb.view(np.uint32))
    rho = plda(emb).cpu().numpy()
    assert np.array_equal(out.rho128.view(np.uint64), rho.view(np.uint64))
    assert out.chunk_indices.tolist() == [r[0] for r in want["records"]]
    assert out.speaker_indices.tolist() == [r[1] for r in want["records"]]
    phi = np.abs(rng.standard_normal(128)) + 0.5
    rcfg = fa.ReconstructionConfig(zero_vote_enabled=True)
    se = span_embedder(audio, embed, cfg, ctx=gpu_ctx)
    got = fa.diarize_segments(out.embedding256, out.rho128, out.chunk_indices, out.speaker_indices, phi, seg, reconstruction=rcfg,
                              span_embedder=se, ctx=gpu_ctx)
    ref = fa.diarize_segments(emb, rho, np.array([r[0] for r in want["records"]], np.int32), np.array([r[1] for r in want["records"]], np.int32),
                              phi, seg, reconstruction=rcfg, span_embedder=se, ctx=gpu_ctx)
    key = [(s.speaker_id, s.start_time_seconds, s.end_time_seconds, s.quality_score) for s in got.segments]
    assert key == [(s.speaker_id, s.start_time_seconds, s.end_time_seconds, s.quality_score) for s in ref.segments] and key
    # the span path on its own: embedSpan's inputs through the restatement give the same embedding
    win, wts, ok = E.span_inputs(audio, [(12.0, 15.5)], E.Config())
    e_ref = embed(torch.from_numpy(win).cuda(da.device), torch.from_numpy(wts).cuda(da.device), torch.zeros(1, dtype=torch.int64, device=da.device))
    assert np.array_equal(se(12.0, 15.5), e_ref.cpu().numpy()[0]) and se(20.0, 20.0) is None


def test_extract_embeddings_moves_host_weights_to_the_device(fa, gpu_ctx):
    """Speaker weights on the host: the embedder still receives torch CUDA weights, and the embeddings equal the device-weights run."""
    import torch
    from fluidaudio_amd.pipeline import extract_embeddings
    rng = np.random.default_rng(31)
    seg = hard_weights(fa, gpu_ctx, 12, seed=31)
    total = 16000 * 130
    audio = rng.standard_normal(total).astype(f32)
    embed = synthetic_embedder(torch.from_numpy(rng.standard_normal((200, 256))).double().cuda(gpu_ctx.device))
    seen = []

    def checked(windows, weights, wor):
        seen.append(weights.is_cuda and windows.is_cuda and wor.is_cuda)
        return embed(windows, weights, wor)

    def plda(e):
        return np.asarray(e, np.float64)[:, :128]
    host = fa.SegmentationOutput(seg.speaker_weights.cpu().numpy(), seg.chunk_offsets, seg.frame_duration)
    a = extract_embeddings(host, audio, checked, plda, ctx=gpu_ctx)
    b = extract_embeddings(seg, audio, checked, plda, ctx=gpu_ctx)
    assert seen and all(seen) and a.embedding256.shape[0] > 0
    assert np.array_equal(a.embedding256.view(np.uint32), b.embedding256.view(np.uint32)) and a.chunk_indices.tolist() == b.chunk_indices.tolist()


@pytest.mark.parametrize("F,S", [(3000, 3), (9000, 2)])
def test_long_chunks_read_in_place(fa, gpu_ctx, F, S):
    """Chunks too large for LDS are read in place; past 8192 frames the overlap flags are recomputed per frame."""
    rng = np.random.default_rng(F)
    w = np.zeros((6, F, S), f32)
    for c in range(6):
        for s in range(S):                                                # speaker s mostly in its own third, partly overlapping the next
            a = s * F // 3 + int(rng.integers(0, F // 20))
            w[c, a:a + F // 3 + int(rng.integers(0, F // 10)), s] = rng.uniform(0.5, 1.0)
    _, want = check(fa, gpu_ctx, w, np.arange(6) * 10.0, 16000 * 70, weight_frames=589, skip_threshold=0.5)
    assert len(want["records"]) >= 6 and want["skipped"] > 0


@pytest.mark.parametrize("skip", [None, 0.95])
@pytest.mark.parametrize("C", [512, 513])
def test_compaction_block_boundary(fa, gpu_ctx, C, skip):
    """One compaction workgroup covers 256 x 8 = 2048 (window, speaker) items: four speakers and 512 planned chunks fill one exactly, 513 spill
    four items into a second; both compactions (valid masks -> jobs, jobs that run the model -> runs) cross the boundary."""
    rng = np.random.default_rng(C)
    w = (rng.random((C, 8, 4)) < 0.3).astype(f32)
    w[rng.random(C) < 0.3] = 0                                            # silent chunks: empty masks between the jobs
    w[-2:] = 0
    w[-2:, :, 0] = 1                                                      # a lone speaker in the last two chunks: jobs past the boundary when C = 513
    _, want = check(fa, gpu_ctx, w, np.arange(C) * 1.0, 16000 * (C + 20), weight_frames=5, skip_threshold=skip)
    assert want["evaluated"] == 4 * C and len(want["windows"]) == C
    assert 200 < len(want["records"]) < 4 * C and want["empty"] > 200 and want["records"][-1][0] == C - 1
    if skip is not None:
        assert 0 < want["skipped"] < len(want["records"])


@pytest.mark.parametrize("C", [2047, 2048, 2049, 4095, 4096, 4097])
def test_compaction_kept_none_all_and_the_last_item(fa, gpu_ctx, C):
    """One speaker: an item per planned chunk, so C items end one short of, at, and one past the first and the second compaction workgroup
    (256 x 8 items each).  No item kept, every item kept, and the last item alone."""
    for kind in ("none", "all", "last"):
        w = np.zeros((C, 8, 1), f32)
        if kind != "none":
            w[0 if kind == "all" else C - 1:] = 1
        _, want = check(fa, gpu_ctx, w, np.arange(C) * 1.0, 16000 * (C + 20), weight_frames=5)
        assert want["evaluated"] == C and len(want["records"]) == {"none": 0, "all": C, "last": 1}[kind]
        assert kind == "none" or want["records"][-1][0] == C - 1


def test_plan_early_exits(fa, gpu_ctx):
    """The status, the error text and the fa_embedding_info fields at every exit fa_embedding_plan takes before it touches the device, in the
    order it checks: a call that is wrong in two ways reports the earlier one."""
    import ctypes as C
    L = fa._lib
    f = L.lib().fa_embedding_plan
    F, S = 4, 3
    w = np.zeros((2, F, S), f32)
    rec = np.zeros(8, fa.embedding.RECORD_DTYPE)
    roj, wor, wch = (np.full(8, -7, np.int32) for _ in range(3))
    wst = np.full(8, -7, np.int64)
    rows = np.zeros((8, 589), f32)
    outs = (rec.ctypes.data, roj.ctypes.data, wor.ctypes.data, wst.ctypes.data, wch.ctypes.data, rows.ctypes.data, None)
    no_outs = (None,) * 7
    good = fa.EmbeddingConfig().c_config()
    bad = fa.EmbeddingConfig(sample_rate=0).c_config()
    zero = dict.fromkeys((k for k, _ in L.EmbeddingInfo._fields_), 0)

    def call(ctx, cfg, weights, nc, nf, ns, total, outputs):
        info = L.EmbeddingInfo(*([-7] * len(L.EmbeddingInfo._fields_)))
        st = f(ctx, C.byref(cfg) if cfg is not None else None, weights, nc, nf, ns, None, 0, total, *outputs, C.byref(info))
        return st, info.as_dict(), (gpu_ctx.last_error() if st != L.SUCCESS else None)

    untouched = dict.fromkeys(zero, -7)
    # 1. no context: nothing is written, not even info
    assert call(None, bad, None, -1, F, S, 1000, no_outs) == (L.INVALID_ARGUMENT, untouched, gpu_ctx.last_error())
    # 2. a bad config, before the arguments are looked at
    for cfg in (None, bad):
        assert call(gpu_ctx.handle, cfg, None, -1, F, S, 1000, no_outs) == (L.INVALID_ARGUMENT, zero, "embedding plan: bad config")
    # 3. bad arguments (a negative size; weights missing), before the outputs are looked at
    assert call(gpu_ctx.handle, good, w.ctypes.data, -1, F, S, 1000, no_outs) == (L.INVALID_ARGUMENT, zero, "embedding plan: bad arguments")
    assert call(gpu_ctx.handle, good, None, 2, F, S, 1000, no_outs) == (L.INVALID_ARGUMENT, zero, "embedding plan: bad arguments")
    # 4. missing outputs, before the mask limit
    assert call(gpu_ctx.handle, good, w.ctypes.data, 2 ** 29, F, S, 1000, no_outs) == (
        L.INVALID_ARGUMENT, zero, "embedding plan: records, run_of_job, window_of_run and run_weights are required")
    # 5. more than 2^30 (chunk, speaker) or (frame, speaker) pairs; no weight is read
    assert call(gpu_ctx.handle, good, w.ctypes.data, 2 ** 29, F, S, 1000, outs) == (L.INDEX_OVERFLOW, zero, "embedding plan: more than 2^30 masks")
    assert call(gpu_ctx.handle, good, w.ctypes.data, 2, 2 ** 29, S, 1000, outs) == (L.INDEX_OVERFLOW, zero, "embedding plan: more than 2^30 masks")
    # 6. no chunk, or no frame: the config's geometry is reported
    geom = dict(zero, samples_per_window=160000, batch_size=32)
    assert call(gpu_ctx.handle, good, None, 0, 589, S, 1000, no_outs) == (L.SUCCESS, dict(geom, frame_duration=10.0 / 589, min_frames=59), None)
    assert call(gpu_ctx.handle, good, None, 3, 0, S, 1000, no_outs) == (L.SUCCESS, dict(geom, frame_duration=0.0, min_frames=1), None)
    # 7. no planned window (no audio): the counts of the plan are zero and no output is written
    assert call(gpu_ctx.handle, good, w.ctypes.data, 2, F, S, 0, outs) == (L.SUCCESS, dict(geom, frame_duration=2.5, min_frames=1), None)
    assert wst.tolist() == [-7] * 8 and wch.tolist() == [-7] * 8 and roj.tolist() == [-7] * 8
