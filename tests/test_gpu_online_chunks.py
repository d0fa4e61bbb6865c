"""The online diarizer around the networks on the device — fa_online_chunk_plan, fa_online_pack_waveforms_dev, fa_online_chunk_finish_dev
(csrc/online.hip, csrc/online_host.hip) — against the line-by-line restatement of DiarizerManager.processChunkWithSpeakerTracking and
EmbeddingExtractor.getEmbeddings (tests/online_restatement.py).  No tolerances: integers as they are, fp32 as bits.  The same file is run
on the poisoned-workspace library (make POISON=1).  Expectations are computed on the CPU; sizes are the smallest that can go wrong."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
FRAMES = (1, 63, 64, 65, 589)
STEP = 0.016875
SOFT = (1.0, 1.0, 0.5, 0.31, 0.3, 0.29, 0.2, 0.16, 0.15, 0.14, 0.05)


def unit(rng):
    v = rng.standard_normal(256).astype(F)
    return v / F(np.sqrt(np.sum(v.astype(np.float64) ** 2)))


def cfg_for(frames):
    """The reference's ten active frames where a chunk can hold them; runs of 16 frames are exactly the minimum duration at offset 0."""
    small = frames < 32
    min_speech = F((0.0 + 1.0 * STEP) - 0.0) if small else F((0.0 + 16.0 * STEP) - 0.0)
    return dict(frames=frames, chunk_samples=160000, min_active_frames=1.0 if small else 10.0, min_speech_duration=float(min_speech))


def draw_weights(rng, frames, soft):
    """Per speaker runs and gaps of 1 .. 70 frames (15, 16, 17 round the minimum duration; 70 crosses a 64-frame boundary), hard or soft values."""
    w = np.zeros((frames, 3), F)
    for s in range(3):
        f = 0 if rng.random() < 0.5 else int(rng.integers(1, 20))
        while f < frames:
            n = int((1, 2, 15, 16, 17, 40, 70)[rng.integers(7)])
            value = F(SOFT[rng.integers(len(SOFT))]) if soft else F(1.0)
            if soft and rng.random() < 0.3:
                w[f:f + n, s] = rng.choice(np.array(SOFT, F), min(n, frames - f))
            else:
                w[f:f + n, s] = value
            f += n + int((1, 3, 16, 30)[rng.integers(4)])
    return w


def crafted(frames):
    """Speakers 0 and 1 start together at frame 0 for 16 frames (equal starts, a run of exactly the minimum duration at offset 0); speaker 2 is
    active on exactly ten frames, the last ten (at the minimum: it passes createTimedSegments' `<` and not the gate's `>`)."""
    w = np.zeros((frames, 3), F)
    w[:16, 0] = 1.0
    w[:16, 1] = 1.0
    if frames >= 40:
        w[frames - 10:, 2] = 1.0
        w[20:30, 0] = 1.0                     # the same for a speaker that was given an id: ten more frames would pass, these are exactly 26 > 10
    return w


def to_bits_records(segments, b, c):
    return [(b, c, s, id, f0, f1, R.bits1(t0), R.bits1(t1), R.bits1(q)) for s, id, f0, f1, t0, t1, q in segments]


def seg_tuples(rec):
    return [(int(r["stream"]), int(r["chunk"]), int(r["local_speaker"]), int(r["id"]), int(r["start_frame"]), int(r["end_frame"]),
             R.bits1(r["start"]), R.bits1(r["end"]), R.bits1(r["quality"])) for r in rec]


@pytest.mark.parametrize("frames", FRAMES)
def test_plan_rows_runs_and_activities(fa, gpu_ctx, frames):
    import torch
    rng = np.random.default_rng(frames)
    kw = cfg_for(frames)
    cfg, rcfg = fa.OnlineChunkConfig(**kw), R.ChunkConfig(**kw)
    full = kw["chunk_samples"]
    samples = np.array([[0, 1, full // 2, full, full - 1]] * 3, np.int32)
    logits = torch.from_numpy(rng.standard_normal((5, frames, 7)).astype(F) * 3).cuda()
    hard = fa.powerset_decode(logits, ctx=gpu_ctx).speaker_weights                             # 0/1 weights as fa_powerset_decode_dev leaves them
    w = torch.stack([hard, torch.from_numpy(np.stack([draw_weights(rng, frames, True) for _ in range(5)])).cuda(),
                     torch.from_numpy(np.stack([draw_weights(rng, frames, False) for _ in range(5)])).cuda()]).contiguous()
    w[2, :, :, 2] = 0                                                                  # a silent speaker: it runs no model
    hw = w.cpu().numpy()
    assert set(np.unique(hw[0]).tolist()) <= {0.0, 1.0}
    R.CHUNK_BRANCHES.clear()
    want_act, want_runs, want_rows = np.zeros((3, 5, 3), F), [], []
    for b in range(3):
        for c in range(5):
            want_act[b, c], rows = R.plan_chunk(hw[b, c], int(samples[b, c]), rcfg)
            for s, row in enumerate(rows):
                if row is not None:
                    want_runs.append((b, c, s))
                    want_rows.append(row)
    act, runs, rows = fa.online_chunk_plan(w, samples, config=cfg, ctx=gpu_ctx)
    assert R.bits(act.cpu().numpy()).tolist() == R.bits(want_act).tolist()
    assert [tuple(int(x) for x in r) for r in runs.tolist()] == want_runs
    assert R.bits(rows.cpu().numpy()).tolist() == R.bits(np.array(want_rows, F).reshape(-1, frames)).tolist()
    taken = dict(R.CHUNK_BRANCHES)
    assert taken.get("run", 0) > 0 and (frames == 1 or (taken.get("row_zero", 0) > 0 and taken.get("row_repeat", 0) > 0 and taken.get("no_run", 0) > 0)), taken
    act2, runs2, rows2 = fa.online_chunk_plan(w, None, config=cfg, ctx=gpu_ctx)          # NULL: chunk_samples everywhere
    assert len(runs2) == len(runs) and R.bits(act2.cpu().numpy()).tolist() == R.bits(want_act).tolist()
    masks = [R.clean_masks(hw[b, c])[s] for b, c, s in want_runs]
    assert R.bits(rows2.cpu().numpy()).tolist() == R.bits(np.array(masks, F).reshape(-1, frames)).tolist()


@pytest.mark.parametrize("chunk_samples", (1000, 1003, 7))
def test_pack_both_modes_at_ragged_lengths(fa, gpu_ctx, chunk_samples):
    import torch
    rng = np.random.default_rng(chunk_samples)
    lengths = np.array([0, 1, 5, 7, 333, chunk_samples - 1, chunk_samples, chunk_samples + 3], np.int32)
    offsets = np.concatenate([[3], 3 + np.cumsum(lengths[:-1] + 1)]).astype(np.int64)     # odd offsets: the sources are not 16-byte aligned
    audio = rng.standard_normal(int(offsets[-1] + lengths[-1] + 5)).astype(F)
    dev = torch.from_numpy(audio).cuda()
    for mode, repeat in ((fa.ONLINE_PACK_ZERO_TAIL, False), (fa.ONLINE_PACK_REPEAT, True)):
        got = fa.online_pack_waveforms(dev, offsets, lengths, chunk_samples, mode, ctx=gpu_ctx).cpu().numpy()
        want = np.stack([R.pack_waveform(audio[o:o + n], chunk_samples, repeat) for o, n in zip(offsets, lengths)])
        assert R.bits(got).tolist() == R.bits(want).tolist()


def finish_case(frames, chunks, seed, B=3):
    """B streams: weights (soft, hard, crafted first chunk), embeddings (voices with noise, a zero row, a row under the magnitude),
    offsets (0 for the first chunk), and the restatement's records, assignments and state."""
    rng = np.random.default_rng(seed)
    kw = cfg_for(frames)
    rcfg = R.ChunkConfig(**kw)
    ar = R.Arith(R.dot256)
    mgrs = [R.SpeakerManager(ar, max_speakers=4, raw_capacity=3, min_speech_duration=0.1) for _ in range(B)]
    voices = [unit(rng) for _ in range(4)]
    w = np.zeros((B, chunks, frames, 3), F)
    emb = np.zeros((B, chunks, 3, 256), F)
    off = np.zeros((B, chunks))
    want_seg, want_assign, want_counts = [], np.zeros((B, chunks, 3), [("id", np.int32), ("slot", np.int32), ("kind", np.int32), ("distance", np.uint32)]), \
        np.zeros((B, chunks), np.int32)
    for b in range(B):
        for c in range(chunks):
            is_crafted = b == 2 and c == 0 and frames >= 16
            w[b, c] = crafted(frames) if is_crafted else draw_weights(rng, frames, soft=b == 0)
            off[b, c] = 0.0 if c == 0 else c * 10.0 + b * 0.37
            for s in range(3):
                u = 1.0 if is_crafted else rng.random()
                emb[b, c, s] = 0 if u < 0.1 else voices[0] * F(0.05) if u < 0.2 else F(3.0) * (voices[rng.integers(4)] + F(0.2) * unit(rng))
            segs, assigns = R.finish_chunk(mgrs[b], w[b, c], emb[b, c], off[b, c], rcfg, tick=7)
            want_seg += to_bits_records(segs, b, c)
            want_assign[b, c] = assigns
            want_counts[b, c] = len(segs)
    return kw, w, emb, off, want_seg, want_assign, want_counts, mgrs


@pytest.fixture(scope="module")
def finish_cases():
    R.CHUNK_BRANCHES.clear()
    cases = {(frames, chunks): finish_case(frames, chunks, 1000 + frames * 7 + chunks) for frames in FRAMES for chunks in (1, 4)}
    cases["branches"] = dict(R.CHUNK_BRANCHES)
    return cases


def test_the_finish_inputs_reach_every_branch(finish_cases):
    taken = finish_cases["branches"]
    print(taken)
    names = [n for n in R.CHUNK_BRANCH_NAMES if not n.startswith(("row_", "run", "no_run"))]
    assert all(taken.get(n, 0) > 0 for n in names), {n: taken.get(n, 0) for n in names}


def device_state(db, b):
    return [(sp.id, sp.slot, R.bits(sp.current_embedding).tolist(), [R.bits(r).tolist() for r in sp.raw_embeddings], R.bits1(sp.duration), sp.update_count,
             sp.created_tick, sp.updated_tick) for sp in (db.get(b, i) for i in db.ids(b))]


def restated_state(m):
    return [(sp.id, s, R.bits(sp.current).tolist(), [R.bits(r.embedding).tolist() for r in sp.raws], R.bits1(sp.duration), sp.update_count, sp.created, sp.updated)
            for s, sp in m.speakers()]


@pytest.mark.parametrize("chunks", (1, 4))
@pytest.mark.parametrize("frames", FRAMES)
def test_finish_equals_the_restatement(fa, gpu_ctx, finish_cases, frames, chunks):
    import torch
    kw, w, emb, off, want_seg, want_assign, want_counts, mgrs = finish_cases[(frames, chunks)]
    cfg = fa.OnlineChunkConfig(**kw)
    dw, de = torch.from_numpy(w).cuda(), torch.from_numpy(emb).cuda()
    act, _, _ = fa.online_chunk_plan(dw, None, config=cfg, ctx=gpu_ctx)
    for capacity in (len(want_seg) - 1, None):
        db = fa.SpeakerDatabase(3, fa.SpeakerDbConfig(max_speakers=4, raw_capacity=3, min_speech_duration=0.1), ctx=gpu_ctx)
        try:
            if capacity is not None:
                if capacity < 0:
                    continue
                with pytest.raises(fa.FluidAudioHipError) as err:                       # one record short: the count is set all the same
                    fa.online_chunk_finish(db, dw, act, de, off, config=cfg, tick=7, capacity=capacity)
                assert err.value.status == fa._lib.OUTPUT_TOO_SMALL and err.value.count == len(want_seg)
                continue
            seg, assign, counts = fa.online_chunk_finish(db, dw, act, de, off, config=cfg, tick=7)
            assert assign["id"].tolist() == want_assign["id"].tolist() and assign["slot"].tolist() == want_assign["slot"].tolist()
            assert assign["kind"].tolist() == want_assign["kind"].tolist() and assign["distance"].view(np.uint32).tolist() == want_assign["distance"].tolist()
            assert counts.tolist() == want_counts.tolist()
            assert seg_tuples(seg) == want_seg
            for b in range(3):
                assert device_state(db, b) == restated_state(mgrs[b])
        finally:
            db.close()


@pytest.mark.parametrize("streams,chunks", ((85, 1), (43, 2), (171, 1), (128, 2)))
def test_plan_scans_more_triples_than_one_pass_holds(fa, gpu_ctx, streams, chunks):
    """255, 258, 513 and 768 (stream, chunk, speaker) triples — a triple count is a multiple of 3, so these are the counts next to one
    pass of the 256-thread scan, one past two passes, and three whole passes.  One frame per chunk: a speaker runs when it alone is
    active.  Triples 254 and 256 (round the end of the first pass) are made to run where they exist, and so is one of the last chunk."""
    import torch
    frames = FRAMES[0]
    rng = np.random.default_rng(streams * 10 + chunks)
    kw = cfg_for(frames)
    cfg, rcfg = fa.OnlineChunkConfig(**kw), R.ChunkConfig(**kw)
    full, n = kw["chunk_samples"], streams * chunks
    hw = (rng.random((n, frames, 3)) < 0.4).astype(F)
    for chunk, speaker in ((n - 1, 2), (84, 2), (85, 1)):
        if chunk < n:
            hw[chunk] = 0
            hw[chunk, :, speaker] = 1
    hw = hw.reshape(streams, chunks, frames, 3)
    samples = rng.choice(np.array([1, full // 2, full - 1, full], np.int32), (streams, chunks))
    want_act, want_runs, want_rows = np.zeros((streams, chunks, 3), F), [], []
    for b in range(streams):
        for c in range(chunks):
            want_act[b, c], rows = R.plan_chunk(hw[b, c], int(samples[b, c]), rcfg)
            for s, row in enumerate(rows):
                if row is not None:
                    want_runs.append((b, c, s))
                    want_rows.append(row)
    flat = [(b * chunks + c) * 3 + s for b, c, s in want_runs]
    assert 20 < len(flat) < n * 3 and all(t in flat for t in (254, 256) if t < n * 3) and flat[-1] >= n * 3 - 3   # the inputs
    act, runs, rows = fa.online_chunk_plan(torch.from_numpy(hw).cuda(), samples, config=cfg, ctx=gpu_ctx)
    assert R.bits(act.cpu().numpy()).tolist() == R.bits(want_act).tolist()
    assert [tuple(int(x) for x in r) for r in runs.tolist()] == want_runs
    assert R.bits(rows.cpu().numpy()).tolist() == R.bits(np.array(want_rows, F).reshape(-1, frames)).tolist()


@pytest.mark.parametrize("streams,chunks", ((128, 2), (257, 1), (129, 2)))
def test_finish_scans_more_chunks_than_one_pass_holds(fa, gpu_ctx, streams, chunks):
    """256, 257 and 258 (stream, chunk) pairs: the scan of the chunks' segment counts fills one pass of its 256 threads exactly, and runs
    one and two pairs into a second.  17 frames a chunk, the smallest size class whose chunks keep segments."""
    import torch
    frames, n = 17, streams * chunks
    kw, w, emb, off, want_seg, want_assign, want_counts, mgrs = finish_case(frames, chunks, 77 + n, B=streams)
    flat_counts = want_counts.reshape(-1)
    assert len(want_seg) > 256 and flat_counts[:256].sum() > 0 and (n == 256 or flat_counts[256:].sum() > 0)   # the inputs
    cfg = fa.OnlineChunkConfig(**kw)
    dw, de = torch.from_numpy(w).cuda(), torch.from_numpy(emb).cuda()
    act, _, _ = fa.online_chunk_plan(dw, None, config=cfg, ctx=gpu_ctx)
    config = fa.SpeakerDbConfig(max_speakers=4, raw_capacity=3, min_speech_duration=0.1)
    short = fa.SpeakerDatabase(streams, config, ctx=gpu_ctx)
    try:
        with pytest.raises(fa.FluidAudioHipError) as err:                               # one record short: the count is still the full one
            fa.online_chunk_finish(short, dw, act, de, off, config=cfg, tick=7, capacity=len(want_seg) - 1)
        assert err.value.status == fa._lib.OUTPUT_TOO_SMALL and err.value.count == len(want_seg)
    finally:
        short.close()
    db = fa.SpeakerDatabase(streams, config, ctx=gpu_ctx)
    try:
        seg, assign, counts = fa.online_chunk_finish(db, dw, act, de, off, config=cfg, tick=7)
        assert assign["id"].tolist() == want_assign["id"].tolist() and assign["slot"].tolist() == want_assign["slot"].tolist()
        assert assign["kind"].tolist() == want_assign["kind"].tolist() and assign["distance"].view(np.uint32).tolist() == want_assign["distance"].tolist()
        assert counts.tolist() == want_counts.tolist()
        assert seg_tuples(seg) == want_seg
        for b in (0, 2, streams - 1):
            assert device_state(db, b) == restated_state(mgrs[b])
    finally:
        db.close()


def test_end_to_end_eight_streams_of_five_chunks(fa, gpu_ctx):
    """plan -> a stand-in network (a fixed random projection of the masked audio, in torch on the device) -> finish, against the restatement's
    performCompleteDiarization loop record for record; one chunks = 5 call and five chunks = 1 calls give the same records and state."""
    import torch
    B, Cn, frames, spf = 8, 5, 65, 16
    chunk = frames * spf
    kw = dict(frames=frames, chunk_samples=chunk, min_active_frames=10.0, min_speech_duration=float(F(16.0 * STEP)))
    cfg, rcfg = fa.OnlineChunkConfig(**kw), R.ChunkConfig(**kw)
    rng = np.random.default_rng(5)
    lengths = rng.integers(Cn * chunk - chunk + 1, Cn * chunk + 1, B)                  # ragged recordings: the last chunk is short
    starts = np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64)
    audio = torch.from_numpy(rng.standard_normal(int(lengths.sum())).astype(F)).cuda()
    offsets = np.array([[starts[b] + c * chunk for c in range(Cn)] for b in range(B)], np.int64).reshape(-1)
    rows_len = np.array([[min(chunk, lengths[b] - c * chunk) for c in range(Cn)] for b in range(B)], np.int32)
    wave = fa.online_pack_waveforms(audio, offsets, rows_len.reshape(-1), chunk, fa.ONLINE_PACK_ZERO_TAIL, ctx=gpu_ctx).reshape(B, Cn, chunk)
    w = np.stack([np.stack([draw_weights(rng, frames, soft=bool(b & 1)) for _ in range(Cn)]) for b in range(B)])
    dw = torch.from_numpy(w).cuda()
    act, runs, rows = fa.online_chunk_plan(dw, rows_len, config=cfg, ctx=gpu_ctx)
    proj = torch.from_numpy(rng.standard_normal((chunk, 256)).astype(F) / 8).cuda()
    de = torch.zeros((B, Cn, 3, 256), dtype=torch.float32, device="cuda")
    for k, (b, c, s) in enumerate(runs.tolist()):                                       # the stand-in network, one run at a time
        de[b, c, s] = (wave[b, c] * rows[k].repeat_interleave(spf)) @ proj
    emb = de.cpu().numpy()
    off = np.array([[c * chunk / 16000.0 for c in range(Cn)] for _ in range(B)])
    ar = R.Arith(R.dot256)
    mgrs = [R.SpeakerManager(ar, max_speakers=6, raw_capacity=3, min_speech_duration=0.1) for _ in range(B)]
    want, want_runs = [], []
    for b in range(B):
        for c in range(Cn):
            _, mask_rows = R.plan_chunk(w[b, c], int(rows_len[b, c]), rcfg)
            want_runs += [(b, c, s) for s, row in enumerate(mask_rows) if row is not None]
            segs, _ = R.finish_chunk(mgrs[b], w[b, c], emb[b, c], off[b, c], rcfg, tick=c)
            want += to_bits_records(segs, b, c)
    assert [tuple(int(x) for x in r) for r in runs.tolist()] == want_runs and len(want) > 10
    one = fa.SpeakerDatabase(B, fa.SpeakerDbConfig(max_speakers=6, raw_capacity=3, min_speech_duration=0.1), ctx=gpu_ctx)
    five = fa.SpeakerDatabase(B, fa.SpeakerDbConfig(max_speakers=6, raw_capacity=3, min_speech_duration=0.1), ctx=gpu_ctx)
    try:
        got = []
        for c in range(Cn):                                                            # the live shape: a call per chunk, the tick = the chunk
            seg, _, _ = fa.online_chunk_finish(five, dw[:, c:c + 1].contiguous(), act[:, c:c + 1].contiguous(), de[:, c:c + 1].contiguous(), off[:, c:c + 1],
                                               config=cfg, tick=c)
            seg["chunk"] = c
            got += seg_tuples(seg)
        assert sorted(got) == sorted(want) and [g for g in got if g[0] == 3] == [x for x in want if x[0] == 3]
        for b in range(B):
            assert device_state(five, b) == restated_state(mgrs[b])
        # one call for the whole recording: the same records (in stream, chunk order) and, ticks apart, the same state
        seg, _, _ = fa.online_chunk_finish(one, dw, act, de, off, config=cfg, tick=0)
        assert seg_tuples(seg) == want
        strip = lambda st: [x[:6] for x in st]  # noqa: E731
        for b in range(B):
            assert strip(device_state(one, b)) == strip(restated_state(mgrs[b]))
    finally:
        one.close()
        five.close()
