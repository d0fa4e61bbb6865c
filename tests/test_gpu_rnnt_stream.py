"""The Nemotron streaming session on the device (csrc/rnnt_stream.hip) against the restatement (tests/rnnt_stream_restatement.py, run in
the library's deferred order by tests/rnnt_stream_cases.py) on the scripted sessions of the cases module.  After every step every
stream's whole state (read back with get: the scalars, the span audio, the pre-roll tail, the mel cache), every output and every status is
compared with ==; floats as bits.  d_rms equals the library's host emulation bit for bit and lies within (n / 64 + 8) * 2^-24 (relative,
on the mean square) of the float64 value.  No other tolerance.  The same file is run on the poisoned-workspace library (make POISON=1).
What the cases contain is asserted without a GPU in test_rnnt_stream_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_stream_cases as K  # noqa: E402
import rnnt_stream_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32
OK, INACTIVE, BAD_OPERAND, TOO_SMALL, NO_LEXICAL = range(5)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def expectations():
    return {name: K.expected(sc) for name, sc in K.SCENARIOS.items()}


def state_differences(snap, s: R.Session):
    W = s.cfg.window_samples
    want = dict(frame_cursor=s.rescue_frame_cursor, span_open=int(s.span_open), span_start_frame=s.span_start_frame, span_last_speech_frame=s.span_last_speech_frame,
                span_speech_windows=s.span_speech_windows, span_pre_roll_frames=s.span_pre_roll_frames, silent_window_run=s.silent_window_run,
                span_overflowed=int(s.span_overflowed), span_samples=len(s.span_audio) * W, pre_roll_samples=len(s.pre_roll_tail) * W,
                vad_consecutive_low_chunks=s.vad_low, vad_skip_count=s.vad_skips, absolute_frame_base=s.absolute_frame_base, detected_blank_spans=s.detected,
                blank_rescues=s.rescued, mel_cache_frames=0 if s.mel_cache is None else s.mel_cache.shape[1])
    bad = [f"{k} {getattr(snap, k)} != {v}" for k, v in want.items() if getattr(snap, k) != v]
    cat = lambda ws: np.concatenate(ws) if ws else np.zeros(0, F)   # noqa: E731
    arrays = dict(span_audio=cat(s.span_audio), pre_roll=cat(s.pre_roll_tail), mel_cache=s.mel_cache if s.mel_cache is not None else np.zeros((s.cfg.mel_features, 0), F))
    return bad + [k for k, v in arrays.items() if not same_bits(getattr(snap, k), v)]


class Live:
    """The live token arrays, on the host and mirrored to the device."""

    def __init__(self, B, cap, dev):
        self.ids, self.frames, self.timed = np.zeros((B, cap), I), np.zeros((B, cap), I), np.zeros((B, cap), I)
        self.id_count, self.timed_count, self.dev = np.zeros(B, I), np.zeros(B, I), dev

    def append(self, b, tokens):
        for frame, token_id in tokens:
            self.ids[b, self.id_count[b]] = token_id
            self.id_count[b] += 1
            if frame is not None:
                self.frames[b, self.timed_count[b]], self.timed[b, self.timed_count[b]] = frame, token_id
                self.timed_count[b] += 1

    def upload(self):
        import torch
        self.d = [torch.from_numpy(x.copy()).to(self.dev) for x in (self.ids, self.frames, self.timed, self.id_count, self.timed_count)]
        return self.d

    def download(self):
        self.ids, self.frames, self.timed, self.id_count, self.timed_count = (x.cpu().numpy() for x in self.d)

    def differences(self, fa, b, s: R.Session):
        n, m = int(self.id_count[b]), int(self.timed_count[b])
        bad = [] if self.ids[b, :n].tolist() == s.ids else ["live ids"]
        if fa.rnnt_stream_seconds(self.frames[b, :m]).tolist() != [t.start_time for t in s.timings]:
            bad.append("live timings")
        if self.timed[b, :m].tolist() != [t.token_id for t in s.timings]:
            bad.append("live timed ids")
        return bad


def check_requests(where, sc, tracked, slots_of, want, request_capacity, arena_capacity, bad):
    """The records, the arena and the statuses of one track / finalize against the requests the restatement found."""
    count = int(tracked.request_count.cpu()[0])
    if count != len(want):
        bad.append(f"{where}: {count} requests, restatement {len(want)}")
        return
    records, arena, status = tracked.records(), tracked.arena.cpu().numpy(), tracked.status.cpu().numpy()
    at, short = 0, set()
    for i, q in enumerate(want):
        padded = q.padded(sc.rescue_chunk_samples)
        recorded = i < request_capacity
        placed = recorded and at + padded.size <= arena_capacity
        if recorded:
            r = records[i]
            got = (int(r["stream"]), int(r["span_start_frame"]), int(r["span_end_frame"]), int(r["speech_windows"]), int(r["audio_samples"]), int(r["decode_chunks"]),
                   int(r["status"]), int(r["audio_offset"]))
            exp = (q.stream, q.span_start_frame, q.span_end_frame, q.speech_windows, len(q.audio), q.decode_chunks(sc.rescue_chunk_samples), OK if placed else TOO_SMALL,
                   at if placed else -1)
            if got != exp:
                bad.append(f"{where}: request {i} {got} != {exp}")
            elif placed and not same_bits(arena[at:at + padded.size], padded):
                bad.append(f"{where}: request {i}: the arena's audio")
        if not placed:
            short.add(q.stream)
        at += padded.size
    for slot, b in slots_of:
        if status[slot] != (TOO_SMALL if b in short else OK):
            bad.append(f"{where}: status of stream {b} {status[slot]}")


def staged_arrays(sc, requests, capacity):
    ids, frames, nid, nfr = np.zeros((capacity, sc.staged_capacity), I), np.zeros((capacity, sc.staged_capacity), I), np.zeros(capacity, I), np.zeros(capacity, I)
    for r, q in enumerate(requests[:capacity]):
        a, b = K.stub_decoder(q)
        ids[r, :len(a)], frames[r, :len(b)], nid[r], nfr[r] = a, b, len(a), len(b)
    return ids, frames, nid, nfr


def run_scenario(fa, ctx, sc: K.Scenario, exp: K.Expected, stop_after=None, request_capacity=None, arena_capacity=None):
    import torch
    dev, B, cfg = f"cuda:{ctx.device}", sc.streams, sc.cfg
    rc = sc.request_capacity if request_capacity is None else request_capacity
    ac = sc.arena_capacity if arena_capacity is None else arena_capacity
    st = fa.RnntStreamState(B, fa.RnntStreamConfig(**vars(cfg)), ctx)
    d_class = torch.from_numpy(K.class_table()).to(dev)
    live, bad, rms_err = Live(B, sc.token_capacity, dev), [], 0.0
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731

    def merge(where, tracked, requests, commits):
        sid, sfr, nid, nfr = staged_arrays(sc, requests, rc)
        status = st.merge_rescued_dev(tracked, to(sid), to(sfr), to(nid), to(nfr), *live.d, d_class)
        ctx.synchronize()
        live.download()
        got = status.cpu().numpy()[:min(len(requests), rc)].tolist()
        if got != [OK if c else NO_LEXICAL for c in commits][:rc]:
            bad.append(f"{where}: request statuses {got}, commits {commits}")

    for t, step in enumerate(sc.steps):
        where = f"{sc.name} step {t}"
        chunk, mel = sc.chunk(t), sc.mel(t)
        active = step.active or [1] * B
        d_chunk, d_active = to(chunk), to(np.array(active, I)) if step.active else None
        # gate
        rms, skip, run_list, run_count, status = st.gate_dev(d_chunk, d_active)
        ctx.synchronize()
        skips, run = exp.gate[t]
        n_run = int(run_count.cpu()[0])
        if run_list.cpu().numpy()[:n_run].tolist() != run:
            bad.append(f"{where}: run list {run_list.cpu().numpy()[:n_run].tolist()} != {run}")
        for b in range(B):
            if status.cpu()[b] != (OK if active[b] else INACTIVE) or (active[b] and int(skip.cpu()[b]) != skips[b]):
                bad.append(f"{where}: gate of stream {b}")
            if active[b] and cfg.vad_rms_threshold > 0:
                got, want64 = rms.cpu().numpy()[b], R.rms64(chunk[b])
                if bits(got) != bits(fa.rnnt_stream_rms(chunk[b], gate=True)):
                    bad.append(f"{where}: rms of stream {b} is not the host emulation's")
                rms_err = max(rms_err, abs(float(got) ** 2 / want64 ** 2 - 1.0) / ((chunk.shape[1] / 64 + 8) * 2.0 ** -24))
        # mel_inputs, advance
        d_mel = to(mel)[:, :, ::step.mel_stride]
        rows, mstatus = st.mel_inputs_dev(d_mel, run_list, run_count)
        st.advance_dev(run_list, run_count, frames=sc.enc_frames)
        ctx.synchronize()
        if not same_bits(rows.cpu().numpy()[:n_run], exp.rows[t]) or mstatus.cpu().numpy()[:n_run].tolist() != [OK] * n_run:
            bad.append(f"{where}: mel rows")
        # the decode walk's tokens, track
        for b in range(B):
            live.append(b, step.tokens.get(b, []))
        d_live = live.upload()
        tracked = st.track_dev(d_chunk, d_live[1], d_live[2], d_live[4], d_class, sc.rescue_chunk_samples, rc, ac, d_active)
        ctx.synchronize()
        check_requests(where, sc, tracked, [(b, b) for b in range(B) if active[b]], exp.requests[t], rc, ac, bad)
        if [int(tracked.status.cpu()[b]) for b in range(B) if not active[b]] != [INACTIVE] * active.count(0):
            bad.append(f"{where}: an inactive stream's status")
        if stop_after == t:
            return bad, rms_err
        merge(where, tracked, exp.requests[t], exp.commits[t])
        for b in range(B):
            diff = state_differences(st.get(b), exp.states[t][b]) + live.differences(fa, b, exp.states[t][b])
            if diff:
                bad.append(f"{where} stream {b}: {diff}")
    if sc.finalize:
        where = f"{sc.name} finalize"
        streams = to(np.array(list(sc.finalize), I))
        tracked = st.finalize_dev(streams, to(np.array([len(sc.finalize)], I)), live.d[1], live.d[2], live.d[4], d_class, sc.rescue_chunk_samples, rc, ac)
        ctx.synchronize()
        check_requests(where, sc, tracked, list(enumerate(sc.finalize)), exp.final_requests, rc, ac, bad)
        merge(where, tracked, exp.final_requests, exp.final_commits)
        for b in range(B):
            diff = state_differences(st.get(b), exp.final_states[b]) + live.differences(fa, b, exp.final_states[b])
            if diff:
                bad.append(f"{where} stream {b}: {diff}")
    st.close()
    return bad, rms_err


@pytest.mark.parametrize("name", list(K.SCENARIOS))
def test_scenario_equals_the_restatement(fa, gpu_ctx, expectations, name):
    bad, rms_err = run_scenario(fa, gpu_ctx, K.SCENARIOS[name], expectations[name])
    assert not bad, bad[:6]
    assert rms_err <= 1.0, rms_err


def test_record_and_arena_capacity_one_short(fa, gpu_ctx, expectations):
    sc, exp = K.SCENARIOS["main"], expectations["main"]
    t = max(range(len(sc.steps)), key=lambda i: len(exp.requests[i]))
    want = exp.requests[t]
    assert len(want) >= 3
    bad, _ = run_scenario(fa, gpu_ctx, sc, exp, stop_after=t, request_capacity=len(want) - 1)
    assert not bad, bad[:6]
    total = sum(q.padded(sc.rescue_chunk_samples).size for q in want)
    bad, _ = run_scenario(fa, gpu_ctx, sc, exp, stop_after=t, request_capacity=len(want), arena_capacity=total - 1)
    assert not bad, bad[:6]


def test_get_set_reset_round_trip(fa, gpu_ctx, expectations):
    """A session restored on another handle continues bit for bit: the state after step 3 of `main`, set, then compared; reset clears it."""
    import torch
    sc, exp = K.SCENARIOS["main"], expectations["main"]
    a = fa.RnntStreamState(sc.streams, fa.RnntStreamConfig(**vars(sc.cfg)), gpu_ctx)
    b = fa.RnntStreamState(sc.streams, fa.RnntStreamConfig(**vars(sc.cfg)), gpu_ctx)
    d_class = torch.from_numpy(K.class_table()).cuda()
    empty, zero = torch.zeros((sc.streams, 1), dtype=torch.int32, device="cuda"), torch.zeros(sc.streams, dtype=torch.int32, device="cuda")
    for t in range(2):      # no tokens: only the span machine matters here
        a.track_dev(torch.from_numpy(sc.chunk(t)).cuda(), empty, empty, zero, d_class, sc.rescue_chunk_samples, 8, sc.arena_capacity)
    for s in range(sc.streams):
        snap = a.get(s)
        b.set(s, snap)
        again = b.get(s)
        assert all(getattr(snap, f) == getattr(again, f) for f in fa.rnnt_stream._INFO_FIELDS), s
        assert same_bits(snap.span_audio, again.span_audio) and same_bits(snap.pre_roll, again.pre_roll)
    chunk = torch.from_numpy(sc.chunk(2)).cuda()
    ta = a.track_dev(chunk, empty, empty, zero, d_class, sc.rescue_chunk_samples, 8, sc.arena_capacity)
    tb = b.track_dev(chunk, empty, empty, zero, d_class, sc.rescue_chunk_samples, 8, sc.arena_capacity)
    gpu_ctx.synchronize()
    ra, rb = ta.records(), tb.records()
    assert len(ra) > 0 and ra.tobytes() == rb.tobytes()
    n = int(ra["audio_offset"][-1] + ra["decode_chunks"][-1] * sc.rescue_chunk_samples)
    assert same_bits(ta.arena.cpu().numpy()[:n], tb.arena.cpu().numpy()[:n])
    b.reset(1)
    assert all(getattr(b.get(1), f) == 0 for f in fa.rnnt_stream._INFO_FIELDS) and b.get(0).frame_cursor == a.get(0).frame_cursor
    a.close(), b.close()


def test_gate_empty_chunk_and_host_twin(fa, gpu_ctx):
    """An empty chunk is silent: the counter runs, the second one skips and advances the base by 0 frames.  The host twin agrees."""
    import torch
    st = fa.RnntStreamState(3, fa.RnntStreamConfig(total_mel_frames=20, vad_rms_threshold=0.01), gpu_ctx)
    empty = torch.zeros((3, 0), dtype=torch.float32, device="cuda")
    first = [x.cpu().numpy().copy() for x in st.gate_dev(empty)]
    second = [x.cpu().numpy().copy() for x in st.gate_dev(empty)]
    assert first[1].tolist() == [0, 0, 0] and int(first[3][0]) == 3 and second[1].tolist() == [1, 1, 1] and int(second[3][0]) == 0
    loud = K.audio(["1111111", "0000000", "0000001"], 1280, 9)
    rms, skip, run, status = st.gate(loud, active=[1, 1, 0])
    assert skip.tolist()[:2] == [0, 1] and run.tolist() == [0] and status.tolist() == [0, 0, 1]
    assert bits(rms[0]) == bits(fa.rnnt_stream_rms(loud[0], gate=True)) and bits(rms[1]) == bits(fa.rnnt_stream_rms(loud[1], gate=True))
    snap = [st.get(b) for b in range(3)]
    assert [s.vad_consecutive_low_chunks for s in snap] == [0, 3, 2] and [s.vad_skip_count for s in snap] == [1, 2, 1] and [s.absolute_frame_base for s in snap] == [0, 7, 0]
    st.close()


MERGE_CASES = [
    # (live ids, live (frame, id) timings, staged ids, staged frames, span start, span end, merged ids, merged frames): the reference's four, on frames
    ([10, 20], [(12, 10), (62, 20)], [30], [37], 36, 40, [10, 30, 20], [12, 37, 62]),               # testMergeRescuedTokensInsertsAtTimestampPosition
    ([10], [(12, 10)], [30, 31], [37, 38], 36, 40, [10, 30, 31], [12, 37, 38]),                    # ...AppendsWhenSpanIsLatest
    ([K.TAG_EN, 10], [(62, 10)], [30], [25], 24, 30, [K.TAG_EN, 30, 10], [25, 62]),                # ...SkipsLeadingLangTag
    ([], [], [30], [6], 5, 9, [30], [6]),                                                         # ...EmptyLive
]


def test_merge_reference_cases_no_commit_and_capacity(fa, gpu_ctx):
    """The four testMergeRescuedTokens* cases as four streams of one call (host twin), beside: staged tokens that are all tags or all
    punctuation (no commit), a live capacity one short (nothing merged), a request whose counts disagree (refused)."""
    table = K.class_table()
    extra = [([10], [(12, 10)], [K.TAG_EN, K.TAG_DE], [], 1, 4, [10], [12]), ([10], [(12, 10)], [K.DOT, K.COMMA], [3, 4], 1, 4, [10], [12]),
             ([20, 21, 22, 23, 24], [(1, 20), (2, 21), (3, 22), (4, 23), (5, 24)], [30, 31], [2, 9], 1, 4, [20, 21, 22, 23, 24], [1, 2, 3, 4, 5]),
             ([10], [(12, 10)], [30, 31], [3], 1, 4, [10], [12])]
    cases = MERGE_CASES + extra
    B, cap = len(cases), 6
    st = fa.RnntStreamState(B, fa.RnntStreamConfig(total_mel_frames=20), gpu_ctx)
    req = np.zeros(B, fa.rnnt_stream.RNNT_STREAM_REQUEST_DTYPE)
    ids, frames, timed, idc, tc = np.full((B, cap), -7, I), np.full((B, cap), -7, I), np.full((B, cap), -7, I), np.zeros(B, I), np.zeros(B, I)
    sid, sfr, nid, nfr = np.zeros((B, 4), I), np.zeros((B, 4), I), np.zeros(B, I), np.zeros(B, I)
    for b, (lid, ltm, si, sf, start, end, _, _) in enumerate(cases):
        req[b]["stream"], req[b]["span_start_frame"], req[b]["span_end_frame"] = b, start, end
        ids[b, :len(lid)], idc[b], tc[b] = lid, len(lid), len(ltm)
        frames[b, :len(ltm)], timed[b, :len(ltm)] = [f for f, _ in ltm], [i for _, i in ltm]
        sid[b, :len(si)], sfr[b, :len(sf)], nid[b], nfr[b] = si, sf, len(si), len(sf)
    out_ids, out_frames, out_timed, out_idc, out_tc, status = st.merge_rescued(req, sid, sfr, nid, nfr, ids, frames, timed, idc, tc, table)
    assert status.tolist() == [OK] * 4 + [NO_LEXICAL, NO_LEXICAL, TOO_SMALL, BAD_OPERAND]
    for b, (lid, ltm, si, sf, start, end, want_ids, want_frames) in enumerate(cases):
        assert out_ids[b, :out_idc[b]].tolist() == want_ids and out_frames[b, :out_tc[b]].tolist() == want_frames, b
        assert (out_ids[b, out_idc[b]:] == -7).all() and (out_frames[b, out_tc[b]:] == -7).all(), b
        # the restatement on the reference's doubles
        s = R.Session(R.Config(), table, ids=list(lid), timings=[R.Timing(i, f * R.SECONDS_PER_FRAME) for f, i in ltm])
        if status[b] in (OK, NO_LEXICAL):
            s.commit(R.Request(b, start, end, 2, np.zeros(0, F)), si, sf)
        assert s.ids == want_ids and [t.start_time for t in s.timings] == fa.rnnt_stream_seconds(out_frames[b, :out_tc[b]]).tolist()
        assert [t.token_id for t in s.timings] == out_timed[b, :out_tc[b]].tolist()
    assert [st.get(b).blank_rescues for b in range(B)] == [1] * 4 + [0] * 4
    st.close()


def test_mel_stream_left_out_and_bad_slot(fa, gpu_ctx):
    """A stream that is not listed keeps its cache; a slot naming a stream outside the state is refused and nothing is written for it."""
    import torch
    cfg = fa.RnntStreamConfig(total_mel_frames=12, mel_features=3, pre_encode_cache=4)
    st = fa.RnntStreamState(3, cfg, gpu_ctx)
    rng = np.random.default_rng(5)
    m0, m1 = rng.standard_normal((3, 3, 8)).astype(F), rng.standard_normal((3, 3, 8)).astype(F)
    every, one = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda"), torch.tensor([2, 7, 0], dtype=torch.int32, device="cuda")
    st.mel_inputs_dev(torch.from_numpy(m0).cuda(), every, torch.tensor([3], dtype=torch.int32, device="cuda"))
    rows, status = st.mel_inputs_dev(torch.from_numpy(m1).cuda(), one, torch.tensor([2], dtype=torch.int32, device="cuda"))
    gpu_ctx.synchronize()
    want = np.zeros((3, 12), F)
    want[:, :4], want[:, 4:] = m0[2][:, 4:], m1[2]
    assert status.cpu().numpy()[:2].tolist() == [OK, BAD_OPERAND] and same_bits(rows.cpu().numpy()[0], want)
    assert same_bits(st.get(2).mel_cache, m1[2][:, 4:]) and same_bits(st.get(0).mel_cache, m0[0][:, 4:]) and same_bits(st.get(1).mel_cache, m0[1][:, 4:])
    st.close()
