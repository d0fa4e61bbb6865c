"""The streaming Sortformer state on the device (fa_sortformer_stream_*: csrc/sortformer_stream.hip, csrc/sortformer_stream_host.hip) against
the line-by-line restatement (tests/sortformer_stream_restatement.py) on the shared cases (tests/sortformer_stream_cases.py).

After every step every stream's whole state (read back with get: both slabs with their zero rows, both pred arrays and their flags, the
lengths, the silence mean and count), the confirmed / tentative rows, their counts and the statuses are compared with ==.  The restatement
is advanced on the same operands with log_scores = the rows the device wrote: the base scores go through a log, which no two libraries
round alike, so they are held to a float64 yardstick instead — within 4 times the largest error a float32 emulation in the same
operation order shows on the same cases (two fp32 logs, each good to about an ulp, can differ by a few ulp over the S + 2 summed terms).
Everything behind the base scores is IEEE add / multiply / divide and comparisons and has no tolerance.
The same file is run on the poisoned-workspace library (make POISON=1)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sortformer_stream_cases as K  # noqa: E402
import sortformer_stream_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32


def fa_config(fa, cfg: R.Config):
    return fa.SortformerStreamConfig(**{f: getattr(cfg, f) for f in ("speakers", "d_model", "chunk_len", "chunk_left_context", "chunk_right_context", "fifo_len", "spkcache_len",
                                                                       "spkcache_update_period", "sil_frames_per_spk", "max_index", "max_chunk_frames", "subsampling", "n_mels",
                                                                       "silence_threshold", "pred_score_threshold", "scores_boost_latest", "strong_boost_rate", "weak_boost_rate",
                                                                       "min_pos_scores_rate")})


def padded(rows, n, width):
    out = np.zeros((n, width), F)
    if rows is not None and len(rows):
        out[:len(rows)] = rows
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def state_differences(cfg, snap, state: R.State):
    """The fields in which a stream's device state (a snapshot) differs from the restatement's."""
    want = {"spkcache_length": state.spkcache_length, "fifo_length": state.fifo_length, "spkcache_preds_present": state.spkcache_preds is not None,
            "fifo_preds_present": state.fifo_preds is not None, "silence_frame_count": state.silence_frame_count}
    bad = [k for k, v in want.items() if getattr(snap, k) != v]
    arrays = {"spkcache": padded(state.spkcache, cfg.spkcache_len, cfg.d_model), "spkcache_preds": padded(state.spkcache_preds, cfg.spkcache_len, cfg.speakers),
              "fifo": padded(state.fifo, cfg.fifo_len, cfg.d_model), "fifo_preds": padded(state.fifo_preds, cfg.fifo_len, cfg.speakers), "mean_silence": state.mean_silence}
    return bad + [k for k, v in arrays.items() if not same_bits(getattr(snap, k), v)]


def run_case(fa, ctx, case: K.Case):
    import torch
    cfg, steps = K.operands(case)
    dev = f"cuda:{ctx.device}"
    B = case.streams
    st = fa.SortformerStreamState(B, fa_config(fa, cfg), ctx)
    states = [R.State(cfg.d_model, cfg.speakers) for _ in range(B)]
    pointers = st.input_pointers()
    res = dict(mismatches=[], compressions=0, dev_err=0.0, emu_err=0.0, refused=0, advanced_beside_refusal=0, regimes=set(), pointers_fixed=True, steps=0)
    out = None
    for t, step in enumerate(steps):
        embs = torch.from_numpy(step.chunk).to(dev)
        if case.f16:
            embs = embs.half()   # the rows are multiples of 1/64 below 4 in magnitude: exact in fp16
        ops = [torch.from_numpy(x).to(dev) for x in (step.emb_len, step.preds, step.pred_rows, step.left, step.right, step.active)]
        out = st.update_dev(embs, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], log_scores=True, out=out)
        ctx.synchronize()
        status, counts = out.status.cpu().numpy(), out.counts.cpu().numpy()
        conf, tent, scores = out.confirmed.cpu().numpy(), out.tentative.cpu().numpy(), out.log_scores.cpu().numpy()
        modes = set()
        for b in range(B):
            before = (states[b].spkcache_length, states[b].fifo_length)
            want_status, want_conf, want_tent, base = K.advance(cfg, states[b], step, b, log_scores=scores[b])
            where = f"{case.name} step {t} stream {b}"
            if status[b] != want_status or status[b] != step.expect[b]:
                res["mismatches"].append(f"{where}: status {status[b]}, restatement {want_status}, injected {step.expect[b]}")
            if want_status == R.OK:
                if counts[b].tolist() != [len(want_conf), len(want_tent)] or not same_bits(conf[b, :len(want_conf)], want_conf) or not same_bits(tent[b, :len(want_tent)], want_tent):
                    res["mismatches"].append(f"{where}: confirmed / tentative rows")
                modes.add("compress" if base is not None else "pop" if states[b].spkcache_length != before[0] else "append")
            elif counts[b].tolist() != [0, 0]:
                res["mismatches"].append(f"{where}: counts of a refused stream {counts[b].tolist()}")
            if base is not None:   # every compression step is compared, and its base scores are held to the yardstick
                res["compressions"] += 1
                P = states[b].scored_preds
                ref = R.log_scores_f64(cfg, P)
                res["dev_err"] = max(res["dev_err"], float(np.max(np.abs(scores[b, :len(P)].astype(np.float64) - ref))))
                res["emu_err"] = max(res["emu_err"], float(np.max(np.abs(R.log_scores_f32(cfg, P).astype(np.float64) - ref))))
            diff = state_differences(cfg, st.get(b), states[b])   # a refused or inactive stream: the state the last step left, bit for bit
            if diff:
                res["mismatches"].append(f"{where} (status {want_status}): {diff}")
            if want_status not in (R.OK, R.INACTIVE):
                res["refused"] += 1
                res["advanced_beside_refusal"] += int(any(step.expect[o] == R.OK for o in range(B) if o != b))
        res["regimes"].add(frozenset(modes))
        res["pointers_fixed"] = res["pointers_fixed"] and st.input_pointers() == pointers
        res["steps"] += 1
        if len(res["mismatches"]) > 5:
            break
    st.close()
    return res


@pytest.fixture(scope="module")
def runs(fa, gpu_ctx):
    done = {}

    def get(case):
        if case.name not in done:
            done[case.name] = run_case(fa, gpu_ctx, case)
        return done[case.name]
    return get


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_every_step_equals_the_restatement(runs, case):
    res = runs(case)
    assert not res["mismatches"], res["mismatches"]
    assert res["steps"] == case.steps and res["compressions"] > 0 and res["pointers_fixed"]


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_base_scores_are_within_four_times_the_emulations_error(runs, case):
    res = runs(case)
    emu = max(runs(c)["emu_err"] for c in K.CASES)   # the bound comes from the emulation on the same cases, never from the device
    print(f"{case.name}: device max |error| {res['dev_err']:.3e}, float32 emulation max |error| {res['emu_err']:.3e} (all cases {emu:.3e}), bound {4 * emu:.3e}")
    assert res["compressions"] > 0 and emu > 0
    assert res["dev_err"] <= 4 * emu, (res["dev_err"], emu)


def test_refused_streams_stay_put_while_their_neighbours_advance_and_one_call_holds_all_regimes(runs):
    small = [runs(c) for c in K.CASES if c.streams == 5]
    assert all(r["refused"] == len(K.REFUSALS) and r["advanced_beside_refusal"] == r["refused"] and not r["mismatches"] for r in small)
    assert any(len(m) == 3 for r in small for m in r["regimes"])


def crafted(cfg, kind, rng):
    """A state put together by hand: a full cache and a full FIFO, so that the next chunk pops and compresses."""
    S, D = cfg.speakers, cfg.d_model
    level = {"ties": F(0.75), "silent": F(0.4), "capacity": None}[kind]
    draw = (lambda n: np.full((n, S), level, F)) if level is not None else (lambda n: rng.random((n, S), dtype=F))
    rows = lambda n: (rng.integers(-256, 257, (n, D)) / 64).astype(F)  # noqa: E731
    state = R.State(D, S, spkcache=rows(cfg.spkcache_len), spkcache_preds=None if kind == "capacity" else draw(cfg.spkcache_len), fifo=rows(cfg.fifo_len),
                    fifo_preds=draw(cfg.fifo_len), mean_silence=rows(1)[0], silence_frame_count=5)
    emb_len = cfg.chunk_left_context + cfg.chunk_len + cfg.chunk_right_context
    return state, rows(emb_len), draw(cfg.spkcache_len + cfg.fifo_len + emb_len)


def test_crafted_states_through_set_and_the_host_entry(fa, gpu_ctx):
    """All preds equal (every comparison a tie), all preds <= 0.5 (every slot disabled: the whole cache is the silence mean), a state exactly at
    capacity whose preds are still absent (the first overflow of a non-empty cache).  Three streams of one state object, one host-pointer call."""
    cfg = K.geometry("small")
    rng = np.random.default_rng(21)
    kinds = ("ties", "silent", "capacity")
    st = fa.SortformerStreamState(3, fa_config(fa, cfg), gpu_ctx)
    states, chunks, preds = zip(*(crafted(cfg, k, rng) for k in kinds))
    for b, s in enumerate(states):
        st.set(b, fa.SortformerStreamSnapshot(s.spkcache_length, s.fifo_length, s.spkcache_preds is not None, True, s.silence_frame_count, s.spkcache,
                                              padded(s.spkcache_preds, cfg.spkcache_len, cfg.speakers), s.fifo, s.fifo_preds, s.mean_silence))
        assert not state_differences(cfg, st.get(b), s), kinds[b]
    M = cfg.max_chunk_frames
    conf, tent, counts, status, scores = st.update(np.stack(chunks), [M] * 3, np.stack(preds), [preds[0].shape[0]] * 3, [cfg.chunk_left_context] * 3,
                                                   [cfg.chunk_right_context] * 3, log_scores=True)
    assert status.tolist() == [R.OK] * 3 and counts.tolist() == [[cfg.chunk_len, cfg.chunk_right_context]] * 3
    for b, s in enumerate(states):
        want_conf, want_tent, base = R.streaming_update(cfg, s, chunks[b], preds[b], cfg.chunk_left_context, cfg.chunk_right_context, log_scores=scores[b])
        assert base is not None and same_bits(conf[b, :cfg.chunk_len], want_conf) and same_bits(tent[b, :cfg.chunk_right_context], want_tent), kinds[b]
        assert not state_differences(cfg, st.get(b), s), kinds[b]
    silent = st.get(1)
    assert same_bits(silent.spkcache, np.tile(states[1].mean_silence, (cfg.spkcache_len, 1))) and not silent.spkcache_preds.any()
    # reset = cleanup(): one stream, its neighbours untouched
    st.reset(1)
    assert not state_differences(cfg, st.get(1), R.State(cfg.d_model, cfg.speakers)) and not state_differences(cfg, st.get(0), states[0])
    st.close()


def test_pack_and_the_plan_functions_reproduce_the_chunk_loop(fa, gpu_ctx):
    """Mel frames arriving a few at a time for three streams: fa_sortformer_stream_chunk_plan against getNextChunkFeaturesLocked, the packed rows
    against the buffer's frames with their zero tail, and fa_sortformer_stream_file_chunks against the loader."""
    import torch
    cfg = R.Config(speakers=4, d_model=24, chunk_len=3, chunk_left_context=1, chunk_right_context=2, fifo_len=5, spkcache_len=32, spkcache_update_period=4, subsampling=2, n_mels=6)
    fcfg = fa_config(fa, cfg)
    rng = np.random.default_rng(31)
    totals = [57, 40, 23]
    mel = [rng.standard_normal((n, cfg.n_mels)).astype(F) for n in totals]
    base = np.concatenate([[0], np.cumsum(totals)])[:3]
    d_mel = torch.from_numpy(np.concatenate(mel)).to(f"cuda:{gpu_ctx.device}")
    T = (cfg.chunk_len + cfg.chunk_left_context + cfg.chunk_right_context) * cfg.subsampling
    arrived, dropped, start, emitted = [0] * 3, [0] * 3, [0] * 3, 0
    for round_ in range(40):
        for b in range(3):
            arrived[b] = min(totals[b], arrived[b] + (5, 3, 7)[b])
        while True:
            buffered = [arrived[b] - dropped[b] for b in range(3)]
            got = fa.sortformer_stream_chunk_plan(buffered, start, fcfg)
            want = [R.next_chunk_features(cfg, buffered[b], start[b]) for b in range(3)]
            assert [tuple(int(x) for x in g) for g in got.tolist()] == [w.tuple() for w in want], round_
            if not any(w.ready for w in want):
                break
            rows = fa.sortformer_stream_pack_chunks(d_mel, base + np.array(dropped), got, fcfg, gpu_ctx).cpu().numpy()
            for b, w in enumerate(want):
                expect = np.zeros((T, cfg.n_mels), F)
                if w.ready:
                    expect[:w.rows] = mel[b][dropped[b] + w.start_frame:dropped[b] + w.start_frame + w.rows]
                    emitted += 1
                assert same_bits(rows[b], expect), (round_, b)
                dropped[b] += w.frames_to_drop
                start[b] = w.new_start_feat
    assert emitted > 10
    for feat, seq in ((0, 0), (5, 5), (57, 50), (100, 100), (333, 320)):
        num, chunks = fa.sortformer_stream_file_chunks(feat, seq, fcfg)
        want_num, want = R.file_chunks(cfg, feat, seq)
        assert num == want_num and [tuple(int(x) for x in c) for c in chunks.tolist()] == [w.tuple() for w in want], feat
