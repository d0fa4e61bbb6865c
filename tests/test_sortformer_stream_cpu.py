"""Streaming Sortformer's state without a GPU: the restatement (tests/sortformer_stream_restatement.py) against the reference's literal
tests (Tests/FluidAudioTests/Diarizer/Sortformer/SortformerStateUpdaterTests.swift), its two insertion loops against the rank orders the
kernels implement with keys, fluidaudio_amd/csrc/sortformer_stream_core.h under the address and undefined-behaviour sanitizers in a
stand-alone program against the restatement's integers, and the proof that the shared cases (tests/sortformer_stream_cases.py) together
contain every decision kind the GPU test is meant to cover."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sortformer_stream_cases as K  # noqa: E402
import sortformer_stream_restatement as R  # noqa: E402

F = np.float32


# ---- the reference's literal cases
def literal_config():
    """The literal tests size their chunk by config.coreFrames (chunkLen * subsamplingFactor = 48) + both contexts: 56 rows."""
    return R.Config(max_chunk_frames=6 * 8 + 1 + 7)


def test_insufficient_preds_is_the_short_preds_status():
    """testStreamingUpdateThrowsOnInsufficientPreds: a 56-row chunk and one float of preds (no whole row) -> insufficientPredsLength, here the
    short-preds status of the chunk rows; the state is untouched."""
    cfg = literal_config()
    state = R.State(cfg.d_model, cfg.speakers)
    preds = np.zeros(1, F)
    with pytest.raises(R.Refused) as e:
        R.streaming_update(cfg, state, np.zeros((56, 512), F), preds[:preds.size // 4 * 4].reshape(-1, 4), 1, 7)
    assert e.value.status == R.SHORT_PREDS_CHUNK
    assert state.fifo_length == 0 and state.fifo_preds is None


def test_basic_flow_gives_core_frames_times_speakers_confirmed_values():
    """testStreamingUpdateBasicFlow: 56 rows of chunk and of preds -> confirmed.count == coreFrames * numSpeakers = 48 * 4."""
    cfg = literal_config()
    state = R.State(cfg.d_model, cfg.speakers)
    conf, tent, _ = R.streaming_update(cfg, state, np.zeros((56, 512), F), np.zeros((56, 4), F), 1, 7)
    assert conf.size == 48 * 4 and tent.size == 7 * 4
    # 48 rows into a FIFO of 40: the period of 31 pops, all 31 frames are silent, nothing overflows
    assert state.fifo_length == 17 and state.spkcache_length == 31 and state.spkcache_preds is None and state.fifo_preds.shape == (17, 4)
    assert state.silence_frame_count == 31 and not state.mean_silence.any()


def test_config_clamps_and_defaults():
    c = R.Config(chunk_len=0, spkcache_len=3, spkcache_update_period=1000)
    assert (c.chunk_len, c.spkcache_len, c.spkcache_update_period) == (1, 16, 41)
    assert R.Config().quotas() == (44, 33, 66, 22) and R.Config(spkcache_len=16).quotas() == (1, 0, 1, 0)


# ---- the licence for the kernels' keys
def tied_and_random_columns():
    rng = np.random.default_rng(11)
    for n, levels in ((1, 2), (7, 2), (40, 3), (219, 5), (219, 0), (64, 1)):
        for _ in range(6):
            v = rng.standard_normal(n).astype(F) if levels == 0 else (rng.integers(0, levels, n) / 4).astype(F)
            v[rng.random(n) < 0.3] = R.NEG_INF
            yield v


def test_the_boost_insertion_loop_is_the_rank_order():
    for v in tied_and_random_columns():
        for k in (1, 2, 5, 33, 66, len(v), len(v) + 3):
            k_eff = min(k, len(v))
            assert sorted(R.boost_insertion(v, k_eff)) == sorted(R.boost_rank_order(v, k_eff)), (v, k)


def test_the_selection_insertion_loop_is_the_rank_order():
    rng = np.random.default_rng(12)
    for frames, S, levels in ((3, 1, 2), (9, 4, 2), (35, 4, 3), (35, 3, 0), (60, 2, 1), (100, 4, 4)):
        for k in (1, 4, 32, frames * S - 1, frames * S, frames * S + 5):
            sc = rng.standard_normal((frames, S)).astype(F) if levels == 0 else (rng.integers(0, levels, (frames, S)) / 4).astype(F)
            sc[rng.random((frames, S)) < 0.4] = R.NEG_INF
            sc[-3:] = R.POS_INF
            idx, val = R.topk_insertion(sc, frames, k)
            ridx, rval = R.topk_rank_order(sc, frames, k)
            assert idx == ridx and [float(x) for x in val] == [float(x) for x in rval], (frames, S, k)


# ---- the shared integers under the sanitizers
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sortformer_stream") / "sortformer_stream_core_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "sortformer_stream_core_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


GEOS = [(4, 188, 40, 6, 1, 7, 31, 3, 0.75, 1.5, 0.5), (4, 188, 188, 6, 1, 7, 144, 3, 0.75, 1.5, 0.5), (4, 188, 40, 340, 1, 40, 300, 3, 0.75, 1.5, 0.5),
        (4, 188, 40, 25, 1, 7, 31, 3, 0.75, 1.5, 0.5), (4, 32, 5, 3, 1, 2, 4, 3, 0.75, 1.5, 0.5), (2, 32, 5, 3, 1, 2, 4, 3, 0.3, 0.7, 0.9),
        (3, 32, 5, 3, 1, 2, 4, 3, 0.7, 1.1, 0.35), (4, 16, 5, 3, 1, 2, 4, 3, 0.75, 1.5, 0.5), (4, 3, 2, 0, 0, 0, 100, 3, 0.75, 1.5, 0.5),
        (1, 50, 7, 4, 2, 3, 1, 0, 0.1, 0.0, 1.0), (3, 100, 0, 5, 0, 0, 9, 1, 0.99, 2.5, 0.01)]


def plan_py(cfg, spk, fifo, present, emb, rows, stride, lc, rc):
    """plan_update by the restatement: status, mode, core, pop, new_fifo, new_spk, first_overflow, chunk_start."""
    refused = lambda s: (s, 0, 0, 0, fifo, spk, 0, 0)  # noqa: E731
    if rows < 0:
        return refused(R.BAD_OPERAND)
    state = R.State(cfg.d_model, cfg.speakers, spkcache=np.zeros((spk, cfg.d_model), F), fifo=np.zeros((fifo, cfg.d_model), F),
                    spkcache_preds=np.zeros((spk, cfg.speakers), F) if present else None)
    try:
        core, start = R.validate(cfg, state, emb, np.zeros((rows, cfg.speakers), F), lc, rc, stride)
    except R.Refused as e:
        core = emb - lc - rc if e.status in (R.SHORT_PREDS_CHUNK, R.SHORT_PREDS_TENTATIVE, R.NEGATIVE_CORE) else 0
        return (e.status, 0, core, 0, fifo, spk, 0, 0)
    context = core + fifo
    if context <= cfg.fifo_len:
        return (R.OK, 1, core, 0, context, spk, 0, start)
    pop = R.pop_out_length(cfg, context)
    if spk + pop > cfg.spkcache_len:
        return (R.OK, 3, core, pop, context - pop, cfg.spkcache_len, 0 if present else 1, start)
    return (R.OK, 2, core, pop, context - pop, spk + pop, 0, start)


def expected_lines():
    out = []
    for i, (S, cache, fifo, chunk, lc, rc, period, sil, strong, weak, minpos) in enumerate(GEOS):
        cfg = R.Config(speakers=S, d_model=8, chunk_len=chunk, chunk_left_context=lc, chunk_right_context=rc, fifo_len=fifo, spkcache_len=cache, spkcache_update_period=period,
                       sil_frames_per_spk=sil, strong_boost_rate=strong, weak_boost_rate=weak, min_pos_scores_rate=minpos)
        out.append(f"GEO {i} {cfg.chunk_len} {cfg.spkcache_len} {cfg.spkcache_update_period} 0")
        out.append("QUOTA " + " ".join(str(x) for x in cfg.quotas()))
        out.append(f"SLAB {cfg.max_pop} {cfg.score_rows} {cfg.fifo_len + cfg.max_chunk_frames} {(cfg.score_rows + sil) * S}")
        out.append("POP " + " ".join(str(R.pop_out_length(cfg, cfg.fifo_len + 1 + k)) for k in range(cfg.max_chunk_frames)))
        stride = cfg.spkcache_len + cfg.fifo_len + cfg.max_chunk_frames + 1
        for spk in (0, cfg.spkcache_len // 2, cfg.spkcache_len):
            for ff in (0, cfg.fifo_len // 2, cfg.fifo_len):
                for present in (0, 1):
                    for emb in (0, cfg.chunk_len + rc, cfg.max_chunk_frames, cfg.max_chunk_frames + 1):
                        for l in (0, lc, -1):
                            for r in (-1, rc):
                                for cut in (0, 1, rc + 1, emb + 1):
                                    rows = spk + ff + emb - cut
                                    out.append(f"PLAN {spk} {ff} {present} {emb} {l} {r} {rows} : " + " ".join(str(x) for x in plan_py(cfg, spk, ff, present, emb, rows, stride, l, r)))
        buffered = start = 0
        for _ in range(60):
            buffered += 13
            while True:
                k = R.next_chunk_features(cfg, buffered, start)
                if not k.ready:
                    break
                out.append("CHUNK " + " ".join(str(x) for x in k.tuple()))
                buffered -= k.frames_to_drop
                start = k.new_start_feat
        for feat in (0, 5, 100, 777, 3001):
            seq = feat - 9 if feat > 9 else feat
            num, chunks = R.file_chunks(cfg, feat, seq)
            out.append(f"FILE {feat} {seq} {num}" + "".join(f" {c.chunk_length},{c.left_offset},{c.right_offset},{c.start_frame},{c.rows},{c.new_start_feat}" for c in chunks) + f" | {len(chunks)}")
    return out


def test_the_shared_integers_equal_the_restatement_under_the_sanitizers(program):
    want = expected_lines()
    assert len(program) == len(want)
    for got, exp in zip(program, want):
        assert got == exp
    assert sum(l.startswith("CHUNK") for l in want) > 100 and any(l.startswith("PLAN") and " : 0 3 " in l for l in want)


# ---- the shared cases contain every decision kind
KINDS = ("append_only", "pop_no_overflow", "first_overflow_empty", "first_overflow_nonempty", "later_compression", "silent_frame", "quota_disabled", "boost_cuts",
         "neg_inf_selected", "frame_twice", "non_monotone", "tie_at_cut", "lc_zero") + tuple(f"refused_{s}" for s in K.REFUSALS)


@pytest.fixture(scope="module")
def taken():
    R.BRANCHES.clear()
    per_case = {}
    for case in K.CASES:
        before = dict(R.BRANCHES)
        cfg, steps = K.operands(case)
        states = [R.State(cfg.d_model, cfg.speakers) for _ in range(case.streams)]
        kinds_in_call = set()
        for step in steps:
            lengths = [(s.spkcache_length, s.fifo_length) for s in states]
            modes = set()
            for b, state in enumerate(states):
                snapshot = state.copy()
                status, conf, _, base = K.advance(cfg, state, step, b)
                assert status == step.expect[b], (case.name, b, status, step.expect[b])
                if status != R.OK:   # a refusal leaves the state as it was
                    assert (state.spkcache_length, state.fifo_length) == lengths[b] and np.array_equal(state.fifo, snapshot.fifo)
                else:
                    modes.add("compress" if base is not None else "pop" if state.spkcache_length != lengths[b][0] else "append")
                assert state.fifo_length <= cfg.fifo_len and state.spkcache_length <= cfg.spkcache_len
            kinds_in_call.add(frozenset(modes))
        per_case[case.name] = (kinds_in_call, {k: R.BRANCHES[k] - before.get(k, 0) for k in R.BRANCHES})
    return dict(R.BRANCHES), per_case


def test_the_shared_cases_contain_every_decision_kind(taken):
    total, per_case = taken
    print(total)
    missing = [k for k in KINDS if total.get(k, 0) == 0]
    assert not missing, missing
    # not through the degenerate 16-row cache, and the staggered streams put all three regimes into one call
    assert all(K.geometry(c.geometry).spkcache_len >= 32 for c in K.CASES)
    assert any({"append", "pop", "compress"} <= set().union(*calls) and any(len(m) == 3 for m in calls) for calls, _ in per_case.values())
    # every geometry compresses
    for case in K.CASES:
        got = per_case[case.name][1]
        assert got.get("first_overflow_empty", 0) + got.get("first_overflow_nonempty", 0) + got.get("later_compression", 0) > 0, case.name
