"""The online speaker database on the device (fa_speaker_db_*: csrc/online.hip, csrc/online_host.hip) against the line-by-line
restatement of the reference (tests/online_restatement.py) with the library's dot256.  No tolerances: integers as they are, fp32 as bits.
Several successive calls per database, so state carries across launches; between them the management entries.  The same file is run on
the poisoned-workspace library (make POISON=1).  Every expectation is computed once per module, on the CPU, before anything is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
CALLS = 4
# streams, max_speakers, raw_capacity, per, validate_min_magnitude: every listed size occurs; validation on (DiarizerManager) and off (SpeakerManager)
CASES = {
    "one": (1, 1, 1, 1, -1.0),
    "small": (3, 2, 3, 3, 0.1),
    "ring50": (3, 5, 50, 7, -1.0),
    "many_streams": (130, 5, 3, 3, 0.1),
    "all_slots": (3, 64, 1, 7, -1.0),
}


def unit(rng):
    v = rng.standard_normal(256).astype(F)
    return v / F(np.sqrt(np.sum(v.astype(np.float64) ** 2)))


def draw_item(rng, voices, prev):
    """A few unit voices plus noise at scales that put the distance below 0.45, between 0.45 and 0.65 and above 0.65; exact duplicates, zero
    vectors, a magnitude just under 0.1, a NaN, a vector too small to carry energy; durations on both sides of the minimum; skips."""
    u = rng.random()
    if u < 0.05 and prev is not None:
        e = prev.copy()
    elif u < 0.08:
        e = np.zeros(256, F)
    elif u < 0.11:
        e = voices[0] * F(0.0999)
    elif u < 0.14:
        e = voices[0].copy()
        e[rng.integers(256)] = np.nan
    elif u < 0.18:
        e = voices[0] * F(1e-20)
    else:
        v = voices[rng.integers(len(voices))]
        s = F((0.1, 1.0, 1.9, 4.0)[rng.integers(4)])
        e = F((0.5, 1.0, 7.0)[rng.integers(3)]) * (v + s * unit(rng))
    return e.astype(F), F(0.5 if rng.random() < 0.2 else 2.0), int(rng.random() < 0.08)


def snapshot(m):
    return [(sp.id, s, R.bits(sp.current).tolist(), [R.bits(r.embedding).tolist() for r in sp.raws], R.bits1(sp.duration), sp.update_count, sp.created,
             sp.updated, sp.permanent) for s, sp in m.speakers()]


def seed_stream(m, ar, voices, S, Rcap, rng):
    """Enrolment before the first call, as (id, current, duration, raws, permanent) upserts: two identical speakers (the tie goes to the lowest
    slot), an existing id overwritten with a non-unit row (the cosine's general branch), a ring one short of full, and for the 64-slot
    table all but two slots taken."""
    ups = []
    if S >= 2:
        ups.append((1, voices[0], 3.0, [], False))
    if S >= 5:
        ups += [(2, voices[0], 3.0, [], False), (3, voices[1], 1.0, [], True), (3, voices[1] * F(2.5), 4.0, [], False),
                (4, voices[2], 2.0, [R.RawEmbedding(ar, unit(rng) + voices[2]) for _ in range(Rcap - 1)], False)]
    if S == 1:
        ups += [(9, voices[0], 1.0, [], False), (9, voices[0] * F(2.5), 1.5, [], False)]
    if S == 64:
        ups += [(10 + k, unit(rng), 1.0, [], False) for k in range(57)]
    for id, cur, dur, raws, perm in ups:
        assert m.upsert_speaker(id, cur, dur, raws, update_count=2, created=1, updated=2, permanent=perm)
    return ups


@pytest.fixture(scope="module")
def db_cases():
    """Per case: the enrolment, CALLS calls (inputs, the restatement's records, and after each the whole state, the distances of the call's
    own embeddings and the mergeable pairs), and the management steps between them.  Nothing here touches the device."""
    R.BRANCHES.clear()
    ar = R.Arith(R.dot256)
    cases = {}
    for ci, (name, (B, S, Rcap, per, vmin)) in enumerate(CASES.items()):
        rng = np.random.default_rng(100 + ci)
        mgrs = [R.SpeakerManager(ar, max_speakers=S, raw_capacity=Rcap, validate_min_magnitude=vmin) for _ in range(B)]
        voices = [[unit(rng) for _ in range(S + 2 if S < 64 else 8)] for _ in range(B)]
        seeds = [seed_stream(mgrs[b], ar, voices[b], S, Rcap, rng) for b in range(B)]
        calls = []
        for c in range(CALLS):
            tick = 10 * c + 5
            emb, dur, skip = np.zeros((B, per, 256), F), np.zeros((B, per), F), np.zeros((B, per), np.int32)
            want = np.zeros((B, per), [("id", np.int32), ("slot", np.int32), ("kind", np.int32), ("distance", np.uint32)])
            for b in range(B):
                prev = None
                for i in range(per):
                    emb[b, i], dur[b, i], skip[b, i] = draw_item(rng, voices[b], prev)
                    prev = emb[b, i]
                    if skip[b, i]:
                        R.BRANCHES["SKIPPED"] += 1
                        want[b, i] = (0, -1, 0, R.bits1(R.INF))
                        continue
                    sp = mgrs[b].assign_speaker(emb[b, i], dur[b, i], tick=tick)
                    kind, slot, dist = mgrs[b].last
                    want[b, i] = (sp.id if sp is not None else 0, slot, R.KINDS.index(kind), R.bits1(dist))
            manage = []
            if c == 1:   # between the calls: permanence, removal, inactivity — mirrored on the device by the same list
                for b in range(B):
                    ids = mgrs[b].speaker_ids
                    if ids:
                        manage.append(("set_permanent", b, ids[0], True))
                        manage.append(("remove", b, ids[0], True))      # kept: it is permanent
                    if len(ids) > 1:
                        manage.append(("remove", b, ids[-1], True))
                manage.append(("remove_inactive", -1, 3, True))           # everything enrolled at tick 2 and not heard since
            if c == 2:
                manage.append(("reset", B - 1, True))
                if B > 1:
                    manage.append(("set_permanent", 0, mgrs[0].speaker_ids[0] if mgrs[0].speaker_ids else 1, False))
            for op in manage:
                targets = range(B) if op[1] < 0 else [op[1]]
                for b in targets:
                    if op[0] == "set_permanent":
                        (mgrs[b].make_speaker_permanent if op[3] else mgrs[b].revoke_permanence)(op[2])
                    elif op[0] == "remove":
                        mgrs[b].remove_speaker(op[2], keep_if_permanent=op[3])
                    elif op[0] == "remove_inactive":
                        mgrs[b].remove_speakers_inactive(op[2], keep_if_permanent=op[3])
                    else:
                        mgrs[b].reset(keep_if_permanent=op[2])
            dist = np.zeros((B, per, S), np.uint32)
            best = np.zeros((B, per), np.int32)
            for b in range(B):
                for i in range(per):
                    d, at = mgrs[b].distances(emb[b, i])
                    dist[b, i], best[b, i] = R.bits(d), at
            pairs = [[(a, d, R.bits1(x)) for a, d, x in mgrs[b].find_mergeable_pairs(speaker_threshold=0.5, exclude_if_both_permanent=bool(c & 1))]
                     for b in range(B)]
            calls.append(dict(tick=tick, emb=emb, dur=dur, skip=skip, want=want, manage=manage, state=[snapshot(m) for m in mgrs],
                              next_id=[m.next_id for m in mgrs], dist=dist, best=best, pairs=pairs, excl=bool(c & 1)))
        cases[name] = dict(shape=(B, S, Rcap, per, vmin), seeds=seeds, calls=calls)
    cases["branches"] = dict(R.BRANCHES)
    return cases


def test_the_inputs_reach_every_kind_the_wrap_both_cosine_branches_and_the_tie(db_cases):
    taken = db_cases["branches"]
    print(taken)
    assert all(taken.get(name, 0) > 0 for name in R.BRANCH_NAMES), {n: taken.get(n, 0) for n in R.BRANCH_NAMES}


def device_snapshot(fa, db, b):
    out = []
    for id in db.ids(b):
        sp = db.get(b, id)
        out.append((sp.id, sp.slot, R.bits(sp.current_embedding).tolist(), [R.bits(r).tolist() for r in sp.raw_embeddings], R.bits1(sp.duration),
                    sp.update_count, sp.created_tick, sp.updated_tick, sp.is_permanent))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_database_equals_the_restatement_call_after_call(fa, gpu_ctx, db_cases, name):
    case = db_cases[name]
    B, S, Rcap, per, vmin = case["shape"]
    db = fa.SpeakerDatabase(B, fa.SpeakerDbConfig(max_speakers=S, raw_capacity=Rcap, validate_min_magnitude=vmin), ctx=gpu_ctx)
    try:
        assert db.counts().tolist() == [0] * B
        for b, ups in enumerate(case["seeds"]):
            for id, cur, dur, raws, perm in ups:
                db.upsert(b, fa.Speaker(id, cur, float(dur), np.array([r.embedding for r in raws], F).reshape(-1, 256), 2, 1, 2, perm))
        for call in case["calls"]:
            got = db.assign(call["emb"], call["dur"], call["skip"], tick=call["tick"])
            want = call["want"]
            assert got["id"].tolist() == want["id"].tolist()
            assert got["slot"].tolist() == want["slot"].tolist() and got["kind"].tolist() == want["kind"].tolist()
            assert got["distance"].view(np.uint32).tolist() == want["distance"].tolist()
            for op in call["manage"]:
                if op[0] == "set_permanent":
                    db.set_permanent(op[1], op[2], op[3])
                elif op[0] == "remove":
                    db.remove(op[1], op[2], keep_if_permanent=op[3])
                elif op[0] == "remove_inactive":
                    db.remove_inactive(op[2], stream=op[1], keep_if_permanent=op[3])
                else:
                    db.reset(stream=op[1], keep_if_permanent=op[2])
            for b in range(B):
                assert device_snapshot(fa, db, b) == call["state"][b], (name, call["tick"], b)
            assert db.counts().tolist() == [len(s) for s in call["state"]]
            dist, best = db.distances(call["emb"])
            assert dist.view(np.uint32).tolist() == call["dist"].tolist() and best.tolist() == call["best"].tolist()
            pairs = db.mergeable_pairs(speaker_threshold=0.5, exclude_if_both_permanent=call["excl"])
            assert [[(int(p["source_id"]), int(p["destination_id"]), R.bits1(p["distance"])) for p in ps] for ps in pairs] == call["pairs"]
    finally:
        db.close()


def test_find_speaker_and_matching_speakers_on_the_device(fa, gpu_ctx):
    """testFindSpeakerAndMatchingSpeakers through the device entries: the filter and the sort are the mirror's."""
    ar = R.Arith(R.dot256)
    arg = lambda p: np.sin(((np.arange(256) + p * 100).astype(F) * F(0.1)).astype(np.float64)).astype(F)  # noqa: E731
    n1, n2 = ar.l2_normalize(arg(1)), ar.l2_normalize(arg(2))
    m = R.SpeakerManager(ar, speaker_threshold=0.8, max_speakers=4)
    db = fa.SpeakerDatabase(2, fa.SpeakerDbConfig(speaker_threshold=0.8, max_speakers=4, raw_capacity=2), ctx=gpu_ctx)
    try:
        o0, o1 = np.zeros(256, F), np.zeros(256, F)
        o0[0], o1[1] = 1, 1
        for id, cur in ((1, n1), (2, n2), (3, o0)):
            m.upsert_speaker(id, cur, 5.0)
            db.upsert(1, fa.Speaker(id, cur, 5.0))
        match, d = db.find_speaker(1, n1)
        want, wd = m.find_speaker(n1)
        assert match == want == 1 and R.bits1(d) == R.bits1(wd)
        assert db.find_speaker(1, o1, speaker_threshold=0.5)[0] is None and db.find_speaker(0, n1)[0] is None
        q = ar.l2_normalize((n1 + n2) / F(2))
        got = db.find_matching_speakers(1, q, speaker_threshold=2.0)
        assert [(i, R.bits1(x)) for i, x in got] == [(i, R.bits1(x)) for i, x in m.find_matching_speakers(q, speaker_threshold=2.0)] and len(got) == 3
        full = fa.Speaker(4, n2, 1.0)
        db.upsert(1, full)
        with pytest.raises(fa.FluidAudioHipError) as err:
            db.upsert(1, fa.Speaker(5, n2, 1.0))
        assert err.value.status == fa._lib.OUTPUT_TOO_SMALL
    finally:
        db.close()


def test_the_cpp_mirror_on_the_device_equals_the_restatement(fa, gpu_ctx, tmp_path_factory):
    """tests/cabi/online.cpp in its device mode: the mirror's SpeakerManager through the scenarios of testEmbeddingUpdateWithinAssignSpeaker,
    testMinDurationFiltering, upsert, findSpeaker, findMatchingSpeakers, findMergeablePairs, removal and reset; one child process."""
    import test_cabi_online as T
    r = subprocess.run([T.build_host(fa, tmp_path_factory), "device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ar = R.Arith(R.dot256)
    m = R.SpeakerManager(ar, speaker_threshold=0.3, embedding_threshold=0.2, max_speakers=4, raw_capacity=3)
    want = []

    def spk(sp):
        if sp is None:
            return ["SPK", "none"]
        return ["SPK", str(sp.id), str(len(sp.raws)), str(sp.update_count), f"{R.bits1(sp.duration):08x}", str(sp.created), str(sp.updated), str(int(sp.permanent))] + \
            [f"{b:08x}" for b in R.bits(sp.current)]

    e2 = T.distinct(1)
    e2[0] += F(0.01)
    for e, dur, tick in ((T.distinct(1), 3.0, 5), (e2, 0.5, 6), (T.distinct(2), 0.5, 7), (T.distinct(2), 2.0, 8)):
        sp = m.assign_speaker(e, dur, tick=tick)
        kind, slot, dist = m.last
        want += [spk(sp), ["REC", str(sp.id if sp is not None else 0), str(slot), str(R.KINDS.index(kind)), f"{R.bits1(dist):08x}"]]
    m.upsert_speaker(7, T.distinct(3), 5.0, created=1, updated=2, permanent=True)
    fid, fd = m.find_speaker(ar.l2_normalize(T.distinct(3)))
    want.append(["FIND", str(fid or 0), f"{R.bits1(fd):08x}"])
    want += [["MATCH", str(i), f"{R.bits1(d):08x}"] for i, d in m.find_matching_speakers(ar.l2_normalize(T.distinct(1)), speaker_threshold=2.0)]
    want += [["PAIR", str(a), str(b)] for a, b, _ in m.find_mergeable_pairs(speaker_threshold=2.0, exclude_if_both_permanent=False)]
    m.remove_speaker(7)
    m.reset(keep_if_permanent=True)
    want.append(["IDS"] + [str(i) for i in sorted(m.speaker_ids)] + ["|", str(m.speaker_count)])
    assert [l.split() for l in r.stdout.splitlines()] == want
    assert [w[1] for w in want if w[0] == "REC"] == ["1", "1", "0", "2"] and want[-1] == ["IDS", "7", "|", "1"]
