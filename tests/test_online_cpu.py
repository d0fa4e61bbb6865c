"""tests/online_restatement.py held to the reference's own model-free tests (Tests/FluidAudioTests/Diarizer/SpeakerManagerTests.swift,
SpeakerTests.swift, SpeakerOperationsTests.swift: the cases named in each test below), with integer ids for the reference's strings and
ticks for its dates.  Every outcome is computed twice: with the library's dot256 and with a float64 sequential dot as a second opinion;
the reference's assertions hold under both, so they do not rest on the summation order.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_restatement as R  # noqa: E402

F = np.float32


def distinct(pattern):
    """createDistinctEmbedding: sin(Float(i + pattern * 100) * 0.1), the sine of the fp32 argument rounded to fp32"""
    arg = (np.arange(256) + pattern * 100).astype(F) * F(0.1)
    return np.sin(arg.astype(np.float64)).astype(F)


@pytest.fixture(params=["dot256", "dot64"])
def ar(request):
    return R.Arith(getattr(R, request.param))


def manager(ar, **kw):
    return R.SpeakerManager(ar, **kw)


def test_dot256_agrees_in_every_lane_and_the_patterns_lie_far_from_the_thresholds():
    ar = R.Arith()
    n = [ar.l2_normalize(distinct(p)) for p in (1, 2, 3)]
    for a in n:
        for b in n:
            lanes = R.dot256_lanes(a, b)
            assert np.all(R.bits(lanes) == R.bits(lanes)[0])
    d12, d23, d13 = ar.cosine_distance(n[0], n[1]), ar.cosine_distance(n[1], n[2]), ar.cosine_distance(n[0], n[2])
    print(d12, d23, d13)
    assert min(abs(float(d) - t) for d in (d12, d23, d13) for t in (0.65, 0.45, 0.5, 0.3, 0.2, 0.8)) > 0.05
    bumped = distinct(1)
    bumped[0] += F(0.001)
    assert ar.cosine_distance(n[0], ar.l2_normalize(bumped)) < 1e-5


# ---- SpeakerManagerTests
def test_assign_new_existing_multiple(ar):
    m = manager(ar)
    assert m.speaker_count == 0 and m.speaker_ids == []                      # testInitialization
    assert m.assign_speaker(distinct(1), 2.0).id == 1 and m.speaker_count == 1   # testAssignNewSpeaker
    m = manager(ar, speaker_threshold=0.3)                                  # testAssignExistingSpeaker
    s1 = m.assign_speaker(distinct(1), 2.0)
    e2 = distinct(1)
    e2[0] += F(0.001)
    assert m.assign_speaker(e2, 2.0).id == s1.id and m.speaker_count == 1
    m = manager(ar, speaker_threshold=0.5)                                  # testMultipleSpeakers
    a, b = m.assign_speaker(distinct(1), 2.0), m.assign_speaker(distinct(2), 2.0)
    assert a is not None and b is not None and a.id != b.id and m.speaker_count == 2
    assert manager(ar).assign_speaker(np.full(128, 0.5, F), 2.0) is None    # testInvalidEmbeddingSize
    assert manager(ar).assign_speaker(np.zeros(0, F), 2.0) is None          # testEmptyEmbedding


def test_known_speakers_skip_overwrite_reset(ar):
    m = manager(ar)                                                         # testInitializeKnownSpeakers
    m.initialize_known_speakers([R.Speaker(ar, 10, distinct(10)), R.Speaker(ar, 20, distinct(20))])
    assert m.speaker_count == 2 and set(m.speaker_ids) == {10, 20} and m.next_id == 21
    m = manager(ar, speaker_threshold=0.3)                                  # testRecognizeKnownSpeaker
    m.initialize_known_speakers([R.Speaker(ar, 7, distinct(10))])
    assert m.assign_speaker(distinct(10), 2.0).id == 7
    m = manager(ar)                                                         # ...PreservesPermanentByDefault
    m.initialize_known_speakers([R.Speaker(ar, 7, distinct(10), duration=4.0)])
    m.make_speaker_permanent(7)
    m.initialize_known_speakers([R.Speaker(ar, 7, distinct(20), duration=8.0)], mode="overwrite", preserve_if_permanent=True)
    assert m.get_speaker(7).duration == F(4.0)
    m = manager(ar)                                                         # ...OverwriteCanReplacePermanentWhenAllowed
    m.initialize_known_speakers([R.Speaker(ar, 7, distinct(10), duration=4.0, permanent=True)])
    m.initialize_known_speakers([R.Speaker(ar, 7, distinct(20), duration=10.0)], mode="overwrite", preserve_if_permanent=False)
    assert m.get_speaker(7).duration == F(10.0) and not m.get_speaker(7).permanent
    m.initialize_known_speakers([R.Speaker(ar, 7, distinct(30), duration=1.0)])          # .skip keeps the stored one
    assert m.get_speaker(7).duration == F(10.0)
    m.initialize_known_speakers([R.Speaker(ar, 9, distinct(30), duration=1.0)], mode="reset", preserve_if_permanent=True)
    assert m.speaker_ids == [9]


def test_find_speaker_and_matching_speakers(ar):
    m = manager(ar, speaker_threshold=0.8)                                  # testFindSpeakerAndMatchingSpeakers
    n1, n2 = ar.l2_normalize(distinct(1)), ar.l2_normalize(distinct(2))
    m.upsert_speaker(1, n1, 5.0)
    m.upsert_speaker(2, n2, 5.0)
    match, distance = m.find_speaker(n1)
    assert match == 1 and abs(float(distance)) < 1e-4
    o0, o1 = np.zeros(256, F), np.zeros(256, F)
    o0[0], o1[1] = 1, 1
    m.upsert_speaker(3, o0, 5.0)
    assert m.find_speaker(o1, speaker_threshold=0.5) == (None, R.INF)
    matches = m.find_matching_speakers(ar.l2_normalize((n1 + n2) / F(2)), speaker_threshold=2.0)
    assert len(matches) == 3 and matches[0][1] <= matches[1][1] <= matches[2][1] and {i for i, _ in matches} == {1, 2, 3}


def test_upsert_new_and_existing(ar):
    m = manager(ar)                                                         # testUpsertNewSpeaker
    m.upsert_speaker(4, distinct(1), 5.0)
    info = m.get_speaker(4)
    assert m.speaker_count == 1 and info.duration == F(5.0) and info.update_count == 1 and m.next_id == 5
    assert R.bits(info.current).tolist() == R.bits(ar.l2_normalize(distinct(1))).tolist()
    m.upsert_speaker(4, distinct(2), 10.0, update_count=5, created=99, updated=7)   # testUpsertExistingSpeaker
    info = m.get_speaker(4)
    assert m.speaker_count == 1 and R.bits(info.current).tolist() == R.bits(distinct(2)).tolist()   # NOT normalised
    assert info.duration == F(10.0) and info.update_count == 5 and info.created == 0 and info.updated == 7
    sp = R.Speaker(ar, 6, distinct(1), duration=7.5)                        # testUpsertWithSpeakerObject
    sp.add_raw_embedding(R.RawEmbedding(ar, distinct(1)), 0)
    m.upsert_speaker(sp.id, sp.current, sp.duration, sp.raws)
    assert len(m.get_speaker(6).raws) == 1 and m.get_speaker(6).duration == F(7.5)


def test_permanence_mergeable_pairs_removal_reset(ar):
    m = manager(ar)                                                         # testMakeAndRevokePermanentSpeakers
    sid = m.assign_speaker(distinct(1), 2.5).id
    m.make_speaker_permanent(sid)
    m.remove_speaker(sid)
    assert m.get_speaker(sid) is not None
    m.revoke_permanence(sid)
    m.remove_speaker(sid)
    assert m.get_speaker(sid) is None
    m = manager(ar, speaker_threshold=0.3)                                  # testFindMergeablePairsRespectsPermanentExclusion
    base = ar.l2_normalize(distinct(1))
    close = base.copy()
    close[0] += F(0.001)
    m.upsert_speaker(1, base, 5.0)
    m.upsert_speaker(2, ar.l2_normalize(close), 5.0)
    m.upsert_speaker(3, ar.l2_normalize(distinct(80)), 5.0)
    pairs = m.find_mergeable_pairs(speaker_threshold=0.2)
    assert [(a, b) for a, b, _ in pairs] == [(2, 1)]
    m.make_speaker_permanent(2)
    assert [(a, b) for a, b, _ in m.find_mergeable_pairs(speaker_threshold=0.2)] == [(1, 2)]   # :318-323
    m.make_speaker_permanent(1)
    assert m.find_mergeable_pairs(speaker_threshold=0.2, exclude_if_both_permanent=True) == []
    assert len(m.find_mergeable_pairs(speaker_threshold=0.2, exclude_if_both_permanent=False)) == 1
    m = manager(ar)                                                         # testRemoveSpeakersInactive...
    m.upsert_speaker(1, ar.l2_normalize(distinct(3)), 2.0, updated=-120)
    m.upsert_speaker(2, ar.l2_normalize(distinct(4)), 2.0, updated=0)
    m.remove_speakers_inactive(-60)
    assert m.speaker_ids == [2]
    m = manager(ar)                                                         # testResetKeepsPermanentSpeakers, testResetSpeakers
    a, b = m.assign_speaker(distinct(1), 2.0).id, m.assign_speaker(distinct(2), 2.0).id
    m.make_speaker_permanent(a)
    m.reset(keep_if_permanent=True)
    assert m.speaker_ids == [a] and m.next_id == a + 1 and b != a
    m.reset()
    assert m.speaker_count == 0 and m.next_id == 1


def test_embedding_update_fifo_thresholds_min_duration(ar):
    for second_duration in (3.0, 0.5):                                      # testEmbeddingUpdateWithinAssignSpeaker, testNoEmbeddingUpdateForShortDuration
        m = manager(ar, speaker_threshold=0.3, embedding_threshold=0.2)
        s1 = m.assign_speaker(distinct(1), 3.0)
        before = s1.update_count
        e2 = distinct(1)
        e2[0] += F(0.01)
        assert m.assign_speaker(e2, second_duration).id == s1.id and m.last[0] == "UPDATED"
        info = m.get_speaker(s1.id)
        assert info.update_count > before and info.duration > F(3.0) and not np.array_equal(info.current, distinct(1))
    m = manager(ar, speaker_threshold=0.3, embedding_threshold=0.2)        # testRawEmbeddingFIFOInManager
    s = m.assign_speaker(distinct(1), 3.0)
    for i in range(60):
        e = distinct(1)
        e[0] += F(i) * F(0.001)
        m.assign_speaker(e, 2.5)
    assert m.speaker_count == 1 and len(m.get_speaker(s.id).raws) == 50 and m.get_speaker(s.id).update_count == 61
    m = manager(ar, speaker_threshold=0.01)                                 # testSpeakerThresholdBoundaries
    m.assign_speaker(distinct(1), 2.0)
    e = distinct(1)
    e[0] += F(0.001)
    m.assign_speaker(e, 2.0)
    assert m.speaker_count == 1
    m = manager(ar, speaker_threshold=0.001)
    m.assign_speaker(distinct(1), 2.0)
    m.assign_speaker(distinct(1), 2.0)
    assert m.speaker_count == 1
    m = manager(ar, speaker_threshold=0.5, embedding_threshold=0.3, min_speech_duration=2.0)   # testMinDurationFiltering
    assert m.assign_speaker(distinct(1), 0.5) is None and m.speaker_count == 0 and m.last[0] == "TOO_SHORT"
    s2 = m.assign_speaker(distinct(1), 3.0)
    assert s2 is not None and m.speaker_count == 1
    assert m.assign_speaker(distinct(1), 0.5).id == s2.id


# ---- SpeakerTests
def test_update_main_embedding(ar):
    sp = R.Speaker(ar, 1, distinct(1))                                      # testUpdateMainEmbedding
    sp.update_main_embedding(3.0, distinct(2), 0, alpha=0.9)
    assert not np.array_equal(sp.current, distinct(1)) and not np.array_equal(sp.current, distinct(2))
    assert len(sp.raws) == 1 and sp.update_count == 2 and sp.duration == F(3.0)
    sp = R.Speaker(ar, 1, np.full(256, 1.0, F))                             # testUpdateMainEmbeddingWithAlpha
    sp.update_main_embedding(3.0, np.full(256, 0.5, F), 0, alpha=0.8)
    assert np.max(np.abs(sp.current - ar.l2_normalize(np.full(256, 0.5, F)))) < 0.001 and len(sp.raws) == 1 and sp.update_count == 2
    sp = R.Speaker(ar, 1, distinct(1))                                      # testUpdateMainEmbeddingLowMagnitude
    sp.update_main_embedding(3.0, np.full(256, 0.001, F), 0, alpha=0.9)
    assert np.max(np.abs(sp.current - ar.l2_normalize(distinct(1)))) < 1e-4 and len(sp.raws) == 0 and sp.update_count == 1 and sp.duration == F(0)


def test_raw_fifo_and_recalculate(ar):
    sp = R.Speaker(ar, 1, distinct(1))                                      # testAddRawEmbedding
    sp.add_raw_embedding(R.RawEmbedding(ar, distinct(2)), 0)
    sp.add_raw_embedding(R.RawEmbedding(ar, distinct(3)), 0)
    assert len(sp.raws) == 2
    sp = R.Speaker(ar, 1, distinct(1))                                      # testRawEmbeddingFIFO
    for i in range(60):
        sp.add_raw_embedding(R.RawEmbedding(ar, distinct(i)), 0)
    assert len(sp.raws) == 50 and abs(float(sp.raws[0].embedding[0] - ar.l2_normalize(distinct(10))[0])) < 0.001
    sp = R.Speaker(ar, 1, np.zeros(256, F))                                 # testRecalculateMainEmbedding
    for v in (1.0, 2.0, 3.0):
        sp.add_raw_embedding(R.RawEmbedding(ar, np.full(256, v, F)), 0)
    sp.recalculate_main_embedding(0)
    assert np.max(np.abs(sp.current - ar.l2_normalize(np.full(256, 1.0, F)))) < 1e-4
    sp = R.Speaker(ar, 1, distinct(1))                                      # testRecalculateMainEmbeddingEmpty
    sp.recalculate_main_embedding(0)
    assert np.max(np.abs(sp.current - ar.l2_normalize(distinct(1)))) < 1e-4


# ---- SpeakerOperationsTests
def test_cosine_distance_and_validate_embedding(ar):
    n1, n2 = distinct(1) / np.sqrt(np.sum(distinct(1) ** 2)), distinct(2) / np.sqrt(np.sum(distinct(2) ** 2))   # createNormalizedEmbedding
    assert abs(float(ar.cosine_distance(n1, n1))) < 0.001                   # testCosineDistance (both suites)
    assert abs(float(ar.cosine_distance(distinct(1), distinct(1)))) < 1e-4
    assert 0.0 < ar.cosine_distance(n1, n2) <= 2.0 and ar.cosine_distance(distinct(1), distinct(2)) > 0
    e3, e4 = np.zeros(256, F), np.zeros(256, F)
    e3[0], e4[1] = 1, 1
    assert abs(float(ar.cosine_distance(e3, e4)) - 1.0) < 1e-4
    assert ar.cosine_distance(distinct(1), np.full(128, 0.5, F)) == R.INF   # testCosineDistanceWithDifferentSizes
    assert ar.cosine_distance(np.zeros(256, F), distinct(1)) == R.INF       # testCosineDistanceWithZeroVectors
    assert ar.validate_embedding(distinct(1))                               # testValidateEmbedding (its 128-element case: this library takes 256 only)
    assert not ar.validate_embedding(np.zeros(256, F))
    low, custom = np.zeros(256, F), np.zeros(256, F)
    low[0], custom[0] = 0.01, 0.2
    assert not ar.validate_embedding(low, 0.1) and ar.validate_embedding(custom, 0.1)
    bad = distinct(1)
    bad[5] = np.nan
    assert not ar.validate_embedding(bad)
