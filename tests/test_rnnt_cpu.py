"""The decode calls of tests/rnnt_cases.py, judged by the restatement alone (no GPU): every call holds at least one decision of each
kind its vocabulary can hold (all fifteen from vocab_with_blank = 129 on; at 3 the two calls hold them between them), the logits stay
in the normal range, a chunk split at a frame into two calls equals the one call, and a vocabulary that matches no piece is the plain
walk."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_cases as K  # noqa: E402
import rnnt_restatement as R  # noqa: E402

IDS = [c.name for c in K.CALLS]


@pytest.mark.parametrize("call", K.CALLS, ids=IDS)
def test_every_call_holds_every_kind(call):
    t = K.table(call)
    found = set().union(*(K.kinds_of(t, b) for b in range(t.B)))
    assert not set(call.kinds) - found, sorted(set(call.kinds) - found)
    if call.variant == "general":
        assert set(call.kinds) == set(K.KINDS) and len(K.KINDS) == 15
    assert t.logits.shape == (call.B, call.U, call.T, call.V1 + K.PAD)
    assert (R.VocabularyBias(t.v.terms, t.v.pieces).tail_cap == 70) == call.long


def test_vocabulary_of_three_holds_all_kinds_between_its_two_calls():
    assert set(K.BY_NAME["f32_V3"].kinds) | set(K.BY_NAME["f32_V3_eou"].kinds) == set(K.KINDS)


@pytest.mark.parametrize("call", K.CALLS, ids=IDS)
def test_answers_are_what_the_programs_wrote(call):
    """The walk ends where its program ended, flips are recorded with the displaced argmax, and the outputs respect max_out."""
    t = K.table(call)
    for b, r in enumerate(t.expected):
        n = min(r["count"], call.max_out)
        assert len(r["tokens"]) == len(r["frames"]) == len(r["flips"]) == n
        assert all(f == -1 or f != tok for f, tok in zip(r["flips"], r["tokens"]))
        assert list(r["frames"]) == sorted(r["frames"]) and (n == 0 or (t.skip[b] <= r["frames"][0] and r["frames"][-1] < min(t.frames[b], call.T)))
        emitted = [e for e in t.trace[b] if e["emitted"]]
        assert [e["picked"] for e in emitted][:n] == list(r["tokens"]) and r["final_u"] == len(emitted) == r["count"]
        assert (t.v.blank not in r["tokens"]) and (t.v.eou not in r["tokens"])
        assert len(r["tail"]) <= R.VocabularyBias(t.v.terms, t.v.pieces).tail_cap


@pytest.mark.parametrize("call", [c for c in K.CALLS if not c.f16], ids=[c.name for c in K.CALLS if not c.f16])
def test_split_chunk_equals_one_call(call):
    """Frames [skip, split) in one call, [split, frames) in a second whose logits start at the first's final_u and whose tail is the
    first's: the tokens, frames and flips concatenate to the one call's, the final tail is the same."""
    t = K.table(call)
    U = call.U
    for split in (3, 6):
        carried = 0
        for b in range(t.B):
            whole = K.run(t, b, max_out=U)
            bias = K.new_bias(t)
            first = K.run(t, b, bias=bias, frames=min(t.frames[b], split), max_out=U)
            if first["eou"] or first["status"] != R.SUCCESS:
                assert first["count"] == whole["count"] and np.array_equal(first["tokens"], whole["tokens"])
                continue
            rebased = np.full_like(t.logits[b], 50.0)
            rebased[:U - first["final_u"]] = t.logits[b][first["final_u"]:]
            second = K.run(t, b, bias=bias, skip=max(split, t.skip[b]), logits=rebased[:max(1, U - first["final_u"])], max_out=U)
            for key in ("tokens", "frames", "flips"):
                assert np.array_equal(np.concatenate([first[key], second[key]]), whole[key]), (call.name, split, b, key)
            assert first["final_u"] + second["final_u"] == whole["final_u"] and second["eou"] == whole["eou"]
            assert np.array_equal(second["tail"], whole["tail"])
            carried += first["tail"].size > 0 and bool((second["flips"] >= 0).any())
        assert split != 3 or call.variant == "V3_eou" or carried >= 1      # a flip of the second call hangs on the first call's tail


def test_a_vocabulary_that_matches_no_piece_is_the_plain_walk():
    t = K.table(K.BY_NAME["f32_V129"])
    changed = 0
    for b in range(t.B):
        plain = K.run(t, b, bias=None)
        inert = K.run(t, b, bias=K.new_bias(t, ["wvu wvu"]))
        for key in ("status", "count", "final_u", "eou"):
            assert plain[key] == inert[key]
        assert np.array_equal(plain["tokens"], inert["tokens"]) and np.all(inert["flips"] == -1)
        changed += not np.array_equal(plain["tokens"], t.expected[b]["tokens"])
    assert changed >= 3           # and the call's own vocabulary does change the walk
