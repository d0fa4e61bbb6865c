"""The edit-distance restatement (tests/wer_restatement.py) against the reference's own pinned answers, and the argument contract of
fluidaudio_amd/wer.py and of fa_edit_distance_batch / _dev, which is decided before any device work.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wer_restatement as R  # noqa: E402


def test_restatement_gives_the_reference_tests_answers():
    """Tests/FluidAudioTests/Shared/StringUtilsTests.swift:10-66 and Tests/FluidAudioTests/ASR/Parakeet/NemotronBenchmarkTests.swift:15-120."""
    for a, b, d in R.LEVENSHTEIN_CASES:
        assert R.levenshtein_distance(a, b) == d
        assert R.edit_distance(a, b).total == d
    for ref, hyp, errors, words in R.WER_CASES:
        e = R.edit_distance(hyp.split(), ref.split())
        assert (e.total, len(ref.split())) == (errors, words)
        assert e.total == e.insertions + e.deletions + e.substitutions
    # (total, insertions, deletions, substitutions): a word the hypothesis has too many is a row taken alone, which the reference's
    # traceback counts as a deletion (:222-224); a word it lacks is a column taken alone, an insertion (:225-227)
    assert [tuple(R.edit_distance(h.split(), r.split())) for r, h, _, _ in R.WER_CASES[1:4]] == [(1, 0, 0, 1), (1, 0, 1, 0), (1, 1, 0, 0)]
    assert tuple(R.edit_distance([], ["hello", "world"])) == (2, 2, 0, 0) and tuple(R.edit_distance(["hello", "world"], [])) == (2, 0, 2, 0)


def test_traceback_total_is_the_levenshtein_distance():
    rng = np.random.default_rng(11)
    for _ in range(400):
        k = int(rng.integers(1, 6))
        a, b = rng.integers(0, k, int(rng.integers(0, 20))).tolist(), rng.integers(0, k, int(rng.integers(0, 20))).tolist()
        e = R.edit_distance(a, b)
        assert e.total == R.levenshtein_distance(a, b) == e.insertions + e.deletions + e.substitutions
        assert len(a) - e.deletions + e.insertions == len(b)


def test_priority_on_ties_depends_on_the_side():
    """Substitution before deletion before insertion: the two sequences may not be swapped."""
    assert tuple(R.edit_distance([0, 1], [1, 0, 0])) == (2, 1, 0, 1) and tuple(R.edit_distance([1, 0, 0], [0, 1])) == (2, 0, 1, 1)
    assert tuple(R.edit_distance([0, 1, 1], [1, 1, 0])) == (2, 0, 0, 2)


def test_python_argument_contract_needs_no_device(fa):
    for bad in ([(np.zeros((2, 2), np.int32), [1])], [([0.5], [1])], [([2 ** 31], [1])], [([1], [-2 ** 31 - 1])], [([1], [1], [1])]):
        with pytest.raises(fa.FluidAudioHipError) as e:
            fa.edit_distance_batch(bad)
        assert e.value.status == fa.INVALID_ARGUMENT
    assert fa.edit_distance_batch([]).size == 0 and fa.edit_distance_batch([]).dtype == fa.EDIT_COUNTS_DTYPE
    assert fa.wer_metrics_batch([]) == ([], fa.CorpusErrorRate(0, 0, 0.0, 0, 0, 0.0))
    assert fa.wer_and_cer_batch([]) == ([], fa.CorpusErrorRate(0, 0, 0.0, 0, 0, 0.0))
    assert fa.EDIT_COUNTS_DTYPE.itemsize == C.sizeof(fa._lib.EditCounts) == 24


@pytest.mark.parametrize("entry", ["fa_edit_distance_batch", "fa_edit_distance_batch_dev"])
def test_c_argument_contract_needs_no_device(fa, entry):
    """The status is decided from the ranges alone: with no context at all a call that is otherwise well-formed ends in INVALID_ARGUMENT,
    an overlong side in INDEX_OVERFLOW — and nothing is read through the symbol pointers, nothing written."""
    f = getattr(fa.lib(), entry)
    sym = np.zeros(4, np.int32)
    out = np.full(12, 7, np.int32)
    i64 = lambda *v: np.array(v, np.int64)   # noqa: E731

    def call(hyp_range, ref_range, n, hyp=sym, ref=sym, res=out):
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return f(None, ptr(hyp), ptr(hyp_range), ptr(ref), ptr(ref_range), n, ptr(res))

    ok = i64(0, 2, 4)
    assert call(ok, ok, -1) == 1
    assert call(None, ok, 2) == 1 and call(ok, None, 2) == 1 and call(ok, ok, 2, res=None) == 1
    assert call(i64(0, 3, 2), ok, 2) == 1 and call(ok, i64(2, 1, 4), 2) == 1        # descending
    assert call(i64(-1, 2, 4), ok, 2) == 1                                          # a negative start
    assert call(ok, ok, 2, hyp=None) == 1 and call(ok, ok, 2, ref=None) == 1        # symbols without an array
    assert call(i64(0, 2 ** 31), i64(0, 1), 1) == 2 and call(i64(0, 1), i64(5, 5 + 2 ** 31), 1) == 2   # a side longer than INT32_MAX
    assert call(i64(0, 2 ** 31 - 1), i64(0, 1), 1) == 1                             # INT32_MAX itself is a length; what is missing is the context
    assert call(ok, ok, 2 ** 31 - 1) == 2                                           # too many pairs: answered before the ranges are read
    assert call(ok, ok, 2) == 1 and call(ok, ok, 0) == 1 and call(None, None, 0, None, None, None) == 1   # no context
    assert out.tolist() == [7] * 12
