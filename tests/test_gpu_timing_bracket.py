"""fa_ctx_set_timing / fa_ctx_last_device_ms across the entries: the ones that bracket their launches (edit distance, Paraformer's CIF,
keyword spotting, CTC beam search; the TDT merge's is in tests/test_gpu_tdt_merge.py) report a positive time below the sanity cap that
test uses, the ones without a bracket (DER, timeline, k-means) leave the value alone, and so does every entry once timing is off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP_MS = 1000.0


@pytest.fixture
def timed(fa, gpu_ctx):
    """(library, context) with timing on; switched off again afterwards."""
    lib = fa.lib()
    lib.fa_ctx_set_timing(gpu_ctx.handle, 1)
    try:
        yield lib, gpu_ctx
    finally:
        lib.fa_ctx_set_timing(gpu_ctx.handle, 0)


def wer_call(fa, ctx):
    rng = np.random.default_rng(0)
    pairs = [(rng.integers(0, 5, m).tolist(), rng.integers(0, 5, n).tolist()) for m, n in ((3, 4), (70, 65))]
    out = fa.edit_distance_batch(pairs, ctx=ctx)
    assert len(out) == 2


def cif_call(fa, ctx):
    rng = np.random.default_rng(1)
    res = fa.cif_batch(rng.standard_normal((1, 8, 64)).astype(np.float32), np.full((1, 8), 0.3, np.float32), ctx=ctx)
    assert res.token_counts.shape == (1,)


def kws_call(fa, ctx):
    tie = np.asarray([[[-1.0, -2.0], [-1.0, 0.0]]], np.float32)                  # one utterance, one keyword: the tie of tests/test_gpu_kws.py
    dets, _ = fa.spot_keywords_batch(tie, [[0]], blank_id=1, merge_overlap=False, thresholds=[-100.0], ctx=ctx)
    assert len(dets) == 1


def beam_call(fa, ctx):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1, 4, 8)).astype(np.float32)
    x -= np.log(np.exp(x).sum(-1, keepdims=True))
    ids, scores = fa.ctc_beam_search_ids_batch(x, None, None, 8, 0.0, 0.0, 7, 3, ctx=ctx)
    assert len(ids) == 1 and np.isfinite(scores).all()


def der_call(fa, ctx):
    S = fa.DERSpeakerSegment
    fa.compute_der([S("A", 0.0, 1.0), S("B", 0.5, 1.5)], [S("x", 0.0, 1.5)], ctx=ctx)


def timeline_call(fa, ctx):
    act = np.zeros((6, 4), np.float32)
    act[1:4, 0] = 0.9
    recs, counts = fa.timeline_segments(act, [6], ctx=ctx)
    assert counts.tolist() == [1] and len(recs) == 1


def kmeans_call(fa, ctx):
    rows = [[1.0, 0.0], [1.1, 0.1], [0.0, 1.0], [0.1, 1.1]]
    assert len(fa.KMeansClustering.cluster(rows, 2, 20, 42, ctx=ctx)) == 4


def test_nothing_is_recorded_before_a_call(timed):
    lib, ctx = timed
    assert lib.fa_ctx_last_device_ms(ctx.handle) == -1.0


@pytest.mark.parametrize("entry", [wer_call, cif_call, kws_call, beam_call])
def test_bracketed_entries_report_device_time(fa, timed, entry):
    lib, ctx = timed
    entry(fa, ctx)
    ms = lib.fa_ctx_last_device_ms(ctx.handle)
    print(entry.__name__, ms)
    assert 0.0 < ms < CAP_MS


@pytest.mark.parametrize("entry", [der_call, timeline_call, kmeans_call])
def test_entries_without_a_bracket_leave_the_value(fa, timed, entry):
    lib, ctx = timed
    entry(fa, ctx)
    assert lib.fa_ctx_last_device_ms(ctx.handle) == -1.0


def test_timing_off_records_nothing(fa, gpu_ctx):
    lib = fa.lib()
    lib.fa_ctx_set_timing(gpu_ctx.handle, 1)
    lib.fa_ctx_set_timing(gpu_ctx.handle, 0)
    wer_call(fa, gpu_ctx)
    assert lib.fa_ctx_last_device_ms(gpu_ctx.handle) == -1.0
