"""The one allocation-failure branch of the host entries (fa::take, fa_common.h), reached through fa_debug_inject_fault: armed with a
count of 2, FAULT_DEVBUF_MALLOC fails the first hipMalloc of a cached-buffer request AND its retry, so the request fails for good — with
no memory pressure and nothing going wrong on the device.  Every entry must then return ALLOCATION_FAILURE with the helper's text, and
must give its usual result, bit for bit, on the next call.

Only entries whose buffers come from the context's buffer cache pass through that site.  The entries that take one-call hipMalloc
buffers (the CTC decoders, the host-pointer beam search, k-means, the mel featurizer, the resamplers, the linkage batch and row minima)
go through the same helper but cannot be reached by this hook; a real out-of-memory is not provoked to cover them."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _der(fa, ctx):
    seg = fa.DERSpeakerSegment
    return fa.compute_der([seg("a", 0.0, 1.0)], [seg("x", 0.0, 1.0)], ctx=ctx)


def _edit_distance(fa, ctx):
    return fa.edit_distance_batch([(np.array([1, 2, 3], np.int32), np.array([1, 3, 3], np.int32))], ctx=ctx)


def _timeline(fa, ctx):
    p = np.zeros((4, 4), np.float32)
    p[1:3, 0] = 0.9
    return fa.timeline_segments(p, ctx=ctx)


def _cif_config(fa):
    cfg = fa.paraformer.default_config()
    cfg.max_tokens, cfg.enc_frames = 4, 4
    return cfg


def _paraformer_cif(fa, ctx):
    enc = np.arange(16, dtype=np.float32).reshape(1, 4, 4) / 16
    return fa.cif_batch(enc, np.full((1, 4), 0.6, np.float32), config=_cif_config(fa), ctx=ctx)


def _paraformer_timestamps(fa, ctx):
    audio = np.sin(np.arange(640, dtype=np.float32) / 7)
    return fa.timestamps_batch(np.full((1, 4), 0.6, np.float32), None, np.array([[3, 4, 0, 0]], np.int32), np.array([2], np.int32), np.ones(8, np.uint8), [audio],
                               config=_cif_config(fa), ctx=ctx)


def _tdt_merge(fa, ctx):
    tok = np.array([[1, 2, 3, 0], [3, 4, 5, 0]], np.int32)
    tim = np.array([[0, 10, 20, 0], [20, 30, 40, 0]], np.int32)
    m = fa.merge_windows(tok, tim, np.ones((2, 4), np.int32), np.full((2, 4), 0.5, np.float32), np.array([3, 3], np.int32), [0, 2], ctx=ctx)
    n = int(m.counts[0])   # the slice has room for more tokens than the merge emits: what lies behind them is not part of the result
    return m.tokens[:n], m.timestamps[:n], m.durations[:n], m.confidences[:n], m.out_range, m.counts, m.statuses, m.routes


def _kws_spot(fa, ctx):
    lp = np.log(np.full((1, 4, 5), 0.2, np.float32))
    return fa.spot_keywords_batch(lp, [[1, 2]], blank_id=0, ctx=ctx)


def _weight_resample(fa, ctx):
    return fa.weight_resample(np.array([[0.0, 1.0, 0.5, 0.25]], np.float32), 6, ctx=ctx)


def _powerset(fa, ctx):
    return fa.powerset_decode(np.arange(28, dtype=np.float32).reshape(1, 4, 7) % 5, log_probs=True, ctx=ctx)


CASES = {"der": _der, "edit_distance_batch": _edit_distance, "timeline_segments": _timeline, "paraformer_cif": _paraformer_cif,
         "paraformer_timestamps": _paraformer_timestamps, "tdt_merge_windows": _tdt_merge, "kws_spot": _kws_spot, "weight_resample": _weight_resample,
         "powerset_decode": _powerset}


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if dataclasses.is_dataclass(a):
        return type(a) is type(b) and _same(vars(a), vars(b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("name", list(CASES))
def test_a_failed_device_allocation_is_reported_and_leaves_the_context_usable(fa, gpu_ctx, name):
    L = fa.lib()
    assert L.fa_debug_hooks_enabled() == 1
    call = CASES[name]
    ctx = fa.Context(0)
    try:
        first = call(fa, ctx)
        ctx.trim()                                                       # empty cache: the next request reaches hipMalloc
        L.fa_debug_inject_fault(fa._lib.FAULT_DEVBUF_MALLOC, 2)          # that hipMalloc and its retry
        with pytest.raises(fa.FluidAudioHipError) as err:
            call(fa, ctx)
        assert err.value.status == fa._lib.ALLOCATION_FAILURE
        text = ctx.last_error()
        assert text.endswith("device allocation failed") or (name == "tdt_merge_windows" and "device allocation failed (" in text), text
        assert _same(call(fa, ctx), first)
    finally:
        L.fa_debug_inject_fault(fa._lib.FAULT_DEVBUF_MALLOC, 0)
        ctx.close()
