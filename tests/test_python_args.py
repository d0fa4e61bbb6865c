"""What the Python wrappers decide before any device is asked: the empty-batch returns and the refusals of every host / _dev pair, with the
shape and dtype of every returned piece and the whole message of every refusal, and then the helpers of fluidaudio_amd/_args.py the
wrappers share.  The first part is written against the wrappers as they were before they shared a helper module, and passes there.
No GPU, and no call reaches the library."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import fluidaudio_amd as fa
from fluidaudio_amd import paraformer, tdt_merge, tdt_plan, vad, wer

L = fa._lib
F32, I32, I64 = np.float32, np.int32, np.int64
NO_CTX = object()                                         # stands for a context where an entry takes one before it looks at the batch
CIF = L.ParaformerCifConfig(1.0, 0.45, 128, 512)          # given, so that no default is asked of the library


@contextlib.contextmanager
def refused(message):
    with pytest.raises(L.FluidAudioHipError) as e:
        yield
    assert type(e.value) is L.FluidAudioHipError and e.value.status == fa.INVALID_ARGUMENT and str(e.value) == message


def is_array(x, shape, dtype):
    return isinstance(x, np.ndarray) and x.shape == tuple(shape) and x.dtype == dtype


# ---------------------------------------------------------------- empty batches

def test_vad_empty_batches():
    segs, counts = vad.segment_speech_batch([], np.zeros(0))
    assert is_array(segs, (0,), fa.VAD_SEGMENT_DTYPE) and is_array(counts, (0,), I64)
    rows, chunk_range = vad.pack_chunks([])
    assert is_array(rows, (0, vad.MODEL_INPUT_SIZE), F32) and is_array(chunk_range, (1,), I64) and chunk_range.tolist() == [0]
    for audio, offsets in (([np.ones(5, F32)], None), (np.ones(5, F32), [0, 5]), ([], None)):
        out, out_range = vad.gather_segments(audio, np.zeros(0, fa.VAD_SEGMENT_DTYPE), offsets)
        assert is_array(out, (0,), F32) and is_array(out_range, (1,), I64) and out_range.tolist() == [0]
    events = vad.stream_advance(np.zeros((0, 3), F32), vad.initial_stream_states(0))
    assert is_array(events, (0,), fa.VAD_STREAM_EVENT_DTYPE)
    assert is_array(vad.initial_stream_states(2), (2,), fa.VAD_STREAM_STATE_DTYPE)


def test_tdt_plan_empty_batches():
    plan = tdt_plan.plan_windows([])
    assert is_array(plan.windows, (0,), fa.TDT_WINDOW_DTYPE) and is_array(plan.window_range, (1,), I64) and plan.window_range.tolist() == [0]
    assert is_array(plan.speech_end, (0,), I64) and is_array(plan.statuses, (0,), I32)
    assert all(is_array(getattr(plan, name), (0,), I32) for name in tdt_plan.FIVE)
    plan = tdt_plan.plan_windows(np.zeros(0, F32), [0], capacity=3)
    assert is_array(plan.windows, (0,), fa.TDT_WINDOW_DTYPE) and all(is_array(getattr(plan, name), (0,), I32) for name in tdt_plan.FIVE)
    rows, lengths = tdt_plan.pack_windows([np.ones(7, F32)], np.zeros(0, fa.TDT_WINDOW_DTYPE))
    assert is_array(rows, (0, 240000), F32) and is_array(lengths, (0,), I32)
    cfg = L.TdtWindowConfig(max_model_samples=32)
    rows, lengths = tdt_plan.pack_windows(np.ones(7, F32), np.zeros(0, fa.TDT_WINDOW_DTYPE), [0, 3, 7], config=cfg)
    assert is_array(rows, (0, 32), F32) and is_array(lengths, (0,), I32)
    thresholds, frames, seconds, statuses = tdt_plan.speech_gate([], ctx=NO_CTX)
    assert is_array(thresholds, (0,), F32) and is_array(frames, (0,), I64) and is_array(seconds, (0,), np.float64) and is_array(statuses, (0,), I32)


def test_tdt_merge_empty_batch():
    z = np.zeros((0, 4), I32)
    m = tdt_merge.merge_windows(z, z, z, z.astype(F32), np.zeros(0, I32), [0])
    assert all(is_array(getattr(m, k), (0,), I32) for k in ("tokens", "timestamps", "durations", "counts", "statuses", "routes"))
    assert is_array(m.confidences, (0,), F32) and is_array(m.out_range, (1,), I64) and m.out_range.tolist() == [0]
    z = np.zeros((3, 4), I32)                               # windows that belong to no recording
    m = tdt_merge.merge_windows(z, z, z, z.astype(F32), np.zeros(3, I32), [0])
    assert is_array(m.tokens, (0,), I32) and is_array(m.routes, (3,), I32) and m.routes.tolist() == [fa.MERGE_NO_SEAM] * 3


def test_paraformer_empty_batches():
    for pack in (False, True):
        r = paraformer.cif_batch(np.zeros((0, 5, 8), F32), np.zeros((0, 6), F32), config=CIF, pack_enc=pack)
        assert is_array(r.ac, (0, 128, 8), F32) and is_array(r.token_counts, (0,), I32) and is_array(r.fire_counts, (0,), I32)
        assert is_array(r.fire_frames, (0, 6), I32) and (is_array(r.enc_packed, (0, 512, 8), F32) if pack else r.enc_packed is None)
    r = paraformer.cif_batch(np.zeros((0, 5, 8), np.float16), np.zeros((0, 5), F32), dim=3, config=CIF)
    assert is_array(r.ac, (0, 128, 3), F32)
    spans, utt = paraformer.timestamps_batch(np.zeros((0, 5), F32), None, np.zeros((0, 128), I32), [], np.ones(4, np.uint8), [], config=CIF)
    assert is_array(spans, (0,), fa.PARAFORMER_SPAN_DTYPE) and is_array(utt, (0,), I64)


def test_wer_empty_batch():
    assert is_array(wer.edit_distance_batch([]), (0,), fa.EDIT_COUNTS_DTYPE)


# ---------------------------------------------------------------- refusals of the host entries

def test_vad_host_refusals():
    with refused("fa_vad_segments: INVALID_ARGUMENT (probs is one-dimensional, covers frame_range, and total_samples holds one entry per recording)"):
        vad.segment_speech_batch(np.zeros((2, 3), F32), [1, 1], [0, 3, 6])                 # wrong rank
    with refused("fa_vad_segments: INVALID_ARGUMENT (probs is one-dimensional, covers frame_range, and total_samples holds one entry per recording)"):
        vad.segment_speech_batch(np.zeros(5, F32), [1, 1], [0, 3, 6])                      # the range ends beyond the data
    with refused("fa_vad_segments: INVALID_ARGUMENT (probs is one-dimensional, covers frame_range, and total_samples holds one entry per recording)"):
        vad.segment_speech_batch([np.zeros(3, F32), np.zeros(2, F32)], [1])                # total_samples of the wrong length
    for bad in ([[0, 3]], []):
        with refused("fa_vad_segments: INVALID_ARGUMENT (a range holds batch + 1 offsets)"):
            vad.segment_speech_batch(np.zeros(3, F32), [1], bad)
    with refused("fa_vad_pack_chunks: INVALID_ARGUMENT (a range holds batch + 1 offsets)"):
        vad.pack_chunks(np.zeros(3, F32), [])
    with refused("fa_vad_pack_chunks: INVALID_ARGUMENT (audio is one-dimensional and covers audio_offsets)"):
        vad.pack_chunks(np.zeros((2, 3), F32), [0, 3])
    with refused("fa_vad_pack_chunks: INVALID_ARGUMENT (audio is one-dimensional and covers audio_offsets)"):
        vad.pack_chunks(np.zeros(10, F32), [0, 11])
    none = np.zeros(0, fa.VAD_SEGMENT_DTYPE)
    with refused("fa_vad_gather_segments: INVALID_ARGUMENT (a range holds batch + 1 offsets)"):
        vad.gather_segments(np.zeros(3, F32), none, [[0, 3]])
    with refused("fa_vad_gather_segments: INVALID_ARGUMENT (audio is one-dimensional and covers audio_offsets)"):
        vad.gather_segments(np.zeros(10, F32), none, [0, 11])
    with refused("fa_vad_gather_segments: INVALID_ARGUMENT (segments is a one-dimensional array of VAD_SEGMENT_DTYPE)"):
        vad.gather_segments([np.zeros(10, F32)], np.zeros((1, 1), fa.VAD_SEGMENT_DTYPE))
    with refused("fa_vad_stream_advance: INVALID_ARGUMENT (probs is [S, K] and states holds S contiguous records of VAD_STREAM_STATE_DTYPE)"):
        vad.stream_advance(np.zeros(3, F32), vad.initial_stream_states(3))
    with refused("fa_vad_stream_advance: INVALID_ARGUMENT (probs is [S, K] and states holds S contiguous records of VAD_STREAM_STATE_DTYPE)"):
        vad.stream_advance(np.zeros((2, 3), F32), vad.initial_stream_states(3))
    with refused("fa_vad_stream_advance: INVALID_ARGUMENT (chunk_counts is [S] and chunk_samples [S, K])"):
        vad.stream_advance(np.zeros((2, 3), F32), vad.initial_stream_states(2), chunk_counts=[3])
    with refused("fa_vad_stream_advance: INVALID_ARGUMENT (chunk_counts is [S] and chunk_samples [S, K])"):
        vad.stream_advance(np.zeros((2, 3), F32), vad.initial_stream_states(2), chunk_samples=np.zeros((2, 2), I32))


def test_tdt_plan_host_refusals():
    none = np.zeros(0, fa.TDT_WINDOW_DTYPE)
    calls = {"fa_tdt_plan_windows": lambda audio, offsets: tdt_plan.plan_windows(audio, offsets),
             "fa_tdt_pack_windows": lambda audio, offsets: tdt_plan.pack_windows(audio, none, offsets),
             "fa_tdt_speech_gate": lambda audio, offsets: tdt_plan.speech_gate(audio, None, offsets, ctx=NO_CTX)}
    for where, call in calls.items():
        for bad in ([[0, 3]], []):
            with refused(f"{where}: INVALID_ARGUMENT (audio_offsets holds batch + 1 offsets)"):
                call(np.zeros(3, F32), bad)
        with refused(f"{where}: INVALID_ARGUMENT (audio is one-dimensional and covers audio_offsets)"):
            call(np.zeros((2, 3), F32), [0, 3])
        with refused(f"{where}: INVALID_ARGUMENT (audio is one-dimensional and covers audio_offsets)"):
            call(np.zeros(10, F32), [0, 11])
    with refused("fa_tdt_pack_windows: INVALID_ARGUMENT (windows is a one-dimensional array of TDT_WINDOW_DTYPE)"):
        tdt_plan.pack_windows([np.zeros(3, F32)], np.zeros((1, 1), fa.TDT_WINDOW_DTYPE))
    with refused("fa_tdt_speech_gate: INVALID_ARGUMENT (a span names a recording outside the batch)"):
        tdt_plan.speech_gate([], np.zeros(1, fa.TDT_SPAN_DTYPE), ctx=NO_CTX)                # a span, and an empty batch
    with refused("fa_tdt_speech_gate: INVALID_ARGUMENT (spans is a one-dimensional array of TDT_SPAN_DTYPE, override_thresholds holds one value per recording)"):
        tdt_plan.speech_gate([], override_thresholds=[0.5], ctx=NO_CTX)


def merge_args(windows=3, max_out=4):
    z = np.zeros((windows, max_out), I32)
    return [z, z, z, z.astype(F32), np.zeros(windows, I32)]


def test_tdt_merge_host_refusals():
    a = merge_args()
    with refused("merge_windows: INVALID_ARGUMENT (the window arrays are [windows, max_out] and the counts [windows])"):
        tdt_merge.merge_windows(a[0][0], a[1][0], a[2][0], a[3][0], a[4], [0, 3])          # wrong rank
    with refused("merge_windows: INVALID_ARGUMENT (the window arrays are [windows, max_out] and the counts [windows])"):
        tdt_merge.merge_windows(*a[:4], np.zeros(2, I32), [0, 3])
    with refused("merge_windows: INVALID_ARGUMENT (window_range holds n_recordings + 1 ascending entries inside the windows)"):
        tdt_merge.merge_windows(*a, [0, 4])                                                # ends beyond the windows
    with refused("merge_windows: INVALID_ARGUMENT (window_range holds n_recordings + 1 ascending entries inside the windows)"):
        tdt_merge.merge_windows(*a, [])
    with refused("merge_windows: INVALID_ARGUMENT (one non-negative capacity per recording)"):
        tdt_merge.merge_windows(*a, [0, 3], capacities=[1, 2])
    with refused("merge_windows: INVALID_ARGUMENT (a table is one-dimensional)"):
        tdt_merge.merge_windows(*a, [0, 3], splice_safe=np.zeros((2, 2), np.uint8))
    with refused("merge_windows: INVALID_ARGUMENT (the tables disagree about the vocabulary's size)"):
        tdt_merge.merge_windows(*a, [0, 3], splice_safe=np.zeros(4, np.uint8), case_canon=np.zeros(5, I32))
    with refused("merge_windows: INVALID_ARGUMENT (a table is shorter than the vocabulary)"):
        tdt_merge.merge_windows(*a, [0, 3], splice_safe=np.zeros(4, np.uint8), vocab=5)


def test_paraformer_host_refusals():
    enc, alphas, ids = np.zeros((2, 5, 8), F32), np.zeros((2, 5), F32), np.zeros((2, 128), I32)
    with refused("fa_paraformer_cif: INVALID_ARGUMENT (enc is [B, T, S] float32 or float16)"):
        paraformer.cif_batch(enc[0], alphas, config=CIF)
    with refused("fa_paraformer_cif: INVALID_ARGUMENT (enc is [B, T, S] float32 or float16)"):
        paraformer.cif_batch(enc.astype(np.float64), alphas, config=CIF)
    with refused("fa_paraformer_cif: INVALID_ARGUMENT (alphas is [B, >= T])"):
        paraformer.cif_batch(enc, alphas[:, :4], config=CIF)
    with refused("fa_paraformer_cif: INVALID_ARGUMENT (valid_frames holds one entry per utterance)"):
        paraformer.cif_batch(enc, alphas, valid_frames=[5], config=CIF)
    audio, keep = [np.zeros(10, F32), np.zeros(4, F32)], np.ones(4, np.uint8)
    with refused("fa_paraformer_timestamps: INVALID_ARGUMENT (alphas is [B, T] and token_ids [B, max_tokens])"):
        paraformer.timestamps_batch(alphas, None, ids[:, :100], [1, 1], keep, audio, config=CIF)
    with refused("fa_paraformer_timestamps: INVALID_ARGUMENT (valid_frames holds one entry per utterance)"):
        paraformer.timestamps_batch(alphas, [5], ids, [1, 1], keep, audio, config=CIF)
    with refused("fa_paraformer_timestamps: INVALID_ARGUMENT (token_counts [B], keep [vocab] and audio_offsets [B + 1] are required)"):
        paraformer.timestamps_batch(alphas, None, ids, [1], keep, audio, config=CIF)        # token_counts of the wrong length
    with refused("fa_paraformer_timestamps: INVALID_ARGUMENT (token_counts [B], keep [vocab] and audio_offsets [B + 1] are required)"):
        paraformer.timestamps_batch(alphas, None, ids, [1, 1], keep, np.zeros(14, F32), [0, 14], config=CIF)
    with refused("fa_paraformer_timestamps: INVALID_ARGUMENT (audio_offsets end beyond the samples)"):
        paraformer.timestamps_batch(alphas, None, ids, [1, 1], keep, np.zeros(14, F32), [0, 10, 15], config=CIF)


def test_wer_host_refusals():
    with refused("edit_distance_batch: INVALID_ARGUMENT (a pair is (hypothesis, reference))"):
        wer.edit_distance_batch([([1], [2], [3])])
    with refused("edit_distance_batch: INVALID_ARGUMENT (a sequence must be a one-dimensional array of integers)"):
        wer.edit_distance_batch([([[1, 2]], [2])])
    with refused("edit_distance_batch: INVALID_ARGUMENT (a sequence must be a one-dimensional array of integers)"):
        wer.edit_distance_batch([([1.5], [2])])
    with refused("edit_distance_batch: INVALID_ARGUMENT (a symbol does not fit int32)"):
        wer.edit_distance_batch([([2 ** 31], [2])])
    flat, rng = wer._pack([np.array([1, 2], I32), np.zeros(0, I32), np.array([3], I32)])
    assert is_array(flat, (3,), I32) and flat.tolist() == [1, 2, 3] and is_array(rng, (4,), I64) and rng.tolist() == [0, 2, 2, 3]
    flat, rng = wer._pack([])
    assert is_array(flat, (0,), I32) and is_array(rng, (1,), I64)


# ---------------------------------------------------------------- the _dev entries refuse what is not on a device

DEV_AUDIO = "audio is a contiguous one-dimensional float32 tensor on the device"


@pytest.mark.parametrize("host", [lambda a: a, torch.from_numpy], ids=["numpy", "cpu-tensor"])
def test_dev_entries_refuse_host_arrays(host):
    audio, states = host(np.zeros(10, F32)), vad.initial_stream_states(2)
    with refused("fa_vad_segments_dev: INVALID_ARGUMENT (probs is a contiguous one-dimensional float32 tensor on the device)"):
        vad.segment_speech_batch_dev(audio, [0, 10], [40960])
    with refused(f"fa_vad_pack_chunks_dev: INVALID_ARGUMENT ({DEV_AUDIO})"):
        vad.pack_chunks_dev(audio, [0, 10])
    with refused(f"fa_vad_gather_segments_dev: INVALID_ARGUMENT ({DEV_AUDIO})"):
        vad.gather_segments_dev(audio, [0, 10], np.zeros(0, fa.VAD_SEGMENT_DTYPE))
    with refused("fa_vad_stream_advance_dev: INVALID_ARGUMENT (probs is a contiguous [S, K] float32 tensor on the device, chunk_samples an int32 one of the same shape)"):
        vad.stream_advance_dev(host(np.zeros((2, 3), F32)), states)
    with refused(f"fa_tdt_plan_windows_dev: INVALID_ARGUMENT ({DEV_AUDIO})"):
        tdt_plan.plan_windows_dev(audio, [0, 10])
    with refused(f"fa_tdt_pack_windows_dev: INVALID_ARGUMENT ({DEV_AUDIO})"):
        tdt_plan.pack_windows_dev(audio, [0, 10], np.zeros(0, fa.TDT_WINDOW_DTYPE))
    with refused(f"fa_tdt_speech_gate_dev: INVALID_ARGUMENT ({DEV_AUDIO})"):
        tdt_plan.speech_gate_dev(audio, [0, 10])
    with refused("merge_windows: INVALID_ARGUMENT (the window arrays must be contiguous int32 / float32 tensors on the device)"):
        tdt_merge.merge_windows_dev(*[host(a) for a in merge_args()], [0, 3])
    with refused("fa_paraformer_cif_dev: INVALID_ARGUMENT (enc is a [B, T, S] float32 or float16 tensor on the device with contiguous rows)"):
        paraformer.cif_batch_dev(host(np.zeros((2, 5, 8), F32)), host(np.zeros((2, 5), F32)), config=CIF)
    with refused("fa_paraformer_timestamps_dev: INVALID_ARGUMENT (alphas is a [B, A] float32 tensor on the device with contiguous rows)"):
        paraformer.timestamps_batch_dev(host(np.zeros((2, 5), F32)), None, host(np.zeros((2, 128), I32)), [1, 1], np.ones(4, np.uint8), audio, [0, 5, 10], config=CIF)
    symbols = host(np.zeros(4, I32))
    with refused("edit_distance_batch: INVALID_ARGUMENT (the symbols must be contiguous one-dimensional int32 tensors on the device)"):
        wer.edit_distance_batch_dev(symbols, [0, 4], symbols, [0, 4])
    with refused("edit_distance_batch: INVALID_ARGUMENT (the ranges hold n_pairs + 1 entries each)"):
        wer.edit_distance_batch_dev(symbols, [0, 4], symbols, [0, 2, 4])


# ---------------------------------------------------------------- the helpers of _args.py

def test_ragged_normaliser():
    from fluidaudio_amd import _args as A
    flat, offsets = A.ragged([[1, 2, 3], np.zeros((2, 2)), []], None, F32, "w", "d")
    assert is_array(flat, (7,), F32) and flat.tolist() == [1, 2, 3, 0, 0, 0, 0] and flat.flags.c_contiguous
    assert is_array(offsets, (4,), I64) and offsets.tolist() == [0, 3, 7, 7]
    flat, offsets = A.ragged(np.arange(10, dtype=np.float64)[::2], [0, 2, 5], F32, "w", "d")
    assert is_array(flat, (5,), F32) and flat.tolist() == [0, 2, 4, 6, 8] and flat.flags.c_contiguous and is_array(offsets, (3,), I64) and offsets.tolist() == [0, 2, 5]
    flat, offsets = A.ragged([], None, F32, "w", "d")
    assert is_array(flat, (0,), F32) and is_array(offsets, (1,), I64) and offsets.tolist() == [0]
    for bad in ([], [[0, 1]]):
        with refused("w: INVALID_ARGUMENT (d)"):
            A.ragged(np.zeros(3, F32), bad, F32, "w", "d")
    t = torch.zeros(4)
    assert A.ragged(t, [0, 4], F32, "w", "d")[0] is t       # a tensor is the caller's to judge: it is handed through


def test_invalid_and_cfg_ref():
    from fluidaudio_amd import _args as A
    e = A.invalid("here", "why")
    assert type(e) is L.FluidAudioHipError and e.status == fa.INVALID_ARGUMENT and str(e) == "here: INVALID_ARGUMENT (why)"
    assert A.cfg_ref(None) is None
    cfg = L.DerConfig(0.01, 0.25)
    assert C.cast(A.cfg_ref(cfg), C.POINTER(L.DerConfig)).contents.collar == 0.25


def address(p):
    return p.value if isinstance(p, C.c_void_p) else p


def test_pointer_of():
    from fluidaudio_amd import _args as A
    assert A.ptr(None) is None
    a = np.arange(6, dtype=I32)
    assert address(A.ptr(a)) == a.ctypes.data and address(A.ptr(a[2:])) == a.ctypes.data + 8
    t = torch.arange(6, dtype=torch.int32)
    assert address(A.ptr(t)) == t.data_ptr() and address(A.ptr(t[2:])) == t.data_ptr() + 8
    assert C.cast(A.ptr(t[2:]), C.POINTER(C.c_int32))[0] == 2 and C.cast(A.ptr(a[3:]), C.POINTER(C.c_int32))[0] == 3


def test_device_predicate_and_outputs_beside_an_input():
    from fluidaudio_amd import _args as A
    assert not A.is_dev(np.zeros(3, F32), "float32") and not A.is_dev(torch.zeros(3), "float32") and not A.is_dev(None, "float32", 1)
    for like, kind in ((np.zeros(2, F32), np.ndarray), (torch.zeros(2), torch.Tensor)):
        out = A.beside(like, (2, 3), "int32")
        assert isinstance(out, kind) and tuple(out.shape) == (2, 3) and not np.asarray(out).any()
        assert out.dtype == (I32 if kind is np.ndarray else torch.int32)
        out = A.beside(like, 4, "float32", torch_empty=True)
        assert isinstance(out, kind) and tuple(out.shape) == (4,) and (kind is torch.Tensor or not out.any())   # a host output is always zero-filled


class OnDevice0:
    device = 0


def test_placement_without_a_device():
    from fluidaudio_amd import _args as A
    x, on_device = A.placed(torch.arange(6, dtype=torch.float64).reshape(2, 3).t(), OnDevice0)
    assert not on_device and is_array(x, (3, 2), F32) and x.flags.c_contiguous and x.tolist() == [[0, 3], [1, 4], [2, 5]]
    x, on_device = A.placed([[1, 2]], OnDevice0)
    assert not on_device and is_array(x, (1, 2), F32)
    for host in (np.zeros(3, F32), torch.zeros(3)):
        with pytest.raises(TypeError, match="a torch CUDA tensor is required"):
            A.device_tensor(host, OnDevice0)


@pytest.mark.parametrize("B,T,W", [(1, 4, 5), (3, 1, 5), (3, 4, 1), (1, 1, 5), (1, 1, 1), (3, 4, 5)])
def test_stride_rule(B, T, W):
    """The stride of a size-1 dimension is whatever the producer left there; the rule puts the dense one in its place."""
    from fluidaudio_amd import _args as A
    base = torch.zeros((B + 1, 2 * T + 1, W + 2))
    x = base[:B, :2 * T:2, :W]                              # rows 2 * (W + 2) apart, matrices (2 T + 1)(W + 2) apart
    row, matrix = 2 * (W + 2), (2 * T + 1) * (W + 2)
    want_row = row if T > 1 else W
    assert A.dense_strides(x) == [matrix if B > 1 else T * want_row, want_row]
    odd = torch.as_strided(base, (B, T, W), (7777 if B == 1 else matrix, 5555 if T == 1 else row, 1))
    assert A.dense_strides(odd) == A.dense_strides(x)
    if B == 1 or T == 1:
        assert A.dense_strides(odd) != list(odd.stride()[:2])
    else:
        assert A.dense_strides(x) == list(x.stride()[:2])
    if T == 1:
        assert A.dense_strides(x, dense_last=9) == [matrix if B > 1 else 9, 9]
    assert A.dense_strides(x[0]) == [want_row]               # two dimensions: rows of a matrix
