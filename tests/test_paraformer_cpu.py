"""The restatement of Paraformer's host loop (tests/paraformer_restatement.py) pinned by hand-derived cases — the reference has no unit
test of ParaformerCif or of the timestamp routine, so these cases are what says the restatement reads the Swift lines right —, the
text side of fluidaudio_amd.paraformer, and the argument contract of the four entries, which is answered without a device."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import paraformer_restatement as R  # noqa: E402

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- ParaformerCif.swift:19-50 by hand
H = np.array([[1.0, -2.0, 0.5], [4.0, 8.0, -1.0], [-3.0, 0.25, 2.0]], np.float32)


def test_two_halves_make_one_token_and_the_tail_adds_none():
    embeds, fires = R.integrate_and_fire(H[:2], [0.5, 0.5])
    assert fires == [1]                                   # 0.5 + 0.5 reaches 1.0 at frame 1; 0 + 0.45 stays below
    assert np.array_equal(bits(embeds), bits([F(0.5) * H[0] + F(0.5) * H[1]]))


def test_the_tail_frame_fires_with_the_zero_row():
    embeds, fires = R.integrate_and_fire(H, [0.25] * 3)
    assert fires == [3]                                   # 0.75 + 0.45 >= 1 at t == T
    want = (F(0.25) * H[0] + F(0.25) * H[1]) + F(0.25) * H[2]
    assert np.array_equal(bits(embeds), bits([want + F(0)]))


def test_an_alpha_above_one_fires_on_consecutive_frames():
    embeds, fires = R.integrate_and_fire(H[:2], [2.5, 0.0])
    assert fires == [0, 1]
    # t = 0: integrate 2.5, used = 2.5 - 1.5 = 1, leftover 1.5; t = 1: integrate 1.5, used = 0 - 0.5 (negative), leftover 0.5;
    # the tail: 0.5 + 0.45 < 1
    assert np.array_equal(bits(embeds), bits([F(1.0) * H[0], H[0] * F(1.5) + F(-0.5) * H[1]]))


def test_no_frames_no_tokens():
    embeds, fires = R.integrate_and_fire(np.zeros((0, 3), np.float32), [])
    assert fires == [] and embeds.shape == (0, 3)


def test_the_seed_is_a_product_and_keeps_the_sign_of_zero():
    embeds, fires = R.integrate_and_fire(np.array([[-1.0, 1.0]] * 4, np.float32), [0.5, 0.5, 0.5, 0.5])
    assert fires == [1, 3]                                # the leftover of frame 1 is exactly 0: the seed is [-0.0, 0.0]
    assert np.array_equal(bits(embeds[1]), bits([-1.0, 1.0])) and np.signbit(np.array([-1.0], np.float32) * F(0))[0]
    ac, n, fires, enc = R.decoder_inputs(np.array([[-1.0, 1.0]] * 4, np.float32), [0.5] * 4, enc_frames=6, max_tokens=1)
    assert n == 1 and fires == [1, 3] and ac.shape == (1, 2) and not enc[4:].any() and np.array_equal(enc[:4, 0], [-1.0] * 4)


# ---- the timestamp helpers (ParaformerManager.swift:262-358)
def test_fire_indices_subtract_one_not_the_threshold():
    thr = F(F(1.0) - F(1e-4))
    assert R.cif_wo_hidden_fire_indices([F(0.5)] * 6, thr) == [1, 3, 5]
    # 0.9999 reaches the threshold; the remainder is 0.9999 - 1 < 0, not 0
    assert R.cif_wo_hidden_fire_indices([thr, F(1e-4), thr], thr) == [0, 2]


def test_percentile_positions():
    for n, q, pos in [(1, 0.1, 0), (10, 0.1, 0), (11, 0.1, 1), (21, 0.1, 2), (31, 0.1, 3), (2, 0.5, 0), (3, 0.5, 1), (4, 0.5, 1), (5, 0.5, 2)]:
        values = np.arange(n, dtype=np.float32)[::-1] * F(2)
        assert R.percentile(values, q) == F(2 * pos), (n, q)
    assert R.percentile([], 0.1) == 0


def test_smoothing_needs_more_frames_than_the_window():
    x = np.array([1, 2, 6], np.float32)
    assert R.smooth(x, 3) is x
    y = R.smooth(np.array([1, 2, 6, 3], np.float32), 3)
    assert np.array_equal(bits(y), bits([F(3) / F(2), F(9) / F(3), F(11) / F(3), F(9) / F(2)]))


def test_envelope_frames():
    assert R.energy_envelope(np.ones(160, np.float32)).size == 0          # audio.count > hop is required
    assert R.energy_envelope(np.ones(161, np.float32)).tolist() == [1.0]
    assert R.energy_envelope(np.ones(479, np.float32)).size == 2
    tiny = R.energy_envelope(np.full(320, 1e-20, np.float32))
    assert tiny.size == 2 and 0.9e-20 < tiny[0] < 1.1e-20                   # the squares are denormal, not zero


def test_energy_span_runs_and_ties():
    env = np.zeros(20, np.float32)
    env[2:5] = 1
    env[8:11] = 1
    env[13:15] = 1                                                         # two frames: below minRun
    span = lambda a, b, c: R.energy_span(a, b, c, env, 0.01, F(0.5), 3)    # noqa: E731
    assert span(0.0, 0.195, 0.065) == (2 * 0.01, 4 * 0.01)                 # |6 - 12| == |18 - 12|: the first of equals
    assert span(0.0, 0.195, 0.075) == (8 * 0.01, 10 * 0.01)
    assert span(0.0, 0.195, 0.0) == (2 * 0.01, 4 * 0.01)
    assert span(0.035, 0.195, 0.0) == (8 * 0.01, 10 * 0.01)                # the window cuts the first run down to two frames
    assert span(0.115, 0.195, 0.14) is None                                # only the short run
    assert span(0.1, 0.1, 0.1) is None and R.energy_span(0.0, 1.0, 0.5, env[:0], 0.01, F(0.5), 3) is None
    assert span(0.0, 0.095, 0.2) == (2 * 0.01, 4 * 0.01)                   # a run ending at the window's end is cut to it: 8 ... 9 is too short


VOCAB = {0: "<blank>", 1: "<s>", 2: "</s>", 3: "▁he", 4: "llo", 5: "cu@@", 6: "t", 7: "▁", 8: "", 9: "▁wor@@", 10: "▁ld", 11: "x@@"}


def test_both_fire_paths():
    audio = np.zeros(16000, np.float32)
    keep = R.keep_table(VOCAB, 12)
    assert keep.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1]
    ids = [1, 3, 4, 0, 5, 6, 8, 2, 40, 4, 4, 4, 4, 4]                      # 9 kept: blank, <s>, </s>, the empty string and id 40 are dropped
    trace = {}
    raw = R.raw_spans(ids, keep, np.full(66, 0.051, np.float32), audio, trace)
    assert not trace["fallback"] and len(trace["fires"]) == 10 and [r[0] for r in raw] == [1, 2, 4, 5, 9, 10, 11, 12, 13]
    trace = {}
    raw = R.raw_spans(ids, keep, np.full(66, 0.2, np.float32), audio, trace)
    assert trace["fallback"] and len(raw) == min(9, len(trace["fires"]) - 1)
    # silence: every span is the fallback span from the cursor on
    assert trace["no_run"] == list(range(len(raw))) and raw[0][1] == 0.0 and all(a[2] == b[1] for a, b in zip(raw, raw[1:]))
    assert R.raw_spans([0, 1, 2, 8, 40], keep, np.full(66, 0.2, np.float32), audio) == []
    assert R.raw_spans(ids, keep, [], audio) == []                         # the tail alone, rescaled: one fire


def test_segment_emission(fa):
    pieces = ["▁he", "llo", "cu@@", "t", "▁", "▁wor@@", "▁ld", "x@@"]
    spans = [(-0.5, 0.1), (0.1, 0.2), (0.2, 0.3), (0.3, 0.4), (0.4, 0.5), (0.5, 0.6), (0.6, 0.7), (0.7, 0.8)]
    want = [(0.0, 0.1, "he"), (0.1, 0.2, "llo"), (0.2, 0.4, "cut"), (0.5, 0.7, "world"), (0.7, 0.8, "x")]
    assert R.segments_from_spans(pieces, spans) == want
    ids = np.array([3, 4, 5, 6, 7, 9, 10, 11], np.int32)
    rec = np.zeros(8, fa.PARAFORMER_SPAN_DTYPE)
    rec["token_index"] = np.arange(8)
    rec["start"], rec["end"] = [s for s, _ in spans], [e for _, e in spans]
    assert [tuple(s) for s in fa.segments_from_spans(VOCAB, ids, rec)] == want
    assert R.decode_tokens([1, 3, 4, 0, 7, 9, 10, 2, 99], VOCAB) == fa.decode_tokens([1, 3, 4, 0, 7, 9, 10, 2, 99], VOCAB) == "hello  wor@@ ld"
    assert fa.keep_table(VOCAB, 12).tolist() == R.keep_table(VOCAB, 12).tolist()
    assert fa.ParaformerConfig.pickEncoderBucket(129) == 256 and fa.ParaformerConfig.pickEncoderBucket(5000) == 1800


def test_argument_errors_without_a_device(fa):
    """NULL and negative sizes -> INVALID_ARGUMENT, counts beyond INT32_MAX -> INDEX_OVERFLOW, a well-formed call without a context ->
    INVALID_ARGUMENT; nothing is written."""
    lib = fa.lib()
    cfg = fa._lib.ParaformerCifConfig()
    lib.fa_paraformer_cif_default_config(C.byref(cfg))
    assert (cfg.threshold, round(cfg.tail_threshold, 6), cfg.max_tokens, cfg.enc_frames) == (1.0, 0.45, 128, 512)
    lib.fa_paraformer_cif_default_config(None)
    enc, alphas = np.zeros((2, 4, 8), np.float32), np.zeros((2, 4), np.float32)
    ac, tc, fc, ff = np.full((2, 128, 8), 7, np.float32), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full((2, 5), 7, np.int32)
    p = lambda a: a.ctypes.data   # noqa: E731

    def cif(f=lib.fa_paraformer_cif, enc=p(enc), dtype=0, batch=2, frames=4, dim=8, rs=8, ms=32, al=p(alphas), astride=4, ac_=p(ac), tc_=p(tc), fc_=p(fc), ff_=p(ff), c=cfg):
        return f(None, C.byref(c), enc, dtype, batch, frames, dim, rs, ms, al, astride, None, ac_, None, tc_, fc_, ff_)
    bad = [cif(batch=-1), cif(frames=-1), cif(dim=0), cif(rs=7), cif(ms=31), cif(astride=3), cif(dtype=2), cif(enc=None), cif(al=None), cif(ac_=None), cif(tc_=None),
           cif(fc_=None), cif(ff_=None), cif(f=lib.fa_paraformer_cif_dev, ff_=None)]
    assert bad == [1] * len(bad)
    zero = fa._lib.ParaformerCifConfig(1.0, 0.45, 0, 512)
    assert cif(c=zero) == 1
    assert cif(batch=1 << 20, frames=1 << 12, astride=1 << 12, ms=1 << 15) == 2 and cif(f=lib.fa_paraformer_cif_dev, batch=1 << 25) == 2
    assert cif() == 1 and cif(batch=0) == 1 and cif(f=lib.fa_paraformer_cif_dev) == 1       # well-formed, no context
    assert (ac == 7).all() and (tc == 7).all() and (fc == 7).all() and (ff == 7).all()

    ids, counts, keep = np.zeros((2, 128), np.int32), np.array([3, 128], np.int32), np.ones(5, np.uint8)
    audio, off = np.zeros(100, np.float32), np.array([0, 40, 100], np.int64)
    spans, utt, count = np.full(8, 7, fa.PARAFORMER_SPAN_DTYPE), np.full(2, 7, np.int64), C.c_int64(7)

    def stamps(f=lib.fa_paraformer_timestamps, al=p(alphas), astride=4, batch=2, frames=4, ids_=p(ids), tc_=p(counts), keep_=p(keep), vocab=5, audio_=p(audio), off_=p(off),
               cap=8, count_=C.byref(count)):
        return f(None, C.byref(cfg), al, astride, batch, frames, None, ids_, tc_, keep_, vocab, audio_, off_, p(spans), cap, count_, p(utt))
    over, down, below, huge = np.array([3, 129], np.int32), np.array([0, 50, 40], np.int64), np.array([-1, 40, 100], np.int64), np.array([0, 40, 1 << 32], np.int64)
    bad = [stamps(batch=-1), stamps(frames=-1), stamps(astride=3), stamps(vocab=-1), stamps(cap=-1), stamps(count_=None), stamps(al=None), stamps(ids_=None),
           stamps(tc_=None), stamps(keep_=None), stamps(audio_=None), stamps(off_=None), stamps(tc_=p(over)), stamps(tc_=p(-over)), stamps(off_=p(down)),
           stamps(off_=p(below)), stamps(f=lib.fa_paraformer_timestamps_dev, off_=p(down))]
    assert bad == [1] * len(bad)
    assert stamps(off_=p(huge)) == 2 and stamps(f=lib.fa_paraformer_timestamps_dev, off_=p(huge)) == 2
    assert stamps() == 1 and stamps(batch=0) == 1 and stamps(f=lib.fa_paraformer_timestamps_dev) == 1
    assert count.value == 7 and (utt == 7).all() and spans.tobytes() == np.full(8, 7, fa.PARAFORMER_SPAN_DTYPE).tobytes()
