"""TDT greedy control loop on the device vs the CPU restatement, over random joint-decision tables."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_logits_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def within_bound(got, ref, V1, W, dtype):
    """The elementwise bound of tests/tdt_logits_restatement.py beside the flat rtol: |confidence - reference| <= tolerance, for a contiguous,
    16-byte aligned matrix of rows of W logits (fp16 rows of even W are read as pairs); half an ulp more for the float32 table the oracle
    reads its probability from.  A reference of 0 (an undefined probability after the clamp) has to be met exactly."""
    form = "streaming" if V1 > R.FITS_LOGITS else ("pairs" if dtype == "float16" and W % 2 == 0 else "registers")
    ref = np.asarray(ref, np.float64)
    return bool((np.abs(np.asarray(got, np.float64) - ref) <= R.tolerance(ref, V1, form) + 2.0 ** -25 * ref).all())


@pytest.mark.parametrize("B,U,T,p_blank,seed", [(64, 40, 60, 0.7, 0), (200, 160, 188, 0.85, 1), (32, 12, 30, 0.3, 2)])
def test_batched_walk_matches_oracle(fa, gpu_ctx, oracle_mod, B, U, T, p_blank, seed):
    import torch
    rng = np.random.default_rng(seed)
    blank = 8192
    tok = rng.integers(0, 50, (B, U, T)).astype(np.int32)
    tok[rng.random((B, U, T)) < p_blank] = blank
    bn = rng.integers(0, 5, (B, U, T)).astype(np.int32)
    pr = rng.uniform(-0.2, 1.2, (B, U, T)).astype(np.float32)
    pr[rng.random((B, U, T)) < 0.01] = np.nan
    enc = rng.integers(max(2, T // 2), T + 1, B).astype(np.int32)
    enc[0] = 1                                           # guard (:110-112)
    af = np.minimum(enc, rng.integers(T // 2, T + 5, B)).astype(np.int32)
    t0 = rng.integers(0, 8, B).astype(np.int32)
    t0[1] = T + 3                                        # starts beyond the chunk (:150-152)
    last = (rng.random(B) < 0.4).astype(np.int32)
    goff = rng.integers(0, 400, B).astype(np.int32)
    ea = [None if rng.random() < 0.7 else int(goff[b] + rng.integers(0, 20)) for b in range(B)]
    bn[2, 0, :] = 6                                      # duration bin out of range -> per-chunk error status
    got = fa.tdt_decode_tables(torch.from_numpy(tok).cuda(), torch.from_numpy(bn).cuda(), torch.from_numpy(pr).cuda(), enc, af, t0,
                               last, goff, ea, max_out=256, ctx=gpu_ctx)
    for b in range(B):
        ref = oracle_mod.tdt_greedy(tok[b], bn[b], pr[b], enc[b], af[b], t0[b], bool(last[b]), goff[b], ea[b], max_out=256)
        g = got[b]
        assert g["status"] == ref["status"], b
        assert g["count"] == ref["count"] and g["final_u"] == ref["final_u"] and g["final_time"] == ref["final_time"], b
        for k in ("tokens", "timestamps", "durations"):
            np.testing.assert_array_equal(g[k], ref[k])
        np.testing.assert_array_equal(g["confidences"], ref["confidences"])
    assert got[0]["final_time"] is None and got[1]["final_time"] is None and got[2]["status"] == 5
    assert sum(g["count"] for g in got) > B   # the tables do produce tokens


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_walk_on_joint_logits_equals_walk_on_tables(fa, gpu_ctx, oracle_mod, dtype):
    """fa_tdt_greedy_logits_dev: the joint decisions (first-index argmax over the token logits, its softmax probability,
    first-index argmax over the duration logits) are taken inside the walk, on the visited rows only — the same result as
    building the decision tables for the whole (u, t) grid first (numpy) and walking those (CPU restatement)."""
    import torch
    rng = np.random.default_rng(11)
    B, U, T, V1, nd = 24, 40, 50, 130, 5
    blank = V1 - 1
    lg = rng.standard_normal((B, U, T, V1 + nd)).astype(np.float32)
    lg[..., blank] += 3.2                                  # ~75 % blanks
    lg[3, 0, 0, 5] = lg[3, 0, 0, 9] = 9.0                  # exact tie -> lowest index
    lg[4, 0, 1, :V1] = np.nan                              # NaN never wins: an all-NaN row decodes to token 0, probability 0
    lg[5, 0, :4, 7] = np.nan                              # one NaN among finite logits: the token is the finite argmax, the probability 0 after the clamp
    lg[6, 0, :4, :V1] = -np.inf                          # nothing above -inf: token 0, probability 0
    lg[7, 0, :4, 3:90] = -np.inf                          # -inf entries contribute nothing to the denominator
    lg = lg.astype(dtype)
    x = lg.astype(np.float32)
    tok = np.argmax(np.where(np.isnan(x[..., :V1]), -np.inf, x[..., :V1]), axis=-1).astype(np.int32)
    bn = np.argmax(x[..., V1:], axis=-1).astype(np.int32)
    mx = np.max(np.where(np.isnan(x[..., :V1]), -np.inf, x[..., :V1]), axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        pr = (1.0 / np.exp(x[..., :V1].astype(np.float64) - mx).sum(-1)).astype(np.float32)
    assert tok[3, 0, 0] == 5 and tok[4, 0, 1] == 0
    enc = rng.integers(T // 2, T + 1, B).astype(np.int32)
    t0 = rng.integers(0, 4, B).astype(np.int32)
    last = (rng.random(B) < 0.5).astype(np.int32)
    cfg = fa.TdtConfig(blank_id=blank)
    got = fa.tdt_decode_logits(torch.from_numpy(lg).cuda(), V1, enc, None, t0, last, None, None, config=cfg, max_out=256, ctx=gpu_ctx)
    for b in range(B):
        ref = oracle_mod.tdt_greedy(tok[b], bn[b], pr[b], enc[b], None, t0[b], bool(last[b]), 0, None, max_out=256, blank_id=blank)
        g = got[b]
        assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (ref["status"], ref["count"], ref["final_u"], ref["final_time"]), b
        for k in ("tokens", "timestamps", "durations"):
            np.testing.assert_array_equal(g[k], ref[k])
        np.testing.assert_allclose(g["confidences"], ref["confidences"], rtol=2e-5, atol=1e-7)
        assert within_bound(g["confidences"], ref["confidences"], V1, V1 + nd, dtype), b
    assert sum(g["count"] for g in got) > B


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("V1", [5, 64, 130, 1025, 1087, 1088, 1089, 2500])   # fp16 rows of even stride (5, 1025, 1087 + 5 durations) take the pair requests
def test_logits_walk_every_row_form_and_every_option(fa, gpu_ctx, oracle_mod, dtype, V1):
    """Round 5: the walk on joint logits is a state machine with one joint evaluation per iteration (tdt_walk); rows of up to 17 x 64 logits
    are decided from registers (row maximum + first index holding it, soft-max only when the token is emitted: tdt_logits_fits_kernel), longer
    rows in one streaming pass.  Every row form (1 .. 17 pieces, the 17th piece partly filled, both sides of the 1 088-logit boundary) with every
    per-chunk option of the entry — audio_frames, start frames beyond the chunk, last-chunk flush, global offsets, emit_after, a joint grid too
    small for the walk (OUTPUT_TOO_SMALL), room for fewer tokens than the walk emits — against the CPU restatement on tables built by numpy."""
    import torch
    rng = np.random.default_rng(V1)
    B, U, T, nd = 40, 14, 36, 5
    blank = V1 - 1
    lg = rng.standard_normal((B, U, T, V1 + nd)).astype(np.float32)
    lg[..., blank] += 2.0 + 0.25 * np.log2(V1)            # ~70 % blanks at every row length
    lg[3, 0, 0, 0] = lg[3, 0, 0, min(4, V1 - 2)] = 30.0    # exact tie -> lowest index
    lg[4, 0, 1, :V1] = np.nan                              # all NaN -> token 0, probability 0
    lg[5, 0, :4, min(2, V1 - 2)] = np.nan                  # one NaN among finite logits
    lg[6, 0, :4, :V1] = -np.inf                          # nothing above -inf -> token 0
    lg[7, 0, :3, V1 - 2] = 40.0                            # the maximum in the row's last-but-one slot (the clamped duplicates sit behind it)
    lg[8, 0, :3, V1:] = -np.inf                           # duration logits all -inf -> bin 0
    lg[9, 0, :3, V1 + 1] = np.nan                          # a NaN duration logit never wins
    lg = lg.astype(dtype)
    x = lg.astype(np.float32)
    xt = np.where(np.isnan(x[..., :V1]), -np.inf, x[..., :V1])
    tok = np.argmax(xt, axis=-1).astype(np.int32)
    xd = np.where(np.isnan(x[..., V1:]), -np.inf, x[..., V1:])
    bn = np.argmax(xd, axis=-1).astype(np.int32)
    mx = np.max(xt, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        pr = (1.0 / np.exp(x[..., :V1].astype(np.float64) - mx).sum(-1)).astype(np.float32)
    enc = rng.integers(T // 2, T + 1, B).astype(np.int32)
    enc[0] = 1
    af = np.minimum(enc, rng.integers(T // 2, T + 4, B)).astype(np.int32)
    t0 = rng.integers(0, 5, B).astype(np.int32)
    t0[1] = T + 2
    last = (rng.random(B) < 0.5).astype(np.int32)
    goff = rng.integers(0, 300, B).astype(np.int32)
    ea = [None if rng.random() < 0.6 else int(goff[b] + rng.integers(0, 12)) for b in range(B)]
    cfg = fa.TdtConfig(blank_id=blank)
    for max_out in (64, 1):                                 # 1: room for fewer tokens than the walk emits (OUTPUT_TOO_SMALL, counts keep counting)
        got = fa.tdt_decode_logits(torch.from_numpy(lg).cuda(), V1, enc, af, t0, last, goff, ea, config=cfg, max_out=max_out, ctx=gpu_ctx)
        statuses = set()
        for b in range(B):
            ref = oracle_mod.tdt_greedy(tok[b], bn[b], pr[b], enc[b], af[b], t0[b], bool(last[b]), goff[b], ea[b], max_out=max_out, blank_id=blank)
            g = got[b]
            statuses.add(ref["status"])
            assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (ref["status"], ref["count"], ref["final_u"], ref["final_time"]), (b, max_out)
            for k in ("tokens", "timestamps", "durations"):
                np.testing.assert_array_equal(g[k], ref[k])
            np.testing.assert_allclose(g["confidences"], ref["confidences"], rtol=3e-5, atol=1e-7)
            assert within_bound(g["confidences"], ref["confidences"], V1, V1 + nd, dtype), (b, max_out)
        assert 0 in statuses
        if max_out == 64:
            assert sum(g["count"] for g in got) > B // 2        # the rows do produce tokens


# ---- the rare rules of the walk, on hand-built tables: one chunk per rule.  Random tables almost never put ten zero-duration tokens on one frame
# or 150 tokens into a chunk, so the limits are small here: the oracle takes them as max_symbols / max_tokens / blank_limit.
RARE_B, RARE_U, RARE_T = 10, 16, 24
RARE_TOKENS, RARE_BLANKS = 4, 2                     # max_tokens_per_chunk, consecutive_blank_limit
(FORCE, ZERO_AFTER_EMIT, BLANK_ZERO, CAP_LAST, CAP_NOT_LAST, FLUSH_BLANKS, FLUSH_SYMBOLS, FLUSH_EMIT_AFTER, CAP_EXACT, FORCE_LAST) = range(RARE_B)


def rare_chunks():
    """tok [B, U, T] with -1 for the blank, bin [B, U, T] (bin k = duration k), and the per-chunk options.  Everything not set is a blank of
    duration 1: the walk moves one frame and stays at its u."""
    B, U, T = RARE_B, RARE_U, RARE_T
    tok, bn = np.full((B, U, T), -1, np.int32), np.ones((B, U, T), np.int32)
    enc, t0, last = np.full(B, T, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    af, goff, ea = enc.copy(), (10 * np.arange(B)).astype(np.int32), [None] * B

    def put(b, cells):
        for u, t, k, d in cells:
            tok[b, u, t], bn[b, u, t] = k, d

    # frame 5 answers a token of duration 0 at every u: the blank-advance loop arrives there, emits (0, 5), stays; the next outer step emits
    # (1, 5) with its duration raised to 1 (:318-323), which moves the walk to frame 6 — so no third token can share the timestamp, and only
    # max_symbols_per_step <= 2 reaches the force-advance (:453-462), which skips frame 6: the third token is then frame 7's
    for b in (FORCE, FORCE_LAST):
        put(b, [(u, 5, 1 + u % 5, 0) for u in range(U)] + [(2, 6, 5, 1), (2, 7, 6, 1)])
    last[FORCE_LAST] = 1
    put(ZERO_AFTER_EMIT, [(0, 3, 2, 0), (1, 3, 3, 0)])       # an outer step emits at frame 3 with duration 0; the next one is at frame 3 again
    t0[ZERO_AFTER_EMIT] = 3
    put(BLANK_ZERO, [(0, 0, -1, 0), (0, 1, -1, 0), (0, 2, 4, 2)])   # a blank of duration 0 in the outer step (:327-329) and in the blank-advance loop (:377-379)
    for b in (CAP_LAST, CAP_NOT_LAST, FLUSH_EMIT_AFTER):     # a fifth token at frame 4: the cap of 4 stops the walk behind it, at frame 5
        put(b, [(u, u, 1 + u, 1) for u in range(5)])
    last[CAP_LAST] = last[FLUSH_EMIT_AFTER] = 1
    put(CAP_LAST, [(4, 5, 6, 0)])                            # the flush starts at frame 5 with the predictor state of four tokens
    # flush tokens at frames 5, 9, 13 (durations 4, 4, 0 move the flush's frame pointer); emit_after cuts the walk's tokens and the first of them
    put(FLUSH_EMIT_AFTER, [(4, 5, 6, 4), (5, RARE_T - 1, 1, 4), (6, RARE_T - 2, 2, 0)])
    ea[FLUSH_EMIT_AFTER] = int(goff[FLUSH_EMIT_AFTER]) + 9
    # 20 of 24 frames hold audio: the walk ends at frame 20, the flush looks at frames min(20, 23), 19, 18 — a token, then two blanks
    af[FLUSH_BLANKS], t0[FLUSH_BLANKS], last[FLUSH_BLANKS] = 20, 17, 1
    put(FLUSH_BLANKS, [(0, 20, 1, 0), (1, 20, 5, 1), (1, 17, 5, 1)])
    # the walk jumps from frame 22 over the end; the flush finds a token at each of its frames 23, 23, 22
    t0[FLUSH_SYMBOLS], last[FLUSH_SYMBOLS] = 22, 1
    put(FLUSH_SYMBOLS, [(0, 22, -1, 2), (0, 23, 1, 3), (1, 23, 2, 0), (2, 22, 3, 1)])
    put(CAP_EXACT, [(u, 2 * u, 1 + u, 2) for u in range(4)])   # exactly max_tokens_per_chunk tokens: the cap does not fire
    return tok, bn, enc, af, t0, last, goff, ea


def rare_reference(oracle_mod, symbols, blank, prob):
    """The oracle on every chunk, after a look at ITS output: each table reaches the rule it was built for."""
    tok, bn, enc, af, t0, last, goff, ea = rare_chunks()
    tk = np.where(tok < 0, blank, tok).astype(np.int32)
    ref = [oracle_mod.tdt_greedy(tk[b], bn[b], prob[b], enc[b], af[b], t0[b], bool(last[b]), goff[b], ea[b], blank_id=blank, max_symbols=symbols,
                                 max_tokens=RARE_TOKENS, blank_limit=RARE_BLANKS, max_out=16) for b in range(RARE_B)]
    assert all(r["status"] == 0 for r in ref)
    ts = lambda b: (ref[b]["timestamps"] - goff[b]).tolist()   # noqa: E731
    T = RARE_T
    third = 7 if symbols <= 2 else 6                         # the force-advance skips frame 6
    assert ts(FORCE) == [5, 5, third] and ref[FORCE]["tokens"].tolist() == [1, 2, third - 1] and ref[FORCE]["durations"].tolist() == [0, 1, 1]
    assert ref[FORCE]["final_time"] == T and ref[FORCE]["joint_calls"] == 5 + 2 + (T - third)
    assert ts(FORCE_LAST)[:3] == ts(FORCE) and ref[FORCE_LAST]["joint_calls"] == ref[FORCE]["joint_calls"] + min(symbols, RARE_BLANKS)
    assert ts(ZERO_AFTER_EMIT) == [3, 3] and ref[ZERO_AFTER_EMIT]["durations"].tolist() == [0, 1] and ref[ZERO_AFTER_EMIT]["final_time"] == T
    assert ts(BLANK_ZERO) == [2] and ref[BLANK_ZERO]["joint_calls"] == 3 + (T - 4)      # frames 0, 1, 2, then 4 .. 23: no frame twice
    assert ref[CAP_NOT_LAST]["count"] == RARE_TOKENS and ts(CAP_NOT_LAST) == [0, 1, 2, 3]
    assert ref[CAP_NOT_LAST]["final_time"] == 5 and ref[CAP_NOT_LAST]["final_u"] == 4   # stopped mid-way, behind the fifth token's frame
    assert ts(CAP_LAST) == [0, 1, 2, 3, 5] and ref[CAP_LAST]["tokens"][4] == 6 and (ref[CAP_LAST]["final_time"], ref[CAP_LAST]["final_u"]) == (5, 5)
    assert ref[CAP_EXACT]["count"] == RARE_TOKENS and ref[CAP_EXACT]["final_time"] == T
    # the flush token's timestamp is min(fp, Teff - 1) + offset: frame pointer 20, 20 frames of audio
    assert ts(FLUSH_BLANKS) == [min(20, 20 - 1)] and ref[FLUSH_BLANKS]["final_time"] == 20
    assert ref[FLUSH_BLANKS]["joint_calls"] == 3 + min(symbols, 3)          # 3: frames 20, 19, 18 — all three variants —, ended by two blanks in a row
    assert ts(FLUSH_SYMBOLS) == [T - 1] * symbols and ref[FLUSH_SYMBOLS]["tokens"].tolist() == [1, 2, 3][:symbols]   # ended by max_symbols_per_step: no blank
    assert ref[FLUSH_SYMBOLS]["joint_calls"] == 1 + symbols and ref[FLUSH_SYMBOLS]["final_time"] == T
    assert ts(FLUSH_EMIT_AFTER) == [9, 13][:symbols - 1] and ref[FLUSH_EMIT_AFTER]["final_u"] == 4 + symbols          # five tokens cut, the walk's four among them
    return tk, bn, enc, af, t0, last, goff, ea, ref


def rare_compare(got, ref, exact, bound=None):
    for b in range(RARE_B):
        g, r = got[b], ref[b]
        assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (r["status"], r["count"], r["final_u"], r["final_time"]), b
        for k in ("tokens", "timestamps", "durations"):
            np.testing.assert_array_equal(g[k], r[k], err_msg=str(b))
        if exact:
            np.testing.assert_array_equal(g["confidences"], r["confidences"], err_msg=str(b))
        else:
            np.testing.assert_allclose(g["confidences"], r["confidences"], rtol=3e-5, atol=1e-7, err_msg=str(b))
            assert within_bound(g["confidences"], r["confidences"], *bound), b


# max_symbols_per_step = 3 with 4 tokens per chunk and 2 blanks in a row; = 2 as well, the largest value at which the force-advance can fire at all
@pytest.mark.parametrize("symbols", [3, 2])
def test_rare_rules_on_tables(fa, gpu_ctx, oracle_mod, symbols):
    import torch
    rng = np.random.default_rng(5)
    pr = rng.uniform(-0.2, 1.2, (RARE_B, RARE_U, RARE_T)).astype(np.float32)
    pr[rng.random(pr.shape) < 0.05] = np.nan
    tk, bn, enc, af, t0, last, goff, ea, ref = rare_reference(oracle_mod, symbols, 8192, pr)
    cfg = fa.TdtConfig(max_symbols_per_step=symbols, max_tokens_per_chunk=RARE_TOKENS, consecutive_blank_limit=RARE_BLANKS)
    got = fa.tdt_decode_tables(torch.from_numpy(tk).cuda(), torch.from_numpy(bn).cuda(), torch.from_numpy(pr).cuda(), enc, af, t0, last, goff, ea,
                               config=cfg, max_out=16, ctx=gpu_ctx)
    rare_compare(got, ref, exact=True)


# rows of 13 logits: one per request (W = 1); 14 halves: the pair route; 1 105: the streaming kernel
@pytest.mark.parametrize("V1,dtype", [(8, "float32"), (8, "float16"), (9, "float16"), (1100, "float32")])
@pytest.mark.parametrize("symbols", [3, 2])
def test_rare_rules_on_logits(fa, gpu_ctx, oracle_mod, symbols, V1, dtype):
    """The same decisions as logits: a large value on the chosen token and on the chosen bin, noise below it elsewhere."""
    import torch
    nd, blank = 5, V1 - 1
    tok, bn = rare_chunks()[:2]
    tk = np.where(tok < 0, blank, tok)
    rng = np.random.default_rng(V1)
    lg = (0.5 * rng.standard_normal((RARE_B, RARE_U, RARE_T, V1 + nd))).astype(np.float32)
    np.put_along_axis(lg, tk[..., None].astype(np.int64), 8.0, axis=-1)
    np.put_along_axis(lg, (V1 + bn)[..., None].astype(np.int64), 8.0, axis=-1)
    lg = lg.astype(dtype)
    x = lg.astype(np.float64)
    assert (np.argmax(x[..., :V1], -1) == tk).all() and (np.argmax(x[..., V1:], -1) == bn).all()
    pr = (1.0 / np.exp(x[..., :V1] - 8.0).sum(-1)).astype(np.float32)
    tk, bn, enc, af, t0, last, goff, ea, ref = rare_reference(oracle_mod, symbols, blank, pr)
    cfg = fa.TdtConfig(blank_id=blank, max_symbols_per_step=symbols, max_tokens_per_chunk=RARE_TOKENS, consecutive_blank_limit=RARE_BLANKS)
    got = fa.tdt_decode_logits(torch.from_numpy(lg).cuda(), V1, enc, af, t0, last, goff, ea, config=cfg, max_out=16, ctx=gpu_ctx)
    rare_compare(got, ref, exact=False, bound=(V1, V1 + nd, dtype))
