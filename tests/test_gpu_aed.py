"""The AED unit on the device against the restatement (tests/aed_restatement.py) over the shared cases (tests/aed_cases.py): every step
of both feeds (tokens, counts, end reasons, steps, input_id, position_id, the Canary input_ids / decoder_mask, the self-mask row), the
masks, the context transpose, the hidden gather and the seam merge.  Every comparison is EQUAL: the values are integers or exactly
rounded fp32.  Rows of finished utterances and — in the token feed — of the discarded prompt steps are NaN, as is the padding."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aed_cases as K  # noqa: E402
import aed_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = K.scripted_cases() + K.random_cases()


def bits(t):
    """a mask tensor as numbers that compare exactly: float32 as it is, float16 as its bits"""
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.float16 else t.cpu().numpy()


def run_decode(fa, ctx, case, mask, poison_discarded, offset):
    import torch
    cfgd, prompts, rows = case["cfg"], case["prompts"], case["rows"]
    keys = ("mode", "vocab", "eos_id", "max_seq", "max_new", "no_repeat_ngram", "repetition_penalty", "window_tokens", "min_match", "chunk_samples", "hop_samples")
    cfg = fa.AedConfig(**{k: cfgd[k] for k in keys})
    seq, V, S, B = cfgd["mode"] == 1, cfgd["vocab"], cfgd["max_seq"], len(prompts)
    feeds = [(R.SequenceFeed if seq else R.TokenFeed)(p, cfgd) for p in prompts]
    st = fa.AedDecodeState(prompts, cfg, self_mask=mask, ctx=ctx)
    f16 = mask == "float16"
    want_in = np.array([f.input_id() for f in feeds], np.int32) if not seq else None
    want_pos = np.zeros(B, np.int32)
    want_mask = np.stack([R.self_mask_row(0, S, f16) for _ in feeds]) if mask and not seq else None

    def compare(where):
        got = st.finish()
        assert [t.tolist() for t in got.tokens] == [f.output_tokens for f in feeds], where
        assert got.counts.tolist() == [len(f.output_tokens) for f in feeds] and got.reasons.tolist() == [f.reason for f in feeds], where
        assert got.steps.tolist() == [f.pos if seq else f.step_index for f in feeds], where
        if seq:
            assert np.array_equal(st.input_ids.cpu().numpy(), np.stack([f.input_ids for f in feeds])), where
            assert np.array_equal(st.decoder_mask.cpu().numpy(), np.stack([f.decoder_mask for f in feeds])), where
        else:
            assert np.array_equal(st.input_id.cpu().numpy(), want_in) and np.array_equal(st.position_id.cpu().numpy(), want_pos), where
            if mask:
                assert np.array_equal(bits(st.self_mask), want_mask), where

    compare("begin")
    W = V + 3 + offset                                                            # a row stride above V: odd, so the rows' alignment differs
    for s, now in enumerate(list(rows) + [np.zeros_like(rows[0])] if len(rows) else []):
        host = np.full((B, W), np.nan, rows.dtype)                                # the padding, finished utterances and discarded rows: NaN
        for b, f in enumerate(feeds):
            if f.reason == R.RUNNING and s < len(rows) and not (poison_discarded and not seq and not f.decides()):
                host[b, offset:offset + V] = now[b]
        d = torch.from_numpy(host).to(f"cuda:{ctx.device}")
        st.step(d[:, offset:offset + V])
        for b, f in enumerate(feeds):
            if f.reason != R.RUNNING:
                continue
            f.step(now[b])
            if not seq and f.reason == R.RUNNING:                                 # an utterance that goes on gets the next step's inputs
                want_in[b], want_pos[b] = f.input_id(), f.position_id()
                if mask:
                    want_mask[b] = R.self_mask_row(f.step_index, S, f16)
        compare(f"step {s}")
    assert all(f.reason != R.RUNNING for f in feeds)
    tok, cnt, why, steps = st.finish_dev()
    got = st.finish()
    assert np.array_equal(cnt.cpu().numpy(), got.counts) and np.array_equal(why.cpu().numpy(), got.reasons) and np.array_equal(steps.cpu().numpy(), got.steps)
    assert tok.shape == (B, cfg.max_out) and [tok[b, :got.counts[b]].tolist() for b in range(B)] == [t.tolist() for t in got.tokens]
    assert all(not tok[b, got.counts[b]:].any() for b in range(B))


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_decode_steps_equal_the_restatement(fa, gpu_ctx, index):
    case = CASES[index]
    run_decode(fa, gpu_ctx, case, (None, "float32", "float16")[index % 3], False, index % 2)
    if case["cfg"]["mode"] == 0:                                                  # the discarded prompt steps' rows are never read
        run_decode(fa, gpu_ctx, case, ("float16", None, "float32")[index % 3], True, (index + 1) % 2)


def test_decode_refusals_and_sizes(fa, gpu_ctx):
    cfg = fa.AedConfig.cohere()
    assert cfg.max_out == 108 and fa.AedConfig.canary().max_out == 128 and fa.AedConfig(max_new=4, max_seq=16).max_out == 5
    with pytest.raises(fa.FluidAudioHipError):
        fa.AedDecodeState([[1], []], cfg, ctx=gpu_ctx)                            # P < 1
    with pytest.raises(fa.FluidAudioHipError):
        fa.AedDecodeState([[1] * 109], cfg, ctx=gpu_ctx)                          # a prompt beyond max_seq
    with pytest.raises(fa.FluidAudioHipError):
        fa.AedDecodeState([[1]], fa.AedConfig(vocab=0), ctx=gpu_ctx)


@pytest.mark.parametrize("f16", [False, True])
def test_cross_mask(fa, gpu_ctx, f16):
    valid = [0, 1, 17, 64, 65, 437, 438, 439, 9999, -5]
    for length in (1, 65, 438):
        got = bits(fa.aed_cross_attention_mask(valid, length, "float16" if f16 else "float32", ctx=gpu_ctx))
        assert np.array_equal(got, np.stack([R.cross_mask(length, v, f16) for v in valid]))


@pytest.mark.parametrize("D,T,pad,dtype", [(64, 1, 0, "float32"), (64, 63, 1, "float16"), (100, 188, 4, "float32"), (100, 63, 0, "float16"), (64, 188, 4, "float16"), (100, 1, 7, "float32")])
def test_encoder_context(fa, gpu_ctx, D, T, pad, dtype):
    import torch
    rng = np.random.default_rng(D * 1000 + T)
    B = 3
    host = rng.standard_normal((B, D, T + pad)).astype(dtype)
    host[:, :, T:] = np.nan                                                       # the stride padding is never read
    lengths = [0, T // 2 + 1, T + 5]
    d = torch.from_numpy(host).to(f"cuda:{gpu_ctx.device}")
    emb, mask = fa.aed_encoder_context(d[:, :, :T], lengths, ctx=gpu_ctx)
    assert emb.shape == (B, T, D) and emb.dtype == torch.float32 and emb.is_contiguous()
    assert np.array_equal(emb.cpu().numpy(), host[:, :, :T].transpose(0, 2, 1).astype(np.float32))
    assert np.array_equal(mask.cpu().numpy(), np.stack([R.context_mask(n, T) for n in lengths]))
    if T == 63:                                                                   # the element loop of the reference on one matrix; a time-major producer
        want, _ = R.decoder_context(host[1, :, :T], lengths[1])
        assert np.array_equal(emb[1].cpu().numpy(), want)
        td = torch.from_numpy(np.ascontiguousarray(host[:, :, :T].transpose(0, 2, 1))).to(d.device)
        emb2, _ = fa.aed_encoder_context(td.permute(0, 2, 1), lengths, ctx=gpu_ctx)
        assert torch.equal(emb2, emb)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_gather_hidden_rows(fa, gpu_ctx, dtype):
    import torch
    cfgd = K.seq_cfg(12, 12)
    cfg = fa.AedConfig(**{k: cfgd[k] for k in ("mode", "vocab", "eos_id", "max_seq", "max_new", "no_repeat_ngram", "repetition_penalty")})
    prompts = [[7, 7, 4], [1], [2] * 12, [5] * 11]                               # pos 3, 1, 12 (capped at begin), 11
    st = fa.AedDecodeState(prompts, cfg, ctx=gpu_ctx)
    S, D = 12, 70
    host = np.random.default_rng(3).standard_normal((4, S, D + 2)).astype(dtype)
    d = torch.from_numpy(host).to(f"cuda:{gpu_ctx.device}")
    got = st.gather_hidden(d[:, :, 1:D + 1]).cpu().numpy()                        # a padded row: element 1 ... D of D + 2
    want = np.zeros((4, D), np.float32)
    for b, pos in ((0, 3), (1, 1), (3, 11)):
        want[b] = host[b, pos - 1, 1:D + 1].astype(np.float32)
    assert np.array_equal(got, want)
    logits = np.full((4, 12), -1.0, np.float32)
    logits[:, 6] = 1.0
    logits[1, 3] = 5.0                                                            # utterance 1 ends with EOS, utterance 3 reaches pos == S: no longer gathered
    st.step(torch.from_numpy(logits).to(d.device))
    tm = torch.from_numpy(np.ascontiguousarray(host.transpose(1, 0, 2))).to(d.device).permute(1, 0, 2)   # [S][B][D] storage: other strides
    got = st.gather_hidden(tm[:, :, :D]).cpu().numpy()
    want = np.zeros((4, D), np.float32)
    want[0] = host[0, 3, :D].astype(np.float32)
    assert np.array_equal(got, want)


def check_merge(fa, ctx, recordings, wt, mm, dev):
    import torch
    if dev:
        flat = [t for r in recordings for w in r for t in w]
        offs = np.concatenate([[0], np.cumsum([len(w) for r in recordings for w in r])]).astype(np.int64)
        rng = np.concatenate([[0], np.cumsum([len(r) for r in recordings])]).astype(np.int64)
        got = fa.aed_merge_token_windows_dev(torch.tensor(flat, dtype=torch.int32, device=f"cuda:{ctx.device}"), offs, rng, wt, mm, ctx=ctx)
        tokens = got.tokens.cpu().numpy()
    else:
        got = fa.aed_merge_token_windows(recordings, window_tokens=wt, min_match=mm, ctx=ctx)
        tokens = got.tokens
    w = 0
    for r, windows in enumerate(recordings):
        merged, seams = R.merge_recording(windows, wt, mm)
        assert tokens[got.out_range[r]:got.out_range[r] + got.counts[r]].tolist() == merged, (r, wt)
        assert list(zip(got.best_len[w:w + len(windows)].tolist(), got.best_s_end[w:w + len(windows)].tolist())) == seams, (r, wt)
        w += len(windows)


@pytest.mark.parametrize("dev", [False, True])
def test_merge_shared_cases(fa, gpu_ctx, dev):
    for name, windows, wt, mm, want in K.MERGE_LITERAL + K.MERGE_OWN:
        check_merge(fa, gpu_ctx, [windows], wt, mm, dev)
        if want is not None:
            assert fa.aed_merge_token_streams(windows[0], windows[1], wt, mm, ctx=gpu_ctx) == want, name
    by_window = {}
    for _, windows, wt, mm, _ in K.MERGE_LITERAL + K.MERGE_OWN:                   # ... and batched: every case of one (window, min_match) in one call
        by_window.setdefault((wt, mm), []).append(windows)
    for (wt, mm), recordings in by_window.items():
        check_merge(fa, gpu_ctx, recordings, wt, mm, dev)


@pytest.mark.parametrize("wt", [1, 7, 32, 64])
def test_merge_random_streams(fa, gpu_ctx, wt):
    recordings = K.random_merge_recordings(40 + wt, 70, wt)
    for mm in (4, 1, 2):
        check_merge(fa, gpu_ctx, recordings, wt, mm, mm != 1)
    with pytest.raises(fa.FluidAudioHipError):
        fa.aed_merge_token_windows(recordings, window_tokens=65, ctx=gpu_ctx)
    with pytest.raises(fa.FluidAudioHipError):
        fa.aed_merge_token_windows(recordings, window_tokens=0, ctx=gpu_ctx)
