"""fa_rnnt_greedy_logits_dev (csrc/rnnt.hip: rnnt_greedy_kernel<false>, <true>) against the restatement of the reference
(tests/rnnt_restatement.py) on the calls of tests/rnnt_cases.py: vocab_with_blank = 3 (two calls, see rnnt_cases), 129, 1 025 and
8 193, fp32 and fp16, two of the vocabularies with a form of 70 scalars (tail_cap > 64).  The launch plan has no row-length switch
(rnnt_launch.h), so there are no lengths on either side of one.  tests/test_rnnt_cpu.py proves that every call holds every decision
kind.  Everything compared is an integer and must be EQUAL: tokens, frames, the displaced plain argmax, counts, final_u, eou, status,
the tail and its length — the only arithmetic is one fp32 add.  No test feeds the kernel a malformed blob
(tests/test_rnnt_bias_core_asan.py walks those on the host)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_cases as K  # noqa: E402
import rnnt_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [c.name for c in K.CALLS]
SENTINEL = 77


def config_of(fa, t):
    return fa.RnntConfig(blank_id=t.v.blank, eou_id=t.v.eou, max_symbols_per_step=K.MAX_SYMBOLS)


def bias_of(fa, t, terms=None, vocab=None):
    return fa.rnnt_bias_build(t.v.terms if terms is None else terms, t.v.pieces, vocab=t.call.V1 if vocab is None else vocab)


def same(got, want, where, tail=True):
    assert (got["status"], got["count"], got["final_u"], got["eou"]) == (want["status"], want["count"], want["final_u"], want["eou"]), (where, got, want)
    for key in ("tokens", "frames", "flips") + (("tail",) if tail else ()):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{where} {key}")


@pytest.mark.parametrize("call", K.CALLS, ids=IDS)
def test_biased_walk(fa, gpu_ctx, call):
    import torch
    t = K.table(call)
    bias = bias_of(fa, t)
    assert (bias.tail_cap == 70) == call.long and bias.tail_cap == K.new_bias(t).tail_cap
    got = fa.rnnt_decode_logits(torch.from_numpy(t.logits).cuda(), call.V1, t.frames, t.skip, bias=bias, config=config_of(fa, t), max_out=call.max_out, ctx=gpu_ctx)
    assert len(got) == t.B
    for b in range(t.B):
        same(got[b], t.expected[b], f"{call.name} stream {b}")
    assert any((r["flips"] >= 0).any() for r in got)


@pytest.mark.parametrize("call", K.CALLS, ids=IDS)
def test_unbiased_walk_and_a_vocabulary_that_matches_nothing(fa, gpu_ctx, call):
    """d_bias = NULL equals the restatement without a vocabulary; a blob whose terms match no piece equals that call bit for bit."""
    import torch
    t = K.table(call)
    x = torch.from_numpy(t.logits).cuda()
    kw = dict(config=config_of(fa, t), max_out=call.max_out, ctx=gpu_ctx)
    plain = fa.rnnt_decode_logits(x, call.V1, t.frames, t.skip, **kw)
    inert_bias = bias_of(fa, t, ["wvu wvu"])
    assert inert_bias.blob.size and fa.rnnt_bias_candidates(inert_bias) == {}
    inert = fa.rnnt_decode_logits(x, call.V1, t.frames, t.skip, bias=inert_bias, **kw)
    for b in range(t.B):
        want = K.run(t, b, bias=None)
        same(plain[b], want, f"{call.name} stream {b} unbiased")
        same(inert[b], plain[b], f"{call.name} stream {b} inert", tail=False)
        assert plain[b]["tail"].size == 0 and not (plain[b]["flips"] >= 0).any()


@pytest.mark.parametrize("name", ["f32_V3", "f16_V129", "f32_V1025_long", "f16_V8193_long"])
def test_split_chunk_carries_the_match_state(fa, gpu_ctx, name):
    """A chunk split at a frame into two calls — the second's logits re-based at the first's final_u, the tail carried over — equals the
    one call."""
    import torch
    call = K.BY_NAME[name]
    t = K.table(call)
    U, split = call.U, 3
    bias, cfg = bias_of(fa, t), config_of(fa, t)
    x = torch.from_numpy(t.logits).cuda()
    first = fa.rnnt_decode_logits(x, call.V1, [min(f, split) for f in t.frames], t.skip, bias=bias, config=cfg, max_out=U, ctx=gpu_ctx)
    rebased = np.full_like(t.logits, 50.0)
    for b in range(t.B):
        rebased[b, :U - first[b]["final_u"]] = t.logits[b, first[b]["final_u"]:]
    second = fa.rnnt_decode_logits(torch.from_numpy(rebased).cuda(), call.V1, t.frames, [max(split, s) for s in t.skip], bias=bias,
                                   tails=[r["tail"] for r in first], config=cfg, max_out=U, ctx=gpu_ctx)
    carried = 0
    for b in range(t.B):
        whole = K.run(t, b, max_out=U)
        if first[b]["eou"] or first[b]["status"] != R.SUCCESS:
            same(first[b], K.run(t, b, frames=min(t.frames[b], split), max_out=U), f"{name} stream {b} first part")
            continue
        carried += first[b]["tail"].size > 0 and bool((second[b]["flips"] >= 0).any())     # a flip of the second call hangs on the first call's tail
        if whole["status"] != R.SUCCESS:      # the one call runs out of its U rows; the second call has U rows of its own: equal up to there
            for key in ("tokens", "frames", "flips"):
                np.testing.assert_array_equal(np.concatenate([first[b][key], second[b][key]])[:whole["count"]], whole[key], err_msg=f"{name} stream {b} {key}")
            continue
        for key in ("tokens", "frames", "flips"):
            np.testing.assert_array_equal(np.concatenate([first[b][key], second[b][key]]), whole[key], err_msg=f"{name} stream {b} {key}")
        assert first[b]["final_u"] + second[b]["final_u"] == whole["final_u"] and second[b]["eou"] == whole["eou"], (name, b)
        assert first[b]["count"] + second[b]["count"] == whole["count"]
        np.testing.assert_array_equal(second[b]["tail"], whole["tail"], err_msg=f"{name} stream {b} tail")
    assert carried >= 1


def test_a_blob_for_another_vocabulary_is_refused_per_stream(fa, gpu_ctx):
    """A WELL-FORMED blob built for another vocab (or used with another tail_cap): INVALID_ARGUMENT in d_status, no tokens, the tail untouched."""
    import torch
    call = K.BY_NAME["f32_V129"]
    t = K.table(call)
    x = torch.from_numpy(t.logits).cuda()
    other = bias_of(fa, t, vocab=call.V1 + 1)
    tails = [[0x2581, 0x61]] * t.B
    for bias in (other._replace(vocab=call.V1), bias_of(fa, t)._replace(tail_cap=9)):
        got = fa.rnnt_decode_logits(x, call.V1, t.frames, t.skip, bias=bias, tails=tails, config=config_of(fa, t), max_out=call.max_out, ctx=gpu_ctx)
        for b, g in enumerate(got):
            assert (g["status"], g["count"], g["final_u"], g["eou"], g["tokens"].size) == (fa._lib.INVALID_ARGUMENT, 0, 0, False, 0), b
            assert g["tail"].tolist() == [0x2581, 0x61]


def test_entry_contract(fa, gpu_ctx):
    """Every refusal of the header's list is FA_INVALID_ARGUMENT before any launch: the sentinel-filled outputs are untouched.  The
    same call with good arguments succeeds."""
    import torch
    lib, L = fa._lib, fa.lib()
    call = K.BY_NAME["f32_V129"]
    t = K.table(call)
    B, U, T, W = t.logits.shape
    x = torch.from_numpy(t.logits).cuda()
    frames = torch.tensor(t.frames, dtype=torch.int32, device="cuda")
    bias = bias_of(fa, t)
    blob = torch.from_numpy(bias.blob).cuda()
    cfg = config_of(fa, t).c()

    def outputs():
        o = {k: torch.full((B, U), SENTINEL, dtype=torch.int32, device="cuda") for k in ("tok", "frame", "plain")}
        o.update({k: torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda") for k in ("count", "final_u", "eou", "status")})
        o["tail"] = torch.full((B, bias.tail_cap), SENTINEL, dtype=torch.int32, device="cuda")
        o["tail_len"] = torch.zeros(B, dtype=torch.int32, device="cuda")
        return o

    good = dict(ctx=gpu_ctx.handle, cfg=C.byref(cfg), x=x.data_ptr(), dtype=lib.DTYPE_F32, B=B, U=U, T=T, V1=call.V1, W=W, frames=frames.data_ptr(),
                blob=blob.data_ptr(), cap=bias.tail_cap, max_out=U)

    def entry(o, drop=(), **change):
        a = dict(good, **change)
        p = lambda name: None if name in drop else C.c_void_p(o[name].data_ptr())  # noqa: E731
        q = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
        st = L.fa_rnnt_greedy_logits_dev(a["ctx"], a["cfg"], q(a["x"]), a["dtype"], a["B"], a["U"], a["T"], a["V1"], a["W"], q(a["frames"]), None, q(a["blob"]),
                                         bias.blob.size, a["cap"], p("tail"), p("tail_len"), a["max_out"], p("tok"), p("frame"), p("plain"), p("count"),
                                         p("final_u"), p("eou"), p("status"))
        gpu_ctx.synchronize()
        return st

    refusals = {"null_cfg": dict(cfg=None), "null_logits": dict(x=None), "null_frames": dict(frames=None), "batch_0": dict(B=0), "batch_negative": dict(B=-1),
                "U_0": dict(U=0), "T_0": dict(T=0), "vocab_0": dict(V1=0), "stride_below_vocab": dict(W=call.V1 - 1), "tail_cap_negative": dict(cap=-1),
                "tail_cap_257": dict(cap=257), "dtype": dict(dtype=7), "max_out_negative": dict(max_out=-1)}
    for name, change in refusals.items():
        o = outputs()
        assert entry(o, **change) == lib.INVALID_ARGUMENT, name
        assert all(bool((v == SENTINEL).all()) for k, v in o.items() if k != "tail_len"), name
    for drop in ("tail", "tail_len", "tok", "frame", "plain", "count", "final_u", "eou", "status"):
        o = outputs()
        assert entry(o, drop=(drop,)) == lib.INVALID_ARGUMENT, drop
        assert all(bool((v == SENTINEL).all()) for k, v in o.items() if k != "tail_len"), drop
    o = outputs()
    assert entry(o) == lib.SUCCESS
    r = K.run(t, 0, max_out=U)
    assert int(o["count"][0]) == r["count"] and o["tok"][0, :r["count"]].cpu().numpy().tolist() == r["tokens"].tolist()
    assert int(o["tail_len"][0]) == len(r["tail"]) and o["tail"][0, :len(r["tail"])].cpu().numpy().tolist() == r["tail"].tolist()
