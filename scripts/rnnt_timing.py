"""Times fa_rnnt_greedy_logits_dev on one MI355X: the biased entry against the same entry unbiased on the same logits, alternating,
200 launches on resident operands between two device events (DESIGN.md quotes the figures).  A chunk of a streaming model: T = 16 frames, U = 24 decoder steps,
fp16 joint logits, 256 streams; random logits with blank on top of three frames in four, and pieces / terms drawn from a seed so
that partial matches occur.  --dry builds the tables and stops (no GPU needed)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vocabulary(rng, V1, n_terms):
    letters = "abcdefghijklmnopqrstuvwxyz"
    word = lambda lo, hi: "".join(rng.choice(list(letters), rng.integers(lo, hi)))  # noqa: E731
    pieces = [("▁" if rng.integers(0, 2) else "") + word(1, 5) for _ in range(V1 - 1)] + [None]
    terms = []
    for _ in range(n_terms):       # a term is a word spelt by two to four pieces, so that the decoder's own pieces continue it
        parts = [pieces[int(rng.integers(0, V1 - 1))].replace("▁", "") for _ in range(int(rng.integers(2, 5)))]
        terms.append("".join(parts))
    return pieces, terms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--terms", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    args = ap.parse_args()
    import fluidaudio_amd as fa
    results = []
    for V1 in (1025, 8193):
        rng = np.random.default_rng(V1)
        pieces, terms = vocabulary(rng, V1, args.terms)
        bias = fa.rnnt_bias_build(terms, pieces, vocab=V1)
        fresh = fa.rnnt_bias_candidates(bias)
        print(f"V1 {V1}: blob {bias.blob.size} words, tail_cap {bias.tail_cap}, {len(fresh)} fresh-start candidates", flush=True)
        if args.dry:
            continue
        import torch
        ctx = fa.default_context(0)
        B, U, T = args.streams, 24, 16
        g = torch.Generator(device="cuda").manual_seed(V1)
        # a spread of 8 between logits: a boost of 4.5 flips a decision now and then, as on speech, instead of every time
        x = 8.0 * torch.randn((B, U, T, V1), generator=g, device="cuda", dtype=torch.float32)
        x[..., V1 - 1] += torch.where(torch.rand((B, U, T), generator=g, device="cuda") < 0.75, 48.0, 0.0)
        x = x.to(torch.float16).contiguous()
        cfg = fa.RnntConfig(blank_id=V1 - 1)
        own = torch.cuda.ExternalStream(ctx.stream, device=ctx.device)
        torch.cuda.synchronize()

        import ctypes as C
        L, lib = fa._lib, fa.lib()
        c_cfg = cfg.c()
        d_frames = torch.full((B,), T, dtype=torch.int32, device="cuda")
        d_blob = torch.from_numpy(bias.blob).cuda()
        d_tail = torch.zeros((B, bias.tail_cap), dtype=torch.int32, device="cuda")
        d_len = torch.zeros(B, dtype=torch.int32, device="cuda")
        o_tok, o_frame, o_plain = (torch.zeros((B, U), dtype=torch.int32, device="cuda") for _ in range(3))
        o_cnt, o_fu, o_eou, o_st = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(4))
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        inner = 200                             # launches per timed window

        def call(b):
            """inner launches of the entry on resident operands between two device events -> ms per launch"""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(own):        # torch's fills, the events and the entry's launches on the context's stream
                e0.record(own)
                for _ in range(inner):
                    d_len.zero_()               # resetMatchState: every launch does the same work
                    ctx.check(lib.fa_rnnt_greedy_logits_dev(ctx.handle, C.byref(c_cfg), p(x), L.DTYPE_F16, B, U, T, V1, V1, p(d_frames), None,
                                                            p(d_blob) if b else None, int(bias.blob.size) if b else 0, bias.tail_cap if b else 0,
                                                            p(d_tail) if b else None, p(d_len) if b else None, U, p(o_tok), p(o_frame), p(o_plain), p(o_cnt),
                                                            p(o_fu), p(o_eou), p(o_st)), "fa_rnnt_greedy_logits_dev")
                e1.record(own)
            ctx.synchronize()
            torch.cuda.synchronize()
            assert int(o_st.max()) in (L.SUCCESS, L.OUTPUT_TOO_SMALL)
            return dict(count=int(o_cnt.sum()), flips=int((o_plain >= 0).logical_and(torch.arange(U, device="cuda")[None, :] < o_cnt[:, None]).sum())), e0.elapsed_time(e1) / inner

        for _ in range(3):                     # warm both
            call(None), call(bias)
        times = {"unbiased": [], "biased": []}
        for _ in range(args.repeats):          # alternating
            r0, t0 = call(None)
            r1, t1 = call(bias)
            times["unbiased"].append(t0)
            times["biased"].append(t1)
        tokens, flips = r1["count"], r1["flips"]
        decisions = tokens + B * T                             # every frame ends in a blank or the cap: an upper bound
        row = dict(V1=V1, streams=B, U=U, T=T, dtype="f16", blob_words=int(bias.blob.size), tail_cap=bias.tail_cap, fresh_candidates=len(fresh),
                   tokens=tokens, tokens_unbiased=r0["count"], flips=flips, decisions_at_most=decisions,
                   launch_ms={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in times.items()})
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out and not args.dry:
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
