"""Times fa_aed_step_dev on one MI355X against fa_ctc_greedy_batch_dev on the same rows (DESIGN.md quotes the figures).  Token feed,
penalty 1.1, n = 3, V = 16384, a history of 100 tokens, B in {1, 64, 1024}, fp32 and fp16.  A step advances its state, so every timed
launch is preceded by a device copy that puts the state back to the history of 100; the same copy precedes the yardstick's launches and
is also timed alone, and the figures below are launch + copy minus copy.  200 launches on resident operands between two device events
on the context's stream, the three alternating, the median of 10 rounds.  The yardstick reads the same bytes: B matrices of one frame
(one workgroup per row, as the step has) and one matrix of B frames.  --dry stops before the device work (no GPU needed)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC = 8.0e12          # bytes / s, MI355X data sheet
HBM_COPY = 6.29e12         # bytes / s, what a float4 copy reaches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    args = ap.parse_args()
    import fluidaudio_amd as fa
    cfg = fa.AedConfig.cohere()
    V, H = cfg.vocab, args.history
    assert H + 2 <= cfg.max_seq
    print(f"config: V {V}, max_seq {cfg.max_seq}, penalty {cfg.repetition_penalty:g}, n {cfg.no_repeat_ngram}, state {cfg.c().max_seq} tokens, history {H}", flush=True)
    if args.dry:
        return
    import torch
    L, lib = fa._lib, fa.lib()
    ctx = fa.default_context(0)
    own = torch.cuda.ExternalStream(ctx.stream, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for B in args.batches:
        for dtype in (torch.float32, torch.float16):
            g = torch.Generator(device="cuda").manual_seed(B)
            st = fa.AedDecodeState([[7]] * B, cfg, ctx=ctx)
            for _ in range(H):                                   # H steps of random rows without EOS: a history of H tokens, repeats and bans as they come
                x = (4.0 * torch.randn((B, V), generator=g, device="cuda")).to(dtype)
                x[:, cfg.eos_id] = -100.0
                st.step(x)
            ctx.synchronize()
            got = st.finish()
            assert (got.reasons == fa.AED_RUNNING).all() and (got.steps == H).all()
            saved = st.state.clone()
            x = (4.0 * torch.randn((B, V), generator=g, device="cuda")).to(dtype)
            x[:, cfg.eos_id] = -100.0
            dt = L.DTYPE_F16 if dtype == torch.float16 else L.DTYPE_F32
            c_cfg = cfg.c()
            ids, toks, lens = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
            torch.cuda.synchronize()

            def launch(kind):
                if kind == "step":
                    ctx.check(lib.fa_aed_step_dev(ctx.handle, C.byref(c_cfg), B, p(st.state), p(x), dt, V, p(st.input_id), p(st.position_id), None, 0, None, None), "fa_aed_step_dev")
                elif kind == "argmax_rows":                      # B matrices of one frame
                    ctx.check(lib.fa_ctc_greedy_batch_dev(ctx.handle, p(x), dt, B, 1, V, V, V, None, V - 1, p(ids), p(toks), p(lens)), "fa_ctc_greedy_batch_dev")
                elif kind == "argmax_matrix":                    # one matrix of B frames
                    ctx.check(lib.fa_ctc_greedy_batch_dev(ctx.handle, p(x), dt, 1, B, V, V, B * V, None, V - 1, p(ids), p(toks), p(lens)), "fa_ctc_greedy_batch_dev")

            def window(kind):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(own):
                    e0.record(own)
                    for _ in range(args.inner):
                        st.state.copy_(saved)
                        launch(kind)
                    e1.record(own)
                ctx.synchronize()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / args.inner    # microseconds per (copy + launch)

            kinds = ("copy", "step", "argmax_rows", "argmax_matrix")
            for k in kinds:
                window(k), window(k)
            times = {k: [] for k in kinds}
            for _ in range(args.repeats):
                for k in kinds:
                    times[k].append(window(k))
            med = {k: float(np.median(v)) for k, v in times.items()}
            step, a_rows, a_mat = (max(med[k] - med["copy"], 1e-3) for k in ("step", "argmax_rows", "argmax_matrix"))
            nbytes = B * V * x.element_size()
            row = dict(B=B, dtype=str(dtype).split(".")[-1], history=H, bytes_per_step=nbytes, us=dict(copy=med["copy"], step=step, argmax_rows=a_rows, argmax_matrix=a_mat),
                       spread_us={k: [float(np.min(v)), float(np.max(v))] for k, v in times.items()},
                       hbm_fraction_spec=nbytes / (step * 1e-6) / HBM_SPEC, hbm_fraction_copy=nbytes / (step * 1e-6) / HBM_COPY,
                       step_over_argmax_rows=step / a_rows, step_over_argmax_matrix=step / a_mat)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
