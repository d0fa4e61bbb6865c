"""What the language mode of the TDT walk costs ("TDT language mode").  At the bench leg's shape — B chunks of joint logits
[U = 64, T = 188, V1 + 5] fp32 resident in HBM, ~75 % blanks — it times, alternately and in one process:

  plain        fa_tdt_greedy_logits_dev of this library
  baseline     the same entry of another build of the library (--baseline-lib: the parent commit's), on the same logits
  lang_never   fa_tdt_greedy_logits_lang_dev with a table in which every token matches: one class byte per non-blank decision
  lang_p       the same entry with a share p of the vocabulary in the wrong script (--shares), top_k = 64, blocklist on (2 % of the
               tokens on it): the replaced decisions are counted by the device (swap_counts) and, on the first chunks, by the float64
               restatement (tests/tdt_lang_restatement.py), which must agree

Each arm is timed `--rounds` times as `--reps` back-to-back calls between two device events; the table gives the median and the spread
(min .. max) of every arm, the plain entry's change against the baseline beside the spread of both, and the ratios to the plain entry.

    python scripts/tdt_lang_time.py --vocab 1025 --chunks 1024 [--baseline-lib path/to/libfluidaudio_hip.so]
    python scripts/tdt_lang_time.py --vocab 8193 --chunks 256        # the fp32 grid of 1 024 chunks would be 404 GB
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=1025)
    ap.add_argument("--chunks", type=int, default=1024)
    ap.add_argument("--U", type=int, default=64)
    ap.add_argument("--T", type=int, default=188)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shares", type=float, nargs="*", default=[0.01, 0.1])
    ap.add_argument("--check-chunks", type=int, default=2)
    ap.add_argument("--baseline-lib", default=None)
    a = ap.parse_args()
    import torch

    import fluidaudio_amd as fa
    import tdt_lang_restatement as G
    from fluidaudio_amd import _lib as L
    B, U, T, V1, nd = a.chunks, a.U, a.T, a.vocab, 5
    W = V1 + nd
    ctx = fa.default_context(0)
    gen = torch.Generator(device="cuda").manual_seed(17)
    lg = torch.empty((B, U, T, W), device="cuda", dtype=torch.float32)
    for b0 in range(0, B, 64):                                    # the logits of bench.py's tdt leg
        part = torch.randn((min(64, B - b0), U, T, W), generator=gen, device="cuda", dtype=torch.float32)
        part[..., V1 - 1] += 4.0
        lg[b0:b0 + 64] = part
        del part
    cfg = fa.TdtConfig(blank_id=V1 - 1).c()
    enc = torch.full((B,), T, dtype=torch.int32, device="cuda")
    o = [torch.zeros((B, U), dtype=torch.int32, device="cuda") for _ in range(4)]
    o_conf = torch.zeros((B, U), dtype=torch.float32, device="cuda")
    o1 = [torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(4)]
    swaps = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    pp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = torch.cuda.ExternalStream(ctx.stream)

    def plain_of(lib, handle):
        def run():
            st = lib.fa_tdt_greedy_logits_dev(handle, C.byref(cfg), pp(lg), L.DTYPE_F32, B, U, T, V1, W, pp(enc), None, None, None, None, None, U, pp(o[0]),
                                              pp(o[1]), pp(o[2]), pp(o_conf), pp(o1[0]), pp(o1[1]), pp(o1[2]), pp(o1[3]))
            assert st == 0, st
        return run

    def lang_of(classes):
        d_cls = torch.from_numpy(classes).cuda()

        def run():
            ctx.check(fa.lib().fa_tdt_greedy_logits_lang_dev(ctx.handle, C.byref(cfg), pp(lg), L.DTYPE_F32, B, U, T, V1, W, pp(enc), None, None, None, None, None, U,
                                                             pp(o[0]), pp(o[1]), pp(o[2]), pp(o_conf), pp(o1[0]), pp(o1[1]), pp(o1[2]), pp(o1[3]), pp(d_cls), 0, 1, 64,
                                                             pp(o[3]), pp(swaps)), "fa_tdt_greedy_logits_lang_dev")
        run.classes = d_cls
        return run

    arms = {"plain": plain_of(fa.lib(), ctx.handle)}
    if a.baseline_lib:
        base = C.CDLL(os.path.abspath(a.baseline_lib))
        base.fa_tdt_greedy_logits_dev.argtypes = fa.lib().fa_tdt_greedy_logits_dev.argtypes
        base.fa_ctx_create.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        assert base.fa_ctx_create(0, C.c_void_p(ctx.stream), C.byref(h)) == 0      # the same stream: one timeline for every arm
        arms["baseline"] = plain_of(base, h)
    ok = np.uint8(G.LATIN_OK | G.IN_VOCAB)
    arms["lang_never"] = lang_of(np.full(V1, ok, np.uint8))
    rng = np.random.default_rng(3)
    tables = {}
    for p in a.shares:
        cls = np.full(V1, ok, np.uint8)
        draw = rng.random(V1)
        cls[draw < p] = np.uint8(G.CYRILLIC_OK | G.IN_VOCAB)
        cls[(draw >= p) & (draw < p + 0.02)] |= np.uint8(G.BLOCKLISTED)
        cls[V1 - 1] = ok
        tables[f"lang_{p:g}"] = cls
        arms[f"lang_{p:g}"] = lang_of(cls)

    # results: the plain entry of both builds bit for bit; lang_never = plain bit for bit; the replaced decisions of the first chunks
    # against the restatement
    def outputs():
        ctx.synchronize()
        return [t.cpu().numpy().copy() for t in (o[0], o[1], o[2], o_conf, o1[0], o1[1], o1[2], o1[3])]

    arms["plain"]()
    ref = outputs()
    tokens = int(ref[4].sum())
    report = {"shape": dict(B=B, U=U, T=T, V1=V1, dtype="float32", logits_GB=round(lg.numel() * 4 / 1e9, 1)), "tokens": tokens}
    for name in ("baseline", "lang_never"):
        if name in arms:
            arms[name]()
            got = outputs()
            report[f"{name}_equals_plain_bitwise"] = all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                                                         for x, y in zip(got, ref))
            assert report[f"{name}_equals_plain_bitwise"], name
    fired = {}
    for name, cls in tables.items():
        arms[name]()
        ctx.synchronize()
        sw = swaps.cpu().numpy()
        vocab = {i: ("▁при" if cls[i] & G.CYRILLIC_OK and not cls[i] & G.LATIN_OK else "▁le") for i in range(V1)}
        block = frozenset(int(i) for i in np.flatnonzero(cls & G.BLOCKLISTED))
        mode = G.LanguageMode(G.LATIN, vocab, 64, block)
        decisions = 0
        for b in range(min(a.check_chunks, B)):
            r = G.walk_logits(lg[b].cpu().numpy(), V1, nd, T, mode, blank_id=V1 - 1, max_out=U)
            assert r["swap_counts"] == tuple(int(v) for v in sw[b]), (name, b, r["swap_counts"], sw[b])
            assert r["tokens"].tolist() == o[0][b, :r["count"]].cpu().numpy().tolist(), (name, b)
            decisions += r["joint_calls"]
        per_chunk = decisions / min(a.check_chunks, B)
        fired[name] = dict(script_swaps=int(sw[:, 0].sum()), blocklist_swaps=int(sw[:, 1].sum()), decisions_per_chunk_restatement=per_chunk,
                           share_of_decisions=round(float(sw.sum()) / (per_chunk * B), 5))
    report["replaced_decisions"] = fired

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for run in arms.values():                                      # warm every arm
        run()
    ctx.synchronize()
    times = {name: [] for name in arms}
    for _ in range(a.rounds):                                      # alternately: every arm once per round
        for name, run in arms.items():
            e0.record(stream)
            for _ in range(a.reps):
                run()
            e1.record(stream)
            ctx.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    report["ms"] = {k: dict(median=round(med[k], 5), min=round(min(v), 5), max=round(max(v), 5)) for k, v in times.items()}
    report["ratio_to_plain"] = {k: round(med[k] / med["plain"], 3) for k in arms if k != "plain"}
    if "baseline" in med:
        spread = max(max(times[k]) - min(times[k]) for k in ("plain", "baseline"))
        report["plain_vs_baseline"] = dict(change_ms=round(med["plain"] - med["baseline"], 5), run_to_run_spread_ms=round(spread, 5),
                                           inside_spread=bool(abs(med["plain"] - med["baseline"]) <= spread))
    for name in tables:
        extra_us = (med[name] - med["lang_never"]) * 1e3
        n = fired[name]["script_swaps"] + fired[name]["blocklist_swaps"]
        report.setdefault("per_replaced_decision", {})[name] = dict(launch_extra_us=round(extra_us, 2), replaced_per_chunk=round(n / B, 2),
                                                                      chunk_chain_extra_us_per_replacement=round(extra_us / max(n / B, 1e-9), 3))
    print(json.dumps(report))


if __name__ == "__main__":
    main()
