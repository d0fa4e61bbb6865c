"""Numbers for fa_ctc_kws_spot_batch_dev at the reference's "extra-large vocabulary" size: 256 utterances of 188 frames, 1025 columns,
670 keywords of 2-12 tokens (synthetic: peaky frames — blank on four of five, one hot token otherwise — with a few keywords planted).
Prints one JSON line: device time per call (the context's event bracket around the launches, median of the repeats) and host-clock time,
jobs per second, time per DP frame step (device time over jobs x frames), and — when --fetch-bytes gives the FETCH_SIZE-derived bytes of
one kws_walk launch from a counter run of its own (scripts/pmc_summary.py) — the log-prob bytes fetched relative to B T V 4.  Every
--restatement-sample-th job is also run through tests/kws_restatement.py on one thread: its time is context only (the reference's Swift
cannot be timed here), its records are compared with the device's.  Fails without a GPU.

    python scripts/kws_probe.py [--utterances 256] [--frames 188] [--keywords 670] [--repeats 10] [--fetch-bytes N] [--out profiles/kws_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fluidaudio_amd as fa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--frames", type=int, default=188)
    ap.add_argument("--vocab", type=int, default=1025)
    ap.add_argument("--keywords", type=int, default=670)
    ap.add_argument("--min-score", type=float, default=-3.0)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--restatement-sample", type=int, default=100, help="0: skip")
    ap.add_argument("--fetch-bytes", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("kws_probe: no GPU visible (there is no CPU fallback)")
    ctx = fa.default_context(0)
    B, T, V, K, blank = a.utterances, a.frames, a.vocab, a.keywords, a.vocab - 1
    rng = np.random.default_rng(2406)
    keywords = [rng.integers(0, blank, int(n)).tolist() for n in rng.integers(2, 13, K)]
    hot = np.where(rng.random((B, T)) < 0.8, blank, rng.integers(0, blank, (B, T)))
    for i in range(min(64, K)):   # keyword i planted in utterance i % B from frame 10 on, a blank between its tokens
        for n, t in enumerate(keywords[i]):
            if 10 + 2 * n < T:
                hot[i % B, 10 + 2 * n] = t
    g = torch.Generator(device="cuda").manual_seed(7)
    logits = torch.randn((B, T, V), generator=g, device="cuda", dtype=torch.float32)
    logits.scatter_add_(2, torch.from_numpy(hot).cuda().unsqueeze(2), torch.full((B, T, 1), 14.0, device="cuda"))
    d_lp = fa.ctc_log_probs_dev(ctx, logits, blank_id=blank)
    torch.cuda.synchronize()
    lib = fa.lib()
    lib.fa_ctx_set_timing(ctx.handle, 1)
    dev_ms, host_ms, dets = [], [], None
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        dets, counts = fa.spot_keywords_batch(d_lp, keywords, min_score=a.min_score, blank_id=blank, ctx=ctx)
        if i >= a.warmup:
            host_ms.append(1e3 * (time.perf_counter() - t0))
            dev_ms.append(float(lib.fa_ctx_last_device_ms(ctx.handle)))
    lib.fa_ctx_set_timing(ctx.handle, 0)
    jobs = B * sum(1 for k in keywords if 0 < len(k) <= T)
    med = statistics.median(dev_ms)
    line = dict(probe="kws_spot_batch_dev", utterances=B, frames=T, vocab=V, keywords=K, tokens_min=2, tokens_max=12, jobs=jobs, detections=int(len(dets)),
                device_ms_median=med, device_ms_min=min(dev_ms), device_ms_max=max(dev_ms), wrapper_call_ms_median=statistics.median(host_ms),
                jobs_per_s=jobs / (med * 1e-3), ns_per_dp_frame_step=med * 1e6 / (jobs * T), log_prob_bytes=B * T * V * 4,
                fetch_bytes_per_launch=a.fetch_bytes, fetch_over_log_prob_bytes=None if a.fetch_bytes is None else a.fetch_bytes / (B * T * V * 4),
                sclk_mhz=ctx.sclk_mhz(), repeats=a.repeats, warmup=a.warmup)
    ok = True
    if a.restatement_sample > 0:
        import kws_restatement as R
        lp = d_lp.cpu().numpy()
        got = {}
        for d in dets:
            got.setdefault((int(d["utterance"]), int(d["keyword"])), []).append((R.bits(d["score"]), int(d["start_frame"]), int(d["end_frame"])))
        sample = [(u, k) for u in range(B) for k in range(K)][::a.restatement_sample]
        t0 = time.perf_counter()
        for u, k in sample:
            want = [(R.bits(s), x, y) for s, x, y in R.word_spot_multiple(list(lp[u]), keywords[k], R.adjusted_threshold(a.min_score, len(keywords[k])), True, blank)]
            ok = ok and want == got.get((u, k), [])
        line.update(restatement_jobs=len(sample), restatement_single_thread_s=time.perf_counter() - t0, sample_matches_restatement=bool(ok))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
