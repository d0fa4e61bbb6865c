"""Timing of the embedding-input stage at 8 h (14 400 windows of 10 s at a 2 s step, 589 frames, 3 speakers; the weights are
fa_powerset_decode of seeded random logits): the fa_embedding_plan_dev call (device-synchronised wall clock, best of --reps, with and
without the mask rows and with maskSimilarity 0.95), the fbank window fill per batch of 32, and the numpy CPU restatement on the same input
(tests/embedding_restatement.py; a CPU restatement, not the Swift reference).  Prints one JSON line with the bytes each call must move.
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split (--no-restatement skips the CPU part there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def best_of(reps, fn):
    import torch
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts[1:]), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    import torch
    import fluidaudio_amd as fa
    import embedding_restatement as E
    ctx = fa.default_context(0)
    n, F = 14400, 589
    rng = np.random.default_rng(8)
    logits = rng.standard_normal((n, F, 7)).astype(np.float32)
    logits[..., 1:4] += 1.0
    for c in range(n):
        a = int(rng.integers(0, F // 2))
        logits[c, a:a + F // 2, int(rng.integers(0, 7))] += 6.0
    seg = fa.powerset_decode(torch.from_numpy(logits).cuda(), np.arange(n) * 2.0, ctx=ctx)
    total = 16000 * (2 * n + 8)
    audio = torch.from_numpy(rng.standard_normal(total).astype(np.float32) * 0.1).cuda()
    cfg = fa.EmbeddingConfig()
    t_plan, p = best_of(args.reps, lambda: fa.plan_embeddings(seg, total, cfg, ctx=ctx))
    t_masks, _ = best_of(args.reps, lambda: fa.plan_embeddings(seg, total, cfg, mask_rows=True, ctx=ctx))
    t_skip, ps = best_of(args.reps, lambda: fa.plan_embeddings(seg, total, fa.EmbeddingConfig(skip_threshold=0.95), ctx=ctx))
    t_win, _ = best_of(args.reps, lambda: p.windows(p.batches // 2, audio))
    jobs, runs = p.info["jobs"], p.info["runs"]
    out = {"chunks": n, "jobs": jobs, "runs": runs, "runs_skip095": ps.info["runs"],
           "plan_dev_ms": 1e3 * t_plan, "plan_dev_mask_rows_ms": 1e3 * t_masks, "plan_dev_skip095_ms": 1e3 * t_skip,
           "window_batch32_ms": 1e3 * t_win,
           "plan_bytes": int(seg.speaker_weights.numel() * 4 + runs * cfg.weight_frames * 4),
           "mask_rows_bytes": int(jobs * F * 4), "window_batch32_bytes": int(32 * 160000 * 4 * 2)}
    if not args.no_restatement:
        w = seg.speaker_weights.cpu().numpy()
        t0 = time.perf_counter()
        want = E.plan(w, np.arange(n) * 2.0, total, E.Config())
        out["cpu_restatement_s"] = time.perf_counter() - t0
        out["matches_restatement"] = bool(np.array_equal(p.run_of_job, want["run_of_job"]) and
                                          np.array_equal(p.run_weights.cpu().numpy(), want["run_rows"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
