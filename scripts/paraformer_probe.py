"""Numbers for fa_paraformer_cif_dev and fa_paraformer_timestamps_dev at a user-sized batch: 256 utterances of T = 512 encoder frames of
dim 512 whose alphas give about 100 tokens each, with 30 s of 16 kHz audio each, the inputs resident on the device.  Prints one JSON
line: per leg the median host-clock time of the ABI call (it ends in the call's one stream synchronisation) and the device time between
the call's two events (fa_ctx_set_timing); for CIF also the algorithmic bytes (rows read once + ac written) over the device time as a
share of the HBM peak; and the time of the single-core C++ baseline (scripts/paraformer_baseline.cpp, -O2 -ffp-contract=off) on the
first --baseline-utts utterances, scaled to the batch, whose checksums over those utterances must equal the device's.  Fails without a
GPU.  The per-kernel split of the timestamps call is read from a kernel trace of this script, not from here.

    python scripts/paraformer_probe.py [--batch 256] [--repeats 15] [--baseline-utts 32] [--out profiles/paraformer_probe.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluidaudio_amd as fa  # noqa: E402
from fluidaudio_amd import _lib as L  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK_GBS = 8000.0   # MI355X, vendor figure


def timed(ctx, call, repeats, warmup):
    for _ in range(warmup):
        call()
    host, dev = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        host.append(time.perf_counter() - t0)
        dev.append(L.lib().fa_ctx_last_device_ms(ctx.handle))
    return dict(call_ms_median=1e3 * statistics.median(host), call_ms_min=1e3 * min(host), call_ms_max=1e3 * max(host),
                device_ms_median=statistics.median(dev), device_ms_min=min(dev), repeats=repeats, warmup=warmup)


def checksums(ac, cif, spans):
    u64 = lambda a: int(a.astype(np.uint64).sum(dtype=np.uint64))   # noqa: E731
    return [u64(np.ascontiguousarray(ac).view(np.uint32)), int(cif.fire_frames[cif.fire_frames >= 0].astype(np.int64).sum()), int(cif.token_counts.sum()),
            int(cif.fire_counts.sum()), int(spans.size), u64(np.ascontiguousarray(spans["start"]).view(np.uint64)), u64(np.ascontiguousarray(spans["end"]).view(np.uint64))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-utts", type=int, default=32)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("paraformer_probe: no GPU visible (there is no CPU fallback)")
    ctx = fa.default_context(0)
    L.lib().fa_ctx_set_timing(ctx.handle, 1)
    B, T, D, n = a.batch, a.frames, a.dim, int(a.seconds * 16000)
    gen = torch.Generator(device="cuda").manual_seed(2025)
    enc = torch.randn((B, T, D), generator=gen, device="cuda", dtype=torch.float32)
    half = enc.to(torch.float16)
    alphas = torch.rand((B, T), generator=gen, device="cuda", dtype=torch.float32) * 0.39          # about 100 tokens in 512 frames
    # speech-like audio: noise bursts of 0.15 s every 0.3 s over a floor
    t = torch.arange(n, device="cuda")
    gate = ((t // 2400) % 2 == 0).to(torch.float32) * 0.2 + 0.001
    audio = (torch.randn((B, n), generator=gen, device="cuda", dtype=torch.float32) * gate).reshape(-1).contiguous()
    offsets = np.arange(B + 1, dtype=np.int64) * n
    valid = np.full(B, T, np.int32)
    cfg = fa.paraformer.default_config()
    vocab = 8404
    keep = np.ones(vocab, np.uint8)
    keep[:3] = 0
    torch.cuda.synchronize()

    legs = []
    res = {}

    def cif32():
        res["cif"] = fa.cif_batch_dev(enc, alphas, valid, config=cfg, pack_enc=False, ctx=ctx)

    def cif16():
        res["cif16"] = fa.cif_batch_dev(half, alphas, valid, config=cfg, pack_enc=False, ctx=ctx)
    for name, call, esz in (("cif_fp32", cif32, 4), ("cif_fp16", cif16, 2)):
        r = timed(ctx, call, a.repeats, a.warmup)
        algo = B * T * D * esz + B * cfg.max_tokens * D * 4
        r.update(leg=name, algorithmic_bytes=algo, gbs_device=algo / r["device_ms_median"] / 1e6, hbm_share=algo / r["device_ms_median"] / 1e6 / HBM_PEAK_GBS)
        legs.append(r)
    cif = res["cif"]
    # the decoder's argmax stands in: ids over the vocabulary, a few dropped ones among them
    ids = torch.randint(0, vocab, (B, cfg.max_tokens), generator=gen, device="cuda", dtype=torch.int32)

    def stamps():
        res["spans"] = fa.timestamps_batch_dev(alphas, valid, ids, cif.token_counts, keep, audio, offsets, config=cfg, ctx=ctx)
    r = timed(ctx, stamps, a.repeats, a.warmup)
    r.update(leg="timestamps", audio_bytes=int(audio.numel()) * 4, spans=int(res["spans"][0].size))
    legs.append(r)

    line = dict(probe="paraformer", batch=B, frames=T, dim=D, seconds=a.seconds, tokens_mean=float(cif.fire_counts.mean()), sclk_mhz=ctx.sclk_mhz(), legs=legs)
    ok = True
    if not a.no_baseline:
        exe = os.path.join(HERE, "paraformer_baseline")
        if not os.path.exists(exe):
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(HERE, "paraformer_baseline.cpp"), "-o", exe], check=True)
        k = min(a.baseline_utts, B)
        sub_cif = fa.cif_batch_dev(enc[:k], alphas[:k], valid[:k], config=cfg, ctx=ctx)
        sub_spans = fa.timestamps_batch_dev(alphas[:k], valid[:k], ids[:k].contiguous(), sub_cif.token_counts, keep, audio[:k * n], offsets[:k + 1], config=cfg, ctx=ctx)[0]
        with tempfile.NamedTemporaryFile(suffix=".bin") as f:
            f.write(np.array([k, T, D, cfg.max_tokens, vocab], np.int64).tobytes())
            for part in (enc[:k].cpu().numpy(), alphas[:k].cpu().numpy(), valid[:k], ids[:k].cpu().numpy(), sub_cif.token_counts, keep, offsets[:k + 1], audio[:k * n].cpu().numpy()):
                f.write(np.ascontiguousarray(part).tobytes())
            f.flush()
            out = subprocess.run([exe, f.name], capture_output=True, text=True, check=True).stdout.split()
        want, got = [int(x) for x in out[2:]], checksums(sub_cif.ac.cpu().numpy(), sub_cif, sub_spans)
        ok = want == got
        scale = B / k
        line["baseline"] = dict(utterances=k, cif_ms=float(out[0]), timestamps_ms=float(out[1]), cif_ms_scaled=float(out[0]) * scale, timestamps_ms_scaled=float(out[1]) * scale,
                                cif_over_call=float(out[0]) * scale / legs[0]["call_ms_median"], timestamps_over_call=float(out[1]) * scale / legs[2]["call_ms_median"],
                                matches_device=ok, checksums=got)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
